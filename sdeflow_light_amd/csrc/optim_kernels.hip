// optim_kernels.hip — the optimizer stage of a training step on a flat parameter bucket: a deterministic global
// gradient norm, Adam with device-resident hyper-parameters, gradient clipping, a weight EMA (with warm-up), weight decay
// and a non-finite step guard in the one pass over [p, g, m, v] (replaces torch.optim.Adam MSGM_higherDim.py:792,
// torch.nn.utils.clip_grad_norm_ and update_ema model/nn_utils.py:117-127; msgm_optim_step also
// torch.optim.Adam(weight_decay), torch.optim.AdamW and the skipped step of a GradScaler-style loop).  gfx950 only.  HBM-bound kernels; the element update is adam_elem of optim_elem.h, the
// same copy msgm_adam_step runs ("Optimizer stage").
#include "common.h"
#include "optim_elem.h"

// ============================================================ slice layout of the squared norm
// A function of n only: slices of OPT_SLICE elements (256 threads x 8 quads) while that gives at most OPT_MAX_SLICES of
// them, beyond that OPT_MAX_SLICES slices of ceil(n / OPT_MAX_SLICES) elements rounded up to a multiple of 1024 (every
// slice starts on a quad and gives each thread whole quads).  Never the device's CU count or the launched grid: the
// same n sums in the same order on every device.
static const int64_t OPT_SLICE = 8192;
static const int64_t OPT_MAX_SLICES = 1024;

static inline int64_t opt_slice_len(int64_t n) {
  if (n <= OPT_SLICE * OPT_MAX_SLICES) return OPT_SLICE;
  const int64_t per = (n + OPT_MAX_SLICES - 1) / OPT_MAX_SLICES;
  return (per + 1023) / 1024 * 1024;
}

// Sum of one double per thread over the 256 threads of the workgroup, a fixed order: xor tree inside each wave
// (offsets 32, 16, ..., 1), then (w0 + w1) + (w2 + w3) through LDS.  Every thread gets the sum.  Called by all threads.
__device__ __forceinline__ double block_sum_f64(double v) {
  __shared__ double red[4];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return r;
}

// partials[s] = sum over slice s of (g[e] * gscale)^2: the product g * gscale is rounded to float32 (the value the update
// sees), its square and every add are double.  Quad q of the slice (elements 4q .. 4q+3 from the slice's start) belongs
// to thread q % 256; a thread adds its quads in rising order, the elements of a quad in rising order; the threads
// meet in block_sum_f64.  The scalar body walks the same quads, so an unaligned buffer gives the same bits.
__global__ void __launch_bounds__(256) k_grad_sqnorm(const float* __restrict__ g, int64_t n, int64_t slice_len, float gscale,
                                                     double* __restrict__ partials) {
  const int64_t e_begin = (int64_t)blockIdx.x * slice_len;
  const int64_t e_end = e_begin + slice_len < n ? e_begin + slice_len : n;
  const bool vec = (n & 3) == 0 && aligned16(g);
  double acc = 0.0;
  for (int64_t e0 = e_begin + 4 * (int64_t)threadIdx.x; e0 < e_end; e0 += 1024) {
    if (vec) {
      const f32x4 gv = ld4(g + e0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float gg = gv[k] * gscale;
        acc += (double)gg * (double)gg;
      }
    } else {
      for (int k = 0; k < 4; ++k) {
        if (e0 + k >= e_end) break;
        const float gg = g[e0 + k] * gscale;
        acc += (double)gg * (double)gg;
      }
    }
  }
  acc = block_sum_f64(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// ============================================================ Adam + clip + EMA (+ decay, guard, warm-up)
// opt = {lr, beta1, beta2, eps, max_grad_norm, ema_rate[, weight_decay]}: doubles ON THE DEVICE, read at every launch
// (msgm_opt_t: six, msgm_optim_t: seven; the seventh is read by the decay instantiations only).
// Prologue (partials != NULL), every workgroup alike: thread t adds partials[t], partials[t + 256], ... in rising order,
// block_sum_f64, norm = sqrt(sum), and with clip coef = (float)min(1, max_grad_norm / (norm + 1e-6)) written so that a NaN
// norm gives a NaN coefficient (clip_grad_norm_ with error_if_nonfinite=False).  Body: gg = (g * gscale) * coef, two
// roundings, then adam_elem with scale 1 (exact), then ema = ema * rate + p_new * (1 - rate): two products, one add.
//
// One kernel, three options compiled in or out; <0, false, false> is the code msgm_adam_step_ex always ran.
//  WD     adam_elem_decay of optim_elem.h: 1 = torch.optim.Adam(weight_decay), 2 = torch.optim.AdamW.
//  GUARD  the skip of a GradScaler-style loop, decided on the device: verdict = the double sum of the partials is not
//         finite (true exactly when some float32 (g * gscale) is Inf or NaN: squares of finite floats cannot overflow a
//         double).  Every workgroup forms the same verdict from the same adds and, when it is true, returns before the
//         first load of p, g, m, v, ema.  skipped[2] counts the skipped steps without atomics and without a race: a step
//         whose attempt count (*step_dev, 1-based) is st READS skipped[st & 1] and thread 0 of block 0 WRITES
//         skipped[(st + 1) & 1] = skipped[st & 1] + verdict, the slot the next step reads.  Several launches of one
//         step write the same value.  Bias corrections and the warm-up use k_eff = st - skipped[st & 1].
//  WARM   rate_k = min(rate, (1 + k_eff) / (10 + k_eff)) in double, then the EMA form above with (float)rate_k and
//         (float)(1 - rate_k).
template <int WD, bool GUARD, bool WARM>
__global__ void __launch_bounds__(256) k_adam_ex(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, float* __restrict__ ema, int64_t n,
                                                 const double* __restrict__ opt, float gscale,
                                                 const int64_t* __restrict__ step_dev, const double* __restrict__ partials,
                                                 int32_t n_partials, float* __restrict__ grad_norm_out, int32_t clip,
                                                 int64_t* __restrict__ skipped) {
  float coef = 1.0f;
  int64_t k_eff = step_dev[0];
  if (partials) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 256) acc += partials[i];
    const double sum = block_sum_f64(acc);
    const double norm = sqrt(sum);
    if (clip) {
      const double ratio = opt[4] / (norm + 1e-6);
      coef = (float)(ratio > 1.0 ? 1.0 : ratio);
    }
    if (grad_norm_out && blockIdx.x == 0 && threadIdx.x == 0) grad_norm_out[0] = (float)norm;
    if constexpr (GUARD) {
      const int64_t done = skipped[k_eff & 1];
      const bool bad = !(fabs(sum) <= 1.79769313486231570e308);          // Inf or NaN
      if (blockIdx.x == 0 && threadIdx.x == 0) skipped[(k_eff + 1) & 1] = done + (bad ? 1 : 0);
      if (bad) return;                                                   // before any load of p, g, m, v, ema
      k_eff -= done;
    }
  }
  const AdamCoef c = adam_coef(opt[0], opt[1], opt[2], opt[3], 1.0f, k_eff);
  float wd = 0.0f;
  if constexpr (WD == 1) wd = (float)opt[6];
  if constexpr (WD == 2) wd = (float)(1.0 - opt[0] * opt[6]);
  double rate_k = opt[5];
  if constexpr (WARM) {
    const double w = (1.0 + (double)k_eff) / (10.0 + (double)k_eff);
    rate_k = rate_k < w ? rate_k : w;
  }
  const float rate = (float)rate_k, orate = (float)(1.0 - rate_k);
  const int64_t nq = (n + 3) >> 2;
  const bool vec = (n & 3) == 0 && aligned16(p, g, m, v, ema);
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = q << 2;
    if (vec) {
      f32x4 pv = ld4(p + e0), gv = ld4(g + e0), mv = ld4(m + e0), vv = ld4(v + e0);
      f32x4 ev = {0.f, 0.f, 0.f, 0.f};
      if (ema) ev = ld4(ema + e0);                 // in flight with the other four loads
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const AdamPmv r = adam_elem_decay<WD>(c, wd, pv[k], (gv[k] * gscale) * coef, mv[k], vv[k]);
        pv[k] = r.p; mv[k] = r.m; vv[k] = r.v;
      }
      st4(p + e0, pv); st4(m + e0, mv); st4(v + e0, vv);
      if (ema) {
#pragma unroll
        for (int k = 0; k < 4; ++k) ev[k] = ev[k] * rate + pv[k] * orate;
        st4(ema + e0, ev);
      }
    } else {
      for (int k = 0; k < 4; ++k) {
        const int64_t e = e0 + k;
        if (e >= n) break;
        const AdamPmv r = adam_elem_decay<WD>(c, wd, p[e], (g[e] * gscale) * coef, m[e], v[e]);
        p[e] = r.p; m[e] = r.m; v[e] = r.v;
        if (ema) ema[e] = ema[e] * rate + r.p * orate;
      }
    }
  }
}

using adam_ex_fn = void (*)(float*, const float*, float*, float*, float*, int64_t, const double*, float, const int64_t*,
                            const double*, int32_t, float*, int32_t, int64_t*);
template <int WD>
static adam_ex_fn adam_ex_pick(bool guard, bool warm) {
  if (guard) return warm ? k_adam_ex<WD, true, true> : k_adam_ex<WD, true, false>;
  return warm ? k_adam_ex<WD, false, true> : k_adam_ex<WD, false, false>;
}

// a <-> b, in place.  The two buffers must not overlap.
__global__ void __launch_bounds__(256) k_swap(float* __restrict__ a, float* __restrict__ b, int64_t n) {
  const int64_t nq = (n + 3) >> 2;
  const bool vec = (n & 3) == 0 && aligned16(a, b);
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = q << 2;
    if (vec) {
      const f32x4 av = ld4(a + e0), bv = ld4(b + e0);
      st4(a + e0, bv); st4(b + e0, av);
    } else {
      for (int k = 0; k < 4; ++k) {
        const int64_t e = e0 + k;
        if (e >= n) break;
        const float t = a[e];
        a[e] = b[e]; b[e] = t;
      }
    }
  }
}

// ============================================================ C ABI
extern "C" {

int32_t msgm_grad_sqnorm_partials(int64_t n) {
  if (n <= 0) return 0;
  const int64_t len = opt_slice_len(n);
  return (int32_t)((n + len - 1) / len);
}

int msgm_grad_sqnorm(const float* g, int64_t n, float gscale, double* partials, int32_t* n_partials_out,
                     msgm_stream_t stream) {
  if (!g || !partials || n <= 0) return MSGM_E_BADARG;
  const int32_t np = msgm_grad_sqnorm_partials(n);
  if (n_partials_out) *n_partials_out = np;
  hipLaunchKernelGGL(k_grad_sqnorm, dim3(np), dim3(256), 0, S(stream), g, n, opt_slice_len(n), gscale, partials);
  return msgm_check_launch();
}

int msgm_adam_step_ex(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const msgm_opt_t* opt_dev,
                      float gscale, const int64_t* step_dev, const double* partials, int32_t n_partials,
                      float* grad_norm_out, msgm_stream_t stream) {
  if (!p || !g || !m || !v || !opt_dev || !step_dev || n <= 0) return MSGM_E_BADARG;
  if (partials && n_partials < 1) return MSGM_E_BADARG;
  hipLaunchKernelGGL((k_adam_ex<0, false, false>), dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, S(stream), p, g, m, v,
                     ema, n, reinterpret_cast<const double*>(opt_dev), gscale, step_dev, partials,
                     partials ? n_partials : 0, grad_norm_out, 1, (int64_t*)nullptr);
  return msgm_check_launch();
}

int msgm_optim_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const msgm_optim_t* opt_dev,
                    float gscale, const int64_t* step_dev, const double* partials, int32_t n_partials,
                    float* grad_norm_out, int32_t decay_mode, int32_t flags, int64_t* skipped_dev, msgm_stream_t stream) {
  if (!p || !g || !m || !v || !opt_dev || !step_dev || n <= 0) return MSGM_E_BADARG;
  if (partials && n_partials < 1) return MSGM_E_BADARG;
  if (decay_mode < MSGM_DECAY_NONE || decay_mode > MSGM_DECAY_DECOUPLED) return MSGM_E_BADARG;
  if (flags & ~(MSGM_OPTIM_CLIP | MSGM_OPTIM_EMA_WARMUP)) return MSGM_E_BADARG;
  const bool clip = flags & MSGM_OPTIM_CLIP, warm = flags & MSGM_OPTIM_EMA_WARMUP;
  if ((clip || skipped_dev) && !partials) return MSGM_E_BADARG;       // both need the norm
  if (warm && !ema) return MSGM_E_BADARG;
  const adam_ex_fn k = decay_mode == MSGM_DECAY_L2          ? adam_ex_pick<1>(skipped_dev != nullptr, warm)
                       : decay_mode == MSGM_DECAY_DECOUPLED ? adam_ex_pick<2>(skipped_dev != nullptr, warm)
                                                            : adam_ex_pick<0>(skipped_dev != nullptr, warm);
  hipLaunchKernelGGL(k, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, S(stream), p, g, m, v, ema, n,
                     reinterpret_cast<const double*>(opt_dev), gscale, step_dev, partials, partials ? n_partials : 0,
                     grad_norm_out, (int32_t)clip, skipped_dev);
  return msgm_check_launch();
}

int msgm_swap(float* a, float* b, int64_t n, msgm_stream_t stream) {
  if (!a || !b || n <= 0) return MSGM_E_BADARG;
  if (a < b ? a + n > b : b + n > a) return MSGM_E_BADARG;        // overlapping buffers
  hipLaunchKernelGGL(k_swap, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, S(stream), a, b, n);
  return msgm_check_launch();
}

}  // extern "C"
