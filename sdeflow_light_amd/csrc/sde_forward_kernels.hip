// sde_forward_kernels.hip — y_t | y_0 of the multiplicative SDE in one launch (msgm_forward_perturb).  gfx950 only.
//
// The composed route (sde_scheme.msgm_forward_perturb_composed) integrates EVERY row through all nsf RK4-Stratonovich
// steps of the forward process with one launch per stage, combine and masked capture: 6 nsf + 9 launches that stream
// 12-24 B per element each.  Rows never interact, so here a row lives in registers, takes exactly the steps it needs —
// k_b = forward_step_k(t_b) of them on the nsf-step grid, or one step of length t_b when k_b = 0 — and is stored once.
// Every formula is the function of sde_stage.h the stage kernels call, in the composed route's order, and the build
// keeps -ffp-contract=off: the result is the composed route's, bit for bit.
//
// Three regimes (msgm_forward_perturb picks by kind and n only, never by the batch):
//   sparse, n <= 256        a group of 1..64 lanes per row, 4 contiguous elements per lane, several rows per wave.  The
//                           chunk-edge values of the stage input and the previous chunk's last noise travel by __shfl:
//                           no LDS, no barrier.  The rows of a wave stop at different k_b: the loop runs to the wave's
//                           largest count with finished rows predicated off, so no shuffle sits under a k_b branch.
//   sparse, 256 < n <= 12288   one workgroup per row, 4 (n <= 4096) or 16 contiguous elements per thread; the same
//                           edge values go through a double-buffered LDS table (24 KB), one __syncthreads per stage.
//                           k_b is uniform in the workgroup.  The bound is the register file, not the LDS: state,
//                           increment, running sum and stage input are 4 x 16 registers, the kernel needs 144 VGPRs, so
//                           a workgroup has at most 768 threads (three waves per SIMD at <= 168) and 768 x 16 = 12288;
//                           at 1024 threads (128 VGPRs) it spills.  The 16-element form takes n % 4 == 0 and 16-byte
//                           aligned operands only.
//   dense, n <= 64          a lane per element, a group of pow2 >= n lanes per row; the stage input and the increment of
//                           a row sit in LDS for dense_g, G and L_G too when n <= 16 (17 KB), else they come through L2
//                           as in k_stage_rows.  The loop runs to the workgroup's largest count.
//
// All-times mode (template parameter PATHS, msgm_forward_paths): the same kernels for the time-integrated SSM loss
// (PluginReverseSDE(ssm_intT=True), SDEs.py:648-706).  Every row takes all nsf grid steps — no row time, no short step, no
// k_out, a uniform trip count — and the state after each step it >= first_keep is stored to y_all[(it - first_keep) B + b, :],
// one store per element, in place of the single store at the end.  The store follows the step's last exchange / barrier and
// sits under `on && it >= first_keep`: uniform in `it`, per lane in `on`, no shuffle or barrier inside it.  Same regimes,
// support set and alignment rules; the result equals rk4_stratonovich_sampler(forward_SDE, keep_all_samples)[first_keep:]
// bit for bit.  The 16-element form needs 147 VGPRs in this mode (144 without), still three waves per SIMD: the bound on n
// stays 12288.  No instantiation uses scratch (profiles/ssm_intT/kernel_regs.txt).
#include "common.h"
#include "sde_stage.h"

struct FwdArgs {
  const float* x0; const float* t; float* y; int32_t* k_out;
  int64_t B; int64_t n; int32_t nsf; const float* ts;
  float delta, sqrt_delta, t_half, t_full;
  const float* z_main; const float* z_short; const uint64_t* rng;
  float b0, b1, T; const float* G; const float* L_G;
  int vec;                     // n % 4 == 0 and x0, y, z_main, z_short 16-byte aligned: float4 loads and stores
  int gs;                      // lanes per row of the lane-group regimes (a power of two)
  int32_t first_keep;          // PATHS only: the first step whose state is stored (y is y_all, t and k_out are unused)
};

__device__ __forceinline__ f32x4 fw_ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void fw_st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// What row b has to do: its stop index, the number of RK4 steps it takes and whether that is the one short step of
// length t_b (k = 0).  An index outside [0, nsf] (a negative time) is never captured by the composed route's
// msgm_keep_rows, whose buffer starts as zeros: no step, and the row is written as zeros.
// PATHS (msgm_forward_paths): every row takes all nsf grid steps; there is no row time and no short step.
struct RowPlan { int32_t k; int nsteps; bool brief; };
template <bool PATHS>
__device__ __forceinline__ RowPlan row_plan(const FwdArgs& F, int64_t b, bool live) {
  if (!live) return {-1, 0, false};
  if constexpr (PATHS) return {F.nsf, F.nsf, false};
  const int32_t k = forward_step_k(F.t[b], F.nsf, F.T);
  return {k, k == 0 ? 1 : (k > 0 && k <= F.nsf ? k : 0), k == 0};
}

// The forward process in Stratonovich form, lmbd = 0: what stage_coef, stage_mu and stage_sig_scale are asked with.
__device__ __forceinline__ StageArgs forward_stage_args(const FwdArgs& F) {
  StageArgs A = {};
  A.proc = MSGM_PROC_FORWARD; A.strato = 1; A.lmbd = 0.f;
  A.b0 = F.b0; A.b1 = F.b1; A.T = F.T; A.delta = F.delta; A.sqrt_delta = F.sqrt_delta;
  return A;
}

// Coefficients of a row's step `it` at its three distinct stage times.  Grid steps: ts[it], ts[it] + t_half,
// ts[it] + t_full (fp32 adds, as _Run.clock forms them), kernel-wide delta.  The short step: stage_coef's delta_rows /
// t_frac form with delta_b = t_b and times 0 + {0, 1/2, 1} t_b.
struct StepCoef { StageCoef c0, c1, c2; };
__device__ __forceinline__ StepCoef step_coef(const FwdArgs& F, StageArgs A, bool brief, int it, int64_t b) {
  float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, f1 = 0.0f, f2 = 0.0f;
  if (brief) {
    A.delta_rows = F.t; f1 = 0.5f; f2 = 1.0f;
  } else {
    t0 = F.ts[it]; t1 = __fadd_rn(t0, F.t_half); t2 = __fadd_rn(t0, F.t_full);
  }
  StepCoef s;
  A.t_frac = 0.0f; s.c0 = stage_coef(A, t0, b);
  A.t_frac = f1; s.c1 = stage_coef(A, t1, b);
  A.t_frac = f2; s.c2 = stage_coef(A, t2, b);
  return s;
}
// the standard normals of a step: where the injected ones start for row b, and the Philox offset otherwise
__device__ __forceinline__ const float* step_z(const FwdArgs& F, bool brief, int it, int64_t b) {
  if (brief) return F.z_short ? F.z_short + b * F.n : nullptr;
  return F.z_main ? F.z_main + ((int64_t)it * F.B + b) * F.n : nullptr;
}
__device__ __forceinline__ uint64_t step_extra(const FwdArgs& F, bool brief, int it) {
  return brief ? (uint64_t)F.nsf + 1 : (uint64_t)it;
}

// ============================================================ sparse
// A lane's chunk: E contiguous elements from i0, the first cnt of them inside the row (cnt = 0: an idle lane).
template <int E>
__device__ __forceinline__ void chunk_load(const float* row, int i0, int cnt, bool vec, float (&v)[E]) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < E / 4; ++q)
      if (4 * q < cnt) {
        const f32x4 r = fw_ld4(row + i0 + 4 * q);
        v[4 * q] = r[0]; v[4 * q + 1] = r[1]; v[4 * q + 2] = r[2]; v[4 * q + 3] = r[3];
      }
  } else {
#pragma unroll
    for (int k = 0; k < E; ++k)
      if (k < cnt) v[k] = row[i0 + k];
  }
}
template <int E>
__device__ __forceinline__ void chunk_store(float* row, int i0, int cnt, bool vec, const float (&v)[E]) {
  if (vec) {
#pragma unroll
    for (int q = 0; q < E / 4; ++q)
      if (4 * q < cnt) fw_st4(row + i0 + 4 * q, f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]});
  } else {
#pragma unroll
    for (int k = 0; k < E; ++k)
      if (k < cnt) row[i0 + k] = v[k];
  }
}
// The last live value of a chunk is picked up where the values are produced (`last = k < cnt ? value : last` on the value
// just computed).  As a walk of its own over the finished array the optimiser rewrites it to v[cnt - 1] before it unrolls
// anything, and the runtime index keeps the array out of registers (scratch, or LDS the kernel never asked for).
// The chunk's Wiener increment sqd * z: z injected, or the Philox numbers stage_noise / k_stage_sparse_flat draw for
// the same global elements (quads when rows start on a quad, philox_normal1 per element otherwise: same blocks).
template <int E>
__device__ __forceinline__ void chunk_noise(const FwdArgs& F, bool vec, const float* zrow, uint64_t extra, int64_t b, int i0, int cnt,
                                            float sqd, float (&w)[E], float& wlast) {
#pragma unroll
  for (int k = 0; k < E; ++k) w[k] = 0.f;
  if (zrow) {
    chunk_load<E>(zrow, i0, cnt, vec, w);
  } else {
    const int64_t e0 = b * F.n + i0;
    if (vec || (F.n & 3) == 0) {
#pragma unroll
      for (int q = 0; q < E / 4; ++q)
        if (4 * q < cnt) {
          const f32x4 r = philox_normal4(F.rng, extra, RNG_STREAM_DW, (uint64_t)(e0 >> 2) + q);
          w[4 * q] = r[0]; w[4 * q + 1] = r[1]; w[4 * q + 2] = r[2]; w[4 * q + 3] = r[3];
          __builtin_amdgcn_sched_barrier(0);       // one Philox block at a time: interleaved, a long chunk's blocks spill
        }
    } else {
#pragma unroll
      for (int k = 0; k < E; ++k)
        if (k < cnt) {
          w[k] = philox_normal1(F.rng, extra, RNG_STREAM_DW, (uint64_t)(e0 + k));
          __builtin_amdgcn_sched_barrier(0);
        }
    }
  }
  wlast = 0.f;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const float wk = sqd * w[k];
    w[k] = wk;
    wlast = (k < cnt) ? wk : wlast;
  }
}

// Every chunk's first and last value (and, with NV = 3, its last noise) meet the neighbouring chunks': xm = the last
// value of the chunk before (circular), xp = the first of the chunk after, wm = the last noise of the chunk before.
// WG: through LDS, tables [2][3][1024] used alternately — a table is rewritten two exchanges later, after the barrier
// of the exchange in between, which no thread passes before it has read this one.  Otherwise: shuffles inside the wave.
template <bool WG, int NV>
__device__ __forceinline__ void edge_exchange(float first, float last, float wlast, int self, int srcm, int srcp, float* tables,
                                              int& phase, float& xm, float& xp, float& wm) {
  if constexpr (WG) {
    float* tb = tables + phase * (3 * 1024);
    tb[self] = first; tb[1024 + self] = last;
    if (NV == 3) tb[2048 + self] = wlast;
    __syncthreads();
    xm = tb[1024 + srcm]; xp = tb[srcp];
    if (NV == 3) wm = tb[2048 + srcm];
    phase ^= 1;
  } else {
    xm = __shfl(last, srcm, 64); xp = __shfl(first, srcp, 64);
    if (NV == 3) wm = __shfl(wlast, srcm, 64);
  }
}

// One stage on the chunk.  The bare increment at the stage input xin (chunk-edge neighbours xm_e, xp_e) is
// k_stage_sparse_flat's lines (f and divSigma do not enter the forward Stratonovich drift: stage_mu returns fs = 0 for it).
// It goes into the running sum as _rk4_step and msgm_rk4_combine take it, and xout receives what the next stage reads:
// x + K1/2, x + K2/2, x + K3, and after K4 the step's result.  K4 is stored by the composed stage as 0 + 1 * increment
// (base = NULL), which turns -0 into +0.  xout may be xin, and after K4 it is x: the walk keeps the one old value it still
// needs.  last: the last live value written.
template <int E, int STAGE>
__device__ __forceinline__ void sparse_stage(const StageArgs& A, const StageCoef& c, const float (&x)[E], const float (&xin)[E],
                                             float xm_e, float xp_e, const float (&w)[E], float wm_e, int cnt, float (&s)[E],
                                             float (&xout)[E], bool act, float& last) {
  const float sig_scale = stage_sig_scale(A);
  float xm = xm_e;
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int kn = k + 1 < E ? k + 1 : k, kp = k > 0 ? k - 1 : 0;
    const float xi = xin[k];
    const float xp = (k + 1 < E && k + 1 < cnt) ? xin[kn] : xp_e;
    const float gw = sparse_g(c.sb, xp, xm, w[k], k > 0 ? w[kp] : wm_e);
    const float inc = stage_mu(A, 0.f, 0.f, 0.f, 0.f) * c.delta + sig_scale * gw;
    xm = xi;
    float o;
    if (STAGE == 1) { s[k] = inc; o = x[k] + 0.5f * inc; }
    if (STAGE == 2) { s[k] = rk4_add(s[k], inc); o = x[k] + 0.5f * inc; }
    if (STAGE == 3) { s[k] = rk4_add(s[k], inc); o = x[k] + 1.0f * inc; }
    if (STAGE == 4) { const float xn = rk4_close(x[k], s[k], 0.f + 1.0f * inc); o = act ? xn : x[k]; }   // a finished row keeps its state
    xout[k] = o;
    last = (k < cnt) ? o : last;
  }
}

// VEC: the launch guarantees n % 4 == 0 and 16-byte aligned operands (the 16-element chunks: with the scalar loads and the
// per-element Philox calls compiled in as well, that kernel spills).
// PATHS: the state after every step it >= first_keep is stored to y_all[(it - first_keep) * B + b, :] and nothing else is;
// the store sits under a condition that is uniform in it and per lane in `on`, after the step's last exchange.
template <int E, bool WG, bool VEC, int THREADS, bool PATHS = false>
__global__ void __launch_bounds__(THREADS) k_forward_perturb_sparse(FwdArgs F) {
  const bool vec = VEC || F.vec;
  __shared__ float tables[WG ? 2 * 3 * 1024 : 1];
  const int n = (int)F.n;
  const int chunks = (n + E - 1) / E;                 // lanes of a row that hold elements
  int64_t b; int self, lane_t, base;
  if constexpr (WG) {
    b = blockIdx.x; lane_t = threadIdx.x; self = threadIdx.x; base = 0;
  } else {
    const int gs = F.gs;
    b = (int64_t)blockIdx.x * (blockDim.x / gs) + threadIdx.x / gs;
    self = threadIdx.x & 63; lane_t = self & (gs - 1); base = self - lane_t;
  }
  const bool live = b < F.B;
  const bool on = live && lane_t < chunks;
  const int i0 = lane_t * E;
  const int cnt = on ? (n - i0 < E ? n - i0 : E) : 0;
  // idle lanes take part in every exchange; their sources stay inside the row's own lanes
  const int srcm = base + (lane_t == 0 ? chunks - 1 : (lane_t < chunks ? lane_t - 1 : 0));
  const int srcp = base + (lane_t + 1 < chunks ? lane_t + 1 : 0);
  const RowPlan plan = row_plan<PATHS>(F, b, live);
  if constexpr (!PATHS) {
    if (on && lane_t == 0 && F.k_out) F.k_out[b] = plan.k;
  }
  int steps = plan.nsteps;                            // WG: the same in every thread
  if constexpr (!WG) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int other = __shfl_xor(steps, o, 64); steps = other > steps ? other : steps; }
  }
  const StageArgs A = forward_stage_args(F);
  float x[E];
#pragma unroll
  for (int k = 0; k < E; ++k) x[k] = 0.f;
  const bool go = on && plan.nsteps > 0;
  if (go) chunk_load<E>(F.x0 + b * F.n, i0, cnt, vec, x);
  float xlast = go ? F.x0[b * F.n + i0 + cnt - 1] : 0.f;
  int phase = 0;
  for (int it = 0; it < steps; ++it) {
    const bool act = on && it < plan.nsteps;
    const StepCoef sc = step_coef(F, A, plan.brief, it, live ? b : 0);
    float w[E], s[E], xe[E];
    float wlast = 0.f, elast = 0.f;
    if (act) chunk_noise<E>(F, vec, step_z(F, plan.brief, it, b), step_extra(F, plan.brief, it), b, i0, cnt, sc.c0.sqd, w, wlast);
    else {
#pragma unroll
      for (int k = 0; k < E; ++k) w[k] = 0.f;
    }
    float xm, xp, wm = 0.f, unused = 0.f;
    edge_exchange<WG, 3>(x[0], xlast, wlast, self, srcm, srcp, tables, phase, xm, xp, wm);
    sparse_stage<E, 1>(A, sc.c0, x, x, xm, xp, w, wm, cnt, s, xe, act, elast);          // K1 at t
    edge_exchange<WG, 2>(xe[0], elast, 0.f, self, srcm, srcp, tables, phase, xm, xp, unused);
    sparse_stage<E, 2>(A, sc.c1, x, xe, xm, xp, w, wm, cnt, s, xe, act, elast);         // K2 at t + delta/2
    edge_exchange<WG, 2>(xe[0], elast, 0.f, self, srcm, srcp, tables, phase, xm, xp, unused);
    sparse_stage<E, 3>(A, sc.c1, x, xe, xm, xp, w, wm, cnt, s, xe, act, elast);         // K3 at t + delta/2
    edge_exchange<WG, 2>(xe[0], elast, 0.f, self, srcm, srcp, tables, phase, xm, xp, unused);
    sparse_stage<E, 4>(A, sc.c2, x, xe, xm, xp, w, wm, cnt, s, x, act, xlast);          // K4 at t + delta
    if constexpr (PATHS) {
      if (on && it >= F.first_keep) chunk_store<E>(F.y + ((int64_t)(it - F.first_keep) * F.B + b) * F.n, i0, cnt, vec, x);
    }
  }
  if constexpr (!PATHS) {
    if (on) chunk_store<E>(F.y + b * F.n, i0, cnt, vec, x);
  }
}

// ============================================================ dense
// Lane lane_t of a row's group owns element lane_t.  xs / ws: the stage input and the Wiener increment of the group's
// row, read by every lane of the group in dense_g.
template <bool G_LDS, bool PATHS = false>
__global__ void __launch_bounds__(256) k_forward_perturb_dense(FwdArgs F) {
  __shared__ float Gs[G_LDS ? 16 * 16 * 16 + 16 * 16 : 1];
  __shared__ float xs[256], ws[256];
  __shared__ int steps_s;
  const int n = (int)F.n, gs = F.gs, tid = threadIdx.x;
  const int lane_t = tid & (gs - 1), base = tid - lane_t;
  const int64_t b = (int64_t)blockIdx.x * (blockDim.x / gs) + tid / gs;
  const bool live = b < F.B, on = live && lane_t < n;
  const float* G = F.G;
  const float* LG = F.L_G;
  if (tid == 0) steps_s = 0;
  if constexpr (G_LDS) {
    for (int i = tid; i < n * n * n; i += 256) Gs[i] = F.G[i];
    for (int i = tid; i < n * n; i += 256) Gs[n * n * n + i] = F.L_G[i];
    G = Gs; LG = Gs + n * n * n;
  }
  const RowPlan plan = row_plan<PATHS>(F, b, live);
  if constexpr (!PATHS) {
    if (on && lane_t == 0 && F.k_out) F.k_out[b] = plan.k;
  }
  __syncthreads();
  atomicMax(&steps_s, plan.nsteps);
  __syncthreads();
  const int steps = steps_s;
  const StageArgs A = forward_stage_args(F);
  const float sig_scale = stage_sig_scale(A);
  const int64_t e = b * F.n + lane_t;
  float x = (on && plan.nsteps > 0) ? F.x0[e] : 0.f;
  // the bare increment of a stage whose input the group has in xs: k_stage_rows' dense branch (dense_g's sums; the
  // forward Stratonovich drift is stage_mu's fs = 0, so f and G a are not needed: the increment stands in for the score)
  auto stage = [&](const StageCoef& c) {
    float inc = 0.f;
    if (lane_t < n) {
      const DenseTerms d = dense_g(G, LG, n, lane_t, c.beta, c.sb, xs + base, ws + base, ws + base);
      inc = stage_mu(A, 0.f, 0.f, 0.f, 0.f) * c.delta + sig_scale * d.gw;
    }
    return inc;
  };
  for (int it = 0; it < steps; ++it) {
    const bool act = on && it < plan.nsteps;
    const StepCoef sc = step_coef(F, A, plan.brief, it, live ? b : 0);
    float w = 0.f;
    if (act) {
      const float* zrow = step_z(F, plan.brief, it, b);
      const float z = zrow ? zrow[lane_t] : philox_normal1(F.rng, step_extra(F, plan.brief, it), RNG_STREAM_DW, (uint64_t)e);
      w = sc.c0.sqd * z;
    }
    ws[tid] = w; xs[tid] = x;
    __syncthreads();
    float inc = stage(sc.c0);                        // K1 at x
    float s = inc;
    __syncthreads();
    xs[tid] = x + 0.5f * inc;
    __syncthreads();
    inc = stage(sc.c1);                              // K2 at x + K1/2
    s = rk4_add(s, inc);
    __syncthreads();
    xs[tid] = x + 0.5f * inc;
    __syncthreads();
    inc = stage(sc.c1);                              // K3 at x + K2/2
    s = rk4_add(s, inc);
    __syncthreads();
    xs[tid] = x + 1.0f * inc;
    __syncthreads();
    inc = stage(sc.c2);                              // K4 at x + K3, stored by the composed stage as 0 + 1 * increment
    const float xn = rk4_close(x, s, 0.f + 1.0f * inc);
    x = act ? xn : x;
    if constexpr (PATHS) {
      if (on && it >= F.first_keep) F.y[(int64_t)(it - F.first_keep) * F.B * F.n + e] = x;
    }
    __syncthreads();
  }
  if constexpr (!PATHS) {
    if (on) F.y[e] = x;
  }
}

// ============================================================ C ABI
enum { FWD_SPARSE_GROUP_MAX = 256, FWD_SPARSE_E4_MAX = 4096, FWD_SPARSE_MAX = 12288, FWD_DENSE_MAX = 64, FWD_DENSE_LDS_MAX = 16 };

static int pow2_at_least(int64_t v) { int g = 1; while (g < v) g <<= 1; return g; }

// The launch of either entry: the regime by kind and n only.  F.vec and F.gs are set here.
template <bool PATHS>
static int forward_launch(FwdArgs F, int32_t kind, uintptr_t ptrs, msgm_stream_t stream) {
  const int64_t B = F.B, n = F.n;
  F.vec = (n % 4 == 0 && (ptrs & 15) == 0) ? 1 : 0;
  F.gs = 1;
  if (kind == MSGM_SDE_MSGM_DENSE) {
    F.gs = pow2_at_least(n);
    const int64_t grid = (B + 256 / F.gs - 1) / (256 / F.gs);
    if (grid > INT32_MAX) return MSGM_E_UNSUPPORTED;
    if (n <= FWD_DENSE_LDS_MAX) hipLaunchKernelGGL((k_forward_perturb_dense<true, PATHS>), dim3((unsigned)grid), dim3(256), 0, S(stream), F);
    else hipLaunchKernelGGL((k_forward_perturb_dense<false, PATHS>), dim3((unsigned)grid), dim3(256), 0, S(stream), F);
    return msgm_check_launch();
  }
  if (n <= FWD_SPARSE_GROUP_MAX) {
    F.gs = pow2_at_least((n + 3) / 4);
    const int64_t grid = (B + 256 / F.gs - 1) / (256 / F.gs);
    if (grid > INT32_MAX) return MSGM_E_UNSUPPORTED;
    hipLaunchKernelGGL((k_forward_perturb_sparse<4, false, false, 256, PATHS>), dim3((unsigned)grid), dim3(256), 0, S(stream), F);
    return msgm_check_launch();
  }
  if (B > INT32_MAX) return MSGM_E_UNSUPPORTED;
  if (n <= FWD_SPARSE_E4_MAX) {
    const int threads = (int)(((n + 3) / 4 + 63) / 64) * 64;
    hipLaunchKernelGGL((k_forward_perturb_sparse<4, true, false, 1024, PATHS>), dim3((unsigned)B), dim3(threads), 0, S(stream), F);
  } else {
    if (!F.vec) return MSGM_E_UNSUPPORTED;                                   // operands that are only 4-byte aligned
    const int threads = (int)(((n + 15) / 16 + 63) / 64) * 64;
    hipLaunchKernelGGL((k_forward_perturb_sparse<16, true, true, 768, PATHS>), dim3((unsigned)B), dim3(threads), 0, S(stream), F);
  }
  return msgm_check_launch();
}

extern "C" {

int msgm_forward_perturb_supported(int32_t kind, int64_t n) {
  if (n < 1) return 0;
  if (kind == MSGM_SDE_MSGM_SPARSE) return n <= FWD_SPARSE_E4_MAX || (n <= FWD_SPARSE_MAX && n % 4 == 0);
  if (kind == MSGM_SDE_MSGM_DENSE) return n <= FWD_DENSE_MAX;
  return 0;
}

int msgm_forward_perturb(const float* x0, const float* t, float* y, int32_t* k_out, int64_t B, int64_t n,
                         const msgm_sde_t* sde, int32_t nsf, const float* ts, float delta, float sqrt_delta,
                         float t_half, float t_full, const float* z_main, const float* z_short, const uint64_t* rng,
                         msgm_stream_t stream) {
  if (!x0 || !t || !y || !sde || !ts || B <= 0 || n <= 0 || nsf <= 0) return MSGM_E_BADARG;
  if ((!z_main || !z_short) && !rng) return MSGM_E_BADARG;
  if (sde->kind < 0 || sde->kind > 2) return MSGM_E_BADARG;
  if (y + B * n > x0 && x0 + B * n > y) return MSGM_E_BADARG;              // the stencil / contraction reads neighbours of x0
  if (sde->kind == MSGM_SDE_MSGM_DENSE && (!sde->G || !sde->L_G)) return MSGM_E_BADARG;
  if (!msgm_forward_perturb_supported(sde->kind, n)) return MSGM_E_UNSUPPORTED;
  const uintptr_t ptrs = reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(z_main) |
                         reinterpret_cast<uintptr_t>(z_short);
  const FwdArgs F{x0, t, y, k_out, B, n, nsf, ts, delta, sqrt_delta, t_half, t_full, z_main, z_short, rng,
                  sde->beta_min, sde->beta_max, sde->T, sde->G, sde->L_G, 0, 1, 0};
  return forward_launch<false>(F, sde->kind, ptrs, stream);
}

int msgm_forward_paths(const float* x0, float* y_all, int64_t B, int64_t n, const msgm_sde_t* sde, int32_t nsf,
                       int32_t first_keep, const float* ts, float delta, float sqrt_delta, float t_half, float t_full,
                       const float* z_main, const uint64_t* rng, msgm_stream_t stream) {
  if (!x0 || !y_all || !sde || !ts || B <= 0 || n <= 0 || nsf <= 0) return MSGM_E_BADARG;
  if (first_keep < 0 || first_keep >= nsf) return MSGM_E_BADARG;          // at least one state is kept
  if (!z_main && !rng) return MSGM_E_BADARG;
  if (sde->kind < 0 || sde->kind > 2) return MSGM_E_BADARG;
  if (y_all + (int64_t)(nsf - first_keep) * B * n > x0 && x0 + B * n > y_all) return MSGM_E_BADARG;   // rows are stored while others still read x0
  if (sde->kind == MSGM_SDE_MSGM_DENSE && (!sde->G || !sde->L_G)) return MSGM_E_BADARG;
  if (!msgm_forward_perturb_supported(sde->kind, n)) return MSGM_E_UNSUPPORTED;
  const uintptr_t ptrs = reinterpret_cast<uintptr_t>(x0) | reinterpret_cast<uintptr_t>(y_all) | reinterpret_cast<uintptr_t>(z_main);
  const FwdArgs F{x0, nullptr, y_all, nullptr, B, n, nsf, ts, delta, sqrt_delta, t_half, t_full, z_main, nullptr, rng,
                  sde->beta_min, sde->beta_max, sde->T, sde->G, sde->L_G, 0, 1, first_keep};
  return forward_launch<true>(F, sde->kind, ptrs, stream);
}

}  // extern "C"
