// metrics_kernels.hip — reporting metric next to the hot path: the RBF kernel of
// compute_kernel / compute_mmd (quantitative_comparison.py:22-46),
//     k(x_i, y_j) = exp(-mean_d((x_i - y_j)^2) / d) = exp(-sum_d (x_i - y_j)^2 / d^2),
// as ONE pass over 64 x 64 tiles of pairs: the (Nx, Ny, d) broadcast tensor the reference materialises
// (x.expand / y.expand, :29-31) never exists, and for the MMD only the SUM of the kernel matrix leaves the chip.
// The squared differences are formed directly (not via |x|^2 + |y|^2 - 2 x.y), so near pairs do not cancel.
//
// Second metric: the 1-D Gaussian kernel density of the multiplicative SDE's latent radii (SDEs.py:239-240, 503-509),
// evaluated in log space — k_kde_partial / k_kde_merge below.
#include "common.h"
#include <math.h>

#define RB_T 64      // pairs tile: 64 x rows by 64 y rows
#define RB_K 32      // feature chunk
#define RB_P 33      // LDS pitch: consecutive rows hit consecutive banks

__global__ void __launch_bounds__(256) k_rbf(const float* __restrict__ x, const float* __restrict__ y, int64_t Nx, int64_t Ny,
                                             int d, float* __restrict__ K, double* __restrict__ sum) {
  __shared__ float xs[RB_T * RB_P], ys[RB_T * RB_P];
  __shared__ float red[4];
  const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int64_t i0 = (int64_t)blockIdx.y * RB_T, j0 = (int64_t)blockIdx.x * RB_T;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  for (int k0 = 0; k0 < d; k0 += RB_K) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (RB_T * RB_K) / 256; ++k) {
      const int idx = tid + 256 * k, row = idx >> 5, col = idx & 31;
      const bool kin = k0 + col < d;
      xs[row * RB_P + col] = (kin && i0 + row < Nx) ? x[(i0 + row) * d + k0 + col] : 0.f;
      ys[row * RB_P + col] = (kin && j0 + row < Ny) ? y[(j0 + row) * d + k0 + col] : 0.f;
    }
    __syncthreads();
    const int kmax = min(RB_K, d - k0);
    for (int k = 0; k < kmax; ++k) {
      float xv[4], yv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = xs[(4 * ti + r) * RB_P + k];
#pragma unroll
      for (int c = 0; c < 4; ++c) yv[c] = ys[(tj + 16 * c) * RB_P + k];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { const float df = xv[r] - yv[c]; acc[r][c] += df * df; }
    }
  }
  const float scale = -1.0f / ((float)d * (float)d);
  float s = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int64_t i = i0 + 4 * ti + r, j = j0 + tj + 16 * c;
      if (i < Nx && j < Ny) {
        const float v = expf(acc[r][c] * scale);
        if (K) K[i * Ny + j] = v;
        s += v;
      }
    }
  if (sum) {
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) atomicAdd(sum, (double)((red[0] + red[1]) + (red[2] + red[3])));
  }
}

// ------------------------------------------------------------------ 1-D Gaussian KDE log-density
//   out[m] = -log(Ns) - log(h) - log(2 pi)/2 + logsumexp_i( -((q[m] - r[i]) / h)^2 / 2 )
// which is what sklearn's KernelDensity(kernel='gaussian', bandwidth=h).fit(r).score_samples(q) returns (exact sum).
// Everything is relative to the NEAREST sample, whose term is the largest: with t_i = |q - r_i| c, c = sqrt(log2(e)/2)/h,
//   sum_i exp(-((q - r_i)/h)^2/2) = 2^(-t_min^2) * sum_i 2^((t_min - t_i)(t_min + t_i)),
// every exponent is <= 0 and the nearest sample's is exactly 0 (t_min is one of the t_i, bit for bit), so the sum lies in
// [1, Ns] however many bandwidths the query sits from the samples; the factored exponent does not cancel.  The leading
// term -(d_min/h)^2/2 is added in double by the merge, from the fp32 distance.
// Work split: a block owns KDE_Q queries (one per thread) and one slab of samples, which it walks in chunks of KDE_S
// staged in LDS — every lane reads the same address (broadcast).  Per chunk: pass 1 finds the chunk's nearest distance,
// pass 2 sums the exponentials into KDE_U independent partial sums; chunks of one slab are folded in order.  The block
// writes (d_min, sum) per (slab, query); k_kde_merge folds the slabs in index order.  No atomics: bitwise repeatable.
#define KDE_Q 256     // queries per block
#define KDE_S 512     // samples per LDS chunk
#define KDE_U 8       // partial sums per thread (one 2 x ds_read_b128 group)

// 2^x for x <= 0 in one v_exp_f32 (flushes below 2^-126, which is what a vanishing term should do)
__device__ __forceinline__ float kde_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// (d, s) <- (d, s) folded with (d2, s2); each sum is relative to 2^(-(its d * c)^2)
__device__ __forceinline__ void kde_fold(float& d, float& s, float d2, float s2, float c) {
  const float ta = d * c, tb = d2 * c;
  if (d2 < d) { s = s * kde_exp2((tb - ta) * (tb + ta)) + s2; d = d2; }
  else        { s = s + s2 * kde_exp2((ta - tb) * (ta + tb)); }
}

__global__ void __launch_bounds__(KDE_Q) k_kde_partial(const float* __restrict__ q, int64_t M, const float* __restrict__ r,
                                                       int64_t Ns, float c, int64_t slab_len, f32x2* __restrict__ ws) {
  __shared__ __attribute__((aligned(16))) float rs[KDE_S];
  const int tid = threadIdx.x;
  const int64_t m = (int64_t)blockIdx.y * KDE_Q + tid;
  const float qv = m < M ? q[m] : 0.f;
  const int64_t i_begin = (int64_t)blockIdx.x * slab_len, i_end = min(Ns, i_begin + slab_len);
  float dmin = 0.f, sum = 0.f;
  for (int64_t i0 = i_begin; i0 < i_end; i0 += KDE_S) {
    const int n = (int)min((int64_t)KDE_S, i_end - i0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KDE_S / KDE_Q; ++k) {
      const int idx = tid + KDE_Q * k;
      rs[idx] = idx < n ? r[i0 + idx] : INFINITY;          // padding: infinitely far, its term is 2^-inf = 0
    }
    __syncthreads();
    const int n8 = (n + KDE_U - 1) & ~(KDE_U - 1);
    float cm = INFINITY;
    for (int i = 0; i < n8; i += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(&rs[i]);
#pragma unroll
      for (int u = 0; u < 4; ++u) cm = fminf(cm, fabsf(qv - v[u]));
    }
    const float tm = cm * c;
    float acc[KDE_U];
#pragma unroll
    for (int u = 0; u < KDE_U; ++u) acc[u] = 0.f;
    for (int i = 0; i < n8; i += KDE_U) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(&rs[i]), v1 = *reinterpret_cast<const f32x4*>(&rs[i + 4]);
#pragma unroll
      for (int u = 0; u < KDE_U; ++u) {
        const float a = fabsf(qv - (u < 4 ? v0[u & 3] : v1[u & 3])) * c;
        acc[u] += kde_exp2((tm - a) * (tm + a));
      }
    }
    const float cs = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    if (i0 == i_begin) { dmin = cm; sum = cs; }
    else kde_fold(dmin, sum, cm, cs, c);
  }
  if (m < M) ws[(int64_t)blockIdx.x * M + m] = f32x2{dmin, sum};
}

__global__ void __launch_bounds__(256) k_kde_merge(const f32x2* __restrict__ ws, int64_t M, int nslab, float c, double inv_h,
                                                   double log_norm, float* __restrict__ out) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  float dmin = INFINITY;
  for (int s = 0; s < nslab; ++s) dmin = fminf(dmin, ws[(int64_t)s * M + m][0]);
  const float tm = dmin * c;
  double tot = 0.0;
  for (int s = 0; s < nslab; ++s) {
    const f32x2 p = ws[(int64_t)s * M + m];
    const float ta = p[0] * c;
    tot += (double)(p[1] * kde_exp2((tm - ta) * (tm + ta)));
  }
  const double z = (double)dmin * inv_h;
  out[m] = (float)(log_norm - 0.5 * z * z + log(tot));
}

// slabs for (M, Ns): every chunk its own slab until the grid passes ~2048 blocks, then several chunks per slab
static inline int64_t kde_slabs(int64_t M, int64_t Ns) {
  const int64_t chunks = (Ns + KDE_S - 1) / KDE_S, qtiles = (M + KDE_Q - 1) / KDE_Q;
  const int64_t per = (chunks * qtiles + 2047) / 2048;
  return (chunks + per - 1) / per;
}

extern "C" {

int msgm_rbf_kernel(const float* x, const float* y, int64_t Nx, int64_t Ny, int32_t d, float* K, double* sum,
                    msgm_stream_t stream) {
  if (!x || !y || Nx <= 0 || Ny <= 0 || d <= 0 || (!K && !sum)) return MSGM_E_BADARG;
  const int64_t gx = (Ny + RB_T - 1) / RB_T, gy = (Nx + RB_T - 1) / RB_T;
  if (gy > 65535 || gx > 0x7fffffffLL) return MSGM_E_UNSUPPORTED;
  if (sum && msgm_zero_async(sum, sizeof(double), S(stream)) != MSGM_OK) return MSGM_E_LAUNCH;
  hipLaunchKernelGGL(k_rbf, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, S(stream), x, y, Nx, Ny, d, K, sum);
  return msgm_check_launch();
}

size_t msgm_kde_workspace(int64_t M, int64_t Ns) {
  if (M <= 0 || Ns <= 0) return 0;
  return (size_t)kde_slabs(M, Ns) * (size_t)M * sizeof(f32x2);
}

int msgm_kde_logpdf(const float* q, int64_t M, const float* r, int64_t Ns, double h, float* out, void* workspace,
                    size_t workspace_bytes, msgm_stream_t stream) {
  if (!q || !r || !out || !workspace || M <= 0 || Ns <= 0 || !(h > 0.0) || !std::isfinite(h)) return MSGM_E_BADARG;
  const float c = (float)(sqrt(0.5 * 1.4426950408889634) / h);
  const int64_t qtiles = (M + KDE_Q - 1) / KDE_Q, chunks = (Ns + KDE_S - 1) / KDE_S;
  if (qtiles > 65535 || !std::isfinite(c) || !(c > 0.f)) return MSGM_E_UNSUPPORTED;
  // a smaller workspace than msgm_kde_workspace() asks for is fine: fewer, longer slabs
  const int64_t fit = (int64_t)(workspace_bytes / ((size_t)M * sizeof(f32x2)));
  if (fit < 1) return MSGM_E_WORKSPACE;
  const int64_t want = std::min(kde_slabs(M, Ns), fit), per = (chunks + want - 1) / want, nslab = (chunks + per - 1) / per;
  hipLaunchKernelGGL(k_kde_partial, dim3((unsigned)nslab, (unsigned)qtiles), dim3(KDE_Q), 0, S(stream), q, M, r, Ns, c,
                     per * KDE_S, static_cast<f32x2*>(workspace));
  if (msgm_check_launch() != MSGM_OK) return MSGM_E_LAUNCH;
  const double log_norm = -log((double)Ns) - log(h) - 0.5 * log(2.0 * M_PI);
  hipLaunchKernelGGL(k_kde_merge, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, S(stream),
                     static_cast<const f32x2*>(workspace), M, (int)nslab, c, 1.0 / h, log_norm, out);
  return msgm_check_launch();
}

}  // extern "C"
