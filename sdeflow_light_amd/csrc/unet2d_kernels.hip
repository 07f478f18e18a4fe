// unet2d_kernels.hip — the 2-D U-Net's non-convolution ops on gfx950:
//   K7  GroupNorm(min(C,32) groups) [+ SiLU] on dual numbers, forward and backward
//       (model/nn_utils.py:39-46,107-114; model/unet.py:140-143,152-155,214,443-444)
//   K8  single-head attention pieces: batched fp32-MFMA GEMM + dual softmax rows
//       (model/unet.py:236-250)
//   K10 sinusoidal timestep embedding (model/nn_utils.py:130-148)
//   K9  layout glue: flat <-> channels-last image (NNUnet.py:19-77), 2x2 block sum
//       (adjoint of the nearest-2x upsample folded into the conv gather)
// Activations are channels-last [N][P][C]; the forward-mode tangent is the second
// half of the batch (rows n >= Bp).
#include "common.h"
#include <stdlib.h>
typedef double f64x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ GroupNorm dual
// Two fully parallel launches per direction (a per-sample workgroup would leave the
// chip idle at 32 samples/GPU):
//   1. k_gn_*_reduce: grid (sample, pixel chunk); threads run along channels (coalesced,
//      256/C pixel lanes), fp32 partials -> LDS -> ONE double per (sample, chunk, group, moment)
//      stored in that chunk's own slot — no atomics: the slots of a sample are added in chunk
//      order by the finalise kernels, so the result is bitwise reproducible.  The fp32 partials
//      are SHIFTED moments: sums of u = x - k, u^2, xdot, u xdot with the pivot k = the sample's own
//      first pixel of that channel (the tangent keeps raw sums: its mean is of the size of its spread), so a group whose mean is large against its spread loses nothing in the fp32
//      squares (raw x^2 rounds by 2^-24 x^2 per element, which no later double arithmetic removes: the error of
//      xhat grew like (mean/std)^2).  Every thread puts its pivots back in double before the group sums, so the
//      slots hold the raw moments (sum x, sum x^2, sum xdot, sum x xdot) and E[x^2] - mu^2 is formed in double
//      only: exact 0 for a constant group, 2^-53 mean^2 otherwise.
//   2. k_gn_*_apply: grid-stride elementwise pass that rebuilds {mean - pivot, inv_std,
//      mean(xdot), a = mean(xhat xdot)} from the moments (gn_pivot: why the mean is kept relative to a pivot).
// acc[b][chunk < GN_SLOTS][g][8] doubles: forward uses moments 0..3, backward 0..4; the per-channel
// parameter gradients of the backward go to per-(sample, chunk) slots too and are summed in a fixed order.
#define GN_SLOTS 32
// widest tensor: the VEC builds (C % 4 == 0) take C <= GN_MAX_C (C/4 <= 256 channel vectors, one per thread), the scalar
// builds one channel per thread (C <= 256); gn_max_c() is the ONE place the entries ask
#define GN_MAX_C 1024
static inline int gn_max_c(int C) { return C % 4 == 0 ? GN_MAX_C : 256; }
struct GnArgs {
  const float* x; const float* gamma; const float* beta;
  float* out; double* acc; float* stats;
  int P, C, G, Bp, dual, silu, chunk;   // chunk: pixels per workgroup (a multiple of sub in the reduce kernels)
  float eps;
  // backward
  const float* gout; float* gx; float* dgamma; float* dbeta;
  // input = channel concatenation of two tensors (x: C0 channels, x1: C - C0; both (primal | tangent) stacked when
  // dual): the decoder's cat([h, skip]) (model/unet.py:514) is never materialised.  out / gout stay ONE tensor of C
  // channels; the backward writes the input cotangent into gx (C0 channels) and gx1 (C - C0).
  const float* x1; int C0;
  float* gx1;
  int sub;      // reduce kernels: pixels per fp32 partial sum — fixed per sample, whatever the batch size
  int nch;      // pixel chunks (= slots) per sample of the reduce kernel that filled acc
  double* accf; // backward: the five moments summed over the slots, [Bp][G][8]
  float* pslots;// backward: dgamma | dbeta partials, [2][Bp * GN_SLOTS][C]
  const float* resid;   // backward apply: added to gx (skip-branch cotangent), may alias gx
  const float* resid2;  // a second addend (the cotangent that reached this tensor through the U-Net's skip stack)
  // dropout after the SiLU (model/unet.py:152-158), read by the DROP builds only: msgm_dropout_t's Philox state, stream,
  // keep threshold and scale
  const uint64_t* drng; uint32_t dstream, dthr; float dscale;
};

// ------------------------------------------------------------------ dropout mask (include/msgm_hip.h, msgm_dropout_t)
// The mask is never stored: every kernel that touches an element regenerates its keep bit from the Philox block of its
// channel quad.  The state words are read once per thread; the key / counter folding is msgm_philox's.
struct DropKey { uint64_t row0; uint32_t k0, k1, off, stream, thr; float s; };
__device__ __forceinline__ DropKey drop_key(const uint64_t* rng, uint32_t stream, uint32_t thr, float s) {
  const uint64_t seed = rng[0], off = rng[1];
  return DropKey{rng[2], (uint32_t)seed, (uint32_t)(seed >> 32) ^ (uint32_t)(off >> 32), (uint32_t)off, stream, thr, s};
}
// keep * scale of channels c .. c+3 (c % 4 == 0) of primal row b, pixel p: element e = ((row0 + b) P + p) C + c of the
// GLOBAL channels-last index, words 0..3 of Philox block e / 4; kept iff (word >> 8) >= thr
__device__ __forceinline__ f32x4 drop_mul4(const DropKey& k, int b, int P, int C, int p, int c) {
  const uint64_t q = (((k.row0 + (uint64_t)b) * (uint64_t)P + (uint64_t)p) * (uint64_t)C + (uint64_t)c) >> 2;
  const Philox4 r = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), k.stream, k.off, k.k0, k.k1);
  return f32x4{(r.x >> 8) >= k.thr ? k.s : 0.f, (r.y >> 8) >= k.thr ? k.s : 0.f, (r.z >> 8) >= k.thr ? k.s : 0.f,
               (r.w >> 8) >= k.thr ? k.s : 0.f};
}

// ---- the phases the four GroupNorm kernels share
// gn_lane: a thread's place in the 256-thread workgroup: channel vector cv (channels V*cv .. V*cv+V-1; V = 4 with VEC, else 1)
// of pixel lane pl, CV <= 256 vectors per pixel (VEC: C <= 1024), PL = 256 / CV pixel lanes, so PL C <= 1024 elements per LDS
// image.  Threads beyond CV*PL (C = 96: 240; C = 640: 160, one pixel lane) are not live: (0, 0).
struct GnLane { int cv, pl, CV, PL; bool live; };
template <bool VEC>
__device__ __forceinline__ GnLane gn_lane(int tid, int C) {
  const int CV = C / (VEC ? 4 : 1), PL = 256 / CV;
  const bool live = tid < CV * PL;
  return GnLane{live ? tid % CV : 0, live ? tid / CV : 0, CV, PL, live};
}

// gn_src: where channel c of the possibly two-source input lives.  `base` points at that channel in x (pitch C0) or in x1
// (pitch C - C0) — a channel vector never straddles the sources (C0 % 4 == 0) — so element (sample b, pixel p) is
// base[(b P + p) pitch]; `half` is the primal -> tangent offset of that source.
struct GnSrc { const float* base; long half; int pitch; };
__device__ __forceinline__ GnSrc gn_src(const GnArgs& A, int c) {
  const int C0 = A.x1 ? A.C0 : A.C;
  const bool second = c >= C0;
  const int pitch = second ? A.C - C0 : C0;
  return GnSrc{(second ? A.x1 : A.x) + (second ? c - C0 : c), (long)A.Bp * A.P * pitch, pitch};
}

// gn_pivot: the pivot of (sample b, group g) — the sample's own first pixel of the group's first channel.  The saved mean is
// kept RELATIVE to it (stats[0] = mean - pivot, rounded to fp32 from double) and xhat = ((x - pivot) - stats[0]) inv: a mean
// that is large against the spread would lose the group's position to the fp32 rounding of the mean itself
// (2^-25 |mean| / sigma in xhat), while x - pivot is (nearly) exact and what is left to round is of the size of sigma.
__device__ __forceinline__ float gn_pivot(const GnArgs& A, int b, int g, int cpg) {
  const GnSrc s = gn_src(A, g * cpg);
  return s.base[(long)b * A.P * s.pitch];
}

// gn_load_x: the thread's V primal elements at source offset ex and, when dual, their tangents (xd is left untouched
// otherwise).  VEC: one 16-byte load each.
template <bool VEC>
__device__ __forceinline__ void gn_load_x(const GnSrc& sx, long ex, bool dual, float (&x)[VEC ? 4 : 1], float (&xd)[VEC ? 4 : 1]) {
  if constexpr (VEC) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(sx.base + ex);
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = xv[k];
    if (dual) {
      const f32x4 dv = *reinterpret_cast<const f32x4*>(sx.base + ex + sx.half);
#pragma unroll
      for (int k = 0; k < 4; ++k) xd[k] = dv[k];
    }
  } else {
    x[0] = sx.base[ex];
    if (dual) xd[0] = sx.base[ex + sx.half];
  }
}

// gn_group_tail: the LDS tail of the reduce kernels.  red: nm images [pixel lane][C] of double partials, 1024 apart, visible
// (the caller's ONE barrier); one thread per (moment, group): the pixel lanes in order, the group's channels inside -> dst[g][m].
__device__ __forceinline__ void gn_group_tail(const double* red, double* dst, int nm, int tid, int C, int G, int PL) {
  const int cpg = C / G;
  for (int i = tid; i < nm * G; i += 256) {
    const int m = i / G, g = i - m * G;
    const double* r = red + m * 1024 + g * cpg;
    double t = 0.0;
    for (int p = 0; p < PL; ++p)
      for (int cc = 0; cc < cpg; ++cc) t += r[p * C + cc];
    dst[(size_t)g * 8 + m] = t;
  }
}

// Reduce kernels: every thread holds V double partials per moment (per-thread fp32 sums over one sub-chunk are widened and
// from there on everything is added in double).  ALL moments go to LDS at once and gn_group_tail finishes the chunk.
// The forward's fp32 sums run over u = x - k (k: pixel 0 of this sample, the same for every workgroup and batch size) and
// u xdot; with n the pixels this thread summed, sum x = s0 + n k, sum x^2 = s1 + 2 k s0 + n k^2, sum x xdot = s3 + k s2,
// in double.
template <bool VEC>
__global__ void __launch_bounds__(256) k_gn_fwd_reduce(GnArgs A) {
  constexpr int V = VEC ? 4 : 1;
  __shared__ double red[4 * 1024];       // all moments at once: ONE barrier in the tail instead of two per moment
  const int tid = threadIdx.x, b = blockIdx.x;
  const int C = A.C, P = A.P, G = A.G;
  const GnLane L = gn_lane<VEC>(tid, C);
  const GnSrc sx = gn_src(A, V * L.cv);
  const int p0 = blockIdx.y * A.chunk, p1 = min(p0 + A.chunk, P);
  double d0[V], d1[V], d2[V], d3[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { d0[k] = 0.0; d1[k] = 0.0; d2[k] = 0.0; d3[k] = 0.0; }
  float kx[V];
#pragma unroll
  for (int k = 0; k < V; ++k) kx[k] = 0.f;
  if (L.live) { float kz[V]; gn_load_x<VEC>(sx, (long)b * P * sx.pitch, false, kx, kz); }
  int n = 0;
  if (L.live)
   for (int ps = p0; ps < p1; ps += max(A.sub, 1)) {
    const int pe = min(ps + max(A.sub, 1), p1);
    float s0[V], s1[V], s2[V], s3[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { s0[k] = 0.f; s1[k] = 0.f; s2[k] = 0.f; s3[k] = 0.f; }
    for (int p = ps + L.pl; p < pe; p += L.PL) {
      float xv[V], dv[V];
      gn_load_x<VEC>(sx, ((long)b * P + p) * sx.pitch, A.dual, xv, dv);
      ++n;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const float u = xv[k] - kx[k];
        s0[k] += u; s1[k] += u * u;
        if (A.dual) { s2[k] += dv[k]; s3[k] += u * dv[k]; }
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) { d0[k] += (double)s0[k]; d1[k] += (double)s1[k]; d2[k] += (double)s2[k]; d3[k] += (double)s3[k]; }
   }
  if (L.live) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const double kk = (double)kx[k], nn = (double)n, u0 = d0[k];
      d0[k] = u0 + nn * kk; d1[k] = d1[k] + 2.0 * kk * u0 + nn * kk * kk;
      d3[k] = d3[k] + kk * d2[k];
      const int e = L.pl * C + V * L.cv + k;
      red[e] = d0[k]; red[1024 + e] = d1[k];
      if (A.dual) { red[2048 + e] = d2[k]; red[3072 + e] = d3[k]; }
    }
  }
  __syncthreads();
  gn_group_tail(red, A.acc + ((size_t)b * GN_SLOTS + blockIdx.y) * G * 8, A.dual ? 4 : 2, tid, C, G, L.PL);
}

// moments of (sample b, group g): the chunk slots added in chunk order.  The loads of up to 4 slots are issued before the
// first add (the slots are independent addresses; a plain loop waited for every slot's round trip in turn).
__device__ __forceinline__ void gn_sum_slots(const GnArgs& A, int b, int g, int nm, double (&a8)[8]) {
#pragma unroll
  for (int m = 0; m < 8; ++m) a8[m] = 0.0;
  const double* base = A.acc + ((size_t)b * GN_SLOTS * A.G + g) * 8;
  const size_t sstride = (size_t)A.G * 8;
  for (int ch0 = 0; ch0 < A.nch; ch0 += 4) {
    double v[4][5];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ch = min(ch0 + j, A.nch - 1);                // clamped: every load unconditional
      const double* p = base + (size_t)ch * sstride;
      const f64x2 q0 = *reinterpret_cast<const f64x2*>(p), q1 = *reinterpret_cast<const f64x2*>(p + 2);
      v[j][0] = q0[0]; v[j][1] = q0[1]; v[j][2] = q1[0]; v[j][3] = q1[1];
      v[j][4] = nm > 4 ? p[4] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (ch0 + j < A.nch) {
#pragma unroll
        for (int m = 0; m < 5; ++m) if (m < nm) a8[m] += v[j][m];
      }
  }
}

// kg: the group's pivot (0: mu is the mean itself)
__device__ __forceinline__ void gn_stats(const double* a8, double cnt, float eps, double kg, float& mu, float& inv, float& md, float& a) {
  const double m = a8[0] / cnt;
  double var = a8[1] / cnt - m * m;
  if (var < 0) var = 0;
  const double iv = 1.0 / sqrt(var + (double)eps);
  const double d = a8[2] / cnt;
  mu = (float)(m - kg); inv = (float)iv; md = (float)d;
  a = (float)(iv * (a8[3] / cnt - m * d));
}

// GroupNorm as a per-(sample, channel) affine map y = a x + b (a = gamma/sigma, b = beta - mean a) for a consumer that
// applies it while reading x (msgm_conv_forward_fused).  One block per sample.
__global__ void __launch_bounds__(256) k_gn_affine(GnArgs A, float* __restrict__ scale, float* __restrict__ shift) {
  const int b = blockIdx.x, cpg = A.C / A.G;
  const double cnt = (double)A.P * cpg;
  for (int c = threadIdx.x; c < A.C; c += 256) {
    float mu, inv, md, a;
    double a8[8];
    gn_sum_slots(A, b, c / cpg, 2, a8);
    gn_stats(a8, cnt, A.eps, 0.0, mu, inv, md, a);
    const float sc = inv * A.gamma[c];
    scale[(size_t)b * A.C + c] = sc;
    shift[(size_t)b * A.C + c] = A.beta[c] - mu * sc;
  }
}

// gn_consts: the constants of the thread's V channels c0 ..: {mean - pivot, inv_std, mean(xdot), a} of each one's group from the
// f32x4 table[row + group] (k_gn_fwd_apply: this sample's LDS copy, row 0; backward: A.stats, row b G), the group's pivot kg
// of sample b and the affine parameters.
template <int V> struct GnConsts { float mu[V], inv[V], md[V], a[V], ga[V], be[V], kg[V]; };
template <int V>
__device__ __forceinline__ GnConsts<V> gn_consts(const GnArgs& A, const f32x4* table, size_t row, int b, int c0, int cpg) {
  GnConsts<V> K;
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int c = c0 + k;
    const f32x4 st = table[row + c / cpg];
    K.mu[k] = st[0]; K.inv[k] = st[1]; K.md[k] = st[2]; K.a[k] = st[3];
    K.ga[k] = A.gamma[c]; K.be[k] = A.beta[c];
    K.kg[k] = gn_pivot(A, b, c / cpg, cpg);
  }
  return K;
}

// Elementwise pass.  VEC: grid (pixel chunk, sample); a thread owns 4 consecutive channels (its statistics and
// affine parameters are loaded once) and walks over pixels — 16-B loads/stores, consecutive threads on consecutive
// addresses.  !VEC (C % 4 != 0): one thread per channel, same walk.
// DROP (VEC only): the post-SiLU primal and tangent are multiplied by keep * scale of the dropout mask.
template <bool VEC, bool DROP = false>
__global__ void __launch_bounds__(256) k_gn_fwd_apply(GnArgs A) {
  static_assert(VEC || !DROP, "dropout masks are drawn per channel quad");
  constexpr int V = VEC ? 4 : 1;
  __shared__ f32x4 sst[64];
  const int C = A.C, P = A.P, G = A.G, cpg = C / G;
  const int tid = threadIdx.x, b = blockIdx.y;
  // {mean - pivot, inv_std, mean(xdot), a} of this sample's groups, rebuilt by every workgroup from the chunk slots the reduce
  // kernel left (thread g: the slots of group g in chunk order, in double — the arithmetic of the former one-thread-per-
  // (sample, group) finalise launch, which cost 5-10 us per GroupNorm at the 32-row shard for a few KB of work).
  // The sample's first workgroup keeps them for the backward.
  if (tid < G) {
    float mu, inv, md, a;
    double a8[8];
    const float kg = gn_pivot(A, b, tid, cpg);               // issued ahead of the slot loads, not after their sums
    gn_sum_slots(A, b, tid, A.dual ? 4 : 2, a8);
    gn_stats(a8, (double)P * cpg, A.eps, (double)kg, mu, inv, md, a);
    sst[tid] = f32x4{mu, inv, md, a};
    if (A.stats && blockIdx.x == 0) *reinterpret_cast<f32x4*>(A.stats + ((size_t)b * G + tid) * 4) = f32x4{mu, inv, md, a};
  }
  __syncthreads();
  const GnLane L = gn_lane<VEC>(tid, C);
  if (!L.live) return;
  const int cv = L.cv;
  const long tot = (long)A.Bp * P * C;
  const GnConsts<V> K = gn_consts<V>(A, sst, 0, b, V * cv, cpg);
  const int p0 = blockIdx.x * A.chunk, p1 = min(p0 + A.chunk, P);
  const GnSrc sx = gn_src(A, V * cv);
  DropKey dk;
  if constexpr (DROP) dk = drop_key(A.drng, A.dstream, A.dthr, A.dscale);
  for (int p = p0 + L.pl; p < p1; p += L.PL) {
    const long e = ((long)b * P + p) * C + V * cv;
    float x[V], xd[V], y[V], yd[V];
    gn_load_x<VEC>(sx, ((long)b * P + p) * sx.pitch, A.dual, x, xd);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const float xh = ((x[k] - K.kg[k]) - K.mu[k]) * K.inv[k];
      y[k] = K.ga[k] * xh + K.be[k];
      yd[k] = A.dual ? K.ga[k] * (K.inv[k] * ((xd[k] - K.md[k]) - xh * K.a[k])) : 0.f;
      if (A.silu) {
        float z0, z1, z2;
        silu012(y[k], z0, z1, z2);
        y[k] = z0; yd[k] = z1 * yd[k];
      }
    }
    if constexpr (DROP) {
      const f32x4 m = drop_mul4(dk, b, P, C, p, V * cv);
#pragma unroll
      for (int k = 0; k < V; ++k) { y[k] *= m[k]; yd[k] *= m[k]; }
    }
    if (VEC) {
      f32x4 o, od;
#pragma unroll
      for (int k = 0; k < V; ++k) { o[k] = y[k]; od[k] = yd[k]; }
      *reinterpret_cast<f32x4*>(A.out + e) = o;
      if (A.dual) *reinterpret_cast<f32x4*>(A.out + e + tot) = od;
    } else {
      A.out[e] = y[0];
      if (A.dual) A.out[e + tot] = yd[0];
    }
  }
}

// Backward over the dual pair.  With X = gamma*zbar, W = gamma*zdotbar (cotangents of xhat and of
// its tangent what = inv (xdot_c - xhat a)):
//   xdotbar = inv (W - mean W - xhat p),                      p = mean(xhat W)
//   xbar    = inv (X - mean X - xhat mean(xhat X)) - inv (c xhat + a xdotbar + p what),  c = mean(W what)
// (derived by hand, checked against autograd in tests/test_unet2d_gpu.py).
// DROP (VEC only): both incoming cotangents are multiplied by keep * scale as they are loaded (the moments see the masked
// cotangent), in this kernel and in k_gn_bwd_apply.
// gn_load_cot: both incoming cotangents (zb: of the output, zdb: of its tangent, `tot` floats later) of the thread's V
// channels at output offset e = ((b P + p) C + c); DROP multiplies them by the keep * scale of (b, p, c .. c+3).
template <bool VEC, bool DROP>
__device__ __forceinline__ void gn_load_cot(const GnArgs& A, const DropKey& dk, long e, long tot, int b, int p, int c,
                                            float (&zb)[VEC ? 4 : 1], float (&zdb)[VEC ? 4 : 1]) {
  if constexpr (VEC) {
    const f32x4 v2 = *reinterpret_cast<const f32x4*>(A.gout + e), v3 = *reinterpret_cast<const f32x4*>(A.gout + e + tot);
#pragma unroll
    for (int k = 0; k < 4; ++k) { zb[k] = v2[k]; zdb[k] = v3[k]; }
  } else {
    zb[0] = A.gout[e]; zdb[0] = A.gout[e + tot];
  }
  if constexpr (DROP) {
    const f32x4 m = drop_mul4(dk, b, A.P, A.C, p, c);
#pragma unroll
    for (int k = 0; k < 4; ++k) { zb[k] *= m[k]; zdb[k] *= m[k]; }
  }
}

// gn_bwd_elem: the backward's per-element chain for channel k of the thread's constants K — xh = xhat, wh = what, the
// cotangents (zbk, zdbk) pulled back through the SiLU when there is one, X = gamma zbar, W = gamma zdotbar.  The ONE text of
// it: k_gn_bwd_reduce sums moments of these quantities and k_gn_bwd_apply subtracts them, so both must see the same values.
struct GnElem { float xh, wh, zbk, zdbk, X, W; };
template <int V>
__device__ __forceinline__ GnElem gn_bwd_elem(float x, float xd, const GnConsts<V>& K, int k, int silu, float zb, float zdb) {
  GnElem E;
  E.xh = ((x - K.kg[k]) - K.mu[k]) * K.inv[k];
  E.wh = K.inv[k] * ((xd - K.md[k]) - E.xh * K.a[k]);
  E.zbk = zb; E.zdbk = zdb;
  if (silu) {
    float z0, z1, z2;
    silu012(K.ga[k] * E.xh + K.be[k], z0, z1, z2);
    const float yd = K.ga[k] * E.wh;
    const float nzb = E.zbk * z1 + E.zdbk * (z2 * yd);
    E.zdbk = E.zdbk * z1;
    E.zbk = nzb;
  }
  E.X = K.ga[k] * E.zbk; E.W = K.ga[k] * E.zdbk;
  return E;
}

template <bool VEC, bool DROP = false>
__global__ void __launch_bounds__(256) k_gn_bwd_reduce(GnArgs A) {
  static_assert(VEC || !DROP, "dropout masks are drawn per channel quad");
  constexpr int V = VEC ? 4 : 1;
  __shared__ double redd[5 * 1024];      // the five moments and (below) both parameter partials: ONE barrier in the tail
  __shared__ float red[2 * 1024];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int C = A.C, P = A.P, G = A.G, cpg = C / G;
  const GnLane L = gn_lane<VEC>(tid, C);
  const int cv = L.cv, pl = L.pl;
  const long tot = (long)A.Bp * P * C;
  const GnConsts<V> K = gn_consts<V>(A, reinterpret_cast<const f32x4*>(A.stats), (size_t)b * G, b, V * cv, cpg);
  const int p0 = blockIdx.y * A.chunk, p1 = min(p0 + A.chunk, P);
  const GnSrc sx = gn_src(A, V * cv);
  double dX[V], dXx[V], dW[V], dWx[V], dWw[V];
  float dga[V], dbe[V];
#pragma unroll
  for (int k = 0; k < V; ++k) { dX[k] = dXx[k] = dW[k] = dWx[k] = dWw[k] = 0.0; dga[k] = dbe[k] = 0.f; }
  DropKey dk;
  if constexpr (DROP) dk = drop_key(A.drng, A.dstream, A.dthr, A.dscale);
  if (L.live)
   for (int ps = p0; ps < p1; ps += max(A.sub, 1)) {
    const int pe = min(ps + max(A.sub, 1), p1);
    float sX[V], sXx[V], sW[V], sWx[V], sWw[V];
#pragma unroll
    for (int k = 0; k < V; ++k) { sX[k] = sXx[k] = sW[k] = sWx[k] = sWw[k] = 0.f; }
    for (int p = ps + pl; p < pe; p += L.PL) {
      float x[V], xd[V], zb[V], zdb[V];
      gn_load_x<VEC>(sx, ((long)b * P + p) * sx.pitch, true, x, xd);
      gn_load_cot<VEC, DROP>(A, dk, ((long)b * P + p) * C + V * cv, tot, b, p, V * cv, zb, zdb);
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const GnElem E = gn_bwd_elem(x[k], xd[k], K, k, A.silu, zb[k], zdb[k]);
        sX[k] += E.X; sXx[k] += E.X * E.xh; sW[k] += E.W; sWx[k] += E.W * E.xh; sWw[k] += E.W * E.wh;
        dga[k] += E.zbk * E.xh + E.zdbk * E.wh; dbe[k] += E.zbk;
      }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
      dX[k] += (double)sX[k]; dXx[k] += (double)sXx[k]; dW[k] += (double)sW[k]; dWx[k] += (double)sWx[k]; dWw[k] += (double)sWw[k];
    }
   }
  const size_t slot = (size_t)b * gridDim.y + blockIdx.y, nslots = (size_t)gridDim.x * gridDim.y;
  if (L.live) {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int e = pl * C + V * cv + k;
      redd[e] = dX[k]; redd[1024 + e] = dXx[k]; redd[2048 + e] = dW[k]; redd[3072 + e] = dWx[k]; redd[4096 + e] = dWw[k];
      red[e] = dga[k]; red[1024 + e] = dbe[k];
    }
  }
  __syncthreads();
  gn_group_tail(redd, A.acc + ((size_t)b * GN_SLOTS + blockIdx.y) * G * 8, 5, tid, C, G, L.PL);
  // per-channel parameter gradients: the pixel lanes in order, one value per channel into this (sample, chunk)'s slot
  for (int i = tid; i < 2 * C; i += 256) {
    const int which = i / C, c = i - which * C;
    float t = 0.f;
    for (int p = 0; p < L.PL; ++p) t += red[which * 1024 + p * C + c];
    A.pslots[((size_t)which * nslots + slot) * C + c] = t;
  }
}

// dgamma[c] += sum over the (sample, chunk) slots, dbeta alike (blockIdx.y = 0 / 1): 32 channels x 32 slot slices per
// workgroup (1024 threads: the grid is only C/32 x 2 workgroups, so the parallelism has to come from inside), every
// slice walks its slots in order and the 32 slices are added in order — no atomics, same bits every run.
__global__ void __launch_bounds__(1024) k_gn_param_reduce(const float* __restrict__ pslots, size_t nslots, int C,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, int nbc) {
  __shared__ float red[32][32];
  const int bid = blockIdx.x, bx = bid % nbc, by = bid / nbc;
  const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int c = bx * 32 + cl;
  const float* p = pslots + (size_t)by * nslots * C;
  float t = 0.f;
  if (c < C)
    for (size_t s = sl; s < nslots; s += 32) t += p[s * C + c];
  red[sl][cl] = t;
  __syncthreads();
  if (sl == 0 && c < C) {
    float r = red[0][cl];
#pragma unroll
    for (int k = 1; k < 32; ++k) r += red[k][cl];
    float* dst = by == 0 ? dgamma : dbeta;
    dst[c] += r;
  }
}

template <bool VEC, bool DROP = false>
__global__ void __launch_bounds__(256) k_gn_bwd_apply(GnArgs A) {
  static_assert(VEC || !DROP, "dropout masks are drawn per channel quad");
  constexpr int V = VEC ? 4 : 1;
  const int C = A.C, P = A.P, G = A.G, cpg = C / G;
  const int tid = threadIdx.x, b = blockIdx.y;
  // the five backward moments of this sample's groups: every workgroup adds the reduce kernel's chunk slots itself (thread
  // g, chunk order, double) instead of a finalise launch in between
  __shared__ float sm5[64][5];
  if (tid < G) {
    double a8[8];
    gn_sum_slots(A, b, tid, 5, a8);
#pragma unroll
    for (int m = 0; m < 5; ++m) sm5[tid][m] = (float)a8[m];
  }
  __syncthreads();
  const GnLane L = gn_lane<VEC>(tid, C);
  if (!L.live) return;
  const int cv = L.cv;
  const long tot = (long)A.Bp * P * C;
  const float rc = 1.0f / ((float)P * (float)cpg);
  const GnConsts<V> K = gn_consts<V>(A, reinterpret_cast<const f32x4*>(A.stats), (size_t)b * G, b, V * cv, cpg);
  float mX[V], mXx[V], mW[V], pp[V], cc[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const int g = (V * cv + k) / cpg;
    mX[k] = sm5[g][0] * rc; mXx[k] = sm5[g][1] * rc; mW[k] = sm5[g][2] * rc; pp[k] = sm5[g][3] * rc;
    cc[k] = sm5[g][4] * rc;
  }
  const int p0 = blockIdx.x * A.chunk, p1 = min(p0 + A.chunk, P);
  const GnSrc sx = gn_src(A, V * cv);
  // destination of the input cotangent: the source's own tensor when the input is a concatenation
  float* gbase = A.x1 ? ((V * cv >= A.C0) ? A.gx1 + (V * cv - A.C0) : A.gx + V * cv) : A.gx + V * cv;
  const float* rbase = A.resid ? A.resid + V * cv : nullptr;            // single-source only (host checks)
  const float* rbase2 = A.resid2 ? A.resid2 + V * cv : nullptr;
  DropKey dk;
  if constexpr (DROP) dk = drop_key(A.drng, A.dstream, A.dthr, A.dscale);
  for (int p = p0 + L.pl; p < p1; p += L.PL) {
    const long ex = ((long)b * P + p) * sx.pitch;
    float x[V], xd[V], zb[V], zdb[V], xb[V], xdb[V];
    gn_load_x<VEC>(sx, ex, true, x, xd);
    gn_load_cot<VEC, DROP>(A, dk, ((long)b * P + p) * C + V * cv, tot, b, p, V * cv, zb, zdb);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const GnElem E = gn_bwd_elem(x[k], xd[k], K, k, A.silu, zb[k], zdb[k]);
      xdb[k] = K.inv[k] * (E.W - mW[k] - E.xh * pp[k]);
      xb[k] = K.inv[k] * (E.X - mX[k] - E.xh * mXx[k]) - K.inv[k] * (cc[k] * E.xh + K.a[k] * xdb[k] + pp[k] * E.wh);
    }
    if (VEC) {
      f32x4 o, od;
#pragma unroll
      for (int k = 0; k < V; ++k) { o[k] = xb[k]; od[k] = xdb[k]; }
      if (rbase) { o += *reinterpret_cast<const f32x4*>(rbase + ex); od += *reinterpret_cast<const f32x4*>(rbase + ex + sx.half); }
      if (rbase2) { o += *reinterpret_cast<const f32x4*>(rbase2 + ex); od += *reinterpret_cast<const f32x4*>(rbase2 + ex + sx.half); }
      *reinterpret_cast<f32x4*>(gbase + ex) = o;
      *reinterpret_cast<f32x4*>(gbase + ex + sx.half) = od;
    } else {
      gbase[ex] = xb[0] + (rbase ? rbase[ex] : 0.f) + (rbase2 ? rbase2[ex] : 0.f);
      gbase[ex + sx.half] = xdb[0] + (rbase ? rbase[ex + sx.half] : 0.f) + (rbase2 ? rbase2[ex + sx.half] : 0.f);
    }
  }
}

// ------------------------------------------------------------------ batched GEMM
// C[b](i,j) (+)= alpha * ( sum_k A[b](i,k) B[b](k,j)  [+ sum_k A2[b](i,k) B2[b](k,j)] ) with element strides.
// The optional second operand pair (same strides) fuses the two-term products of the dual attention
// (Wdot = qdot k^T + q kdot^T, adot = Pdot v + P vdot, and their adjoints) into one pass over the output.
// One wave computes a (16 MT) x (16 NT) tile, 4 waves a 2x2 arrangement.  K runs in groups of 16 with the
// permuted mapping k = 16g + 4q + r (lane quarter q, MFMA step r): an operand that is contiguous along K is
// read with one 16-B load per group (AVEC / BVEC), otherwise with 4 coalesced dword loads.  The host swaps the
// operand roles so that the output's contiguous dimension is the MFMA row index: the 4 accumulator registers of
// a lane are then 4 consecutive addresses and the tile is stored with 16-B stores (CVEC).
struct BmmArgs {
  const float* A; const float* B; const float* A2; const float* B2; float* C;
  int M, N, K, batch;
  long sAb, sAi, sAk, sBb, sBk, sBj, sCb, sCi, sCj;
  float alpha; int accumulate;
  // DUAL: a second output C3 = alpha * A3 . B that shares the (big) B operand of the first pair — the dual-number
  // attention always needs P v next to Pdot v + P vdot (and the three adjoint pairs alike), so the (T,T) operand is
  // streamed once for both.  A3 has A's strides, C3 has C's.
  const float* A3; float* C3;
};
template <bool VEC>
__device__ __forceinline__ f32x4 bmm_frag(const float* p, long sk, bool valid) {
  if (!valid) return f32x4{0, 0, 0, 0};
  if (VEC) return *reinterpret_cast<const f32x4*>(p);
  return f32x4{p[0], p[sk], p[2 * sk], p[3 * sk]};
}
template <int MT, int NT, bool AVEC, bool BVEC, bool DUAL = false>
__global__ void __launch_bounds__(256) k_bmm(BmmArgs P) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, il = lane & 15, q = lane >> 4;
  const int tiles_n = (P.N + 32 * NT - 1) / (32 * NT);
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const int i0 = tm * 32 * MT + (w >> 1) * 16 * MT, j0 = tn * 32 * NT + (w & 1) * 16 * NT;
  if (i0 >= P.M || j0 >= P.N) return;
  f32x4 acc[MT][NT], acc3[DUAL ? MT : 1][DUAL ? NT : 1];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) { acc[m][n] = f32x4{0, 0, 0, 0}; if (DUAL) acc3[m][n] = f32x4{0, 0, 0, 0}; }
  bool vi[MT], vj[NT];
#pragma unroll
  for (int m = 0; m < MT; ++m) vi[m] = i0 + 16 * m + il < P.M;
#pragma unroll
  for (int n = 0; n < NT; ++n) vj[n] = j0 + 16 * n + il < P.N;
  const int ngroups = P.K >> 4;                     // host guarantees K % 16 == 0
  for (int pair = 0; pair < 2; ++pair) {
    const float* Ab = (pair ? P.A2 : P.A);
    const float* Bb = (pair ? P.B2 : P.B);
    if (!Ab) break;
    Ab += (size_t)blockIdx.y * P.sAb;
    Bb += (size_t)blockIdx.y * P.sBb;
    const float* ap[MT];
    const float* bp[NT];
#pragma unroll
    for (int m = 0; m < MT; ++m) ap[m] = Ab + (size_t)(vi[m] ? i0 + 16 * m + il : 0) * P.sAi + (size_t)(4 * q) * P.sAk;
#pragma unroll
    for (int n = 0; n < NT; ++n) bp[n] = Bb + (size_t)(vj[n] ? j0 + 16 * n + il : 0) * P.sBj + (size_t)(4 * q) * P.sBk;
    const size_t stepA = (size_t)16 * P.sAk, stepB = (size_t)16 * P.sBk;
    const bool third = DUAL && pair == 0;                 // A3 rides along with the first pair's B operand
    const float* ap3[MT];
    f32x4 na[MT], nb[NT], na3[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) na[m] = bmm_frag<AVEC>(ap[m], P.sAk, vi[m]);
#pragma unroll
    for (int n = 0; n < NT; ++n) nb[n] = bmm_frag<BVEC>(bp[n], P.sBk, vj[n]);
    if (third) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        ap3[m] = P.A3 + (size_t)blockIdx.y * P.sAb + (size_t)(vi[m] ? i0 + 16 * m + il : 0) * P.sAi + (size_t)(4 * q) * P.sAk;
        na3[m] = bmm_frag<AVEC>(ap3[m], P.sAk, vi[m]);
      }
    }
    for (int g = 0; g < ngroups; ++g) {
      f32x4 a[MT], b[NT], a3[MT];
#pragma unroll
      for (int m = 0; m < MT; ++m) { a[m] = na[m]; ap[m] += stepA; if (third) { a3[m] = na3[m]; ap3[m] += stepA; } }
#pragma unroll
      for (int n = 0; n < NT; ++n) { b[n] = nb[n]; bp[n] += stepB; }
      if (g + 1 < ngroups) {
#pragma unroll
        for (int m = 0; m < MT; ++m) na[m] = bmm_frag<AVEC>(ap[m], P.sAk, vi[m]);
#pragma unroll
        for (int n = 0; n < NT; ++n) nb[n] = bmm_frag<BVEC>(bp[n], P.sBk, vj[n]);
        if (third) {
#pragma unroll
          for (int m = 0; m < MT; ++m) na3[m] = bmm_frag<AVEC>(ap3[m], P.sAk, vi[m]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            acc[m][n] = mfma16(a[m][r], b[n][r], acc[m][n]);
            if (third) acc3[m][n] = mfma16(a3[m][r], b[n][r], acc3[m][n]);
          }
    }
  }
#pragma unroll
  for (int which = 0; which < (DUAL ? 2 : 1); ++which) {
  float* Cb = (which ? P.C3 : P.C) + (size_t)blockIdx.y * P.sCb;
  const bool cvec = P.sCi == 1 && (P.sCj & 3) == 0 && (P.sCb & 3) == 0 && ((reinterpret_cast<uintptr_t>(which ? P.C3 : P.C) & 15) == 0);
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int j = j0 + 16 * n + il;
      if (j >= P.N) continue;
      const int i = i0 + 16 * m + 4 * q;
      if (i >= P.M) continue;
      f32x4 v = P.alpha * (which ? acc3[DUAL ? m : 0][DUAL ? n : 0] : acc[m][n]);
      if (cvec && i + 3 < P.M) {
        float* cp = Cb + (size_t)j * P.sCj + i;
        if (P.accumulate) v += *reinterpret_cast<const f32x4*>(cp);
        *reinterpret_cast<f32x4*>(cp) = v;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (i + r >= P.M) continue;
          float* cp = Cb + (size_t)(i + r) * P.sCi + (size_t)j * P.sCj;
          *cp = P.accumulate ? *cp + v[r] : v[r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------ batched GEMM, LDS-staged
// The same contract as k_bmm (BmmArgs), for operands with ONE unit stride each: a workgroup owns a 64 x 64 output tile
// and walks K in blocks of 32.  Per block the A rows [64][32], the B columns [64][32] (and the A3 rows when DUAL) are
// brought in with coalesced 16-byte global loads — along k when k is the contiguous index (KV), along the row index when
// the operand is stored transposed (RV: the float4 is scattered into four LDS rows) — into a canonical [row][k] LDS image
// (pitch 36 floats), double-buffered, with the next block's loads in flight during this block's MFMAs.  Every wave then
// reads its fragments with ds_read_b128, like k_conv_tile.  k_bmm (register-direct, no LDS) stays as the fallback for
// operands without a unit stride / unaligned bases.
#define BL_P 36
enum { BL_KV = 0, BL_RV = 1 };
template <int MODE>
__device__ __forceinline__ void bl_load(f32x4 (&dst)[2], const float* base, long sRow, long sK, int row0, int rmax, int k0, int tid) {
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    f32x4 v = {0, 0, 0, 0};
    if (MODE == BL_KV) {
      const int row = (tid >> 3) + 32 * ps, k4 = tid & 7;
      if (row0 + row < rmax) v = *reinterpret_cast<const f32x4*>(base + (size_t)(row0 + row) * sRow + k0 + 4 * k4);
    } else {
      // lanes run along k (32 consecutive k of one row quad): the transposed LDS store below then hits 32 distinct banks per
      // half wave (with lanes along the rows it was an 8-way conflict: PMC LDSBankConflict 27-37 % in these kernels)
      const int kk = tid & 31, r4 = (tid >> 5) + 8 * ps;
      if (row0 + 4 * r4 < rmax) v = *reinterpret_cast<const f32x4*>(base + (size_t)(k0 + kk) * sK + row0 + 4 * r4);
    }
    dst[ps] = v;
  }
}
template <int MODE>
__device__ __forceinline__ void bl_store(float* L, const f32x4 (&src)[2], int tid) {
#pragma unroll
  for (int ps = 0; ps < 2; ++ps) {
    if (MODE == BL_KV) {
      const int row = (tid >> 3) + 32 * ps, k4 = tid & 7;
      *reinterpret_cast<f32x4*>(L + row * BL_P + 4 * k4) = src[ps];
    } else {
      const int kk = tid & 31, r4 = (tid >> 5) + 8 * ps;
#pragma unroll
      for (int r = 0; r < 4; ++r) L[(4 * r4 + r) * BL_P + kk] = src[ps][r];
    }
  }
}

template <int AMODE, int BMODE, bool DUAL>
__global__ void __launch_bounds__(256) k_bmm_lds(BmmArgs P) {
  __shared__ __attribute__((aligned(16))) float lds[2][(DUAL ? 3 : 2) * 64 * BL_P];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, il = lane & 15, q = lane >> 4;
  const int tiles_n = (P.N + 63) / 64;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const int i0 = tm * 64, j0 = tn * 64;
  const int wi = (w >> 1) * 32, wj = (w & 1) * 32;
  f32x4 acc[2][2], acc3[DUAL ? 2 : 1][DUAL ? 2 : 1];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) { acc[m][n] = f32x4{0, 0, 0, 0}; if (DUAL) acc3[m][n] = f32x4{0, 0, 0, 0}; }
  const int nkb = P.K >> 5;                               // host guarantees K % 32 == 0
  const int npairs = P.A2 ? 2 : 1;
  const int total = nkb * npairs;                         // the second operand pair simply continues the K loop
  f32x4 ra[2], rb[2], ra3[2];
  auto gload = [&](int it) __attribute__((always_inline)) {
    const int pair = it / nkb, k0 = (it - pair * nkb) * 32;
    const float* Ab = (pair ? P.A2 : P.A) + (size_t)blockIdx.y * P.sAb;
    const float* Bb = (pair ? P.B2 : P.B) + (size_t)blockIdx.y * P.sBb;
    bl_load<AMODE>(ra, Ab, P.sAi, P.sAk, i0, P.M, k0, tid);
    bl_load<BMODE>(rb, Bb, P.sBj, P.sBk, j0, P.N, k0, tid);
    if (DUAL) {
      if (pair == 0) bl_load<AMODE>(ra3, P.A3 + (size_t)blockIdx.y * P.sAb, P.sAi, P.sAk, i0, P.M, k0, tid);
    }
  };
  auto lstore = [&](int buf, int it) __attribute__((always_inline)) {
    float* L = lds[buf];
    bl_store<AMODE>(L, ra, tid);
    bl_store<BMODE>(L + 64 * BL_P, rb, tid);
    if (DUAL) {
      if (it < nkb) bl_store<AMODE>(L + 128 * BL_P, ra3, tid);
    }
  };
  gload(0);
  lstore(0, 0);
  __syncthreads();
  for (int it = 0; it < total; ++it) {
    const int cur = it & 1;
    if (it + 1 < total) gload(it + 1);
    const float* LA = lds[cur];
    const float* LB = LA + 64 * BL_P;
    const float* LA3 = LA + 128 * BL_P;
    const bool third = DUAL && it < nkb;                  // A3 rides along with the first pair's B operand
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      f32x4 a[2], b[2], a3[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        a[m] = *reinterpret_cast<const f32x4*>(LA + (wi + 16 * m + il) * BL_P + 16 * g + 4 * q);
        if (third) a3[m] = *reinterpret_cast<const f32x4*>(LA3 + (wi + 16 * m + il) * BL_P + 16 * g + 4 * q);
      }
#pragma unroll
      for (int n = 0; n < 2; ++n) b[n] = *reinterpret_cast<const f32x4*>(LB + (wj + 16 * n + il) * BL_P + 16 * g + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n) {
            acc[m][n] = mfma16(a[m][r], b[n][r], acc[m][n]);
            if (third) acc3[m][n] = mfma16(a3[m][r], b[n][r], acc3[m][n]);
          }
    }
    if (it + 1 < total) lstore(cur ^ 1, it + 1);          // the other buffer: its readers finished before the last barrier
    __syncthreads();
  }
#pragma unroll
  for (int which = 0; which < (DUAL ? 2 : 1); ++which) {
    float* Cb = (which ? P.C3 : P.C) + (size_t)blockIdx.y * P.sCb;
    const bool cvec = P.sCi == 1 && (P.sCj & 3) == 0 && (P.sCb & 3) == 0 && ((reinterpret_cast<uintptr_t>(which ? P.C3 : P.C) & 15) == 0);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        const int j = j0 + wj + 16 * n + il;
        if (j >= P.N) continue;
        const int i = i0 + wi + 16 * m + 4 * q;
        if (i >= P.M) continue;
        f32x4 v = P.alpha * (which ? acc3[DUAL ? m : 0][DUAL ? n : 0] : acc[m][n]);
        if (cvec && i + 3 < P.M) {
          float* cp = Cb + (size_t)j * P.sCj + i;
          if (P.accumulate) v += *reinterpret_cast<const f32x4*>(cp);
          *reinterpret_cast<f32x4*>(cp) = v;
        } else {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (i + r >= P.M) continue;
            float* cp = Cb + (size_t)(i + r) * P.sCi + (size_t)j * P.sCj;
            *cp = P.accumulate ? *cp + v[r] : v[r];
          }
        }
      }
  }
}

// generic-K fallback (K % 16 != 0): scalar, one k per lane quarter.  DUAL: the second output C3 = alpha A3.B rides along
// with the first pair's B element in an accumulator chain of its own (two independent chains also hide the MFMA's
// dependent latency); k runs in the same order for both outputs, so C3 is bitwise what a launch of its own would give.
template <bool DUAL>
__global__ void __launch_bounds__(256) k_bmm_slow(BmmArgs P) {
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, il = lane & 15, q = lane >> 4;
  const int tiles_n = (P.N + 31) / 32;
  const int tm = blockIdx.x / tiles_n, tn = blockIdx.x - tm * tiles_n;
  const int i0 = tm * 32 + (w >> 1) * 16, j0 = tn * 32 + (w & 1) * 16;
  if (i0 >= P.M || j0 >= P.N) return;
  f32x4 acc = {0, 0, 0, 0}, acc3 = {0, 0, 0, 0};
  const bool vi = i0 + il < P.M, vj = j0 + il < P.N;
  for (int pair = 0; pair < 2; ++pair) {
    const float* Ab = (pair ? P.A2 : P.A);
    const float* Bb = (pair ? P.B2 : P.B);
    if (!Ab) break;
    const size_t offA = (size_t)blockIdx.y * P.sAb + (size_t)(vi ? i0 + il : 0) * P.sAi;
    Ab += offA;
    Bb += (size_t)blockIdx.y * P.sBb + (size_t)(vj ? j0 + il : 0) * P.sBj;
    const bool third = DUAL && pair == 0;
    const float* Ab3 = third ? P.A3 + offA : nullptr;
    for (int k0 = 0; k0 < P.K; k0 += 4) {
      const int k = k0 + q;
      const float a = (vi && k < P.K) ? Ab[(size_t)k * P.sAk] : 0.f;
      const float b = (vj && k < P.K) ? Bb[(size_t)k * P.sBk] : 0.f;
      acc = mfma16(a, b, acc);
      if (third) {
        const float a3 = (vi && k < P.K) ? Ab3[(size_t)k * P.sAk] : 0.f;
        acc3 = mfma16(a3, b, acc3);
      }
    }
  }
  const int j = j0 + il;
  if (j >= P.N) return;
#pragma unroll
  for (int which = 0; which < (DUAL ? 2 : 1); ++which) {
    float* Cb = (which ? P.C3 : P.C) + (size_t)blockIdx.y * P.sCb;
    const f32x4 av = which ? acc3 : acc;
    for (int r = 0; r < 4; ++r) {
      const int i = i0 + 4 * q + r;
      if (i >= P.M) continue;
      float* cp = Cb + (size_t)i * P.sCi + (size_t)j * P.sCj;
      const float v = P.alpha * av[r];
      *cp = P.accumulate ? *cp + v : v;
    }
  }
}

// ------------------------------------------------------------------ dual softmax rows
// forward: S (primal logits, in place -> P); Wd (tangent logits, kept); Pd <- P (Wd - sum P Wd)
__global__ void __launch_bounds__(256) k_softmax_dual_fwd(float* __restrict__ S, const float* __restrict__ Wd,
                                                          float* __restrict__ Pd, long rows, int T, int dual) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float* s = S + row * T;
  float mx = -3.0e38f;
  for (int j = lane; j < T; j += 64) mx = fmaxf(mx, s[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float sum = 0.f;
  for (int j = lane; j < T; j += 64) { const float e = expf(s[j] - mx); s[j] = e; sum += e; }
  sum = wave_sum(sum);
  const float rs = 1.0f / sum;
  float r = 0.f;
  for (int j = lane; j < T; j += 64) {
    const float p = s[j] * rs;
    s[j] = p;
    if (dual) r += p * Wd[row * T + j];
  }
  if (dual) {
    r = wave_sum(r);
    for (int j = lane; j < T; j += 64) Pd[row * T + j] = s[j] * (Wd[row * T + j] - r);
  }
}
// backward (in place): Pb <- Wbar, Pdb <- Wdbar given P, Wd
__global__ void __launch_bounds__(256) k_softmax_dual_bwd(const float* __restrict__ Pm, const float* __restrict__ Wd,
                                                          float* __restrict__ Pb, float* __restrict__ Pdb, long rows, int T) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const float* p = Pm + row * T;
  const float* wd = Wd + row * T;
  float* pb = Pb + row * T;
  float* pdb = Pdb + row * T;
  float r = 0.f, m = 0.f;
  for (int j = lane; j < T; j += 64) { r += p[j] * wd[j]; m += p[j] * pdb[j]; }
  r = wave_sum(r); m = wave_sum(m);
  float s2 = 0.f;
  for (int j = lane; j < T; j += 64) {
    const float pt = pb[j] + pdb[j] * (wd[j] - r) - wd[j] * m;
    pb[j] = pt;
    s2 += p[j] * pt;
  }
  s2 = wave_sum(s2);
  for (int j = lane; j < T; j += 64) {
    pb[j] = p[j] * (pb[j] - s2);
    pdb[j] = p[j] * (pdb[j] - m);
  }
}

// ------------------------------------------------------------------ embedding / layout glue
// emb[b][j] = cos(t_b f_j), emb[b][half + j] = sin(t_b f_j), f_j = exp(-ln(max_period) j / half)
__global__ void k_timestep_embedding(const float* __restrict__ t, float* __restrict__ emb, int B, int dim, float max_period) {
  const int half = dim / 2;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < B * dim; e += gridDim.x * blockDim.x) {
    const int b = e / dim, j = e - b * dim;
    float v = 0.f;
    if (j < 2 * half) {
      const int jj = j < half ? j : j - half;
      const float f = expf(-logf(max_period) * (float)jj / (float)half);
      const float arg = t[b] * f;
      v = j < half ? cosf(arg) : sinf(arg);
    }
    emb[e] = v;
  }
}
// dual-number version for an argument that depends on the input (log-radius conditioning, NNUnet.py:101-105):
// rows b < Bp primal, rows Bp + b hold the tangent tdot:  d/dt cos(t f) = -f sin(t f) tdot, d/dt sin = f cos tdot
__global__ void k_timestep_embedding_dual(const float* __restrict__ t, float* __restrict__ emb, int Bp, int dim, float max_period) {
  const int half = dim / 2;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < Bp * dim; e += gridDim.x * blockDim.x) {
    const int b = e / dim, j = e - b * dim;
    float v = 0.f, vd = 0.f;
    if (j < 2 * half) {
      const int jj = j < half ? j : j - half;
      const float f = expf(-logf(max_period) * (float)jj / (float)half);
      const float arg = t[b] * f, td = t[Bp + b];
      const float c = cosf(arg), s = sinf(arg);
      v = j < half ? c : s;
      vd = j < half ? -f * s * td : f * c * td;
    }
    emb[e] = v;
    emb[(size_t)Bp * dim + e] = vd;
  }
}

// NormalizeLogRadius on dual numbers (NN.py:56-70 followed by the x sqrt(n) rescale of NNUnet.py:205 /
// NNUnet1D.py:134): r = |x| + eps; out = scale x / r; logr = log r; tangent: rdot = x.xdot/|x|,
// outdot = scale (xdot / r - x rdot / r^2), logr_dot = rdot / r.   One wave per row.
__global__ void __launch_bounds__(256) k_normalize_dual(const float* __restrict__ x, float* __restrict__ out,
                                                        float* __restrict__ logr, int Bp, int n, int dual, float scale,
                                                        float eps) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= Bp) return;
  const float* xp = x + (size_t)b * n;
  const float* xt = x + (size_t)(b + Bp) * n;
  float ss = 0.f, sd = 0.f;
  for (int i = lane; i < n; i += 64) { const float v = xp[i]; ss += v * v; if (dual) sd += v * xt[i]; }
  ss = wave_sum(ss);
  if (dual) sd = wave_sum(sd);
  const float nr = sqrtf(ss), r = nr + eps;
  const float rdot = dual ? sd / nr : 0.f;
  for (int i = lane; i < n; i += 64) {
    const float v = xp[i];
    out[(size_t)b * n + i] = scale * (v / r);
    if (dual) out[(size_t)(b + Bp) * n + i] = scale * (xt[i] / r - v * rdot / (r * r));
  }
  if (lane == 0) { logr[b] = logf(r); if (dual) logr[Bp + b] = rdot / r; }
}

// flat (B, C*H*W) channel-major, per-channel 'C' (h*W+w) or 'F' (w*H+h) order  <->  [B][H][W][C], with scale
__global__ void k_flat_to_cl(const float* __restrict__ flat, float* __restrict__ img, int B, int C, int H, int W, int forder,
                             float scale) {
  const long tot = (long)B * H * W * C;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int w = (int)((e / C) % W);
    const int h = (int)((e / ((long)C * W)) % H);
    const long b = e / ((long)C * W * H);
    const long idx = forder ? (long)w * H + h : (long)h * W + w;
    img[e] = flat[(b * C + c) * (long)H * W + idx] * scale;
  }
}
__global__ void k_cl_to_flat(const float* __restrict__ img, float* __restrict__ flat, int B, int C, int H, int W, int forder,
                             float scale) {
  const long tot = (long)B * H * W * C;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int w = (int)((e / C) % W);
    const int h = (int)((e / ((long)C * W)) % H);
    const long b = e / ((long)C * W * H);
    const long idx = forder ? (long)w * H + h : (long)h * W + w;
    flat[(b * C + c) * (long)H * W + idx] = img[e] * scale;
  }
}
// out[n][h][w][c] = sum of the 2x2 block of in[n][2h+dh][2w+dw][c]
__global__ void k_sum2x2(const float* __restrict__ in, float* __restrict__ out, int N, int H, int W, int C) {
  const long tot = (long)N * H * W * C;
  for (long e = blockIdx.x * (long)blockDim.x + threadIdx.x; e < tot; e += (long)gridDim.x * blockDim.x) {
    const int c = (int)(e % C);
    const int w = (int)((e / C) % W);
    const int h = (int)((e / ((long)C * W)) % H);
    const long n = e / ((long)C * W * H);
    const float* p = in + ((n * 2 * H + 2 * h) * (long)(2 * W) + 2 * w) * C + c;
    out[e] = (p[0] + p[C]) + (p[(long)2 * W * C] + p[(long)2 * W * C + C]);
  }
}

// ------------------------------------------------------------------ embedding-projection bank
// Every ResBlock projects the SAME time embedding through its own Linear(4*mc -> co) (emb_layers, model/unet.py:145-151,
// applied at :176-180).  Upstream that is 22 tiny GEMMs forward and 22 x (wgrad + bias sum + dgrad) backward per step —
// 4-16 us launches that are pure latency at the 32-row shard.  The bank runs them as ONE launch per direction straight on
// the PyTorch-layout parameters (no packed images): job j = one ResBlock; a workgroup owns 32 output channels of one job.
//   forward : out_j[r][c]  = (r < n_bias ? b_j[c] : 0) + sum_k semb[r][k] W_j[c][k]
//   wgrad   : dW_j[c][k]   = sum_r dout_j[r][c] semb[r][k]          (rows in order: deterministic)
//             db_j[c]      = sum_{r < n_bias} dout_j[r][c]          (also written to db2_j: the conv bias that is added at
//                                                                    the same place has the same gradient)
//   dgrad   : dsemb[r][k]  = sum_j sum_c dout_j[r][c] W_j[c][k]     (jobs and channels in order)
// K <= 512 and a multiple of 4; out_j / dout_j are [rows][co] contiguous per job.
#define EB_ROWS 64
template <int MODE>    // 0 forward, 1 wgrad
__global__ void __launch_bounds__(256) k_emb_bank(const msgm_emb_job_t* __restrict__ jobs, int n_jobs, const float* __restrict__ semb,
                                                  int R, int K, int n_bias) {
  extern __shared__ float lds[];
  const int KP = K + 4;                              // pitch: rows 16-byte aligned, consecutive rows on different banks
  float* sS = lds;                                   // [EB_ROWS][KP]   semb rows of the current row tile
  float* sW = lds + EB_ROWS * KP;                    // forward: [32][KP] weight rows; wgrad: [EB_ROWS][32] dout tile
  int lo = 0, hi = n_jobs - 1;
  const int blk = blockIdx.x;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].block_begin <= blk) lo = mid; else hi = mid - 1; }
  const msgm_emb_job_t J = jobs[lo];
  const int c0 = (blk - J.block_begin) * 32, tid = threadIdx.x;
  const int K4 = K >> 2;
  if (MODE == 0) {
    for (int i = tid; i < 32 * K4; i += 256) {       // weight rows c0..c0+31, coalesced 16-byte loads
      const int c = i / K4, k4 = i - c * K4;
      f32x4 w = f32x4{0.f, 0.f, 0.f, 0.f};
      if (c0 + c < J.co) w = *reinterpret_cast<const f32x4*>(J.W + (size_t)(c0 + c) * K + 4 * k4);
      *reinterpret_cast<f32x4*>(sW + c * KP + 4 * k4) = w;
    }
    const int cl = tid & 31, rg = tid >> 5;
    const bool okc = c0 + cl < J.co;
    const float bias = (okc && J.b) ? J.b[c0 + cl] : 0.f;
    for (int r0 = blockIdx.y * EB_ROWS; r0 < R; r0 += gridDim.y * EB_ROWS) {
      __syncthreads();
      for (int i = tid; i < EB_ROWS * K4; i += 256) {
        const int r = i / K4, k4 = i - r * K4;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r0 + r < R) v = *reinterpret_cast<const f32x4*>(semb + (size_t)(r0 + r) * K + 4 * k4);
        *reinterpret_cast<f32x4*>(sS + r * KP + 4 * k4) = v;
      }
      __syncthreads();
      float acc[EB_ROWS / 8];
#pragma unroll
      for (int j = 0; j < EB_ROWS / 8; ++j) acc[j] = 0.f;
      for (int k4 = 0; k4 < K4; ++k4) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(sW + cl * KP + 4 * k4);
#pragma unroll
        for (int j = 0; j < EB_ROWS / 8; ++j) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(sS + (rg + 8 * j) * KP + 4 * k4);
          acc[j] = fmaf(v[0], w[0], acc[j]); acc[j] = fmaf(v[1], w[1], acc[j]);
          acc[j] = fmaf(v[2], w[2], acc[j]); acc[j] = fmaf(v[3], w[3], acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < EB_ROWS / 8; ++j) {
        const int r = r0 + rg + 8 * j;
        if (okc && r < R) J.out[(size_t)r * J.co + c0 + cl] = acc[j] + (r < n_bias ? bias : 0.f);
      }
    }
  } else {
    // thread: 4 consecutive k (k4 = tid % K4 ... strided over K4) x 4 channels (cg = group of 4 of the 32)
    const int kt = tid & 31, cg = tid >> 5;          // kt walks k4 = kt, kt + 32, ...; K4 <= 128 -> at most 4 rounds
    float acc[4][4][4];                              // [round][channel][k]
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[a][b][c] = 0.f;
    float bsum = 0.f;                                // threads 0..31: bias gradient of channel c0 + tid
    for (int r0 = 0; r0 < R; r0 += EB_ROWS) {
      __syncthreads();
      for (int i = tid; i < EB_ROWS * K4; i += 256) {
        const int r = i / K4, k4 = i - r * K4;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r0 + r < R) v = *reinterpret_cast<const f32x4*>(semb + (size_t)(r0 + r) * K + 4 * k4);
        *reinterpret_cast<f32x4*>(sS + r * KP + 4 * k4) = v;
      }
      for (int i = tid; i < EB_ROWS * 32; i += 256) {
        const int r = i >> 5, c = i & 31;
        sW[r * 36 + c] = (r0 + r < R && c0 + c < J.co) ? J.dout[(size_t)(r0 + r) * J.co + c0 + c] : 0.f;
      }
      __syncthreads();
      const int rend = min(EB_ROWS, R - r0);
      for (int r = 0; r < rend; ++r) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(sW + r * 36 + 4 * cg);
#pragma unroll
        for (int a = 0; a < 4; ++a) {
          const int k4 = kt + 32 * a;
          if (k4 < K4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(sS + r * KP + 4 * k4);
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
              for (int c = 0; c < 4; ++c) acc[a][b][c] = fmaf(g[b], v[c], acc[a][b][c]);
          }
        }
      }
      if (tid < 32) {
        const int rb = min(rend, n_bias - r0);
        for (int r = 0; r < rb; ++r) bsum += sW[r * 36 + tid];
      }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int k4 = kt + 32 * a;
      if (k4 < K4) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int c = c0 + 4 * cg + b;
          if (c < J.co) *reinterpret_cast<f32x4*>(J.dW + (size_t)c * K + 4 * k4) = f32x4{acc[a][b][0], acc[a][b][1], acc[a][b][2], acc[a][b][3]};
        }
      }
    }
    if (tid < 32 && c0 + tid < J.co) {
      if (J.db) J.db[c0 + tid] = bsum;
      if (J.db2) J.db2[c0 + tid] = bsum;
    }
  }
}

// dsemb[r][k] = sum over jobs and their channels, in a fixed order.  Grid (row tiles of 8, k tiles of 32); thread (k, cs):
// channel slice cs of 8 takes the channels c = cs (mod 8) of every 64-channel chunk, the 8 slices meet through LDS in slice
// order.  (One thread per k walking all ~1400 channels alone was 125 us at 32 rows: a serial chain of dependent loads.)
__global__ void __launch_bounds__(256) k_emb_bank_dgrad(const msgm_emb_job_t* __restrict__ jobs, int n_jobs, float* __restrict__ dsemb,
                                                        int R, int K) {
  __shared__ float sG[8][68];
  __shared__ float red[8][8][33];
  const int tid = threadIdx.x, kl = tid & 31, cs = tid >> 5;
  const int k = blockIdx.y * 32 + kl, r0 = blockIdx.x * 8;
  const bool okk = k < K;
  float acc[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) acc[r] = 0.f;
  for (int j = 0; j < n_jobs; ++j) {
    const msgm_emb_job_t J = jobs[j];
    for (int cb = 0; cb < J.co; cb += 64) {
      __syncthreads();
      for (int i = tid; i < 8 * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        sG[r][c] = (r0 + r < R && cb + c < J.co) ? J.dout[(size_t)(r0 + r) * J.co + cb + c] : 0.f;
      }
      __syncthreads();
      float w[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {                      // this slice's 8 channels of the chunk: loads first, then the FMAs
        const int c = cb + cs + 8 * i;
        w[i] = (okk && c < J.co) ? J.W[(size_t)c * K + k] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = fmaf(sG[r][cs + 8 * i], w[i], acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 8; ++r) red[cs][r][kl] = acc[r];
  __syncthreads();
  {                                                      // thread (kl, r = cs): the 8 slices of row r in slice order
    const int r = cs;
    float t = red[0][r][kl];
#pragma unroll
    for (int sl = 1; sl < 8; ++sl) t += red[sl][r][kl];
    if (okk && r0 + r < R) dsemb[(size_t)(r0 + r) * K + k] = t;
  }
}

// ============================================================ C ABI
// the builds of a GroupNorm kernel, picked in ONE place: [0] scalar, [1] VEC (C % 4 == 0), [2] VEC + DROP (gn_set_dropout checks)
typedef void (*gn_kernel_t)(GnArgs);
static const gn_kernel_t GN_FWD_REDUCE[3] = {k_gn_fwd_reduce<false>, k_gn_fwd_reduce<true>, k_gn_fwd_reduce<true>};
static const gn_kernel_t GN_FWD_APPLY[3] = {k_gn_fwd_apply<false>, k_gn_fwd_apply<true>, k_gn_fwd_apply<true, true>};
static const gn_kernel_t GN_BWD_REDUCE[3] = {k_gn_bwd_reduce<false>, k_gn_bwd_reduce<true>, k_gn_bwd_reduce<true, true>};
static const gn_kernel_t GN_BWD_APPLY[3] = {k_gn_bwd_apply<false>, k_gn_bwd_apply<true>, k_gn_bwd_apply<true, true>};
static void gn_launch(const gn_kernel_t (&builds)[3], bool drop, bool vec, dim3 grid, msgm_stream_t stream, const GnArgs& A) {
  hipLaunchKernelGGL(builds[drop ? 2 : vec ? 1 : 0], grid, dim3(256), 0, S(stream), A);
}

extern "C" {

static int gn_chunks(int Bp, int P, int* chunk, int* sub) {
  // fp32 partial sums run over the SAME sub-chunks of a sample whatever the batch size (32 per sample, >= 64 pixels
  // each) and are combined in double: a row's statistics — bit for bit — do not depend on how many other rows share
  // the launch, so a row's result is the same in a 32-row shard and in the 256-row batch (tests/test_fullsize_gpu.py).
  // How many consecutive sub-chunks one workgroup takes is free (the test pairs of test_fullsize_gpu.py hold bit for bit;
  // across very different batch sizes the double-precision regrouping could move a float by an ulp).
  int c = (P + 31) / 32;
  if (c < 64) c = 64;
  if (c > P) c = P;
  *sub = c;
  const int nsub = (P + c - 1) / c;
  // ~512 workgroups in all: every workgroup ends with a fixed tail (LDS group sums of up to 5 moments + the parameter
  // partials), so fewer, fatter workgroups win — measured 1024 -> 512: B = 32 step 23.5 -> 23.1 ms, B = 256 129.7 -> 128.8 ms
  constexpr int target = 512;
  int want = (target + Bp - 1) / Bp;            // workgroups per sample
  if (want < 1) want = 1;
  int m = nsub / want;
  if (m < 1) m = 1;
  *chunk = m * c;
  return (P + m * c - 1) / (m * c);
}

// the elementwise passes have no summation order to protect: enough (sample, chunk) workgroups to fill 256 CUs a few
// times over, >= 64 pixels per chunk
static int gn_chunks_apply(int Bp, int P, int* chunk) {
  int n = (1024 + Bp - 1) / Bp;
  if (n < 1) n = 1;
  int c = (P + n - 1) / n;
  if (c < 64) c = 64;
  if (c > P) c = P;
  *chunk = c;
  return (P + c - 1) / c;
}

// workspace: acc[Bp][GN_SLOTS][G][8] doubles (per-chunk moment slots) | accf[Bp][G][8] doubles (backward moments summed)
// | [Bp][G][4] floats (finalised forward statistics) | [2][Bp*GN_SLOTS][max(C, 256)] floats (dgamma / dbeta slots; the
// kernels use pitch C inside it).  msgm_groupnorm_workspace is the C <= 256 value; every entry checks its own C's.
// Nothing in it has to be zero on entry: every slot that is read was written by the same call.
static inline size_t gn_acc_bytes(int32_t Bp, int32_t G) { return (size_t)Bp * GN_SLOTS * (size_t)G * 8 * sizeof(double); }
static inline size_t gn_accf_bytes(int32_t Bp, int32_t G) { return (size_t)Bp * (size_t)G * 8 * sizeof(double); }
static inline size_t gn_stats_bytes(int32_t Bp, int32_t G) { return (size_t)Bp * (size_t)G * 4 * sizeof(float); }
size_t msgm_groupnorm_workspace_c(int32_t Bp, int32_t G, int32_t C) {
  return gn_acc_bytes(Bp, G) + gn_accf_bytes(Bp, G) + gn_stats_bytes(Bp, G) +
         (size_t)2 * Bp * GN_SLOTS * (size_t)(C > 256 ? C : 256) * sizeof(float);
}
size_t msgm_groupnorm_workspace(int32_t Bp, int32_t G) { return msgm_groupnorm_workspace_c(Bp, G, 256); }

// dropout descriptor -> the DROP kernels' arguments (single-source input, C % 4 == 0: one Philox block per channel quad)
static int gn_set_dropout(GnArgs& A, const msgm_dropout_t* drop) {
  if (!drop->rng || drop->thr > (1u << 24) || !(drop->scale >= 1.0f)) return MSGM_E_BADARG;
  if (A.x1 || A.C % 4) return MSGM_E_UNSUPPORTED;
  A.drng = drop->rng; A.dstream = drop->stream; A.dthr = drop->thr; A.dscale = drop->scale;
  return MSGM_OK;
}

// forward and msgm_groupnorm_affine: checks of what the caller put into A, chunking, launch of the moment reduce (`vec` build)
static int gn_forward_reduce(GnArgs& A, size_t workspace_bytes, const msgm_dropout_t* drop, bool vec, msgm_stream_t stream) {
  const int C = A.C, C0 = A.C0, G = A.G;
  if (!A.x || !A.gamma || !A.beta || !A.acc || A.Bp <= 0 || A.P <= 0 || C <= 0 || G <= 0) return MSGM_E_BADARG;
  if (C % G || C > gn_max_c(C) || G > 64 || (A.x1 && (C0 % 4 || (C - C0) % 4 || C0 <= 0 || C0 >= C))) return MSGM_E_UNSUPPORTED;
  if (workspace_bytes < msgm_groupnorm_workspace_c(A.Bp, G, C)) return MSGM_E_WORKSPACE;
  if (drop) {
    const int rc = gn_set_dropout(A, drop);
    if (rc != MSGM_OK) return rc;
  }
  A.nch = gn_chunks(A.Bp, A.P, &A.chunk, &A.sub);
  if (A.nch > GN_SLOTS) return MSGM_E_UNSUPPORTED;
  gn_launch(GN_FWD_REDUCE, drop, vec, dim3(A.Bp, A.nch), stream, A);
  return MSGM_OK;
}

static int gn_forward_impl(const float* x, int32_t C0, const float* x1, int32_t C, const float* gamma, const float* beta, float* out,
                           float* stats, int32_t Bp, int32_t P, int32_t G, int32_t dual, int32_t silu, float eps, void* workspace,
                           size_t workspace_bytes, msgm_stream_t stream, const msgm_dropout_t* drop = nullptr) {
  if (!out) return MSGM_E_BADARG;
  GnArgs A{x, gamma, beta, out, reinterpret_cast<double*>(workspace), stats, P, C, G, Bp, dual, silu, 0, eps,
           nullptr, nullptr, nullptr, nullptr, x1, C0};
  // two launches: chunk moments -> slots, then the apply pass (every workgroup finalises its sample's statistics itself)
  const int rc = gn_forward_reduce(A, workspace_bytes, drop, C % 4 == 0, stream);
  if (rc != MSGM_OK) return rc;
  const int nap = gn_chunks_apply(Bp, P, &A.chunk);
  gn_launch(GN_FWD_APPLY, drop, C % 4 == 0, dim3(nap, Bp), stream, A);
  return msgm_check_launch();
}

int msgm_groupnorm_dual_forward(const float* x, const float* gamma, const float* beta, float* out, float* stats, int32_t Bp,
                                int32_t P, int32_t C, int32_t G, int32_t dual, int32_t silu, float eps, void* workspace,
                                size_t workspace_bytes, msgm_stream_t stream) {
  return gn_forward_impl(x, C, nullptr, C, gamma, beta, out, stats, Bp, P, G, dual, silu, eps, workspace, workspace_bytes, stream);
}

int msgm_groupnorm_dual_forward2(const float* x0, int32_t C0, const float* x1, int32_t C1, const float* gamma, const float* beta,
                                 float* out, float* stats, int32_t Bp, int32_t P, int32_t G, int32_t dual, int32_t silu, float eps,
                                 void* workspace, size_t workspace_bytes, msgm_stream_t stream) {
  if (!x1 || C1 <= 0) return MSGM_E_BADARG;
  return gn_forward_impl(x0, C0, x1, C0 + C1, gamma, beta, out, stats, Bp, P, G, dual, silu, eps, workspace, workspace_bytes, stream);
}

int msgm_groupnorm_dual_forward_dropout(const float* x, const float* gamma, const float* beta, float* out, float* stats, int32_t Bp,
                                        int32_t P, int32_t C, int32_t G, int32_t dual, int32_t silu, float eps, void* workspace,
                                        size_t workspace_bytes, const msgm_dropout_t* drop, msgm_stream_t stream) {
  if (!drop) return MSGM_E_BADARG;
  return gn_forward_impl(x, C, nullptr, C, gamma, beta, out, stats, Bp, P, G, dual, silu, eps, workspace, workspace_bytes, stream,
                         drop);
}

// the 0/1 keep mask of msgm_dropout_t, [Bp][P][C]: one thread per channel quad, the quads of the tensor in order
__global__ void __launch_bounds__(256) k_dropout_mask(const uint64_t* __restrict__ rng, uint32_t stream, uint32_t thr, int Bp, int P,
                                                      int C, float* __restrict__ keep) {
  const DropKey dk = drop_key(rng, stream, thr, 1.0f);
  const int CQ = C / 4;
  const size_t nq = (size_t)Bp * P * CQ;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (size_t)gridDim.x * 256) {
    const int cq = (int)(i % CQ);
    const size_t bp = i / CQ;
    const int p = (int)(bp % P), b = (int)(bp / P);
    *reinterpret_cast<f32x4*>(keep + 4 * i) = drop_mul4(dk, b, P, C, p, 4 * cq);
  }
}

int msgm_dropout_mask(const msgm_dropout_t* drop, int32_t Bp, int32_t P, int32_t C, float* keep_out, msgm_stream_t stream) {
  if (!drop || !drop->rng || !keep_out || Bp <= 0 || P <= 0 || C <= 0 || drop->thr > (1u << 24)) return MSGM_E_BADARG;
  if (C % 4) return MSGM_E_UNSUPPORTED;
  const int64_t nq = (int64_t)Bp * P * (C / 4);
  hipLaunchKernelGGL(k_dropout_mask, dim3(grid_for(nq, 256, 4096)), dim3(256), 0, S(stream), drop->rng, drop->stream, drop->thr,
                     (int)Bp, (int)P, (int)C, keep_out);
  return msgm_check_launch();
}

int msgm_groupnorm_affine(const float* x0, int32_t C0, const float* x1, int32_t C1, const float* gamma, const float* beta,
                          float* scale, float* shift, int32_t Bp, int32_t P, int32_t G, float eps, void* workspace,
                          size_t workspace_bytes, msgm_stream_t stream) {
  if (!scale || !shift || C0 <= 0 || (x1 && C1 <= 0)) return MSGM_E_BADARG;
  const int C = C0 + (x1 ? C1 : 0);
  GnArgs A{x0, gamma, beta, nullptr, reinterpret_cast<double*>(workspace), nullptr, P, C, G, Bp, 0, 0, 0, eps,
           nullptr, nullptr, nullptr, nullptr, x1, C0};
  const int rc = gn_forward_reduce(A, workspace_bytes, nullptr, C % 4 == 0 && C0 % 4 == 0, stream);
  if (rc != MSGM_OK) return rc;
  hipLaunchKernelGGL(k_gn_affine, dim3(Bp), dim3(256), 0, S(stream), A, scale, shift);
  return msgm_check_launch();
}

// The same affine map from the per-channel partial sums a producing convolution left behind (msgm_conv_fuse_t.chanstats:
// cs[n][slot][{sum, sum of squares}][Csrc], fp32 sums over one wave's 64..256 pixels): thread c adds the slots of its
// channel in slot order in double, the channels of a group are combined in double — no pass over the tensor itself.
// One block per sample; two sources = the decoder's cat([h, skip]) (each source has its own producer and slot count).
__global__ void __launch_bounds__(256) k_gn_affine_cs(const float* __restrict__ cs0, int S0, int C0, const float* __restrict__ cs1,
                                                      int S1, int C1, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, int P, int G, float eps,
                                                      float* __restrict__ scale, float* __restrict__ shift) {
  __shared__ double red[2][GN_MAX_C];
  const int b = blockIdx.x, C = C0 + C1, cpg = C / G;
  for (int c = threadIdx.x; c < C; c += 256) {
    const bool second = c >= C0;
    const int Cs = second ? C1 : C0, S = second ? S1 : S0, cc = second ? c - C0 : c;
    const float* p = (second ? cs1 : cs0) + (size_t)b * S * 2 * Cs + cc;
    double s = 0.0, ss = 0.0;
    for (int k = 0; k < S; ++k) { s += (double)p[(size_t)(2 * k) * Cs]; ss += (double)p[(size_t)(2 * k + 1) * Cs]; }
    red[0][c] = s; red[1][c] = ss;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    const int g0 = (c / cpg) * cpg;
    double a8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < cpg; ++k) { a8[0] += red[0][g0 + k]; a8[1] += red[1][g0 + k]; }
    float mu, inv, md, a;
    gn_stats(a8, (double)P * cpg, eps, 0.0, mu, inv, md, a);
    const float sc = inv * gamma[c];
    scale[(size_t)b * C + c] = sc;
    shift[(size_t)b * C + c] = beta[c] - mu * sc;
  }
}

int msgm_groupnorm_affine_chanstats(const float* cs0, int32_t S0, int32_t C0, const float* cs1, int32_t S1, int32_t C1,
                                    const float* gamma, const float* beta, float* scale, float* shift, int32_t Bp, int32_t P,
                                    int32_t G, float eps, msgm_stream_t stream) {
  if (!cs0 || !gamma || !beta || !scale || !shift || Bp <= 0 || P <= 0 || C0 <= 0 || S0 <= 0 || G <= 0) return MSGM_E_BADARG;
  if (cs1 ? (C1 <= 0 || S1 <= 0) : (C1 != 0)) return MSGM_E_BADARG;
  const int C = C0 + C1;
  if (C % G || C > gn_max_c(C) || G > 64) return MSGM_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_gn_affine_cs, dim3(Bp), dim3(256), 0, S(stream), cs0, S0, C0, cs1, S1, C1, gamma, beta, P, G, eps, scale,
                     shift);
  return msgm_check_launch();
}

// pslots_ext != nullptr: the per-(sample, chunk) dgamma | dbeta partials go to the CALLER's buffer and their slot-ordered
// sums are described in jobs_out[0..1] instead of being launched — a backward pass batches the parameter reductions of all
// its GroupNorms (and its convolutions' weight gradients) into ONE msgm_slot_reduce_batched launch.
static int gn_backward_impl(const float* x, int32_t C0, const float* x1, int32_t C, const float* gamma, const float* beta,
                            const float* stats, const float* gout, float* gx, float* gx1, float* dgamma, float* dbeta, int32_t Bp,
                            int32_t P, int32_t G, int32_t silu, float eps, const float* residual, void* workspace,
                            size_t workspace_bytes, msgm_stream_t stream, float* pslots_ext = nullptr, size_t pslots_bytes = 0,
                            msgm_reduce_job_t* jobs_out = nullptr, int32_t* n_jobs_out = nullptr, const float* residual2 = nullptr,
                            const msgm_dropout_t* drop = nullptr) {
  if (!x || !gamma || !beta || !stats || !gout || !gx || !dgamma || !dbeta || !workspace || Bp <= 0 || P <= 0 || C <= 0 || G <= 0)
    return MSGM_E_BADARG;
  if (C % G || C > gn_max_c(C) || G > 64) return MSGM_E_UNSUPPORTED;
  if (x1 && (!gx1 || residual || residual2 || C0 % 4 || (C - C0) % 4 || C0 <= 0 || C0 >= C)) return MSGM_E_UNSUPPORTED;
  if (workspace_bytes < msgm_groupnorm_workspace_c(Bp, G, C)) return MSGM_E_WORKSPACE;
  GnArgs A{x, gamma, beta, nullptr, reinterpret_cast<double*>(workspace), const_cast<float*>(stats), P, C, G, Bp, 1, silu, 0,
           eps, gout, gx, dgamma, dbeta, x1, C0, gx1};
  if (drop) {
    const int rc = gn_set_dropout(A, drop);
    if (rc != MSGM_OK) return rc;
  }
  const int nch = gn_chunks(Bp, P, &A.chunk, &A.sub);
  if (nch > GN_SLOTS) return MSGM_E_UNSUPPORTED;
  A.nch = nch;
  char* wsb = reinterpret_cast<char*>(workspace);
  A.accf = nullptr;
  A.pslots = reinterpret_cast<float*>(wsb + gn_acc_bytes(Bp, G) + gn_accf_bytes(Bp, G) + gn_stats_bytes(Bp, G));
  const size_t nslots = (size_t)Bp * nch;
  if (pslots_ext) {
    if (!jobs_out || !n_jobs_out || pslots_bytes < 2 * nslots * C * sizeof(float)) return MSGM_E_WORKSPACE;
    A.pslots = pslots_ext;
  }
  A.resid = residual;
  A.resid2 = residual2;
  gn_launch(GN_BWD_REDUCE, drop, C % 4 == 0, dim3(Bp, nch), stream, A);
  if (pslots_ext) {
    for (int w = 0; w < 2; ++w)
      jobs_out[w] = msgm_reduce_job_t{A.pslots + (size_t)w * nslots * C, w == 0 ? dgamma : dbeta, nullptr, (int64_t)C, (int64_t)C, 0, 0,
                                      (int32_t)nslots, 1, 0, 0, 0, 0, 1, 0};
    *n_jobs_out = 2;
  } else {
    const int nbc = (C + 31) / 32;
    hipLaunchKernelGGL(k_gn_param_reduce, dim3(2 * nbc), dim3(1024), 0, S(stream), (const float*)A.pslots, nslots, C, dgamma, dbeta,
                       nbc);
  }
  const int nap = gn_chunks_apply(Bp, P, &A.chunk);
  gn_launch(GN_BWD_APPLY, drop, C % 4 == 0, dim3(nap, Bp), stream, A);
  return msgm_check_launch();
}

size_t msgm_groupnorm_param_slots_bytes(int32_t Bp, int32_t P, int32_t C) {
  if (Bp <= 0 || P <= 0 || C <= 0) return 0;
  int chunk, sub;
  const int nch = gn_chunks(Bp, P, &chunk, &sub);
  return (size_t)2 * Bp * nch * C * sizeof(float);
}

int msgm_groupnorm_dual_backward_slots(const float* x0, int32_t C0, const float* x1, int32_t C1, const float* gamma,
                                       const float* beta, const float* stats, const float* gout, float* gx0, float* gx1,
                                       float* dgamma, float* dbeta, int32_t Bp, int32_t P, int32_t G, int32_t silu, float eps,
                                       const float* residual, const float* residual2, void* workspace, size_t workspace_bytes,
                                       float* pslots, size_t pslots_bytes, msgm_reduce_job_t* jobs_out, int32_t* n_jobs_out,
                                       msgm_stream_t stream) {
  if (!pslots || !jobs_out || !n_jobs_out || (x1 ? C1 <= 0 : C1 != 0)) return MSGM_E_BADARG;
  *n_jobs_out = 0;
  return gn_backward_impl(x0, C0, x1, C0 + C1, gamma, beta, stats, gout, gx0, gx1, dgamma, dbeta, Bp, P, G, silu, eps, residual,
                          workspace, workspace_bytes, stream, pslots, pslots_bytes, jobs_out, n_jobs_out, residual2);
}

int msgm_groupnorm_dual_backward_slots_dropout(const float* x, const float* gamma, const float* beta, const float* stats,
                                               const float* gout, float* gx, float* dgamma, float* dbeta, int32_t Bp, int32_t P,
                                               int32_t C, int32_t G, int32_t silu, float eps, const float* residual,
                                               const float* residual2, void* workspace, size_t workspace_bytes, float* pslots,
                                               size_t pslots_bytes, msgm_reduce_job_t* jobs_out, int32_t* n_jobs_out,
                                               const msgm_dropout_t* drop, msgm_stream_t stream) {
  if (!pslots || !jobs_out || !n_jobs_out || !drop) return MSGM_E_BADARG;
  *n_jobs_out = 0;
  return gn_backward_impl(x, C, nullptr, C, gamma, beta, stats, gout, gx, nullptr, dgamma, dbeta, Bp, P, G, silu, eps, residual,
                          workspace, workspace_bytes, stream, pslots, pslots_bytes, jobs_out, n_jobs_out, residual2, drop);
}

int msgm_groupnorm_dual_backward(const float* x, const float* gamma, const float* beta, const float* stats, const float* gout,
                                 float* gx, float* dgamma, float* dbeta, int32_t Bp, int32_t P, int32_t C, int32_t G,
                                 int32_t silu, float eps, const float* residual, void* workspace, size_t workspace_bytes,
                                 msgm_stream_t stream) {
  return gn_backward_impl(x, C, nullptr, C, gamma, beta, stats, gout, gx, nullptr, dgamma, dbeta, Bp, P, G, silu, eps, residual,
                          workspace, workspace_bytes, stream);
}

int msgm_groupnorm_dual_backward2(const float* x0, int32_t C0, const float* x1, int32_t C1, const float* gamma, const float* beta,
                                  const float* stats, const float* gout, float* gx0, float* gx1, float* dgamma, float* dbeta,
                                  int32_t Bp, int32_t P, int32_t G, int32_t silu, float eps, void* workspace,
                                  size_t workspace_bytes, msgm_stream_t stream) {
  if (!x1 || C1 <= 0) return MSGM_E_BADARG;
  return gn_backward_impl(x0, C0, x1, C0 + C1, gamma, beta, stats, gout, gx0, gx1, dgamma, dbeta, Bp, P, G, silu, eps, nullptr,
                          workspace, workspace_bytes, stream);
}

int msgm_bmm(const float* A, const float* B, const float* A2, const float* B2, float* C, int32_t M, int32_t N, int32_t K,
             int32_t batch, int64_t sAb, int64_t sAi, int64_t sAk, int64_t sBb, int64_t sBk, int64_t sBj, int64_t sCb,
             int64_t sCi, int64_t sCj, float alpha, int32_t accumulate, msgm_stream_t stream) {
  return msgm_bmm_dual(A, B, A2, B2, nullptr, C, nullptr, M, N, K, batch, sAb, sAi, sAk, sBb, sBk, sBj, sCb, sCi, sCj, alpha,
                       accumulate, stream);
}

int msgm_bmm_dual(const float* A, const float* B, const float* A2, const float* B2, const float* B3, float* C, float* C3,
                  int32_t M, int32_t N, int32_t K, int32_t batch, int64_t sAb, int64_t sAi, int64_t sAk, int64_t sBb,
                  int64_t sBk, int64_t sBj, int64_t sCb, int64_t sCi, int64_t sCj, float alpha, int32_t accumulate,
                  msgm_stream_t stream) {
  if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || batch <= 0 || ((A2 == nullptr) != (B2 == nullptr))) return MSGM_E_BADARG;
  if ((B3 == nullptr) != (C3 == nullptr)) return MSGM_E_BADARG;
  // the second output shares the A operand: C3 = alpha A.B3 — built for the case where the host swap below turns A
  // into the kernel's B role (outputs contiguous along j, as every attention product here); any K
  if (B3 && !(sCj == 1 && sCi != 1)) return MSGM_E_UNSUPPORTED;
  BmmArgs P{A, B, A2, B2, C, M, N, K, batch, sAb, sAi, sAk, sBb, sBk, sBj, sCb, sCi, sCj, alpha, accumulate, B3, C3};
  if (sCj == 1 && sCi != 1) {
    // C^T = B^T A^T: make the output's contiguous dimension the MFMA row index (16-B stores)
    P.A = B; P.B = A; P.A2 = B2; P.B2 = A2;
    P.M = N; P.N = M;
    P.sAb = sBb; P.sAi = sBj; P.sAk = sBk;
    P.sBb = sAb; P.sBk = sAk; P.sBj = sAi;
    P.sCi = sCj; P.sCj = sCi;
  }
  if (K % 16) {
    dim3 grid((unsigned)(((P.M + 31) / 32) * ((P.N + 31) / 32)), (unsigned)batch);
    if (P.A3) hipLaunchKernelGGL(k_bmm_slow<true>, grid, dim3(256), 0, S(stream), P);
    else hipLaunchKernelGGL(k_bmm_slow<false>, grid, dim3(256), 0, S(stream), P);
    return msgm_check_launch();
  }
  auto al16 = [](const float* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  // LDS-staged kernel: every operand has a unit stride (along k or along its row index), 16-byte aligned bases and
  // strides, K a multiple of 32, M and N multiples of 4
  {
    auto mode = [&](long sRow, long sK, long sB) { return (sK == 1 && sRow % 4 == 0 && sB % 4 == 0) ? (int)BL_KV
                                                        : (sRow == 1 && sK % 4 == 0 && sB % 4 == 0) ? (int)BL_RV : -1; };
    const int am = mode(P.sAi, P.sAk, P.sAb), bm = mode(P.sBj, P.sBk, P.sBb);
    if (am >= 0 && bm >= 0 && P.K % 32 == 0 && P.M % 4 == 0 && P.N % 4 == 0 && al16(P.A) && al16(P.A2) && al16(P.B) &&
        al16(P.B2) && al16(P.A3)) {
      dim3 grid((unsigned)(((P.M + 63) / 64) * ((P.N + 63) / 64)), (unsigned)batch);
#define BL_GO(AM, BM)                                                                                              \
  do {                                                                                                             \
    if (P.A3) hipLaunchKernelGGL((k_bmm_lds<AM, BM, true>), grid, dim3(256), 0, S(stream), P);                      \
    else hipLaunchKernelGGL((k_bmm_lds<AM, BM, false>), grid, dim3(256), 0, S(stream), P);                          \
  } while (0)
      if (am == BL_KV && bm == BL_KV) BL_GO(BL_KV, BL_KV);
      else if (am == BL_KV) BL_GO(BL_KV, BL_RV);
      else if (bm == BL_KV) BL_GO(BL_RV, BL_KV);
      else BL_GO(BL_RV, BL_RV);
#undef BL_GO
      return msgm_check_launch();
    }
  }
  const bool avec = P.sAk == 1 && (P.sAi % 4 == 0) && (P.sAb % 4 == 0) && al16(P.A) && al16(P.A2);
  const bool bvec = P.sBk == 1 && (P.sBj % 4 == 0) && (P.sBb % 4 == 0) && al16(P.B) && al16(P.B2);
  const int tiles = ((P.M + 63) / 64) * ((P.N + 63) / 64);
  dim3 grid((unsigned)tiles, (unsigned)batch);
  if (P.A3) {
    const bool avec3 = avec && al16(P.A3);
    if (avec3 && bvec) hipLaunchKernelGGL((k_bmm<2, 2, true, true, true>), grid, dim3(256), 0, S(stream), P);
    else if (avec3) hipLaunchKernelGGL((k_bmm<2, 2, true, false, true>), grid, dim3(256), 0, S(stream), P);
    else if (bvec) hipLaunchKernelGGL((k_bmm<2, 2, false, true, true>), grid, dim3(256), 0, S(stream), P);
    else hipLaunchKernelGGL((k_bmm<2, 2, false, false, true>), grid, dim3(256), 0, S(stream), P);
    return msgm_check_launch();
  }
  if (avec && bvec) hipLaunchKernelGGL((k_bmm<2, 2, true, true>), grid, dim3(256), 0, S(stream), P);
  else if (avec) hipLaunchKernelGGL((k_bmm<2, 2, true, false>), grid, dim3(256), 0, S(stream), P);
  else if (bvec) hipLaunchKernelGGL((k_bmm<2, 2, false, true>), grid, dim3(256), 0, S(stream), P);
  else hipLaunchKernelGGL((k_bmm<2, 2, false, false>), grid, dim3(256), 0, S(stream), P);
  return msgm_check_launch();
}

int msgm_softmax_dual_forward(float* Sm, const float* Wd, float* Pd, int64_t rows, int32_t T, int32_t dual, msgm_stream_t stream) {
  if (!Sm || rows <= 0 || T <= 0 || (dual && (!Wd || !Pd))) return MSGM_E_BADARG;
  hipLaunchKernelGGL(k_softmax_dual_fwd, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, S(stream), Sm, Wd, Pd, (long)rows, T, dual);
  return msgm_check_launch();
}

int msgm_softmax_dual_backward(const float* Pm, const float* Wd, float* Pb, float* Pdb, int64_t rows, int32_t T,
                               msgm_stream_t stream) {
  if (!Pm || !Wd || !Pb || !Pdb || rows <= 0 || T <= 0) return MSGM_E_BADARG;
  hipLaunchKernelGGL(k_softmax_dual_bwd, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, S(stream), Pm, Wd, Pb, Pdb, (long)rows, T);
  return msgm_check_launch();
}

int msgm_timestep_embedding(const float* t, float* emb, int32_t B, int32_t dim, float max_period, msgm_stream_t stream) {
  if (!t || !emb || B <= 0 || dim <= 0) return MSGM_E_BADARG;
  hipLaunchKernelGGL(k_timestep_embedding, dim3(grid_for((int64_t)B * dim, 256)), dim3(256), 0, S(stream), t, emb, B, dim, max_period);
  return msgm_check_launch();
}

int msgm_timestep_embedding_dual(const float* t, float* emb, int32_t Bp, int32_t dim, float max_period, msgm_stream_t stream) {
  if (!t || !emb || Bp <= 0 || dim <= 0) return MSGM_E_BADARG;
  hipLaunchKernelGGL(k_timestep_embedding_dual, dim3(grid_for((int64_t)Bp * dim, 256)), dim3(256), 0, S(stream), t, emb, Bp, dim, max_period);
  return msgm_check_launch();
}

int msgm_normalize_dual(const float* x, float* out, float* logr, int32_t Bp, int32_t n, int32_t dual, float scale, float eps,
                        msgm_stream_t stream) {
  if (!x || !out || !logr || Bp <= 0 || n <= 0) return MSGM_E_BADARG;
  hipLaunchKernelGGL(k_normalize_dual, dim3((Bp + 3) / 4), dim3(256), 0, S(stream), x, out, logr, Bp, n, dual, scale, eps);
  return msgm_check_launch();
}

int msgm_flat_to_image(const float* flat, float* img, int32_t B, int32_t C, int32_t H, int32_t W, int32_t forder, float scale,
                       msgm_stream_t stream) {
  if (!flat || !img || B <= 0 || C <= 0 || H <= 0 || W <= 0) return MSGM_E_BADARG;
  hipLaunchKernelGGL(k_flat_to_cl, dim3(grid_for((int64_t)B * C * H * W, 256)), dim3(256), 0, S(stream), flat, img, B, C, H, W, forder, scale);
  return msgm_check_launch();
}

int msgm_image_to_flat(const float* img, float* flat, int32_t B, int32_t C, int32_t H, int32_t W, int32_t forder, float scale,
                       msgm_stream_t stream) {
  if (!flat || !img || B <= 0 || C <= 0 || H <= 0 || W <= 0) return MSGM_E_BADARG;
  hipLaunchKernelGGL(k_cl_to_flat, dim3(grid_for((int64_t)B * C * H * W, 256)), dim3(256), 0, S(stream), img, flat, B, C, H, W, forder, scale);
  return msgm_check_launch();
}

int msgm_sum2x2(const float* in, float* out, int32_t N, int32_t H, int32_t W, int32_t C, msgm_stream_t stream) {
  if (!in || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0) return MSGM_E_BADARG;
  hipLaunchKernelGGL(k_sum2x2, dim3(grid_for((int64_t)N * H * W * C, 256)), dim3(256), 0, S(stream), in, out, N, H, W, C);
  return msgm_check_launch();
}

int msgm_emb_bank_forward(const msgm_emb_job_t* jobs_dev, int32_t n_jobs, int32_t total_blocks, const float* semb, int32_t R,
                          int32_t K, int32_t n_bias, msgm_stream_t stream) {
  if (!jobs_dev || !semb || n_jobs <= 0 || total_blocks <= 0 || R <= 0 || K <= 0 || n_bias < 0) return MSGM_E_BADARG;
  if (K % 4 || K > 512) return MSGM_E_UNSUPPORTED;
  const size_t lds = (size_t)(EB_ROWS + 32) * (K + 4) * sizeof(float);
  static const int once = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_emb_bank<0>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_emb_bank<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return 0;
  }();
  (void)once;
  int ry = (R + EB_ROWS - 1) / EB_ROWS;
  if (ry > 8) ry = 8;
  hipLaunchKernelGGL(k_emb_bank<0>, dim3((unsigned)total_blocks, (unsigned)ry), dim3(256), lds, S(stream), jobs_dev, n_jobs, semb, R, K,
                     n_bias);
  return msgm_check_launch();
}

int msgm_emb_bank_backward(const msgm_emb_job_t* jobs_dev, int32_t n_jobs, int32_t total_blocks, const float* semb, float* dsemb,
                           int32_t R, int32_t K, int32_t n_bias, msgm_stream_t stream) {
  if (!jobs_dev || !semb || !dsemb || n_jobs <= 0 || total_blocks <= 0 || R <= 0 || K <= 0 || n_bias < 0) return MSGM_E_BADARG;
  if (K % 4 || K > 512) return MSGM_E_UNSUPPORTED;
  size_t lds = (size_t)EB_ROWS * (K + 4) * sizeof(float) + (size_t)EB_ROWS * 36 * sizeof(float);
  const size_t lds_f = (size_t)(EB_ROWS + 32) * (K + 4) * sizeof(float);
  if (lds < lds_f) lds = lds_f;                      // one carve formula for both modes (sW starts at EB_ROWS * KP)
  static const int once = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_emb_bank<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return 0;
  }();
  (void)once;
  hipLaunchKernelGGL(k_emb_bank<1>, dim3((unsigned)total_blocks), dim3(256), lds, S(stream), jobs_dev, n_jobs, semb, R, K, n_bias);
  hipLaunchKernelGGL(k_emb_bank_dgrad, dim3((unsigned)((R + 7) / 8), (unsigned)((K + 31) / 32)), dim3(256), 0, S(stream), jobs_dev,
                     n_jobs, dsemb, R, K);
  return msgm_check_launch();
}

}  // extern "C"
