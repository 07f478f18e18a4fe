// sde_dense_mm_kernels.hip — one integrator stage of the multiplicative SDE with a DENSE rotation tensor, the n^3
// contraction on the matrix cores (msgm_sde_stage_dense_mm).  gfx950 only.
//
// The stage is msgm_sde_stage's: out = base + c_out (mu delta + sig_scale gw) (sde_stage.h; SDEs.py:415,432,556-588;
// sde_scheme.py:36-40).  k_stage_rows' dense branch gives every output element to one lane that runs an n^2 scalar loop
// over its own G[i,:,:] slice; here a workgroup of 4 waves owns a tile of 32 rows and forms
//   T[r,(i,k)] = sum_j x_rj G[i,j,k]
// as a GEMM (DenseMM of mlp_kernels.hip, generalised from NP = 32 to NP = 16, 32, 48, 64):
//   M = the tile's 32 rows: two 16-row tiles, two independent accumulator chains that share every B fragment; the A operand
//       (x, j >= n masked to +0) lives in registers, KP/4 floats per row tile;
//   K = j padded to KP = NP = 16 ceil(n/16);
//   N-block = the 16 values of i of one i-block at a FIXED k: KP/4 v_mfma_f32_16x16x4_f32 per row tile.  D holds
//       T[row 4q + r][i = il] in register r, and the lane multiplies it by its rows' w_k and a_k (LDS broadcasts) and sums
//       with fmaf in registers: gw_ri = sum_k T w_rk, ga_ri = sum_k T a_rk.  Nothing crosses lanes inside the k loop.
// One more block with L_G in G's place gives L_G x.  The B fragments are b128 buffer loads from the packed image
// (ops.pack_dense_g_stage: include/msgm_hip.h) in L2, requested one block ahead.
// Wave split (NB = NP/16 i-blocks; a wave owns IBW of them and one of KSL k-slices, k = ks, ks + KSL, ..):
//   NB = 1: (1 i-block, 4 k-slices)   NB = 2: (i-half, k-half)   NB = 3: (all 3 i-blocks, 4 k-slices)   NB = 4: (1 i-block, all k)
// The partial sums of the k-slices land in one LDS image each and are added by the reader in the order ks = 0, 1, ..; the
// row sum of the norm correction is 8 partial sums a row (elements i = p, p + 8, ..), added in the order p = 0 .. 7.  No
// atomics: same inputs, same bits.  An fp32 MFMA is a j-ordered fma chain, so these are not k_stage_rows' bits: parity
// of this kernel is to float64 (tests/test_stage_dense_mm_gpu.py).
// Rows >= B of the last tile are neither loaded nor stored; no element of x, a, z, dW beyond B n is touched.
#include "common.h"
#include "sde_stage.h"

typedef __amdgpu_buffer_rsrc_t sdm_rsrc_t;

// LDS hand-off: LDS traffic completes in order, so lgkmcnt(0) + s_barrier is what a producer / consumer pair needs; the B
// fragments in flight stay in flight.
__device__ __forceinline__ void sdm_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <int NB_>
struct SdmCfg {
  static constexpr int NB = NB_;                        // i-blocks = 16-wide K groups
  static constexpr int NP = 16 * NB;                    // padded n
  static constexpr int KS = NP / 4;                     // MFMA steps of a block
  static constexpr int IBW = NB == 3 ? 3 : 1;           // i-blocks of a wave
  static constexpr int IBG = NB / IBW;                  // waves that share a k-slice
  static constexpr int KSL = 4 / IBG;                   // k-slices
  static constexpr int P = NP + 4;                      // row pitch of every image: q's four rows fall into different bank groups
  static constexpr int IMG = 32 * P;
  static constexpr int XS = 0, WS = IMG, AS = 2 * IMG;  // x | w | a rows of the tile
  static constexpr int FI = 3 * IMG;                    // L_G x, later the updated row under norm correction
  static constexpr int GWI = FI + IMG;                  // sum_k T w, one image per k-slice
  static constexpr int GAI = GWI + KSL * IMG;           // sum_k T a
  static constexpr int RED = GAI + KSL * IMG;           // [32][8] partial row sums
  static constexpr int FLOATS = RED + 32 * 8;
  static_assert(IBG * KSL == 4 && FLOATS * 4 <= 160 * 1024, "four waves; the carve must fit a CU");
};

__device__ __forceinline__ bool sdm_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The tile's x, w, a rows -> LDS, by quads of the flat element index (a tile starts at a multiple of 4 elements, so a quad
// is also a Philox block: one draw per quad, the numbers stage_noise gives element by element).  dW_out is stored here, from
// the value that goes to LDS.  Elements at or behind B n are +0 in LDS and touch no memory.
template <class C>
__device__ __forceinline__ void sdm_fill(const StageArgs& A, float* lds, int64_t row0, int n, int tid) {
  const int64_t tot = A.B * (int64_t)n, e0 = row0 * n;
  const int nquad = 8 * n;                                                      // 32 n / 4
  const bool vx = sdm_al16(A.x), va = sdm_al16(A.a), vz = sdm_al16(A.dW ? A.dW : A.z), vo = sdm_al16(A.dW_out);
  for (int qd = tid; qd < nquad; qd += 256) {
    const int64_t e = e0 + 4 * (int64_t)qd;
    if (e >= tot) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int idx = 4 * qd + k, c = idx / n, o = idx - c * n;
        lds[C::XS + c * C::P + o] = 0.f; lds[C::WS + c * C::P + o] = 0.f; lds[C::AS + c * C::P + o] = 0.f;
      }
      continue;
    }
    const bool full = e + 3 < tot;
    f32x4 xv = {0.f, 0.f, 0.f, 0.f}, av = {0.f, 0.f, 0.f, 0.f}, wv = {0.f, 0.f, 0.f, 0.f};
    if (full && vx) xv = *reinterpret_cast<const f32x4*>(A.x + e);
    else
      for (int k = 0; k < 4; ++k) if (e + k < tot) xv[k] = A.x[e + k];
    if (A.a) {
      if (full && va) av = *reinterpret_cast<const f32x4*>(A.a + e);
      else
        for (int k = 0; k < 4; ++k) if (e + k < tot) av[k] = A.a[e + k];
    }
    const float* wsrc = A.dW ? A.dW : A.z;
    if (wsrc) {
      if (full && vz) wv = *reinterpret_cast<const f32x4*>(wsrc + e);
      else
        for (int k = 0; k < 4; ++k) if (e + k < tot) wv[k] = wsrc[e + k];
    } else {
      wv = philox_normal4(A.rng, stage_step(A), RNG_STREAM_DW, (uint64_t)(e >> 2));
    }
    if (!A.dW) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int c = (4 * qd + k) / n;
        const float sqd = A.delta_rows ? ((row0 + c < A.B) ? sqrtf(A.delta_rows[row0 + c]) : 0.f) : A.sqrt_delta;
        wv[k] = sqd * wv[k];                                                    // delta**0.5 * randn   sde_scheme.py:84
      }
    }
    if (A.dW_out) {
      if (full && vo) *reinterpret_cast<f32x4*>(A.dW_out + e) = wv;
      else
        for (int k = 0; k < 4; ++k) if (e + k < tot) A.dW_out[e + k] = wv[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = 4 * qd + k, c = idx / n, o = idx - c * n;
      const bool ok = e + k < tot;
      lds[C::XS + c * C::P + o] = ok ? xv[k] : 0.f;
      lds[C::WS + c * C::P + o] = ok ? wv[k] : 0.f;
      lds[C::AS + c * C::P + o] = ok ? av[k] : 0.f;
    }
  }
}

template <int NB>
__global__ void __launch_bounds__(256) k_stage_dense_mm(StageArgs A, const float* __restrict__ Gp) {
  using C = SdmCfg<NB>;
  __shared__ __attribute__((aligned(16))) float lds[C::FLOATS];
  const int tid = threadIdx.x, n = (int)A.n;
  const int64_t row0 = (int64_t)blockIdx.x * 32;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lane = tid & 63, il = lane & 15, q = lane >> 4;
  const int ibg = w % C::IBG, ks = w / C::IBG, ib0 = ibg * C::IBW;

  // fragment sg of i-block ib of block kk (all three scalar: the fragment's place is the buffer load's scalar offset)
  const sdm_rsrc_t GR = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Gp), 0, (n + 1) * (NB * NB * 1024), 0x00020000);
  auto frag = [&](int kk, int ib, int sg) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(GR, lane * 16, ((kk * NB + ib) * NB + sg) * 1024, 0));
  };
  // the wave's first block (block n = L_G where its k-slice is empty) goes out ahead of the fill
  f32x4 g[C::IBW][NB];
  {
    const int k0 = ks < n ? ks : n;
#pragma unroll
    for (int bi = 0; bi < C::IBW; ++bi)
#pragma unroll
      for (int sg = 0; sg < NB; ++sg) g[bi][sg] = frag(k0, ib0 + bi, sg);
  }

  sdm_fill<C>(A, lds, row0, n, tid);
  sdm_lds_barrier();

  // A operand: x[row 16 mt + il][j = 4 s + q], j >= n masked to +0
  float xa[2][C::KS];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int s = 0; s < C::KS; ++s) {
      const int j = 4 * s + q;
      xa[mt][s] = j < n ? lds[C::XS + (16 * mt + il) * C::P + j] : 0.f;
    }
  // one block: acc[mt] = x (row tile mt) . the block whose fragments are c[0 .. NB)
  auto block = [&](const f32x4 (&c)[NB], f32x4 (&acc)[2]) {
    acc[0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < C::KS; ++s) {
      const float b = c[s >> 2][s & 3];
      acc[0] = mfma16(xa[0][s], b, acc[0]);
      acc[1] = mfma16(xa[1][s], b, acc[1]);
    }
  };

  f32x4 gw[C::IBW][2], ga[C::IBW][2];
#pragma unroll
  for (int bi = 0; bi < C::IBW; ++bi)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) { gw[bi][mt] = f32x4{0.f, 0.f, 0.f, 0.f}; ga[bi][mt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  for (int kk = ks; kk < n; kk += C::KSL) {
    const int nk = kk + C::KSL < n ? kk + C::KSL : n;   // behind the wave's last k: the L_G block (used by the waves of the last slice)
    f32x4 c[C::IBW][NB];
#pragma unroll
    for (int bi = 0; bi < C::IBW; ++bi)
#pragma unroll
      for (int sg = 0; sg < NB; ++sg) { c[bi][sg] = g[bi][sg]; g[bi][sg] = frag(nk, ib0 + bi, sg); }
    float wv[2][4], av[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * mt + 4 * q + r;
        wv[mt][r] = lds[C::WS + row * C::P + kk];
        av[mt][r] = lds[C::AS + row * C::P + kk];
      }
    __builtin_amdgcn_sched_barrier(0);                  // loads and LDS reads go out ahead of the MFMAs that hide them
#pragma unroll
    for (int bi = 0; bi < C::IBW; ++bi) {
      f32x4 acc[2];
      block(c[bi], acc);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gw[bi][mt][r] = __builtin_fmaf(acc[mt][r], wv[mt][r], gw[bi][mt][r]);
          ga[bi][mt][r] = __builtin_fmaf(acc[mt][r], av[mt][r], ga[bi][mt][r]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  if (ks == C::KSL - 1) {
#pragma unroll
    for (int bi = 0; bi < C::IBW; ++bi) {
      f32x4 acc[2];
      block(g[bi], acc);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[C::FI + (16 * mt + 4 * q + r) * C::P + 16 * (ib0 + bi) + il] = acc[mt][r];
    }
  }
#pragma unroll
  for (int bi = 0; bi < C::IBW; ++bi)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = ks * C::IMG + (16 * mt + 4 * q + r) * C::P + 16 * (ib0 + bi) + il;
        lds[C::GWI + at] = gw[bi][mt][r];
        lds[C::GAI + at] = ga[bi][mt][r];
      }
  sdm_lds_barrier();

  // the stage update: thread t owns the elements idx = t, t + 256, .. of the tile (row c = idx / n, output o)
  const float sig_scale = stage_sig_scale(A);
  const float tnow = stage_time(A);
  const int nel = 32 * n;
  for (int idx = tid; idx < nel; idx += 256) {
    const int c = idx / n, o = idx - c * n;
    const int64_t b = row0 + c;
    if (b >= A.B) continue;
    const int64_t e = b * n + o;
    const StageCoef sc = stage_coef(A, tnow, b);
    const int at = c * C::P + o;
    float tw = lds[C::GWI + at], ta = lds[C::GAI + at];
#pragma unroll
    for (int s = 1; s < C::KSL; ++s) { tw += lds[C::GWI + s * C::IMG + at]; ta += lds[C::GAI + s * C::IMG + at]; }
    const float f = sc.beta * lds[C::FI + at];                                  // SDEs.py:415
    const float gwv = sc.sb * tw, gav = sc.sb * ta;                             // SDEs.py:432; sde_scheme.py:36
    const float inc = stage_mu(A, gav, f, 0.f, 2.0f * f) * sc.delta + sig_scale * gwv;   // sde_scheme.py:40
    const float bv = A.base ? (A.base == A.x ? lds[C::XS + at] : A.base[e]) : 0.f;
    const float ov = bv + A.c_out * inc;
    if (A.inc_out) A.inc_out[e] = inc;
    if (A.norm0) lds[C::FI + at] = ov;                                          // the same thread read this place
    else A.out[e] = ov;
  }
  if (A.norm0) {                                                                // kernel-uniform
    // norm correction x <- x norm0 / ||x|| (sde_scheme.py:85-86): thread (row c = t / 8, part p = t % 8) sums the squares of
    // the row's elements p, p + 8, ..; the 8 parts are added in the order 0 .. 7 by every reader
    sdm_lds_barrier();
    {
      const int c = tid >> 3, p = tid & 7;
      float ss = 0.f;
      for (int o = p; o < n; o += 8) { const float v = lds[C::FI + c * C::P + o]; ss += v * v; }
      lds[C::RED + tid] = ss;
    }
    sdm_lds_barrier();
    for (int idx = tid; idx < nel; idx += 256) {
      const int c = idx / n, o = idx - c * n;
      const int64_t b = row0 + c;
      if (b >= A.B) continue;
      float ss = lds[C::RED + 8 * c];
#pragma unroll
      for (int p = 1; p < 8; ++p) ss += lds[C::RED + 8 * c + p];
      const float scale = A.norm0[b] / sqrtf(ss);
      A.out[b * n + o] = lds[C::FI + c * C::P + o] * scale;
    }
  }
}

extern "C" {

size_t msgm_dense_g_stage_floats(int64_t n) {
  if (n < 1 || n > 64) return 0;
  const size_t nb = (size_t)((n + 15) / 16);
  return (size_t)(n + 1) * nb * nb * 256;
}

int msgm_sde_stage_dense_mm(float* out, const float* base, float c_out, const float* x, const float* a, const float* dW,
                            const float* z, float sqrt_delta, const uint64_t* rng, uint64_t rng_step, float* dW_out,
                            float* inc_out, int64_t B, int64_t n, const msgm_sde_t* sde, int32_t proc, int32_t strato, float t,
                            float delta, float lmbd, const float* norm0, const float* delta_rows, float t_frac,
                            const float* t_dev, const int64_t* step_dev, const float* packed, msgm_stream_t stream) {
  if (!out || !x || !sde || B <= 0 || n <= 0) return MSGM_E_BADARG;
  if (sde->kind != MSGM_SDE_MSGM_DENSE || n > 64) return MSGM_E_UNSUPPORTED;
  if (!dW && !z && !rng) return MSGM_E_BADARG;
  if (proc == MSGM_PROC_REVERSE && !a) return MSGM_E_BADARG;
  if (proc != MSGM_PROC_REVERSE && proc != MSGM_PROC_FORWARD) return MSGM_E_BADARG;
  if (out == x || !packed) return MSGM_E_BADARG;                            // the contraction reads the whole row
  // the forward process has no score: `a` is not read (k_stage_rows reads it whenever it is given; its ga is unused there)
  StageArgs A{out, base, c_out, x, proc == MSGM_PROC_REVERSE ? a : nullptr, dW, z, sqrt_delta, rng, rng_step, dW_out, B, n,
              sde->kind, proc, strato, sde->beta_min, sde->beta_max, sde->T, t, delta, lmbd, sde->G, sde->L_G, norm0, inc_out,
              delta_rows, t_frac, t_dev, step_dev};
  const dim3 grid((unsigned)((B + 31) / 32)), block(256);
  switch ((n + 15) / 16) {
    case 1: hipLaunchKernelGGL(k_stage_dense_mm<1>, grid, block, 0, S(stream), A, packed); break;
    case 2: hipLaunchKernelGGL(k_stage_dense_mm<2>, grid, block, 0, S(stream), A, packed); break;
    case 3: hipLaunchKernelGGL(k_stage_dense_mm<3>, grid, block, 0, S(stream), A, packed); break;
    default: hipLaunchKernelGGL(k_stage_dense_mm<4>, grid, block, 0, S(stream), A, packed); break;
  }
  return msgm_check_launch();
}

}  // extern "C"
