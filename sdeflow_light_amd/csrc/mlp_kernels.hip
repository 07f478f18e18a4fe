// mlp_kernels.hip — K5: the MLP score network (NN.py:73-120) as ONE fused
// kernel per use: forward (sampling), forward + Euler–Maruyama update, and the
// whole sliced-score-matching training pass (forward + forward-mode tangent +
// loss + backward), on fp32 MFMA (v_mfma_f32_16x16x4_f32, exact fp32).
//
// Design (gfx950, 4 waves / workgroup, 1 workgroup / CU, persistent grid):
//   * orientation Z[feature][sample] = W[feature][k] . H[k][sample]: the weight
//     is the MFMA A operand, activations the B operand.  The C/D layout then has
//     the sample on lane&15 and 4 consecutive features in the 4 accumulator
//     registers, which is exactly the B-operand layout of the next layer — the
//     only thing that crosses waves is the activation tile, exchanged through LDS
//     in [sample][feature] order with b128 reads/writes.
//   * wave w owns output features [32w, 32w+32) of every layer (2 row tiles).
//     Its weight fragments are streamed from L2 straight into registers one phase
//     ahead (the 128x128 weights never sit in LDS); its slice of dW2/dW3 lives in
//     accumulator registers for the whole kernel.
//   * a tile is 16 samples = 16 primal + 16 tangent columns (forward-mode dual
//     numbers: tangent = J.v), so primal and tangent of one sample share a lane
//     and the Swish first/second derivatives are applied in registers.
//   * per-workgroup gradient slabs are written once at the end and reduced by a
//     second (deterministic) kernel — no float atomics.
#include "common.h"
#include "sde_stage.h"

#define HID 128

// Diagnostic build only (-DMLP_STAMPS): per-phase s_memtime sums of workgroup 0 /
// wave 0, read back with msgm_debug_stamps().  No stamp executes in the shipped .so.
#ifdef MLP_STAMPS
__device__ unsigned long long g_stamps[16];
#define STAMP_DECL unsigned long long st_acc[12] = {0,0,0,0,0,0,0,0,0,0,0,0}; unsigned long long st_prev = __builtin_amdgcn_s_memtime();
#define STAMP(i) do { unsigned long long _t = __builtin_amdgcn_s_memtime(); st_acc[i] += _t - st_prev; st_prev = _t; } while (0)
#define STAMP_FLUSH do { if (blockIdx.x == 0 && threadIdx.x == 0) { for (int _i = 0; _i < 12; ++_i) g_stamps[_i] = st_acc[_i]; } } while (0)
#else
#define STAMP_DECL
#define STAMP(i)
#define STAMP_FLUSH
#endif
#define ACT_P 132   // LDS pitch of an activation row ([sample][feature])

// Workgroup barrier for LDS hand-offs inside the tile loop.  __syncthreads() also drains vmcnt, i.e. it would wait for
// the weight fragments and the next tile's inputs that are deliberately left in flight across phase boundaries;
// LDS traffic completes in order, so lgkmcnt(0) + s_barrier is all an LDS producer/consumer pair needs.  hipcc's
// own waitcnt insertion still guards the first use of every in-flight load.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// row pitch of a gradient slab: n_params + 1 (loss) rounded up to 4 floats, so the reduction reads 16-B vectors
__host__ __device__ static inline int64_t slab_stride(int64_t n_params) { return (n_params + 1 + 3) & ~(int64_t)3; }

// ---- LDS carve (floats), per (mode, width) ------------------------------------
// NARROW nets (in_dim <= 16 and d <= 16) use 20-float small rows and 16 padded outputs; the forward / sampler
// modes drop the backward-only buffers — 67 KB instead of 134 KB, so TWO workgroups share a CU there and each
// one's barrier bubbles are filled by the other's MFMAs.
// TINY (inference modes, in_dim <= 4 and d <= 4 — the C1/C2 nets): the small rows shrink to 8 floats, only 4 rows of
// W4 are kept (the MFMA's other 12 output rows are zeros and are fed from registers), so the carve drops from 74 KB
// to 52 KB and THREE workgroups share a CU.
template <int MODE, bool WIDE, int NW, bool TINY = false>
struct MlpLds {
  static_assert(!TINY || (MODE != 2 && !WIDE), "the tiny carve is for the narrow inference modes");
  static constexpr int SMP = WIDE ? 36 : (TINY ? 8 : 20);   // pitch of h0 / abar / W1 rows
  static constexpr int PP = TINY ? 8 : SMP;        // pitch of a layer-4 partial row
  static constexpr int DP = WIDE ? 32 : 16;        // padded output width
  static constexpr int DROWS = TINY ? 4 : DP;      // rows of W4 held in LDS
  static constexpr bool TRAIN = MODE == 2;
  static constexpr bool SDE = MODE == 3;
  static constexpr int SPT = TRAIN ? 16 : 32;      // samples per tile
  static constexpr int DMAX = WIDE ? 32 : (TINY ? 4 : 16);   // raw rows are packed (pitch d), sized for d <= DMAX
  // one raw input buffer: the tile's y | v | u chunks (sampler loop: y | dW), t and cst, copied verbatim from global one
  // tile ahead
  static constexpr int RY = 0;
  static constexpr int RV = RY + SPT * DMAX;
  static constexpr int RU = RV + (TRAIN ? SPT * DMAX : 0);
  static constexpr int RW = RU + (TRAIN ? SPT * DMAX : 0);
  static constexpr int RT = RW + (SDE ? SPT * DMAX : 0);
  static constexpr int RWT = RT + 16;              // train (16 rows a tile): the optional row weights, in RT's upper half
  static constexpr int RC = RT + 32;
  static constexpr int RAWN = RC + 16;
  static constexpr int X = 0;
  static constexpr int Y = X + 32 * ACT_P;
  static constexpr int Z = Y + 32 * ACT_P;
  static constexpr int U = Z + (TRAIN ? 32 * ACT_P : 0);
  static constexpr int H0 = U + (TRAIN ? 32 * ACT_P : 0);
  static constexpr int ABAR = H0 + 2 * 32 * SMP;   // h0 is double-buffered (built one tile ahead)
  static constexpr int PART = ABAR + (TRAIN ? 32 * SMP : 0);
  static constexpr int W1 = PART + NW * 32 * PP;    // one layer-4 K-slice per wave
  static constexpr int W4 = W1 + HID * SMP;
  static constexpr int B1 = W4 + DROWS * ACT_P;
  static constexpr int B2 = B1 + HID;
  static constexpr int B3 = B2 + HID;
  static constexpr int B4 = B3 + HID;
  static constexpr int DB4 = B4 + 32;
  static constexpr int RED = DB4 + (TRAIN ? 16 * DP : 0);
  static constexpr int RAW = RED + 64;
  static constexpr int FLOATS = RAW + 2 * RAWN;
  static constexpr int BYTES = FLOATS * 4;
};

struct MlpArgs {
  msgm_mlp_params_t P;
  const float* y;        // (B,d) inputs (x_t for the sampler)
  const float* t;        // (B) per-sample time, or null => t_scalar
  const float* v;        // (B,d) probe (train)
  const float* u;        // (B,d) optional: cotangent direction of adot, loss_b = adot.u + cst + |a|^2/2 (MSGM); null => SGM closed form
  const float* cst;      // (B) optional per-sample constant of the loss
  float* out;            // forward: a (B,d); EM: x updated in place (== y)
  int64_t B;
  int in_dim, in4, d4;   // in_dim = d + 1 (+1 with premodule); in4 = ceil(in/4); d4 = ceil(d/4)
  float t_scalar;
  // SDE (SGM)
  float b0, b1, T;
  // EM step
  float delta, sqrt_delta, lmbd;
  const float* z; const uint64_t* rng; uint64_t rng_step;
  int n_steps; const float* ts;   // EM loop: n_steps > 1 steps in ONE launch, time of step i = ts[i] (device array)
  // train
  float inv_batch;
  const float* row_w;    // (B) optional per-row weights of the loss: the row's seed is inv_batch * row_w[b]; null => inv_batch
  float* loss_per; float* slabs;   // slabs: [gridDim.x][slab_stride], element n_params = loss sum; stride = 4-aligned
  int64_t n_params;
  // sampler loop (MODE_SDE): n_stages = 1 (EM), 2 (Heun) or 4 (RK4-Stratonovich) stages per step, SDE family `kind`
  int n_stages, kind;
  float t_half, t_full;            // fp32 delta/2 and delta: what the later stages add to ts[i]
  const float* G; const float* L_G;   // dense tensor (n <= 16), read through L2 by every row
  const float* norm0;              // (B) optional: rows are rescaled to this norm at the end of a step
  float* ws;                       // (3, B, d) stage state: evaluation point | Wiener increment | running sum of increments
  float* traj; int include_t0;     // optional (N[+1], B, d): row i + include_t0 receives the state after step i
  const int32_t* keep_stop; float* kept;   // optional: row b of kept receives the state after step keep_stop[b] - include_t0
  const float* Gp;                 // dense tensor, 17 <= n <= 30 (k_mlp<MODE_SDE, wide, DENSE_MM>): G and L_G in fragment order
};

enum { MODE_FWD = 0, MODE_EM = 1, MODE_TRAIN = 2, MODE_SDE = 3 };
// the modes whose net is the score of a reverse process: its time argument is T - t
constexpr bool mode_reverse(int mode) { return mode == MODE_EM || mode == MODE_SDE; }

// Item `item` of the sampler loop = (step i, stage): the stage index runs fastest.
struct SdeItem { int i, stage; };
__device__ __forceinline__ SdeItem sde_item(const MlpArgs& A, int item) {
  const int i = item / A.n_stages;
  return {i, item - i * A.n_stages};
}
// Stage times ts[i], ts[i] + fp32(delta/2) (RK4's two middle stages), ts[i] + fp32(delta): fp32 adds, as k_time_tick.
__device__ __forceinline__ float sde_item_time(const MlpArgs& A, SdeItem it) {
  const float add = it.stage == 0 ? 0.f : ((A.n_stages == 4 && it.stage < 3) ? A.t_half : A.t_full);
  return add != 0.f ? __fadd_rn(A.ts[it.i], add) : A.ts[it.i];
}
// A word that this workgroup wrote an item ago: device-scope load, so no stale L1 line is served.
__device__ __forceinline__ float load_agent(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Swish and its first two derivatives from z.
__device__ __forceinline__ void swish012(float z, float& s0, float& s1, float& s2) {
  float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-z));
  float om = 1.0f - sg;
  s0 = z * sg;
  s1 = sg * (1.0f + z * om);
  s2 = sg * om * (2.0f + z * (1.0f - 2.0f * sg));
}
__device__ __forceinline__ float swish0(float z) { return z * __builtin_amdgcn_rcpf(1.0f + __expf(-z)); }

// A fragment of one 128x128 weight for this wave's 32 output rows, k-group g:
//  !TR: rows = out features of W (forward);  A[r] = W[32w+16it+il][16g+4q+r]
//   TR: rows = in features (dgrad, A = W^T); A[r] = W[16g+4q+r][32w+16it+il]
// Buffer loads (SGPR descriptor + ONE per-lane 32-bit offset + a compile-time scalar offset per fragment) keep the
// address arithmetic out of the vector registers: with flat loads hipcc hoists a 64-bit address per (matrix, k-group)
// out of the persistent tile loop — 32+ VGPRs — and spills.
typedef __amdgpu_buffer_rsrc_t wrsrc_t;
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ wrsrc_t make_wrsrc(const float* W) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(W), 0, HID * HID * 4, 0x00020000);
}
template <bool TR>
__device__ __forceinline__ f32x4 load_afrag(wrsrc_t W, int fb, int il, int q, int it, int g) {
  if (!TR) {
    const int voff = ((fb + il) * HID + 4 * q) * 4;
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(W, voff, (16 * it * HID + 16 * g) * 4, 0));
  }
  const int voff = (4 * q * HID + fb + il) * 4;
  const int so = (16 * g * HID + 16 * it) * 4;
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(W, voff + r * HID * 4, so, 0));
  return v;
}

// The weights are streamed from L2 into registers PF k-groups ahead of use
// (a k-group = 16 MFMAs = 512 cycles of matrix pipe per wave), so only
// (PF+1) x 8 registers hold weights at any time; `pre` carries groups
// 0..PF-1 of the NEXT gemm across the phase boundary.
constexpr int PF = 2;
struct WPre { f32x4 a[PF]; };     // fragments j = 0..PF-1 of the next gemm (j = it*8 + g: row tile 0 first)

template <bool TR>
__device__ __forceinline__ void prefetch_w(wrsrc_t W, int fb, int il, int q, WPre& pre) {
#pragma unroll
  for (int j = 0; j < PF; ++j) pre.a[j] = load_afrag<TR>(W, fb, il, q, j >> 3, j & 7);
}

// acc[it][ck] += sum_k A[it][k] * buf[ck*16+il][k]   (K = 128, B operand from LDS), row tile 0 first, then
// row tile 1.  Software-pipelined by hand: the LDS reads of step j+1 and the global loads of step j+PF are
// issued ahead of the 8 MFMAs of step j; sched_barrier keeps hipcc from hoisting every load (which spills).
// HOOK: while the matrix pipe works on row tile 1, the VALU applies bias + Swish to the finished row tile 0
// (an MFMA occupies the vector issue port for only 8 of its 32 cycles):
//   HOOK 1 (train): h[0][0] = s(z), h[0][1] = s'(z) zdot;   HOOK 2 (inference): both column halves are primal.
template <bool TR, int HOOK, int IT>
__device__ __forceinline__ void gemm128(wrsrc_t W, const WPre& pre, const float* buf, int fb, int il,
                                        int q, f32x4 (&acc)[IT][2], const float* bias_lds, f32x4 (&h)[IT][2]) {
  constexpr int NJ = 8 * IT;
  constexpr bool OVL = HOOK && IT == 2;   // a second row tile to hide the first one's Swish under
  f32x4 ring[PF + 1];
#pragma unroll
  for (int j = 0; j < PF; ++j) ring[j] = pre.a[j];
  const float* bp0 = buf + il * ACT_P + 4 * q;
  const float* bp1 = buf + (16 + il) * ACT_P + 4 * q;
  f32x4 bn0 = *reinterpret_cast<const f32x4*>(bp0), bn1 = *reinterpret_cast<const f32x4*>(bp1);
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int it = j >> 3;
    const f32x4 b0 = bn0, b1 = bn1;
    if (j + PF < NJ) ring[(j + PF) % (PF + 1)] = load_afrag<TR>(W, fb, il, q, (j + PF) >> 3, (j + PF) & 7);
    if (j + 1 < NJ) {
      bn0 = *reinterpret_cast<const f32x4*>(bp0 + 16 * ((j + 1) & 7));
      bn1 = *reinterpret_cast<const f32x4*>(bp1 + 16 * ((j + 1) & 7));
    }
    if (OVL && j == 8) {        // row tile 0 is complete: bias
      const f32x4 bb = *reinterpret_cast<const f32x4*>(bias_lds + fb + 4 * q);
      acc[0][0] += bb;
      if (HOOK == 2) acc[0][1] += bb;
    }
    if (OVL && j >= 8 && j < 12) {   // one register per step
      const int r = j - 8;
      if (HOOK == 1) {
        float s0, s1, s2;
        swish012(acc[0][0][r], s0, s1, s2);
        h[0][0][r] = s0; h[0][1][r] = s1 * acc[0][1][r];
      } else {
        h[0][0][r] = swish0(acc[0][0][r]); h[0][1][r] = swish0(acc[0][1][r]);
      }
    }
    const f32x4 a = ring[j % (PF + 1)];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      acc[it][0] = mfma16(a[r], b0[r], acc[it][0]);
      acc[it][1] = mfma16(a[r], b1[r], acc[it][1]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}
// row tiles whose bias + Swish the caller still has to apply after gemm128<.., HOOK != 0, IT>
template <int IT> struct GemmTail { static constexpr int FIRST = IT == 2; };

// bias + (dual) Swish of row tiles [first, IT): train -> h = (s(z), s'(z) zdot); inference -> both halves primal
template <bool TRAIN, int IT>
__device__ __forceinline__ void bias_swish(f32x4 (&z)[IT][2], f32x4 (&h)[IT][2], const float* bias_lds, int fb, int q, int first) {
#pragma unroll
  for (int it = 0; it < IT; ++it) {
    if (it < first) continue;
    const f32x4 bb = *reinterpret_cast<const f32x4*>(bias_lds + fb + 16 * it + 4 * q);
    z[it][0] += bb;
    if (!TRAIN) z[it][1] += bb;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (TRAIN) {
        float s0, s1, s2; swish012(z[it][0][r], s0, s1, s2);
        h[it][0][r] = s0; h[it][1][r] = s1 * z[it][1][r];
      } else { h[it][0][r] = swish0(z[it][0][r]); h[it][1][r] = swish0(z[it][1][r]); }
    }
  }
}

// store this wave's C-layout tile pair to an activation buffer ([sample][feature])
template <int IT>
__device__ __forceinline__ void store_act(float* buf, int fb, int il, int q, const f32x4 (&h)[IT][2]) {
#pragma unroll
  for (int it = 0; it < IT; ++it)
#pragma unroll
    for (int ck = 0; ck < 2; ++ck)
      *reinterpret_cast<f32x4*>(buf + (ck * 16 + il) * ACT_P + fb + 16 * it + 4 * q) = h[it][ck];
}

// dW[it][kt] += sum_n ZB[feat][n] * HB[k][n] over the 32 dual columns.
// A (lane il = feature) and B (lane il = k) are read as b32 from [sample][feature]
// buffers, one (ck,s) step ahead of the MFMAs that consume them.
// SWISH: the dual Swish backward of the NEXT pointwise stage is hidden under the MFMAs: step st also turns
// (gP,gT) -> (zbarP, zbarT), in place, for register (it = st>>2, r = st&3).
template <int KT, int IT, bool SWISH>
__device__ __forceinline__ void wgrad_core(const float* zb, const float* hb, int hb_pitch, int fb, int il, int q,
                                           f32x4 (&dW)[IT][KT], const f32x4 (*z)[2], f32x4 (*g)[2]) {
  if (KT * IT <= 4) {
    // thin products (dW1, dW4: one or two MFMAs per step): a one-step-ahead pipeline would expose one LDS round trip
    // per step (~8 x 130 cycles for 8 x 32 cycles of MFMA), so ALL operands are fetched first
    float pa[8][IT], pb[8][KT];
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      const int n = (st >> 2) * 16 + 4 * (st & 3) + q;
#pragma unroll
      for (int it = 0; it < IT; ++it) pa[st][it] = zb[n * ACT_P + fb + 16 * it + il];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) pb[st][kt] = hb[n * hb_pitch + 16 * kt + il];
    }
    if (SWISH) {
#pragma unroll
      for (int st = 0; st < 4 * IT; ++st) {
        const int it = st >> 2, r = st & 3;
        float s0, s1, s2;
        swish012(z[it][0][r], s0, s1, s2);
        const float gt = g[it][1][r];
        g[it][0][r] = g[it][0][r] * s1 + gt * (s2 * z[it][1][r]);
        g[it][1][r] = gt * s1;
      }
    }
#pragma unroll
    for (int st = 0; st < 8; ++st)
#pragma unroll
      for (int kt = 0; kt < KT; ++kt)
#pragma unroll
        for (int it = 0; it < IT; ++it) dW[it][kt] = mfma16(pa[st][it], pb[st][kt], dW[it][kt]);
    return;
  }
  float na[IT], nb[KT];
  {
    const int n = q;
#pragma unroll
    for (int it = 0; it < IT; ++it) na[it] = zb[n * ACT_P + fb + 16 * it + il];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) nb[kt] = hb[n * hb_pitch + 16 * kt + il];
  }
#pragma unroll
  for (int st = 0; st < 8; ++st) {
    float a[IT], b[KT];
#pragma unroll
    for (int it = 0; it < IT; ++it) a[it] = na[it];
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) b[kt] = nb[kt];
    if (st + 1 < 8) {
      const int n = ((st + 1) >> 2) * 16 + 4 * ((st + 1) & 3) + q;
#pragma unroll
      for (int it = 0; it < IT; ++it) na[it] = zb[n * ACT_P + fb + 16 * it + il];
#pragma unroll
      for (int kt = 0; kt < KT; ++kt) nb[kt] = hb[n * hb_pitch + 16 * kt + il];
    }
    if (SWISH && st < 4 * IT) {
      const int it = st >> 2, r = st & 3;
      float s0, s1, s2;
      swish012(z[it][0][r], s0, s1, s2);
      const float gt = g[it][1][r];
      g[it][0][r] = g[it][0][r] * s1 + gt * (s2 * z[it][1][r]);     // in place: g becomes (zbarP, zbarT)
      g[it][1][r] = gt * s1;
    }
#pragma unroll
    for (int kt = 0; kt < KT; ++kt)
#pragma unroll
      for (int it = 0; it < IT; ++it) dW[it][kt] = mfma16(a[it], b[kt], dW[it][kt]);
    __builtin_amdgcn_sched_barrier(0);
  }
}
// dual Swish backward in registers, in place: (gP,gT) cotangents of (hP,hT) -> cotangents of (zP,zT)
template <int IT>
__device__ __forceinline__ void swish_bwd_inplace(const f32x4 (&z)[IT][2], f32x4 (&g)[IT][2]) {
#pragma unroll
  for (int it = 0; it < IT; ++it)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s0, s1, s2;
      swish012(z[it][0][r], s0, s1, s2);
      const float gt = g[it][1][r];
      g[it][0][r] = g[it][0][r] * s1 + gt * (s2 * z[it][1][r]);
      g[it][1][r] = gt * s1;
    }
}

template <int KT, int IT>
__device__ __forceinline__ void wgrad(const float* zb, const float* hb, int hb_pitch, int fb, int il, int q, f32x4 (&dW)[IT][KT]) {
  wgrad_core<KT, IT, false>(zb, hb, hb_pitch, fb, il, q, dW, nullptr, nullptr);
}
template <int KT, int IT>
__device__ __forceinline__ void wgrad_swish(const float* zbuf, const float* hb, int hb_pitch, int fb, int il, int q,
                                            f32x4 (&dW)[IT][KT], const f32x4 (&z)[IT][2], f32x4 (&g)[IT][2]) {
  wgrad_core<KT, IT, true>(zbuf, hb, hb_pitch, fb, il, q, dW, z, g);
}

// ============================================================ phases that the two fused kernels share
// Each takes the thread's indices (il, q, tid, ...) from its caller: k_mlp_xw derives its own from an opaque lane value.
template <int IT, int K>
__device__ __forceinline__ void zero_tiles(f32x4 (&a)[IT][K]) {
#pragma unroll
  for (int it = 0; it < IT; ++it)
#pragma unroll
    for (int k = 0; k < K; ++k) a[it][k] = f32x4{0, 0, 0, 0};
}
template <int IT>
__device__ __forceinline__ void zero_tiles(f32x4 (&a)[IT]) {
#pragma unroll
  for (int it = 0; it < IT; ++it) a[it] = f32x4{0, 0, 0, 0};
}

// Offsets of the parameters in the flat parameter vector, which is also the layout of a gradient slab:
// W1 b1 W2 b2 W3 b3 W4 b4, every weight row-major [out][in].
struct MlpLayout {
  int64_t oW1, ob1, oW2, ob2, oW3, ob3, oW4, ob4, n_params;
  __host__ __device__ MlpLayout(int d, int in_dim) {
    oW1 = 0; ob1 = oW1 + (int64_t)HID * in_dim;
    oW2 = ob1 + HID; ob2 = oW2 + HID * HID;
    oW3 = ob2 + HID; ob3 = oW3 + HID * HID;
    oW4 = ob3 + HID; ob4 = oW4 + (int64_t)d * HID;
    n_params = ob4 + d;
  }
};

// ---- input pipeline: the tile's y / v / u / t / cst chunks (contiguous in global memory) are fetched into
// registers ONE TILE AHEAD (raw_issue), parked in LDS a phase later (raw_commit) and turned into the layer-1
// operand h0 at the end of the previous tile (build_h0) — no global-load latency sits on the tile's critical path.
// A thread holds NR elements of each chunk (element ev + NT k of the tile, ev = its index in the workgroup), and
// thread tid < SPT the t / cst of sample tid.  STAGE_U: the u chunk travels the same way (else its reader fetches it).
template <int NR> struct RawRegs { float y[NR], v[NR], u[NR], t = 0.f, c = 0.f, rw = 0.f, w[NR]; };

template <int MODE, class LO, int NT, bool STAGE_U, int NR>
__device__ __forceinline__ void raw_issue(const MlpArgs& A, RawRegs<NR>& pf, int ev, int tid, int64_t tl, int step) {
  constexpr int SPT = LO::SPT;
  const int d = A.P.d;
  const int64_t etot = A.B * d;
  const int64_t e0 = tl * SPT * d;                 // tl past the last tile => e0 >= etot => zeros
  const int cnt = SPT * d;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int e = ev + NT * k;
    const bool ok = e < cnt && e0 + e < etot;
    // EM loop: x was rewritten by THIS workgroup a sweep ago — device-scope load so no stale L1 line is served
    if (MODE == MODE_EM) pf.y[k] = ok ? __hip_atomic_load(A.y + e0 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.f;
    else if (MODE == MODE_SDE) {
      // sampler loop: the net's input is the state (stage 0) or the evaluation point the previous stage left in the
      // workspace, which also holds the step's Wiener increment since stage 0
      const int stage = sde_item(A, step).stage;
      pf.y[k] = ok ? load_agent((stage == 0 ? A.y : A.ws) + e0 + e) : 0.f;
      pf.w[k] = (ok && stage > 0) ? load_agent(A.ws + etot + e0 + e) : 0.f;
    } else pf.y[k] = ok ? A.y[e0 + e] : 0.f;
    if (MODE == MODE_TRAIN) {
      pf.v[k] = ok ? A.v[e0 + e] : 0.f;
      if (STAGE_U) pf.u[k] = (ok && A.u) ? A.u[e0 + e] : 0.f;
    }
  }
  if (tid < SPT) {
    const int64_t smp = tl * SPT + tid;
    if (MODE == MODE_SDE) pf.t = smp < A.B ? sde_item_time(A, sde_item(A, step)) : 0.f;
    else pf.t = smp < A.B ? (A.t ? A.t[smp] : ((MODE == MODE_EM && A.ts) ? A.ts[step] : A.t_scalar)) : 0.f;
    if (MODE == MODE_TRAIN) {
      pf.c = (smp < A.B && A.u && A.cst) ? A.cst[smp] : 0.f;
      // the ONLY test of the weight pointer (workgroup-uniform); in flight with t and cst.  Unweighted: 1, and x * 1 is x
      // to the bit, so everything after this line is one instruction sequence for both forms
      pf.rw = A.row_w ? (smp < A.B ? A.row_w[smp] : 0.f) : 1.f;
    }
  }
}
template <int MODE, class LO, int NT, bool STAGE_U, int NR>
__device__ __forceinline__ void raw_commit(const MlpArgs& A, const RawRegs<NR>& pf, float* R, int ev, int tid) {
  constexpr int SPT = LO::SPT, CHUNK = SPT * LO::DMAX;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int e = ev + NT * k;
    if (NR * NT == CHUNK || e < CHUNK) {           // (the last round may be a partial one)
      R[LO::RY + e] = pf.y[k];
      if (MODE == MODE_TRAIN) R[LO::RV + e] = pf.v[k];
      if constexpr (MODE == MODE_TRAIN && STAGE_U) R[LO::RU + e] = pf.u[k];
      if constexpr (MODE == MODE_SDE) R[LO::RW + e] = pf.w[k];
    }
  }
  if (tid < SPT) {
    R[LO::RT + tid] = pf.t;
    if (MODE == MODE_TRAIN) {
      R[LO::RC + tid] = pf.c;
      R[LO::RWT + tid] = pf.rw;
    }
  }
}
// h0 (and its tangent) of tile tl from its raw buffer, GS threads per sample row: thread (l, sub) takes the elements
// sub, sub + GS, .. of row l, and the norm of NormalizeLogRadius meets by shuffle within the group.
// premodule none: h0 = [y, t], h0dot = [v, 0]                     NN.py:113-119
// NormalizeLogRadius: h0 = [y/r, log r, t], r = |y| + 1e-6          NN.py:56-70
template <int MODE, class LO, int GS, int PITCH>
__device__ __forceinline__ void build_h0(const MlpArgs& A, float* H0b, const float* R, int64_t tl, int l, int sub) {
  constexpr bool TRN = MODE == MODE_TRAIN;
  const int d = A.P.d;
  const int64_t smp = tl * LO::SPT + l;
  const bool live = smp < A.B;
  float* hp = H0b + l * PITCH;
  float* ht = H0b + (16 + l) * PITCH;   // tangent row (train only)
  float tt = 0.f;
  if (live) {
    tt = R[LO::RT + l];
    if (mode_reverse(MODE)) tt = A.T - tt;                              // s = T - t  SDEs.py:556-557
  }
  const float* yr = R + LO::RY + l * d;
  const float* vr = R + LO::RV + l * d;
  if (A.P.premodule == 0) {
    for (int i = sub; i < d; i += GS) {
      hp[i] = yr[i];
      if (TRN) ht[i] = vr[i];
    }
    if (sub == 0) { hp[d] = tt; if (TRN) ht[d] = 0.f; }
  } else {
    float ss = 0.f, yv = 0.f;
    for (int i = sub; i < d; i += GS) {
      const float yi = live ? yr[i] : 1.0f;
      ss += yi * yi;
      if (TRN) yv += yi * vr[i];
    }
#pragma unroll
    for (int m = GS / 2; m > 0; m >>= 1) { ss += __shfl_xor(ss, m, 64); if (TRN) yv += __shfl_xor(yv, m, 64); }
    const float nr = sqrtf(ss);
    const float r = nr + 1e-6f;
    const float rdot = yv / nr;                                          // d|y| along v
    for (int i = sub; i < d; i += GS) {
      const float yi = live ? yr[i] : 1.0f;
      hp[i] = yi / r;
      if (TRN) ht[i] = vr[i] / r - yi * rdot / (r * r);
    }
    if (sub == 0) {
      hp[d] = logf(r);
      hp[d + 1] = tt;
      if (TRN) { ht[d] = rdot / r; ht[d + 1] = 0.f; }
    }
  }
}

// One hidden layer (2 or 3) of the forward pass: z = W . in (`pre` holds W's first fragments and leaves with those of
// Wnext, the next gemm's weights, transposed if NEXT_TR), h = Swish(z + bias) (train: and its tangent).
template <bool TRN, bool NEXT_TR, int IT>
__device__ __forceinline__ void fwd_hidden(wrsrc_t W, wrsrc_t Wnext, WPre& pre, const float* in, const float* bias_lds,
                                           int fb, int il, int q, f32x4 (&z)[IT][2], f32x4 (&h)[IT][2]) {
  zero_tiles(z);
  gemm128<false, (TRN ? 1 : 2), IT>(W, pre, in, fb, il, q, z, bias_lds, h);
  prefetch_w<NEXT_TR>(Wnext, fb, il, q, pre);         // head of the next gemm's weights
  bias_swish<TRN, IT>(z, h, bias_lds, fb, q, GemmTail<IT>::FIRST);
}

// One hidden layer (3 or 2) of the backward pass.  zb holds the layer's zbar (cotangent of its pre-activation, dual),
// hb its input activations, z the pre-activations of the layer below:
//   g = W^T . zbar (dgrad), dW += zbar . hb^T, g <- Swish'(z) g in place (zbar of the layer below), db += g, g -> dst.
// wgrad_first: the weight gradient (which needs only this wave's zbar columns) runs before the dgrad, Swish' last.
template <bool NEXT_TR, int IT>
__device__ __forceinline__ void bwd_hidden(wrsrc_t W, wrsrc_t Wnext, WPre& pre, const float* zb, const float* hb, float* dst,
                                           int fb, int il, int q, f32x4 (&dW)[IT][8], const f32x4 (&z)[IT][2],
                                           f32x4 (&db)[IT], f32x4 (&g)[IT][2], bool wgrad_first) {
  f32x4 unused[IT][2];
  zero_tiles(g);
  if (!wgrad_first) {
    gemm128<true, 0, IT>(W, pre, zb, fb, il, q, g, nullptr, unused);
    prefetch_w<NEXT_TR>(Wnext, fb, il, q, pre);
    wgrad_swish<8, IT>(zb, hb, ACT_P, fb, il, q, dW, z, g);
  } else {
    wgrad<8, IT>(zb, hb, ACT_P, fb, il, q, dW);
    gemm128<true, 0, IT>(W, pre, zb, fb, il, q, g, nullptr, unused);
    prefetch_w<NEXT_TR>(Wnext, fb, il, q, pre);
    swish_bwd_inplace<IT>(z, g);
  }
#pragma unroll
  for (int it = 0; it < IT; ++it) db[it] += g[it][0];
  store_act<IT>(dst, fb, il, q, g);
}

// Euler–Maruyama update of one element x of a sample at time t_raw, a = the network's output for it:
// x += [(1-l/2) sqrt(beta) a + 1/2 beta x] delta + sqrt(1-l) sqrt(beta) dW, ca = 1 - l/2
// (SDEs.py:556-561,587-588; sde_scheme.py:82-84,38-40); e = the element's index in x, which also keys its noise.
__device__ __forceinline__ float em_update(const MlpArgs& A, float ca, float a, float x, float t_raw, int64_t e, int step) {
  const float s = A.T - t_raw;
  const float beta = sde_beta(A.b0, A.b1, s);
  const float sb = sqrtf(beta);
  const float zz = A.z ? A.z[e] : philox_normal1(A.rng, A.rng_step + (uint64_t)step, RNG_STREAM_DW, (uint64_t)e);
  const float mu = ca * (sb * a) - (-0.5f * beta * x);
  return x + (mu * A.delta + (sqrtf(1.0f - A.lmbd) * sb) * (A.sqrt_delta * zz));
}

// ---- dense tensor with 17 <= n <= 30 (DENSE_MM): the contraction as a GEMM on the matrix cores, between the layer-4 reduce
// and the stage update.  With T[r,(i,k)] = sum_j x_rj G[i,j,k] both products come from one pass: gw_ri = sb sum_k T[r,i,k] w_rk
// and ga_ri likewise with a; one more block of the same shape, L_G in G's place, gives f_ri = beta sum_j L_G[i,j] x_rj.
//   M = the tile's 32 rows (A operand: the evaluation point in the raw row, j >= n masked to +0), K = j padded to 32,
//   N-block = 16 values of i at a FIXED k, so D holds T[row 4q + r][i = il] in register r and the lane multiplies it by
//   its rows' w_k / a_k (LDS broadcasts) and sums in registers: no cross-lane reduction.
// Wave (ib, kh) takes the i-half ib of the blocks k = kh, kh + 2, ..; the waves kh = 1 also take the L_G block.  A block is
// 2 x 8 MFMAs, the two row tiles being independent accumulator chains, and its B fragments (two b128 buffer loads a lane
// from the packed image, ops.pack_dense_g's layout: include/msgm_hip.h) are requested one block ahead.  The two k-halves of gw and ga land in
// two images each and are added by the reader, always in the order kh = 0, 1.
constexpr int DMM_P = 36;            // pitch of an image row [sample][o]: q's four rows fall into four different bank groups
constexpr int DMM_BLOCK = 2 * 2 * 64 * 4;   // floats of one block (k or L_G): [ib][sg][lane][r]
template <int NW>
struct MlpDenseLds : MlpLds<MODE_SDE, true, NW> {
  using Base = MlpLds<MODE_SDE, true, NW>;
  static constexpr int FI = Base::FLOATS;                 // L_G x
  static constexpr int GWI = FI + 32 * DMM_P;             // sum_k T w, k-half 0 | 1
  static constexpr int GAI = GWI + 2 * 32 * DMM_P;        // sum_k T a, k-half 0 | 1
  static constexpr int FLOATS = GAI + 2 * 32 * DMM_P;
  static constexpr int BYTES = FLOATS * 4;
  static_assert(NW == 4, "one wave per (i-half, k-half)");
  static_assert(Base::BYTES == 115456 && BYTES == 138496 && BYTES <= 160 * 1024, "the wide sampler carve plus five images must fit a CU");
};

struct NoDenseMM {
  static constexpr bool ON = false;
  struct Pre {};
  __device__ __forceinline__ Pre issue() const { return {}; }
  __device__ __forceinline__ void run(const Pre&) const {}
};
template <class LO, int AP>
struct DenseMM {
  static constexpr bool ON = true;
  const MlpArgs& A; const float* R; const float* AIMG; float* lds; int tid;
  struct Pre { f32x4 g0, g1; float xa[2][8]; };
  __device__ __forceinline__ wrsrc_t rsrc() const {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.Gp), 0, (A.P.d + 1) * DMM_BLOCK * 4, 0x00020000);
  }
  // fragment sg of block kk for i-half ib (all three scalar: the block's place is the buffer load's scalar offset)
  __device__ __forceinline__ f32x4 frag(wrsrc_t GR, int kk, int ib, int sg) const {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(GR, (tid & 63) * 16, ((kk * 2 + ib) * 2 + sg) * 1024, 0));
  }
  // at the head of the stage update: the wave's first block is requested and the A operand read while a and dW are formed
  __device__ __forceinline__ Pre issue() const {
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int il = tid & 15, q = (tid & 63) >> 4, n = A.P.d;
    const wrsrc_t GR = rsrc();
    Pre p;
    p.g0 = frag(GR, w >> 1, w & 1, 0); p.g1 = frag(GR, w >> 1, w & 1, 1);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const int j = 4 * s + q;
        p.xa[mt][s] = j < n ? R[LO::RY + (16 * mt + il) * n + j] : 0.f;
      }
    return p;
  }
  // after the barrier behind `gather` (a and the Wiener increment are complete); ends with the barrier its readers need
  __device__ __forceinline__ void run(const Pre& p) const {
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63, il = lane & 15, q = lane >> 4;
    const int ib = w & 1, kh = w >> 1, n = A.P.d;
    const wrsrc_t GR = rsrc();
    f32x4 g0 = p.g0, g1 = p.g1;
    const float (&xa)[2][8] = p.xa;
    // one block: acc[mt] = x (row tile mt) . the block whose fragments are c0 | c1
    auto block = [&](const f32x4& c0, const f32x4& c1, f32x4 (&acc)[2]) {
      acc[0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const float b = s < 4 ? c0[s & 3] : c1[s & 3];
        acc[0] = mfma16(xa[0][s], b, acc[0]);
        acc[1] = mfma16(xa[1][s], b, acc[1]);
      }
    };
    f32x4 gw[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}}, ga[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int kk = kh; kk < n; kk += 2) {
      const int nk = kk + 2 < n ? kk + 2 : n;         // behind the wave's last k: the L_G block (used by the waves kh = 1)
      const f32x4 c0 = g0, c1 = g1;
      g0 = frag(GR, nk, ib, 0); g1 = frag(GR, nk, ib, 1);
      float wv[2][4], av[2][4];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * mt + 4 * q + r;
          wv[mt][r] = R[LO::RW + row * n + kk];
          av[mt][r] = AIMG[row * AP + kk];
        }
      __builtin_amdgcn_sched_barrier(0);             // loads and LDS reads go out ahead of the MFMAs that hide them
      f32x4 acc[2];
      block(c0, c1, acc);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gw[mt][r] = __builtin_fmaf(acc[mt][r], wv[mt][r], gw[mt][r]);
          ga[mt][r] = __builtin_fmaf(acc[mt][r], av[mt][r], ga[mt][r]);
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (kh == 1) {
      f32x4 acc[2];
      block(g0, g1, acc);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) lds[LO::FI + (16 * mt + 4 * q + r) * DMM_P + 16 * ib + il] = acc[mt][r];
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int at = (kh * 32 + 16 * mt + 4 * q + r) * DMM_P + 16 * ib + il;
        lds[LO::GWI + at] = gw[mt][r];
        lds[LO::GAI + at] = ga[mt][r];
      }
    lds_barrier();
  }
  // element (c, o) of the row's f, gw, ga: dense_g's results
  __device__ __forceinline__ DenseTerms terms(int c, int o, float beta, float sb) const {
    const int at = c * DMM_P + o;
    const float tw = lds[LO::GWI + at] + lds[LO::GWI + 32 * DMM_P + at];
    const float ta = lds[LO::GAI + at] + lds[LO::GAI + 32 * DMM_P + at];
    return {beta * lds[LO::FI + at], sb * tw, sb * ta};
  }
};

// ---- sampler loop (MODE_SDE): the stage update behind the layer-4 reduce.  Thread (sample c, output o) owns element
// idx = c d + o of the tile — the element it fetched in raw_issue — and forms the stage's increment with the formulas of
// msgm_sde_stage (sde_stage.h), in the order of _em_step / _heun_step / _rk4_step (sde_scheme.py):
//   EM    stage 0: x <- x + K                                   (Ito form, norm correction)
//   Heun  stage 0: E = x + K1, S = K1;  stage 1 at E: x <- (x + S/2) + K2/2          (norm correction)
//   RK4   stage 0: E = x + K1/2, S = K1;  1 at E: E = x + K2/2, S += 2 K2;  2 at E: E = x + K3, S += 2 K3;
//         stage 3 at E: x <- x + (S + K4)/6                                           (norm correction)
// E (the next stage's evaluation point), the step's Wiener increment and S live in the caller's workspace and only travel
// to L2 and back.  Neighbours of x, a and dW in the row (sparse stencil, dense contraction) and the row sum of the norm
// correction are read from LDS: the raw row, the reduced layer-4 outputs (parked in wave 0's partial slice) and the
// updated row (in wave 1's slice, dead after the reduce).
template <int NR> struct SdeRegs { float xb[NR], sm[NR]; };
template <> struct SdeRegs<0> {};   // the other modes carry nothing

// the step's state x and the running sum S of this thread's elements: issued ahead of the layer-3 gemm
template <class LO, int NT, int NR>
__device__ __forceinline__ void sde_issue(const MlpArgs& A, SdeRegs<NR>& sr, const float* R, int64_t s_base, int tid, SdeItem it) {
  const int d = A.P.d;
  const int64_t etot = A.B * d;
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int idx = tid + NT * k;
    const int64_t e = s_base * d + idx;
    const bool ok = idx < LO::SPT * d && e < etot;
    sr.xb[k] = 0.f; sr.sm[k] = 0.f;
    if (ok && it.stage == 0) sr.xb[k] = R[LO::RY + idx];          // stage 0 is evaluated at x itself
    if (ok && it.stage > 0) { sr.xb[k] = load_agent(A.y + e); sr.sm[k] = load_agent(A.ws + 2 * etot + e); }
  }
}

// What the two kernels do differently is handed in: AIMG, the LDS image [sample][o] (pitch AP) of the net's output a, which
// `gather(c, o)` completes for element (c, o) before the first barrier (k_mlp: the bias plus the waves' K-slices; k_mlp_xw:
// nothing, layer 4 left it there); VIMG, a free image of the same pitch that takes the updated row under norm correction;
// `row_of(idx)` = idx / d.  ROWSUM: the row's sum of squares is formed once per row by the NT / SPT threads of a group
// (contiguous elements each, partial sums met by shuffle in a fixed order) and passed through RED, instead of every
// thread summing the whole row (at d = 128 that would be 128 LDS reads per element).  `dense` (DenseMM, else nothing): the
// phase that forms the dense tensor's f, gw and ga of the whole tile on the matrix cores once a and dW are complete (its
// first loads go out at the head); the dense branch then takes its terms from that phase's images instead of dense_g.
template <class LO, int NT, int AP, bool ROWSUM, int NR, class ROW, class GATHER, class DENSE = NoDenseMM>
__device__ __forceinline__ void sde_update(const MlpArgs& A, const SdeRegs<NR>& sr, const float* AIMG, float* VIMG, float* RED,
                                           ROW row_of, GATHER gather, float* R, int64_t s_base, int tid, SdeItem it,
                                           const DENSE dense = DENSE{}) {
  const int d = A.P.d, NS = A.n_stages;
  const int64_t etot = A.B * d;
  const bool last = it.stage == NS - 1;
  const bool nc = last && A.norm0;
  [[maybe_unused]] const typename DENSE::Pre dense_pre = dense.issue();
  StageArgs S{};
  S.kind = A.kind; S.proc = MSGM_PROC_REVERSE; S.strato = NS > 1;
  S.b0 = A.b0; S.b1 = A.b1; S.T = A.T; S.delta = A.delta; S.sqrt_delta = A.sqrt_delta; S.lmbd = A.lmbd;
  const float sig_scale = stage_sig_scale(S);
  // a into its image; stage 0 draws the step's Wiener increment
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int idx = tid + NT * k, c = row_of(idx), o = idx - c * d;
    const int64_t e = s_base * d + idx;
    if (idx < LO::SPT * d && e < etot) {
      gather(c, o);
      if (it.stage == 0) {
        const float zz = A.z ? A.z[(int64_t)it.i * etot + e]
                             : philox_normal1(A.rng, A.rng_step + (uint64_t)it.i, RNG_STREAM_DW, (uint64_t)e);
        const float w = A.sqrt_delta * zz;                     // delta**0.5 * randn   sde_scheme.py:84
        R[LO::RW + idx] = w;
        if (NS > 1) A.ws[etot + e] = w;
      }
    }
  }
  lds_barrier();
  if constexpr (DENSE::ON) dense.run(dense_pre);
  float val[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int idx = tid + NT * k, c = row_of(idx), o = idx - c * d;
    const int64_t e = s_base * d + idx;
    val[k] = 0.f;
    if (idx < LO::SPT * d && e < etot) {
      const float* xr = R + LO::RY + c * d;
      const float* wr = R + LO::RW + c * d;
      const float* ar = AIMG + c * AP;
      const StageCoef sc = stage_coef<false>(S, R[LO::RT + c], 0);
      const float xi = xr[o];
      float inc;
      if (A.kind == MSGM_SDE_SGM && !nc) {       // the flat kernel's spelling; with norm correction the row kernel's
        inc = diag_inc(S, DiagCoef{sc.beta, sc.sb, 1.0f - 0.5f * A.lmbd, sig_scale * sc.sb}, xi, ar[o], wr[o]);
      } else {
        float f, fs = 0.f, div, ga, gw;
        if (A.kind == MSGM_SDE_SGM) {
          f = -0.5f * sc.beta * xi; fs = f; div = 0.f;
          ga = sc.sb * ar[o]; gw = sc.sb * wr[o];
        } else if (A.kind == MSGM_SDE_MSGM_SPARSE) {
          const int ip = (o + 1 == d) ? 0 : o + 1, im = (o == 0) ? d - 1 : o - 1;
          const float xp = xr[ip], xm = xr[im];
          f = 0.5f * sc.beta * xi; div = 2.0f * f;
          gw = sparse_g(sc.sb, xp, xm, wr[o], wr[im]);
          ga = sparse_g(sc.sb, xp, xm, ar[o], ar[im]);
        } else {
          DenseTerms t;
          if constexpr (DENSE::ON) t = dense.terms(c, o, sc.beta, sc.sb);
          else t = dense_g(A.G, A.L_G, d, o, sc.beta, sc.sb, xr, wr, ar);
          f = t.f; div = 2.0f * f; gw = t.gw; ga = t.ga;
        }
        inc = stage_mu(S, ga, f, fs, div) * sc.delta + sig_scale * gw;      // sde_scheme.py:40
      }
      const float x = sr.xb[k];
      if (!last) {
        const float c_out = (NS == 4 && it.stage < 2) ? 0.5f : 1.0f;
        A.ws[e] = x + c_out * inc;
        A.ws[2 * etot + e] = it.stage == 0 ? inc : rk4_add(sr.sm[k], inc);
      } else {
        float v;
        if (NS == 1) v = x + 1.0f * inc;
        else if (NS == 2) { v = 1.0f * x; v += 0.5f * sr.sm[k]; v = v + 0.5f * inc; }
        else v = rk4_close(x, sr.sm[k], 0.f + 1.0f * inc);
        val[k] = v;
        if (nc) VIMG[c * AP + o] = v;
      }
    }
  }
  if (!last) return;
  if (nc) lds_barrier();
  if constexpr (ROWSUM) {
    if (nc) {
      constexpr int GS = NT / LO::SPT;                         // threads per row: elements [sub per, sub per + per) each
      const int c = tid / GS, sub = tid % GS, per = (d + GS - 1) / GS;
      const float* row = VIMG + c * AP;
      float ss = 0.f;
      for (int j = sub * per; j < (sub + 1) * per && j < d; ++j) ss += row[j] * row[j];
#pragma unroll
      for (int m = 1; m < GS; m <<= 1) ss += __shfl_xor(ss, m, 64);
      if (sub == 0) RED[c] = ss;
      lds_barrier();
    }
  }
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    const int idx = tid + NT * k, c = row_of(idx);
    const int64_t e = s_base * d + idx, smp = s_base + c;
    if (idx < LO::SPT * d && e < etot) {
      float v = val[k];
      if (nc) {                                                // x <- x norm0/|x|   sde_scheme.py:85-86
        float ss = 0.f;
        if constexpr (ROWSUM) ss = RED[c];
        else {
          const float* row = VIMG + c * AP;
          for (int j = 0; j < d; ++j) ss += row[j] * row[j];
        }
        v *= A.norm0[smp] / sqrtf(ss);
      }
      A.out[e] = v;
      const int index = it.i + A.include_t0;
      if (A.traj) A.traj[(int64_t)index * etot + e] = v;
      if (A.keep_stop && A.keep_stop[smp] == index) A.kept[e] = v;   // msgm_keep_rows after the step
    }
  }
}

// Sliced-score-matching terms of one output o of one sample: returns its share of the sample's loss and sets the
// cotangents of a and adot (wgt = ssm_seed: 1/batch, 0 for a dead row).  p = u_o in the general form, v_o in the SGM closed form:
//   general (MSGM): loss_b = sum_o adot_o u_o + cst_b + 1/2 a_o^2, u = (d mu/d a)^T v = G(y)^T v
//   SGM: loss_b = sum_o v_o (sqrt(beta) adot_o + 1/2 beta v_o) + 1/2 a_o^2     SDEs.py:631-646
__device__ __forceinline__ float ssm_terms(bool general, float a, float ad, float p, float beta, float sb, float wgt,
                                           float& ab, float& adb) {
  ab = a * wgt;
  if (general) { adb = p * wgt; return ad * p + 0.5f * a * a; }
  adb = sb * p * wgt;
  return p * (sb * ad + 0.5f * beta * p) + 0.5f * a * a;
}
// The seed of one sample row: inv_batch times the row's weight rw (its slot in the tile's raw buffer, read by the sample's
// 16 lanes as one LDS broadcast; exactly 1 without weights: inv_batch * 1 is inv_batch to the bit); 0 for a dead row.
// Zero-weight rows still go through the arithmetic: the caller keeps them finite.
__device__ __forceinline__ float ssm_seed(const MlpArgs& A, bool live, float rw) {
  return live ? A.inv_batch * rw : 0.f;
}
// The 16 threads (ol = 0..15) of a sample add up their terms; thread ol == 0 adds cst, counts the sample and stores it.
// The workgroup's sum takes rw * loss_b (rw: the row's weight, 1 without weights); the stored loss_per stays unweighted.
__device__ __forceinline__ void ssm_sample_loss(const MlpArgs& A, float lj, int ol, bool live, int64_t smp, const float* cst_lds,
                                                float rw, float& loss_acc) {
#pragma unroll
  for (int m = 8; m > 0; m >>= 1) lj += __shfl_xor(lj, m, 64);
  if (ol == 0 && live) {
    if (A.u && A.cst) lj += *cst_lds;
    loss_acc += rw * lj;
    if (A.loss_per) A.loss_per[smp] = lj;
  }
}

// Epilogue of a training workgroup: the resident dW2 / dW3 (lane (k = 16kt+il, q), reg r -> row fb+16it+4q+r) and the
// bias gradients of the hidden layers (primal cotangents summed over the 16 sample lanes) go to its slab.
template <int IT>
__device__ __forceinline__ void store_hidden_grads(float* slab, const MlpLayout& L, int fb, int il, int q,
                                                   const f32x4 (&dW2)[IT][8], const f32x4 (&dW3)[IT][8],
                                                   const f32x4 (&db1)[IT], const f32x4 (&db2)[IT], const f32x4 (&db3)[IT]) {
#pragma unroll
  for (int it = 0; it < IT; ++it)
#pragma unroll
    for (int kt = 0; kt < 8; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = fb + 16 * it + 4 * q + r, col = 16 * kt + il;
        slab[L.oW2 + row * HID + col] = dW2[it][kt][r];
        slab[L.oW3 + row * HID + col] = dW3[it][kt][r];
      }
#pragma unroll
  for (int it = 0; it < IT; ++it)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s1 = db1[it][r], s2 = db2[it][r], s3 = db3[it][r];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); s3 += __shfl_xor(s3, o, 64); }
      if (il == 0) {
        const int feat = fb + 16 * it + 4 * q + r;
        slab[L.ob1 + feat] = s1; slab[L.ob2 + feat] = s2; slab[L.ob3 + feat] = s3;
      }
    }
}
// The workgroup's loss: the 16 sample leaders (threads 0, 16, .. 240 of the loss phase) meet in RED, in a fixed order.
__device__ __forceinline__ void store_loss_sum(float* RED, int tid, float loss_acc, float* dst) {
  if (tid < 256 && (tid & 15) == 0) RED[tid >> 4] = loss_acc;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int j = 0; j < 16; ++j) s += RED[j];
    *dst = s;
  }
}

template <int MODE, bool WIDE, int NW, bool TINY = false, bool DENSE_MM = false>
__global__ void __launch_bounds__(64 * NW, 1) k_mlp(MlpArgs A) {
  static_assert(!DENSE_MM || (MODE == MODE_SDE && WIDE && !TINY), "the dense contraction phase belongs to the wide sampler loop");
  constexpr int NT = 64 * NW;         // threads
  constexpr int IT = 8 / NW;          // 16-feature row tiles per wave: 4 waves x 2 or 8 waves x 1
  constexpr int FW = 16 * IT;         // features owned by a wave
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int KT1 = WIDE ? 2 : 1;   // k-tiles of the first layer's input (in_dim <= 16 / 32)
  constexpr int OT = WIDE ? 2 : 1;    // o-tiles of the last layer's output (d <= 16 / 32)
  constexpr int SPT = (MODE == MODE_TRAIN) ? 16 : 32;   // samples per tile
  const int tid = threadIdx.x;
  const int w = tid >> 6, lane = tid & 63, il = lane & 15, q = lane >> 4;
  const int d = A.P.d;
  const int fb = FW * w;              // this wave's first feature
  using LO = std::conditional_t<DENSE_MM, MlpDenseLds<NW>, MlpLds<MODE, WIDE, NW, TINY>>;
  constexpr int SM_P = LO::SMP, DPAD = LO::DP, PP = LO::PP, DROWS = LO::DROWS;
  float* X = lds + LO::X; float* Y = lds + LO::Y; float* Z = lds + LO::Z; float* U = lds + LO::U;
  float* H0 = lds + LO::H0; float* ABAR = lds + LO::ABAR; float* PART = lds + LO::PART;
  float* W1s = lds + LO::W1; float* W4s = lds + LO::W4;
  float* B1s = lds + LO::B1; float* B2s = lds + LO::B2; float* B3s = lds + LO::B3; float* B4s = lds + LO::B4;
  float* DB4 = lds + LO::DB4; float* RED = lds + LO::RED;

  // persistent accumulators (train)
  f32x4 dW2[IT][8], dW3[IT][8], dW1[IT][KT1], dW4[IT][OT], db1[IT], db2[IT], db3[IT];
  float loss_acc = 0.f;
  if (MODE == MODE_TRAIN) {
    zero_tiles(dW2); zero_tiles(dW3); zero_tiles(dW1); zero_tiles(dW4);
    zero_tiles(db1); zero_tiles(db2); zero_tiles(db3);
  }

  // input pipeline (see raw_issue): one thread per sample row builds h0
  constexpr int NR = (SPT * LO::DMAX + NT - 1) / NT;
  float* RAW0 = lds + LO::RAW;
  RawRegs<NR> pf;
  [[maybe_unused]] SdeRegs<MODE == MODE_SDE ? NR : 0> sr;   // sampler loop: the stage update's own operands
  auto issue = [&](int64_t tl, int step = 0) { raw_issue<MODE, LO, NT, true>(A, pf, tid, tid, tl, step); };
  auto commit = [&](float* R) { raw_commit<MODE, LO, NT, true>(A, pf, R, tid, tid); };
  auto h0_row = [&](float* H0b, const float* R, int64_t tl, int l) { build_h0<MODE, LO, 1, SM_P>(A, H0b, R, tl, l, 0); };

  // ---- prologue.  The first tile's inputs and the first weight fragments go out first; the one-time staging of
  // the small layers and biases is written as fixed-trip loops with all global loads ahead of the LDS stores, so its
  // latency is ONE L2 round trip, not one per element (at the C2 sampler size a workgroup only has 4 tiles to
  // amortise this over).
  issue(blockIdx.x);
  const wrsrc_t R2 = make_wrsrc(A.P.W2), R3 = make_wrsrc(A.P.W3);
  WPre pre;
  prefetch_w<false>(R2, fb, il, q, pre);
  {
    constexpr int N1 = (HID * SM_P + NT - 1) / NT, N4 = (DROWS * ACT_P + NT - 1) / NT;
    float v1[N1], v4[N4], vb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < N1; ++k) {
      const int i = tid + NT * k, r = i / SM_P, c = i - r * SM_P;
      v1[k] = (i < HID * SM_P && c < A.in_dim) ? A.P.W1[r * A.in_dim + c] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < N4; ++k) {
      const int i = tid + NT * k, r = i / ACT_P, c = i - r * ACT_P;
      v4[k] = (i < DROWS * ACT_P && r < d && c < HID) ? A.P.W4[r * HID + c] : 0.f;
    }
    if (tid < HID) { vb[0] = A.P.b1[tid]; vb[1] = A.P.b2[tid]; vb[2] = A.P.b3[tid]; }
    if (tid < d) vb[3] = A.P.b4[tid];
#pragma unroll
    for (int k = 0; k < N1; ++k) { const int i = tid + NT * k; if (i < HID * SM_P) W1s[i] = v1[k]; }
#pragma unroll
    for (int k = 0; k < N4; ++k) { const int i = tid + NT * k; if (i < DROWS * ACT_P) W4s[i] = v4[k]; }
    if (tid < HID) { B1s[tid] = vb[0]; B2s[tid] = vb[1]; B3s[tid] = vb[2]; }
    if (tid < 32) B4s[tid] = vb[3];
    if (MODE == MODE_TRAIN) {
      for (int i = tid; i < 16 * DPAD; i += NT) DB4[i] = 0.f;
      for (int i = tid; i < 32 * SM_P; i += NT) ABAR[i] = 0.f;
    }
    for (int i = tid; i < 2 * 32 * SM_P; i += NT) H0[i] = 0.f;
  }
  commit(RAW0);
  __syncthreads();
  if (tid < SPT) h0_row(H0, RAW0, blockIdx.x, tid);
  __syncthreads();

  // layer 1 (K = in_dim, weights from LDS) of the tile whose h0 sits in H0b: z1 stays in registers (train: needed
  // again by the Swish backward), h1 goes to `dst`.  It runs one tile AHEAD — in the prologue for the first tile, then
  // at the tail of every tile for the next one, into the activation buffer that tile no longer needs — so the tile
  // loop starts directly with the layer-2 gemm and has no layer-1 phase / barrier of its own.
  constexpr bool TRN = MODE == MODE_TRAIN;
  f32x4 z1[IT][2];
  auto layer1 = [&](const float* H0b, float* dst) {
    f32x4 h1[IT][2];
    zero_tiles(z1);
    for (int s = 0; s < A.in4; ++s) {
      const float bP = H0b[il * SM_P + 4 * s + q];
      const float bT = H0b[(16 + il) * SM_P + 4 * s + q];
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        const float a = W1s[(fb + 16 * it + il) * SM_P + 4 * s + q];
        z1[it][0] = mfma16(a, bP, z1[it][0]); z1[it][1] = mfma16(a, bT, z1[it][1]);
      }
    }
    bias_swish<TRN, IT>(z1, h1, B1s, fb, q, 0);
    store_act<IT>(dst, fb, il, q, h1);
  };
  layer1(H0, X);
  __syncthreads();

  STAMP_DECL
  const int64_t n_tiles = (A.B + SPT - 1) / SPT;
  const float ca = 1.0f - 0.5f * A.lmbd;
  int cur = 0;      // parity of the tile: selects the h0 / raw buffers and which of X / Y holds h1
  // Waves w and w + NW/2 share a SIMD and would otherwise walk through the backward phases in lockstep (both in their
  // LDS-latency head, both in their VALU tail).  The second one runs its weight-gradient product BEFORE its dgrad, so
  // one wave's heads and tails fall under the other's MFMAs.
  const bool late = NW == 8 && w >= NW / 2;

  // Work items are (step, tile) with the tile index fastest; training / forward / single-step EM have one step.
  // EM loop (n_steps > 1): rows never interact (sde_scheme.py:82-86), so a workgroup takes its tiles through ALL
  // steps in one launch — weights and biases are staged once, x only travels to L2 and back.  The host guarantees
  // >= 2 tiles per workgroup, so the item prefetched one ahead is always a tile whose previous step is complete.
  // Sampler loop (MODE_SDE): items are (step, stage, tile); `step` counts (step, stage) pairs, see sde_item.  A stage reads
  // what the tile's previous stage wrote, so the same two-tile guarantee covers it.
  const int n_steps = MODE == MODE_SDE ? A.n_steps * A.n_stages : ((MODE == MODE_EM && A.n_steps > 1) ? A.n_steps : 1);
  int step = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles;) {
    const int64_t s_base = tile * SPT;
    int64_t ntile = tile + gridDim.x;           // the next item
    int nstep = step;
    if (ntile >= n_tiles) { ++nstep; ntile = nstep < n_steps ? (int64_t)blockIdx.x : n_tiles; }
    const float* H0c = H0 + cur * 32 * SM_P;
    float* H0n = H0 + (cur ^ 1) * 32 * SM_P;
    const float* Rc = RAW0 + cur * LO::RAWN;
    float* Rn = RAW0 + (cur ^ 1) * LO::RAWN;
    float* Xc = cur ? Y : X;          // h1 of this tile (written one tile ahead)
    float* Yc = cur ? X : Y;          // h2 of this tile; after phase 6 (train) / 3 (inference): h1 of the next tile
    f32x4 z2[IT][2], z3[IT][2], h[IT][2];
    cur ^= 1;

    // ---- phase 2: layer 2 --------------------------------------------------
    if (MODE != MODE_TRAIN) issue(ntile, nstep);
    fwd_hidden<TRN, false, IT>(R2, R3, pre, Xc, B2s, fb, il, q, z2, h);
    store_act<IT>(Yc, fb, il, q, h);
    if (MODE != MODE_TRAIN) commit(Rn);
    lds_barrier();
    STAMP(2);

    // ---- phase 3: layer 3, then this wave's K-slice of layer 4 -------------
    if (MODE != MODE_TRAIN) { if (tid < SPT) h0_row(H0n, Rn, ntile, tid); }   // next item's layer-1 operand
    else issue(ntile);                                       // train: next tile's inputs, in flight during the gemm
    if constexpr (MODE == MODE_SDE) sde_issue<LO, NT>(A, sr, Rc, s_base, tid, sde_item(A, step));   // sampler loop: likewise
    fwd_hidden<TRN, TRN, IT>(R3, TRN ? R3 : R2, pre, Yc, B3s, fb, il, q, z3, h);   // then W3^T for dgrad / next tile's layer 2
    if (MODE == MODE_TRAIN) store_act<IT>(Z, fb, il, q, h);   // h3 is the dW4 operand later
    {
      // partial[o][col] = sum_{k in this wave's FW features} W4[o][k] h3[k][col]; B operand = registers
#pragma unroll
      for (int ot = 0; ot < OT; ++ot) {
        f32x4 p0 = {0, 0, 0, 0}, p1 = {0, 0, 0, 0};
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          f32x4 a4 = {0.f, 0.f, 0.f, 0.f};                  // output rows >= DROWS are zero padding
          if (16 * ot + il < DROWS) a4 = *reinterpret_cast<const f32x4*>(W4s + (16 * ot + il) * ACT_P + fb + 16 * it + 4 * q);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            p0 = mfma16(a4[r], h[it][0][r], p0);
            p1 = mfma16(a4[r], h[it][1][r], p1);
          }
        }
        if (16 * ot + 4 * q < PP) {                         // (tiny carve: only the first 8 output columns exist)
          *reinterpret_cast<f32x4*>(PART + (w * 32 + il) * PP + 16 * ot + 4 * q) = p0;
          *reinterpret_cast<f32x4*>(PART + (w * 32 + 16 + il) * PP + 16 * ot + 4 * q) = p1;
        }
      }
    }
    if (MODE == MODE_TRAIN) commit(Rn);
    lds_barrier();
    STAMP(3);

    // ---- phase 4: reduce layer-4 partials; outputs / loss ------------------
    if constexpr (MODE == MODE_SDE) {
      // the update first: its stores drain to L2 under the next item's layer 1
      // a = b4 + the waves' K-slices, parked in wave 0's slice; the updated row goes to wave 1's (dead after the reduce)
      auto row_of = [=](int idx) { return idx / d; };
      auto gather = [=](int c, int o) {
        float a = B4s[o];
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) a += PART[(ww * 32 + c) * PP + o];
        PART[c * PP + o] = a;
      };
      // (stage 0 parks dW in the raw row)
      if constexpr (DENSE_MM)
        sde_update<LO, NT, PP, false>(A, sr, PART, PART + 32 * PP, nullptr, row_of, gather, const_cast<float*>(Rc), s_base, tid,
                                      sde_item(A, step), DenseMM<LO, PP>{A, Rc, PART, lds, tid});
      else
        sde_update<LO, NT, PP, false>(A, sr, PART, PART + 32 * PP, nullptr, row_of, gather, const_cast<float*>(Rc), s_base, tid,
                                      sde_item(A, step));
      layer1(H0n, Yc);                                         // next item's h1 (h2 is dead)
      __syncthreads();   // + vmcnt(0): what this item wrote must have left the CU before a later item re-reads it
      tile = ntile; step = nstep;
      continue;
    }
    if (MODE == MODE_FWD || MODE == MODE_EM) {
      layer1(H0n, Yc);                                         // next tile's h1 (h2 is dead)
      // 32 samples x d outputs
      for (int idx = tid; idx < 32 * d; idx += NT) {
        const int c = idx / d, o = idx - c * d;
        const int64_t smp = s_base + c;
        if (smp < A.B) {
          float a = B4s[o];
#pragma unroll
          for (int ww = 0; ww < NW; ++ww) a += PART[(ww * 32 + c) * PP + o];
          const int64_t e = smp * d + o;
          // EM: the sample's time is this item's (ts[step] in the EM loop)
          A.out[e] = MODE == MODE_FWD ? a : em_update(A, ca, a, Rc[LO::RY + idx], Rc[LO::RT + c], e, step);
        }
      }
      if (n_steps > 1) __syncthreads();   // + vmcnt(0): this tile's new x must have left the CU before it is re-read
      else lds_barrier();                 // PART / H0 are rewritten by the next tile
      tile = ntile; step = nstep;
      continue;
    }

    if (MODE == MODE_TRAIN) {
      if (tid < 256) {
        // thread (c = sample, ol = output): a, adot from the K-slices; the sample's loss terms meet by shuffle
        const int c = tid >> 4, ol = tid & 15;
        const int64_t smp = s_base + c;
        const bool live = smp < A.B;
        const float rw = Rc[LO::RWT + c];
        const float wgt = ssm_seed(A, live, rw);
        float beta = 0.f, sb = 0.f;
        if (!A.u) { beta = sde_beta(A.b0, A.b1, Rc[LO::RT + c]); sb = sqrtf(beta); }
        float lj = 0.f;
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) {
          const int o = 16 * ot + ol;
          const bool oo = o < d;
          float a = B4s[o], ad = 0.f;
#pragma unroll
          for (int ww = 0; ww < NW; ++ww) { a += PART[(ww * 32 + c) * PP + o]; ad += PART[(ww * 32 + 16 + c) * PP + o]; }
          const float p = oo ? Rc[(A.u ? LO::RU : LO::RV) + c * d + o] : 0.f;
          float ab, adb;
          lj += ssm_terms(A.u != nullptr, a, ad, p, beta, sb, wgt, ab, adb);
          ABAR[c * SM_P + o] = ab;
          ABAR[(16 + c) * SM_P + o] = adb;
          DB4[c * DPAD + o] += ab;
        }
        ssm_sample_loss(A, lj, ol, live, smp, Rc + LO::RC + c, rw, loss_acc);
      }
      // next tile's layer-1 operand, by a wave that has no part in the loss when there are eight
      if (tid >= NT - 64 && tid < NT - 64 + 16) h0_row(H0n, Rn, ntile, tid - (NT - 64));
      lds_barrier();
      STAMP(4);

      // ---- phase 5: layer-4 backward, dW4, Swish' on layer 3 --------------
      f32x4 g[IT][2];
      zero_tiles(g);
      for (int s = 0; s < A.d4; ++s) {
        const float bP = ABAR[il * SM_P + 4 * s + q];
        const float bT = ABAR[(16 + il) * SM_P + 4 * s + q];
#pragma unroll
        for (int it = 0; it < IT; ++it) {
          const float a = W4s[(4 * s + q) * ACT_P + fb + 16 * it + il];
          g[it][0] = mfma16(a, bP, g[it][0]); g[it][1] = mfma16(a, bT, g[it][1]);
        }
      }
      wgrad_swish<OT, IT>(Z, ABAR, SM_P, fb, il, q, dW4, z3, g);  // dW4^T[feat][o] += h3 . abar, Swish' hidden
#pragma unroll
      for (int it = 0; it < IT; ++it) db3[it] += g[it][0];
      store_act<IT>(U, fb, il, q, g);
      lds_barrier();
      STAMP(5);

      // ---- phase 6: dgrad layer 3 (W3^T, then W2^T goes out for the next dgrad), dW3, Swish' on layer 2; zbar2 -> Z
      // (h3 is dead after phase 5)
      bwd_hidden<true, IT>(R3, R2, pre, U, Yc, Z, fb, il, q, dW3, z2, db2, g, late);
      lds_barrier();
      STAMP(6);

      // ---- phase 7: dgrad layer 2 (W2^T, then the next tile's layer 2 goes out), dW2, Swish' on layer 1; zbar1 -> U
      // (zbar3 is dead after phase 6)
      bwd_hidden<false, IT>(R2, R2, pre, Z, Xc, U, fb, il, q, dW2, z1, db1, g, late);
      STAMP(7);
      // dW1 reads only THIS wave's columns of zbar1 (just written by this wave) and h0: no barrier in between
      wgrad<KT1, IT>(U, H0c, SM_P, fb, il, q, dW1);
      layer1(H0n, Yc);                                     // next tile's h1 (h2 is dead since phase 6)
      lds_barrier();     // ABAR/PART/.. are rewritten by the next tile
      STAMP(8);
    }
    tile = ntile; step = nstep;
  }

  // ---- epilogue (train): write this workgroup's gradient slab -------------
  if (MODE == MODE_TRAIN) {
    STAMP(9);
    float* slab = A.slabs + (int64_t)blockIdx.x * slab_stride(A.n_params);
    const int in_dim = A.in_dim;
    const MlpLayout L(d, in_dim);
    store_hidden_grads<IT>(slab, L, fb, il, q, dW2, dW3, db1, db2, db3);
    // dW1: lane (k = 16kt+il, q), reg r -> row 32w+16it+4q+r
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int kt = 0; kt < KT1; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = fb + 16 * it + 4 * q + r, col = 16 * kt + il;
          if (col < in_dim) slab[L.oW1 + (int64_t)row * in_dim + col] = dW1[it][kt][r];
        }
    // dW4 held transposed: lane (o = 16ot+il, q), reg r -> feature 32w+16it+4q+r
#pragma unroll
    for (int it = 0; it < IT; ++it)
#pragma unroll
      for (int ot = 0; ot < OT; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int feat = fb + 16 * it + 4 * q + r, o = 16 * ot + il;
          if (o < d) slab[L.oW4 + (int64_t)o * HID + feat] = dW4[it][ot][r];
        }
    __syncthreads();
    if (tid < d) {
      float s = 0.f;
      for (int j = 0; j < 16; ++j) s += DB4[j * DPAD + tid];
      slab[L.ob4 + tid] = s;
    }
    store_loss_sum(RED, tid, loss_acc, slab + A.n_params);
    STAMP(10);
    STAMP_FLUSH;
  }
}

// ============================================================ the extra-wide class (31 <= d <= 128)
// Once d can reach 128, layers 1 and 4 have the shape of layers 2 and 3 (128 x <= 132 and <= 128 x 128) and are run
// the same way: their weight fragments are streamed from L2 by buffer loads (nothing but activations and biases sits
// in LDS), and every wave owns output features of layer 4 too — row tiles w and w + 4, so d = 32 already spreads over
// two waves — instead of the narrow classes' K-split + LDS partial sum.  The loss phase reads a and adot from an LDS
// image of layer 4's output; the layer-4 dgrad is the transposed-A path with K = d padded to 16.  K of layer 1
// (in_dim) and of the layer-4 backward (d) is a run-time count of k-groups / k-tiles, so the work follows d.
// Registers: dW2 and dW3 are resident accumulators as in k_mlp; dW4 and dW1 (with them resident too the kernel
// spills) accumulate in the workgroup's own gradient slab: the wave's slice is read into registers a block at a time,
// extended by the tile's product and written back.  Only this lane ever touches those slab words, so no atomics, and
// the summation order is fixed.
#define XP 148   // pitch of an h0 row: in_dim <= 130 -> 9 k-groups of 16 (144) + 4

template <int MODE>
struct MlpLdsXW {
  static constexpr bool TRAIN = MODE == 2;
  static constexpr bool SDE = MODE == 3;
  static constexpr int SPT = TRAIN ? 16 : 32;      // samples per tile
  // raw input buffer: y | v (pitch d; sampler loop: y | dW), t, cst; u is read straight from global memory by the loss phase
  static constexpr int DMAX = HID;                 // raw rows are packed (pitch d), sized for d <= DMAX
  static constexpr int RY = 0;
  static constexpr int RV = RY + SPT * DMAX;
  static constexpr int RW = RV + (TRAIN ? SPT * DMAX : 0);
  static constexpr int RT = RW + (SDE ? SPT * DMAX : 0);
  static constexpr int RWT = RT + 16;              // train (16 rows a tile): the optional row weights, in RT's upper half
  static constexpr int RC = RT + 32;
  static constexpr int RAWN = RC + 16;
  static constexpr int X = 0;
  static constexpr int Y = X + 32 * ACT_P;
  static constexpr int Z = Y + 32 * ACT_P;                     // train: h3, then zbar2 (inference: h3 goes to X|Y)
  static constexpr int U = Z + (TRAIN ? 32 * ACT_P : 0);       // train: layer-4 output image, then zbar3, then zbar1
  static constexpr int ABAR = U + ((TRAIN || SDE) ? 32 * ACT_P : 0);   // (sampler loop: the image is all U holds); train: cotangent of layer 4's output [sample][o]
  static constexpr int H0 = ABAR + (TRAIN ? 32 * ACT_P : 0);   // double-buffered (built one tile ahead)
  static constexpr int B1 = H0 + 2 * 32 * XP;
  static constexpr int B2 = B1 + HID;
  static constexpr int B3 = B2 + HID;
  static constexpr int B4 = B3 + HID;
  static constexpr int RED = B4 + HID;
  static constexpr int RAW = RED + 64;
  static constexpr int FLOATS = RAW + 2 * RAWN;
  static constexpr int BYTES = FLOATS * 4;
  static_assert(BYTES <= 160 * 1024, "the extra-wide carve must fit the 160 KiB of LDS of a CU");
};

// Wait states written out after the last MFMAs of a loop with run-time trip count: their results are read by VALU
// code or stores behind a branch target, where hipcc has been seen to insert none.
__device__ __forceinline__ void mfma_drain() {
  asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// acc[it][ck] += sum_{g < ng} A(it, g) . buf[ck*16+il][16g + 4q + r] for the row tiles it < nit (both wave-uniform):
// the A fragments come from `afrag` (buffer loads, two k-groups ahead), the B operand from LDS one k-group ahead.
template <int IT, int GMAX, typename AF>
__device__ __forceinline__ void gemm_xw(AF afrag, const float* buf, int pitch, int il, int q, f32x4 (&acc)[IT][2],
                                        int ng, int nit) {
  f32x4 ring[3][IT];
  const float* bp0 = buf + il * pitch + 4 * q;
  const float* bp1 = buf + (16 + il) * pitch + 4 * q;
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int it = 0; it < IT; ++it) ring[j][it] = (j < ng && it < nit) ? afrag(it, j) : f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 bn0 = *reinterpret_cast<const f32x4*>(bp0), bn1 = *reinterpret_cast<const f32x4*>(bp1);
#pragma unroll
  for (int g = 0; g < GMAX; ++g) {
    if (g >= ng) continue;
    const f32x4 b0 = bn0, b1 = bn1;
    if (g + 2 < ng) {
#pragma unroll
      for (int it = 0; it < IT; ++it)
        if (it < nit) ring[(g + 2) % 3][it] = afrag(it, g + 2);
    }
    if (g + 1 < ng) {
      bn0 = *reinterpret_cast<const f32x4*>(bp0 + 16 * (g + 1));
      bn1 = *reinterpret_cast<const f32x4*>(bp1 + 16 * (g + 1));
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      if (it >= nit) continue;
      const f32x4 a = ring[g % 3][it];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[it][0] = mfma16(a[r], b0[r], acc[it][0]);
        acc[it][1] = mfma16(a[r], b1[r], acc[it][1]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  mfma_drain();
}

template <int MODE>
__global__ void __launch_bounds__(256, 1) k_mlp_xw(MlpArgs A) {
  constexpr int NW = 4, NT = 256, IT = 2, FW = 32;
  constexpr bool TRN = MODE == MODE_TRAIN;
  constexpr int SPT = TRN ? 16 : 32;
  constexpr int KT1 = 9;              // k-tiles of dW1 (in_dim <= 130)
  using LO = MlpLdsXW<MODE>;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x;
  const int w = tid >> 6, lane = tid & 63, il = lane & 15, q = lane >> 4;
  const int d = A.P.d, in_dim = A.in_dim;
  const int fb = FW * w;
  // Lane-dependent offsets of the streamed operands are derived from lane_v, which the tile loop re-defines opaquely
  // every iteration: otherwise hipcc hoists every (matrix, k-group, row) offset and mask out of the persistent loop as
  // a loop invariant — over a hundred registers — and spills.
  int lane_v = lane;
  const int ng1 = (in_dim + 15) >> 4;                          // k-groups of layer 1 = k-tiles of dW1
  const int nk4 = (d + 15) >> 4;                               // 16-output tiles of layer 4
  const int nit4 = (d > 16 * w ? 1 : 0) + (d > 16 * (w + NW) ? 1 : 0);   // this wave's layer-4 row tiles (w, w + 4)
  float* X = lds + LO::X; float* Y = lds + LO::Y; float* Z = lds + LO::Z; float* U = lds + LO::U;
  float* ABAR = lds + LO::ABAR; float* H0 = lds + LO::H0;
  float* B1s = lds + LO::B1; float* B2s = lds + LO::B2; float* B3s = lds + LO::B3; float* B4s = lds + LO::B4;
  float* RED = lds + LO::RED; float* RAW0 = lds + LO::RAW;

  f32x4 dW2[IT][8], dW3[IT][8], db1[IT], db2[IT], db3[IT];
  float db4[8];                       // thread (sample c, output lane ol) of the loss phase: outputs 16 ot + ol
  float loss_acc = 0.f;
  if (TRN) {
    zero_tiles(dW2); zero_tiles(dW3);
    zero_tiles(db1); zero_tiles(db2); zero_tiles(db3);
#pragma unroll
    for (int k = 0; k < 8; ++k) db4[k] = 0.f;
  }

  // input pipeline (see raw_issue); u is not staged: the loss phase reads it from global memory.  ALL threads build
  // h0, GS = NT / SPT per sample row.
  constexpr int NR = SPT * LO::DMAX / NT, GS = NT / SPT;
  RawRegs<NR> pf;
  [[maybe_unused]] SdeRegs<MODE == MODE_SDE ? NR : 0> sr;   // sampler loop: the stage update's own operands
  auto issue = [&](int64_t tl, int step = 0) { raw_issue<MODE, LO, NT, false>(A, pf, (w << 6) + lane_v, tid, tl, step); };
  auto commit = [&](float* R) { raw_commit<MODE, LO, NT, false>(A, pf, R, (w << 6) + lane_v, tid); };
  auto h0_rows = [&](float* H0b, const float* R, int64_t tl) {
    const int tv = (w << 6) + lane_v;
    build_h0<MODE, LO, GS, XP>(A, H0b, R, tl, tv / GS, tv % GS);
  };

  // ---- weight fragments.  W1 has pitch in_dim, W4 has d rows.  A lane whose element lies outside the matrix (a column
  // >= in_dim, a row >= d) gets a voffset past the buffer: it fetches nothing and reads an exact zero.  (The range
  // check does not cover the scalar offset, so the out-of-range lanes are moved in the voffset.)
  const wrsrc_t R1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.P.W1), 0, HID * in_dim * 4, 0x00020000);
  const wrsrc_t R2 = make_wrsrc(A.P.W2), R3 = make_wrsrc(A.P.W3);
  const wrsrc_t R4 = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(A.P.W4), 0, d * HID * 4, 0x00020000);
  constexpr int OFF_NONE = 0x7ffffff0;   // past every buffer here
  auto af1 = [&](int it, int g) {         // A[r] = W1[fb+16it+il][16g+4q+r]
    const int il_ = lane_v & 15, q_ = lane_v >> 4;
    const int voff1 = ((fb + il_) * in_dim + 4 * q_) * 4;
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 16 * g + 4 * q_ + r < in_dim ? voff1 + 4 * r : OFF_NONE;
      v[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(R1, o, (16 * it * in_dim + 16 * g) * 4, 0));
    }
    return v;
  };
  auto af4 = [&](int it, int g) {         // A[r] = W4[16(w+4it)+il][16g+4q+r]: this wave's output rows
    const int il_ = lane_v & 15, q_ = lane_v >> 4;
    const int o = 16 * (w + NW * it) + il_ < d ? ((16 * w + il_) * HID + 4 * q_) * 4 : OFF_NONE;
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(R4, o, (64 * it * HID + 16 * g) * 4, 0));
  };
  auto af4t = [&](int it, int g) {        // A = W4^T: A[r] = W4[16g+4q+r][fb+16it+il]
    const int il_ = lane_v & 15, q_ = lane_v >> 4;
    const int voff4t = (4 * q_ * HID + fb + il_) * 4;
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int o = 16 * g + 4 * q_ + r < d ? voff4t + r * HID * 4 : OFF_NONE;
      v[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(R4, o, (16 * g * HID + 16 * it) * 4, 0));
    }
    return v;
  };

  // ---- prologue
  issue(blockIdx.x);
  WPre pre;
  prefetch_w<false>(R2, fb, il, q, pre);
  if (tid < HID) {
    B1s[tid] = A.P.b1[tid]; B2s[tid] = A.P.b2[tid]; B3s[tid] = A.P.b3[tid];
    B4s[tid] = tid < d ? A.P.b4[tid] : 0.f;
  }
  for (int i = tid; i < 2 * 32 * XP; i += NT) H0[i] = 0.f;
  commit(RAW0);
  __syncthreads();
  h0_rows(H0, RAW0, blockIdx.x);
  __syncthreads();

  f32x4 z1[IT][2];
  auto layer1 = [&](const float* H0b, float* dst) {
    f32x4 h1[IT][2];
    zero_tiles(z1);
    gemm_xw<IT, KT1>(af1, H0b, XP, il, q, z1, ng1, IT);
    bias_swish<TRN, IT>(z1, h1, B1s, fb, q, 0);
    store_act<IT>(dst, fb, il, q, h1);
  };
  layer1(H0, X);
  __syncthreads();

  const int64_t n_tiles = (A.B + SPT - 1) / SPT;
  const float ca = 1.0f - 0.5f * A.lmbd;
  int cur = 0;
  float* slab = TRN ? A.slabs + (int64_t)blockIdx.x * slab_stride(A.n_params) : nullptr;
  const MlpLayout L(d, in_dim);
  // the slab's dW1 / dW4 words by buffer loads / stores (one per-lane offset per row; a masked-off word gets an offset
  // past the slab, where a load reads 0 and a store is dropped)
  const wrsrc_t RS = __builtin_amdgcn_make_buffer_rsrc(slab, 0, TRN ? (int)(slab_stride(A.n_params) * 4) : 0, 0x00020000);
  // dW1[fb + 4q][il] (+ r rows, + (it, kt) scalar) and dW4[o = il][fb + 4q] (+ (it, kt) scalar)
  auto vo1 = [&] { return (((fb + 4 * (lane_v >> 4)) * in_dim + (lane_v & 15)) * 4); };
  auto vo4 = [&] { return (int)((L.oW4 + (int64_t)(lane_v & 15) * HID + fb + 4 * (lane_v >> 4)) * 4); };
  // Items as in k_mlp: (step, tile), or (step, stage, tile) in the sampler loop, the tile fastest, >= 2 tiles per workgroup.
  const int n_steps = MODE == MODE_SDE ? A.n_steps * A.n_stages : ((MODE == MODE_EM && A.n_steps > 1) ? A.n_steps : 1);
  // sampler loop: idx / d for idx < 32 d <= 4096 by one multiply (idx r < 2^20 for the r <= d that mdiv d exceeds 2^20 by)
  const unsigned mdiv = (1u << 20) / (unsigned)d + 1u;
  int step = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles;) {
    asm volatile("" : "+v"(lane_v));
    const int64_t s_base = tile * SPT;
    int64_t ntile = tile + gridDim.x;
    int nstep = step;
    if (ntile >= n_tiles) { ++nstep; ntile = nstep < n_steps ? (int64_t)blockIdx.x : n_tiles; }
    const float* H0c = H0 + cur * 32 * XP;
    float* H0n = H0 + (cur ^ 1) * 32 * XP;
    const float* Rc = RAW0 + cur * LO::RAWN;
    float* Rn = RAW0 + (cur ^ 1) * LO::RAWN;
    float* Xc = cur ? Y : X;
    float* Yc = cur ? X : Y;
    f32x4 z2[IT][2], z3[IT][2], z4[IT][2], h[IT][2];
    cur ^= 1;

    // ---- layer 2
    if (!TRN) issue(ntile, nstep);
    fwd_hidden<TRN, false, IT>(R2, R3, pre, Xc, B2s, fb, il, q, z2, h);
    store_act<IT>(Yc, fb, il, q, h);
    if (!TRN) commit(Rn);
    lds_barrier();

    // ---- layer 3; h3 -> Z (train) / Xc (inference: h1 is dead)
    if (!TRN) h0_rows(H0n, Rn, ntile);
    else issue(ntile);
    if constexpr (MODE == MODE_SDE) sde_issue<LO, NT>(A, sr, Rc, s_base, (w << 6) + lane_v, sde_item(A, step));   // x and S, in flight during the gemm
    fwd_hidden<TRN, TRN, IT>(R3, TRN ? R3 : R2, pre, Yc, B3s, fb, il, q, z3, h);   // then W3^T for dgrad / next tile's layer 2
    float* H3 = TRN ? Z : Xc;
    store_act<IT>(H3, fb, il, q, h);
    if (TRN) commit(Rn);
    lds_barrier();

    // ---- layer 4: this wave's output row tiles 16(w + 4it), K = 128
    zero_tiles(z4);
    gemm_xw<IT, 8>(af4, H3, ACT_P, il, q, z4, 8, nit4);
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      if (it >= nit4) continue;
      const int o0 = 16 * (w + NW * it);
      const f32x4 bb = *reinterpret_cast<const f32x4*>(B4s + o0 + 4 * q);
      z4[it][0] += bb;
      if (!TRN) z4[it][1] += bb;
    }

    if constexpr (MODE == MODE_SDE) {
      // the stage update: thread tv owns elements tv + 256 k of the tile; a is read from the image, the updated row of the
      // norm correction goes to Yc (h2 is dead, the next item's h1 is not written yet), its row sums to RED.  Its stores
      // drain to L2 under the next item's layer 1.
      // layer-4 output image [sample][o], as the training mode's
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        if (it >= nit4) continue;
        const int o0 = 16 * (w + NW * it);
#pragma unroll
        for (int ck = 0; ck < 2; ++ck) *reinterpret_cast<f32x4*>(U + (ck * 16 + il) * ACT_P + o0 + 4 * q) = z4[it][ck];
      }
      lds_barrier();
      sde_update<LO, NT, ACT_P, true>(A, sr, U, Yc, RED, [&](int idx) { return (int)(((unsigned)idx * mdiv) >> 20); },
                                      [](int, int) {}, const_cast<float*>(Rc), s_base, (w << 6) + lane_v,
                                      sde_item(A, step));   // (stage 0 parks dW in Rc)
      layer1(H0n, Yc);                                   // next item's h1
      __syncthreads();   // + vmcnt(0): what this item wrote must have left the CU before a later item re-reads it
      tile = ntile; step = nstep;
      continue;
    } else if (!TRN) {
      // outputs straight from the accumulators: lane (sample 16ck + il), register r -> output o0 + 4q + r
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        if (it >= nit4) continue;
        const int o0 = 16 * (w + NW * it);
#pragma unroll
        for (int ck = 0; ck < 2; ++ck)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = 16 * ck + il, o = o0 + 4 * q + r;
            const int64_t smp = s_base + c;
            if (o < d && smp < A.B) {
              const float a = z4[it][ck][r];
              const int64_t e = smp * d + o;
              A.out[e] = MODE == MODE_FWD ? a : em_update(A, ca, a, Rc[LO::RY + c * d + o], Rc[LO::RT + c], e, step);
            }
          }
      }
      layer1(H0n, Yc);                                   // next item's h1 (h2 is dead)
      if (n_steps > 1) __syncthreads();                  // + vmcnt(0): this tile's new x must leave the CU before it is re-read
      else lds_barrier();
      tile = ntile; step = nstep;
      continue;
    }

    if (TRN) {
      // layer-4 output image [sample][o] for the loss phase
#pragma unroll
      for (int it = 0; it < IT; ++it) {
        if (it >= nit4) continue;
        const int o0 = 16 * (w + NW * it);
#pragma unroll
        for (int ck = 0; ck < 2; ++ck) *reinterpret_cast<f32x4*>(U + (ck * 16 + il) * ACT_P + o0 + 4 * q) = z4[it][ck];
      }
      lds_barrier();

      // ---- loss: thread (c = sample, ol) takes outputs 16 ot + ol; the sample's terms meet by shuffle
      {
        const int tv = (w << 6) + lane_v;
        const int c = tv >> 4, ol = tv & 15;
        const int64_t smp = s_base + c;
        const bool live = smp < A.B;
        const float rw = Rc[LO::RWT + c];
        const float wgt = ssm_seed(A, live, rw);
        float beta = 0.f, sb = 0.f;
        if (!A.u) { beta = sde_beta(A.b0, A.b1, Rc[LO::RT + c]); sb = sqrtf(beta); }
        float uo[8];
#pragma unroll
        for (int ot = 0; ot < 8; ++ot) {
          const int o = 16 * ot + ol;
          uo[ot] = (A.u && live && o < d) ? A.u[smp * d + o] : 0.f;
        }
        float lj = 0.f;
#pragma unroll
        for (int ot = 0; ot < 8; ++ot) {
          if (ot >= nk4) continue;
          const int o = 16 * ot + ol;
          const bool oo = o < d;
          const float a = oo ? U[c * ACT_P + o] : 0.f, ad = oo ? U[(16 + c) * ACT_P + o] : 0.f;
          const float p = A.u ? uo[ot] : (oo ? Rc[LO::RV + c * d + o] : 0.f);
          float ab, adb;
          lj += ssm_terms(A.u != nullptr, a, ad, p, beta, sb, wgt, ab, adb);
          ABAR[c * ACT_P + o] = ab;
          ABAR[(16 + c) * ACT_P + o] = adb;
          db4[ot] += ab;
        }
        ssm_sample_loss(A, lj, ol, live, smp, Rc + LO::RC + c, rw, loss_acc);
      }
      h0_rows(H0n, Rn, ntile);                           // next tile's layer-1 operand
      lds_barrier();

      // ---- layer-4 backward: dgrad (W4^T, K = d), dW4 into the slab, Swish' on layer 3
      const bool first = tile == (int64_t)blockIdx.x;
      f32x4 g[IT][2];
      zero_tiles(g);
      gemm_xw<IT, 8>(af4t, ABAR, ACT_P, il, q, g, nk4, IT);
      // dW4^T[feat][o] += h3 . abar through the slab, in blocks of two 16-output tiles: lane (o = 16kt + il, q),
      // register r -> feature fb + 16it + 4q + r
#pragma unroll
      for (int kb = 0; kb < 8; kb += 2) {
        if (kb >= nk4) continue;
        f32x4 dW4[IT][2];
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            const int v = (!first && 16 * (kb + kt) + (lane_v & 15) < d) ? vo4() : OFF_NONE;
            dW4[it][kt] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(RS, v, (16 * (kb + kt) * HID + 16 * it) * 4, 0));
          }
        wgrad<2, IT>(Z, ABAR + 16 * kb, ACT_P, fb, il, q, dW4);
        mfma_drain();
#pragma unroll
        for (int it = 0; it < IT; ++it)
#pragma unroll
          for (int kt = 0; kt < 2; ++kt) {
            const int v = 16 * (kb + kt) + (lane_v & 15) < d ? vo4() : OFF_NONE;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, dW4[it][kt]), RS, v, (16 * (kb + kt) * HID + 16 * it) * 4, 0);
          }
      }
      swish_bwd_inplace<IT>(z3, g);                      // Swish' of layer 3
#pragma unroll
      for (int it = 0; it < IT; ++it) db3[it] += g[it][0];
      store_act<IT>(U, fb, il, q, g);
      lds_barrier();

      // ---- dgrad layer 3 (W3^T), dW3, Swish' on layer 2; zbar2 -> Z
      bwd_hidden<true, IT>(R3, R2, pre, U, Yc, Z, fb, il, q, dW3, z2, db2, g, false);
      lds_barrier();

      // ---- dgrad layer 2 (W2^T), dW2, Swish' on layer 1, zbar1 -> U; dW1 (K = in_dim) into the slab; next tile's layer 1
      bwd_hidden<false, IT>(R2, R2, pre, Z, Xc, U, fb, il, q, dW2, z1, db1, g, false);
      // dW1 (this wave's own zbar1 columns: no barrier in between) through the slab, in blocks of one row tile x three
      // k-tiles (48 columns of h0; the columns past in_dim are zeros and are not stored):
      // lane (k = 16kt + il, q), register r -> row fb + 16it + 4q + r
#pragma unroll
      for (int it = 0; it < IT; ++it)
#pragma unroll
        for (int kb = 0; kb < KT1; kb += 3) {
          if (kb >= ng1) continue;
          f32x4 dW1[1][3];
#pragma unroll
          for (int kt = 0; kt < 3; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int v = (!first && 16 * (kb + kt) + (lane_v & 15) < in_dim) ? vo1() + r * in_dim * 4 : OFF_NONE;
              dW1[0][kt][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(RS, v, (16 * it * in_dim + 16 * (kb + kt)) * 4, 0));
            }
          wgrad<3, 1>(U, H0c + 16 * kb, XP, fb + 16 * it, il, q, dW1);
          mfma_drain();
#pragma unroll
          for (int kt = 0; kt < 3; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int v = 16 * (kb + kt) + (lane_v & 15) < in_dim ? vo1() + r * in_dim * 4 : OFF_NONE;
              float x = dW1[0][kt][r];
              asm volatile("" : "+v"(x));   // without it hipcc (ROCm 7.2) stores register 0 of the fragment for all four r
              __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x), RS, v, (16 * it * in_dim + 16 * (kb + kt)) * 4, 0);
            }
        }
      layer1(H0n, Yc);
      lds_barrier();
    }
    tile = ntile; step = nstep;
  }

  // ---- epilogue (train): the rest of this workgroup's gradient slab (dW1 and dW4 are already there)
  if (TRN) {
    store_hidden_grads<IT>(slab, L, fb, il, q, dW2, dW3, db1, db2, db3);
    __syncthreads();
    {
      const int c = tid >> 4, ol = tid & 15;
#pragma unroll
      for (int ot = 0; ot < 8; ++ot) X[c * HID + 16 * ot + ol] = db4[ot];   // X is free: 16 x 128 per-sample-lane sums
    }
    store_loss_sum(RED, tid, loss_acc, slab + A.n_params);   // (its barrier also covers X)
    if (tid < d) {
      float s = 0.f;
      for (int j = 0; j < 16; ++j) s += X[j * HID + tid];
      slab[L.ob4 + tid] = s;
    }
  }
}

// grads[p] = sum_wg slab[wg][p]; element n_params = loss sum (x inv_batch -> mean).
// 64 parameters (16 quads) x 16 slab groups per block, 16-B loads, fixed summation order (see the kernel).
// ADAM: one thread per parameter then applies the fused Adam update
// (single-GPU step: no all-reduce sits between the two), and thread 0 advances the
// Philox offset (nothing after this kernel reads it within the step).
template <bool ADAM>
__global__ void __launch_bounds__(256) k_slab_reduce(const float* __restrict__ slabs, int n_slabs, int64_t stride,
                                                     float* __restrict__ grads, int64_t n_params,
                                                     float* __restrict__ loss_sum, float inv_batch,
                                                     float* __restrict__ prm, float* __restrict__ m, float* __restrict__ v,
                                                     double lr, double b1, double b2, double eps,
                                                     const int64_t* __restrict__ step_dev, uint64_t* rng_advance) {
  // 64 parameters per block = 16 quads x 16 slab groups: thread (quad, group) sums every 16th slab with 16-B loads
  // (16 independent loads in flight), the 16 partial quads meet in LDS in a fixed order — deterministic.
  __shared__ f32x4 part[16][16];
  const int q4 = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int64_t p0 = (int64_t)blockIdx.x * 64 + 4 * q4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (p0 <= n_params)
    for (int g = grp; g < n_slabs; g += 16) acc += *reinterpret_cast<const f32x4*>(slabs + (int64_t)g * stride + p0);
  part[grp][q4] = acc;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int px = threadIdx.x;
    const int64_t p = (int64_t)blockIdx.x * 64 + px;
    if (p <= n_params) {
      float s = 0.f;
#pragma unroll
      for (int g = 0; g < 16; ++g) s += part[g][px >> 2][px & 3];
      if (p < n_params) {
        if (grads) grads[p] = s;
        if (ADAM) {
          const int64_t st = step_dev[0];
          const double bc1 = 1.0 - pow(b1, (double)st), bc2 = 1.0 - pow(b2, (double)st);
          const float step_size = (float)(lr / bc1), bc2_sqrt = (float)sqrt(bc2);
          const float w1 = (float)(1.0 - b1), b2f = (float)b2, w2 = (float)(1.0 - b2);
          const float mm = m[p] + w1 * (s - m[p]);
          const float vv = v[p] * b2f + w2 * (s * s);
          prm[p] = prm[p] - step_size * (mm / (sqrtf(vv) / bc2_sqrt + (float)eps));
          m[p] = mm; v[p] = vv;
        }
      } else if (loss_sum) loss_sum[0] = s * inv_batch;
    }
  }
  if (ADAM && rng_advance && blockIdx.x == 0 && threadIdx.x == 0) rng_advance[1] += 1;
}

// ============================================================ C ABI
static const int MLP_MAX_GRID = 256;

// Waves per workgroup.  Training at narrow width runs 8 waves x 16 features: two waves per SIMD, so one wave's
// Swish / LDS / barrier latencies are covered by the other's MFMAs (each holds half of the dW accumulators).  The
// wide carve (d > 15) has no LDS left for eight layer-4 K-slices and stays at 4 waves x 32 features.
template <int MODE, bool WIDE>
struct MlpCfg { static constexpr int NW = WIDE ? 4 : (MODE == MODE_TRAIN ? 8 : 4); };

// Launch kernel K with LDS bytes of dynamic LDS; the first launch raises the kernel's dynamic-LDS limit to that.
template <void (*K)(MlpArgs), int LDS, int BLOCK>
static int launch_kernel(const MlpArgs& A, int grid, hipStream_t st) {
  static const int once = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(K), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    return 0;
  }();
  (void)once;
  hipLaunchKernelGGL(K, dim3(grid), dim3(BLOCK), LDS, st, A);
  return msgm_check_launch();
}

// workgroups that fit one CU with this carve (inference modes: 2, or 3 with the tiny carve, 1 with the extra-wide one)
static bool mlp_tiny(const MlpArgs& A) { return A.in_dim <= 4 && A.P.d <= 4; }
static bool mlp_xwide(const MlpArgs& A) { return A.P.d > 30 || A.in_dim > 32; }
static int64_t mlp_wg_per_cu(const MlpArgs& A) { return mlp_xwide(A) ? 1 : (mlp_tiny(A) ? 3 : 2); }

template <int MODE>
static int launch_mlp(const MlpArgs& A, int grid, hipStream_t st) {
  if (mlp_xwide(A)) return launch_kernel<k_mlp_xw<MODE>, MlpLdsXW<MODE>::BYTES, 256>(A, grid, st);
  constexpr int nw_w = MlpCfg<MODE, true>::NW, nw_n = MlpCfg<MODE, false>::NW;
  if (A.in_dim > 16 || A.P.d > 16)
    return launch_kernel<k_mlp<MODE, true, nw_w, false>, MlpLds<MODE, true, nw_w>::BYTES, 64 * nw_w>(A, grid, st);
  constexpr bool T = MODE != MODE_TRAIN;     // the tiny carve is never instantiated for training
  if (T && mlp_tiny(A)) return launch_kernel<k_mlp<MODE, false, nw_n, T>, MlpLds<MODE, false, nw_n, T>::BYTES, 64 * nw_n>(A, grid, st);
  return launch_kernel<k_mlp<MODE, false, nw_n, false>, MlpLds<MODE, false, nw_n>::BYTES, 64 * nw_n>(A, grid, st);
}

static int fill_common(MlpArgs& A, const msgm_mlp_params_t* P, int64_t B) {
  if (!P || !P->W1 || !P->b1 || !P->W2 || !P->b2 || !P->W3 || !P->b3 || !P->W4 || !P->b4 || B <= 0) return MSGM_E_BADARG;
  if (P->d < 1 || P->d > HID || (P->premodule != 0 && P->premodule != 1)) return MSGM_E_UNSUPPORTED;
  A.P = *P; A.B = B;
  A.in_dim = P->d + 1 + (P->premodule ? 1 : 0);
  A.in4 = (A.in_dim + 3) / 4; A.d4 = (P->d + 3) / 4;
  return MSGM_OK;
}

// the arguments of a reverse-SDE Euler–Maruyama step on x (in place)
static int fill_em(MlpArgs& A, float* x, const msgm_sde_t* sde, float t, float delta, float lmbd, const float* z,
                   const uint64_t* rng, uint64_t rng_step) {
  if (!x || !sde) return MSGM_E_BADARG;
  if (sde->kind != MSGM_SDE_SGM) return MSGM_E_UNSUPPORTED;
  A.y = x; A.out = x; A.t = nullptr; A.t_scalar = t;
  A.b0 = sde->beta_min; A.b1 = sde->beta_max; A.T = sde->T;
  A.delta = delta; A.sqrt_delta = (float)sqrt((double)delta); A.lmbd = lmbd;
  A.z = z; A.rng = rng; A.rng_step = rng_step;
  return MSGM_OK;
}

extern "C" {

int64_t msgm_mlp_num_params(int32_t d, int32_t premodule) {
  return MlpLayout(d, d + 1 + (premodule ? 1 : 0)).n_params;
}

size_t msgm_mlp_ssm_workspace(int32_t d, int32_t premodule) {
  return (size_t)MLP_MAX_GRID * (size_t)slab_stride(msgm_mlp_num_params(d, premodule)) * sizeof(float);
}

int msgm_mlp_forward(const msgm_mlp_params_t* P, const float* y, const float* t, float* a, int64_t B,
                     msgm_stream_t stream) {
  MlpArgs A{};
  int rc = fill_common(A, P, B);
  if (rc) return rc;
  if (!y || !t || !a) return MSGM_E_BADARG;
  A.y = y; A.t = t; A.out = a;
  const int64_t tiles = (B + 31) / 32;
  const int64_t cap = mlp_wg_per_cu(A) * MLP_MAX_GRID;   // forward modes: two (tiny carve: three, extra-wide: one) workgroups per CU
  return launch_mlp<MODE_FWD>(A, (int)(tiles < cap ? tiles : cap), S(stream));
}

int msgm_mlp_em_step(const msgm_mlp_params_t* P, float* x, int64_t B, const msgm_sde_t* sde, float t, float delta,
                     float lmbd, const float* z, const uint64_t* rng, uint64_t rng_step, msgm_stream_t stream) {
  MlpArgs A{};
  int rc = fill_common(A, P, B);
  if (rc) return rc;
  if (!z && !rng) return MSGM_E_BADARG;
  rc = fill_em(A, x, sde, t, delta, lmbd, z, rng, rng_step);
  if (rc) return rc;
  const int64_t tiles = (B + 31) / 32;
  const int64_t cap = mlp_wg_per_cu(A) * MLP_MAX_GRID;
  return launch_mlp<MODE_EM>(A, (int)(tiles < cap ? tiles : cap), S(stream));
}

int msgm_mlp_em_loop(const msgm_mlp_params_t* P, float* x, int64_t B, const msgm_sde_t* sde, const float* ts, int32_t n_steps,
                     float delta, float lmbd, const uint64_t* rng, uint64_t rng_step0, msgm_stream_t stream) {
  MlpArgs A{};
  int rc = fill_common(A, P, B);
  if (rc) return rc;
  if (!ts || !rng || n_steps < 1) return MSGM_E_BADARG;
  rc = fill_em(A, x, sde, 0.f, delta, lmbd, nullptr, rng, rng_step0);
  if (rc) return rc;
  const int64_t tiles = (B + 31) / 32;
  if (tiles < 2) return MSGM_E_UNSUPPORTED;              // a workgroup needs two tiles to prefetch one ahead
  A.n_steps = n_steps; A.ts = ts;
  const int64_t cap = mlp_wg_per_cu(A) * MLP_MAX_GRID;
  const int64_t grid = tiles / 2 < cap ? tiles / 2 : cap;
  return launch_mlp<MODE_EM>(A, (int)grid, S(stream));
}

static int sde_loop_stages(int32_t method) {
  return method == MSGM_METHOD_EM ? 1 : (method == MSGM_METHOD_HEUN ? 2 : (method == MSGM_METHOD_RK4 ? 4 : 0));
}

int msgm_mlp_sde_loop_supported(int32_t d, int32_t premodule, int32_t kind, int64_t n, int64_t B) {
  if (d < 1 || d > 30 || d + 1 + (premodule ? 1 : 0) > 32 || n != d) return 0;     // the extra-wide class: msgm_mlp_xw_sde_loop
  if (kind != MSGM_SDE_SGM && kind != MSGM_SDE_MSGM_SPARSE && kind != MSGM_SDE_MSGM_DENSE) return 0;
  if (kind == MSGM_SDE_MSGM_DENSE && n > 16) return 0;   // dense_g is n^2 terms per element: 17 <= n <= 30 is msgm_mlp_dense_sde_loop's
  return B > 32;                                           // a workgroup needs two tiles to prefetch one ahead
}

size_t msgm_mlp_sde_loop_workspace(int64_t B, int32_t d, int32_t method) {
  if (B <= 0 || d <= 0 || sde_loop_stages(method) < 2) return 0;   // Euler-Maruyama keeps no state between stages
  return (size_t)3 * (size_t)B * (size_t)d * sizeof(float);
}

int msgm_mlp_xw_sde_loop_supported(int32_t d, int32_t premodule, int32_t kind, int64_t n, int64_t B) {
  if (d < 1 || d > HID || n != d) return 0;
  if (d <= 30 && d + 1 + (premodule ? 1 : 0) <= 32) return 0;                       // the narrower classes: msgm_mlp_sde_loop
  if (kind != MSGM_SDE_SGM && kind != MSGM_SDE_MSGM_SPARSE) return 0;              // a dense tensor stops at n = 30 (msgm_mlp_dense_sde_loop)
  return B > 32;                                           // a workgroup needs two tiles to prefetch one ahead
}

size_t msgm_mlp_xw_sde_loop_workspace(int64_t B, int32_t d, int32_t method) { return msgm_mlp_sde_loop_workspace(B, d, method); }

// Where the public samplers route to the loop: the supported shapes whose Heun and RK4 calls beat the composed route at the
// driver's size (B = 10 000, N = 128; DESIGN §4 has the table) — SGM up to d = 64, the sparse tensor up to d = 40.  Wider
// rows make an item longer than the composed route's launches, and the workgroup that carries a third tile sets the time.
int msgm_mlp_xw_sde_loop_preferred(int32_t d, int32_t premodule, int32_t kind, int64_t n, int64_t B) {
  if (!msgm_mlp_xw_sde_loop_supported(d, premodule, kind, n, B)) return 0;
  return kind == MSGM_SDE_SGM ? d <= 64 : d <= 40;
}

int msgm_mlp_dense_sde_loop_supported(int32_t d, int32_t premodule, int32_t kind, int64_t n, int64_t B) {
  if (kind != MSGM_SDE_MSGM_DENSE || n != d || d < 17 || d > 30 || d + 1 + (premodule ? 1 : 0) > 32) return 0;
  return B > 64;                                           // 32-row tiles, two a workgroup: B <= 64 is one workgroup on one CU
}

size_t msgm_mlp_dense_sde_loop_workspace(int64_t B, int32_t d, int32_t method) { return msgm_mlp_sde_loop_workspace(B, d, method); }

// Where the public samplers route to the dense loop: the supported shapes measured faster than the composed route of the
// same build by more than that route's own spread (tools/time_mlp_sde.py; DESIGN §4 has the table).
int msgm_mlp_dense_sde_loop_preferred(int32_t d, int32_t premodule, int32_t kind, int64_t n, int64_t B) {
  return msgm_mlp_dense_sde_loop_supported(d, premodule, kind, n, B);
}

size_t msgm_dense_g_packed_floats(int64_t n) { return n >= 1 && n <= 32 ? (size_t)(n + 1) * DMM_BLOCK : 0; }

// The sampler-loop entries: every check and argument in one place, `supported` is the entry's own shape rule.  `packed`
// and `dense_mm` belong to msgm_mlp_dense_sde_loop alone.
static int sde_loop_launch(int (*supported)(int32_t, int32_t, int32_t, int64_t, int64_t), const msgm_mlp_params_t* P, float* x,
                           int64_t B, const msgm_sde_t* sde, int32_t method, const float* ts, int32_t n_steps, float delta,
                           float sqrt_delta, float lmbd, const float* z, const uint64_t* rng, uint64_t rng_step0,
                           const float* norm0, float* traj, int32_t include_t0, const int32_t* keep_stop, float* kept,
                           void* workspace, size_t workspace_bytes, msgm_stream_t stream, bool dense_mm = false,
                           const float* packed = nullptr) {
  MlpArgs A{};
  int rc = fill_common(A, P, B);
  if (rc) return rc;
  const int stages = sde_loop_stages(method);
  if (!x || !sde || !ts || n_steps < 1 || !stages || (!z && !rng) || (keep_stop && !kept)) return MSGM_E_BADARG;
  if (sde->kind == MSGM_SDE_MSGM_DENSE && (!sde->G || !sde->L_G)) return MSGM_E_BADARG;
  if (dense_mm && !packed) return MSGM_E_BADARG;
  if (!supported(P->d, P->premodule, sde->kind, P->d, B)) return MSGM_E_UNSUPPORTED;
  const size_t need = msgm_mlp_sde_loop_workspace(B, P->d, method);
  if (need && (!workspace || workspace_bytes < need)) return MSGM_E_WORKSPACE;
  A.y = x; A.out = x; A.t = nullptr;
  A.b0 = sde->beta_min; A.b1 = sde->beta_max; A.T = sde->T;
  A.delta = delta; A.sqrt_delta = sqrt_delta; A.lmbd = lmbd;
  A.z = z; A.rng = rng; A.rng_step = rng_step0;
  A.n_steps = n_steps; A.ts = ts;
  A.n_stages = stages; A.kind = sde->kind;
  A.t_half = 0.5f * delta; A.t_full = delta;
  A.G = sde->G; A.L_G = sde->L_G;
  A.norm0 = norm0; A.ws = reinterpret_cast<float*>(workspace);
  A.traj = traj; A.include_t0 = include_t0 ? 1 : 0; A.keep_stop = keep_stop; A.kept = kept;
  const int64_t tiles = (B + 31) / 32;
  const int64_t cap = mlp_wg_per_cu(A) * MLP_MAX_GRID;
  const int64_t grid = tiles / 2 < cap ? tiles / 2 : cap;   // at least two tiles per workgroup
  if (dense_mm) {                                           // one workgroup per CU (138 496 B of LDS)
    A.Gp = packed;
    constexpr int nw = MlpCfg<MODE_SDE, true>::NW;
    return launch_kernel<k_mlp<MODE_SDE, true, nw, false, true>, MlpDenseLds<nw>::BYTES, 64 * nw>(
        A, (int)(grid < MLP_MAX_GRID ? grid : MLP_MAX_GRID), S(stream));
  }
  return launch_mlp<MODE_SDE>(A, (int)grid, S(stream));
}

int msgm_mlp_sde_loop(const msgm_mlp_params_t* P, float* x, int64_t B, const msgm_sde_t* sde, int32_t method, const float* ts,
                      int32_t n_steps, float delta, float sqrt_delta, float lmbd, const float* z, const uint64_t* rng,
                      uint64_t rng_step0, const float* norm0, float* traj, int32_t include_t0, const int32_t* keep_stop, float* kept,
                      void* workspace, size_t workspace_bytes, msgm_stream_t stream) {
  return sde_loop_launch(msgm_mlp_sde_loop_supported, P, x, B, sde, method, ts, n_steps, delta, sqrt_delta, lmbd, z, rng, rng_step0,
                         norm0, traj, include_t0, keep_stop, kept, workspace, workspace_bytes, stream);
}

// k_mlp_xw<MODE_SDE>: one workgroup per CU, so the grid is min(tiles / 2, 256)
int msgm_mlp_xw_sde_loop(const msgm_mlp_params_t* P, float* x, int64_t B, const msgm_sde_t* sde, int32_t method, const float* ts,
                         int32_t n_steps, float delta, float sqrt_delta, float lmbd, const float* z, const uint64_t* rng,
                         uint64_t rng_step0, const float* norm0, float* traj, int32_t include_t0, const int32_t* keep_stop,
                         float* kept, void* workspace, size_t workspace_bytes, msgm_stream_t stream) {
  return sde_loop_launch(msgm_mlp_xw_sde_loop_supported, P, x, B, sde, method, ts, n_steps, delta, sqrt_delta, lmbd, z, rng,
                         rng_step0, norm0, traj, include_t0, keep_stop, kept, workspace, workspace_bytes, stream);
}

// k_mlp<MODE_SDE, wide, DENSE_MM>: the dense tensor with 17 <= n <= 30, its contraction on the matrix cores
int msgm_mlp_dense_sde_loop(const msgm_mlp_params_t* P, float* x, int64_t B, const msgm_sde_t* sde, int32_t method, const float* ts,
                            int32_t n_steps, float delta, float sqrt_delta, float lmbd, const float* z, const uint64_t* rng,
                            uint64_t rng_step0, const float* norm0, float* traj, int32_t include_t0, const int32_t* keep_stop,
                            float* kept, void* workspace, size_t workspace_bytes, const float* g_packed, msgm_stream_t stream) {
  return sde_loop_launch(msgm_mlp_dense_sde_loop_supported, P, x, B, sde, method, ts, n_steps, delta, sqrt_delta, lmbd, z, rng,
                         rng_step0, norm0, traj, include_t0, keep_stop, kept, workspace, workspace_bytes, stream, true, g_packed);
}

int msgm_mlp_ssm_partial(const msgm_mlp_params_t* P, const float* y, const float* t, const float* v, const float* u,
                         const float* cst, int64_t B, const msgm_sde_t* sde, float inv_batch, float* loss_per,
                         void* workspace, size_t workspace_bytes, int32_t* n_slabs, msgm_stream_t stream) {
  return msgm_mlp_ssm_partial_w(P, y, t, v, u, cst, B, sde, inv_batch, nullptr, loss_per, workspace, workspace_bytes, n_slabs, stream);
}

int msgm_mlp_ssm_partial_w(const msgm_mlp_params_t* P, const float* y, const float* t, const float* v, const float* u,
                           const float* cst, int64_t B, const msgm_sde_t* sde, float inv_batch, const float* row_w,
                           float* loss_per, void* workspace, size_t workspace_bytes, int32_t* n_slabs,
                           msgm_stream_t stream) {
  MlpArgs A{};
  int rc = fill_common(A, P, B);
  if (rc) return rc;
  if (!y || !t || !v || !sde || !workspace || !n_slabs) return MSGM_E_BADARG;
  if (sde->kind != MSGM_SDE_SGM && !u) return MSGM_E_UNSUPPORTED;      // MSGM needs u = G(y)^T v (msgm_ssm_terms)
  if (workspace_bytes < msgm_mlp_ssm_workspace(P->d, P->premodule)) return MSGM_E_WORKSPACE;
  A.y = y; A.t = t; A.v = v; A.u = u; A.cst = cst;
  A.b0 = sde->beta_min; A.b1 = sde->beta_max; A.T = sde->T;
  A.inv_batch = inv_batch; A.row_w = row_w; A.loss_per = loss_per; A.slabs = reinterpret_cast<float*>(workspace);
  A.n_params = msgm_mlp_num_params(P->d, P->premodule);
  const int64_t tiles = (B + 15) / 16;
  const int grid = (int)(tiles < MLP_MAX_GRID ? tiles : MLP_MAX_GRID);
  *n_slabs = grid;
  return launch_mlp<MODE_TRAIN>(A, grid, S(stream));
}

int msgm_mlp_ssm_reduce(int32_t d, int32_t premodule, const void* workspace, int32_t n_slabs, float inv_batch,
                        float* grads, float* loss_sum, msgm_stream_t stream) {
  if (!workspace || !grads || n_slabs < 1 || n_slabs > MLP_MAX_GRID) return MSGM_E_BADARG;
  const int64_t n_params = msgm_mlp_num_params(d, premodule);
  hipLaunchKernelGGL(k_slab_reduce<false>, dim3((unsigned)((n_params + 1 + 63) / 64)), dim3(256), 0, S(stream),
                     reinterpret_cast<const float*>(workspace), n_slabs, slab_stride(n_params), grads, n_params, loss_sum, inv_batch,
                     (float*)nullptr, (float*)nullptr, (float*)nullptr, 0.0, 0.0, 0.0, 0.0, (const int64_t*)nullptr,
                     (uint64_t*)nullptr);
  return msgm_check_launch();
}

int msgm_mlp_ssm_reduce_adam(int32_t d, int32_t premodule, const void* workspace, int32_t n_slabs, float inv_batch,
                             float* grads, float* loss_sum, float* params, float* m, float* v, double lr, double beta1,
                             double beta2, double eps, const int64_t* step_dev, uint64_t* rng_advance,
                             msgm_stream_t stream) {
  if (!workspace || !params || !m || !v || !step_dev || n_slabs < 1 || n_slabs > MLP_MAX_GRID) return MSGM_E_BADARG;
  const int64_t n_params = msgm_mlp_num_params(d, premodule);
  hipLaunchKernelGGL(k_slab_reduce<true>, dim3((unsigned)((n_params + 1 + 63) / 64)), dim3(256), 0, S(stream),
                     reinterpret_cast<const float*>(workspace), n_slabs, slab_stride(n_params), grads, n_params, loss_sum, inv_batch,
                     params, m, v, lr, beta1, beta2, eps, step_dev, rng_advance);
  return msgm_check_launch();
}

int msgm_mlp_ssm_grad(const msgm_mlp_params_t* P, const float* y, const float* t, const float* v, const float* u,
                      const float* cst, int64_t B, const msgm_sde_t* sde, float inv_batch, float* grads, float* loss_per,
                      float* loss_sum, void* workspace, size_t workspace_bytes, msgm_stream_t stream) {
  return msgm_mlp_ssm_grad_w(P, y, t, v, u, cst, B, sde, inv_batch, nullptr, grads, loss_per, loss_sum, workspace, workspace_bytes, stream);
}

int msgm_mlp_ssm_grad_w(const msgm_mlp_params_t* P, const float* y, const float* t, const float* v, const float* u,
                        const float* cst, int64_t B, const msgm_sde_t* sde, float inv_batch, const float* row_w,
                        float* grads, float* loss_per, float* loss_sum, void* workspace, size_t workspace_bytes,
                        msgm_stream_t stream) {
  if (!grads) return MSGM_E_BADARG;
  int32_t n_slabs = 0;
  int rc = msgm_mlp_ssm_partial_w(P, y, t, v, u, cst, B, sde, inv_batch, row_w, loss_per, workspace, workspace_bytes, &n_slabs, stream);
  if (rc) return rc;
  return msgm_mlp_ssm_reduce(P->d, P->premodule, workspace, n_slabs, inv_batch, grads, loss_sum, stream);
}

#ifdef MLP_STAMPS
int msgm_debug_stamps(unsigned long long* out_host) {
  return hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 12) == hipSuccess ? 0 : -4;
}
#endif

}  // extern "C"
