// attention_small_kernels.hip — self-attention at T = 16 tokens (the 4x4 level of the 16x16 U-Net; AttentionBlock /
// QKVAttention, model/unet.py:220-250): sampler forward, dual-number forward and dual-number backward, ONE launch each.
//
// At 16 tokens a (sample, head) pair's whole logit matrix is one 16x16 MFMA tile, so nothing here is "flash": no online
// softmax, no key-block slabs, no reduce kernel, no statistics handed from the forward to the backward and no workspace.
// A workgroup owns one pair.  Every wave of it forms the pair's 16x16 quantities in registers (the same instructions on the
// same operands in each wave, so the same bits) and the waves then share out the independent 16-channel output tiles.
//
// Layout of a 16x16 quantity X[t][s] (query t, key s) in a wave, "query-major": lane (g = lane / 16, t = lane % 16) holds
// X[t][4g + r] in element r of an f32x4.  It is what v_mfma_f32_16x16x4_f32 leaves for the transposed product X^T = A B^T
// with A = the key-side rows and B = the query-side rows, both read from global memory as float4 (lane (g, row) takes the
// channels 16 i + 4 g .. + 3, i = 0 .. D/16 - 1: the contraction order is free as long as A and B agree).  A lane owns one
// query, so max / sum / rbar / c / delta are per-lane scalars after two shuffles (quad_max / quad_sum).  Element r of such a
// fragment IS the B operand of the products that contract over keys (o = P v, qbar = Sbar k, ...), with A = the source rows
// 4g + r; the products that contract over queries (kbar, vbar, ...) want the "key-major" fragment, lane (g, s) holding
// X[4g + r][s], which one pass through a padded 1 KB LDS tile provides.  Both kinds then run the same small_tiles().
//
// expf and a true division, not the hardware approximations: the backward multiplies P by differences that cancel.
#include "attention_common.h"

namespace {

constexpr int TS = 16;                     // tokens
constexpr int LP = 17;                     // padded row of an LDS tile

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ float sum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// small_softmax: query-major S (and Sd when DUAL) of one pair from the q / k rows -> P, Pd and rbar.
// q, k: the lane's row (lane % 16) at its first channel 4g; hq: offset of the tangent rows.
template <int D, bool DUAL>
__device__ __forceinline__ void small_softmax(const float* q, const float* k, size_t hq, float scale, f32x4& P, f32x4& Sd, f32x4& Pd,
                                              float& rbar) {
  f32x4 S = {0.f, 0.f, 0.f, 0.f};
  Sd = S;
#pragma unroll
  for (int i = 0; i < D / 16; ++i) {
    const f32x4 q4 = ld4(q + 16 * i), k4 = ld4(k + 16 * i);
    f32x4 qd4 = q4, kd4 = k4;
    if constexpr (DUAL) { qd4 = ld4(q + hq + 16 * i); kd4 = ld4(k + hq + 16 * i); }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      S = mfma16(k4[e], q4[e], S);
      if constexpr (DUAL) { Sd = mfma16(kd4[e], q4[e], Sd); Sd = mfma16(k4[e], qd4[e], Sd); }
    }
  }
  S *= scale;
  const float m = quad_max(fmaxf(fmaxf(S[0], S[1]), fmaxf(S[2], S[3])));
  f32x4 ex;
#pragma unroll
  for (int r = 0; r < 4; ++r) ex[r] = expf(S[r] - m);
  const float l = quad_sum(sum4(ex));
#pragma unroll
  for (int r = 0; r < 4; ++r) P[r] = ex[r] / l;
  if constexpr (DUAL) {
    Sd *= scale;
    rbar = quad_sum(sum4(P * Sd));
#pragma unroll
    for (int r = 0; r < 4; ++r) Pd[r] = P[r] * (Sd[r] - rbar);
  }
}

// small_tiles: the 16-channel output tiles of one product pair, wave wv of NW taking every NW-th:
//   out2[row][c] = alpha sum_j Xc[row][j] A[j][c]          out1[row][c] = alpha sum_j (Xa[row][j] A[j][c] + Xb[row][j] B[j][c])
// (out1 only when TWO).  X*: fragments whose lane (g, row) holds X[row][4g + r]; A, B: source rows j of stride LDs; outputs
// of row stride LDo.  Each lane writes the channels 4g .. 4g + 3 of its row with one 16-byte store, every element once.
template <int D, int NW, bool TWO>
__device__ __forceinline__ void small_tiles(float* out1, float* out2, int LDo, const float* A, const float* B, int LDs, f32x4 Xa,
                                            f32x4 Xb, f32x4 Xc, float alpha, int wv, int r16, int g) {
#pragma unroll
  for (int ct = wv; ct < D / 16; ct += NW) {
    const size_t src = (size_t)(4 * g) * LDs + 16 * ct + r16, dst = (size_t)r16 * LDo + 16 * ct + 4 * g;
    f32x4 acc1 = {0.f, 0.f, 0.f, 0.f}, acc2 = acc1;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float a = A[src + (size_t)r * LDs];
      acc2 = mfma16(a, Xc[r], acc2);
      if constexpr (TWO) {
        acc1 = mfma16(a, Xa[r], acc1);
        acc1 = mfma16(B[src + (size_t)r * LDs], Xb[r], acc1);
      }
    }
    *reinterpret_cast<f32x4*>(out2 + dst) = acc2 * alpha;
    if constexpr (TWO) *reinterpret_cast<f32x4*>(out1 + dst) = acc1 * alpha;
  }
}

// query-major fragment -> key-major fragment through one padded LDS tile of the wave
__device__ __forceinline__ void small_put(float* tile, f32x4 X, int r16, int g) {
#pragma unroll
  for (int r = 0; r < 4; ++r) tile[r16 * LP + 4 * g + r] = X[r];
}
__device__ __forceinline__ f32x4 small_get(const float* tile, int r16, int g) {
  f32x4 X;
#pragma unroll
  for (int r = 0; r < 4; ++r) X[r] = tile[(4 * g + r) * LP + r16];
  return X;
}

// forward of one pair per workgroup: out = o (and od hq / ha floats further on when DUAL)
template <int D, int NW, bool DUAL>
__global__ void __launch_bounds__(64 * NW) k_attn_small_fwd(const float* __restrict__ qkv, float* __restrict__ att, int nh, size_t hq,
                                                            size_t ha, float scale) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const AttnHead h = attn_head<true, D>((int)blockIdx.x, nh);
  const float* q = qkv + (size_t)h.smp * TS * h.LD + h.qcol;
  float* o = att + (size_t)h.smp * TS * h.LA + h.acol;
  f32x4 P, Sd, Pd = {0.f, 0.f, 0.f, 0.f};
  float rbar = 0.f;
  small_softmax<D, DUAL>(q + (size_t)r16 * h.LD + 4 * g, q + D + (size_t)r16 * h.LD + 4 * g, hq, scale, P, Sd, Pd, rbar);
  const float* v = q + 2 * D;
  small_tiles<D, NW, DUAL>(o + ha, o, h.LA, v, v + hq, h.LD, Pd, P, P, 1.f, wv, r16, g);      // od = Pd v + P vd | o = P v
}

// backward of one pair per workgroup: all of DESIGN 4c's adjoints, written straight into dqkv.  c and delta are taken from
// the tile (c_t = sum_s P D, delta_t = sum_s P (Pbar + D (Sd - rbar) - c Sd): the softmax Jacobian as written), so neither
// the forward's output nor any statistics of it are read.
template <int D, int NW>
__global__ void __launch_bounds__(64 * NW) k_attn_small_bwd(const float* __restrict__ qkv, const float* __restrict__ datt,
                                                            float* __restrict__ dqkv, int nh, size_t hq, size_t ha, float scale) {
  __shared__ float lds[NW][4][TS * LP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
  const AttnHead h = attn_head<true, D>((int)blockIdx.x, nh);
  const size_t qo = (size_t)h.smp * TS * h.LD + h.qcol;
  const float *q = qkv + qo, *k = q + D, *v = q + 2 * D;
  const float* go = datt + (size_t)h.smp * TS * h.LA + h.acol;             // g = obar, gd = odbar ha further on
  float *dq = dqkv + qo, *dk = dq + D, *dv = dq + 2 * D;
  f32x4 P, Sd, Pd;
  float rbar;
  small_softmax<D, true>(q + (size_t)r16 * h.LD + 4 * g, k + (size_t)r16 * h.LD + 4 * g, hq, scale, P, Sd, Pd, rbar);
  // Pbar = g v^T + gd vd^T, Dm = gd v^T, query-major like S: A = the v rows, B = the cotangent rows
  f32x4 Pb = {0.f, 0.f, 0.f, 0.f}, Dm = Pb;
  {
    const float* vr = v + (size_t)r16 * h.LD + 4 * g;
    const float* gr = go + (size_t)r16 * h.LA + 4 * g;
#pragma unroll
    for (int i = 0; i < D / 16; ++i) {
      const f32x4 v4 = ld4(vr + 16 * i), vd4 = ld4(vr + hq + 16 * i), g4 = ld4(gr + 16 * i), gd4 = ld4(gr + ha + 16 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        Pb = mfma16(v4[e], g4[e], Pb);
        Pb = mfma16(vd4[e], gd4[e], Pb);
        Dm = mfma16(v4[e], gd4[e], Dm);
      }
    }
  }
  const float c = quad_sum(sum4(P * Dm));
  f32x4 u, Sb, Sdb;
#pragma unroll
  for (int r = 0; r < 4; ++r) u[r] = Pb[r] + Dm[r] * (Sd[r] - rbar) - c * Sd[r];
  const float delta = quad_sum(sum4(P * u));
#pragma unroll
  for (int r = 0; r < 4; ++r) { Sb[r] = P[r] * (u[r] - delta); Sdb[r] = P[r] * (Dm[r] - c); }
  small_put(lds[wv][0], Sb, r16, g);
  small_put(lds[wv][1], Sdb, r16, g);
  small_put(lds[wv][2], P, r16, g);
  small_put(lds[wv][3], Pd, r16, g);
  // qbar = s2 (Sbar k + Sdbar kd) | qdbar = s2 Sdbar k
  small_tiles<D, NW, true>(dq, dq + hq, h.LD, k, k + hq, h.LD, Sb, Sdb, Sdb, scale, wv, r16, g);
  __syncthreads();
  const f32x4 SbT = small_get(lds[wv][0], r16, g), SdbT = small_get(lds[wv][1], r16, g);
  const f32x4 PT = small_get(lds[wv][2], r16, g), PdT = small_get(lds[wv][3], r16, g);
  // kbar = s2 (Sbar^T q + Sdbar^T qd) | kdbar = s2 Sdbar^T q
  small_tiles<D, NW, true>(dk, dk + hq, h.LD, q, q + hq, h.LD, SbT, SdbT, SdbT, scale, wv, r16, g);
  // vbar = Pd^T gd + P^T g | vdbar = P^T gd
  small_tiles<D, NW, true>(dv, dv + hq, h.LD, go + ha, go, h.LA, PdT, PT, PT, 1.f, wv, r16, g);
}

// shapes: exactly 16 tokens, D = C / heads in {16, 32, 64, 128}
bool attn_small_ok(int32_t T, int32_t heads, int32_t D) {
  return T == TS && heads >= 1 && heads <= 64 && (D == 16 || D == 32 || D == 64 || D == 128);
}
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// D -> <D, NW>: one wave per 16-channel tile, four at the most
template <bool DUAL>
int launch_small_fwd(const float* qkv, float* att, int64_t n, int nh, int D, float scale, hipStream_t st) {
  const size_t hq = (size_t)n * TS * 3 * D * nh, ha = (size_t)n * TS * D * nh;    // tangent halves (unused without DUAL)
  const dim3 grid((unsigned)(n * nh));
#define GO(D_, NW_) hipLaunchKernelGGL((k_attn_small_fwd<D_, NW_, DUAL>), grid, dim3(64 * NW_), 0, st, qkv, att, nh, hq, ha, scale)
  if (D == 128) GO(128, 4);
  else if (D == 64) GO(64, 4);
  else if (D == 32) GO(32, 2);
  else GO(16, 1);
#undef GO
  return msgm_check_launch();
}

int launch_small_bwd(const float* qkv, const float* datt, float* dqkv, int64_t n, int nh, int D, float scale, hipStream_t st) {
  const size_t hq = (size_t)n * TS * 3 * D * nh, ha = (size_t)n * TS * D * nh;
  const dim3 grid((unsigned)(n * nh));
#define GO(D_, NW_) hipLaunchKernelGGL((k_attn_small_bwd<D_, NW_>), grid, dim3(64 * NW_), 0, st, qkv, datt, dqkv, nh, hq, ha, scale)
  if (D == 128) GO(128, 4);
  else if (D == 64) GO(64, 4);
  else if (D == 32) GO(32, 2);
  else GO(16, 1);
#undef GO
  return msgm_check_launch();
}

}  // namespace

extern "C" {

int msgm_attention_small_supported(int32_t T, int32_t heads, int32_t D) { return attn_small_ok(T, heads, D); }

int msgm_attention_small_forward(const float* qkv, float* out, int64_t N, int32_t T, int32_t heads, int32_t D, float scale,
                                 msgm_stream_t stream) {
  if (!qkv || !out || N <= 0 || T <= 0 || heads <= 0 || D <= 0 || !aligned16(qkv) || !aligned16(out)) return MSGM_E_BADARG;
  if (!attn_small_ok(T, heads, D) || N * heads > 0x7fffffffLL) return MSGM_E_UNSUPPORTED;
  return launch_small_fwd<false>(qkv, out, N, heads, D, scale, S(stream));
}

int msgm_attention_small_dual_forward(const float* qkv, float* att, int64_t Bp, int32_t T, int32_t heads, int32_t D, float scale,
                                      msgm_stream_t stream) {
  if (!qkv || !att || Bp <= 0 || T <= 0 || heads <= 0 || D <= 0 || !aligned16(qkv) || !aligned16(att)) return MSGM_E_BADARG;
  if (!attn_small_ok(T, heads, D) || Bp * heads > 0x7fffffffLL) return MSGM_E_UNSUPPORTED;
  return launch_small_fwd<true>(qkv, att, Bp, heads, D, scale, S(stream));
}

int msgm_attention_small_dual_backward(const float* qkv, const float* datt, float* dqkv, int64_t Bp, int32_t T, int32_t heads,
                                       int32_t D, float scale, msgm_stream_t stream) {
  if (!qkv || !datt || !dqkv || Bp <= 0 || T <= 0 || heads <= 0 || D <= 0 || !aligned16(qkv) || !aligned16(datt) || !aligned16(dqkv))
    return MSGM_E_BADARG;
  if (!attn_small_ok(T, heads, D) || Bp * heads > 0x7fffffffLL) return MSGM_E_UNSUPPORTED;
  return launch_small_bwd(qkv, datt, dqkv, Bp, heads, D, scale, S(stream));
}

}  // extern "C"
