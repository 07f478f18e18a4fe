// attention_kernels.hip — K8b: fused single-head self-attention forward for the SAMPLER path
// (QKVAttention, model/unet.py:236-250: softmax((q ch^-1/4)(k ch^-1/4)^T) v, fp32) without materialising the
// (B,T,T) probabilities.  The training path keeps the three-kernel form (bmm / dual softmax / bmm) because its
// backward needs P and the tangent logits; here there is no tangent and nothing to keep.
//
// Layout: qkv [N][T][3C] channels-last (q | k | v channel slices, as msgm_conv_forward writes them),
// out [N][T][C].  One workgroup = 4 waves = 64*QT queries of one sample; keys/values stream through LDS in blocks
// of 64 (register-prefetched one block ahead).  Everything is computed TRANSPOSED so that the query sits on lane&15:
//   S^T[key][query] = K[key][:] . Q[query][:]      A = K fragment (LDS, b128), B = Q fragment (registers, resident)
//   O^T[c][query]  += V^T[c][key] . P^T[key][query]  A = V fragment (LDS, b32),  B = the S^T accumulator itself
// In the C/D layout of v_mfma_f32_16x16x4_f32 a lane holds 4 consecutive keys of ITS query, so the running max / sum
// of the online softmax are per-lane scalars (+ two xor-shuffles across the four key groups), the rescale of O is a
// per-lane multiply, and exp(S - m) is directly the B operand of the second product (same k-permutation trick as
// the MLP kernel: MFMA step r of key tile kt contracts key 16kt + 4q + r on both operands).
//
// Multi-head (MH, AttentionBlock with num_heads = H, model/unet.py:220-250): qkv.reshape(B*H, 3C/H, T) gives head h the
// qkv channels [3Dh, 3D(h+1)) (q | k | v of D = C/H each), and h.reshape(B, -1, T) puts its output at channels [Dh, D(h+1)).
// The kernel body is the single-head one at channel count D; a workgroup serves one (sample, head) pair, reads rows of
// stride 3C from column 3Dh and writes rows of stride C from column Dh.  MH = false is the single-head build (strides
// compile-time 3C / C, no head index).
#include "attention_common.h"

template <int CT, int QT, bool MH = false>   // C = 16*CT channels (per head); QT tiles of 16 queries per wave
__global__ void __launch_bounds__(256) k_attn_fwd(const float* __restrict__ qkv, float* __restrict__ out, int T, int nqb, float scale,
                                                  int nh) {
  constexpr int C = 16 * CT, KP = C + 4;
  constexpr int NV = (64 * C / 4) / 256;                  // float4 per thread per matrix and key block
  static_assert(NV >= 1 && (64 * C / 4) % 256 == 0, "key block does not divide over the workgroup's threads");
  extern __shared__ __attribute__((aligned(16))) float at_lds[];
  float* Ks = at_lds;
  float* Vs = at_lds + 64 * KP;
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, il = lane & 15, q = lane >> 4;
  const int pr = blockIdx.x / nqb, qb = blockIdx.x - pr * nqb;     // (sample, head) pair, query block of 64*QT
  const AttnHead H = attn_head<MH, C>(pr, nh);
  const float* base = qkv + (size_t)H.smp * T * H.LD + H.qcol;
  const int q0 = (qb * 4 + w) * 16 * QT;                  // first query of this wave

  f32x4 qf[QT][CT], o[QT][CT];
  float m[QT], l[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
    for (int g = 0; g < CT; ++g) {
      qf[qt][g] = *reinterpret_cast<const f32x4*>(base + (size_t)(q0 + 16 * qt + il) * H.LD + 16 * g + 4 * q);
      o[qt][g] = f32x4{0, 0, 0, 0};
    }
    m[qt] = -INFINITY; l[qt] = 0.f;
  }

  f32x4 pk[NV], pv[NV];
  auto gload = [&](int kb) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const AttnSlot s = attn_slot<C, 256>(tid, i);
      const float* p = base + (size_t)(kb * 64 + s.row) * H.LD + 4 * s.c4;
      pk[i] = *reinterpret_cast<const f32x4*>(p + C);
      pv[i] = *reinterpret_cast<const f32x4*>(p + 2 * C);
    }
  };
  gload(0);
  const int nkb = T / 64;
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();                                       // the previous block's readers are done
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const AttnSlot s = attn_slot<C, 256>(tid, i);
      *reinterpret_cast<f32x4*>(Ks + s.row * KP + 4 * s.c4) = pk[i];
      *reinterpret_cast<f32x4*>(Vs + s.row * KP + 4 * s.c4) = pv[i];
    }
    __syncthreads();
    if (kb + 1 < nkb) gload(kb + 1);

    // ---- S^T = K Q^T for the 4 key tiles of the block
    f32x4 s[QT][4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) s[qt][kt] = f32x4{0, 0, 0, 0};
#pragma unroll
      for (int g = 0; g < CT; ++g) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(Ks + (16 * kt + il) * KP + 16 * g + 4 * q);
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) s[qt][kt] = mfma16(a[r], qf[qt][g][r], s[qt][kt]);
      }
    }
    // ---- online softmax: this lane's query, its 16 keys of the block (+ the other three key groups by shuffle)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      float mb = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { s[qt][kt][r] *= scale; mb = fmaxf(mb, s[qt][kt][r]); }
      const float mn = fmaxf(m[qt], quad_max(mb));
      const float alpha = __expf(m[qt] - mn);
      m[qt] = mn;
      float ls = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float p = __expf(s[qt][kt][r] - mn); s[qt][kt][r] = p; ls += p; }
      l[qt] = l[qt] * alpha + ls;                          // per key group; the four groups meet at the end
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) o[qt][ct] *= alpha;
    }
    // ---- O^T += V^T P^T
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        float a[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) a[r] = Vs[(16 * kt + 4 * q + r) * KP + 16 * ct + il];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) o[qt][ct] = mfma16(a[r], s[qt][kt][r], o[qt][ct]);
      }
  }
  // ---- normalise and store: lane (query il, q) holds channels 16ct + 4q + r
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float inv = 1.0f / quad_sum(l[qt]);
    float* orow = out + ((size_t)H.smp * T + q0 + 16 * qt + il) * H.LA + H.acol;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) *reinterpret_cast<f32x4*>(orow + 16 * ct + 4 * q) = o[qt][ct] * inv;
  }
}

template <int CT, int QT, bool MH = false>
static int launch_attn(const float* qkv, float* out, int64_t N, int T, float scale, hipStream_t st, int nh = 1) {
  constexpr int C = 16 * CT;
  constexpr size_t lds = (size_t)2 * 64 * (C + 4) * sizeof(float);
  static const int once = attn_allow_lds(&k_attn_fwd<CT, QT, MH>, lds); (void)once;
  const int nqb = T / (64 * QT);
  hipLaunchKernelGGL((k_attn_fwd<CT, QT, MH>), dim3((unsigned)(N * nh * nqb)), dim3(256), lds, st, qkv, out, T, nqb, scale, nh);
  return msgm_check_launch();
}

// D -> <CT, QT>, once: 128 queries per workgroup when T allows — except at D = 128, where the second query tile costs the second
// resident wave per SIMD (357 registers): 89 vs 102 TFLOP/s at T = 256.  D = 16 is multi-head only.
template <bool MH>
static int attn_fwd_go(const float* qkv, float* out, int64_t N, int T, int D, int nh, float scale, hipStream_t st) {
  const bool two = T % 128 == 0;
  if constexpr (MH)
    if (D == 16) return two ? launch_attn<1, 2, MH>(qkv, out, N, T, scale, st, nh) : launch_attn<1, 1, MH>(qkv, out, N, T, scale, st, nh);
  if (D == 32) return two ? launch_attn<2, 2, MH>(qkv, out, N, T, scale, st, nh) : launch_attn<2, 1, MH>(qkv, out, N, T, scale, st, nh);
  if (D == 64) return two ? launch_attn<4, 2, MH>(qkv, out, N, T, scale, st, nh) : launch_attn<4, 1, MH>(qkv, out, N, T, scale, st, nh);
  if (D == 128) return launch_attn<8, 1, MH>(qkv, out, N, T, scale, st, nh);
  return MSGM_E_UNSUPPORTED;
}

// the shapes the kernels take: D channels per head (16 only through the multi-head entries), T a multiple of 64
static bool attn_shape_ok(int32_t T, int32_t heads, int32_t D, bool mh) {
  return heads >= 1 && heads <= 64 && ((mh && D == 16) || D == 32 || D == 64 || D == 128) && T >= 64 && T % 64 == 0;
}

// both forward entries; one head runs the single-head instantiations through either (same kernels, same bits; D = 16 has none)
static int attn_forward(const float* qkv, float* out, int64_t N, int32_t T, int32_t heads, int32_t D, bool mh, float scale,
                        msgm_stream_t stream) {
  if (!qkv || !out || N <= 0 || T <= 0 || heads <= 0 || D <= 0) return MSGM_E_BADARG;
  if (!attn_shape_ok(T, heads, D, mh) || N * heads * (int64_t)(T / 64) > 0x7fffffffLL) return MSGM_E_UNSUPPORTED;
  if (!mh || (heads == 1 && attn_shape_ok(T, 1, D, false))) return attn_fwd_go<false>(qkv, out, N, T, D, 1, scale, S(stream));
  return attn_fwd_go<true>(qkv, out, N, T, D, heads, scale, S(stream));
}

extern "C" {

int msgm_attention_supported(int32_t T, int32_t C) { return attn_shape_ok(T, 1, C, false); }

int msgm_attention_forward(const float* qkv, float* out, int64_t N, int32_t T, int32_t C, float scale, msgm_stream_t stream) {
  return attn_forward(qkv, out, N, T, 1, C, false, scale, stream);
}

int msgm_attention_mh_supported(int32_t T, int32_t heads, int32_t D) { return attn_shape_ok(T, heads, D, true); }

int msgm_attention_mh_forward(const float* qkv, float* out, int64_t N, int32_t T, int32_t heads, int32_t D, float scale,
                              msgm_stream_t stream) {
  return attn_forward(qkv, out, N, T, heads, D, true, scale, stream);
}

}  // extern "C"
