// data_kernels.hip — the data stage of a training step on the device: a fresh minibatch per replay
// instead of the reference loop's host-side `x = sampler.sample(batch_size).to(device)` (MSGM_higherDim.py:806).
//   msgm_data_gather       x[b,:] = data[idx_b,:], idx_b drawn with replacement (data.py:691-697)
//   msgm_ssm_prep_gather   msgm_data_gather + msgm_ssm_prep in one launch (the additive SDE's prologue)
//   msgm_data_gather_epoch x[b,:] = data[pi_e(p),:], epochs WITHOUT replacement from a device cursor; msgm_counter_add moves it
//   msgm_data_synth        SwissRoll / Gaussian / Cauchy / GaussianCauchy (data.py:702-802)
// gfx950 only.  Streams: RNG_STREAM_DATA by global row, RNG_STREAM_DATA_ELEM by global element, RNG_STREAM_DATA_CALL one
// scalar per call, RNG_STREAM_DATA_PERM the keys of an epoch's permutation (common.h).  No atomics; every output element
// is written by exactly one lane.
#include "common.h"
#include "sde_stage.h"
#include "optim_elem.h"          // ld4 / st4 / aligned16

__device__ __forceinline__ uint32_t philox_word(const Philox4& p, uint64_t e) {
  const int k = (int)(e & 3);
  return k == 0 ? p.x : k == 1 ? p.y : k == 2 ? p.z : p.w;
}

// ============================================================ the index rule
// Row b of the batch reads table row idx = (uint64(word) * N) >> 32, word = word e & 3 of block e >> 2 of RNG_STREAM_DATA at
// the state's current offset, e = row_base + b: np.random.randint(0, N, size=n) of data.py:692 as an integer map that
// tests/philox_np.py restates exactly (bias <= N 2^-32 per bin).  An injected index is clamped into [0, N): a bad value
// must not become a read outside the table.
__device__ __forceinline__ int64_t data_row_index(const uint64_t* __restrict__ rng, int64_t b, int64_t N,
                                                  const int32_t* __restrict__ idx_in) {
  if (idx_in) {
    const int64_t i = idx_in[b];
    return i < 0 ? 0 : (i >= N ? N - 1 : i);
  }
  const uint64_t e = rng[2] + (uint64_t)b;
  const Philox4 p = msgm_philox(rng, 0, RNG_STREAM_DATA, e >> 2);
  return (int64_t)(((uint64_t)philox_word(p, e) * (uint64_t)N) >> 32);
}

// One lane per UNIT of the flat (B, d) batch — a 16-byte quad (VEC = 4: d % 4 == 0, 16-byte aligned table and batch) or a
// dword (VEC = 1: short or unaligned rows).  Consecutive lanes take consecutive units, so a wave sweeps min(row, 1 KiB)
// contiguous bytes of one table row and moves on to the next batch row only where a row ends: 64 lanes meet 64 rows only
// when a row IS one unit.  Every lane forms its own row's index (one Philox block, ~100 integer operations per 16 bytes
// moved at worst: below the memory time at every shape, and the same rule the prologue kernels follow for a row's time).
template <int VEC>
__global__ void __launch_bounds__(256) k_data_gather(const float* __restrict__ data, int64_t N, float* __restrict__ x, int64_t B,
                                                     int64_t d, const int32_t* __restrict__ idx_in, int32_t* __restrict__ idx_out,
                                                     const uint64_t* __restrict__ rng) {
  const int64_t upr = d / VEC, n = B * upr;
  int64_t b_prev = -1, idx = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / upr, c = (i - b * upr) * VEC;
    if (b != b_prev) { idx = data_row_index(rng, b, N, idx_in); b_prev = b; }
    if constexpr (VEC == 4) st4(x + b * d + c, ld4(data + idx * d + c));
    else x[b * d + c] = data[idx * d + c];
    if (idx_out && c == 0) idx_out[b] = (int32_t)idx;
  }
}

// ============================================================ the epoch index rule
// Sampling WITHOUT replacement: the data order is one endless stream of independent permutations pi_0, pi_1, ... of
// [0, N); stream position P reads row pi_e(p), e = P / N, p = P % N, so every aligned window of N positions holds every
// row once.  pi_e is a 12-round unbalanced Feistel network on bits = max(8, bit_length(N - 1)) bits (halves a = bits / 2
// and b = bits - a, changing sides every round) with cycle walking: a bijection of [0, 2^bits), re-applied until the
// value is a row.  2^bits < 2 N for N > 128, so the mean number of passes stays below 2.  The twelve round keys are the
// words of blocks 4 e + j, j = 0, 1, 2, of RNG_STREAM_DATA_PERM at offset 0 and with NO shard base: they depend on the
// seed and the epoch only, so every step and every rank of an epoch sees the same permutation.  All uint32 arithmetic;
// tests/data_epoch_ref.py restates it to the bit.
__device__ __forceinline__ uint32_t perm_round(uint32_t r, uint32_t k) {
  uint32_t x = (r + k) * 0x9E3779B1u;
  x ^= x >> 15;
  x *= 0x85EBCA77u;
  x ^= x >> 13;
  x *= 0xC2B2AE3Du;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ int64_t data_epoch_index(const uint64_t* __restrict__ rng, uint64_t P, int64_t N) {
  if (N == 1) return 0;
  const uint64_t e = P / (uint64_t)N;
  const uint32_t n = (uint32_t)N, p = (uint32_t)(P - e * (uint64_t)N);
  const uint64_t seed = rng[0];
  uint32_t k[12];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const uint64_t q = 4 * e + (uint64_t)j;
    const Philox4 w = philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), RNG_STREAM_DATA_PERM, 0u, (uint32_t)seed,
                                    (uint32_t)(seed >> 32));
    k[4 * j] = w.x; k[4 * j + 1] = w.y; k[4 * j + 2] = w.z; k[4 * j + 3] = w.w;
  }
  const int bits = max(8, 32 - __clz(n - 1)), a = bits >> 1, b = bits - a;        // bits <= 31: N < 2^31
  const uint32_t ma = (1u << a) - 1u, mb = (1u << b) - 1u;
  uint32_t v = p;
  do {
    uint32_t L = v >> b, R = v & mb;                 // L holds a bits, R holds b
#pragma unroll
    for (int i = 0; i < 12; i += 2) {                // two rounds (L, R) <- (R, L ^ F(R)): the widths are back in place
      const uint32_t t = L ^ (perm_round(R, k[i]) & ma);
      const uint32_t u = R ^ (perm_round(t, k[i + 1]) & mb);
      L = t; R = u;
    }
    v = (L << b) | R;
  } while (v >= n);
  return (int64_t)v;
}

// k_data_gather with the row of stream position cursor[0] + row_base + b.  The cursor is only READ here: every lane of
// the launch must see the same value, so the advance is a launch of its own behind this one (msgm_counter_add).
template <int VEC>
__global__ void __launch_bounds__(256) k_data_gather_epoch(const float* __restrict__ data, int64_t N, float* __restrict__ x,
                                                           int64_t B, int64_t d, int32_t* __restrict__ idx_out,
                                                           const uint64_t* __restrict__ rng,
                                                           const int64_t* __restrict__ cursor) {
  const int64_t upr = d / VEC, n = B * upr;
  const uint64_t P0 = (uint64_t)cursor[0] + rng[2];
  int64_t b_prev = -1, idx = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / upr, c = (i - b * upr) * VEC;
    if (b != b_prev) { idx = data_epoch_index(rng, P0 + (uint64_t)b, N); b_prev = b; }
    if constexpr (VEC == 4) st4(x + b * d + c, ld4(data + idx * d + c));
    else x[b * d + c] = data[idx * d + c];
    if (idx_out && c == 0) idx_out[b] = (int32_t)idx;
  }
}

__global__ void k_counter_add(int64_t* c, int64_t delta) { c[0] += delta; }

// msgm_data_gather + k_ssm_prep (sde_kernels.hip) in one launch: the quad walk of k_ssm_prep with x0[e] read through the
// row's index and the gathered value written to x as well.  Same streams, same indices, vp_row / vp_value: the bits of the
// two launches from the same stream state.  VEC: d % 4 == 0 and 16-byte aligned operands — a quad lies in one row and
// moves as 16 bytes.
template <bool VEC>
__global__ void __launch_bounds__(256) k_ssm_prep_gather(const float* __restrict__ data, int64_t N, float* __restrict__ x,
                                                         float* __restrict__ y, float* __restrict__ t_out, float* __restrict__ v,
                                                         int64_t B, int64_t d, float b0, float b1, float T, float t_eps,
                                                         const uint64_t* __restrict__ rng, int64_t* step_ctr) {
  const VpSde P = {b0, b1, T, t_eps};
  const int64_t n = B * d;
  const int64_t nq = (n + 3) >> 2;
  if (step_ctr && blockIdx.x == 0 && threadIdx.x == 0) step_ctr[0] += 1;
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = q << 2;
    const f32x4 ez = philox_normal4(rng, 0, RNG_STREAM_EPS, q);
    const f32x4 uv = philox_uniform4(rng, 0, RNG_STREAM_V, q);
    if constexpr (VEC) {
      const int64_t b = e0 / d;
      const VpRow r = vp_row(P, b, rng, nullptr, nullptr);
      const f32x4 xq = ld4(data + data_row_index(rng, b, N, nullptr) * d + (e0 - b * d));
      f32x4 yq, vq;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        yq[k] = vp_value(r, ez[k], xq[k]);
        vq[k] = (uv[k] >= 0.5f) ? 1.0f : -1.0f;
      }
      st4(x + e0, xq); st4(y + e0, yq); st4(v + e0, vq);
      if (e0 - b * d == 0) t_out[b] = r.t;
    } else {
      int64_t b_prev = -1, src = 0;
      VpRow r = {0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int64_t e = e0 + k;
        if (e >= n) break;
        const int64_t b = e / d;
        if (b != b_prev) {                                                          // once per row the quad touches
          r = vp_row(P, b, rng, nullptr, nullptr);
          src = (data_row_index(rng, b, N, nullptr) - b) * d;                       // data[idx d + (e - b d)] = data[src + e]
          b_prev = b;
        }
        const float xe = data[src + e];
        x[e] = xe;
        y[e] = vp_value(r, ez[k], xe);
        v[e] = (uv[k] >= 0.5f) ? 1.0f : -1.0f;
        if (e - b * d == 0) t_out[b] = r.t;
      }
    }
  }
}

// ============================================================ synthetic samplers
// Standard Cauchy from the 24-bit integer k of a draw (k = word >> 8, or (int)(u 2^24) of an injected uniform): the quantile
// tan(pi (u - 1/2)) = -cot(pi u) folded onto (0, 1/2): m = min(k, 2^24 - 1 - k), w = (m + 1/2) 2^-24 (exact in fp32),
// cot(pi w) with the sign of the half k lies in.  Finite for every k (|c| <= cot(pi 2^-25) ~ 1.07e7), relative accuracy in
// both tails and at the centre (sincospif reduces its argument exactly), and k and 2^24 - 1 - k give exact negatives.  The
// direct form loses all relative accuracy near the poles and is infinite at u = 0.
__device__ __forceinline__ float cauchy_from_k(uint32_t k) {
  const uint32_t m = min(k, 0xFFFFFFu - k);
  const float w = ((float)m + 0.5f) * (1.0f / 16777216.0f);
  float s, c;
  sincospif(w, &s, &c);
  const float q = c / s;
  return k < 0x800000u ? -q : q;
}
__device__ __forceinline__ float cauchy_from_u(float u) {
  int k = (int)(u * 16777216.0f);
  k = k < 0 ? 0 : (k > 0xFFFFFF ? 0xFFFFFF : k);
  return cauchy_from_k((uint32_t)k);
}
__device__ __forceinline__ f32x4 block_cauchy(const Philox4& p) {
  return f32x4{cauchy_from_k(p.x >> 8), cauchy_from_k(p.y >> 8), cauchy_from_k(p.z >> 8), cauchy_from_k(p.w >> 8)};
}
__device__ __forceinline__ f32x4 block_normal(const Philox4& p) {
  f32x4 r;
  float a, b, c, d;
  box_muller(p.x, p.y, a, b);
  box_muller(p.z, p.w, c, d);
  r[0] = a; r[1] = b; r[2] = c; r[3] = d;
  return r;
}
// GaussianCauchy's one Cauchy(0, 1) scalar per call (data.py:799): word 0 of block 0 of RNG_STREAM_DATA_CALL, no shard base —
// every rank of a data-parallel run scales its rows by the same number.
__device__ __forceinline__ float data_call_cauchy(const uint64_t* __restrict__ rng, const float* __restrict__ u) {
  if (u) return cauchy_from_u(u[0]);
  return cauchy_from_k(msgm_philox(rng, 0, RNG_STREAM_DATA_CALL, 0).x >> 8);
}

#define CAUCHY_SCALE 0.02f               /* Cauchy(0, 1/50), data.py:738; the (1.0/50) of data.py:799 */

// A = identity (any d) and the swiss roll: one lane per element-quad of the flat batch, as k_fill.
template <int KIND>
__global__ void __launch_bounds__(256) k_data_synth_flat(float* __restrict__ x, int64_t B, int64_t d, float noise,
                                                         const float* __restrict__ u, const float* __restrict__ z,
                                                         const uint64_t* __restrict__ rng) {
  const int64_t n = B * d;
  const int64_t nq = (n + 3) >> 2;
  float s_call = 1.0f;
  if constexpr (KIND == MSGM_DATA_GAUSSIAN_CAUCHY) s_call = data_call_cauchy(rng, u);
  for (int64_t q = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e0 = q << 2;
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if constexpr (KIND == MSGM_DATA_CAUCHY) {
      if (u) {
        for (int k = 0; k < 4 && e0 + k < n; ++k) r[k] = cauchy_from_u(u[e0 + k]);
      } else {
        r = block_cauchy(msgm_philox(rng, 0, RNG_STREAM_DATA_ELEM, (uint64_t)q + (rng[3] >> 2)));
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = CAUCHY_SCALE * r[k];
    } else {
      if (z) {
        for (int k = 0; k < 4 && e0 + k < n; ++k) r[k] = z[e0 + k];
      } else {
        r = philox_normal4(rng, 0, RNG_STREAM_DATA_ELEM, (uint64_t)q);
      }
      if constexpr (KIND == MSGM_DATA_GAUSSIAN_CAUCHY) {
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = (CAUCHY_SCALE * r[k]) * s_call;
      }
      if constexpr (KIND == MSGM_DATA_SWISS) {
        // sklearn's make_swiss_roll, columns [0, 2], / 5 (data.py:713-714): t = 1.5 pi (1 + 2 u).  t reaches 14.2: sincosf.
#pragma unroll
        for (int k = 0; k < 4; k += 2) {
          const int64_t e = e0 + k;
          if (e < n) {                                       // d == 2: a row is elements e, e + 1 of this quad
            const int64_t b = e >> 1;
            const float ub = u ? u[b] : philox_uniform1(rng, 0, RNG_STREAM_DATA, (uint64_t)b);
            const float t = 4.71238898038469f * (1.0f + 2.0f * ub);
            float sn, cs;
            sincosf(t, &sn, &cs);
            r[k] = (t * cs + noise * r[k]) / 5.0f;
            r[k + 1] = (t * sn + noise * r[k + 1]) / 5.0f;
          }
        }
      }
    }
    if (e0 + 3 < n && aligned16(x)) {
      st4(x + e0, r);
    } else {
      for (int k = 0; k < 4 && e0 + k < n; ++k) x[e0 + k] = r[k];
    }
  }
}

// x = draws A^T for a dense A, d <= 128 (the MLP's range).  A workgroup keeps A transposed in LDS (At[j][i], odd pitch:
// the transposing fill and the reads — consecutive lanes, consecutive i — are both conflict-free) and takes tiles of R rows:
// the tile's R d draws are one contiguous range of the element-indexed stream, drawn by quads into LDS, then lane (r, i)
// forms sum_j draw[r][j] A[i][j] in fp64 (d <= 128 terms: no slower than the draws) and rounds it to fp32 once — a heavy
// Cauchy tail puts one huge term next to ordinary ones, and the value must not depend on the order they are added in.
template <int KIND>
__global__ void __launch_bounds__(256) k_data_synth_rows(float* __restrict__ x, int64_t B, int d, int R,
                                                         const float* __restrict__ A, const float* __restrict__ u,
                                                         const float* __restrict__ z, const uint64_t* __restrict__ rng) {
  extern __shared__ __attribute__((aligned(16))) float ds_lds[];
  const int dp = d | 1;
  float* At = ds_lds;                      // d x dp
  float* zr = ds_lds + d * dp;             // R x d
  const int tid = threadIdx.x;
  for (int f = tid; f < d * d; f += 256) {
    const int i = f / d, j = f - i * d;
    At[j * dp + i] = A[f];
  }
  float s_call = 1.0f;
  if constexpr (KIND == MSGM_DATA_GAUSSIAN_CAUCHY) s_call = data_call_cauchy(rng, u);
  const float* inj = (KIND == MSGM_DATA_CAUCHY) ? u : z;
  const int64_t tiles = (B + R - 1) / R;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    __syncthreads();                       // At is filled (first trip); the previous tile's draws have been read
    const int64_t b0 = tile * R;
    const int rows = (int)((B - b0 < R) ? (B - b0) : R), cnt = rows * d;
    if (inj) {
      for (int o = tid; o < cnt; o += 256) {
        const float w = inj[b0 * d + o];
        zr[o] = (KIND == MSGM_DATA_CAUCHY) ? CAUCHY_SCALE * cauchy_from_u(w) : w;
      }
    } else {
      const uint64_t g0 = rng[3] + (uint64_t)b0 * (uint64_t)d;          // global element of the tile's first draw
      const uint64_t q1 = (g0 + (uint64_t)cnt - 1) >> 2;
      for (uint64_t q = (g0 >> 2) + (uint64_t)tid; q <= q1; q += 256) {
        const Philox4 p = msgm_philox(rng, 0, RNG_STREAM_DATA_ELEM, q);
        f32x4 r;
        if constexpr (KIND == MSGM_DATA_CAUCHY) {
          r = block_cauchy(p);
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = CAUCHY_SCALE * r[k];
        } else {
          r = block_normal(p);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int64_t o = (int64_t)((q << 2) + (uint64_t)k) - (int64_t)g0;
          if (o >= 0 && o < cnt) zr[o] = r[k];
        }
      }
    }
    __syncthreads();
    for (int o = tid; o < cnt; o += 256) {
      const int r = o / d, i = o - r * d;
      const float* zrow = zr + r * d;
      double a0 = 0.0, a1 = 0.0;                    // fp64 sums: products exact, the row's value rounded to fp32 once
      int j = 0;
      for (; j + 1 < d; j += 2) {
        a0 = fma((double)zrow[j], (double)At[j * dp + i], a0);
        a1 = fma((double)zrow[j + 1], (double)At[(j + 1) * dp + i], a1);
      }
      if (j < d) a0 = fma((double)zrow[j], (double)At[j * dp + i], a0);
      float acc = (float)(a0 + a1);
      if constexpr (KIND == MSGM_DATA_GAUSSIAN_CAUCHY) acc = (CAUCHY_SCALE * acc) * s_call;
      x[(b0 + r) * d + i] = acc;
    }
  }
}

static int synth_rows_tile(int64_t d) { return d >= 32 ? 8 : (int)(256 / d); }

template <int KIND>
static int launch_synth_rows(float* x, int64_t B, int64_t d, const float* A, const float* u, const float* z, const uint64_t* rng,
                             msgm_stream_t stream) {
  const int R = synth_rows_tile(d);
  const size_t lds = (size_t)(d * (d | 1) + R * d) * sizeof(float);          // 70 144 B at d = 128: above the 64 KiB default
  static bool raised = false;
  if (!raised) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_data_synth_rows<KIND>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              72 * 1024);
    raised = true;
  }
  hipLaunchKernelGGL(k_data_synth_rows<KIND>, dim3(grid_for((B + R - 1) / R, 1, 512)), dim3(256), lds, S(stream), x, B, (int)d, R,
                     A, u, z, rng);
  return msgm_check_launch();
}

template <int KIND>
static int launch_synth_flat(float* x, int64_t B, int64_t d, float noise, const float* u, const float* z, const uint64_t* rng,
                             msgm_stream_t stream) {
  hipLaunchKernelGGL(k_data_synth_flat<KIND>, dim3(grid_for((B * d + 3) / 4, 256)), dim3(256), 0, S(stream), x, B, d, noise, u, z,
                     rng);
  return msgm_check_launch();
}

extern "C" {

int msgm_data_gather(const float* data, int64_t N, float* x, int64_t B, int64_t d, const int32_t* idx_in, int32_t* idx_out,
                     const uint64_t* rng, msgm_stream_t stream) {
  if (!data || !x || B <= 0 || d <= 0 || N <= 0 || (!idx_in && !rng)) return MSGM_E_BADARG;
  if (N >= ((int64_t)1 << 31)) return MSGM_E_UNSUPPORTED;                   // the index is an int32
  if (d % 4 == 0 && aligned16(data, x)) {
    hipLaunchKernelGGL(k_data_gather<4>, dim3(grid_for(B * (d / 4), 256)), dim3(256), 0, S(stream), data, N, x, B, d, idx_in,
                       idx_out, rng);
  } else {
    hipLaunchKernelGGL(k_data_gather<1>, dim3(grid_for(B * d, 256)), dim3(256), 0, S(stream), data, N, x, B, d, idx_in, idx_out,
                       rng);
  }
  return msgm_check_launch();
}

int msgm_data_gather_epoch(const float* data, int64_t N, float* x, int64_t B, int64_t d, int32_t* idx_out, const uint64_t* rng,
                           const int64_t* cursor, msgm_stream_t stream) {
  if (!data || !x || !rng || !cursor || B <= 0 || d <= 0 || N <= 0) return MSGM_E_BADARG;
  if (N >= ((int64_t)1 << 31)) return MSGM_E_UNSUPPORTED;                   // the index is an int32, the network uint32
  if (d % 4 == 0 && aligned16(data, x)) {
    hipLaunchKernelGGL(k_data_gather_epoch<4>, dim3(grid_for(B * (d / 4), 256)), dim3(256), 0, S(stream), data, N, x, B, d,
                       idx_out, rng, cursor);
  } else {
    hipLaunchKernelGGL(k_data_gather_epoch<1>, dim3(grid_for(B * d, 256)), dim3(256), 0, S(stream), data, N, x, B, d, idx_out,
                       rng, cursor);
  }
  return msgm_check_launch();
}

int msgm_counter_add(int64_t* ctr, int64_t delta, msgm_stream_t stream) {
  if (!ctr) return MSGM_E_BADARG;
  hipLaunchKernelGGL(k_counter_add, dim3(1), dim3(1), 0, S(stream), ctr, delta);
  return msgm_check_launch();
}

int msgm_ssm_prep_gather(const float* data, int64_t N, float* x, float* y, float* t_out, float* v, int64_t B, int64_t d,
                         const msgm_sde_t* sde, const uint64_t* rng, int64_t* step_ctr, msgm_stream_t stream) {
  if (!data || !x || !y || !t_out || !v || !sde || !rng || B <= 0 || d <= 0 || N <= 0) return MSGM_E_BADARG;
  if (sde->kind != MSGM_SDE_SGM || N >= ((int64_t)1 << 31)) return MSGM_E_UNSUPPORTED;
  const dim3 grid(grid_for((B * d + 3) / 4, 256));
  if (d % 4 == 0 && aligned16(data, x, y, v)) {
    hipLaunchKernelGGL(k_ssm_prep_gather<true>, grid, dim3(256), 0, S(stream), data, N, x, y, t_out, v, B, d, sde->beta_min,
                       sde->beta_max, sde->T, sde->t_epsilon, rng, step_ctr);
  } else {
    hipLaunchKernelGGL(k_ssm_prep_gather<false>, grid, dim3(256), 0, S(stream), data, N, x, y, t_out, v, B, d, sde->beta_min,
                       sde->beta_max, sde->T, sde->t_epsilon, rng, step_ctr);
  }
  return msgm_check_launch();
}

int msgm_data_synth(int32_t kind, float* x, int64_t B, int64_t d, const float* A, float noise, const float* u, const float* z,
                    const uint64_t* rng, msgm_stream_t stream) {
  if (!x || B <= 0 || d <= 0) return MSGM_E_BADARG;
  bool philox;                                                             // does the call draw anything itself?
  switch (kind) {
    case MSGM_DATA_SWISS: philox = !u || !z; break;
    case MSGM_DATA_GAUSSIAN: philox = !z; break;
    case MSGM_DATA_CAUCHY: philox = !u; break;
    case MSGM_DATA_GAUSSIAN_CAUCHY: philox = !u || !z; break;
    default: return MSGM_E_BADARG;
  }
  if (philox && !rng) return MSGM_E_BADARG;
  if (kind == MSGM_DATA_SWISS) {
    if (d != 2 || A) return MSGM_E_BADARG;
    return launch_synth_flat<MSGM_DATA_SWISS>(x, B, d, noise, u, z, rng, stream);
  }
  if (A && d > 128) return MSGM_E_UNSUPPORTED;
  if (kind == MSGM_DATA_GAUSSIAN)
    return A ? launch_synth_rows<MSGM_DATA_GAUSSIAN>(x, B, d, A, u, z, rng, stream)
             : launch_synth_flat<MSGM_DATA_GAUSSIAN>(x, B, d, noise, u, z, rng, stream);
  if (kind == MSGM_DATA_CAUCHY)
    return A ? launch_synth_rows<MSGM_DATA_CAUCHY>(x, B, d, A, u, z, rng, stream)
             : launch_synth_flat<MSGM_DATA_CAUCHY>(x, B, d, noise, u, z, rng, stream);
  return A ? launch_synth_rows<MSGM_DATA_GAUSSIAN_CAUCHY>(x, B, d, A, u, z, rng, stream)
           : launch_synth_flat<MSGM_DATA_GAUSSIAN_CAUCHY>(x, B, d, noise, u, z, rng, stream);
}

}  // extern "C"
