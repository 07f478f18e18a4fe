// sde_stage.h — the arithmetic of one integrator stage (msgm_sde_stage), shared by the stage kernels of
// sde_kernels.hip and by the stage-update phase of the fused MLP sampler loop (mlp_kernels.hip, MODE_SDE).  One copy
// of each formula; the build keeps -ffp-contract=off, so every kernel that calls one of these gives the same bits.
#pragma once
#include "common.h"

struct StageArgs {
  float* out; const float* base; float c_out;
  const float* x; const float* a; const float* dW; const float* z; float sqrt_delta;
  const uint64_t* rng; uint64_t rng_step; float* dW_out;
  int64_t B; int64_t n;
  int kind, proc, strato;
  float b0, b1, T, t, delta, lmbd;
  const float* G; const float* L_G;
  const float* norm0;
  float* inc_out;              // optional: the bare increment
  const float* delta_rows;     // optional per-row step length (MSGM short-time rows, SDEs.py:112-117)
  float t_frac;                // with delta_rows: t_b = t + t_frac * delta_b
  const float* t_dev;          // optional device scalar overriding t   (graph replay: time lives on the device)
  const int64_t* step_dev;     // optional device scalar overriding rng_step
};

__device__ __forceinline__ uint64_t stage_step(const StageArgs& A) { return A.step_dev ? (uint64_t)A.step_dev[0] : A.rng_step; }
__device__ __forceinline__ float stage_time(const StageArgs& A) { return A.t_dev ? A.t_dev[0] : A.t; }
__device__ __forceinline__ float stage_noise(const StageArgs& A, int64_t e, float sqrt_delta) {
  if (A.dW) return A.dW[e];
  float zz = A.z ? A.z[e] : philox_normal1(A.rng, stage_step(A), RNG_STREAM_DW, (uint64_t)e);
  return sqrt_delta * zz;                                  // delta**0.5 * randn   sde_scheme.py:84
}

// Row b's stage coefficients at the stage time tnow (= stage_time(A): host t or t_dev): step length delta_b and its root
// (per row with delta_rows, then also t_b = tnow + t_frac delta_b), beta at t_b — at T - t_b for the reverse process — and its
// root.  PER_ROW = false is the kernel-uniform form of k_stage_diag_flat, which msgm_sde_stage never sends delta_rows to.
struct StageCoef { float delta, sqd, beta, sb; };
template <bool PER_ROW = true>
__device__ __forceinline__ StageCoef stage_coef(const StageArgs& A, float tnow, int64_t b) {
  const float* dr = PER_ROW ? A.delta_rows : nullptr;
  const float delta = dr ? dr[b] : A.delta;
  const float sqd = dr ? sqrtf(delta) : A.sqrt_delta;
  const float tb = dr ? tnow + A.t_frac * delta : tnow;
  const float s = A.proc == MSGM_PROC_REVERSE ? A.T - tb : tb;
  const float beta = sde_beta(A.b0, A.b1, s);
  return {delta, sqd, beta, sqrtf(beta)};
}
// sigma's factor besides sqrt(beta): sqrt(1-l) for the reverse process (SDEs.py:587-588)
__device__ __forceinline__ float stage_sig_scale(const StageArgs& A) {
  return (A.proc == MSGM_PROC_REVERSE) ? sqrtf(1.0f - A.lmbd) : 1.0f;
}

// The drift of a stage from ga = G a, f, fs (f of the Stratonovich forward form) and div = divSigma.
__device__ __forceinline__ float stage_mu(const StageArgs& A, float ga, float f, float fs, float div) {
  const float l = A.lmbd;
  float mu;
  if (A.proc == MSGM_PROC_REVERSE) {
    mu = (1.0f - 0.5f * l) * ga - f + (1.0f - l) * div;          // SDEs.py:560-561
    if (A.strato) mu = mu - 0.5f * (1.0f - l) * div;             // SDEs.py:583-584
  } else {
    mu = fs;                                                      // SDEs.py:42-43
    if (!A.strato) mu = mu + 0.5f * div;                          // SDEs.py:38-39
  }
  return mu;
}

// Sparse rotation tensor, element i of G(x) w: entries (I=i,J=i+1,K=i,V=+c) and (I=i,J=i-1,K=i-1,V=-c), c = sqrt(2)/2, circular
// (SDEs.py:369-399,425-430; sde_scheme.py:27-32): c sb (x_{i+1} w_i - x_{i-1} w_{i-1}).  w is the noise (gw) or the score (ga).
__device__ __forceinline__ float sparse_g(float sb, float xp, float xm, float w_i, float w_m) {
  const float cV = 0.5f * sqrtf(2.0f);
  return (cV * (sb * xp)) * w_i + (-cV * (sb * xm)) * w_m;
}

// Dense tensor, element i of a row whose state xr, Wiener increment wr and score ar are all at hand (the fused sampler loop:
// the three rows sit in LDS): gw_i = sum_jk G[i,j,k] (sb x_j) w_k, ga_i likewise with a (SDEs.py:432; sde_scheme.py:36) and
// f_i = sum_j L_G[i,j] (beta x_j) (SDEs.py:415), summed in the order of k_stage_rows' dense branch.
struct DenseTerms { float f, gw, ga; };
__device__ __forceinline__ DenseTerms dense_g(const float* __restrict__ G, const float* __restrict__ L_G, int n, int i, float beta,
                                              float sb, const float* xr, const float* wr, const float* ar) {
  float accw = 0.f, acca = 0.f, accf = 0.f;
  const float* Gi = G + i * n * n;
  for (int j = 0; j < n; ++j) {
    const float yj = sb * xr[j];
    accf += L_G[i * n + j] * (beta * xr[j]);
    float rw = 0.f, ra = 0.f;
    for (int k = 0; k < n; ++k) {
      const float g = Gi[j * n + k];
      rw += g * wr[k];
      ra += g * ar[k];
    }
    accw += yj * rw; acca += yj * ra;
  }
  return {accf, accw, acca};
}

// SGM (diagonal), one element: the bare increment.  Reverse: mu = (1-l/2) sqrt(beta) a + 1/2 beta x (SDEs.py:560-561,183-194
// with divSigma = 0); sigma = sqrt(1-l) sqrt(beta).  Forward: mu = -1/2 beta x.
// This is NOT stage_mu(sb a, f, f, 0) with f = -1/2 beta x: that form adds (1-l) 0 (reverse) or 1/2 0 (forward, Ito) to mu,
// which turns a mu of -0 into +0 — x = +-0 with a Wiener increment of -0 (a Box-Muller radius of 0) then gives the other
// zero.  The flat kernel keeps the parent's spelling and its bits; k_stage_rows (SGM with norm0 / delta_rows) keeps stage_mu's.
struct DiagCoef { float beta, sb, ca, sig; };
__device__ __forceinline__ float diag_inc(const StageArgs& A, const DiagCoef& c, float x, float a, float w) {
  float mu;
  if (A.proc == MSGM_PROC_REVERSE) mu = c.ca * (c.sb * a) - (-0.5f * c.beta * x);
  else mu = -0.5f * c.beta * x;
  return mu * A.delta + c.sig * w;
}

// Row stop index of the forward perturbation: k = trunc((nsf t)/T) in fp32 without contraction, rows with t >= T forced to
// nsf (SDEs.py:89-101).  k_forward_step_index and k_forward_perturb_* both call it.
__device__ __forceinline__ int32_t forward_step_k(float tb, int32_t nsf, float T) {
  const float f = __fdiv_rn(__fmul_rn((float)nsf, tb), T);
  int32_t kk = (int32_t)truncf(f);
  if (tb >= T) kk = nsf;
  return kk;
}

// x + (k1 + 2k2 + 2k3 + k4)/6                                  sde_scheme.py:250-253
// The sum is taken left to right, so it can also be carried one increment at a time: s = k1, s = rk4_add(s, k2),
// s = rk4_add(s, k3), x_new = rk4_close(x, s, k4) — the same bits as rk4_value with all four at hand.
__device__ __forceinline__ float rk4_add(float s, float k) { return s + 2.0f * k; }
__device__ __forceinline__ float rk4_close(float x, float s, float k4) { return x + (s + k4) / 6.0f; }
__device__ __forceinline__ float rk4_value(float x, float k1, float k2, float k3, float k4) {
  return rk4_close(x, rk4_add(rk4_add(k1, k2), k3), k4);
}

// ------------------------------------------------------------ K1: the additive SDE's closed-form perturbation
// k_perturb_vp, k_ssm_prep (sde_kernels.hip) and k_ssm_prep_gather (data_kernels.hip) take a row's time from vp_row and an
// element's value from vp_value: same streams, same indices, same bits.
struct VpSde { float b0, b1, T, t_eps; };
struct VpRow { float t, mw, sd; };

// Row b's time — as given (SGMsde.sample(t, y0): no clamp, SDEs.py:134-146), or u_b T with u_b injected or drawn from
// RNG_STREAM_T, clamped by mask arithmetic as upstream — and its mean weight and standard deviation (one Philox block + two exp).
__device__ __forceinline__ VpRow vp_row(const VpSde& P, int64_t b, const uint64_t* __restrict__ rng, const float* __restrict__ u,
                                        const float* __restrict__ t_given) {
  float t;
  if (t_given) {
    t = t_given[b];
  } else {
    const float ub = u ? u[b] : philox_uniform1(rng, 0, RNG_STREAM_T, (uint64_t)b);
    t = ub * P.T;
    const float m = (t <= P.t_eps) ? 1.0f : 0.0f;
    t = m * P.t_eps + (1.0f - m) * t;
  }
  return {t, vp_mean_weight(P.b0, P.b1, t), sqrtf(vp_var(P.b0, P.b1, t))};
}
__device__ __forceinline__ float vp_value(const VpRow& r, float eps, float x0) { return eps * r.sd + r.mw * x0; }
