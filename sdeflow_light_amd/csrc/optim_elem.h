// optim_elem.h — the pieces sde_kernels.hip (K13, msgm_adam_step) and optim_kernels.hip (msgm_adam_step_ex, msgm_optim_step) share:
// 16-byte access to flat buffers and THE Adam element update.  One copy: the build keeps -ffp-contract=off, so two
// kernels that call adam_elem give the same bits.
#pragma once
#include "common.h"

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
// every pointer 16-byte aligned (a null pointer counts as aligned: optional operands)
template <typename... P>
__host__ __device__ __forceinline__ bool aligned16(P... p) { return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0; }

// torch.optim.Adam (defaults, no weight decay / amsgrad): MSGM_higherDim.py:792.
// Mirrors torch's single-tensor update: m.lerp_(g, 1-b1); v = v*b2 + (1-b2) g g;
// denom = sqrt(v)/sqrt(bc2) + eps; p += -(lr/bc1) * (m/denom), with the bias
// corrections formed in double precision as the Python scalars upstream are.
struct AdamCoef { float step_size, bc2_sqrt, w1, b2f, w2, epsf, gscale; };
struct AdamPmv { float p, m, v; };
// The coefficients at step st (1-based, after the increment): doubles in, rounded once each.
__device__ __forceinline__ AdamCoef adam_coef(double lr, double b1, double b2, double eps, float gscale, int64_t st) {
  const double bc1 = 1.0 - pow(b1, (double)st);
  const double bc2 = 1.0 - pow(b2, (double)st);
  return {(float)(lr / bc1), (float)sqrt(bc2), (float)(1.0 - b1), (float)b2, (float)(1.0 - b2), (float)eps, gscale};
}
__device__ __forceinline__ AdamPmv adam_elem(const AdamCoef& c, float p, float g, float m, float v) {
  const float gg = g * c.gscale;
  m = m + c.w1 * (gg - m);
  v = v * c.b2f + c.w2 * (gg * gg);
  const float denom = sqrtf(v) / c.bc2_sqrt + c.epsf;
  return {p - c.step_size * (m / denom), m, v};
}
// Weight decay around THE element update, compiled in by WD: 0 none (adam_elem as it is, p and g untouched),
// 1 L2 (torch.optim.Adam(weight_decay): g + wd * p, one product and one add, wd = (float)weight_decay),
// 2 decoupled (torch.optim.AdamW: p * wd first, wd = (float)(1 - lr * weight_decay) formed in double).
template <int WD>
__device__ __forceinline__ AdamPmv adam_elem_decay(const AdamCoef& c, float wd, float p, float g, float m, float v) {
  if constexpr (WD == 1) g = g + wd * p;
  if constexpr (WD == 2) p = p * wd;
  return adam_elem(c, p, g, m, v);
}
