"""Plain-torch restatement of the three options msgm_optim_step adds to msgm_adam_step_ex (csrc/optim_kernels.hip): weight
decay (L2 and decoupled), the non-finite step guard and the EMA warm-up, in the style of tests/optim_ref.py, whose
``adam_clip_step``, ``ema_step``, ``ratio`` and ``kernel_inputs`` it reuses.  Each function evaluates the kernel's
documented formula in ``dtype`` (float64 = the truth, float32 = the kernel's arithmetic) and returns ``(value, magnitude)``;
the magnitude is the same expression with every term replaced by its absolute value.
Comparison: |kernel - ref64| <= c * 2^-24 * magnitude per element, c = 4 x the measured float32 ratio (``c_of``).
"""
import math

import numpy as np
import torch

import optim_ref as O
from optim_ref import adam_clip_step, ema_step, kernel_inputs, ratio  # noqa: F401  (reused, and re-exported for the tests)
from sde_stage_ref import c32

NONE, L2, DECOUPLED = 0, 1, 2                     # decay_mode of msgm_optim_step

# ------------------------------------------------------------------------------------------------ tolerance constants
# Measured by tests/test_optim_decay_ref.py on the CPU.
#   torch64: worst |restatement64 - torch| / (2^-53 magnitude) over five float64 steps of torch.optim.Adam(weight_decay) and
#     torch.optim.AdamW with clip_grad_norm_ (test_restatement_equals_torch_float64, which bounds it by 4 x this), with
#     the float32 rounding of the kernel's constants (c32) taken out, so that reassociation is all that differs.  With
#     the rounding in, the same comparison measures 2.1e9 (2.4e-7 of the magnitude: a few float32 roundings).
#   adam_l2 / adamw / ema_warmup: worst |ref32 - ref64| / (2^-24 magnitude) over KERNEL_N, five steps each
#     (test_tolerance_constants asserts they stay within c / 4), rounded up to the next 0.1.
MEASURED = {
    "torch64": 17.4,                            # measured 17.362  in units of 2^-53 magnitude
    "adam_l2": 5.7,                             # measured 5.656  p, m, v after ((g * gscale) * coef) + wd * p
    "adamw": 5.2,                               # measured 5.196  p, m, v after p * (1 - lr wd)
    "ema_warmup": 2.0,                          # measured 1.933
}


def c_of(family):
    return 4.0 * MEASURED[family]


# Kernel shapes of the GPU test: the vector body and (through a shifted view) the scalar body, the scalar tail, 4096, two
# slices (the verdict and the norm cross workgroups), and about 2 M (a thread walks several quads, 257 partials).
KERNEL_N = (4, 7, 4096, O.SLICE + 1, 2097156)
GSCALE, RATE, WD, STEPS = 0.5, 0.999, 0.05, 5


# ------------------------------------------------------------------------------------------------ weight decay
def decay_step(mode, wd, p, g, m, v, step, norm32, max_norm, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, gscale=1.0,
               dtype=torch.float64):
    """One step of msgm_optim_step without EMA.  mode NONE: ``adam_clip_step``.  L2 (torch.optim.Adam(weight_decay)):
    g' = ((g * gscale) * coef) + float32(wd) * p, one product and one add, then the Adam update on g'.  DECOUPLED
    (torch.optim.AdamW): p' = p * float32(1 - lr * wd), the factor formed in double, then the Adam update on p'.
    ``step`` is the EFFECTIVE count.  Returns ((p, mag), (m, mag), (v, mag))."""
    kw = dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, dtype=dtype)
    P = p.detach().to(dtype).reshape(-1)
    if mode == NONE:
        return adam_clip_step(P, g, m, v, step, norm32, max_norm, gscale=gscale, **kw)
    if mode == DECOUPLED:
        f = c32(1.0 - lr * wd)
        return adam_clip_step(P * (np.float32(f) if dtype == torch.float32 else f), g, m, v, step, norm32, max_norm,
                              gscale=gscale, **kw)
    coef = 1.0 if max_norm is None else O.clip_coef(norm32, max_norm, dtype)[0]
    G = g.detach().to(dtype).reshape(-1)
    if dtype == torch.float32:
        gg = (G * np.float32(gscale)) * np.float32(coef)
        g2 = gg + np.float32(wd) * P
    else:
        gg = (G * c32(gscale)) * coef
        g2 = gg + c32(wd) * P
    (pn, _), (mn, _), (vn, _) = adam_clip_step(P, g2, m, v, step, None, None, gscale=1.0, **kw)
    # magnitudes: every term of g' by its absolute value (gg and wd * p may cancel)
    ga = gg.abs().double() + c32(wd) * P.abs().double()
    M, V = m.detach().double().reshape(-1), v.detach().double().reshape(-1)
    w1, b2f, w2 = c32(1.0 - beta1), c32(beta2), c32(1.0 - beta2)
    ss, bs = c32(lr / (1.0 - beta1 ** step)), c32(math.sqrt(1.0 - beta2 ** step))
    mm = M.abs() + w1 * (ga + M.abs())
    den = vn.double().sqrt() / bs + c32(eps)
    return (pn, P.abs().double() + ss * (mm / den)), (mn, mm), (vn, V * b2f + w2 * (ga * ga))


# ------------------------------------------------------------------------------------------------ EMA warm-up
def warmup_rate(rate, k):
    """rate_k = min(rate, (1 + k) / (10 + k)) in double, k the 1-based effective count including this update."""
    return min(float(rate), (1.0 + k) / (10.0 + k))


def ema_warmup_step(ema, p_new, rate, k, dtype=torch.float64):
    """``ema_step`` with float32(rate_k) and float32(1 - rate_k)."""
    return ema_step(ema, p_new, warmup_rate(rate, k), dtype)


# ------------------------------------------------------------------------------------------------ non-finite guard
def nonfinite_verdict(gs, gscale):
    """The guard's verdict over the gradient buffers ``gs`` of one step: the float64 sum of all their partials (products
    g * gscale rounded to float32, squares and adds in double, the kernel's order) is not finite."""
    parts = torch.cat([O.sqnorm_partials(g, gscale) for g in gs])
    return not math.isfinite(float(O.sum_partials(parts)))
