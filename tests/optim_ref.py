"""Plain-torch restatement of csrc/optim_kernels.hip (global gradient norm, Adam with clipping, weight EMA), for float64
parity tests, in the style of tests/sde_stage_ref.py: each function evaluates the kernel's documented formula in ``dtype``
(float64 = the truth, float32 = the kernel's arithmetic, the one the tolerance constants are measured on) and returns
``(value, magnitude)``; the magnitude is the same expression with every term replaced by its absolute value.
Comparison: |kernel - ref64| <= c * 2^-24 * magnitude per element, c = 4 x the measured float32 ratio (``c_of``).

The squared norm accumulates in DOUBLE in the kernel, so its float32 restatement does too (the product g * gscale is
rounded to float32, squares and adds are double) and the ``gnorm`` constant has no buckets by n.
"""
import math

import numpy as np
import torch

import sde_stage_ref as R
from sde_stage_ref import c32, ratio  # noqa: F401  (re-exported for the tests)

# ------------------------------------------------------------------------------------------------ tolerance constants
# Worst |ref32 - ref64| / (2^-24 magnitude) over the shapes of tests/test_optim_stage_gpu.py (KERNEL_N), five steps each,
# measured by tests/test_optim_ref.py::test_tolerance_constants, which asserts they stay within c / 4.
MEASURED = {
    # family: worst ratio of the float32 restatement against float64 (torch CPU), rounded up to the next 0.1
    "gnorm": 0.7,                               # measured 0.642  (float) of a double norm: the final rounding alone
    "adam_clip": 6.5,                           # measured 6.433  p, m, v after (g * gscale) * coef
    "ema": 2.0,                                 # measured 1.997
}


def c_of(family):
    return 4.0 * MEASURED[family]


# ------------------------------------------------------------------------------------------------ slice layout
SLICE, MAX_SLICES = 8192, 1024


def slice_len(n):
    """Elements per slice of msgm_grad_sqnorm: a function of n only."""
    if n <= SLICE * MAX_SLICES:
        return SLICE
    per = -(-n // MAX_SLICES)
    return -(-per // 1024) * 1024


def n_partials(n):
    return -(-n // slice_len(n))


# Kernel shapes of the GPU tests: the scalar body (4 elements through an unaligned view, 7), 4096, one slice exactly and
# one element more, the last n at the base slice length and the first past the cap, about 2 M (not a multiple of 8192).
KERNEL_N = (4, 7, 4096, SLICE, SLICE + 1, SLICE * MAX_SLICES, SLICE * MAX_SLICES + 1, 2097156)


def _block_sum(acc):
    """(..., 256) doubles -> (...): the xor tree inside each 64-lane wave, then (w0 + w1) + (w2 + w3)."""
    acc = acc.reshape(*acc.shape[:-1], 4, 64)
    while acc.shape[-1] > 1:
        h = acc.shape[-1] // 2
        acc = acc[..., :h] + acc[..., h:]
    acc = acc[..., 0]
    return (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])


def sqnorm_partials(g, gscale):
    """The kernel's partials, to the bit: gg = float32(g * gscale); quad q of a slice belongs to thread q % 256, a thread
    adds gg^2 (double) over its quads in rising order, elements of a quad in rising order; then ``_block_sum``."""
    g = g.detach().reshape(-1)
    n, L = g.numel(), slice_len(g.numel())
    S = -(-n // L)
    gg = (g.float() * np.float32(gscale)).double()
    sq = torch.zeros(S * L, dtype=torch.float64, device=g.device)
    sq[:n] = gg * gg
    sq = sq.reshape(S, L // 1024, 256, 4)
    acc = torch.zeros(S, 256, dtype=torch.float64, device=g.device)
    for trip in range(L // 1024):
        for k in range(4):
            acc = acc + sq[:, trip, :, k]
    return _block_sum(acc)


def sum_partials(partials):
    """The prologue of msgm_adam_step_ex: thread t adds partials[t], partials[t + 256], ... in turn, then ``_block_sum``."""
    k = partials.numel()
    pad = torch.zeros(-(-k // 256) * 256, dtype=torch.float64, device=partials.device)
    pad[:k] = partials
    pad = pad.reshape(-1, 256)
    acc = torch.zeros(256, dtype=torch.float64, device=partials.device)
    for r in range(pad.shape[0]):
        acc = acc + pad[r]
    return _block_sum(acc)


def sqnorm(g, gscale, dtype=torch.float64):
    """sum (g * gscale)^2.  float64: the plain sum.  float32: the kernel's slices and reduction order (double adds)."""
    if dtype == torch.float32:
        s = sum_partials(sqnorm_partials(g, gscale))
    else:
        s = ((g.detach().double().reshape(-1) * c32(gscale)) ** 2).sum()
    return s, s


def gnorm(g, gscale, dtype=torch.float64):
    """The reported pre-clip norm: sqrt(sqnorm), rounded to float32 in the float32 restatement."""
    s = sqnorm(g, gscale, dtype)[0].sqrt()
    if dtype == torch.float32:
        s = s.float()
    return s, s.double()


def clip_coef(norm32, max_norm, dtype=torch.float64):
    """clip_grad_norm_'s coefficient min(1, max_norm / (norm + 1e-6)) from the REPORTED norm (a float32 value), formed in
    double; the float32 restatement rounds it to float32 as the kernel does."""
    c = min(1.0, float(max_norm) / (float(norm32) + 1e-6)) if math.isfinite(float(norm32)) else float("nan")
    if dtype == torch.float32:
        c = c32(c)
    return c, abs(c)


def adam_clip_step(p, g, m, v, step, norm32, max_norm, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, gscale=1.0,
                   dtype=torch.float64):
    """One step of msgm_adam_step_ex without EMA: gg = (g * gscale) * coef (two float32 roundings in the float32
    restatement), then the Adam update of sde_stage_ref.adam_step on gg.  max_norm None: no clipping (coef = 1).
    Returns ((p, mag), (m, mag), (v, mag))."""
    coef = 1.0 if max_norm is None else clip_coef(norm32, max_norm, dtype)[0]
    G = g.detach().to(dtype).reshape(-1)
    if dtype == torch.float32:
        gg = (G * np.float32(gscale)) * np.float32(coef)
    else:
        gg = (G * c32(gscale)) * coef
    return R.adam_step(p, gg, m, v, step, lr=lr, beta1=beta1, beta2=beta2, eps=eps, gscale=1.0, dtype=dtype)


def ema_step(ema, p_new, rate, dtype=torch.float64):
    """ema * float32(rate) + p_new * float32(1 - rate): two products, one add (update_ema, model/nn_utils.py:117-127)."""
    r, o = c32(rate), c32(1.0 - rate)
    E, P = ema.detach().to(dtype).reshape(-1), p_new.detach().to(dtype).reshape(-1)
    if dtype == torch.float32:
        r, o = np.float32(r), np.float32(o)
    return E * r + P * o, E.abs() * float(r) + P.abs() * float(o)


def kernel_inputs(n, seed=None, device="cpu"):
    """(p, g-generator) of the kernel cases: p ~ 0.1 N(0,1), gradients ~ 0.01 N(0,1), float32 rounded from float64 draws."""
    gen = torch.Generator(device=device).manual_seed(n if seed is None else seed)
    p = R.randn(n, generator=gen, device=device) * 0.1
    return p, (lambda: R.randn(n, generator=gen, device=device) * 0.01)
