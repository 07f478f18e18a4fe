"""Shared by tests/test_unet1d_deep_ref.py (CPU) and tests/test_unet1d_deep_gpu.py: the seven 1-D U-Net cases at which every
level of the net counts, their closed-form parameters, inputs and float64 / float32 oracle results (each computed once per
process and never modified), and the oracle's forward restated with one switchable wiring mistake.

The fill is ``oracle.det_params.init_like_state_dict(gain=3.0)``.  Under the sinusoidal ``det_state_dict`` everything below
the net's top level moves the output by 1e-5 .. 1e-11, and under the gain-1 well-conditioned fill 26 of 46 gradient tensors lie
below 1e-3 of the largest; gain 3 puts every tensor above 5e-4 of the largest at all seven shapes (test_unet1d_deep_ref.py
asserts >= 1e-4), so ``conftest.parity_vs_fp64(floor_frac=1e-4)`` measures every tensor against its own norm."""
import math

import torch
import torch.nn.functional as F

from oracle import nets_ref as N, sde_ref as S, ssm_ref as LR
from oracle.det_params import init_like_state_dict
from oracle.shapes import unet1d_shapes

GAIN = 3.0
FLOOR_FRAC = 1e-4
NLR = "NormalizeLogRadius"
DEFAULT = dict(base=32, mults=(1, 2, 4), emb=128)
# L, B, premodule, net.  Lengths per level (level_lengths): A 100 / 50 / 25 / 12 (one pad 24 -> 25; the top level on a ragged
# 128-position tile, below it the GEMM kernels), B 37 / 18 / 9 / 4 (pads 8 -> 9 and 36 -> 37; no level reaches 64 positions),
# C as B with tangent-carrying embedding rows, D 9 / 4 / 2 / 1 (middle block at one position), E 8 / 4 / 2 / 1 (paired: 4 / 2 /
# 1 pairs), F 256 / 128 / 64 / 32 (paired, tile kernels), G 13 / 6 / 3 on a two-level net with 16 | 32 channels.
CASES = {
    "A": dict(L=100, B=2, pre=None, **DEFAULT),
    "B": dict(L=37, B=3, pre=None, **DEFAULT),
    "C": dict(L=37, B=3, pre=NLR, **DEFAULT),
    "D": dict(L=9, B=3, pre=NLR, **DEFAULT),
    "E": dict(L=8, B=3, pre=None, **DEFAULT),
    "F": dict(L=256, B=2, pre=None, **DEFAULT),
    "G": dict(L=13, B=3, pre=NLR, base=16, mults=(1, 2), emb=32),
}
UNPAIRED = ("A", "B", "C", "D", "G")
PAIRED = ("E", "F")
MISTAKES = ("pad_left", "swap_cat", "emb_border", "down_tap", "skip_grad")


def levels(case):
    return len(CASES[case]["mults"])


def shapes(case):
    c = CASES[case]
    return unet1d_shapes(c["L"], c["pre"], c["base"], c["mults"], c["emb"])


def params(case, fill=None):
    """Fresh float32 parameters (a new dict of new tensors on every call)."""
    return (fill or (lambda sh: init_like_state_dict(sh, gain=GAIN)))(shapes(case))


def draws(case):
    """x, u, eps, u_v of one SSM evaluation (the order tests/test_unet2d_sizes_gpu.py draws them in), seeded by L."""
    c = CASES[case]
    B, L = c["B"], c["L"]
    torch.manual_seed(L)
    return torch.randn(B, L) * 3, torch.rand(B), torch.randn(B, L), torch.rand(B, L)


def forward_draws(case, rows=5):
    L = CASES[case]["L"]
    torch.manual_seed(1000 + L)
    return torch.randn(rows, L) * 3, torch.rand(rows) * 0.9 + 0.05


def score(case, mistake=None):
    c = CASES[case]
    if mistake is None:
        return lambda prm, yy, tt: N.unet1d_forward(prm, yy, tt, c["pre"], levels=len(c["mults"]))
    return lambda prm, yy, tt: forward_with_mistake(prm, yy, tt, c["pre"], len(c["mults"]), mistake)


def ssm_inputs(case):
    x, u, eps, uv = draws(case)
    sp = S.SdeSpec()
    t = S.clamp_time(sp, u.reshape(-1, 1))
    return sp, t, S.vp_perturb(sp, t, x, eps), S.rademacher_from_uniform(uv)


def ssm_oracle(case, dtype, mistake=None, p=None):
    """(per-sample loss, {name: gradient}) of the SGM sliced-score-matching loss in ``dtype``."""
    sp, t, y, v = ssm_inputs(case)
    p = p if p is not None else params(case)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _, per, g = LR.ssm_mean_and_grads(sp, score(case, mistake), {k: w.to(dtype) for k, w in p.items()}, t.to(dtype), y.to(dtype),
                                      v.to(dtype))
    return per, g


_ORACLE = {}


def oracle(case, dtype):
    """ssm_oracle(case, dtype) of the unmodified net, computed once; callers must not write into it."""
    if (case, dtype) not in _ORACLE:
        _ORACLE[case, dtype] = ssm_oracle(case, dtype)
    return _ORACLE[case, dtype]


def oracle_fn(case):
    """The ``oracle(dtype)`` argument of conftest.parity_vs_fp64."""
    return lambda dtype: oracle(case, dtype)


# ------------------------------------------------------------------------------------------------ one wiring mistake
def forward_with_mistake(p, x, t, premodule, nlev, mistake):
    """oracle.nets_ref.unet1d_forward, restated so that one wiring mistake can be switched on, each at the deepest level where
    it applies (``mistake=None`` reproduces the oracle bit for bit; test_unet1d_deep_ref.py asserts that):

    pad_left    the deepest F.pad puts its zero column on the left,
    swap_cat    the deepest decoder block reads [skip, up] instead of [up, skip],
    emb_border  the middle block's first convolution sees the broadcast embedding continue past both borders (not zero-padded),
    down_tap    the deepest downsampling convolution loses its last tap,
    skip_grad   the gradient that reaches the encoder through the deepest skip tensor is dropped (forward values and tangents
                unchanged: the skip is computed a second time from detached parameters)."""
    assert mistake is None or mistake in MISTAKES
    deep = nlev - 1
    h = x.unsqueeze(1) if x.ndim == 2 else x
    t = t.reshape(-1, 1).to(h.dtype)
    emb = N._lin(p, "time_mlp.2", F.gelu(N._lin(p, "time_mlp.0", t)))
    q = {k: w.detach() for k, w in p.items()} if mistake == "skip_grad" else None
    embq = None
    if q is not None:
        embq = N._lin(q, "time_mlp.2", F.gelu(N._lin(q, "time_mlp.0", t)))
    if premodule == NLR:
        h, lr = N.normalize_log_radius(h)
        h = h * math.sqrt(h.shape[-1])
        lr = lr.reshape(lr.shape[0], -1)
        emb = emb + N._lin(p, "scale_embed.2", F.gelu(N._lin(p, "scale_embed.0", lr)))
        if q is not None:
            embq = embq + N._lin(q, "scale_embed.2", F.gelu(N._lin(q, "scale_embed.0", lr)))
    emb = emb.unsqueeze(-1)
    rep = lambda z, e=emb: e.expand(-1, -1, z.shape[-1])       # noqa: E731
    skips = []
    hq = h
    for i in range(nlev):
        h = N._conv_block_1d(p, f"enc_blocks.{i}", torch.cat([h, rep(h)], dim=1))
        s = h
        if q is not None:                                      # the same values from parameters that carry no gradient
            hq = N._conv_block_1d(q, f"enc_blocks.{i}", torch.cat([hq, rep(hq, embq.unsqueeze(-1))], dim=1))
            if i == deep:
                s = hq
            else:
                hq = F.conv1d(hq, q[f"downs.{i}.weight"], q[f"downs.{i}.bias"], stride=2, padding=1)
        skips.append(s)
        w = p[f"downs.{i}.weight"]
        if mistake == "down_tap" and i == deep:
            w = torch.cat([w[..., :3], torch.zeros_like(w[..., 3:])], dim=-1)
        h = F.conv1d(h, w, p[f"downs.{i}.bias"], stride=2, padding=1)
    cat = torch.cat([h, rep(h)], dim=1)
    if mistake == "emb_border":
        c = h.shape[1]
        wm, ones = p["middle.net.0.weight"], torch.ones_like(cat[:, c:, :1])
        h = F.conv1d(torch.cat([F.pad(cat[:, :c], (1, 1)), torch.cat([emb * ones, cat[:, c:], emb * ones], dim=-1)], dim=1), wm,
                     p["middle.net.0.bias"])
        h = F.gelu(F.conv1d(F.gelu(h), p["middle.net.2.weight"], p["middle.net.2.bias"], padding=1))
    else:
        h = N._conv_block_1d(p, "middle", cat)
    padded = False
    for i in range(nlev):
        h = F.conv_transpose1d(h, p[f"up_convs.{i}.weight"], p[f"up_convs.{i}.bias"], stride=2, padding=1)
        s = skips.pop()
        if h.shape[-1] != s.shape[-1]:
            d = s.shape[-1] - h.shape[-1]
            h = F.pad(h, (d, 0) if mistake == "pad_left" and not padded else (0, d))
            padded = True
        first = [s, h] if mistake == "swap_cat" and i == 0 else [h, s]
        h = N._conv_block_1d(p, f"dec_blocks.{i}", torch.cat(first + [rep(h)], dim=1))
    return F.conv1d(h, p["final.weight"], p["final.bias"]).squeeze(1)
