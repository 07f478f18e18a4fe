"""The dual-number attention kernels (k_attn_dual_fwd / k_attn_dual_bwd) at the smallest shapes that reach each of their paths:
one and several key blocks, both branches of the XCD-aware block decode, the two-launch backward, the C = 32 text and the
D = 64 kernels through the multi-head entries.  Reference: float64 torch.func.jvp + autograd on the CPU."""
import math

import pytest
import torch

from conftest import rel_l2
from sdeflow_light_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BOUND = 2e-5          # what test_fused_dual_attention_forward_backward holds the same eight tensors to


def _attn(x, H, D):
    """QKVAttention.forward's arithmetic (model/unet.py:236-250): head h owns channels [3Dh, 3D(h+1)) as q | k | v."""
    B, T, _ = x.shape
    xh = x.view(B, T, H, 3, D)
    q, k, v = xh[..., 0, :], xh[..., 1, :], xh[..., 2, :]
    s = D ** -0.25
    w = torch.softmax(torch.einsum("bthc,bshc->bhts", q * s, k * s), -1)
    return torch.einsum("bhts,bshc->bthc", w, v).reshape(B, T, H * D)


def _reference(qkv, g, Bp, H, D, dtype):
    xp, xt = qkv[:Bp].to(dtype).requires_grad_(True), qkv[Bp:].to(dtype).requires_grad_(True)
    o, od = torch.func.jvp(lambda x: _attn(x, H, D), (xp,), (xt,))
    ((o * g[:Bp].to(dtype)).sum() + (od * g[Bp:].to(dtype)).sum()).backward()
    return o.detach(), od.detach(), xp.grad, xt.grad


# Bp, T, heads, D, multi-head entries
CASES = [(1, 64, 1, 64, False),       # one key block, two query blocks, one forward workgroup
         (3, 192, 1, 64, False),      # three key blocks (odd), six query blocks
         (9, 128, 1, 64, False),      # both branches of the XCD-aware decode: 8 full pairs + tail
         (1024, 128, 1, 64, False),   # the two-launch backward (NP nkb / 2 >= 1024): first + ACC
         (3, 64, 1, 32, False),       # the <2,...> text
         (5, 128, 2, 64, True)]       # D = 64 through the multi-head entries (128 channels, 2 heads)


@pytest.mark.parametrize("Bp,T,H,D,mh", CASES)
def test_dual_attention_paths_float64(Bp, T, H, D, mh):
    """Forward pair and all six gradients vs float64 (rel-L2 <= 2e-5 each; float32 torch's own distance printed next to it);
    a second forward and a second backward give the same bits."""
    C = H * D
    torch.manual_seed(T + C + Bp)
    qkv = torch.randn(2 * Bp, T, 3 * C) * 1.2
    qkv[0, : T // 2, :D] *= 3.0                          # a few peaked rows: exercises the running-max rescale
    g = torch.randn(2 * Bp, T, C)
    ref = _reference(qkv, g, Bp, H, D, torch.float64)
    t32 = _reference(qkv, g, Bp, H, D, torch.float32)
    scale = 1.0 / math.sqrt(D)
    dq_, dg_ = qkv.to(DEV).contiguous().view(-1), g.to(DEV).contiguous().view(-1)
    if mh:
        assert ops.attention_dual_mh_supported(T, H, D)
        fwd = lambda: ops.attention_dual_mh_forward(dq_, Bp, T, H, D, scale)                          # noqa: E731
        bwd = lambda att, stats: ops.attention_dual_mh_backward(dq_, att, dg_, stats, Bp, T, H, D, scale)   # noqa: E731
    else:
        assert ops.attention_dual_supported(T, C)
        fwd = lambda: ops.attention_dual_forward(dq_, Bp, T, C, scale)                                # noqa: E731
        bwd = lambda att, stats: ops.attention_dual_backward(dq_, att, dg_, stats, Bp, T, C, scale)   # noqa: E731
    att, stats = fwd()
    dqkv = bwd(att, stats)
    att2, stats2 = fwd()
    dqkv2 = bwd(att, stats)
    a, d = att.view(2 * Bp, T, C).cpu(), dqkv.view(2 * Bp, T, 3 * C).cpu().view(2 * Bp, T, H, 3, D)
    gp, gt = ref[2].view(Bp, T, H, 3, D), ref[3].view(Bp, T, H, 3, D)
    g32p, g32t = t32[2].view(Bp, T, H, 3, D), t32[3].view(Bp, T, H, 3, D)
    got = {"o": (a[:Bp], ref[0], t32[0]), "odot": (a[Bp:], ref[1], t32[1])}
    for i, nm in enumerate(("q", "k", "v")):
        got[nm + "bar"] = (d[:Bp, :, :, i], gp[:, :, :, i], g32p[:, :, :, i])
        got[nm + "dotbar"] = (d[Bp:, :, :, i], gt[:, :, :, i], g32t[:, :, :, i])
    errs = {k: (rel_l2(x.double(), r), rel_l2(t.double(), r)) for k, (x, r, t) in got.items()}
    print(f"dual attention paths Bp={Bp} T={T} " + (f"heads={H} D={D}" if mh else f"C={C}") + " vs float64 (float32 torch): "
          + " ".join(f"{k} {e:.1e} ({t:.1e})" for k, (e, t) in errs.items()))
    for k, (e, _) in errs.items():
        assert e <= BOUND, (k, e)
    assert torch.equal(att, att2) and torch.equal(stats, stats2), "a second forward gave other bits"
    assert torch.equal(dqkv, dqkv2), "a second backward gave other bits"
