"""The dual-number attention kernels at 128 channels per head (k_attn_dual_fwd<8,1,16,*>, k_attn_dual_bwd<8,2,*>), at the smallest
shapes that reach each of their paths: the two- and the four-wave forward (the build that runs at two waves per SIMD), one and
several key blocks, a T that is no multiple of 64, both branches of the XCD-aware block decode, the two-launch backward whose
second launch asks for its slab addends ahead of phase 1, and the multi-head builds.  Reference: float64 torch.func.jvp +
autograd on the CPU.  The harness is tests/test_attn_dual_paths_gpu.py's."""
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
CASES = [(1, 32, 1, 128, False),      # one key block, one query block, the NW = 2 forward
         (3, 96, 1, 128, False),      # three key blocks, T not a multiple of 64
         (9, 64, 1, 128, False),      # both branches of the XCD-aware decode: 8 full pairs + tail
         (512, 128, 1, 128, False),   # the NW = 4 forward (two waves per SIMD); the two-launch backward, two slab groups: first + ACC
         (5, 64, 2, 128, True),       # the multi-head builds, NW = 2
         (256, 64, 2, 128, True)]     # the multi-head NW = 4 forward


@pytest.mark.parametrize("Bp,T,H,D,mh", CASES)
def test_dual_attention_c128_float64(Bp, T, H, D, mh):
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
    print(f"dual attention C128 Bp={Bp} T={T} " + (f"heads={H} D={D}" if mh else f"C={C}") + " vs float64 (float32 torch): "
          + " ".join(f"{k} {e:.1e} ({t:.1e})" for k, (e, t) in errs.items()))
    for k, (e, _) in errs.items():
        assert e <= BOUND, (k, e)
    assert torch.equal(att, att2) and torch.equal(stats, stats2), "a second forward gave other bits"
    assert torch.equal(dqkv, dqkv2), "a second backward gave other bits"
