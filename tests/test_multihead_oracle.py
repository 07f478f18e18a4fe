"""Multi-head attention (AttentionBlock num_heads > 1, model/unet.py:220-250) in the CPU oracle, pinned to the reference.

The oracle's attention_block is single-head.  This file restates it for H heads — the reference's reshape of qkv (B, 3C, T)
to (B*H, 3D, T), so head h owns the qkv channels [3Dh, 3D(h+1)) as q | k | v, the scale D^-1/4 on q and on k, and the
output reshape that puts head h at channels [Dh, D(h+1)) — installs it in place of oracle.nets_ref.attention_block, and
checks the whole network against g18 (tools/make_golden.py g18: the reference's VorticityUNet(num_heads=H)).
CPU only; the GPU tests (test_multihead_attention_gpu.py) reuse the restatement as their oracle."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_l2, check_digest
from oracle import nets_ref as N
from oracle import sde_ref as S
from oracle import ssm_ref as L

CASES = [("s32h2", 32, 2), ("s32h4", 32, 4), ("s16h2", 16, 2)]


def mh_attention_block(num_heads, num_heads_upsample=-1):
    """attention_block(p, key, x) for num_heads heads; decoder blocks (keys under output_blocks.) use num_heads_upsample,
    -1 meaning num_heads (model/unet.py:321-322, 431-435)."""
    up = num_heads if num_heads_upsample == -1 else num_heads_upsample

    def block(p, key, x):
        H = up if key.startswith("output_blocks.") else num_heads
        b, c = x.shape[:2]
        xf = x.reshape(b, c, -1)
        T = xf.shape[2]
        D = c // H
        hn = F.group_norm(xf, min(c, 32), p[key + ".norm.weight"], p[key + ".norm.bias"], eps=1e-5)
        qkv = F.conv1d(hn, p[key + ".qkv.weight"], p[key + ".qkv.bias"]).reshape(b * H, 3 * D, T)
        q, k, v = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:]
        s = 1.0 / math.sqrt(math.sqrt(D))
        w = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
        a = torch.einsum("bts,bcs->bct", w, v).reshape(b, c, T)
        a = F.conv1d(a, p[key + ".proj_out.weight"], p[key + ".proj_out.bias"])
        return (xf + a).reshape(x.shape)
    return block


def g18_inputs(g, tag):
    sp = S.SdeSpec()
    t = S.clamp_time(sp, g[tag + "_u_t"])
    y = S.vp_perturb(sp, t, g[tag + "_x"], g[tag + "_eps"])
    v = S.rademacher_from_uniform(g[tag + "_u_v"])
    return sp, t, y, v


def g18_attention_grads(g, tag, grads, prefix="a."):
    """(name, ours, reference) for the stored attention-parameter gradients of g18: the vectors in full, the (rows, C, 1)
    weights at every row and the input columns listed under {tag}_cols:: (spread over all heads)."""
    cols = g.sub(tag + "_cols::")
    out = []
    for k, ref in g.sub(tag + "_grad::").items():
        got = grads[k[len(prefix):]]
        if k in cols:
            got = got[:, cols[k]]
        out.append((k, got, ref))
    assert len(out) == 18 and len(cols) == 6
    return out


def g18_params(S_, dtype=torch.float32):
    from oracle.det_params import init_like_state_dict
    from oracle.shapes import unet2d_shapes
    p = init_like_state_dict(unet2d_shapes(N.UNet2DConfig(in_space=S_), "core."))
    return {k: v.to(dtype) for k, v in p.items()}


def test_restatement_is_the_oracle_at_one_head(monkeypatch):
    """At H = 1 the restatement is the oracle's own single-head block."""
    torch.manual_seed(0)
    c, T = 64, 16
    p = {"a.norm.weight": torch.randn(c), "a.norm.bias": torch.randn(c), "a.qkv.weight": torch.randn(3 * c, c, 1) * 0.2,
         "a.qkv.bias": torch.randn(3 * c) * 0.1, "a.proj_out.weight": torch.randn(c, c, 1) * 0.2, "a.proj_out.bias": torch.randn(c)}
    x = torch.randn(2, c, 4, 4)
    assert rel_l2(mh_attention_block(1)(p, "a", x), N.attention_block(p, "a", x)) <= 1e-6
    assert rel_l2(mh_attention_block(2)(p, "a", x), N.attention_block(p, "a", x)) > 1e-3


def test_restatement_head_layout():
    """Head h reads q | k | v from the qkv channels [3Dh, 3D(h+1)) and writes the output channels [Dh, D(h+1)):
    zeroing the value rows of head 1 changes only the output channels of head 1."""
    torch.manual_seed(1)
    c, H = 32, 2
    D = c // H
    p = {"a.norm.weight": torch.ones(c), "a.norm.bias": torch.zeros(c), "a.qkv.weight": torch.randn(3 * c, c, 1) * 0.3,
         "a.qkv.bias": torch.zeros(3 * c), "a.proj_out.weight": torch.eye(c).reshape(c, c, 1), "a.proj_out.bias": torch.zeros(c)}
    x = torch.randn(1, c, 4, 4)
    y0 = mh_attention_block(H)(p, "a", x)
    p2 = dict(p)
    w = p["a.qkv.weight"].clone()
    w[3 * D + 2 * D: 6 * D] = 0                     # v of head 1
    p2["a.qkv.weight"] = w
    y1 = mh_attention_block(H)(p2, "a", x)
    diff = (y1 - y0).reshape(c, -1).abs().amax(1)
    assert float(diff[:D].max()) == 0.0 and float(diff[D:].min()) > 0.0


@pytest.mark.parametrize("tag,S_,H", CASES)
def test_g18_multihead_oracle(tag, S_, H, monkeypatch):
    """The restated multi-head oracle against the reference: forward, per-sample SSM loss, the stored attention-parameter
    gradients (g18_attention_grads), digests of all gradients — at the g17 tolerances of test_oracle_golden.py."""
    g = load_golden("g18_multihead")
    assert int(g[tag + "_heads"]) == H
    monkeypatch.setattr(N, "attention_block", mh_attention_block(H))
    cfg = N.UNet2DConfig(in_space=S_)
    p = g18_params(S_)
    score = lambda prm, yy, tt: N.vorticity_unet_forward(prm, yy, tt, cfg, None, "F")
    with torch.no_grad():
        e = rel_l2(score(p, g[tag + "_x"], g[tag + "_fwd_t"]), g[tag + "_fwd"])
    assert e <= 5e-6, e
    sp, t, y, v = g18_inputs(g, tag)
    loss, per, grads = L.ssm_mean_and_grads(sp, score, p, t, y, v, form="jvp")
    assert rel_l2(per, g[tag + "_per"]) <= 1e-5, rel_l2(per, g[tag + "_per"])
    for k, got, ref in g18_attention_grads(g, tag, grads):
        e = rel_l2(got, ref)
        assert e <= 1e-4, (k, e)
    check_digest(g, tag, grads, "a.", 1e-4)


def test_g18_heads_matter():
    """The attention branch is live in the fixture: the single-head oracle at the same weights and input is far from the
    reference's two-head output (a net that ignored num_heads could not match g18)."""
    g = load_golden("g18_multihead")
    cfg = N.UNet2DConfig(in_space=32)
    with torch.no_grad():
        y1 = N.vorticity_unet_forward(g18_params(32), g["s32h2_x"], g["s32h2_fwd_t"], cfg, None, "F")
    e = rel_l2(y1, g["s32h2_fwd"])
    print(f"single-head oracle vs the two-head reference: rel-L2 {e:.2e}")
    assert e > 1e-3, e
