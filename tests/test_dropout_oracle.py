"""Dropout in the 2-D U-Net (ResBlock out_layers = GroupNorm, SiLU, Dropout(p), conv; model/unet.py:152-158): the NumPy
restatement of the mask rule (philox_np.py) against the Random123 known-answer vectors, the oracle with the rule's masks
injected, and the constructor surface.  CPU only; test_dropout_gpu.py reuses the oracle patch."""
import numpy as np
import pytest
import torch

from oracle import nets_ref as N
import philox_np as PX

_GN_SILU = N._gn_silu          # the oracle's own block: a patch never wraps an earlier patch


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32_10."""
    cases = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in cases:
        got = tuple(int(w) for w in PX.philox4x32_10(*ctr, *key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])


def test_mask_rule_threshold_and_scale():
    assert PX.dropout_threshold(0.0) == (0, np.float32(1.0))
    thr, s = PX.dropout_threshold(0.1)
    assert thr == 1677722 and s == np.float32(1.0 / 0.9)
    assert PX.dropout_threshold(0.5)[0] == 1 << 23
    keep = PX.dropout_keep(7, 3, 0, 0, 0.0, 2, 16, 8)
    assert keep.min() == 1.0                                       # p = 0 keeps everything
    keep = PX.dropout_keep(7, 3, 0, 0, 0.3, 4, 256, 32)
    rate = float(keep.mean())
    sd = (0.3 * 0.7 / keep.size) ** 0.5
    assert abs(rate - 0.7) < 5 * sd, rate


def test_mask_is_addressed_by_global_row():
    """A shard at row_base draws the rows the one-GPU run draws at those rows; other layers / offsets draw other masks."""
    full = PX.dropout_keep(11, 5, 0, 3, 0.4, 8, 16, 12)
    assert np.array_equal(PX.dropout_keep(11, 5, 4, 3, 0.4, 4, 16, 12), full[4:])
    assert not np.array_equal(PX.dropout_keep(11, 5, 0, 4, 0.4, 8, 16, 12), full)
    assert not np.array_equal(PX.dropout_keep(11, 6, 0, 3, 0.4, 8, 16, 12), full)


def test_resblock_order_is_named_modules_order():
    """Layer index = position among all ResBlocks, input_blocks -> middle_block -> output_blocks (named_modules())."""
    from sdeflow_light_amd.NNUnet import ResBlock, VorticityUNet
    for kw in ({}, {"channel_mults": (1, 2), "num_res_blocks": 1, "attention_resolutions": (2,)}):
        net = VorticityUNet(base_channels=32, in_space=16, dropout=0.1, **kw)
        names = [k[len("core."):] for k, m in net.named_modules() if isinstance(m, ResBlock)]
        keys = PX.resblock_keys(channel_mult=kw.get("channel_mults", (1, 2, 4)), num_res_blocks=kw.get("num_res_blocks", 2))
        assert names == list(keys) and list(keys.values()) == list(range(len(names)))


def dropout_gn_silu(seed, offset, row_base, p, keys=None):
    """oracle.nets_ref._gn_silu with the mask rule applied to every ResBlock's out_layers.0 (NCHW: the channels-last mask
    permuted).  Called once per network pass, so under torch.func.jvp the primal and the tangent share the mask."""
    keys = PX.resblock_keys() if keys is None else keys
    real = _GN_SILU

    def gn_silu(prm, key, h):
        out = real(prm, key, h)
        if key.endswith(".out_layers.0"):
            B, C, H, W = h.shape
            m = PX.dropout_multiplier(seed, offset, row_base, keys[key[:-len(".out_layers.0")]], p, B, H, W, C)
            out = out * torch.from_numpy(m).to(out.dtype)
        return out
    return gn_silu


def _params(S_, dtype=torch.float64):
    from oracle.det_params import init_like_state_dict
    from oracle.shapes import unet2d_shapes
    p = init_like_state_dict(unet2d_shapes(N.UNet2DConfig(in_space=S_), "core."))
    return {k: v.to(dtype) for k, v in p.items()}


def test_oracle_patch_at_p0_is_the_oracle_and_masks_matter(monkeypatch):
    cfg = N.UNet2DConfig(in_space=16)
    p = _params(16)
    torch.manual_seed(0)
    x, t = torch.randn(2, 256, dtype=torch.float64) * 2, torch.tensor([0.3, 0.7], dtype=torch.float64)
    with torch.no_grad():
        y0 = N.vorticity_unet_forward(p, x, t, cfg, None, "F")
        monkeypatch.setattr(N, "_gn_silu", dropout_gn_silu(3, 1, 0, 0.0))
        y1 = N.vorticity_unet_forward(p, x, t, cfg, None, "F")
        monkeypatch.setattr(N, "_gn_silu", dropout_gn_silu(3, 1, 0, 0.3))
        y2 = N.vorticity_unet_forward(p, x, t, cfg, None, "F")
    assert torch.equal(y0, y1)
    assert float((y2 - y0).norm() / y0.norm()) > 1e-3


def test_oracle_jvp_shares_the_mask(monkeypatch):
    """Under forward mode the patched block multiplies primal and tangent by the same mask: a zero of the mask zeroes both."""
    monkeypatch.setattr(N, "_gn_silu", dropout_gn_silu(5, 0, 0, 0.5, keys={"b": 0}))
    torch.manual_seed(1)
    C = 32
    prm = {"b.out_layers.0.weight": torch.randn(C, dtype=torch.float64),
           "b.out_layers.0.bias": torch.randn(C, dtype=torch.float64)}
    h, hd = torch.randn(2, C, 4, 4, dtype=torch.float64), torch.randn(2, C, 4, 4, dtype=torch.float64)
    out, tan = torch.func.jvp(lambda z: N._gn_silu(prm, "b.out_layers.0", z), (h,), (hd,))
    keep = PX.dropout_multiplier(5, 0, 0, 0, 0.5, 2, 4, 4, C) != 0
    assert torch.equal(out == 0, torch.from_numpy(~keep)) and torch.equal(tan == 0, torch.from_numpy(~keep))


def test_constructor_accepts_dropout_and_keeps_state_dict():
    from sdeflow_light_amd.NNUnet import UNetModelWithLogNorm, VorticityUNet
    from sdeflow_light_amd._lib import MsgmError
    kw = dict(in_channels=1, model_channels=32, out_channels=1, in_space=16, num_res_blocks=2, attention_resolutions=(2, 4),
              channel_mult=(1, 2, 4))
    a, b = UNetModelWithLogNorm(dropout=0.1, **kw), UNetModelWithLogNorm(dropout=0, **kw)
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape for k in sa)
    assert isinstance(a.input_blocks[1][0].out_layers[2], torch.nn.Dropout) and a.input_blocks[1][0].out_layers[2].p == 0.1
    for p in (1.0, -0.1, 1.5):
        with pytest.raises(MsgmError):
            UNetModelWithLogNorm(dropout=p, **kw)
        with pytest.raises(MsgmError):
            VorticityUNet(dropout=p)
    for bad in ({"use_scale_shift_norm": True}, {"learn_potential": True}, {"conv_resample": False}, {"num_classes": 10}):
        with pytest.raises(MsgmError):
            UNetModelWithLogNorm(dropout=0.1, **kw, **bad)
    net = VorticityUNet(dropout=0.2)
    assert net.dropout_active()
    net.eval()
    assert not net.dropout_active()
    assert not VorticityUNet(dropout=0.0).dropout_active()


# ------------------------------------------------------------------------------------------------------------ g19
G19 = [("s32", 32, None), ("s16m", 16, "NormalizeLogRadius")]


def g19_case(g, tag):
    """(p, seed, ssm offset, forward offset) of a g19 case."""
    return float(g[tag + "_p"]), int(g[tag + "_seed"]), int(g[tag + "_offset"]), int(g[tag + "_fwd_offset"])


def g19_params(S_, pre, p):
    """The well-conditioned fill the reference was run with (load_init_like_ on the same state_dict keys)."""
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from oracle.det_params import load_init_like_
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=pre, in_space=S_,
                        attention_resolutions=(2, 4), flatten_order="F", dropout=p)
    load_init_like_(net)
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


def g19_grads(g, tag, grads, prefix="a."):
    """(name, ours, reference) for the stored gradients of g19: vectors in full, conv weights at the stored rows / columns."""
    out = []
    for k, ref in g.sub(tag + "_grad::").items():
        got = grads[k[len(prefix):]]
        if f"{tag}_rows::{k}" in g:
            got = got[g[f"{tag}_rows::{k}"]][:, g[f"{tag}_cols::{k}"]]
        out.append((k, got, ref))
    assert len(out) == 24
    return out


def g19_worst(g, tag, grads, prefix="a."):
    """Worst stored-gradient error, per tensor relative to max(|ref|, 1e-3 x the largest stored norm): a conv bias feeding a
    one-channel-per-group GroupNorm (in_layers.2.bias at 32 channels) has an analytically zero gradient and holds rounding
    noise only (the floor of conftest.check_digest).  Returns (error, name)."""
    trip = g19_grads(g, tag, grads, prefix)
    top = max(float(ref.double().norm()) for _, _, ref in trip)
    errs = {k: float((got.double().cpu() - ref.double()).norm()) / max(float(ref.double().norm()), 1e-3 * top)
            for k, got, ref in trip}
    k = max(errs, key=errs.get)
    return errs[k], k


def g19_inputs(g, tag, S_):
    """(spec, t, y, v) of the SSM case: SGM with the three draws forced, or the sparse MSGM SDE with (t, y) given."""
    from oracle import sde_ref as S
    if tag == "s32":
        sp = S.SdeSpec()
        t = S.clamp_time(sp, g[tag + "_u_t"])
        return sp, t, S.vp_perturb(sp, t, g[tag + "_x"], g[tag + "_eps"]), S.rademacher_from_uniform(g[tag + "_u_v"])
    sp = S.SdeSpec(kind=S.MSGM_SPARSE, n=S_ * S_, num_steps_forward=4)
    return sp, g[tag + "_t"], g[tag + "_y"], S.rademacher_from_uniform(g[tag + "_u_v"])


@pytest.mark.parametrize("tag,S_,pre", G19)
def test_g19_dropout_oracle(tag, S_, pre, monkeypatch):
    """The oracle with the rule's masks injected against the reference's VorticityUNet(dropout=p) in train mode with the same
    masks forced into its Dropout modules (g19): train-mode forward, per-sample SSM loss and gradients at row_base 0 and 4, at
    the g18 tolerances."""
    from conftest import load_golden, rel_l2, check_digest
    from oracle import ssm_ref as L
    g = load_golden("g19_dropout")
    p, seed, off, off_fwd = g19_case(g, tag)
    cfg = N.UNet2DConfig(in_space=S_, use_log_norm=pre is not None)
    prm = g19_params(S_, pre, p)
    score = lambda q, yy, tt: N.vorticity_unet_forward(q, yy, tt, cfg, pre, "F")
    monkeypatch.setattr(N, "_gn_silu", dropout_gn_silu(seed, off_fwd, 0, p))
    with torch.no_grad():
        e = rel_l2(score(prm, g[tag + "_fwd_x"], g[tag + "_fwd_t"]), g[tag + "_fwd"])
    assert e <= 5e-6, e
    sp, t, y, v = g19_inputs(g, tag, S_)
    for rb in (0, 4):
        monkeypatch.setattr(N, "_gn_silu", dropout_gn_silu(seed, off, rb, p))
        _, per, grads = L.ssm_mean_and_grads(sp, score, prm, t, y, v, form="jvp")
        assert rel_l2(per, g[f"{tag}_rb{rb}_per"]) <= 1e-5, (rb, rel_l2(per, g[f"{tag}_rb{rb}_per"]))
        if rb == 0:
            e, k = g19_worst(g, f"{tag}_rb0", grads)
            assert e <= 1e-4, (k, e)
        check_digest(g, f"{tag}_rb{rb}", grads, "a.", 1e-4)
    assert float((g[f"{tag}_rb4_per"] - g[f"{tag}_rb0_per"]).abs().max()) > 1e-3     # the row base selects other masks
