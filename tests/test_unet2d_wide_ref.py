"""2-D U-Nets wider than the driver's 32 x (1, 2, 4) on the CPU: the nets of tests/test_unet2d_wide_gpu.py, their float64
oracle, and the oracle held to the reference's own outputs (tests/golden/g23_unet2d_wide.npz, tools/make_golden.py g23).

W64 = base_channels 64, (1, 2, 4); D4 = 32, (1, 2, 4, 8): both normalise cat([h, skip]) of 512 channels in
output_blocks.0 — twice the widest GroupNorm of the driver's net.  The oracle needs nothing new: UNet2DConfig's
model_channels / channel_mult with oracle.shapes.unet2d_shapes describe them, the state-dict keys are the reference's."""
import pytest
import torch

from conftest import check_digest, load_golden, rel_l2
from oracle import nets_ref as N
from oracle import ssm_ref as L
from oracle.det_params import det_state_dict, init_like_state_dict
from oracle.shapes import unet2d_shapes
from test_multihead_oracle import g18_inputs, mh_attention_block

S = 16
# tag: (base_channels, channel_mults, num_heads, premodule)
NETS = {
    "W64": (64, (1, 2, 4), 1, None),
    "D4": (32, (1, 2, 4, 8), 1, None),
    "W64h4": (64, (1, 2, 4), 4, None),
    "D4log": (32, (1, 2, 4, 8), 1, "NormalizeLogRadius"),
}
WIDEST = "core.output_blocks.0.0.in_layers.0."      # GroupNorm over cat([h, skip]): 512 channels in every net above


def wide_cfg(tag):
    base, mults, _, pre = NETS[tag]
    return N.UNet2DConfig(model_channels=base, channel_mult=mults, in_space=S, use_log_norm=pre is not None)


def wide_oracle(tag, fill, monkeypatch):
    """(parameters, score) of the float32 / float64 oracle of net `tag`; fill: "det" or "init_like"."""
    _, _, heads, pre = NETS[tag]
    cfg = wide_cfg(tag)
    shapes = unet2d_shapes(cfg, "core.")
    p = det_state_dict(shapes) if fill == "det" else init_like_state_dict(shapes)
    if heads != 1:
        monkeypatch.setattr(N, "attention_block", mh_attention_block(heads))
    return p, (lambda prm, yy, tt: N.vorticity_unet_forward(prm, yy, tt, cfg, pre, "F"))


@pytest.mark.parametrize("tag", list(NETS))
def test_widest_groupnorm_is_512(tag):
    base, mults, _, _ = NETS[tag]
    shapes = unet2d_shapes(wide_cfg(tag), "core.")
    norms = {k: s[0] for k, s in shapes.items() if k.endswith((".in_layers.0.weight", ".out_layers.0.weight", ".norm.weight", "out.0.weight"))}
    assert max(norms.values()) == 2 * base * max(mults) == 512 and norms[WIDEST + "weight"] == 512
    assert 4 * base <= 512                                              # the embedding bank's K


@pytest.mark.parametrize("tag", ["W64", "D4"])
def test_g23_oracle_vs_reference(tag, monkeypatch):
    """Forward, per-sample SSM loss, the widest norm's gradients in full and the digests of all gradients, at the tolerances
    the g17 / g18 oracle tests use; the parameter names and shapes are the reference's."""
    g = load_golden("g23_unet2d_wide")
    p, score = wide_oracle(tag, "init_like", monkeypatch)
    names = [str(s) for s in g[tag + "_param_names"]]
    shapes = [tuple(int(v) for v in str(s).split(",") if v) for s in g[tag + "_param_shapes"]]
    assert dict(zip(names, shapes)) == {k: tuple(v.shape) for k, v in p.items()}
    with torch.no_grad():
        e = rel_l2(score(p, g[tag + "_x"], g[tag + "_fwd_t"]), g[tag + "_fwd"])
    assert e <= 5e-6, e
    sp, t, y, v = g18_inputs(g, tag)
    _, per, grads = L.ssm_mean_and_grads(sp, score, p, t, y, v, form="jvp")
    assert rel_l2(per, g[tag + "_per"]) <= 1e-5, rel_l2(per, g[tag + "_per"])
    for k in ("weight", "bias"):
        ref = g[f"{tag}_grad::a.{WIDEST}{k}"]
        assert ref.numel() == 512
        assert rel_l2(grads[WIDEST + k], ref) <= 1e-4, (k, rel_l2(grads[WIDEST + k], ref))
    check_digest(g, tag, grads, "a.", 1e-4)
