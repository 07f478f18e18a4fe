"""The 2-D U-Net wider than the driver's 32 x (1, 2, 4), end to end on the HIP path (nets and oracle: test_unet2d_wide_ref).

W64 (64, (1, 2, 4)), D4 (32, (1, 2, 4, 8)), W64h4 (W64 with four heads) and D4log (D4 with NormalizeLogRadius) at in_space 16
all normalise cat([h, skip]) of 512 channels.  Before the GroupNorm kernels took more than 256 channels every one of them
constructed, loaded its state dict and then raised MsgmError("msgm_groupnorm_... failed: unsupported") in the middle of
its first pass.

Per net: (a) the training pass (SSM loss and every parameter gradient, B = 2) at conftest.parity_vs_fp64's default slack
(2, 4); (b) the eval-mode sampler forward at 5 rows, no further from the float64 oracle than max(2 x the float32 oracle,
1e-6) — the rule of test_unet2d_sizes_gpu; (c) spies on the routes: the two-source GroupNorm at 512 channels (training; the
sampler concatenates at 4x4 / 2x2 pixels and normalises 512 channels from one source), the folded-statistics route of the
sampler, fused attention where the shape has a kernel (T = 64 at C = 128 / 64, four heads of
32; T = 16 on the one-launch kernel up to head width 128) and the composed chain at head width 256 (W64's 4x4 level and
middle block, D4's 2x2 middle block; none in W64h4).  (d) UNetScoreTrainer on W64: graph replay equals eager bit for bit.
The g23 fixture (the reference's own outputs) at the absolute tolerances of g17 in test_round3_gpu.
Nets past the limits are refused by name before any launch.

Measured on one MI355X (profiles/wide_unet/parity_measured.txt; HIP | float32 oracle, both against float64).  (a) flat
gradient: W64 7.98e-5 | 2.06e-4, D4 8.08e-4 | 5.88e-4, W64h4 4.85e-5 | 6.78e-5, D4log (init_like fill) 6.81e-6 | 3.69e-6.
(b) W64 1.01e-5 | 2.03e-5, D4 6.84e-6 | 3.69e-6 (1.85 of the 2 allowed), W64h4 2.19e-5 | 1.30e-5, D4log 1.96e-6 | 1.20e-6.
What (b) does NOT show: on the ill-conditioned det fill both figures move by 2-3x with the input, and at other input seeds
the same rule reads 0.5 ... 3.1 for W64 (seed 17: 1.84e-5 | 5.88e-6); on the well-conditioned fill the 64-wide nets stand at
a steady 2.1x (2.1e-6 | 1.0e-6; 2.5x on the direct convolution kernels, so it is not the Winograd transforms), the four-level
nets at 1.5-1.6x.  The inputs here are the ones test_unet2d_sizes_gpu uses (seed = in_space), fixed before anything was run."""
import sys

import pytest
import torch

from conftest import check_digest, load_golden, rel_l2, within
from sdeflow_light_amd import ops
from sdeflow_light_amd._lib import MsgmError
from test_unet2d_wide_ref import NETS, S, WIDEST, wide_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda"
# The parameter fill of (a) and (b): oracle.det_params' sinusoidal det fill, except for D4log.  With four levels AND the
# log-radius conditioning the det fill is too ill-conditioned for a 2x yardstick (training pass, flat gradient vs float64:
# HIP 8.9e-4 | float32 oracle 3.2e-4, worst tensor 4.1e-3 | 1.2e-3, the float32 oracle itself 100x its figure on the
# well-conditioned fill), so that net runs on load_init_like_ (HIP 6.8e-6 | 3.7e-6) — the slack stays (2, 4).
FILL = {"W64": "det", "D4": "det", "W64h4": "det", "D4log": "init_like"}
FUSED = ("attention_forward", "attention_dual_forward", "attention_dual_backward")
FUSED_MH = ("attention_mh_forward", "attention_dual_mh_forward", "attention_dual_mh_backward")
SMALL = ("attention_small_forward", "attention_small_dual_forward", "attention_small_dual_backward")
COMPOSED = ("bmm", "softmax_dual_forward", "softmax_dual_backward")
GN = ("groupnorm_dual_forward", "groupnorm_dual_forward2", "groupnorm_dual_backward2", "groupnorm_affine", "groupnorm_affine_cs")


def _net(tag, fill=None, **kw):
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from oracle.det_params import load_det_, load_init_like_
    base, mults, heads, pre = NETS[tag]
    net = VorticityUNet(base_channels=base, channel_mults=mults, num_res_blocks=2, attention_resolutions=(2, 4), in_space=S,
                        premodule=pre, num_heads=heads, flatten_order="F", **kw)
    (load_det_ if (fill or FILL[tag]) == "det" else load_init_like_)(net)
    return net.to(DEV)


def _spy(monkeypatch):
    """Call counters on the attention entry points, and the channel split (C0, C1) of every two-source-capable GroupNorm call."""
    calls = {k: 0 for k in FUSED + FUSED_MH + SMALL + COMPOSED}
    splits = {k: [] for k in GN}

    def count(name):
        real = getattr(ops, name)

        def w(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        monkeypatch.setattr(ops, name, w)
    for name in calls:
        count(name)

    def split(name, where):
        real = getattr(ops, name)

        def w(*a, **k):
            splits[name].append(where(a, k))
            return real(*a, **k)
        monkeypatch.setattr(ops, name, w)
    split("groupnorm_dual_forward", lambda a, k: (a[5], 0))
    split("groupnorm_dual_forward2", lambda a, k: (a[1], a[3]))
    split("groupnorm_dual_backward2", lambda a, k: (a[1], a[3]))
    split("groupnorm_affine", lambda a, k: (a[1], k.get("C1", 0) if k.get("x1") is not None else 0))
    split("groupnorm_affine_cs", lambda a, k: (a[2], k.get("C1", 0) if k.get("cs1") is not None else 0))
    return calls, splits


def _routes_ok(tag, calls, splits, train):
    _, _, heads, _ = NETS[tag]
    n = lambda names: sum(calls[k] for k in names)                      # noqa: E731
    wide2 = lambda name: [s for s in splits[name] if s[1] and s[0] + s[1] == 512]      # noqa: E731
    if train:
        assert wide2("groupnorm_dual_forward2") and wide2("groupnorm_dual_backward2"), splits
    else:
        # at 16x16 the 512-channel blocks sit at 4x4 / 2x2 pixels, where conv1 cannot fold its input transform: the sampler
        # concatenates there and the GroupNorm runs on ONE source of 512 channels (the two-source affine entries at 256 + 256
        # are tests/test_groupnorm_wide_gpu.py's)
        widest = {k: max([c0 + c1 for c0, c1 in v], default=0) for k, v in splits.items()}
        print(f"{tag} sampler: widest GroupNorm per entry {widest}")
        assert max(widest.values()) == 512, widest
        assert splits["groupnorm_affine_cs"], "the sampler never took the folded-statistics route"
    fused, other = (FUSED_MH, FUSED) if heads > 1 else (FUSED, FUSED_MH)
    assert n(fused) > 0 and n(other) == 0, calls                         # T = 64
    if tag.startswith("W64h4"):
        assert n(SMALL) > 0 and n(COMPOSED) == 0, calls                  # T = 16 at head width 64: the one-launch kernel
    elif tag.startswith("W64"):
        assert n(SMALL) == 0 and calls["bmm"] > 0 and calls["softmax_dual_forward"] > 0, calls      # T = 16 at head width 256
    else:
        assert n(SMALL) > 0 and calls["bmm"] > 0 and calls["softmax_dual_forward"] > 0, calls       # T = 16 at 128; T = 4 at 256
    assert (calls["softmax_dual_backward"] > 0) == (train and not tag.startswith("W64h4")), calls


@pytest.mark.parametrize("tag", list(NETS))
def test_training_pass_vs_float64_oracle(tag, monkeypatch):
    from test_host_gpu import make_gen
    from test_round2_gpu import ssm_parity_vs_fp64
    gen = make_gen("sgm", _net(tag))
    p, score = wide_oracle(tag, FILL[tag], monkeypatch)
    torch.manual_seed(0)
    B, d = 2, S * S
    x, u, eps, uv = torch.randn(B, d) * 3, torch.rand(B), torch.randn(B, d), torch.rand(B, d)
    calls, splits = _spy(monkeypatch)
    ssm_parity_vs_fp64(gen, score, p, x, u, eps, uv, f"VorticityUNet {tag} {S}x{S}, B=2")
    _routes_ok(tag, calls, splits, train=True)


@pytest.mark.parametrize("tag", list(NETS))
def test_sampler_forward_vs_float64_oracle(tag, monkeypatch):
    net = _net(tag).eval()
    p, score = wide_oracle(tag, FILL[tag], monkeypatch)
    torch.manual_seed(S)
    x, t = torch.randn(5, S * S) * 3, torch.rand(5) * 0.9 + 0.05
    calls, splits = _spy(monkeypatch)
    y = net(x.to(DEV), t.to(DEV)).cpu()
    _routes_ok(tag, calls, splits, train=False)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        r32 = score(p, x, t)
        r64 = score({k: w.double() for k, w in p.items()}, x.double(), t.double())
    e, e32 = rel_l2(y, r64), rel_l2(r32, r64)
    print(f"VorticityUNet {tag} {S}x{S} sampler forward, 5 rows: rel-L2 vs the float64 oracle {e:.2e} | float32 oracle {e32:.2e}")
    assert bool(torch.isfinite(y).all()) and e <= max(2 * e32, 1e-6), (e, e32)


def test_trainer_graph_replay_equals_eager_w64():
    """W64, B = 3: the graphed trainer's losses and parameters equal the eager trainer's bit for bit over 4 steps (one eager
    step, the capture, then replays), and the parameters move."""
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    from sdeflow_light_amd.train import UNetScoreTrainer
    B, d = 3, S * S
    out = {}
    for use_graph in (False, True):
        net = _net("W64")
        T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
        gen = PluginReverseSDE(SGMsde(T=T, num_steps_forward=16, device=DEV), net, T, deviceReverseSDE=DEV).to(DEV)
        tr = UNetScoreTrainer(gen, B, d, lr=1e-3, use_graph=use_graph, seed=5)
        p0 = net.flat_parameters()[0].clone()
        torch.manual_seed(0)
        tr.set_data(torch.randn(B, d, device=DEV))
        losses = [float(tr.step()) for _ in range(4)]
        assert (tr.graph is not None) == use_graph
        flat, _ = net.flat_parameters()
        assert float((flat - p0).abs().max()) > 1e-6, "parameters did not move"
        out[use_graph] = (losses, flat.clone().cpu())
    print(f"W64 {S}x{S} B=3 graph replay vs eager: losses {out[True][0]} vs {out[False][0]}")
    assert all(l == l and abs(l) != float("inf") for l in out[True][0])
    assert out[True][0] == out[False][0]
    assert torch.equal(out[True][1], out[False][1])


@pytest.mark.parametrize("tag", ["W64", "D4"])
def test_g23_reference_fixture(tag):
    """The HIP path against the REFERENCE's own outputs on the well-conditioned fill, at g17's absolute tolerances
    (test_round3_gpu: forward 3e-6, per-sample loss 6e-7, gradient digest 3e-5), and the widest norm's gradients in full."""
    from test_host_gpu import make_gen
    g = load_golden("g23_unet2d_wide")
    gen = make_gen("sgm", _net(tag, "init_like"))
    out = gen.a(g[tag + "_x"].to(DEV), g[tag + "_fwd_t"].to(DEV))
    within(rel_l2(out.cpu(), g[tag + "_fwd"]), 3e-6, f"VorticityUNet {tag} forward vs reference (well-conditioned fill)")
    gen.zero_grad()
    per = gen.ssm(g[tag + "_x"].to(DEV), u=g[tag + "_u_t"].reshape(-1).to(DEV), eps=g[tag + "_eps"].to(DEV),
                  u_v=g[tag + "_u_v"].to(DEV))
    within(rel_l2(per.detach().cpu(), g[tag + "_per"]), 6e-7, f"VorticityUNet {tag} per-sample SSM loss vs reference")
    per.mean().backward()
    grads = {k: p.grad.cpu() for k, p in gen.a.named_parameters()}
    for k in ("weight", "bias"):
        within(rel_l2(grads[WIDEST + k], g[f"{tag}_grad::a.{WIDEST}{k}"]), 3e-5, f"{tag} d{WIDEST}{k} (512 channels) vs reference")
    check_digest(g, tag, grads, "a.", 3e-5)


# ------------------------------------------------------------------------------------------------ refusals
class _CountingLib:
    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("msgm_"):
            return fn

        def w(*a, **k):
            self._log.append(name)
            return fn(*a, **k)
        return w


@pytest.mark.parametrize("kw,layer,limit", [
    (dict(base_channels=160, channel_mults=(1, 2, 4)), "core.time_embed", "512"),
    (dict(base_channels=96, channel_mults=(1, 2, 4, 8)), "core.output_blocks.0.0.in_layers.0", "1024"),
])
def test_nets_past_the_limits_are_refused_by_name_before_any_launch(kw, layer, limit, monkeypatch):
    """Construction and .to() still work; the first call (sampler forward and training pass alike) raises MsgmError naming the
    layer and the limit, with no call into the native library."""
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from test_host_gpu import make_gen
    net = VorticityUNet(num_res_blocks=2, attention_resolutions=(2, 4), in_space=S, flatten_order="F", **kw).to(DEV)
    gen = make_gen("sgm", net)
    x, t = torch.randn(2, S * S, device=DEV), torch.rand(2, device=DEV)
    torch.cuda.synchronize()
    log = []
    for name, mod in list(sys.modules.items()):
        if name.startswith("sdeflow_light_amd") and callable(getattr(mod, "lib", None)):
            monkeypatch.setattr(mod, "lib", (lambda real: lambda: _CountingLib(real(), log))(mod.lib))
    with pytest.raises(MsgmError) as e:
        net(x, t)
    assert layer in str(e.value) and limit in str(e.value), str(e.value)
    assert log == [], log
    with pytest.raises(MsgmError) as e:
        net.ssm_grad(x, t, torch.randn_like(x), torch.randn_like(x), torch.zeros(2, device=DEV), 0.5)
    assert layer in str(e.value) and log == [], (str(e.value), log)
    del gen
