"""The 1-D U-Net end to end against the float64 oracle where its deep levels count and at lengths that are no multiple of 8.

Every other whole-network test of UNet1D loads the sinusoidal det_params fill, under which everything below the top level
moves the output by 1e-5 .. 1e-11 (tests/test_unet1d_deep_ref.py::test_sinusoidal_fill_hides_the_same_mistake), and only a
forward ever ran the unpaired route.  Here the net carries ``init_like_state_dict(gain=3.0)`` (tests/unet1d_deep.py: no
gradient tensor under 5e-4 of the largest, so the yardstick runs with floor_frac = 1e-4) at seven cases:

  A 100 / 50 / 25 / 12   unpaired (ConvOp k = 4, s = 2 and convT), one pad 24 -> 25; top level on a ragged 128-position tile
  B 37 / 18 / 9 / 4      unpaired, pads 8 -> 9 and 36 -> 37; no convolution reaches 64 positions (k_conv_gemm, k_conv_wgrad)
  C as B + NormalizeLogRadius: the embedding rows carry a tangent
  D 9 / 4 / 2 / 1        + NormalizeLogRadius; the middle block at ONE position (both border corrections on the same pixel)
  E 8 / 4 / 2 / 1        paired (Stride2PairOp) with 4 / 2 / 1 pairs
  F 256 / 128 / 64 / 32  paired, halo-tile kernels at 256 / 128 / 64
  G 13 / 6 / 3           two levels, 16 | 32 channels (CoutP = 16), emb 32, + NormalizeLogRadius

Every test prints what it measured (profiles/unet1d_deep/parity_measured.txt is this file's output)."""
import pytest
import torch

import unet1d_deep as U
from conftest import check_digest, load_golden, parity_vs_fp64, rel_l2
from sdeflow_light_amd import ops
from sdeflow_light_amd.NNUnet1D import level_lengths
from sdeflow_light_amd.convnet import ConvOp, Stride2PairOp
from test_host_gpu import make_gen

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _net(case):
    from oracle.det_params import load_init_like_
    from sdeflow_light_amd.NNUnet1D import UNet1D
    c = U.CASES[case]
    net = UNet1D(input_dim=c["L"], base_channels=c["base"], channel_mults=c["mults"], num_res_blocks=2, premodule=c["pre"],
                 emb_dim=c["emb"])
    load_init_like_(net, gain=U.GAIN)
    return net.to(DEV)


def _spy(monkeypatch):
    """(stride, gather mode, output positions per sample) of every ops.conv_forward call (forwards, and the dgrads, which run
    as the transposed gather of the same kernel) and of every ops.conv_wgrad call."""
    fwd, wgrad = [], []
    geo = lambda g: (g.strideW, g.mode, g.Ho * g.Wo, g.KW)                     # noqa: E731
    real_f, real_w = ops.conv_forward, ops.conv_wgrad
    monkeypatch.setattr(ops, "conv_forward", lambda geom, *a, **k: (fwd.append(geo(geom)), real_f(geom, *a, **k))[1])
    monkeypatch.setattr(ops, "conv_wgrad", lambda geom, *a, **k: (wgrad.append(geo(geom)), real_w(geom, *a, **k))[1])
    return fwd, wgrad


def _routes_ok(case, net, fwd, wgrad, train):
    """The case ran on the route it is here for."""
    o = net._ops
    lens = level_lengths(U.CASES[case]["L"], U.levels(case))
    resamplers = [v for k, v in o.items() if k[0] in "du"]
    assert len(resamplers) == 2 * U.levels(case)
    if case in U.PAIRED:
        assert all(isinstance(v, Stride2PairOp) for v in resamplers)
        assert not any(s == 2 for s, *_ in fwd + wgrad)                         # pairs: 3-tap stride-1 convolutions only
    else:
        assert all(isinstance(v, ConvOp) and v.stride == 2 and v.KW == 4 for v in resamplers)
        s2 = {m for s, m, _, _ in fwd if s == 2}
        # forward only: downs gather forward (0), up-convs transposed (1); a training pass adds each one's dgrad in the other mode
        assert s2 == {0, 1}, s2
        if train:
            n_s2 = sum(1 for s, *_ in fwd if s == 2)
            assert n_s2 == 4 * U.levels(case), n_s2                            # each resampler: one forward, one dgrad
            assert {m for s, m, _, _ in wgrad if s == 2} == {0, 1}
    if case in ("B", "C"):
        assert max(p for _, _, p, _ in fwd + wgrad) == lens[0] < 64             # no halo-tile kernel anywhere in the net
    if case == "D":
        assert lens[-1] == 1 and sum(1 for s, _, p, kw in fwd if p == 1 and kw == 3 and s == 1) >= 2   # the middle block
    if case == "F":
        assert lens == [256, 128, 64, 32]
    assert bool(train) == bool(wgrad)


def _triple(per, grads, case):
    """(per-sample loss, flat gradient, worst tensor relative to its own norm) against float64, for the HIP result and for the
    float32 oracle."""
    per32, g32 = U.oracle(case, torch.float32)
    per64, g64 = U.oracle(case, torch.float64)
    keys = list(g64)
    cat = lambda g: torch.cat([g[k].reshape(-1).double().cpu() for k in keys])   # noqa: E731
    wt = lambda g: max((float((g[k].double().cpu() - g64[k]).norm()) / float(g64[k].norm()), k) for k in keys)   # noqa: E731
    return ((rel_l2(per.cpu(), per64), rel_l2(cat(grads), cat(g64)), wt(grads)),
            (rel_l2(per32, per64), rel_l2(cat(g32), cat(g64)), wt(g32)))


@pytest.mark.parametrize("case", list(U.CASES))
def test_training_pass_vs_float64_oracle(case, monkeypatch):
    """SSM loss and every parameter gradient at the yardstick's default slack (2 x the float32 oracle's own distance from
    float64 for the loss and the flat gradient, 4 x for the worst tensor), floor_frac = 1e-4, on the route the case names.
    Measured on an MI355X as multiples of the float32 oracle's own distance (loss / flat gradient / worst tensor relative to
    its own norm; profiles/unet1d_deep/parity_measured.txt): A 1.34 / 1.80 / 1.77, B 0.56 / 1.47 / 1.56, C 1.35 / 1.69 / 1.78,
    D 1.24 / 1.59 / 1.46, E 2.51 / 1.35 / 1.42, F 0.59 / 1.34 / 1.39, G 1.78 / 0.49 / 0.65; every absolute figure is under
    8e-6.  E's loss (5.4e-7 against the float32 oracle's 2.2e-7 over three samples of eight positions) is the one figure over
    its multiple; it passes on the yardstick's absolute floor of 1e-5, and every kernel call of E's training step replayed
    through the layer census lies within its bounds (profiles/unet1d_deep/census_caseE.txt).  No slack was raised."""
    from test_round2_gpu import ssm_parity_vs_fp64
    c = U.CASES[case]
    net = _net(case)
    gen = make_gen("sgm", net)
    x, u, eps, uv = U.draws(case)
    fwd, wgrad = _spy(monkeypatch)
    what = f"case {case}: UNet1D L={c['L']} B={c['B']} levels {level_lengths(c['L'], U.levels(case))}"
    ssm_parity_vs_fp64(gen, U.score(case), U.params(case), x, u, eps, uv, what, floor_frac=U.FLOOR_FRAC)
    _routes_ok(case, net, fwd, wgrad, train=True)
    gen.zero_grad()
    per = gen.ssm(x.to(DEV), u=u.to(DEV), eps=eps.to(DEV), u_v=uv.to(DEV))
    per.mean().backward()
    h, r = _triple(per.detach(), {k: p.grad.detach() for k, p in net.named_parameters()}, case)
    print(f"MEASURED case {case}: loss {h[0]:.2e} ({h[0] / r[0]:.2f} x float32 oracle {r[0]:.2e}) | flat gradient {h[1]:.2e} "
          f"({h[1] / r[1]:.2f} x {r[1]:.2e}) | worst tensor vs its own norm {h[2][0]:.2e} {h[2][1]} ({h[2][0] / r[2][0]:.2f} x "
          f"{r[2][0]:.2e} {r[2][1]})")


@pytest.mark.parametrize("case", ["B", "C"])
def test_golden_digests(case):
    """Per-sample loss and gradient digest against the reference's own float32 run (g22_unet1d_deep), as
    test_unet1d_ssm_golden does at L = 256.  Tolerances by the triangle inequality from the yardstick: the recorded run is
    itself a float32 evaluation, d away from float64 in the same metric (computed here from the float64 oracle), and the HIP
    path may be 2 d (loss) / 4 d (worst tensor) away from float64, so 3 d / 5 d from the record; d is floored at 1e-6, the
    digest's own resolution (heads are stored in float32)."""
    g = load_golden("g22_unet1d_deep")
    net = _net(case)
    gen = make_gen("sgm", net)
    gen.zero_grad()
    per = gen.ssm(g[f"{case}_x"].to(DEV), u=g[f"{case}_u_t"].reshape(-1).to(DEV), eps=g[f"{case}_eps"].to(DEV),
                  u_v=g[f"{case}_u_v"].to(DEV))
    per.mean().backward()
    per64, g64 = U.oracle(case, torch.float64)
    d_per = max(rel_l2(g[f"{case}_per"], per64), 1e-6)
    e_per = rel_l2(per.detach().cpu(), g[f"{case}_per"])
    print(f"case {case}: per-sample loss vs the reference {e_per:.2e} (the reference from float64: {d_per:.2e})")
    assert e_per <= 3 * d_per
    d_dig = max(check_digest(g, case, g64, "a.", 1.0), 1e-6)                    # the record's own deviation from float64
    check_digest(g, case, {k: p.grad.cpu() for k, p in net.named_parameters()}, "a.", 5 * d_dig)


@pytest.mark.parametrize("case", list(U.CASES))
def test_sampler_forward_vs_float64_oracle(case, monkeypatch):
    """The no-tangent forward at 5 rows: no further from the float64 oracle than 2 x the float32 oracle."""
    net = _net(case)
    x, t = U.forward_draws(case)
    p = U.params(case)
    fwd, wgrad = _spy(monkeypatch)
    y = net(x.to(DEV), t.to(DEV)).cpu()
    _routes_ok(case, net, fwd, wgrad, train=False)
    with torch.no_grad():
        r32 = U.score(case)(p, x, t)
        r64 = U.score(case)({k: w.double() for k, w in p.items()}, x.double(), t.double())
    e, e32 = rel_l2(y, r64), rel_l2(r32, r64)
    print(f"case {case} forward, 5 rows: rel-L2 vs the float64 oracle {e:.2e} | float32 oracle {e32:.2e}")
    assert bool(torch.isfinite(y).all()) and e <= max(2 * e32, 1e-6), (e, e32)


@pytest.mark.parametrize("case", ["B", "D", "E"])
def test_one_net_trained_then_called_at_another_batch_size(case):
    """The ops, weight images and embedding work buffers are cached on the net: after a training pass (6 dual rows) a forward
    at 5 rows and then at 2 rows gives the bits of a fresh net that never trained."""
    x, t = U.forward_draws(case)
    fresh = _net(case)
    want5, want2 = fresh(x.to(DEV), t.to(DEV)).clone(), fresh(x[:2].to(DEV), t[:2].to(DEV)).clone()
    net = _net(case)
    gen = make_gen("sgm", net)
    xs, u, eps, uv = U.draws(case)
    gen.ssm(xs.to(DEV), u=u.to(DEV), eps=eps.to(DEV), u_v=uv.to(DEV)).mean().backward()
    got5 = net(x.to(DEV), t.to(DEV)).clone()
    got2 = net(x[:2].to(DEV), t[:2].to(DEV)).clone()
    assert bool(torch.isfinite(got5).all()) and torch.equal(got5, want5) and torch.equal(got2, want2)
    assert torch.equal(want5[:2], want2)                       # and a row does not depend on how many rows ran with it


def test_euler_maruyama_sampler_vs_float64_oracle():
    """euler_maruyama_sampler, 6 steps with injected noise, case B (L = 37), 5 rows: no further from the float64 oracle's
    trajectory end than 2 x the float32 oracle's."""
    from oracle import sde_ref as S
    from sdeflow_light_amd import sde_scheme as SS
    case = "B"
    L = U.CASES[case]["L"]
    gen = make_gen("sgm", _net(case))
    torch.manual_seed(2000 + L)
    x0, z = torch.randn(5, L), torch.randn(6, 5, L)
    xs = SS.euler_maruyama_sampler(gen, x0.to(DEV), num_steps=6, keep_all_samples=False, noise=z)
    p = U.params(case)
    p64 = {k: w.double() for k, w in p.items()}
    sc = U.score(case)
    with torch.no_grad():
        r32 = S.euler_maruyama(S.ReverseProcess(S.SdeSpec(), lambda y, s: sc(p, y, s)), x0, 6, z)
        r64 = S.euler_maruyama(S.ReverseProcess(S.SdeSpec(), lambda y, s: sc(p64, y, s)), x0.double(), 6, z.double())
    e, e32 = rel_l2(xs.cpu(), r64), rel_l2(r32, r64)
    print(f"MEASURED sampler case {case}: 6 Euler-Maruyama steps, 5 rows: rel-L2 vs the float64 oracle {e:.2e} | float32 oracle {e32:.2e}")
    assert bool(torch.isfinite(xs).all()) and e <= 2 * e32, (e, e32)


def test_multiplicative_sde_vs_float64_oracle():
    """make_gen("sparse", n = 37, nsf = 4) with case C's net through the general (u, cst) loss form, as
    test_ssm_unet1d_msgm_sparse_vs_oracle does at L = 64 — with the yardstick instead of a fixed tolerance."""
    from oracle import sde_ref as S, ssm_ref as LR
    case = "C"
    L, B = U.CASES[case]["L"], U.CASES[case]["B"]
    net = _net(case)
    torch.manual_seed(3000 + L)
    gen = make_gen("sparse", net, n=L, nsf=4)
    t, y, uv = torch.rand(B, 1).clamp_min(1e-3), torch.randn(B, L), torch.rand(B, L)
    sp = S.SdeSpec(kind=S.MSGM_SPARSE, n=L)
    v = S.rademacher_from_uniform(uv)
    p = U.params(case)

    def hip():
        gen.zero_grad()
        per = gen.ssm_loss(t.to(DEV), y.to(DEV), y.to(DEV), u_v=uv.to(DEV))
        per.mean().backward()
        return per.detach(), {k: q.grad.detach() for k, q in net.named_parameters()}

    def oracle(dt):
        _, per, g = LR.ssm_mean_and_grads(sp, U.score(case), {k: w.to(dt) for k, w in p.items()}, t.to(dt), y.to(dt), v.to(dt))
        return per, g
    parity_vs_fp64(hip, oracle, f"multiplicative SDE (sparse) + case {case}", floor_frac=U.FLOOR_FRAC)


def test_trainer_graph_replay_equals_eager():
    """Case B, 4 steps: the zero-padded up-conv outputs are allocated inside the captured step.  The graphed trainer's losses
    and parameters equal the eager trainer's bit for bit, and the parameters moved."""
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    from sdeflow_light_amd.train import UNetScoreTrainer
    case = "B"
    B, d = U.CASES[case]["B"], U.CASES[case]["L"]
    out = {}
    for use_graph in (False, True):
        net = _net(case)
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
    print(f"case {case} graph replay vs eager: losses {out[True][0]} vs {out[False][0]}")
    assert all(l == l and abs(l) != float("inf") for l in out[True][0])
    assert out[True][0] == out[False][0]
    assert torch.equal(out[True][1], out[False][1])
