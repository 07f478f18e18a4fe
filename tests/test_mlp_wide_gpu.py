"""The MLP score net at 31 <= d <= 128 — the extra-wide class of the fused kernel (k_mlp_xw) — against the reference's
own numbers (tests/golden/g20_mlp_wide.npz, weights rebuilt by oracle.det_params) and the float64 oracle: forward,
the fused SSM training pass (SGM closed form and the general u / cst form), the EM step and whole-loop sampler, and
the graph-replayed trainer."""
import pytest
import torch

from conftest import load_golden, rel_l2, within, check_digest, parity_vs_fp64
from oracle import sde_ref as S, nets_ref as N, ssm_ref as LR
from oracle.det_params import load_init_like_

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRE = "NormalizeLogRadius"


def Tp():
    return torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)


def make_net(d, pre=None):
    from sdeflow_light_amd.NN import MLP
    net = MLP(d, premodule=pre)
    load_init_like_(net)
    return net


def make_gen(net, kind="sgm", nsf=16, x_init=None, G=None):
    from sdeflow_light_amd.SDEs import SGMsde, MSGMsde, PluginReverseSDE
    T = Tp()
    if kind == "sgm":
        base = SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=nsf, device=DEV)
    else:
        base = MSGMsde(x_init, beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=nsf, device=DEV,
                       denseTensor=(kind == "dense"), norm_map="log", G=G)
    return PluginReverseSDE(base, net.to(DEV), T, deviceReverseSDE=DEV).to(DEV)


def params_of(net, dtype=torch.float64):
    return {k: v.detach().cpu().to(dtype) for k, v in net.state_dict().items()}


@pytest.mark.parametrize("tag,d,pre", [("f31", 31, None), ("f32", 32, None), ("f64n", 64, PRE), ("f128", 128, None)])
def test_forward_golden(tag, d, pre):
    g = load_golden("g20_mlp_wide")
    net = make_net(d, pre).to(DEV)
    out = net(g[tag + "_x"].to(DEV), g[tag + "_t"].to(DEV))
    within(rel_l2(out.cpu(), g[tag + "_out"]), 1e-5, f"MLP({d}, {pre}) forward vs the reference")


@pytest.mark.parametrize("d,pre", [(31, None), (37, PRE), (100, None), (127, PRE)])
@pytest.mark.parametrize("B", [1, 33, 1000, 9001])
def test_forward_fp64_oracle(d, pre, B):
    """B = 9001: 282 tiles of 32 on a grid of 256, so workgroups carry a second tile through the pipeline."""
    torch.manual_seed(d * 1000 + B)
    net = make_net(d, pre).to(DEV)
    x, t = torch.randn(B, d) * 1.5, torch.rand(B)
    out = net(x.to(DEV), t.to(DEV)).cpu()
    ref = N.mlp_forward(params_of(net), x.double(), t.double(), premodule=pre)
    assert torch.isfinite(out).all()
    within(rel_l2(out, ref), 1e-5, f"MLP({d}, {pre}) forward at B={B} vs the float64 oracle")


def test_ssm_golden_d32():
    """ssm(x).mean().backward() at d = 32 against the reference's double backward, at the narrow tests' bounds."""
    g = load_golden("g20_mlp_wide")
    gen = make_gen(make_net(32))
    gen.zero_grad()
    per = gen.ssm(g["s32_x"].to(DEV), u=g["s32_u_t"].reshape(-1).to(DEV), eps=g["s32_eps"].to(DEV), u_v=g["s32_u_v"].to(DEV))
    assert rel_l2(per.detach().cpu(), g["s32_per"]) <= 1e-5
    per.mean().backward()
    within(max(rel_l2(p.grad.cpu(), g[f"s32_grad::{k}"]) for k, p in gen.named_parameters() if p.requires_grad), 5e-7,
           "MLP(32): worst per-tensor gradient rel-L2 vs the reference's double backward")


def test_ssm_golden_d128_premodule():
    g = load_golden("g20_mlp_wide")
    gen = make_gen(make_net(128, PRE))
    gen.zero_grad()
    t = "s128n"
    per = gen.ssm(g[t + "_x"].to(DEV), u=g[t + "_u_t"].reshape(-1).to(DEV), eps=g[t + "_eps"].to(DEV), u_v=g[t + "_u_v"].to(DEV))
    assert rel_l2(per.detach().cpu(), g[t + "_per"]) <= 1e-5
    per.mean().backward()
    check_digest(g, t, {k: p.grad.cpu() for k, p in gen.named_parameters() if p.grad is not None}, "", 1e-5)


@pytest.mark.parametrize("d,pre,B", [(32, None, 200), (128, PRE, 100), (32, None, 5000), (128, PRE, 5000)])
def test_ssm_parity_vs_fp64(d, pre, B):
    """The fused training pass against the float64 oracle at conftest.parity_vs_fp64's default slack.  B = 5000 is 313
    tiles of 16 on a grid of 256: workgroups take a second tile, which runs the cross-tile paths (dW1 / dW4 extended
    through the slab, dW2 / dW3 / bias sums carried in registers, the next tile's inputs, h0 and layer 1 built ahead)."""
    torch.manual_seed(d + B)
    net = make_net(d, pre)
    gen = make_gen(net)
    p0 = params_of(net, torch.float32)
    x, u, eps, uv = torch.randn(B, d) * 1.5, torch.rand(B), torch.randn(B, d), torch.rand(B, d)
    sp = S.SdeSpec()

    def hip():
        gen.zero_grad()
        per = gen.ssm(x.to(DEV), u=u.to(DEV), eps=eps.to(DEV), u_v=uv.to(DEV))
        per.mean().backward()
        return per.detach().cpu(), {k[2:]: p.grad.detach().cpu() for k, p in gen.named_parameters() if p.requires_grad}

    def oracle(dt):
        t = S.clamp_time(sp, u.reshape(B, 1).to(dt))
        y = S.vp_perturb(sp, t, x.to(dt), eps.to(dt))
        v = S.rademacher_from_uniform(uv.to(dt))
        _, per, gr = LR.ssm_mean_and_grads(sp, lambda prm, yy, tt: N.mlp_forward(prm, yy, tt, premodule=pre),
                                           {k: w.to(dt) for k, w in p0.items()}, t, y, v)
        return per, gr

    parity_vs_fp64(hip, oracle, f"MLP({d}, {pre}) fused SSM pass, B={B}")


@pytest.mark.parametrize("B", [96, 5000])
def test_ssm_gaussian_probe_vs_oracle(B):
    """A Gaussian probe takes the general (u, cst) form of the loss (B = 5000: two tiles per workgroup)."""
    torch.manual_seed(5)
    d = 48
    net = make_net(d)
    gen = make_gen(net)
    x, u, eps, v = torch.randn(B, d) * 1.5, torch.rand(B), torch.randn(B, d), torch.randn(B, d)
    gen.zero_grad()
    per = gen.ssm(x.to(DEV), u=u.to(DEV), eps=eps.to(DEV), v=v.to(DEV))
    per.mean().backward()
    sp = S.SdeSpec()
    t = S.clamp_time(sp, u.reshape(B, 1).double())
    y = S.vp_perturb(sp, t, x.double(), eps.double())
    _, per64, g64 = LR.ssm_mean_and_grads(sp, lambda prm, yy, tt: N.mlp_forward(prm, yy, tt), params_of(net), t, y, v.double())
    within(rel_l2(per.detach().cpu(), per64), 1e-5, "Gaussian probe: per-sample loss vs the float64 oracle")
    within(max(rel_l2(p.grad.cpu(), g64[k[2:]]) for k, p in gen.named_parameters() if p.requires_grad), 1e-4,
           "Gaussian probe: worst per-tensor gradient vs the float64 oracle")


@pytest.mark.parametrize("tag,d,kind", [("m32d", 32, "dense"), ("m128s", 128, "sparse")])
def test_ssm_msgm_golden(tag, d, kind):
    """ssm_loss(t, x, y) of the multiplicative SDE (general form of the fused loss) against the reference."""
    g = load_golden("g20_mlp_wide")
    gen = make_gen(make_net(d), kind, nsf=4, x_init=g[tag + "_x_init"], G=g.get(tag + "_G"))
    gen.zero_grad()
    per = gen.ssm_loss(g[tag + "_t"].to(DEV), g[tag + "_y"].to(DEV), g[tag + "_y"].to(DEV), u_v=g[tag + "_u_v"].to(DEV))
    within(rel_l2(per.detach().cpu(), g[tag + "_per"]), 2e-5, f"MSGM {kind} d={d}: per-sample loss vs the reference")
    per.mean().backward()
    check_digest(g, tag, {k: p.grad.cpu() for k, p in gen.named_parameters() if p.grad is not None}, "", 3e-4)


@pytest.mark.parametrize("B", [40, 4500])
def test_ssm_msgm_dense_d64_vs_fp64(B):
    """MSGM dense tensor at d = 64 (the general u / cst form of the fused loss) against the float64 oracle of
    ssm_loss(t, x, y), at conftest.parity_vs_fp64's default slack; B = 4500 gives workgroups a second tile."""
    torch.manual_seed(64)
    d = 64
    net = make_net(d)
    gen = make_gen(net, "dense", nsf=4, x_init=torch.randn(64, d) * 1.5)
    G = gen.base_sde.G.detach().cpu()
    p0 = params_of(net, torch.float32)
    t = torch.rand(B, 1).clamp_min(1e-3)
    y = torch.randn(B, d) * 1.3
    uv = torch.rand(B, d)

    def hip():
        gen.zero_grad()
        per = gen.ssm_loss(t.to(DEV), y.to(DEV), y.to(DEV), u_v=uv.to(DEV))
        per.mean().backward()
        return per.detach().cpu(), {k[2:]: p.grad.detach().cpu() for k, p in gen.named_parameters() if p.grad is not None}

    def oracle(dt):
        sp = S.SdeSpec(kind=S.MSGM_DENSE, n=d, num_steps_forward=4, G=G.to(dt))
        _, per, gr = LR.ssm_mean_and_grads(sp, lambda prm, yy, tt: N.mlp_forward(prm, yy, tt),
                                           {k: w.to(dt) for k, w in p0.items()}, t.to(dt), y.to(dt),
                                           S.rademacher_from_uniform(uv.to(dt)))
        return per, gr

    parity_vs_fp64(hip, oracle, f"MSGM dense d={d}, B={B}")


@pytest.mark.parametrize("d,pre", [(32, None), (128, PRE)])
def test_em_loop_equals_per_step_kernels(d, pre):
    from sdeflow_light_amd import ops
    torch.manual_seed(d)
    B, N = 1000, 6
    gen = make_gen(make_net(d, pre))
    base = gen.base_sde
    P, st = gen.a.kernel_params(), base.struct()
    T = base.T_float()
    ts = torch.linspace(0, 1, N + 1) * T
    delta = T / N
    x0 = torch.randn(B, d, device=DEV)
    rng = base.philox(DEV)
    ref = x0.clone()
    for i in range(N):
        ops.mlp_em_step(P, ref, st, ts[i].item(), delta, 0.0, rng=rng, rng_step=i)
    one = x0.clone()
    ops.mlp_em_loop(P, one, st, ts.to(DEV), delta, 0.0, rng, 0)
    assert torch.isfinite(one).all()
    within(rel_l2(one.cpu(), ref.cpu()), 1e-6, f"d={d}: one-launch EM loop vs {N} single-step launches")


@pytest.mark.parametrize("d,pre,lmbd", [(32, None, 0.0), (100, PRE, 0.5)])
def test_em_step_vs_oracle(d, pre, lmbd):
    """One fused reverse EM step against the float64 reverse step (SDEs.py:556-561,587-588; sde_scheme.py:38-40)."""
    from sdeflow_light_amd import ops
    torch.manual_seed(7 + d)
    B = 333
    net = make_net(d, pre)
    gen = make_gen(net)
    base = gen.base_sde
    x = torch.randn(B, d)
    z = torch.randn(B, d)
    t, delta = 0.3, 1.0 / 16
    out = ops.mlp_em_step(gen.a.kernel_params(), x.clone().to(DEV), base.struct(), t, delta, lmbd, z=z.to(DEV)).cpu()
    sp = S.SdeSpec()
    s = torch.full((B, 1), 1.0 - t, dtype=torch.float64)
    beta = S.beta(sp, s)
    a = N.mlp_forward(params_of(net), x.double(), s.reshape(-1), premodule=pre)
    mu = (1 - 0.5 * lmbd) * beta.sqrt() * a + 0.5 * beta * x.double()
    ref = x.double() + mu * delta + (1 - lmbd) ** 0.5 * beta.sqrt() * delta ** 0.5 * z.double()
    within(rel_l2(out, ref), 1e-6, f"d={d}: fused EM step vs the float64 reverse step")


def _trainer(d, B, use_graph, seed=3, row_base=0, x=None):
    from sdeflow_light_amd.train import MLPScoreTrainer
    torch.manual_seed(0)
    gen = make_gen(make_net(d))
    tr = MLPScoreTrainer(gen, B, lr=1e-3, use_graph=use_graph, seed=seed, row_base=row_base)
    tr.set_data(x if x is not None else torch.randn(B, d, device=DEV))
    return tr


@pytest.mark.parametrize("d", [32, 128])
def test_trainer_graph_equals_eager_bitwise(d):
    torch.manual_seed(1)
    x = torch.randn(5000, d, device=DEV)            # two tiles per workgroup
    outs = []
    for use_graph in (False, True):
        tr = _trainer(d, 5000, use_graph, x=x)
        losses = [float(tr.step()) for _ in range(4)]
        outs.append((losses, tr.flat.clone()))
    assert all(abs(l) < 1e6 for l in outs[0][0])
    assert outs[0][0] == outs[1][0]
    assert torch.equal(outs[0][1], outs[1][1])


def test_trainer_runs_are_bitwise_reproducible():
    torch.manual_seed(2)
    x = torch.randn(6007, 64, device=DEV)           # ragged, two tiles per workgroup
    runs = []
    for _ in range(2):
        tr = _trainer(64, 6007, True, x=x)
        losses = [float(tr.step()) for _ in range(3)]
        runs.append((losses, tr.flat.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])


def test_trainer_row_base_shards_reproduce_the_full_run():
    """Two 32-row shards (row_base = 0, 32) draw what the 64-row run draws for their rows, and the mean of their
    gradients is the 64-row run's gradient."""
    d = 40
    torch.manual_seed(3)
    x = torch.randn(64, d, device=DEV)
    full = _trainer(d, 64, False, x=x)
    lf = float(full.step())
    shards = [_trainer(d, 32, False, row_base=b, x=x[b:b + 32].contiguous()) for b in (0, 32)]
    ls = [float(s.step()) for s in shards]
    for i, s in enumerate(shards):
        rows = slice(32 * i, 32 * i + 32)
        assert torch.equal(s.y, full.y[rows]) and torch.equal(s.t, full.t[rows]) and torch.equal(s.vp, full.vp[rows])
    assert (ls[0] + ls[1]) / 2 == pytest.approx(lf, rel=1e-6)
    gmean = 0.5 * (shards[0].gflat + shards[1].gflat)
    within(rel_l2(gmean.cpu(), full.gflat.cpu()), 1e-6, "mean of the two shards' gradients vs the 64-row run")


def test_three_train_steps_golden():
    """3 SSM + Adam steps at d = 32 against the reference's loss sequence and final parameters (g20, as g11)."""
    from sdeflow_light_amd.optim import FusedAdam
    g = load_golden("g20_mlp_wide")
    gen = make_gen(make_net(32))
    opt = FusedAdam(gen.parameters(), lr=1e-3)
    for i in range(3):
        opt.zero_grad()
        loss = gen.ssm(g["tr_x"][i].to(DEV), u=g["tr_u_t"][i].reshape(-1).to(DEV), eps=g["tr_eps"][i].to(DEV),
                       u_v=g["tr_u_v"][i].to(DEV)).mean()
        loss.backward()
        opt.step()
        assert float(loss.detach()) == pytest.approx(float(g["tr_loss"][i]), rel=2e-5)
    sd = {k: v.cpu() for k, v in gen.state_dict().items() if k.startswith("a.")}
    check_digest(g, "tr_final", sd, "", 2e-5)
