"""The time-integrated SSM loss, PluginReverseSDE(ssm_intT=True): the one-launch path kernel (msgm_forward_paths, the
all-times mode of csrc/sde_forward_kernels.hip), ssm() / sample_txy() / evaluate on the nsf' B time-major rows, and the
trainers.

Kernel vs composed (sde_scheme.msgm_forward_paths_composed: the RK4 sampler on forward_SDE with every state kept) is
BITWISE: both evaluate the functions of csrc/sde_stage.h in the same order under -ffp-contract=off.  The kernel's output is
pre-filled with NaN and asserted finite over its whole extent; the parity cases call the C entry on their own buffer.

Shape -> kernel (launch conditions of msgm_forward_paths, those of msgm_forward_perturb):
  sparse n <= 256            lane groups: (1,1) (5,3) (5,6) scalar body, (33,8) (67,36) float4 body and several workgroups,
                             (2,256) the regime's last n
  sparse 256 < n <= 4096     workgroup, 4 elements per thread: (2,257) first n, (2,4096) last n
  sparse 4096 < n <= 12288   workgroup, 16 elements per thread: (2,4100) first n, (2,12288) the supported bound
  dense n <= 16 / n <= 64    G in LDS: 2, 7, 16; G through L2: 17, 64; B 1 and 9
first_keep 0, 1 and nsf - 1 in every case (nsf = 1 has 0 only)."""
import math

import pytest
import torch

import sde_stage_ref as R
import ssm_intT_ref as IR
from conftest import load_golden, rel_l2, within

pytestmark = pytest.mark.gpu
DEV = "cuda"
T_END, T_EPS = 1.0, 1e-3


@pytest.fixture(scope="module")
def ops():
    from sdeflow_light_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def L():
    from sdeflow_light_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def SS():
    from sdeflow_light_amd import sde_scheme
    return sde_scheme


def Tp():
    return torch.nn.Parameter(torch.FloatTensor([T_END]), requires_grad=False)


_BASES = {}


def make_base(kind, n, nsf):
    from sdeflow_light_amd.SDEs import MSGMsde
    key = (kind, n, nsf)
    if key not in _BASES:
        g = torch.Generator().manual_seed(n)
        G = R.dense_G(n)[0] if kind == "dense" else None
        _BASES[key] = MSGMsde(torch.randn(64, n, generator=g), beta_min=R.B0, beta_max=R.B1, t_epsilon=T_EPS, T=Tp(),
                              num_steps_forward=nsf, device=DEV, denseTensor=(kind == "dense"), norm_map="log", G=G).to(DEV)
    return _BASES[key]


def c_forward_paths(L, SS, base, x0, first_keep, zm=None, rng=None):
    """msgm_forward_paths through the C ABI on a NaN-filled y_all, asserted finite everywhere."""
    B, n = x0.shape
    nsf = base.num_steps_forward
    ts, delta = SS._forward_grid(base, nsf, x0.device)
    y = torch.full((nsf - first_keep, B, n), float("nan"), device=DEV)
    L.check(L.lib().msgm_forward_paths(L.ptr(x0), L.ptr(y), B, n, base.struct(), nsf, first_keep, L.ptr(ts), float(delta),
                                       float(delta ** 0.5), float(delta * 0.5), float(delta * 1.0), L.ptr(zm),
                                       None if rng is None else rng.ptr(), L.stream()), "msgm_forward_paths")
    assert bool(torch.isfinite(y).all()), "the kernel left part of y_all unwritten (or not finite)"
    return y


def parity_case(ops, L, SS, kind, B, n, nsf):
    base = make_base(kind, n, nsf)
    assert ops.forward_perturb_supported(base.kind, n)
    gen = torch.Generator().manual_seed(1000 * n + 10 * B + nsf)
    x0 = (torch.randn(B, n, generator=gen) * 1.5).to(DEV)
    zm = torch.randn(nsf, B, n, generator=gen).to(DEV)
    grid = SS._forward_grid(base, nsf, x0.device)
    for fk in sorted({0, 1, nsf - 1} & set(range(nsf))):
        tag = (kind, B, n, nsf, fk)
        # injected noise
        want = SS.msgm_forward_paths_composed(base, x0, fk, zm)
        assert want.shape == (nsf - fk, B, n) and want.is_cuda
        got = c_forward_paths(L, SS, base, x0, fk, zm)
        assert torch.equal(got, want), (tag, "injected", float((got - want).abs().max()))
        assert torch.equal(ops.forward_paths(x0, base.struct(), nsf, fk, *grid, z_main=zm), got)
        # Philox: composed, the kernel on its own buffer, and the public function, each from the same stream state
        base.rng = L.PhiloxState(4242 + fk, DEV, offset=5)
        s0 = base.rng.state.clone()
        want = SS.msgm_forward_paths_composed(base, x0, fk)
        s_composed = base.rng.state.clone()
        base.rng.state.copy_(s0)
        got = c_forward_paths(L, SS, base, x0, fk, rng=base.rng)
        assert torch.equal(base.rng.state, s0)                       # the C entry reads the stream, the caller advances it
        assert torch.equal(got, want), (tag, "philox", float((got - want).abs().max()))
        got2 = SS.msgm_forward_paths(base, x0, fk)
        assert torch.equal(got2, want) and got2.is_cuda
        assert torch.equal(base.rng.state, s_composed)
        assert int(s_composed[1]) - int(s0[1]) == nsf and torch.equal(s_composed[[0, 2, 3]], s0[[0, 2, 3]])


SPARSE_SMALL = [(1, 1), (5, 3), (5, 6), (33, 8), (67, 36), (2, 256)]
SPARSE_LONG = [(2, 257), (2, 4096), (2, 4100), (2, 12288)]


@pytest.mark.parametrize("nsf", [1, 4, 16])
@pytest.mark.parametrize("B,n", SPARSE_SMALL)
def test_sparse_small_bitwise_equals_composed(ops, L, SS, B, n, nsf):
    parity_case(ops, L, SS, "sparse", B, n, nsf)


@pytest.mark.parametrize("B,n", SPARSE_LONG)
def test_sparse_long_bitwise_equals_composed(ops, L, SS, B, n):
    parity_case(ops, L, SS, "sparse", B, n, 4)


@pytest.mark.parametrize("nsf", [1, 4, 16])
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("n", [2, 7, 16, 17, 64])
def test_dense_bitwise_equals_composed(ops, L, SS, n, B, nsf):
    parity_case(ops, L, SS, "dense", B, n, nsf)


def test_routing(ops, L, SS, monkeypatch):
    """The public function takes the kernel where supported and aligned, the composed chain otherwise; same bits."""
    calls = []
    real = ops.forward_paths

    def rec(*a, **kw):
        calls.append(a[0].shape)
        return real(*a, **kw)
    monkeypatch.setattr(ops, "forward_paths", rec)
    nsf = 4
    base = make_base("sparse", 8, nsf)
    gen = torch.Generator().manual_seed(0)
    x0, zm = torch.randn(33, 8, generator=gen).to(DEV), torch.randn(nsf, 33, 8, generator=gen).to(DEV)
    want = SS.msgm_forward_paths_composed(base, x0, 1, zm)
    assert calls == []
    assert torch.equal(SS.msgm_forward_paths(base, x0, 1, zm), want) and len(calls) == 1
    with monkeypatch.context() as m:
        m.setattr(ops, "forward_perturb_supported", lambda kind, n: False)
        assert torch.equal(SS.msgm_forward_paths(base, x0, 1, zm), want) and len(calls) == 1
    view = torch.zeros(33 * 8 + 1, device=DEV)[1:].view(33, 8)           # 4-byte aligned only
    view.copy_(x0)
    assert torch.equal(SS.msgm_forward_paths(base, view, 1, zm), want) and len(calls) == 1
    big = make_base("sparse", 12292, 1)                                   # past the bound
    xb, zb = torch.randn(1, 12292, generator=gen).to(DEV), torch.randn(1, 1, 12292, generator=gen).to(DEV)
    got = SS.msgm_forward_paths(big, xb, 0, zb)
    assert len(calls) == 1 and bool(torch.isfinite(got).all())
    from sdeflow_light_amd.SDEs import SGMsde                             # the additive SDE: composed only
    sgm = SGMsde(T=Tp(), num_steps_forward=nsf, device=DEV).to(DEV)
    got = SS.msgm_forward_paths(sgm, x0, 0, zm)
    assert len(calls) == 1 and got.shape == (nsf, 33, 8) and bool(torch.isfinite(got).all())
    with pytest.raises(L.MsgmError):
        SS.msgm_forward_paths(base, x0, nsf, zm)


def test_c_entry_refusals(L):
    BADARG = -1
    nsf = 4
    lib = L.lib()
    ts = (torch.linspace(0, 1, nsf + 1) * T_END).to(DEV)
    rng = L.PhiloxState(1, DEV)

    def rc(st, x0, y, n, zm, rng, ts, fk=0, B=2):
        return lib.msgm_forward_paths(L.ptr(x0), L.ptr(y), B, n, st, nsf, fk, L.ptr(ts), 0.25, 0.5, 0.125, 0.25, L.ptr(zm),
                                      None if rng is None else rng.ptr(), L.stream())

    def bufs(n):
        return torch.zeros(2, n, device=DEV), torch.zeros(nsf, 2, n, device=DEV), torch.zeros(nsf, 2, n, device=DEV)

    sparse = L.sde_struct(L.SDE_MSGM_SPARSE, R.B0, R.B1, T_END, T_EPS)
    x, y, zm = bufs(8)
    assert rc(sparse, x, y, 8, zm, None, ts) == L.MSGM_OK
    assert rc(sparse, x, y, 8, None, rng, ts, fk=3) == L.MSGM_OK
    assert rc(L.sde_struct(L.SDE_SGM, R.B0, R.B1, T_END, T_EPS), x, y, 8, zm, rng, ts) == L.MSGM_E_UNSUPPORTED
    assert rc(sparse, x, y, 8, None, None, ts) == BADARG                          # neither noise nor a stream
    assert rc(sparse, x, y, 8, zm, rng, None) == BADARG                           # no time grid
    assert rc(sparse, None, y, 8, zm, rng, ts) == BADARG and rc(sparse, x, None, 8, zm, rng, ts) == BADARG
    assert rc(None, x, y, 8, zm, rng, ts) == BADARG
    assert rc(sparse, x, y, 8, zm, rng, ts, fk=nsf) == BADARG and rc(sparse, x, y, 8, zm, rng, ts, fk=-1) == BADARG
    assert rc(sparse, x, y, 8, zm, rng, ts, B=0) == BADARG
    # overlap: x0 inside y_all, at its start and in its last kept slab
    assert rc(sparse, y[0], y, 8, zm, rng, ts) == BADARG
    assert rc(sparse, y[nsf - 1], y, 8, zm, rng, ts) == BADARG
    assert rc(sparse, y[nsf - 1], y, 8, zm, rng, ts, fk=1) == L.MSGM_OK           # (3, B, n) kept: the last slab is outside
    assert rc(L.sde_struct(L.SDE_MSGM_DENSE, R.B0, R.B1, T_END, T_EPS), x, y, 8, zm, rng, ts) == BADARG      # no tensor
    x, y, zm = bufs(12292)
    assert rc(sparse, x, y, 12292, zm, rng, ts) == L.MSGM_E_UNSUPPORTED
    torch.cuda.synchronize()


# ------------------------------------------------------------------ ssm() / sample_txy() / evaluate against g24
B_G, NSF_G = 3, 4
FAMILIES = {"sg": ("sgm", 2, None), "sp": ("sparse", 6, "NormalizeLogRadius"), "dn": ("dense", 4, None)}


@pytest.fixture(scope="module")
def g():
    return load_golden("g24_ssm_intT")


def golden_gen(g, tag, t_eps, ssm_intT=True):
    from oracle.det_params import load_det_
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.SDEs import MSGMsde, PluginReverseSDE, SGMsde
    kind, d, pre = FAMILIES[tag]
    T = Tp()
    if kind == "sgm":
        base = SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=t_eps, T=T, num_steps_forward=NSF_G, device=DEV)
    else:
        base = MSGMsde(g[tag + "_y0"], beta_min=0.1, beta_max=20.0, t_epsilon=t_eps, T=T, num_steps_forward=NSF_G, device=DEV,
                       denseTensor=(kind == "dense"), norm_map="log", G=g.get("dn_G") if kind == "dense" else None,
                       estim_cst_norm_dens_r_T=False)
    net = MLP(d, premodule=pre)
    load_det_(net)
    return PluginReverseSDE(base, net.to(DEV), T, ssm_intT=ssm_intT, deviceReverseSDE=DEV).to(DEV)


@pytest.mark.parametrize("sub,t_eps,k0", [("drop", 0.3, 1), ("all", 1e-3, 0)])
@pytest.mark.parametrize("tag", ["sp", "dn"])
def test_ssm_golden(g, tag, sub, t_eps, k0):
    """ssm(x, eps=, u_v=) against the reference's ssm() with ssm_intT=True: t exact, y within test_golden_g08's 1e-4, per-row
    loss and gradients within test_host_gpu.py::test_ssm_msgm_mlp_golden's 2e-5 and 3e-4."""
    key = f"{tag}_{sub}"
    gen = golden_gen(g, tag, t_eps)
    x, eps, u_v = g[key + "_x"].to(DEV), g[key + "_eps"].to(DEV), g[key + "_u_v"].to(DEV)
    rows = (NSF_G - k0) * B_G
    t, xt, y = gen.sample_txy(x, eps=eps)
    assert t.shape == (rows, 1) and y.shape == (rows, x.shape[1]) and torch.equal(xt, x.repeat(NSF_G - k0, 1))
    assert torch.equal(t.cpu(), g[key + "_t"])
    e_y = rel_l2(y.cpu(), g[key + "_y"])
    gen.zero_grad()
    s0 = gen.base_sde.philox(x.device).state.clone()
    per = gen.ssm(x, eps=eps, u_v=u_v)
    assert torch.equal(gen.base_sde.rng.state, s0)                     # every draw injected: the stream stays
    assert per.shape == (rows,)
    e_per = rel_l2(per.detach().cpu(), g[key + "_per"])
    print(f"g24 {key}: y rel-L2 {e_y:.2e}, per-row loss {e_per:.2e}")
    assert e_y <= 1e-4 and e_per <= 2e-5
    per.mean().backward()
    for k, p in gen.named_parameters():
        if p.requires_grad:
            e = rel_l2(p.grad.cpu(), g[f"{key}_grad::{k}"])
            assert e <= 3e-4, (k, e)


@pytest.mark.parametrize("tag", ["sg", "sp", "dn"])
def test_evaluate_golden(g, tag):
    """elbo_random_t_slice on the nsf' B rows with the path noise, the probe uniforms and yT injected, against the reference's
    rows (rel-L2 2e-5, the bound of the per-row loss: the latent term is the same kernel as in tests/test_kde_gpu.py's ELBO
    case, which holds it to that bound too), and evaluate's two numbers formed from them.  |mean(a) - mean(b)| <= rms(a - b)
    and |std(a) - std(b)| <= |a - b| / sqrt(R - 1), so both follow from the row bound."""
    from sdeflow_light_amd.NN import evaluate
    key = f"{tag}_ev"
    gen = golden_gen(g, tag, 1e-3)
    x = g[key + "_x"].to(DEV)
    rows = NSF_G * B_G
    elbo = gen.elbo_random_t_slice(x, eps=g[key + "_eps"].to(DEV), u_v=g[key + "_u_v"].to(DEV), yT=g[key + "_yT"].to(DEV))
    assert elbo.shape == (rows,)
    ref = g[key + "_elbo"]
    e = rel_l2(elbo.cpu(), ref)
    mean, sem = elbo.mean().cpu(), (elbo.std() / B_G ** 0.5).cpu()
    d_mean, d_sem = abs(float(mean) - float(g[key + "_mean"])), abs(float(sem) - float(g[key + "_sem"]))
    print(f"g24 {key}: ELBO rows rel-L2 {e:.2e}, mean off by {d_mean:.2e}, standard error off by {d_sem:.2e}")
    assert e <= 2e-5
    slack = 2e-5 * float(ref.double().norm())
    assert d_mean <= slack / rows ** 0.5 + 1e-6 * abs(float(g[key + "_mean"]))
    assert d_sem <= slack / (rows - 1) ** 0.5 / B_G ** 0.5 + 1e-6 * abs(float(g[key + "_sem"]))
    # nothing injected, as the driver calls it: the latent sample and the density run on the tiled x
    m, s = evaluate(gen, x)
    assert m.dim() == 0 and s.dim() == 0 and math.isfinite(float(m)) and math.isfinite(float(s)) and gen.training


def test_ssm_loss_ignores_the_flag(g):
    """ssm_loss(t_, x, y) with ssm_intT on equals the same call with it off (upstream's ssm_loss never reads the flag)."""
    key = "sp_all"
    on, off = golden_gen(g, "sp", 1e-3), golden_gen(g, "sp", 1e-3, ssm_intT=False)
    t, y, u_v = g[key + "_t"].to(DEV), g[key + "_y"].to(DEV), g[key + "_u_v"].to(DEV)
    assert torch.equal(on.ssm_loss(t, y, y, u_v=u_v).detach(), off.ssm_loss(t, y, y, u_v=u_v).detach())


def test_eager_philox_positions_and_cotangents(g, ops):
    """Nothing injected: the path draws take nsf stream positions, the probe the next one.  A non-uniform cotangent runs the
    second pass over the nsf' B saved rows and agrees with the same weights given as row_weight (two fp32 evaluations of the
    same 9-term sums, one scaled by 1/9 and back: 1e-5 on the flat gradient)."""
    gen = golden_gen(g, "sp", 0.3)
    x = g["sp_drop_x"].to(DEV)
    rows = 3 * B_G
    rng = gen.base_sde.philox(x.device)
    s0 = rng.state.clone()
    per = gen.ssm(x)
    assert per.shape == (rows,) and bool(torch.isfinite(per).all())
    assert int(rng.state[1]) - int(s0[1]) == NSF_G + 1
    rng.state.copy_(s0)
    t, _, y = gen.sample_txy(x)
    v = ops.rademacher((rows, 6), x.device, rng=rng)
    # the same rows through the (t, y, v)-given entry: the same kernels on the same operands
    assert torch.equal(gen.ssm(y, y=y, t_given=t, v=v).detach(), per.detach())
    w = torch.linspace(0.5, 2.0, rows, device=DEV)
    rng.state.copy_(s0)
    gen.zero_grad()
    (gen.ssm(x) * w).sum().backward()
    g1 = torch.cat([p.grad.reshape(-1) for p in gen.a.parameters()]).clone()
    rng.state.copy_(s0)
    gen.zero_grad()
    got = gen.ssm(x, row_weight=w)
    assert torch.equal(got.detach(), per.detach() * w)
    got.sum().backward()
    g2 = torch.cat([p.grad.reshape(-1) for p in gen.a.parameters()])
    within(rel_l2(g1.cpu(), g2.cpu()), 1e-5, "ssm_intT: cotangent w vs row_weight w, flat gradient rel-L2")
    with pytest.raises(Exception):
        gen.ssm(x, row_weight=torch.ones(B_G, device=DEV))           # one weight per RETURNED row


def test_ssm_unet1d_vs_oracle():
    """UNet1D, L = 64, B = 2, nsf = 4, sparse tensor, against tests/ssm_intT_ref.py; the bounds of
    tests/test_host_gpu.py::test_ssm_unet1d_msgm_sparse_vs_oracle (2e-6 on the per-row loss and on the flat gradient)."""
    from oracle import nets_ref as N, sde_ref as S
    from oracle.det_params import det_state_dict, load_det_
    from oracle.shapes import unet1d_shapes
    from sdeflow_light_amd.NNUnet1D import UNet1D
    from sdeflow_light_amd.SDEs import MSGMsde, PluginReverseSDE
    torch.manual_seed(0)
    L_, B, nsf, t_eps = 64, 2, 4, 0.3
    net = UNet1D(input_dim=L_, base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, premodule=None, emb_dim=128)
    load_det_(net)
    T = Tp()
    base = MSGMsde(torch.randn(64, L_), beta_min=0.1, beta_max=20.0, t_epsilon=t_eps, T=T, num_steps_forward=nsf, device=DEV,
                   denseTensor=False, norm_map="log")
    gen = PluginReverseSDE(base, net.to(DEV), T, ssm_intT=True, deviceReverseSDE=DEV).to(DEV)
    rows = 3 * B
    x, eps, uv = torch.randn(B, L_), torch.randn(nsf, B, L_), torch.rand(rows, L_)
    gen.zero_grad()
    per = gen.ssm(x.to(DEV), eps=eps.to(DEV), u_v=uv.to(DEV))
    per.mean().backward()
    sp = S.SdeSpec(kind=S.MSGM_SPARSE, n=L_, num_steps_forward=nsf, t_epsilon=t_eps)
    p = det_state_dict(unet1d_shapes(L_, None))
    score = lambda prm, yy, tt: N.unet1d_forward(prm, yy, tt, None)
    t_ref, y_ref, _, per_ref, gref = IR.ssm(sp, score, p, x, eps, uv)
    t, _, y = gen.sample_txy(x.to(DEV), eps=eps.to(DEV))
    assert torch.equal(t.cpu(), t_ref)
    print(f"ssm_intT + UNet1D: y rel-L2 {rel_l2(y.cpu(), y_ref):.2e}")
    flat = torch.cat([pp.grad.reshape(-1).cpu() for _, pp in gen.a.named_parameters()])
    ref = torch.cat([gref[k].reshape(-1) for k, _ in gen.a.named_parameters()])
    e_per, e_flat = rel_l2(per.detach().cpu(), per_ref), rel_l2(flat, ref)
    print(f"ssm_intT + UNet1D: per-row loss rel-L2 {e_per:.2e}, flat gradient rel-L2 {e_flat:.2e} (tolerance 2e-6 each)")
    assert per.shape == (rows,)
    assert e_per <= 2e-6
    assert e_flat <= 2e-6


# ------------------------------------------------------------------ trainers
NSF_T, B_T = 4, 8
TRAINERS = {"mlp6": ("sparse", 6, 0.3), "mlp4": ("dense", 4, 1e-3), "unet1d": ("sparse", 64, 0.3)}


def _gen(which, ssm_intT=True, kind=None, nsf=NSF_T, t_eps=None):
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.NNUnet1D import UNet1D
    from sdeflow_light_amd.SDEs import MSGMsde, PluginReverseSDE, SGMsde
    k, d, te = TRAINERS[which]
    kind, t_eps = kind or k, te if t_eps is None else t_eps
    torch.manual_seed(3)
    if which == "unet1d":
        net = UNet1D(input_dim=d, base_channels=16, channel_mults=(1, 2), emb_dim=32, premodule="NormalizeLogRadius")
    else:
        net = MLP(d, premodule="NormalizeLogRadius" if which == "mlp6" else None)
    T = Tp()
    if kind == "sgm":
        base = SGMsde(beta_min=R.B0, beta_max=R.B1, t_epsilon=t_eps, T=T, num_steps_forward=nsf, device=DEV)
    else:
        base = MSGMsde(torch.randn(64, d), beta_min=R.B0, beta_max=R.B1, t_epsilon=t_eps, T=T, num_steps_forward=nsf, device=DEV,
                       denseTensor=(kind == "dense"), norm_map="log", G=R.dense_G(d)[0] if kind == "dense" else None)
    return PluginReverseSDE(base, net.to(DEV), T, ssm_intT=ssm_intT, deviceReverseSDE=DEV).to(DEV)


def _trainer(which, **kw):
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    gen = _gen(which)
    d = TRAINERS[which][1]
    if which == "unet1d":
        tr = UNetScoreTrainer(gen, B_T, d, lr=1e-3, seed=11, **kw)
    else:
        tr = MLPScoreTrainer(gen, B_T, lr=1e-3, seed=11, **kw)
    torch.manual_seed(5)
    tr.set_data(torch.randn(B_T, d, device=DEV) * 1.5)
    return tr


def _run(tr, steps=3):
    losses = [float(tr.step()) for _ in range(steps)]
    return losses, tr.flat.clone(), tr.m.clone(), tr.v.clone(), tr.rng.state.clone()


def _same(a, b):
    assert all(v == v for v in a[0]) and a[0] == b[0], (a[0], b[0])
    for p, q in zip(a[1:], b[1:]):
        assert torch.equal(p, q)


@pytest.mark.parametrize("which", list(TRAINERS))
def test_trainer_graph_eager_and_composed_agree(ops, SS, monkeypatch, which):
    """Three captured steps equal three eager steps, and the kernel route equals the composed trajectory (eager: it holds
    copy nodes), bit for bit: losses, parameters, Adam moments, Philox state.  The captured step holds kernel nodes only."""
    rows = (NSF_T - (1 if TRAINERS[which][2] == 0.3 else 0)) * B_T
    tr = _trainer(which, use_graph=True)
    assert tr.rows == rows and tr.t.shape == (rows,) and tr.inv_batch == 1.0 / rows
    graphed = _run(tr)
    kinds = ops.graph_node_kinds(tr.graph)
    assert set(kinds) == {"kernel"}, kinds
    eager = _run(_trainer(which, use_graph=False))
    _same(graphed, eager)
    assert int(graphed[4][1]) - 3 * (NSF_T + 1) == int(_trainer(which, use_graph=False).rng.state[1])
    with monkeypatch.context() as m:
        m.setattr(SS, "msgm_forward_paths", SS.msgm_forward_paths_composed)
        composed = _run(_trainer(which, use_graph=False))
    _same(graphed, composed)


@pytest.mark.parametrize("which", list(TRAINERS))
def test_trainer_step_draws_equal_eager(ops, which):
    """Step 1's (y, v) equal eager sample_txy plus the probe from the same stream state."""
    tr = _trainer(which, use_graph=False)
    s0 = tr.rng.state.clone()
    tr.step()
    y, v = tr._live[0].clone(), tr._live[1].clone()
    s1 = tr.rng.state.clone()
    tr.rng.state.copy_(s0)
    t, _, y2 = tr.gen_sde.sample_txy(tr.x)
    v2 = ops.rademacher((tr.rows, tr.d), tr.dev, rng=tr.rng)
    tr.rng.advance(1)
    assert torch.equal(t.reshape(-1), tr.t) and torch.equal(y2, y) and torch.equal(v2, v)
    assert torch.equal(tr.rng.state, s1)


@pytest.mark.parametrize("which", list(TRAINERS))
def test_trainer_unit_row_weights_change_nothing(which):
    tr = _trainer(which, use_graph=True, row_weights=True)
    assert tr.w.shape == (tr.rows,)
    tr.set_data(tr.x.clone(), weight=torch.ones(tr.rows, device=DEV))
    _same(_run(tr), _run(_trainer(which, use_graph=True)))


def test_trainer_options_keep_working():
    """The data stage and every optimizer-stage option with the integrated loss: the captured step equals the eager one
    bit for bit (parameters, Adam moments, weight average, Philox state) and every step draws a fresh x of B paths."""
    from sdeflow_light_amd.data import Gaussian
    from sdeflow_light_amd.train import MLPScoreTrainer, warmup_cosine

    def run(use_graph):
        tr = MLPScoreTrainer(_gen("mlp6"), B_T, lr=1e-3, seed=11, use_graph=use_graph, max_grad_norm=0.5, ema_rate=0.9,
                             lr_schedule=warmup_cosine(1e-3, 2, 10), data=Gaussian(6, device=DEV, seed=4))
        xs = []
        for _ in range(3):
            tr.step()
            xs.append(tr.x.clone())
        assert tr.x.shape == (B_T, 6) and not torch.equal(xs[0], xs[1]) and bool(torch.isfinite(tr.loss).all())
        return tr.flat.clone(), tr.m.clone(), tr.v.clone(), tr.ema.clone(), tr.rng.state.clone(), torch.stack(xs)
    for p, q in zip(run(True), run(False)):
        assert torch.equal(p, q)


def test_refusals(L):
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.SDEs import MSGMsde, PluginReverseSDE
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    E = L.MsgmError
    x = torch.randn(B_T, 6, device=DEV)
    none_left = _gen("mlp6", t_eps=1.0)                                    # nsf' == 0
    s0 = none_left.base_sde.philox(x.device).state.clone()
    for call in (lambda: none_left.ssm(x), lambda: none_left.sample_txy(x), lambda: MLPScoreTrainer(none_left, B_T)):
        with pytest.raises(E):
            call()
    assert torch.equal(none_left.base_sde.rng.state, s0)
    gen = _gen("mlp6")
    for call in (lambda: gen.ssm(x, u=torch.rand(B_T, device=DEV)), lambda: gen.sample_txy(x, u=torch.rand(B_T, device=DEV))):
        with pytest.raises(E):
            call()
    with pytest.raises(E):
        MLPScoreTrainer(_gen("mlp6", kind="sgm"), B_T)                     # the additive SDE
    with pytest.raises(E):
        UNetScoreTrainer(_gen("unet1d", kind="sgm"), B_T, 64)
    with pytest.raises(E):
        MLPScoreTrainer(gen, B_T, world=2)
    with pytest.raises(E):
        UNetScoreTrainer(_gen("unet1d"), B_T, 64, world=2)
    T = Tp()                                                              # a row length the kernel does not take
    wide = PluginReverseSDE(MSGMsde(torch.randn(64, 65), T=T, num_steps_forward=NSF_T, device=DEV, denseTensor=True, norm_map="log",
                                    G=R.dense_G(65)[0]), MLP(65).to(DEV), T, ssm_intT=True, deviceReverseSDE=DEV).to(DEV)
    with pytest.raises(E):
        MLPScoreTrainer(wide, B_T)
    MLPScoreTrainer(_gen("mlp6", ssm_intT=False, kind="sgm"), B_T)          # the flag off: built as before
