"""The one-launch MLP sampler loop (msgm_mlp_sde_loop: Euler-Maruyama, Heun and RK4-Stratonovich, all three SDE families)
against the reference's recorded trajectories (g07), against the float64 oracle with the composed path of the same build
as the yardstick, and against the composed path on the Philox stream; shard invariance, fallbacks and graph capture."""
import itertools

import pytest
import torch

from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
NLR = "NormalizeLogRadius"


def Tp():
    return torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)


def make_gen(kind, d, pre, g=None, prefix=None, G=None, out_scale=None):
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.SDEs import SGMsde, MSGMsde, PluginReverseSDE
    T = Tp()
    if kind == "sgm":
        base = SGMsde(beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=16, device=DEV)
    else:
        base = MSGMsde(torch.randn(64, d), beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=T, num_steps_forward=16,
                       device=DEV, denseTensor=(kind == "dense"), norm_map="log", G=G)
    gen = PluginReverseSDE(base, MLP(d, premodule=pre).to(DEV), T, deviceReverseSDE=DEV).to(DEV)
    if g is not None:
        missing = gen.load_state_dict(g.sub(prefix), strict=False)
        assert set(missing.missing_keys) <= {"T", "base_sde.T"} and not missing.unexpected_keys
    if out_scale is not None:
        with torch.no_grad():
            gen.a.main[6].weight.mul_(out_scale)
            gen.a.main[6].bias.mul_(out_scale)
    return gen


def run_loop(gen, method, x0, N, *, lmbd=0.0, z=None, rng=None, nc=False, keep_all=True, include_t0=True, keep=None,
             workspace=None):
    """ops.mlp_sde_loop as _Run.mlp_loop calls it; returns (final state, trajectory or kept rows or None), on the device."""
    from sdeflow_light_amd import ops
    base = gen.base_sde
    T = base.T_float()
    ts = (torch.linspace(0, 1, N + 1) * T).to(DEV)
    x = x0.to(DEV).clone()
    B, d = x.shape
    norm0 = ops.row_norm(x) if nc else None
    traj = kept = None
    if keep_all:
        traj = torch.zeros(N + int(include_t0), B, d, device=DEV)
        if include_t0:
            traj[0].copy_(x)
    elif keep is not None:
        keep = keep.to(torch.int32).to(DEV).contiguous()
        kept = torch.zeros(B, d, device=DEV)
    ops.mlp_sde_loop(gen.a.kernel_params(), x, base.struct(), method, ts, T / N, lmbd, z=None if z is None else z.to(DEV),
                     rng=rng, norm0=norm0, traj=traj, include_t0=include_t0, keep=keep, kept=kept, workspace=workspace)
    return x, (traj if keep_all else kept)


# ------------------------------------------------------------------ 1. the reference's recorded trajectories
G07 = [  # (prefix, kind, d, premodule, copies, tag, method, norm correction, lmbd, include_t0)
    ("sgm", "sgm", 2, None, 3, "sgm_em", "em", False, 0.0, True),
    ("sgm", "sgm", 2, None, 3, "sgm_heun", "heun", False, 0.0, True),
    ("sgm", "sgm", 2, None, 3, "sgm_rk4", "rk4", False, 0.0, True),
    ("sgm", "sgm", 2, None, 3, "sgm_em_l05", "em", False, 0.5, False),
] + [("sp", "sparse", 6, NLR, 5, f"sp_{m}_nc{nc}", m, bool(nc), 0.0, True) for nc in (0, 1) for m in ("em", "heun", "rk4")] + [
    ("dn", "dense", 4, None, 5, f"dn_{m}", m, True, 0.0, True) for m in ("em", "rk4")]


@pytest.mark.parametrize("prefix,kind,d,pre,copies,tag,method,nc,lmbd,inc", G07, ids=[c[5] for c in G07])
def test_reference_trajectories(prefix, kind, d, pre, copies, tag, method, nc, lmbd, inc):
    """The fixture's rows replicated (rows are independent): every copy within the fixture's 1e-4 of the reference's
    trajectory, and the copies — in different tiles and workgroups, the last tile ragged — equal to the bit."""
    g = load_golden("g07_samplers")
    gen = make_gen(kind, d, pre, g, prefix + "::", G=g["dn_G"] if kind == "dense" else None)
    x0, z, ref = g[prefix + "_x0"], g[tag + "_z"], g[tag + "_traj"]
    b0 = x0.shape[0]
    _, traj = run_loop(gen, method, x0.repeat(copies, 1), z.shape[0], lmbd=lmbd, z=z.repeat(1, copies, 1), nc=nc, include_t0=inc)
    traj = traj.cpu()
    assert traj.shape == (ref.shape[0], copies * b0, d) and torch.isfinite(traj).all()
    errs = [rel_l2(traj[:, k * b0:(k + 1) * b0], ref) for k in range(copies)]
    print(f"{tag} x{copies}: rel-L2 of each copy vs the reference {['%.2e' % e for e in errs]}")
    assert max(errs) <= 1e-4
    for k in range(1, copies):
        assert torch.equal(traj[:, k * b0:(k + 1) * b0], traj[:, :b0]), k


def test_reference_final_state_and_kept_rows():
    """keep_all_samples=False: the final state alone, and the samplesToKeep rows (sgm_em_keep stop indices)."""
    g = load_golden("g07_samplers")
    gen = make_gen("sgm", 2, None, g, "sgm::")
    x0 = g["sgm_x0"].repeat(3, 1)
    x, none = run_loop(gen, "em", x0, 8, z=g["sgm_em_final_z"].repeat(1, 3, 1), keep_all=False)
    assert none is None
    x = x.cpu()
    for k in range(3):
        assert rel_l2(x[32 * k:32 * (k + 1)], g["sgm_em_final"]) <= 1e-4
    _, kept = run_loop(gen, "em", x0, 8, z=g["sgm_em_keep_z"].repeat(1, 3, 1), keep_all=False, include_t0=False,
                       keep=g["sgm_em_keep_idx"].repeat(3))
    kept = kept.cpu()
    for k in range(3):
        assert rel_l2(kept[32 * k:32 * (k + 1)], g["sgm_em_keep"]) <= 1e-4
        assert torch.equal(kept[32 * k:32 * (k + 1)], kept[:32])


# ------------------------------------------------------------------ 2. float64 yardstick
def oracle_traj(gen, kind, pre, method, x0, z, lmbd, nc, dtype):
    from oracle import sde_ref as S, nets_ref as N
    base = gen.base_sde
    p = {k[2:]: v.detach().cpu().to(dtype) for k, v in gen.state_dict().items() if k.startswith("a.")}
    okind = {"sgm": S.SGM, "sparse": S.MSGM_SPARSE, "dense": S.MSGM_DENSE}[kind]
    spec = S.SdeSpec(kind=okind, n=x0.shape[1], G=base.G.cpu().to(dtype) if kind == "dense" else None)
    proc = S.ReverseProcess(spec, lambda y, s: N.mlp_forward(p, y, s, pre), lmbd)
    fn = {"em": S.euler_maruyama, "heun": S.heun, "rk4": S.rk4_stratonovich}[method]
    return fn(proc, x0.to(dtype), z.shape[0], z.to(dtype), norm_correction=nc, keep_all=True, include_t0=True)


YARD = [(2, None, "sgm"), (2, NLR, "dense"), (3, None, "sparse"), (6, NLR, "sparse"), (16, None, "dense"), (16, NLR, "sparse"),
        (20, None, "sparse"), (30, NLR, "sgm")]


@pytest.mark.parametrize("d,pre,kind", YARD, ids=[f"d{d}-{'nlr' if p else 'none'}-{k}" for d, p, k in YARD])
def test_float64_yardstick(d, pre, kind):
    """Truth: the oracle integrators with nets_ref.mlp_forward in float64.  Yardstick: the composed path of this build
    through the public sampler with noise=z, and the same oracle in float32 (1.0e-7 to 2.4e-7 from the truth on the g07
    cases).  The loop may be no further from the truth than 2 x the larger of the two (the margin of parity_vs_fp64).
    B = 33: two tiles, one live row in the second; 65: three tiles in one workgroup; 160: a 3 / 2 split; 1000: many
    workgroups.  Heun and RK4 at N = 4, Euler-Maruyama at N = 6 (multiplicative SDEs: the additive one keeps its own
    kernels); lmbd 0 and 0.5; norm correction off and on for the multiplicative SDEs; include_t0 trajectories.
    The net is an untrained one with its output layer scaled by 0.1: at full size the multiplicative drift G(x) a(x) of a
    net without premodule grows quadratically in |x| and, at these step lengths, rows of the float64 truth itself
    overflow within four steps (d = 3, 16 and 20 on the CPU oracle); scaled, every trajectory stays below 2e3 and still
    depends on the score at the 1e-2 level, five orders above the bound."""
    from sdeflow_light_amd import sde_scheme as SS
    torch.manual_seed(100 * d + len(kind))
    gen = make_gen(kind, d, pre, out_scale=0.1)
    msgm = kind != "sgm"
    public = {"em": SS.euler_maruyama_sampler, "heun": SS.heun_sampler, "rk4": SS.rk4_stratonovich_sampler}
    methods = [("heun", 4), ("rk4", 4)] + ([("em", 6)] if msgm else [])
    worst = 0.0
    for B, (method, N), lmbd, nc in itertools.product((33, 65, 160, 1000), methods, (0.0, 0.5), (False, True) if msgm else (False,)):
        x0, z = torch.randn(B, d), torch.randn(N, B, d)
        truth = oracle_traj(gen, kind, pre, method, x0, z, lmbd, nc, torch.float64)
        assert torch.isfinite(truth).all()
        e32 = rel_l2(oracle_traj(gen, kind, pre, method, x0, z, lmbd, nc, torch.float32), truth)
        comp = public[method](gen, x0.to(DEV), num_steps=N, lmbd=lmbd, keep_all_samples=True, include_t0=True,
                              norm_correction=nc, noise=z)
        ec = rel_l2(comp, truth)
        _, traj = run_loop(gen, method, x0, N, lmbd=lmbd, z=z, nc=nc)
        el = rel_l2(traj.cpu(), truth)
        print(f"yardstick d={d} pre={pre} {kind} B={B} {method} N={N} lmbd={lmbd} nc={int(nc)}: "
              f"loop {el:.3e} | composed {ec:.3e} | float32 oracle {e32:.3e}  (vs float64)")
        worst = max(worst, el / max(ec, e32))
        assert torch.isfinite(traj).all()
        assert el <= 2.0 * max(ec, e32), (B, method, lmbd, nc, el, ec, e32)
    print(f"yardstick d={d} pre={pre} {kind}: worst loop / max(composed, float32 oracle) = {worst:.2f}")


# ------------------------------------------------------------------ 3. Philox path through the public samplers
@pytest.mark.parametrize("kind,d,pre,nc", [("sgm", 2, None, False), ("sparse", 6, NLR, True)])
@pytest.mark.parametrize("method", ["rk4", "heun"])
def test_public_sampler_takes_the_loop_on_the_philox_stream(monkeypatch, method, kind, d, pre, nc):
    from sdeflow_light_amd import ops, sde_scheme as SS
    torch.manual_seed(3)
    gen = make_gen(kind, d, pre)
    public, composed = {"rk4": (SS.rk4_stratonovich_sampler, SS.rk4_stratonovich_composed),
                        "heun": (SS.heun_sampler, SS.heun_composed)}[method]
    calls = []
    real = ops.mlp_sde_loop
    monkeypatch.setattr(ops, "mlp_sde_loop", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    N, B = 5, 160
    x0 = torch.randn(B, d, device=DEV)
    rng = gen.base_sde.philox(DEV)
    st = rng.state.clone()
    kw = dict(num_steps=N, keep_all_samples=True, include_t0=True, norm_correction=nc)
    a = public(gen, x0, **kw)
    off_loop = rng.state.clone()
    assert calls == [method]
    rng.state.copy_(st)
    ref = composed(gen, x0, **kw)
    assert calls == [method]                                   # the composed functions stay composed
    assert torch.equal(rng.state, off_loop)                     # the stream advances by N either way
    assert int(off_loop[1] - st[1]) == N
    e = rel_l2(a, ref)
    print(f"{method} {kind} d={d} nc={int(nc)}: loop vs composed on the Philox stream rel-L2 {e:.2e} (bound 2e-6)")
    assert a.shape == ref.shape == (N + 1, B, d) and e <= 2e-6
    b = public(gen, x0, **kw)                                   # second run: fresh noise
    assert not torch.equal(a, b) and torch.isfinite(b).all()
    rng.state.copy_(st)
    assert torch.equal(public(gen, x0, **kw), a)                # same state: the same bits


def test_euler_maruyama_msgm_takes_the_loop_sgm_keeps_its_kernels(monkeypatch):
    from sdeflow_light_amd import ops, sde_scheme as SS
    torch.manual_seed(4)
    calls = []
    real = ops.mlp_sde_loop
    monkeypatch.setattr(ops, "mlp_sde_loop", lambda *a, **k: (calls.append(a[3]), real(*a, **k))[1])
    gen = make_gen("sparse", 6, NLR)
    x0 = torch.randn(160, 6, device=DEV)
    rng = gen.base_sde.philox(DEV)
    st = rng.state.clone()
    a = SS.euler_maruyama_sampler(gen, x0, num_steps=5, keep_all_samples=True, norm_correction=True)
    assert calls == ["em"]
    # the composed Euler-Maruyama steps from the same stream state
    rng.state.copy_(st)
    monkeypatch.setattr(ops, "mlp_sde_loop_supported", lambda *a: False)
    ref = SS.euler_maruyama_sampler(gen, x0, num_steps=5, keep_all_samples=True, norm_correction=True)
    assert calls == ["em"] and rel_l2(a, ref) <= 2e-6
    monkeypatch.undo()
    calls2 = []
    monkeypatch.setattr(ops, "mlp_sde_loop", lambda *a, **k: calls2.append(a[3]))
    SS.euler_maruyama_sampler(make_gen("sgm", 2, None), torch.randn(160, 2, device=DEV), num_steps=3, keep_all_samples=True)
    assert calls2 == []


# ------------------------------------------------------------------ 4. shard invariance
def test_shard_invariance():
    """Rows [0, 64) and [64, 128) as two calls with set_shard draw the numbers of the 128-row call."""
    from sdeflow_light_amd._lib import PhiloxState
    torch.manual_seed(5)
    gen = make_gen("sparse", 6, NLR)
    x0 = torch.randn(128, 6)
    xf, tf = run_loop(gen, "rk4", x0, 3, rng=PhiloxState(11, DEV), nc=True)
    for lo in (0, 64):
        xs, tsh = run_loop(gen, "rk4", x0[lo:lo + 64], 3, rng=PhiloxState(11, DEV, row_base=lo, n=6), nc=True)
        assert torch.equal(xs, xf[lo:lo + 64]) and torch.equal(tsh, tf[:, lo:lo + 64])
    assert not torch.equal(tf[:, :64], tf[:, 64:])


# ------------------------------------------------------------------ 5. fallbacks
@pytest.mark.parametrize("kind,d,B", [("sgm", 2, 32), ("sgm", 31, 64), ("dense", 17, 64)])
def test_unsupported_shapes_are_refused_and_stay_composed(monkeypatch, kind, d, B):
    from sdeflow_light_amd import ops, sde_scheme as SS
    from sdeflow_light_amd._lib import MsgmError
    torch.manual_seed(6)
    gen = make_gen(kind, d, None)
    x0 = torch.randn(B, d)
    with pytest.raises(MsgmError):
        run_loop(gen, "rk4", x0, 3, z=torch.randn(3, B, d))
    calls = []
    monkeypatch.setattr(ops, "mlp_sde_loop", lambda *a, **k: calls.append(a[3]))
    rng = gen.base_sde.philox(DEV)
    st = rng.state.clone()
    a = SS.rk4_stratonovich_sampler(gen, x0.to(DEV), num_steps=3, keep_all_samples=True)
    rng.state.copy_(st)
    b = SS.rk4_stratonovich_composed(gen, x0.to(DEV), num_steps=3, keep_all_samples=True)
    assert calls == [] and torch.isfinite(a).all() and torch.equal(a, b)


# ------------------------------------------------------------------ 6. graph capture
def test_graph_capture_is_one_kernel_chain():
    from sdeflow_light_amd import ops, sde_scheme as SS
    torch.manual_seed(7)
    gen = make_gen("sparse", 6, NLR)
    base = gen.base_sde
    N, B, d = 4, 160, 6
    T = base.T_float()
    ts = (torch.linspace(0, 1, N + 1) * T).to(DEV)
    x0 = torch.randn(B, d, device=DEV)
    x = x0.clone()
    norm0 = ops.row_norm(x)
    traj = torch.zeros(N + 1, B, d, device=DEV)
    ws = ops.mlp_sde_loop_workspace(B, d, "rk4", DEV)
    rng = base.philox(DEV)
    P, st = gen.a.kernel_params(), base.struct()

    def body():
        ops.mlp_sde_loop(P, x, st, "rk4", ts, T / N, 0.0, rng=rng, norm0=norm0, traj=traj, include_t0=True, workspace=ws)
        rng.advance(N)

    graph = SS._capture(body, DEV)
    kinds = ops.graph_node_kinds(graph)
    print(f"captured sampler loop = {kinds}")
    assert set(kinds) == {"kernel"}, kinds
    state = rng.state.clone()
    x.copy_(x0)
    traj.zero_()
    body()
    eager_x, eager_traj, after = x.clone(), traj.clone(), rng.state.clone()
    rng.state.copy_(state)
    x.copy_(x0)
    traj.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, eager_x) and torch.equal(traj, eager_traj) and torch.equal(rng.state, after)
    assert torch.isfinite(x).all() and not torch.equal(x, x0)
