"""-m gpu: the optimizer stage (csrc/optim_kernels.hip) — deterministic global gradient norm, Adam with device-resident
hyper-parameters, clipping and a weight EMA — from the C ABI up to the trainers and FusedAdam.

Kernels: per element against the float64 restatement of tests/optim_ref.py, |kernel - ref64| <= c * 2^-24 * magnitude with
c = 4 x the CPU float32 measurement (optim_ref.MEASURED, guarded by tests/test_optim_ref.py).  The update is checked
against the restatement fed the kernel's OWN reported norm and the EMA against the kernel's own new parameters, so each
check sees one stage's error.  Bitwise: the partial sums against the documented order, aligned against unaligned buffers,
two runs, coef = 1 without EMA against msgm_adam_step, swap twice.  n: 4 (vector body; scalar through the unaligned
view) and 7 (scalar body), 4096, one slice exactly and one element more, the last n at the base slice length and the
first past the cap (slices lengthen), and 2 097 156.

Trainers: every step against the restatement with that step's scheduled learning rate; graph replay against eager;
the default trainers never reach the new kernels and an option trainer that cannot clip (max_grad_norm = 1e30) is bitwise
the default one; EMA swap, checkpoints, FusedAdam.
"""
import ctypes

import pytest
import torch

import optim_ref as O
from test_host_gpu import make_gen

pytestmark = pytest.mark.gpu
DEV = "cuda"
GSCALE, RATE, STEPS = 0.5, 0.999, 5


@pytest.fixture(scope="module")
def ops():
    from sdeflow_light_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def L():
    from sdeflow_light_amd import _lib
    return _lib


def shifted(t):
    """The same values in a contiguous buffer that is 4-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def bound(what, y, ref, mag, family):
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite output"
    r, c = O.ratio(y.reshape(-1), ref.reshape(-1), mag.reshape(-1)), O.c_of(family)
    print(f"{what}: ratio {r:.3f} (bound {c:.1f})")
    assert r <= c, f"{what}: {r:.3f} x 2^-24 magnitude exceeds c = {c:.1f}"


def c_sqnorm(L, g, gscale, partials):
    cnt = ctypes.c_int32(-1)
    L.check(L.lib().msgm_grad_sqnorm(L.ptr(g), g.numel(), float(gscale), L.ptr(partials), ctypes.byref(cnt), L.stream()),
            "msgm_grad_sqnorm")
    return cnt.value


def c_adam_ex(L, p, g, m, v, ema, hyper, gscale, step_dev, partials, norm_out):
    L.check(L.lib().msgm_adam_step_ex(L.ptr(p), L.ptr(g), L.ptr(m), L.ptr(v), L.ptr(ema), p.numel(), L.ptr(hyper),
                                      float(gscale), L.ptr(step_dev), L.ptr(partials),
                                      0 if partials is None else partials.numel(), L.ptr(norm_out), L.stream()),
            "msgm_adam_step_ex")


_INPUTS = {}


def inputs(n):
    """(p0, [g_1 .. g_STEPS], max_norm = half the float64 norm of g_1 * GSCALE) on the device, drawn once per n."""
    if n not in _INPUTS:
        p, draw = O.kernel_inputs(n, device=DEV)
        gs = [draw() for _ in range(STEPS)]
        _INPUTS.clear()                                   # one n resident at a time (the large cases hold 200 MB)
        _INPUTS[n] = (p, gs, 0.5 * float(O.gnorm(gs[0], GSCALE)[0]))
    return _INPUTS[n]


def run_kernels(ops, L, n, shift=False, check=False, max_norm="half", ema_on=True):
    """STEPS steps of grad_sqnorm + adam_step_ex from the kernel's own state, lr_k = 1e-3 k written to the device
    hyper-parameters between the launches.  Returns (p, m, v, ema, [reported norms], last partials)."""
    p0, gs, half = inputs(n)
    max_norm = half if max_norm == "half" else max_norm
    place = shifted if shift else (lambda t: t.clone())
    p, m, v = place(p0), place(torch.zeros_like(p0)), place(torch.zeros_like(p0))
    ema = place(p0) if ema_on else None
    hyper = ops.opt_hyper(DEV, 1e-3, max_grad_norm=max_norm, ema_rate=RATE)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    need = ops.grad_sqnorm_partials(n)
    assert need == O.n_partials(n)
    norms, clipped = [], []
    for k in range(1, STEPS + 1):
        g = place(gs[k - 1])
        lr = 1e-3 * k
        hyper[ops.OPT_LR:ops.OPT_LR + 1].fill_(lr)
        ops.counter_inc(step_dev)
        partials = torch.full((need,), float("nan"), dtype=torch.float64, device=DEV)     # outputs start as NaN
        norm = torch.full((), float("nan"), device=DEV)
        before = [t.clone() for t in (p, m, v)] + [ema.clone() if ema_on else None]
        assert c_sqnorm(L, g, GSCALE, partials) == need
        c_adam_ex(L, p, g, m, v, ema, hyper, GSCALE, step_dev, partials, norm)
        norms.append(norm.clone())
        if check:
            what = f"n={n} step {k}"
            assert torch.equal(partials, O.sqnorm_partials(g, GSCALE)), f"{what}: partials are not the documented order"
            bound(f"{what} grad_norm", norm, *O.gnorm(g, GSCALE), "gnorm")
            clipped.append(O.clip_coef(float(norm), max_norm)[0] < 1.0)
            ref = O.adam_clip_step(before[0], g, before[1], before[2], k, float(norm), max_norm, lr=lr, gscale=GSCALE)
            for nm, got, (r, mag) in zip("pmv", (p, m, v), ref):
                bound(f"{what} {nm}", got, r, mag, "adam_clip")
            if ema_on:
                bound(f"{what} ema", ema, *O.ema_step(before[3], p, RATE), "ema")
    if check:
        assert clipped[0], clipped        # max_norm is half the first norm; a later step of a tiny n may stay under it
    return p, m, v, ema, norms, partials


@pytest.mark.parametrize("n", O.KERNEL_N)
def test_kernels_against_float64(ops, L, n):
    """Both bodies where n allows: the aligned buffers take the vector body when n % 4 == 0, the unaligned ones the scalar
    body; both must meet the bounds and each other bit for bit, and a second run must repeat the first."""
    a = run_kernels(ops, L, n, check=True)
    s = run_kernels(ops, L, n, shift=True, check=(n == 4))        # n = 4: the scalar body's only route to the bounds
    again = run_kernels(ops, L, n)
    for nm, x, y, z in zip(("p", "m", "v", "ema"), a, s, again):
        assert torch.equal(x, y), f"n={n} {nm}: aligned and unaligned buffers differ"
        assert torch.equal(x, z), f"n={n} {nm}: two runs differ"
    for x, y, z in zip(a[4], s[4], again[4]):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(a[5], s[5]) and torch.equal(a[5], again[5])


@pytest.mark.parametrize("n", O.KERNEL_N)
def test_no_clip_no_ema_is_bitwise_adam_step(ops, L, n):
    """max_grad_norm = 1e30 (coef = 1) and ema = NULL: the bits of msgm_adam_step with the same lr, over five steps."""
    p0, gs, _ = inputs(n)
    p, m, v, ema, norms, _ = run_kernels(ops, L, n, max_norm=1e30, ema_on=False)
    assert ema is None and all(bool(torch.isfinite(x)) for x in norms)
    q, qm, qv = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for k in range(1, STEPS + 1):
        ops.adam_step(q, gs[k - 1], qm, qv, step=k, lr=1e-3 * k, gscale=GSCALE)
    assert torch.equal(p, q) and torch.equal(m, qm) and torch.equal(v, qv)


def test_partials_of_two_buffers_give_one_global_norm(ops, L):
    """Each buffer writes its slice of one partials buffer; the update of either reads all of it."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    ga, gb = O.R.randn(3 * O.SLICE + 5, generator=gen, device=DEV) * 0.01, O.R.randn(4099, generator=gen, device=DEV) * 0.02
    ka, kb = ops.grad_sqnorm_partials(ga.numel()), ops.grad_sqnorm_partials(gb.numel())
    assert (ka, kb) == (4, 1)
    parts = torch.full((ka + kb,), float("nan"), dtype=torch.float64, device=DEV)
    ops.grad_sqnorm(ga, GSCALE, parts[:ka])
    ops.grad_sqnorm(gb, GSCALE, parts[ka:])
    hyper = ops.opt_hyper(DEV, 1e-3, max_grad_norm=1e-3)
    step_dev = torch.ones(1, dtype=torch.int64, device=DEV)
    norms = []
    for g in (ga, gb):
        p, m, v = torch.zeros_like(g), torch.zeros_like(g), torch.zeros_like(g)
        norm = torch.full((), float("nan"), device=DEV)
        ops.adam_step_ex(p, g, m, v, hyper, step_dev, gscale=GSCALE, partials=parts, grad_norm_out=norm)
        bound(f"global norm read by the buffer of {g.numel()}", norm, *O.gnorm(torch.cat([ga, gb]), GSCALE), "gnorm")
        ref = O.adam_clip_step(torch.zeros_like(g), g, torch.zeros_like(g), torch.zeros_like(g), 1, float(norm), 1e-3,
                               gscale=GSCALE)
        for nm, got, (r, mag) in zip("pmv", (p, m, v), ref):
            bound(f"two buffers, {g.numel()}: {nm}", got, r, mag, "adam_clip")
        norms.append(norm)
    assert torch.equal(norms[0], norms[1])


@pytest.mark.parametrize("n", (4, 7, 4096, 2097156 + 1))
def test_swap_twice_is_the_identity(ops, n):
    gen = torch.Generator(device=DEV).manual_seed(n)
    a0, b0 = O.R.randn(n, generator=gen, device=DEV), O.R.randn(n, generator=gen, device=DEV)
    for place in ((lambda t: t.clone()), shifted):               # vector body (n % 4 == 0, aligned) and scalar body
        a, b = place(a0), place(b0)
        ops.swap_(a, b)
        assert torch.equal(a, b0) and torch.equal(b, a0)
        ops.swap_(a, b)
        assert torch.equal(a, a0) and torch.equal(b, b0)


def test_nonfinite_norm_propagates(ops):
    """clip_grad_norm_(error_if_nonfinite=False): an inf gradient makes the norm inf and the coefficient 0 (0 * inf = NaN
    at that element, 0 elsewhere); a NaN gradient makes the coefficient NaN and poisons every element."""
    for bad, all_nan in ((float("inf"), False), (float("nan"), True)):
        g = torch.full((4096,), 0.01, device=DEV)
        g[17] = bad
        p, m, v = torch.ones(4096, device=DEV), torch.zeros(4096, device=DEV), torch.zeros(4096, device=DEV)
        norm = torch.zeros((), device=DEV)
        ops.adam_step_ex(p, g, m, v, ops.opt_hyper(DEV, 1e-3, max_grad_norm=1.0), torch.ones(1, dtype=torch.int64, device=DEV),
                         partials=ops.grad_sqnorm(g), grad_norm_out=norm)
        assert not bool(torch.isfinite(norm)) and bool(torch.isnan(p[17]))
        ok = torch.ones(4096, dtype=torch.bool, device=DEV)
        ok[17] = False
        assert bool(torch.isnan(p[ok]).all()) if all_nan else bool((p[ok] == 1.0).all())


# ================================================================================================ trainers
SCHEDULE = lambda k: 1e-3 / k                 # noqa: E731   distinct lr_k


def _x(B, d):
    return torch.randn(B, d, generator=torch.Generator().manual_seed(1)).to(DEV)


def make_trainer(kind, **kw):
    """'mlp': MLP(2), B = 64, SGM.  'mlp_msgm': MLP(6, NormalizeLogRadius) under the sparse multiplicative SDE.  'unet': the small 1-D U-Net,
    B = 4.  Same seeds every time, so two trainers of a kind start from the same bits."""
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.NNUnet1D import UNet1D
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    torch.manual_seed(0)
    if kind == "mlp":
        B, d = 64, 2
        tr = MLPScoreTrainer(make_gen("sgm", MLP(2)), B, lr=1e-3, seed=3, **kw)
    elif kind == "mlp_msgm":
        B, d = 64, 6
        tr = MLPScoreTrainer(make_gen("sparse", MLP(6, premodule="NormalizeLogRadius"), n=6, nsf=4), B, lr=1e-3, seed=3, **kw)
    else:
        B, d = 4, 16
        net = UNet1D(input_dim=16, base_channels=16, channel_mults=(1, 2), emb_dim=32)
        tr = UNetScoreTrainer(make_gen("sgm", net), B, d, lr=1e-3, seed=3, **kw)
    tr.set_data(_x(B, d))
    return tr


_PROBE = {}


def probe_norm(kind, **kw):
    """The gradient norm of the first step (a trainer that reports it and cannot clip)."""
    key = (kind, tuple(sorted(kw.items())))
    if key not in _PROBE:
        tr = make_trainer(kind, max_grad_norm=1e30, use_graph=False, **kw)
        tr.step()
        _PROBE[key] = float(tr.grad_norm)
        assert _PROBE[key] > 0
    return _PROBE[key]


def run_trainer(tr, steps=4, check=None):
    """``steps`` steps; check = (max_norm, rate, schedule): every step against the float64 restatement with that step's
    lr_k from the snapshot taken before it.  Returns (flat, ema, [losses], [norms])."""
    losses, norms = [], []
    for k in range(1, steps + 1):
        before = [t.clone() for t in (tr.flat, tr.m, tr.v)] + [None if tr.ema is None else tr.ema.clone()]
        losses.append(tr.step().clone())
        if tr.grad_norm is not None:
            norms.append(tr.grad_norm.clone())
        if check is not None:
            max_norm, rate, sched = check
            g, what = tr.gbuf[: tr.n], f"{type(tr).__name__} step {k}"
            assert int(tr.step_dev) == k
            bound(f"{what} grad_norm", tr.grad_norm, *O.gnorm(g, 1.0), "gnorm")
            assert O.clip_coef(float(tr.grad_norm), max_norm)[0] < 1.0, "clipping is not active"
            ref = O.adam_clip_step(before[0], g, before[1], before[2], k, float(tr.grad_norm), max_norm, lr=sched(k))
            for nm, got, (r, mag) in zip("pmv", (tr.flat, tr.m, tr.v), ref):
                bound(f"{what} {nm}", got, r, mag, "adam_clip")
            bound(f"{what} ema", tr.ema, *O.ema_step(before[3], tr.flat, rate), "ema")
    return tr.flat.clone(), None if tr.ema is None else tr.ema.clone(), losses, norms


@pytest.mark.parametrize("kind", ["mlp", "mlp_msgm", "unet"])
def test_trainer_steps_against_float64_graph_and_eager(kind):
    """Clipping at half the probed norm, EMA, a schedule of distinct lr_k: each of 4 graph-replayed steps against the
    restatement; the eager twin is bitwise the same; a constant-lr run is not."""
    max_norm = 0.5 * probe_norm(kind)
    kw = dict(max_grad_norm=max_norm, ema_rate=0.9)
    tr = make_trainer(kind, lr_schedule=SCHEDULE, use_graph=True, **kw)
    assert tr.device_lr and torch.equal(tr.ema, tr.flat)
    f, e, losses, norms = run_trainer(tr, check=(max_norm, 0.9, SCHEDULE))
    assert tr.graph is not None and tr.lr == SCHEDULE(4) and float(tr.hyper[0]) == SCHEDULE(4)
    f2, e2, losses2, norms2 = run_trainer(make_trainer(kind, lr_schedule=SCHEDULE, use_graph=False, **kw))
    assert torch.equal(f, f2) and torch.equal(e, e2)
    assert all(torch.equal(a, b) for a, b in zip(losses + norms, losses2 + norms2))
    f3, e3, _, _ = run_trainer(make_trainer(kind, use_graph=True, **kw))
    assert not torch.equal(f, f3) and not torch.equal(e, e3)


@pytest.mark.parametrize("kind", ["mlp", "unet"])
def test_default_trainer_never_reaches_the_new_kernels(kind, monkeypatch):
    from sdeflow_light_amd import ops as _ops

    def refuse(*a, **k):
        raise AssertionError("the default path called the option route")
    monkeypatch.setattr(_ops, "adam_step_ex", refuse)
    monkeypatch.setattr(_ops, "grad_sqnorm", refuse)
    tr = make_trainer(kind)
    assert not tr.device_lr and tr.hyper is None and tr.ema is None and tr.grad_norm is None
    p0 = tr.flat.clone()
    for _ in range(3):
        tr.step()
    assert not torch.equal(p0, tr.flat) and int(tr.step_dev) == 3
    assert set(tr.state_dict()) == {"state", "param_groups", "philox"}
    with pytest.raises(_ops.MsgmError, match="learning rate baked in"):
        tr.set_lr(5e-4)
    with pytest.raises(_ops.MsgmError, match="ema_rate"):
        tr.ema_state_dict()


def test_unet_option_route_that_cannot_clip_is_bitwise_the_default():
    f, _, losses, _ = run_trainer(make_trainer("unet", max_grad_norm=1e30))
    f0, _, losses0, _ = run_trainer(make_trainer("unet"))
    assert torch.equal(f, f0) and all(torch.equal(a, b) for a, b in zip(losses, losses0))


def test_mlp_option_route_that_cannot_clip_is_bitwise_the_split_default(monkeypatch):
    """The default MLP step on one GPU fuses the slab reduction with Adam; its reduce -> [all-reduce] -> adam_step branch
    (the N-rank one; without a process group the all-reduce is a no-op) is the one the option route mirrors."""
    from sdeflow_light_amd import parallel
    f, _, losses, _ = run_trainer(make_trainer("mlp", max_grad_norm=1e30))
    monkeypatch.setattr(parallel, "multi", lambda world: True)
    tr0 = make_trainer("mlp")
    assert not tr0.use_graph
    f0, _, losses0, _ = run_trainer(tr0)
    assert torch.equal(f, f0) and all(torch.equal(a, b) for a, b in zip(losses, losses0))


def test_unet_two_ranks_without_a_process_group():
    """world = 2: the graph ends before the collective and grad_sqnorm + adam_step_ex follow eagerly."""
    from sdeflow_light_amd import ops as _ops
    max_norm = 0.5 * probe_norm("unet", world=2)
    kw = dict(max_grad_norm=max_norm, ema_rate=0.9, lr_schedule=SCHEDULE, world=2)
    tr = make_trainer("unet", use_graph=True, **kw)
    f, e, losses, _ = run_trainer(tr, check=(max_norm, 0.9, SCHEDULE))
    assert tr.graph is not None and set(_ops.graph_node_kinds(tr.graph)) == {"kernel"}
    f2, e2, losses2, _ = run_trainer(make_trainer("unet", use_graph=False, **kw))
    assert torch.equal(f, f2) and torch.equal(e, e2) and all(torch.equal(a, b) for a, b in zip(losses, losses2))


def test_captured_option_step_holds_kernel_nodes_only():
    from sdeflow_light_amd import ops as _ops
    for kind in ("mlp", "unet"):
        tr = make_trainer(kind, max_grad_norm=1.0, ema_rate=0.9)
        tr.step()
        assert set(_ops.graph_node_kinds(tr.graph)) == {"kernel"}
        tr.set_lr(3e-4)                                      # between replays, no re-capture
        g = tr.graph
        tr.step()
        assert tr.graph is g and float(tr.hyper[0]) == 3e-4


def test_ema_weights_swap_unet1d():
    from sdeflow_light_amd import _lib
    from sdeflow_light_amd.NNUnet1D import UNet1D
    tr = make_trainer("unet", ema_rate=0.5)
    run_trainer(tr, steps=3)
    assert not torch.equal(tr.ema, tr.flat)
    x, t = _x(4, 16), torch.tensor([0.1, 0.4, 0.7, 1.0], device=DEV)
    net2 = UNet1D(input_dim=16, base_channels=16, channel_mults=(1, 2), emb_dim=32).to(DEV)
    sd = tr.ema_state_dict()
    assert list(sd) == list(tr.net.state_dict()) and all(sd[k].shape == v.shape for k, v in tr.net.state_dict().items())
    net2.load_state_dict(sd)
    p0, e0, live = tr.flat.clone(), tr.ema.clone(), tr.net(x, t).clone()
    addr = tr.flat.data_ptr()
    with tr.ema_weights():
        assert torch.equal(tr.flat, e0) and torch.equal(tr.ema, p0) and tr.flat.data_ptr() == addr
        out = tr.net(x, t).clone()
        for what in (tr.step, tr.capture):
            with pytest.raises(_lib.MsgmError, match="ema_weights"):
                what()
        with pytest.raises(_lib.MsgmError, match="nest"):
            with tr.ema_weights():
                pass
    assert torch.equal(out, net2(x, t)) and not torch.equal(out, live)
    assert torch.equal(tr.flat, p0) and torch.equal(tr.ema, e0) and torch.equal(tr.net(x, t), live)
    tr.step()                                                # and the trainer goes on


def test_ema_weights_swap_unet2d_packed_and_winograd_weights():
    """Forward only, B = 2: the 2-D U-Net's packed and Winograd weight images are rebuilt from the live bucket on every
    pass, so inside the context the forward is bitwise that of a second net holding the average, and a GraphedStepSampler
    captured before entering samples from the average (its pack launches are nodes of the graph)."""
    from oracle.det_params import load_det_
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from sdeflow_light_amd.sde_scheme import GraphedStepSampler
    from sdeflow_light_amd.train import UNetScoreTrainer
    mk = lambda: VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), in_space=16)      # noqa: E731
    net = mk()
    load_det_(net)
    tr = UNetScoreTrainer(make_gen("sgm", net), 2, 256, lr=1e-4, seed=1, ema_rate=0.9)
    tr.ema.mul_(1.0 + 0.05 * torch.sin(torch.arange(tr.n, device=DEV, dtype=torch.float32)))     # an average unlike the weights
    x, t = _x(2, 256), torch.tensor([0.3, 0.8], device=DEV)
    net2 = mk().to(DEV)
    net2.load_state_dict(tr.ema_state_dict())
    gs = GraphedStepSampler(tr.gen_sde, 2, 256, 2)           # a sampler graph captured BEFORE entering the context
    stream0 = gs.rng.state.clone()

    def sample():
        gs.rng.state.copy_(stream0)                          # the same noise every time
        return gs.run(x).clone()
    p0, live, s_live = tr.flat.clone(), tr.net(x, t).clone(), sample()
    with tr.ema_weights():
        out, s_ema = tr.net(x, t).clone(), sample()
    assert torch.equal(out, net2(x, t)) and not torch.equal(out, live)
    assert torch.equal(tr.flat, p0) and torch.equal(tr.net(x, t), live) and torch.equal(sample(), s_live)
    # the graph repacks its weight images on every replay: inside the context it sampled from the average
    tr.flat.copy_(tr.ema)
    assert torch.equal(sample(), s_ema) and not torch.equal(s_ema, s_live) and bool(torch.isfinite(s_ema).all())


def test_checkpoint_round_trip_and_adam_interchange():
    """2 steps, save, load into a fresh trainer built with another lr, 2 more steps: parameters, EMA and losses are the
    uninterrupted run's bits; the dictionary also loads into torch.optim.Adam(gen_sde.parameters())."""
    max_norm = 0.5 * probe_norm("mlp")
    kw = dict(max_grad_norm=max_norm, ema_rate=0.9)
    f, e, losses, _ = run_trainer(make_trainer("mlp", **kw))
    a = make_trainer("mlp", **kw)
    _, _, la, _ = run_trainer(a, steps=2)
    sd, model = a.state_dict(), {k: v.clone() for k, v in a.gen_sde.state_dict().items()}
    assert set(sd) == {"state", "param_groups", "philox", "ema"} and set(sd["ema"]) == set(sd["state"])
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.train import MLPScoreTrainer
    torch.manual_seed(123)
    gen = make_gen("sgm", MLP(2))
    b = MLPScoreTrainer(gen, 64, lr=7e-2, seed=99, **kw)
    gen.load_state_dict(model)
    b.load_state_dict(sd)
    b.set_data(_x(64, 2))
    assert b.lr == 1e-3 and float(b.hyper[0]) == 1e-3 and b._k == 2
    fb, eb, lb, _ = run_trainer(b, steps=2)
    assert torch.equal(fb, f) and torch.equal(eb, e) and all(torch.equal(x, y) for x, y in zip(la + lb, losses))
    sd2 = dict(b.state_dict())
    sd2["param_groups"] = [dict(sd2["param_groups"][0], lr=2e-4)]
    b.load_state_dict(sd2)                                   # after the capture: a device-lr trainer sets it
    assert b.graph is not None and float(b.hyper[0]) == 2e-4
    sd3 = {k: v for k, v in sd.items() if k != "ema"}        # a checkpoint without an average: seeded from the parameters
    b.load_state_dict(sd3)
    assert torch.equal(b.ema, b.flat)
    adam = torch.optim.Adam(a.gen_sde.parameters(), lr=1e-3)
    adam.load_state_dict(a.state_dict())
    got = [s["exp_avg"] for s in adam.state.values()]
    assert len(got) == len(list(a.net.parameters())) and torch.equal(torch.cat([q.reshape(-1) for q in got]), a.m)


def test_fused_adam_clip_and_ema_reference_loop():
    """The reference loop (MSGM_higherDim.py:803-809) with FusedAdam(max_grad_norm, ema_rate) on the MLP, lr changed
    through the param group between the steps as a torch lr_scheduler does."""
    from sdeflow_light_amd import _lib
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.optim import FusedAdam
    torch.manual_seed(0)
    net = MLP(2)
    gen = make_gen("sgm", net)
    x = _x(64, 2)
    gen.zero_grad()
    gen.ssm(x).mean().backward()
    flat, gflat = net.flat_parameters()
    max_norm, rate = 0.5 * float(gflat.double().norm()), 0.9
    opt = FusedAdam(gen.parameters(), lr=1e-3, max_grad_norm=max_norm, ema_rate=rate)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 1.0 / (e + 1))
    index = {id(p): i for i, p in enumerate(gen.parameters())}
    for k in range(1, 4):
        opt.zero_grad()
        gen.ssm(x).mean().backward()
        lr = opt.param_groups[0]["lr"]
        assert lr == pytest.approx(1e-3 / k)
        run = opt._runs[0] if opt._runs else None
        before = [flat.clone()] + ([run.m.clone(), run.v.clone(), run.ema.clone()] if run else
                                   [torch.zeros_like(flat), torch.zeros_like(flat), flat.clone()])
        opt.step()
        sched.step()
        run = opt._runs[0]
        assert len(opt._runs) == 1
        bound(f"FusedAdam step {k} grad_norm", opt.grad_norm, *O.gnorm(gflat, 1.0), "gnorm")
        assert O.clip_coef(float(opt.grad_norm), max_norm)[0] < 1.0
        ref = O.adam_clip_step(before[0], gflat, before[1], before[2], k, float(opt.grad_norm), max_norm, lr=lr)
        for nm, got, (r, mag) in zip("pmv", (flat, run.m, run.v), ref):
            bound(f"FusedAdam step {k} {nm}", got, r, mag, "adam_clip")
        bound(f"FusedAdam step {k} ema", run.ema, *O.ema_step(before[3], flat, rate), "ema")
    es = opt.ema_state_dict()
    assert sorted(es) == sorted(index[id(p)] for p in net.parameters())
    assert torch.equal(torch.cat([es[index[id(p)]].reshape(-1) for p in net.parameters()]), run.ema)
    assert all(es[index[id(p)]].shape == p.shape for p in net.parameters())
    # scattered gradients: refused, not silently updated without the global norm
    for p in net.parameters():
        p.grad = torch.zeros_like(p)                         # one run of parameters, gradients in separate buffers
    with pytest.raises(_lib.MsgmError, match="contiguous"):
        FusedAdam(net.parameters(), max_grad_norm=1.0).step()
