"""-m gpu: msgm_optim_step (csrc/optim_kernels.hip) — weight decay (L2 and decoupled), the non-finite step guard and the EMA
warm-up in the one pass of msgm_adam_step_ex — from the C ABI up to the trainers and FusedAdam.

Kernels: per element against the float64 restatement of tests/optim_decay_ref.py, |kernel - ref64| <= c * 2^-24 * magnitude
with c = 4 x the CPU float32 measurement (optim_decay_ref.MEASURED, guarded by tests/test_optim_decay_ref.py), fed the
kernel's OWN reported norm and, for the EMA, its own new parameters.  Bitwise: aligned against shifted buffers, two runs,
every option off against msgm_adam_step_ex, a skipped step against the clones taken before it.  n: 4 (vector body; scalar
through the shifted view), 7 (scalar tail), 4096, 8193 (two slices: verdict and norm cross workgroups), 2 097 156.

Trainers (the three kinds of tests/test_optim_stage_gpu.py): graph against eager and each step against the restatement, a
poisoned batch with and without the guard, kernel nodes only, the default route, checkpoints, FusedAdam with two groups.
"""
import pytest
import torch

import optim_decay_ref as D
import optim_ref as O
from test_optim_stage_gpu import _x, make_trainer, probe_norm, shifted

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMILY = {D.NONE: "adam_clip", D.L2: "adam_l2", D.DECOUPLED: "adamw"}


@pytest.fixture(scope="module")
def ops():
    from sdeflow_light_amd import ops as _ops
    _ops.lib()
    return _ops


def bound(what, y, ref, mag, family):
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite output"
    c = O.c_of(family) if family in O.MEASURED else D.c_of(family)
    r = D.ratio(y.reshape(-1), ref.reshape(-1), mag.reshape(-1))
    print(f"{what}: ratio {r:.3f} (bound {c:.1f})")
    assert r <= c, f"{what}: {r:.3f} x 2^-24 magnitude exceeds c = {c:.1f}"


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


_INPUTS = {}


def inputs(n):
    """(p0, [g_1 .. g_STEPS]) on the device, drawn once per n (one n resident at a time)."""
    if n not in _INPUTS:
        p, draw = D.kernel_inputs(n, device=DEV)
        gs = [draw() for _ in range(D.STEPS)]
        _INPUTS.clear()
        _INPUTS[n] = (p, gs)
    return _INPUTS[n]


def check_step(what, mode, before, after, g, k_eff, norm, max_norm, lr, gscale, rate, warm=True):
    """One update against the restatement evaluated at the effective count k_eff."""
    p, m, v, ema = after
    ref = D.decay_step(mode, D.WD, before[0], g, before[1], before[2], k_eff, float(norm), max_norm, lr=lr, gscale=gscale)
    for nm, got, (r, mag) in zip("pmv", (p, m, v), ref):
        bound(f"{what} {nm}", got, r, mag, FAMILY[mode])
    if ema is not None:
        e = D.ema_warmup_step(before[3], p, rate, k_eff) if warm else O.ema_step(before[3], p, rate)
        bound(f"{what} ema", ema, *e, "ema_warmup" if warm else "ema")


def run_kernels(ops, n, mode, shift=False, check=False, guard=False, poison=None, steps=D.STEPS, gscale=D.GSCALE):
    """``steps`` steps of grad_sqnorm + optim_step from the kernel's own state with clipping at half the first norm, EMA
    with warm-up and lr_k = 1e-3 k.  poison = (k, f): f(g) spoils the gradient of step k, which must then change nothing.
    Returns (p, m, v, ema, [reported norms], skipped count)."""
    p0, gs = inputs(n)
    max_norm = 0.5 * float(O.gnorm(gs[0], gscale)[0])
    place = shifted if shift else (lambda t: t.clone())
    p, m, v, ema = place(p0), place(torch.zeros_like(p0)), place(torch.zeros_like(p0)), place(p0)
    hyper = ops.optim_hyper(DEV, 1e-3, max_grad_norm=max_norm, ema_rate=D.RATE, weight_decay=D.WD)
    step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
    skipped = ops.skipped_counter(DEV) if guard else None
    need, norms, done = ops.grad_sqnorm_partials(n), [], 0
    for k in range(1, steps + 1):
        g = gs[k - 1].clone()
        bad = poison is not None and poison[0] == k
        if bad:
            poison[1](g)
        g = place(g)
        lr = 1e-3 * k
        hyper[ops.OPT_LR:ops.OPT_LR + 1].fill_(lr)
        ops.counter_inc(step_dev)
        partials = torch.full((need,), float("nan"), dtype=torch.float64, device=DEV)
        norm = torch.full((), float("nan"), device=DEV) if not bad else torch.zeros((), device=DEV)
        before = [t.clone() for t in (p, m, v, ema)]
        ops.grad_sqnorm(g, gscale, partials)
        ops.optim_step(p, g, m, v, hyper, step_dev, ema=ema, gscale=gscale, partials=partials, grad_norm_out=norm,
                       clip=True, decay_mode=mode, skipped=skipped, ema_warmup=True)
        norms.append(norm.clone())
        what = f"n={n} mode {mode} step {k}"
        if bad:
            assert D.nonfinite_verdict([g], gscale), "the test's own poison is not one"
            done += 1
            for nm, x, y in zip(("p", "m", "v", "ema"), (p, m, v, ema), before):
                assert same_bits(x, y), f"{what}: {nm} changed in a skipped step"
            assert not bool(torch.isfinite(norm)), f"{what}: reported norm {float(norm)} of a skipped step"
        elif check:
            check_step(what, mode, before, (p, m, v, ema), g, k - done, norm, max_norm, lr, gscale, D.RATE)
        if guard:
            assert ops.skipped_count(skipped, step_dev) == done, f"{what}: skipped count"
    return p, m, v, ema, norms, done


# ================================================================================================ kernels
@pytest.mark.parametrize("mode", [D.L2, D.DECOUPLED])
@pytest.mark.parametrize("n", D.KERNEL_N)
def test_kernels_against_float64(ops, n, mode):
    """Five steps, clipping, EMA + warm-up: p, m, v, ema per element within the bound; aligned and shifted buffers agree
    bit for bit (n = 4: the scalar body's only route to the bounds), and so do two runs."""
    a = run_kernels(ops, n, mode, check=True)
    s = run_kernels(ops, n, mode, shift=True, check=(n == 4))
    again = run_kernels(ops, n, mode)
    for nm, x, y, z in zip(("p", "m", "v", "ema"), a, s, again):
        assert torch.equal(x, y), f"n={n} {nm}: aligned and shifted buffers differ"
        assert torch.equal(x, z), f"n={n} {nm}: two runs differ"
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(a[4], s[4], again[4]))


@pytest.mark.parametrize("n", D.KERNEL_N)
def test_options_off_is_bitwise_adam_step_ex(ops, n):
    """Mode 0, no guard, no warm-up through the new entry: the bits of msgm_adam_step_ex over five steps, with clipping and
    EMA and without either, for a p that holds an Inf (g + 0 * p would make it NaN) while the device weight_decay is 0.05."""
    p0, gs = inputs(n)
    p0 = p0.clone()
    p0[1] = float("inf")
    max_norm = 0.5 * float(O.gnorm(gs[0], D.GSCALE)[0])
    for clip_ema in (True, False):
        outs = []
        for new in (False, True):
            p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
            ema = p0.clone() if clip_ema else None
            args = (DEV, 1e-3, (0.9, 0.999), 1e-8, max_norm, D.RATE)
            hyper = ops.optim_hyper(*args, weight_decay=D.WD) if new else ops.opt_hyper(*args)
            step_dev = torch.zeros(1, dtype=torch.int64, device=DEV)
            norm = torch.zeros((), device=DEV)
            for k in range(1, D.STEPS + 1):
                ops.counter_inc(step_dev)
                parts = ops.grad_sqnorm(gs[k - 1], D.GSCALE) if clip_ema else None
                kw = dict(ema=ema, gscale=D.GSCALE, partials=parts, grad_norm_out=norm if clip_ema else None)
                if new:
                    ops.optim_step(p, gs[k - 1], m, v, hyper, step_dev, decay_mode=ops.DECAY_NONE, **kw)
                else:
                    ops.adam_step_ex(p, gs[k - 1], m, v, hyper, step_dev, **kw)
            outs.append([p, m, v, norm] + ([ema] if clip_ema else []))
        assert bool(torch.isinf(outs[0][0][1])) and int(torch.isfinite(outs[0][0]).sum()) == n - 1
        assert all(same_bits(x, y) for x, y in zip(*outs)), f"n={n} clip/ema {clip_ema}"


def _nan_last(g):
    g[-1] = float("nan")


def _overflow(g):
    g[3] = 3e38                                              # finite; times gscale = 2 it overflows in float32


SKIP_CASES = [(O.SLICE + 1, _nan_last, D.GSCALE), (7, _overflow, 2.0)]


@pytest.mark.parametrize("n,poison,gscale", SKIP_CASES)
@pytest.mark.parametrize("mode", [D.L2, D.DECOUPLED])
def test_skipped_step_changes_nothing(ops, n, poison, gscale, mode):
    """Step 2 of 4 is non-finite (a NaN alone in the second slice; a product that overflows): p, m, v, ema are bitwise
    the clones taken before it, the reported norm is non-finite, the skipped count is 1 (asserted in run_kernels)."""
    for shift in (False, True):
        out = run_kernels(ops, n, mode, shift=shift, guard=True, poison=(2, poison), steps=4, gscale=gscale)
        assert out[5] == 1 and all(bool(torch.isfinite(t).all()) for t in out[:4])
        assert [bool(torch.isfinite(x)) for x in out[4]] == [True, False, True, True]


@pytest.mark.parametrize("n,poison,gscale", SKIP_CASES)
@pytest.mark.parametrize("mode", [D.L2, D.DECOUPLED])
def test_effective_step_count_after_a_skip(ops, n, poison, gscale, mode):
    """Steps 3 and 4 after the skip meet the restatement at k_eff = 2 and 3 (bias corrections and warm-up); the attempt
    count would miss by tens of percent."""
    run_kernels(ops, n, mode, check=True, guard=True, poison=(2, poison), steps=4, gscale=gscale)


def test_guard_without_a_skip_is_bitwise_the_unguarded_run(ops):
    for mode in (D.L2, D.DECOUPLED):
        a, b = run_kernels(ops, 8193, mode), run_kernels(ops, 8193, mode, guard=True)
        assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and b[5] == 0


def test_finite_huge_gradient_is_clipped_not_skipped(ops):
    n = 4096
    g = torch.full((n,), 1e30, device=DEV)
    p0 = D.kernel_inputs(n, device=DEV)[0]
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    step_dev, skipped = torch.ones(1, dtype=torch.int64, device=DEV), ops.skipped_counter(DEV)
    norm = torch.zeros((), device=DEV)
    ops.optim_step(p, g, m, v, ops.optim_hyper(DEV, 1e-3, max_grad_norm=1.0), step_dev, partials=ops.grad_sqnorm(g),
                   grad_norm_out=norm, clip=True, skipped=skipped)
    assert ops.skipped_count(skipped, step_dev) == 0 and bool(torch.isfinite(norm)) and float(norm) > 1e31
    assert not torch.equal(p, p0)
    check_step("g = 1e30", D.NONE, (p0, torch.zeros_like(p0), torch.zeros_like(p0), None), (p, m, v, None), g, 1, norm, 1.0,
               1e-3, 1.0, None)


def test_two_buffers_one_counter(ops):
    """The second buffer's gradient is poisoned: both buffers stay untouched and the count rises by one, not two; the next
    (finite) step updates both at k_eff = 1."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    sizes = (3 * O.SLICE + 5, 4099)
    ps = [O.R.randn(k, generator=gen, device=DEV) * 0.1 for k in sizes]
    ms, vs = [torch.zeros_like(q) for q in ps], [torch.zeros_like(q) for q in ps]
    es = [q.clone() for q in ps]
    ks = [ops.grad_sqnorm_partials(k) for k in sizes]
    hyper = ops.optim_hyper(DEV, 1e-3, max_grad_norm=1e-3, ema_rate=D.RATE, weight_decay=D.WD)
    step_dev, skipped = torch.zeros(1, dtype=torch.int64, device=DEV), ops.skipped_counter(DEV)
    for attempt, eff in ((1, None), (2, 1)):
        gs = [O.R.randn(k, generator=gen, device=DEV) * 0.01 for k in sizes]
        if eff is None:
            gs[1][-1] = float("nan")
        parts = torch.full((sum(ks),), float("nan"), dtype=torch.float64, device=DEV)
        ops.grad_sqnorm(gs[0], D.GSCALE, parts[:ks[0]])
        ops.grad_sqnorm(gs[1], D.GSCALE, parts[ks[0]:])
        ops.counter_inc(step_dev)
        before = [[t.clone() for t in grp] for grp in (ps, ms, vs, es)]
        norm = torch.zeros((), device=DEV)
        for i in range(2):
            ops.optim_step(ps[i], gs[i], ms[i], vs[i], hyper, step_dev, ema=es[i], gscale=D.GSCALE, partials=parts,
                           grad_norm_out=norm, clip=True, decay_mode=ops.DECAY_DECOUPLED, skipped=skipped, ema_warmup=True)
        assert ops.skipped_count(skipped, step_dev) == 1
        for i in range(2):
            if eff is None:
                assert all(same_bits(now[i], was[i]) for now, was in zip((ps, ms, vs, es), before))
                assert not bool(torch.isfinite(norm))
            else:
                check_step(f"buffer {i} after the skip", D.DECOUPLED, [grp[i] for grp in before],
                           (ps[i], ms[i], vs[i], es[i]), gs[i], eff, norm, 1e-3, 1e-3, D.GSCALE, D.RATE)


def test_wrapper_refusals(ops):
    z = torch.zeros(8, device=DEV)
    h, st = ops.optim_hyper(DEV), torch.ones(1, dtype=torch.int64, device=DEV)
    with pytest.raises(ops.MsgmError, match="partials"):
        ops.optim_step(z, z, z.clone(), z.clone(), h, st, skipped=ops.skipped_counter(DEV))
    with pytest.raises(ops.MsgmError, match="ema"):
        ops.optim_step(z, z, z.clone(), z.clone(), h, st, ema_warmup=True)
    with pytest.raises(ops.MsgmError, match="decay_mode"):
        ops.optim_step(z, z, z.clone(), z.clone(), h, st, decay_mode=3)
    with pytest.raises(ops.MsgmError, match="hyper"):
        ops.optim_step(z, z, z.clone(), z.clone(), ops.opt_hyper(DEV), st)


# ================================================================================================ trainers
KINDS = ["mlp", "mlp_msgm", "unet"]
RATE_T = 0.9


def mode_of(tr):
    return tr.decay_mode


def step_checked(tr, k_eff, what, max_norm):
    """One step against the restatement at the effective count, given the trainer's own gradient."""
    before = [t.clone() for t in (tr.flat, tr.m, tr.v)] + [None if tr.ema is None else tr.ema.clone()]
    loss = tr.step().clone()
    g = tr.gbuf[: tr.n]
    bound(f"{what} grad_norm", tr.grad_norm, *O.gnorm(g, 1.0), "gnorm")
    check_step(what, mode_of(tr), before, (tr.flat, tr.m, tr.v, tr.ema), g, k_eff, tr.grad_norm, max_norm, tr.lr, 1.0,
               RATE_T, warm=tr.ema_warmup)
    return loss


@pytest.mark.parametrize("decoupled", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_trainer_graph_against_eager_and_float64(kind, decoupled):
    max_norm = 0.5 * probe_norm(kind)
    kw = dict(weight_decay=D.WD, decoupled_weight_decay=decoupled, max_grad_norm=max_norm, ema_rate=RATE_T, ema_warmup=True)
    tr = make_trainer(kind, use_graph=True, **kw)
    assert tr.device_lr and tr.decay_mode == (D.DECOUPLED if decoupled else D.L2) and tr.hyper.numel() == 7
    losses = [step_checked(tr, k, f"{kind} graph step {k}", max_norm) for k in range(1, 5)]
    assert tr.graph is not None and O.clip_coef(float(tr.grad_norm), max_norm)[0] < 1.0 and tr.skipped_steps == 0
    te = make_trainer(kind, use_graph=False, **kw)
    losses2 = [te.step().clone() for _ in range(4)]
    assert torch.equal(tr.flat, te.flat) and torch.equal(tr.ema, te.ema) and torch.equal(tr.m, te.m)
    assert all(torch.equal(a, b) for a, b in zip(losses, losses2))
    plain = make_trainer(kind, max_grad_norm=max_norm, ema_rate=RATE_T)
    for _ in range(4):
        plain.step()
    assert not torch.equal(plain.flat, tr.flat) and not torch.equal(plain.ema, tr.ema)


def poisoned_x(B, d):
    x = _x(B, d)
    x[B // 2, d - 1] = float("inf")
    return x


@pytest.mark.parametrize("kind", KINDS)
def test_trainer_poisoned_step(kind):
    """set_data with one inf entry makes step 2 non-finite.  With skip_nonfinite the bucket, m, v and the average are
    bitwise unchanged, the count is 1 and the next (finite) step meets the restatement at k_eff = 2; without it the
    parameters end as NaN: the behaviour the guard exists for."""
    kw = dict(weight_decay=D.WD, ema_rate=RATE_T, ema_warmup=True)
    tr = make_trainer(kind, skip_nonfinite=True, **kw)
    B, d = tr.x.shape
    assert tr.grad_norm is not None and tr.max_grad_norm is None
    tr.step()
    tr.set_data(poisoned_x(B, d))
    before = [t.clone() for t in (tr.flat, tr.m, tr.v, tr.ema)]
    tr.step()
    assert not bool(torch.isfinite(tr.grad_norm)) and tr.skipped_steps == 1 and int(tr.step_dev) == 2
    for nm, now, was in zip(("flat", "m", "v", "ema"), (tr.flat, tr.m, tr.v, tr.ema), before):
        assert same_bits(now, was), f"{kind}: {nm} changed in the skipped step"
    tr.set_data(_x(B, d))
    step_checked(tr, 2, f"{kind} step after the skip", None)
    assert tr.skipped_steps == 1 and int(tr.step_dev) == 3 and bool(torch.isfinite(tr.flat).all())
    assert float(tr.state_dict()["state"][max(tr.state_dict()["state"])]["step"]) == 2.0
    bare = make_trainer(kind, **kw)
    bare.step()
    bare.set_data(poisoned_x(B, d))
    bare.step()
    bare.set_data(_x(B, d))
    bare.step()
    assert bare.skipped_steps == 0 and not bool(torch.isfinite(bare.flat).any())


def test_captured_step_with_every_option_holds_kernel_nodes_only():
    from sdeflow_light_amd import ops as _ops
    for kind in ("mlp", "unet"):
        tr = make_trainer(kind, max_grad_norm=1.0, ema_rate=0.9, weight_decay=D.WD, skip_nonfinite=True, ema_warmup=True)
        tr.step()
        assert set(_ops.graph_node_kinds(tr.graph)) == {"kernel"}
        g = tr.graph
        tr.step()
        assert tr.graph is g and tr.skipped_steps == 0


@pytest.mark.parametrize("kind", ["mlp", "unet"])
def test_trainers_without_the_new_options_never_reach_the_new_wrapper(kind, monkeypatch):
    from sdeflow_light_amd import ops as _ops

    def refuse(*a, **k):
        raise AssertionError("a trainer without the new options called optim_step")
    monkeypatch.setattr(_ops, "optim_step", refuse)
    for kw in ({}, dict(max_grad_norm=1.0, ema_rate=0.9), dict(weight_decay=0.0, decoupled_weight_decay=False)):
        tr = make_trainer(kind, **kw)
        for _ in range(2):
            tr.step()
        assert tr.skipped is None and tr.skipped_steps == 0 and "skipped" not in tr.state_dict()
        assert tr.hyper is None or tr.hyper.numel() == 6
        grp = tr.state_dict()["param_groups"][0]
        assert grp["weight_decay"] == 0 and grp["decoupled_weight_decay"] is False
    assert not make_trainer(kind).device_lr
    with pytest.raises(AssertionError, match="optim_step"):
        make_trainer(kind, ema_rate=0.9, ema_warmup=True).step()


def test_trainer_refusals_at_construction():
    from sdeflow_light_amd import _lib
    with pytest.raises(_lib.MsgmError, match="weight_decay"):
        make_trainer("mlp", weight_decay=-1e-3)
    with pytest.raises(_lib.MsgmError, match="ema_rate"):
        make_trainer("mlp", ema_warmup=True)
    with pytest.raises(_lib.MsgmError, match="ema_rate"):
        make_trainer("unet", ema_warmup=True)


def test_checkpoint_round_trip_across_a_skipped_step():
    """Steps 1, 2 (skipped), save, load into a fresh trainer, steps 3, 4: the bits of the uninterrupted run.  The
    dictionary holds the effective count, the truthful decay settings and "skipped"; torch.optim.AdamW loads it; a
    checkpoint without "skipped" loads with count 0."""
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.train import MLPScoreTrainer
    from test_host_gpu import make_gen
    kw = dict(weight_decay=D.WD, skip_nonfinite=True, max_grad_norm=0.5 * probe_norm("mlp"), ema_rate=RATE_T, ema_warmup=True,
              lr_schedule=lambda k: 1e-3 / k)

    def two_and_two(tr, first=True, second=True):
        out = []
        if first:
            out.append(tr.step().clone())
            tr.set_data(poisoned_x(64, 2))
            out.append(tr.step().clone())
        if second:
            tr.set_data(_x(64, 2))
            out += [tr.step().clone(), tr.step().clone()]
        return out
    whole = make_trainer("mlp", **kw)
    lw = two_and_two(whole)
    assert whole.skipped_steps == 1 and int(whole.step_dev) == 4
    a = make_trainer("mlp", **kw)
    la = two_and_two(a, second=False)
    sd, model = a.state_dict(), {k: v.clone() for k, v in a.gen_sde.state_dict().items()}
    assert set(sd) == {"state", "param_groups", "philox", "ema", "skipped"} and sd["skipped"] == 1
    assert all(float(e["step"]) == 1.0 for e in sd["state"].values())
    assert sd["param_groups"][0]["weight_decay"] == D.WD and sd["param_groups"][0]["decoupled_weight_decay"] is True
    torch.manual_seed(123)
    gen = make_gen("sgm", MLP(2))
    b = MLPScoreTrainer(gen, 64, lr=7e-2, seed=99, **kw)
    gen.load_state_dict(model)
    b.load_state_dict(sd)
    assert b.skipped_steps == 1 and int(b.step_dev) == 2 and b._k == 2
    lb = two_and_two(b, first=False)
    assert torch.equal(b.flat, whole.flat) and torch.equal(b.ema, whole.ema) and torch.equal(b.m, whole.m)
    assert all(same_bits(x, y) for x, y in zip(la + lb, lw))
    assert b.skipped_steps == 1 and float(b.state_dict()["state"][1]["step"]) == 3.0
    adamw = torch.optim.AdamW(a.gen_sde.parameters(), lr=1e-3)
    adamw.load_state_dict(a.state_dict())
    assert adamw.param_groups[0]["weight_decay"] == D.WD
    got = [s["exp_avg"] for s in adamw.state.values()]
    assert torch.equal(torch.cat([q.reshape(-1) for q in got]), a.m) and all(float(s["step"]) == 1.0 for s in adamw.state.values())
    old = {k: v for k, v in sd.items() if k != "skipped"}
    b.load_state_dict(old)
    assert b.skipped_steps == 0 and int(b.step_dev) == 1 and b._k == 1


# ================================================================================================ FusedAdam
def _two_groups(**kw):
    from sdeflow_light_amd.optim import FusedAdam
    gen = torch.Generator(device=DEV).manual_seed(11)
    a = torch.nn.Parameter(O.R.randn(O.SLICE + 1, generator=gen, device=DEV) * 0.1)
    b = torch.nn.Parameter(O.R.randn(37, generator=gen, device=DEV) * 0.1)
    opt = FusedAdam([{"params": [a]}, {"params": [b], "weight_decay": 0.0}], lr=1e-3, weight_decay=D.WD, **kw)
    return a, b, opt, gen


def test_fused_adam_two_groups_follow_torch_adamw():
    """Two param groups, one without decay, three steps with the lr changed through the groups: each step from the
    optimizer's own state against clip_grad_norm_ + torch.optim.AdamW in float64 (and against the restatement)."""
    max_norm = 0.05
    a, b, opt, gen = _two_groups(max_grad_norm=max_norm)
    ra, rb = (torch.nn.Parameter(q.detach().double().cpu()) for q in (a, b))
    ref = torch.optim.AdamW([{"params": [ra]}, {"params": [rb], "weight_decay": 0.0}], lr=1e-3, weight_decay=D.WD)
    for k in range(1, 4):
        lr = 1e-3 / k
        for grp in opt.param_groups + ref.param_groups:
            grp["lr"] = lr
        a.grad, b.grad = (O.R.randn(q.numel(), generator=gen, device=DEV) * 0.01 for q in (a, b))
        before = {}
        for q, r in ((a, ra), (b, rb)):
            st = opt.state.get(q, {})
            m0 = st["exp_avg"].clone() if st else torch.zeros_like(q)
            v0 = st["exp_avg_sq"].clone() if st else torch.zeros_like(q)
            before[q] = (q.detach().clone(), m0, v0)
            r.data.copy_(q.detach().double().cpu())
            r.grad = q.grad.double().cpu()
            ref.state[r] = {"step": torch.tensor(float(k - 1)), "exp_avg": m0.double().cpu(), "exp_avg_sq": v0.double().cpu()}
        torch.nn.utils.clip_grad_norm_([ra, rb], max_norm)
        ref.step()
        opt.step()
        assert O.clip_coef(float(opt.grad_norm), max_norm)[0] < 1.0
        bound(f"FusedAdam step {k} grad_norm", opt.grad_norm, *O.gnorm(torch.cat([a.grad, b.grad]), 1.0), "gnorm")
        for q, r, mode in ((a, ra, D.DECOUPLED), (b, rb, D.NONE)):
            p0, m0, v0 = before[q]
            st = opt.state[q]
            assert float(st["step"]) == k
            rs = D.decay_step(mode, D.WD, p0, q.grad, m0, v0, k, float(opt.grad_norm), max_norm, lr=lr)
            for nm, got, (val, mag), tv in zip("pmv", (q.detach(), st["exp_avg"], st["exp_avg_sq"]), rs,
                                              (r.detach(), ref.state[r]["exp_avg"], ref.state[r]["exp_avg_sq"])):
                bound(f"FusedAdam step {k} group mode {mode} {nm} (restatement)", got, val, mag, FAMILY[mode])
                bound(f"FusedAdam step {k} group mode {mode} {nm} (torch AdamW)", got, tv.to(DEV), mag, FAMILY[mode])
    assert opt.skipped_steps == 0 and "skipped" not in opt.state_dict()


def test_fused_adam_poisoned_grad_leaves_both_groups_untouched():
    a, b, opt, gen = _two_groups(skip_nonfinite=True, ema_rate=RATE_T, ema_warmup=True)
    for k, bad in ((1, False), (2, True), (3, False)):
        a.grad, b.grad = (O.R.randn(q.numel(), generator=gen, device=DEV) * 0.01 for q in (a, b))
        if bad:
            b.grad[5] = float("nan")
        was = [t.detach().clone() for t in (a, b)] + ([r.m.clone() for r in opt._runs] + [r.v.clone() for r in opt._runs]
                                                     + [r.ema.clone() for r in opt._runs] if opt._runs else [])
        opt.step()
        now = [a.detach(), b.detach()] + [r.m for r in opt._runs] + [r.v for r in opt._runs] + [r.ema for r in opt._runs]
        if bad:
            assert all(same_bits(x, y) for x, y in zip(now, was)) and not bool(torch.isfinite(opt.grad_norm))
        else:
            assert not torch.equal(now[0], was[0]) and not torch.equal(now[1], was[1])
        eff = k - (1 if k >= 2 else 0)
        assert opt.skipped_steps == (1 if k >= 2 else 0) and all(float(opt.state[q]["step"]) == eff for q in (a, b))
    sd = opt.state_dict()
    assert sd["skipped"] == 1 and all(float(s["step"]) == 2.0 for s in sd["state"].values())
    a2, b2, opt2, _ = _two_groups(skip_nonfinite=True, ema_rate=RATE_T, ema_warmup=True)
    opt2.load_state_dict(sd)
    assert opt2.skipped_steps == 1 and int(opt2._step_dev) == 3 and opt2._step_host == 3
