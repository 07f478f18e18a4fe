"""CPU checks of tests/optim_decay_ref.py: (1) the float64 restatement of both decay modes against torch.optim.Adam(weight_decay)
and torch.optim.AdamW with clip_grad_norm_; (2) the tolerance constants of tests/test_optim_decay_gpu.py are what the
restatement evaluated in float32 measures against float64 at the GPU test's shapes; (3) the guard's verdict and the
warm-up's rate at their edge cases; (4) host-side refusals that need no device."""
import math

import pytest
import torch

import optim_decay_ref as D
import optim_ref as O

F64 = torch.float64
EPS64 = 2.0 ** -53


def measure_torch64():
    """Worst |restatement64 - torch| / (2^-53 magnitude) over five steps, both modes, each from its own trajectory."""
    worst = 0.0
    for mode, cls in ((D.L2, torch.optim.Adam), (D.DECOUPLED, torch.optim.AdamW)):
        torch.manual_seed(4)
        n, max_norm, lr, wd = 50, 0.03, 2e-3, 0.05
        tp = torch.nn.Parameter(torch.randn(n, dtype=F64) * 0.1)
        opt = cls([tp], lr=lr, weight_decay=wd)
        p, m, v = tp.detach().clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
        clipped = []
        for step in range(1, 6):
            g = torch.randn(n, dtype=F64) * 0.01 * (0.25 if step % 2 else 1.0)      # odd steps stay under max_norm
            tp.grad = 0.5 * g
            tn = torch.nn.utils.clip_grad_norm_([tp], max_norm)
            opt.step()
            norm, mn = O.gnorm(g, 0.5)
            assert abs(float(norm) - float(tn)) <= 1e-12 * float(mn)
            clipped.append(O.clip_coef(float(norm), max_norm)[0] < 1.0)
            (p, mp), (m, mm), (v, mv) = D.decay_step(mode, wd, p, g, m, v, step, float(norm), max_norm, lr=lr, gscale=0.5)
            st = opt.state[tp]
            for q, qo, mag in ((p, tp.detach(), mp), (m, st["exp_avg"], mm), (v, st["exp_avg_sq"], mv)):
                worst = max(worst, float(((q - qo).abs() / (EPS64 * mag)).max()))
                assert bool((mag >= q.abs() * (1 - 1e-12)).all())
        assert any(clipped) and not all(clipped), clipped
    return worst


def test_restatement_equals_torch_float64(monkeypatch):
    """Ties the restatement to torch, not to the kernel.  The kernel's constants are float32-rounded doubles
    (sde_stage_ref.c32); with that rounding taken out (c32 = float in the three modules) the restatement differs from
    torch by reassociation only, and the bound is 4 x the figure measured here and written into MEASURED["torch64"], in
    units of 2^-53 magnitude.  With the rounding in, the two agree to 1e-6 of the magnitude per step taken
    (test_optim_ref's bound for the same reason)."""
    import sde_stage_ref as R
    rounded = measure_torch64()
    assert rounded * EPS64 <= 5e-6, rounded
    for mod in (R, O, D):
        monkeypatch.setattr(mod, "c32", float)
    r = measure_torch64()
    print(f"torch64: ratio {r:.3f} x 2^-53 magnitude (bound {D.c_of('torch64'):.1f}); with float32 constants {rounded:.4g}")
    assert r <= D.c_of("torch64"), (r, D.c_of("torch64"))


def test_decay_modes_differ_and_mode_none_is_adam_clip_step():
    p, draw = D.kernel_inputs(64)
    g, z = draw(), torch.zeros(64)
    a = D.decay_step(D.NONE, 0.05, p, g, z, z, 1, 1.0, 0.5)
    b = O.adam_clip_step(p, g, z, z, 1, 1.0, 0.5)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    l2, dec = (D.decay_step(md, 0.05, p, g, z, z, 1, 1.0, 0.5) for md in (D.L2, D.DECOUPLED))
    assert not torch.equal(l2[0][0], a[0][0]) and not torch.equal(dec[0][0], a[0][0]) and not torch.equal(l2[0][0], dec[0][0])
    assert torch.equal(dec[1][0], a[1][0]) and not torch.equal(l2[1][0], a[1][0])      # AdamW leaves the moments alone


# ------------------------------------------------------------------------------------------------ tolerance constants
def measure(n_list=D.KERNEL_N, steps=D.STEPS):
    """{family: worst |ref32 - ref64| / (2^-24 magnitude)} over the kernel cases of the GPU test: five steps from the
    float32 restatement's own state, gscale = 0.5, max_norm = half the first norm, wd = 0.05, EMA rate 0.999 with warm-up."""
    acc = {"adam_l2": 0.0, "adamw": 0.0, "ema_warmup": 0.0}
    for n in n_list:
        for mode, fam in ((D.L2, "adam_l2"), (D.DECOUPLED, "adamw")):
            p, draw = D.kernel_inputs(n)
            m, v, e = torch.zeros(n), torch.zeros(n), p.clone()
            max_norm = None
            for step in range(1, steps + 1):
                g = draw()
                n32 = O.gnorm(g, D.GSCALE, torch.float32)[0]
                if max_norm is None:
                    max_norm = 0.5 * float(n32)
                kw = dict(lr=1e-3 * step, gscale=D.GSCALE)
                r32 = D.decay_step(mode, D.WD, p, g, m, v, step, float(n32), max_norm, dtype=torch.float32, **kw)
                r64 = D.decay_step(mode, D.WD, p, g, m, v, step, float(n32), max_norm, **kw)
                for (got, _), (ref, mag) in zip(r32, r64):
                    acc[fam] = max(acc[fam], D.ratio(got, ref, mag))
                p, m, v = (q[0] for q in r32)
                e32 = D.ema_warmup_step(e, p, D.RATE, step, torch.float32)[0]
                acc["ema_warmup"] = max(acc["ema_warmup"], D.ratio(e32, *D.ema_warmup_step(e, p, D.RATE, step)))
                e = e32
    return acc


def test_tolerance_constants():
    got = measure()
    for fam, r in sorted(got.items()):
        c = D.c_of(fam)
        print(f"{fam:10s}: float32 restatement ratio {r:.3f}, c = {c:.2f}")
        assert r <= c / 4, (fam, r, c)
        assert r >= c / 16, (fam, r, c, "the constant is far above what float32 arithmetic needs: measure again")
    assert set(got) | {"torch64"} == set(D.MEASURED)


# ------------------------------------------------------------------------------------------------ guard and warm-up
def test_guard_verdict_cases():
    n = O.SLICE + 1                                          # two slices: the last element is alone in the last one
    base = D.kernel_inputs(n)[1]()
    assert not D.nonfinite_verdict([base], 1.0)
    for bad in (float("nan"), float("inf"), float("-inf")):
        g = base.clone()
        g[-1] = bad
        assert D.nonfinite_verdict([g], 1.0), bad
        assert D.nonfinite_verdict([base, g], 1.0) and D.nonfinite_verdict([g, base], 1.0)      # several buffers, one verdict
    g = base.clone()
    g[-1] = 3e38                                             # finite, but g * 2 overflows in float32
    assert not D.nonfinite_verdict([g], 1.0) and D.nonfinite_verdict([g], 2.0)
    g[-1] = 1e30                                             # finite and huge: clipped, never skipped (1e60 fits a double)
    assert not D.nonfinite_verdict([g], 1.0) and not D.nonfinite_verdict([g], 2.0)
    g = torch.full((7,), 3e38)                               # every square 9e76: the double sum stays finite
    assert not D.nonfinite_verdict([g], 1.0)


@pytest.mark.parametrize("rate", [0.9, 0.99, 0.999, 0.9999, 0.5, 0.1])
def test_warmup_meets_rate_exactly(rate):
    ks = [k for k in range(1, 200000) if (1.0 + k) / (10.0 + k) >= rate]
    k0 = ks[0] if ks else None
    assert k0 is not None
    for k in range(1, k0):
        assert D.warmup_rate(rate, k) == (1.0 + k) / (10.0 + k) < rate
    for k in (k0, k0 + 1, 10 * k0, 2 ** 20):
        assert D.warmup_rate(rate, k) == rate                # the float itself, not a neighbour
    e, p = torch.ones(3), torch.zeros(3)
    assert torch.equal(D.ema_warmup_step(e, p, rate, k0)[0], O.ema_step(e, p, rate)[0])
    assert float(D.ema_warmup_step(e, p, 0.999, 1)[0][0]) == pytest.approx(2.0 / 11.0, rel=1e-6)


# ------------------------------------------------------------------------------------------------ host side
def test_host_side_refusals_and_hyper_layout():
    from sdeflow_light_amd import ops, _lib
    from sdeflow_light_amd.optim import FusedAdam
    h = ops.optim_hyper("cpu", lr=3e-4, betas=(0.8, 0.9), eps=1e-6, max_grad_norm=2.0, ema_rate=0.5, weight_decay=0.01)
    assert h.dtype == torch.float64 and h.tolist() == [3e-4, 0.8, 0.9, 1e-6, 2.0, 0.5, 0.01]
    assert torch.equal(h[:6], ops.opt_hyper("cpu", lr=3e-4, betas=(0.8, 0.9), eps=1e-6, max_grad_norm=2.0, ema_rate=0.5))
    assert ops.OPT_WEIGHT_DECAY == 6 and (ops.DECAY_NONE, ops.DECAY_L2, ops.DECAY_DECOUPLED) == (D.NONE, D.L2, D.DECOUPLED)
    z = torch.zeros(8)
    with pytest.raises(_lib.MsgmError, match="no CPU fallback"):
        ops.optim_step(z, z, z.clone(), z.clone(), ops.optim_hyper("cpu"), torch.ones(1, dtype=torch.int64))
    w = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(_lib.MsgmError, match="weight_decay"):
        FusedAdam([w], weight_decay=-0.1)
    with pytest.raises(_lib.MsgmError, match="ema_rate"):
        FusedAdam([w], ema_warmup=True)
    opt = FusedAdam([{"params": [w]}, {"params": [torch.nn.Parameter(torch.zeros(2))], "weight_decay": 0.0}], weight_decay=0.1)
    assert [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0] and opt.skipped_steps == 0
