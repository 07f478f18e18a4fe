"""CPU checks of tests/optim_ref.py: (1) the float64 restatement equals torch.optim.Adam + clip_grad_norm_ + the
reference's update_ema formula; (2) the tolerance constants of tests/test_optim_stage_gpu.py are what the restatement
evaluated in float32 measures against float64 at the GPU test's shapes (protocol of test_sde_stage_ref.py); (3) host-side
behaviour of the new wrappers, the ready-made schedule and the slice layout."""
import math

import pytest
import torch

import optim_ref as O

F64 = torch.float64


def test_restatement_equals_torch_adam_clip_ema_float64():
    """float64 torch.optim.Adam fed gradients scaled by 0.5 and clipped by clip_grad_norm_, then update_ema's
    mul_(rate).add_(src, alpha=1 - rate) (model/nn_utils.py:117-127).  The restatement carries the kernel's float32-rounded
    constants, so the two agree to 1e-6 of the magnitude per step taken (test_adam_equals_oracle_float64's bound)."""
    torch.manual_seed(4)
    n, max_norm, rate, lr = 50, 0.03, 0.99, 2e-3
    tp = torch.nn.Parameter(torch.randn(n, dtype=F64) * 0.1)
    opt = torch.optim.Adam([tp], lr=lr)
    te = tp.detach().clone()
    p, m, v, e = tp.detach().clone(), torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64), te.clone()
    clipped = []
    for step in range(1, 6):
        g = torch.randn(n, dtype=F64) * 0.01 * (0.25 if step % 2 else 1.0)      # odd steps stay under max_norm
        tp.grad = 0.5 * g
        tn = torch.nn.utils.clip_grad_norm_([tp], max_norm)
        opt.step()
        te.mul_(rate).add_(tp.detach(), alpha=1 - rate)
        norm, mn = O.gnorm(g, 0.5)
        assert abs(float(norm) - float(tn)) <= 1e-12 * float(mn)
        clipped.append(O.clip_coef(float(norm), max_norm)[0] < 1.0)
        (p, mp), (m, mm), (v, mv) = O.adam_clip_step(p, g, m, v, step, float(norm), max_norm, lr=lr, gscale=0.5)
        e, me = O.ema_step(e, p, rate)
        st = opt.state[tp]
        for q, qo, mag in ((p, tp.detach(), mp), (m, st["exp_avg"], mm), (v, st["exp_avg_sq"], mv), (e, te, me)):
            assert float(((q - qo).abs() / mag).max()) <= 1e-6 * step
            assert bool((mag >= q.abs() * (1 - 1e-12)).all())
    assert any(clipped) and not all(clipped), clipped


def test_float32_sqnorm_is_the_documented_order():
    """The float32 restatement's partials are per slice, their count is the layout's, and a plain double loop in the
    documented order gives the same bits at a small n with a ragged last quad."""
    n = 2 * O.SLICE + 1027
    g = O.R.randn(n, generator=torch.Generator().manual_seed(1))
    parts = O.sqnorm_partials(g, 0.5)
    assert parts.numel() == O.n_partials(n) == 3
    gg = (g * 0.5).double()
    lanes = [0.0] * 256
    seg = gg[2 * O.SLICE:]
    for e in range(seg.numel()):
        lanes[(e // 4) % 256] += float(seg[e]) ** 2
    w = []
    for k in range(4):
        a = lanes[64 * k:64 * k + 64]
        while len(a) > 1:
            h = len(a) // 2
            a = [a[i] + a[i + h] for i in range(h)]
        w.append(a[0])
    assert float(parts[2]) == (w[0] + w[1]) + (w[2] + w[3])
    s32, s64 = O.sqnorm(g, 0.5, torch.float32)[0], O.sqnorm(g, 0.5)[0]
    assert abs(float(s32) - float(s64)) <= 1e-13 * float(s64)


# ------------------------------------------------------------------------------------------------ tolerance constants
def measure(n_list=O.KERNEL_N, steps=5):
    """{family: worst |ref32 - ref64| / (2^-24 magnitude)} over the kernel cases of the GPU test: five steps from the
    float32 restatement's own state, gscale = 0.5, max_norm = half the first norm (clipping active), EMA rate 0.999."""
    acc = {"gnorm": 0.0, "adam_clip": 0.0, "ema": 0.0}
    for n in n_list:
        p, draw = O.kernel_inputs(n)
        m, v, e = torch.zeros(n), torch.zeros(n), p.clone()
        max_norm = None
        for step in range(1, steps + 1):
            g = draw()
            n32 = O.gnorm(g, 0.5, torch.float32)[0]
            acc["gnorm"] = max(acc["gnorm"], O.ratio(n32, *O.gnorm(g, 0.5)))
            if max_norm is None:
                max_norm = 0.5 * float(n32)
            kw = dict(lr=1e-3 * step, gscale=0.5)
            r32 = O.adam_clip_step(p, g, m, v, step, float(n32), max_norm, dtype=torch.float32, **kw)
            r64 = O.adam_clip_step(p, g, m, v, step, float(n32), max_norm, **kw)
            for (got, _), (ref, mag) in zip(r32, r64):
                acc["adam_clip"] = max(acc["adam_clip"], O.ratio(got, ref, mag))
            p, m, v = (q[0] for q in r32)
            acc["ema"] = max(acc["ema"], O.ratio(O.ema_step(e, p, 0.999, torch.float32)[0], *O.ema_step(e, p, 0.999)))
            e = O.ema_step(e, p, 0.999, torch.float32)[0]
    return acc


def test_tolerance_constants():
    got = measure()
    for fam, r in sorted(got.items()):
        c = O.c_of(fam)
        print(f"{fam:10s}: float32 restatement ratio {r:.3f}, c = {c:.2f}")
        assert r <= c / 4, (fam, r, c)
        assert r >= c / 16, (fam, r, c, "the constant is far above what float32 arithmetic needs: measure again")
    assert set(got) == set(O.MEASURED)


# ------------------------------------------------------------------------------------------------ host side
def test_new_wrappers_refuse_cpu_tensors():
    from sdeflow_light_amd import ops, _lib
    z = torch.zeros(8)
    with pytest.raises(_lib.MsgmError, match="no CPU fallback"):
        ops.grad_sqnorm(z)
    with pytest.raises(_lib.MsgmError, match="no CPU fallback"):
        ops.adam_step_ex(z, z, z.clone(), z.clone(), ops.opt_hyper("cpu"), torch.ones(1, dtype=torch.int64))
    with pytest.raises(_lib.MsgmError, match="no CPU fallback"):
        ops.swap_(z, z.clone())
    h = ops.opt_hyper("cpu", lr=3e-4, betas=(0.8, 0.9), eps=1e-6, max_grad_norm=2.0, ema_rate=0.5)
    assert h.dtype == torch.float64 and h.tolist() == [3e-4, 0.8, 0.9, 1e-6, 2.0, 0.5]
    assert math.isinf(float(ops.opt_hyper("cpu")[ops.OPT_MAX_GRAD_NORM]))


def test_warmup_cosine_endpoints():
    from sdeflow_light_amd.train import warmup_cosine
    f = warmup_cosine(1e-3, warmup=10, total=100, min_lr=1e-5)
    assert f(1) == pytest.approx(1e-4) and f(10) == pytest.approx(1e-3) and f(5) == pytest.approx(5e-4)
    assert f(100) == pytest.approx(1e-5) and f(1000) == pytest.approx(1e-5)
    assert f(55) == pytest.approx(1e-5 + 0.5 * (1e-3 - 1e-5))
    assert all(f(k) >= f(k + 1) for k in range(10, 100)) and all(f(k) < f(k + 1) for k in range(1, 10))
    g = warmup_cosine(2e-3, warmup=0, total=4)
    assert g(1) == pytest.approx(2e-3 * 0.5 * (1 + math.cos(math.pi * 0.25))) and g(4) == pytest.approx(0.0, abs=1e-18)


def test_grad_sqnorm_slice_layout():
    import __graft_entry__ as g
    g.build()
    from sdeflow_light_amd import _lib
    q = _lib.lib().msgm_grad_sqnorm_partials
    assert q(1) == q(7) == q(O.SLICE) == 1 and q(O.SLICE + 1) == 2 and q(2 * O.SLICE) == 2 and q(2 * O.SLICE + 1) == 3
    assert q(O.SLICE * O.MAX_SLICES) == O.MAX_SLICES
    for n in (O.SLICE * O.MAX_SLICES + 1, 4 * O.SLICE * O.MAX_SLICES + 5, 2 ** 31 + 5, 2 ** 34):
        assert 1 <= q(n) <= O.MAX_SLICES and q(n) == O.n_partials(n), n
        assert O.slice_len(n) % 1024 == 0 and O.slice_len(n) * q(n) >= n > O.slice_len(n) * (q(n) - 1)
    for n in O.KERNEL_N + (33794, 819265, 4023233):
        assert q(n) == O.n_partials(n), n
    assert q(0) == 0
