"""msgm_sde_stage_dense_mm (k_stage_dense_mm: the dense stage with its contraction on the matrix cores) on the GPU: the stage
against float64 with the unchanged msgm_sde_stage and the float32 restatement as the yardstick, bounds, the noise identity,
determinism, refusals, the routing in _Clock.stage, the public samplers against the float64 oracle, the Philox stream and
the graph-captured step.  An fp32 MFMA sums in another order than k_stage_rows' dense branch, so nothing here compares the
two entries' out to the bit; only dW_out, which both form as sqd * z, is compared that way.

MSGM_PARITY_OUT=<file>: the measured ratios are appended there as well as printed (profiles/stage_dense_mm/parity_measured.txt
is such a run)."""
import itertools
import os

import pytest
import torch

import sde_stage_ref as R
from conftest import rel_l2
from test_mlp_sde_loop_gpu import DEV, NLR, make_gen, oracle_traj

pytestmark = pytest.mark.gpu


def record(line):
    print(line)
    path = os.environ.get("MSGM_PARITY_OUT")
    if path:
        with open(path, "a") as fh:
            fh.write(line + "\n")


def sde(L, G, L_G, kind=None):
    return L.sde_struct(L.SDE_MSGM_DENSE if kind is None else kind, R.B0, R.B1, R.T_END, R.T_EPS, G, L_G)


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def row_err(y, ref):
    """Worst per-row relative L2 error."""
    y, ref = y.double(), ref.double()
    return float(((y - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)).max())


class Tensor:
    """G, L_G and the packed image of one width, built once per module."""
    cache = {}

    def __new__(cls, n):
        if n not in cls.cache:
            from sdeflow_light_amd import ops
            self = super().__new__(cls)
            self.G, self.L_G = R.dense_G(n, device=DEV)
            self.packed = ops.pack_dense_g_stage(self.G, self.L_G)
            cls.cache[n] = self
        return cls.cache[n]


def call(entry, L, tz, d, proc, strato, lmbd, *, base, norm0, noise, dW=None, rng=None, rng_step=0, dr=False, t_frac=0.0,
         t=R.T0, t_dev=None, step_dev=None, **extra):
    """One launch of `entry` (ops.sde_stage or ops.sde_stage_dense_mm) on NaN-filled outputs -> (out, inc_out, dW_out)."""
    x = d["x"]
    B, n = x.shape
    out, inc, dwo = nan(B, n), nan(B, n), nan(B, n)
    bs = {"x": x, "none": None, "other": d["base"]}[base]
    kw = {"z": d["z"]} if noise == "z" else {"dW": dW} if noise == "dW" else {"rng": rng, "rng_step": rng_step, "step_dev": step_dev}
    entry(out, bs, 0.5, x, d["a"] if proc == "reverse" else None, sde(L, tz.G, tz.L_G),
          L.PROC_REVERSE if proc == "reverse" else L.PROC_FORWARD, strato, t, R.DELTA, lmbd, dW_out=dwo, inc_out=inc,
          norm0=d["norm0"] if norm0 else None, delta_rows=d["delta_rows"] if dr else None, t_frac=t_frac, t_dev=t_dev,
          **kw, **extra)
    return out, inc, dwo


def reference(tz, d, proc, strato, lmbd, dtype, *, base, norm0, W, dr=False, t_frac=0.0, t=R.T0):
    bs = {"x": d["x"], "none": None, "other": d["base"]}[base]
    return R.stage("dense", proc, strato, d["x"], d["a"], t=t, delta=R.DELTA, lmbd=lmbd, dW=W, base=bs, c_out=0.5,
                   norm0=d["norm0"] if norm0 else None, delta_rows=d["delta_rows"] if dr else None, t_frac=t_frac,
                   G=tz.G, L_G=tz.L_G, dtype=dtype)


# ------------------------------------------------------------------ 1. the stage against float64
# (proc, strato, lmbd, norm0, base, noise): every value of every option on both processes, each pair of (base, noise) once
OPTIONS = [("reverse", False, 0.0, False, "none", "z"), ("reverse", True, 0.5, True, "x", "dW"),
           ("reverse", False, 0.5, False, "other", "philox"), ("reverse", True, 0.0, True, "other", "z"),
           ("reverse", True, 0.0, False, "x", "philox"), ("reverse", False, 0.5, True, "none", "dW"),
           ("reverse", True, 0.5, False, "none", "philox"), ("reverse", False, 0.0, True, "x", "z"),
           ("reverse", True, 0.5, True, "other", "dW"),
           ("forward", False, 0.0, False, "other", "z"), ("forward", True, 0.0, True, "x", "dW"),
           ("forward", True, 0.5, False, "none", "philox"), ("forward", False, 0.5, True, "other", "philox"),
           ("forward", True, 0.0, False, "none", "dW"), ("forward", False, 0.0, True, "x", "z")]
STAGE_N = (17, 31, 32, 33, 47, 48, 49, 63, 64)
STAGE_B = (1, 31, 33, 65)


def one_parity(ops, L, tz, d, opt, tag, rule="rows", **more):
    """The new entry's worst per-row error of out and inc_out against float64 over max(parent kernel, float32 restatement):
    returned, and with rule="rows" asserted to be at most 2.  rule="elements" asserts sde_stage_ref's per-element bound
    instead, |new - float64| <= c 2^-24 magnitude with the dense families' c (what tests/test_sde_paths_gpu.py holds
    msgm_sde_stage's dense branch to), and only prints the per-row figures."""
    from sdeflow_light_amd._lib import PhiloxState
    proc, strato, lmbd, norm0, base, noise = opt
    rng = PhiloxState(4242, DEV) if noise == "philox" else None
    kw = dict(base=base, norm0=norm0, noise=noise, rng=rng, rng_step=3, **more)
    if noise == "dW":
        kw["dW"] = R.c32(R.DELTA ** 0.5) * d["z"]
    old = call(ops.sde_stage, L, tz, d, proc, strato, lmbd, **kw)
    new = call(ops.sde_stage_dense_mm, L, tz, d, proc, strato, lmbd, packed=tz.packed, **kw)
    assert all(bool(torch.isfinite(v).all()) for v in new + old), tag
    assert torch.equal(new[2], old[2]), tag + ": dW_out"        # both form sqd * z (or pass dW on): the same bits
    W = old[2]
    rk = {k: v for k, v in more.items() if k in ("dr", "t_frac", "t")}
    r64 = reference(tz, d, proc, strato, lmbd, torch.float64, base=base, norm0=norm0, W=W, **rk)
    r32 = reference(tz, d, proc, strato, lmbd, torch.float32, base=base, norm0=norm0, W=W, **rk)
    worst = 0.0
    for k, nm in ((0, "out"), (1, "inc")):
        truth = r64[nm][0]
        e_new, e_old, e_32 = row_err(new[k], truth), row_err(old[k], truth), row_err(r32[nm][0], truth)
        ratio = e_new / max(e_old, e_32)
        worst = max(worst, ratio)
        print(f"{tag} {nm}: new {e_new:.3e} | parent {e_old:.3e} | float32 {e_32:.3e} | ratio {ratio:.2f}")
        if rule == "rows":
            assert e_new <= 2.0 * max(e_old, e_32), (tag, nm, e_new, e_old, e_32)
        else:
            n = d["x"].shape[1]
            fam = "dense_nc" if (norm0 and nm == "out") else "dense"
            r_new, r_old, c = R.ratio(new[k], *r64[nm]), R.ratio(old[k], *r64[nm]), R.c_of(fam, n)
            print(f"{tag} {nm}: per element, in units of 2^-24 magnitude: new {r_new:.3f} | parent {r_old:.3f} (c = {c:.2f})")
            assert r_new <= c, (tag, nm, fam, r_new, c)
    return worst


@pytest.mark.parametrize("n", STAGE_N)
def test_stage_vs_float64(n):
    """Truth = sde_stage_ref.stage in float64.  The worst per-row relative L2 error of out and inc_out may be at most 2 x the
    larger of the unchanged ops.sde_stage's and the float32 restatement's on the same inputs (the project's rule for
    kernels that sum in another order).  n: each side of every 16-wide i-block and K pad; B: a lone row, a tile short by
    one, a tile plus one live row, three tiles.  B = 33 also runs delta_rows + t_frac on both processes; t_dev / step_dev:
    test_stage_device_clock_and_step.  Measured on an MI355X: profiles/stage_dense_mm/parity_measured.txt."""
    from sdeflow_light_amd import _lib as L, ops
    tz = Tensor(n)
    for B in STAGE_B:
        d = R.stage_inputs(B, n, 977 * n + B, DEV)
        worst = 0.0
        for opt in OPTIONS:
            worst = max(worst, one_parity(ops, L, tz, d, opt, f"stage ({B},{n}) {opt}"))
        if B == 33:
            worst = max(worst, one_parity(ops, L, tz, d, ("reverse", True, 0.5, True, "other", "z"), f"stage ({B},{n}) delta_rows",
                                          dr=True, t_frac=0.5))
            worst = max(worst, one_parity(ops, L, tz, d, ("forward", True, 0.0, False, "x", "philox"), f"stage ({B},{n}) delta_rows fwd",
                                          dr=True, t_frac=1.0))
        record(f"stage B={B:3d} n={n:2d}: worst new / max(parent, float32) over out, inc_out = {worst:.2f}")


@pytest.mark.parametrize("n", [2, 7, 16])
def test_stage_narrow_widths_vs_float64(n):
    """The entry takes 1 <= n <= 64 though nothing routes n <= 30 to it: the NP = 16 instantiation (four k-slices, one
    i-block; at n = 2 two of the slices are empty), B = 33 (a tile plus one live row), every option set.
    The bound here is sde_stage_ref's per-element one — |new - float64| <= c 2^-24 magnitude, c = c_of("dense" |
    "dense_nc", n) = 4 x the float32 restatement's own measured ratio — the rule tests/test_sde_paths_gpu.py holds
    msgm_sde_stage's dense branch to at exactly these widths, not the per-row ratio of test_stage_vs_float64: a row of 2 or
    7 elements is no norm to speak of, its relative L2 error is the relative error of one or two elements, and where the
    drift terms of such a row cancel (reverse, Stratonovich: ga - f + 2f - f) that is unbounded for ANY float32
    evaluation, so the ratio of two kernels' worst rows is a ratio of two draws, not a property of either.  Measured on an
    MI355X with the per-row rule at n = 2 (reverse, Stratonovich, lmbd 0, base = x, Philox), inc_out: new 2.73e-06 | parent
    5.92e-07 | float32 restatement 5.92e-07, i.e. 4.6 x where that rule allows 2 x; the per-row figures are still printed and
    recorded."""
    from sdeflow_light_amd import _lib as L, ops
    tz = Tensor(n)
    d = R.stage_inputs(33, n, 977 * n + 33, DEV)
    worst = max(one_parity(ops, L, tz, d, opt, f"stage (33,{n}) {opt}", rule="elements") for opt in OPTIONS)
    record(f"stage B= 33 n={n:2d}: per-element bound held; worst per-row new / max(parent, float32) over out, inc_out = {worst:.2f} (not asserted)")


@pytest.mark.parametrize("n", [33, 64])
def test_stage_device_clock_and_step(n):
    """t_dev / step_dev override the host t and rng_step: the result is the bits of the call given them by value, and within
    the float64 bound."""
    from sdeflow_light_amd import _lib as L, ops
    from sdeflow_light_amd._lib import PhiloxState
    tz = Tensor(n)
    B = 33
    d = R.stage_inputs(B, n, 5 * n, DEV)
    t_dev = torch.tensor([R.T0], device=DEV)
    step_dev = torch.tensor([3], dtype=torch.int64, device=DEV)
    rng = PhiloxState(4242, DEV)
    kw = dict(base="x", norm0=True, noise="philox", rng=rng, packed=tz.packed)
    by_value = call(ops.sde_stage_dense_mm, L, tz, d, "reverse", True, 0.5, rng_step=3, **kw)
    by_dev = call(ops.sde_stage_dense_mm, L, tz, d, "reverse", True, 0.5, rng_step=999, t=-7.0, t_dev=t_dev, step_dev=step_dev, **kw)
    for a, b in zip(by_value, by_dev):
        assert torch.isfinite(a).all() and torch.equal(a, b)
    old = call(ops.sde_stage, L, tz, d, "reverse", True, 0.5, base="x", norm0=True, noise="philox", rng=rng, rng_step=999, t=-7.0,
               t_dev=t_dev, step_dev=step_dev)
    assert torch.equal(old[2], by_dev[2])
    r64 = reference(tz, d, "reverse", True, 0.5, torch.float64, base="x", norm0=True, W=old[2])
    r32 = reference(tz, d, "reverse", True, 0.5, torch.float32, base="x", norm0=True, W=old[2])
    for k, nm in ((0, "out"), (1, "inc")):
        e_new, e_old, e_32 = (row_err(v, r64[nm][0]) for v in (by_dev[k], old[k], r32[nm][0]))
        record(f"stage B={B} n={n} t_dev/step_dev {nm}: new {e_new:.3e} | parent {e_old:.3e} | float32 {e_32:.3e}")
        assert e_new <= 2.0 * max(e_old, e_32)


# ------------------------------------------------------------------ 2. nothing outside the rows
@pytest.mark.parametrize("n,B", [(33, 33), (49, 1)])
def test_nothing_outside_the_rows(n, B):
    """x, a, z (and norm0) are views into NaN-filled buffers with NaN guards in front and behind — the C ABI takes contiguous
    (B, n) operands, so the guards are whole rows plus a few elements, which also leaves the views only 4-byte aligned; out,
    inc_out and dW_out have sentinel rows behind row B.  Every output is finite, equals the call on exact-size aligned
    buffers to the bit, and the sentinels are untouched."""
    from sdeflow_light_amd import _lib as L, ops
    tz = Tensor(n)
    d = R.stage_inputs(B, n, 31 * n + B, DEV)
    front, back = 2 * n + 3, 40 * n

    def guarded(v, fill):
        buf = torch.full((front + v.numel() + back,), fill, device=DEV)
        view = buf[front:front + v.numel()].view(v.shape)
        view.copy_(v)
        return buf, view

    g = {k: guarded(d[k], float("nan")) for k in ("x", "a", "z", "norm0")}
    SENT = 12345.0
    outs = [guarded(torch.zeros(B, n, device=DEV), SENT) for _ in range(3)]
    st = sde(L, tz.G, tz.L_G)
    ops.sde_stage_dense_mm(outs[0][1], d["base"], 0.5, g["x"][1], g["a"][1], st, L.PROC_REVERSE, True, R.T0, R.DELTA, 0.5,
                           z=g["z"][1], dW_out=outs[2][1], inc_out=outs[1][1], norm0=g["norm0"][1], packed=tz.packed)
    torch.cuda.synchronize()
    exact = call(ops.sde_stage_dense_mm, L, tz, d, "reverse", True, 0.5, base="other", norm0=True, noise="z", packed=tz.packed)
    for (buf, view), ref in zip(outs, exact):
        assert torch.isfinite(view).all() and torch.equal(view, ref)
        assert (buf[:front] == SENT).all() and (buf[front + B * n:] == SENT).all()
    for buf, view in g.values():
        assert torch.isnan(buf[:front]).all() and torch.isnan(buf[front + view.numel():]).all()


# ------------------------------------------------------------------ 3. noise identity
@pytest.mark.parametrize("n,B", [(33, 33), (64, 65)])
def test_noise_identity(n, B):
    """With the same Philox state and rng_step, dW_out is ops.sde_stage's to the bit; the same with z."""
    from sdeflow_light_amd import _lib as L, ops
    from sdeflow_light_amd._lib import PhiloxState
    tz = Tensor(n)
    d = R.stage_inputs(B, n, 7 * n + B, DEV)
    for noise in ("philox", "z"):
        for dr in (False, True):
            kw = dict(base="x", norm0=False, noise=noise, rng=PhiloxState(99, DEV, offset=5), rng_step=11, dr=dr, t_frac=0.5)
            old = call(ops.sde_stage, L, tz, d, "reverse", True, 0.0, **kw)
            new = call(ops.sde_stage_dense_mm, L, tz, d, "reverse", True, 0.0, packed=tz.packed, **kw)
            assert torch.isfinite(new[2]).all() and new[2].abs().sum() > 0
            assert torch.equal(new[2], old[2]), (noise, dr)


# ------------------------------------------------------------------ 4. determinism
def test_two_calls_give_the_same_bits():
    from sdeflow_light_amd import _lib as L, ops
    n, B = 48, 65
    tz = Tensor(n)
    d = R.stage_inputs(B, n, 48065, DEV)
    kw = dict(base="other", norm0=True, noise="z", packed=tz.packed)
    a = call(ops.sde_stage_dense_mm, L, tz, d, "reverse", True, 0.5, **kw)
    b = call(ops.sde_stage_dense_mm, L, tz, d, "reverse", True, 0.5, **kw)
    for u, v in zip(a, b):
        assert torch.isfinite(u).all() and torch.equal(u, v)


# ------------------------------------------------------------------ 5. refusals
def test_refusals_come_before_any_launch():
    from sdeflow_light_amd import _lib as L, ops
    from sdeflow_light_amd._lib import MsgmError
    tz = Tensor(33)
    d = R.stage_inputs(9, 33, 1, DEV)
    out = nan(9, 33)
    st = sde(L, tz.G, tz.L_G)
    rev = (L.PROC_REVERSE, True, R.T0, R.DELTA)
    x65, p64 = torch.randn(9, 65, device=DEV), Tensor(64).packed
    o65 = nan(9, 65)
    with pytest.raises(MsgmError, match=r"\(-2\)"):             # MSGM_E_UNSUPPORTED: n = 65
        ops.sde_stage_dense_mm(o65, None, 1.0, x65, x65.clone(), st, *rev, z=x65.clone(), packed=p64)
    with pytest.raises(MsgmError, match=r"\(-2\)"):             # a sparse struct
        ops.sde_stage_dense_mm(out, None, 1.0, d["x"], d["a"], sde(L, None, None, L.SDE_MSGM_SPARSE), *rev, z=d["z"], packed=tz.packed)
    with pytest.raises(MsgmError, match=r"\(-1\)"):             # MSGM_E_BADARG: out is x
        ops.sde_stage_dense_mm(d["x"], None, 1.0, d["x"], d["a"], st, *rev, z=d["z"], packed=tz.packed)
    with pytest.raises(MsgmError, match=r"\(-1\)"):             # no noise source
        ops.sde_stage_dense_mm(out, None, 1.0, d["x"], d["a"], st, *rev, packed=tz.packed)
    with pytest.raises(MsgmError, match=r"\(-1\)"):             # the reverse process without a
        ops.sde_stage_dense_mm(out, None, 1.0, d["x"], None, st, *rev, z=d["z"], packed=tz.packed)
    with pytest.raises(MsgmError, match=r"\(-1\)"):             # no image
        ops.sde_stage_dense_mm(out, None, 1.0, d["x"], d["a"], st, *rev, z=d["z"])
    with pytest.raises(MsgmError, match="pack_dense_g_stage"):  # an image of the wrong size: refused in ops
        ops.sde_stage_dense_mm(out, None, 1.0, d["x"], d["a"], st, *rev, z=d["z"], packed=Tensor(32).packed)
    with pytest.raises(MsgmError, match="pack_dense_g_stage"):
        ops.sde_stage_dense_mm(out, None, 1.0, d["x"], d["a"], st, *rev, z=d["z"], packed=tz.packed.double())
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(o65).all()


# ------------------------------------------------------------------ 6. routing
def count_calls(monkeypatch):
    from sdeflow_light_amd import ops
    calls = {"new": 0, "old": 0}
    for tag, name in (("new", "sde_stage_dense_mm"), ("old", "sde_stage")):
        real = getattr(ops, name)

        def wrapped(*a, _t=tag, _r=real, **k):
            calls[_t] += 1
            return _r(*a, **k)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


@pytest.mark.parametrize("d", [31, 64])
def test_routing_takes_the_new_stage(monkeypatch, d):
    """Dense d = 31 and 64, B = 33 and 160, N = 3: 4N new-entry calls for RK4, 2N for Heun, N for Euler-Maruyama and none of
    the old entry — on the public samplers, with noise= and through the composed functions."""
    from sdeflow_light_amd import sde_scheme as SS
    torch.manual_seed(d)
    gen = make_gen("dense", d, None, out_scale=0.1)
    calls = count_calls(monkeypatch)
    N = 3
    for B in (33, 160):
        x0 = torch.randn(B, d, device=DEV)
        z = torch.randn(N, B, d)
        runs = [(SS.rk4_stratonovich_sampler, 4), (SS.heun_sampler, 2), (SS.euler_maruyama_sampler, 1),
                (SS.rk4_stratonovich_composed, 4), (SS.heun_composed, 2)]
        for fn, per_step in runs:
            for kw in ({}, {"noise": z}):
                calls.update(new=0, old=0)
                out = fn(gen, x0, num_steps=N, keep_all_samples=True, norm_correction=True, **kw)
                assert torch.isfinite(out).all()
                assert calls == {"new": per_step * N, "old": 0}, (fn.__name__, B, bool(kw), calls)


def test_routing_leaves_the_rest_alone(monkeypatch):
    """Dense d = 30 at B = 64, a sparse d = 32 and the forward process at dense n = 32 never reach the new entry."""
    from sdeflow_light_amd import sde_scheme as SS
    from sdeflow_light_amd.SDEs import forward_SDE
    torch.manual_seed(3)
    calls = count_calls(monkeypatch)
    N = 3
    for kind, d, B in (("dense", 30, 64), ("sparse", 32, 160)):
        gen = make_gen(kind, d, None, out_scale=0.1)
        x0 = torch.randn(B, d, device=DEV)
        for fn in (SS.rk4_stratonovich_composed, SS.heun_composed):
            assert torch.isfinite(fn(gen, x0, num_steps=N, keep_all_samples=True, norm_correction=True)).all()
        assert torch.isfinite(SS.euler_maruyama_sampler(gen, x0, num_steps=N, noise=torch.randn(N, B, d))).all()
        assert calls["new"] == 0 and calls["old"] == (4 + 2 + 1) * N, (kind, calls)
        calls.update(new=0, old=0)
    gen = make_gen("dense", 32, None, out_scale=0.1)
    fwd = forward_SDE(gen.base_sde, gen.base_sde.T)
    out = SS.rk4_stratonovich_sampler(fwd, torch.randn(33, 32, device=DEV), num_steps=N, keep_all_samples=True)
    assert torch.isfinite(out).all() and calls == {"new": 0, "old": 4 * N}, calls


# ------------------------------------------------------------------ 7. the samplers against float64
YARD = [(31, None), (31, NLR), (48, None), (48, NLR), (64, None), (64, NLR)]


@pytest.mark.parametrize("d,pre", YARD, ids=[f"d{d}-{'nlr' if p else 'none'}" for d, p in YARD])
def test_sampler_float64_yardstick(monkeypatch, d, pre):
    """The rule of test_mlp_dense_sde_loop_gpu.test_float64_yardstick: truth = the oracle integrators with
    nets_ref.mlp_forward in float64 (the untrained net with its output layer x 0.1); the routed sampler may be no further
    from it than 2 x the larger of the float32 oracle and the same call with ops.stage_dense_mm_preferred patched to False —
    the parent route.  B = 33 and 65; Heun and RK4 at N = 4, Euler-Maruyama at N = 6; lmbd 0 / 0.5; norm correction on / off;
    explicit z."""
    from sdeflow_light_amd import ops, sde_scheme as SS
    torch.manual_seed(100 * d + 7)
    gen = make_gen("dense", d, pre, out_scale=0.1)
    public = {"em": SS.euler_maruyama_sampler, "heun": SS.heun_sampler, "rk4": SS.rk4_stratonovich_sampler}
    preferred = ops.stage_dense_mm_preferred
    worst = 0.0
    for B, (method, N), lmbd, nc in itertools.product((33, 65), (("heun", 4), ("rk4", 4), ("em", 6)), (0.0, 0.5), (False, True)):
        x0, z = torch.randn(B, d), torch.randn(N, B, d)
        truth = oracle_traj(gen, "dense", pre, method, x0, z, lmbd, nc, torch.float64)
        assert torch.isfinite(truth).all()
        e32 = rel_l2(oracle_traj(gen, "dense", pre, method, x0, z, lmbd, nc, torch.float32), truth)
        kw = dict(num_steps=N, lmbd=lmbd, keep_all_samples=True, include_t0=True, norm_correction=nc, noise=z)
        routed = public[method](gen, x0.to(DEV), **kw)
        with monkeypatch.context() as m:
            m.setattr(ops, "stage_dense_mm_preferred", lambda *a: False)
            parent = public[method](gen, x0.to(DEV), **kw)
        assert ops.stage_dense_mm_preferred is preferred and torch.isfinite(routed).all()
        assert not torch.equal(routed, parent)                  # two kernels: the patch reached the route
        er, ep = rel_l2(routed, truth), rel_l2(parent, truth)
        print(f"yardstick d={d} pre={pre} B={B} {method} N={N} lmbd={lmbd} nc={int(nc)}: routed {er:.3e} | parent {ep:.3e} | "
              f"float32 oracle {e32:.3e}  (vs float64)")
        worst = max(worst, er / max(ep, e32))
        assert er <= 2.0 * max(ep, e32), (B, method, lmbd, nc, er, ep, e32)
    record(f"sampler d={d} pre={pre}: worst routed / max(parent route, float32 oracle) = {worst:.2f}")


# ------------------------------------------------------------------ 8. Philox and graph
def test_philox_stream_of_the_public_sampler():
    """The public RK4 sampler from a Philox state equals its own noise=z call bit for bit, z being the device fill of
    RNG_STREAM_DW at offset + i; the stream advances by N."""
    from sdeflow_light_amd import _lib as L, ops, sde_scheme as SS
    torch.manual_seed(8)
    d, B, N = 33, 65, 4
    gen = make_gen("dense", d, NLR, out_scale=0.1)
    x0 = torch.randn(B, d, device=DEV)
    rng = gen.base_sde.philox(DEV)
    st = rng.state.clone()
    seed, offset = int(st[0]), int(st[1])
    kw = dict(num_steps=N, keep_all_samples=True, include_t0=True, norm_correction=True)
    a = SS.rk4_stratonovich_sampler(gen, x0, **kw)
    assert int(rng.state[1] - st[1]) == N
    z = torch.stack([ops.fill_normal(nan(B, d), L.PhiloxState(seed, DEV, offset + i), L.RNG_STREAM_DW) for i in range(N)])
    assert torch.isfinite(z).all()
    b = SS.rk4_stratonovich_sampler(gen, x0, noise=z, **kw)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    assert int(rng.state[1] - st[1]) == N                       # noise= draws nothing
    c = SS.rk4_stratonovich_sampler(gen, x0, **kw)              # fresh numbers from the advanced stream
    assert not torch.equal(a, c)


def test_graphed_step_equals_eager_steps(monkeypatch):
    """GraphedStepSampler (MLP, dense d = 33, B = 65, RK4, norm correction): two replays equal the two eager steps bit for
    bit, the captured step holds kernel nodes only, and its four stages are the new entry's."""
    from sdeflow_light_amd import ops, sde_scheme as SS
    d, B, N = 33, 65, 2
    calls = count_calls(monkeypatch)

    def make():
        torch.manual_seed(21)
        gen = make_gen("dense", d, NLR, out_scale=0.1)
        return gen, SS.GraphedStepSampler(gen, B, d, N, lmbd=0.5, norm_correction=True, method="rk4")

    x0 = torch.randn(B, d, generator=torch.Generator().manual_seed(2)).to(DEV)
    gA, sA = make()
    assert calls == {"new": 8, "old": 0}, calls                 # the eager pass and the capture, four stages each
    kinds = ops.graph_node_kinds(sA.graph)
    print(f"captured dense RK4 step = {kinds}")
    assert set(kinds) == {"kernel"}, kinds
    outA = sA.run(x0).clone()
    gB, sB = make()
    ops.lincomb(sB.x, x0, 1.0)
    ops.lincomb(sB.norm0, ops.row_norm(sB.x), 1.0)
    sB.step.zero_()
    for _ in range(N):
        sB._body()
    assert torch.isfinite(outA).all() and not torch.equal(outA, x0)
    assert torch.equal(outA, sB.x)
