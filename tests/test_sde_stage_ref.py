"""CPU checks of tests/sde_stage_ref.py: (1) the float64 restatement equals the oracle (oracle/sde_ref.py,
oracle/ssm_ref.py) evaluated in float64 on small inputs; (2) the tolerance constants of the GPU parity tests are what the
restatement evaluated in float32 measures against float64 on the GPU tests' case shapes — the float32 arithmetic stays
within c / 4, so the constants cannot drift."""
import math

import pytest
import torch

import sde_stage_ref as R
from oracle import sde_ref as S
from oracle import ssm_ref as LR

F64 = torch.float64


def _spec(kind, n=0, G=None):
    k = {"sgm": S.SGM, "sparse": S.MSGM_SPARSE, "dense": S.MSGM_DENSE}[kind]
    sp = S.SdeSpec(kind=k, beta_min=R.c32(R.B0), beta_max=R.c32(R.B1), T=1.0, n=n, G=None if G is None else G.double())
    return sp


@pytest.mark.parametrize("kind,n", [("sgm", 5), ("sparse", 1), ("sparse", 2), ("sparse", 6), ("dense", 2), ("dense", 7)])
@pytest.mark.parametrize("proc,strato,lmbd", R.COMBOS)
def test_stage_equals_oracle_float64(kind, n, proc, strato, lmbd):
    B = 5
    d = R.stage_inputs(B, n, 11 * n + B)
    G, L_G = R.dense_G(n) if kind == "dense" else (None, None)
    sp = _spec(kind, n, G)
    if kind == "dense":
        assert torch.allclose(sp.L_G, L_G.double(), atol=1e-6)
        sp.L_G = L_G.double()
    x, a, z, base = (d[k].double() for k in ("x", "a", "z", "base"))
    t, delta = R.c32(R.T0), R.DELTA
    pr = S.ReverseProcess(sp, lambda y, s: a, lmbd) if proc == "reverse" else S.ForwardProcess(sp)
    tt = torch.full((B, 1), t, dtype=F64)
    mu = pr.drift_strato(tt, x) if strato else pr.drift(tt, x)
    dW = delta ** 0.5 * z
    inc = S.em_increment(sp, mu, delta, pr.sigma(tt, x), dW)
    for nc in (False, True):
        r = R.stage(kind, proc, strato, d["x"], d["a"], t=t, delta=delta, lmbd=lmbd, dW=dW, base=d["base"], c_out=0.5,
                    norm0=d["norm0"] if nc else None, G=G, L_G=L_G)
        ref = base + 0.5 * inc
        if nc:
            ref = S._renorm(ref, d["norm0"].double())
        (o, mo), (i, mi) = r["out"], r["inc"]
        assert float(((o - ref).abs() / mo).max()) <= 1e-12
        assert float(((i - inc).abs() / mi).max()) <= 1e-12
        assert bool((mo >= o.abs() * (1 - 1e-12)).all()) and bool((mi >= i.abs() * (1 - 1e-12)).all())
    # z with the float32 sqrt(delta) is the same draw as dW
    r2 = R.stage(kind, proc, strato, d["x"], d["a"], t=t, delta=delta, lmbd=lmbd, z=d["z"], G=G, L_G=L_G)
    assert torch.allclose(r2["inc"][0], inc, rtol=0, atol=1e-12)


def test_stage_delta_rows_equals_per_row_scalar_calls():
    B, n = 4, 8
    d = R.stage_inputs(B, n, 3)
    for kind in ("sgm", "sparse"):
        for tf in (0.0, 0.5, 1.0):
            r = R.stage(kind, "forward", True, d["x"], t=R.T0, delta=0.0, z=d["z"], delta_rows=d["delta_rows"], t_frac=tf)
            for b in range(B):
                db = float(d["delta_rows"][b])
                sp = _spec(kind, n)
                tt = torch.full((1, 1), R.c32(R.T0) + R.c32(tf) * db, dtype=F64)
                xb = d["x"][b:b + 1].double()
                pr = S.ForwardProcess(sp)
                inc = S.em_increment(sp, pr.drift_strato(tt, xb), db, pr.sigma(tt, xb), db ** 0.5 * d["z"][b:b + 1].double())
                assert torch.allclose(r["inc"][0][b:b + 1], inc, rtol=1e-12, atol=1e-14)


def test_rk4_rownorm_perturb_lincomb_equal_oracle():
    torch.manual_seed(2)
    B, n = 6, 9
    x, k1, k2, k3, k4 = (torch.randn(B, n) for _ in range(5))
    n0 = x.norm(dim=1)
    ref = x.double() + (k1.double() + 2 * k2.double() + 2 * k3.double() + k4.double()) / 6
    assert torch.allclose(R.rk4_combine(x, k1, k2, k3, k4)[0], ref, rtol=1e-14)
    assert torch.allclose(R.rk4_combine(x, k1, k2, k3, k4, n0)[0], S._renorm(ref, n0.double()), rtol=1e-13)
    assert torch.allclose(R.row_norm(x)[0], torch.norm(x.double(), dim=1), rtol=1e-14)
    sp = _spec("sgm")
    t = torch.tensor([1e-4, 5e-4, 1e-3, 0.2, 0.7, 1.0])
    eps = torch.randn(B, n)
    y, my = R.perturb_vp(x, t, eps)
    assert torch.allclose(y, S.vp_perturb(sp, t.double().reshape(B, 1), x.double(), eps.double()), rtol=1e-13)
    assert bool((my >= y.abs()).all())
    u = torch.tensor([0.0, 5e-4, 1e-3, 0.0010001, 0.5, 1.0])
    assert torch.equal(R.clamp_time(u), S.clamp_time(S.SdeSpec(), u))
    v, m = R.lincomb(x, 0.5, k1, -2.0, k2, 0.25)
    assert torch.allclose(v, 0.5 * x.double() - 2 * k1.double() + 0.25 * k2.double(), rtol=1e-14)
    assert torch.allclose(m, 0.5 * x.double().abs() + 2 * k1.double().abs() + 0.25 * k2.double().abs(), rtol=1e-14)


@pytest.mark.parametrize("kind,n", [("sgm", 5), ("sparse", 1), ("sparse", 2), ("sparse", 6), ("dense", 2), ("dense", 7)])
def test_ssm_terms_and_loss_equal_oracle_float64(kind, n):
    """A linear score a(y) = y M + c has the tangent adot = v M: per = adot.u + cst + |a|^2 / 2 against the oracle's
    forward-mode SSM loss.  (Dense: the oracle carries v^T G(v) a, analytically zero, as float64 rounding noise.)"""
    torch.manual_seed(n)
    B = 4
    G, L_G = R.dense_G(n) if kind == "dense" else (None, None)
    sp = _spec(kind, n, G)
    y, v = torch.randn(B, n), (torch.rand(B, n) >= 0.5).float() * 2 - 1
    t = torch.tensor([1e-3, 0.2, 0.63, 1.0])
    M, c = torch.randn(n, n, dtype=F64), torch.randn(n, dtype=F64)
    score = lambda prm, yy, tt: yy @ M + c
    per_ref = LR.ssm_loss_jvp(sp, score, {}, t.double().reshape(B, 1), y.double(), v.double())
    a, ad = y.double() @ M + c, v.double() @ M
    (u, mu), (cst, mc) = R.ssm_terms(kind, y, v, t, G)
    (per, mper), (ga, _), (gad, _) = R.ssm_loss(torch.cat([a, ad]), u, cst, 0.25)
    assert float(((per - per_ref).abs() / mper).max()) <= 1e-12
    assert torch.equal(ga, a * 0.25) and torch.equal(gad, u * 0.25)
    if kind == "sgm":
        (per2, mp2), (g1, _), (g2, _) = R.ssm_loss_diag(torch.cat([a, ad]), v, t, 0.25)
        assert float(((per2 - per_ref).abs() / mp2).max()) <= 1e-12
        assert torch.equal(g1, ga) and torch.allclose(g2, gad, rtol=1e-14)


def test_adam_equals_oracle_float64():
    """The kernel's float32 constants (1 - b1, b2, 1 - b2, eps, step size, sqrt(bc2)) differ from the oracle's doubles by
    6e-8 relative each, so the two agree to 1e-6 of the magnitude per step taken, not to float64 rounding."""
    torch.manual_seed(4)
    n = 50
    p, m, v = torch.randn(n, dtype=F64) * 0.1, torch.zeros(n, dtype=F64), torch.zeros(n, dtype=F64)
    po, mo, vo = p.clone(), m.clone(), v.clone()
    for step in range(1, 6):
        g = torch.randn(n, dtype=F64) * 0.01
        (p, mp), (m, mm), (v, mv) = R.adam_step(p, g, m, v, step, gscale=0.5)
        po, mo, vo = LR.adam_step(po, 0.5 * g, mo, vo, step)
        for q, qo, mag in ((p, po, mp), (m, mo, mm), (v, vo, mv)):
            assert float(((q - qo).abs() / mag).max()) <= 1e-6 * step


# ------------------------------------------------------------------------------------------------ tolerance constants
MAX_ELEMS = 2_200_000         # case shapes up to this many elements fit in about a second of CPU time each


def _upd(acc, family, n, val, ref, mag):
    key = (family, n)
    acc[key] = max(acc.get(key, 0.0), R.ratio(val, ref, mag))


def measure():
    """{(family, n): worst |ref32 - ref64| / (2^-24 magnitude)} over the GPU tests' case shapes."""
    acc = {}
    flat = [(3, 4), (5, 3), (2049, 1024), (699051, 3)] + [(B, n) for n in (8, 12, 256) for B in (1, 33)] + [(33, 6)]
    shapes = {"sgm": flat[:4] + R.row_shapes(), "sparse": flat[2:3] + flat[4:] + [(3, 1024)] + R.row_shapes(),
              "dense": [(B, n) for n in R.DENSE_N for B in (1, 9)]}
    for kind, shp in shapes.items():
        for (B, n) in shp:
            if B * n > MAX_ELEMS:
                continue
            d = R.stage_inputs(B, n, 7 * n + B)
            G, L_G = R.dense_G(n) if kind == "dense" else (None, None)
            combos = R.COMBOS if B * n <= 300_000 else R.COMBOS[1::4]      # the large shapes: one forward, one reverse
            for proc, strato, lmbd in combos:
                for dr in (False, True):
                    kw = dict(t=R.T0, delta=R.DELTA, lmbd=lmbd, z=d["z"], base=d["x"], G=G, L_G=L_G,
                              delta_rows=d["delta_rows"] if dr else None, t_frac=0.5)
                    for nc in (False, True):
                        kw["norm0"] = d["norm0"] if nc else None
                        r64 = R.stage(kind, proc, strato, d["x"], d["a"], **kw)
                        r32 = R.stage(kind, proc, strato, d["x"], d["a"], dtype=torch.float32, **kw)
                        fam = ("dense" if kind == "dense" else "stage") + ("_nc" if nc else "")
                        _upd(acc, fam, n, r32["out"][0], *r64["out"])
                        if not nc:
                            _upd(acc, fam, n, r32["inc"][0], *r64["inc"])
                            _upd(acc, "stage", n, r32["dW"][0], *r64["dW"])
    for (B, n) in R.row_shapes():
        if B * n > MAX_ELEMS:
            continue
        g = torch.Generator().manual_seed(5 * n + B)
        x, k1, k2, k3, k4, a, ad = (R.randn(B, n, generator=g) for _ in range(7))
        v = (torch.rand(B, n, generator=g) >= 0.5).float() * 2 - 1
        t = R.clamp_time(torch.rand(B, generator=g))
        n0 = x.double().norm(dim=1).float()
        _upd(acc, "stage", n, R.rk4_combine(x, k1, k2, k3, k4, dtype=torch.float32)[0], *R.rk4_combine(x, k1, k2, k3, k4))
        _upd(acc, "stage_nc", n, R.rk4_combine(x, k1, k2, k3, k4, n0, torch.float32)[0], *R.rk4_combine(x, k1, k2, k3, k4, n0))
        _upd(acc, "rows", n, R.row_norm(x, torch.float32)[0], *R.row_norm(x))
        out = torch.cat([a, ad])
        for kind in ("sgm", "sparse"):
            (u32, _), (c32_, _) = R.ssm_terms(kind, x, v, t, dtype=torch.float32)
            (u, mu), (cst, mc) = R.ssm_terms(kind, x, v, t)
            _upd(acc, "stage", n, u32, u, mu)
            _upd(acc, "rows", n, c32_, cst, mc)
            for got, (ref, mag) in zip(R.ssm_loss(out, u32, c32_, 1.0 / B, torch.float32), R.ssm_loss(out, u32, c32_, 1.0 / B)):
                _upd(acc, "rows" if got[0].dim() == 1 else "stage", n, got[0], ref, mag)
        for got, (ref, mag) in zip(R.ssm_loss_diag(out, v, t, 1.0 / B, torch.float32), R.ssm_loss_diag(out, v, t, 1.0 / B)):
            _upd(acc, "rows" if got[0].dim() == 1 else "stage", n, got[0], ref, mag)
    for n in (2, 7, 64):
        g = torch.Generator().manual_seed(n)
        G, _ = R.dense_G(n)
        y, v = R.randn(9, n, generator=g), R.randn(9, n, generator=g)
        t = R.clamp_time(torch.rand(9, generator=g))
        _upd(acc, "dense", n, R.ssm_terms("dense", y, v, t, G, torch.float32)[0][0], *R.ssm_terms("dense", y, v, t, G)[0])
    for d in (1, 2, 3, 5, 1024):
        B = 37
        g = torch.Generator().manual_seed(d)
        x0, eps = R.randn(B, d, generator=g), R.randn(B, d, generator=g)
        t = torch.rand(B, generator=g)
        t[:6] = torch.tensor([1e-4, 2.5e-4, 5e-4, 9e-4, 1e-3, 1.0])
        _upd(acc, "perturb", 0, R.perturb_vp(x0, t, eps, torch.float32)[0], *R.perturb_vp(x0, t, eps))
    for n in (1, 1023, 524289):
        g = torch.Generator().manual_seed(n)
        a, b, c = (R.randn(n, generator=g) for _ in range(3))
        _upd(acc, "lincomb", 0, R.lincomb(a, 0.5, b, -2.0, c, 1.0 / 3, torch.float32)[0], *R.lincomb(a, 0.5, b, -2.0, c, 1.0 / 3))
    for n in (4, 7, 4096, 2097156):
        g = torch.Generator().manual_seed(n)
        p, m, v = R.randn(n, generator=g) * 0.1, torch.zeros(n), torch.zeros(n)
        for step in range(1, 6):
            gr = R.randn(n, generator=g) * 0.01
            r32 = R.adam_step(p, gr, m, v, step, gscale=0.5, dtype=torch.float32)
            r64 = R.adam_step(p, gr, m, v, step, gscale=0.5)
            for (got, _), (ref, mag) in zip(r32, r64):
                _upd(acc, "adam", 0, got, ref, mag)
            p, m, v = (q[0] for q in r32)
    return acc


def bucketed(acc):
    out = {}
    for (fam, n), r in acc.items():
        m = R.MEASURED[fam]
        key = (fam, min(k for k in m if n <= k)) if isinstance(m, dict) else (fam, None)
        out[key] = max(out.get(key, 0.0), r)
    return out


def test_tolerance_constants():
    got = bucketed(measure())
    for (fam, nmax), r in sorted(got.items(), key=str):
        c = R.c_of(fam, nmax)
        print(f"{fam:10s} n<={nmax}: float32 restatement ratio {r:.3f}, c = {c:.2f}")
        assert r <= c / 4, (fam, nmax, r, c)
        assert r >= c / 16, (fam, nmax, r, c, "the constant is far above what float32 arithmetic needs: measure again")
    for fam, m in R.MEASURED.items():                  # every constant is backed by a measurement
        for nmax in (m if isinstance(m, dict) else (None,)):
            assert (fam, nmax) in got, (fam, nmax)


if __name__ == "__main__":
    import time
    t0 = time.time()
    for k, r in sorted(bucketed(measure()).items(), key=str):
        print(k, round(r, 3))
    print("seconds", round(time.time() - t0, 1))
