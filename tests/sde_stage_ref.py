"""Plain-torch restatement of every operation of csrc/sde_kernels.hip, for float64 parity tests.

Each function evaluates the formula of the kernel's comment (oracle/sde_ref.py) in ``dtype`` (float64 = the
truth, float32 = the reference arithmetic the tolerance constants are measured on) on whatever device its inputs live
on, and returns ``(value, magnitude)`` pairs.  The MAGNITUDE is the same expression with every product and summand
replaced by its absolute value: the scale on which one float32 rounding of the expression lives, also where the value
itself cancels (the sparse stencil at n = 1, ``1 - exp(-x)`` at small times).  Where a cancelling quantity is fed
through a function, the magnitude carries the function's derivative:

* beta = b0 + (b1 - b0) s with s = T - t loses |db| (T + |t|) / beta relative digits: every term that holds beta or
  sqrt(beta) is scaled by kb = (b0 + |db| (T + |t|)) / beta >= 1;
* sqrt(var) with var = 1 - E: magnitude (1 + E) / (2 sqrt(var)) + sqrt(var);
* the norm correction o * norm0 / sqrt(sum o^2): magnitude scale * (m_o + |o| sum(|o| m_o) / sum o^2).

Scalars are rounded to float32 first (the C ABI takes floats), so the float64 result has the kernel's inputs, not
nearby ones.  Comparison: |kernel - ref64| <= c * 2^-24 * magnitude per element, c per family below.
"""
import math

import numpy as np
import torch

EPS32 = 2.0 ** -24
B0, B1, T_END, T_EPS = 0.1, 20.0, 1.0, 1e-3
CV32 = float(np.float32(0.5) * np.sqrt(np.float32(2.0)))          # the kernels' 0.5f * sqrtf(2.0f)


def c32(v):
    """The float32 the C ABI receives for a Python scalar."""
    return float(np.float32(v))


# ------------------------------------------------------------------------------------------------ tolerance constants
# Worst |ref32 - ref64| / (2^-24 magnitude) of the restatement evaluated in float32 (torch CPU), over the case shapes of
# tests/test_sde_paths_gpu.py up to 2.2M elements (tests/test_sde_stage_ref.py::test_tolerance_constants measures them
# again and asserts they stay within c / 4).  c = 4 x the measured ratio: the lane groups sum in another order and the
# device expf / sqrtf / division may be a few ulp off correct rounding.  Reductions and the dense contraction grow with
# the number of summands n (float32 sums of n terms, added in the kernels' documented order, see _rsum): measured per
# bucket of n.
MEASURED = {
    # family: worst ratio of the float32 restatement against float64 (torch CPU), rounded up to the next 0.1
    "stage": 5.3,                               # measured 5.252  elementwise outputs: out, inc, dW, u, g, rk4 without norm
    "stage_nc": {64: 2.7, 2050: 2.7},           # measured 2.661 / 2.659  (n <= key) out after the norm correction
    "dense": {16: 2.2, 64: 0.6},                # measured 2.183 / 0.535  dense contraction: the magnitude (a sum of n^2
    "dense_nc": {16: 1.1, 64: 0.4},             # measured 1.063 / 0.399   absolute values) outgrows the rounding error
    "rows": {64: 3.4, 2050: 6.3},               # measured 3.388 / 6.231  per-row sums: row_norm, cst, per
    "adam": 4.9,                                # measured 4.822
    "perturb": 5.3,                             # measured 5.236
    "lincomb": 2.0,                             # measured 1.920
}


def c_of(family, n=None):
    """Tolerance factor c of an output family (4 x the measured float32 ratio); n selects the bucket of a reduction."""
    m = MEASURED[family]
    if isinstance(m, dict):
        for nmax in sorted(m):
            if n <= nmax:
                return 4.0 * m[nmax]
        raise KeyError(f"{family}: no measured bucket for n = {n}")
    return 4.0 * m


def ratio(y, ref, mag):
    """Worst |y - ref| / (2^-24 mag) over the elements (0/0 counts as 0: an exact zero must be met exactly)."""
    d = (y.double() - ref.double()).abs()
    m = mag.double() * EPS32
    r = torch.where(d == 0, torch.zeros_like(d), d / m)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ helpers
def _beta(t, rev, dt):
    """beta(s), its amplification kb, for row times t (tensor in dt); s = T - t on the reverse process."""
    b0, b1, T = c32(B0), c32(B1), c32(T_END)
    db = c32(b1 - b0) if dt == torch.float32 else b1 - b0
    s, ms = (T - t, T + t.abs()) if rev else (t, t.abs())
    beta = b0 + db * s
    return beta, (b0 + abs(db) * ms) / beta


def _rsum(x, lanes=None):
    """Sum over the last axis.  float64: torch's sum.  float32: elementwise adds only, in the order the kernels
    document — element i goes to lane i % GS (GS = launch_rows' group width for n), a lane adds its elements in turn,
    the lanes meet in a halving tree (GS = 256: per 64-lane wave, then (w0 + w1) + (w2 + w3)); lanes=1 is the plain
    loop of the dense contraction.  So the float32 figures behind the tolerance constants are the same bits on every
    CPU (torch's own float32 sum and einsum follow the SIMD width and the BLAS at hand)."""
    if x.dtype == torch.float64:
        return x.sum(-1)
    n = x.shape[-1]
    gs = lanes or group_width(n)
    if n % gs:
        x = torch.nn.functional.pad(x, (0, gs - n % gs))
    x = x.reshape(*x.shape[:-1], -1, gs)
    acc = x[..., 0, :]
    for r in range(1, x.shape[-2]):
        acc = acc + x[..., r, :]
    w = min(gs, 64)
    acc = acc.reshape(*acc.shape[:-1], gs // w, w)
    while acc.shape[-1] > 1:
        h = acc.shape[-1] // 2
        acc = acc[..., :h] + acc[..., h:]
    acc = acc[..., 0]
    return (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3]) if gs == 256 else acc[..., 0]


def _dense3(G, y, w):
    """sum_jk G_ijk y_bj w_bk -> (b, i)"""
    return _rsum(_rsum(G[None] * w[:, None, None, :], 1) * y[:, None, :], 1)


def _dense2(M, y):
    """sum_j M_ij y_bj -> (b, i)"""
    return _rsum(M[None] * y[:, None, :], 1)


def _renorm(o, mo, norm0):
    ss = _rsum(o * o)[:, None]
    scale = norm0.reshape(-1, 1) / ss.sqrt()
    return o * scale, scale.abs() * (mo + o.abs() * _rsum(o.abs() * mo)[:, None] / ss)


def dense_G(n, seed=0, device="cpu"):
    """A skew tensor G (n,n,n) scaled so that trace(L_G) = -n/2 and L_G = 1/2 sum_jk G_ijk G_jmk, both float32
    (oracle/sde_ref.py:make_dense_G, SdeSpec.__post_init__)."""
    g = torch.Generator().manual_seed(1000 + n + seed)
    F = torch.randn(n, n, n, generator=g, dtype=torch.float64)
    G = 0.5 * (F - F.transpose(1, 2))                   # G0[k] = (F_k - F_k^T) / 2
    G = G.permute(1, 2, 0).contiguous()                 # G[:, :, k]
    L = 0.5 * torch.einsum("ijk,jmk->im", G, G)
    G = (torch.sqrt(-0.5 * n / torch.trace(L)) * G).float()
    L = (0.5 * torch.einsum("ijk,jmk->im", G.double(), G.double())).float()
    return G.to(device), L.to(device)


# ------------------------------------------------------------------------------------------------ integrator stage
def stage(kind, proc, strato, x, a=None, *, t, delta, lmbd=0.0, dW=None, z=None, sqrt_delta=None, base=None, c_out=1.0,
          norm0=None, delta_rows=None, t_frac=0.0, G=None, L_G=None, dtype=torch.float64):
    """out = base + c_out * (mu * delta + sigma . dW)  (k_stage_diag_flat / k_stage_sparse_flat / k_stage_rows).
    kind 'sgm' | 'sparse' | 'dense'; proc 'reverse' | 'forward'.  Returns {'out','inc','dW'}: (value, magnitude)."""
    dt, rev = dtype, proc == "reverse"
    X = x.to(dt)
    Bn = X.shape[0]
    l = c32(lmbd)
    if delta_rows is not None:
        d = delta_rows.to(dt).reshape(Bn, 1)
        sqd = d.sqrt()
        tb = c32(t) + c32(t_frac) * d
    else:
        d = torch.full((Bn, 1), c32(delta), dtype=dt, device=X.device)
        sqd = torch.full_like(d, c32(delta ** 0.5 if sqrt_delta is None else sqrt_delta))
        tb = torch.full_like(d, c32(t))
    beta, kb = _beta(tb, rev, dt)
    sb = beta.sqrt()
    W = dW.to(dt) if dW is not None else sqd * z.to(dt)
    A = a.to(dt) if (rev and a is not None) else None
    sig = math.sqrt(1.0 - l) if rev else 1.0
    zero = torch.zeros_like(X)
    if kind == "sgm":
        f = -0.5 * beta * X
        mf = kb * f.abs()
        fs, mfs, div, mdiv = f, mf, zero, zero
        gw, mgw = sb * W, kb * (sb * W).abs()
        ga, mga = (sb * A, kb * (sb * A).abs()) if A is not None else (zero, zero)
    elif kind == "sparse":
        xp, xm = torch.roll(X, -1, 1), torch.roll(X, 1, 1)
        f = 0.5 * beta * X
        mf = kb * f.abs()
        fs, mfs, div, mdiv = zero, zero, 2.0 * f, 2.0 * mf
        cp, cm = CV32 * (sb * xp), -CV32 * (sb * xm)
        gw = cp * W + cm * torch.roll(W, 1, 1)
        mgw = kb * (cp.abs() * W.abs() + cm.abs() * torch.roll(W, 1, 1).abs())
        if A is not None:
            ga = cp * A + cm * torch.roll(A, 1, 1)
            mga = kb * (cp.abs() * A.abs() + cm.abs() * torch.roll(A, 1, 1).abs())
        else:
            ga, mga = zero, zero
    else:
        Gd, Ld = G.to(dt), L_G.to(dt)
        f = _dense2(Ld, beta * X)
        mf = kb * _dense2(Ld.abs(), beta * X.abs())
        fs, mfs, div, mdiv = zero, zero, 2.0 * f, 2.0 * mf
        y, Ga = sb * X, Gd.abs()
        gw = _dense3(Gd, y, W)
        mgw = kb * _dense3(Ga, y.abs(), W.abs())
        if A is not None:
            ga = _dense3(Gd, y, A)
            mga = kb * _dense3(Ga, y.abs(), A.abs())
        else:
            ga, mga = zero, zero
    if rev:
        mu = (1.0 - 0.5 * l) * ga - f + (1.0 - l) * div
        mmu = (1.0 - 0.5 * l) * mga + mf + (1.0 - l) * mdiv
        if strato:
            mu = mu - 0.5 * (1.0 - l) * div
            mmu = mmu + 0.5 * (1.0 - l) * mdiv
    else:
        mu, mmu = fs, mfs
        if not strato:
            mu = mu + 0.5 * div
            mmu = mmu + 0.5 * mdiv
    inc = mu * d + sig * gw
    minc = mmu * d + sig * mgw
    co = c32(c_out)
    if base is not None:
        o, mo = base.to(dt) + co * inc, base.to(dt).abs() + abs(co) * minc
    else:
        o, mo = co * inc, abs(co) * minc
    if norm0 is not None:
        o, mo = _renorm(o, mo, norm0.to(dt))
    return {"out": (o, mo), "inc": (inc, minc), "dW": (W, W.abs())}


# ------------------------------------------------------------------------------------------------ row kernels
def rk4_combine(x, k1, k2, k3, k4, norm0=None, dtype=torch.float64):
    x, k1, k2, k3, k4 = (v.to(dtype) for v in (x, k1, k2, k3, k4))
    o = x + (k1 + 2.0 * k2 + 2.0 * k3 + k4) / 6.0
    mo = x.abs() + (k1.abs() + 2.0 * k2.abs() + 2.0 * k3.abs() + k4.abs()) / 6.0
    if norm0 is not None:
        o, mo = _renorm(o, mo, norm0.to(dtype))
    return o, mo


def row_norm(x, dtype=torch.float64):
    r = _rsum(x.to(dtype) ** 2).sqrt()
    return r, r


def ssm_terms(kind, y, v, t, G=None, dtype=torch.float64):
    """(u, cst): loss_b = adot.u + cst + |a|^2 / 2  (k_ssm_terms).  Returns ((u, mag), (cst, mag))."""
    Y, V = y.to(dtype), v.to(dtype)
    beta, kb = _beta(t.to(dtype).reshape(-1, 1), False, dtype)
    sb = beta.sqrt()
    if kind == "sgm":
        u = sb * V
        cst = _rsum(0.5 * beta * V * V)
        return (u, kb * u.abs()), (cst, _rsum(kb * 0.5 * beta * V * V))
    zero = torch.zeros(Y.shape[0], dtype=dtype, device=Y.device)
    if kind == "sparse":
        yp, vp = torch.roll(Y, -1, 1), torch.roll(V, -1, 1)
        u = (CV32 * sb) * (V * yp - vp * Y)
        return (u, kb * (CV32 * sb) * ((V * yp).abs() + (vp * Y).abs())), (zero, zero)
    Gd = G.to(dtype)
    Gt = Gd.permute(2, 0, 1)                            # [k][i][j]: u_k = sb sum_i (sum_j G_ijk y_j) v_i
    u = sb * _dense3(Gt, V, Y)
    return (u, kb * sb * _dense3(Gt.abs(), V.abs(), Y.abs())), (zero, zero)


def ssm_loss(out, u, cst, w, dtype=torch.float64):
    """per[b] = adot.u + cst + |a|^2 / 2; g[:B] = a w; g[B:] = u w  (k_ssm_loss_generic; out = [a ; adot]).
    Returns ((per, mag), (g_a, mag), (g_adot, mag))."""
    Bn, n = u.shape
    O, U, w = out.to(dtype).reshape(2 * Bn, n), u.to(dtype), c32(w)
    a, ad = O[:Bn], O[Bn:]
    per = _rsum(ad * U + 0.5 * a * a) + cst.to(dtype)
    mper = _rsum((ad * U).abs() + 0.5 * a * a) + cst.to(dtype).abs()
    return (per, mper), (a * w, (a * w).abs()), (U * w, (U * w).abs())


def ssm_loss_diag(out, v, t, w, dtype=torch.float64):
    """SGM: per[b] = sum_i v_i (sqrt(beta) adot_i + beta v_i / 2) + a_i^2 / 2; g[:B] = a w; g[B:] = sqrt(beta) v w."""
    Bn, n = v.shape
    O, V, w = out.to(dtype).reshape(2 * Bn, n), v.to(dtype), c32(w)
    a, ad = O[:Bn], O[Bn:]
    beta, kb = _beta(t.to(dtype).reshape(-1, 1), False, dtype)
    sb = beta.sqrt()
    per = _rsum(V * (sb * ad + 0.5 * beta * V) + 0.5 * a * a)
    mper = _rsum(kb * V.abs() * ((sb * ad).abs() + 0.5 * beta * V.abs()) + 0.5 * a * a)
    g2 = sb * V * w
    return (per, mper), (a * w, (a * w).abs()), (g2, kb * g2.abs())


# ------------------------------------------------------------------------------------------------ elementwise
def perturb_vp(x0, t, eps, dtype=torch.float64):
    """y = eps sqrt(1 - E) + mw x0 at row times t, used as given (k_perturb_vp)."""
    b0, b1 = c32(B0), c32(B1)
    db = c32(b1 - b0) if dtype == torch.float32 else b1 - b0
    tt = t.to(dtype).reshape(-1, 1)
    X, Ez = x0.to(dtype), eps.to(dtype)
    ex = lambda q: torch.exp(q.double()).to(dtype)      # float32: the correctly rounded exp, the same bits on every CPU
    mw = ex(-0.25 * (tt * tt) * db - 0.5 * tt * b0)
    E = ex(-0.5 * (tt * tt) * db - tt * b0)
    sd = (1.0 - E).sqrt()
    y = Ez * sd + mw * X
    return y, Ez.abs() * (sd + (1.0 + E) / (2.0 * sd)) + mw * X.abs()


def clamp_time(u):
    """float32, exact: t = u T, rows with t <= t_eps set to t_eps by mask arithmetic."""
    t = u.float() * np.float32(T_END)
    m = (t <= np.float32(T_EPS)).float()
    return m * np.float32(T_EPS) + (1.0 - m) * t


def time_tick(ts, step, B, t_add=0.0):
    """float32, exact: t = ts[min(step, n_ts - 1)] (+ t_add), s_out = T - t.  Returns (t, s_out[B]) on the CPU."""
    tv = ts.detach().cpu().float()[min(int(step), ts.numel() - 1)]
    if t_add != 0.0:
        tv = tv + torch.tensor(np.float32(t_add))
    return tv, (torch.tensor(np.float32(T_END)) - tv).expand(B).clone()


def lincomb(a, c0, b=None, c1=0.0, c=None, c2=0.0, dtype=torch.float64):
    v = c32(c0) * a.to(dtype)
    m = v.abs()
    for cc, tt in ((c1, b), (c2, c)):
        if tt is not None:
            v = v + c32(cc) * tt.to(dtype)
            m = m + (c32(cc) * tt.to(dtype)).abs()
    return v, m


def adam_step(p, g, m, v, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, gscale=1.0, dtype=torch.float64):
    """One Adam step as k_adam forms it: bias corrections in double, then float32 step size, sqrt(bc2), 1 - b1, b2,
    1 - b2 and eps.  Returns ((p, mag), (m, mag), (v, mag))."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    ss, bs = c32(lr / bc1), c32(math.sqrt(bc2))
    w1, b2f, w2, ef = c32(1.0 - beta1), c32(beta2), c32(1.0 - beta2), c32(eps)
    P, Gr, M, V = (q.to(dtype).reshape(-1) for q in (p, g, m, v))
    gg = Gr * c32(gscale)
    mn = M + w1 * (gg - M)
    mm = M.abs() + w1 * (gg.abs() + M.abs())
    vn = V * b2f + w2 * (gg * gg)
    den = vn.sqrt() / bs + ef
    pn = P - ss * (mn / den)
    return (pn, P.abs() + ss * (mm / den)), (mn, mm), (vn, vn)


# ------------------------------------------------------------------------------------------------ case shapes
# Shared by the CPU tolerance measurement and the GPU tests (tests/test_sde_paths_gpu.py documents which kernel and body
# each one reaches).  GS is launch_rows' lane-group width for n; the ragged batch 2 * (256 / GS) + 1 fills two
# workgroups and one group of a third.
N_LIST = (1, 2, 3, 5, 9, 17, 33, 65, 2047, 2048, 2050)
CAP_SHAPES = ((524293, 2), (16387, 33), (4099, 2048))           # past the 4096-block cap: a second trip of the row loop
DENSE_N = (2, 7, 16, 64)
COMBOS = (("forward", False, 0.0), ("forward", True, 0.0), ("reverse", False, 0.0), ("reverse", True, 0.0),
          ("reverse", False, 0.25), ("reverse", True, 0.25))


def group_width(n):
    gs = 2
    while gs < 64 and gs < n:
        gs <<= 1
    return 256 if n >= 2048 else gs


def ragged_B(n):
    return 2 * (256 // group_width(n)) + 1


def row_shapes(with_cap=True):
    s = [(B, n) for n in N_LIST for B in (1, ragged_B(n))]
    return s + list(CAP_SHAPES) if with_cap else s


T0, DELTA = 0.37, 1.0 / 16


def randn(*shape, generator, device="cpu"):
    """Standard normals as float32, drawn in float64 and rounded: torch's float32 CPU randn gives other bits on CPUs with
    another vector width, and the figures behind the tolerance constants must not depend on the machine."""
    return torch.randn(*shape, generator=generator, device=device, dtype=torch.float64).float()


def stage_inputs(B, n, seed, device="cpu"):
    """x, a, z, base (B,n), norm0 (B,) = |x| rows, delta_rows (B,) uniform in (1e-4, 0.05): float32 on ``device``."""
    g = torch.Generator(device=device).manual_seed(seed)
    r = lambda *s: randn(*s, generator=g, device=device)
    x, a, z, base = r(B, n), r(B, n), r(B, n), r(B, n)
    dr = 1e-4 + (0.05 - 1e-4) * torch.rand(B, generator=g, device=device)
    return {"x": x, "a": a, "z": z, "base": base, "norm0": x.double().norm(dim=1).float(), "delta_rows": dr}
