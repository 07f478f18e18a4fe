"""Float64 parity of csrc/sde_kernels.hip on every dispatch path.

Every output is compared PER ELEMENT with the float64 restatement of tests/sde_stage_ref.py, evaluated by torch on the
device: |kernel - ref64| <= c * 2^-24 * magnitude, c per output family from the CPU float32 measurement
(sde_stage_ref.MEASURED, guarded by tests/test_sde_stage_ref.py).  Output buffers are pre-filled with NaN and asserted
finite over their whole extent first.  Integer outputs, masks, times and everything documented as exact are bit-exact.

Case -> kernel and body, from the dispatch conditions of msgm_sde_stage, msgm_rk4_combine and launch_rows
(GS: 1-2 -> 2, 3-4 -> 4, 5-8 -> 8, 9-16 -> 16, 17-32 -> 32, 33-2047 -> 64, >= 2048 -> 256 through LDS; grid caps: rows
4096 blocks, flat 2048 blocks of 256 quads, k_time_tick 256 blocks):

  test / case                                   kernel                     body / what is new in it
  --------------------------------------------  -------------------------  ------------------------------------------------
  stage_flat sgm (3,4)                          k_stage_diag_flat          vector body (B n % 4 == 0, all aligned)
  stage_flat sgm (2049,1024)                    k_stage_diag_flat          vector body, 524 544 quads: one quad past the cap
  stage_flat sgm (5,3)                          k_stage_diag_flat          scalar body (15 % 4 != 0), ragged last quad
  stage_flat sgm (3,4) x shifted                k_stage_diag_flat          scalar body (x 4-byte aligned only)
  stage_flat sgm (699051,3) forward             k_stage_diag_flat          scalar body, 2 097 153 elements: grid-stride trip
  stage_flat sparse n 8|12|256, B 1|33          k_stage_sparse_flat        quads open / close rows (em, ep), one / many rows
  stage_flat sparse (2049,1024)                 k_stage_sparse_flat        second grid-stride trip
  stage_sparse_falls_back n 3|4|6               k_stage_rows<4|4|8>        n % 4 != 0 or n < 8
  stage_sparse_falls_back norm0 (33,8)          k_stage_rows<8>            norm0 given
  stage_sparse_falls_back shifted (33,8)        k_stage_rows<8>            x misaligned; bitwise equal to the flat kernel
  stage_rows sgm+norm0 | sgm+delta_rows |       k_stage_rows<GS>           n in N_LIST: GS 2,2,4,8,16,32,64,64,64,256,256;
    sparse+norm0, (B,n) in row_shapes()                                    B = 1 and 2 (256 / GS) + 1 (third workgroup);
                                                                           (524293,2) (16387,33) (4099,2048): second trip
                                                                           of the rows_pad loop with dead padded rows
  stage_dense n 2|7|16|64, B 1|9, +-norm0       k_stage_rows<2|8|16|64>    dense contraction; n = 65 refused
  stage_options                                 diag_flat / sparse_flat /  base None | x | third, c_out, inc_out, dW_out,
                                                k_stage_rows<8>            dW vs z, delta_rows x t_frac, t_dev, in place
  stage_inkernel_noise                          diag vec (33,8); diag      philox_normal4 / philox_normal1 / the __shfl_up
                                                scalar (5,3); sparse flat  neighbour draw: row-opening fall-back (n 8,
                                                (33,8) (3,256) (33,12)     256), lane-0 fall-back mid-row (n 12, 1024);
                                                (3,1024); rows             shard base; step_dev
  row_kernels (B,n) in row_shapes()             k_rk4_combine_flat         B n % 4 == 0 and aligned
                                                k_rk4_combine<GS>          B n % 4 != 0, shifted buffer, norm0
                                                k_row_norm<GS>, k_ssm_terms<GS> (sgm, sparse), k_ssm_loss_generic<GS>,
                                                k_ssm_loss_diag<GS>
  ssm_terms_dense n 2|7|64                      k_ssm_terms<2|8|64>        dense; 65 refused
  perturb_*                                     k_perturb_vp               d 1|2|3|5|1024: quads over 4, 2-3, 2, 1-2 rows
  ssm_prep (5,3) (3,4) (33,8) (7,1)             k_ssm_prep                 quads over 2, 1, 1, 4 rows, ragged last quad (15, 7
                                                                           elements); shard base; the step counter; bitwise
                                                                           k_perturb_vp and k_rademacher (vp_row / vp_value)
  time_tick                                     k_time_tick                B 65541: past the 256-block cap; clamp
  lincomb / keep_rows / adam / fill             k_lincomb, k_keep_rows, k_adam (vector and scalar body), k_fill<>
"""
import os
import re

import numpy as np
import pytest
import torch

import sde_stage_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}                    # family -> worst kernel ratio seen (written to $SDE_PARITY_REPORT, for information only)


@pytest.fixture(scope="module")
def ops():
    from sdeflow_light_amd import ops as _ops
    _ops.lib()
    yield _ops
    path = os.environ.get("SDE_PARITY_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("worst |kernel - ref64| / (2^-24 magnitude) per output family on the MI355X (bound c in brackets)\n")
            for k in sorted(WORST, key=str):
                fam = k[0] if k[1] is None else f"{k[0]} n<={k[1]}"
                f.write(f"{fam:18s} {WORST[k][0]:.3f}  [{WORST[k][1]:.2f}]  {WORST[k][2]}\n")


@pytest.fixture(scope="module")
def L():
    from sdeflow_light_amd import _lib
    return _lib


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# The ops wrappers of these entry points allocate their outputs themselves (torch.empty), so a NaN pre-fill cannot be
# handed to them: the tests call the C ABI on their own NaN buffers, and test_wrappers_equal_c_abi ties the wrappers to it.
def _call(L, name, *args):
    L.check(getattr(L.lib(), name)(*args, L.stream()), name)


def c_row_norm(L, x):
    (B, n), out = x.shape, nan(x.shape[0])
    _call(L, "msgm_row_norm", L.ptr(x), L.ptr(out), B, n)
    return out


def c_ssm_terms(L, y, v, t, st):
    (B, n), u, cst = y.shape, nan(*y.shape), nan(y.shape[0])
    _call(L, "msgm_ssm_terms", L.ptr(y), L.ptr(v), L.ptr(t), L.ptr(u), L.ptr(cst), B, n, st)
    return u, cst


def c_ssm_loss(L, out, u, cst, w):
    (B, n), per, g = u.shape, nan(u.shape[0]), nan(2 * u.numel())
    _call(L, "msgm_ssm_loss", L.ptr(out), L.ptr(u), L.ptr(cst), L.ptr(per), L.ptr(g), B, n, float(w))
    return per, g


def c_ssm_loss_diag(L, out, v, t, st, w):
    (B, n), per, g = v.shape, nan(v.shape[0]), nan(2 * v.numel())
    _call(L, "msgm_ssm_loss_diag", L.ptr(out), L.ptr(v), L.ptr(t), L.ptr(per), L.ptr(g), B, n, st, float(w))
    return per, g


def c_perturb_vp(L, x0, st, u, eps):
    (B, d), y, t = x0.shape, nan(*x0.shape), nan(x0.shape[0])
    _call(L, "msgm_perturb_vp", L.ptr(x0), L.ptr(y), L.ptr(t), None, B, d, st, L.ptr(u), L.ptr(eps), None)
    return y, t


def c_perturb_vp_at(L, x0, st, t, eps=None, rng=None):
    (B, d), y = x0.shape, nan(*x0.shape)
    eo = nan(B, d) if rng is not None else None
    _call(L, "msgm_perturb_vp_at", L.ptr(x0), L.ptr(y), L.ptr(eo), B, d, st, L.ptr(t), L.ptr(eps),
          rng.ptr() if rng is not None else None)
    return (y, eo) if rng is not None else y


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "msgm_hip.h")) as _h:
    MSGM_E_BADARG = int(re.search(r"MSGM_E_BADARG\s*=\s*(-?\d+)", _h.read()).group(1))      # _lib carries MSGM_E_UNSUPPORTED only


def c_ssm_prep(L, x0, st, rng, ctr):
    (B, d), y, t, v = x0.shape, nan(*x0.shape), nan(x0.shape[0]), nan(*x0.shape)
    _call(L, "msgm_ssm_prep", L.ptr(x0), L.ptr(y), L.ptr(t), L.ptr(v), B, d, st, rng.ptr(), L.ptr(ctr))
    return y, t, v


def shifted(t):
    """The same values in a contiguous buffer that is 4-byte but not 16-byte aligned."""
    buf = torch.empty(t.numel() + 4, device=DEV, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def check(family, n, y, ref_mag, what):
    """finite everywhere, then per element within c 2^-24 magnitude of the float64 reference"""
    ref, mag = ref_mag
    assert y.shape == ref.shape or y.numel() == ref.numel(), what
    y = y.reshape(ref.shape)
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite output (an unwritten NaN pre-fill?)"
    r, c = R.ratio(y, ref, mag), R.c_of(family, n)
    m = R.MEASURED[family]
    key = (family, min(k for k in m if n <= k) if isinstance(m, dict) else None)
    if r > WORST.get(key, (-1.0,))[0]:
        WORST[key] = (r, c, what)
    print(f"{what}: {family} ratio {r:.3f} (c = {c:.2f})")
    assert r <= c, (what, family, r, c)


def sde(L, kind, G=None, L_G=None):
    k = {"sgm": L.SDE_SGM, "sparse": L.SDE_MSGM_SPARSE, "dense": L.SDE_MSGM_DENSE}[kind]
    return L.sde_struct(k, R.B0, R.B1, R.T_END, R.T_EPS, G, L_G)


def run_stage(ops, L, kind, proc, strato, lmbd, d, *, x=None, base="x", c_out=1.0, noise="z", norm0=False, dr=False,
              t_frac=0.5, t=R.T0, t_dev=None, G=None, L_G=None, out=None, rng=None, rng_step=0, step_dev=None, dW=None):
    """One msgm_sde_stage launch on NaN-filled out / inc_out / dW_out.  Returns (out, inc_out, dW_out)."""
    x = d["x"] if x is None else x
    B, n = x.shape
    out = nan(B, n) if out is None else out
    inc, dwo = nan(B, n), nan(B, n)
    bs = {"x": x, "none": None, "third": d["base"]}[base]
    kw = {"z": d["z"]} if noise == "z" else {"dW": dW} if noise == "dW" else {"rng": rng, "rng_step": rng_step, "step_dev": step_dev}
    ops.sde_stage(out, bs, c_out, x, d["a"] if proc == "reverse" else None, sde(L, kind, G, L_G),
                  L.PROC_REVERSE if proc == "reverse" else L.PROC_FORWARD, strato, t, R.DELTA, lmbd, dW_out=dwo, inc_out=inc,
                  norm0=d["norm0"] if norm0 else None, delta_rows=d["delta_rows"] if dr else None, t_frac=t_frac, t_dev=t_dev,
                  **kw)
    return out, inc, dwo


def ref_stage(kind, proc, strato, lmbd, d, *, base="x", c_out=1.0, norm0=False, dr=False, t_frac=0.5, t=R.T0, G=None, L_G=None,
              dW=None):
    bs = {"x": d["x"], "none": None, "third": d["base"]}[base]
    return R.stage(kind, proc, strato, d["x"], d["a"], t=t, delta=R.DELTA, lmbd=lmbd, z=None if dW is not None else d["z"],
                   dW=dW, base=bs, c_out=c_out, norm0=d["norm0"] if norm0 else None,
                   delta_rows=d["delta_rows"] if dr else None, t_frac=t_frac, G=G, L_G=L_G)


def stage_case(ops, L, kind, B, n, what, combos=R.COMBOS, fam=None, shift_x=False, **opt):
    """All (proc, strato, lmbd) of one shape and option set against float64: out, inc_out and dW_out."""
    d = R.stage_inputs(B, n, 131 * n + B, DEV)
    G, L_G = R.dense_G(n, device=DEV) if kind == "dense" else (None, None)
    xs = shifted(d["x"]) if shift_x else None
    nc = opt.get("norm0", False)
    fam = fam or (("dense" if kind == "dense" else "stage") + ("_nc" if nc else ""))
    for proc, strato, lmbd in combos:
        out, inc, dwo = run_stage(ops, L, kind, proc, strato, lmbd, d, x=xs, G=G, L_G=L_G, **opt)
        ref = ref_stage(kind, proc, strato, lmbd, d, G=G, L_G=L_G, **opt)
        tag = f"{what} {kind} ({B},{n}) {proc} strato={strato} lmbd={lmbd}"
        check(fam, n, out, ref["out"], tag + " out")
        check("dense" if kind == "dense" else "stage", n, inc, ref["inc"], tag + " inc_out")
        check("stage", n, dwo, ref["dW"], tag + " dW_out")


# ================================================================================================ (a) dispatch paths
FLAT = [("sgm", 3, 4, False), ("sgm", 2049, 1024, False), ("sgm", 5, 3, False), ("sgm", 3, 4, True)] + \
       [("sparse", B, n, False) for n in (8, 12, 256) for B in (1, 33)] + [("sparse", 2049, 1024, False)]


@pytest.mark.parametrize("kind,B,n,shift", FLAT)
def test_stage_flat(ops, L, kind, B, n, shift):
    torch.manual_seed(B * 1000 + n)
    stage_case(ops, L, kind, B, n, "flat" + (" shifted-x" if shift else ""), shift_x=shift)


def test_stage_flat_scalar_body_grid_stride(ops, L):
    torch.manual_seed(1)
    stage_case(ops, L, "sgm", 699051, 3, "flat", combos=R.COMBOS[:2])          # forward, both strato


@pytest.mark.parametrize("n", [3, 4, 6])
def test_stage_sparse_falls_back_to_rows(ops, L, n):
    torch.manual_seed(n)
    stage_case(ops, L, "sparse", 33, n, "fallback")


def test_stage_sparse_falls_back_with_norm0(ops, L):
    torch.manual_seed(8)
    stage_case(ops, L, "sparse", 33, 8, "fallback norm0", norm0=True)


def test_stage_sparse_rows_bitwise_equals_flat(ops, L):
    """The source promises the same bits from k_stage_sparse_flat and k_stage_rows; a misaligned x selects the latter."""
    torch.manual_seed(9)
    for dr in (False, True):
        d = R.stage_inputs(33, 8, 77, DEV)
        xs = shifted(d["x"])
        for proc, strato, lmbd in R.COMBOS:
            f = run_stage(ops, L, "sparse", proc, strato, lmbd, d, base="third", c_out=0.5, dr=dr)
            r = run_stage(ops, L, "sparse", proc, strato, lmbd, d, x=xs, base="third", c_out=0.5, dr=dr)
            for a, b, nm in zip(f, r, ("out", "inc_out", "dW_out")):
                assert bool(torch.isfinite(a).all()) and torch.equal(a, b), (nm, proc, strato, lmbd, dr)
            check("stage", 8, r[0], ref_stage("sparse", proc, strato, lmbd, d, base="third", c_out=0.5, dr=dr)["out"],
                  f"rows via shifted x {proc} {strato} {lmbd} dr={dr}")


ROWS_VARIANTS = {"sgm_norm0": ("sgm", dict(norm0=True)), "sgm_delta_rows": ("sgm", dict(dr=True)),
                 "sparse_norm0": ("sparse", dict(norm0=True))}


@pytest.mark.parametrize("B,n", R.row_shapes())
@pytest.mark.parametrize("variant", list(ROWS_VARIANTS))
def test_stage_rows(ops, L, variant, B, n):
    torch.manual_seed(B + n)
    kind, opt = ROWS_VARIANTS[variant]
    stage_case(ops, L, kind, B, n, variant, combos=R.COMBOS if B * n < 1_000_000 else R.COMBOS[1::4] + R.COMBOS[4:5], **opt)


@pytest.mark.parametrize("n", R.DENSE_N)
@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("nc", [False, True])
def test_stage_dense(ops, L, n, B, nc):
    torch.manual_seed(n + B)
    stage_case(ops, L, "dense", B, n, "dense", norm0=nc)


def test_stage_dense_65_refused(ops, L):
    d = R.stage_inputs(2, 65, 1, DEV)
    G, L_G = torch.zeros(65, 65, 65, device=DEV), torch.zeros(65, 65, device=DEV)
    with pytest.raises(L.MsgmError):
        run_stage(ops, L, "dense", "forward", False, 0.0, d, G=G, L_G=L_G)
    with pytest.raises(L.MsgmError):
        ops.ssm_terms(d["x"], d["a"], torch.rand(2, device=DEV), sde(L, "dense", G, L_G))


# ================================================================================================ (b) options
OPT_SHAPES = [("sgm", 33, 8, {}), ("sgm", 33, 8, {"norm0": True}), ("sparse", 33, 8, {}), ("sparse", 33, 6, {}),
              ("dense", 9, 7, {})]


@pytest.mark.parametrize("kind,B,n,opt", OPT_SHAPES)
def test_stage_options(ops, L, kind, B, n, opt):
    torch.manual_seed(n + len(opt))
    for base in ("none", "x", "third"):
        for c_out in (1.0, 0.5):
            stage_case(ops, L, kind, B, n, f"base={base} c_out={c_out}", combos=R.COMBOS[3:5], base=base, c_out=c_out, **opt)
    for tf in (0.0, 0.5, 1.0):                                  # sgm: delta_rows always selects k_stage_rows
        stage_case(ops, L, kind, B, n, f"delta_rows t_frac={tf}", combos=R.COMBOS[1::2], dr=True, t_frac=tf, base="third", **opt)
    d = R.stage_inputs(B, n, 5, DEV)
    if kind == "dense":
        opt = dict(opt, **dict(zip(("G", "L_G"), R.dense_G(n, device=DEV))))
    sqd = torch.tensor(np.float32(R.DELTA ** 0.5), device=DEV)
    for proc, strato, lmbd in R.COMBOS[1::2]:
        z_run = run_stage(ops, L, kind, proc, strato, lmbd, d, base="third", **opt)
        w_run = run_stage(ops, L, kind, proc, strato, lmbd, d, base="third", noise="dW", dW=sqd * d["z"], **opt)
        for a, b in zip(z_run, w_run):                          # dW = fl32(sqrt(delta)) z is the very same float32 product
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
        # the device time wins over a deliberately different host t
        t_dev = torch.tensor([np.float32(R.T0)], device=DEV)
        td = run_stage(ops, L, kind, proc, strato, lmbd, d, base="third", t=0.9, t_dev=t_dev, **opt)
        for a, b in zip(z_run, td):
            assert torch.equal(a, b)
        host = run_stage(ops, L, kind, proc, strato, lmbd, d, base="third", t=0.9, **opt)
        assert not torch.equal(host[0], z_run[0])
        if kind == "sgm":                                       # in place: out is x (and base is x)
            ref_run = run_stage(ops, L, kind, proc, strato, lmbd, d, **opt)
            xi = d["x"].clone()
            ip = run_stage(ops, L, kind, proc, strato, lmbd, d, x=xi, out=xi, **opt)
            assert ip[0].data_ptr() == xi.data_ptr() and torch.equal(ip[0], ref_run[0]) and torch.equal(ip[1], ref_run[1])


# ================================================================================================ (c) in-kernel noise
SEED, OFFSET, STEP = (1 << 40) + 12345, (1 << 33) + 7, 5
NOISE_CASES = [("sgm", 33, 8, {}, "diag vector"), ("sgm", 5, 3, {}, "diag scalar"), ("sparse", 33, 8, {}, "sparse flat"),
               ("sparse", 3, 256, {}, "sparse flat"), ("sparse", 33, 8, {"dr": True}, "sparse flat"),
               ("sparse", 33, 12, {}, "sparse flat, rows cross waves"), ("sparse", 3, 1024, {}, "sparse flat, rows cross waves"),
               ("sparse", 3, 1024, {"dr": True}, "sparse flat, rows cross waves"),
               ("sparse", 33, 6, {}, "rows"), ("sgm", 33, 8, {"norm0": True}, "rows"), ("sgm", 33, 5, {"dr": True}, "rows"),
               ("sparse", 9, 2048, {"norm0": True}, "rows<256>")]


@pytest.mark.parametrize("kind,B,n,opt,path", NOISE_CASES)
@pytest.mark.parametrize("row_base", [0, 4])
def test_stage_inkernel_noise(ops, L, kind, B, n, opt, path, row_base):
    """dW_out equals the device fill of RNG_STREAM_DW at offset + step, scaled by fl32(sqrt(delta)) or sqrtf(delta_b);
    out equals the same call given that noise through dW=.  (The normals use fast __logf / __sincosf: the device fill
    is the reference for the draws, float64 parity given dW covers the arithmetic.)
    The sparse flat kernel takes the previous element's draw from the neighbouring lane, except where the quad opens a
    row (i0 == 0) or sits in lane 0 of its wave.  Quad q runs in lane q % 64.  n = 8 (2 quads per row): every even quad
    opens a row.  n = 256 (64 quads = one wave per row): lane 0 always opens a row.  n = 12 (3 quads per row) and
    n = 1024 (256 quads = four waves per row): lane 0 of later waves is mid-row, the lane-0 branch on its own."""
    torch.manual_seed(n)
    d = R.stage_inputs(B, n, 3 * n + B, DEV)
    rng = L.PhiloxState(SEED, DEV, OFFSET, row_base, n)
    z = ops.fill_normal(nan(B, n), L.PhiloxState(SEED, DEV, OFFSET + STEP, row_base, n), L.RNG_STREAM_DW)
    assert bool(torch.isfinite(z).all())
    if row_base:                                             # a shard draws other numbers than the unsharded state
        assert not torch.equal(z, ops.fill_normal(nan(B, n), L.PhiloxState(SEED, DEV, OFFSET + STEP), L.RNG_STREAM_DW))
    if opt.get("dr"):
        sqd = d["delta_rows"].sqrt().reshape(B, 1)                            # the device's float32 sqrtf
    else:
        sqd = torch.tensor(np.float32(R.DELTA ** 0.5), device=DEV)
    dW = sqd * z
    step_dev = torch.tensor([STEP], dtype=torch.int64, device=DEV)
    for proc, strato, lmbd in R.COMBOS[1::2]:
        got = run_stage(ops, L, kind, proc, strato, lmbd, d, base="third", noise="rng", rng=rng, rng_step=STEP, **opt)
        assert all(bool(torch.isfinite(g).all()) for g in got)
        bad = (got[2] != dW).nonzero()
        assert bad.numel() == 0, (path, "dW_out differs from the device fill first at (row, col)", bad[0].tolist())
        giv = run_stage(ops, L, kind, proc, strato, lmbd, d, base="third", noise="dW", dW=dW, **opt)
        assert torch.equal(got[0], giv[0]) and torch.equal(got[1], giv[1]), path
        sd = run_stage(ops, L, kind, proc, strato, lmbd, d, base="third", noise="rng", rng=rng, rng_step=999, step_dev=step_dev, **opt)
        assert all(torch.equal(a, b) for a, b in zip(got, sd)), path
        check("stage" + ("_nc" if opt.get("norm0") else ""), n, got[0],
              ref_stage(kind, proc, strato, lmbd, d, base="third", dW=dW, **opt)["out"], f"in-kernel noise {path} ({B},{n})")


# ================================================================================================ (d) row kernels
@pytest.mark.parametrize("B,n", R.row_shapes())
def test_row_kernels(ops, L, B, n):
    g = torch.Generator(device=DEV).manual_seed(17 * n + B)
    x, k1, k2, k3, k4, a, ad = (torch.randn(B, n, generator=g, device=DEV) for _ in range(7))
    v = (torch.rand(B, n, generator=g, device=DEV) >= 0.5).float() * 2 - 1
    t = R.clamp_time(torch.rand(B, generator=g, device=DEV))
    n0 = x.double().norm(dim=1).float()
    tag = f"({B},{n})"
    # rk4_combine: flat when B n % 4 == 0 (all aligned), rows otherwise, rows through a shifted buffer, rows with norm0
    ref = R.rk4_combine(x, k1, k2, k3, k4)
    check("stage", n, ops.rk4_combine(nan(B, n), x, k1, k2, k3, k4), ref, "rk4_combine " + tag)
    check("stage", n, ops.rk4_combine(nan(B, n), x, shifted(k1), k2, k3, k4), ref, "rk4_combine rows (shifted k1) " + tag)
    check("stage_nc", n, ops.rk4_combine(nan(B, n), x, k1, k2, k3, k4, norm0=n0), R.rk4_combine(x, k1, k2, k3, k4, n0),
          "rk4_combine norm0 " + tag)
    check("rows", n, c_row_norm(L, x), R.row_norm(x), "row_norm " + tag)
    out = torch.cat([a, ad]).contiguous()
    w = 1.0 / B
    for kind in ("sgm", "sparse"):
        u, cst = c_ssm_terms(L, x, v, t, sde(L, kind))
        ru, rc = R.ssm_terms(kind, x, v, t)
        check("stage", n, u, ru, f"ssm_terms {kind} u " + tag)
        if kind == "sparse":
            assert bool((cst == 0).all()), "the sparse constant is exactly zero"
        else:
            check("rows", n, cst, rc, f"ssm_terms {kind} cst " + tag)
        per, gg = c_ssm_loss(L, out, u, cst, w)
        rper, rga, rgad = R.ssm_loss(out, u, cst, w)
        check("rows", n, per, rper, f"ssm_loss {kind} per " + tag)
        check("stage", n, gg[:B * n], rga, f"ssm_loss {kind} g[:B] " + tag)
        check("stage", n, gg[B * n:], rgad, f"ssm_loss {kind} g[B:] " + tag)
        if kind == "sgm":
            # the fused SGM kernel and ssm_terms + ssm_loss are two orders of the same sum: each against float64
            dper, dga, dgad = R.ssm_loss_diag(out, v, t, w)
            check("rows", n, per, dper, "ssm_terms + ssm_loss vs the fused formula, per " + tag)
            per2, g2 = c_ssm_loss_diag(L, out, v, t, sde(L, "sgm"), w)
            check("rows", n, per2, dper, "ssm_loss_diag per " + tag)
            check("stage", n, g2[:B * n], dga, "ssm_loss_diag g[:B] " + tag)
            check("stage", n, g2[B * n:], dgad, "ssm_loss_diag g[B:] " + tag)


@pytest.mark.parametrize("n", [2, 7, 64])
@pytest.mark.parametrize("B", [1, 9])
def test_ssm_terms_dense(ops, L, n, B):
    g = torch.Generator(device=DEV).manual_seed(n + B)
    G, L_G = R.dense_G(n, device=DEV)
    y, v = torch.randn(B, n, generator=g, device=DEV), torch.randn(B, n, generator=g, device=DEV)
    t = R.clamp_time(torch.rand(B, generator=g, device=DEV))
    u, cst = c_ssm_terms(L, y, v, t, sde(L, "dense", G, L_G))
    check("dense", n, u, R.ssm_terms("dense", y, v, t, G)[0], f"ssm_terms dense ({B},{n})")
    assert bool((cst == 0).all())


def test_wrappers_equal_c_abi(ops, L):
    """ops.row_norm / ssm_terms / ssm_loss / ssm_loss_diag / perturb_vp / perturb_vp_at give the bits of the C entry
    points the tests above call on their own buffers."""
    g = torch.Generator(device=DEV).manual_seed(1)
    B, n = 37, 10
    x, v, a = (torch.randn(B, n, generator=g, device=DEV) for _ in range(3))
    t = R.clamp_time(torch.rand(B, generator=g, device=DEV))
    out, st = torch.cat([x, a]).contiguous(), sde(L, "sgm")
    eq = lambda p, q: all(torch.equal(i, j) for i, j in zip(p, q))
    assert torch.equal(ops.row_norm(x), c_row_norm(L, x))
    u, cst = c_ssm_terms(L, x, v, t, st)
    assert eq(ops.ssm_terms(x, v, t, st), (u, cst))
    assert eq(ops.ssm_loss(out, u, cst, 1.0 / B), c_ssm_loss(L, out, u, cst, 1.0 / B))
    assert eq(ops.ssm_loss_diag(out, v, t, st, 1.0 / B), c_ssm_loss_diag(L, out, v, t, st, 1.0 / B))
    assert eq(ops.perturb_vp(x, st, u=t, eps=a), c_perturb_vp(L, x, st, t, a))
    assert torch.equal(ops.perturb_vp_at(x, st, t, eps=a), c_perturb_vp_at(L, x, st, t, eps=a))
    rng = L.PhiloxState(SEED, DEV, OFFSET)
    assert eq(ops.perturb_vp_at(x, st, t, rng=rng, return_eps=True), c_perturb_vp_at(L, x, st, t, rng=rng))


# ================================================================================================ (e) elementwise
@pytest.mark.parametrize("d", [1, 2, 3, 5, 1024])
def test_perturb_vp_at(ops, L, d):
    B = 37
    g = torch.Generator(device=DEV).manual_seed(d)
    x0, eps = torch.randn(B, d, generator=g, device=DEV), torch.randn(B, d, generator=g, device=DEV)
    t = torch.rand(B, generator=g, device=DEV)
    t[:6] = torch.tensor([1e-4, 2.5e-4, 5e-4, 9e-4, 1e-3, 1.0], device=DEV)        # below t_epsilon: used as given
    y = c_perturb_vp_at(L, x0, sde(L, "sgm"), t, eps=eps)
    check("perturb", 0, y, R.perturb_vp(x0, t, eps), f"perturb_vp_at eps= d={d}")
    rng = L.PhiloxState(SEED, DEV, OFFSET)
    y2, eo = c_perturb_vp_at(L, x0, sde(L, "sgm"), t, rng=rng)
    assert torch.equal(eo, ops.fill_normal(nan(B, d), rng, L.RNG_STREAM_EPS))
    check("perturb", 0, y2, R.perturb_vp(x0, t, eo), f"perturb_vp_at rng= d={d}")


@pytest.mark.parametrize("d", [1, 2, 3, 5, 1024])
def test_perturb_vp_writes_every_row_time(ops, L, d):
    B = 37
    g = torch.Generator(device=DEV).manual_seed(100 + d)
    x0, eps = torch.randn(B, d, generator=g, device=DEV), torch.randn(B, d, generator=g, device=DEV)
    u = torch.rand(B, generator=g, device=DEV)
    u[:4] = torch.tensor([0.0, 5e-4, 1e-3, 1.0], device=DEV)
    y, t = c_perturb_vp(L, x0, sde(L, "sgm"), u, eps)
    assert torch.equal(t, R.clamp_time(u)), "t_out: every row, bit-exact under the clamp"
    check("perturb", 0, y, R.perturb_vp(x0, t, eps), f"perturb_vp d={d}")


SSM_PREP_SHAPES = [(5, 3), (3, 4), (33, 8), (7, 1)]


@pytest.mark.parametrize("B,d", SSM_PREP_SHAPES)
@pytest.mark.parametrize("row_base", [0, 4])
def test_ssm_prep(ops, L, B, d, row_base):
    """The kernel that opens every training step: y and t are the bits of msgm_perturb_vp(rng=) and v those of
    msgm_rademacher(rng=) from an identical Philox state (same streams and indices, shared vp_row / vp_value,
    contraction off), the step counter ticks once, the Philox state is only read; y also against float64 with the
    perturb family's constant."""
    g = torch.Generator(device=DEV).manual_seed(31 * B + d)
    x0, st = torch.randn(B, d, generator=g, device=DEV), sde(L, "sgm")
    rng = L.PhiloxState(SEED, DEV, OFFSET, row_base, d)
    state0 = rng.state.clone()
    ctr = torch.tensor([41], dtype=torch.int64, device=DEV)
    y, t, v = c_ssm_prep(L, x0, st, rng, ctr)
    assert all(bool(torch.isfinite(o).all()) for o in (y, t, v)), "non-finite output (an unwritten NaN pre-fill?)"
    assert int(ctr) == 42 and torch.equal(rng.state, state0)
    yp, tp = ops.perturb_vp(x0, st, rng=rng)
    assert torch.equal(y, yp) and torch.equal(t, tp)
    # independent of vp_row: the row times are the clamp (bit-exact restatement) of the device fill of RNG_STREAM_T
    assert torch.equal(t, R.clamp_time(ops.fill_uniform(nan(B), rng, L.RNG_STREAM_T)))
    assert torch.equal(v, ops.rademacher((B, d), DEV, rng=rng))
    if row_base:                                             # a shard draws other numbers than the unsharded state
        assert not torch.equal(t, ops.perturb_vp(x0, st, rng=L.PhiloxState(SEED, DEV, OFFSET))[1])
    eps = ops.fill_normal(nan(B, d), rng, L.RNG_STREAM_EPS)
    check("perturb", 0, y, R.perturb_vp(x0, t, eps), f"ssm_prep ({B},{d}) row_base={row_base}")
    assert all(torch.equal(a, b) for a, b in zip(c_ssm_prep(L, x0, st, rng, None), (y, t, v))), "null step counter"
    assert int(ctr) == 42
    args = lambda s, r: (L.ptr(x0), L.ptr(y), L.ptr(t), L.ptr(v), B, d, s, r, L.ptr(ctr), L.stream())   # noqa: E731
    assert L.lib().msgm_ssm_prep(*args(sde(L, "sparse"), rng.ptr())) == L.MSGM_E_UNSUPPORTED
    assert L.lib().msgm_ssm_prep(*args(st, None)) == MSGM_E_BADARG
    assert int(ctr) == 42


@pytest.mark.parametrize("B", [1, 255, 257, 65541])
def test_time_tick(ops, B):
    n_ts, delta = 17, 0.0371                   # times that are not round: ts[i] + t_add and T - t both round in float32
    ts = (0.37 + delta * torch.arange(n_ts, dtype=torch.float64)).float().to(DEV)
    for step in (0, n_ts - 1, n_ts + 3):
        for t_add in (0.0, float(np.float32(delta / 2)), float(np.float32(delta))):
            t_dev, s_out = nan(1), nan(B)
            ops.time_tick(ts, torch.tensor([step], dtype=torch.int64, device=DEV), R.T_END, t_dev, s_out, t_add)
            t_ref, s_ref = R.time_tick(ts, step, B, t_add)
            assert torch.equal(t_dev.cpu().reshape(()), t_ref), (step, t_add)
            assert torch.equal(s_out.cpu(), s_ref), (step, t_add)


@pytest.mark.parametrize("n", [1, 1023, 524289])
def test_lincomb(ops, n):
    g = torch.Generator(device=DEV).manual_seed(n)
    a, b, c = (torch.randn(n, generator=g, device=DEV) for _ in range(3))
    check("lincomb", 0, ops.lincomb(nan(n), a, 0.5), R.lincomb(a, 0.5), f"lincomb 1 operand n={n}")
    check("lincomb", 0, ops.lincomb(nan(n), a, 0.5, b, -2.0), R.lincomb(a, 0.5, b, -2.0), f"lincomb 2 operands n={n}")
    ref = R.lincomb(a, 0.5, b, -2.0, c, 1.0 / 3)
    check("lincomb", 0, ops.lincomb(nan(n), a, 0.5, b, -2.0, c, 1.0 / 3), ref, f"lincomb 3 operands n={n}")
    ai = a.clone()
    check("lincomb", 0, ops.lincomb(ai, ai, 0.5, b, -2.0, c, 1.0 / 3), ref, f"lincomb in place n={n}")


@pytest.mark.parametrize("B,n", [(37, 1), (37, 10), (8193, 10)])
def test_keep_rows(ops, B, n):
    g = torch.Generator(device=DEV).manual_seed(B + n)
    x, kept0 = torch.randn(B, n, generator=g, device=DEV), torch.randn(B, n, generator=g, device=DEV)
    stop = torch.randint(0, 3, (B,), generator=g, device=DEV, dtype=torch.int32)
    kept = ops.keep_rows(kept0.clone(), x, stop, 1)
    assert torch.equal(kept, torch.where((stop == 1)[:, None], x, kept0))


@pytest.mark.parametrize("n", [4, 7, 4096, 2097156])
def test_adam(ops, n):
    """Five steps, each from the kernel's own state, against the float64 restatement; gscale != 1; the device step
    counter against the host step; the vector body (aligned, n % 4 == 0) bitwise against the scalar body (shifted)."""
    g = torch.Generator(device=DEV).manual_seed(n)
    p, m, v = torch.randn(n, generator=g, device=DEV) * 0.1, torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for step in range(1, 6):
        gr = torch.randn(n, generator=g, device=DEV) * 0.01
        ref = R.adam_step(p, gr, m, v, step, gscale=0.5)
        ps, ms, vs, gs = shifted(p), shifted(m), shifted(v), shifted(gr)
        pd, md, vd = p.clone(), m.clone(), v.clone()
        ops.adam_step(p, gr, m, v, step, gscale=0.5)
        for got, rm, nm in zip((p, m, v), ref, "pmv"):
            check("adam", 0, got, rm, f"adam n={n} step {step} {nm}")
        ops.adam_step(ps, gs, ms, vs, step, gscale=0.5)                                   # scalar body
        assert torch.equal(ps, p) and torch.equal(ms, m) and torch.equal(vs, v)
        ops.adam_step(pd, gr, md, vd, 0, gscale=0.5, step_dev=torch.tensor([step], dtype=torch.int64, device=DEV))
        assert torch.equal(pd, p) and torch.equal(md, m) and torch.equal(vd, v)


@pytest.mark.parametrize("normal", [True, False])
def test_fill_prefix_and_misaligned(ops, L, normal):
    rng = L.PhiloxState(SEED, DEV, OFFSET)
    fill = ops.fill_normal if normal else ops.fill_uniform
    full = fill(nan(1028), rng, 21)
    assert bool(torch.isfinite(full).all())
    for n in (1, 2, 3, 1025, 1026, 1027, 1028):
        assert torch.equal(fill(nan(n), rng, 21), full[:n]), n                # the ragged last quad
        buf = nan(n + 8)
        fill(buf[1:1 + n], rng, 21)                                            # 4-byte aligned: the scalar stores
        assert torch.equal(buf[1:1 + n], full[:n]), n
        assert bool(torch.isnan(buf[0])) and bool(torch.isnan(buf[1 + n:]).all()), "wrote outside its extent"
