"""Per-row float64 parity of the fused MLP kernels (csrc/mlp_kernels.hip): cases, inputs, references, the row comparator
and the tolerance table shared by tests/test_mlp_rows_ref.py (CPU) and tests/test_mlp_rows_gpu.py.

Every output is compared with the float64 evaluation of the same formulas (the truth).  The yardstick of a case
(d, premodule, mode) is what the FLOAT32 evaluation of those formulas (torch CPU) loses against float64 at the case's
largest batch; a kernel passes when ``hip_metric <= MEASURED[class][family] * float32_metric``.  Smaller batches of a case
are judged on the largest batch's yardstick: the worst of 32 871 rows is a stable figure, the error of one row is luck.

Parameters are the hash fill (oracle.det_params.init_like_state_dict; weight gain 1 except GAIN); the inputs of batch B
are the first B rows of the case's largest batch, drawn once from one seed per case.
"""
import functools
import math
import zlib

import torch

from oracle import nets_ref as N, sde_ref as S, ssm_ref as LR
from oracle.det_params import init_like_state_dict
from tests_util import mlp_shapes
import sde_stage_ref as R

PRE = "NormalizeLogRadius"
NAMES = tuple(f"main.{i}.{w}" for i in (0, 2, 4, 6) for w in ("weight", "bias"))      # the order of the flat gradient
WEIGHTS = tuple(k for k in NAMES if k.endswith("weight"))

# ------------------------------------------------------------------------------------------------ tolerance constants
# constant = max(default, 2 x the family's largest measured multiple hip_metric / float32_metric, rounded up to 0.1);
# default 2 for a norm, 4 for a worst-of-many (conftest.parity_vs_fp64's slack / slack_worst).  The multiples of every
# case are in profiles/mlp_rows/parity_measured.txt (MI355X).  The condition on every constant is the mutation test of
# tests/test_mlp_rows_ref.py: with it, each planted fault still falls outside the bound by a factor 2.
#
# The gradient families are the only ones above their default, and only through the batches of 1, 15 and 17 rows: the
# yardstick is taken at B = 8245, where every gradient entry is a mean over 8245 rows whose rounding errors average out,
# while at B = 1 a row of dW is zbar_f h^T of ONE sample, with zbar_f a cancelling sum over 128 features.  The float32
# oracle shows the same: against its own B = 8245 figures it stands at 2.5-2.9x (flat), 3-4.4x (worst tensor) and
# 20-57x (worst weight row) at B = 1, 4-8x (worst weight row) at B = 15 / 17, and 1.0-1.2x at B = 4097 — the kernels'
# multiples below.  At B >= 4097 no gradient multiple of a kernel exceeds 1.3, and there the GPU tests hold the gradient
# families to DEFAULTS as well.
MEASURED = {
    "k_mlp": {                  # tiny, narrow and wide carves: d <= 30 and in_dim <= 32
        "fwd_worst": 4.0,       # measured 1.170  fwd/17/B=32871
        "fwd_rel": 3.6,         # measured 1.767  fwd/4/B=1 (one row against the whole-tensor yardstick); B >= 31: 1.150
        "em_worst": 4.0,        # measured 1.345  em/3/B=49255/t=0.75/lmbd=0.5
        "em_rel": 2.7,          # measured 1.308  em/3/B=33/t=0.75/lmbd=0.5
        "loss_worst": 4.0,      # measured 1.124  ssm_general/15n/B=8245
        "loss_rel": 2.9,        # measured 1.414  ssm/30/B=1
        "grad_flat": 7.3,       # measured 3.626  ssm_general/30/B=17
        "grad_tensor": 7.7,     # measured 3.803  ssm/14n/B=1
        "grad_wrow": 51.6,      # measured 25.751 ssm/14n/B=1; B = 15 / 17: 5.827; B >= 4097: 0.922
    },
    "xw": {                     # extra-wide class (k_mlp_xw): d > 30 or in_dim > 32; test b has no extra-wide case
        "fwd_worst": 4.0,       # measured 1.042  fwd/128n/B=16487
        "fwd_rel": 2.4,         # measured 1.187  fwd/31/B=1
        "loss_worst": 4.0,      # measured 0.970  ssm/31/B=8245
        "loss_rel": 2.8,        # measured 1.359  ssm/31/B=1
        "grad_flat": 4.9,       # measured 2.448  ssm/31/B=15
        "grad_tensor": 7.5,     # measured 3.712  ssm/31/B=1
        "grad_wrow": 69.0,      # measured 34.455 ssm/31/B=1; B = 15 / 17: 3.894; B >= 4097: 0.559
    },
}
DEFAULTS = {"fwd_worst": 4.0, "fwd_rel": 2.0, "em_worst": 4.0, "em_rel": 2.0, "loss_worst": 4.0, "loss_rel": 2.0,
            "grad_flat": 2.0, "grad_tensor": 4.0, "grad_wrow": 4.0}
FLOOR_FRAC = 1e-3               # parity_vs_fp64's floor for a near-zero gradient tensor; never engages under this fill

# ------------------------------------------------------------------------------------------------ cases
CASES = ((1, None), (3, None), (2, PRE),                                    # tiny
         (3, PRE), (4, None), (15, None), (14, PRE),                        # narrow
         (15, PRE), (16, None), (17, None), (30, None), (30, PRE),          # wide
         (31, None), (128, PRE))                                            # extra-wide
EM_CASES = ((3, None), (14, PRE), (17, None), (30, PRE))
GENERAL_CASES = ((3, None), (15, PRE), (30, None))
CLASS_CASES = ((3, None), (14, PRE), (17, None), (31, None))                # one per class
EM_POINTS = ((0.0, 0.0), (0.75, 0.5))                                       # (t, lmbd)
EM_DELTA = 0.25
TRAIN_BATCHES = (1, 15, 17, 4097, 8245)         # 16-row tiles, grid cap 256: 8245 = 16 * 515 + 5, three tiles for four workgroups
GENERAL_BATCHES = (17, 8245)


def in_dim(d, pre):
    return d + 1 + (1 if pre else 0)


def klass(d, pre):
    """The carve launch_mlp chooses, restated: three comparisons on d and in_dim."""
    i = in_dim(d, pre)
    if d > 30 or i > 32:
        return "xwide"
    if i > 16 or d > 16:
        return "wide"
    return "tiny" if (i <= 4 and d <= 4) else "narrow"


def table(d, pre):
    return "xw" if klass(d, pre) == "xwide" else "k_mlp"


def fwd_cap(d, pre):
    """Grid cap of the forward and EM launches: workgroups per CU (1 extra-wide, 3 tiny, else 2) x 256."""
    return {"xwide": 256, "tiny": 768}.get(klass(d, pre), 512)


def fwd_batches(d, pre):
    """1, 31, 33; 32 cap + 1: workgroup 0 takes a second tile with one live row; 32 (2 cap + 3) + 7: every workgroup
    takes two tiles and three take a third, ragged end."""
    cap = fwd_cap(d, pre)
    return (1, 31, 33, 32 * cap + 1, 32 * (2 * cap + 3) + 7)


def case_id(d, pre):
    return f"{d}{'n' if pre else ''}"


def _seed(d, pre, mode):
    return zlib.crc32(f"mlp_rows/{d}/{pre}/{mode}/0".encode())


def _gen(d, pre, mode):
    return torch.Generator().manual_seed(_seed(d, pre, mode))


def _rand(*shape, generator):
    return torch.rand(*shape, generator=generator, dtype=torch.float64).float()


# Weight gain of the hash fill (oracle.det_params.init_like_tensor's ``gain``, the remedy the 1-D U-Net parity tests use for
# levels that carry no signal).  MLP(128, NormalizeLogRadius) at gain 1 feeds 130 inputs of size ~0.09 through weights of
# size ~0.09: the gradient is mostly the output bias's, and the first layer's bias gradient is 2.57e-2 of it, under the
# 3e-2 that tests/test_mlp_rows_ref.py::test_fill_conditions requires of every tensor (float64 oracle, B = 8245: 5.65e-2
# at gain 1.25, 1.17e-1 at gain 1.5, 3.36e-1 at gain 2).  1.5 is the smallest of these steps that clears 3e-2 by more
# than the factor 2 the project leaves for other seeds.  Every other case meets the condition at gain 1 and keeps it.
GAIN = {(128, PRE): 1.5}


@functools.lru_cache(maxsize=None)
def params(d, pre):
    return init_like_state_dict(mlp_shapes(d, pre), gain=GAIN.get((d, pre), 1.0))


def cast(p, dt):
    return {k: w.to(dt) for k, w in p.items()}


def split_flat(flat, d, pre):
    """The flat gradient bucket (W1, b1, .. W4, b4) as a dict of tensors."""
    out, off = {}, 0
    for k, s in mlp_shapes(d, pre).items():
        n = math.prod(s)
        out[k] = flat[off:off + n].reshape(s)
        off += n
    assert off == flat.numel()
    return out


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def fwd_inputs(d, pre):
    """x = 1.5 randn, t = rand, z = randn at the case's largest forward batch (float32)."""
    g = _gen(d, pre, "fwd")
    B = fwd_batches(d, pre)[-1]
    return {"x": 1.5 * R.randn(B, d, generator=g), "t": _rand(B, generator=g), "z": R.randn(B, d, generator=g)}


@functools.lru_cache(maxsize=None)
def train_inputs(d, pre):
    """t, y, v of tests/test_kernels_gpu.py::test_mlp_ssm_grad_vs_oracle at B = 8245, and normal u, cst for the general
    form (float32)."""
    g = _gen(d, pre, "train")
    B = TRAIN_BATCHES[-1]
    sp = S.SdeSpec()
    t = S.clamp_time(sp, _rand(B, 1, generator=g))
    y = S.vp_perturb(sp, t, 1.5 * R.randn(B, d, generator=g), R.randn(B, d, generator=g))
    v = S.rademacher_from_uniform(_rand(B, d, generator=g))
    return {"t": t, "y": y, "v": v, "u": R.randn(B, d, generator=g), "cst": R.randn(B, generator=g)}


# ------------------------------------------------------------------------------------------------ references
def forward(p, x, t, pre, dt):
    return N.mlp_forward(cast(p, dt), x.to(dt), t.to(dt), pre)


def em_step(p, x, z, pre, t, lmbd, dt, delta=EM_DELTA):
    """One reverse Euler-Maruyama step of the SGM: the net at T - t, then the stage update with the given z."""
    s = torch.full((x.shape[0],), R.c32(R.T_END) - R.c32(t), dtype=dt)
    a = N.mlp_forward(cast(p, dt), x.to(dt), s, pre)
    return R.stage("sgm", "reverse", False, x, a, t=t, delta=delta, lmbd=lmbd, z=z, base=x, dtype=dt)["out"][0]


def ssm(p, t, y, v, pre, dt):
    """SGM closed form: (mean, per-sample, grads) of oracle.ssm_ref.ssm_mean_and_grads."""
    return LR.ssm_mean_and_grads(S.SdeSpec(), lambda prm, yy, tt: N.mlp_forward(prm, yy, tt, pre), cast(p, dt), t.to(dt),
                                 y.to(dt), v.to(dt))


def ssm_general(p, t, y, v, u, cst, pre, dt):
    """General form: per_b = (J_a v)_b . u_b + cst_b + |a_b|^2 / 2, gradients of its mean."""
    leaf = {k: w.to(dt).clone().requires_grad_(True) for k, w in p.items()}
    tt = t.to(dt).reshape(-1)
    a, ad = torch.func.jvp(lambda yy: N.mlp_forward(leaf, yy, tt, pre), (y.to(dt),), (v.to(dt),))
    per = (ad * u.to(dt)).sum(1) + cst.to(dt) + 0.5 * (a * a).sum(1)
    loss = per.mean()
    gs = torch.autograd.grad(loss, [leaf[k] for k in NAMES])
    return loss.detach(), per.detach(), dict(zip(NAMES, gs))


@functools.lru_cache(maxsize=None)
def fwd_ref(d, pre, dt=torch.float64):
    """Forward at the largest batch; its first B rows are the reference of batch B (rows never interact)."""
    i = fwd_inputs(d, pre)
    return forward(params(d, pre), i["x"], i["t"], pre, dt)


@functools.lru_cache(maxsize=None)
def em_ref(d, pre, t, lmbd, dt=torch.float64):
    i = fwd_inputs(d, pre)
    return em_step(params(d, pre), i["x"], i["z"], pre, t, lmbd, dt)


@functools.lru_cache(maxsize=None)
def train_ref(d, pre, B, general=False, dt=torch.float64):
    i = {k: w[:B] for k, w in train_inputs(d, pre).items()}
    if general:
        return ssm_general(params(d, pre), i["t"], i["y"], i["v"], i["u"], i["cst"], pre, dt)
    return ssm(params(d, pre), i["t"], i["y"], i["v"], pre, dt)


# ------------------------------------------------------------------------------------------------ comparators
def row_errors(y, ref64):
    """err_b = |y_b - ref_b|_2 / max(|ref_b|_2, 0.1 rms_b |ref_b|_2) for a (rows, width) output; a 1-D output is width 1."""
    r = ref64.double()
    r = r.reshape(r.shape[0], -1)
    e = (y.double().reshape(r.shape) - r).norm(dim=1)
    rn = r.norm(dim=1)
    return e / torch.clamp(rn, min=0.1 * float(rn.pow(2).mean().sqrt()))


def row_cmp(y, ref64):
    """(rel-L2 over the tensor, worst row, index of the worst row)."""
    err = row_errors(y, ref64)
    b = int(err.argmax())
    rel = float((y.double().reshape(-1) - ref64.double().reshape(-1)).norm() / max(float(ref64.double().norm()), 1e-300))
    return rel, float(err[b]), b


def rows_metrics(prefix, y, ref64):
    rel, worst, b = row_cmp(y, ref64)
    return {prefix + "_rel": rel, prefix + "_worst": worst, prefix + "_row": b}


def train_metrics(per, grads, per64, g64):
    """Per-sample loss by row; gradients flat, worst tensor (parity_vs_fp64's rule) and worst row of a weight gradient
    (rows of dW1 / dW2 / dW3 are features, rows of dW4 outputs)."""
    m = rows_metrics("loss", per, per64)
    cat = lambda g: torch.cat([g[k].double().reshape(-1) for k in NAMES])
    m["grad_flat"] = float((cat(grads) - cat(g64)).norm() / cat(g64).norm())
    top = max(float(g64[k].norm()) for k in NAMES)
    per_t = {k: float((grads[k].double() - g64[k]).norm()) / max(float(g64[k].norm()), FLOOR_FRAC * top) for k in NAMES}
    m["grad_tensor_name"] = max(per_t, key=per_t.get)
    m["grad_tensor"] = per_t[m["grad_tensor_name"]]
    rows = {k: row_cmp(grads[k], g64[k])[1:] for k in WEIGHTS}
    k = max(rows, key=lambda q: rows[q][0])
    m["grad_wrow"], m["grad_wrow_name"] = rows[k][0], f"{k}[{rows[k][1]}]"
    return m


def smallest_tensor_fraction(g64):
    top = max(float(g64[k].norm()) for k in NAMES)
    return min(float(g64[k].norm()) for k in NAMES) / top


def loss_sum_bound(per64, yard_loss_rel, c_loss_rel):
    """|loss_sum - mean(per64)|: the rows' errors, at most rel-L2 |per64|_2 / sqrt(B) in the mean (Cauchy-Schwarz), plus
    the float32 additions a term passes through — its workgroup's tiles, 16 sample leaders, 16 slabs per group and 16
    groups of k_slab_reduce, one product with 1/B — each at most 2^-24 of the running sum of absolute values."""
    B = per64.numel()
    depth = -(-B // (16 * 256)) + 16 + 16 + 16 + 1
    p = per64.double()
    return c_loss_rel * yard_loss_rel * float(p.norm()) / math.sqrt(B) + depth * R.EPS32 * float(p.abs().mean())


# ------------------------------------------------------------------------------------------------ yardsticks
@functools.lru_cache(maxsize=None)
def yardstick(d, pre, mode, point=None):
    """The float32 evaluation's figures against float64 at the largest batch of (d, pre, mode); mode 'fwd' | 'em' (point =
    (t, lmbd)) | 'ssm' | 'ssm_general'."""
    if mode == "fwd":
        return rows_metrics("fwd", fwd_ref(d, pre, torch.float32), fwd_ref(d, pre))
    if mode == "em":
        return rows_metrics("em", em_ref(d, pre, *point, torch.float32), em_ref(d, pre, *point))
    B, general = TRAIN_BATCHES[-1], mode == "ssm_general"
    _, per32, g32 = train_ref(d, pre, B, general, torch.float32)
    _, per64, g64 = train_ref(d, pre, B, general)
    return train_metrics(per32, g32, per64, g64)


def judge(d, pre, what, got, yard, families, tab=None):
    """Print one line with every family's multiple hip / float32 oracle (the case's class in MEASURED), or nothing when
    ``tab`` gives other constants; return the families outside their constant."""
    c = tab or MEASURED[table(d, pre)]
    if tab is None:
        print(f"MLPROWS {what} [{table(d, pre)}] " + "  ".join(
            f"{f} {got[f] / yard[f]:.3f} ({got[f]:.2e} | {yard[f]:.2e}, bound {c[f]})" for f in families))
    return [(f, got[f], c[f] * yard[f]) for f in families if not got[f] <= c[f] * yard[f]]
