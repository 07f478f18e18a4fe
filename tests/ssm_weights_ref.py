"""Per-row weights in the SSM loss: the float64 statement, the case list and the inputs shared by
tests/test_ssm_weights_ref.py (CPU) and tests/test_ssm_weights_gpu.py.

With weights w (B,) and s = inv_batch the kernels promise
    grads = s sum_b w_b dL_b/dtheta,   loss_per[b] = L_b (unweighted),   loss_sum = s sum_b w_b L_b,
and the reference states exactly that on oracle.ssm_ref.ssm_loss_jvp (the per-sample, differentiable loss of any SDE
family) and the float64 MLP of tests/mlp_rows_ref.py.  The yardstick of every float64 comparison is the float32
evaluation of the same statement (conftest.parity_vs_fp64, default slack), never the code under test.
"""
import functools
import math

import torch

from oracle import nets_ref as N, sde_ref as S, ssm_ref as LR
import mlp_rows_ref as M
import sde_stage_ref as R

PRE = M.PRE
# The three training kernels (k_mlp<TRAIN> with eight waves: tiny and narrow carves; k_mlp<TRAIN, WIDE>; k_mlp_xw<TRAIN>),
# each without and with NormalizeLogRadius; all six are cases of mlp_rows_ref.CASES.
CASES = ((4, None), (14, PRE),          # narrow
         (17, None), (30, PRE),         # wide
         (31, None), (128, PRE))        # extra-wide
FORMS = ("sgm", "sparse")               # the fused SGM closed form (u = None) | the general form, u and cst of the sparse MSGM
# Exact properties: mlp_rows_ref.TRAIN_BATCHES' smallest ragged batches (1 and 15 rows of a 16-row tile), its smallest
# batch of more than one workgroup (17) and its smallest where a workgroup walks a second tile, whose weights it fetched
# one tile ahead (4097 = 256 tiles + 1 row, grid cap 256).
EXACT_BATCHES = M.TRAIN_BATCHES[:4]
# float64 parity: the batch at which mlp_rows_ref finds the gradient families of two correct float32 evaluations within
# 1.3x of each other (the error of a 17-row gradient is luck: mlp_rows_ref's table), and which has whole tiles to zero.
PARITY_BATCH = M.TRAIN_BATCHES[3]
SEED_SHAPES = tuple((B, n) for B in (1, 9) for n in (2, 7, 64, 100))    # row-kernel classes GS 2, 8, 64, 64


def spec(form, d):
    return S.SdeSpec() if form == "sgm" else S.SdeSpec(kind=S.MSGM_SPARSE, n=d)


def score(pre):
    return lambda prm, yy, tt: N.mlp_forward(prm, yy, tt, pre)


@functools.lru_cache(maxsize=None)
def weights(B, seed=0):
    """Positive weights in [0.25, 4] (log-uniform), every seventh row and the whole second 16-row tile at exactly 0."""
    g = torch.Generator().manual_seed(977 + seed)
    w = torch.exp2(4.0 * torch.rand(B, generator=g, dtype=torch.float64) - 2.0).float()
    w[3::7] = 0.0
    w[16:32] = 0.0
    return w


def weighted(sp, score_fn, params, t, y, v, w, dt, inv_batch=None, seed_form=False):
    """(inv_batch sum_b w_b L_b, per-sample L (unweighted), d/dparams of the former) in dtype dt; inv_batch defaults to
    1/B.  ``seed_form``: the same gradient as the vector-Jacobian product of L with the cotangent inv_batch * w (what the
    kernels seed), a second evaluation order of the same statement."""
    B = y.shape[0]
    s = 1.0 / B if inv_batch is None else inv_batch
    leaf = {k: p.detach().to(dt).clone().requires_grad_(True) for k, p in params.items()}
    per = LR.ssm_loss_jvp(sp, score_fn, leaf, t.to(dt), y.to(dt), v.to(dt))
    names = list(leaf)
    wd = w.to(dt)
    if seed_form:
        gs = torch.autograd.grad(per, [leaf[k] for k in names], grad_outputs=s * wd, allow_unused=True)
        loss = (wd * per.detach()).sum() * s
    else:
        loss = (wd * per).sum() * s
        gs = torch.autograd.grad(loss, [leaf[k] for k in names], allow_unused=True)
    grads = {k: (g if g is not None else torch.zeros_like(leaf[k])) for k, g in zip(names, gs)}
    return loss.detach(), per.detach(), grads


def mlp_inputs(d, pre, B):
    return {k: x[:B] for k, x in M.train_inputs(d, pre).items()}


@functools.lru_cache(maxsize=None)
def mlp_weighted(d, pre, form, B, dt=torch.float64, seed_form=False):
    i = mlp_inputs(d, pre, B)
    return weighted(spec(form, d), score(pre), M.params(d, pre), i["t"], i["y"], i["v"], weights(B), dt, seed_form=seed_form)


def loss_sum_bound(per64, w, per_rel_bound, inv_batch):
    """|loss_sum - s sum_b w_b L64_b|: the rows' errors, at most |w|_2 |dL|_2 with |dL|_2 <= per_rel_bound |L64|_2
    (Cauchy-Schwarz), plus the float32 operations a term passes through — the product with w_b, its workgroup's tiles, 16
    sample leaders, 16 slabs per group and 16 groups of the slab reduction, the product with s — each at most 2^-24 of the
    running sum of absolute values."""
    B = per64.numel()
    depth = -(-B // (16 * 256)) + 16 + 16 + 16 + 2
    p, wd = per64.double(), w.double()
    return inv_batch * (per_rel_bound * float(wd.norm()) * float(p.norm()) + depth * R.EPS32 * float((wd * p).abs().sum()))
