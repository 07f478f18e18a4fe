"""The GroupNorm kernels at 256 < C <= 1024 (the VEC builds; scalar builds keep C <= 256) against float64, under the
per-(sample, group) criterion of tests/test_groupnorm_cond_gpu.py, whose helpers and entry tests run here at the wide
shapes: the worst error of every output in a (sample, group) <= max(3 x fp32 PyTorch's in that group, census bound x the
group's reference RMS).  Outputs are pre-filled with NaN.  Shapes, conditionings and splits: tests/test_gn_wide_ref.py,
which pins their lane geometry (three / two / one pixel lanes, dead threads, more than one sub-chunk) and shows on the CPU
that the kernels' arithmetic meets the criterion.  Every judged output prints one GNCOND line.

Before the kernels took more than 256 channels every case of this file raised MsgmError("... unsupported").

groupnorm_affine_cs reads raw fp32 channel sums (no pivot): as in test_groupnorm_cond_gpu, it is asserted at the
well-conditioned end and its error at |mean| / std = 100 is printed, not asserted (the known limit)."""
import pytest
import torch

import gn_moments_ref as M
import layer_ref as R
import test_groupnorm_cond_gpu as K
from test_gn_wide_ref import WIDE_CONDS, WIDE_SHAPES, WIDE_SPLITS
from sdeflow_light_amd import ops
from sdeflow_light_amd._lib import MsgmError

pytestmark = pytest.mark.gpu
DEV = K.DEV
_ids = lambda v: "-".join(f"{t:g}" for t in v)      # noqa: E731


@pytest.mark.parametrize("cond", WIDE_CONDS, ids=_ids)
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=_ids)
def test_wide_plain_entries(shape, cond):
    """Dual and non-dual forward with and without SiLU, the saved statistics, the backward, the one-source affine."""
    (C, G, P, B), (mean, std) = shape, cond
    x, xd, gamma, beta = M.make_inputs(C, G, P, B, mean, std, seed=C + P)
    assert M.fair(x, G) and M.gn_chunks(B, P)[2] <= 32
    K._finish(*[K._run(f"C{C} G{G} P{P} B{B} mean {mean:g} std {std:g} silu {int(silu)}", x, xd, gamma, beta, G, silu,
                       affine=not silu)[0] for silu in (False, True)])


@pytest.fixture
def wide_entry(monkeypatch):
    """Points test_groupnorm_cond_gpu's entry tests (ENTRY, _entry_case) at a wide shape; ill picks the conditioning."""
    def use(shape):
        C, G, P, B = shape
        monkeypatch.setattr(K, "ENTRY", dict(C=C, G=G, P=P, B=B))
        monkeypatch.setattr(K, "_entry_case", lambda ill: M.make_inputs(C, G, P, B, *WIDE_CONDS[ill], seed=7 + ill + C))
    return use


@pytest.mark.parametrize("ill", [0, 1])
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=_ids)
def test_wide_backward_residuals_and_deferred_reduces(wide_entry, shape, ill):
    wide_entry(shape)
    K.test_backward_residuals_and_deferred_reduces(ill)


@pytest.mark.parametrize("ill", [0, 1])
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=_ids)
def test_wide_dropout_entries(wide_entry, shape, ill):
    wide_entry(shape)
    K.test_dropout_entries(ill)


def _two_source(C0, C1, ill, P=9, B=3, G=32):
    """Inputs of a C0 + C1 concatenation (another mean in each source) and their device halves, primal | tangent stacked."""
    C = C0 + C1
    x, xd, gamma, beta = M.make_inputs(C, G, P, B, 0.0, 1.0, seed=21 + ill + C0, src_means=(C0, 100.0, 30.0) if ill else (C0, 0.5, 2.0))
    assert M.fair(x, G)
    x0 = K._stack(x[..., :C0].contiguous(), xd[..., :C0].contiguous())
    x1 = K._stack(x[..., C0:].contiguous(), xd[..., C0:].contiguous())
    return (x, xd, gamma, beta), (x0, x1), (C, G, P, B)


@pytest.mark.parametrize("ill", [0, 1])
@pytest.mark.parametrize("split", WIDE_SPLITS, ids=lambda s: f"{s[0]}+{s[1]}")
def test_wide_two_source_entries(split, ill):
    """groupnorm_dual_forward2 / _backward2 (plain and inside a DeferredReduces pass) and the two-source affine on the decoder
    concatenations."""
    C0, C1 = split
    (x, xd, gamma, beta), (x0, x1), (C, G, P, B) = _two_source(C0, C1, ill)
    half, silu = B * P * C, True
    gam, bet = gamma.to(DEV), beta.to(DEV)
    x64, xd64, g64, b64 = x.double(), xd.double(), gamma.double(), beta.double()
    g = M.Groups(f"C{C0}+{C1} G{G} P{P} B{B} ill {ill} two sources")
    stats = K._nan(B * G * 4)
    out = ops.groupnorm_dual_forward2(x0, C0, x1, C1, gam, bet, B, P, G, True, silu, stats=stats)
    rp, rt = R.gn_dual_forward(x64, xd64, g64, b64, G, silu)
    tp, tt = M.torch_fp32_forward(x, xd, gamma, beta, G, silu)
    g.tensor("primal", out[:half].cpu().view(B, P, C), rp, tp, G, K.FWD)
    g.tensor("tangent", out[half:].cpu().view(B, P, C), rt, tt, G, K.FWD)
    g.stats(stats.cpu().view(B, G, 4), x64, xd64, G, K.FWD)
    gp, gt = K._cot((B, P, C), 22)
    ref = R.gn_dual_backward(x64, xd64, g64, b64, G, silu, gp.double(), gt.double())
    yard = M.torch_fp32_backward(x, xd, gamma, beta, G, silu, gp, gt)
    h0, h1 = B * P * C0, B * P * C1
    for deferred in (False, True):
        dga, dbe = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        if deferred:
            with ops.DeferredReduces.on(DEV):
                gx0, gx1 = ops.groupnorm_dual_backward2(x0, C0, x1, C1, gam, bet, stats, K._stack(gp, gt), dga, dbe, B, P, G, silu)
        else:
            gx0, gx1 = ops.groupnorm_dual_backward2(x0, C0, x1, C1, gam, bet, stats, K._stack(gp, gt), dga, dbe, B, P, G, silu)
        nm = ".d" if deferred else ""
        dx = torch.cat([gx0[:h0].cpu().view(B, P, C0), gx1[:h1].cpu().view(B, P, C1)], -1)
        dxd = torch.cat([gx0[h0:].cpu().view(B, P, C0), gx1[h1:].cpu().view(B, P, C1)], -1)
        g.tensor("dx" + nm, dx, ref[0], yard[0], G, K.BWD)
        g.tensor("dxdot" + nm, dxd, ref[1], yard[1], G, K.BWD)
        g.per_channel("dgamma" + nm, dga.cpu().view(1, C), ref[2].view(1, C), yard[2].view(1, C), G, K.PARAM, whole=True)
        g.per_channel("dbeta" + nm, dbe.cpu().view(1, C), ref[3].view(1, C), yard[3].view(1, C), G, K.PARAM, whole=True)
    aff = ops.groupnorm_affine(x[..., :C0].reshape(-1).to(DEV), C0, gam, bet, B, P, G, x1=x[..., C0:].reshape(-1).to(DEV), C1=C1)
    K._judge_affine(g, "2src.", aff, x, gamma, beta, G)
    K._finish(g)


def _chanstats(x, S):
    """cs [n][S][{sum, sum of squares}][C] as a producing convolution leaves them: fp32 sums over the pixels p = s mod S."""
    n, P, C = x.shape
    cs = torch.zeros(n, S, 2, C)
    for s in range(S):
        part = x[:, s::S]
        cs[:, s, 0], cs[:, s, 1] = part.sum(1), (part * part).sum(1)
    return cs.reshape(-1).to(DEV)


def _wide_cs(C0, C1, P, B, cond, S0=3, S1=2, G=32):
    C = C0 + C1
    x, _, gamma, beta = M.make_inputs(C, G, P, B, *cond, seed=51 + C0)
    cs0 = _chanstats(x[..., :C0].contiguous(), S0)
    cs1 = _chanstats(x[..., C0:].contiguous(), S1) if C1 else None
    got = ops.groupnorm_affine_cs(cs0, S0, C0, gamma.to(DEV), beta.to(DEV), B, P, G, cs1=cs1, S1=S1 if C1 else 0, C1=C1)
    g = M.Groups(f"chanstats route C{C0}+{C1} G{G} P{P} B{B} S{S0}|{S1 if C1 else 0} mean {cond[0]:g} std {cond[1]:g}")
    K._judge_affine(g, "cs.", got, x, gamma, beta, G)
    return g


CS_CASES = [(C, 0, P, B) for C, _, P, B in WIDE_SHAPES[:5]] + [(C0, C1, 9, 3) for C0, C1 in WIDE_SPLITS]


@pytest.mark.parametrize("case", CS_CASES, ids=_ids)
def test_wide_chanstats_route(case):
    """groupnorm_affine_cs (one thread per channel became a loop over channels) on one and on two sources."""
    K._finish(_wide_cs(*case, WIDE_CONDS[0]))
    g = _wide_cs(*case, WIDE_CONDS[1])
    print("\n".join("GNCOND (not asserted) " + ln for ln in g.lines))


def _all_outputs(shape):
    """Every entry once on one input; returns all outputs (for the bitwise comparison of two runs)."""
    C, G, P, B = shape
    x, xd, gamma, beta = M.make_inputs(C, G, P, B, 0.0, 1.0, seed=C + P)
    gam, bet, xs = gamma.to(DEV), beta.to(DEV), K._stack(x, xd)
    half = B * P * C
    out, stats = K._nan(2 * half), K._nan(B * G * 4)
    ops.groupnorm_dual_forward(xs, gam, bet, B, P, C, G, True, True, stats=stats, out=out)
    gp, gt = K._cot((B, P, C), 5)
    res = []
    for deferred in (False, True):
        dga, dbe, gx = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), K._nan(2 * half)
        if deferred:
            with ops.DeferredReduces.on(DEV):
                ops.groupnorm_dual_backward(xs, gam, bet, stats, K._stack(gp, gt), dga, dbe, B, P, C, G, True, gx=gx)
        else:
            ops.groupnorm_dual_backward(xs, gam, bet, stats, K._stack(gp, gt), dga, dbe, B, P, C, G, True, gx=gx)
        res += [dga, dbe, gx]
    C0 = C // 2 if (C // 2) % 4 == 0 else 128
    x0, x1 = x[..., :C0].reshape(-1).to(DEV), x[..., C0:].reshape(-1).to(DEV)
    res += list(ops.groupnorm_affine(x.reshape(-1).to(DEV), C, gam, bet, B, P, G))
    res += list(ops.groupnorm_affine(x0, C0, gam, bet, B, P, G, x1=x1, C1=C - C0))
    res += list(ops.groupnorm_affine_cs(_chanstats(x, 3), 3, C, gam, bet, B, P, G))
    torch.cuda.synchronize()
    return [out, stats] + res


@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=_ids)
def test_two_runs_are_bitwise_equal(shape):
    a, b = _all_outputs(shape), _all_outputs(shape)
    for i, (u, v) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v), f"output {i} differs between two runs"


# ------------------------------------------------------------------------------------------------ refusals
def _refused(fn, *outs):
    """fn raises MsgmError (an argument check that returns before any launch) and the NaN-filled outputs stay NaN."""
    with pytest.raises(MsgmError, match="unsupported"):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o).all())


@pytest.mark.parametrize("C,G", [(1028, 4), (258, 6)], ids=["1028-above-the-limit", "258-scalar-build-above-256"])
def test_too_wide_is_refused(C, G):
    P, B = 5, 2
    half = B * P * C
    gam, bet = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    xs = torch.randn(2 * half, device=DEV)
    out, stats, gx = K._nan(2 * half), K._nan(B * G * 4), K._nan(2 * half)
    dga, dbe = K._nan(C), K._nan(C)
    st = torch.ones(B * G * 4, device=DEV)
    _refused(lambda: ops.groupnorm_dual_forward(xs, gam, bet, B, P, C, G, True, True, stats=stats, out=out), out, stats)
    _refused(lambda: ops.groupnorm_dual_forward(xs[:half], gam, bet, B, P, C, G, False, False, out=out), out)
    _refused(lambda: ops.groupnorm_dual_backward(xs, gam, bet, st, xs.clone(), dga, dbe, B, P, C, G, True, gx=gx), gx, dga, dbe)
    with ops.DeferredReduces.on(DEV):
        _refused(lambda: ops.groupnorm_dual_backward(xs, gam, bet, st, xs.clone(), dga, dbe, B, P, C, G, True, gx=gx), gx, dga, dbe)
    _refused(lambda: ops.groupnorm_affine(xs[:half], C, gam, bet, B, P, G))
    _refused(lambda: ops.groupnorm_affine_cs(torch.ones(B * 2 * 2 * C, device=DEV), 2, C, gam, bet, B, P, G))


def test_unaligned_wide_split_is_refused():
    """510 + 2: a channel vector would straddle the sources."""
    C0, C1, G, P, B = 510, 2, 32, 5, 2
    C = C0 + C1
    gam, bet = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    x0, x1 = torch.randn(2 * B * P * C0, device=DEV), torch.randn(2 * B * P * C1, device=DEV)
    stats, dga, dbe = K._nan(B * G * 4), K._nan(C), K._nan(C)
    st = torch.ones(B * G * 4, device=DEV)
    _refused(lambda: ops.groupnorm_dual_forward2(x0, C0, x1, C1, gam, bet, B, P, G, True, True, stats=stats), stats)
    _refused(lambda: ops.groupnorm_dual_backward2(x0, C0, x1, C1, gam, bet, st, torch.randn(2 * B * P * C, device=DEV), dga, dbe,
                                                  B, P, G, True), dga, dbe)
    _refused(lambda: ops.groupnorm_affine(x0[:B * P * C0], C0, gam, bet, B, P, G, x1=x1[:B * P * C1], C1=C1))
