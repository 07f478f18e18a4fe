"""GroupNorm kernels against float64 where a group's mean is large against its spread, and on constant groups.

Every output of every entry that shares k_gn_fwd_reduce — primal and tangent, the saved statistics, both input cotangents,
dgamma / dbeta, the affine entries' scale / shift — is judged per (sample, group) (gn_moments_ref.Groups): the worst absolute
error against the float64 references of layer_ref must be <= max(3 x the error of fp32 PyTorch on the CPU in the same
group, the census bound of the family (worst element / reference RMS, imported from test_layer_census_gpu) x the group's
reference RMS).  Outputs are pre-filled with NaN and asserted finite first.  Inputs: gn_moments_ref.make_inputs /
make_degenerate (tests/test_gn_moments_ref.py shows that they are fair and what the kernels' arithmetic predicts).
Every judged output prints one GNCOND line (kernel error, yardstick error, floor of its worst group);
profiles/gn_cond/parity_measured.txt is that output of one MI355X run, one line per case.

What "the group's reference RMS" is where the output is not a [sample][pixel][channel] tensor (gn_moments_ref.Groups): the
saved statistics are judged entry by entry against each entry's own magnitude; dgamma / dbeta (sums over all samples)
per group of channels against the RMS of the whole vector, as the census does; shift against the RMS of the output it
offsets where its own is smaller (a one-channel group's beta - mean scale cancels to nothing).
The issue's (32, 32, 2050) at 20 samples has one sub-chunk per workgroup; 32 samples are what reaches two (m = 2), so the
shape runs at both (tests/test_gn_moments_ref.py pins the geometry of every shape).

Measured with the raw-moment reduce of the parent commit (profiles/gn_cond/parity_parent_raw_moments.txt): every case of
the sweep from |mean| / std = 100 on fails, single groups at 10, and the constant groups at c = 10 and c = -300.
"""
import functools

import pytest
import torch

import gn_moments_ref as M
import layer_ref as R
from test_layer_census_gpu import BOUNDS
from sdeflow_light_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD, BWD, PARAM, AFF = (BOUNDS[k][2] for k in ("gn_fwd", "gn_bwd", "gn_param", "gn_affine"))


def _nan(n):
    return torch.full((n,), float("nan"), device=DEV)


def _stack(a, b):
    return torch.cat([a.reshape(-1), b.reshape(-1)]).to(DEV)


def _cot(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g), torch.randn(shape, generator=g)


def _affine_refs(x, gamma, beta, G):
    """(float64 reference, fp32 PyTorch yardstick) of the affine entries: (scale, shift) [n][C] each."""
    n, P, C = x.shape
    _, mean, rstd = torch.native_group_norm(x.permute(0, 2, 1).contiguous(), gamma, beta, n, C, P, G, M.EPS)
    sc = rstd.repeat_interleave(C // G, 1) * gamma
    return R.groupnorm_affine(x.double(), gamma.double(), beta.double(), G), (sc, beta - mean.repeat_interleave(C // G, 1) * sc)


def _judge_affine(g, name, got, x, gamma, beta, G):
    n, _, C = x.shape
    (rs, rh), (ts, th) = _affine_refs(x, gamma, beta, G)
    g.per_channel(name + "scale", got[0].cpu().view(n, C), rs, ts, G, AFF)
    out_rms = (gamma.double() ** 2 + beta.double() ** 2).view(G, C // G).mean(1).sqrt()
    g.per_channel(name + "shift", got[1].cpu().view(n, C), rh, th, G, AFF, at_least=out_rms)


def _run(tag, x, xd, gamma, beta, G, silu, fwd_only=False, affine=True):
    """The plain entries on one input: dual and non-dual forward, saved statistics, backward, one-source affine."""
    B, P, C = x.shape
    half = B * P * C
    g = M.Groups(tag)
    x64, xd64, g64, b64 = x.double(), xd.double(), gamma.double(), beta.double()
    gam, bet = gamma.to(DEV), beta.to(DEV)
    rp, rt = R.gn_dual_forward(x64, xd64, g64, b64, G, silu)
    tp, tt = M.torch_fp32_forward(x, xd, gamma, beta, G, silu)
    assert bool(torch.isfinite(rp).all() and torch.isfinite(rt).all() and torch.isfinite(tp).all() and torch.isfinite(tt).all())
    out1 = _nan(half)
    ops.groupnorm_dual_forward(x.reshape(-1).to(DEV), gam, bet, B, P, C, G, False, silu, out=out1)
    g.tensor("primal1", out1.cpu().view(B, P, C), rp, tp, G, FWD)
    if not fwd_only:
        xs = _stack(x, xd)
        out, stats = _nan(2 * half), _nan(B * G * 4)
        ops.groupnorm_dual_forward(xs, gam, bet, B, P, C, G, True, silu, stats=stats, out=out)
        g.tensor("primal", out[:half].cpu().view(B, P, C), rp, tp, G, FWD)
        g.tensor("tangent", out[half:].cpu().view(B, P, C), rt, tt, G, FWD)
        g.stats(stats.cpu().view(B, G, 4), x64, xd64, G, FWD)
        gp, gt = _cot((B, P, C), C + P)
        ref = R.gn_dual_backward(x64, xd64, g64, b64, G, silu, gp.double(), gt.double())
        yard = M.torch_fp32_backward(x, xd, gamma, beta, G, silu, gp, gt)
        dga, dbe, gx = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), _nan(2 * half)
        ops.groupnorm_dual_backward(xs, gam, bet, stats, _stack(gp, gt), dga, dbe, B, P, C, G, silu, gx=gx)
        g.tensor("dx", gx[:half].cpu().view(B, P, C), ref[0], yard[0], G, BWD)
        g.tensor("dxdot", gx[half:].cpu().view(B, P, C), ref[1], yard[1], G, BWD)
        g.per_channel("dgamma", dga.cpu().view(1, C), ref[2].view(1, C), yard[2].view(1, C), G, PARAM, whole=True)
        g.per_channel("dbeta", dbe.cpu().view(1, C), ref[3].view(1, C), yard[3].view(1, C), G, PARAM, whole=True)
    if affine:
        _judge_affine(g, "", ops.groupnorm_affine(x.reshape(-1).to(DEV), C, gam, bet, B, P, G), x, gamma, beta, G)
    return g, (rp, rt)


def _finish(*groups):
    lines = [ln for g in groups for ln in g.lines]
    print("\n".join("GNCOND " + ln for ln in lines))
    for g in groups:
        g.finish()


# the second 2050-pixel shape (two sub-chunks per workgroup) runs the ends and the middle of the sweep
SWEEP = [(s, c) for s in M.SHAPES for c in M.CONDS if s[3] != 32 or c in ((0.0, 1.0), (100.0, 1.0), (1000.0, 0.1))]


@pytest.mark.parametrize("shape,cond", SWEEP, ids=lambda v: "-".join(f"{t:g}" for t in v))
def test_conditioning_sweep(shape, cond):
    (C, G, P, B, fwd_only), (mean, std) = shape, cond
    x, xd, gamma, beta = M.make_inputs(C, G, P, B, mean, std, seed=C + P)
    assert M.gn_chunks(B, P)[2] <= 32
    gs = [_run(f"C{C} G{G} P{P} B{B} mean {mean:g} std {std:g} silu {int(silu)}", x, xd, gamma, beta, G, silu, fwd_only,
               affine=not silu)[0] for silu in (False, True)]
    _finish(*gs)


@pytest.mark.parametrize("c", [0.0, 10.0, -300.0])
@pytest.mark.parametrize("C,G,P", [(6, 6, 49), (6, 3, 64), (96, 32, 81), (192, 32, 16)])
def test_degenerate_groups(C, G, P, c):
    """One exactly constant group and one group of per-channel constants inside random data: the float64 reference, which
    for the constant group is primal = act(beta), tangent = gamma eps^-1/2 (xdot - mean xdot)."""
    B, cpg = 3, C // G
    x, xd, gamma, beta = M.make_degenerate(C, G, P, B, c, seed=C + P)
    gs = []
    for silu in (False, True):
        g, (rp, rt) = _run(f"C{C} G{G} P{P} B{B} constant group c {c:g} silu {int(silu)}", x, xd, gamma, beta, G, silu,
                           affine=not silu)
        gs.append(g)
        if not silu:                                        # the reference itself, against the closed form
            d = xd[1, :, :cpg].double()
            assert torch.allclose(rp[1, :, :cpg], beta[:cpg].double().expand(P, cpg), rtol=0, atol=1e-12)
            assert torch.allclose(rt[1, :, :cpg], gamma[:cpg].double() * (d - d.mean()) / (M.EPS ** 0.5), rtol=1e-9, atol=0)
    _finish(*gs)


@functools.lru_cache(maxsize=None)
def _entry_case(ill):
    """(96, 32, 81), B = 3: one well-conditioned case and one at |mean| / std = 100, shared by the entry tests."""
    return M.make_inputs(96, 32, 81, 3, 100.0 if ill else 0.3, 1.0, seed=7 + ill)


ENTRY = dict(C=96, G=32, P=81, B=3)


@pytest.mark.parametrize("ill", [0, 1])
def test_backward_residuals_and_deferred_reduces(ill):
    """residual in the plain backward; residual + residual2 inside a DeferredReduces pass (the slots form)."""
    C, G, P, B = (ENTRY[k] for k in "CGPB")
    x, xd, gamma, beta = _entry_case(ill)
    half, silu = B * P * C, True
    gam, bet, xs = gamma.to(DEV), beta.to(DEV), _stack(x, xd)
    stats = _nan(B * G * 4)
    ops.groupnorm_dual_forward(xs, gam, bet, B, P, C, G, True, silu, stats=stats)
    gp, gt = _cot((B, P, C), 11)
    (r1p, r1t), (r2p, r2t) = _cot((B, P, C), 12), _cot((B, P, C), 13)
    ref = R.gn_dual_backward(x.double(), xd.double(), gamma.double(), beta.double(), G, silu, gp.double(), gt.double())
    yard = M.torch_fp32_backward(x, xd, gamma, beta, G, silu, gp, gt)
    gs = []
    for deferred in (False, True):
        g = M.Groups(f"C{C} G{G} P{P} B{B} ill {ill} backward residual{'s, deferred' if deferred else ''}")
        dga, dbe, gx = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), _nan(2 * half)
        if deferred:
            with ops.DeferredReduces.on(DEV):
                ops.groupnorm_dual_backward(xs, gam, bet, stats, _stack(gp, gt), dga, dbe, B, P, C, G, silu, gx=gx,
                                            residual=_stack(r1p, r1t), residual2=_stack(r2p, r2t))
        else:
            ops.groupnorm_dual_backward(xs, gam, bet, stats, _stack(gp, gt), dga, dbe, B, P, C, G, silu, gx=gx,
                                        residual=_stack(r1p, r1t))
        ap, at = (r1p + r2p, r1t + r2t) if deferred else (r1p, r1t)
        g.tensor("dx", gx[:half].cpu().view(B, P, C), ref[0] + ap.double(), yard[0] + ap, G, BWD)
        g.tensor("dxdot", gx[half:].cpu().view(B, P, C), ref[1] + at.double(), yard[1] + at, G, BWD)
        g.per_channel("dgamma", dga.cpu().view(1, C), ref[2].view(1, C), yard[2].view(1, C), G, PARAM, whole=True)
        g.per_channel("dbeta", dbe.cpu().view(1, C), ref[3].view(1, C), yard[3].view(1, C), G, PARAM, whole=True)
        gs.append(g)
    _finish(*gs)


@pytest.mark.parametrize("ill", [0, 1])
def test_two_source_entries(ill):
    """groupnorm_dual_forward2 / _backward2 and the two-source affine: the concatenation split at C0 = 32 of 96 (group 10
    straddles the sources), another mean in each source."""
    C, G, P, B = (ENTRY[k] for k in "CGPB")
    C0, C1, silu = 32, 64, True
    x, xd, gamma, beta = M.make_inputs(C, G, P, B, 0.0, 1.0, seed=21 + ill, src_means=(C0, 100.0, 30.0) if ill else (C0, 0.5, 2.0))
    assert M.fair(x, G)
    half = B * P * C
    gam, bet = gamma.to(DEV), beta.to(DEV)
    x0, x1 = _stack(x[..., :C0].contiguous(), xd[..., :C0].contiguous()), _stack(x[..., C0:].contiguous(), xd[..., C0:].contiguous())
    x64, xd64, g64, b64 = x.double(), xd.double(), gamma.double(), beta.double()
    g = M.Groups(f"C{C0}+{C1} G{G} P{P} B{B} ill {ill} two sources")
    stats = _nan(B * G * 4)
    out = ops.groupnorm_dual_forward2(x0, C0, x1, C1, gam, bet, B, P, G, True, silu, stats=stats)
    rp, rt = R.gn_dual_forward(x64, xd64, g64, b64, G, silu)
    tp, tt = M.torch_fp32_forward(x, xd, gamma, beta, G, silu)
    g.tensor("primal", out[:half].cpu().view(B, P, C), rp, tp, G, FWD)
    g.tensor("tangent", out[half:].cpu().view(B, P, C), rt, tt, G, FWD)
    g.stats(stats.cpu().view(B, G, 4), x64, xd64, G, FWD)
    gp, gt = _cot((B, P, C), 22)
    ref = R.gn_dual_backward(x64, xd64, g64, b64, G, silu, gp.double(), gt.double())
    yard = M.torch_fp32_backward(x, xd, gamma, beta, G, silu, gp, gt)
    dga, dbe = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    gx0, gx1 = ops.groupnorm_dual_backward2(x0, C0, x1, C1, gam, bet, stats, _stack(gp, gt), dga, dbe, B, P, G, silu)
    h0, h1 = B * P * C0, B * P * C1
    dx = torch.cat([gx0[:h0].cpu().view(B, P, C0), gx1[:h1].cpu().view(B, P, C1)], -1)
    dxd = torch.cat([gx0[h0:].cpu().view(B, P, C0), gx1[h1:].cpu().view(B, P, C1)], -1)
    g.tensor("dx", dx, ref[0], yard[0], G, BWD)
    g.tensor("dxdot", dxd, ref[1], yard[1], G, BWD)
    g.per_channel("dgamma", dga.cpu().view(1, C), ref[2].view(1, C), yard[2].view(1, C), G, PARAM, whole=True)
    g.per_channel("dbeta", dbe.cpu().view(1, C), ref[3].view(1, C), yard[3].view(1, C), G, PARAM, whole=True)
    aff = ops.groupnorm_affine(x[..., :C0].reshape(-1).to(DEV), C0, gam, bet, B, P, G, x1=x[..., C0:].reshape(-1).to(DEV), C1=C1)
    _judge_affine(g, "2src.", aff, x, gamma, beta, G)
    _finish(g)


@pytest.mark.parametrize("ill", [0, 1])
def test_dropout_entries(ill):
    """The dropout builds at p = 0.3: the references multiplied by the keep mask of ops.dropout_mask times the scale."""
    from sdeflow_light_amd import _lib as L
    C, G, P, B = (ENTRY[k] for k in "CGPB")
    x, xd, gamma, beta = _entry_case(ill)
    half, silu, p = B * P * C, True, 0.3
    rng = L.PhiloxState(41 + ill, DEV, offset=2, row_base=4, n=4)
    desc = ops.dropout_desc(rng, 3, p)
    keep = ops.dropout_mask(desc, B, P, C, DEV).cpu().view(B, P, C)
    assert 0.5 < float(keep.mean()) < 0.9 and bool(((keep == 0) | (keep == 1)).all())
    m = keep * torch.tensor(ops.dropout_threshold(p)[1], dtype=torch.float32)            # keep * fp32(scale)
    gam, bet, xs = gamma.to(DEV), beta.to(DEV), _stack(x, xd)
    x64, xd64, g64, b64 = x.double(), xd.double(), gamma.double(), beta.double()
    g = M.Groups(f"C{C} G{G} P{P} B{B} ill {ill} dropout p {p}")
    out, stats = _nan(2 * half), _nan(B * G * 4)
    ops.groupnorm_dual_forward(xs, gam, bet, B, P, C, G, True, silu, stats=stats, out=out, dropout=desc)
    rp, rt = R.gn_dual_forward(x64, xd64, g64, b64, G, silu)
    tp, tt = M.torch_fp32_forward(x, xd, gamma, beta, G, silu)
    g.tensor("primal", out[:half].cpu().view(B, P, C), rp * m.double(), tp * m, G, FWD)
    g.tensor("tangent", out[half:].cpu().view(B, P, C), rt * m.double(), tt * m, G, FWD)
    g.stats(stats.cpu().view(B, G, 4), x64, xd64, G, FWD)
    gp, gt = _cot((B, P, C), 31)
    # the mask follows the activation, so the masked layer's cotangents are the plain layer's at the masked output cotangents
    ref = R.gn_dual_backward(x64, xd64, g64, b64, G, silu, gp.double() * m.double(), gt.double() * m.double())
    yard = M.torch_fp32_backward(x, xd, gamma, beta, G, silu, gp, gt, mask=m)
    dga, dbe, gx = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), _nan(2 * half)
    ops.groupnorm_dual_backward(xs, gam, bet, stats, _stack(gp, gt), dga, dbe, B, P, C, G, silu, gx=gx, dropout=desc)
    g.tensor("dx", gx[:half].cpu().view(B, P, C), ref[0], yard[0], G, BWD)
    g.tensor("dxdot", gx[half:].cpu().view(B, P, C), ref[1], yard[1], G, BWD)
    g.per_channel("dgamma", dga.cpu().view(1, C), ref[2].view(1, C), yard[2].view(1, C), G, PARAM, whole=True)
    g.per_channel("dbeta", dbe.cpu().view(1, C), ref[3].view(1, C), yard[3].view(1, C), G, PARAM, whole=True)
    _finish(g)


# ------------------------------------------------------------------------------------------------ the sampler's folded route
def _chanstats_affine(mean, std):
    """An identity 1x1 convolution (64 channels, 256 pixels) leaves the channel sums of its output behind; (scale, shift) from
    them, judged against float64 on the convolution's own fp32 output."""
    from sdeflow_light_amd.convnet import ConvOp
    C, G, P, B = 64, 32, 256, 3
    x, _, gamma, beta = M.make_inputs(C, G, P, B, mean, std, seed=51)
    w = torch.nn.Parameter(torch.eye(C).reshape(C, C, 1).to(DEV))
    w.grad = torch.zeros_like(w)
    op = ConvOp(w, None, "conv", (1,), 1, 0, [C], 0, False)
    op.pack()
    op.zero_grad_images()
    out, _, _ = op.forward([x.reshape(-1).to(DEV)], B, 1, P, n_bias=B, stats=True)
    cs, S = out._msgm_cs
    y = out.cpu().view(B, P, C)
    assert M.fair(y, G)
    got = ops.groupnorm_affine_cs(cs, S, C, gamma.to(DEV), beta.to(DEV), B, P, G)
    g = M.Groups(f"chanstats route C{C} G{G} P{P} B{B} S{S} mean {mean:g} std {std:g}")
    _judge_affine(g, "cs.", got, y, gamma, beta, G)
    return g


@pytest.mark.parametrize("mean,std", [(0.0, 1.0), (3.0, 1.0)])
def test_chanstats_route_holds_at_small_means(mean, std):
    _finish(_chanstats_affine(mean, std))


def test_chanstats_route_known_limit_is_measured():
    """groupnorm_affine_cs reads raw fp32 channel sums written by the convolution epilogues, where no pivot is available:
    beyond |mean| / std = 3 its error is measured (profiles/gn_cond/parity_measured.txt), not asserted."""
    for mean, std in ((10.0, 1.0), (100.0, 1.0), (100.0, 0.1)):
        g = _chanstats_affine(mean, std)
        print("\n".join("GNCOND (not asserted) " + ln for ln in g.lines))
