"""The epilogue the Winograd forward kernels share (wino_epilogue: bias, per-sample bias, accumulate, residual, channel
statistics), checked against the same kernel's own plain output.  The pipe-versus-sampler equality of
test_wino_pipe_gpu.py cannot see an epilogue bug: both sides run the same function.  Here every subset of the options is one
fused call that must EQUAL ((Y + add) + out0) + residual composed in torch fp32 in the kernel's order from the plain output
Y — exact in IEEE arithmetic (the library is built with -ffp-contract=off) — and Y itself is held against the direct kernel."""
import functools
import itertools

import pytest
import torch

from conftest import rel_l2
from sdeflow_light_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (N, H, C0, C1, Cout, CoutP, ups), all through k_conv_wino_pipe
PIPE_SHAPES = [
    (3, 16, 16, 0, 32, 32, False),       # one channel group per item: every group crosses an item boundary
    (2, 16, 32, 0, 64, 64, False),       # two output-channel blocks
    (3, 32, 16, 16, 32, 32, False),      # two sources
    (3, 32, 16, 16, 32, 32, True),       # ... and the folded 2x upsample
    (2, 16, 16, 0, 30, 32, False),       # ragged quads: the per-quad path (no statistics: Cout % 4 != 0)
    (130, 32, 16, 0, 32, 32, False),     # 520 tiles: some workgroups walk two items of one group each
]
# the sampler kernels (identity folded transform): k_conv_wino with register weights (Ktot = 32) and LDS weights (Ktot = 64)
SAMPLER_SHAPES = [(3, 32, 32, 0, 32, 32, False), (3, 32, 64, 0, 64, 64, False)]
OPTIONS = ("bias", "samp", "acc", "res")


@functools.lru_cache(maxsize=None)
def _operands(N, H, C0, C1, Cout, CoutP, ups, sampler):
    """The operands of one shape, built as test_winograd_forward_equals_direct_conv builds them (a ConvOp packs the direct and
    the Winograd image of the same weights), the option tensors, and the plain output Y of the kernel under test."""
    from sdeflow_light_amd.convnet import ConvOp
    g = torch.Generator(device=DEV).manual_seed(1000 * N + H + C0 + C1 + Cout + int(ups))
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)   # noqa: E731
    Ctot = C0 + C1
    w = torch.nn.Parameter(rnd(Cout, Ctot, 3, 3) * (2.0 / (9 * Ctot)) ** 0.5)
    op = ConvOp(w, None, "conv", (3, 3), 1, 1, [C0, C1] if C1 else [C0], ups=ups)
    op.pack()
    assert op.wino_capable() and op.CoutP == CoutP
    ops.PackTable(op.wino_jobs(), DEV).run_wino()
    Hi = H // 2 if ups else H
    geom = ops.conv_geom(N, Hi, Hi, H, H, 3, 3, 1, 1, 0, int(ups))
    assert ops.conv_wino_supported(geom, C0, C1, CoutP)
    n_out = N * H * H * Cout
    n_bias, n_samp = (N + 1) // 2, max(1, N // 3)
    assert n_bias < N and n_samp < N
    d = dict(op=op, geom=geom, src0=rnd(N * Hi * Hi * C0), src1=rnd(N * Hi * Hi * C1) if C1 else None, bias=rnd(Cout) * 0.5,
             n_bias=n_bias, samp=rnd(n_samp * Cout) * 0.5, n_samp=n_samp, out0=rnd(n_out), res=rnd(n_out), n_out=n_out,
             S=ops.conv_chanstats_slots(geom, C0, C1, Cout, CoutP, wino=True),
             ident=dict(in_scale=torch.ones(N * Ctot, device=DEV), in_shift=torch.zeros(N * Ctot, device=DEV)) if sampler else {})
    d["Y"], _ = _run(d, N, C0, C1, Cout, CoutP, ())
    assert torch.isfinite(d["Y"]).all()
    return d


def _run(d, N, C0, C1, Cout, CoutP, opts, stats=False, wino=True):
    """One convolution with the options `opts` fused; the output starts NaN-filled (from out0 where it accumulates)."""
    out = d["out0"].clone() if "acc" in opts else torch.full((d["n_out"],), float("nan"), device=DEV)
    cs = torch.full((N * d["S"] * 2 * Cout,), float("nan"), device=DEV) if stats else None
    kw = dict(src1=d["src1"], C1=C1, CoutP=CoutP, wino=wino, accumulate="acc" in opts, chanstats=cs)
    if "bias" in opts:
        kw.update(bias=d["bias"], n_bias=d["n_bias"])
    if "samp" in opts:
        kw.update(samp_bias=d["samp"], n_samp=d["n_samp"])
    if "res" in opts:
        kw.update(residual=d["res"])
    if wino:
        kw.update(d["ident"])
    ops.conv_forward(d["geom"], d["src0"], C0, d["op"].WpW if wino else d["op"].Wp, Cout, out, **kw)
    return out, cs


def _composed(d, N, H, Cout, opts):
    """((Y + add) + out0) + residual in fp32, add = bias (rows n < n_bias) + per-sample bias (rows n < n_samp) as the kernel
    forms it: it starts from zero, a bias row REPLACES it, a per-sample row is added to it."""
    add = torch.zeros(N, Cout, device=DEV)
    if "bias" in opts:
        add[:d["n_bias"]] = d["bias"]
    if "samp" in opts:
        add[:d["n_samp"]] += d["samp"].view(d["n_samp"], Cout)
    v = d["Y"].view(N, H * H, Cout) + add.view(N, 1, Cout)
    if "acc" in opts:
        v = v + d["out0"].view(N, H * H, Cout)
    if "res" in opts:
        v = v + d["res"].view(N, H * H, Cout)
    return v.reshape(-1)


def _check_composition(shape, sampler):
    N, H, C0, C1, Cout, CoutP, ups = shape
    d = _operands(*shape, sampler)
    for k in range(len(OPTIONS) + 1):
        for opts in itertools.combinations(OPTIONS, k):
            want = _composed(d, N, H, Cout, opts)
            for stats in ((False, True) if d["S"] else (False,)):
                got, cs = _run(d, N, C0, C1, Cout, CoutP, opts, stats)
                assert torch.isfinite(got).all(), (opts, stats)
                assert torch.equal(got, want), f"{opts} stats={stats}: max |diff| {float((got - want).abs().max()):.3e}"
                if stats:                               # as test_conv_channel_statistics_byproduct: sums of the FINAL values
                    assert torch.isfinite(cs).all(), opts
                    o = got.view(N, H * H, Cout).double()
                    tot = cs.view(N, d["S"], 2, Cout).double().sum(1)
                    e1, e2 = rel_l2(tot[:, 0].cpu(), o.sum(1).cpu()), rel_l2(tot[:, 1].cpu(), (o * o).sum(1).cpu())
                    assert e1 <= 2e-6 and e2 <= 2e-6, (opts, e1, e2)


@pytest.mark.parametrize("shape", PIPE_SHAPES)
def test_wino_pipe_fused_options_equal_composition(shape):
    _check_composition(shape, sampler=False)


@pytest.mark.parametrize("shape", SAMPLER_SHAPES)
def test_wino_sampler_fused_options_equal_composition(shape):
    _check_composition(shape, sampler=True)


@pytest.mark.parametrize("shape", PIPE_SHAPES)
def test_wino_plain_output_against_direct_kernel(shape):
    """Both are fp32 and differ by the rounding of the Winograd transforms only."""
    N, H, C0, C1, Cout, CoutP, ups = shape
    d = _operands(*shape, False)
    ref, _ = _run(d, N, C0, C1, Cout, CoutP, (), wino=False)
    assert torch.isfinite(ref).all()
    e = rel_l2(d["Y"].cpu(), ref.cpu())
    print(f"Winograd (pipe) vs direct N={N} {H}x{H} {C0}+{C1}->{Cout}/{CoutP} ups={ups}: rel-L2 {e:.2e}")
    assert e <= 2e-6
    assert not torch.equal(d["Y"], ref)                    # it really took the other kernel
