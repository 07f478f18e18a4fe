"""The paths of k_conv_wino_pipe that the full-size tests do not separate (tests/test_wino_pipe_gpu.py runs 32x32, which has
no interior tile, and the C4 sizes): its halo fill works out a lane's source offsets when the stream of channel groups
enters an item or changes source, and leaves the zero border to the range check of the buffer loads.

Bitwise: the pipelined kernel against the folded-identity route (the sampler kernels, whose staging is independent; the
method of tests/test_wino_pipe_gpu.py::_both), outputs and channel statistics with torch.equal.  3 rows (a ragged last XCD
round); 16x16 (one tile, all four borders), 48x48 (an interior tile, a workgroup walks items of different border classes)
and the non-square 48x16; single-group items (16 channels), 32 channels, a source switch inside an item (48 + 16) and three
output-channel blocks per tile (96); each with and without the folded 2x upsample and with the option sets plain, bias +
per-sample bias + statistics, bias + residual + statistics, accumulate.

Float64: the packed-weight route (ConvOp, ConvOpSet.pack_wino(train=True)) at 3 rows, 48x48, 32 -> 32 and 48 + 16 -> 64
against torch.nn.functional.conv2d in float64 on the CPU; bound 2x the rel-L2 distance of float32 torch from the same
float64 result (the rule of tests/test_conv_tail_gpu.py); both distances are printed."""
import pytest
import torch
import torch.nn.functional as F

from sdeflow_light_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [(16, 16), (48, 48), (48, 16)]                                           # (H, W) of the output
CHANNELS = [(16, 0, 32, 32), (32, 0, 32, 32), (48, 16, 64, 64), (32, 32, 96, 96)]  # C0, C1 -> Cout / CoutP
OPTIONS = [dict(), dict(bias=True, samp=True, stats=True), dict(bias=True, res=True, stats=True), dict(acc=True)]


def _both(N, H, W, C0, C1, Cout, CoutP, ups, seed, acc=False, res=False, bias=False, samp=False, stats=False):
    """One convolution through the pipelined kernel and through the folded-transform kernels on the same inputs."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda n: torch.randn(n, device=DEV, generator=g)   # noqa: E731
    Hi, Wi = (H // 2, W // 2) if ups else (H, W)
    geom = ops.conv_geom(N, Hi, Wi, H, W, 3, 3, 1, 1, 0, 1 if ups else 0)
    assert ops.conv_wino_supported(geom, C0, C1, CoutP)
    Ktot = C0 + C1
    Wp = rnd(16 * CoutP * Ktot) * (1.0 / Ktot) ** 0.5
    src0 = rnd(N * Hi * Wi * C0)
    src1 = rnd(N * Hi * Wi * C1) if C1 else None
    out0 = rnd(N * H * W * Cout)
    kw = dict(src1=src1, C1=C1, CoutP=CoutP, wino=True, accumulate=acc)
    if bias:
        kw.update(bias=rnd(Cout), n_bias=2)                 # rows with and without the bias
    if samp:
        kw.update(samp_bias=rnd(1 * Cout), n_samp=1)
    if res:
        kw.update(residual=rnd(N * H * W * Cout))
    S = (H // 16) * (W // 16) * 4
    outs, css = [], []
    for identity in (False, True):
        out = out0.clone() if acc else torch.full_like(out0, float("nan"))
        cs = torch.full((N * S * 2 * Cout,), float("nan"), device=DEV) if stats else None
        extra = dict(in_scale=torch.ones(N * Ktot, device=DEV), in_shift=torch.zeros(N * Ktot, device=DEV)) if identity else {}
        ops.conv_forward(geom, src0, C0, Wp, Cout, out, chanstats=cs, **kw, **extra)
        outs.append(out)
        css.append(cs)
    torch.cuda.synchronize()
    what = f"{H}x{W} {C0}+{C1}->{Cout} ups={int(ups)} acc={int(acc)} res={int(res)} bias={int(bias)} samp={int(samp)}"
    assert torch.isfinite(outs[0]).all(), what
    assert torch.equal(outs[0], outs[1]), f"{what}: max |diff| {float((outs[0] - outs[1]).abs().max()):.3e}"
    if stats:
        assert torch.isfinite(css[0]).all(), what
        assert torch.equal(css[0], css[1]), what


@pytest.mark.parametrize("C0,C1,Cout,CoutP", CHANNELS)
@pytest.mark.parametrize("H,W", SIZES)
def test_wino_pipe_paths_equal_folded_identity(H, W, C0, C1, Cout, CoutP):
    for ups in (False, True):
        for k, o in enumerate(OPTIONS):
            _both(3, H, W, C0, C1, Cout, CoutP, ups, seed=1000 * H + 10 * W + C0 + C1 + Cout + 2 * k + int(ups), **o)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("C0,C1,Cout", [(32, 0, 32), (48, 16, 64)])
def test_wino_pipe_packed_route_float64(C0, C1, Cout):
    from sdeflow_light_amd.convnet import ConvOp, ConvOpSet
    N, H = 3, 48
    g = torch.Generator().manual_seed(C0 + Cout)
    Wt = torch.randn(Cout, C0 + C1, 3, 3, generator=g) * (2.0 / (9 * (C0 + C1))) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.5
    x = torch.randn(N, C0 + C1, H, H, generator=g)
    r64 = F.conv2d(x.double(), Wt.double(), b.double(), padding=1)
    d32 = _rel(F.conv2d(x, Wt, b, padding=1), r64)
    op = ConvOp(torch.nn.Parameter(Wt.to(DEV)), torch.nn.Parameter(b.to(DEV)), "conv", (3, 3), 1, 1, [C0] + ([C1] if C1 else []))
    st = ConvOpSet([op])
    st.pack()
    st.pack_wino(train=True)
    assert op.train_wino
    cl = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV).reshape(-1)   # noqa: E731
    srcs = [cl(x[:, :C0])] + ([cl(x[:, C0:])] if C1 else [])
    out, Ho, Wo = op.forward(srcs, N, H, H, n_bias=N)
    torch.cuda.synchronize()
    got = out.view(N, Ho, Wo, Cout).permute(0, 3, 1, 2).cpu()
    d = _rel(got, r64)
    print(f"wino_pipe {C0}+{C1}->{Cout} {H}x{H} N={N}: hip vs f64 {d:.3e}  torch f32 vs f64 {d32:.3e}  bound {2 * d32:.3e}")
    assert d <= 2 * d32, (d, d32)
