"""The training path's Winograd kernel (k_conv_wino_pipe: every msgm_conv_forward_wino call without a folded input
transform) against the kernels the sampler keeps (k_conv_wino / k_conv_wino_p32, reached through the same entry point with
an identity folded transform: v * 1 + 0 is exact).  Both do the same arithmetic in the same order, so the outputs and the
channel statistics must be EQUAL, not close."""
import pytest
import torch

from sdeflow_light_amd import ops

pytestmark = pytest.mark.gpu


def _both(N, H, C0, C1, Cout, CoutP, ups=False, acc=False, res=False, bias=False, n_bias=None, samp=False, n_samp=None,
          stats=False, seed=0):
    """One convolution through the pipelined kernel and through the folded-transform kernels on the same inputs."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda n: torch.randn(n, device=dev, generator=g)   # noqa: E731
    Hi = H // 2 if ups else H
    geom = ops.conv_geom(N, Hi, Hi, H, H, 3, 3, 1, 1, 0, 1 if ups else 0)
    assert ops.conv_wino_supported(geom, C0, C1, CoutP)
    Ktot = C0 + C1
    Wp = rnd(16 * CoutP * Ktot) * (1.0 / Ktot) ** 0.5
    src0 = rnd(N * Hi * Hi * C0)
    src1 = rnd(N * Hi * Hi * C1) if C1 else None
    out0 = rnd(N * H * H * Cout)
    kw = dict(src1=src1, C1=C1, CoutP=CoutP, wino=True, accumulate=acc)
    if bias:
        kw.update(bias=rnd(Cout), n_bias=N if n_bias is None else n_bias)
    if samp:
        ns = N if n_samp is None else n_samp
        kw.update(samp_bias=rnd(ns * Cout), n_samp=ns)
    if res:
        kw.update(residual=rnd(N * H * H * Cout))
    S = (H // 16) ** 2 * 4
    outs, css = [], []
    for identity in (False, True):
        out = out0.clone()
        cs = torch.full((N * S * 2 * Cout,), float("nan"), device=dev) if stats else None
        extra = dict(in_scale=torch.ones(N * Ktot, device=dev), in_shift=torch.zeros(N * Ktot, device=dev)) if identity else {}
        ops.conv_forward(geom, src0, C0, Wp, Cout, out, chanstats=cs, **kw, **extra)
        outs.append(out)
        css.append(cs)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), f"max |diff| {float((outs[0] - outs[1]).abs().max()):.3e}"
    if stats:
        assert torch.isfinite(css[0]).all()
        assert torch.equal(css[0], css[1])


def _c4_winograd_calls():
    """Every distinct (C0, C1, Cout, CoutP, H, ups, fused options) that one training step of the C4 model (VorticityUNet
    64x64x3, base 32, mults 1-2-4) sends to msgm_conv_forward_wino, recorded from a 2-row step."""
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from sdeflow_light_amd.SDEs import SGMsde, PluginReverseSDE
    from sdeflow_light_amd.train import UNetScoreTrainer
    from sdeflow_light_amd.data import random_images
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = VorticityUNet(base_channels=32, channel_mults=(1, 2, 4), num_res_blocks=2, in_space=64, attention_resolutions=(2, 4),
                        flatten_order="F", channels=3).to(dev)
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    gen = PluginReverseSDE(SGMsde(T=T, num_steps_forward=16, device=dev), net, T, deviceReverseSDE=dev).to(dev)
    tr = UNetScoreTrainer(gen, 2, 3 * 64 * 64, lr=1e-4, use_graph=False)
    tr.set_data(random_images(2, 3, 64, 64, device=dev))
    calls = set()
    real = ops.conv_forward

    def rec(geom, src0, C0, Wp, Cout, out, src1=None, C1=0, **kw):
        if kw.get("wino") and kw.get("in_scale") is None:
            calls.add((C0, C1 if src1 is not None else 0, Cout, kw.get("CoutP") or Cout, geom.Ho, bool(geom.ups),
                       bool(kw.get("accumulate")), kw.get("residual") is not None, kw.get("bias") is not None,
                       kw.get("samp_bias") is not None, kw.get("chanstats") is not None))
        return real(geom, src0, C0, Wp, Cout, out, src1=src1, C1=C1, **kw)

    ops.conv_forward = rec
    try:
        tr.step()
        torch.cuda.synchronize()
    finally:
        ops.conv_forward = real
    return sorted(calls)


def test_wino_pipe_equals_wino_on_every_c4_call():
    calls = _c4_winograd_calls()
    assert len(calls) >= 6, calls
    for i, (C0, C1, Cout, CoutP, H, ups, acc, res, bias, samp, stats) in enumerate(calls):
        for N in (2, 13):                    # 13 rows: tile counts that do not divide over the XCDs / workgroups
            _both(N, H, C0, C1, Cout, CoutP, ups=ups, acc=acc, res=res, bias=bias, n_bias=N // 2, samp=samp, stats=stats,
                  seed=100 * i + N)
    print(f"{len(calls)} distinct Winograd calls of the C4 training step: equal outputs")


@pytest.mark.parametrize("C0,C1,Cout,CoutP", [(32, 0, 32, 32), (32, 0, 64, 64), (32, 0, 96, 96),     # Ktot = 32
                                              (48, 16, 80, 96),                                       # not multiples of 32
                                              (16, 0, 30, 32), (64, 32, 32, 32), (128, 128, 128, 128)])
@pytest.mark.parametrize("ups", [False, True])
def test_wino_pipe_shapes_and_fused_options(C0, C1, Cout, CoutP, ups):
    stats = Cout % 4 == 0
    _both(3, 32, C0, C1, Cout, CoutP, ups=ups, acc=True, res=True, bias=True, n_bias=2, samp=True, n_samp=1, stats=stats,
          seed=C0 + C1 + Cout)
    _both(5, 16, C0, C1, Cout, CoutP, ups=ups, bias=True, n_bias=5, stats=stats, seed=7 + Cout)


@pytest.mark.parametrize("N,H,C0,C1,Cout", [(512, 64, 32, 0, 32), (512, 64, 64, 32, 32), (512, 32, 128, 0, 64),
                                            (512, 16, 128, 128, 128), (260, 32, 64, 0, 64)])
def test_wino_pipe_c4_sizes(N, H, C0, C1, Cout):
    """At the C4 step's row count (256 samples, primal + tangent rows) and one that leaves a ragged last round."""
    _both(N, H, C0, C1, Cout, Cout, bias=True, n_bias=N // 2, res=True, stats=True, seed=N + H)
