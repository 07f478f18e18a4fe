"""Parity of the parity-class dgrad of the stride-2 3x3 pad-1 convolutions (k_dgrad_s2) against a float64
``conv_transpose2d`` on the CPU, and of the vector-ALU weight gradient of the 3 -> 32 / 32 -> 3 convolutions (k_wgrad3,
through the slot reduction) against float64 autograd.

Bound: the same quantity computed by float32 torch on the CPU lies some rel-L2 distance d32 from float64; the HIP result
may lie at most 2 * d32 away (twice, because the tiled kernel sums in another order than torch does).  Both distances
are printed before the assertion.  Shapes: the smallest that still reach every path — one tile, a 4x4 image inside an
8x16 tile, a 12x12 image with partial tiles in both directions, two output-channel blocks and two 32-channel chunks
(64 -> 64), dual batches of 2 and 6 rows.  Weight gradients: 16x16 (two full tiles) and 24x24 (partial tiles in x, more
tiles than one workgroup takes), bias gradient over the primal half of the batch only."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"

VARIANTS = ("plain", "bias", "samp_bias", "accumulate")
SHAPES = [(32, 32, 16), (64, 64, 8), (32, 32, 24)]          # (Cin, Cout, H = W of the convolution's input)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def cl2(x):   # (N,C,H,W) -> [N][H][W][C]
    return x.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=None)
def _case(Cin, Cout, H, W_, N):
    """Inputs of one case and, per variant, (float64 reference, float32 torch's distance from it)."""
    g = torch.Generator().manual_seed(1000 * Cin + 10 * H + N)
    Ho, Wo = (H - 1) // 2 + 1, (W_ - 1) // 2 + 1
    Wt = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.2
    gy = torch.randn(N, Cout, Ho, Wo, generator=g)
    bias = torch.randn(Cin, generator=g) * 0.5
    sb = torch.randn(N // 2, Cin, generator=g) * 0.5
    base = torch.randn(N, Cin, H, W_, generator=g)
    op_h, op_w = H - (2 * (Ho - 1) + 1), W_ - (2 * (Wo - 1) + 1)      # output_padding that restores H x W

    def ref(dt):
        d = F.conv_transpose2d(gy.to(dt), Wt.to(dt), stride=2, padding=1, output_padding=(op_h, op_w))
        out = {"plain": d}
        b = d.clone(); b[:N // 2] += bias.to(dt)[None, :, None, None]; out["bias"] = b
        s = d.clone(); s[:N // 2] += sb.to(dt)[:, :, None, None]; out["samp_bias"] = s
        out["accumulate"] = base.to(dt) + d
        return out
    r64, r32 = ref(torch.float64), ref(torch.float32)
    return Wt, gy, bias, sb, base, {v: (r64[v], _rel(r32[v], r64[v])) for v in VARIANTS}


def _dgrad(Cin, Cout, H, W_, N, variant):
    """The input cotangent through ops.conv_forward with the transposed-gather geometry ConvOp._dgrad uses."""
    from sdeflow_light_amd import ops
    from sdeflow_light_amd.convnet import ConvOp
    Wt, gy, bias, sb, base, _ = _case(Cin, Cout, H, W_, N)
    op = ConvOp(torch.nn.Parameter(Wt.to(DEV)), None, "conv", (3, 3), 2, 1, [Cin])
    op.pack()
    Ho, Wo = gy.shape[2], gy.shape[3]
    gd = ops.conv_geom(N, Ho, Wo, H, W_, 3, 3, 2, 1, 1, 0)
    out = cl2(base).to(DEV).reshape(-1).clone() if variant == "accumulate" else torch.full((N * H * W_ * Cin,), float("nan"), device=DEV)
    ops.conv_forward(gd, cl2(gy).to(DEV).reshape(-1), Cout, op.Wd[0], Cin, out, CoutP=ops.pad16(Cin),
                     bias=bias.to(DEV) if variant == "bias" else None,
                     samp_bias=sb.to(DEV).reshape(-1) if variant == "samp_bias" else None,
                     n_bias=N // 2, accumulate=variant == "accumulate")
    torch.cuda.synchronize()
    return out.view(N, H, W_, Cin).cpu()


def _check(Cin, Cout, H, W_, N, variants=VARIANTS):
    refs = _case(Cin, Cout, H, W_, N)[5]
    bad = []
    for v in variants:
        got = _dgrad(Cin, Cout, H, W_, N, v)
        again = _dgrad(Cin, Cout, H, W_, N, v)
        r64, d32 = refs[v]
        d = _rel(got, cl2(r64))
        print(f"dgrad_s2 {Cout}->{Cin} {H}x{W_} N={N} {v}: hip vs f64 {d:.3e}  torch f32 vs f64 {d32:.3e}  bound {2 * d32:.3e}")
        assert torch.equal(got, again), f"{v}: two runs differ"
        if not d <= 2 * d32:
            bad.append((v, d, d32))
    assert not bad, bad


@pytest.mark.parametrize("N", [2, 6])
@pytest.mark.parametrize("Cin,Cout,H", SHAPES)
def test_dgrad_s2_parity(Cin, Cout, H, N):
    _check(Cin, Cout, H, H, N)


@pytest.mark.parametrize("Cin,Cout,H,W_", [(32, 32, 15, 15), (48, 48, 16, 16), (32, 48, 16, 16)])
def test_dgrad_s2_fallback(Cin, Cout, H, W_):
    """Just outside the plan (odd size: the cotangent's grid is not 2x gy's; 48 channels on either side): the shape keeps
    the strided gather and still matches."""
    _check(Cin, Cout, H, W_, 2, ("plain", "accumulate"))


def test_dgrad_s2_through_backward():
    """ConvOp.backward reaches the kernel: d(src) of a 32 -> 32 stride-2 convolution, added onto a skip cotangent."""
    from sdeflow_light_amd.convnet import ConvOp
    Cin, Cout, H, N = 32, 32, 24, 2
    Wt, gy, _, _, base, refs = _case(Cin, Cout, H, H, N)
    w = torch.nn.Parameter(Wt.to(DEV)); w.grad = torch.zeros_like(w)
    op = ConvOp(w, None, "conv", (3, 3), 2, 1, [Cin])
    op.pack(); op.zero_grad_images()
    x = torch.randn(N * H * H * Cin, device=DEV)
    d = cl2(base).to(DEV).reshape(-1).clone()
    (dx,) = op.backward(cl2(gy).to(DEV).reshape(-1), [x], N, H, H, n_bias=N // 2, dsrc=[d], dacc=[True])
    r64, d32 = refs["accumulate"]
    dist = _rel(dx.view(N, H, H, Cin).cpu(), cl2(r64))
    print(f"dgrad_s2 through backward: hip vs f64 {dist:.3e}  torch f32 vs f64 {d32:.3e}")
    assert dist <= 2 * d32


# ------------------------------------------------------------------ 3-channel weight gradients
@functools.lru_cache(maxsize=None)
def _wcase(Cin, Cout, H, N):
    g = torch.Generator().manual_seed(77 * Cin + 5 * H + N)
    x = torch.randn(N, Cin, H, H, generator=g)
    gy = torch.randn(N, Cout, H, H, generator=g)
    Wt = torch.randn(Cout, Cin, 3, 3, generator=g) * 0.2

    def ref(dt):
        w = Wt.to(dt).requires_grad_(True)
        (F.conv2d(x.to(dt), w, None, padding=1) * gy.to(dt)).sum().backward()
        return w.grad, gy.to(dt)[:N // 2].sum((0, 2, 3))
    (w64, b64), (w32, b32) = ref(torch.float64), ref(torch.float32)
    return x, gy, Wt, (w64, _rel(w32, w64)), (b64, _rel(b32, b64))


def _wgrad(Cin, Cout, H, N):
    from sdeflow_light_amd.convnet import ConvOp
    x, gy, Wt, _, _ = _wcase(Cin, Cout, H, N)
    w, b = torch.nn.Parameter(Wt.to(DEV)), torch.nn.Parameter(torch.zeros(Cout, device=DEV))
    w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)
    op = ConvOp(w, b, "conv", (3, 3), 1, 1, [Cin])
    op.pack(); op.zero_grad_images()
    op.backward(cl2(gy).to(DEV).reshape(-1), [cl2(x).to(DEV).reshape(-1)], N, H, H, n_bias=N // 2, need=[False])
    op.unpack_grads()
    torch.cuda.synchronize()
    return w.grad.cpu(), b.grad.cpu()


def _wcheck(Cin, Cout, H, N):
    _, _, _, (w64, dw32), (b64, db32) = _wcase(Cin, Cout, H, N)
    gw, gb = _wgrad(Cin, Cout, H, N)
    gw2, gb2 = _wgrad(Cin, Cout, H, N)
    dw, db = _rel(gw, w64), _rel(gb, b64)
    print(f"wgrad3 {Cin}->{Cout} {H}x{H} N={N}: dW hip vs f64 {dw:.3e}  torch f32 vs f64 {dw32:.3e}  bound {2 * dw32:.3e} | "
          f"dbias hip vs f64 {db:.3e}  torch f32 vs f64 {db32:.3e}  bound {2 * db32:.3e}")
    assert torch.equal(gw, gw2) and torch.equal(gb, gb2), "two runs differ"
    assert dw <= 2 * dw32 and db <= 2 * db32, (dw, dw32, db, db32)


@pytest.mark.parametrize("N", [2, 6])
@pytest.mark.parametrize("H", [16, 24])
@pytest.mark.parametrize("Cin,Cout", [(3, 32), (32, 3)])
def test_wgrad3_parity(Cin, Cout, H, N):
    _wcheck(Cin, Cout, H, N)


@pytest.mark.parametrize("Cin,Cout,H", [(1, 32, 16), (32, 1, 16), (3, 48, 16)])
def test_wgrad3_fallback(Cin, Cout, H):
    """Just outside the plan (one channel, 48 channels): the shape keeps its present kernel and still matches."""
    _wcheck(Cin, Cout, H, 2)
