"""Winograd F(3x3, 2x2) weight gradient of the 3x3 stride-1 "same" convolutions (k_wgrad_wino).

CPU: the transform matrices reproduce the 3x3 correlation of a 4x4 patch with a 2x2 cotangent block in float64.
GPU: ops.conv_wgrad(..., wino=True) against the float64 reference of tests/layer_ref.py with the census bounds of the
conv_wgrad family (tests/test_layer_census_gpu.py): channel counts 32 / 64 / 128, a second source at a K offset (the
decoder's concatenation), the folded 2x upsample, sample counts and image sizes whose tiles do not divide the workgroup
plan, the bias gradient over the primal rows only, per-call and deferred (DeferredReduces) slot reductions; two runs give
the same bits; a ConvOp whose geometry ops.conv_wino_supported refuses goes back to the direct kernel; wino = 1 is a
preference: on shapes the plan declines the raw ABI runs what wino = 0 runs."""
import numpy as np
import pytest
import torch

import layer_ref as R

DEV = "cuda"

# F(3x3, 2x2): dW = A^T [(G g G^T) .* (B^T d B)] A, the matrices k_wgrad_wino applies (conv_kernels.hip)
AT = np.array([[1, 1, 1, 0], [0, 1, -1, 0], [0, 1, 1, 1]], dtype=np.float64)
G = np.array([[1, 0], [0.5, 0.5], [0.5, -0.5], [0, 1]], dtype=np.float64)
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]], dtype=np.float64)

# conv_wgrad bounds of the census (rel-L2, worst row, worst element / RMS) and its conv_bias bounds
WGRAD_BOUNDS = (5.7e-6, 6.0e-6, 2.7e-5)
BIAS_BOUNDS = (2.6e-6, 2.6e-6, 6.6e-6)


def test_transform_matrices_reproduce_the_correlation():
    rng = np.random.default_rng(0)
    for _ in range(100):
        g = rng.standard_normal((2, 2))
        d = rng.standard_normal((4, 4))
        want = np.array([[sum(g[a, b] * d[a + kh, b + kw] for a in range(2) for b in range(2)) for kw in range(3)]
                         for kh in range(3)])
        got = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)
    # linear in the blocks: the sum over blocks goes into the 16 products before A^T . A (one accumulator per position)
    gs, ds = rng.standard_normal((7, 2, 2)), rng.standard_normal((7, 4, 4))
    M = sum((G @ g @ G.T) * (BT @ d @ BT.T) for g, d in zip(gs, ds))
    want = sum(np.array([[(g * d[kh:kh + 2, kw:kw + 2]).sum() for kw in range(3)] for kh in range(3)]) for g, d in zip(gs, ds))
    np.testing.assert_allclose(AT @ M @ AT.T, want, rtol=0, atol=1e-12)
    # every factor is 0, +-1 or +-1/2: exact in fp32
    for m in (AT, G, BT):
        assert set(np.unique(m)) <= {-1.0, -0.5, 0.0, 0.5, 1.0}


def metrics(y, r):
    """(rel-L2, worst per-row rel-L2 with the census' 0.1 x RMS-row floor, worst element / RMS); a row = an output channel."""
    y, r = y.double().reshape(r.shape[0], -1), r.double().reshape(r.shape[0], -1)
    assert bool(torch.isfinite(y).all())
    d = y - r
    de, rn = (d * d).sum(1), (r * r).sum(1)
    rms = float((r * r).mean().sqrt())
    floor = 0.1 * float(rn.mean().sqrt())
    return (float(de.sum().sqrt() / rn.sum().sqrt()), float((de.sqrt() / rn.sqrt().clamp_min(floor)).max()),
            float(d.abs().max()) / rms)


def within(m, bounds):
    return all(a <= b for a, b in zip(m, bounds))


def _wgrad_all(geom, gy, xs, srcC, Cout, CoutP, Ktot, base, db0, nb, wino, deferred):
    """One call per source (the second at K offset C0), the bias gradient with the first, as ConvOp.backward calls them."""
    from sdeflow_light_amd import ops
    dWp, db = base.clone(), db0.clone()

    def calls():
        koff = 0
        for s, (x, C) in enumerate(zip(xs, srcC)):
            ops.conv_wgrad(geom, gy, x, C, koff, dWp, Cout, CoutP, Ktot, dbias=db if s == 0 else None, n_bias=nb, wino=wino)
            koff += C
    if deferred:
        with ops.DeferredReduces.on(DEV):
            calls()
    else:
        calls()
    torch.cuda.synchronize()
    return dWp, db


# (N, n_bias, H, W of the output, ups, source channels, Cout): C, Cout in {32, 64, 128}; the decoder's concatenations (two
# sources, the second at K offset C0); folded upsample (input H/2 x W/2); 13 samples (tiles that do not divide the plan's
# tiles per workgroup); images whose 8 x 16 tiles are partial (24 x 40, 12 x 20) or odd-sized (9 x 11)
CASES = [
    (6, 3, 32, 32, False, (32,), 32),
    (4, 2, 32, 32, False, (64,), 32),
    (4, 2, 32, 32, False, (32,), 64),
    (4, 2, 16, 16, False, (64,), 64),
    (4, 2, 16, 16, False, (128,), 64),
    (4, 2, 16, 16, False, (64,), 128),
    (6, 3, 16, 16, False, (128,), 128),
    (4, 2, 32, 32, False, (64, 64), 64),
    (4, 2, 16, 16, False, (128, 128), 128),
    (4, 2, 64, 64, False, (32, 64), 32),
    (4, 2, 32, 32, True, (64,), 64),
    (4, 2, 64, 64, True, (64,), 64),
    (13, 7, 16, 16, False, (128,), 128),
    (13, 5, 32, 32, True, (128,), 128),
    (3, 2, 24, 40, False, (32,), 64),
    (3, 1, 12, 20, False, (64,), 32),
    (3, 2, 9, 11, False, (32,), 32),
]


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("N,nb,H,W_,ups,srcC,Cout", CASES)
def test_wgrad_wino_vs_float64(N, nb, H, W_, ups, srcC, Cout, deferred):
    from sdeflow_light_amd import ops
    torch.manual_seed(N * 1000 + H + sum(srcC) + Cout)
    Hi, Wi = (H // 2, W_ // 2) if ups else (H, W_)
    Ktot, CoutP = ops.pad16(sum(srcC)), ops.pad16(Cout)
    gy = torch.randn(N * H * W_ * Cout, device=DEV)
    xs = [torch.randn(N * Hi * Wi * C, device=DEV) for C in srcC]
    base = torch.randn(9 * CoutP * Ktot, device=DEV)                # the packed image is accumulated into
    db0 = torch.randn(Cout, device=DEV)
    geom = ops.conv_geom(N, Hi, Wi, H, W_, 3, 3, 1, 1, 0, int(ups))
    # float64 reference of the weight gradient over the concatenated sources, [Cout][Cin][3][3]
    ref = R.conv_grads(gy.view(N, H, W_, Cout).double(), [x.view(N, Hi, Wi, C).double() for x, C in zip(xs, srcC)],
                       torch.zeros(Cout, sum(srcC), 3, 3, device=DEV, dtype=torch.float64), pad=1, ups=ups)["weight"]
    want = ref.permute(0, 2, 3, 1).reshape(Cout, 9, sum(srcC))           # [co][tap = 3 kh + kw][c]
    wb = gy.view(N, H * W_, Cout)[:nb].double().sum((0, 1))
    args = (geom, gy, xs, srcC, Cout, CoutP, Ktot, base, db0, nb)
    got, got_d = _wgrad_all(*args, True, deferred)
    dir_w, dir_d = _wgrad_all(*args, False, deferred)
    img = got.view(9, CoutP, Ktot)
    added = lambda t: (t.view(9, CoutP, Ktot).double() - base.view(9, CoutP, Ktot).double())[:, :Cout, :sum(srcC)].permute(1, 0, 2)  # noqa: E731
    m = metrics(added(got), want)
    md = metrics(added(dir_w), want)
    mb = metrics((got_d.double() - db0.double()).view(1, -1), wb.view(1, -1))
    print(f"wgrad wino N={N} nb={nb} {H}x{W_} ups={ups} C={srcC} Cout={Cout} deferred={deferred}: "
          f"rel-L2 {m[0]:.2e} row {m[1]:.2e} elem {m[2]:.2e} | direct {md[0]:.2e} {md[1]:.2e} {md[2]:.2e} | "
          f"bias {mb[0]:.2e} {mb[1]:.2e} {mb[2]:.2e}")
    assert within(m, WGRAD_BOUNDS), m
    assert within(mb, BIAS_BOUNDS), mb
    # the bias gradient is the same by-product of the staged cotangent as in the direct kernel: the same bits
    assert torch.equal(got_d, dir_d)
    # entries outside the written block (padding rows / columns of the packed image) are untouched
    keep = torch.ones(9, CoutP, Ktot, dtype=torch.bool, device=DEV)
    keep[:, :Cout, :sum(srcC)] = False
    assert torch.equal(img[keep], base.view(9, CoutP, Ktot)[keep])
    # slot order: the same bits on a second run
    again, again_d = _wgrad_all(*args, True, deferred)
    assert torch.equal(again, got) and torch.equal(again_d, got_d)


@pytest.mark.gpu
@pytest.mark.parametrize("supported", [True, False])
def test_conv_op_routes_wgrad(monkeypatch, supported):
    """ConvOp.backward (two sources) and backward_ups ask for the Winograd wgrad only under train_wino and when
    ops.conv_wino_supported accepts the geometry; otherwise the direct kernel, bit for bit what ops.conv_wgrad computes."""
    from sdeflow_light_amd import ops
    from sdeflow_light_amd.convnet import ConvOp, ConvOpSet
    torch.manual_seed(3)
    N, nb, H = 4, 2, 16
    calls = []
    orig = ops.conv_wgrad

    def spy(*a, **kw):
        calls.append(bool(kw.get("wino", False)))
        return orig(*a, **kw)

    monkeypatch.setattr(ops, "conv_wgrad", spy)
    if not supported:
        monkeypatch.setattr(ops, "conv_wino_supported", lambda *a, **kw: False)
    W = torch.nn.Parameter(torch.randn(64, 96, 3, 3, device=DEV) * 0.05)
    b = torch.nn.Parameter(torch.zeros(64, device=DEV))
    op = ConvOp(W, b, "conv", (3, 3), 1, 1, [64, 32])
    Wu = torch.nn.Parameter(torch.randn(32, 32, 3, 3, device=DEV) * 0.05)
    bu = torch.nn.Parameter(torch.zeros(32, device=DEV))
    opu = ConvOp(Wu, bu, "conv", (3, 3), 1, 1, [32], ups=True)
    st = ConvOpSet([op, opu])
    st.pack()
    st.pack_wino(train=True)
    assert op.train_wino and opu.train_wino
    srcs = [torch.randn(N * H * H * 64, device=DEV), torch.randn(N * H * H * 32, device=DEV)]
    gy = torch.randn(N * H * H * 64, device=DEV)
    b.grad = torch.zeros(64, device=DEV)
    op.backward(gy, srcs, N, H, H, nb)
    xu = torch.randn(N * 8 * 8 * 32, device=DEV)
    gyu = torch.randn(N * H * H * 32, device=DEV)
    bu.grad = torch.zeros(32, device=DEV)
    opu.backward_ups(gyu, xu, N, 8, 8, nb)
    torch.cuda.synchronize()
    print(f"conv_wino_supported patched to False: {not supported}; wgrad calls asked for wino: {calls}")
    assert calls == [supported] * 3
    # the op's packed gradients against direct calls of the same kind
    monkeypatch.setattr(ops, "conv_wgrad", orig)
    for o, gys, xs, Hi in ((op, gy, srcs, H), (opu, gyu, [xu], 8)):
        geom, _, _ = o._geom(N, Hi, Hi)
        want = torch.zeros_like(o.dWp)
        for s, C in enumerate(o.srcC):
            orig(geom, gys, xs[s], C, o.koff[s], want, o.Cout, o.CoutP, o.Ktot, wino=supported)
        torch.cuda.synchronize()
        assert torch.equal(o.dWp, want)


# shapes the Winograd plan declines: the U-Net's 3-channel input conv (2-D 3x3), a 1-D 3-tap, a 1x1
# (N, n_bias, Hi, Wi, KH, KW, pad, C, Cout)
DECLINED = [
    (4, 2, 32, 32, 3, 3, 1, 3, 32),
    (4, 2, 1, 256, 1, 3, 1, 64, 64),
    (4, 2, 16, 16, 1, 1, 0, 64, 128),
]


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("N,nb,Hi,Wi,KH,KW,pad,C,Cout", DECLINED)
def test_wgrad_wino_preference_on_declined_shapes(N, nb, Hi, Wi, KH, KW, pad, C, Cout, deferred):
    """msgm_conv_wgrad_det / _slabs with wino = 1 on a shape the plan declines: status 0, the workspace of wino = 0, and
    the weight and bias gradients of wino = 0, bit for bit."""
    import ctypes as C_
    from sdeflow_light_amd import ops, _lib as L
    torch.manual_seed(N * 1000 + Wi + C + Cout)
    geom = ops.conv_geom(N, Hi, Wi, Hi, Wi, KH, KW, 1, pad)
    CoutP, Ktot = ops.pad16(Cout), ops.pad16(C)
    gy = torch.randn(N * Hi * Wi * Cout, device=DEV)
    x = torch.randn(N * Hi * Wi * C, device=DEV)
    base = torch.randn(KH * KW * CoutP * Ktot, device=DEV)
    db0 = torch.randn(Cout, device=DEV)
    lib = L.lib()
    need = [int(lib.msgm_conv_wgrad_workspace(geom, C, Cout, CoutP, nb, w)) for w in (0, 1)]
    assert need[0] == need[1] > 0

    def run(wino):
        dWp, db = base.clone(), db0.clone()
        args = (geom, L.ptr(gy), L.ptr(x), C, 0, L.ptr(dWp), Cout, CoutP, Ktot, L.ptr(db), nb, None, None)
        if deferred:
            d = ops.DeferredReduces(DEV)
            ws, nbytes = d.take(need[wino])
            jobs, nj = (L.ReduceJobT * 2)(), C_.c_int32(0)
            assert lib.msgm_conv_wgrad_slabs(*args, ws, nbytes, jobs, C_.byref(nj), wino, L.stream()) == 0
            d.add(jobs, nj.value, None)
            d.flush()
        else:
            ws = torch.empty(need[wino] // 4, device=DEV)
            assert lib.msgm_conv_wgrad_det(*args, L.ptr(ws), ws.numel() * 4, wino, L.stream()) == 0
        torch.cuda.synchronize()
        return dWp, db

    w0, b0 = run(0)
    w1, b1 = run(1)
    assert not torch.equal(w0, base) and not torch.equal(b0, db0)
    assert torch.equal(w1, w0) and torch.equal(b1, b0)
