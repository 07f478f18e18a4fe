"""The staging and the operands of k_wgrad_wino (conv_kernels.hip) at the smallest shapes at which they can go wrong.  The kernel
has ONE staging path, with per-element bounds tests; the shapes put every kind of tile through it: a tile whose halo lies
wholly inside the image next to border tiles on all four sides, with and without the folded 2x upsample;
channel counts that leave the last 32-channel block partial; workgroups that own a single tile (no buffer swap) or an odd
number of them; a second source at a K offset with the bias gradient over the primal rows only.

GPU: ops.conv_wgrad(..., wino=True) against the float64 reference of tests/layer_ref.py under the bounds
tests/test_wgrad_wino_gpu.py holds the kernel to (imported, not restated), per-call and deferred slot reduction, and two runs
give the same bits.  CPU: the float64 reference of these very inputs agrees with torch.nn.grad.conv2d_weight in float64 far
inside those bounds, so a failure on the GPU is the kernel's."""
import functools

import pytest
import torch

import layer_ref as R
from test_wgrad_wino_gpu import BIAS_BOUNDS, WGRAD_BOUNDS, _wgrad_all, metrics, within

# (N, n_bias, H, W of the output, ups, source channels, Cout)
CASES = [
    (2, 1, 24, 48, False, (32,), 32),        # 3 x 3 tiles: exactly one interior tile among eight border tiles
    (2, 1, 24, 48, True, (32,), 32),         # the same with the folded 2x upsample (input 12 x 24)
    (2, 1, 20, 40, False, (36,), 44),        # channel counts that are multiples of 4 but not of 32, ragged tiles in both directions
    (2, 1, 8, 16, False, (32,), 32),         # one tile per image, nothing but border
    (3, 2, 40, 16, False, (32, 32), 64),     # an odd number of tiles per workgroup, second source at a K offset, bias over the primal rows
    (1, 1, 8, 16, False, (32,), 32),         # added to the issue's rows: one tile in all, a workgroup that owns a single tile (no buffer swap)
]

IDS = [f"N{c[0]}-{c[2]}x{c[3]}-ups{int(c[4])}-{'+'.join(map(str, c[5]))}to{c[6]}" for c in CASES]


@functools.lru_cache(maxsize=None)
def _inputs(case, dev):
    """Seeded inputs of a case and their float64 references (weight gradient [Cout][9][sum C], bias gradient), made once."""
    N, nb, H, W_, ups, srcC, Cout = case
    g = torch.Generator(device="cpu").manual_seed(N * 1000 + H * 7 + W_ + sum(srcC) + Cout + int(ups))
    Hi, Wi = (H // 2, W_ // 2) if ups else (H, W_)
    gy = torch.randn(N * H * W_ * Cout, generator=g).to(dev)
    xs = [torch.randn(N * Hi * Wi * C, generator=g).to(dev) for C in srcC]
    ref = R.conv_grads(gy.view(N, H, W_, Cout).double(), [x.view(N, Hi, Wi, C).double() for x, C in zip(xs, srcC)],
                       torch.zeros(Cout, sum(srcC), 3, 3, device=dev, dtype=torch.float64), pad=1, ups=ups)["weight"]
    want = ref.permute(0, 2, 3, 1).reshape(Cout, 9, sum(srcC))           # [co][tap = 3 kh + kw][c]
    wb = gy.view(N, H * W_, Cout)[:nb].double().sum((0, 1))
    return gy, xs, want, wb


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float64_reference_alone(case):
    """CPU: layer_ref's weight gradient of these inputs against torch.nn.grad.conv2d_weight in float64 (the upsample written out)."""
    N, nb, H, W_, ups, srcC, Cout = case
    gy, xs, want, _ = _inputs(case, "cpu")
    Hi, Wi = (H // 2, W_ // 2) if ups else (H, W_)
    x = torch.cat([t.view(N, Hi, Wi, C).double() for t, C in zip(xs, srcC)], dim=3).permute(0, 3, 1, 2)
    if ups:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    gw = torch.nn.grad.conv2d_weight(x, (Cout, sum(srcC), 3, 3), gy.view(N, H, W_, Cout).double().permute(0, 3, 1, 2), padding=1)
    other = gw.permute(0, 2, 3, 1).reshape(Cout, 9, sum(srcC))
    m = metrics(other, want)
    print(f"float64 reference vs conv2d_weight: rel-L2 {m[0]:.2e} row {m[1]:.2e} elem {m[2]:.2e}")
    assert within(m, tuple(1e-6 * b for b in WGRAD_BOUNDS)), m


@pytest.mark.gpu
@pytest.mark.parametrize("deferred", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wgrad_wino_paths_vs_float64(case, deferred):
    from sdeflow_light_amd import ops
    N, nb, H, W_, ups, srcC, Cout = case
    gy, xs, want, wb = _inputs(case, "cuda")
    Hi, Wi = (H // 2, W_ // 2) if ups else (H, W_)
    Ktot, CoutP = ops.pad16(sum(srcC)), ops.pad16(Cout)
    g = torch.Generator(device="cpu").manual_seed(17)
    base = torch.randn(9 * CoutP * Ktot, generator=g).cuda()         # the packed image is accumulated into
    db0 = torch.randn(Cout, generator=g).cuda()
    geom = ops.conv_geom(N, Hi, Wi, H, W_, 3, 3, 1, 1, 0, int(ups))
    args = (geom, gy, xs, srcC, Cout, CoutP, Ktot, base, db0, nb)
    got, got_d = _wgrad_all(*args, True, deferred)
    added = (got.view(9, CoutP, Ktot).double() - base.view(9, CoutP, Ktot).double())[:, :Cout, :sum(srcC)].permute(1, 0, 2)
    m = metrics(added, want)
    mb = metrics((got_d.double() - db0.double()).view(1, -1), wb.view(1, -1))
    print(f"wgrad wino paths N={N} nb={nb} {H}x{W_} ups={ups} C={srcC} Cout={Cout} deferred={deferred}: "
          f"rel-L2 {m[0]:.2e} row {m[1]:.2e} elem {m[2]:.2e} | bias {mb[0]:.2e} {mb[1]:.2e} {mb[2]:.2e}")
    assert within(m, WGRAD_BOUNDS), m
    assert within(mb, BIAS_BOUNDS), mb
    # entries outside the written block (padding rows / columns of the packed image) are untouched
    keep = torch.ones(9, CoutP, Ktot, dtype=torch.bool, device="cuda")
    keep[:, :Cout, :sum(srcC)] = False
    assert torch.equal(got.view(9, CoutP, Ktot)[keep], base.view(9, CoutP, Ktot)[keep])
    # the same bits on a second run
    again, again_d = _wgrad_all(*args, True, deferred)
    assert torch.equal(again, got) and torch.equal(again_d, got_d)
