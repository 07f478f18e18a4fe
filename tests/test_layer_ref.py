"""The float64 layer references of tests/layer_ref.py (the yardstick of test_layer_census_gpu.py) against
torch.nn.functional / torch.autograd in float64 on the CPU, at small shapes."""
import pytest
import torch
import torch.nn.functional as F

import layer_ref as R

D = torch.float64


def cl(x):                                             # NCHW / NCL -> channels-last [n][H][W][C]
    return x.permute(0, 2, 3, 1) if x.dim() == 4 else x.permute(0, 2, 1)[:, None]


def close(a, b, tol=1e-12):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).norm() / max(float(b.norm()), 1e-300))
    assert err <= tol, err


@pytest.mark.parametrize("k,stride,pad,H", [(3, 1, 1, 7), (3, 2, 1, 8), (3, 2, 1, 7), (1, 1, 0, 5)])
def test_conv2d_forward_matches_functional(k, stride, pad, H):
    torch.manual_seed(k + stride + H)
    x, w, b = torch.randn(3, 5, H, H + 1, dtype=D), torch.randn(4, 5, k, k, dtype=D), torch.randn(4, dtype=D)
    ref = cl(F.conv2d(x, w, b, stride=stride, padding=pad))
    close(R.conv_forward([cl(x)], w, b, stride=stride, pad=pad, n_bias=3), ref)
    # bias on the first n_bias rows only (the tangent rows of a dual batch get none)
    y = R.conv_forward([cl(x)], w, b, stride=stride, pad=pad, n_bias=2)
    close(y[:2], ref[:2])
    close(y[2:], cl(F.conv2d(x[2:], w, None, stride=stride, padding=pad)))


@pytest.mark.parametrize("k,stride,pad", [(3, 1, 1), (4, 2, 1), (1, 1, 0)])
def test_conv1d_and_linear_forward_match_functional(k, stride, pad):
    torch.manual_seed(k)
    x, w, b = torch.randn(2, 6, 16, dtype=D), torch.randn(3, 6, k, dtype=D), torch.randn(3, dtype=D)
    close(R.conv_forward([cl(x)], w, b, stride=stride, pad=pad, n_bias=2), cl(F.conv1d(x, w, b, stride=stride, padding=pad)))
    xl, wl = torch.randn(5, 7, dtype=D), torch.randn(4, 7, dtype=D)
    close(R.conv_forward([xl[:, None, None]], wl, b[:3].repeat(2)[:4], kind="linear", n_bias=5)[:, 0, 0],
          F.linear(xl, wl, b[:3].repeat(2)[:4]))


def test_conv_transpose1d_matches_functional():
    torch.manual_seed(3)
    x, w, b = torch.randn(3, 6, 9, dtype=D), torch.randn(6, 4, 4, dtype=D), torch.randn(4, dtype=D)
    ref = cl(F.conv_transpose1d(x, w, b, stride=2, padding=1))
    close(R.conv_forward([cl(x)], w, b, kind="convT", stride=2, pad=1, n_bias=3), ref)


def test_conv_upsample_two_sources_affine_and_row_options():
    torch.manual_seed(4)
    n, H, C0, C1, Co = 4, 5, 3, 2, 6
    a, s = torch.randn(n, C0, H, H, dtype=D), torch.randn(n, C1, H, H, dtype=D)
    w, b = torch.randn(Co, C0 + C1, 3, 3, dtype=D), torch.randn(Co, dtype=D)
    sc, sh = torch.rand(n, C0 + C1, dtype=D) + 0.5, torch.randn(n, C0 + C1, dtype=D)
    sb = torch.randn(2, Co, dtype=D)
    res, base = torch.randn(n, 2 * H, 2 * H, Co, dtype=D), torch.randn(n, 2 * H, 2 * H, Co, dtype=D)
    xin = F.silu(torch.cat([a, s], 1) * sc[:, :, None, None] + sh[:, :, None, None])
    up = F.interpolate(xin, scale_factor=2, mode="nearest")
    ref = cl(F.conv2d(up, w, None, padding=1))
    ref = ref + torch.cat([b.expand(3, Co), torch.zeros(1, Co, dtype=D)])[:, None, None]
    ref = ref + torch.cat([sb, torch.zeros(2, Co, dtype=D)])[:, None, None] + res + base
    y = R.conv_forward([cl(a), cl(s)], w, b, pad=1, ups=True, n_bias=3, samp_bias=sb, emb_rows=2, in_affine=(sc, sh), in_act=1,
                       residual=res, base=base)
    close(y, ref)
    # a row subset sees the masks of its global rows
    rows = torch.tensor([3, 1])
    ys = R.conv_forward([cl(a)[rows], cl(s)[rows]], w, b, pad=1, ups=True, rows=rows, n_bias=3, samp_bias=sb, emb_rows=2,
                        in_affine=(sc[rows], sh[rows]), in_act=1, residual=res[rows], base=base[rows])
    close(ys, ref[rows])


def test_conv1d_embedding_channels():
    """The 1-D U-Net's blocks read cat([h, emb broadcast along L]) (NNUnet1D.py:156): rows >= emb_rows (the tangent rows)
    carry no embedding."""
    torch.manual_seed(5)
    n, L, C, E, Co, er = 4, 12, 3, 5, 4, 2
    x, e = torch.randn(n, C, L, dtype=D), torch.randn(er, E, dtype=D)
    w, b = torch.randn(Co, C + E, 3, dtype=D), torch.randn(Co, dtype=D)
    ecat = torch.cat([e, torch.zeros(n - er, E, dtype=D)])[:, :, None].expand(n, E, L)
    ref = cl(F.conv1d(torch.cat([x, ecat], 1), w, None, padding=1)) + torch.cat([b.expand(er, Co),
                                                                                 torch.zeros(n - er, Co, dtype=D)])[:, None, None]
    close(R.conv_forward([cl(x)], w, b, pad=1, n_bias=er, emb=e), ref)


def test_conv_grads_match_autograd_of_functional():
    """dgrad, wgrad, bias, per-sample bias and embedding cotangents against autograd of F.conv1d / F.conv2d."""
    torch.manual_seed(6)
    n, L, C0, C1, E, Co, er = 4, 10, 3, 2, 5, 4, 2
    x0, x1 = torch.randn(n, C0, L, dtype=D, requires_grad=True), torch.randn(n, C1, L, dtype=D, requires_grad=True)
    e = torch.randn(er, E, dtype=D, requires_grad=True)
    w = torch.randn(Co, C0 + C1 + E, 3, dtype=D, requires_grad=True)
    b = torch.randn(Co, dtype=D, requires_grad=True)
    ecat = torch.cat([e, torch.zeros(n - er, E, dtype=D)])[:, :, None].expand(n, E, L)
    y = F.conv1d(torch.cat([x0, x1, ecat], 1), w, None, padding=1) + torch.cat([b.expand(er, Co),
                                                                                torch.zeros(n - er, Co, dtype=D)])[:, :, None]
    gy = torch.randn_like(y)
    (y * gy).sum().backward()
    g = R.conv_grads(cl(gy), [cl(x0.detach()), cl(x1.detach())], w.detach(), b.detach(), emb=e.detach(), pad=1, n_bias=er)
    close(g["src0"], cl(x0.grad))
    close(g["src1"], cl(x1.grad))
    close(g["weight"], w.grad)
    close(g["bias"], b.grad)
    close(g["emb"], e.grad)
    # per-sample bias: its cotangent is the spatial sum of gy over the rows that carry it
    sb = torch.randn(er, Co, dtype=D)
    g2 = R.conv_grads(cl(gy), [cl(x0.detach())], w.detach()[:, :C0], samp_bias=sb, pad=1, n_bias=0, emb_rows=er)
    close(g2["samp_bias"], gy[:er].sum(2))
    # 2-D, stride 2
    x = torch.randn(3, 4, 9, 9, dtype=D, requires_grad=True)
    w2 = torch.randn(5, 4, 3, 3, dtype=D, requires_grad=True)
    y2 = F.conv2d(x, w2, padding=1, stride=2)
    g2y = torch.randn_like(y2)
    (y2 * g2y).sum().backward()
    g3 = R.conv_grads(cl(g2y), [cl(x.detach())], w2.detach(), stride=2, pad=1)
    close(g3["src0"], cl(x.grad))
    close(g3["weight"], w2.grad)


@pytest.mark.parametrize("silu", [False, True])
def test_groupnorm_dual_matches_functional(silu):
    torch.manual_seed(7)
    n, C, H, G = 3, 8, 5, 4
    x, xd = torch.randn(n, C, H, H, dtype=D) * 1.5 + 0.3, torch.randn(n, C, H, H, dtype=D)
    gam, bet = 1 + 0.2 * torch.randn(C, dtype=D), 0.2 * torch.randn(C, dtype=D)
    f = lambda a, g_, b_: (F.silu if silu else (lambda t: t))(F.group_norm(a, G, g_, b_, eps=1e-5))   # noqa: E731
    gp, gt = torch.randn(n, C, H, H, dtype=D), torch.randn(n, C, H, H, dtype=D)
    xg, xdg = x.clone().requires_grad_(True), xd.clone().requires_grad_(True)
    gg, bg = gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    yp, yt = torch.func.jvp(lambda a: f(a, gg, bg), (xg,), (xdg,))
    ((yp * gp).sum() + (yt * gt).sum()).backward()
    flat = lambda t: cl(t).reshape(n, H * H, C)   # noqa: E731
    rp, rt = R.gn_dual_forward(flat(x), flat(xd), gam, bet, G, silu)
    close(rp, flat(yp.detach()))
    close(rt, flat(yt.detach()))
    dxp, dxt, dga, dbe = R.gn_dual_backward(flat(x), flat(xd), gam, bet, G, silu, flat(gp), flat(gt))
    close(dxp, flat(xg.grad))
    close(dxt, flat(xdg.grad))
    close(dga, gg.grad)
    close(dbe, bg.grad)
    sc, sh = R.groupnorm_affine(flat(x), gam, bet, G)
    close(flat(x) * sc[:, None] + sh[:, None], flat(F.group_norm(x, G, gam, bet, eps=1e-5)))


def test_attention_dual_matches_autograd():
    torch.manual_seed(8)
    n, T, C = 2, 6, 4
    qkv, qd = torch.randn(n, 3 * C, T, dtype=D), torch.randn(n, 3 * C, T, dtype=D)
    s = C ** -0.25

    def qkv_attention(a):                                # model/unet.py:236-250 on [n][3C][T]
        q, k, v = a.split(C, dim=1)
        w = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
        return torch.einsum("bts,bcs->bct", w, v)
    xp, xt = qkv.clone().requires_grad_(True), qd.clone().requires_grad_(True)
    o, od = torch.func.jvp(qkv_attention, (xp,), (xt,))
    gp, gt = torch.randn_like(o), torch.randn_like(od)
    ((o * gp).sum() + (od * gt).sum()).backward()
    t = lambda a: a.transpose(1, 2)   # noqa: E731
    close(R.attention(t(qkv), s * s), t(qkv_attention(qkv)))
    rp, rt = R.attention_dual_forward(t(qkv), t(qd), s * s)
    close(rp, t(o.detach()))
    close(rt, t(od.detach()))
    dp, dt = R.attention_dual_backward(t(qkv), t(qd), s * s, t(gp), t(gt))
    close(dp, t(xp.grad))
    close(dt, t(xt.grad))


@pytest.mark.parametrize("act", [0, 1])
def test_act_dual_matches_autograd(act):
    torch.manual_seed(9 + act)
    z, zd = torch.randn(40, dtype=D) * 2, torch.randn(40, dtype=D)
    fn = (lambda a: F.gelu(a)) if act == 0 else F.silu
    zg, zdg = z.clone().requires_grad_(True), zd.clone().requires_grad_(True)
    hp, ht = torch.func.jvp(fn, (zg,), (zdg,))
    gp, gt = torch.randn(40, dtype=D), torch.randn(40, dtype=D)
    ((hp * gp).sum() + (ht * gt).sum()).backward()
    rp, rt = R.act_dual_forward(act, z, zd)
    close(rp, hp.detach())
    close(rt, ht.detach())
    dp, dt = R.act_dual_backward(act, z, zd, gp, gt)
    close(dp, zg.grad)
    close(dt, zdg.grad)


def test_emb_bank_matches_linear():
    torch.manual_seed(10)
    rows, K, nb = 5, 6, 3
    semb = torch.randn(rows, K, dtype=D, requires_grad=True)
    items = [(torch.randn(co, K, dtype=D, requires_grad=True), torch.randn(co, dtype=D, requires_grad=True)) for co in (4, 3)]
    outs = [torch.cat([F.linear(semb[:nb], w, b), F.linear(semb[nb:], w)]) for w, b in items]
    douts = [torch.randn_like(o) for o in outs]
    sum((o * d).sum() for o, d in zip(outs, douts)).backward()
    for r, o in zip(R.emb_bank_forward(semb.detach(), [(w.detach(), b.detach()) for w, b in items], nb), outs):
        close(r, o.detach())
    ds, wb = R.emb_bank_backward(semb.detach(), [(w.detach(), b.detach()) for w, b in items], nb, douts)
    close(ds, semb.grad)
    for (dw, db), (w, b) in zip(wb, items):
        close(dw, w.grad)
        close(db, b.grad)
