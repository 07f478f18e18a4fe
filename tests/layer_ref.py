"""Plain float64 restatements of the single layers the U-Net score nets run on the HIP kernels, written from the PyTorch-layout
parameters and the reference modules' semantics (model/unet.py, NNUnet1D.py) — no packed weight images, nothing from the
package.  tests/test_layer_census_gpu.py compares every kernel call of the benchmarked steps against them;
tests/test_layer_ref.py checks them against torch.nn.functional / torch.autograd on the CPU.

Conventions (those of the kernels): activations are channels-last ``[n][H][W][C]`` (1-D: H = 1) and the forward-mode
tangent rides as extra rows.  ``rows`` holds the GLOBAL row index of every row of a chunk, so that a row subset (or a chunk
of a reduction over all rows) sees the bias / per-sample-bias masks of its place in the launch: the conv bias applies to
rows < n_bias, a per-sample bias / embedding to rows < emb_rows.  Backward references are torch.autograd of these forwards
(dual forms: torch.func.jvp, then autograd of the pair)."""
import torch
import torch.nn.functional as F

EPS = 1e-5


def silu(x):
    return x * torch.sigmoid(x)


def gelu(x):                                           # exact erf form (nn.GELU default, NNUnet1D.py:18,20)
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


ACTS = {0: gelu, 1: silu}                              # ops.ACT_GELU, ops.ACT_SILU


# ----------------------------------------------------------------------------------------------- convolution
def _w4(weight, kind):
    """Any conv / linear / convT weight as [Cout][Cin][KH][KW]."""
    w = weight
    if kind == "convT":                                 # (Cin, Cout, k...) -> (Cout, Cin, k...)
        w = w.transpose(0, 1)
    if w.dim() == 2:
        w = w[:, :, None, None]
    elif w.dim() == 3:
        w = w[:, :, None, :]
    return w


def conv_taps(x, w4, stride, pad, pad_h):
    """Cross-correlation of channels-last x [n][H][W][Ci] with w4 [Co][Ci][KH][KW] as a sum over taps of shifted
    channels-last einsums (zero padding: pad on W, pad_h on H)."""
    n, H, W, _ = x.shape
    KH, KW = w4.shape[2], w4.shape[3]
    xp = F.pad(x, (0, 0, pad, pad, pad_h, pad_h))
    sh = stride if KH > 1 else 1
    Ho, Wo = (H + 2 * pad_h - KH) // sh + 1, (W + 2 * pad - KW) // stride + 1
    y = None
    for kh in range(KH):
        for kw in range(KW):
            xs = xp[:, kh: kh + sh * (Ho - 1) + 1: sh, kw: kw + stride * (Wo - 1) + 1: stride, :]
            t = torch.einsum("nhwc,oc->nhwo", xs, w4[:, :, kh, kw])
            y = t if y is None else y + t
    return y


def conv_forward(srcs, weight, bias=None, *, kind="conv", stride=1, pad=0, ups=False, rows=None, n_bias=0, emb=None,
                 samp_bias=None, emb_rows=None, in_affine=None, in_act=0, residual=None, base=None):
    """One ConvOp / Stride2PairOp call.  srcs: list of [n][Hi][Wi][Cs] (two = channel concatenation, model/unet.py:514 /
    NNUnet1D.py:175); weight / bias: PyTorch layout of Conv1d / Conv2d / ConvTranspose1d / Linear; rows: global row ids
    [n] (default 0..n-1); bias on rows < n_bias; samp_bias [emb_rows][Cout] and emb [emb_rows][E] (the 1-D U-Net's time
    embedding, broadcast along L as extra input channels after the sources, zero-padded like them, NNUnet1D.py:156) on rows
    < emb_rows, indexed by the global row; in_affine (scale, shift) [n][Cin] applied per (row, channel) before the conv,
    then SiLU when in_act (GroupNorm+SiLU folded into the input); nearest 2x upsample of the input when ups
    (model/unet.py:60-73); residual / base (accumulate) [n][Ho][Wo][Cout] added to the output."""
    x = torch.cat(list(srcs), -1) if len(srcs) > 1 else srcs[0]
    n = x.shape[0]
    rows = torch.arange(n, device=x.device) if rows is None else rows
    er = n_bias if emb_rows is None else emb_rows
    if in_affine is not None:
        x = x * in_affine[0][:, None, None, :] + in_affine[1][:, None, None, :]
        if in_act:
            x = silu(x)
    if ups:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    on = (rows < er).to(x.dtype)
    ridx = rows.clamp(max=max(er - 1, 0))
    if emb is not None:
        e = emb[ridx] * on[:, None]
        x = torch.cat([x, e[:, None, None, :].expand(n, x.shape[1], x.shape[2], e.shape[1])], -1)
    w4 = _w4(weight, kind)
    KH, KW = w4.shape[2], w4.shape[3]
    pad_h = pad if KH > 1 else 0
    if kind == "convT":
        # out[o] = sum_{i, k: o = s i - p + k} x[i] W[ci][co][k]: zero-insert the input, pad k-1-p, correlate with the
        # flipped kernel
        assert x.shape[1] == 1 and KH == 1
        L = x.shape[2]
        xd = x.new_zeros(n, 1, (L - 1) * stride + 1, x.shape[3])
        xd[:, :, ::stride] = x
        y = conv_taps(xd, w4.flip(3), 1, KW - 1 - pad, 0)
    else:
        y = conv_taps(x, w4, stride, pad, pad_h)
    if bias is not None:
        y = y + bias * (rows < n_bias).to(y.dtype)[:, None, None, None]
    if samp_bias is not None:
        y = y + (samp_bias[ridx] * on[:, None])[:, None, None, :]
    if residual is not None:
        y = y + residual
    if base is not None:
        y = y + base
    return y


def conv_grads(gy, srcs, weight, bias=None, emb=None, samp_bias=None, **kw):
    """Cotangents of conv_forward for the output cotangent gy: {"src0", "src1", "weight", "bias", "emb",
    "samp_bias"} (those whose inputs were given)."""
    named = {f"src{i}": s for i, s in enumerate(srcs)}
    named.update(weight=weight, bias=bias, emb=emb, samp_bias=samp_bias)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in named.items() if v is not None}
    with torch.enable_grad():
        y = conv_forward([leaves[f"src{i}"] for i in range(len(srcs))], leaves["weight"], leaves.get("bias"),
                         emb=leaves.get("emb"), samp_bias=leaves.get("samp_bias"), **kw)
        gs = torch.autograd.grad(y, list(leaves.values()), gy, allow_unused=True)
    return {k: (g if g is not None else torch.zeros_like(leaves[k])) for k, g in zip(leaves, gs)}


# ----------------------------------------------------------------------------------------------- GroupNorm
def groupnorm(x, gamma, beta, G, eps=EPS):
    """GroupNorm over x [n][P][C] (statistics per row and group of C / G channels, model/nn_utils.py:107-114)."""
    n, P, C = x.shape
    xr = x.reshape(n, P, G, C // G)
    mu = xr.mean(dim=(1, 3), keepdim=True)
    var = ((xr - mu) ** 2).mean(dim=(1, 3), keepdim=True)
    return ((xr - mu) / torch.sqrt(var + eps)).reshape(n, P, C) * gamma + beta


def groupnorm_affine(x, gamma, beta, G, eps=EPS):
    """GroupNorm of x [n][P][C] as a per-(row, channel) map: (scale, shift) [n][C] with GN(x) = scale x + shift."""
    n, P, C = x.shape
    xr = x.reshape(n, P, G, C // G)
    mu = xr.mean(dim=(1, 3))
    var = ((xr - mu[:, None, :, None]) ** 2).mean(dim=(1, 3))
    inv = 1.0 / torch.sqrt(var + eps)
    scale = inv.repeat_interleave(C // G, 1) * gamma
    return scale, beta - mu.repeat_interleave(C // G, 1) * scale


def gn_act(x, gamma, beta, G, act):
    y = groupnorm(x, gamma, beta, G)
    return silu(y) if act else y


def gn_dual_forward(xp, xt, gamma, beta, G, act):
    """(primal, tangent) of GroupNorm(+SiLU) at xp in the direction xt."""
    return torch.func.jvp(lambda a: gn_act(a, gamma, beta, G, act), (xp,), (xt,))


def gn_dual_backward(xp, xt, gamma, beta, G, act, gp, gt):
    """Cotangents (dxp, dxt, dgamma, dbeta) of sum(yp gp) + sum(yt gt) for (yp, yt) = gn_dual_forward(...)."""
    a, b, g_, b_ = (t.detach().clone().requires_grad_(True) for t in (xp, xt, gamma, beta))
    with torch.enable_grad():
        yp, yt = torch.func.jvp(lambda u: gn_act(u, g_, b_, G, act), (a,), (b,))
        return torch.autograd.grad((yp * gp).sum() + (yt * gt).sum(), (a, b, g_, b_))


# ----------------------------------------------------------------------------------------------- attention
def attention(qkv, scale):
    """QKVAttention (model/unet.py:236-250) on channels-last qkv [n][T][3C] (q | k | v): softmax(scale q k^T) v
    (scale = (C^-1/4)^2)."""
    C = qkv.shape[-1] // 3
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    return torch.einsum("bts,bsc->btc", torch.softmax(scale * torch.einsum("btc,bsc->bts", q, k), -1), v)


def attention_dual_forward(qp, qt, scale):
    return torch.func.jvp(lambda a: attention(a, scale), (qp,), (qt,))


def attention_dual_backward(qp, qt, scale, gp, gt):
    """(dqkv_primal, dqkv_tangent) of sum(o gp) + sum(odot gt)."""
    a, b = qp.detach().clone().requires_grad_(True), qt.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        o, od = torch.func.jvp(lambda u: attention(u, scale), (a,), (b,))
        return torch.autograd.grad((o * gp).sum() + (od * gt).sum(), (a, b))


# ----------------------------------------------------------------------------------------------- activations, embedding
def act_dual_forward(act, zp, zt):
    return torch.func.jvp(ACTS[act], (zp,), (zt,))


def act_dual_backward(act, zp, zt, gp, gt):
    a, b = zp.detach().clone().requires_grad_(True), zt.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        hp, ht = torch.func.jvp(ACTS[act], (a,), (b,))
        return torch.autograd.grad((hp * gp).sum() + (ht * gt).sum(), (a, b))


def emb_bank_forward(semb, items, n_bias):
    """Every ResBlock's emb_layers[1] Linear (model/unet.py:145-151, 176-180): out_i [rows][co_i], bias on rows < n_bias."""
    on = (torch.arange(semb.shape[0], device=semb.device) < n_bias).to(semb.dtype)[:, None]
    return [semb @ w.T + on * b for w, b in items]


def emb_bank_backward(semb, items, n_bias, douts):
    """(dsemb, [(dW_i, db_i)]) for the output cotangents douts; db_i is also the gradient of the conv bias added at the
    same place."""
    s = semb.detach().clone().requires_grad_(True)
    leaves = [(w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)) for w, b in items]
    with torch.enable_grad():
        outs = emb_bank_forward(s, leaves, n_bias)
        loss = sum((o * d).sum() for o, d in zip(outs, douts))
        flat = torch.autograd.grad(loss, [s] + [t for wb in leaves for t in wb])
    return flat[0], [(flat[1 + 2 * i], flat[2 + 2 * i]) for i in range(len(items))]
