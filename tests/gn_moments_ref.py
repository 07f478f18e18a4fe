"""The GroupNorm reduce kernels' moment arithmetic restated in numpy, the ill-conditioned input cases of
tests/test_groupnorm_cond_gpu.py, and the per-(sample, group) criterion both test files apply.

Restated (csrc/unet2d_kernels.hip): gn_chunks' sub-chunking of a sample's pixels, gn_lane's pixel lanes (PL = 256 / (C / V)
lanes, lane pl takes pixels ps + pl, ps + pl + PL, ... of a sub-chunk), one fp32 partial sum per (lane, channel, moment) over a
sub-chunk, widened to double there and added in double from then on, gn_stats' finalisation (double, results rounded to
fp32) and k_gn_fwd_apply's fp32 element chain without the activation.  Every fp32 product, difference and sum is one
numpy float32 operation (the kernels are built without contraction).  What is NOT restated is the ORDER of the double
additions (lanes, channels of a group, chunk slots): their rounding is 2^-53 relative, nine orders below what is measured.

Two forms of the per-element terms:
  raw      x, x^2, xdot, x xdot                                        (the kernels up to and including commit b1de595)
  shifted  u = x - k, u^2, xdot, u xdot with k the sample's own first pixel of that channel, and the pivot put back in
           double before the group sums:  sum x = s0 + n k,  sum x^2 = s1 + 2 k s0 + n k^2,  sum x xdot = s3 + k s2
           (n = pixels the lane summed; the tangent's own sums stay raw)
KERNEL_FORM names the one k_gn_fwd_reduce uses now.  With it goes the form of the mean: raw keeps mu as one fp32 number and
xhat = (x - mu) inv; shifted keeps it relative to the group's pivot kg (the sample's first pixel of the group's first
channel), stats[0] = fp32(mean - kg) and xhat = ((x - kg) - stats[0]) inv — an fp32 mean alone is off by up to
2^-25 |mean| / sigma in xhat, which fp32 PyTorch undercuts by chance in single groups.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

KERNEL_FORM = "shifted"
EPS = 1e-5
f32 = np.float32


# ------------------------------------------------------------------------------------------------ launch geometry
def gn_chunks(Bp, P):
    """(chunk, sub, nch) of a reduce launch over Bp samples of P pixels."""
    c = min(max((P + 31) // 32, 64), P)
    nsub = -(-P // c)
    want = max(-(-512 // Bp), 1)
    m = max(nsub // want, 1)
    return m * c, c, -(-P // (m * c))


def gn_lane(C, vec):
    """(V, CV, PL): channels per thread, channel vectors per pixel, pixel lanes."""
    V = 4 if vec else 1
    CV = C // V
    return V, CV, 256 // CV


# ------------------------------------------------------------------------------------------------ the reduce
def reduce_moments(x, xd, G, Bp, form=KERNEL_FORM, vec=None):
    """Moments [G][4] (double: sum x, sum x^2, sum xdot, sum x xdot) of ONE sample x [P][C] (fp32; xd its tangent or None)
    as a launch over Bp samples accumulates them."""
    assert x.dtype == f32 and form in ("raw", "shifted")
    P, C = x.shape
    vec = (C % 4 == 0) if vec is None else vec
    _, _, PL = gn_lane(C, vec)
    chunk, sub, nch = gn_chunks(Bp, P)
    assert nch <= 32
    if xd is None:
        xd = np.zeros_like(x)
    k = x[0].copy() if form == "shifted" else np.zeros(C, f32)
    u = x - k                                                    # fp32 (raw: exact)
    T = np.stack([u, u * u, xd, u * xd])                         # fp32 terms [4][P][C]
    assert T.dtype == f32
    kk = k.astype(np.float64)
    acc = np.zeros((4, G))
    for ch in range(nch):
        p0, p1 = ch * chunk, min((ch + 1) * chunk, P)
        d = np.zeros((4, PL, C))
        n = np.zeros((PL, 1))
        for ps in range(p0, p1, sub):
            pe = min(ps + sub, p1)
            s = np.zeros((4, PL, C), f32)
            for lo in range(ps, pe, PL):
                hi = min(lo + PL, pe)
                s[:, :hi - lo] += T[:, lo:hi]                    # one fp32 add per (lane, channel, moment)
                n[:hi - lo] += 1
            d += s                                               # widened once per sub-chunk
        if form == "shifted":
            d = np.stack([d[0] + n * kk, d[1] + 2.0 * kk * d[0] + n * kk * kk, d[2], d[3] + kk * d[2]])
        acc += d.reshape(4, PL, G, C // G).sum(axis=(1, 3))
    return acc.T.copy()


def gn_stats(mom, cnt, kg=None, eps=EPS):
    """gn_stats of the kernels: moments [G][4] -> fp32 (mu - kg, inv, md, a) [G][4]; kg [G]: the groups' pivots (fp32; None: 0,
    the plain fp32 mean of the kernels up to commit b1de595)."""
    m = mom[:, 0] / cnt
    var = np.maximum(mom[:, 1] / cnt - m * m, 0.0)
    iv = 1.0 / np.sqrt(var + np.float64(f32(eps)))
    d = mom[:, 2] / cnt
    m0 = m if kg is None else m - kg.astype(np.float64)
    return np.stack([m0, iv, d, iv * (mom[:, 3] / cnt - m * d)], 1).astype(f32)


def forward(x, xd, gamma, beta, G, Bp=None, form=KERNEL_FORM, vec=None):
    """Dual GroupNorm forward without activation as the kernels compute it: x, xd [n][P][C] fp32 ->
    (primal, tangent, stats [n][G][4]), all fp32."""
    n, P, C = x.shape
    cpg = C // G
    Bp = n if Bp is None else Bp
    yp, yt, st = np.empty_like(x), np.empty_like(x), np.empty((n, G, 4), f32)
    ga, be = gamma.astype(f32), beta.astype(f32)
    for b in range(n):
        kg = x[b, 0, ::cpg].copy() if form == "shifted" else np.zeros(G, f32)
        st[b] = gn_stats(reduce_moments(x[b], xd[b], G, Bp, form, vec), float(P * cpg), kg)
        mu, inv, md, a = (np.repeat(st[b][:, i], cpg) for i in range(4))
        xh = ((x[b] - np.repeat(kg, cpg)) - mu) * inv
        yp[b] = ga * xh + be
        yt[b] = ga * (inv * ((xd[b] - md) - xh * a))
    assert yp.dtype == f32 and yt.dtype == f32
    return yp, yt, st


# ------------------------------------------------------------------------------------------------ input cases
# (mean, std) of the conditioning sweep: per-group |mean| / std up to 0, 10, 100, 10, 100, 10^3 ... 10^4
CONDS = ((0.0, 1.0), (10.0, 1.0), (100.0, 1.0), (10.0, 0.1), (100.0, 0.1), (1000.0, 0.1))
# (C, G, P, B, forward_only): the smallest shapes that reach each launch geometry of the reduce
SHAPES = (
    (6, 6, 49, 3, False),        # !VEC build, cpg = 1, four dead threads, P < 64: sub = chunk = P
    (6, 3, 64, 3, False),        # !VEC build, cpg = 2
    (130, 26, 36, 3, False),     # !VEC build with one pixel lane, 126 dead threads
    (96, 32, 81, 3, False),      # VEC build, cpg = 3, 240 live threads, ragged last sub-chunk
    (192, 32, 16, 3, False),     # cpg = 6, P below one lane sweep
    (256, 32, 25, 3, False),     # four pixel lanes, the C <= 256 limit
    (32, 32, 2050, 20, False),   # 32 sub-chunks of 65 pixels and a ragged tail (one per workgroup at 20 samples)
    (32, 32, 2050, 32, False),   # the same with two sub-chunks per workgroup (m = 2 needs >= 32 samples)
    (64, 32, 4096, 1, True),     # all 32 slots of a sample in use; non-dual forward and affine only
)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_inputs(C, G, P, B, mean, std, seed, src_means=None):
    """fp32 (x, xdot, gamma, beta) of one case, x / xdot [B][P][C].  Every (sample, group) gets a mean of its own,
    +-mean U(0.8, 1) with the sign drawn per group, and noise standardised per (sample, group) in float64 before it is
    scaled by std, so that the group's own variance is std^2 whatever its size: the nominal |mean| / std is the upper end
    and no group is worse conditioned than the case says.  The tangent has mean 1 and unit spread.
    src_means = (C0, m0, m1): the channels below / from C0 get |mean| m0 / m1 instead (a two-source concatenation)."""
    g = _gen(seed)
    cpg = C // G
    z = torch.randn(B, P, G, cpg, generator=g, dtype=torch.float64)
    z = (z - z.mean(dim=(1, 3), keepdim=True)) / z.var(dim=(1, 3), unbiased=False, keepdim=True).sqrt()
    sign = torch.where(torch.rand(B, 1, G, 1, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0)
    mag = 0.8 + 0.2 * torch.rand(B, 1, G, 1, generator=g, dtype=torch.float64)
    x = (sign * mag * mean + std * z).reshape(B, P, C)
    if src_means is not None:
        C0, m0, m1 = src_means
        off = torch.cat([torch.full((C0,), float(m0)), torch.full((C - C0,), float(m1))]).double()
        x = (std * z).reshape(B, P, C) + (sign * mag).expand(B, 1, G, cpg).reshape(B, 1, C) * off
    xd = 1.0 + torch.randn(B, P, C, generator=g, dtype=torch.float64)
    gamma = 1.0 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    return tuple(t.float().contiguous() for t in (x, xd, gamma, beta))


def make_degenerate(C, G, P, B, c, seed):
    """Random well-conditioned data (mean 0.3, std 1.5) with, in sample 1, group 0 exactly constant (= c) and — when a group
    has more than one channel — group G - 1 constant per channel, the channels at c + 1, c + 2, ..."""
    x, xd, gamma, beta = make_inputs(C, G, P, B, 0.0, 1.0, seed)
    x = x * 1.5 + 0.3
    cpg = C // G
    s = min(1, B - 1)
    x[s, :, :cpg] = c
    if cpg > 1:
        x[s, :, C - cpg:] = c + torch.arange(1, cpg + 1, dtype=torch.float32)
    return x.contiguous(), xd, gamma, beta


# ------------------------------------------------------------------------------------------------ references
def torch_fp32_forward(x, xd, gamma, beta, G, silu):
    """The yardstick: PyTorch fp32 on the CPU, F.group_norm (+SiLU) through torch.func.jvp.  x, xd [n][P][C] (any float
    type; the computation runs in that type).  Returns (primal, tangent) [n][P][C]."""
    def f(a):
        y = F.group_norm(a.permute(0, 2, 1), G, gamma, beta, eps=EPS).permute(0, 2, 1)
        return y * torch.sigmoid(y) if silu else y
    yp, yt = torch.func.jvp(f, (x,), (xd,))
    return yp.contiguous(), yt.contiguous()


def torch_fp32_backward(x, xd, gamma, beta, G, silu, gp, gt, mask=None):
    """(dx, dxdot, dgamma, dbeta) of sum(yp gp) + sum(yt gt) by autograd of the jvp pair, in the inputs' type; mask: a
    multiplier applied to both outputs (dropout)."""
    a, b, g_, b_ = (t.detach().clone().requires_grad_(True) for t in (x, xd, gamma, beta))

    def f(u):
        y = F.group_norm(u.permute(0, 2, 1), G, g_, b_, eps=EPS).permute(0, 2, 1)
        y = y * torch.sigmoid(y) if silu else y
        return y if mask is None else y * mask
    with torch.enable_grad():
        yp, yt = torch.func.jvp(f, (a,), (b,))
        return torch.autograd.grad((yp * gp).sum() + (yt * gt).sum(), (a, b, g_, b_))


def stats_of(x, xd, G, eps=EPS):
    """(mu, inv, md, a) [n][G][4] by the two-pass definition in the inputs' type (float64: the reference of the saved
    statistics; float32: their yardstick) and, last, the spread of xdot per group [n][G]."""
    n, P, C = x.shape
    xr, dr = x.reshape(n, P, G, C // G), xd.reshape(n, P, G, C // G)
    mu, md = xr.mean(dim=(1, 3), keepdim=True), dr.mean(dim=(1, 3), keepdim=True)
    var = ((xr - mu) ** 2).mean(dim=(1, 3), keepdim=True)
    inv = 1.0 / torch.sqrt(var + eps)
    a = inv * ((xr - mu) * (dr - md)).mean(dim=(1, 3), keepdim=True)
    sd = ((dr - md) ** 2).mean(dim=(1, 3)).sqrt()
    return torch.stack([t.reshape(n, G) for t in (mu, inv, md, a)], -1), sd


# ------------------------------------------------------------------------------------------------ the criterion
class Groups:
    """Per-(sample, group) criterion: the worst absolute error of `got` against the float64 `ref` in a group must be
    <= max(3 x the worst error of the fp32 PyTorch yardstick in the same group, bound x the group's reference RMS).
    Collects one line per output for the profile file and the failures."""

    def __init__(self, tag):
        self.tag, self.lines, self.bad = tag, [], []

    def _judge(self, name, ek, et, floor):
        allow = torch.maximum(3.0 * et, floor)
        frac = ek / allow.clamp_min(1e-300)
        i = int(frac.argmax())
        vs = float((ek / et.clamp_min(1e-300))[et > 0].max()) if bool((et > 0).any()) else 0.0
        line = (f"{self.tag:<58} {name:<8} worst group: kernel {float(ek.flatten()[i]):.2e}  torch-fp32 "
                f"{float(et.flatten()[i]):.2e}  floor {float(floor.flatten()[i]):.2e}  used {float(frac.max()):.3f} of the "
                f"allowance; worst kernel/torch {vs:.2f}")
        self.lines.append(line)
        if not float(frac.max()) <= 1.0:
            self.bad.append(line)

    def tensor(self, name, got, ref, yard, G, bound):
        """[n][P][C] outputs, groups of C / G channels of one sample."""
        assert bool(torch.isfinite(got).all()), f"{self.tag} {name}: non-finite values"
        n, P, C = ref.shape
        gr = lambda t: t.double().reshape(n, P, G, C // G)      # noqa: E731
        ek = (gr(got) - gr(ref)).abs().amax(dim=(1, 3))
        et = (gr(yard) - gr(ref)).abs().amax(dim=(1, 3))
        self._judge(name, ek, et, bound * (gr(ref) ** 2).mean(dim=(1, 3)).sqrt())

    def per_channel(self, name, got, ref, yard, G, bound, whole=False, at_least=None):
        """[n][C] per-(sample, channel) outputs (scale / shift), or [1][C] parameter gradients: groups of C / G channels.
        whole: the floor's RMS runs over the whole row (a parameter gradient sums over every sample and pixel, a single
        channel of it can cancel to nothing; the census measures it against the vector too).
        at_least [G]: a lower limit of the RMS the floor uses.  shift = beta - mean scale is a difference that cancels to
        nothing where beta does (a group can be ONE channel); it offsets the output scale x + shift, so its error is measured
        against that output's RMS over the group, sqrt(mean(gamma^2 + beta^2)), where its own RMS is smaller."""
        assert bool(torch.isfinite(got).all()), f"{self.tag} {name}: non-finite values"
        n, C = ref.shape
        gr = lambda t: t.double().reshape(n, G, C // G)         # noqa: E731
        ek, et = (gr(got) - gr(ref)).abs().amax(2), (gr(yard) - gr(ref)).abs().amax(2)
        rms = (ref.double() ** 2).mean(1, keepdim=True).sqrt().expand(n, G) if whole else (gr(ref) ** 2).mean(2).sqrt()
        if at_least is not None:
            rms = torch.maximum(rms, at_least.double().expand(n, G))
        self._judge(name, ek, et, bound * rms)

    def stats(self, got, x64, xd64, G, bound, pivot=True):
        """The saved (mu, inv, md, a) [n][G][4].  The four entries have four units, so each is measured against its own
        magnitude in place of one RMS over the row: mu against the RMS of the group's x, inv against inv, md against the RMS
        of the group's xdot, a (= the correlation of x and xdot times the spread of xdot) against that spread.
        The kernels keep the mean relative to the group's pivot (the sample's first pixel of the group's first channel):
        entry 0 is judged as pivot + stats[0], added in double."""
        assert bool(torch.isfinite(got).all()), f"{self.tag} stats: non-finite values"
        ref, sd = stats_of(x64, xd64, G)
        got = got.double().clone()
        if pivot:
            got[..., 0] += x64[:, 0, ::x64.shape[2] // G]
        yard, _ = stats_of(x64.float(), xd64.float(), G)
        mag = torch.stack([(ref[..., 0] ** 2 + 1.0 / ref[..., 1] ** 2).sqrt(), ref[..., 1], (ref[..., 2] ** 2 + sd ** 2).sqrt(),
                           sd], -1)
        for i, nm in enumerate(("mu", "inv", "md", "a")):
            self._judge("stats." + nm, (got.double()[..., i] - ref[..., i]).abs(), (yard.double()[..., i] - ref[..., i]).abs(),
                        bound * mag[..., i])

    def finish(self):
        assert not self.bad, "outside the per-(sample, group) criterion:\n" + "\n".join(self.bad)
        return self.lines


def fair(x, G):
    """The case is a fair one: the float64 variance of every (sample, group) is exactly 0 or at least 1e-8 mean^2."""
    n, P, C = x.shape
    xr = x.double().reshape(n, P, G, C // G)
    mu = xr.mean(dim=(1, 3))
    var = ((xr - mu[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return bool(((var == 0) | (var >= 1e-8 * mu * mu)).all()) and math.isfinite(float(var.sum()))
