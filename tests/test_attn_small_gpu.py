"""The one-launch T = 16 attention kernels (csrc/attention_small_kernels.hip; ops.attention_small_*): the 4x4 level of the
16x16 U-Net, where a (sample, head) pair's logits are one 16x16 MFMA tile.

Reference: tests/test_attn_dual_paths_gpu.py's ``_reference`` (float64 torch.func.jvp + autograd on the CPU), evaluated in
float32 as well, on that file's input recipe (randn * 1.2, the first 8 rows of sample 0's q scaled by 3, seed T + C + Bp).
Each of the eight tensors o, odot, qbar, qdotbar, kbar, kdotbar, vbar, vdotbar is held to
  (i)  rel-L2 against float64 <= 2 x float32 torch's own rel-L2 on the same tensor, and never above BOUND = 2e-5;
  (ii) the worst row error <= 4 x float32 torch's worst row for that tensor and case, a row being one (sample, token, head,
       q | k | v) slice of D values and its error ||row - ref row|| / (the RMS row norm of that sample's reference tensor) —
       not the row's own norm: gradient rows cancel, and float32 torch itself reaches 1e-4 that way.
2 and 4 are conftest.parity_vs_fp64's slack / slack_worst.  No row is excluded or floored.  Every measured pair is printed;
with ATTN_SMALL_PARITY_REPORT=<path> the lines are also written there (profiles/attn_small/parity_measured.txt is that output
of one MI355X run)."""
import math
import os

import pytest
import torch

from conftest import rel_l2
from test_attn_dual_paths_gpu import BOUND, _reference
from sdeflow_light_amd import ops
from sdeflow_light_amd._lib import MsgmError

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = 16
SLACK, SLACK_WORST = 2.0, 4.0
NAMES = ("o", "odot", "qbar", "qdotbar", "kbar", "kdotbar", "vbar", "vdotbar")

# Bp, heads, D
CASES = [(1, 1, 128),      # a single pair, the driver's shape
         (5, 1, 64),       # the other single-head channel counts
         (2, 1, 32),
         (3, 2, 64),       # row stride 3C != 3D
         (7, 4, 16),       # one 16-channel tile, most heads
         (37, 1, 128),     # a pair count that is no multiple of any workgroup packing
         (300, 1, 128)]    # more workgroups than CUs
LINES = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("ATTN_SMALL_PARITY_REPORT")
    if path and LINES:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("T = 16 attention kernels vs float64 (float32 torch in brackets): rel-L2 and worst row error per tensor\n")
            f.write("\n".join(LINES) + "\n")


_CACHE = {}


def _case(Bp, H, D):
    """Inputs and the two references of one case, computed once and shared (never modified)."""
    key = (Bp, H, D)
    if key not in _CACHE:
        C = H * D
        torch.manual_seed(T + C + Bp)
        qkv = torch.randn(2 * Bp, T, 3 * C) * 1.2
        qkv[0, : T // 2, :D] *= 3.0
        g = torch.randn(2 * Bp, T, C)
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _CACHE[key] = (qkv, g, _split(_reference(qkv, g, Bp, H, D, torch.float64), Bp, H, D),
                       _split(_reference(qkv, g, Bp, H, D, torch.float32), Bp, H, D))
    return _CACHE[key]


def _split(res, Bp, H, D):
    """(o, od, xp.grad, xt.grad) -> the eight tensors as [Bp][rows][D], rows = (token, head)."""
    o, od, gp, gt = res
    out = {"o": o.reshape(Bp, T * H, D), "odot": od.reshape(Bp, T * H, D)}
    gp, gt = gp.reshape(Bp, T, H, 3, D), gt.reshape(Bp, T, H, 3, D)
    for i, nm in enumerate(("q", "k", "v")):
        out[nm + "bar"] = gp[:, :, :, i].reshape(Bp, T * H, D)
        out[nm + "dotbar"] = gt[:, :, :, i].reshape(Bp, T * H, D)
    return out


def _worst_row(x, ref):
    """max over rows of ||row - ref row|| / (RMS row norm of the sample's reference tensor)."""
    x, ref = x.double(), ref.double()
    rms = ref.pow(2).sum(-1).mean(-1, keepdim=True).sqrt()                # [Bp][1]
    return float(((x - ref).norm(dim=-1) / rms).max())


def _check(tag, got, ref64, ref32, names):
    parts, bad = [], []
    for nm in names:
        e, e32 = rel_l2(got[nm], ref64[nm]), rel_l2(ref32[nm], ref64[nm])
        w, w32 = _worst_row(got[nm], ref64[nm]), _worst_row(ref32[nm], ref64[nm])
        parts.append(f"{nm} {e:.2e} ({e32:.2e}) row {w:.2e} ({w32:.2e})")
        if not (e <= SLACK * e32 and e <= BOUND):
            bad.append((nm, "rel-L2", e, e32))
        if not w <= SLACK_WORST * w32:
            bad.append((nm, "worst row", w, w32))
    line = f"{tag}: " + " | ".join(parts)
    print(line)
    LINES.append(line)
    assert not bad, bad


def _run_dual(qkv, g, Bp, H, D):
    s2 = 1.0 / math.sqrt(D)
    att = ops.attention_small_dual_forward(qkv, Bp, T, H, D, s2)
    return att, ops.attention_small_dual_backward(qkv, g, Bp, T, H, D, s2)


@pytest.mark.parametrize("Bp,H,D", CASES)
def test_dual_forward_backward_vs_float64(Bp, H, D):
    """The eight tensors against float64 under (i) and (ii); a second forward and a second backward give the same bits."""
    C = H * D
    qkv, g, ref64, ref32 = _case(Bp, H, D)
    assert ops.attention_small_supported(T, H, D)
    dq_, dg_ = qkv.to(DEV).contiguous().view(-1), g.to(DEV).contiguous().view(-1)
    att, dqkv = _run_dual(dq_, dg_, Bp, H, D)
    att2, dqkv2 = _run_dual(dq_, dg_, Bp, H, D)
    got = _split((att.view(2, Bp, T, C)[0].cpu(), att.view(2, Bp, T, C)[1].cpu(), dqkv.view(2, Bp, T, 3 * C)[0].cpu(),
                  dqkv.view(2, Bp, T, 3 * C)[1].cpu()), Bp, H, D)
    _check(f"dual Bp={Bp} heads={H} D={D}", got, ref64, ref32, NAMES)
    assert torch.equal(att, att2), "a second forward gave other bits"
    assert torch.equal(dqkv, dqkv2), "a second backward gave other bits"


@pytest.mark.parametrize("Bp,H,D", CASES)
def test_sampler_forward_vs_float64(Bp, H, D):
    """The no-tangent entry on the primal rows: o under the same two criteria, and repeatable."""
    C = H * D
    qkv, _, ref64, ref32 = _case(Bp, H, D)
    x = qkv[:Bp].to(DEV).contiguous().view(-1)
    s2 = 1.0 / math.sqrt(D)
    out = ops.attention_small_forward(x, torch.full((Bp * T * C,), float("nan"), device=DEV), Bp, T, H, D, s2)
    out2 = ops.attention_small_forward(x, torch.empty(Bp * T * C, device=DEV), Bp, T, H, D, s2)
    _check(f"sampler Bp={Bp} heads={H} D={D}", {"o": out.view(Bp, T * H, D).cpu()}, ref64, ref32, ("o",))
    assert torch.equal(out, out2)


def test_batch_invariance():
    """Samples 0, 36 and 299 of the 300-sample case, each alone (Bp = 1, its own primal and tangent rows), give bitwise the
    rows they have in the batch: a pair's result depends neither on Bp nor on its place in the grid."""
    Bp, H, D = 300, 1, 128
    C = H * D
    qkv, g, _, _ = _case(Bp, H, D)
    att, dqkv = _run_dual(qkv.to(DEV).contiguous().view(-1), g.to(DEV).contiguous().view(-1), Bp, H, D)
    s2 = 1.0 / math.sqrt(D)
    smp = ops.attention_small_forward(qkv[:Bp].to(DEV).contiguous().view(-1), torch.empty(Bp * T * C, device=DEV), Bp, T, H, D, s2)
    att, dqkv, smp = att.view(2, Bp, T, C), dqkv.view(2, Bp, T, 3 * C), smp.view(Bp, T, C)
    for i in (0, 36, 299):
        q1 = torch.stack([qkv[i], qkv[Bp + i]]).to(DEV).contiguous().view(-1)
        g1 = torch.stack([g[i], g[Bp + i]]).to(DEV).contiguous().view(-1)
        a1, d1 = _run_dual(q1, g1, 1, H, D)
        assert torch.equal(a1.view(2, T, C), att[:, i]), i
        assert torch.equal(d1.view(2, T, 3 * C), dqkv[:, i]), i
        s1 = ops.attention_small_forward(q1[: T * 3 * C].contiguous(), torch.empty(T * C, device=DEV), 1, T, H, D, s2)
        assert torch.equal(s1.view(T, C), smp[i]), i


@pytest.mark.parametrize("Bp,H,D", [(3, 2, 64), (7, 4, 16), (37, 1, 128)])
def test_nothing_written_outside_the_documented_extent(Bp, H, D):
    """att, out and dqkv sit inside larger buffers filled with a sentinel pattern on both sides (the library entries are
    called directly: the ops wrappers allocate their outputs themselves).  The pattern survives, the extent is overwritten,
    and the results are those of the ops wrappers."""
    from sdeflow_light_amd import _lib as L
    C = H * D
    qkv, g, _, _ = _case(Bp, H, D)
    dq_, dg_ = qkv.to(DEV).contiguous().view(-1), g.to(DEV).contiguous().view(-1)
    s2 = 1.0 / math.sqrt(D)
    PAD = 4096                                                       # floats on each side (a multiple of 4: 16-byte alignment)

    def padded(n):
        big = torch.arange(n + 2 * PAD, dtype=torch.float32, device=DEV) * 0.5 - 7.0
        return big, big.clone(), big[PAD: PAD + n]
    bufs = {k: padded(n) for k, n in (("att", 2 * Bp * T * C), ("dqkv", 2 * Bp * T * 3 * C), ("out", Bp * T * C))}
    lib, st = L.lib(), L.stream()
    L.check(lib.msgm_attention_small_dual_forward(L.ptr(dq_), L.ptr(bufs["att"][2]), Bp, T, H, D, s2, st), "dual forward")
    L.check(lib.msgm_attention_small_dual_backward(L.ptr(dq_), L.ptr(dg_), L.ptr(bufs["dqkv"][2]), Bp, T, H, D, s2, st), "dual backward")
    L.check(lib.msgm_attention_small_forward(L.ptr(dq_), L.ptr(bufs["out"][2]), Bp, T, H, D, s2, st), "forward")
    for k, (big, before, mid) in bufs.items():
        n = mid.numel()
        assert torch.equal(big[:PAD], before[:PAD]) and torch.equal(big[PAD + n:], before[PAD + n:]), k
    att0, dqkv0 = _run_dual(dq_, dg_, Bp, H, D)
    assert torch.equal(bufs["att"][2], att0) and torch.equal(bufs["dqkv"][2], dqkv0)
    assert torch.equal(bufs["out"][2], att0[: Bp * T * C])


def test_predicates_and_refusals():
    for D in (16, 32, 64, 128):
        for h in (1, 4, 64):
            assert ops.attention_small_supported(16, h, D), (h, D)
    for t in (4, 9, 32, 36, 64):
        assert not ops.attention_small_supported(t, 1, 64), t
    for D in (8, 48, 256):
        assert not ops.attention_small_supported(16, 1, D), D
    assert not ops.attention_small_supported(16, 0, 64) and not ops.attention_small_supported(16, 65, 64)
    # the existing predicates do not move
    assert not ops.attention_supported(16, 64) and not ops.attention_mh_supported(16, 2, 64)
    assert not ops.attention_dual_supported(16, 128) and not ops.attention_dual_mh_supported(16, 2, 64)
    for t, h, D in ((32, 1, 64), (16, 1, 48), (16, 65, 16), (9, 2, 32)):
        n = 2 * t * 3 * h * D
        x, gg = torch.zeros(n, device=DEV), torch.zeros(n // 3, device=DEV)
        with pytest.raises(MsgmError):
            ops.attention_small_forward(x, torch.zeros(n // 3, device=DEV), 2, t, h, D, 1.0)
        with pytest.raises(MsgmError):
            ops.attention_small_dual_forward(x, 1, t, h, D, 1.0)
        with pytest.raises(MsgmError):
            ops.attention_small_dual_backward(x, gg, 1, t, h, D, 1.0)
    x, gg = torch.zeros(2 * 16 * 192), torch.zeros(2 * 16 * 64)
    with pytest.raises(MsgmError):
        ops.attention_small_forward(x, torch.zeros(2 * 16 * 64), 2, 16, 1, 64, 0.125)
    with pytest.raises(MsgmError):
        ops.attention_small_dual_forward(x, 1, 16, 1, 64, 0.125)
    with pytest.raises(MsgmError):
        ops.attention_small_dual_backward(x, gg, 1, 16, 1, 64, 0.125)
    with pytest.raises(MsgmError):                                       # too small a buffer is refused before the launch
        ops.attention_small_dual_backward(torch.zeros(100, device=DEV), torch.zeros(100, device=DEV), 1, 16, 1, 64, 0.125)
