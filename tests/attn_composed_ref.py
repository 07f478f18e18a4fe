"""Float64 restatement of the composed attention route of the 2-D U-Net and of its glue kernels, written from the C ABI
comments of include/msgm_hip.h (msgm_bmm / msgm_bmm_dual, msgm_softmax_dual_*, msgm_timestep_embedding[_dual],
msgm_normalize_dual, msgm_flat_to_image / msgm_image_to_flat, msgm_sum2x2).  Plain torch, nothing imported from the package.

Every function returns (value, magnitude) pairs: the value in `dtype` (float64 by default) and a per-element magnitude
such that a float32 evaluation in ANY order stays within c * 2^-24 * magnitude of the float64 value.

  * batched GEMM: the magnitude is |alpha| (sum_k |a||b| + sum_k |a2||b2|) + |base| and the bound is a-priori:
    (K_total + 2) 2^-24 magnitude, K_total = the number of products summed (both pairs).  K_total - 1 additions and one
    rounding per product (none with FMA) give the classic gamma_K; the two extra units pay for alpha and the base.
  * everything else: c = 4 x MEASURED[family] (floored at 4), MEASURED = this restatement evaluated in float32 on the
    CPU against float64 over the case lists below (tests/test_attn_composed_ref.py recomputes it).  The factor 4 pays
    for the device's expf / logf / sinf / cosf / reciprocals (1-2 ulp from libm) and the wave-tree summation order.

The case lists of tests/test_composed_attention_gpu.py live here (BMM_CASES, SOFTMAX_T, ...), so the CPU test can
measure over exactly those cases and prove with bmm_path() that the GEMM list reaches every kernel instantiation.
"""
import math

import numpy as np
import torch

F64 = torch.float64
EPS32 = 2.0 ** -24
TINY = 2.0 ** -126 / EPS32          # magnitude floor: a float32 result below the smallest normal may be flushed to zero
BATCH = 3


def c32(v):
    """The float32 the C ABI receives for a Python scalar."""
    return float(np.float32(v))


MEASURED = {
    # family: worst ratio of the float32 restatement against float64 (torch CPU) over the case lists
    "softmax_fwd": 4.682,     # P and Pdot: the exp argument, exp, the row sum of up to 144 terms and the division
    "softmax_bwd": 4.003,     # Wbar and Wdotbar: three row sums
    "temb": 0.571,            # cos / sin of t f_j  (c is floored at 4)
    "temb_dual": 0.784,       # ... and their tangents  (floored at 4)
    "normalize": 3.310,       # x / r, its tangent, log r, rdot / r: row sums of up to 576 terms
}


def c_of(family):
    return max(4.0, 4.0 * MEASURED[family])


def gemm_c(case):
    """(K_total + 2): the a-priori factor of the GEMM bound."""
    return case["K"] * (2 if case.get("pair2") else 1) + 2


def ratio(y, ref, mag):
    """Worst |y - ref| / (2^-24 mag) over the elements (0/0 counts as 0: an exact zero must be met exactly)."""
    d = (y.double() - ref.double()).abs()
    m = mag.double() * EPS32
    r = torch.where(d == 0, torch.zeros_like(d), d / m)
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------ batched GEMM
def span(off, s, dims):
    """One past the last element an operand with offset `off`, strides s and extents dims touches."""
    return off + sum((d - 1) * st for d, st in zip(dims, s)) + 1


def bmm_strided(A, a_off, B, b_off, C, c_off, M, N, K, batch, sA, sB, sC, alpha=1.0, accumulate=False, pair2=None, third=None):
    """msgm_bmm_dual on flat buffers with element strides sA = (batch, i, k), sB = (batch, k, j), sC = (batch, i, j):
         C[b](i,j)  (+)= alpha (sum_k A[b](i,k) B[b](k,j) + sum_k A2[b](i,k) B2[b](k,j))     pair2 = (A2, a2_off, B2, b2_off)
         C3[b](i,j) (+)= alpha  sum_k A[b](i,k) B3[b](k,j)                                    third = (B3, b3_off, C3, c3_off)
    Returns [(Cnew, mag)] or [(Cnew, mag), (C3new, mag3)]: Cnew = the whole flat buffer C in float64 after the call (C3new
    likewise; when C3 is the same tensor as C both outputs are in both), mag (batch, M, N) as described in the module text."""
    al = c32(alpha)
    v = lambda X, off, s, dims: X.as_strided(dims, s, off).double()
    Av, Bv = v(A, a_off, sA, (batch, M, K)), v(B, b_off, sB, (batch, K, N))
    val, mag = Av @ Bv, Av.abs() @ Bv.abs()
    if pair2 is not None:
        A2, a2_off, B2, b2_off = pair2
        A2v, B2v = v(A2, a2_off, sA, (batch, M, K)), v(B2, b2_off, sB, (batch, K, N))
        val, mag = val + A2v @ B2v, mag + A2v.abs() @ B2v.abs()
    outs = [(C, c_off, al * val, abs(al) * mag)]
    if third is not None:
        B3, b3_off, C3, c3_off = third
        B3v = v(B3, b3_off, sB, (batch, K, N))
        outs.append((C3, c3_off, al * (Av @ B3v), abs(al) * (Av.abs() @ B3v.abs())))
    new = {}
    res = []
    for X, off, val, mag in outs:
        buf = new.setdefault(id(X), X.double().clone())
        view = buf.as_strided((batch, M, N), sC, off)
        if accumulate:
            base = X.as_strided((batch, M, N), sC, off).double()
            val, mag = val + base, mag + base.abs()
        view.copy_(val)
        res.append((buf, mag))
    return res


def bmm_path(M, N, K, sA, sB, sC, addr, pair2=False, third=False):
    """The kernel instantiation msgm_bmm_dual launches, restated from its dispatch: "slow" / "slow_dual" (K % 16 != 0),
    "lds<AM,BM,dual>" (AM, BM in KV | RV) or "reg<avec,bvec,dual>"; "unsupported" for a second output on an output layout
    other than sCj == 1, sCi != 1.  addr = byte addresses {"A", "B", "A2", "B2", "B3"} (absent / None = NULL).
    Returns (label, flags): flags = {"swap", "cvec", "tail"} — the host operand swap, the 16-byte store path of the
    epilogue for C, and whether a store quad straddles the end of the kernel's M (the i + 3 >= M branch)."""
    (sAb, sAi, sAk), (sBb, sBk, sBj), (sCb, sCi, sCj) = sA, sB, sC
    if third and not (sCj == 1 and sCi != 1):
        return "unsupported", {}
    a, b, a2, b2, a3 = (addr.get(k) for k in ("A", "B", "A2", "B2", "B3"))
    if not pair2:
        a2 = b2 = None
    if not third:
        a3 = None
    swap = sCj == 1 and sCi != 1
    if swap:
        a, b, a2, b2 = b, a, b2, a2
        M, N = N, M
        (sAb, sAi, sAk), (sBb, sBk, sBj) = (sBb, sBj, sBk), (sAb, sAk, sAi)
        sCi, sCj = sCj, sCi
    al16 = lambda p: p is None or p % 16 == 0
    flags = {"swap": swap, "tail": M % 4 != 0}
    flags["cvec"] = sCi == 1 and sCj % 4 == 0 and sCb % 4 == 0 and al16(addr.get("C")) and (not third or al16(addr.get("C3")))
    dual = a3 is not None
    if K % 16:
        flags["cvec"] = False
        return ("slow_dual" if dual else "slow"), flags

    def mode(sRow, sK, sB_):
        if sK == 1 and sRow % 4 == 0 and sB_ % 4 == 0:
            return "KV"
        if sRow == 1 and sK % 4 == 0 and sB_ % 4 == 0:
            return "RV"
        return None
    am, bm = mode(sAi, sAk, sAb), mode(sBj, sBk, sBb)
    if am and bm and K % 32 == 0 and M % 4 == 0 and N % 4 == 0 and all(al16(p) for p in (a, a2, b, b2, a3)):
        return f"lds<{am},{bm},{int(dual)}>", flags
    avec = sAk == 1 and sAi % 4 == 0 and sAb % 4 == 0 and al16(a) and al16(a2)
    bvec = sBk == 1 and sBj % 4 == 0 and sBb % 4 == 0 and al16(b) and al16(b2)
    if dual:
        avec = avec and al16(a3)
    return f"reg<{int(avec)},{int(bvec)},{int(dual)}>", flags


ALL_BMM_CLASSES = (["slow", "slow_dual"] + [f"lds<{a},{b},{d}>" for a in ("KV", "RV") for b in ("KV", "RV") for d in (0, 1)]
                   + [f"reg<{a},{b},{d}>" for a in (0, 1) for b in (0, 1) for d in (0, 1)])


def _case(name, M, N, K, sA, sB, sC, a_off=0, b_off=0, c_off=8, alpha=1.0, acc=False, pair2=False, third=False, c3_gap=8):
    """One GEMM case on buffers of its own: A / A2 share strides and offset (two tensors), B / B2 / B3 likewise; C and C3
    lie in ONE wide buffer, C3 behind C with `c3_gap` sentinel elements between them."""
    c3_off = span(c_off, sC, (BATCH, M, N)) + c3_gap
    c3_off += (c_off - c3_off) % 4                       # the same 16-byte phase as C
    return dict(name=name, M=M, N=N, K=K, batch=BATCH, sA=tuple(sA), sB=tuple(sB), sC=tuple(sC), a_off=a_off, a2_off=a_off,
                b_off=b_off, b2_off=b_off, b3_off=b_off, c_off=c_off, c3_off=c3_off, alpha=alpha, acc=acc, pair2=pair2, third=third)


def _att(form, T, D, ld=None, **kw):
    """The attention layouts on a fused qkv tensor [b][T][ld] (ld = 3 D unless given), probabilities [b][T][T], attention
    output / cotangent g [b][T][D]:   qkT: S = q k^T (NT)     Pv: a = P v (NN)     PTg: vbar = P^T g (TN)     gvT: Pbar = g v^T"""
    ld = ld or 3 * D
    sq, skT, sP, sPt, sa = (T * ld, ld, 1), (T * ld, 1, ld), (T * T, T, 1), (T * T, 1, T), (T * D, D, 1)
    M, N, K, sA, sB, sC = {"qkT": (T, T, D, sq, skT, sP), "Pv": (T, D, T, sP, sq, sa), "PTg": (T, D, T, sPt, sa, sq),
                           "gvT": (T, T, D, sa, skT, sP)}[form]
    opt = " ".join(f"{k}={v}" for k, v in kw.items())
    return _case(f"{form} T={T} D={D}" + (f" ld={ld}" if ld != 3 * D else "") + (" " + opt if opt else ""), M, N, K, sA, sB, sC, **kw)


def _bmm_cases():
    P2, P3 = dict(pair2=True), dict(pair2=True, third=True)
    c = []
    # k_bmm_slow: K = T in {9, 25, 36, 100}; the kernel's 32-tiles against 36 / 100 / 64 / 128 rows and columns
    c += [_att("Pv", 36, 64), _att("Pv", 36, 128, **P3), _att("PTg", 100, 64, alpha=0.125, **P3),
          _att("Pv", 25, 64, acc=True, pair2=True), _att("Pv", 9, 128, alpha=0.0883883, acc=True, **P3),
          _att("PTg", 100, 128, acc=True), _att("PTg", 25, 128, **P3), _att("Pv", 100, 64, third=True),
          _att("PTg", 9, 64, pair2=True), _att("PTg", 36, 64, acc=True, third=True)]
    # k_bmm_lds: ragged 64-tiles with M = N in {36, 100, 144} (K = D), K = T = 160 for the P v / P^T g forms
    c += [_att("qkT", 36, 64, alpha=0.125), _att("qkT", 100, 128, alpha=0.0883883, pair2=True), _att("qkT", 144, 64, **P3),
          _att("gvT", 100, 64, pair2=True), _att("gvT", 36, 128, acc=True, third=True),
          _att("Pv", 160, 64), _att("Pv", 160, 128, **P3), _att("PTg", 160, 64, acc=True), _att("PTg", 160, 128, alpha=0.0883883, **P3)]
    # lds<KV,RV>: A given transposed (i contiguous), B given as X[j][k] (k contiguous) — no attention product, built all the same
    for (M, N, K, kw) in ((100, 36, 64, dict(alpha=0.5)), (36, 144, 128, P3), (144, 100, 64, dict(acc=True, pair2=True))):
        c.append(_case(f"AtBt M={M} N={N} K={K} " + " ".join(f"{k}={v}" for k, v in kw.items()),
                       M, N, K, (K * M, 1, M), (N * K, 1, K), (M * N, N, 1), **kw))
    # k_bmm (register-direct): K % 32 != 0 (K = T = 144), M or N not divisible by 4 (T = 25, 9 with K = D)
    c += [_att("Pv", 144, 64), _att("Pv", 144, 128, **P3), _att("PTg", 144, 64, acc=True, **P3),
          _att("qkT", 25, 64, alpha=0.125, pair2=True), _att("qkT", 9, 128, **P3), _att("gvT", 25, 128, acc=True)]
    # a base that breaks the 16-byte alignment turns avec / bvec off one at a time (a_off: the kernel's B after the swap)
    for kw in ({}, P3):
        c += [_att("qkT", 36, 64, b_off=1, **kw), _att("qkT", 36, 64, a_off=1, **kw), _att("qkT", 36, 64, a_off=2, b_off=3, **kw)]
    c += [_att("qkT", 36, 64, c_off=9, **P3),                         # C, C3 misaligned: scalar stores
          _att("qkT", 36, 64, ld=193, pair2=True),                      # operand row stride % 4 != 0: no vector loads at all
          _att("qkT", 100, 64, ld=194, **P3)]
    # C row stride % 4 != 0 (37), and the i + 3 >= M tail inside a vector-store tile: 25 columns in rows of pitch 28
    c.append(_case("qkT T=36 D=64 C pitch 37", 36, 36, 64, (36 * 192, 192, 1), (36 * 192, 1, 192), (36 * 37, 37, 1), pair2=True))
    c.append(_case("tail M=36 N=25 D=64 C pitch 28", 36, 25, 64, (36 * 192, 192, 1), (25 * 192, 1, 192), (36 * 28, 28, 1), **P3))
    c.append(_case("tail M=36 N=25 D=64 C pitch 28 c_off=9", 36, 25, 64, (36 * 192, 192, 1), (25 * 192, 1, 192), (36 * 28, 28, 1), c_off=9, pair2=True))
    c.append(_case("tail M=100 N=9 D=128 C pitch 12 acc", 100, 9, 128, (100 * 384, 384, 1), (9 * 384, 1, 384), (100 * 12, 12, 1), acc=True))
    # outputs that are not contiguous along j: no host swap (column-major C; C with no unit stride)
    c.append(_case("colmajor C M=36 N=100 K=64", 36, 100, 64, (36 * 192, 192, 1), (100 * 192, 1, 192), (3600, 1, 36), pair2=True))
    c.append(_case("C stride 2 M=25 N=36 K=36", 25, 36, 36, (25 * 36, 36, 1), (36 * 36, 36, 1), (25 * 72, 72, 2), acc=True))
    return c


BMM_CASES = _bmm_cases()
# a second output on an output that is not contiguous along j is refused by design (MSGM_E_UNSUPPORTED): pinned, not run
BMM_REFUSED = _case("third on column-major C", 36, 100, 64, (36 * 192, 192, 1), (100 * 192, 1, 192), (3600, 1, 36), third=True)


def bmm_buffers(case, seed=0, pad=8):
    """Float32 CPU operands of a case: {"A", "B", "A2", "B2", "B3", "C"}; each input buffer is exactly as long as its span
    (+ the offset), C is the wide output buffer (pad elements behind the last output) holding the accumulate base."""
    g = torch.Generator().manual_seed(seed)
    M, N, K, b = case["M"], case["N"], case["K"], case["batch"]
    sp = lambda key, s, dims: span(case[key], case[s], dims)
    nA, nB = sp("a_off", "sA", (b, M, K)), sp("b_off", "sB", (b, K, N))
    nC = max(sp("c_off", "sC", (b, M, N)), sp("c3_off", "sC", (b, M, N)) if case["third"] else 0) + pad
    r = lambda n: torch.randn(n, generator=g)
    d = {"A": r(nA), "B": r(nB), "A2": r(sp("a2_off", "sA", (b, M, K))) if case["pair2"] else None,
         "B2": r(sp("b2_off", "sB", (b, K, N))) if case["pair2"] else None,
         "B3": r(sp("b3_off", "sB", (b, K, N))) if case["third"] else None, "C": r(nC)}
    return d


def bmm_case_path(case, base=None):
    """bmm_path of a case; base = {"A": byte address of the buffer, ...} (16-byte aligned buffers when omitted)."""
    base = base or {}
    ad = lambda k, off: base.get(k, 0) + 4 * off
    addr = {"A": ad("A", case["a_off"]), "B": ad("B", case["b_off"]), "A2": ad("A2", case["a2_off"]), "B2": ad("B2", case["b2_off"]),
            "B3": ad("B3", case["b3_off"]), "C": ad("C", case["c_off"]), "C3": ad("C", case["c3_off"])}
    return bmm_path(case["M"], case["N"], case["K"], case["sA"], case["sB"], case["sC"], addr, case["pair2"], case["third"])


def bmm_case_ref(case, d):
    """bmm_strided on the buffers of bmm_buffers (any device)."""
    p2 = (d["A2"], case["a2_off"], d["B2"], case["b2_off"]) if case["pair2"] else None
    th = (d["B3"], case["b3_off"], d["C"], case["c3_off"]) if case["third"] else None
    return bmm_strided(d["A"], case["a_off"], d["B"], case["b_off"], d["C"], case["c_off"], case["M"], case["N"], case["K"],
                       case["batch"], case["sA"], case["sB"], case["sC"], case["alpha"], case["acc"], p2, th)


# ------------------------------------------------------------------------------------------------ dual softmax
SOFTMAX_T = (9, 25, 36, 100, 144)


def softmax_inputs(T, seed=0, rows=None):
    """(S, Wd, Pb, Pdb) float32 (rows, T), rows = 3 T (75 at T = 25, 27 at T = 9: not multiples of the 4 rows of a
    workgroup).  Row 0: logits spread over +-60 (exp underflows to 0 for most entries); row 1: constant; row 2: one
    dominant entry; row 3: two equal maxima; the rest N(0, 3^2)."""
    g = torch.Generator().manual_seed(1000 + T + seed)
    rows = rows or BATCH * T
    S = torch.randn(rows, T, generator=g) * 3
    S[0] = torch.linspace(-60, 60, T)[torch.randperm(T, generator=g)]
    S[1] = 1.75
    S[2, T // 2] += 40.0
    S[3, 0] = S[3, T - 1] = 11.0
    Wd, Pb, Pdb = (torch.randn(rows, T, generator=g) for _ in range(3))
    return S, Wd, Pb, Pdb


def softmax_dual_forward(S, Wd=None, dtype=F64):
    """P = softmax(S) over the last axis (row max subtracted); with Wd: Pd = P (Wd - sum_j P Wd).
    Magnitudes: the float32 argument s - max carries a rounding of 2^-24 |s - max|, which exp turns into a RELATIVE
    error of that size, so P's scale is P (1 + |s - max|), not P; Pd inherits it through both factors:
    P (1 + |s - max|) (|Wd| + |r|) + P sum_j P (1 + |s - max|) |Wd|.  TINY is added: results below 2^-126 may flush."""
    s = S.to(dtype)
    d = s - s.max(dim=-1, keepdim=True).values
    e = torch.exp(d)
    P = e / e.sum(dim=-1, keepdim=True)
    Pm = P.double() * (1 + d.double().abs())
    if Wd is None:
        return [(P, Pm + TINY)]
    wd = Wd.to(dtype)
    r = (P * wd).sum(dim=-1, keepdim=True)
    Pd = P * (wd - r)
    rmag = (Pm * wd.double().abs()).sum(dim=-1, keepdim=True)
    return [(P, Pm + TINY), (Pd, Pm * (wd.double().abs() + r.double().abs()) + P.double() * rmag + TINY)]


def softmax_dual_backward(P, Wd, Pb, Pdb, dtype=F64):
    """Cotangents (Pb, Pdb) of (P, Pd) -> cotangents (Wbar, Wdbar) of (S, Wd), as documented above k_softmax_dual_bwd:
         r = sum P Wd, m = sum P Pdb, pt = Pb + Pdb (Wd - r) - Wd m, Wbar = P (pt - sum P pt), Wdbar = P (Pdb - m).
    P is an input here, so the magnitudes are the plain sums of absolute values of every term."""
    p, wd, pb, pdb = (x.to(dtype) for x in (P, Wd, Pb, Pdb))
    sm = lambda x: x.sum(dim=-1, keepdim=True)
    r, m = sm(p * wd), sm(p * pdb)
    pt = pb + pdb * (wd - r) - wd * m
    W, Wdb = p * (pt - sm(p * pt)), p * (pdb - m)
    pa, wa, pba, pdba = (x.double().abs() for x in (P, Wd, Pb, Pdb))
    rm, mm = sm(pa * wa), sm(pa * pdba)
    ptm = pba + pdba * (wa + rm) + wa * mm
    return [(W, pa * (ptm + sm(pa * ptm)) + TINY), (Wdb, pa * (pdba + mm) + TINY)]


# ------------------------------------------------------------------------------------------------ glue
TEMB_DIMS = (32, 33, 128)
NORMALIZE_CASES = [(Bp, n) for n in (9, 144, 400, 576) for Bp in (1, 3, 5)]
IMAGE_CASES = [(2, 1, 6, 4), (3, 3, 6, 4), (1, 1, 5, 12), (2, 3, 5, 12)]           # (B, C, H, W), H != W
SUM2X2_CASES = [(2, 3, 5, 3), (1, 6, 2, 32), (3, 1, 7, 1)]                         # (N, H, W, C) of the OUTPUT, H != W


def temb_inputs(Bp=5, seed=0):
    """sde times in [t_epsilon, 1] for the plain embedding; [log-radius ; its tangent] (2 Bp) for the dual: the nets pass
    log(|x| + eps) of a flat image, |x| between 1e-2 and a few hundred."""
    g = torch.Generator().manual_seed(77 + seed)
    t = torch.cat([torch.tensor([1e-3, 1.0]), torch.rand(Bp, generator=g)])
    logr = torch.cat([torch.tensor([-4.6, 6.2]), torch.rand(Bp - 2, generator=g) * 8 - 3])
    return t, torch.cat([logr, torch.randn(Bp, generator=g)])


def timestep_embedding(t, dim, max_period=10000.0, dtype=F64, tdot=None):
    """emb[b] = [cos(t_b f_j) | sin(t_b f_j) | 0 if dim is odd], f_j = exp(-ln(max_period) j / half), half = dim // 2;
    with tdot also the tangent [-f sin(t f) tdot | f cos(t f) tdot | 0].
    Magnitude: f carries a relative error of 2^-24 (1 + ln(max_period) j / half) (the rounded exp argument), the argument
    t f that and one more, and cos / sin turn the argument's ABSOLUTE error into their own: 1 + |t f| (2 + |ln f|)."""
    half = dim // 2
    lf = -(math.log(c32(max_period)) * torch.arange(half, dtype=F64) / half)
    f = torch.exp(lf.to(dtype))
    arg = t.to(dtype).reshape(-1, 1) * f
    pad = [torch.zeros(arg.shape[0], dim - 2 * half, dtype=dtype)]
    c, s = torch.cos(arg), torch.sin(arg)
    amag = arg.double().abs() * (2 + lf.abs())
    emb = torch.cat([c, s] + pad, dim=1)
    mag = torch.cat([1 + amag, 1 + amag] + [pad[0].double()], dim=1)
    if tdot is None:
        return [(emb, mag)]
    td = tdot.to(dtype).reshape(-1, 1)
    embd = torch.cat([-f * s * td, f * c * td] + pad, dim=1)
    dm = (f.double() * td.double().abs()) * (1 + lf.abs() + amag)
    return [(emb, mag), (embd, torch.cat([dm, dm] + [pad[0].double()], dim=1))]


def normalize_inputs(Bp, n, seed=0):
    g = torch.Generator().manual_seed(31 * n + Bp + seed)
    x = torch.randn(2 * Bp, n, generator=g) * 3
    return x


def normalize_dual(x, Bp, dual, scale, eps=1e-6, dtype=F64):
    """x (2 Bp, n) = [x ; xdot] (or (Bp, n) without dual): r = |x| + eps, out = scale x / r, logr = log r and the tangents
    rdot = x.xdot / |x|, outdot = scale (xdot / r - x rdot / r^2), logr_dot = rdot / r.  Returns [(out, mag), (logr, mag)]
    stacked like the kernel's outputs.  log r: a relative error of r is an absolute error of its logarithm, hence 1 + |log r|."""
    sc, ep = c32(scale), c32(eps)
    X = x.to(dtype)
    xp = X[:Bp]
    nr = (xp * xp).sum(dim=1, keepdim=True).sqrt()
    r = nr + ep
    out, lg = sc * (xp / r), torch.log(r)
    om, lm = out.double().abs(), 1 + lg.double().abs()
    if not dual:
        return [(out, om), (lg.reshape(-1), lm.reshape(-1))]
    xt = X[Bp:]
    rdot = (xp * xt).sum(dim=1, keepdim=True) / nr
    outd = sc * (xt / r - xp * rdot / (r * r))
    rdm = (xp * xt).double().abs().sum(dim=1, keepdim=True) / nr.double()
    odm = abs(sc) * (xt.double().abs() / r.double() + xp.double().abs() * rdm / (r * r).double())
    return [(torch.cat([out, outd]), torch.cat([om, odm])),
            (torch.cat([lg, rdot / r]).reshape(-1), torch.cat([lm, rdm / r.double()]).reshape(-1))]


def flat_to_image(flat, B, C, H, W, forder, scale):
    """float32, exact: flat (B, C H W) channel-major with per-channel order 'C' (h W + w) or 'F' (w H + h) -> channels-last
    [B][H][W][C] times float32(scale)."""
    x = flat.float().reshape(B, C, W, H).transpose(2, 3) if forder else flat.float().reshape(B, C, H, W)
    return (x.permute(0, 2, 3, 1) * torch.tensor(scale, dtype=torch.float32)).contiguous()


def image_to_flat(img, B, C, H, W, forder, scale):
    """float32, exact: the inverse layout map, times float32(scale)."""
    x = img.float().reshape(B, H, W, C).permute(0, 3, 1, 2) * torch.tensor(scale, dtype=torch.float32)
    return (x.transpose(2, 3) if forder else x).contiguous().reshape(B, C * H * W)


def sum2x2(x, N, H, W, C):
    """float32, exact: out[n][h][w][c] = (p00 + p01) + (p10 + p11) of the 2x2 block of x [N][2H][2W][C]."""
    v = x.float().reshape(N, H, 2, W, 2, C)
    return ((v[:, :, 0, :, 0] + v[:, :, 0, :, 1]) + (v[:, :, 1, :, 0] + v[:, :, 1, :, 1])).contiguous()
