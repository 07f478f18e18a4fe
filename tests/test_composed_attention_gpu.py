"""Float64 parity of the composed attention route — msgm_bmm_dual, msgm_softmax_dual_* — and of the layout / embedding glue
of csrc/unet2d_kernels.hip, at the shapes a 2-D U-Net sees when its image side is not a power of two (T = 9, 25, 36, 100,
144: no fused attention kernel; n = 144, 400, 576: rows that are no multiple of 64 lanes).

Every output is compared PER ELEMENT with the float64 restatement of tests/attn_composed_ref.py:
|kernel - ref64| <= c 2^-24 magnitude.  GEMM: c = K_total + 2, a-priori (any summation order, with or without FMA).
Softmax / embedding / normalize: c = 4 x attn_composed_ref.MEASURED[family] (the CPU float32 evaluation of the restatement,
guarded by tests/test_attn_composed_ref.py), floored at 4.  Layout maps and sum2x2 are bit-exact.  Every case runs on
caller-owned buffers: outputs are NaN before the call and finite after it over their extent, they are slices of a wider
tensor whose other elements must keep their bits, and a second run must give the same bits.

Case -> kernel (attn_composed_ref.bmm_path restates msgm_bmm_dual's dispatch; test_attn_composed_ref.py proves the list
reaches all 18 instantiations, this file asserts the label again with the real device addresses):

  test / case (attn_composed_ref.BMM_CASES)        kernel                        what is new in it
  -----------------------------------------------  ----------------------------  ---------------------------------------------
  bmm Pv | PTg, T = K in 9 25 36 100               k_bmm_slow<false|true>        K % 16 != 0; 32-tiles against 9..128 rows;
                                                                                 pair2, accumulate, transposed A, the second
                                                                                 output (refused before this test existed)
  bmm "C stride 2"                                 k_bmm_slow<false>             no host swap, output without a unit stride
  bmm qkT | gvT, T in 36 100 144, K = D            k_bmm_lds<KV,KV,dual>         ragged 64-tiles, M = N % 4 == 0
  bmm Pv | PTg, T = K = 160                        k_bmm_lds<RV,KV|RV,dual>      ragged row tile, transposed operands
  bmm AtBt                                         k_bmm_lds<KV,RV,dual>         the one mode pair attention does not use
  bmm "C pitch 37", c_off = 9, "colmajor C"        k_bmm_lds<KV,KV,*>            scalar epilogue (stride / base); no swap
  bmm Pv | PTg, T = K = 144                        k_bmm<2,2,0,b,dual>           K % 32 != 0
  bmm qkT | gvT, T in 25 9                         k_bmm<2,2,1,1,dual>           M, N % 4 != 0, C row stride % 4 != 0
  bmm qkT a_off | b_off odd, ld = 193 | 194        k_bmm<2,2,a,b,dual>           avec / bvec turned off one at a time by a base,
                                                                                 both by a row stride
  bmm "tail ..." C pitch 28 | 12                   k_bmm<2,2,1,1,dual>           16-byte stores with the i + 3 >= M quad
  bmm "tail ..." c_off = 9                         k_bmm<2,2,1,1,0>              the same with C's base misaligned
  bmm_second_output_refused_on_other_layouts       (host)                        MSGM_E_UNSUPPORTED, message pinned
  softmax T in 9 25 36 100 144                     k_softmax_dual_fwd / _bwd     3 T rows (27, 75: ragged last workgroup); rows
                                                                                 with +-60 logits, constant, one dominant entry
  timestep_embedding dim 32 | 33 | 128             k_timestep_embedding[_dual]   the zero-pad column; sde time / log-radius
  normalize n 9 144 400 576, Bp 1 3 5              k_normalize_dual              rows shorter than / no multiple of 64 lanes
  layout (6,4) (5,12), C 1 | 3, both orders        k_flat_to_cl, k_cl_to_flat    H != W; bit-exact
  sum2x2                                           k_sum2x2                      H != W; (p00 + p01) + (p10 + p11) bit-exact
"""
import math
import os

import pytest
import torch

import attn_composed_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}                    # (family, class) -> worst kernel ratio seen (written to $ODD_SIZE_PARITY_REPORT, for information only)
SENTINEL = -12345.678


def write_report(path):
    with open(path, "a") as f:
        f.write("worst |kernel - ref64| / (2^-24 magnitude) per family and kernel class on the MI355X (bound c in brackets)\n")
        for k in sorted(WORST):
            f.write(f"{k[0]:12s} {k[1]:14s} {WORST[k][0]:8.3f}  [{WORST[k][1]:.2f}]  {WORST[k][2]}\n")


@pytest.fixture(scope="module")
def ops():
    from sdeflow_light_amd import ops as _ops
    _ops.lib()
    yield _ops
    path = os.environ.get("ODD_SIZE_PARITY_REPORT")
    if path:
        write_report(path)


@pytest.fixture(scope="module")
def L():
    from sdeflow_light_amd import _lib
    return _lib


def _call(L, name, *args):
    L.check(getattr(L.lib(), name)(*args, L.stream()), name)


def note(family, cls, r, c, what):
    if r > WORST.get((family, cls), (-1.0,))[0]:
        WORST[(family, cls)] = (r, c, what)
    print(f"{what}: {family} {cls} ratio {r:.3f} (c = {c:.2f})")


def bits(t):
    return t.contiguous().view(torch.int32)


def wide(n, off, pad=12):
    """A sentinel-filled buffer with a NaN window of n elements at `off`: (buffer, window view, copy of the buffer)."""
    buf = torch.full((off + n + pad,), SENTINEL, device=DEV)
    win = buf[off:off + n]
    win.fill_(float("nan"))
    return buf, win, buf.clone()


def outside_unchanged(buf, before, off, n, what):
    a, b = bits(buf), bits(before)
    assert torch.equal(a[:off], b[:off]) and torch.equal(a[off + n:], b[off + n:]), f"{what}: wrote outside its output"


def check(family, cls, y, ref_mag, what, c=None):
    """finite everywhere, then per element within c 2^-24 magnitude of the float64 reference"""
    ref, mag = ref_mag
    assert y.numel() == ref.numel(), what
    y = y.reshape(ref.shape).cpu()
    assert bool(torch.isfinite(y).all()), f"{what}: non-finite output (an unwritten NaN pre-fill?)"
    c = R.c_of(family) if c is None else c
    r = R.ratio(y, ref.cpu(), mag.cpu())
    note(family, cls, r, c, what)
    assert r <= c, (what, family, r, c)


# ------------------------------------------------------------------------------------------------ batched GEMM
def run_bmm_case(ops, case, seed=0, expect=None):
    """One msgm_bmm_dual call through ops.bmm on the case's buffers, twice; returns (kernel class, the output buffer)."""
    what = "bmm " + case["name"]
    M, N, b, sC = case["M"], case["N"], case["batch"], case["sC"]
    d = R.bmm_buffers(case, seed)
    refs = R.bmm_case_ref(case, d)                       # float64 on the CPU: the accumulate base is d["C"] itself
    offs = [case["c_off"]] + ([case["c3_off"]] if case["third"] else [])
    g = {k: (v.to(DEV) if v is not None else None) for k, v in d.items()}
    label, flags = R.bmm_case_path(case, {k: v.data_ptr() for k, v in g.items() if v is not None})
    assert all(v is None or v.data_ptr() % 16 == 0 for v in g.values())
    assert (label, flags) == R.bmm_case_path(case) and (expect is None or label == expect), (what, label)
    runs = []
    for _ in range(2):
        Cg = g["C"].clone()
        if not case["acc"]:
            for off in offs:
                Cg.as_strided((b, M, N), sC, off).fill_(float("nan"))
        p2 = (g["A2"], case["a2_off"], g["B2"], case["b2_off"]) if case["pair2"] else None
        th = (g["B3"], case["b3_off"], Cg, case["c3_off"]) if case["third"] else None
        ops.bmm(g["A"], case["a_off"], g["B"], case["b_off"], Cg, case["c_off"], M, N, case["K"], b, case["sA"], case["sB"], sC,
                alpha=case["alpha"], accumulate=case["acc"], pair2=p2, third=th)
        runs.append(Cg.cpu())
    torch.cuda.synchronize()
    out = runs[0]
    assert torch.equal(bits(out), bits(runs[1])), f"{what}: two runs differ"
    mask = torch.ones(out.numel(), dtype=torch.bool)
    for i, off in enumerate(offs):
        mask.as_strided((b, M, N), sC, off).fill_(False)
        ref, mag = refs[i]
        check("gemm" + ("" if i == 0 else "_C3"), label, out.as_strided((b, M, N), sC, off), (ref.as_strided((b, M, N), sC, off), mag),
              what, c=R.gemm_c(case) if i == 0 else case["K"] + 2)
    assert torch.equal(bits(out[mask]), bits(d["C"][mask])), f"{what}: wrote outside its outputs"
    return label, out


@pytest.mark.parametrize("case", R.BMM_CASES, ids=[c["name"].replace(" ", "_") for c in R.BMM_CASES])
def test_bmm(ops, case):
    run_bmm_case(ops, case, seed=len(case["name"]))


def test_bmm_case_list_covers_every_class(ops):
    """The same condition tests/test_attn_composed_ref.py checks on the CPU, here with 16-byte aligned device buffers."""
    assert sorted({R.bmm_case_path(c)[0] for c in R.BMM_CASES}) == sorted(R.ALL_BMM_CLASSES)


def test_bmm_second_output_refused_on_other_layouts(ops, L):
    """A second output is built for outputs that are contiguous along j only; any other layout fails loudly and writes nothing."""
    case = R.BMM_REFUSED
    g = {k: (v.to(DEV) if v is not None else None) for k, v in R.bmm_buffers(case, 3).items()}
    before = g["C"].clone()
    with pytest.raises(L.MsgmError, match=r"msgm_bmm failed: unsupported shape/configuration for this kernel \(-2\)"):
        ops.bmm(g["A"], 0, g["B"], 0, g["C"], case["c_off"], case["M"], case["N"], case["K"], case["batch"], case["sA"], case["sB"],
                case["sC"], third=(g["B3"], 0, g["C"], case["c3_off"]))
    torch.cuda.synchronize()
    assert torch.equal(bits(g["C"]), bits(before))


def test_bmm_second_output_equals_a_call_of_its_own(ops):
    """C3 of the generic-K kernel is bitwise what msgm_bmm(A, B3) alone writes, and does not depend on the batch size."""
    case = next(c for c in R.BMM_CASES if c["name"].startswith("Pv T=36 D=128"))
    M, N, K, b = case["M"], case["N"], case["K"], case["batch"]
    g = {k: v.to(DEV) for k, v in R.bmm_buffers(case, 5).items()}
    both, alone, one = g["C"].clone(), g["C"].clone(), g["C"].clone()
    ops.bmm(g["A"], 0, g["B"], 0, both, case["c_off"], M, N, K, b, case["sA"], case["sB"], case["sC"],
            pair2=(g["A2"], 0, g["B2"], 0), third=(g["B3"], 0, both, case["c3_off"]))
    ops.bmm(g["A"], 0, g["B3"], 0, alone, case["c3_off"], M, N, K, b, case["sA"], case["sB"], case["sC"])
    ops.bmm(g["A"], 0, g["B"], 0, one, case["c_off"], M, N, K, 1, case["sA"], case["sB"], case["sC"],
            pair2=(g["A2"], 0, g["B2"], 0), third=(g["B3"], 0, one, case["c3_off"]))
    v = lambda t, off, nb: bits(t.as_strided((nb, M, N), case["sC"], off))
    assert torch.equal(v(both, case["c3_off"], b), v(alone, case["c3_off"], b))
    assert torch.equal(v(both, case["c3_off"], 1), v(one, case["c3_off"], 1)) and torch.equal(v(both, case["c_off"], 1), v(one, case["c_off"], 1))


# ------------------------------------------------------------------------------------------------ dual softmax
def run_softmax(ops, S, Wd, Pb, Pdb, what, off=5):
    """Forward without and with the tangent, then the backward, each twice on windows of wider buffers.  Returns the outputs."""
    rows, T = S.shape
    n = rows * T
    Wg = Wd.to(DEV).reshape(-1)
    keep = {}
    for dual in (0, 1):
        ref = R.softmax_dual_forward(S, Wd if dual else None)
        outs = []
        for _ in range(2):
            sb, sw, _ = wide(n, off)
            sw.copy_(S.reshape(-1))
            s0 = sb.clone()
            pb_, pw, p0 = wide(n, off + 4)
            ops.softmax_dual_forward(sw, T, Wg if dual else None, pw if dual else None)
            outside_unchanged(sb, s0, off, n, what)
            outside_unchanged(pb_, p0, off + 4, n, what)
            if not dual:
                assert bool(torch.isnan(pw).all()), f"{what}: Pd written without a tangent"
            outs.append((sw.clone(), pw.clone()))
        assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and (not dual or torch.equal(bits(outs[0][1]), bits(outs[1][1])))
        check("softmax_fwd", f"dual{dual}", outs[0][0], ref[0], f"{what} P dual={dual}")
        if dual:
            check("softmax_fwd", "dual1", outs[0][1], ref[1], f"{what} Pd")
        keep[dual] = outs[0][0]
    assert torch.equal(bits(keep[0]), bits(keep[1])), f"{what}: P depends on the tangent"
    Pk = keep[1]                                            # the kernel's own float32 P is the backward's input
    ref = R.softmax_dual_backward(Pk.cpu().reshape(rows, T), Wd, Pb, Pdb)
    outs = []
    for _ in range(2):
        bb, bw, _ = wide(n, off + 1)
        db, dw, _ = wide(n, off + 2)
        bw.copy_(Pb.reshape(-1))
        dw.copy_(Pdb.reshape(-1))
        b0, d0 = bb.clone(), db.clone()
        ops.softmax_dual_backward(Pk, Wg, bw, dw, T)
        outside_unchanged(bb, b0, off + 1, n, what)
        outside_unchanged(db, d0, off + 2, n, what)
        outs.append((bw.clone(), dw.clone()))
    assert torch.equal(bits(outs[0][0]), bits(outs[1][0])) and torch.equal(bits(outs[0][1]), bits(outs[1][1]))
    check("softmax_bwd", "Wbar", outs[0][0], ref[0], f"{what} Wbar")
    check("softmax_bwd", "Wdbar", outs[0][1], ref[1], f"{what} Wdbar")
    return {"P": keep[1], "Wbar": outs[0][0], "Wdbar": outs[0][1]}


@pytest.mark.parametrize("T", R.SOFTMAX_T)
def test_softmax_dual(ops, T):
    S, Wd, Pb, Pdb = R.softmax_inputs(T)
    assert S.shape[0] == 3 * T
    run_softmax(ops, S, Wd, Pb, Pdb, f"softmax T={T} rows={S.shape[0]}")


# ------------------------------------------------------------------------------------------------ glue
@pytest.mark.parametrize("dim", R.TEMB_DIMS)
def test_timestep_embedding(ops, L, dim):
    t, tl = R.temb_inputs()
    B, Bp = t.numel(), tl.numel() // 2
    tg, tlg = t.to(DEV), tl.to(DEV)
    for rep in range(2):
        eb, ew, e0 = wide(B * dim, 3)
        _call(L, "msgm_timestep_embedding", L.ptr(tg), L.ptr(ew), B, dim, 10000.0)
        outside_unchanged(eb, e0, 3, B * dim, "timestep_embedding")
        db, dw, d0 = wide(2 * Bp * dim, 7)
        _call(L, "msgm_timestep_embedding_dual", L.ptr(tlg), L.ptr(dw), Bp, dim, 10000.0)
        outside_unchanged(db, d0, 7, 2 * Bp * dim, "timestep_embedding_dual")
        if rep:
            assert torch.equal(bits(ew), bits(first[0])) and torch.equal(bits(dw), bits(first[1]))
        first = (ew.clone(), dw.clone())
    check("temb", f"dim{dim}", ew, R.timestep_embedding(t, dim)[0], f"timestep_embedding dim={dim}")
    (e, m), (ed, md) = R.timestep_embedding(tl[:Bp], dim, tdot=tl[Bp:])
    check("temb_dual", f"dim{dim}", dw, (torch.cat([e, ed]), torch.cat([m, md])), f"timestep_embedding_dual dim={dim}")
    assert torch.equal(ops.timestep_embedding(tg, dim).reshape(-1), ew) and torch.equal(ops.timestep_embedding_dual(tlg, Bp, dim).reshape(-1), dw)
    if dim % 2:
        assert float(ew.view(B, dim)[:, -1].abs().max()) == 0.0 and float(dw.view(2 * Bp, dim)[:, -1].abs().max()) == 0.0


@pytest.mark.parametrize("Bp,n", R.NORMALIZE_CASES)
def test_normalize_dual(ops, L, Bp, n):
    x = R.normalize_inputs(Bp, n)
    sc = math.sqrt(n)
    for dual in (0, 1):
        Nr = 2 * Bp if dual else Bp
        xg = x[:Nr].contiguous().to(DEV)
        for rep in range(2):
            ob, ow, o0 = wide(Nr * n, 3)
            lb, lw, l0 = wide(Nr, 6)
            _call(L, "msgm_normalize_dual", L.ptr(xg), L.ptr(ow), L.ptr(lw), Bp, n, dual, sc, 1e-6)
            outside_unchanged(ob, o0, 3, Nr * n, "normalize_dual out")
            outside_unchanged(lb, l0, 6, Nr, "normalize_dual logr")
            if rep:
                assert torch.equal(bits(ow), bits(first[0])) and torch.equal(bits(lw), bits(first[1]))
            first = (ow.clone(), lw.clone())
        ref = R.normalize_dual(x[:Nr], Bp, bool(dual), sc)
        check("normalize", f"dual{dual}", ow, ref[0], f"normalize_dual Bp={Bp} n={n} dual={dual} out")
        check("normalize", f"dual{dual}", lw, ref[1], f"normalize_dual Bp={Bp} n={n} dual={dual} logr")
        o, lr = ops.normalize_dual(xg, Bp, n, dual, sc)
        assert torch.equal(o.reshape(-1), ow) and torch.equal(lr, lw)


@pytest.mark.parametrize("B,C,H,W", R.IMAGE_CASES)
@pytest.mark.parametrize("forder", [0, 1])
def test_layout_maps_are_bit_exact(ops, L, B, C, H, W, forder):
    g = torch.Generator().manual_seed(B + C + H + W)
    flat = torch.randn(B, C * H * W, generator=g)
    n = flat.numel()
    for rep in range(2):
        ib, iw, i0 = wide(n, 3)
        _call(L, "msgm_flat_to_image", L.ptr(flat.to(DEV)), L.ptr(iw), B, C, H, W, forder, 0.2)
        outside_unchanged(ib, i0, 3, n, "flat_to_image")
        fb, fw, f0 = wide(n, 5)
        _call(L, "msgm_image_to_flat", L.ptr(iw), L.ptr(fw), B, C, H, W, forder, 5.0)
        outside_unchanged(fb, f0, 5, n, "image_to_flat")
    ri = R.flat_to_image(flat, B, C, H, W, forder, 0.2)
    assert torch.equal(bits(iw.cpu()), bits(ri.reshape(-1))), "flat_to_image is not fp32(x) * fp32(scale)"
    assert torch.equal(bits(fw.cpu()), bits(R.image_to_flat(ri, B, C, H, W, forder, 5.0).reshape(-1)))
    assert torch.equal(ops.flat_to_image(flat.to(DEV), B, C, H, W, forder, 0.2), iw)
    assert torch.equal(ops.image_to_flat(iw.clone(), B, C, H, W, forder, 5.0).reshape(-1), fw)


@pytest.mark.parametrize("N,H,W,C", R.SUM2X2_CASES)
def test_sum2x2_is_bit_exact(ops, L, N, H, W, C):
    g = torch.Generator().manual_seed(N + H + W + C)
    x = torch.randn(N, 2 * H, 2 * W, C, generator=g)
    n = N * H * W * C
    for rep in range(2):
        ob, ow, o0 = wide(n, 3)
        _call(L, "msgm_sum2x2", L.ptr(x.to(DEV)), L.ptr(ow), N, H, W, C)
        outside_unchanged(ob, o0, 3, n, "sum2x2")
    assert torch.equal(bits(ow.cpu()), bits(R.sum2x2(x, N, H, W, C).reshape(-1)))
    assert torch.equal(ops.sum2x2(x.to(DEV), N, H, W, C), ow)
