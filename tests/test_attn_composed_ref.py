"""CPU checks of tests/attn_composed_ref.py: (1) the float64 restatement equals torch einsum / torch.func.jvp + autograd /
oracle/nets_ref.py in float64; (2) MEASURED, the source of the tolerance constants of tests/test_composed_attention_gpu.py,
is what the restatement evaluated in float32 measures against float64 over that test's case lists; (3) the GEMM case list
reaches every kernel instantiation of msgm_bmm_dual (bmm_path restates the dispatch) and every epilogue branch."""
import math

import pytest
import torch

import attn_composed_ref as R
from oracle import nets_ref as N

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ (1) the restatement
@pytest.mark.parametrize("T,D", [(9, 16), (25, 32), (36, 64)])
def test_bmm_strided_equals_einsum_on_the_attention_layouts(T, D):
    """NT (q k^T + qdot-pair), NN (P v with the second output) and TN (P^T g, accumulated) on channel slices of a fused
    (2 Bn, T, 3 D) qkv tensor with the tangent rows behind the primal ones, as NNUnet._attn_fwd / _attn_bwd_composed call it."""
    g = torch.Generator().manual_seed(T)
    Bn, ld = 3, 3 * D
    qkv = torch.randn(2 * Bn, T, ld, generator=g)
    P, Pd = torch.randn(Bn, T, T, generator=g), torch.randn(Bn, T, T, generator=g)
    half = Bn * T * ld
    q, k, v, qd, kd, vd = (qkv[a:a + Bn, :, c * D:(c + 1) * D].double() for a in (0, Bn) for c in range(3))
    sq, skT, sP, sPt, sa = (T * ld, ld, 1), (T * ld, 1, ld), (T * T, T, 1), (T * T, 1, T), (T * D, D, 1)
    flat = qkv.reshape(-1)
    # NT with a second pair and alpha
    Wd = torch.full((Bn * T * T + 5,), 7.0)
    [(out, mag)] = R.bmm_strided(flat, half, flat, D, Wd, 5, T, T, D, Bn, sq, skT, sP, alpha=0.5, pair2=(flat, 0, flat, half + D))
    ref = R.c32(0.5) * (torch.einsum("btc,bsc->bts", qd, k) + torch.einsum("btc,bsc->bts", q, kd))
    assert torch.allclose(out[5:].view(Bn, T, T), ref, rtol=1e-13, atol=1e-13) and bool((out[:5] == 7.0).all())
    mref = 0.5 * (torch.einsum("btc,bsc->bts", qd.abs(), k.abs()) + torch.einsum("btc,bsc->bts", q.abs(), kd.abs()))
    assert torch.allclose(mag, mref, rtol=1e-13) and bool((mag >= ref.abs() * (1 - 1e-12)).all())
    # NN with the second pair and the second output, both into one (2 Bn, T, D) tensor
    att = torch.full((2 * Bn * T * D,), float("nan"))
    (o1, m1), (o3, m3) = R.bmm_strided(P.reshape(-1), 0, flat, half + 2 * D, att, Bn * T * D, T, D, T, Bn, sP, sq, sa,
                                       pair2=(Pd.reshape(-1), 0, flat, 2 * D), third=(flat, 2 * D, att, 0))
    assert o1 is o3
    o = o1.view(2 * Bn, T, D)
    assert torch.allclose(o[:Bn], torch.einsum("bts,bsc->btc", P.double(), v), rtol=1e-13, atol=1e-13)
    assert torch.allclose(o[Bn:], torch.einsum("bts,bsc->btc", P.double(), vd) + torch.einsum("bts,bsc->btc", Pd.double(), v),
                          rtol=1e-13, atol=1e-13)
    assert torch.allclose(m3, torch.einsum("bts,bsc->btc", P.double().abs(), v.abs()), rtol=1e-13)
    # TN, accumulated onto a non-zero base in the k slice of a dqkv tensor; the other slices keep their contents
    dq = torch.randn(2 * Bn * T * ld, generator=g)
    gq, gq3 = torch.randn(Bn, T, D, generator=g), torch.randn(Bn, T, D, generator=g)
    (o1, m1), (o3, m3) = R.bmm_strided(P.reshape(-1), 0, gq.reshape(-1), 0, dq, D, T, D, T, Bn, sPt, sa, sq, alpha=-2.0,
                                       accumulate=True, third=(gq3.reshape(-1), 0, dq, half + D))
    o, b = o1.view(2 * Bn, T, ld), dq.double().view(2 * Bn, T, ld)
    assert torch.allclose(o[:Bn, :, D:2 * D], b[:Bn, :, D:2 * D] - 2 * torch.einsum("bts,btc->bsc", P.double(), gq.double()), rtol=1e-13, atol=1e-13)
    assert torch.allclose(o[Bn:, :, D:2 * D], b[Bn:, :, D:2 * D] - 2 * torch.einsum("bts,btc->bsc", P.double(), gq3.double()), rtol=1e-13, atol=1e-13)
    assert torch.equal(o[:, :, :D], b[:, :, :D]) and torch.equal(o[:, :, 2 * D:], b[:, :, 2 * D:])
    assert torch.allclose(m1, 2 * torch.einsum("bts,btc->bsc", P.double().abs(), gq.double().abs()) + b[:Bn, :, D:2 * D].abs(), rtol=1e-13)


@pytest.mark.parametrize("T", R.SOFTMAX_T)
def test_softmax_pair_equals_jvp_and_autograd_float64(T):
    S, Wd, Pb, Pdb = (x.double() for x in R.softmax_inputs(T))
    S = S.clone().requires_grad_(True)
    Wdr = Wd.clone().requires_grad_(True)
    P, Pd = torch.func.jvp(lambda s: torch.softmax(s, -1), (S,), (Wdr,))
    (Pr, mP), (Pdr, mPd) = R.softmax_dual_forward(S.detach(), Wd)
    assert torch.allclose(Pr, P.detach(), rtol=1e-13, atol=1e-300) and float(((Pdr - Pd.detach()).abs() / mPd).max()) <= 1e-13
    assert bool((mP >= Pr).all()) and bool((mPd >= Pdr.abs() * (1 - 1e-12)).all())
    assert torch.equal(R.softmax_dual_forward(S.detach())[0][0], Pr)
    ((P * Pb).sum() + (Pd * Pdb).sum()).backward()
    (W, mW), (Wdb, mWd) = R.softmax_dual_backward(Pr, Wd, Pb, Pdb)
    assert float(((W - S.grad).abs() / mW).max()) <= 1e-13 and float(((Wdb - Wdr.grad).abs() / mWd).max()) <= 1e-13
    assert bool((mW >= W.abs() * (1 - 1e-12)).all()) and bool((mWd >= Wdb.abs() * (1 - 1e-12)).all())


def test_softmax_reference_is_finite_on_the_extreme_rows():
    """Rows 0-3 of softmax_inputs (logits spread over +-60, constant, one dominant entry, two equal maxima): the row maximum
    is subtracted, so the float64 AND the float32 evaluation stay finite and every row sums to 1."""
    for T in R.SOFTMAX_T:
        S, Wd, Pb, Pdb = R.softmax_inputs(T)
        assert float(S[0].max() - S[0].min()) > 60 and float(S[1].max() - S[1].min()) == 0
        for dt in (F64, torch.float32):
            (P, mP), (Pd, mPd) = R.softmax_dual_forward(S, Wd, dtype=dt)
            (W, mW), (Wdb, mWd) = R.softmax_dual_backward(P, Wd, Pb, Pdb, dtype=dt)
            for x in (P, mP, Pd, mPd, W, mW, Wdb, mWd):
                assert bool(torch.isfinite(x).all())
            assert torch.allclose(P.sum(-1), torch.ones(P.shape[0], dtype=dt), rtol=1e-5)
        p0 = R.softmax_dual_forward(S, dtype=torch.float32)[0][0][0]
        assert int((p0 == 0).sum()) >= 1 and int((p0 < 1e-12).sum()) > T // 2                          # exp underflowed
        assert float(R.softmax_dual_forward(S)[0][0][2].max()) > 1 - 1e-12                              # the dominant entry


def test_glue_equals_oracle():
    t, tl = R.temb_inputs()
    Bp = tl.numel() // 2
    for dim in R.TEMB_DIMS:
        [(e, m)] = R.timestep_embedding(t, dim)
        assert e.shape == (t.numel(), dim) and torch.allclose(e, N.sinusoidal_embedding(t.double(), dim), rtol=0, atol=2e-6)
        lr = tl[:Bp].double().clone().requires_grad_(True)           # the tangent: d emb / d logr . tdot
        (e, m), (ed, md) = R.timestep_embedding(tl[:Bp], dim, tdot=tl[Bp:])
        _, jv = torch.func.jvp(lambda a: N.sinusoidal_embedding(a, dim), (lr,), (tl[Bp:].double(),))
        assert torch.allclose(ed, jv.detach(), rtol=0, atol=2e-6 * float(tl[Bp:].abs().max()))
        assert bool((m >= e.abs()).all()) and bool((md >= ed.abs() * (1 - 1e-12)).all())
        if dim % 2:
            assert bool((e[:, -1] == 0).all()) and bool((ed[:, -1] == 0).all())
    for Bp, n in R.NORMALIZE_CASES:
        x = R.normalize_inputs(Bp, n)
        sc = math.sqrt(n)
        f = lambda a: N.normalize_log_radius(a)
        (u, lg), (ud, lgd) = torch.func.jvp(f, (x[:Bp].double(),), (x[Bp:].double(),))
        (out, om), (logr, lm) = R.normalize_dual(x, Bp, True, sc)
        assert torch.allclose(out, torch.cat([u, ud]) * sc, rtol=1e-6, atol=1e-9)
        assert torch.allclose(logr, torch.cat([lg, lgd]).reshape(-1), rtol=1e-6, atol=1e-9)
        assert bool((om >= out.abs() * (1 - 1e-12)).all()) and bool((lm >= logr.abs() * (1 - 1e-12)).all())
        (o1, _), (l1, _) = R.normalize_dual(x[:Bp], Bp, False, sc)
        assert torch.equal(o1, out[:Bp]) and torch.equal(l1, logr[:Bp])
    for B, C, H, W in R.IMAGE_CASES:
        flat = torch.randn(B, C * H * W)
        for forder, order in ((0, "C"), (1, "F")):
            img = R.flat_to_image(flat, B, C, H, W, forder, 1.0 / N.IMAGE_SCALE)
            ref = N.flat_to_image(flat, H, W, order, C).permute(0, 2, 3, 1)
            assert img.shape == (B, H, W, C) and torch.allclose(img, ref, rtol=2e-7, atol=0)
            back = R.image_to_flat(img, B, C, H, W, forder, N.IMAGE_SCALE)
            assert torch.allclose(back, N.image_to_flat(img.permute(0, 3, 1, 2), order), rtol=0, atol=0)
            assert torch.allclose(back, flat, rtol=3e-7)
    for Nn, H, W, C in R.SUM2X2_CASES:
        x = torch.randn(Nn, 2 * H, 2 * W, C)
        up = torch.randn(Nn, H, W, C, dtype=F64)
        # adjoint of the nearest 2x upsample (model/unet.py:67): <sum2x2(x), u> = <x, upsample(u)>
        rep = up.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        s = R.sum2x2(x, Nn, H, W, C)
        assert s.dtype == torch.float32 and abs(float((s.double() * up).sum() - (x.double() * rep).sum())) <= 1e-4 * x.numel() ** 0.5


# ------------------------------------------------------------------------------------------------ (2) tolerance constants
def _upd(acc, family, pairs32, pairs64):
    for (v32, _), (v64, mag) in zip(pairs32, pairs64):
        acc[family] = max(acc.get(family, 0.0), R.ratio(v32, v64, mag))


def measure():
    """{family: worst |ref32 - ref64| / (2^-24 magnitude)} over the GPU test's case lists."""
    acc = {}
    f32 = torch.float32
    for T in R.SOFTMAX_T:
        S, Wd, Pb, Pdb = R.softmax_inputs(T)
        _upd(acc, "softmax_fwd", R.softmax_dual_forward(S, Wd, dtype=f32), R.softmax_dual_forward(S, Wd))
        P = R.softmax_dual_forward(S, dtype=f32)[0][0]              # the backward's P is a float32 input
        _upd(acc, "softmax_bwd", R.softmax_dual_backward(P, Wd, Pb, Pdb, dtype=f32), R.softmax_dual_backward(P, Wd, Pb, Pdb))
    t, tl = R.temb_inputs()
    Bp = tl.numel() // 2
    for dim in R.TEMB_DIMS:
        _upd(acc, "temb", R.timestep_embedding(t, dim, dtype=f32), R.timestep_embedding(t, dim))
        _upd(acc, "temb_dual", R.timestep_embedding(tl[:Bp], dim, dtype=f32, tdot=tl[Bp:]), R.timestep_embedding(tl[:Bp], dim, tdot=tl[Bp:]))
    for Bp, n in R.NORMALIZE_CASES:
        x = R.normalize_inputs(Bp, n)
        for dual in (False, True):
            xx = x if dual else x[:Bp]
            _upd(acc, "normalize", R.normalize_dual(xx, Bp, dual, math.sqrt(n), dtype=f32), R.normalize_dual(xx, Bp, dual, math.sqrt(n)))
    return acc


def test_measured_constants_are_reproduced():
    got = measure()
    assert set(got) == set(R.MEASURED)
    for fam, r in sorted(got.items()):
        print(f"{fam:12s}: float32 restatement ratio {r:.3f}  (MEASURED {R.MEASURED[fam]}, c = {R.c_of(fam):.2f})")
        assert abs(r - R.MEASURED[fam]) <= 0.1 * R.MEASURED[fam], (fam, r, R.MEASURED[fam])


# ------------------------------------------------------------------------------------------------ (3) coverage of the dispatch
def test_gemm_case_list_reaches_every_kernel_instantiation():
    """A condition, not a measurement: the list may not leave out one of the 18 instantiations (k_bmm_slow<dual>, eight
    k_bmm_lds<AM,BM,dual>, eight k_bmm<2,2,avec,bvec,dual>) nor one of the epilogue's branches."""
    seen = {}
    for case in R.BMM_CASES:
        label, fl = R.bmm_case_path(case)
        assert label != "unsupported", case["name"]
        seen.setdefault(label, []).append((case, fl))
        assert case["batch"] == 3 and max(case["M"], case["N"], case["K"]) <= 160
    for label in sorted(seen):
        print(f"{label:14s} " + "; ".join(c["name"] for c, _ in seen[label]))
    assert sorted(seen) == sorted(R.ALL_BMM_CLASSES) and len(R.ALL_BMM_CLASSES) == 18
    assert len({c["name"] for c in R.BMM_CASES}) == len(R.BMM_CASES)
    has = lambda pred: any(pred(c, f, lab) for lab, v in seen.items() for c, f in v)
    slow = lambda lab: lab.startswith("slow")
    # k_bmm_slow: K = T in {9, 25, 36, 100}, D in {64, 128}, with and without pair2, accumulate, the transposed A
    assert {c["K"] for lab, v in seen.items() if slow(lab) for c, _ in v} >= {9, 25, 36, 100}
    for K in (9, 25, 36, 100):
        assert has(lambda c, f, lab: slow(lab) and c["K"] == K and c["third"]), K
    assert has(lambda c, f, lab: slow(lab) and c["pair2"] and c["acc"]) and has(lambda c, f, lab: slow(lab) and not c["pair2"] and c["acc"])
    assert has(lambda c, f, lab: slow(lab) and c["sA"][1] == 1) and has(lambda c, f, lab: slow(lab) and not f["swap"])
    # k_bmm_lds: ragged 64-tiles at M = N in {36, 100, 144}, K = 160 with a ragged row tile
    assert {c["M"] for lab, v in seen.items() if lab.startswith("lds") for c, _ in v if c["M"] == c["N"]} >= {36, 100, 144}
    assert has(lambda c, f, lab: lab.startswith("lds") and c["K"] == 160)
    # k_bmm: K % 32 != 0, M or N % 4 != 0, and both store paths with and without the tail
    reg = lambda lab: lab.startswith("reg")
    assert has(lambda c, f, lab: reg(lab) and c["K"] == 144) and has(lambda c, f, lab: reg(lab) and c["M"] % 4)
    assert has(lambda c, f, lab: reg(lab) and f["cvec"] and f["tail"]) and has(lambda c, f, lab: reg(lab) and not f["cvec"] and f["tail"])
    assert has(lambda c, f, lab: reg(lab) and not f["cvec"] and c["c_off"] % 4)              # C's base misaligned
    assert has(lambda c, f, lab: reg(lab) and not f["cvec"] and c["sC"][1] % 4 and not c["c_off"] % 4)      # C's row stride
    assert has(lambda c, f, lab: reg(lab) and c["sA"][1] % 4 == 1)                            # an operand row stride % 4 != 0
    for opt in ("pair2", "third", "acc"):
        for kind in ("slow", "lds", "reg"):
            assert has(lambda c, f, lab: lab.startswith(kind) and c[opt]), (opt, kind)
    assert has(lambda c, f, lab: c["alpha"] != 1.0 and lab.startswith("lds")) and has(lambda c, f, lab: c["alpha"] != 1.0 and slow(lab))
    assert R.bmm_case_path(R.BMM_REFUSED)[0] == "unsupported"


def test_bmm_buffers_hold_every_operand():
    for case in R.BMM_CASES:
        d = R.bmm_buffers(case, 1)
        outs = R.bmm_case_ref(case, d)
        assert len(outs) == 1 + int(case["third"])
        for buf, mag in outs:
            assert bool(torch.isfinite(buf).all()) and bool((mag > 0).all())
        # everything outside the outputs' extents is the buffer's own contents
        mask = torch.ones(d["C"].numel(), dtype=torch.bool)
        for off in [case["c_off"]] + ([case["c3_off"]] if case["third"] else []):
            mask.as_strided((case["batch"], case["M"], case["N"]), case["sC"], off).fill_(False)
        assert int(mask.sum()) >= 16 and torch.equal(outs[0][0][mask], d["C"].double()[mask])
