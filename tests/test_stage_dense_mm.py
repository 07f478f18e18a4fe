"""msgm_sde_stage_dense_mm without a GPU: the packed image (ops.pack_dense_g_stage) against pack_dense_g and its own layout
rule, the kernel's walk over the image emulated lane by lane in float64 against sde_stage_ref's contraction, the routing
predicate, and the two entries through the layers (header, _lib.SIGNATURES, the built library)."""
import os
import re

import numpy as np
import pytest
import torch

import sde_stage_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("msgm_dense_g_stage_floats", "msgm_sde_stage_dense_mm")


def _rand_g(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, n, n, generator=g), torch.randn(n, n, generator=g)


# ------------------------------------------------------------------ packer
@pytest.mark.parametrize("n", [17, 24, 31, 32])
def test_packer_equals_pack_dense_g(n):
    from sdeflow_light_amd import ops
    G, LG = _rand_g(n, n)
    a, b = ops.pack_dense_g_stage(G, LG), ops.pack_dense_g(G, LG)
    assert a.shape == b.shape == (n + 1, 2, 2, 64, 4) and a.dtype == torch.float32 and a.is_contiguous()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", [1, 16, 33, 48, 49, 64])
def test_packer_shape_layout_and_padding(n):
    from sdeflow_light_amd import ops
    G, LG = _rand_g(n, 100 + n)
    G[0, 0, 0] = -0.0                                           # a live -0 stays -0: only the padding is +0
    nb = (n + 15) // 16
    img = ops.pack_dense_g_stage(G, LG)
    assert img.shape == (n + 1, nb, nb, 64, 4) and img.dtype == torch.float32 and img.is_contiguous()
    lane = torch.arange(64).view(1, 1, 64, 1)
    i = (16 * torch.arange(nb).view(nb, 1, 1, 1) + (lane & 15)).expand(nb, nb, 64, 4)
    j = (4 * (4 * torch.arange(nb).view(1, nb, 1, 1) + torch.arange(4).view(1, 1, 1, 4)) + (lane >> 4)).expand(nb, nb, 64, 4)
    pad = (i >= n) | (j >= n)
    bits = img.view(torch.int32)
    assert (bits[:, pad] == 0).all()                            # +0: sign bit clear
    blocks = torch.cat([G.permute(2, 0, 1), LG.unsqueeze(0)], 0)
    live = ~pad
    assert torch.equal(bits[:, live], blocks[:, i[live], j[live]].contiguous().view(torch.int32))
    assert img.numel() == (n + 1) * nb * nb * 256


def test_packer_refuses_65_and_bad_shapes():
    from sdeflow_light_amd import ops
    from sdeflow_light_amd._lib import MsgmError
    with pytest.raises(MsgmError):
        ops.pack_dense_g_stage(torch.zeros(65, 65, 65), torch.zeros(65, 65))
    with pytest.raises(MsgmError):
        ops.pack_dense_g_stage(torch.zeros(8, 8, 7), torch.zeros(8, 8))
    with pytest.raises(MsgmError):
        ops.pack_dense_g_stage(torch.zeros(8, 8, 8), torch.zeros(8, 7))


def test_packed_g_stage_is_cached_plain_and_dropped_by_to():
    from sdeflow_light_amd import ops
    from sdeflow_light_amd.SDEs import MSGMsde
    from sdeflow_light_amd._lib import MsgmError
    torch.manual_seed(0)
    base = MSGMsde(torch.randn(16, 33), denseTensor=True)
    p = base.packed_G_stage()
    assert p is base.packed_G_stage() and torch.equal(p, ops.pack_dense_g_stage(base.G, base.L_G))
    assert not any("packed" in k for k in base.state_dict())
    assert base.to("cpu")._G_packed_stage is None
    b32 = MSGMsde(torch.randn(16, 32), denseTensor=True)
    assert b32.packed_G_stage() is b32.packed_G()              # one image serves both kernels up to n = 32
    with pytest.raises(MsgmError):
        MSGMsde(torch.randn(16, 33), denseTensor=False).packed_G_stage()


# ------------------------------------------------------------------ fragment-order emulation
def _wave_split(nb):
    """(i-blocks of a wave, k-slices) of k_stage_dense_mm<NB>."""
    ibw = 3 if nb == 3 else 1
    return ibw, 4 // (nb // ibw)


def _emulate(img, x, w, a, n):
    """gw, ga, f of a 32-row tile as k_stage_dense_mm's lanes form them, in float64: lane (il, q) of the wave that owns
    (i-block ib, k-slice ks) holds x[16 mt + il][4 s + q] (j >= n masked) as its A operand and the image's [k][ib][s >> 2]
    [lane][s & 3] as its B operand of MFMA step s; D[row 16 mt + 4 q + r][i = 16 ib + il] sits in register r of lane
    (il, q) and is multiplied by the row's w_k and a_k; the k-slices meet in the order ks = 0, 1, ..."""
    nb = (n + 15) // 16
    ibw, ksl = _wave_split(nb)
    ks_steps = 4 * nb
    img = img.numpy().astype(np.float64)
    x, w, a = (v.numpy().astype(np.float64) for v in (x, w, a))
    lanes = np.arange(64)
    il, q = lanes & 15, lanes >> 4

    def block(kk, ib):                                          # D of both row tiles: [mt][lane][r]
        D = np.zeros((2, 64, 4))
        for s in range(ks_steps):
            j = 4 * s + q                                       # per lane
            bop = img[kk, ib, s >> 2, lanes, s & 3]             # B[k = q][n = il] held by lane (il, q)
            for mt in range(2):
                aop = np.where(j < n, x[16 * mt + il, np.minimum(j, n - 1)], 0.0)      # A[m = il][k = q]
                # one 16x16x4 step: D[m][nn] += sum_kq A[m][kq] B[kq][nn]; lane (nn, qq) holds rows m = 4 qq + r
                Am = np.zeros((16, 4)); Bm = np.zeros((4, 16))
                Am[il, q] = aop
                Bm[q, il] = bop
                P = Am @ Bm
                for r in range(4):
                    D[mt, :, r] += P[4 * q + r, il]
        return D

    part_w = np.zeros((ksl, 32, 16 * nb)); part_a = np.zeros_like(part_w); f = np.zeros((32, 16 * nb))
    for wave in range(4):
        ibg, ks = wave % (nb // ibw), wave // (nb // ibw)
        for bi in range(ibw):
            ib = ibg * ibw + bi
            for kk in range(ks, n, ksl):
                D = block(kk, ib)
                for mt in range(2):
                    for r in range(4):
                        rows = 16 * mt + 4 * q + r
                        part_w[ks, rows, 16 * ib + il] += D[mt, :, r] * w[rows, kk]
                        part_a[ks, rows, 16 * ib + il] += D[mt, :, r] * a[rows, kk]
            if ks == ksl - 1:
                D = block(n, ib)
                for mt in range(2):
                    for r in range(4):
                        f[16 * mt + 4 * q + r, 16 * ib + il] = D[mt, :, r]
    gw, ga = part_w[0].copy(), part_a[0].copy()
    for s in range(1, ksl):
        gw += part_w[s]; ga += part_a[s]
    return gw, ga, f


@pytest.mark.parametrize("n", [31, 33, 48, 64])
def test_fragment_order_emulation(n):
    from sdeflow_light_amd import ops
    G, LG = R.dense_G(n)
    g = torch.Generator().manual_seed(7 + n)
    x, w, a = (torch.randn(32, n, generator=g, dtype=torch.float64) for _ in range(3))
    gw, ga, f = _emulate(ops.pack_dense_g_stage(G, LG), x, w, a, n)
    Gd, Ld = G.double(), LG.double()
    for name, got, ref in (("gw", gw, R._dense3(Gd, x, w)), ("ga", ga, R._dense3(Gd, x, a)), ("f", f, R._dense2(Ld, x))):
        got = torch.from_numpy(got)
        assert (got[:, n:] == 0).all(), name                    # outputs i >= n: the image's zero padding
        err = float((got[:, :n] - ref).norm() / ref.norm())
        assert err <= 1e-12, (name, n, err)


# ------------------------------------------------------------------ predicate
def test_predicate_truth_table():
    from sdeflow_light_amd import _lib as L, ops
    pref = ops.stage_dense_mm_preferred
    assert pref(L.SDE_MSGM_DENSE, 31, L.PROC_REVERSE) and pref(L.SDE_MSGM_DENSE, 64, L.PROC_REVERSE)
    assert not pref(L.SDE_MSGM_DENSE, 30, L.PROC_REVERSE) and not pref(L.SDE_MSGM_DENSE, 65, L.PROC_REVERSE)
    for n in (1, 16, 30, 31, 32, 48, 64, 65, 128):
        assert not pref(L.SDE_MSGM_DENSE, n, L.PROC_FORWARD)
        for proc in (L.PROC_REVERSE, L.PROC_FORWARD):
            assert not pref(L.SDE_MSGM_SPARSE, n, proc) and not pref(L.SDE_SGM, n, proc)


# ------------------------------------------------------------------ ABI
def _declared_arity():
    txt = open(os.path.join(ROOT, "include", "msgm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: len([a for a in args.split(",") if a.strip()])
            for name, args in re.findall(r"\b(msgm_dense_g_stage_floats|msgm_sde_stage_dense_mm)\s*\(([^)]*)\)\s*;", txt)}


def test_entries_declared_with_matching_signatures():
    from sdeflow_light_amd import _lib
    decl = _declared_arity()
    assert set(decl) == set(ENTRIES), decl
    for n in ENTRIES:
        assert n in _lib.SIGNATURES, n
        assert len(_lib.SIGNATURES[n][1]) == decl[n], (n, decl[n])
    # the stage's argument list is msgm_sde_stage's plus `packed` ahead of the stream
    a, b = _lib.SIGNATURES["msgm_sde_stage"][1], _lib.SIGNATURES["msgm_sde_stage_dense_mm"][1]
    assert b[:len(a) - 1] == a[:-1] and len(b) == len(a) + 1


def test_header_cites_the_reference():
    txt = open(os.path.join(ROOT, "include", "msgm_hip.h")).read()
    block = txt[txt.index("int msgm_sde_stage_dense_mm") - 2600: txt.index("int msgm_sde_stage_dense_mm")]
    assert "SDEs.py:415" in block and "SDEs.py:432" in block and "sde_scheme.py:36" in block


def test_library_exports_and_host_queries():
    import __graft_entry__ as g
    g.build()
    from sdeflow_light_amd import _lib
    Lb = _lib.lib()
    for n in ENTRIES:
        assert hasattr(Lb, n), n
    fl = Lb.msgm_dense_g_stage_floats
    assert fl(33) == 34 * 3 * 3 * 256
    assert fl(1) == 2 * 256 and fl(16) == 17 * 256 and fl(64) == 65 * 16 * 256
    assert fl(0) == 0 and fl(65) == 0
    for n in (17, 30, 32):
        assert fl(n) == Lb.msgm_dense_g_packed_floats(n)
    # null pointers are refused before anything is launched (MSGM_E_BADARG = -1)
    assert Lb.msgm_sde_stage_dense_mm(None, None, 1.0, None, None, None, None, 1.0, None, 0, None, None, 1, 33, None, 0, 0,
                                      0.0, 0.1, 0.0, None, None, 0.0, None, None, None, None) == -1
