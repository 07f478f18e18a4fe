"""Host side of the one-launch sampler loop for dense tensors with 17 <= n <= 30 (msgm_mlp_dense_sde_loop): what needs no
GPU — the shape table of msgm_mlp_dense_sde_loop_supported, the two older predicates unchanged, the workspace size, the
refusal of CPU tensors, and the layout of the packed tensor against a NumPy restatement of the kernel's fragment order."""
import itertools

import numpy as np
import pytest
import torch

from sdeflow_light_amd import _lib as L
from sdeflow_light_amd import ops
from sdeflow_light_amd._lib import MsgmError

DENSE, SPARSE, SGM = L.SDE_MSGM_DENSE, L.SDE_MSGM_SPARSE, L.SDE_SGM


@pytest.mark.parametrize("d,pre,kind,n,B,yes", [
    (17, False, DENSE, 17, 65, True),
    (24, False, DENSE, 24, 65, True),
    (30, False, DENSE, 30, 65, True),
    (30, True, DENSE, 30, 65, True),                   # in_dim 32
    (24, True, DENSE, 24, 10000, True),
    (31, False, DENSE, 31, 65, False),                 # the extra-wide class
    (30, False, DENSE, 30, 64, False),                 # two tiles: one workgroup on one CU
    (16, False, DENSE, 16, 65, False),                 # the old entry's
    (16, False, DENSE, 16, 10000, False),
    (20, False, SPARSE, 20, 65, False),
    (20, False, SGM, 20, 65, False),
    (20, False, DENSE, 19, 65, False),                 # the state is not the net's input
    (19, False, DENSE, 20, 65, False),
    (20, False, 3, 20, 65, False),
])
def test_supported_truth_table(d, pre, kind, n, B, yes):
    assert ops.mlp_dense_sde_loop_supported(d, pre, kind, n, B) is yes


def test_the_two_old_predicates_are_unchanged():
    assert ops.mlp_sde_loop_supported(17, False, DENSE, 17, 64) is False
    assert ops.mlp_xw_sde_loop_supported(31, False, DENSE, 31, 64) is False
    for d, pre, B in itertools.product(range(1, 40), (False, True), (64, 65, 10000)):
        assert ops.mlp_sde_loop_supported(d, pre, DENSE, d, B) == (d <= 16)
        assert not ops.mlp_xw_sde_loop_supported(d, pre, DENSE, d, B)


def test_no_shape_is_taken_by_two_entries_and_preferred_implies_supported():
    for d, pre, kind, B in itertools.product(range(0, 40), (False, True), (0, 1, 2, 3), (33, 64, 65, 10000)):
        took = [ops.mlp_sde_loop_supported(d, pre, kind, d, B), ops.mlp_xw_sde_loop_supported(d, pre, kind, d, B),
                ops.mlp_dense_sde_loop_supported(d, pre, kind, d, B)]
        assert sum(took) <= 1, (d, pre, kind, B)
        if ops.mlp_dense_sde_loop_preferred(d, pre, kind, d, B):
            assert took[2], (d, pre, kind, B)


@pytest.mark.parametrize("method", ["heun", "rk4"])
@pytest.mark.parametrize("B,d", [(65, 17), (160, 24), (10000, 30)])
def test_workspace_is_three_state_arrays(method, B, d):
    assert int(L.lib().msgm_mlp_dense_sde_loop_workspace(B, d, ops.SDE_LOOP_METHODS[method])) == 3 * B * d * 4


def test_workspace_euler_maruyama_keeps_no_stage_state():
    assert int(L.lib().msgm_mlp_dense_sde_loop_workspace(10000, 30, L.METHOD_EM)) == 0


def test_cpu_tensors_are_refused():
    """There is no CPU fallback: a CPU state raises before anything is launched."""
    d = 24
    P = L.MlpParamsT(None, None, None, None, None, None, None, None, d, 0)
    G = torch.zeros(d, d, d)
    LG = torch.zeros(d, d)
    st = L.sde_struct(DENSE, 0.1, 20.0, 1.0, 1e-3)
    x = torch.zeros(160, d)
    ts = torch.linspace(0, 1, 5)
    for method in ("em", "heun", "rk4"):
        with pytest.raises(MsgmError, match="no CPU fallback"):
            ops.mlp_dense_sde_loop(P, x, st, method, ts, 0.25, z=torch.zeros(4, 160, d), packed=ops.pack_dense_g(G, LG))
        assert not x.any()


# ------------------------------------------------------------------ the packed tensor
def mfma_16x16x4(a, b, c):
    """v_mfma_f32_16x16x4_f32 on per-lane operands: a[lane] = A[m = lane & 15][k = lane >> 4], b[lane] = B[k = lane >> 4][n = lane & 15],
    c[lane][r] = C[m = 4 (lane >> 4) + r][n = lane & 15]."""
    lane = np.arange(64)
    A = np.zeros((16, 4), a.dtype)
    Bm = np.zeros((4, 16), a.dtype)
    A[lane & 15, lane >> 4] = a
    Bm[lane >> 4, lane & 15] = b
    C = A @ Bm
    out = c.copy()
    for r in range(4):
        out[:, r] += C[4 * (lane >> 4) + r, lane & 15]
    return out


def contraction_from_packed(packed, X, n):
    """T[row, i, k] = sum_j X[row, j] G[i, j, k] and F[row, i] = sum_j L_G[i, j] X[row, j] for 32 rows, from the packed image
    alone, walking it as the kernel does: block kk, i-half ib, row tile mt, eight MFMA steps s = 4 sg + r."""
    lane = np.arange(64)
    il, q = lane & 15, lane >> 4
    T = np.zeros((32, 32, n + 1), packed.dtype)
    for kk, ib, mt in itertools.product(range(n + 1), range(2), range(2)):
        acc = np.zeros((64, 4), packed.dtype)
        for s in range(8):
            j = 4 * s + q
            a = np.where(j < n, X[16 * mt + il, np.minimum(j, n - 1)], 0)    # the kernel's mask on the A operand
            acc = mfma_16x16x4(a, packed[kk, ib, s >> 2, :, s & 3], acc)
        for r in range(4):
            T[16 * mt + 4 * q + r, 16 * ib + il, kk] = acc[:, r]
    return T[:, :, :n], T[:, :, n]


@pytest.mark.parametrize("n", [17, 24, 30])
def test_pack_layout_against_numpy(n):
    """G and L_G of distinct integers: the contraction rebuilt from the packed image equals einsum exactly (small integers
    are exact in any summation order), every live entry appears once, and the padding is +0."""
    G = torch.arange(1, n ** 3 + 1, dtype=torch.float32).reshape(n, n, n)
    LG = -torch.arange(1, n * n + 1, dtype=torch.float32).reshape(n, n)
    packed = ops.pack_dense_g(G, LG)
    assert packed.shape == (n + 1, 2, 2, 64, 4) and packed.dtype == torch.float32 and packed.is_contiguous()
    assert packed.numel() == int(L.lib().msgm_dense_g_packed_floats(n))
    p = packed.numpy()
    flat = p.reshape(-1)
    assert np.array_equal(np.sort(flat[flat != 0]), np.sort(np.concatenate([G.reshape(-1).numpy(), LG.reshape(-1).numpy()])))
    pad = flat[flat == 0]
    assert pad.size == (n + 1) * (1024 - n * n) and not np.signbit(pad).any()
    rng = np.random.default_rng(n)
    X = rng.integers(-3, 4, size=(32, n)).astype(np.float64)
    T, F = contraction_from_packed(p.astype(np.float64), X, n)
    Gn, Ln = G.numpy().astype(np.float64), LG.numpy().astype(np.float64)
    assert np.array_equal(T[:, :n], np.einsum("rj,ijk->rik", X, Gn))
    assert np.array_equal(F[:, :n], np.einsum("ij,rj->ri", Ln, X))
    assert not T[:, n:].any() and not F[:, n:].any()               # dead outputs are exact zeros


def test_pack_refuses_other_shapes():
    with pytest.raises(MsgmError):
        ops.pack_dense_g(torch.zeros(4, 4, 5), torch.zeros(4, 4))
    with pytest.raises(MsgmError):
        ops.pack_dense_g(torch.zeros(33, 33, 33), torch.zeros(33, 33))


def test_packed_tensor_is_lazy_dropped_by_to_and_not_in_the_state_dict():
    from sdeflow_light_amd.SDEs import MSGMsde
    torch.manual_seed(0)
    base = MSGMsde(torch.randn(16, 17), denseTensor=True)
    assert base._G_packed is None
    p = base.packed_G()
    assert p is base.packed_G() and torch.equal(p, ops.pack_dense_g(base.G, base.L_G))
    assert not any("packed" in k for k in base.state_dict())
    assert base.to("cpu")._G_packed is None
    with pytest.raises(MsgmError):
        MSGMsde(torch.randn(16, 17), denseTensor=False).packed_G()
