"""Host side of the one-launch sampler loop of the extra-wide MLP class (msgm_mlp_xw_sde_loop): what needs no GPU — the
shape table of msgm_mlp_xw_sde_loop_supported, that no shape is taken by both loop entries, the workspace size and the
refusal of CPU tensors."""
import itertools

import pytest
import torch

from sdeflow_light_amd import _lib as L
from sdeflow_light_amd import ops
from sdeflow_light_amd._lib import MsgmError


@pytest.mark.parametrize("d,pre,kind,n,B,yes", [
    (31, False, L.SDE_SGM, 31, 64, True),
    (128, True, L.SDE_MSGM_SPARSE, 128, 33, True),
    (128, True, L.SDE_MSGM_SPARSE, 128, 32, False),    # one tile: nothing to prefetch one ahead
    (30, True, L.SDE_SGM, 30, 64, False),              # in_dim 32: the wide class, the narrow entry's
    (31, False, L.SDE_MSGM_DENSE, 31, 64, False),      # the dense tensor stops at n = 16
    (40, False, L.SDE_MSGM_SPARSE, 39, 64, False),     # the state is not the net's input
    (129, False, L.SDE_SGM, 129, 64, False),
    (0, False, L.SDE_SGM, 0, 64, False),
    (0, True, L.SDE_MSGM_SPARSE, 0, 10000, False),
    (40, False, 3, 40, 64, False),
    (2, False, 3, 2, 64, False),
    (128, True, 3, 128, 10000, False),
])
def test_supported_truth_table(d, pre, kind, n, B, yes):
    assert ops.mlp_xw_sde_loop_supported(d, pre, kind, n, B) is yes


def test_no_shape_is_taken_by_both_entries():
    kinds = (L.SDE_SGM, L.SDE_MSGM_SPARSE, L.SDE_MSGM_DENSE)
    taken = {"narrow": 0, "xw": 0}
    for d, pre, kind, B in itertools.product(range(1, 131), (False, True), kinds, (32, 33)):
        a = ops.mlp_sde_loop_supported(d, pre, kind, d, B)
        b = ops.mlp_xw_sde_loop_supported(d, pre, kind, d, B)
        assert not (a and b), (d, pre, kind, B)
        taken["narrow"] += a
        taken["xw"] += b
        if B == 32 or d > 128:
            assert not a and not b
        elif kind != L.SDE_MSGM_DENSE:
            assert a != b, (d, pre, kind, B)            # SGM and the sparse tensor: exactly one entry up to d = 128
            assert b == (d > 30 or d + 1 + int(pre) > 32)
    assert taken["narrow"] > 0 and taken["xw"] > 0


@pytest.mark.parametrize("d,pre,kind,n,B,yes", [
    (31, False, L.SDE_SGM, 31, 64, True),
    (64, True, L.SDE_SGM, 64, 10000, True),
    (65, False, L.SDE_SGM, 65, 10000, False),          # measured slower than the composed steps from d = 90
    (40, True, L.SDE_MSGM_SPARSE, 40, 160, True),
    (41, True, L.SDE_MSGM_SPARSE, 41, 10000, False),   # the sparse tensor: slower from d = 64
    (128, True, L.SDE_MSGM_SPARSE, 128, 33, False),    # supported, not routed
    (40, True, L.SDE_MSGM_SPARSE, 40, 32, False),
    (30, True, L.SDE_SGM, 30, 64, False),
])
def test_preferred_truth_table(d, pre, kind, n, B, yes):
    """What the public samplers route to the loop: part of what the entry takes."""
    assert ops.mlp_xw_sde_loop_preferred(d, pre, kind, n, B) is yes
    assert ops.mlp_xw_sde_loop_supported(d, pre, kind, n, B) or not yes


def test_preferred_implies_supported():
    for d, pre, kind, B in itertools.product(range(0, 131), (False, True), (0, 1, 2, 3), (32, 33, 10000)):
        if ops.mlp_xw_sde_loop_preferred(d, pre, kind, d, B):
            assert ops.mlp_xw_sde_loop_supported(d, pre, kind, d, B), (d, pre, kind, B)


@pytest.mark.parametrize("method", ["heun", "rk4"])
@pytest.mark.parametrize("B,d", [(33, 31), (64, 40), (10000, 128)])
def test_workspace_is_three_state_arrays(method, B, d):
    assert int(L.lib().msgm_mlp_xw_sde_loop_workspace(B, d, ops.SDE_LOOP_METHODS[method])) == 3 * B * d * 4


def test_workspace_euler_maruyama_keeps_no_stage_state():
    assert int(L.lib().msgm_mlp_xw_sde_loop_workspace(10000, 128, L.METHOD_EM)) == 0


def test_cpu_tensors_are_refused():
    """There is no CPU fallback: a CPU state raises before anything is launched."""
    P = L.MlpParamsT(None, None, None, None, None, None, None, None, 40, 0)
    st = L.sde_struct(L.SDE_SGM, 0.1, 20.0, 1.0, 1e-3)
    x = torch.zeros(64, 40)
    ts = torch.linspace(0, 1, 5)
    for method in ("em", "heun", "rk4"):
        with pytest.raises(MsgmError):
            ops.mlp_xw_sde_loop(P, x, st, method, ts, 0.25, z=torch.zeros(4, 64, 40))
        assert not x.any()
