"""Host side of the one-launch MLP sampler loop (msgm_mlp_sde_loop): what needs no GPU — the refusal of CPU tensors, the
shape table of msgm_mlp_sde_loop_supported and the workspace size."""
import pytest
import torch

from sdeflow_light_amd import _lib as L
from sdeflow_light_amd import ops
from sdeflow_light_amd._lib import MsgmError


def test_cpu_tensors_are_refused():
    """There is no CPU fallback: a CPU state raises before anything is launched."""
    P = L.MlpParamsT(None, None, None, None, None, None, None, None, 2, 0)
    st = L.sde_struct(L.SDE_SGM, 0.1, 20.0, 1.0, 1e-3)
    x = torch.zeros(64, 2)
    ts = torch.linspace(0, 1, 5)
    for method in ("em", "heun", "rk4"):
        with pytest.raises(MsgmError):
            ops.mlp_sde_loop(P, x, st, method, ts, 0.25, z=torch.zeros(4, 64, 2))


@pytest.mark.parametrize("d,pre,kind,n,B,yes", [
    (30, True, L.SDE_SGM, 30, 64, True),              # in_dim 32: the widest the wide carve takes
    (31, False, L.SDE_SGM, 31, 64, False),            # the extra-wide class stays composed
    (16, False, L.SDE_MSGM_DENSE, 16, 64, True),
    (17, False, L.SDE_MSGM_DENSE, 17, 64, False),     # the dense tensor is contracted for n <= 16
    (17, False, L.SDE_MSGM_SPARSE, 17, 64, True),
    (2, False, L.SDE_SGM, 2, 32, False),              # one tile: nothing to prefetch one ahead
    (2, False, L.SDE_SGM, 2, 33, True),
    (2, True, L.SDE_MSGM_DENSE, 2, 10000, True),      # the driver's default
    (6, True, L.SDE_MSGM_SPARSE, 5, 64, False),       # the state is not the net's input
    (0, False, L.SDE_SGM, 0, 64, False),
    (2, False, 3, 2, 64, False),
])
def test_supported_truth_table(d, pre, kind, n, B, yes):
    assert ops.mlp_sde_loop_supported(d, pre, kind, n, B) is yes


@pytest.mark.parametrize("method", ["heun", "rk4"])
def test_workspace_positive_and_grows_with_B(method):
    w = [int(L.lib().msgm_mlp_sde_loop_workspace(B, 6, ops.SDE_LOOP_METHODS[method])) for B in (33, 64, 10000)]
    assert w[0] > 0 and w[0] < w[1] < w[2]
    assert w[2] == 3 * 10000 * 6 * 4                  # evaluation point, Wiener increment, running sum


def test_workspace_euler_maruyama_keeps_no_stage_state():
    assert int(L.lib().msgm_mlp_sde_loop_workspace(10000, 6, L.METHOD_EM)) == 0
