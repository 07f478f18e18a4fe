"""CPU checks of tests/ssm_weights_ref.py (the float64 statement of the weighted SSM loss) and of the public surface that
carries the per-row weights."""
import inspect
import os
import re

import pytest
import torch

import mlp_rows_ref as M
import ssm_weights_ref as W
from conftest import parity_vs_fp64
from oracle import sde_ref as S, ssm_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("form", W.FORMS)
def test_unit_weights_reproduce_the_mean(form):
    d, pre, B = 4, None, 23
    i = W.mlp_inputs(d, pre, B)
    p64 = M.cast(M.params(d, pre), torch.float64)
    args = (W.spec(form, d), W.score(pre), p64, i["t"].double(), i["y"].double(), i["v"].double())
    loss, per, g = LR.ssm_mean_and_grads(*args)
    for seed_form in (False, True):
        lw, pw, gw = W.weighted(*args, torch.ones(B), torch.float64, seed_form=seed_form)
        assert torch.equal(pw, per)
        assert abs(float(lw) - float(loss)) <= 1e-13 * abs(float(loss))
        for k in g:
            assert float((gw[k] - g[k]).norm()) <= 1e-12 * float(g[k].norm()), k


@pytest.mark.parametrize("form", W.FORMS)
def test_gradient_is_linear_in_the_weights(form):
    """The sum over one-hot weights is the all-ones gradient; a weighted call is the weighted sum of the one-hot ones."""
    d, pre, B = 4, M.PRE if form == "sparse" else None, 5
    d = 14 if pre else d
    i = W.mlp_inputs(d, pre, B)
    p64 = M.cast(M.params(d, pre), torch.float64)
    args = (W.spec(form, d), W.score(pre), p64, i["t"].double(), i["y"].double(), i["v"].double())
    hot = [W.weighted(*args, torch.eye(B)[b], torch.float64)[2] for b in range(B)]
    ones = W.weighted(*args, torch.ones(B), torch.float64)[2]
    w = torch.tensor([0.5, -1.0, 0.0, 4.0, 1.75])
    mixed = W.weighted(*args, w, torch.float64)[2]
    for k in ones:
        assert float((sum(h[k] for h in hot) - ones[k]).norm()) <= 1e-12 * float(ones[k].norm()), k
        assert float((sum(float(w[b]) * hot[b][k] for b in range(B)) - mixed[k]).norm()) <= 1e-12 * float(mixed[k].norm()), k


def test_cases_reach_every_training_kernel_and_both_forms():
    """launch_mlp's dispatch restated as in test_mlp_rows_gpu.test_cases_pin_their_class: two cases (without and with
    NormalizeLogRadius) in each of the narrow, wide and extra-wide classes, all of them cases of mlp_rows_ref."""
    want = {"narrow": W.CASES[:2], "wide": W.CASES[2:4], "xwide": W.CASES[4:]}
    for k, cases in want.items():
        assert [pre for _, pre in cases] == [None, M.PRE]
        for d, pre in cases:
            i = d + 1 + (1 if pre else 0)
            got = "xwide" if (d > 30 or i > 32) else ("wide" if (i > 16 or d > 16) else ("tiny" if (i <= 4 and d <= 4) else "narrow"))
            assert got == k == M.klass(d, pre), (d, pre, got)
            assert (d, pre) in M.CASES
    assert W.FORMS == ("sgm", "sparse")
    assert W.EXACT_BATCHES == (1, 15, 17, 4097) and W.PARITY_BATCH == 4097
    w = W.weights(W.PARITY_BATCH)
    assert float(w[16:32].abs().max()) == 0.0 and int((w == 0).sum()) > 16 + 500       # a whole tile and scattered rows
    pos = w[w > 0]
    assert 0.25 <= float(pos.min()) and float(pos.max()) <= 4.0


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("d,pre", W.CASES, ids=[M.case_id(d, pre) for d, pre in W.CASES])
def test_float32_oracle_stays_inside_the_bound(d, pre, form):
    """On the inputs and weights of the GPU parity test, a float32 evaluation of the weighted statement in the other
    order (the seed form: the vector-Jacobian product with inv_batch * w) is inside parity_vs_fp64's default bound,
    whose yardstick is the float32 evaluation of (w . L).sum() / B."""
    B = W.PARITY_BATCH
    torch.set_num_threads(min(16, torch.get_num_threads()))

    def other_order():
        _, per, g = W.mlp_weighted(d, pre, form, B, torch.float32, True)
        return per, g

    def oracle(dt):
        _, per, g = W.mlp_weighted(d, pre, form, B, dt)
        return per, g
    parity_vs_fp64(other_order, oracle, f"float32 seed form, MLP {M.case_id(d, pre)} {form} B={B}")
    per64 = W.mlp_weighted(d, pre, form, B)[1]
    assert torch.isfinite(per64).all() and float(per64.abs().min()) > 0


def test_row_weight_keyword_on_the_public_surface():
    from sdeflow_light_amd import ops, _lib
    from sdeflow_light_amd.NNUnet import VorticityUNet
    from sdeflow_light_amd.NNUnet1D import UNet1D
    from sdeflow_light_amd.SDEs import PluginReverseSDE
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    for fn in (ops.mlp_ssm_grad, ops.ssm_loss, ops.ssm_loss_diag, UNet1D.ssm_grad, VorticityUNet.ssm_grad):
        prm = inspect.signature(fn).parameters
        assert list(prm)[-1] == "row_weight", fn
        assert prm["row_weight"].kind is inspect.Parameter.KEYWORD_ONLY and prm["row_weight"].default is None, fn
    for fn in (PluginReverseSDE.ssm, PluginReverseSDE.ssm_loss):
        prm = inspect.signature(fn).parameters
        assert prm["row_weight"].default is None, fn
    assert list(inspect.signature(PluginReverseSDE.ssm_loss).parameters) == ["self", "t_", "x", "y", "u_v", "row_weight"]
    for cls in (MLPScoreTrainer, UNetScoreTrainer):
        assert inspect.signature(cls.__init__).parameters["row_weights"].default is False
        assert inspect.signature(cls.set_data).parameters["weight"].default is None
    hdr = open(os.path.join(ROOT, "include", "msgm_hip.h")).read()
    for name in ("msgm_mlp_ssm_partial", "msgm_mlp_ssm_grad", "msgm_ssm_loss", "msgm_ssm_loss_diag"):
        old, new = _lib.SIGNATURES[name], _lib.SIGNATURES[name + "_w"]
        assert new[0] is old[0] and len(new[1]) == len(old[1]) + 1          # one more pointer: row_w after inv_batch
        k = old[1].index(_lib.C.c_float) + 1
        assert new[1][:k] == old[1][:k] and new[1][k + 1:] == old[1][k:]
        assert re.search(rf"\b{name}_w\s*\(", hdr)


def test_weights_are_refused_before_any_launch():
    """A CPU weight, a wrong length and a wrong dtype raise MsgmError from the host check every entry shares (no GPU needed:
    the check comes first)."""
    from sdeflow_light_amd import ops
    from sdeflow_light_amd._lib import MsgmError
    assert ops._row_weight(None, 4) is None
    with pytest.raises(MsgmError, match="device tensor"):
        ops._row_weight(torch.ones(4), 4)
    with pytest.raises(MsgmError, match="device tensor"):
        ops._row_weight([1.0] * 4, 4)
