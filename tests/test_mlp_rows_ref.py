"""CPU checks of tests/mlp_rows_ref.py: the class rule and batch lists, the conditions the hash fill must meet, the
general-form oracle, and the mutation test — the float32 oracle with one planted fault stands in for the kernel and must
fall outside the committed constants of MEASURED by a factor 2, where the whole-tensor bounds of
tests/test_kernels_gpu.py (1e-5 forward, 2e-5 loss, 1e-4 flat gradient, against the float32 oracle) let it through."""
import pytest
import torch

from conftest import rel_l2
import mlp_rows_ref as M
from mlp_rows_ref import PRE

F32 = torch.float32
IDS = [M.case_id(d, pre) for d, pre in M.CASES]


def test_class_rule_and_batch_lists():
    want = {"tiny": [(1, None), (3, None), (2, PRE)], "narrow": [(3, PRE), (4, None), (15, None), (14, PRE)],
            "wide": [(15, PRE), (16, None), (17, None), (30, None), (30, PRE)], "xwide": [(31, None), (128, PRE)]}
    assert [c for k in ("tiny", "narrow", "wide", "xwide") for c in want[k]] == list(M.CASES)
    for k, cases in want.items():
        for d, pre in cases:
            assert M.klass(d, pre) == k, (d, pre)
    assert M.fwd_batches(15, None)[-2:] == (16385, 32871)
    assert M.fwd_batches(3, None)[-2:] == (24577, 49255)
    assert M.fwd_batches(31, None)[-2:] == (8193, 16487)
    assert sorted(M.klass(d, pre) for d, pre in M.CLASS_CASES) == ["narrow", "tiny", "wide", "xwide"]
    assert set(M.EM_CASES) | set(M.GENERAL_CASES) | set(M.CLASS_CASES) <= set(M.CASES)


def test_constants_follow_the_rule():
    """No constant under the project's default (2 for a norm, 4 for a worst-of-many); how far above it one may rise is
    decided by test_mutations_are_rejected."""
    assert set(M.MEASURED["k_mlp"]) == set(M.DEFAULTS)
    assert set(M.MEASURED["xw"]) == {f for f in M.DEFAULTS if not f.startswith("em_")}      # test b has no extra-wide case
    for tab in M.MEASURED.values():
        for f, c in tab.items():
            assert c >= M.DEFAULTS[f] and round(c, 1) == c, (f, c)


@pytest.mark.parametrize("d,pre", M.CASES, ids=IDS)
def test_fill_conditions(d, pre):
    """Under the hash fill no gradient tensor is under 3e-2 of the largest (FLOOR_FRAC never engages), and the float32
    oracle's worst forward row is within 25x its median row at the largest batch, so the worst row is a stable yardstick.

    MLP(128, NormalizeLogRadius) meets the first condition through the weight gain of mlp_rows_ref.GAIN (1.17e-1; 2.57e-2
    at gain 1); the other thirteen cases lie between 3.76e-2 and 5.51e-2 at gain 1.  The spread of the second condition
    is 1.4x to 8x except for MLP(1, None), where a row is one number: 23.5x with the seed in use, 19.8x to
    27.6x over six seeds."""
    _, _, g64 = M.train_ref(d, pre, M.TRAIN_BATCHES[-1])
    frac = M.smallest_tensor_fraction(g64)
    err = M.row_errors(M.fwd_ref(d, pre, F32), M.fwd_ref(d, pre))
    spread = float(err.max() / err.median())
    print(f"MLP({d}, {pre}): smallest gradient tensor {frac:.2e} of the largest; float32 forward worst row {float(err.max()):.2e} "
          f"= {spread:.1f} x the median row")
    assert frac >= 3e-2
    assert spread <= 25.0


@pytest.mark.parametrize("d,pre", [(3, None), (15, PRE)])
def test_general_form_equals_closed_form_on_sgm(d, pre):
    """u = sqrt(beta) v, cst = beta |v|^2 / 2 turns the general form into the SGM closed form (float64)."""
    B = 257
    i = {k: w[:B].double() for k, w in M.train_inputs(d, pre).items()}
    beta = M.S.beta(M.S.SdeSpec(), i["t"])
    loss, per, g = M.ssm_general(M.params(d, pre), i["t"], i["y"], i["v"], beta.sqrt() * i["v"],
                                 (0.5 * beta * i["v"] ** 2).sum(1), pre, torch.float64)
    loss0, per0, g0 = M.ssm(M.params(d, pre), i["t"], i["y"], i["v"], pre, torch.float64)
    assert M.row_cmp(per, per0)[1] <= 1e-12
    assert abs(float(loss - loss0)) <= 1e-12 * abs(float(loss0))
    assert max(rel_l2(g[k], g0[k]) for k in M.NAMES) <= 1e-12


# ------------------------------------------------------------------------------------------------ mutation test
FWD_CASE, TRAIN_CASE = (15, None), (15, PRE)
FWD_FAMILIES = ("fwd_worst", "fwd_rel")
TRAIN_FAMILIES = ("loss_worst", "loss_rel", "grad_flat", "grad_tensor", "grad_wrow")


def _row_grads(r):
    """Row r's share of the float32 mean gradient at the training case's largest batch."""
    d, pre = TRAIN_CASE
    B = M.TRAIN_BATCHES[-1]
    i = M.train_inputs(d, pre)
    _, _, g = M.ssm(M.params(d, pre), i["t"][r:r + 1], i["y"][r:r + 1], i["v"][r:r + 1], pre, F32)
    return {k: w / B for k, w in g.items()}


def _forward_faults():
    d, pre = FWD_CASE
    i = M.fwd_inputs(d, pre)
    out32 = M.fwd_ref(d, pre, F32)
    B = out32.shape[0]
    big = int(torch.nonzero(out32.norm(dim=1) >= out32.norm(dim=1).pow(2).mean().sqrt())[0])   # first row of at least rms norm
    f = {}
    o = out32.clone()
    o[big] += 2e-5 * o[big].norm() * torch.nn.functional.normalize(torch.ones(d), dim=0)
    f["one forward row off by 2e-5 of its norm"] = o
    o = out32.clone()
    o[B - 1] = M.forward(M.params(d, pre), i["x"][B - 1:], i["t"][B - 2:B - 1], pre, F32)[0]
    f["last live row at its neighbour's time"] = o
    o = out32.clone()
    o[[31, 32]] = o[[32, 31]]
    f["rows 31 and 32 swapped"] = o
    return out32, f


def _training_faults():
    d, pre = TRAIN_CASE
    B = M.TRAIN_BATCHES[-1]
    _, per32, g32 = M.train_ref(d, pre, B, False, F32)
    last = _row_grads(B - 1)
    big = int(torch.nonzero(per32.abs() >= per32.pow(2).mean().sqrt())[0])
    f = {}
    f["one row's gradient weighted 1.01"] = (per32, {k: g32[k] + 0.01 * last[k] for k in g32})
    p = per32.clone()
    p[big] *= 1.0 + 1e-5
    f["one per-sample loss off by 1e-5"] = (p, g32)
    g = {k: w.clone() for k, w in g32.items()}
    g["main.2.weight"][77] *= 1.0 + 1e-4
    f["row 77 of dW2 scaled by 1 + 1e-4"] = (per32, g)
    f["last row dropped from the gradient sum"] = (per32, {k: g32[k] - last[k] for k in g32})
    return per32, g32, f


def test_mutations_are_rejected():
    """Every planted fault lies outside the committed constants — of either class of MEASURED, on the yardsticks of
    MLP(15) forward at B = 32 871 and MLP(15, NormalizeLogRadius) training at B = 8245 — by at least 2x in one family; the
    first four of the list pass the old whole-tensor bounds against the float32 oracle."""
    old_accepts, margins = {}, {}
    worst_margin = lambda got, yard, fams: min(max(got[f] / (tab[f] * yard[f]) for f in fams) for tab in M.MEASURED.values())

    d, pre = FWD_CASE
    yard, ref64 = M.yardstick(d, pre, "fwd"), M.fwd_ref(d, pre)
    out32, faults = _forward_faults()
    assert not M.judge(d, pre, "float32 oracle, forward", M.rows_metrics("fwd", out32, ref64), yard, FWD_FAMILIES)
    for name, o in faults.items():
        got = M.rows_metrics("fwd", o, ref64)
        margins[name] = worst_margin(got, yard, FWD_FAMILIES)
        old_accepts[name] = rel_l2(o, out32) <= 1e-5

    d, pre = TRAIN_CASE
    yard = M.yardstick(d, pre, "ssm")
    _, per64, g64 = M.train_ref(d, pre, M.TRAIN_BATCHES[-1])
    per32, g32, faults = _training_faults()
    flat = lambda g: torch.cat([g[k].reshape(-1) for k in M.NAMES])
    for name, (p, g) in faults.items():
        got = M.train_metrics(p, g, per64, g64)
        margins[name] = worst_margin(got, yard, TRAIN_FAMILIES)
        old_accepts[name] = rel_l2(p, per32) <= 2e-5 and rel_l2(flat(g), flat(g32)) <= 1e-4

    for name in margins:
        print(f"fault '{name}': outside the new bound by {margins[name]:.1f}x; the old whole-tensor bound "
              f"{'ACCEPTS' if old_accepts[name] else 'rejects'} it")
    assert all(m >= 2.0 for m in margins.values()), margins
    for name in ("one forward row off by 2e-5 of its norm", "one row's gradient weighted 1.01",
                 "one per-sample loss off by 1e-5", "row 77 of dW2 scaled by 1 + 1e-4"):
        assert old_accepts[name], name
