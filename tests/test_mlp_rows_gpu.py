"""The fused MLP kernels (k_mlp in its tiny, narrow and wide carves, k_mlp_xw) against float64, row by row, in every
regime of the tile walk: forward, the one-step EM update and the SSM training pass (SGM closed form and the general
u / cst form) at batches of one tile, a ragged second tile, a second tile for workgroup 0 only, and two to three tiles
for every workgroup.  Bounds: tests/mlp_rows_ref.MEASURED x the float32 oracle's own error (the case's yardstick).
Also: rows of one batch that hold the same input give the same bits, nothing outside [0, B) is read or written, and two
runs agree bit for bit."""
import pytest
import torch

import mlp_rows_ref as M

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL = 40                       # rows allocated past B in the buffer-edge tests: more than one 32-row tile
SENTINEL = 12345.0

ids = lambda cases: [M.case_id(d, pre) for d, pre in cases]
_P = {}


@pytest.fixture(scope="module")
def ops():
    from sdeflow_light_amd import ops as _ops
    _ops.lib()
    return _ops


def kernel_params(ops, d, pre):
    if (d, pre) not in _P:
        keep = [M.params(d, pre)[k].to(DEV).contiguous() for k in M.NAMES]
        _P[d, pre] = (ops.mlp_params(*keep, premodule=pre is not None), keep)
    return _P[d, pre][0]


def sgm_struct():
    from sdeflow_light_amd import _lib as L
    return L.sde_struct(L.SDE_SGM, 0.1, 20.0, 1.0, 1e-3)


def dev(t):
    return t.to(DEV).contiguous()


def padded(t, fill_tail=float("nan")):
    """A [:B] view of an allocation with TAIL more rows, the tail filled with ``fill_tail``; returns (view, allocation)."""
    full = torch.full((t.shape[0] + TAIL,) + tuple(t.shape[1:]), fill_tail, dtype=torch.float32, device=DEV)
    full[:t.shape[0]] = t.to(DEV)
    return full[:t.shape[0]], full


def bits(t):
    return t.contiguous().view(torch.int32)


def run_forward(ops, d, pre, x, t):
    return ops.mlp_forward(kernel_params(ops, d, pre), dev(x), dev(t)).cpu()


def run_em(ops, d, pre, x, z, t, lmbd):
    return ops.mlp_em_step(kernel_params(ops, d, pre), dev(x).clone(), sgm_struct(), t, M.EM_DELTA, lmbd, z=dev(z)).cpu()


def run_train(ops, d, pre, i, general=False):
    """(per-sample loss, loss_sum, flat gradient) of ops.mlp_ssm_grad on the inputs i (device or host tensors)."""
    B = i["y"].shape[0]
    n = ops.mlp_num_params(d, pre is not None)
    grads, per, lsum = torch.empty(n, device=DEV), torch.empty(B, device=DEV), torch.empty(1, device=DEV)
    ws = ops.mlp_ssm_workspace(d, pre is not None, DEV)
    kw = {"u": dev(i["u"]), "cst": dev(i["cst"])} if general else {}
    ops.mlp_ssm_grad(kernel_params(ops, d, pre), dev(i["y"]), dev(i["t"]).reshape(-1), dev(i["v"]), sgm_struct(), 1.0 / B, grads, ws,
                     per, lsum, **kw)
    return per.cpu(), float(lsum), grads.cpu()


def train_batch(d, pre, B):
    return {k: w[:B] for k, w in M.train_inputs(d, pre).items()}


def fwd_grid(cases, batches=lambda d, pre: M.fwd_batches(d, pre)):
    return [pytest.param(d, pre, B, id=f"{M.case_id(d, pre)}-{B}") for d, pre in cases for B in batches(d, pre)]


def test_cases_pin_their_class():
    """launch_mlp's dispatch restated (extra-wide: d > 30 or in_dim > 32; wide: in_dim > 16 or d > 16; tiny: in_dim <= 4
    and d <= 4): each case sits where the case list says, so both sides of every class edge are run."""
    want = {"tiny": M.CASES[:3], "narrow": M.CASES[3:7], "wide": M.CASES[7:12], "xwide": M.CASES[12:]}
    for k, cases in want.items():
        for d, pre in cases:
            i = d + 1 + (1 if pre else 0)
            got = "xwide" if (d > 30 or i > 32) else ("wide" if (i > 16 or d > 16) else ("tiny" if (i <= 4 and d <= 4) else "narrow"))
            assert got == k == M.klass(d, pre), (d, pre, got)
    assert M.CASES[2] == (2, M.PRE) and M.CASES[7] == (15, M.PRE) and M.CASES[11:13] == ((30, M.PRE), (31, None))


# ------------------------------------------------------------------------------------------------ a. forward
@pytest.mark.parametrize("d,pre,B", fwd_grid(M.CASES))
def test_forward_rows(ops, d, pre, B):
    i = M.fwd_inputs(d, pre)
    out = run_forward(ops, d, pre, i["x"][:B], i["t"][:B])
    assert torch.isfinite(out).all()
    got = M.rows_metrics("fwd", out, M.fwd_ref(d, pre)[:B])
    bad = M.judge(d, pre, f"fwd/{M.case_id(d, pre)}/B={B}", got, M.yardstick(d, pre, "fwd"), ("fwd_worst", "fwd_rel"))
    assert not bad, (M.klass(d, pre), got, bad)


# ------------------------------------------------------------------------------------------------ b. one EM step
@pytest.mark.parametrize("t,lmbd", M.EM_POINTS)
@pytest.mark.parametrize("d,pre,B", fwd_grid(M.EM_CASES, lambda d, pre: M.fwd_batches(d, pre)[2:]))
def test_em_step_rows(ops, d, pre, B, t, lmbd):
    i = M.fwd_inputs(d, pre)
    out = run_em(ops, d, pre, i["x"][:B], i["z"][:B], t, lmbd)
    assert torch.isfinite(out).all()
    got = M.rows_metrics("em", out, M.em_ref(d, pre, t, lmbd)[:B])
    bad = M.judge(d, pre, f"em/{M.case_id(d, pre)}/B={B}/t={t}/lmbd={lmbd}", got, M.yardstick(d, pre, "em", (t, lmbd)),
                  ("em_worst", "em_rel"))
    assert not bad, (M.klass(d, pre), got, bad)


# ------------------------------------------------------------------------------------------------ c, d. training
def check_training(ops, d, pre, B, general):
    mode = "ssm_general" if general else "ssm"
    per, lsum, flat = run_train(ops, d, pre, train_batch(d, pre, B), general)
    assert torch.isfinite(per).all() and torch.isfinite(flat).all()
    loss64, per64, g64 = M.train_ref(d, pre, B, general)
    got = M.train_metrics(per, M.split_flat(flat, d, pre), per64, g64)
    yard = M.yardstick(d, pre, mode)
    what = f"{mode}/{M.case_id(d, pre)}/B={B}"
    bad = M.judge(d, pre, what, got, yard, ("loss_worst", "loss_rel", "grad_flat", "grad_tensor", "grad_wrow"))
    if B >= 4097:               # in the yardstick's own regime the gradients also keep the project's default slack
        bad += M.judge(d, pre, what, got, yard, ("grad_flat", "grad_tensor", "grad_wrow"), M.DEFAULTS)
    lbound = M.loss_sum_bound(per64, yard["loss_rel"], M.MEASURED[M.table(d, pre)]["loss_rel"])
    print(f"    {what} loss_sum error {abs(lsum - float(loss64)):.3e} bound {lbound:.3e}; worst tensor "
          f"{got['grad_tensor_name']}, worst weight row {got['grad_wrow_name']}, worst loss row {got['loss_row']}")
    assert not bad, (M.klass(d, pre), got, bad)
    assert abs(lsum - float(loss64)) <= lbound


@pytest.mark.parametrize("d,pre,B", fwd_grid(M.CASES, lambda d, pre: M.TRAIN_BATCHES))
def test_training_rows(ops, d, pre, B):
    check_training(ops, d, pre, B, False)


@pytest.mark.parametrize("d,pre,B", fwd_grid(M.GENERAL_CASES, lambda d, pre: M.GENERAL_BATCHES))
def test_training_general_form_rows(ops, d, pre, B):
    check_training(ops, d, pre, B, True)


# ------------------------------------------------------------------------------------------------ e. position independence
def same_rows(t):
    return torch.equal(bits(t), bits(t[:1].expand_as(t)))


@pytest.mark.parametrize("d,pre", M.CLASS_CASES, ids=ids(M.CLASS_CASES))
@pytest.mark.parametrize("mode", ["fwd", "em", "ssm"])
def test_equal_rows_give_equal_bits(ops, d, pre, mode):
    """Rows never interact and every row of a tile runs the same instruction sequence: a batch that repeats one row
    gives one output row, whatever the tile, the workgroup and the place in the tile."""
    if mode == "ssm":
        B = M.TRAIN_BATCHES[-1]
        rep = {k: w[3:4].expand(B, *w.shape[1:]).contiguous() for k, w in M.train_inputs(d, pre).items()}
        per, _, flat = run_train(ops, d, pre, rep)
        assert torch.isfinite(per).all() and torch.isfinite(flat).all()
        assert same_rows(per)
        return
    B = M.fwd_batches(d, pre)[-1]
    rep = {k: w[3:4].expand(B, *w.shape[1:]).contiguous() for k, w in M.fwd_inputs(d, pre).items()}
    out = run_forward(ops, d, pre, rep["x"], rep["t"]) if mode == "fwd" else run_em(ops, d, pre, rep["x"], rep["z"], 0.75, 0.5)
    assert torch.isfinite(out).all()
    assert same_rows(out)


# ------------------------------------------------------------------------------------------------ f. buffer edges
def edge_grid():
    g = []
    for d, pre in M.CLASS_CASES:
        for mode in ("fwd", "em"):
            g += [pytest.param(mode, d, pre, B, id=f"{mode}-{M.case_id(d, pre)}-{B}") for B in (1, 33, 32 * M.fwd_cap(d, pre) + 1)]
        g += [pytest.param("ssm", d, pre, B, id=f"ssm-{M.case_id(d, pre)}-{B}") for B in (17, 4097)]
    return g


@pytest.mark.parametrize("mode,d,pre,B", edge_grid())
def test_buffer_edges(ops, mode, d, pre, B):
    """Inputs are [:B] views whose allocation goes on with NaN rows, outputs [:B] views filled with NaN whose allocation
    goes on with a sentinel: afterwards every row under B is finite and no bit past B has changed (the ok / live guards
    of raw_issue and build_h0, the stores of the output and loss phases)."""
    from sdeflow_light_amd import _lib as L
    P = kernel_params(ops, d, pre)
    if mode == "ssm":
        i = {k: padded(w)[0] for k, w in train_batch(d, pre, B).items()}
        per, per_all = padded(torch.full((B,), float("nan")), SENTINEL)
        n = ops.mlp_num_params(d, pre is not None)
        grads, lsum = torch.full((n,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
        ws = ops.mlp_ssm_workspace(d, pre is not None, DEV)
        ops.mlp_ssm_grad(P, i["y"], i["t"].reshape(-1), i["v"], sgm_struct(), 1.0 / B, grads, ws, per, lsum)
        assert torch.isfinite(per_all[:B]).all() and torch.isfinite(grads).all() and torch.isfinite(lsum).all()
        assert torch.equal(bits(per_all[B:]), bits(torch.full_like(per_all[B:], SENTINEL)))
        return
    i = {k: w[:B] for k, w in M.fwd_inputs(d, pre).items()}
    if mode == "fwd":
        x, t = padded(i["x"])[0], padded(i["t"])[0]
        out, out_all = padded(torch.full((B, d), float("nan")), SENTINEL)
        L.check(L.lib().msgm_mlp_forward(P, L.ptr(x), L.ptr(t), L.ptr(out), B, L.stream()), "msgm_mlp_forward")
    else:                       # the state is input and output: its allocation goes on with the sentinel, z with NaN
        out, out_all = padded(i["x"], SENTINEL)
        ops.mlp_em_step(P, out, sgm_struct(), 0.75, M.EM_DELTA, 0.5, z=padded(i["z"])[0])
    assert torch.isfinite(out_all[:B]).all()
    assert torch.equal(bits(out_all[B:]), bits(torch.full_like(out_all[B:], SENTINEL)))


# ------------------------------------------------------------------------------------------------ g. determinism
def test_two_runs_agree_bitwise(ops):
    d, pre = 30, M.PRE
    a, b = (run_train(ops, d, pre, train_batch(d, pre, M.TRAIN_BATCHES[-1])) for _ in range(2))
    assert torch.equal(bits(a[0]), bits(b[0])) and a[1] == b[1] and torch.equal(bits(a[2]), bits(b[2]))
    d, pre = 17, None
    i = M.fwd_inputs(d, pre)
    a, b = (run_forward(ops, d, pre, i["x"], i["t"]) for _ in range(2))
    assert a.shape[0] == 32871 and torch.equal(bits(a), bits(b))
