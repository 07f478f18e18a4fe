"""-m gpu: per-row weights in the SSM loss, from the kernels up to ``PluginReverseSDE.ssm`` and the trainers.

(a) exact properties of the three MLP training kernels and the two loss-seed kernels: w = 1 is the unweighted entry to the
    bit, w = c (a power of two) the unweighted entry with inv_batch * c, w = -1 its exact negation;
(b) float64 parity of the weighted gradient, per-sample loss and loss sum (conftest.parity_vs_fp64 at its default slack;
    the yardstick is the float32 oracle of tests/ssm_weights_ref.py);
(c) a non-uniform cotangent through ``ssm``: (w * gen.ssm(x)).sum().backward() against the float64 gradient of
    sum_b w_b L_b and against ssm(x, row_weight=w); .mean().backward() stays what the null-weight entry gives, to the bit;
(d) the trainers' resident weight buffer under graph replay; (e) refusals.
"""
import functools

import pytest
import torch

import mlp_rows_ref as M
import ssm_weights_ref as W
from conftest import parity_vs_fp64
from test_host_gpu import make_gen
from test_mlp_rows_gpu import bits, dev, kernel_params, sgm_struct

pytestmark = pytest.mark.gpu
DEV = "cuda"
ids = [M.case_id(d, pre) for d, pre in W.CASES]


@pytest.fixture(scope="module")
def ops():
    from sdeflow_light_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def L():
    from sdeflow_light_amd import _lib
    return _lib


def sparse_struct(L):
    return L.sde_struct(L.SDE_MSGM_SPARSE, 0.1, 20.0, 1.0, 1e-3)


# ------------------------------------------------------------------------------------------------ MLP kernels
def mlp_operands(ops, L, d, pre, form, B):
    i = W.mlp_inputs(d, pre, B)
    y, t, v = dev(i["y"]), dev(i["t"]).reshape(-1).contiguous(), dev(i["v"])
    if form == "sgm":
        return y, t, v, None, None, sgm_struct()
    st = sparse_struct(L)
    u, cst = ops.ssm_terms(y, v, t, st)
    return y, t, v, u, cst, st


def mlp_call(ops, L, d, pre, operands, inv_batch, w):
    """(flat gradient, per-sample loss, loss sum).  w None: the UNWEIGHTED C entry (msgm_mlp_ssm_grad), else the
    weighted one through ops.mlp_ssm_grad."""
    y, t, v, u, cst, st = operands
    B = y.shape[0]
    n = ops.mlp_num_params(d, pre is not None)
    nan = lambda k: torch.full((k,), float("nan"), device=DEV)
    grads, per, lsum = nan(n), nan(B), nan(1)
    ws = ops.mlp_ssm_workspace(d, pre is not None, DEV)
    P = kernel_params(ops, d, pre)
    if w is None:
        L.check(L.lib().msgm_mlp_ssm_grad(P, L.ptr(y), L.ptr(t), L.ptr(v), L.ptr(u), L.ptr(cst), B, st, float(inv_batch),
                                          L.ptr(grads), L.ptr(per), L.ptr(lsum), L.ptr(ws), ws.numel() * 4, L.stream()),
                "msgm_mlp_ssm_grad")
    else:
        ops.mlp_ssm_grad(P, y, t, v, st, inv_batch, grads, ws, per, lsum, u=u, cst=cst, row_weight=w)
    assert torch.isfinite(grads).all() and torch.isfinite(per).all() and torch.isfinite(lsum).all()
    return grads, per, lsum


def same_bits(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("d,pre", W.CASES, ids=ids)
def test_mlp_exact_properties(ops, L, d, pre, form):
    for B in W.EXACT_BATCHES:
        o = mlp_operands(ops, L, d, pre, form, B)
        s = 1.0 / B
        base = mlp_call(ops, L, d, pre, o, s, None)
        full = lambda c: torch.full((B,), c, device=DEV)
        assert same_bits(mlp_call(ops, L, d, pre, o, s, full(1.0)), base), (B, "w = 1")
        for c in (0.5, 4.0):
            assert same_bits(mlp_call(ops, L, d, pre, o, s, full(c)), mlp_call(ops, L, d, pre, o, s * c, None)), (B, c)
        g, per, lsum = mlp_call(ops, L, d, pre, o, s, full(-1.0))
        assert torch.equal(g, -base[0]) and torch.equal(lsum, -base[2]), (B, "w = -1")
        assert torch.equal(bits(per), bits(base[1])), (B, "loss_per is unweighted")
        assert float(base[0].abs().max()) > 0


@pytest.mark.parametrize("form", W.FORMS)
@pytest.mark.parametrize("d,pre", W.CASES, ids=ids)
def test_mlp_weighted_vs_float64(ops, L, d, pre, form):
    """Weights in [0.25, 4], every seventh row and the second tile at 0, B = 4097 (workgroup 0 walks two tiles)."""
    B = W.PARITY_BATCH
    w = W.weights(B)
    o = mlp_operands(ops, L, d, pre, form, B)
    out = {}

    def hip():
        g, per, lsum = mlp_call(ops, L, d, pre, o, 1.0 / B, dev(w))
        out["lsum"] = float(lsum)
        return per.cpu(), {k: x.cpu() for k, x in M.split_flat(g, d, pre).items()}

    def oracle(dt):
        _, per, g = W.mlp_weighted(d, pre, form, B, dt)
        return per, g
    e_per, _ = parity_vs_fp64(hip, oracle, f"SSMW MLP {M.case_id(d, pre)} {form} B={B}")
    l64, per64, _ = W.mlp_weighted(d, pre, form, B)
    l32, per32, _ = W.mlp_weighted(d, pre, form, B, torch.float32)
    r_per = float((per32.double() - per64).norm() / per64.norm())
    bound = W.loss_sum_bound(per64, w, max(2.0 * r_per, 1e-5), 1.0 / B)
    print(f"SSMW MLP {M.case_id(d, pre)} {form} loss_sum error {abs(out['lsum'] - float(l64)):.3e} (float32 oracle "
          f"{abs(float(l32) - float(l64)):.3e}) bound {bound:.3e}")
    assert abs(out["lsum"] - float(l64)) <= bound


# ------------------------------------------------------------------------------------------------ the two seed kernels
@pytest.mark.parametrize("B,n", W.SEED_SHAPES)
def test_seed_kernels_exact_properties(ops, L, B, n):
    g = torch.Generator().manual_seed(31 * B + n)
    rnd = lambda *s: torch.randn(*s, generator=g).to(DEV)
    out, u, cst, v = rnd(2 * B * n), rnd(B, n), rnd(B), torch.sign(rnd(B, n))
    t = torch.rand(B, generator=g).clamp_min(1e-3).to(DEV)
    st, s = sgm_struct(), 1.0 / B
    nan = lambda k: torch.full((k,), float("nan"), device=DEV)

    def generic(inv, w):
        if w is not None:
            return ops.ssm_loss(out, u, cst, inv, row_weight=w)
        per, gg = nan(B), nan(2 * B * n)
        L.check(L.lib().msgm_ssm_loss(L.ptr(out), L.ptr(u), L.ptr(cst), L.ptr(per), L.ptr(gg), B, n, float(inv), L.stream()), "msgm_ssm_loss")
        return per, gg

    def diag(inv, w):
        if w is not None:
            return ops.ssm_loss_diag(out, v, t, st, inv, row_weight=w)
        per, gg = nan(B), nan(2 * B * n)
        L.check(L.lib().msgm_ssm_loss_diag(L.ptr(out), L.ptr(v), L.ptr(t), L.ptr(per), L.ptr(gg), B, n, st, float(inv), L.stream()),
                "msgm_ssm_loss_diag")
        return per, gg

    full = lambda c: torch.full((B,), c, device=DEV)
    for fn in (generic, diag):
        base = fn(s, None)
        assert torch.isfinite(base[0]).all() and torch.isfinite(base[1]).all()
        assert same_bits(fn(s, full(1.0)), base)
        for c in (0.5, 4.0):
            assert same_bits(fn(s, full(c)), fn(s * c, None)), c
        per, gg = fn(s, full(-1.0))
        assert torch.equal(bits(per), bits(base[0])) and torch.equal(gg, -base[1])
        # rows are seeded one by one: row b of g under mixed weights is row b of the unweighted call with inv_batch * w_b
        w = torch.tensor([0.5, -2.0, 0.0, 4.0, 1.0, 0.25, 8.0, -1.0, 2.0])[:B].to(DEV)
        gm = fn(s, w)[1].view(2, B, n)
        for b in range(B):
            ref = fn(s * float(w[b]), None)[1].view(2, B, n)
            assert torch.equal(gm[:, b], ref[:, b]), b


# ------------------------------------------------------------------------------------------------ ssm() cotangents
WB = (0.25, 4.0, 0.0, 1.5)              # B = 4: positive, one row at exactly 0


def _nets(kind):
    """(gen, the oracle's score function, the oracle's SdeSpec, d): the smallest configurations of the existing GPU tests."""
    from oracle import nets_ref as N, sde_ref as S
    from sdeflow_light_amd.NN import MLP
    torch.manual_seed(13)
    if kind == "mlp_sgm":
        return make_gen("sgm", MLP(2)), (lambda p, y, t: N.mlp_forward(p, y, t)), S.SdeSpec(), 2
    if kind == "mlp_sparse":
        gen = make_gen("sparse", MLP(6, premodule=M.PRE), n=6, nsf=4)
        return gen, (lambda p, y, t: N.mlp_forward(p, y, t, M.PRE)), S.SdeSpec(kind=S.MSGM_SPARSE, n=6), 6
    if kind == "unet1d":
        from test_host_gpu import _unet1d
        return make_gen("sgm", _unet1d(64)), (lambda p, y, t: N.unet1d_forward(p, y, t, None)), S.SdeSpec(), 64
    from test_dropout_gpu import _vunet, _oracle_score
    return make_gen("sgm", _vunet(16, 0.0)), _oracle_score(16, None), S.SdeSpec(), 256


def _grads(gen):
    return {k: q.grad.detach().clone() for k, q in gen.a.named_parameters()}


@pytest.mark.parametrize("kind", ["mlp_sgm", "mlp_sparse", "unet1d", "unet2d"])
def test_nonuniform_cotangent_through_ssm(ops, L, kind):
    """Fails on a bridge that scales the stored gradient of the mean by grad_out.sum(): that is the gradient of
    mean(w) * sum(L), not of sum_b w_b L_b."""
    from oracle import sde_ref as S
    from sdeflow_light_amd.NN import MLP
    gen, score, sp, d = _nets(kind)
    net, B = gen.a, 4
    g = torch.Generator().manual_seed(5)
    x, u, eps, uv = (torch.randn(B, d, generator=g) * 1.5, torch.rand(B, generator=g), torch.randn(B, d, generator=g),
                     torch.rand(B, d, generator=g))
    w = torch.tensor(WB)
    wd = w.to(DEV)
    params = {k: q.detach().cpu().clone() for k, q in net.state_dict().items()}
    rng = gen.base_sde.philox(torch.device(DEV))
    state = rng.state_dict()
    if kind == "mlp_sparse":            # the reference's ssm_loss(t, x, y) entry: (t, y) given
        t0 = S.clamp_time(sp, u.reshape(B, 1))
        call = lambda **kw: gen.ssm_loss(t0.to(DEV), x.to(DEV), x.to(DEV), u_v=uv.to(DEV), **kw)
        t_o, y_o = t0, x
    else:
        call = lambda **kw: gen.ssm(x.to(DEV), u=u.to(DEV), eps=eps.to(DEV), u_v=uv.to(DEV), **kw)
        t_o = S.clamp_time(sp, u.reshape(B, 1))
        y_o = S.vp_perturb(sp, t_o, x, eps)
    v_o = S.rademacher_from_uniform(uv)
    torch.set_num_threads(min(16, torch.get_num_threads()))

    @functools.lru_cache(maxsize=None)
    def ref(dt):                        # (per-sample L, gradient of sum_b w_b L_b)
        _, per, gr = W.weighted(sp, score, params, t_o, y_o, v_o, w, dt, inv_batch=1.0)
        return per, gr

    def run(weighted_after):
        rng.load_state_dict(state)
        gen.zero_grad()
        if weighted_after:
            per = call()
            (wd * per).sum().backward()
        else:
            per = call(row_weight=wd)
            per.sum().backward()
        return per.detach().cpu(), {k: q.cpu() for k, q in _grads(gen).items()}

    a = run(True)
    parity_vs_fp64(lambda: a, ref, f"SSMW {kind}: (w * ssm(x)).sum().backward(), B={B}")
    b = run(False)
    parity_vs_fp64(lambda: b, lambda dt: (w.to(dt) * ref(dt)[0], ref(dt)[1]), f"SSMW {kind}: ssm(x, row_weight=w).sum().backward(), B={B}")
    assert torch.equal(b[0], (wd * a[0].to(DEV)).cpu())                    # the returned tensor is w (.) L

    # .mean().backward() stays what the null-weight entry gives, to the bit
    rng.load_state_dict(state)
    gen.zero_grad()
    call().mean().backward()
    got = torch.cat([q.grad.reshape(-1) for q in net.parameters()]).clone()
    y = dev(y_o) if kind == "mlp_sparse" else gen.sample_txy(x.to(DEV), u=u.to(DEV), eps=eps.to(DEV))[2]
    t = dev(t_o).reshape(-1) if kind == "mlp_sparse" else gen.sample_txy(x.to(DEV), u=u.to(DEV), eps=eps.to(DEV))[0].reshape(-1).contiguous()
    v = ops.rademacher((B, d), torch.device(DEV), u=uv.to(DEV))
    st = gen.base_sde.struct()
    uu = cst = None
    if kind != "mlp_sgm":
        uu, cst = ops.ssm_terms(y, v, t, st)
    if isinstance(net, MLP):
        gmean = torch.empty_like(got)
        ops.mlp_ssm_grad(net.kernel_params(), y, t, v, st, 1.0 / B, gmean, ops.mlp_ssm_workspace(d, net.pre is not None, DEV),
                         u=uu, cst=cst)
    else:
        gen.zero_grad()
        net.ssm_grad(y, t, v, uu, cst, 1.0 / B)
        gmean = net.flat_parameters()[1].clone()
    want = torch.zeros_like(gmean).add_(gmean * torch.full((B,), 1.0 / B, device=DEV).sum())
    assert float(want.abs().max()) > 0 and torch.equal(bits(got), bits(want))


def test_dropout_unet_refuses_the_second_pass_and_takes_row_weight(L):
    from test_dropout_gpu import _vunet
    torch.manual_seed(2)
    gen = make_gen("sgm", _vunet(16, 0.1))
    gen.a.train()
    assert gen.a.dropout_active()
    B, d = 4, 256
    x, w = torch.randn(B, d, device=DEV), torch.tensor(WB, device=DEV)
    gen.zero_grad()
    per = gen.ssm(x)
    with pytest.raises(L.MsgmError, match="row_weight="):
        (w * per).sum().backward()
    gen.zero_grad()
    out = gen.ssm(x, row_weight=w)
    out.sum().backward()
    flat = torch.cat([q.grad.reshape(-1) for q in gen.a.parameters()])
    assert torch.isfinite(out).all() and float(out.detach()[2]) == 0.0 and torch.isfinite(flat).all() and float(flat.abs().max()) > 0
    gen.zero_grad()
    gen.ssm(x).mean().backward()                          # the uniform cotangent still goes through with dropout


# ------------------------------------------------------------------------------------------------ trainers
def _trainer(kind, **kw):
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    torch.manual_seed(7)
    if kind == "mlp":
        gen = make_gen("sgm", MLP(2))
        tr, B, d = MLPScoreTrainer(gen, 64, lr=1e-3, seed=3, **kw), 64, 2
    else:
        from sdeflow_light_amd.NNUnet1D import UNet1D
        gen = make_gen("sgm", UNet1D(input_dim=128, base_channels=16, channel_mults=(1, 2), emb_dim=32))
        tr, B, d = UNetScoreTrainer(gen, 8, 128, lr=1e-3, seed=3, **kw), 8, 128
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(1)).to(DEV)
    return tr, x, B


@pytest.mark.parametrize("kind", ["mlp", "unet1d"])
def test_trainer_row_weights(L, kind):
    def run(weights, **kw):
        tr, x, B = _trainer(kind, **kw)
        tr.set_data(x)
        losses = []
        for k in range(3):
            losses.append(float(tr.step()))
            if weights is not None and k < 2:
                tr.set_data(x, weight=weights[k].to(DEV))
        return losses, tr.net.flat_parameters()[0].clone(), tr

    plain = run(None, row_weights=False)
    ones = run(None, row_weights=True)
    assert plain[0] == ones[0] and torch.equal(bits(plain[1]), bits(ones[1]))          # default weights change nothing
    B = plain[2].B
    g = torch.Generator().manual_seed(9)
    ws = [torch.exp2(4.0 * torch.rand(B, generator=g) - 2.0) for _ in range(2)]
    ws[1][::3] = 0.0
    graph = run(ws, row_weights=True, use_graph=True)
    eager = run(ws, row_weights=True, use_graph=False)
    assert graph[2].graph is not None and eager[2].graph is None
    assert graph[0] == eager[0] and torch.equal(bits(graph[1]), bits(eager[1]))        # replays read the resident buffer
    assert graph[0][0] == plain[0][0] and graph[0][1:] != plain[0][1:]                 # and the weights took effect
    assert not torch.equal(graph[1], plain[1])
    with pytest.raises(L.MsgmError, match="row_weights=True"):
        plain[2].set_data(plain[2].x, weight=ws[0].to(DEV))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ops, L):
    from sdeflow_light_amd.NN import MLP
    d, pre, B = 4, None, 17
    o = mlp_operands(ops, L, d, pre, "sgm", B)
    bad = (torch.ones(B), torch.ones(B + 1, device=DEV), torch.ones(B, device=DEV, dtype=torch.float64))
    out, u, cst = torch.zeros(2 * B * d, device=DEV), torch.zeros(B, d, device=DEV), torch.zeros(B, device=DEV)
    gen = make_gen("sgm", MLP(d))
    tr, x, Bt = _trainer("mlp", row_weights=True)
    for w in bad:
        with pytest.raises(L.MsgmError):
            mlp_call(ops, L, d, pre, o, 1.0 / B, w)
        with pytest.raises(L.MsgmError):
            ops.ssm_loss(out, u, cst, 1.0 / B, row_weight=w)
        with pytest.raises(L.MsgmError):
            ops.ssm_loss_diag(out, o[2], o[1], sgm_struct(), 1.0 / B, row_weight=w)
        with pytest.raises(L.MsgmError):
            gen.ssm(o[0], row_weight=w)
        with pytest.raises(L.MsgmError):
            gen.a.zero_grad()
            gen.ssm_loss(o[1], o[0], o[0], row_weight=w)
    for w in (torch.ones(Bt), torch.ones(Bt + 1, device=DEV), torch.ones(Bt, device=DEV, dtype=torch.float64)):
        with pytest.raises(L.MsgmError):
            tr.set_data(x, weight=w)
    from test_host_gpu import _unet1d
    net = _unet1d(64)
    z = torch.zeros(3, 64, device=DEV)
    for w in (torch.ones(3), torch.ones(4, device=DEV), torch.ones(3, device=DEV, dtype=torch.float64)):
        with pytest.raises(L.MsgmError):
            net.ssm_grad(z, torch.full((3,), 0.5, device=DEV), z, z, torch.zeros(3, device=DEV), 1.0 / 3, row_weight=w)
