"""-m gpu: the data stage (csrc/data_kernels.hip) from the C ABI up to the trainers.

Gather and fused prep: to the bit — against table[idx] with idx from the numpy restatement of the index rule
(tests/data_stage_ref.py), and against msgm_data_gather + msgm_ssm_prep from the same stream state.

Synthetic samplers with injected draws: the truth is the float64 restatement of data_stage_ref.synth, the yardstick the same
restatement in float32; the kernel may be no further from the truth in rel-L2 than 2 x the yardstick's own distance (the
margin conftest.parity_vs_fp64 uses).  Every measured ratio is printed.

Trainers: a trainer with data=ArrayData against a fixed-batch trainer fed the restated rows before every step, to the bit.
"""
import numpy as np
import pytest
import torch

import data_stage_ref as R
from test_host_gpu import make_gen

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 11


@pytest.fixture(scope="module")
def ops():
    from sdeflow_light_amd import ops as _ops
    _ops.lib()
    return _ops


@pytest.fixture(scope="module")
def L():
    from sdeflow_light_amd import _lib
    return _lib


_TABLES = {}


def table(N, d):
    """Row i holds i + o / 1024 at column o (exact in float32); made once per shape."""
    if (N, d) not in _TABLES:
        if d >= 1024:
            _TABLES.clear()
        _TABLES[(N, d)] = (torch.arange(N, device=DEV, dtype=torch.float32)[:, None]
                           + torch.arange(d, device=DEV, dtype=torch.float32)[None, :] / 1024.0).contiguous()
    return _TABLES[(N, d)]


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


# ------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("d", [1, 2, 3, 6, 30, 257, 1024, 12288])
def test_gather_is_table_of_restated_index(ops, L, d):
    for N in (1, 3, 1000):
        tab = table(N, d)
        for B in ((33,) if d == 12288 else (1, 1000)):
            for off in (0, 7):
                rng = L.PhiloxState(SEED, DEV, offset=off)
                idx = torch.from_numpy(R.gather_index(SEED, off, 0, B, N)).to(DEV)
                x, io = nan(B, d), torch.full((B,), -1, dtype=torch.int32, device=DEV)
                ops.data_gather(tab, x, rng=rng, idx_out=io)
                assert torch.equal(io.long(), idx), (N, B, off)
                assert torch.equal(x, tab[idx]), (N, B, off)
                assert rng.state_dict()["offset"] == off                       # not advanced
                x2, io2 = nan(B, d), torch.full((B,), -1, dtype=torch.int32, device=DEV)
                ops.data_gather(tab, x2, idx=io, idx_out=io2)                   # the injected-index route
                assert torch.equal(x2, x) and torch.equal(io2, io)


def test_gather_unaligned_and_clamped(ops, L):
    """A 16-byte-unaligned table or batch at d % 4 == 0 takes the dword path: same bits.  Injected rows outside [0, N) are
    clamped, never read."""
    N, B, d = 50, 37, 8
    tab = table(N, d)
    buf = torch.empty(N * d + 4, device=DEV)
    tab_u = buf[1:1 + N * d].view(N, d)
    tab_u.copy_(tab)
    xbuf = torch.full((B * d + 4,), float("nan"), device=DEV)
    x_u = xbuf[1:1 + B * d].view(B, d)
    assert tab_u.data_ptr() % 16 == 4 and x_u.data_ptr() % 16 == 4
    rng = L.PhiloxState(SEED, DEV)
    want = tab[torch.from_numpy(R.gather_index(SEED, 0, 0, B, N)).to(DEV)]
    assert torch.equal(ops.data_gather(tab_u, nan(B, d), rng=rng), want)
    assert torch.equal(ops.data_gather(tab, x_u, rng=rng), want)
    assert bool(torch.isnan(xbuf[0])) and bool(torch.isnan(xbuf[1 + B * d:]).all())
    bad = torch.tensor([-5, 0, N - 1, N, 2 ** 31 - 1] + [1] * (B - 5), dtype=torch.int32, device=DEV)
    out = torch.empty(B, dtype=torch.int32, device=DEV)
    x = ops.data_gather(tab, nan(B, d), idx=bad, idx_out=out)
    assert out[:5].tolist() == [0, 0, N - 1, N - 1, N - 1] and torch.equal(x, tab[out.long()])


@pytest.mark.parametrize("d", [2, 3, 1024])
def test_gather_shards_are_the_whole_call(ops, L, d):
    N = 1000
    tab = table(N, d)
    whole = ops.data_gather(tab, nan(128, d), rng=L.PhiloxState(SEED, DEV))
    for base in (0, 64):
        part = ops.data_gather(tab, nan(64, d), rng=L.PhiloxState(SEED, DEV, row_base=base, n=d))
        assert torch.equal(part, whole[base:base + 64])


# ------------------------------------------------------------------------------------------------------- fused prep
@pytest.mark.parametrize("d", [2, 3, 1024])
@pytest.mark.parametrize("B", [33, 1000])
def test_fused_prep_is_gather_then_prep(ops, L, d, B):
    N = 777
    tab = table(N, d) * 0.01 - 3.0
    st = L.sde_struct(L.SDE_SGM, 0.1, 20.0, 1.0, 1e-3)
    out = {}
    for route in ("fused", "two"):
        rng = L.PhiloxState(SEED, DEV, offset=5)
        x, y, t, v = nan(B, d), nan(B, d), nan(B), nan(B, d)
        ctr = torch.full((1,), 41, dtype=torch.int64, device=DEV)
        if route == "fused":
            ops.ssm_prep_gather(tab, x, y, t, v, st, rng, ctr)
        else:
            ops.data_gather(tab, x, rng=rng)
            L.check(L.lib().msgm_ssm_prep(x.data_ptr(), y.data_ptr(), t.data_ptr(), v.data_ptr(), B, d, st, rng.ptr(),
                                          ctr.data_ptr(), L.stream()), "msgm_ssm_prep")
        assert int(ctr.item()) == 42 and rng.state_dict()["offset"] == 5
        out[route] = (x, y, t, v)
    for a, b, nm in zip(out["fused"], out["two"], "xytv"):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), nm
    assert torch.equal(out["fused"][0], tab[torch.from_numpy(R.gather_index(SEED, 5, 0, B, N)).to(DEV)])


# --------------------------------------------------------------------------------------- synthetic, injected draws
def draws(kind, B, d, seed):
    """Injected draws on the CPU.  Cauchy uniforms carry the edge integers k = 0, 1, 2^23 - 1, 2^23, 2^24 - 1 in front."""
    g = torch.Generator().manual_seed(seed)
    if kind == "swiss":
        return dict(u=torch.rand(B, generator=g), z=torch.randn(B, 2, generator=g))
    if kind == "gaussian":
        return dict(z=torch.randn(B, d, generator=g))
    edge = torch.tensor(R.CAUCHY_EDGE_K, dtype=torch.float32) / R.K24
    if kind == "cauchy":
        u = torch.rand(B, d, generator=g)
        u.view(-1)[:5] = edge
        return dict(u=u)
    return dict(z=torch.randn(B, d, generator=g), u=torch.rand(1, generator=g))


def parity(ops, what, kind, B, d, A, seed=5):
    dr = draws(kind, B, d, seed)
    x = ops.data_synth(kind, nan(B, d), A=None if A is None else A.to(DEV), **{k: v.to(DEV) for k, v in dr.items()})
    assert bool(torch.isfinite(x).all()), what
    truth, yard = R.synth(kind, torch.float64, A=A, **dr), R.synth(kind, torch.float32, A=A, **dr)
    ek, ey = R.rel_l2(x, truth), R.rel_l2(yard, truth)
    print(f"data_synth {what}: kernel {ek:.3e} | float32 restatement {ey:.3e} | ratio {ek / ey if ey else 0.0:.3f} (bound 2)")
    assert ek <= 2.0 * ey, (what, ek, ey)
    return x, dr


def test_swiss_roll_parity(ops):
    parity(ops, "swiss B=1000", "swiss", 1000, 2, None)


@pytest.mark.parametrize("kind", ["gaussian", "cauchy", "gaussian_cauchy"])
@pytest.mark.parametrize("d", [2, 5, 32, 128])
def test_linear_samplers_parity(ops, kind, d):
    A = torch.randn(d, d, generator=torch.Generator().manual_seed(d))
    for name, a in (("correlated", A), ("identity", None)):
        parity(ops, f"{kind} d={d} {name} B=257", kind, 257, d, a)


@pytest.mark.parametrize("kind", ["gaussian", "cauchy", "gaussian_cauchy"])
def test_identity_parity_at_1024(ops, L, kind):
    parity(ops, f"{kind} d=1024 identity B=257", kind, 257, 1024, None)
    with pytest.raises(L.MsgmError):                                       # a dense A stops at d = 128
        ops.data_synth(kind, nan(4, 129), A=torch.eye(129, device=DEV), rng=L.PhiloxState(1, DEV))


def test_cauchy_is_finite_at_the_edges_and_antisymmetric(ops):
    B, d = 257, 2
    x, dr = parity(ops, "cauchy edges", "cauchy", B, d, None)
    k = (dr["u"].double() * R.K24).long()
    assert k.view(-1)[:5].tolist() == list(R.CAUCHY_EDGE_K)
    mirror = ((R.K24 - 1 - k).float() / R.K24).to(DEV)
    xm = ops.data_synth("cauchy", nan(B, d), u=mirror)
    assert bool(torch.isfinite(xm).all()) and torch.equal(xm, -x)
    head = x.view(-1)[:5].tolist()
    assert head[0] < -1e5 and head[4] > 1e5 and head[2] < 0 < head[3] and abs(head[2]) < 1e-8


# --------------------------------------------------------------------------------------------- synthetic, Philox
SYNTH = [("swiss", 2, False), ("gaussian", 5, True), ("gaussian", 1024, False), ("cauchy", 6, True), ("cauchy", 30, False),
         ("gaussian_cauchy", 5, True), ("gaussian_cauchy", 6, False)]


@pytest.mark.parametrize("kind,d,dense", SYNTH)
def test_philox_draws_repeat_advance_and_shard(ops, L, kind, d, dense):
    A = torch.randn(d, d, generator=torch.Generator().manual_seed(1)).to(DEV) if dense else None
    run = lambda rng, B: ops.data_synth(kind, nan(B, d), A=A, rng=rng)
    rng = L.PhiloxState(SEED, DEV)
    a, b = run(rng, 128), run(rng, 128)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    rng.advance(1)
    c = run(rng, 128)
    assert not torch.equal(a, c) and float((a != c).float().mean()) > 0.99
    for base in (0, 64):
        part = run(L.PhiloxState(SEED, DEV, row_base=base, n=d), 64)
        assert torch.equal(part, a[base:base + 64]), base
    if kind == "gaussian_cauchy" and not dense:
        # x = (z / 50) s with ONE s per call: the same scalar in both shards and in the whole call
        z = ops.data_synth("gaussian", nan(128, d), rng=L.PhiloxState(SEED, DEV))
        s = (a.double() / (0.02 * z.double())).reshape(-1)
        assert float((s.max() - s.min()).abs()) <= 1e-5 * float(s.abs().max())


def test_gaussian_covariance(ops, L):
    """d = 5, B = 65 536: every entry of X^T X / B within 5 standard errors of A A^T; for a zero-mean Gaussian
    Var(x_i x_j) = S_ii S_jj + S_ij^2."""
    from sdeflow_light_amd.data import Gaussian
    torch.manual_seed(2)
    smp = Gaussian(5, True, device=DEV, seed=4)
    x = smp.sample(65536).double().cpu()
    S = (smp.A.double() @ smp.A.double().T)
    se = torch.sqrt((torch.diag(S)[:, None] * torch.diag(S)[None, :] + S * S) / x.shape[0])
    dev = ((x.T @ x / x.shape[0] - S).abs() / se)
    print(f"gaussian covariance: worst entry at {float(dev.max()):.2f} standard errors")
    assert float(dev.max()) <= 5.0


def test_samplers_return_new_batches_and_advance(L):
    from sdeflow_light_amd import data as D
    tab = table(1000, 6)
    for smp in (D.SwissRoll(device=DEV), D.Cauchy(3, device=DEV), D.Gaussian(4, device=DEV), D.GaussianCauchy(4, device=DEV),
                D.ArrayData(tab, tab[:10], seed=2)):
        a, b = smp.sample(64), smp.sample(64)
        assert a.shape == (64, smp.dim) and a.is_cuda and a.dtype == torch.float32 and not torch.equal(a, b)
        assert smp.philox().state_dict()["offset"] == 2
        assert smp.sampletest(8).shape == (8, smp.dim) and smp.philox().state_dict()["offset"] == 3
    arr = D.ArrayData(tab, tab[:10], seed=2)
    sd = arr.philox().state_dict()
    assert torch.equal(arr.sample(64), tab[torch.from_numpy(R.gather_index(sd["seed"], 0, 0, 64, 1000)).to(DEV)])
    assert float(arr.sampletest(64)[:, 0].max()) < 10.0
    assert torch.equal(D.SwissRoll(device=DEV, seed=1).sample(32, 0.0), D.SwissRoll(device=DEV, seed=1).sampletest(32, noise=0.0))


# ------------------------------------------------------------------------------------------------------- trainers
def build(kind, B, data=None, seed=3, **kw):
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    torch.manual_seed(7)
    if kind == "mlp_sgm":
        return MLPScoreTrainer(make_gen("sgm", MLP(2)), B, lr=1e-3, seed=seed, data=data, **kw)
    if kind == "mlp_sparse":
        return MLPScoreTrainer(make_gen("sparse", MLP(6, premodule="NormalizeLogRadius"), n=6, nsf=4), B, lr=1e-3, seed=seed,
                               data=data, **kw)
    from sdeflow_light_amd.NNUnet1D import UNet1D
    return UNetScoreTrainer(make_gen("sgm", UNet1D(input_dim=8)), B, 8, lr=1e-3, seed=seed, data=data, **kw)


CASES = [("mlp_sgm", 2, 1024), ("mlp_sparse", 6, 160), ("unet1d", 8, 8)]


def data_table(d):
    return (torch.randn(500, d, generator=torch.Generator().manual_seed(d)) * 1.5).to(DEV)


@pytest.mark.parametrize("kind,d,B", CASES)
def test_trainer_with_array_data_is_the_fed_trainer(ops, kind, d, B):
    from sdeflow_light_amd.data import ArrayData
    tab = data_table(d)
    P, Q = build(kind, B, data=ArrayData(tab)), build(kind, B)
    prev = None
    for k in range(4):
        idx = torch.from_numpy(R.state_index(P.rng, B, tab.shape[0])).to(DEV)       # the rows step k draws
        assert Q.rng.state_dict() == P.rng.state_dict()
        Q.set_data(tab[idx])
        lp, lq = P.step().clone(), Q.step().clone()
        assert torch.equal(P.x, tab[idx]), k
        assert bool(torch.isfinite(lp).all()) and torch.equal(lp, lq), k
        assert torch.equal(P.flat, Q.flat), k
        assert prev is None or not torch.equal(prev, P.x)
        prev = P.x.clone()
    assert set(ops.graph_node_kinds(P.graph)) == {"kernel"}
    if kind != "mlp_sparse":                         # the gather rides in the prep launch: a fixed-batch step's launch count
        assert ops.graph_node_kinds(P.graph) == ops.graph_node_kinds(Q.graph)


def test_trainer_with_swiss_roll(ops):
    from sdeflow_light_amd.data import SwissRoll
    tr = build("mlp_sgm", 1024, data=SwissRoll())
    seen = []
    for _ in range(4):                               # the capture's eager step, then 3 replays
        assert bool(torch.isfinite(tr.step()).all())
        seen.append(tr.x.clone())
    assert all(not torch.equal(a, b) for a, b in zip(seen, seen[1:])) and bool(torch.isfinite(tr.x).all())
    assert set(ops.graph_node_kinds(tr.graph)) == {"kernel"}


def test_resume_draws_the_batches_of_the_uninterrupted_run():
    from sdeflow_light_amd.data import ArrayData
    tab = data_table(2)
    A, Bt = build("mlp_sgm", 256, data=ArrayData(tab)), build("mlp_sgm", 256, data=ArrayData(tab))
    for _ in range(4):
        A.step()
    for _ in range(2):
        Bt.step()
    sd, net = Bt.state_dict(), {k: v.clone() for k, v in Bt.gen_sde.state_dict().items()}
    assert set(sd) == {"state", "param_groups", "philox"}                # the keys a trainer without data= writes
    C = build("mlp_sgm", 256, data=ArrayData(tab))
    C.gen_sde.load_state_dict(net)
    C.load_state_dict(sd)
    for _ in range(2):
        C.step()
    assert torch.equal(C.flat, A.flat) and torch.equal(C.x, A.x)


def test_set_data_and_dim_mismatch_raise(L):
    from sdeflow_light_amd.data import ArrayData, Gaussian
    tab = data_table(2)
    P = build("mlp_sgm", 64, data=ArrayData(tab))
    with pytest.raises(L.MsgmError, match="set_data"):
        P.set_data(tab[:64])
    with pytest.raises(L.MsgmError, match="dim"):
        build("mlp_sgm", 64, data=Gaussian(3, device=DEV))
    with pytest.raises(L.MsgmError, match="dim"):
        build("unet1d", 8, data=ArrayData(tab))


@pytest.mark.parametrize("kind,d,B", CASES[::2])
def test_trainer_without_data_keeps_its_batch(kind, d, B):
    tr = build(kind, B)
    x = torch.randn(B, d, generator=torch.Generator().manual_seed(1)).to(DEV)
    tr.set_data(x)
    for _ in range(3):
        tr.step()
    assert torch.equal(tr.x, x) and tr.data is None
