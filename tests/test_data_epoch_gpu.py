"""-m gpu: the epoch mode of the data stage (msgm_data_gather_epoch + msgm_counter_add) from the C ABI up to
the trainers.

Gather: to the bit — idx_out against the numpy restatement of the index rule (tests/data_epoch_ref.py), x against
table[idx].  Trainers: a trainer with data=ArrayData(replace=False) against a fixed-batch trainer fed the restated rows
before every step, to the bit; the captured step's node kinds; coverage of the table; resume from a checkpoint."""
import math

import numpy as np
import pytest
import torch

import data_epoch_ref as R
from test_host_gpu import Tp, make_gen

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


def table(N, d):
    """Row i holds fl32(i + o / 1024) at column o: column 0 names the row (exact below 2^24)."""
    return (torch.arange(N, device=DEV, dtype=torch.float32)[:, None]
            + torch.arange(d, device=DEV, dtype=torch.float32)[None, :] / 1024.0).contiguous()


def nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def cursor_at(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def restated(seed, cur, base, B, N):
    return torch.from_numpy(R.batch_index(seed, cur, base, B, N)).to(DEV)


# ------------------------------------------------------------------------------------------------------------ gather
BIG = (2 ** 33 + 5) * 1000 + 7
PARITY = [(10, 24, 2, 0), (1000, 64, 3, 0), (257, 128, 1024, 0), (65537, 256, 4, 65400), (1, 8, 4, 3), (1000, 64, 4, BIG)]


@pytest.mark.parametrize("N,B,d,cur", PARITY)
def test_gather_is_table_of_restated_index(ops, L, N, B, d, cur):
    """(10, 24, 2) crosses two epoch boundaries in one call, (65537, 256, 4) at cursor 65400 one; d = 3 is the dword path,
    d = 1024 and 4 the quad path; the last case an epoch index above 2^33."""
    tab = table(N, d)
    for c0 in sorted({0, cur}):
        rng, cu = L.PhiloxState(SEED, DEV, offset=5), cursor_at(c0)
        idx = restated(SEED, c0, 0, B, N)
        x, io = nan(B, d), torch.full((B,), -1, dtype=torch.int32, device=DEV)
        ops.data_gather_epoch(tab, x, rng, cu, idx_out=io)
        assert torch.equal(io.long(), idx), (N, B, c0)
        assert torch.equal(x, tab[idx]), (N, B, c0)
        assert int(cu.item()) == c0 and rng.state_dict()["offset"] == 5           # neither is advanced


def test_gather_unaligned_takes_the_dword_path(ops, L):
    """(257, 128, 1024) with the table, then the batch, offset by one float: d % 4 == 0 but not 16-byte aligned."""
    N, B, d = 257, 128, 1024
    tab = table(N, d)
    buf = torch.empty(N * d + 4, device=DEV)
    tab_u = buf[1:1 + N * d].view(N, d)
    tab_u.copy_(tab)
    xbuf = torch.full((B * d + 4,), float("nan"), device=DEV)
    x_u = xbuf[1:1 + B * d].view(B, d)
    assert tab_u.data_ptr() % 16 == 4 and x_u.data_ptr() % 16 == 4
    rng, cu = L.PhiloxState(SEED, DEV), cursor_at(200)
    want = tab[restated(SEED, 200, 0, B, N)]
    assert torch.equal(ops.data_gather_epoch(tab_u, nan(B, d), rng, cu), want)
    assert torch.equal(ops.data_gather_epoch(tab, x_u, rng, cu), want)
    assert bool(torch.isnan(xbuf[0])) and bool(torch.isnan(xbuf[1 + B * d:]).all())


def test_one_full_epoch(ops, L):
    """N = 1000, B = 64: 16 calls cover 1024 positions — one permutation, then the head of the next."""
    N, B = 1000, 64
    tab, rng, cu = table(N, 2), L.PhiloxState(SEED, DEV), cursor_at(0)
    got = []
    for k in range(16):
        io = torch.empty(B, dtype=torch.int32, device=DEV)
        x = ops.data_gather_epoch(tab, nan(B, 2), rng, cu, idx_out=io)
        assert torch.equal(x, tab[io.long()])
        ops.counter_add(cu, B)
        got.append(io.cpu().numpy())
    assert int(cu.item()) == 1024
    got = np.concatenate(got)
    assert np.array_equal(np.sort(got[:N]), np.arange(N))
    assert np.array_equal(got, R.stream_index(SEED, np.arange(1024), N))
    assert len(set(got[N:].tolist())) == 24 and not np.array_equal(got[N:], got[:24])


def test_counter_add_adds_delta(ops, L):
    ctr = cursor_at(41)
    for delta, want in ((1, 42), (2 ** 32 + 3, 2 ** 32 + 45), (64 * 8, 2 ** 32 + 45 + 512)):
        ops.counter_add(ctr, delta)
        assert int(ctr.item()) == want
    with pytest.raises(L.MsgmError):
        ops.counter_add(ctr.int(), 1)
    with pytest.raises(L.MsgmError):
        ops.data_gather_epoch(table(4, 2), nan(2, 2), L.PhiloxState(1, DEV), ctr.int())


@pytest.mark.parametrize("d", [2, 1024])
def test_gather_shards_are_the_whole_call(ops, L, d):
    N, cur = 100, 70                                          # 128 positions from 70: two boundaries inside the call
    tab = table(N, d)
    whole = ops.data_gather_epoch(tab, nan(128, d), L.PhiloxState(SEED, DEV), cursor_at(cur))
    assert torch.equal(whole, tab[restated(SEED, cur, 0, 128, N)])
    for base in (0, 64):
        rng = L.PhiloxState(SEED, DEV)
        rng.set_shard(base, d)
        part = ops.data_gather_epoch(tab, nan(64, d), rng, cursor_at(cur))
        assert torch.equal(part, whole[base:base + 64]), base


def test_gather_does_not_depend_on_the_stream_offset(ops, L):
    N, B, d = 1000, 64, 3
    tab, rng, cu = table(N, d), L.PhiloxState(SEED, DEV), cursor_at(990)
    a = ops.data_gather_epoch(tab, nan(B, d), rng, cu)
    rng.advance(3)
    b = ops.data_gather_epoch(tab, nan(B, d), rng, cu)
    assert rng.state_dict()["offset"] == 3 and torch.equal(a, b)
    assert not torch.equal(a, ops.data_gather_epoch(tab, nan(B, d), L.PhiloxState(SEED + 1, DEV), cu))      # the seed does key it


def test_sampler_walks_the_stream(L):
    from sdeflow_light_amd.data import ArrayData
    N = 50
    tab = table(N, 4)
    smp = ArrayData(tab, tab[:5], seed=2, replace=False)
    seed = smp.philox().state_dict()["seed"]
    a, b = smp.sample(32), smp.sample(32)
    assert torch.equal(torch.cat([a, b]), tab[restated(seed, 0, 0, 64, N)])
    assert (smp.position, smp.epoch, smp.stride) == (64, 1, 1) and smp.steps_per_epoch(32) == N / 32
    assert float(smp.sampletest(64)[:, 0].max()) < 5.0 and smp.position == 64          # with replacement, from the test table
    smp.position = 7
    assert torch.equal(smp.sample(8), tab[restated(seed, 7, 0, 8, N)]) and smp.position == 15
    # replace=True stays the sampler of today
    import data_stage_ref as R0
    old = ArrayData(tab, seed=2)
    assert torch.equal(old.sample(64), tab[torch.from_numpy(R0.gather_index(seed, 0, 0, 64, N)).to(DEV)])


# ------------------------------------------------------------------------------------------------------- trainers
def build(kind, B, data=None, seed=3, **kw):
    from sdeflow_light_amd.NN import MLP
    from sdeflow_light_amd.NNUnet1D import UNet1D
    from sdeflow_light_amd.SDEs import MSGMsde, PluginReverseSDE
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    torch.manual_seed(7)
    if kind == "mlp_sgm":
        return MLPScoreTrainer(make_gen("sgm", MLP(2)), B, lr=1e-3, seed=seed, data=data, **kw)
    if kind == "mlp_sparse":
        return MLPScoreTrainer(make_gen("sparse", MLP(6, premodule="NormalizeLogRadius"), n=6, nsf=4), B, lr=1e-3, seed=seed,
                               data=data, **kw)
    if kind == "unet1d":
        net = UNet1D(input_dim=128, base_channels=16, channel_mults=(1, 2), emb_dim=32)
        return UNetScoreTrainer(make_gen("sgm", net), B, 128, lr=1e-3, seed=seed, data=data, **kw)
    T = Tp()                                                  # mlp_intT: the integrated loss under the sparse multiplicative SDE
    base = MSGMsde(torch.randn(64, 6), beta_min=0.1, beta_max=20.0, t_epsilon=0.3, T=T, num_steps_forward=4, device=DEV,
                   denseTensor=False, norm_map="log")
    gen = PluginReverseSDE(base, MLP(6, premodule="NormalizeLogRadius").to(DEV), T, ssm_intT=True, deviceReverseSDE=DEV).to(DEV)
    return MLPScoreTrainer(gen, B, lr=1e-3, seed=seed, data=data, **kw)


CASES = [("mlp_sgm", 2, 64, 100), ("mlp_sparse", 6, 32, 50), ("unet1d", 128, 8, 20), ("mlp_intT", 6, 16, 40)]


def data_table(N, d):
    return (torch.randn(N, d, generator=torch.Generator().manual_seed(d)) * 1.5).to(DEV)


def epoch_data(tab, **kw):
    from sdeflow_light_amd.data import ArrayData
    return ArrayData(tab, replace=False, **kw)


@pytest.mark.parametrize("kind,d,B,N", CASES)
def test_trainer_with_epoch_data_is_the_fed_trainer(ops, kind, d, B, N):
    tab = data_table(N, d)
    P, Q = build(kind, B, data=epoch_data(tab)), build(kind, B)
    seed = P.rng.state_dict()["seed"]
    assert P._table is None and P.data.stride == 1
    for k in range(5):
        idx = restated(seed, k * B, 0, B, N)                  # the rows step k reads
        assert Q.rng.state_dict() == P.rng.state_dict() and P.data.position == k * B
        Q.set_data(tab[idx])
        lp, lq = P.step().clone(), Q.step().clone()
        assert torch.equal(P.x, tab[idx]), k
        assert bool(torch.isfinite(lp).all()) and torch.equal(lp, lq), k
        assert torch.equal(P.flat, Q.flat), k
    assert set(ops.graph_node_kinds(P.graph)) == {"kernel"}


def test_captured_step_is_the_fixed_batch_step_plus_two_kernels(ops):
    from sdeflow_light_amd.data import ArrayData
    tab = data_table(100, 2)
    P, Q, W = build("mlp_sgm", 64, data=epoch_data(tab)), build("mlp_sgm", 64), build("mlp_sgm", 64, data=ArrayData(tab))
    for tr in (P, Q, W):
        tr.step()
    kp, kq, kw = (ops.graph_node_kinds(tr.graph) for tr in (P, Q, W))
    assert set(kp) == {"kernel"} and kp["kernel"] == kq["kernel"] + 2           # gather + cursor advance ahead of the prep launch
    # untouched behaviour: with replacement the gather still rides in the prep launch, and no checkpoint key appears
    assert kw == kq
    assert "data_cursor" not in W.state_dict() and "data_cursor" not in Q.state_dict()
    assert W._table is not None and set(W.state_dict()) == set(Q.state_dict())


def test_an_epoch_trains_on_every_row():
    N, B = 100, 64
    tab = data_table(N, 2)
    tr = build("mlp_sgm", B, data=epoch_data(tab))
    seen = []
    for _ in range(math.ceil(N / B)):
        tr.step()
        seen.append(tr.x.clone())
    x = torch.cat(seen)
    hit = (x[:, None, :] == tab[None, :, :]).all(dim=2)                         # (steps B, N): which table row is row j?
    assert bool((hit.sum(dim=1) == 1).all())                                    # every batch row is one row of the table
    rows = hit.float().argmax(dim=1)
    assert sorted(rows[:N].tolist()) == list(range(N)) and bool(hit.any(dim=0).all())


def test_resume_continues_the_epoch():
    B, N = 64, 100
    tab = data_table(N, 2)
    A, Bt = build("mlp_sgm", B, data=epoch_data(tab)), build("mlp_sgm", B, data=epoch_data(tab))
    for _ in range(6):
        A.step()
    for _ in range(3):
        Bt.step()
    sd, net = Bt.state_dict(), {k: v.clone() for k, v in Bt.gen_sde.state_dict().items()}
    assert set(sd) == {"state", "param_groups", "philox", "data_cursor"} and sd["data_cursor"] == 3 * B
    assert isinstance(sd["data_cursor"], int)
    C = build("mlp_sgm", B, data=epoch_data(tab))
    C.gen_sde.load_state_dict(net)
    C.load_state_dict(sd)
    assert C.data.position == 3 * B
    for _ in range(3):
        C.step()
    assert torch.equal(C.flat, A.flat) and torch.equal(C.x, A.x) and C.data.position == 6 * B == A.data.position
    # a checkpoint without the key starts the data order over; one with the key loads into a trainer without the sampler
    old = {k: v for k, v in sd.items() if k != "data_cursor"}
    C.load_state_dict(old)
    assert C.data.position == 0
    build("mlp_sgm", B).load_state_dict(sd)


def test_refusals(ops, L):
    tab = data_table(100, 2)
    smp = epoch_data(tab)
    P = build("mlp_sgm", 64, data=smp)
    with pytest.raises(L.MsgmError, match="set_data"):
        P.set_data(tab[:64])
    with pytest.raises(L.MsgmError, match="world"):                            # the trainer bound it with world = 1
        smp.bind(2)
    P.step()
    ctr = cursor_at(0)
    g = ops.new_graph()
    with torch.cuda.graph(g):
        ops.counter_add(ctr, 1)
        with pytest.raises(L.MsgmError, match="capture"):
            smp.epoch
        with pytest.raises(L.MsgmError, match="capture"):
            smp.position = 3
    assert smp.epoch == 0 and smp.position == 64
