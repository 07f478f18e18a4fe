"""CPU-side checks of the epoch mode of the data stage: the index rule restated in numpy
(tests/data_epoch_ref.py) against the values the rule was pinned with, as a bijection, as a stream of permutations and
for uniformity over epochs; the new C-ABI names and the argument checks that need no GPU."""
import os
import re

import numpy as np
import pytest
import torch

import data_epoch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = ("msgm_data_gather_epoch", "msgm_counter_add")


def test_pinned_values():
    assert R.stream_index(11, np.arange(20), 10).tolist() == [5, 9, 0, 8, 4, 1, 7, 2, 3, 6, 4, 7, 8, 5, 6, 0, 2, 3, 9, 1]
    assert R.stream_index(11, np.arange(8), 1000).tolist() == [215, 37, 125, 280, 992, 170, 399, 65]
    assert R.stream_index(11, np.arange(65530, 65544), 65537).tolist() == [
        1325, 37742, 25468, 60618, 45602, 13297, 49680, 55853, 5286, 55224, 40597, 4812, 9968, 32932]
    assert [int(k) for k in R.epoch_keys(11, 0)[:4]] == [0x1ce46aa7, 0x8bfe7e92, 0x952835f8, 0xac7fc5b0]
    assert R.RNG_STREAM_DATA_PERM == 8 and R.widths(1) == (4, 4) and R.widths(257) == (4, 5) and R.widths(65537) == (8, 9)
    # the keys are the Philox blocks 4 e + j of stream 8 at offset 0
    assert np.array_equal(R.epoch_keys(11, 3), R.PH.msgm_philox(11, 0, 8, np.array([12, 13, 14], dtype=np.uint64)).reshape(-1))


EPOCHS = (0, 1, 7, 2 ** 33 + 5)


@pytest.mark.parametrize("seed", [0, 11])
def test_rule_is_a_bijection(seed):
    for N in list(range(1, 301)) + [1000, 4097, 65537]:
        p = np.arange(N)
        for e in EPOCHS:
            idx = R.perm_index(seed, e, p, N)
            assert idx.min() >= 0 and idx.max() < N and np.array_equal(np.sort(idx), p), (N, e)


def test_cycle_walk_stays_short():
    """2^bits < 2 N for N > 128: the mean number of passes stays near 2 at the worst table size N = 2^k + 1."""
    walks = []
    R.perm_index(11, 0, np.arange(65537), 65537, walks)
    print(f"N = 65537: mean passes {walks[0].mean():.2f}, worst {walks[0].max()}")
    assert walks[0].mean() < 2.1 and walks[0].max() < 64


def test_stream_windows_are_permutations_and_epochs_differ():
    N = 100
    s = R.stream_index(11, np.arange(6 * N), N).reshape(6, N)
    for e in range(6):
        assert np.array_equal(np.sort(s[e]), np.arange(N)), e
        assert np.array_equal(s[e], R.perm_index(11, e, np.arange(N), N))
    for e in range(5):
        assert not np.array_equal(s[e], s[e + 1])
    # a batch that straddles a boundary reads the tail of one epoch and the head of the next; a shard is its slice
    assert np.array_equal(R.batch_index(11, 90, 0, 24, N), np.concatenate([s[0, 90:], s[1, :14]]))
    assert np.array_equal(R.batch_index(11, 90, 8, 8, N), R.batch_index(11, 90, 0, 24, N)[8:16])
    assert not np.array_equal(R.stream_index(12, np.arange(N), N), s[0])                 # another seed, another order


@pytest.mark.parametrize("N,E", [(3, 4096), (17, 8192), (64, 4096)])
def test_rule_is_uniform_over_epochs(N, E):
    """Seed 5.  cnt[p, r] = the epochs in which position p reads row r; every cell within 5 sigma of E / N,
    sigma^2 = (E / N)(1 - 1 / N)."""
    rows = R.perm_table(5, np.arange(E), N)
    for e in (0, 1, E - 1):                                         # the vectorised form is the pinned one
        assert np.array_equal(rows[e], R.perm_index(5, e, np.arange(N), N))
    cnt = np.zeros((N, N), dtype=np.int64)
    np.add.at(cnt, (np.tile(np.arange(N), E), rows.reshape(-1)), 1)
    assert np.all(cnt.sum(0) == E) and np.all(cnt.sum(1) == E)
    sigma = ((E / N) * (1.0 - 1.0 / N)) ** 0.5
    worst = float(np.abs(cnt - E / N).max()) / sigma
    print(f"N = {N}, E = {E}: worst cell at {worst:.2f} sigma")
    assert worst <= 5.0


def test_abi_names_are_exported_and_signed():
    import __graft_entry__ as g
    g.build()
    from sdeflow_light_amd import _lib
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "msgm_hip.h")).read()
    for n in ABI:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and re.search(rf"\bint {n}\(", hdr), n
    assert _lib.RNG_STREAM_DATA_PERM == 8 == R.RNG_STREAM_DATA_PERM
    common = open(os.path.join(ROOT, "sdeflow_light_amd", "csrc", "common.h")).read()
    assert re.search(r"\bRNG_STREAM_DATA_PERM = 8\b", common)
    # argument checks that need no GPU: null pointers, sizes, the row limit
    assert lib.msgm_data_gather_epoch(None, 4, None, 1, 1, None, None, None, None) == -1
    assert lib.msgm_data_gather_epoch(16, 4, 16, 1, 1, None, 16, None, None) == -1              # no cursor
    assert lib.msgm_data_gather_epoch(16, 4, 16, 1, 1, None, None, 16, None) == -1              # no Philox state
    assert lib.msgm_data_gather_epoch(16, 4, 16, 0, 1, None, 16, 16, None) == -1
    assert lib.msgm_data_gather_epoch(16, 0, 16, 1, 1, None, 16, 16, None) == -1
    assert lib.msgm_data_gather_epoch(16, 2 ** 31, 16, 1, 1, None, 16, 16, None) == _lib.MSGM_E_UNSUPPORTED
    assert lib.msgm_counter_add(None, 1, None) == -1


def test_cpu_tensors_and_devices_are_refused():
    from sdeflow_light_amd import data as D, ops, _lib
    E = _lib.MsgmError
    x, tab = torch.zeros(4, 2), torch.zeros(8, 2)
    with pytest.raises(E, match="no CPU fallback"):
        ops.data_gather_epoch(tab, x, None, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(E):
        ops.counter_add(torch.zeros(1, dtype=torch.int32), 1)
    smp = D.ArrayData(tab, tab, device="cpu", replace=False)
    assert smp.replace is False and smp.stride == 1 and D.ArrayData(tab, device="cpu").replace is True
    for call in (lambda: smp.sample(4), lambda: smp.sampletest(4), lambda: smp.sample_into(torch.zeros(4, 2), None),
                 lambda: smp.position, lambda: smp.epoch):
        with pytest.raises(E, match="no CPU fallback"):
            call()


def test_stride_binding_and_steps_per_epoch():
    from sdeflow_light_amd import data as D, _lib
    tab = torch.zeros(10, 2)
    smp = D.ArrayData(tab, device="cpu", replace=False)
    assert smp.steps_per_epoch(4) == 2.5 and isinstance(smp.steps_per_epoch(5), float)
    smp.bind(2)
    smp.bind(2)                                                     # the same world again: fine
    assert smp.stride == 2
    with pytest.raises(_lib.MsgmError, match="world"):
        smp.bind(4)
    with pytest.raises(_lib.MsgmError, match="replace=False"):      # a with-replacement sampler has no cursor
        D.ArrayData(tab, device="cpu").bind(2)
    with pytest.raises(_lib.MsgmError, match="replace=False"):
        D.ArrayData(tab, device="cpu").position
