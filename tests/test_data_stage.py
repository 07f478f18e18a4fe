"""CPU-side checks of the data stage: the sampler protocol of the reference's data.py on the five device
samplers, the new C-ABI names, the loud refusal of CPU tensors and devices, and the gather's index rule restated in numpy
(tests/data_stage_ref.py) — in range, and uniform to within 5 sigma per bin."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import data_stage_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABI = ("msgm_data_gather", "msgm_ssm_prep_gather", "msgm_data_synth")


def _params(fn):
    return [(p.name, p.kind, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]


def test_constructor_signatures_follow_the_reference():
    from sdeflow_light_amd import data as D
    POS, KW, E = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY, inspect.Parameter.empty
    tail = [("device", KW, None), ("seed", KW, 0)]
    assert _params(D.SwissRoll.__init__) == tail                                                   # data.py:707
    lin = lambda cor: [("dim", POS, 2), ("correlation", POS, cor), ("normalized", POS, False)] + tail
    assert _params(D.Cauchy.__init__) == lin(False)                                                # data.py:723
    assert _params(D.Gaussian.__init__) == lin(True)                                               # data.py:755
    assert _params(D.GaussianCauchy.__init__) == lin(True)                                         # data.py:784
    assert _params(D.ArrayData.__init__) == [("train", POS, E), ("test", POS, None), ("name", POS, "array"),
                                             ("std", POS, None)] + tail
    assert _params(D.SwissRoll.sample) == [("n", POS, E), ("noise", POS, 0.5)]                     # data.py:710
    assert _params(D.SwissRoll.sampletest) == [("n", POS, E), ("noise", POS, 0.5)]
    for cls in (D.SwissRoll, D.Cauchy, D.Gaussian, D.GaussianCauchy, D.ArrayData):
        for m in ("sample", "sampletest", "sample_into"):
            assert callable(getattr(cls, m))
    # the three fixed-seed generators of the benchmark stay
    assert D.gaussian_mixture_2d(8).shape == (8, 2) and D.signals_1d(2, L=16).shape == (2, 16) and D.random_images(2, 1, 2, 2).shape == (2, 4)


def test_names_dims_and_std_are_the_references():
    """The values data.py:707-793 gives, written out: names by (dim, correlation, normalized); std = sqrt(diag(A A^T)) of
    the A first drawn (ones for the identity); ``normalized`` leaves std and makes A's rows unit vectors."""
    from sdeflow_light_amd import data as D
    s = D.SwissRoll()
    assert (s.name, s.dim) == ("swiss", 2)
    for cls, base, cor0 in ((D.Cauchy, "cauchy", False), (D.Gaussian, "gaussian", True), (D.GaussianCauchy, "gaussianCauchy", True)):
        assert cls().name == base + "2" + ("cor" if cor0 else "")
        for dim, cor, nrm, name in ((2, False, False, "2"), (3, True, False, "3cor"), (5, False, True, "5_norm"),
                                    (4, True, True, "4cor_norm")):
            torch.manual_seed(3)
            smp = cls(dim, cor, nrm)
            torch.manual_seed(3)
            A0 = torch.randn(dim, dim) if cor else torch.eye(dim)                  # upstream draws A from the global generator
            std = torch.sqrt(torch.diag(A0 @ A0.T))
            assert (smp.name, smp.dim) == (base + name, dim)
            assert torch.equal(smp.get_std(), std) and smp.get_std() is smp.std
            assert torch.equal(smp.A, torch.diag(1 / std) @ A0 if nrm else A0)
            if not cor:
                assert torch.equal(smp.get_std(), torch.ones(dim)) and torch.equal(smp.A, torch.eye(dim))
            if nrm:
                assert torch.allclose(torch.diag(smp.A @ smp.A.T), torch.ones(dim), atol=1e-6)
    g = D.GaussianCauchy(3)
    assert g.gaussian.std is g.get_std()                                            # data.py:795-796
    tab = np.arange(24, dtype=np.float64).reshape(6, 4) ** 2
    a = D.ArrayData(tab, tab[:2], name="era", device="cpu")
    assert (a.name, a.dim, a.max_nsamples, a.max_nsamplestest) == ("era", 4, 6, 2) and D.ArrayData(tab, device="cpu").name == "array"
    assert a.get_std().dtype == torch.float32 and np.allclose(a.get_std().numpy(), tab.std(axis=0).astype(np.float32))   # data.py:676,700
    assert torch.equal(D.ArrayData(tab, std=[1, 2, 3, 4], device="cpu").get_std(), torch.tensor([1.0, 2.0, 3.0, 4.0]))
    with pytest.raises(Exception):
        D.ArrayData(tab, tab[:, :3], device="cpu")


def test_abi_names_are_exported_and_signed():
    import __graft_entry__ as g
    g.build()
    from sdeflow_light_amd import _lib
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "msgm_hip.h")).read()
    for n in ABI:
        assert hasattr(lib, n) and n in _lib.SIGNATURES and re.search(rf"\bint {n}\(", hdr), n
    assert (_lib.RNG_STREAM_DATA, _lib.RNG_STREAM_DATA_ELEM, _lib.RNG_STREAM_DATA_CALL) == (5, 6, 7)
    assert (_lib.RNG_STREAM_T, _lib.RNG_STREAM_EPS, _lib.RNG_STREAM_V, _lib.RNG_STREAM_DW, _lib.RNG_STREAM_ROWS,
            _lib.RNG_STREAM_USER, _lib.RNG_STREAM_DROPOUT) == (0, 1, 2, 3, 4, 16, 64)
    assert (R.RNG_STREAM_DATA, R.RNG_STREAM_DATA_ELEM, R.RNG_STREAM_DATA_CALL) == (5, 6, 7)
    # argument checks that need no GPU: null pointers, sizes, the dense-A limit
    assert lib.msgm_data_gather(None, 4, None, 1, 1, None, None, None, None) == -1
    assert lib.msgm_ssm_prep_gather(None, 4, None, None, None, None, 1, 1, None, None, None, None) == -1
    assert lib.msgm_data_synth(9, 16, 1, 2, None, 0.5, 16, 16, None, None) == -1               # unknown kind
    assert lib.msgm_data_synth(_lib.DATA_GAUSSIAN, 16, 1, 2, None, 0.5, None, None, None, None) == -1   # Philox without a state
    assert lib.msgm_data_synth(_lib.DATA_GAUSSIAN, 16, 4, 129, 16, 0.5, None, 16, None, None) == _lib.MSGM_E_UNSUPPORTED


def test_cpu_tensors_and_devices_are_refused():
    from sdeflow_light_amd import data as D, ops, _lib
    E = _lib.MsgmError
    x, tab = torch.zeros(4, 2), torch.zeros(8, 2)
    with pytest.raises(E, match="no CPU fallback"):
        ops.data_gather(tab, x, idx=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(E, match="no CPU fallback"):
        ops.data_synth("gaussian", x, z=torch.zeros(4, 2))
    with pytest.raises(E, match="no CPU fallback"):
        ops.ssm_prep_gather(tab, x, x.clone(), torch.zeros(4), x.clone(), _lib.sde_struct(_lib.SDE_SGM, 0.1, 20.0, 1.0, 1e-3), None)
    with pytest.raises(E):
        ops.data_synth("bogus", x)
    for smp in (D.SwissRoll(device="cpu"), D.Cauchy(device="cpu"), D.Gaussian(3, device="cpu"), D.GaussianCauchy(device="cpu"),
                D.ArrayData(tab, tab, device="cpu")):
        with pytest.raises(E, match="no CPU fallback"):
            smp.sample(4)
        with pytest.raises(E, match="no CPU fallback"):
            smp.sampletest(4)
        with pytest.raises(E, match="no CPU fallback"):
            smp.sample_into(torch.zeros(4, smp.dim), None)


def test_trainers_take_data_keyword_only():
    from sdeflow_light_amd.train import MLPScoreTrainer, UNetScoreTrainer
    for cls in (MLPScoreTrainer, UNetScoreTrainer):
        p = inspect.signature(cls.__init__).parameters["data"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None


@pytest.mark.parametrize("N,B", [(64, 65536), (1000, 65536), (3, 4096), (1, 64)])
def test_index_rule_is_in_range_and_uniform(N, B):
    """Seed 11, offset 0, stream 5.  Every bin count within 5 sigma of B / N, sigma^2 = B (1/N)(1 - 1/N) (N = 1: exactly B)."""
    idx = R.gather_index(11, 0, 0, B, N)
    assert idx.shape == (B,) and idx.min() >= 0 and idx.max() < N
    w = R.PH.words(11, 0, R.RNG_STREAM_DATA, np.arange(B, dtype=np.uint64))
    assert np.array_equal(idx, (w.astype(object) * N) // (1 << 32))                         # the rule in exact integers
    cnt = np.bincount(idx, minlength=N)
    sigma = (B * (1.0 / N) * (1.0 - 1.0 / N)) ** 0.5
    worst = float(np.abs(cnt - B / N).max()) / sigma if sigma else float(np.abs(cnt - B).max())
    print(f"N = {N}, B = {B}: worst bin at {worst:.2f} sigma")
    assert np.all(np.abs(cnt - B / N) <= 5.0 * sigma)
    # a shard's rows are the global run's rows
    assert np.array_equal(R.gather_index(11, 0, 16, 8, N), R.gather_index(11, 0, 0, 24, N)[16:])
