"""The GroupNorm reduce arithmetic on the CPU (gn_moments_ref): the analysis of record of raw against shifted fp32 moments,
the fairness of the input cases of tests/test_groupnorm_cond_gpu.py, and the prediction that the form the kernel uses
(gn_moments_ref.KERNEL_FORM) meets that file's criterion on every one of its cases.  An emulation, not a GPU measurement."""
import numpy as np
import pytest
import torch

import gn_moments_ref as M
import layer_ref as R
from test_layer_census_gpu import BOUNDS

FWD = BOUNDS["gn_fwd"][2]
DEGENERATE = [(C, G, P, c) for (C, G, P) in ((6, 6, 49), (6, 3, 64), (96, 32, 81), (192, 32, 16)) for c in (0.0, 10.0, -300.0)]


def test_shapes_reach_the_launch_geometries():
    geo = {}
    for C, G, P, B, _ in M.SHAPES:
        chunk, sub, nch = M.gn_chunks(B, P)
        V, CV, PL = M.gn_lane(C, C % 4 == 0)
        geo[(C, G, P, B)] = (V, C // G, 256 - CV * PL, PL, sub, chunk // sub, nch)
        assert nch <= 32 and C <= 256 and G <= 64
    #                          V  cpg dead PL  sub  m  nch
    assert geo[(6, 6, 49, 3)] == (1, 1, 4, 42, 49, 1, 1)
    assert geo[(6, 3, 64, 3)] == (1, 2, 4, 42, 64, 1, 1)
    assert geo[(130, 26, 36, 3)] == (1, 5, 126, 1, 36, 1, 1)
    assert geo[(96, 32, 81, 3)] == (4, 3, 16, 10, 64, 1, 2)
    assert geo[(192, 32, 16, 3)] == (4, 6, 16, 5, 16, 1, 1)
    assert geo[(256, 32, 25, 3)] == (4, 8, 0, 4, 25, 1, 1)
    assert geo[(32, 32, 2050, 20)] == (4, 1, 0, 32, 65, 1, 32)
    assert geo[(32, 32, 2050, 32)] == (4, 1, 0, 32, 65, 2, 16)
    assert geo[(64, 32, 4096, 1)] == (4, 2, 0, 16, 128, 1, 32)


def _worst(y, ref):
    return float((torch.as_tensor(y).double() - ref).abs().max())


# (C, G, P, mean, std): the table of the analysis — worst element of the normalised output (gamma = 1, beta = 0) against
# float64: PyTorch fp32, raw moments, shifted moments.  Recorded with these seeds: 3.2e-7 / 1.5e-7 / 1.5e-7,
# 2.0e-6 / 3.4e-6 / 6.6e-7, 1.4e-5 / 2.6e-4 / 3.9e-6, 1.2e-5 / 2.0e-4 / 4.7e-6, 1.6e-4 / 6.0e-2 / 3.8e-5, 1.6e-3 / 1.0e+2 / 3.0e-4.
TABLE = [(64, 32, 256, 0.0, 1.0), (64, 32, 256, 10.0, 1.0), (64, 32, 256, 100.0, 1.0), (6, 6, 49, 10.0, 0.1),
         (96, 32, 81, 100.0, 0.1), (64, 32, 256, 1000.0, 0.1)]


@pytest.mark.parametrize("C,G,P,mean,std", TABLE)
def test_raw_moments_lose_to_fp32_pytorch_from_ratio_100(C, G, P, mean, std):
    x, xd, _, _ = M.make_inputs(C, G, P, 3, mean, std, seed=1)
    one, zero = torch.ones(C), torch.zeros(C)
    ref = R.groupnorm(x.double(), one.double(), zero.double(), G)
    e_t = _worst(M.torch_fp32_forward(x, xd, one, zero, G, False)[0], ref)
    e = {f: _worst(M.forward(x.numpy(), xd.numpy(), one.numpy(), zero.numpy(), G, form=f)[0], ref) for f in ("raw", "shifted")}
    print(f"C{C} G{G} P{P} mean {mean:g} std {std:g}: torch fp32 {e_t:.1e}  raw {e['raw']:.1e}  shifted {e['shifted']:.1e}")
    assert e["shifted"] <= 3 * e_t
    if mean / std >= 100:
        assert e["raw"] > 3 * e_t
    else:
        assert e["raw"] <= 3 * e_t
    if mean / std >= 1000:
        assert e["raw"] > 300 * e_t                  # the raw error grows like (mean / std)^2, PyTorch's like mean / std


def _judge(tag, x, xd, gamma, beta, G, Bp, form):
    """The forward outputs of the emulation under the GPU file's criterion (no activation: the reduce is what is restated)."""
    n = min(x.shape[0], 3)
    x, xd = x[:n].contiguous(), xd[:n].contiguous()
    rp, rt = R.gn_dual_forward(x.double(), xd.double(), gamma.double(), beta.double(), G, False)
    tp, tt = M.torch_fp32_forward(x, xd, gamma, beta, G, False)
    for t in (rp, rt, tp, tt):
        assert bool(torch.isfinite(t).all())
    assert M.fair(x, G)
    yp, yt, st = M.forward(x.numpy(), xd.numpy(), gamma.numpy(), beta.numpy(), G, Bp=Bp, form=form)
    g = M.Groups(tag)
    g.tensor("primal", torch.from_numpy(yp), rp, tp, G, FWD)
    g.tensor("tangent", torch.from_numpy(yt), rt, tt, G, FWD)
    g.stats(torch.from_numpy(st), x.double(), xd.double(), G, FWD, pivot=form == "shifted")
    return g


@pytest.mark.parametrize("shape", M.SHAPES, ids=lambda s: "-".join(str(int(v)) for v in s))
def test_kernel_form_meets_the_criterion_on_the_sweep(shape):
    C, G, P, B, _ = shape
    for mean, std in M.CONDS:
        x, xd, gamma, beta = M.make_inputs(C, G, P, B, mean, std, seed=C + P)
        _judge(f"C{C} G{G} P{P} B{B} mean {mean:g} std {std:g}", x, xd, gamma, beta, G, B, M.KERNEL_FORM).finish()


@pytest.mark.parametrize("C,G,P,c", DEGENERATE)
def test_kernel_form_meets_the_criterion_on_the_degenerate_groups(C, G, P, c):
    x, xd, gamma, beta = M.make_degenerate(C, G, P, 3, c, seed=C + P)
    _judge(f"C{C} G{G} P{P} constant group c {c:g}", x, xd, gamma, beta, G, 3, M.KERNEL_FORM).finish()
    # the shifted form sees a constant group as exactly constant: var = 0, inv = eps^-1/2, xhat = 0
    mom = M.reduce_moments(x[1].numpy(), xd[1].numpy(), G, 3, "shifted")
    st = M.gn_stats(mom, float(P * C // G), x[1, 0, ::C // G].numpy())
    assert mom[0, 0] == c * P * (C // G) and st[0, 0] == 0 and st[0, 1] == np.float32(1.0 / np.sqrt(np.float64(np.float32(M.EPS))))


def test_raw_moments_fail_the_criterion_where_the_analysis_says():
    """What the criterion is there to catch: raw fp32 moments are outside it at |mean| / std >= 100 and on a constant group
    with c^2 2^-24 of the size of eps."""
    for C, G, P, B, mean, std in ((96, 32, 81, 3, 100.0, 1.0), (6, 6, 49, 3, 100.0, 0.1), (256, 32, 25, 3, 1000.0, 0.1)):
        x, xd, gamma, beta = M.make_inputs(C, G, P, B, mean, std, seed=C + P)
        assert _judge("raw", x, xd, gamma, beta, G, B, "raw").bad
    for c in (10.0, -300.0):
        x, xd, gamma, beta = M.make_degenerate(96, 32, 81, 3, c, seed=177)
        assert _judge("raw", x, xd, gamma, beta, G=32, Bp=3, form="raw").bad
    x, xd, gamma, beta = M.make_inputs(96, 32, 81, 3, 0.0, 1.0, seed=177)
    assert not _judge("raw", x, xd, gamma, beta, 32, 3, "raw").bad
