"""CPU checks of the multiplicative SDE's latent kernel density: the float64 restatement (tests/kde_ref.py) against the
values recorded from the reference with sklearn (tests/golden/g21_kde.npz), and the parts of ``MSGMsde`` that need no GPU.

Bounds (profiles/kde/parity_measured.txt): 10 x the largest difference measured on the CPU between kde_ref and the
fixture.  ``lp64`` is sklearn's own float64 output: both sides are float64 sums of 257 terms.  ``lp`` and
``cst_log_dens`` went through upstream's cast to float32 (and an fp32 sum for the constant), so their differences sit at
fp32 rounding.  These three are evaluated on the fixture's own ``r_T`` and ``bandwidth``.  Recomputing those two from
``y0`` gave the fixture's bits on the machine that wrote it, but fp32 ``log`` / ``norm`` are not correctly rounded and
differ in the last bit between hosts, so they are held to ``kde_ref.radii_allowance`` instead of equality."""
import math

import pytest
import torch

import kde_ref as R
from conftest import load_golden

CASES = [("a", None, True), ("b", "log", False)]
TOL_LP64 = 5e-14        # measured 4.6e-15
TOL_LP = 7e-7           # measured 6.6e-8
TOL_CST = 6e-7          # measured 5.7e-8 (absolute; the constant is -4.2e-3)


def metric(out, ref):
    ref = ref.double()
    return float(((out.double() - ref).abs() / (1 + ref.abs())).max())


@pytest.fixture(scope="module")
def g():
    return load_golden("g21_kde")


@pytest.mark.parametrize("tag,norm_map,estim", CASES)
def test_kde_ref_reproduces_fixture(g, tag, norm_map, estim):
    r, h = g[tag + "_r_T"], float(g[tag + "_bandwidth"])
    assert R.bandwidth(r) == h                                  # the same double product from the same fp32 radii
    dr, dh = R.radii_allowance(r)
    r_here = R.map_radii(g[tag + "_y0"], norm_map)
    assert float((r_here - r).abs().max()) <= dr and abs(R.bandwidth(r_here) - h) <= dh
    q = torch.linalg.norm(g[tag + "_yT"], dim=1)
    e64 = metric(R.kde_logpdf(q, r, h), g[tag + "_lp64"])
    cst = R.cst_log_dens(r, h) if estim else torch.zeros((), dtype=torch.float64)
    ecst = abs(float(cst) - float(g[tag + "_cst_log_dens"]))
    elp = metric(R.log_latent_pdf(g[tag + "_yT"], r, h, cst), g[tag + "_lp"])
    print(f"g21 {tag}: lp64 {e64:.2e} (tol {TOL_LP64:.0e}), cst_log_dens {ecst:.2e} (tol {TOL_CST:.0e}), "
          f"lp {elp:.2e} (tol {TOL_LP:.0e})")
    assert e64 <= TOL_LP64
    assert ecst <= TOL_CST
    assert elp <= TOL_LP
    assert estim or float(g[tag + "_cst_log_dens"]) == 0.0


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_far_queries_are_finite(g, tag):
    lp = g[tag + "_lp"]
    assert torch.isfinite(lp).all()
    assert float(lp[40:52].max()) < -1e3          # the rows scaled by 10 lie hundreds of bandwidths outside the samples
    h = float(g[tag + "_bandwidth"])
    q = torch.linalg.norm(g[tag + "_yT"], dim=1)
    assert float(((q[40:52, None] - g[tag + "_r_T"][None, :]).abs().min(1).values / h).min()) > 40
    assert torch.isfinite(R.kde_logpdf(q, g[tag + "_r_T"], h)).all()


def test_kde_ref_far_query_closed_form():
    """One sample: the log-density is the Gaussian's, at any distance."""
    r, h = torch.tensor([0.25]), 0.01
    q = torch.tensor([0.25, 0.25 + 1e3 * h, 0.25 + 1e5 * h])
    want = -0.5 * ((q.double() - 0.25) / h) ** 2 - math.log(h) - 0.5 * math.log(2 * math.pi)
    assert torch.allclose(R.kde_logpdf(q, r, h), want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("norm_map", [None, "log"])
def test_kde_sampler_formula(norm_map):
    torch.manual_seed(3)
    r_T = R.map_radii(torch.randn(33, 3) * 0.2, norm_map)
    h = R.bandwidth(r_T)
    n = 4000
    u, z = torch.rand(n), torch.randn(n) * 30       # wide z: plenty of draws below zero
    out = R.kde_radial_sample(r_T, h, u, z, norm_map)
    assert out.shape == (n, 1)
    raw = r_T.double()[torch.floor(u.double() * 33).long()] + h * z.double()
    assert (raw < 0).sum() > 100
    if norm_map is None:
        assert float(out.min()) == 0.0 and torch.equal(out[:, 0], raw.clamp_min(0))
    else:
        assert torch.equal(out[:, 0], torch.exp(raw) - 1e-6) and float(out.min()) > -1e-6
    # u = 0 picks the first sample, u -> 1 the last one
    ends = R.kde_radial_sample(r_T, h, torch.tensor([0.0, 1.0 - 2 ** -24]), torch.zeros(2), None)
    assert torch.equal(ends[:, 0], r_T.double()[[0, 32]].clamp_min(0))


# ---- MSGMsde: what needs no GPU -------------------------------------------------------------------------------------
def _sde(y0, **kw):
    from sdeflow_light_amd.SDEs import MSGMsde
    T = torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)
    return MSGMsde(y0, T=T, num_steps_forward=4, device="cpu", denseTensor=False, **kw)


def test_msgm_bandwidth_and_names(g):
    sde = _sde(g["b_y0"], norm_map="log", estim_cst_norm_dens_r_T=False)
    assert abs(sde.bandwidth - float(g["b_bandwidth"])) <= R.radii_allowance(g["b_r_T"])[1] and sde.cst_log_dens == 0
    assert sde.name_SDE == "MSGM_sparseTenslogNorm"
    assert _sde(g["b_y0"], norm_map="log", norm_sampler="kde").name_SDE == "MSGM_sparseTenskdegaussianlogNorm"


def test_msgm_refuses_lazily():
    from sdeflow_light_amd.SDEs import MsgmError
    y = torch.randn(5, 3)
    for sde in (_sde(torch.randn(1, 3)), _sde(torch.ones(7, 3)), _sde(torch.randn(9, 3), kernel="tophat")):
        with pytest.raises(MsgmError):
            sde.log_latent_pdf(y)
        with pytest.raises(MsgmError):
            sde.cst_log_dens
    for sde in (_sde(torch.randn(1, 3), norm_sampler="kde"), _sde(torch.randn(9, 3), norm_sampler="kde", kernel="tophat")):
        with pytest.raises(MsgmError):
            sde.gen_radial_distribution(4, u=torch.rand(4), z=torch.randn(4))
    with pytest.raises(MsgmError):
        _sde(torch.randn(9, 3), norm_sampler="quantile")
