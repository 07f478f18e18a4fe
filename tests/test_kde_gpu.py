"""GPU checks of the 1-D Gaussian KDE log-density kernel (csrc/metrics_kernels.hip: k_kde_partial / k_kde_merge) and of
what is built on it: ``MSGMsde.log_latent_pdf`` / ``cst_log_dens``, the MSGM ELBO and the KDE latent-radius sampler.

Kernel parity: metric max_m |out - ref| / (1 + |ref|) against the float64 restatement (tests/kde_ref.py) on the same fp32
inputs.  The bound is not fixed in advance: it is 4 x the error, on the same inputs, of the plain fp32 torch composition
(``torch.logsumexp`` over fp32 terms, evaluated on the CPU) against the same float64 restatement — the kernel sums in
another order and its hardware exp2 is about 1 ulp rather than correctly rounded.  Both figures are printed
(profiles/kde/parity_measured.txt).

Kernel geometry (metrics_kernels.hip): a block owns 256 queries and walks its slab of samples in chunks of 512; by
default every chunk is its own slab until the grid passes 2048 blocks; a caller's small workspace makes slabs of several
chunks."""
import math

import pytest
import torch

import kde_ref as R
from conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
Q_TILE, CHUNK = 256, 512

# (M, Ns): the issue's list; one below / at / one above the query tile and the sample chunk; more slabs than queries
SHAPES = [(1, 1), (3, 5), (64, 64), (65, 257), (256, 4097), (1000, 33),
          (Q_TILE - 1, 40), (Q_TILE, 40), (Q_TILE + 1, 40), (7, CHUNK - 1), (7, CHUNK), (7, CHUNK + 1), (3, 4 * CHUNK + 1)]
FAMILIES = ["normal", "equal", "far1e3", "far1e5", "duplicates"]


def metric(out, ref):
    ref = ref.double()
    return float(((out.double().cpu() - ref).abs() / (1 + ref.abs())).max())


def make_inputs(M, Ns, family, seed):
    gen = torch.Generator().manual_seed(seed)
    if family == "duplicates":
        r = torch.randint(0, 5, (Ns,), generator=gen).float() * 0.37 + 0.1
        if Ns > 1:
            r[0], r[-1] = 0.1, 0.1 + 4 * 0.37                  # at least two distinct values: a positive std
    else:
        r = (torch.randn(Ns, generator=gen) * 1.5).abs()
    h = 0.1 * float(r.std()) if Ns > 1 else 0.3
    pick = r[torch.randint(0, Ns, (M,), generator=gen)]
    if family in ("normal", "duplicates"):
        q = (torch.randn(M, generator=gen) * 1.5).abs()
    elif family == "equal":
        q = pick.clone()
    else:
        k = 1e3 if family == "far1e3" else 1e5
        q = torch.where(torch.arange(M) % 2 == 0, r.max() + k * h, r.min() - k * h).float()     # k bandwidths outside
    return q.contiguous(), r.contiguous(), h


def check_parity(q, r, h, out, what, sub=None):
    """out (GPU result for q, or for q[sub]) within 4 x the fp32 CPU composition's own error; prints both."""
    if sub is not None:
        q, out = q[sub], out[sub]
    ref = R.kde_logpdf(q, r, h)
    e_cpu32 = metric(R.kde_logpdf(q, r, h, torch.float32), ref)
    e_hip = metric(out, ref)
    print(f"kde parity {what}: kernel {e_hip:.3e} | fp32 torch composition {e_cpu32:.3e} | bound {4 * e_cpu32:.3e}")
    assert torch.isfinite(out).all()
    assert e_hip <= 4 * e_cpu32, (what, e_hip, e_cpu32)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("M,Ns", SHAPES)
def test_kde_logpdf_parity(M, Ns, family):
    from sdeflow_light_amd import ops
    q, r, h = make_inputs(M, Ns, family, seed=1000 * M + Ns)
    qd, rd = q.to(DEV), r.to(DEV)
    out = ops.kde_logpdf(qd, rd, h)
    assert out.shape == (M,) and out.dtype == torch.float32
    assert torch.equal(out, ops.kde_logpdf(qd, rd, h))            # bitwise repeatable
    check_parity(q, r, h, out, f"({M}, {Ns}) {family}")
    if family.startswith("far"):
        assert float(out.max()) < -0.4 * float(family[3:]) ** 2     # about -k^2 / 2


@pytest.mark.parametrize("family", ["normal", "far1e3"])
@pytest.mark.parametrize("slabs", [1, 2, 3])
def test_kde_logpdf_slabs_of_several_chunks(slabs, family):
    """A workspace for ``slabs`` slabs only: 5 chunks folded 5, 3 + 2 and 2 + 2 + 1 to a slab."""
    from sdeflow_light_amd import ops
    M, Ns = 65, 4 * CHUNK + 1
    q, r, h = make_inputs(M, Ns, family, seed=7)
    ws = torch.empty(2 * M * slabs, dtype=torch.float32, device=DEV)
    out = ops.kde_logpdf(q.to(DEV), r.to(DEV), h, workspace=ws)
    assert torch.equal(out, ops.kde_logpdf(q.to(DEV), r.to(DEV), h, workspace=ws))
    check_parity(q, r, h, out, f"({M}, {Ns}) {family}, workspace for {slabs} slab(s)")


def test_kde_logpdf_grid_past_2048_blocks():
    """3 query tiles x 700 chunks = 2100 blocks: the kernel's own choice becomes 2 chunks per slab.  The float64 comparator
    runs on every 13th query (and the last one) to stay quick."""
    from sdeflow_light_amd import ops
    M, Ns = 2 * Q_TILE + 1, 700 * CHUNK
    q, r, h = make_inputs(M, Ns, "normal", seed=11)
    out = ops.kde_logpdf(q.to(DEV), r.to(DEV), h)
    assert torch.isfinite(out).all()
    sub = torch.cat([torch.arange(0, M, 13), torch.tensor([M - 1])])
    check_parity(q, r, h, out, f"({M}, {Ns}) normal, {sub.numel()} queries compared", sub=sub)


def test_kde_logpdf_bad_arguments():
    from sdeflow_light_amd import ops, _lib as L
    q, r = torch.rand(4, device=DEV), torch.rand(9, device=DEV)
    for h in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(L.MsgmError):
            ops.kde_logpdf(q, r, h)
    for a, b in ((q[:0], r), (q, r[:0]), (q.reshape(2, 2), r), (q.cpu(), r.cpu()), (q.double(), r)):
        with pytest.raises(L.MsgmError):
            ops.kde_logpdf(a, b, 0.1)
    with pytest.raises(L.MsgmError):
        ops.kde_logpdf(q, r, 0.1, workspace=torch.empty(7, device=DEV))
    # the C entry itself
    out, ws = torch.empty(4, device=DEV), torch.empty(8, device=DEV)
    call = lambda M, Ns, h: L.lib().msgm_kde_logpdf(L.ptr(q), M, L.ptr(r), Ns, h, L.ptr(out), L.ptr(ws), 32, L.stream())
    assert call(4, 9, 0.1) == 0
    for bad in ((0, 9, 0.1), (4, 0, 0.1), (-1, 9, 0.1), (4, 9, 0.0), (4, 9, -0.1), (4, 9, float("nan")), (4, 9, float("inf"))):
        assert call(*bad) == -1, bad
    torch.cuda.synchronize()


# ---- MSGMsde ----------------------------------------------------------------------------------------------------------
def Tp():
    return torch.nn.Parameter(torch.FloatTensor([1.0]), requires_grad=False)


def make_sde(y0, dense=False, G=None, nsf=4, **kw):
    from sdeflow_light_amd.SDEs import MSGMsde
    return MSGMsde(y0, beta_min=0.1, beta_max=20.0, t_epsilon=1e-3, T=Tp(), num_steps_forward=nsf, device=DEV,
                   denseTensor=dense, G=G, **kw)


def make_gen(base, net, sd=None):
    from sdeflow_light_amd.SDEs import PluginReverseSDE
    gen = PluginReverseSDE(base, net.to(DEV), base.T, deviceReverseSDE=DEV).to(DEV)
    if sd is not None:
        missing = gen.load_state_dict(sd, strict=False)
        assert set(missing.missing_keys) <= {"T", "base_sde.T"} and not missing.unexpected_keys
    return gen


@pytest.fixture(scope="module")
def g():
    return load_golden("g21_kde")


@pytest.mark.parametrize("tag,norm_map,estim", [("a", None, True), ("b", "log", False)])
def test_msgm_log_latent_pdf_golden(g, tag, norm_map, estim):
    """log_latent_pdf (row norm + kernel - cst_log_dens) of an MSGMsde built from y0, against the reference's values.
    Comparator for the bound: the fp32 composition INCLUDING the fp32 roundings in front of the kernel — the row norm of
    yT and this host's fp32 radii / bandwidth from y0 (``kde_ref.radii_allowance``) — against the float64 restatement on
    the float64 row norm and the fixture's radii."""
    sde = make_sde(g[tag + "_y0"], norm_map=norm_map, estim_cst_norm_dens_r_T=estim)
    yT, r, h = g[tag + "_yT"], g[tag + "_r_T"], float(g[tag + "_bandwidth"])
    dr, dh = R.radii_allowance(r)
    assert float((sde.r_T.cpu() - r).abs().max()) <= dr and abs(sde.bandwidth - h) <= dh
    cst64 = R.cst_log_dens(r, h) if estim else 0.0
    ref = R.kde_logpdf(torch.linalg.norm(yT.double(), dim=1), r, h) - cst64
    cst32 = float(g[tag + "_cst_log_dens"])
    r_here = R.map_radii(g[tag + "_y0"], norm_map)
    e_cpu32 = metric(R.kde_logpdf(torch.linalg.norm(yT, dim=1), r_here, R.bandwidth(r_here), torch.float32) - cst32, ref)
    lp = sde.log_latent_pdf(yT.to(DEV))
    assert lp.shape == (yT.shape[0],) and lp.is_cuda and torch.isfinite(lp).all()
    e_hip = metric(lp, g[tag + "_lp"])
    print(f"log_latent_pdf g21 {tag}: vs the reference {e_hip:.3e} | fp32 torch composition vs float64 {e_cpu32:.3e} | "
          f"bound {4 * e_cpu32:.3e}")
    assert e_hip <= 4 * e_cpu32
    if estim:
        e_cst = abs(float(sde.cst_log_dens) - cst32)
        print(f"cst_log_dens g21 {tag}: {float(sde.cst_log_dens):.8f} vs {cst32:.8f}")
        assert sde.cst_log_dens.is_cuda and e_cst <= 4 * e_cpu32 * (1 + abs(cst32))
    else:
        assert sde.cst_log_dens == 0


def test_msgm_one_row_constructs_and_refuses():
    from sdeflow_light_amd.SDEs import MsgmError
    sde = make_sde(torch.randn(1, 4))
    with pytest.raises(MsgmError):
        sde.log_latent_pdf(torch.randn(3, 4, device=DEV))
    with pytest.raises(MsgmError):
        make_sde(torch.randn(8, 4), kernel="epanechnikov").log_latent_pdf(torch.randn(3, 4, device=DEV))


ELBO = [("sp", False, 6, "NormalizeLogRadius"), ("dn", True, 4, None)]


def elbo_gen(g, tag, dense, d, pre):
    from sdeflow_light_amd.NN import MLP
    base = make_sde(g[tag + "_y0"], dense=dense, G=g.get("dn_G") if dense else None, norm_map="log",
                    estim_cst_norm_dens_r_T=False)
    return make_gen(base, MLP(d, premodule=pre), g.sub(tag + "::"))


@pytest.mark.parametrize("tag,dense,d,pre", ELBO)
def test_msgm_elbo_golden(g, tag, dense, d, pre):
    """elbo_random_t_slice with (t, y), the probe draw and yT injected, against the reference.  Tolerance: the 2e-5 rel-L2
    that tests/test_host_gpu.py::test_ssm_msgm_mlp_golden applies to ``per``."""
    gen = elbo_gen(g, tag, dense, d, pre)
    elbo = gen.elbo_random_t_slice(g[tag + "_x"].to(DEV), y=g[tag + "_y"].to(DEV), t_given=g[tag + "_t"].to(DEV),
                                   u_v=g[tag + "_u_v"].to(DEV), yT=g[tag + "_yT"].to(DEV))
    assert elbo.shape == (48,)
    e, e_lp = rel_l2(elbo.cpu(), g[tag + "_elbo"]), rel_l2(gen.base_sde.log_latent_pdf(g[tag + "_yT"].to(DEV)).cpu(), g[tag + "_lp"])
    print(f"MSGM ELBO g21 {tag}: rel-L2 {e:.3e} (lp term alone {e_lp:.3e}), tolerance 2e-5")
    assert e <= 2e-5


@pytest.mark.parametrize("tag,dense,d,pre", ELBO)
def test_msgm_elbo_and_evaluate_run(g, tag, dense, d, pre):
    """Nothing injected: finite values for the dense and the sparse tensor; evaluate() as the driver calls it."""
    from sdeflow_light_amd.NN import evaluate
    torch.manual_seed(0)
    gen = elbo_gen(g, tag, dense, d, pre)
    x = g[tag + "_x"].to(DEV)
    elbo = gen.elbo_random_t_slice(x)
    assert elbo.shape == (48,) and torch.isfinite(elbo).all()
    mean, sem = evaluate(gen, x)
    assert mean.dim() == 0 and sem.dim() == 0 and math.isfinite(float(mean)) and math.isfinite(float(sem))
    assert gen.training


@pytest.mark.parametrize("norm_map", [None, "log"])
def test_msgm_kde_sampler(norm_map):
    torch.manual_seed(5)
    y0 = torch.randn(257, 4) * (0.05 if norm_map is None else 1.5)      # small radii: h z reaches below zero
    Ns, n = 257, 1001
    # u at least 0.1 / Ns away from a multiple of 1 / Ns (fp32 u Ns must not round across an index), plus the two ends
    u = (torch.randint(0, Ns, (n,)).float() + 0.1 + 0.8 * torch.rand(n)) / Ns
    u[0], u[1] = 0.0, 1.0 - 2 ** -24
    z = torch.randn(n) * (30 if norm_map is None else 1)
    sde = make_sde(y0, norm_map=norm_map, norm_sampler="kde")
    got = sde.gen_radial_distribution(n, u=u.to(DEV), z=z.to(DEV))
    ref = R.kde_radial_sample(sde.r_T.cpu(), sde.bandwidth, u, z, norm_map)
    assert got.shape == (n, 1) and got.dtype == torch.float32
    # fp32 rounding: h -> fp32, h z, the sum (3 roundings of terms no larger than |r_T[i]| + |h z|); the log map adds
    # exp(r) dr, the exponential's own ulps and the final subtraction
    mag = sde.r_T.cpu().double().abs().max() + sde.bandwidth * z.double().abs()
    tol = 4 * 2.0 ** -24 * mag
    if norm_map == "log":
        tol = (ref[:, 0] + 1e-6) * (tol + 4 * 2.0 ** -24)
    err = (got.cpu().double() - ref)[:, 0].abs()
    print(f"kde sampler ({norm_map}): worst error / fp32 rounding allowance {float((err / tol).max()):.2f}")
    assert (err <= tol).all()
    if norm_map is None:
        assert float(got.min()) == 0.0 and int((got == 0).sum()) > 50
    # un-injected: same seed -> same radii; one stream advance per call
    draws = []
    for _ in range(2):
        torch.manual_seed(77)
        s = make_sde(y0, norm_map=norm_map, norm_sampler="kde")
        a = s.gen_radial_distribution(300)
        off = s.rng.state_dict()["offset"]
        b = s.gen_radial_distribution(300)
        assert s.rng.state_dict()["offset"] == off + 1 and not torch.equal(a, b)
        draws.append(torch.cat([a, b]))
    assert torch.equal(draws[0], draws[1]) and torch.isfinite(draws[0]).all()
    lat = make_sde(y0, norm_map=norm_map, norm_sampler="kde").latent_sample(64, 4)
    assert lat.shape == (64, 4) and torch.isfinite(lat).all()
