"""Float64 restatement of the multiplicative SDE's 1-D Gaussian kernel density (SDEs.py:239-265, 438-451, 503-509):
what sklearn's ``KernelDensity(kernel='gaussian', bandwidth=h)`` computes with its default exact sum, written in torch.
The comparator of tests/test_kde_ref.py (against the values recorded from the reference) and tests/test_kde_gpu.py
(against the HIP kernel)."""
import math

import torch


def bandwidth(r_T):
    """0.1 * unbiased std of the mapped radii, taken in the radii's own precision as upstream does (SDEs.py:239)."""
    return 0.1 * torch.std(r_T).item()


def map_radii(y0, norm_map=None):
    """r_T of SDEs.py:233-236."""
    r = torch.linalg.norm(y0, dim=1)
    return torch.log(r + 1e-6) if norm_map == "log" else r


def radii_allowance(r_T):
    """How far two fp32 evaluations of ``map_radii`` / ``bandwidth`` may lie apart: the norm and the log are each within
    an ulp or two of the true value, but not correctly rounded, so their bits depend on the host's vector math library.
    Radii: 4 ulp of the largest |r_T|.  Bandwidth: the std moves by at most sqrt(n / (n - 1)) times the largest change
    of an element; returned as (radius allowance, bandwidth allowance)."""
    n = r_T.numel()
    dr = 4 * 2.0 ** -23 * float(r_T.abs().max())
    return dr, 0.1 * math.sqrt(n / (n - 1.0)) * dr


def kde_logpdf(q, r, h, dtype=torch.float64, chunk=1 << 22):
    """-log(Ns) - log(h) - log(2 pi)/2 + logsumexp_i(-((q_m - r_i)/h)^2 / 2), evaluated in ``dtype`` (float64: the truth;
    float32: the plain torch composition whose error sets the kernel's bound).  Queries go in blocks so that the
    (M, Ns) matrix stays small."""
    q, r = q.reshape(-1).to(dtype), r.reshape(-1).to(dtype)
    out = torch.empty_like(q)
    rows = max(1, chunk // r.numel())
    for a in range(0, q.numel(), rows):
        out[a:a + rows] = torch.logsumexp(-0.5 * ((q[a:a + rows, None] - r[None, :]) / h) ** 2, 1)
    return out - math.log(r.numel()) - math.log(h) - 0.5 * math.log(2 * math.pi)


def cst_log_dens(r_T, h):
    """log(sum(exp(logdens)) * dr) on the 1000-point grid between min and max of r_T (SDEs.py:258-265).  The grid and dr
    are fp32 as upstream builds them; the density is float64 and the sum too (upstream sums fp32 values)."""
    grid = torch.linspace(float(r_T.min()), float(r_T.max()), 1000, dtype=torch.float32)
    dens = torch.exp(kde_logpdf(grid, r_T, h))
    return torch.log(dens.sum() * (grid[1] - grid[0]).double())


def log_latent_pdf(yT, r_T, h, cst=0.0):
    """SDEs.py:503-509: density at the fp32 row norm of yT, minus cst_log_dens."""
    return kde_logpdf(torch.linalg.norm(yT, dim=1), r_T, h) - cst


def kde_radial_sample(r_T, h, u, z, norm_map=None):
    """The KDE latent-radius sampler (SDEs.py:444-451 with KernelDensity.sample for a Gaussian kernel):
    r = r_T[floor(u Ns)] + h z, negative radii set to 0 unless the radii are log-mapped, then exp(.) - 1e-6 for the log
    map.  Returned as (n, 1) like upstream."""
    Ns = r_T.numel()
    i = torch.floor(u.reshape(-1).double() * Ns).long().clamp(max=Ns - 1)
    r = r_T.reshape(-1).double()[i] + h * z.reshape(-1).double()
    if norm_map != "log":
        r = torch.where(r < 0, torch.zeros_like(r), r)
    if norm_map == "log":
        r = torch.exp(r) - 1e-6
    return r.reshape(-1, 1)
