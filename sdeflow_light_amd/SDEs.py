"""SDE definitions and the sliced-score-matching loss on HIP kernels — host
mirror of the reference's ``SDEs.py`` (same class / method names and argument
meaning: ``forward_SDE``, ``SDE``, ``SGMsde``, ``MSGMsde``, ``PluginReverseSDE``).

What runs where
---------------
* hot path (``ssm``, ``mu``, ``mu_Strato``, ``sample``, the integrators in
  ``sde_scheme``): hand-written gfx950 kernels through the C ABI;
* schedule accessors kept for API compatibility (``beta``, ``mean_weight``,
  ``var``, ``f``, ``g`` ...) are one-line tensor expressions evaluated on the
  tensor's own device — the hot path never calls them;
* reporting path: the latent log-densities and the ELBO slice estimate.  The
  multiplicative SDE's latent density is a 1-D Gaussian kernel density of the
  radii (a host-side sklearn ``KernelDensity`` upstream, SDEs.py:240): here one
  log-space kernel on the device (``ops.kde_logpdf``);
* out of scope: plotting / validation branches, non-Gaussian KDE kernels.
* ``ssm_intT=True`` (the time-integrated SSM loss, SDEs.py:648-706) is built: upstream's only defect there is the
  global name ``device`` in ``sample_t_linspace``, which exists in the driver module and not in ``SDEs.py``.

RNG: the reference draws from torch's global generator (CPU mt19937 for t,
device generator for the rest, SDEs.py:688,141,515).  Here every draw comes
from a device-resident Philox stream owned by the object (``.rng``); parity
tests inject explicit noise instead.
"""
from __future__ import annotations

import math

from typing import Optional

import torch
import torch.nn as nn

from . import _lib as L
from . import ops
from ._lib import MsgmError, PhiloxState


class forward_SDE(nn.Module):
    """Adaptor exposing the forward (noising) process to the integrators
    (SDEs.py:30-47): mu = f_strato + 1/2 divSigma, sigma = g."""

    def __init__(self, base_sde, T):
        super().__init__()
        self.base_sde = base_sde
        self.T = T

    def mu(self, s, y, lmbd=0.):
        return self.mu_Strato(s, y) + 0.5 * self.base_sde.div_Sigma(s, y)

    def mu_Strato(self, s, y, lmbd=0.):
        return self.base_sde.f_strato(s, y)

    def sigma(self, s, y, lmbd=0., sparse=False):
        return self.base_sde.g(s, y, sparse=sparse)


class SDE(nn.Module):
    """Base class (SDEs.py:49-76): linear beta schedule and bookkeeping."""
    kind = L.SDE_SGM

    def __init__(self, beta_min=0.1, beta_max=20.0, T=1.0, t_epsilon=0.001, num_steps_forward=100, device="cpu"):
        super().__init__()
        self.device = torch.device(device)
        self.T = T
        self.beta_min, self.beta_max = beta_min, beta_max
        self.t_epsilon = t_epsilon
        self.num_steps_forward = num_steps_forward
        self.norm_correction = False
        self.sparseTensor = False
        self.rng: Optional[PhiloxState] = None
        self._shard = None           # (first global row, n) of this rank's rows in a data-parallel run

    def to(self, device):
        new = super().to(device)
        new.device = torch.device(device)
        if torch.is_tensor(self.T):
            new.T = self.T.to(device)
        return new

    def T_float(self) -> float:
        return L.host_scalar(self.T)          # cached: no device synchronisation per call (graph-capturable)

    def struct(self) -> L.SdeT:
        """msgm_sde_t for the kernels."""
        return L.sde_struct(self.kind, self.beta_min, self.beta_max, self.T_float(), self.t_epsilon,
                            getattr(self, "G", None) if self.kind == L.SDE_MSGM_DENSE else None,
                            getattr(self, "L_G", None) if self.kind == L.SDE_MSGM_DENSE else None)

    def philox(self, device) -> PhiloxState:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.rng is None or self.rng.state.device != device:
            seed = int(torch.initial_seed()) ^ 0x5DE5
            if self._shard is None:
                # no shard placement given: at least give every rank of a distributed run its own stream
                import torch.distributed as dist
                if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                    seed = (seed + 0x9E3779B97F4A7C15 * dist.get_rank()) & 0x7FFFFFFFFFFFFFFF
            self.rng = PhiloxState(seed, device)
            if self._shard is not None:
                self.rng.set_shard(*self._shard)
        return self.rng

    def set_shard(self, row_base: int, n: int) -> None:
        """Place this rank's rows at [row_base, ...) of the GLOBAL batch / sample set: with the same seed on every
        rank the sharded run then draws (t, eps, v, dW, latent) exactly as the single-GPU run does for those rows
        (``parallel.shard_rows`` gives row_base).  Without it, ranks of a distributed run get decorrelated seeds."""
        self._shard = (int(row_base), int(n))
        if self.rng is not None:
            self.rng.set_shard(*self._shard)

    def beta(self, t):
        return self.beta_min + (self.beta_max - self.beta_min) * t

    def IJK(self):
        return None, None, None

    # -- forward-process samplers of the base class (SDEs.py:78-146), same names and arguments ----------------
    @torch.no_grad()
    def sample_scheme(self, t, y0, keep_all_samples=False, return_noise=False):
        """y_t | y_0 by RK4 on the forward process (SDEs.py:78-122) — one device-resident masked multi-stop
        integration instead of the per-row Python loop; ``keep_all_samples`` only chose the capture buffer upstream."""
        if return_noise:
            raise NotImplementedError('See the official repository.')
        from .sde_scheme import msgm_forward_perturb
        return msgm_forward_perturb(self, t, y0)

    @torch.no_grad()
    def sample_scheme_allt(self, y0, include_t0=True, keep_all_samples=True, samplesToKeep=None):
        """y_0, y_{t_1}, ..., y_T | y_0 (SDEs.py:124-132)."""
        from .sde_scheme import rk4_stratonovich_sampler
        return rk4_stratonovich_sampler(forward_SDE(self, self.T).to(self.device), y0, num_steps=self.num_steps_forward, lmbd=0,
                                        keep_all_samples=keep_all_samples, samplesToKeep=samplesToKeep, include_t0=include_t0)

    def sample_Song_et_al(self, t, y0, return_noise=False, eps=None):
        """Closed-form y_t | y_0 of the VP SDE (SDEs.py:134-146) in one kernel; with ``return_noise`` also
        (epsilon, std, g(t, y_t)) as upstream."""
        if self.kind != L.SDE_SGM:
            raise MsgmError("sample_Song_et_al is the closed form of the additive (VP) SDE")
        y, e = ops.perturb_vp_at(y0.contiguous().float(), self.struct(), t, eps=eps,
                                 rng=None if eps is not None else self.philox(y0.device), return_eps=True)
        if eps is None:
            self.rng.advance(1)
        if not return_noise:
            return y
        return y, e, self.var(t) ** 0.5, self.g(t, y)

    def sample_debiasing_t(self, shape):
        raise NotImplementedError('See the official repository.')


class SGMsde(SDE):
    """Variance-preserving SDE (SDEs.py:161-215)."""
    kind = L.SDE_SGM

    def __init__(self, beta_min=0.1, beta_max=20.0, T=1.0, t_epsilon=0.001, num_steps_forward=100, device='cpu'):
        super().__init__(beta_min, beta_max, T, t_epsilon, num_steps_forward, device)
        self.name_SDE = "SGM"

    # -- schedule accessors (API compatibility; not on the hot path) ---------
    def mean_weight(self, t):
        return torch.exp(-0.25 * t ** 2 * (self.beta_max - self.beta_min) - 0.5 * t * self.beta_min)

    def var(self, t):
        return 1. - torch.exp(-0.5 * t ** 2 * (self.beta_max - self.beta_min) - t * self.beta_min)

    def f(self, t, y):
        return -0.5 * self.beta(t) * y

    def f_strato(self, t, y):
        return -0.5 * self.beta(t) * y

    def div_Sigma(self, t, y):
        return torch.zeros_like(y)

    def g(self, t, y, sparse=False):
        return torch.ones_like(y) * self.beta(t) ** 0.5

    # -- hot path --------------------------------------------------------------
    @torch.no_grad()
    def sample(self, t, y0, return_noise=False, eps=None):
        """y_t | y_0 in closed form — ONE kernel (K1) instead of ~8 eager ops.
        ``t`` (B,1) is used exactly as given (no clamp, as upstream: SDEs.py:134-146);
        ``eps`` injects the Gaussian draw (parity tests)."""
        if return_noise:
            raise NotImplementedError('See the official repository.')
        y = ops.perturb_vp_at(y0.contiguous().float(), self.struct(), t, eps=eps,
                              rng=None if eps is not None else self.philox(y0.device))
        if eps is None:
            self.rng.advance(1)
        return y

    def latent_sample(self, num_samples, n):
        dev = self.device
        if dev.type != "cuda":
            raise MsgmError("latent_sample draws on the GPU (Philox); move the SDE to a cuda device")
        x = torch.empty(num_samples, n, dtype=torch.float32, device=dev)
        rng = self.philox(dev)
        ops.fill_normal(x, rng, L.RNG_STREAM_USER)
        rng.advance(1)
        return x

    def cond_latent_sample(self, t_, T, x, eps=None):
        return self.sample(torch.ones_like(t_) * T, x, eps=eps)

    @property
    def logvar_mean_T(self):
        """SDEs.py:171-175."""
        return torch.zeros(1), torch.zeros(1)

    def log_normal(self, x, mean, log_var, eps=0.00001):
        """SDEs.py:213-215."""
        return -(x - mean) ** 2 / (2. * torch.exp(log_var) + eps) - log_var / 2. - 0.5 * math.log(2 * math.pi)

    def log_latent_pdf(self, yT):
        """Standard-normal latent log-density per element (SDEs.py:209-211), on the device."""
        return self.log_normal(yT, torch.zeros_like(yT), torch.zeros_like(yT))


class MSGMsde(SDE):
    """Multiplicative SDE dY = G(Y) o dB (SDEs.py:221-509), dense rank-3
    tensor or sparse nearest-neighbour rotation tensor.

    The radial law of the latent is a 1-D Gaussian kernel density of the mapped
    radii ``r_T`` with bandwidth ``0.1 * std(r_T)`` (SDEs.py:239-240).  It serves
    ``log_latent_pdf`` (the ELBO's latent term), ``cst_log_dens`` and the
    ``norm_sampler="kde"`` latent sampler; ``norm_sampler="ecdf"`` (the default)
    samples radii by empirical quantiles instead.

    The density is needed lazily.  Upstream fits the sklearn estimator in every
    constructor call, so sklearn refuses a bandwidth that is not a positive
    number (one row, or all radii equal) at construction, and an unknown
    ``kernel`` there too.  Here construction succeeds for such inputs — training
    and ECDF sampling do not need the density — and ``log_latent_pdf``,
    ``cst_log_dens`` and the KDE sampler raise ``MsgmError`` when first used.
    Only ``kernel='gaussian'`` is built.

    Upstream's defects of this density are mirrored, not fixed: the missing
    ``|x|^(d-1) / S_(d-1)`` factor (see the WARNING comments at SDEs.py:504-505)
    and, with ``norm_map="log"``, a density fitted on ``log(r + 1e-6)`` but
    queried with the raw norm (SDEs.py:236, 506) — queries then sit many
    bandwidths from every sample and the log-density is large and negative."""

    def __init__(self, y0, beta_min=0.1, beta_max=20.0, T=1.0, t_epsilon=0.001, denseTensor=True,
                 norm_sampler="ecdf", norm_map=None, kernel='gaussian', plot_validate=False,
                 num_steps_forward=100, device='cpu', estim_cst_norm_dens_r_T=True, G=None):
        super().__init__(beta_min, beta_max, T, t_epsilon, num_steps_forward, device)
        if norm_sampler not in ("ecdf", "kde"):
            raise MsgmError("norm_sampler must be 'ecdf' or 'kde'")
        self.sparseTensor = not denseTensor
        self.kind = L.SDE_MSGM_DENSE if denseTensor else L.SDE_MSGM_SPARSE
        self.norm_correction = True
        self.r_T = torch.linalg.norm(y0, dim=1)
        self.norm_map = norm_map
        if norm_map == "log":
            self.r_T = torch.log(self.r_T + 1e-6)
        # SDEs.py:239 (unbiased std of the mapped radii); NaN when there is a single row
        self.bandwidth = 0.1 * torch.std(self.r_T).item() if self.r_T.numel() > 1 else float("nan")
        self.kernel = kernel
        self.r_T = self.r_T.to(self.device)
        self.norm_sampler = norm_sampler
        self.dim = y0.shape[1]
        self.name_SDE = "MSGM"
        if denseTensor:
            self.G = (G if G is not None else self.new_G(self.dim)).to(self.device).contiguous()
            self.L_G = (0.5 * torch.einsum('ijk, jmk -> im', self.G, self.G)).contiguous()      # SDEs.py:246
        else:
            self.name_SDE += "_sparseTens"
            self.sparse_G(self.dim)
            self.L_G = 0.5 * torch.eye(self.dim, device=self.device)
        if norm_sampler != "ecdf":
            self.name_SDE += norm_sampler + kernel                                          # SDEs.py:252-253
        if norm_map == "log":
            self.name_SDE += "logNorm"
        self.estim_cst_norm_dens_r_T = bool(estim_cst_norm_dens_r_T or plot_validate)       # SDEs.py:256-257
        self._cst_log_dens = None
        self._G_packed = None        # G and L_G in the dense sampler loop's fragment order: built on first use (packed_G)
        self._G_packed_stage = None  # the same for msgm_sde_stage_dense_mm above n = 32 (packed_G_stage)

    def to(self, device):
        new = super().to(device)
        new.r_T = self.r_T.to(device)
        if self._cst_log_dens is not None:
            new._cst_log_dens = self._cst_log_dens.to(device)
        if self.sparseTensor:
            for k in ("G_I", "G_J", "G_K", "G_V"):
                setattr(new, k, getattr(self, k).to(device))
        else:
            new.G = self.G.to(device).contiguous()
        new.L_G = self.L_G.to(device).contiguous()
        new._G_packed = None         # rebuilt from the moved tensors when next needed
        new._G_packed_stage = None
        return new

    def packed_G(self):
        """ops.pack_dense_g(G, L_G) for msgm_mlp_dense_sde_loop, built once per tensor on G's device.  A plain attribute:
        not in state_dict() or checkpoints, and dropped by to()."""
        if self.sparseTensor:
            raise MsgmError("packed_G: the sparse tensor has no dense image")
        if self._G_packed is None or self._G_packed.device != self.G.device:
            self._G_packed = ops.pack_dense_g(self.G, self.L_G)
        return self._G_packed

    def packed_G_stage(self):
        """ops.pack_dense_g_stage(G, L_G) for msgm_sde_stage_dense_mm, built once per tensor on G's device.  For
        17 <= n <= 32 the image is packed_G()'s and that one copy serves both kernels.  A plain attribute like packed_G: not in
        state_dict() or checkpoints, and dropped by to()."""
        if self.sparseTensor:
            raise MsgmError("packed_G_stage: the sparse tensor has no dense image")
        if 17 <= self.G.shape[0] <= 32:
            return self.packed_G()
        if self._G_packed_stage is None or self._G_packed_stage.device != self.G.device:
            self._G_packed_stage = ops.pack_dense_g_stage(self.G, self.L_G)
        return self._G_packed_stage

    @staticmethod
    def new_G(n):
        """n skew-symmetrised Gaussian matrices scaled so trace(L_G) = -n/2
        (SDEs.py:315-341); drawn from torch's CPU generator."""
        G = torch.zeros(n, n, n)
        for k in range(n):
            F = torch.randn(n, n)
            G[:, :, k] = 0.5 * (F - F.T)
        L_G = 0.5 * torch.einsum('ijk, jmk -> im', G, G)
        return torch.sqrt(-0.5 * n / torch.trace(L_G)) * G

    def sparse_G(self, n):
        """Index lists of the sparse tensor (SDEs.py:369-399) — kept for API
        compatibility; the stencil kernel never reads them."""
        k = torch.arange(n, dtype=torch.int64)
        kp = (k + 1) % n
        self.G_I = torch.stack([k, kp], 1).reshape(-1).to(self.device)
        self.G_J = torch.stack([kp, k], 1).reshape(-1).to(self.device)
        self.G_K = torch.stack([k, k], 1).reshape(-1).to(self.device)
        c = 0.5 * torch.sqrt(torch.tensor(2, dtype=torch.float32))
        self.G_V = torch.stack([c.expand(n), (-c).expand(n)], 1).reshape(-1).contiguous().to(self.device)

    def IJK(self):
        return (self.G_I, self.G_J, self.G_K) if self.sparseTensor else (None, None, None)

    def sparse_G_full(self, n):
        """Dense (n,n,n) image of the sparse nearest-neighbour rotation tensor (SDEs.py:343-367), for checks."""
        k = torch.arange(n)
        kp = (k + 1) % n
        c = 0.5 * math.sqrt(2.0)
        G = torch.zeros(n, n, n, device=self.device)
        G[k, kp, k] = c
        G[kp, k, k] = -c
        self.G = G
        return G

    # -- accessors (API compatibility) ----------------------------------------
    def f(self, t, y):
        b = self.beta(t)
        return 0.5 * b * y if self.sparseTensor else torch.einsum('ij, bj -> bi', self.L_G, b * y)

    def f_strato(self, t, y):
        return torch.zeros_like(y)

    def div_Sigma(self, t, y):
        return 2 * self.f(t, y)

    def g(self, t, y, sparse=False):
        b = self.beta(t)
        if sparse:
            return self.G_V.unsqueeze(0) * ((b ** 0.5) * y[:, self.G_J])
        return torch.einsum('ijk, bj -> bik', self.G, (b ** 0.5) * y)

    # -- hot path --------------------------------------------------------------
    @torch.no_grad()
    def sample(self, t, y0, return_noise=False, noise_main=None, noise_short=None):
        """y_t | y_0 by RK4 on the forward process, entirely on the device:
        masked multi-stop integration replaces the per-row Python loop and the
        D2H/H2D round trips of SDEs.py:78-122."""
        if return_noise:
            raise NotImplementedError('See the official repository.')
        from .sde_scheme import msgm_forward_perturb
        return msgm_forward_perturb(self, t, y0, noise_main=noise_main, noise_short=noise_short)

    def gen_radial_distribution(self, num_samples, u=None, z=None):
        """Radii of the latent (SDEs.py:438-465).  'ecdf': empirical quantiles of ``r_T`` at ``u``.  'kde': what
        ``KernelDensity.sample`` draws for a Gaussian kernel, ``r_T[floor(u Ns)] + h z``, negative radii set to 0
        unless the radii are log-mapped (upstream's own branch cannot run: undefined global at SDEs.py:444).
        ``u`` (uniform) and ``z`` (normal), each (num_samples,), inject the draws; otherwise they come from the
        SDE's Philox stream, which advances once per call."""
        kde = self.norm_sampler == "kde"
        if kde:
            self._kde_check()
        if u is None or (kde and z is None):
            rng = self.philox(self.device)
            if u is None:
                u = ops.fill_uniform(torch.empty(num_samples, dtype=torch.float32, device=self.device), rng, L.RNG_STREAM_ROWS)
            if kde and z is None:
                z = ops.fill_normal(torch.empty(num_samples, dtype=torch.float32, device=self.device), rng,
                                    L.RNG_STREAM_USER + 2)
            rng.advance(1)
        if kde:
            Ns = self.r_T.numel()
            i = torch.floor(u.reshape(-1) * Ns).long().clamp_(max=Ns - 1)
            r = (self.r_T[i] + self.bandwidth * z.reshape(-1)).reshape(num_samples, 1)
            if self.norm_map != "log":
                r = r.clamp_min(0.)                                                # SDEs.py:445-447
        else:
            r = torch.quantile(self.r_T, u).reshape(num_samples, 1)                # SDEs.py:442
        if self.norm_map == "log":
            r = torch.exp(r) - 1e-6
        return r

    def latent_sample(self, num_samples, n, u=None, z=None):
        r = self.gen_radial_distribution(num_samples, u)
        s = randu_on_sphere((num_samples, self.dim), self.device, z=z, rng=self.philox(self.device))
        return r * s

    def cond_latent_sample(self, t_, T, x):
        r_x = torch.linalg.norm(x.detach().to(self.device), dim=1).reshape(x.shape[0], 1)
        return r_x * randu_on_sphere((x.shape[0], self.dim), self.device, rng=self.philox(self.device))

    def _kde_check(self):
        if self.kernel != 'gaussian':
            raise MsgmError(f"only the Gaussian kernel density is built (kernel={self.kernel!r})")
        if not (math.isfinite(self.bandwidth) and self.bandwidth > 0.):
            raise MsgmError(f"the kernel density of the radii needs a positive bandwidth 0.1 * std(r_T), got "
                            f"{self.bandwidth} (one row, or all radii equal)")

    @property
    def cst_log_dens(self):
        """log of the density's integral over [min r_T, max r_T] by a 1000-point Riemann sum (SDEs.py:258-265) — a device
        scalar, computed when first needed; 0 without ``estim_cst_norm_dens_r_T``."""
        if not self.estim_cst_norm_dens_r_T:
            return 0
        if self._cst_log_dens is None or self._cst_log_dens.device != self.r_T.device:
            self._kde_check()
            r = self.r_T.contiguous()
            lo, hi = r.min(), r.max()
            # torch.linspace(lo, hi, 1000) as the CPU computes it — fp32 fma(step, k, lo) from the left half, fma(-step,
            # 999 - k, hi) from the right — without reading lo / hi on the host.  Bit-exactness matters: upstream's
            # dr = grid[1] - grid[0] is an fp32 difference of neighbours and carries their rounding.
            step = ((hi - lo) / 999.).double()
            k = torch.arange(1000, dtype=torch.float64, device=r.device)
            grid = torch.where(k < 500, lo.double() + step * k, hi.double() - step * (999. - k)).float()
            dens = torch.exp(ops.kde_logpdf(grid, r, self.bandwidth))
            self._cst_log_dens = torch.log(dens.sum() * (grid[1] - grid[0]))
        return self._cst_log_dens

    def log_latent_pdf(self, yT):
        """Log-density (M,) of the latent's radius |yT| under the kernel density of ``r_T``, minus ``cst_log_dens``
        (SDEs.py:503-509): row norm + one log-space KDE kernel on the device, no host synchronisation."""
        self._kde_check()
        cst = self.cst_log_dens
        lp = ops.kde_logpdf(ops.row_norm(yT.detach().contiguous().float()), self.r_T.contiguous(), self.bandwidth)
        return lp - cst


# ---------------------------------------------------------------------------
def sample_rademacher(shape, device, rng: Optional[PhiloxState] = None, u=None):
    """2[U>=1/2]-1 (SDEs.py:514-515) drawn in one kernel."""
    return ops.rademacher(tuple(shape), device, u=u, rng=rng)


def sample_gaussian(shape, device, rng: PhiloxState):
    return ops.fill_normal(torch.empty(tuple(shape), dtype=torch.float32, device=device), rng, L.RNG_STREAM_USER)


def randu_on_sphere(shape, device, z=None, rng: Optional[PhiloxState] = None):
    """Uniform direction: Gaussian / its norm (SDEs.py:520-526)."""
    if z is None:
        z = torch.empty(tuple(shape), dtype=torch.float32, device=device)
        ops.fill_normal(z, rng, L.RNG_STREAM_USER + 1)
        rng.advance(1)
    return z / ops.row_norm(z.contiguous()).reshape(shape[0], 1)


def sample_v(shape, device, vtype='rademacher', rng: Optional[PhiloxState] = None):
    if vtype == 'rademacher':
        return sample_rademacher(shape, device, rng)
    if vtype in ('normal', 'gaussian'):
        return sample_gaussian(shape, device, rng)
    if vtype == 'uniform':
        return randu_on_sphere(shape, device, rng=rng)
    raise MsgmError(f'vtype {vtype} not supported')


def intT_kept_grid(nsf: int, T: float, t_epsilon: float):
    """The time grid of the integrated loss on the host: (kept times (nsf',) fp32, k0).  linspace(T/nsf, T, nsf) with the
    entries <= t_epsilon dropped (SDEs.py:695-706); they are a prefix of length k0 because the grid increases.  nsf' = 0 raises."""
    t_ = torch.linspace(T / nsf, T, nsf)
    k0 = int((t_ <= t_epsilon).sum())
    if k0 == nsf:
        raise MsgmError(f"ssm_intT: every grid time of the {nsf}-step grid is <= t_epsilon = {t_epsilon}; no row is left")
    return t_[k0:], k0


class PluginReverseSDE(nn.Module):
    """Plug-in reverse SDE (SDEs.py:538-729): f <- g a - f, time reversed.

    ``ssm(x)`` is the training entry point.  With an ``MLP`` score net on an
    ``SGMsde`` it runs the fully fused path: perturbation (K1), probe (K14)
    and ONE persistent kernel for forward + tangent + loss + backward (K5),
    which writes the parameter gradients of ``ssm(x).mean()`` straight into
    the flat ``.grad`` bucket.  The returned per-sample tensor carries a
    backward hook that rescales those gradients by ``grad_output.sum()``,
    so the reference loop ``gen_sde.ssm(x).mean().backward()`` works as is
    (uniform reductions only — which is all the driver uses,
    MSGM_higherDim.py:807)."""

    def __init__(self, base_sde, drift_a, T, vtype='rademacher', debias=False, ssm_intT=False, deviceReverseSDE='cpu'):
        super().__init__()
        if ssm_intT and torch.device(deviceReverseSDE).type != "cuda":
            # the integrated loss exists on the HIP path only (one-launch path kernel, fused passes): refused where the
            # object is built, like every other option without a kernel, not at the first ssm() call
            raise MsgmError("ssm_intT=True needs the reverse SDE on a cuda device (deviceReverseSDE=...); there is no CPU fallback")
        self.base_sde = base_sde.to(deviceReverseSDE)
        self.a = drift_a
        self.T = T.to(deviceReverseSDE)
        self.vtype = vtype
        self.ssm_intT = bool(ssm_intT)
        self._intT = {}
        self.debias = debias
        self.deviceReverseSDE = deviceReverseSDE
        self._ws = None

    # ---- drift / diffusion (integrators call the stage kernel directly; these
    # keep the reference's call surface) ---------------------------------------
    def _stage(self, t, y, lmbd, strato):
        T = self.base_sde.T_float()
        B = y.shape[0]
        if torch.is_tensor(t) and t.is_cuda:
            # the reference passes t as a (B,1) device tensor filled with one value (sde_scheme.py:81): keep it on the device
            # — the stage kernel reads its clock from t_dev — instead of a .item() round trip per mu() call
            t0 = t.reshape(-1)[:1].to(device=y.device, dtype=torch.float32).contiguous()
            s = (T - t0).expand(B).contiguous()
            tt, t_dev = 0.0, t0
        else:
            tt, t_dev = (float(t.reshape(-1)[0]) if torch.is_tensor(t) else float(t)), None
            s = torch.full((B,), T - tt, dtype=torch.float32, device=y.device)
        a = self.a(y, s)
        out = torch.empty_like(y)
        zero = torch.zeros_like(y)
        ops.sde_stage(out, None, 1.0, y.contiguous(), a, self.base_sde.struct(), L.PROC_REVERSE, strato, tt, 1.0,
                      lmbd, dW=zero, t_dev=t_dev)
        return out

    def mu(self, t, y, lmbd=0.):
        """Ito drift at reverse time t (batch-uniform t, as the integrators use it)."""
        return self._stage(t, y, lmbd, False)

    def mu_Strato(self, t, y, lmbd=0.):
        return self._stage(t, y, lmbd, True)

    def sigma(self, t, y, lmbd=0., sparse=False):
        return (1. - lmbd) ** 0.5 * self.base_sde.g(self.T - t, y, sparse)

    def ga(self, s, y):
        """g(s, y) . a(y, s) with a per-row forward time s (SDEs.py:563-580).  Accessor-level (the integrators use
        the fused stage kernel through ``mu`` / ``mu_Strato`` instead, which takes a batch-uniform time)."""
        base = self.base_sde
        a = self.a(y, s.reshape(-1))
        if base.kind == L.SDE_SGM:
            return base.g(s, y) * a
        if base.sparseTensor:
            I, _, K = base.IJK()
            return torch.zeros_like(y).scatter_add_(1, I.unsqueeze(0).expand(y.shape[0], -1), base.g(s, y, True) * a[:, K])
        return torch.einsum('bij, bj -> bi', base.g(s, y), a)

    def ga_m_drift(self, s, y, lmbd=0.):
        """Drift of the reverse generative SDE at forward time s (SDEs.py:560-561); mu(t) = ga_m_drift(T - t)."""
        base = self.base_sde
        return (1. - 0.5 * lmbd) * self.ga(s, y) - base.f(s, y) + (1. - lmbd) * base.div_Sigma(s, y)

    def sample_t_linspace(self, x):
        """Gridded t in (0, T] with the entries <= t_epsilon dropped (SDEs.py:695-706); returns (t, mask)."""
        nsf = self.base_sde.num_steps_forward
        T = self.base_sde.T_float()
        t_ = torch.linspace(T / nsf, T, nsf).to(x.device)
        mask_le_t_eps = (t_ <= self.base_sde.t_epsilon)
        return t_[~mask_le_t_eps], mask_le_t_eps

    def intT_grid(self, dev):
        """``ssm_intT``: (the kept grid times on ``dev`` (nsf',), k0 = the number of dropped leading entries).  The grid and
        the ``<=`` mask are ``sample_t_linspace``'s, formed on the host (no device read) and cached per
        (nsf, T, t_epsilon, device); the dropped entries are a prefix because the grid increases.  nsf' = 0 raises."""
        base, dev = self.base_sde, torch.device(dev)
        nsf, T = base.num_steps_forward, base.T_float()
        key = (nsf, T, float(base.t_epsilon), dev)
        if key not in self._intT:
            t_, k0 = intT_kept_grid(nsf, T, base.t_epsilon)
            if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise MsgmError("the ssm_intT time grid is needed for the first time inside a graph capture; run one eager step first")
            self._intT[key] = (t_.to(dev), k0)
        return self._intT[key]

    # ---- SSM loss -------------------------------------------------------------
    def sample_t(self, x, u=None):
        """t ~ U(0,T) clamped at t_epsilon (SDEs.py:684-693) — returned by
        ``sample_txy``; fused into the perturbation kernel."""
        return self.sample_txy(x, u=u)[0]

    @torch.no_grad()
    def sample_txy(self, x, u=None, eps=None):
        """(t, x, y).  With ``ssm_intT`` (SDEs.py:653-676): one RK4 path of the forward process per row of x, every grid
        state with t > t_epsilon a training row, time-major — row j B + b holds (t_grid[k0 + j], x[b], y[k0 + j, b]);
        ``eps`` is the (nsf, B, n) path noise, and ``u`` has no meaning (there is no time draw)."""
        base = self.base_sde
        if self.ssm_intT:
            if u is not None:
                raise MsgmError("ssm_intT: u= injects the time draw, and the integrated loss draws no time")
            from .sde_scheme import msgm_forward_paths
            B, n = x.shape
            tk, k0 = self.intT_grid(x.device)
            y = msgm_forward_paths(base, x, first_keep=k0, noise=eps)
            return (tk.repeat_interleave(B).reshape(-1, 1), x.repeat(tk.numel(), 1), y.reshape(tk.numel() * B, n))
        if base.kind != L.SDE_SGM:
            rng = base.philox(x.device)
            if u is None:
                u = ops.fill_uniform(torch.empty(x.shape[0], device=x.device), rng, L.RNG_STREAM_T)
            T = base.T_float()
            t = u.reshape(-1, 1) * T
            m = (t <= base.t_epsilon).float()
            t = m * base.t_epsilon + (1. - m) * t
            nm, ns = eps if isinstance(eps, (tuple, list)) else (None, None)     # (noise_main, noise_short)
            return t, x, base.sample(t, x, noise_main=nm, noise_short=ns)
        rng = None if (u is not None and eps is not None) else base.philox(x.device)
        y, t = ops.perturb_vp(x.contiguous(), base.struct(), u=u, eps=eps, rng=rng)
        return t.reshape(-1, 1), x, y

    def ssm(self, x, u=None, eps=None, u_v=None, y=None, t_given=None, v=None, row_weight=None):
        """Per-sample SSM loss (B,), gradients of its mean accumulated into the
        score net's ``.grad`` (see class docstring).  ``row_weight`` (B,) float32 on the device, any sign: the returned
        tensor is w (.) L and its ``.mean()`` / ``.sum()`` differentiate as upstream's do; the weights go into the fused
        pass of this call (with a dropout net: the live stream's masks).  Zero-weight rows still flow through the
        arithmetic, so keep them finite.  Any other weighting of the rows of the result (a non-uniform cotangent) costs
        one more fused pass in ``backward``.  ``u``/``eps``/``u_v``
        inject the three draws of SDEs.py:688,141,515 (parity tests); ``v`` injects
        the probe itself (any ``vtype``).  ``vtype`` 'gaussian' / 'uniform' (sphere)
        probes (SDEs.py:517-536) are drawn from the Philox stream and go through the
        general form of the loss (u = (dmu/da)^T v, cst = v^T (d(-f)/dy) v)."""
        from .NN import MLP
        base = self.base_sde
        net = self.a
        if not (isinstance(net, MLP) or hasattr(net, "ssm_grad")):
            raise MsgmError(f"no HIP SSM path for score net {type(net).__name__}")
        if self.vtype not in ('rademacher', 'normal', 'gaussian', 'uniform'):
            raise MsgmError(f'vtype {self.vtype} not supported')
        x = x.contiguous().float()
        B, d = x.shape
        dev = x.device
        intT = self.ssm_intT and y is None           # ssm_loss(t_, x, y) ignores the flag, as upstream does
        if intT:
            if u is not None:
                raise MsgmError("ssm_intT: u= injects the time draw, and the integrated loss draws no time")
            B *= self.intT_grid(dev)[0].numel()      # nsf' B training rows; nsf' = 0 raises here, before any launch
        ops._row_weight(row_weight, B)               # CPU / wrong length / wrong dtype: refused before any launch or draw
        rng = base.philox(dev)
        if y is None:
            t, _, y = self.sample_txy(x, u=u, eps=eps)
        else:                                        # (t, y) given: the ssm_loss(t_, x, y) entry of the reference
            t = t_given.reshape(-1, 1).contiguous().float()
            y = y.contiguous().float()
        pm1 = v is None and self.vtype == 'rademacher'          # probe entries are +-1: |v|^2 = d is baked into the fused kernel
        drew_v = v is None and not (pm1 and u_v is not None)
        if v is not None:
            v = v.contiguous().float()
        elif pm1:
            v = ops.rademacher((B, d), dev, u=u_v, rng=None if u_v is not None else rng)
        else:
            v = sample_v((B, d), dev, self.vtype, rng=rng).contiguous()
        if drew_v or (t_given is None and not intT and (u is None or eps is None)):
            rng.advance(1)                           # (ssm_intT: the path draws advanced the stream by nsf themselves)
        st = base.struct()
        uu = cst = None
        if base.kind != L.SDE_SGM or not isinstance(net, MLP) or not pm1:
            # general form of the loss: loss_b = adot.u + cst + |a|^2/2 (u = G(y)^T v for the multiplicative SDE)
            uu, cst = ops.ssm_terms(y, v, t.reshape(-1).contiguous(), st)
        per, gtmp, gflat = self._ssm_pass(y, t.reshape(-1), v, uu, cst, 1.0 / B, row_weight, rng)
        if row_weight is not None:
            per = per * row_weight                   # the returned tensor is w (.) L; gtmp = (1/B) sum_b w_b dL_b
        return _SSMGradBridge.apply(per, gtmp, gflat, net, B, next(net.parameters()), self,
                                    (y, t, v, uu, cst), row_weight)

    def _ssm_pass(self, y, t, v, uu, cst, inv_batch, row_weight, rng):
        """One fused pass: (per-sample losses, d(inv_batch sum_b w_b L_b)/d(params) as a flat tensor of its own, the
        net's flat gradient bucket, left as it was)."""
        from .NN import MLP
        net = self.a
        B, d = y.shape
        dev = y.device
        flat, gflat = net.flat_parameters()
        if isinstance(net, MLP):
            if self._ws is None or self._ws.device != dev:
                self._ws = ops.mlp_ssm_workspace(d, net.pre is not None, dev)
            per = torch.empty(B, dtype=torch.float32, device=dev)
            gtmp = torch.empty_like(gflat)
            ops.mlp_ssm_grad(net.kernel_params(), y, t, v, self.base_sde.struct(), inv_batch, gtmp, self._ws, loss_per=per, u=uu,
                             cst=cst, row_weight=row_weight)
        else:
            # U-Nets: dual-number forward + hand-written backward; the net writes its flat .grad bucket
            # (what was accumulated so far is put back afterwards; a parameter whose .grad is None — zero_grad() —
            # has accumulated nothing, whatever its slice of the bucket still holds)
            keep = gflat.clone()
            off = 0
            for p_ in net.parameters():
                if p_.grad is None:
                    keep[off:off + p_.numel()].zero_()
                off += p_.numel()
            # a 2-D U-Net with active dropout draws its masks from the SDE's stream (shard base, checkpoint, graph replay)
            per = net.ssm_grad(y, t, v, uu, cst, inv_batch, rng=rng, row_weight=row_weight)
            flat, gflat = net.flat_parameters()
            gtmp = gflat.clone()
            gflat.copy_(keep)
        return per, gtmp, gflat

    def ssm_loss(self, t_, x, y, u_v=None, row_weight=None):
        """Reference entry point (SDEs.py:616-646) with (t, y) given: same fused forward-mode kernels as ``ssm``."""
        return self.ssm(x, u_v=u_v, y=y, t_given=t_, row_weight=row_weight)

    def latent_sample(self, num_samples, n):
        return self.base_sde.latent_sample(num_samples, n)

    def cond_latent_sample(self, t_, T, x):
        return self.base_sde.cond_latent_sample(t_, T, x)

    def elbo_random_t_slice(self, x, u=None, eps=None, u_v=None, eps_T=None, y=None, t_given=None, yT=None):
        """ELBO slice estimate lp(y_T) - ssm(x) T (SDEs.py:708-721); the loss term runs on the same fused kernels as
        training.  The latent term is the standard normal's log-density for the additive SDE and the kernel density
        of the radii for the multiplicative one (``MSGMsde.log_latent_pdf``).  For parity tests ``u``/``eps``/``u_v``
        inject the draws of ``ssm``, ``y``/``t_given`` are forwarded to it, ``eps_T`` is the noise of the additive
        SDE's ``cond_latent_sample`` and ``yT`` replaces that draw altogether."""
        base = self.base_sde
        if base.kind != L.SDE_SGM:
            base._kde_check()                          # refuse before any work is queued
        x = x.contiguous().float()
        qt = 1.0 / base.T_float()
        with torch.no_grad():
            loss_ssm = self.ssm(x, u=u, eps=eps, u_v=u_v, y=y, t_given=t_given).detach() / qt
            if self.ssm_intT and y is None:          # the latent term runs on the tiled x (SDEs.py:717-719)
                x = x.repeat(loss_ssm.numel() // x.shape[0], 1)
            if yT is None:
                t_ = torch.empty(x.shape[0], 1, device=x.device)
                yT = (base.cond_latent_sample(t_, base.T_float(), x, eps=eps_T) if base.kind == L.SDE_SGM
                      else base.cond_latent_sample(t_, base.T_float(), x))
            lp = base.log_latent_pdf(yT).view(x.size(0), -1).sum(1)
        return lp - loss_ssm


class _SSMGradBridge(torch.autograd.Function):
    """Lets ``ssm(x).mean().backward()`` deliver the kernel-computed parameter gradients.  Upstream's ``ssm`` returns an
    ordinary autograd tensor (SDEs.py:607-646), so any weighting of its rows back-propagates; here the gradient of the
    mean, ``gmean = (1/B) sum_b w_b dL_b`` (w = ``row_weight`` or ones), was formed inside the fused pass of the forward
    call, and ``backward`` has two paths:

    * uniform cotangent (every entry bit-equal: ``.mean()``, ``.sum()``, a scalar factor): adds
      ``sum(grad_output) * gmean`` to the flat gradient bucket (sum_b c w_b dL_b = c B gmean).  One element and a
      stride-0 expansion are recognised without a device synchronisation; anything else costs one device comparison,
      whose host read is confined to this eager surface (the trainers never pass through the bridge).
    * non-uniform cotangent: one more fused pass over the saved ``(y, t, v, u, cst)`` with the row weights
      ``grad_output`` (times ``row_weight`` where one was given) and ``inv_batch = 1``.  A 2-D U-Net whose dropout was
      active in the forward call cannot be re-run with the same masks from here and raises ``MsgmError``."""

    @staticmethod
    def forward(ctx, per, gmean, gflat, net, B, anchor, sde=None, saved=None, row_weight=None):
        # `anchor` (a parameter that requires grad) only makes autograd record this node
        ctx.gmean, ctx.gflat, ctx.net, ctx.B = gmean, gflat, net, B
        # by reference, no copies: the operands of a second fused pass
        ctx.sde, ctx.saved, ctx.row_weight = sde, saved, row_weight
        ctx.dropout = bool(getattr(net, "dropout_active", lambda: False)())
        return per.clone()

    @staticmethod
    def _uniform(g) -> bool:
        if g.numel() == 1 or all(st == 0 for st in g.stride()):
            return True
        bits = g.contiguous().view(torch.int32).reshape(-1)
        return bool((bits == bits[0]).all())

    @staticmethod
    def backward(ctx, grad_out):
        net = ctx.net
        gadd = None
        if ctx.saved is not None and not _SSMGradBridge._uniform(grad_out):
            if ctx.dropout:
                raise MsgmError("ssm(): a non-uniform weighting of the rows needs a second pass, and a 2-D U-Net with active "
                                "dropout cannot be re-run with the forward call's masks; pass the weights as "
                                "ssm(x, row_weight=w), which applies them inside the forward call")
            w = grad_out.detach().reshape(-1).contiguous().float()
            if ctx.row_weight is not None:
                w = w * ctx.row_weight
            y, t, v, uu, cst = ctx.saved
            with torch.no_grad():
                _, gadd, _ = ctx.sde._ssm_pass(y, t.reshape(-1), v, uu, cst, 1.0, w, None)
        else:
            scale = grad_out.sum()          # = c*B for a uniform weight c; gmean already carries 1/B
        flat, gflat = net.flat_parameters()
        off = 0
        for p in net.parameters():
            k = p.numel()
            if p.grad is None or p.grad.data_ptr() != gflat[off:off + k].data_ptr():
                gflat[off:off + k].zero_()
                p.grad = gflat[off:off + k].view(p.shape)
            off += k
        gflat.add_(ctx.gmean * scale if gadd is None else gadd)
        return None, None, None, None, None, None, None, None, None
