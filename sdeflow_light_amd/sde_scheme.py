"""SDE integrators on HIP kernels — host mirror of the reference's
``sde_scheme.py`` (same function names, argument lists, return layout and
error behaviour: sde_scheme.py:44-46,73-75,94-99).

Per step the reference launches ~20 eager kernels plus a host ``.item()`` and,
with ``keep_all_samples``, a blocking D2H copy (sde_scheme.py:80-92).  Here a
step is ONE fused stage kernel after the score net (or one kernel in total for
MLP + SGM: ``msgm_mlp_em_step``; with the MLP, Heun, RK4-Stratonovich and the multiplicative Euler-Maruyama are one
kernel for the WHOLE loop, ``msgm_mlp_sde_loop``, ``msgm_mlp_xw_sde_loop`` or ``msgm_mlp_dense_sde_loop``, when ``_Run.mlp_loop`` finds the shape
routed there), the time grid is computed on the host exactly
as upstream (fp32 ``linspace``) and passed by value, trajectories are captured
into a device buffer and copied once at the end, and the whole fused loop can
be replayed as a single hipGraph (``GraphedEMSampler``).

Extra keyword ``noise=`` (steps,B,n) injects the standard-normal draws
(parity tests); otherwise each step uses the Philox stream of the base SDE.
"""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional

import torch

from . import _lib as L
from . import ops
from ._lib import MsgmError


def EMstep(mu, delta, sigma, dW, sparse=False, I=None, K=None):
    """Kept for API compatibility (sde_scheme.py:18-40); the integrators below
    never materialise mu / sigma — they call the fused stage kernel."""
    if sparse:
        prod = sigma * dW[:, K]
        dx = torch.zeros_like(dW)
        dx.scatter_add_(1, I.unsqueeze(0).expand(dW.size(0), -1), prod)
    elif sigma.dim() > 2:
        dx = torch.einsum('bij, bj -> bi', sigma, dW)
    else:
        dx = sigma * dW
    return mu * delta + dx


class _Clock(NamedTuple):
    """The process an integrator step advances and where its stage times, step length and Wiener draw come from.  The
    three calling styles differ here and nowhere else:
      eager samplers (``_Run.clock``): host stage times ``t=``, the step's ``z=`` or the Philox step index ``rng_step=i``;
      ``GraphedStepSampler``: ``t_dev=`` the device clocks ``time_tick`` sets, ``step_dev=`` the device step counter;
      the short rows of ``msgm_forward_perturb_composed``: ``delta_rows=`` with ``t_frac=`` (times 0, t_b/2, t_b), ``delta = 0``."""
    struct: object
    proc: int
    lmbd: float
    delta: float
    at: list            # at[k]: the keywords that place a stage at the step's k-th distinct stage time
    draw: dict          # the keywords of the stage that draws the step's Wiener increment
    score: Callable     # (x, k) -> a(x, T - t_k) for the reverse process, None for the forward one
    packed: object = None   # the dense tensor's fragment image where ``ops.stage_dense_mm_preferred`` routes the stage (``_stage_image``)

    def stage(self, k, out, base, c_out, x, strato, **kw):
        """out = base + c_out * (the increment at x and stage time k); the score is evaluated first.  The one place that
        picks the stage kernel: with ``packed`` the dense contraction runs on the matrix cores (``msgm_sde_stage_dense_mm``)."""
        a = self.score(x, k)
        if self.packed is not None:
            return ops.sde_stage_dense_mm(out, base, c_out, x, a, self.struct, self.proc, strato, delta=self.delta,
                                          lmbd=self.lmbd, packed=self.packed, **self.at[k], **kw)
        return ops.sde_stage(out, base, c_out, x, a, self.struct, self.proc, strato, delta=self.delta,
                             lmbd=self.lmbd, **self.at[k], **kw)


def _stage_image(base, struct, n, proc):
    """The ``packed`` field of a clock: the base SDE's cached fragment image (built here on first use, so before any capture)
    where ``ops.stage_dense_mm_preferred`` takes the shape — the dense tensor, the reverse process, 31 <= n <= 64 — else None."""
    return base.packed_G_stage() if ops.stage_dense_mm_preferred(struct.kind, n, proc) else None


def _em_step(c, x, other, norm0):
    """Euler-Maruyama (sde_scheme.py:80-86).  The additive SDE updates x in place; the stencil / contraction of the
    multiplicative ones reads neighbours, so they write ``other``.  Returns the buffer that holds the new state."""
    out = x if c.struct.kind == L.SDE_SGM else other
    return c.stage(0, out, x, 1.0, x, False, norm0=norm0, **c.draw)


def _heun_step(c, x, bufs, norm0):
    """Heun in Stratonovich form, stage times (t, t + delta) (sde_scheme.py:101-172); the new state is in bufs[-1]."""
    dW, k1, xp, xn = bufs
    c.stage(0, xp, x, 1.0, x, True, dW_out=dW, inc_out=k1, **c.draw)       # predictor x + K1 (keeps K1 and the Wiener increment)
    ops.lincomb(xn, x, 1.0, k1, 0.5)                                       # x + K1/2
    # corrector: (x + K1/2) + K2/2, K2 evaluated at the predictor (out aliases base, not x_eval)
    return c.stage(1, xn, xn, 0.5, xp, True, dW=dW, norm0=norm0)


def _rk4_step(c, x, bufs, norm0):
    """RK4-Stratonovich, stage times (t, t + delta/2, t + delta), one dW (sde_scheme.py:174-269); the new state is in bufs[-1]."""
    dW, k1, k2, k3, k4, xm, xn = bufs
    c.stage(0, xm, x, 0.5, x, True, dW_out=dW, inc_out=k1, **c.draw)       # x + K1/2
    c.stage(1, xn, x, 0.5, xm, True, dW=dW, inc_out=k2)
    c.stage(1, xm, x, 1.0, xn, True, dW=dW, inc_out=k3)
    c.stage(2, k4, None, 1.0, xm, True, dW=dW)
    return ops.rk4_combine(xn, x, k1, k2, k3, k4, norm0=norm0)


def _capture(body, dev):
    """body() once on a side stream (loads the code objects: nothing of that may happen during capture), then captured."""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = ops.new_graph()
    with torch.cuda.graph(graph):
        body()
    return graph


class _Run:
    """Shared set-up of the three samplers (sde_scheme.py:50-78)."""

    def __init__(self, sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_, norm_correction,
                 noise):
        from .SDEs import PluginReverseSDE, forward_SDE
        self.sde = sde
        self.base = sde.base_sde
        self.device = sde.T.device
        if self.device.type != "cuda":
            raise MsgmError("the HIP integrators need the SDE on a cuda device; there is no CPU fallback")
        if x_0.dim() != 2:
            raise MsgmError("state must be 2-D (B,n)")
        self.B, self.n = x_0.shape
        self.T_ = L.host_scalar(sde.T) if (not torch.is_tensor(T_) and T_ == -1) else L.host_scalar(T_)   # sde_scheme.py:54-57
        self.N = num_steps
        self.delta = self.T_ / num_steps
        self.ts = torch.linspace(0, 1, num_steps + 1) * self.T_               # fp32, host (sde_scheme.py:59)
        self.lmbd = float(lmbd)
        self.reverse = isinstance(sde, PluginReverseSDE)
        if not self.reverse and not isinstance(sde, forward_SDE):
            raise MsgmError("sde must be a PluginReverseSDE or a forward_SDE")
        self.proc = L.PROC_REVERSE if self.reverse else L.PROC_FORWARD
        self.struct = self.base.struct()
        self.packed = _stage_image(self.base, self.struct, self.n, self.proc)
        if x_0.is_cuda and x_0.dtype == torch.float32 and x_0.is_contiguous() and x_0.device == self.device:
            # device-to-device copy as a KERNEL (captured steps hold kernel nodes only: see msgm_zero_async in csrc/common.h)
            self.x = ops.lincomb(torch.empty_like(x_0), x_0.detach(), 1.0)
        else:
            self.x = x_0.detach().clone().to(self.device).float().contiguous()
        self.norm0 = ops.row_norm(self.x) if norm_correction else None
        self.include_t0 = bool(include_t0)
        self.keep_all = keep_all_samples
        self.keep = None
        self.traj = None
        if keep_all_samples:
            self.traj = torch.zeros((num_steps + int(self.include_t0), self.B, self.n), device=self.device)
            if self.include_t0:
                self.traj[0].copy_(self.x)
        elif samplesToKeep is not None:
            if not (len(samplesToKeep) == self.B):
                raise ValueError('Error: len(samplesToKeep) must correspond to batch size.')
            self.keep = torch.as_tensor(samplesToKeep).reshape(-1).to(torch.int32).to(self.device).contiguous()
            self.kept = torch.zeros((self.B, self.n), device=self.device)
        self.noise = noise
        if noise is not None and tuple(noise.shape) != (num_steps, self.B, self.n):
            raise MsgmError(f"noise must be (num_steps,B,n) = {(num_steps, self.B, self.n)}")
        self.rng = None if noise is not None else self.base.philox(self.device)
        self.T = self.base.T_float()

    def t(self, i):
        return self.ts[i].item()

    def z(self, i):
        return None if self.noise is None else self.noise[i].to(self.device).contiguous()

    def score(self, x, t):
        """a(x, T - t) for the reverse process (SDEs.py:556-557,569); None for the forward one."""
        if not self.reverse:
            return None
        s = torch.full((self.B,), self.T - t, dtype=torch.float32, device=self.device)
        return self.sde.a(x, s).contiguous()

    def clock(self, i, fracs=()):
        """Step i on the host: stage times t_i and the fp32 sums t_i + f delta upstream forms (sde_scheme.py:150,233-247)."""
        t = self.t(i)
        times = [t] + [float(torch.tensor(t, dtype=torch.float32) + self.delta * f) for f in fracs]
        return _Clock(self.struct, self.proc, self.lmbd, self.delta, [dict(t=s) for s in times],
                      dict(z=self.z(i), rng=self.rng, rng_step=i), lambda x, k: self.score(x, times[k]), self.packed)

    def after_step(self, i):
        if self.keep_all:
            self.traj[i + int(self.include_t0)].copy_(self.x)
        elif self.keep is not None:
            ops.keep_rows(self.kept, self.x, self.keep, i + int(self.include_t0))

    def mlp_loop(self, method):
        """The whole loop as ONE launch when the shapes allow it: the reverse process of the MLP, Philox noise, and a shape
        one of the three kernels takes — ``msgm_mlp_sde_loop`` (``ops.mlp_sde_loop_supported``: d <= 30 and in_dim <= 32, dense
        tensors up to n = 16, B > 32), tried first, then ``msgm_mlp_xw_sde_loop`` (``ops.mlp_xw_sde_loop_preferred``: the part
        of the extra-wide class where the loop was measured faster than the composed steps — SGM up to d = 64, the sparse
        tensor up to d = 40, B > 32), then ``msgm_mlp_dense_sde_loop`` (``ops.mlp_dense_sde_loop_preferred``: dense tensors
        with 17 <= n <= 30, in_dim <= 32 and B > 64, where measured faster; its contraction runs on the matrix cores, so it
        agrees with the composed steps to float64 parity, not to the bit).  Same time grid, stage times and Philox draws as
        the composed steps; trajectory rows and kept rows are written by the kernel.  Returns whether it ran; everything
        else — dense n >= 31, dense B <= 64, ``noise=`` — keeps the composed route, whose dense stage at 31 <= n <= 64 is
        ``msgm_sde_stage_dense_mm`` (``_Clock.stage``)."""
        from .NN import MLP
        net = self.sde.a if self.reverse else None
        if not isinstance(net, MLP) or self.noise is not None or net.input_dim != self.n:
            return False
        shape = (self.n, net.pre is not None, self.struct.kind, self.n, self.B)
        if ops.mlp_sde_loop_supported(*shape):
            loop = ops.mlp_sde_loop
        elif ops.mlp_xw_sde_loop_preferred(*shape):
            loop = ops.mlp_xw_sde_loop
        elif ops.mlp_dense_sde_loop_preferred(*shape):
            def loop(*a, **k):
                return ops.mlp_dense_sde_loop(*a, packed=self.base.packed_G(), **k)
        else:
            return False
        loop(net.kernel_params(), self.x, self.struct, method, self.ts.to(self.device), self.delta, self.lmbd,
             rng=self.rng, rng_step0=0, norm0=self.norm0, traj=self.traj, include_t0=self.include_t0,
             keep=self.keep, kept=self.kept if self.keep is not None else None)
        return True

    def result(self, advance=True):
        if self.rng is not None and advance:
            self.rng.advance(self.N)
        if self.keep_all:
            return self.traj.to('cpu')                                        # (N[+1],B,n)  sde_scheme.py:94-95
        if self.keep is not None:
            return self.kept.to('cpu')
        return self.x.to('cpu')


@torch.no_grad()
def euler_maruyama_sampler(sde, x_0, num_steps=1000, lmbd=0., keep_all_samples=True, samplesToKeep=None,
                           include_t0=False, T_=-1, norm_correction=False, noise=None):
    """Euler–Maruyama (sde_scheme.py:43-99)."""
    return _em(sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_, norm_correction,
               noise).result()


def _em(sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_, norm_correction, noise):
    from .NN import MLP
    r = _Run(sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_, norm_correction, noise)
    fused = r.reverse and isinstance(sde.a, MLP) and r.base.kind == L.SDE_SGM and not norm_correction
    P = sde.a.kernel_params() if fused else None
    if fused and not r.keep_all and r.keep is None and noise is None and r.x.shape[0] > 32:
        # final state only: the whole loop in ONE launch, same time grid and Philox draws as the per-step kernels
        ops.mlp_em_loop(P, r.x, r.struct, r.ts.to(r.device), r.delta, r.lmbd, r.rng, 0)
        return r
    if r.base.kind != L.SDE_SGM and r.mlp_loop("em"):     # the multiplicative SDEs: every stage of every step in one launch
        return r
    other = torch.empty_like(r.x)
    for i in range(num_steps):
        if fused:                     # score net + update in ONE kernel
            ops.mlp_em_step(P, r.x, r.struct, r.t(i), r.delta, r.lmbd, z=r.z(i), rng=r.rng, rng_step=i)
        else:
            new = _em_step(r.clock(i), r.x, other, r.norm0)
            if new is other:
                r.x, other = other, r.x
        r.after_step(i)
    return r


def _integrate(step, fracs, nbuf, sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_, norm_correction,
               noise, loop=None):
    """The eager Heun / RK4 loop: the step's new state (its last buffer) swaps places with the state.  ``loop`` names the
    method of the one-launch MLP route (``_Run.mlp_loop``), tried first; None keeps the composed steps."""
    r = _Run(sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_, norm_correction, noise)
    if loop is not None and r.mlp_loop(loop):
        return r
    bufs = [torch.empty_like(r.x) for _ in range(nbuf)]
    for i in range(num_steps):
        step(r.clock(i, fracs), r.x, bufs, r.norm0)
        r.x, bufs[-1] = bufs[-1], r.x
        r.after_step(i)
    return r


@torch.no_grad()
def heun_sampler(sde, x_0, num_steps=1000, lmbd=0., keep_all_samples=True, samplesToKeep=None,
                 include_t0=False, T_=-1, norm_correction=False, noise=None):
    """Heun / RK2 in Stratonovich form (sde_scheme.py:101-172):
    x <- x + 1/2 (K1 + K2), K = mu_Strato*delta + sigma.dW, one shared dW."""
    return _integrate(_heun_step, (1.0,), 4, sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_,
                      norm_correction, noise, loop="heun").result()


@torch.no_grad()
def heun_composed(sde, x_0, num_steps=1000, lmbd=0., keep_all_samples=True, samplesToKeep=None,
                  include_t0=False, T_=-1, norm_correction=False, noise=None):
    """heun_sampler on the composed route (score net, stage kernel and glue as separate launches), whatever the shape:
    the yardstick of the one-launch loop."""
    return _integrate(_heun_step, (1.0,), 4, sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_,
                      norm_correction, noise).result()


@torch.no_grad()
def rk4_stratonovich_sampler(sde, x_0, num_steps=1000, lmbd=0., keep_all_samples=True, samplesToKeep=None,
                             include_t0=False, T_=-1, norm_correction=False, noise=None):
    """RK4 for Stratonovich SDEs, one dW per step (sde_scheme.py:174-269)."""
    return _rk4(sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_, norm_correction,
                noise, loop="rk4").result()


@torch.no_grad()
def rk4_stratonovich_composed(sde, x_0, num_steps=1000, lmbd=0., keep_all_samples=True, samplesToKeep=None,
                              include_t0=False, T_=-1, norm_correction=False, noise=None):
    """rk4_stratonovich_sampler on the composed route, whatever the shape: the yardstick of the one-launch loop."""
    return _rk4(sde, x_0, num_steps, lmbd, keep_all_samples, samplesToKeep, include_t0, T_, norm_correction, noise).result()


def _rk4(*args, loop=None):
    return _integrate(_rk4_step, (0.5, 1.0), 7, *args, loop=loop)


def _forward_grid(base, nsf, dev):
    """The forward time grid linspace(0,1,nsf+1)*T (fp32, formed on the host as ``_Run`` does) on the device, cached on the
    base SDE per (nsf, T, device): the trainers capture ``msgm_forward_perturb`` into a hipGraph that holds kernel nodes
    only, so the copy to the device happens on first use — their eager warm-up step — and never during a capture."""
    cache = getattr(base, "_forward_ts", None)
    if cache is None:
        cache = base._forward_ts = {}
    T_ = base.T_float()
    key = (int(nsf), T_, dev)
    if key not in cache:
        if torch.cuda.is_current_stream_capturing():
            raise MsgmError("the forward time grid is needed for the first time inside a graph capture; "
                            "run one eager step first")
        cache[key] = ((torch.linspace(0, 1, nsf + 1) * T_).to(dev), T_ / nsf)
    return cache[key]


@torch.no_grad()
def msgm_forward_perturb(base, t, y0, noise_main=None, noise_short=None):
    """y_t | y_0 for the multiplicative SDE (SDE.sample_scheme, SDEs.py:78-122) in ONE launch
    (``msgm_forward_perturb``) where ``ops.forward_perturb_supported`` takes the row length: row b takes exactly its
    k_b = trunc(nsf t_b / T) RK4 steps — or the one step of length t_b when k_b = 0 — with the state in registers, and
    is stored once.  Same time grid, stage times and noise (``noise_main`` / ``noise_short`` or the Philox draws) as
    ``msgm_forward_perturb_composed``, which every other shape takes; the result is the same bit for bit.  Both routes
    advance the stream by 2 nsf + 2."""
    st = base.struct()
    if y0.dim() != 2 or not y0.is_cuda or not ops.forward_perturb_supported(st.kind, y0.shape[1]):
        return msgm_forward_perturb_composed(base, t, y0, noise_main, noise_short)
    dev = y0.device
    nsf = base.num_steps_forward
    x = y0.detach().contiguous().float()
    zm = None if noise_main is None else noise_main.to(dev).contiguous()
    zs = None if noise_short is None else noise_short.to(dev).contiguous()
    if any(v is not None and v.data_ptr() % 16 for v in (x, zm, zs)):
        # views that are only 4-byte aligned: the long-row form of the kernel does not take them
        return msgm_forward_perturb_composed(base, t, y0, noise_main, noise_short)
    ts, delta = _forward_grid(base, nsf, dev)
    rng = base.philox(dev)
    y = ops.forward_perturb(x, t.reshape(-1).contiguous().float(), st, nsf, ts, delta,
                            z_main=zm, z_short=zs, rng=None if (zm is not None and zs is not None) else rng)
    rng.advance(2 * nsf + 2)
    return y


@torch.no_grad()
def msgm_forward_perturb_composed(base, t, y0, noise_main=None, noise_short=None):
    """msgm_forward_perturb on the composed route (index kernel, nsf RK4 steps of stage, combine and masked-capture
    launches, then the short step), whatever the shape: the yardstick of the one-launch kernel.  All rows are
    RK4-integrated over the nsf-step grid and row b is captured when the step count reaches k_b = trunc(nsf t_b / T)
    (bit-exact int32 index kernel); rows with k_b = 0 take one RK4 step of length t_b from y_0 (per-row delta inside
    the stage kernel) — no Python loop over rows, no D2H/H2D round trips."""
    from .SDEs import forward_SDE
    dev = y0.device
    nsf = base.num_steps_forward
    tt = t.reshape(-1).contiguous().float()
    k = ops.forward_step_index(tt, nsf, base.T_float())
    fwd = forward_SDE(base, base.T)
    kept = _rk4(fwd, y0, nsf, 0., False, k, True, -1, False, noise_main).kept
    # rows with k == 0: one RK4 step, delta_b = t_b, stage times 0, t_b/2, t_b/2, t_b
    x = y0.contiguous().float()
    bufs = [torch.empty_like(x) for _ in range(7)]
    rng = None if noise_short is not None else base.philox(dev)
    z = None if noise_short is None else noise_short.to(dev).contiguous()
    c = _Clock(base.struct(), L.PROC_FORWARD, 0.0, 0.0, [dict(t=0.0, delta_rows=tt, t_frac=f) for f in (0.0, 0.5, 1.0)],
               dict(z=z, rng=rng, rng_step=nsf + 1), lambda xx, kk: None)
    ops.keep_rows(kept, _rk4_step(c, x, bufs, None), k, 0)
    base.philox(dev).advance(2 * nsf + 2)
    return kept


@torch.no_grad()
def msgm_forward_paths(base, y0, first_keep=0, noise=None):
    """The grid states y_{t_{first_keep+1}}, ..., y_{t_nsf} of ONE forward path per row, (nsf - first_keep, B, n) on the
    device: SDE.sample_scheme_allt(y0, include_t0=False)[first_keep:] as the integrated SSM loss uses it
    (``PluginReverseSDE(ssm_intT=True)``, SDEs.py:648-706).  ONE launch (``msgm_forward_paths``) where
    ``ops.forward_perturb_supported`` takes the row length and the operands are 16-byte aligned: a row lives in registers
    through all nsf RK4 steps and is stored after every kept one.  Every other shape, and the additive SDE, takes
    ``msgm_forward_paths_composed``; the result is the same bit for bit.  ``noise`` (nsf,B,n) injects the standard normals;
    without it both routes draw from the base SDE's Philox stream and advance it by nsf, as the composed sampler does."""
    st = base.struct()
    nsf = base.num_steps_forward
    if not 0 <= int(first_keep) < nsf:
        raise MsgmError(f"first_keep = {first_keep} keeps no state of the {nsf}-step forward grid")
    if y0.dim() != 2 or not y0.is_cuda or not ops.forward_perturb_supported(st.kind, y0.shape[1]):
        return msgm_forward_paths_composed(base, y0, first_keep, noise)
    dev = y0.device
    x = y0.detach().contiguous().float()
    zm = None if noise is None else noise.to(dev).contiguous()
    if any(v is not None and v.data_ptr() % 16 for v in (x, zm)):
        return msgm_forward_paths_composed(base, y0, first_keep, noise)
    ts, delta = _forward_grid(base, nsf, dev)
    rng = None if zm is not None else base.philox(dev)
    y_all = ops.forward_paths(x, st, nsf, first_keep, ts, delta, z_main=zm, rng=rng)
    if rng is not None:
        rng.advance(nsf)
    return y_all


@torch.no_grad()
def msgm_forward_paths_composed(base, y0, first_keep=0, noise=None):
    """msgm_forward_paths on the composed route (nsf RK4 steps of four stage launches, a combine and a trajectory copy
    each), whatever the shape or SDE: the yardstick of the one-launch kernel.  The trajectory stays on the device."""
    from .SDEs import forward_SDE
    nsf = base.num_steps_forward
    if not 0 <= int(first_keep) < nsf:
        raise MsgmError(f"first_keep = {first_keep} keeps no state of the {nsf}-step forward grid")
    r = _rk4(forward_SDE(base, base.T), y0, nsf, 0., True, None, False, -1, False, noise)
    if r.rng is not None:
        r.rng.advance(nsf)                           # what _Run.result does
    return r.traj[int(first_keep):]


class GraphedEMSampler:
    """The whole fused EM loop (MLP + SGM) captured as ONE hipGraph: N kernel
    nodes with the time grid and Philox step index baked in by value; the state
    buffer and the Philox state live at fixed device addresses, so a replay is a
    single host call.  (hipGraph instead of a tracing compiler.)"""

    def __init__(self, sde, B, num_steps, lmbd=0.0, T_=None):
        from .NN import MLP
        if not (isinstance(sde.a, MLP) and sde.base_sde.kind == L.SDE_SGM):
            raise MsgmError("GraphedEMSampler is built for MLP + SGMsde")
        self.sde, self.N = sde, num_steps
        dev = sde.T.device
        base = sde.base_sde
        self.T_ = base.T_float() if T_ is None else float(T_)
        self.x = torch.zeros(B, sde.a.input_dim, device=dev)
        self.rng = base.philox(dev)
        P = sde.a.kernel_params()
        st = base.struct()
        ts = torch.linspace(0, 1, num_steps + 1) * self.T_
        delta = self.T_ / num_steps
        self.ts_dev = ts.to(dev)
        self._keep = (P, st)
        # B > 32: the whole loop is ONE launch (msgm_mlp_em_loop — rows never interact, so a workgroup carries its rows
        # through all steps); otherwise N single-step kernel nodes.  Same Philox numbers either way.
        one_launch = B > 32

        def body():
            if one_launch:
                ops.mlp_em_loop(P, self.x, st, self.ts_dev, delta, lmbd, self.rng, 0)
            else:
                for i in range(num_steps):
                    ops.mlp_em_step(P, self.x, st, ts[i].item(), delta, lmbd, rng=self.rng, rng_step=i)
            self.rng.advance(num_steps)

        self.graph = _capture(body, dev)

    @torch.no_grad()
    def run(self, x_0):
        self.x.copy_(x_0)
        self.graph.replay()
        return self.x


class GraphedStepSampler:
    """Euler-Maruyama, Heun or RK4-Stratonovich with ANY HIP score net (U-Nets): ONE step — device clock ticks, the
    score-net forward(s) (hundreds of kernels each), the fused stage kernels, step-counter bump — is captured as a
    hipGraph and replayed num_steps times.  The time grid (fp32 ``linspace`` as upstream, sde_scheme.py:59), the stage
    times t + delta/2, t + delta (fp32 adds as upstream, sde_scheme.py:150,233-247) and the step index live on the
    device, so the replays need no host scalar (the reference does ``ts[i].item()`` + ``fill_`` every step,
    sde_scheme.py:81).  ``method='rk4'`` is what the driver generates with (MSGM_higherDim.py:903).  Only kernel nodes
    are captured (no D2D memcpy / memset nodes — see msgm_zero_async in csrc/common.h)."""

    # method -> (the step, the stage times after t as fractions of delta, stage buffers; em: ``other``, multiplicative SDEs only)
    METHODS = {"em": (_em_step, (), 1), "heun": (_heun_step, (1.0,), 4), "rk4": (_rk4_step, (0.5, 1.0), 7)}

    def __init__(self, sde, B, n, num_steps, lmbd=0.0, norm_correction=False, method="em"):
        from .SDEs import PluginReverseSDE
        if not isinstance(sde, PluginReverseSDE):
            raise MsgmError("GraphedStepSampler integrates a PluginReverseSDE")
        if method not in self.METHODS:
            raise MsgmError(f"unknown integrator {method}")
        base = sde.base_sde
        dev = sde.T.device
        self.sde, self.N, self.B, self.n, self.method = sde, num_steps, B, n, method
        T = base.T_float()
        self.ts = (torch.linspace(0, 1, num_steps + 1) * T).to(dev)
        self.step = torch.zeros(1, dtype=torch.int64, device=dev)
        step, fracs, nbuf = self.METHODS[method]
        self.t_dev = [torch.zeros(1, device=dev) for _ in range(1 + len(fracs))]      # distinct stage times
        self.s = [torch.zeros(B, device=dev) for _ in self.t_dev]
        self.x = torch.zeros(B, n, device=dev)
        self.norm0 = torch.zeros(B, device=dev) if norm_correction else None
        self.rng = base.philox(dev)
        st, delta = base.struct(), T / num_steps
        self._keep = st
        if method == "em":
            bufs = None if base.kind == L.SDE_SGM else torch.zeros(B, n, device=dev)
        else:
            bufs = [torch.zeros(B, n, device=dev) for _ in range(nbuf)]
        # the fp32 value upstream adds to the fp32 t; 0.0 (no add) for the step's own time
        t_add = [0.0] + [float(torch.tensor(delta * f, dtype=torch.float32)) for f in fracs]
        clock = _Clock(st, L.PROC_REVERSE, lmbd, delta, [dict(t=0.0, t_dev=td) for td in self.t_dev],
                       dict(rng=self.rng, step_dev=self.step), lambda xx, k: sde.a(xx, self.s[k]).contiguous(),
                       _stage_image(base, st, n, L.PROC_REVERSE))

        def body():
            for td, s, add in zip(self.t_dev, self.s, t_add):
                ops.time_tick(self.ts, self.step, T, td, s, t_add=add)
            new = step(clock, self.x, bufs, self.norm0)
            if new is not self.x:
                ops.lincomb(self.x, new, 1.0)
            ops.counter_inc(self.step)

        # the captured graph holds raw pointers only: the stage buffers live as long as this closure
        self._body = body
        self.graph = _capture(body, dev)

    @torch.no_grad()
    def run(self, x_0):
        ops.lincomb(self.x, x_0.contiguous().float().view(self.B, self.n), 1.0)
        if self.norm0 is not None:
            ops.lincomb(self.norm0, ops.row_norm(self.x), 1.0)
        self.step.zero_()
        for _ in range(self.N):
            self.graph.replay()
        self.rng.advance(self.N)
        return self.x
