"""Fused Adam on flat parameter buckets (K13) — drop-in for the reference's
``torch.optim.Adam(gen_sde.parameters(), lr=lr)`` (MSGM_higherDim.py:792).

Parameters that are consecutive views of one flat buffer (what
``FlatParamMixin`` produces) are updated by ONE kernel launch per step; the
state is exposed per parameter as ``step / exp_avg / exp_avg_sq`` so
``state_dict()`` is wire-compatible with ``torch.optim.Adam`` checkpoints
(NN.py:13-42).  The step counter lives on the device so a captured hipGraph can
replay the update.

``lr`` (like betas and eps) is read from the param group on EVERY eager step, so torch's ``lr_scheduler`` classes work
with this optimizer as they do with ``torch.optim.Adam``.

``max_grad_norm`` / ``ema_rate`` (csrc/optim_kernels.hip) fold ``torch.nn.utils.clip_grad_norm_`` and the reference's
``update_ema`` (model/nn_utils.py:117-127) into the update: the norm is GLOBAL over all runs (each run writes its float64
partial sums into its slice of one buffer, every run's update reads the whole buffer), ``opt.grad_norm`` is a device
scalar holding the pre-clip norm of the last step, ``opt.ema_state_dict()`` maps a parameter's index to its average.
Both need every run's gradients in one contiguous buffer (what ``FlatParamMixin`` nets have): MsgmError otherwise.

``weight_decay`` is a param-group default read from the group on every step like ``lr`` (a no-decay group for biases
works); ``decoupled_weight_decay`` (default True) chooses ``torch.optim.AdamW``'s form over
``torch.optim.Adam(weight_decay)``'s.  ``skip_nonfinite`` leaves every run untouched when the global gradient norm is
not finite, decided on the device (``opt.skipped_steps`` syncs; per-parameter ``state["step"]`` then is a device scalar
holding the effective count).  ``ema_warmup`` ramps the rate as min(rate, (1 + k) / (10 + k)).  Any of the three runs the
update through ``msgm_optim_step`` and needs contiguous gradients too.
"""
from __future__ import annotations

from typing import List

import torch

from . import ops
from ._lib import MsgmError


class _Run:
    __slots__ = ("params", "numel", "m", "v", "group", "hyper", "hyper_host", "ema", "poff", "pnum")

    def __init__(self, params, group):
        self.params: List[torch.nn.Parameter] = params
        self.group = group                     # the param_group whose lr / betas / eps this run is updated with
        self.numel = sum(p.numel() for p in params)
        dev = params[0].device
        self.m = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.v = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.hyper = self.hyper_host = self.ema = None     # the option route: device hyper-parameters, their host copy, EMA
        self.poff = self.pnum = 0                          # this run's slice of the shared partials buffer


def _flat_view(first: torch.Tensor, numel: int) -> torch.Tensor:
    return first.as_strided((numel,), (1,), first.storage_offset())


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale: float = 1.0, max_grad_norm=None,
                 ema_rate=None, weight_decay: float = 0.0, decoupled_weight_decay: bool = True,
                 skip_nonfinite: bool = False, ema_warmup: bool = False):
        if not float(weight_decay) >= 0.0:
            raise MsgmError(f"weight_decay must be >= 0 (got {weight_decay})")
        if ema_warmup and ema_rate is None:
            raise MsgmError("ema_warmup=True needs ema_rate=...: there is no average to warm up")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.grad_scale = grad_scale          # 1/world_size after a sum all-reduce
        self.max_grad_norm, self.ema_rate = max_grad_norm, ema_rate
        self.decoupled_weight_decay, self.skip_nonfinite = bool(decoupled_weight_decay), bool(skip_nonfinite)
        self.ema_warmup = bool(ema_warmup)
        self._ex = None                       # the update goes through msgm_optim_step (fixed at the first step)
        self._skipped = None                  # skip_nonfinite: the two-slot device count of skipped steps
        self.grad_norm = None                 # device scalar: pre-clip global norm of the last step (max_grad_norm set)
        self._partials = None
        self._runs = None
        self._step_dev = None
        self._step_host = 0

    def _build_runs(self):
        runs = []
        for group in self.param_groups:        # a run never spans two groups: each keeps its own hyper-parameters
            cur = []
            for p in group["params"]:
                if not p.requires_grad:
                    continue      # e.g. the horizon T, an nn.Parameter(requires_grad=False) upstream
                if cur and p.data_ptr() == cur[-1].data_ptr() + cur[-1].numel() * 4 and p.device == cur[-1].device:
                    cur.append(p)
                else:
                    if cur:
                        runs.append(_Run(cur, group))
                    cur = [p]
            if cur:
                runs.append(_Run(cur, group))
        if not runs:
            raise ValueError("FusedAdam got no trainable parameters")
        self._runs = runs
        dev = runs[0].params[0].device
        self._step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        if self._options():
            if any(r.params[0].device != dev for r in runs):
                raise MsgmError("FusedAdam(max_grad_norm / ema_rate): all parameters must live on one device")
            self._ex = self._wants_ex()
            if self.skip_nonfinite:
                self._skipped = ops.skipped_counter(dev)
            if self.max_grad_norm is not None or self.skip_nonfinite:       # the guard reads the norm too
                off = 0
                for r in runs:
                    r.poff, r.pnum = off, ops.grad_sqnorm_partials(r.numel)
                    off += r.pnum
                self._partials = torch.zeros(off, dtype=torch.float64, device=dev)
                self.grad_norm = torch.zeros((), dtype=torch.float32, device=dev)
            if self.ema_rate is not None:
                for r in runs:
                    r.ema = _flat_view(r.params[0].data, r.numel).detach().clone()      # seeded from the parameters
        for r in runs:
            off = 0
            for p in r.params:
                k = p.numel()
                self.state[p] = {"step": torch.tensor(float(self._step_host)),
                                 "exp_avg": r.m[off:off + k].view(p.shape),
                                 "exp_avg_sq": r.v[off:off + k].view(p.shape)}
                off += k

    def _wants_ex(self) -> bool:
        return self.skip_nonfinite or self.ema_warmup or any(g.get("weight_decay", 0) != 0 for g in self.param_groups)

    def _options(self) -> bool:
        return self.max_grad_norm is not None or self.ema_rate is not None or self._wants_ex()

    @property
    def skipped_steps(self) -> int:
        """Steps the non-finite guard skipped so far (an int; reading it synchronises).  0 without ``skip_nonfinite``."""
        return 0 if self._skipped is None else ops.skipped_count(self._skipped, self._step_dev)

    @staticmethod
    def _contiguous_grads(r) -> bool:
        p0 = r.params[0]
        if p0.grad is None:
            return False
        ptr = p0.grad.data_ptr()
        for p in r.params:
            if p.grad is None or p.grad.data_ptr() != ptr or not p.grad.is_contiguous():
                return False
            ptr += p.numel() * 4
        return True

    def _prepare_options(self):
        """Before anything is launched: refuse scattered gradients, write the groups' hyper-parameters where they changed."""
        for r in self._runs:
            if not self._contiguous_grads(r):
                raise MsgmError("FusedAdam(max_grad_norm / ema_rate) needs each run's gradients in one contiguous buffer "
                                "(a FlatParamMixin net); this run's .grad tensors are scattered or missing")
            g = r.group
            vals = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], self.max_grad_norm, self.ema_rate)
            if self._ex:
                if not g.get("weight_decay", 0) >= 0:
                    raise MsgmError(f"weight_decay must be >= 0 (got {g['weight_decay']})")
                vals += (g.get("weight_decay", 0),)
            elif g.get("weight_decay", 0) != 0:
                raise MsgmError("a param group gained a weight_decay after the first step of a FusedAdam built without "
                                "one; pass weight_decay= at construction")
            if vals != r.hyper_host:           # read from the group on every step; written when it changed (a scheduler)
                h = (ops.optim_hyper if self._ex else ops.opt_hyper)("cpu", vals[0], vals[1:3], vals[3], *vals[4:])
                if r.hyper is None:
                    r.hyper = h.to(r.m.device)
                else:
                    r.hyper.copy_(h)
                r.hyper_host = vals

    def _step_options(self):
        """[grad_sqnorm per run into its slice of the partials] -> adam_step_ex per run, reading ALL partials."""
        if self._partials is not None:
            for r in self._runs:
                ops.grad_sqnorm(_flat_view(r.params[0].grad, r.numel), self.grad_scale,
                                self._partials[r.poff:r.poff + r.pnum])
        for r in self._runs:
            p0 = r.params[0]
            if not self._ex:
                ops.adam_step_ex(_flat_view(p0.data, r.numel), _flat_view(p0.grad, r.numel), r.m, r.v, r.hyper,
                                 self._step_dev, ema=r.ema, gscale=self.grad_scale, partials=self._partials,
                                 grad_norm_out=self.grad_norm)
                continue
            mode = (ops.DECAY_NONE if r.group.get("weight_decay", 0) == 0 else
                    ops.DECAY_DECOUPLED if self.decoupled_weight_decay else ops.DECAY_L2)
            ops.optim_step(_flat_view(p0.data, r.numel), _flat_view(p0.grad, r.numel), r.m, r.v, r.hyper, self._step_dev,
                           ema=r.ema, gscale=self.grad_scale, partials=self._partials, grad_norm_out=self.grad_norm,
                           clip=self.max_grad_norm is not None, decay_mode=mode, skipped=self._skipped,
                           ema_warmup=self.ema_warmup)

    def ema_state_dict(self) -> dict:
        """{index of the parameter in state_dict()'s numbering: its averaged tensor} (ema_rate set, after the first step
        or load_state_dict)."""
        if self.ema_rate is None:
            raise MsgmError("ema_state_dict() needs FusedAdam(ema_rate=...)")
        if self._runs is None:
            self._build_runs()
        index = {id(p): i for i, p in enumerate(q for g in self.param_groups for q in g["params"])}
        out = {}
        for r in self._runs:
            off = 0
            for p in r.params:
                out[index[id(p)]] = r.ema[off:off + p.numel()].view(p.shape).clone()
                off += p.numel()
        return out

    @torch.no_grad()
    def step(self, closure=None):
        if self._runs is None:
            self._build_runs()
        if self._options():
            self._prepare_options()
        ops.counter_inc(self._step_dev)
        self._step_host += 1
        if self._options():
            self._step_options()
            if self._skipped is None:
                eff = None
            else:                              # the effective count, formed on the device: no sync in step()
                eff = (self._step_dev[0] - self._skipped[(self._step_host + 1) & 1]).float()
            for r in self._runs:
                for p in r.params:
                    self.state[p]["step"] = torch.tensor(float(self._step_host)) if eff is None else eff
            return None
        for r in self._runs:
            g = r.group
            lr, (b1, b2), eps = g["lr"], g["betas"], g["eps"]
            p0 = r.params[0]
            if self._contiguous_grads(r):
                ops.adam_step(_flat_view(p0.data, r.numel), _flat_view(p0.grad, r.numel), r.m, r.v, step=0, lr=lr,
                              beta1=b1, beta2=b2, eps=eps, gscale=self.grad_scale, step_dev=self._step_dev)
            else:
                off = 0
                for p in r.params:
                    k = p.numel()
                    if p.grad is not None:
                        ops.adam_step(p.data.view(-1), p.grad.contiguous().view(-1), r.m[off:off + k], r.v[off:off + k],
                                      step=0, lr=lr, beta1=b1, beta2=b2, eps=eps, gscale=self.grad_scale,
                                      step_dev=self._step_dev)
                    off += k
            for p in r.params:
                self.state[p]["step"] = torch.tensor(float(self._step_host))
        return None

    def state_dict(self):
        sd = super().state_dict()
        if self.skip_nonfinite:                # torch's loader ignores the key
            sd["skipped"] = self.skipped_steps if self._runs is not None else 0
        return sd

    def load_state_dict(self, state_dict):
        if self._runs is None:
            self._build_runs()
        views = {p: (self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]) for r in self._runs for p in r.params}
        super().load_state_dict(state_dict)
        step = 0
        for p, (m, v) in views.items():
            st = self.state[p]
            if "exp_avg" not in st:            # checkpoint of a never-stepped optimizer: empty state
                m.zero_(); v.zero_()
                st["step"] = torch.tensor(0.0)
            else:
                m.copy_(st["exp_avg"]); v.copy_(st["exp_avg_sq"])
                step = int(float(st["step"]))
            st["exp_avg"], st["exp_avg_sq"] = m, v
        if self._skipped is not None:          # "step" is the effective count; the device counter counts attempts
            skipped = int(state_dict.get("skipped", 0))
            step += skipped
            self._skipped.fill_(skipped)
        self._step_host = step
        self._step_dev.fill_(step)
        if self.ema_rate is not None and "ema" in state_dict:      # a trainer's checkpoint carries its average under "ema"
            index = {id(p): i for i, p in enumerate(q for g in self.param_groups for q in g["params"])}
            for r in self._runs:
                off = 0
                for p in r.params:
                    r.ema[off:off + p.numel()].copy_(state_dict["ema"][index[id(p)]].reshape(-1))
                    off += p.numel()
