"""The score-matching training step as the build runs it (replaces the loop
body MSGM_higherDim.py:803-809): perturb (K1) -> probe -> fused
forward/tangent/loss/backward (K5) -> [RCCL all-reduce of the flat gradient
bucket] -> fused Adam (K13).  Everything is enqueued on one stream with no
host synchronisation, so a step can be captured once and replayed as a hipGraph
(single-GPU) — the Philox offset and the Adam step count live on the device.

Both trainers expose ``state_dict()`` / ``load_state_dict()`` in the layout of ``torch.optim.Adam`` (``state`` =
{index: step / exp_avg / exp_avg_sq}, ``param_groups``) plus a ``philox`` entry, so the fast path goes through
``NN.save_checkpoint`` / ``load_checkpoint`` like the reference loop does (MSGM_higherDim.py:794-826, NN.py:13-42)
and a resumed run continues the SAME noise stream.

Optimizer stage (keyword-only, all off by default; csrc/optim_kernels.hip): ``max_grad_norm`` (global-norm
clipping on a deterministic device norm, ``tr.grad_norm``), ``ema_rate`` (``tr.ema``, ``ema_state_dict()``,
``with tr.ema_weights():``, an ``"ema"`` entry in the checkpoint), ``lr_schedule`` (k -> lr, e.g. ``warmup_cosine``) and
``device_lr`` (``set_lr`` between replays); any of the first three implies the last.  A trainer built without them runs
the launches it always ran, with the learning rate baked into the captured step.  ``weight_decay`` (with
``decoupled_weight_decay``: AdamW, the default, or Adam's L2 form), ``skip_nonfinite`` (a step whose gradient norm is
not finite changes nothing, decided on the device; ``tr.skipped_steps``, a ``"skipped"`` entry in the checkpoint) and
``ema_warmup`` also imply ``device_lr`` and run the update through ``msgm_optim_step``.

Data stage (keyword-only ``data=sampler``, off by default; csrc/data_kernels.hip): every step begins by
drawing ``x`` on the device from the trainer's own Philox stream — a fresh minibatch per replay, no host work.  An
``ArrayData`` under the additive SDE rides in the prep launch (msgm_ssm_prep_gather: the launch count of a fixed-batch
step); every other combination is ``sampler.sample_into(tr.x, tr.rng)`` ahead of the existing path.  ``tr.x`` shows the
batch that was trained on.  The stream advances per step as before, so checkpoints keep their keys and a resumed run
draws the batches of the uninterrupted one; indices and draws are keyed by global row / element, so an N-rank run
(every rank holding the whole table) trains on the rows of the 1-rank run.  ``ArrayData(..., replace=False)`` draws epochs
without replacement instead: gather at the sampler's device cursor, then cursor += B_local * world in a launch of its own
(two kernel nodes more than the fixed-batch step, the fused prologue is not used), and the checkpoint gains
``"data_cursor"``.  Epochs across ranks need the same seed on every rank and ``row_base`` = the shard's first global row.

Integrated loss (``gen_sde.ssm_intT``, multiplicative SDE, one rank): ``x`` stays (B, d) and a step trains on
the nsf' B kept grid states of B forward paths — [data stage] -> msgm_forward_paths (one launch) -> probe -> msgm_ssm_terms
-> the fused pass -> reduce and optimizer stage as above.  ``tr.rows`` = nsf' B sizes y, t (the resident tiled grid), v,
u, cst and the row-weight buffer, and ``inv_batch`` = 1 / rows.  The stream advances by nsf + 1 per step, at the positions
eager ``ssm()`` uses.  Refused at construction: the additive SDE, ``world > 1``, a row length the path kernel does not take.
"""
from __future__ import annotations

import contextlib
import math
from typing import Callable, Optional

import torch

from . import _lib as L
from . import ops
from . import parallel
from ._lib import MsgmError


class _TrainerState:
    """Checkpoint surface shared by the trainers (Adam layout of torch.optim.Adam + the device Philox state).

    The reference builds its optimizer over ``gen_sde.parameters()`` (MSGM_higherDim.py:792,899-900): index 0 of that
    list is the non-trainable horizon ``T`` (an nn.Parameter(requires_grad=False), MSGM_higherDim.py:728), the score
    net's tensors follow.  The trainers write / read their Adam state under THOSE indices (``T`` gets a slot in
    ``param_groups[0]['params']`` and no state, exactly as torch.optim.Adam leaves it), so a trainer checkpoint loads
    into ``torch.optim.Adam(gen_sde.parameters())`` / ``FusedAdam`` and vice versa."""

    def _param_index(self):
        """(all parameters of gen_sde in optimizer order, [(index, flat offset, parameter)] of the net's tensors)."""
        offs, off = {}, 0
        for p in self.net.parameters():
            offs[id(p)] = off
            off += p.numel()
        allp = list(self.gen_sde.parameters())
        mine = [(i, offs[id(p)], p) for i, p in enumerate(allp) if id(p) in offs]
        if len(mine) != len(offs):
            raise MsgmError("the score net's parameters are not all reachable from gen_sde.parameters()")
        return allp, mine

    def state_dict(self) -> dict:
        # "step" is the EFFECTIVE count (attempts - skipped steps): what torch.optim.Adam / AdamW would hold
        skipped = self.skipped_steps
        step = float(self.step_dev.item() - skipped)
        allp, mine = self._param_index()
        st = {}
        if step > 0:                              # a never-stepped torch.optim.Adam has an empty state too
            for i, off, p in mine:
                k = p.numel()
                st[i] = {"step": torch.tensor(step), "exp_avg": self.m[off:off + k].view(p.shape).clone(),
                         "exp_avg_sq": self.v[off:off + k].view(p.shape).clone()}
        group = {"lr": self.lr, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": self.weight_decay or 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": self.decay_mode == ops.DECAY_DECOUPLED, "params": list(range(len(allp)))}
        sd = {"state": st, "param_groups": [group], "philox": self.rng.state_dict()}
        if self.skipped is not None:              # torch's loader ignores the key, as it ignores "ema"
            sd["skipped"] = skipped
        if _epoch_data(self):                     # the stream position of the next batch's first global row
            sd["data_cursor"] = self.data.position
        if self.ema is not None:                  # laid out like "state"; torch.optim.Adam's loader ignores the key
            sd["ema"] = {i: self.ema[off:off + p.numel()].view(p.shape).clone() for i, off, p in mine}
        return sd

    def load_state_dict(self, sd: dict) -> None:
        allp, mine = self._param_index()
        saved = sd["param_groups"][0]["params"] if sd.get("param_groups") else list(range(len(allp)))
        if len(saved) == len(allp):
            shift = 0
        elif len(saved) == len(mine):             # written by a round-2 trainer: net tensors only, indexed from 0
            shift = mine[0][0]
        else:
            raise MsgmError(f"optimizer state has {len(saved)} parameters; gen_sde.parameters() has {len(allp)}")
        step = 0
        for i, off, p in mine:
            k = p.numel()
            e = sd["state"].get(i - shift)
            if e is None:                       # never-stepped checkpoint: empty Adam state
                self.m[off:off + k].zero_(); self.v[off:off + k].zero_()
            else:
                self.m[off:off + k].copy_(e["exp_avg"].reshape(-1)); self.v[off:off + k].copy_(e["exp_avg_sq"].reshape(-1))
                step = int(float(e["step"]))
        skipped = int(sd.get("skipped", 0))     # absent in older checkpoints and in torch's own
        self._k = step + skipped                # lr_schedule(k) continues at the call after the loaded one
        if self.skipped is None:
            self.step_dev.fill_(step)           # no guard: the device counter is the effective count
        else:
            self.step_dev.fill_(step + skipped)         # attempts
            self.skipped.fill_(skipped)
        if sd.get("param_groups"):
            self.set_lr(float(sd["param_groups"][0]["lr"]))
        if self.ema is not None:
            if "ema" in sd:
                for i, off, p in mine:
                    self.ema[off:off + p.numel()].copy_(sd["ema"][i - shift].reshape(-1))
            else:                               # a checkpoint without an average: seed it from the loaded parameters
                self.ema.copy_(self.flat)
        if "philox" in sd:                      # absent in checkpoints written by torch.optim.Adam: keep the stream
            self.rng.load_state_dict(sd["philox"])      # stream position only; the shard base stays this rank's
        if _epoch_data(self):                   # absent: the data order starts over; without an epoch sampler: ignored
            self.data.position = int(sd.get("data_cursor", 0))

    # ------------------------------------------------------------------ optimizer stage (csrc/optim_kernels.hip)
    def _init_optim(self, lr, max_grad_norm, ema_rate, lr_schedule, device_lr, weight_decay=0.0,
                    decoupled_weight_decay=True, skip_nonfinite=False, ema_warmup=False):
        """``device_lr``: lr, betas, eps, max_grad_norm and ema_rate live in six float64 values on the device
        (``ops.opt_hyper``) that ``msgm_adam_step_ex`` reads at every launch, so a captured step takes a new learning
        rate without a re-capture.  Clipping, EMA or a schedule imply it.  All off: today's launches, lr baked in.

        ``weight_decay`` (> 0; ``decoupled_weight_decay`` True = ``torch.optim.AdamW``, False =
        ``torch.optim.Adam(weight_decay)``; over the whole flat bucket, as one torch param group), ``skip_nonfinite``
        and ``ema_warmup`` imply it too and move the update to ``msgm_optim_step`` (seven device values,
        ``ops.optim_hyper``); without them the update stays ``msgm_adam_step_ex``."""
        self.max_grad_norm, self.ema_rate, self.lr_schedule = max_grad_norm, ema_rate, lr_schedule
        self.weight_decay, self.ema_warmup = float(weight_decay), bool(ema_warmup)
        if not self.weight_decay >= 0.0:
            raise MsgmError(f"weight_decay must be >= 0 (got {weight_decay})")
        if self.ema_warmup and ema_rate is None:
            raise MsgmError("ema_warmup=True needs ema_rate=...: there is no average to warm up")
        self.decay_mode = (ops.DECAY_NONE if self.weight_decay == 0.0 else
                           ops.DECAY_DECOUPLED if decoupled_weight_decay else ops.DECAY_L2)
        self._optim_ex = self.decay_mode != ops.DECAY_NONE or bool(skip_nonfinite) or self.ema_warmup
        self.device_lr = (bool(device_lr) or self._optim_ex
                          or any(o is not None for o in (max_grad_norm, ema_rate, lr_schedule)))
        self.lr = float(lr)
        self.hyper = self.partials = self.grad_norm = self.ema = self.skipped = None
        self._k, self._in_ema = 0, False          # host count of the step() calls made; inside ema_weights()
        if not self.device_lr:
            return
        if self._optim_ex:
            self.hyper = ops.optim_hyper(self.dev, lr, (0.9, 0.999), 1e-8, max_grad_norm, ema_rate, self.weight_decay)
        else:
            self.hyper = ops.opt_hyper(self.dev, lr, (0.9, 0.999), 1e-8, max_grad_norm, ema_rate)
        if skip_nonfinite:
            self.skipped = ops.skipped_counter(self.dev)
        if max_grad_norm is not None or skip_nonfinite:       # the guard reads the norm too
            self.partials = torch.zeros(ops.grad_sqnorm_partials(self.n), dtype=torch.float64, device=self.dev)
            self.grad_norm = torch.zeros((), dtype=torch.float32, device=self.dev)      # the pre-clip global norm
        if ema_rate is not None:
            self.ema = self.flat.detach().clone()                                       # seeded from the parameters

    def _optim_update(self, g):
        """[grad_sqnorm if clipping] -> adam_step_ex: kernel nodes only.  With N ranks ``g`` is the all-reduced bucket,
        so every rank forms the same norm and the same coefficient and the replicas stay bitwise identical."""
        if self.partials is not None:
            ops.grad_sqnorm(g, 1.0, self.partials)
        if not self._optim_ex:
            ops.adam_step_ex(self.flat, g, self.m, self.v, self.hyper, self.step_dev, ema=self.ema,
                             partials=self.partials, grad_norm_out=self.grad_norm)
            return
        ops.optim_step(self.flat, g, self.m, self.v, self.hyper, self.step_dev, ema=self.ema, partials=self.partials,
                       grad_norm_out=self.grad_norm, clip=self.max_grad_norm is not None, decay_mode=self.decay_mode,
                       skipped=self.skipped, ema_warmup=self.ema_warmup)

    @property
    def skipped_steps(self) -> int:
        """Steps the non-finite guard skipped so far (``skip_nonfinite=True``; 0 without it).  An int: reading it
        synchronises with the device.  A skipped step leaves the parameters, the Adam moments and the average untouched,
        and the bias corrections and the EMA warm-up count effective updates only.  It is still a step in every other
        respect: (1) the ``loss`` it reports is whatever the kernels produced (usually non-finite); (2) its batch
        (``data=``) and its Philox draws are consumed, the stream is not rewound; (3) ``lr_schedule(k)`` stays indexed
        by the host's count of ``step()`` calls, skipped ones included.  With N ranks the norm is taken after the
        all-reduce, so every rank reaches the same verdict."""
        return 0 if self.skipped is None else ops.skipped_count(self.skipped, self.step_dev)

    def set_lr(self, lr: float) -> None:
        """A device-lr trainer: one ordinary fill kernel on the current stream (outside any capture), legal between
        replays.  A default trainer has the learning rate baked into the captured step: only before the capture."""
        lr = float(lr)
        if self.device_lr:
            self.hyper[ops.OPT_LR:ops.OPT_LR + 1].fill_(lr)
        elif lr != self.lr and self.graph is not None:
            raise MsgmError("the captured step has the learning rate baked in; build a new trainer for another lr")
        self.lr = lr

    def _pre_step(self):
        """Host side of ``step()``: refuse inside ``ema_weights()``, apply ``lr_schedule(k)`` for the 1-based number k of
        the update about to be made."""
        if self._in_ema:
            raise MsgmError("step() inside ema_weights(): the parameter bucket holds the average; leave the context first")
        self._k += 1
        if self.lr_schedule is not None:
            self.set_lr(self.lr_schedule(self._k))

    def _pre_capture(self):
        if self._in_ema:
            raise MsgmError("capture() inside ema_weights(): the parameter bucket holds the average")

    def ema_state_dict(self) -> dict:
        """The averaged weights under ``net.state_dict()``'s own keys and shapes (buffers, if any, as they are): loads
        into this net's class and into the reference's modules alike."""
        if self.ema is None:
            raise MsgmError("ema_state_dict() needs a trainer built with ema_rate=...")
        offs, off = {}, 0
        for name, p in self.net.named_parameters():
            offs[name] = (off, p.numel())
            off += p.numel()
        out = type(self.net.state_dict())()
        for k, t in self.net.state_dict().items():
            out[k] = (self.ema[offs[k][0]:offs[k][0] + offs[k][1]].view(t.shape) if k in offs else t).detach().clone()
        return out

    @contextlib.contextmanager
    def ema_weights(self):
        """``with tr.ema_weights():`` — the contents of the parameter bucket and of the average change places
        (msgm_swap, in place: no address changes), so forward, ``ssm`` and the samplers run on the average; the exit
        swaps back bitwise.  The convolution sets repack their images from the live weights on every pass
        (ConvOpSet.pack / pack_wino run inside each forward), and so does a ``GraphedStepSampler`` graph built BEFORE
        entering: its pack launches are kernel nodes of the captured forward, so it needs no rebuild and samples from
        the average inside the context.  ``step()``, ``capture()`` and nesting raise MsgmError here; write checkpoints
        outside the context (inside it ``gen_sde.state_dict()`` holds the average)."""
        if self.ema is None:
            raise MsgmError("ema_weights() needs a trainer built with ema_rate=...")
        if self._in_ema:
            raise MsgmError("ema_weights() does not nest")
        if torch.cuda.is_current_stream_capturing():
            raise MsgmError("ema_weights() inside a graph capture")
        ops.swap_(self.flat, self.ema)
        self._in_ema = True
        try:
            yield self
        finally:
            ops.swap_(self.flat, self.ema)
            self._in_ema = False


def warmup_cosine(base_lr: float, warmup: int, total: int, min_lr: float = 0.0) -> Callable[[int], float]:
    """A ready-made ``lr_schedule``: k -> lr for the 1-based update number k.  Linear warm-up base_lr * k / warmup over
    the first ``warmup`` updates, then half a cosine from base_lr (k = warmup) down to min_lr (k >= total)."""
    if warmup < 0 or total <= warmup:
        raise ValueError("warmup_cosine needs 0 <= warmup < total")

    def lr(k: int) -> float:
        if k <= warmup:
            return base_lr * k / warmup
        q = min(1.0, (k - warmup) / (total - warmup))
        return min_lr + 0.5 * (base_lr - min_lr) * (1.0 + math.cos(math.pi * q))
    return lr


def _msgm_draws(tr):
    """(y, t, v, u, cst) of one training step under the MULTIPLICATIVE SDE, drawn in the order and from the stream
    positions ``PluginReverseSDE.ssm`` uses (SDEs.py:684-693 sample_t, :78-122 sample_scheme, :514-515 probe): uniform t
    clamped at t_epsilon, the device-resident masked RK4 forward perturbation over the nsf-step grid
    (sde_scheme.msgm_forward_perturb), the Rademacher probe, then u = G(y)^T v, cst of the general loss form
    (msgm_ssm_terms).  Every launch is a kernel on the current stream, no host synchronisation: capturable.
    The base SDE draws from the TRAINER's Philox stream (shard placement included)."""
    from .sde_scheme import msgm_forward_paths, msgm_forward_perturb
    base, rng = tr.base, tr.rng
    if tr.intT:
        # the integrated loss (gen_sde.ssm_intT): one path per row of x in one launch, every kept grid state a training
        # row (time-major), tr.t the resident tiled grid; the stream positions are those of eager ssm()
        y = msgm_forward_paths(base, tr.x, first_keep=tr.k0).view(tr.rows, tr.d)      # advances the stream by nsf
        v = ops.rademacher((tr.rows, tr.d), tr.dev, rng=rng)
        rng.advance(1)
        uu, cst = ops.ssm_terms(y, v, tr.t, tr.st)
        return y, tr.t, v, uu, cst
    ops.fill_uniform(tr.u, rng, L.RNG_STREAM_T)
    torch.mul(tr.u, tr.T_host, out=tr.t)
    tr.t.clamp_(min=base.t_epsilon)                  # == m*t_eps + (1-m)*t of SDEs.py:690-692, bit for bit
    y = msgm_forward_perturb(base, tr.t.view(-1, 1), tr.x)          # advances the stream by 2 nsf + 2
    v = ops.rademacher((tr.B, tr.d), tr.dev, rng=rng)
    rng.advance(1)
    uu, cst = ops.ssm_terms(y, v, tr.t, tr.st)
    return y, tr.t, v, uu, cst


def _init_row_weights(tr, row_weights: bool):
    """``row_weights=True``: a resident (B_local,) buffer of per-row loss weights, ones until ``set_data(x, weight=w)``
    copies others in.  Its POINTER goes into the captured step, so later replays read the new values without a
    re-capture.  Weights are per local row; ``inv_batch`` stays 1/(B_local * world), the reported loss is
    inv_batch * sum_b w_b L_b.  A ragged last batch: pad it, weight the valid rows B/n_valid and the padding 0 (the
    padding rows still flow through the arithmetic: keep them finite)."""
    tr.w = torch.ones(tr.rows, dtype=torch.float32, device=tr.dev) if row_weights else None


def _set_data(tr, x, weight):
    if tr.data is not None:
        raise MsgmError("set_data() on a trainer built with data=...: the next step draws its own batch over it")
    if weight is not None:
        if tr.w is None:
            raise MsgmError("set_data(weight=...) needs a trainer built with row_weights=True")
        ops._row_weight(weight, tr.rows)
    tr.x.copy_(x)
    if weight is not None:
        tr.w.copy_(weight)


def _init_data(tr, data):
    """``data=sampler``: a device sampler of sdeflow_light_amd.data whose ``sample_into(x, rng)`` heads every step.  An
    ArrayData under the additive SDE is read by the fused prep launch instead (same bits, one launch fewer)."""
    from .data import ArrayData
    tr.data, tr._table = data, None
    if data is None:
        return
    if not hasattr(data, "sample_into") or not hasattr(data, "dim"):
        raise MsgmError("data= takes a device sampler of sdeflow_light_amd.data (sample_into, dim)")
    if data.dim != tr.d:
        raise MsgmError(f"the {getattr(data, 'name', 'data')} sampler has dim {data.dim}, the score net takes {tr.d}")
    data.to(tr.dev)
    if _epoch_data(tr):
        data.bind(tr.world)       # gather, cursor += B_local * world, then the existing path: the fused prologue has no cursor
    elif isinstance(data, ArrayData) and tr.base.kind == L.SDE_SGM:
        tr._table = data.table()


def _epoch_data(tr) -> bool:
    """Does the trainer draw epochs without replacement (``data=ArrayData(..., replace=False)``)?"""
    from .data import ArrayData
    return isinstance(tr.data, ArrayData) and not tr.data.replace


def _draw_data(tr):
    """Head of a step on the trainer's stream: the sampler's launches, unless the prep launch gathers (tr._table)."""
    if tr.data is not None and tr._table is None:
        tr.data.sample_into(tr.x, tr.rng)


def _ssm_prep(tr):
    """The additive SDE's prep launch: perturbation + probe + step tick, on the resident batch or through the gather."""
    if tr._table is not None:
        ops.ssm_prep_gather(tr._table, tr.x, tr.y, tr.t, tr.vp, tr.st, tr.rng, tr.step_dev)
        return
    ops.check(ops.lib().msgm_ssm_prep(tr.x.data_ptr(), tr.y.data_ptr(), tr.t.data_ptr(), tr.vp.data_ptr(), tr.B, tr.d, tr.st,
                                      tr.rng.ptr(), tr.step_dev.data_ptr(), ops.stream()), "msgm_ssm_prep")


def _training_rows(tr):
    """``tr.rows``: the rows of one step's loss.  B, or with ``gen_sde.ssm_intT`` the nsf' B kept grid states of B forward
    paths (``tr.k0`` leading grid times dropped, ``tr.t_grid`` the kept ones).  The integrated loss is refused here,
    before any launch, where the captured step could not hold it."""
    tr.intT = bool(getattr(tr.gen_sde, "ssm_intT", False))
    tr.rows, tr.k0 = tr.B, 0
    if not tr.intT:
        return
    if tr.base.kind == L.SDE_SGM:
        raise MsgmError("ssm_intT trainers are built for the multiplicative SDE; the additive SDE has a closed-form perturbation")
    if tr.world > 1:
        raise MsgmError("ssm_intT with world > 1: time-major rows break the shard base of the probe draw; not built")
    if not ops.forward_perturb_supported(tr.base.kind, tr.d):
        raise MsgmError(f"ssm_intT trainers need a row length msgm_forward_paths takes in one launch (n = {tr.d} is not): "
                        "the composed trajectory holds copy nodes, and the captured step kernel nodes only")
    tr.t_grid, tr.k0 = tr.gen_sde.intT_grid(tr.dev)
    tr.rows = tr.t_grid.numel() * tr.B


def _adopt_stream(tr):
    """The multiplicative SDE's forward perturbation draws through ``base.philox()``: hand it the trainer's stream."""
    tr.msgm = tr.base.kind != L.SDE_SGM
    if tr.msgm:
        tr.base.rng = tr.rng
        tr.T_host = tr.base.T_float()
        if tr.intT:
            tr.t = tr.t_grid.repeat_interleave(tr.B).contiguous()        # a resident constant: the tiled grid
        else:
            tr.u = torch.empty(tr.B, dtype=torch.float32, device=tr.dev)


class MLPScoreTrainer(_TrainerState):
    """MLP score net (configs C1/C2) under the additive (SGMsde) or the multiplicative SDE (MSGMsde, dense or sparse
    tensor: MSGM_higherDim.py:733-746).  ``x`` is this rank's shard (B_local, d) and stays resident; each ``step()`` draws
    fresh (t, eps | forward-SDE noise, v) on the device — and, with ``data=sampler``, a fresh ``x`` as well."""

    def __init__(self, gen_sde, batch_local: int, lr: float = 1e-3, world: int = 1, use_graph: bool = True,
                 seed: int = 0, row_base: int = 0, row_weights: bool = False, *, max_grad_norm: Optional[float] = None,
                 ema_rate: Optional[float] = None, lr_schedule: Optional[Callable[[int], float]] = None,
                 device_lr: bool = False, data=None, weight_decay: float = 0.0, decoupled_weight_decay: bool = True,
                 skip_nonfinite: bool = False, ema_warmup: bool = False):
        from .NN import MLP
        net, base = gen_sde.a, gen_sde.base_sde
        if not isinstance(net, MLP):
            raise MsgmError("MLPScoreTrainer is built for the MLP score net (SGMsde or MSGMsde)")
        self.gen_sde, self.net, self.base = gen_sde, net, base
        self.dev = next(net.parameters()).device
        self.B, self.d, self.world = batch_local, net.input_dim, world
        _training_rows(self)
        self.flat, self.gflat = net.flat_parameters()
        self.n = self.flat.numel()
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=self.dev)
        # same seed on every rank + the shard's first global row: the N-rank run draws what the 1-rank run draws
        self.rng = L.PhiloxState(seed * 1000003 + 17, self.dev, row_base=row_base, n=self.d)
        self.ws = ops.mlp_ssm_workspace(self.d, net.pre is not None, self.dev)
        # ONE all-reduce bucket per step: [flat gradient | mean loss] = the net's own gradient bucket
        self.gbuf = net.grad_bucket()
        self.loss = self.gbuf[self.n:]
        self.x = torch.zeros(batch_local, self.d, dtype=torch.float32, device=self.dev)
        self.y = torch.empty_like(self.x)
        self.t = torch.empty(batch_local, dtype=torch.float32, device=self.dev)
        self.vp = torch.empty_like(self.x)
        self._init_optim(lr, max_grad_norm, ema_rate, lr_schedule, device_lr, weight_decay, decoupled_weight_decay,
                         skip_nonfinite, ema_warmup)
        self.P = net.kernel_params()
        self.st = base.struct()
        self.inv_batch = 1.0 / (self.rows * world)          # mean over the GLOBAL batch
        self.graph = None
        self.use_graph = use_graph and not parallel.multi(world)
        _init_row_weights(self, row_weights)
        _adopt_stream(self)
        _init_data(self, data)

    def _body(self):
        """3 launches on one GPU: prep (K1 + probe + step tick) -> fused SSM kernel ->
        slab reduction fused with Adam (+ Philox advance).  With N>1 ranks the
        reduction and Adam are split around the RCCL all-reduce of the flat bucket."""
        import ctypes as C
        lib, s = ops.lib(), ops.stream()
        _draw_data(self)
        if self.msgm:
            # multiplicative SDE: no closed-form perturbation — masked RK4 on the device, then the general loss form
            y, t, vp, uu, cst = _msgm_draws(self)
            ops.counter_inc(self.step_dev)
            pu, pc, adv = uu.data_ptr(), cst.data_ptr(), None       # the draws advanced the stream themselves
            self._live = (y, vp, uu, cst)
        else:
            _ssm_prep(self)
            y, t, vp, pu, pc, adv = self.y, self.t, self.vp, None, None, self.rng.ptr()
        nsl = C.c_int32(0)
        ops.check(lib.msgm_mlp_ssm_partial_w(self.P, y.data_ptr(), t.data_ptr(), vp.data_ptr(), pu, pc, self.rows,
                                             self.st, self.inv_batch, ops.ptr(self.w), None, self.ws.data_ptr(),
                                             self.ws.numel() * 4, C.byref(nsl), s), "msgm_mlp_ssm_partial_w")
        pre = int(self.net.pre is not None)
        if self.device_lr:
            # option route: slab reduction -> [all-reduce] -> [grad_sqnorm] -> adam_step_ex -> Philox advance
            ops.check(lib.msgm_mlp_ssm_reduce(self.d, pre, self.ws.data_ptr(), nsl.value, self.inv_batch,
                                              self.gflat.data_ptr(), self.loss.data_ptr(), s), "msgm_mlp_ssm_reduce")
            if parallel.multi(self.world):
                parallel.allreduce_sum_(self.gbuf)
            self._optim_update(self.gflat)
            if not self.msgm:
                self.rng.advance(1)
        elif not parallel.multi(self.world):
            ops.check(lib.msgm_mlp_ssm_reduce_adam(self.d, pre, self.ws.data_ptr(), nsl.value, self.inv_batch,
                                                   self.gflat.data_ptr(), self.loss.data_ptr(), self.flat.data_ptr(),
                                                   self.m.data_ptr(), self.v.data_ptr(), self.lr, 0.9, 0.999, 1e-8,
                                                   self.step_dev.data_ptr(), adv, s), "msgm_mlp_ssm_reduce_adam")
        else:
            ops.check(lib.msgm_mlp_ssm_reduce(self.d, pre, self.ws.data_ptr(), nsl.value, self.inv_batch,
                                              self.gflat.data_ptr(), self.loss.data_ptr(), s), "msgm_mlp_ssm_reduce")
            parallel.allreduce_sum_(self.gbuf)    # grads and loss already carry 1/global_batch
            ops.adam_step(self.flat, self.gflat, self.m, self.v, step=0, lr=self.lr, step_dev=self.step_dev)
            if not self.msgm:
                self.rng.advance(1)

    def capture(self):
        """One ordinary step on a side stream (loads code objects; it is a REAL training step: parameters, Adam state,
        Philox offset and step counter all live on the device), then the capture — which records and executes nothing."""
        self._pre_capture()
        s = torch.cuda.Stream(device=self.dev)
        s.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(s):
            self._body()
        torch.cuda.current_stream(self.dev).wait_stream(s)
        torch.cuda.synchronize(self.dev)
        self.graph = ops.new_graph()
        with torch.cuda.graph(self.graph):
            self._body()

    def set_data(self, x: torch.Tensor, weight: Optional[torch.Tensor] = None):
        _set_data(self, x, weight)

    def step(self):
        self._pre_step()
        if self.use_graph:
            if self.graph is None:
                self.capture()           # its warm-up IS this call's training step (one update per call)
                return self.loss
            self.graph.replay()
        else:
            self._body()
        return self.loss


class UNetScoreTrainer(_TrainerState):
    """A U-Net score net exposing ``ssm_grad`` (configs C3/C4) under the additive SDE or the multiplicative one (the
    paper's model: MSGMsde, sparse tensor for d >= 256, nsf forward RK4 steps — MSGM_higherDim.py:733-746): prep kernel
    (K1 + probe) -> dual-number forward / hand-written backward -> [RCCL all-reduce
    of the flat gradient bucket] -> fused Adam on the flat parameter bucket.

    The step enqueues ~2000 small launches for the 2-D U-Net; at the C4 shard size
    (32 samples per GPU) the launch gaps cost as much as the kernels, so everything
    before the collective is captured ONCE as a hipGraph and replayed (``use_graph``);
    with one rank the Adam update and the Philox advance are inside the graph too."""

    def __init__(self, gen_sde, batch_local: int, dim: int, lr: float = 1e-4, world: int = 1, seed: int = 0,
                 use_graph: Optional[bool] = None, row_base: int = 0, row_weights: bool = False, *,
                 max_grad_norm: Optional[float] = None, ema_rate: Optional[float] = None,
                 lr_schedule: Optional[Callable[[int], float]] = None, device_lr: bool = False, data=None,
                 weight_decay: float = 0.0, decoupled_weight_decay: bool = True, skip_nonfinite: bool = False,
                 ema_warmup: bool = False):
        net, base = gen_sde.a, gen_sde.base_sde
        if not hasattr(net, "ssm_grad"):
            raise MsgmError("UNetScoreTrainer needs a HIP U-Net score net (SGMsde or MSGMsde)")
        self.gen_sde, self.net, self.base = gen_sde, net, base
        self.dev = next(net.parameters()).device
        self.B, self.d, self.world = batch_local, dim, world
        _training_rows(self)
        self.flat, self.gflat = net.flat_parameters()
        self.n = self.flat.numel()
        self._init_optim(lr, max_grad_norm, ema_rate, lr_schedule, device_lr, weight_decay, decoupled_weight_decay,
                         skip_nonfinite, ema_warmup)
        self.m, self.v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self.gbuf = net.grad_bucket()            # ONE bucket [grads | mean loss]: the net's gradient bucket IS the
        self.loss = self.gbuf[self.n:]           # collective buffer (no 16 MB staging copy per step)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.rng = L.PhiloxState(seed * 1000003 + 29, self.dev, row_base=row_base, n=dim)
        self.x = torch.zeros(batch_local, dim, dtype=torch.float32, device=self.dev)
        self.y, self.vp = torch.empty_like(self.x), torch.empty_like(self.x)
        self.t = torch.empty(batch_local, dtype=torch.float32, device=self.dev)
        self.st = base.struct()
        self.inv_batch = 1.0 / (self.rows * world)
        # default: graph everywhere.  With N ranks the graph ends before the collective (capture_error_mode
        # "thread_local": the process group's watchdog thread may touch the runtime during the capture), the
        # all-reduce and Adam follow eagerly on the same stream
        self.use_graph = True if use_graph is None else bool(use_graph)
        self.graph = None
        _init_row_weights(self, row_weights)
        _adopt_stream(self)
        _init_data(self, data)

    def set_data(self, x, weight: Optional[torch.Tensor] = None):
        _set_data(self, x, weight)

    def _fwd_bwd(self):
        """Everything before the collective; leaves [grads | loss] (already x 1/global_batch) in ``gbuf``."""
        _draw_data(self)
        if self.msgm:
            y, t, vp, u, cst = _msgm_draws(self)
            ops.counter_inc(self.step_dev)
            self._live = (y, vp, u, cst)
        else:
            _ssm_prep(self)
            y, t, vp = self.y, self.t, self.vp
            u, cst = ops.ssm_terms(y, vp, t, self.st)
        per = self.net.ssm_grad(y, t, vp, u, cst, self.inv_batch, rng=self.rng,     # 2-D U-Net dropout masks: the trainer's stream
                                row_weight=self.w)
        flat, gflat = self.net.flat_parameters()
        if flat.data_ptr() != self.flat.data_ptr() or gflat.data_ptr() != self.gbuf.data_ptr():
            raise MsgmError("the flat parameter bucket moved; rebuild the trainer")
        # kernel nodes only inside the captured step (no D2D memcpy / memset nodes: see msgm_zero_async in csrc/common.h)
        if self.w is not None:
            per = per * self.w                   # the reported loss is inv_batch * sum_b w_b L_b (an elementwise kernel)
        torch.sum(per.view(1, -1), dim=1, out=self.loss)
        self.loss.mul_(self.inv_batch)

    def _update(self):
        if self.device_lr:
            self._optim_update(self.gbuf[: self.n])
        else:
            ops.adam_step(self.flat, self.gbuf[: self.n], self.m, self.v, step=0, lr=self.lr, step_dev=self.step_dev)
        if not self.msgm:                        # the multiplicative SDE's draws advance the stream as they go
            self.rng.advance(1)

    def _collective_update(self):
        if parallel.multi(self.world):
            parallel.allreduce_sum_(self.gbuf)       # ONE collective: flat gradient bucket + the loss scalar
        self._update()

    def capture(self):
        """One ordinary eager step with the pre-collective part on a side stream (allocations, packed-weight
        images, one-time kernel attributes), then the capture.  Parameters, Adam state, Philox offset and step
        counter all live on the device, so the warm-up is a real training step and every replay is the next one.
        With one rank the graph holds the whole step; with N ranks it ends before the RCCL all-reduce."""
        self._pre_capture()
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            self._fwd_bwd()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        self._collective_update()
        torch.cuda.synchronize(self.dev)
        self._eager_step_done = True
        graph = ops.new_graph()
        mode = "global" if not parallel.multi(self.world) else "thread_local"      # a collective backend's watchdog thread must not
        with torch.cuda.graph(graph, capture_error_mode=mode):       # invalidate the capture
            self._fwd_bwd()
            if not parallel.multi(self.world):
                self._update()
        self.graph = graph

    def step(self):
        self._pre_step()
        if not self.use_graph:
            self._fwd_bwd()
            self._collective_update()
            return self.loss
        if self.graph is None:
            try:
                self.capture()                       # performs this call's step eagerly
            except Exception as e:                   # noqa: BLE001
                # capture() runs the eager step FIRST, so this call's update is already done when the capture itself
                # fails.  With N ranks a failed capture next to a live RCCL communicator must not take the job down:
                # log it and stay on the eager path in the same process (N > 1 RCCL capture is unverified on hardware).
                if not parallel.multi(self.world) or not getattr(self, "_eager_step_done", False):
                    raise
                import sys
                print(f"[msgm] hipGraph capture of the train step failed with {self.world} ranks ({type(e).__name__}: {e}); "
                      "continuing eagerly", file=sys.stderr)
                self.graph, self.use_graph = None, False
            return self.loss
        self.graph.replay()
        if parallel.multi(self.world):
            self._collective_update()
        return self.loss
