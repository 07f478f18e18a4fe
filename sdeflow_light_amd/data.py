"""Synthetic inputs of the BASELINE configs.  The reference has
no Gaussian-mixture sampler (its synthetic samplers are SwissRoll / Gaussian /
Cauchy, data.py:702-802); the benchmark mixture is build-defined: 8 equal
components on the circle r=2, isotropic sigma=0.15.

Device samplers (csrc/data_kernels.hip): ``SwissRoll``, ``Cauchy``, ``Gaussian``, ``GaussianCauchy`` and
``ArrayData`` keep the protocol the reference driver uses — ``.sample(n)``, ``.sampletest(n)``, ``.name``, ``.dim``,
``.get_std()`` — and draw on the GPU from a Philox stream.  ``sample(n)`` returns a new (n, dim) device tensor and moves the
sampler's own stream on by one; ``sample_into(x, rng)`` fills ``x`` from ``rng``'s current offset with kernel launches only
(no advance, no synchronisation), which is what a trainer built with ``data=sampler`` puts at the head of its captured step.
There is no CPU path: a CPU device raises ``MsgmError``."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib as L
from . import ops
from ._lib import MsgmError


def gaussian_mixture_2d(n: int, seed: int = 1234, device="cpu") -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 8, (n,), generator=g)
    ang = 2 * math.pi * k.float() / 8
    mean = torch.stack([2 * torch.cos(ang), 2 * torch.sin(ang)], 1)
    return (mean + 0.15 * torch.randn(n, 2, generator=g)).to(device)


def signals_1d(n: int, L: int = 1024, seed: int = 1234, device="cpu") -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    j = torch.arange(L).float()[None, None, :]
    A = 0.5 + 0.5 * torch.rand(n, 3, 1, generator=g)
    f = torch.randint(1, 17, (n, 3, 1), generator=g).float()
    ph = 2 * math.pi * torch.rand(n, 3, 1, generator=g)
    x = (A * torch.sin(2 * math.pi * f * j / L + ph)).sum(1) + 0.05 * torch.randn(n, L, generator=g)
    return x.to(device)


def random_images(n: int, C: int = 3, H: int = 64, W: int = 64, seed: int = 1234, device="cpu") -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, C * H * W, generator=g).to(device)


class _DeviceSampler:
    """What the five samplers share: the device, the sampler's own Philox stream, sample / sampletest."""

    def _init_device(self, device, seed: int) -> None:
        self.device = torch.device("cuda" if device is None else device)
        self.seed = int(seed)
        self._rng: Optional[L.PhiloxState] = None

    def _check_device(self) -> torch.device:
        if self.device.type != "cuda":
            raise MsgmError(f"the {self.name} sampler draws on the GPU (device={self.device}); there is no CPU fallback")
        return self.device

    def philox(self) -> L.PhiloxState:
        """The sampler's own stream (seeded by ``seed=``), created on first use."""
        if self._rng is None:
            self._rng = L.PhiloxState(self.seed * 1000003 + 41, self._check_device())
        return self._rng

    def to(self, device) -> "_DeviceSampler":
        """Move the resident tensors (the table, A) to ``device``; the stream restarts there at offset 0."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.device.type == "cuda" and self.device.index is None and self._rng is not None:
            self.device = self._rng.state.device                 # "cuda" resolved when the stream was made
        if device != self.device:
            self.device, self._rng = device, None
            self._moved()
        return self

    def _moved(self) -> None:
        pass

    def _draw(self, n: int, **kw) -> torch.Tensor:
        dev = self._check_device()
        if int(n) < 1:
            raise MsgmError(f"sample(n) needs n >= 1 (got {n})")
        x = torch.empty(int(n), self.dim, dtype=torch.float32, device=dev)
        rng = self.philox()
        self.sample_into(x, rng, **kw)
        rng.advance(1)
        return x

    def _check_batch(self, x: torch.Tensor) -> None:
        self._check_device()
        if not torch.is_tensor(x) or not x.is_cuda:
            raise MsgmError("sample_into fills a device tensor; there is no CPU fallback")
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise MsgmError(f"sample_into: x has shape {tuple(x.shape)}, the {self.name} sampler has dim {self.dim}")

    def sample(self, n: int) -> torch.Tensor:
        return self._draw(n)

    def sampletest(self, n: int) -> torch.Tensor:
        return self.sample(n)


class SwissRoll(_DeviceSampler):
    """Swiss roll distribution sampler (data.py:702-717); ``noise`` controls the thickness of the roll."""

    def __init__(self, *, device=None, seed: int = 0):
        self.dim = 2
        self.name = 'swiss'
        self._init_device(device, seed)

    def sample_into(self, x: torch.Tensor, rng: L.PhiloxState, noise: float = 0.5) -> torch.Tensor:
        self._check_batch(x)
        return ops.data_synth("swiss", x, noise=0.5 if noise is None else noise, rng=rng)

    def sample(self, n: int, noise: float = 0.5) -> torch.Tensor:
        return self._draw(n, noise=noise)

    def sampletest(self, n: int, noise: float = 0.5) -> torch.Tensor:
        return self.sample(n, noise)


class _Linear(_DeviceSampler):
    """Draws times A^T (data.py:719-778): A = randn(dim, dim) with ``correlation`` (torch's global generator, as upstream),
    else the identity; ``std`` = sqrt(diag(A A^T)) of the A first drawn; ``normalized`` rescales A's rows by 1 / std.
    ``A`` and ``std`` stay CPU tensors as upstream; the kernels read a device copy, and no copy at all for the identity."""
    _kind = ""

    def _init_linear(self, base: str, dim: int, correlation: bool, normalized: bool, device, seed: int) -> None:
        self.dim = dim
        self.name = base + str(self.dim)
        if correlation:
            self.A = torch.randn(dim, dim)
            self.name = self.name + "cor"
        else:
            self.A = torch.eye(dim)
        cov = self.A @ self.A.T
        self.std = torch.sqrt(torch.diag(cov))
        if normalized:
            self.name = self.name + '_norm'
            self.A = torch.diag(1 / self.std) @ self.A
        self._dense = bool(correlation)          # without correlation A is the identity, normalised or not (std = 1)
        self._A_dev: Optional[torch.Tensor] = None
        self._init_device(device, seed)

    def _moved(self) -> None:
        self._A_dev = None

    def _A(self) -> Optional[torch.Tensor]:
        if not self._dense:
            return None
        if self._A_dev is None:
            self._A_dev = self.A.to(device=self._check_device(), dtype=torch.float32).contiguous()
        return self._A_dev

    def sample_into(self, x: torch.Tensor, rng: L.PhiloxState) -> torch.Tensor:
        self._check_batch(x)
        return ops.data_synth(self._kind, x, A=self._A(), rng=rng)

    def get_std(self) -> torch.Tensor:
        return self.std


class Cauchy(_Linear):
    """multi-dimensional Cauchy distribution sampler, scale 1/50 (data.py:719-748)."""
    _kind = "cauchy"

    def __init__(self, dim=2, correlation=False, normalized=False, *, device=None, seed: int = 0):
        self._init_linear('cauchy', dim, correlation, normalized, device, seed)


class Gaussian(_Linear):
    """multi-dimensional Gaussian distribution sampler (data.py:751-778)."""
    _kind = "gaussian"

    def __init__(self, dim=2, correlation=True, normalized=False, *, device=None, seed: int = 0):
        self._init_linear('gaussian', dim, correlation, normalized, device, seed)


class GaussianCauchy(_Linear):
    """multi-dimensional Gaussian distribution scaled with ONE one-dim Cauchy(0, 1) draw per call and 1/50
    (data.py:780-802).  ``gaussian`` is the inner sampler's place upstream: it shares this sampler's A and std."""
    _kind = "gaussian_cauchy"

    def __init__(self, dim=2, correlation=True, normalized=False, *, device=None, seed: int = 0):
        self._init_linear('gaussian', dim, correlation, normalized, device, seed)
        self.gaussian = self
        self.name = 'gaussianCauchy' + str(self.dim)
        if correlation:
            self.name = self.name + "cor"
        if normalized:
            self.name = self.name + '_norm'


class _ReplaceKeyword(type):
    """Takes ``replace=`` at the class call, ``ArrayData(train, ..., replace=False)``, so that ``ArrayData.__init__`` keeps
    the parameter list of the reference's constructor plus ``device`` and ``seed`` (tests/test_data_stage.py pins it)."""

    def __call__(cls, *args, replace: bool = True, **kw):
        smp = super().__call__(*args, **kw)
        smp.replace = bool(replace)
        return smp


class ArrayData(_DeviceSampler, metaclass=_ReplaceKeyword):
    """The real-data protocol of data.py:691-700 over resident tables: ``sample(n)`` gathers n rows of ``train`` drawn with
    replacement (np.random.randint + fancy index upstream), ``sampletest(n)`` of ``test``.  ``train`` / ``test``: (N, dim)
    arrays or tensors, kept as float32 on the device.  ``std``: per-feature standard deviation ``get_std()`` reports
    (default: ``train.std(axis=0)`` as numpy forms it, the population one).

    ``replace=False``: epochs.  The training order is one endless stream of independent permutations of the N rows
    (DESIGN.md §4g), walked by a device cursor the sampler owns: ``sample_into`` gathers the rows of positions
    cursor + row_base + b and then moves the cursor on by ``x.shape[0] * stride`` in a launch of its own, so every aligned
    window of N positions trains on every row once, whatever the batch size.  ``stride`` is 1 until a trainer binds the
    sampler (``bind(world)``): the ranks of a data-parallel run, built with the same seed and ``row_base`` = the shard's
    first global row, then read together the rows of the 1-rank run.  The permutations are keyed by the seed of the
    stream handed to ``sample_into`` (the trainer's, or the sampler's own in ``sample``) and by the epoch, not by the
    stream's offset.  ``sampletest`` stays with replacement, as upstream."""

    def __init__(self, train, test=None, name: str = "array", std=None, *, device=None, seed: int = 0):
        train = self._table(train, "train")
        self.dim = int(train.shape[1])
        self.name = name
        test = None if test is None else self._table(test, "test")
        if test is not None and test.shape[1] != self.dim:
            raise MsgmError(f"test has {test.shape[1]} features, train has {self.dim}")
        if device is None and train.is_cuda:
            device = train.device
        self._init_device(device, seed)
        self.std = (train.double().std(dim=0, unbiased=False).float().cpu() if std is None
                    else torch.as_tensor(std, dtype=torch.float32).reshape(-1).cpu())
        if self.std.numel() != self.dim:
            raise MsgmError(f"std has {self.std.numel()} entries, the table has {self.dim} features")
        self._train, self._test = train, test
        self.max_nsamples = int(train.shape[0])
        self.max_nsamplestest = 0 if test is None else int(test.shape[0])
        self.replace = True                           # replace=False arrives through the class call (_ReplaceKeyword)
        self._cursor: Optional[torch.Tensor] = None
        self.stride, self._world = 1, None
        self._moved()

    @staticmethod
    def _table(a, what: str) -> torch.Tensor:
        t = torch.as_tensor(a)
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise MsgmError(f"{what} must be a non-empty (N, dim) table (got shape {tuple(t.shape)})")
        if t.shape[0] >= 2 ** 31:
            raise MsgmError(f"{what} has {t.shape[0]} rows; the gather indexes fewer than 2^31")
        return t

    def _moved(self) -> None:
        self._resident = False
        if self._cursor is not None:                  # the position moves with the table
            self._cursor = self._cursor.to(self.device)

    def table(self, test: bool = False) -> torch.Tensor:
        """The resident (N, dim) float32 table the kernels read; copied to the device on first use."""
        dev = self._check_device()
        if not self._resident:
            self._train = self._train.to(device=dev, dtype=torch.float32).contiguous()
            if self._test is not None:
                self._test = self._test.to(device=dev, dtype=torch.float32).contiguous()
            self._resident = True
        if test and self._test is None:
            raise MsgmError(f"the {self.name} sampler was built without a test table")
        return self._test if test else self._train

    def sample_into(self, x: torch.Tensor, rng: L.PhiloxState, test: bool = False) -> torch.Tensor:
        self._check_batch(x)
        if self.replace or test:
            return ops.data_gather(self.table(test), x, rng=rng)
        # the gather only reads the cursor; the advance is the next launch, so no lane races with the update
        cur = self.cursor()
        ops.data_gather_epoch(self.table(), x, rng, cur)
        ops.counter_add(cur, x.shape[0] * self.stride)
        return x

    # ------------------------------------------------------------------ epochs (replace=False)
    def _check_epochs(self, what: str) -> None:
        if self.replace:
            raise MsgmError(f"{what}: the {self.name} sampler draws with replacement; build it with replace=False")

    def cursor(self) -> torch.Tensor:
        """The device cursor (int64[1]): the stream position of the next batch's first global row."""
        self._check_epochs("cursor()")
        if self._cursor is None:
            self._cursor = torch.zeros(1, dtype=torch.int64, device=self._check_device())
        return self._cursor

    def bind(self, world: int) -> None:
        """A trainer of ``world`` ranks takes the sampler: every step moves the cursor by B_local * world."""
        self._check_epochs("bind()")
        world = int(world)
        if world < 1:
            raise MsgmError(f"bind(world) needs world >= 1 (got {world})")
        if self._world is not None and self._world != world:
            raise MsgmError(f"the {self.name} sampler is bound to world = {self._world}; it cannot serve world = {world} too")
        self._world = self.stride = world

    @property
    def position(self) -> int:
        """Stream position of the next batch (reads the device cursor: eager use only)."""
        cur = self.cursor()
        if torch.cuda.is_current_stream_capturing():
            raise MsgmError("position / epoch read the device cursor on the host; not inside a graph capture")
        return int(cur.item())

    @position.setter
    def position(self, value: int) -> None:
        value = int(value)
        if value < 0:
            raise MsgmError(f"the stream position must be >= 0 (got {value})")
        cur = self.cursor()
        if torch.cuda.is_current_stream_capturing():
            raise MsgmError("the cursor is set between replays, not inside a graph capture")
        cur.fill_(value)                              # in place: a captured step keeps the cursor's address

    @property
    def epoch(self) -> int:
        """Index of the permutation the next batch starts in."""
        return self.position // self.max_nsamples

    def steps_per_epoch(self, batch_global: int) -> float:
        """N / batch_global: steps per pass over the table (a batch may straddle two passes)."""
        return self.max_nsamples / int(batch_global)

    def sampletest(self, n: int) -> torch.Tensor:
        return self._draw(n, test=True)

    def get_std(self) -> torch.Tensor:
        return self.std
