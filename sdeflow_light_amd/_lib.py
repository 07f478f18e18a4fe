"""ctypes binding of libmsgm_hip.so, derived from the C ABI declared in include/msgm_hip.h.

Nothing here repeats the header: _abi.py reads it once per process, and SIGNATURES, the Structure classes and the
constants below are computed from what it finds.  A new entry point is an edit of the header and its definition only.

Loading is lazy and LOUD: if the shared library is missing or a symbol is
absent the import of any kernel wrapper raises — there is no CPU / eager
fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _abi
from ._abi import MsgmError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmsgm_hip.so")

_ABI = _abi.load()
CONSTANTS = _ABI.constants       # every enumerator and integer #define of the header, by its C name


def _constants(prefix, *names):
    return (CONSTANTS[prefix + n] for n in names)


MSGM_OK, MSGM_E_UNSUPPORTED = _constants("MSGM_", "OK", "E_UNSUPPORTED")
SDE_SGM, SDE_MSGM_SPARSE, SDE_MSGM_DENSE = _constants("MSGM_SDE_", "SGM", "MSGM_SPARSE", "MSGM_DENSE")
PROC_REVERSE, PROC_FORWARD = _constants("MSGM_PROC_", "REVERSE", "FORWARD")
METHOD_EM, METHOD_HEUN, METHOD_RK4 = _constants("MSGM_METHOD_", "EM", "HEUN", "RK4")          # msgm_mlp_sde_loop
DATA_SWISS, DATA_GAUSSIAN, DATA_CAUCHY, DATA_GAUSSIAN_CAUCHY = _constants(                   # msgm_data_synth
    "MSGM_DATA_", "SWISS", "GAUSSIAN", "CAUCHY", "GAUSSIAN_CAUCHY")
# the Philox stream ids live in csrc/common.h, which is not the interface file
RNG_STREAM_T, RNG_STREAM_EPS, RNG_STREAM_V, RNG_STREAM_DW, RNG_STREAM_ROWS, RNG_STREAM_USER = 0, 1, 2, 3, 4, 16
RNG_STREAM_DATA, RNG_STREAM_DATA_ELEM, RNG_STREAM_DATA_CALL = 5, 6, 7     # the data stage: by row, by element, one scalar per call
RNG_STREAM_DATA_PERM = 8         # the round keys of an epoch's permutation (msgm_data_gather_epoch): seed and epoch only
RNG_STREAM_DROPOUT = 64         # + the ResBlock's index: the U-Net's dropout masks (include/msgm_hip.h, msgm_dropout_t)

# one Structure class per typedef struct of the header, msgm_foo_bar_t -> FooBarT
SdeT, OptT, OptimT, MlpParamsT, ConvGeomT, ConvFuseT, ReduceJobT, PackJobT, DropoutT, EmbJobT = (
    _ABI.classes[n] for n in ("msgm_sde_t", "msgm_opt_t", "msgm_optim_t", "msgm_mlp_params_t", "msgm_conv_geom_t",
                              "msgm_conv_fuse_t", "msgm_reduce_job_t", "msgm_pack_job_t", "msgm_dropout_t", "msgm_emb_job_t"))

# name -> (restype, argtypes), every msgm_* prototype of the header
SIGNATURES = {name: (res, [t for _, t in params]) for name, (res, params) in _ABI.functions.items()}


def bind(cdll: C.CDLL, missing_ok: bool = False) -> C.CDLL:
    """Sets restype and argtypes of every entry point on a loaded library.  ``missing_ok``: a build of another tree may
    lack entries that this header declares; they stay unbound."""
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(cdll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
        elif not missing_ok:
            raise MsgmError(f"{cdll._name} does not export {name}")
    return cdll


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    """The loaded library; raises MsgmError when it cannot be loaded."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MsgmError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        try:
            _lib = bind(C.CDLL(LIB_PATH))
        except OSError as e:  # pragma: no cover
            raise MsgmError(f"cannot load {LIB_PATH}: {e}") from e
    return _lib


def check(rc: int, what: str) -> None:
    if rc != MSGM_OK:
        raise MsgmError(f"{what} failed: {lib().msgm_error_string(rc).decode()} ({rc})")


def ptr(t: Optional[torch.Tensor]):
    """Device pointer of a contiguous CUDA(=HIP) tensor, or NULL for None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise MsgmError("libmsgm_hip kernels need device tensors (got a CPU tensor); there is no CPU fallback")
    if not t.is_contiguous():
        raise MsgmError("libmsgm_hip kernels need contiguous tensors")
    return t.data_ptr()


def f32(t: torch.Tensor, name: str = "tensor") -> torch.Tensor:
    if t.dtype != torch.float32:
        raise MsgmError(f"{name} must be float32 (got {t.dtype})")
    return t


_HOST_SCALARS = {}


def host_scalar(t) -> float:
    """Value of a one-element tensor (the horizon T: an nn.Parameter(requires_grad=False) on the device upstream,
    MSGM_higherDim.py:728) WITHOUT a device synchronisation per call: read once, cached per (storage address, version
    counter) — an in-place update (load_state_dict) bumps the version and is read again.  Needed because the reference's
    ``sde.T.item()`` (sde_scheme.py:54-57) sits inside code that the trainers capture into a hipGraph."""
    if not torch.is_tensor(t):
        return float(t)
    if t.device.type == "cpu":
        return float(t.item())
    key = (t.device.index, t.data_ptr(), t._version)
    v = _HOST_SCALARS.get(key)
    if v is None:
        if torch.cuda.is_current_stream_capturing():
            raise MsgmError("a device scalar (the horizon T) is read for the first time inside a graph capture; "
                            "run one eager step first")
        v = _HOST_SCALARS[key] = float(t.item())
    return v


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def sde_struct(kind: int, beta_min: float, beta_max: float, T: float, t_epsilon: float,
               G: Optional[torch.Tensor] = None, L_G: Optional[torch.Tensor] = None) -> SdeT:
    return SdeT(kind, float(beta_min), float(beta_max), float(T), float(t_epsilon), ptr(G), ptr(L_G))


class PhiloxState:
    """Device-resident Philox state consumed by kernels that draw noise: uint64[4] = {seed, offset, row_base,
    elem_base}.  ``set_shard(row_base, n)`` places this rank's rows inside the global index space of a data-parallel
    run (csrc/common.h), so a sharded run draws the numbers the single-GPU run draws for the same rows."""

    def __init__(self, seed: int, device, offset: int = 0, row_base: int = 0, n: int = 0):
        # int64 storage, reinterpreted as uint64 by the kernels
        self.state = torch.tensor([seed & 0x7FFFFFFFFFFFFFFF, offset, 0, 0], dtype=torch.int64, device=device)
        if row_base:
            self.set_shard(row_base, n)

    def ptr(self):
        return self.state.data_ptr()

    def set_shard(self, row_base: int, n: int) -> None:
        # k_fill / the prep kernels address draws by QUADS of the global index: row-indexed streams (t, the latent rows)
        # by row quads, element-indexed ones by element quads.  A base that is not a multiple of 4 would be truncated
        # and this shard would re-draw the previous rank's numbers.
        if row_base % 4 or (row_base * n) % 4:
            raise MsgmError("shard base: row_base (and row_base * n) must be multiples of 4 — Philox draws are addressed "
                            "by quads of the GLOBAL row / element index")
        self.state[2:].copy_(torch.tensor([row_base, row_base * n], dtype=torch.int64))

    def advance(self, n: int = 1) -> None:
        check(lib().msgm_rng_advance(self.ptr(), n, stream()), "msgm_rng_advance")

    def state_dict(self) -> dict:
        seed, offset, row_base, elem_base = (int(v) for v in self.state.tolist())
        return {"seed": seed, "offset": offset, "row_base": row_base, "elem_base": elem_base}

    def load_state_dict(self, sd: dict) -> None:
        """Restores the STREAM position (seed, offset) only.  The shard base {row_base, elem_base} belongs to the rank
        that loads, not to the rank that wrote the file: in a data-parallel resume every rank loads rank 0's checkpoint
        and must keep drawing the numbers of ITS rows (set_shard), otherwise all ranks would replay rank 0's noise."""
        self.state[:2].copy_(torch.tensor([sd["seed"], sd["offset"]], dtype=torch.int64))
