"""Restatements for the data stage (csrc/data_kernels.hip), used by tests/test_data_stage.py (CPU) and
tests/test_data_stage_gpu.py: the gather's index rule in numpy on top of philox_np.words, and the four synthetic samplers
in torch at a chosen dtype — float64 is the truth, float32 the yardstick (the reference's own arithmetic)."""
import math

import numpy as np
import torch

import philox_np as PH

RNG_STREAM_DATA, RNG_STREAM_DATA_ELEM, RNG_STREAM_DATA_CALL = 5, 6, 7
K24 = 1 << 24
CAUCHY_EDGE_K = (0, 1, (1 << 23) - 1, 1 << 23, K24 - 1)


def gather_index(seed, offset, row_base, B, N):
    """idx_b = (uint64(word_b) * N) >> 32, word_b = word e & 3 of block e >> 2 of RNG_STREAM_DATA, e = row_base + b."""
    w = PH.words(seed, offset, RNG_STREAM_DATA, np.arange(B, dtype=np.uint64) + np.uint64(row_base))
    return ((w.astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


def state_index(rng, B, N):
    """gather_index at a PhiloxState's current (seed, offset, row_base): reads the device state (synchronises)."""
    sd = rng.state_dict()
    return gather_index(sd["seed"], sd["offset"], sd["row_base"], B, N)


def cauchy(u, dtype):
    """Standard Cauchy from float32 uniforms in [0, 1) by the kernel's rule: k = (int)(u 2^24), m = min(k, 2^24 - 1 - k),
    w = (m + 1/2) 2^-24, cos(pi w) / sin(pi w), negative for k < 2^23."""
    k = (u.double() * K24).long().clamp(0, K24 - 1)
    m = torch.minimum(k, K24 - 1 - k)
    w = (m.to(dtype) + 0.5) * (1.0 / K24)
    q = torch.cos(math.pi * w) / torch.sin(math.pi * w)
    return torch.where(k < (1 << 23), -q, q)


def synth(kind, dtype, A=None, u=None, z=None, noise=0.5):
    """x of msgm_data_synth from injected draws (CPU tensors), evaluated in ``dtype``."""
    c = lambda t: None if t is None else t.to(dtype)
    At = None if A is None else c(A).T
    mm = (lambda d: d) if A is None else (lambda d: d @ At)
    if kind == "swiss":
        t = (1.5 * math.pi) * (1.0 + 2.0 * c(u))
        zz = c(z)
        return torch.stack(((t * torch.cos(t) + noise * zz[:, 0]) / 5.0, (t * torch.sin(t) + noise * zz[:, 1]) / 5.0), 1)
    if kind == "gaussian":
        return mm(c(z))
    if kind == "cauchy":
        return mm(0.02 * cauchy(u, dtype))
    if kind == "gaussian_cauchy":
        return (0.02 * mm(c(z))) * cauchy(u, dtype)
    raise ValueError(kind)


def rel_l2(a, b):
    a, b = a.double().reshape(-1).cpu(), b.double().reshape(-1).cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))
