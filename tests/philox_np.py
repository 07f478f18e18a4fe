"""NumPy restatement of the device Philox4x32-10 stream (csrc/common.h) and of the U-Net dropout mask rule
(include/msgm_hip.h, msgm_dropout_t).  Used by the tests and by tools/make_golden.py; the package never
imports it."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
RNG_STREAM_DROPOUT = 64


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on arrays of 32-bit counters: returns the four output words (uint32 arrays)."""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in (c0, c1, c2, c3)]
    c0, c1, c2, c3 = np.broadcast_arrays(*c)
    k0, k1 = np.uint64(int(k0) & MASK), np.uint64(int(k1) & MASK)
    m0, m1, sh, mk = np.uint64(M0), np.uint64(M1), np.uint64(32), np.uint64(MASK)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                       # < 2^64: exact in uint64
        hi0, lo0, hi1, lo1 = p0 >> sh, p0 & mk, p1 >> sh, p1 & mk
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & mk, (k1 + np.uint64(W1)) & mk
    return tuple(v.astype(np.uint32) for v in (c0, c1, c2, c3))


def msgm_philox(seed, offset, stream, quad):
    """The block of msgm_philox(rng, 0, stream, quad): counter (quad lo, quad hi, stream, offset lo), key (seed lo,
    seed hi ^ offset hi).  Returns a (len(quad), 4) uint32 array."""
    q = np.asarray(quad, dtype=np.uint64)
    w = philox4x32_10(q & np.uint64(MASK), q >> np.uint64(32), stream, offset & MASK, seed & MASK,
                      ((seed >> 32) ^ (offset >> 32)) & MASK)
    return np.stack(w, axis=-1)


def words(seed, offset, stream, e):
    """Word e & 3 of block e >> 2 for every element index e."""
    e = np.asarray(e, dtype=np.uint64)
    blk = msgm_philox(seed, offset, stream, e >> np.uint64(2))
    return np.take_along_axis(blk, (e & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]


def fill_uniform(seed, offset, stream, n, base=0):
    """ops.fill_uniform for an element-indexed stream with element base ``base`` (rng[3])."""
    w = words(seed, offset, stream, np.arange(n, dtype=np.uint64) + np.uint64(base))
    return (w >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def dropout_threshold(p):
    """(thr, scale): keep iff (word >> 8) >= thr = ceil(p 2^24); kept values times fp32(1 / (1 - p)), both from double."""
    return int(math.ceil(float(p) * 16777216.0)), np.float32(1.0 / (1.0 - float(p)))


def dropout_keep(seed, offset, row_base, layer, p, Bp, P, C):
    """0/1 keep mask [Bp][P][C] (channels-last) of ResBlock ``layer``: element e = ((row_base + b) P + p) C + c of stream
    RNG_STREAM_DROPOUT + layer."""
    thr, _ = dropout_threshold(p)
    e = np.uint64(row_base * P * C) + np.arange(Bp * P * C, dtype=np.uint64)
    w = words(seed, offset, RNG_STREAM_DROPOUT + layer, e)
    return ((w >> np.uint32(8)) >= np.uint32(thr)).astype(np.float32).reshape(Bp, P, C)


def dropout_multiplier(seed, offset, row_base, layer, p, Bp, H, W, C):
    """keep * scale as an NCHW float32 array [Bp][C][H][W] (the oracle's layout)."""
    _, s = dropout_threshold(p)
    k = dropout_keep(seed, offset, row_base, layer, p, Bp, H * W, C)
    return (k * s).reshape(Bp, H, W, C).transpose(0, 3, 1, 2).copy()


def resblock_keys(channel_mult=(1, 2, 4), num_res_blocks=2, attention_resolutions=(2, 4)):
    """{'input_blocks.i.0' | 'middle_block.0' | 'middle_block.2' | 'output_blocks.j.0': layer index} in the order
    input_blocks -> middle_block -> output_blocks (the order of named_modules() and of the embedding bank)."""
    keys, i = [], 1
    for level, _ in enumerate(channel_mult):
        for _ in range(num_res_blocks):
            keys.append(f"input_blocks.{i}.0")
            i += 1
        if level != len(channel_mult) - 1:
            i += 1                                      # Downsample
    keys += ["middle_block.0", "middle_block.2"]
    keys += [f"output_blocks.{j}.0" for j in range(len(channel_mult) * (num_res_blocks + 1))]
    return {k: l for l, k in enumerate(keys)}
