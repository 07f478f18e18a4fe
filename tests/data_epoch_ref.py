"""NumPy restatement of the epoch index rule of msgm_data_gather_epoch (csrc/data_kernels.hip): the data
order is one endless stream of independent permutations of [0, N), position P reads row pi_e(p), e = P // N, p = P % N.
pi_e is a keyed 12-round unbalanced Feistel network on max(8, bit_length(N - 1)) bits with cycle walking, in uint32
arithmetic; its keys are three Philox blocks of stream RNG_STREAM_DATA_PERM at offset 0, so they depend on the seed and
the epoch only.  Used by the tests; the package never imports it."""
import numpy as np

import philox_np as PH

RNG_STREAM_DATA_PERM = 8
ROUNDS = 12
_U32 = np.uint32


def epoch_keys(seed, e):
    """k[0..11] of epoch e: words x, y, z, w of blocks q = 4e + j, j = 0, 1, 2 (uint32 array of 12)."""
    q = (np.uint64(4) * np.uint64(int(e)) + np.arange(3, dtype=np.uint64))
    return PH.msgm_philox(int(seed), 0, RNG_STREAM_DATA_PERM, q).reshape(-1)


def widths(N):
    bits = max(8, int(N - 1).bit_length())
    a = bits // 2
    return a, bits - a


def round_fn(r, k):
    x = (r + k) * _U32(0x9E3779B1)
    x ^= x >> _U32(15)
    x *= _U32(0x85EBCA77)
    x ^= x >> _U32(13)
    x *= _U32(0xC2B2AE3D)
    x ^= x >> _U32(16)
    return x


def feistel_pass(v, keys, a, b):
    """One pass of the network on a uint32 array of values below 2^(a + b)."""
    L, R = v >> _U32(b), v & _U32((1 << b) - 1)
    wl, wr = a, b
    for i in range(ROUNDS):
        L, R = R, L ^ (round_fn(R, keys[i]) & _U32((1 << wl) - 1))
        wl, wr = wr, wl
    return (L << _U32(wr)) | R


def perm_index(seed, e, p, N, walks=None):
    """pi_e(p) for an array p of positions in [0, N) (int64 result).  ``walks`` (a list) receives the passes each took."""
    p = np.asarray(p, dtype=np.int64)
    if N == 1:
        return np.zeros_like(p)
    a, b = widths(N)
    keys = epoch_keys(seed, e)
    with np.errstate(over="ignore"):
        v = feistel_pass(p.astype(_U32), keys, a, b)
        n = np.ones(p.shape, dtype=np.int64)
        while True:
            out = v >= _U32(N)
            if not out.any():
                break
            v[out] = feistel_pass(v[out], keys, a, b)
            n[out] += 1
    if walks is not None:
        walks.append(n)
    return v.astype(np.int64)


def perm_table(seed, epochs, N):
    """pi_e(p) for every e of ``epochs`` and every p < N, an (E, N) int64 array: perm_index vectorised over the epochs."""
    epochs = np.asarray(epochs, dtype=np.uint64).reshape(-1)
    E = epochs.size
    if N == 1:
        return np.zeros((E, 1), dtype=np.int64)
    a, b = widths(N)
    q = (np.uint64(4) * epochs[:, None] + np.arange(3, dtype=np.uint64)[None, :]).reshape(-1)
    keys = np.repeat(PH.msgm_philox(int(seed), 0, RNG_STREAM_DATA_PERM, q).reshape(E, 12), N, axis=0)       # one row per (e, p)
    v = np.tile(np.arange(N, dtype=_U32), E)
    act = np.arange(E * N)
    with np.errstate(over="ignore"):
        while act.size:
            v[act] = feistel_pass(v[act], keys[act].T, a, b)
            act = act[v[act] >= _U32(N)]
    return v.astype(np.int64).reshape(E, N)


def stream_index(seed, P, N):
    """Table rows of the global stream positions P (any integer array, values below 2^63)."""
    P = np.asarray(P, dtype=np.uint64).reshape(-1)
    e, p = P // np.uint64(N), (P % np.uint64(N)).astype(np.int64)
    out = np.empty(P.shape, dtype=np.int64)
    for ee in np.unique(e):
        m = e == ee
        out[m] = perm_index(seed, int(ee), p[m], N)
    return out


def batch_index(seed, cursor, row_base, B, N):
    """idx_out of one msgm_data_gather_epoch call: positions cursor + row_base + b, b < B."""
    return stream_index(seed, np.uint64(int(cursor) + int(row_base)) + np.arange(B, dtype=np.uint64), N)
