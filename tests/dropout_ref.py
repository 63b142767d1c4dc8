"""Host reference of the regressor dropout mask, written from the specification and
not from csrc/dropout.h: a vectorised numpy Philox4x32-10 and the mask function.  No GPU needed.

  key      (seed_lo, seed_hi)
  counter  (row, quad, call, stream), quad = col // 4; output word i belongs to column 4 quad + i
  keep     word >= T, T = uint32(float64(p) * 2^32), p the float32 rate; p = 0 keeps everything
  scale    s = 1 / (1 - p) in float32; dropped elements are 0
  columns < split use p0, the others p1
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """ctr: 4 arrays (broadcastable), key: 2 arrays; returns 4 uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & _MASK for v in ctr]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _MASK for v in key)
    c = list(np.broadcast_arrays(*c))
    for rnd in range(10):
        if rnd:
            k0 = (k0 + np.uint64(W0)) & _MASK
            k1 = (k1 + np.uint64(W1)) & _MASK
        p0 = c[0] * np.uint64(M0)
        p1 = c[2] * np.uint64(M1)
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _MASK, (p0 >> _S32) ^ c[3] ^ k1, p0 & _MASK]
    return [v.astype(np.uint32) for v in c]


def threshold(p) -> int:
    return int(np.float64(np.float32(p)) * 4294967296.0)


def scale(p) -> np.float32:
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def words(ctr, rows, cols):
    """The (rows, cols) uint32 words of state block ctr = (seed_lo, seed_hi, call, stream)."""
    assert cols % 4 == 0
    seed_lo, seed_hi, call, stream = (int(v) & 0xFFFFFFFF for v in ctr)
    r = np.arange(rows, dtype=np.uint64)[:, None]
    q = np.arange(cols // 4, dtype=np.uint64)[None, :]
    w = philox4x32_10((r, q, call, stream), (seed_lo, seed_hi))
    return np.stack(w, axis=-1).reshape(rows, cols)


def mask(ctr, rows, cols, split, p0, p1):
    """float32 (rows, cols) multiplier: 0 or s."""
    w = words(ctr, rows, cols)
    col = np.arange(cols)[None, :]
    T = np.where(col < split, threshold(p0), threshold(p1)).astype(np.uint64)
    s = np.where(col < split, scale(p0), scale(p1)).astype(np.float32)
    return np.where(w.astype(np.uint64) >= T, s, np.float32(0.0)).astype(np.float32)
