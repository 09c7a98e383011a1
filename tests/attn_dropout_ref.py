"""numpy restatement of the attention-dropout keep-masks documented in include/omlm.h (no GPU, no library)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHI64 = 0x9E3779B97F4A7C15


def hash32(x):
    """lowbias32 on uint32 arrays (uint64 arithmetic, masked)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def salted(seed, salt=None):
    s = int(seed)
    if salt is not None:
        s = (s + int(salt) * PHI64) & 0xFFFFFFFFFFFFFFFF
    return np.uint64(s & 0xFFFFFFFF), np.uint64(s >> 32)


def _keep(w, j, p):
    draw = np.where((j & 1) == 1, w >> np.uint64(16), w & np.uint64(0xFFFF))
    return draw >= np.uint64(int(p * 65536.0 + 0.5))


def attn_keep(B, N, H, p, seed, salt=None, b0=0, h0=0, i0=0, j0=0):
    """keep [B, H, N, N] bool of probabilities (b, h, i, j) (offsets b0 / h0 / i0 / j0 shift the coordinates)."""
    lo, hi = salted(seed, salt)
    b = np.arange(B, dtype=np.uint64)[:, None, None, None] + np.uint64(b0)
    h = np.arange(H, dtype=np.uint64)[None, :, None, None] + np.uint64(h0)
    i = np.arange(N, dtype=np.uint64)[None, None, :, None] + np.uint64(i0)
    j = np.arange(N, dtype=np.uint64)[None, None, None, :] + np.uint64(j0)
    hk = hash32((hash32(hash32(lo ^ b) ^ hi) + h) & M32)
    w = hash32(hk ^ ((i << np.uint64(15)) & M32) ^ (j >> np.uint64(1)))
    return _keep(w, j, p)


def resid_keep(M, D, p, seed, salt=None):
    """keep [M, D] bool of the to_out dropout (row, column)."""
    lo, hi = salted(seed, salt)
    r = np.arange(M, dtype=np.uint64)[:, None]
    c = np.arange(D, dtype=np.uint64)[None, :]
    rk = hash32(hash32(lo ^ (r & M32)) ^ hi)
    w = hash32(rk ^ (c >> np.uint64(1)))
    return _keep(w, c, p)
