"""numpy restatement of the sampler's counter-based uniform stream documented in include/omlm.h (no GPU, no library).

    s0        = h(h(seed_lo) ^ seed_hi)                       seed = seed_hi * 2^32 + seed_lo, h = lowbias32, uint32 arithmetic
    key(t, b) = h(h(s0 + t * 0x9E3779B9) ^ (b * 0x85EBCA6B))  t: index of the sampled id within the call, b: global sample index
    r(t,b,c)  = h(key(t, b) ^ (c * 0x9E3779B9))               c: logit index
    u(t,b,c)  = (r >> 8) * 2^-24
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
GOLD = np.uint64(0x9E3779B9)
MIXB = np.uint64(0x85EBCA6B)


def hash32(x):
    """lowbias32 on uint32 values held in uint64 arrays (masked after every multiply)."""
    x = np.asarray(x, dtype=np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & M32
    x = x ^ (x >> np.uint64(16))
    return x


def words(seed, steps, B, V, row0=0, t0=0):
    """r(t, b, c) as uint64 [steps, B, V] (values < 2^32) for t = t0 .. t0 + steps - 1, b = row0 .. row0 + B - 1, c = 0 .. V - 1."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    s0 = hash32(hash32(lo) ^ hi)
    t = (np.arange(steps, dtype=np.uint64) + np.uint64(t0))[:, None]
    b = (np.arange(B, dtype=np.uint64) + np.uint64(row0))[None, :]
    key = hash32(hash32((s0 + ((t * GOLD) & M32)) & M32) ^ ((b * MIXB) & M32))                  # [steps, B]
    c = np.arange(V, dtype=np.uint64)[None, None, :]
    return hash32(key[:, :, None] ^ ((c * GOLD) & M32))


def uniforms(seed, steps, B, V, row0=0, t0=0):
    """u(t, b, c) as float32 [steps, B, V]: multiples of 2^-24 in [0, 1), exact in float32."""
    return ((words(seed, steps, B, V, row0, t0) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
