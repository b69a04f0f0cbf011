"""Numpy restatement of iwae_binarize's draw, written from csrc/iwae_kernels.h:
Philox4x32-10 on the counter (row, layer << 20 | group, base_lo, base_hi) and
the key (seed_lo, seed_hi) (philox_uniform4), the float32 uniform mapping
u = ((float)c + 0.5f) * 2^-32, and the pixel rule (u < x || x >= 1).  The draw
of output row i, column j is value j % 4 of group j / 4 (iwae_generate's pixel
layout).  Integer arithmetic is exact, the float32 steps are the kernel's, so
the GPU has to match it bit for bit."""
import numpy as np

MAX_LAYERS = 8
LAYER = 2 * MAX_LAYERS + 3          # the binarisation's Philox layer id
SEED = 20240611                     # the seed the GPU tests use (test_binarize_ref.py checks the bounds with it)
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four arrays (or ints) of 32-bit words, key: two; returns four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & np.uint64(MASK) for c in ctr)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c0                        # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return tuple(np.asarray(c).astype(np.uint32) for c in (c0, c1, c2, c3))


def uniform_from_u32(c):
    """((float)c + 0.5f) * 2^-32 in float32 (round to nearest even at every step)."""
    f = np.asarray(c, np.uint32).astype(np.float32)
    return (f + np.float32(0.5)) * np.float32(2.0 ** -32)


def philox_uniforms(seed, base, n, xdim, layer=LAYER):
    """The [n][xdim] uniforms of the call that draws at noise position ``base`` under key ``seed``."""
    ng = (xdim + 3) // 4
    rows = np.repeat(np.arange(n, dtype=np.uint64), ng)
    grps = np.tile(np.arange(ng, dtype=np.uint64), n)
    c1 = np.uint64(layer << 20) | grps
    lo = np.full(n * ng, int(base) & MASK, np.uint64)
    hi = np.full(n * ng, (int(base) >> 32) & MASK, np.uint64)
    words = philox4x32_10((rows, c1, lo, hi), (int(seed) & MASK, (int(seed) >> 32) & MASK))
    u = np.stack([uniform_from_u32(w) for w in words], axis=1)       # [n * ng, 4]
    return u.reshape(n, 4 * ng)[:, :xdim].copy()


def pixel_rule(u, x):
    """(u < x || x >= 1) ? 1.0f : 0.0f; NaN compares false both times."""
    u, x = np.asarray(u, np.float32), np.asarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        return ((u < x) | (x >= np.float32(1.0))).astype(np.float32)


def gather(x, perm):
    """x[perm] with a row of zeros for an index outside [0, len(x))."""
    x = np.asarray(x, np.float32)
    if perm is None:
        return x
    perm = np.asarray(perm, np.int64)
    ok = (perm >= 0) & (perm < len(x))
    out = np.zeros((len(perm), x.shape[1]), np.float32)
    out[ok] = x[perm[ok]]
    return out


def binarize(x, seed, base, perm=None, u=None):
    """What iwae_binarize writes for the call at noise position ``base`` (or with injected ``u``)."""
    xg = gather(x, perm)
    if u is None:
        u = philox_uniforms(seed, base, xg.shape[0], xg.shape[1])
    return pixel_rule(u, xg)
