"""numpy restatement of the dropout generator contract (csrc/dropout_rng.h), independent of the library:

  key     = (seed low 32 bits, seed high 32 bits)
  counter = (b low 32, b high 32, site, step low 32)  with b = e >> 2; element e takes word e & 3 of that block
  keep    = word >= thr,  thr = floor(p * 2^32 + 0.5);  kept elements are multiplied by 1 / (1 - p)
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """ctr: four uint arrays (or ints) of one shape, key: two -> uint32 array [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & MASK32 for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK32, int(key[1]) & MASK32
    for _ in range(10):
        p0 = c[0] * np.uint64(M0)  # 32 x 32 -> 64 bits: exact in uint64
        p1 = c[2] * np.uint64(M1)
        hi0, lo0 = p0 >> np.uint64(32), p0 & MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & MASK32
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack(c, -1).astype(np.uint32)


def threshold(p):
    """(thr, scale) as the host computes them: thr in double, scale rounded to fp32."""
    assert 0.0 <= p < 1.0
    return min(int(np.floor(p * 4294967296.0 + 0.5)), MASK32), float(np.float32(1.0 / (1.0 - p)))


def words(seed, step, site, e):
    """The generator's 32-bit word of every element index in `e` (any shape, python ints or uint64)."""
    e = np.asarray(e, dtype=np.uint64)
    b = e >> np.uint64(2)
    out = philox4x32_10((b & MASK32, b >> np.uint64(32), int(site), int(step) & MASK32),
                        (int(seed) & MASK32, (int(seed) >> 32) & MASK32))
    return np.take_along_axis(out, (e & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]


def keep(seed, step, site, e, thr):
    return (words(seed, step, site, e) >= np.uint32(thr)).astype(np.uint8)


def keep_flat(seed, step, site, n, thr, e0=0):
    """Elementwise sites: elements e0 .. e0 + n - 1 of a flat row-major tensor."""
    return keep(seed, step, site, np.uint64(e0) + np.arange(n, dtype=np.uint64), thr)


def keep_attn(seed, step, site, r, h, l, thr):
    """Attention probabilities: [R, H, L, L] mask, element ((r*H + h)*L + i)*Lp + j with Lp = (L + 3) & ~3."""
    lp = (l + 3) & ~3
    row = np.arange(r * h * l, dtype=np.uint64).reshape(r, h, l, 1) * np.uint64(lp)
    return keep(seed, step, site, row + np.arange(l, dtype=np.uint64), thr)
