"""numpy restatement of the decoder dropout's mask: Philox4x32-10 keyed by the 64-bit seed, counter
{col >> 2, h * rows + i, sample, site_code}, element (h, i, col) kept iff word (col & 3) >= floor(p 2^32)."""
import numpy as np

M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: uint32 array [..., 4]; key: (k0, k1).  Returns uint32 [..., 4]."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0, k1 = np.uint32(key[0]), np.uint32(key[1])
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0, k1 = np.uint32(k0 + W0), np.uint32(k1 + W1)
            p0, p1 = M0 * c[0], M1 * c[2]
            hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK32, p1 >> np.uint64(32), p1 & MASK32
            c = [(hi1 ^ c[1] ^ np.uint64(k0)) & MASK32, lo1, (hi0 ^ c[3] ^ np.uint64(k1)) & MASK32, lo0]
    return np.stack(c, -1).astype(np.uint32)


def threshold(p):
    t = np.floor(np.float64(np.float32(p)) * 4294967296.0)
    return np.uint32(min(t, 4294967295.0))


def scale(p):
    """1 / (1 - p) as the kernels compute it (fp32)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_mask(seed, sample, site_code, p, heads, rows, cols):
    """uint8 [heads, rows, cols], 1 = kept."""
    seed = int(seed) & (2 ** 64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    r = np.arange(heads * rows, dtype=np.uint64)
    c4 = np.arange((cols + 3) // 4, dtype=np.uint64)
    ctr = np.zeros((heads * rows, len(c4), 4), np.uint64)
    ctr[..., 0] = c4[None, :]
    ctr[..., 1] = r[:, None]
    ctr[..., 2] = sample
    ctr[..., 3] = site_code
    words = philox4x32_10(ctr, key).reshape(heads * rows, -1)[:, :cols]
    return (words >= threshold(p)).astype(np.uint8).reshape(heads, rows, cols)
