"""Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in numpy, and the
float64 Box-Muller that gsrt_normal_noise's float32 one is held to. Plain numpy, no library code."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: (..., 4) uint32, key: (..., 2) uint32 (broadcast against the counters); returns (..., 4) uint32"""
    c = np.array(counter, dtype=np.uint32, copy=True)
    k = np.broadcast_to(np.asarray(key, np.uint32), c.shape[:-1] + (2,))
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & MASK).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & MASK).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
            k0 = (k0 + W0).astype(np.uint32)
            k1 = (k1 + W1).astype(np.uint32)
    return np.stack([c0, c1, c2, c3], axis=-1)


# the known-answer vectors of Random123 (kat_vectors: philox4x32 10): counter, key, output
KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def words(seed, stream_id, first_block, blocks):
    """gsrt_normal_noise's blocks: key (seed lo, seed hi), counter (j lo, j hi, stream_id, 0); (blocks, 4) uint32"""
    j = np.uint64(first_block) + np.arange(blocks, dtype=np.uint64)
    ctr = np.stack([(j & MASK).astype(np.uint32), (j >> np.uint64(32)).astype(np.uint32),
                    np.full(blocks, stream_id, np.uint32), np.zeros(blocks, np.uint32)], axis=-1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


def normal_f64(seed, stream_id, count):
    """gsrt_normal_noise's values with the Box-Muller step in float64 from the same words: ua and ub are exact in float64
    up to the float32 rounding of (x >> 8) + 0.5, which is applied (it is part of the definition: it decides the value of
    u, not its error)"""
    blocks = (count + 3) // 4
    w = words(seed, stream_id, 0, blocks)
    out = np.zeros((blocks, 4), np.float64)
    for a in (0, 2):
        ua = ((w[:, a] >> np.uint32(8)).astype(np.float32) + np.float32(0.5)).astype(np.float64) * 2.0 ** -24
        ub = ((w[:, a + 1] >> np.uint32(8)).astype(np.float32) + np.float32(0.5)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(ua))
        th = float(np.float32(6.2831855)) * ub
        out[:, a], out[:, a + 1] = r * np.cos(th), r * np.sin(th)
    return out.reshape(-1)[:count]
