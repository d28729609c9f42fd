"""gaq_perm_dev's formula (include/gaq.h "shuffled minibatches") restated in NumPy unsigned integers: the reference the device kernel
is compared with bit for bit, and what a checkpoint or another rank would run to reproduce a permutation."""
import numpy as np

ROUNDS = 8
STREAM = 140                      # quad_core.hpp RNG_PERM
M0, M1 = 0xD2511F53, 0xCD9E8D57   # Philox's multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85   # Philox's key increments
_U32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al. 2011) of one block, plain Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> 4 words"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _U32, (p0 >> 32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + W0) & _U32, (k1 + W1) & _U32
    return c0, c1, c2, c3


def round_keys(seed, epoch):
    seed, epoch = int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1)
    keys = []
    for j in range(ROUNDS // 4):
        keys += philox4x32_10((epoch & _U32, (epoch >> 32) ^ ((STREAM << 24) & _U32), j, 0), (seed & _U32, seed >> 32))
    return keys


def half_bits(n):
    """h = b / 2, b the smallest even number >= max(2, ceil(log2 n))"""
    b = 2
    while (1 << b) < n:
        b += 2
    return b // 2


def feistel(x, h, keys):
    """P(x) for a uint64 array x < 2^(2 h)"""
    mask = np.uint64((1 << h) - 1)
    u32, s32, sh = np.uint64(_U32), np.uint64(32), np.uint64(h)
    L, R = x >> sh, x & mask
    for r in range(ROUNDS):
        p = np.uint64(M0) * (R ^ np.uint64(keys[r]))              # < 2^64: both factors are below 2^32
        q = np.uint64(M1) * ((p >> s32) ^ (p & u32))
        f = ((q >> s32) ^ (q & u32)) >> np.uint64(32 - h)
        L, R = R, L ^ f
    return (L << sh) | R


def perm_ref(n, seed, epoch=0):
    """idx_out of gaq_perm_dev(n, seed, epoch): int32 [n]"""
    n = int(n)
    assert 1 <= n <= 2 ** 31 - 1
    h, keys = half_bits(n), round_keys(seed, epoch)
    x = feistel(np.arange(n, dtype=np.uint64), h, keys)
    while True:                                                   # cycle walking: ends because P is a bijection (gaq.h)
        big = x >= np.uint64(n)
        if not big.any():
            return x.astype(np.int32)
        x[big] = feistel(x[big], h, keys)
