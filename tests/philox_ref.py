"""Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011; the Random123 library) in plain numpy, and the
two mask rules of csrc/pointwise.hip restated on top of it: dropout_keep (dropout_kernel, the dropout folded into join_fwd_kernel) and
dropout_mask_bytes (dropout_mask_kernel).  Pinned on the CPU to the Random123 known answers (tests/test_exact_bounds.py); the GPU tests
(tests/test_gpu_bnfin_exact.py, tests/test_gpu_bneck_exact.py) hold every mask bit of the kernels to it."""
import functools

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
KEY_XOR = 0x5EED                         # folded into the seed's high word by every mask kernel
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter_words, k0, k1):
    """counter_words [n][4] (32-bit words), key (k0, k1) -> uint32 [n][4].  One round:
    [hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)], then the key is bumped by (W0, W1); ten rounds"""
    c = np.asarray(counter_words, dtype=np.uint64).reshape(-1, 4)
    c0, c1, c2, c3 = (c[:, i].copy() for i in range(4))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2            # 32 x 32 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], 1).astype(np.uint32)


def seed_key(seed):
    """(k0, k1) of a 64-bit seed word: its low half, its high half ^ 0x5EED"""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, (seed >> 32) ^ KEY_XOR


def words_of_counters(ctr, seed):
    """the four output words of the 64-bit counters ctr (in words 0 and 1; words 2 and 3 are 0)"""
    ctr = np.asarray(ctr, dtype=np.uint64)
    cw = np.zeros((ctr.size, 4), dtype=np.uint64)
    cw[:, 0], cw[:, 1] = ctr & _M32, ctr >> _S32
    return philox4x32_10(cw, *seed_key(seed))


@functools.lru_cache(maxsize=8)
def dropout_words(n, seed):
    """the random word of each of n elements: element i uses word i & 3 of counter i >> 2"""
    w = words_of_counters(np.arange((n + 3) // 4, dtype=np.uint64), seed).reshape(-1)[:n]
    w.setflags(write=False)
    return w


def keep_threshold(p):
    """floor(float64(float32(p)) 2^32): an element is kept iff its word is >= this"""
    return int(np.floor(np.float64(np.float32(p)) * 4294967296.0))


def dropout_keep(P, C, p, seed):
    """bool [P][C]: element (pix, c) has the LOGICAL index i = pix C + c -- the pitch of the tensor plays no part"""
    return (dropout_words(P * C, seed) >= np.uint32(keep_threshold(p))).reshape(P, C)


def mask_threshold(p):
    """floor(float64(float32(p)) 65536 + 0.5): a 16-bit half keeps its element iff it is >= this"""
    return int(np.floor(np.float64(np.float32(p)) * 65536.0 + 0.5))


@functools.lru_cache(maxsize=4)
def mask_halves(P, counter):
    """uint16 [P 16][8]: byte b = pix 16 + v has the counter b; its bit j looks at half (j & 1) of output word j >> 1"""
    w = words_of_counters(np.arange(P * 16, dtype=np.uint64), counter)
    h = np.stack([(w[:, j >> 1] >> np.uint32(16 * (j & 1))) & np.uint32(0xFFFF) for j in range(8)], 1).astype(np.uint16)
    h.setflags(write=False)
    return h


def dropout_mask_bytes(P, p, counter):
    """uint8 [P][16]: all 16 bytes of a pixel, whatever the channel count"""
    kept = mask_halves(P, counter) >= np.uint32(mask_threshold(p))
    return (kept.astype(np.uint8) << np.arange(8, dtype=np.uint8)).sum(1).astype(np.uint8).reshape(P, 16)
