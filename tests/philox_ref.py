"""Host reference of the device RNG ("Device RNG contract"): Philox4x32-10 and what every consumer of the stream must
produce, in numpy alone (plain uint64 arithmetic, vectorised over the counter).  No torch, no GPU.

  state          int64[2] {seed, offset}; a draw reads both and leaves offset + 1 (generator_feed with labels: offset + 2)
  4-group i      counter (lo32(i), hi32(i), lo32(offset), hi32(offset)), key (lo32(seed), hi32(seed)); element 4i + e takes word e
  u01(w)         (w >> 8) * 2**-24, in [0, 1)

philox4x32_10 is the standard generator (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123): the
known-answer vectors of that library are in tests/test_rng_cpu.py.
"""
import functools

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
MASK64 = (1 << 64) - 1


def philox4x32_10(ctr4, key2):
    """ctr4: four words, key2: two words (ints or equally shaped integer arrays, each < 2**32) -> the four output words (uint32)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr4)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key2)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                     # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & LO, (p0 >> S32) ^ c3 ^ k1, p0 & LO
        k0, k1 = (k0 + W0) & LO, (k1 + W1) & LO       # bumped after every round
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def words(n_calls, seed, off):
    """uint32 [n_calls, 4], read-only: Philox call i of the draw at `off` of the stream `seed` (both taken as 64-bit patterns).
    The last few results are kept: the consumers of one draw share its words."""
    return _words(int(n_calls), int(seed) & MASK64, int(off) & MASK64)


@functools.lru_cache(maxsize=6)
def _words(n_calls, seed, off):
    i = np.arange(n_calls, dtype=np.uint64)
    w = np.stack(philox4x32_10((i & LO, i >> S32, off & 0xFFFFFFFF, off >> 32), (seed & 0xFFFFFFFF, seed >> 32)), axis=1)
    w.setflags(write=False)
    return w


def u01(w):
    """float32 in [0, 1): the upper 24 bits (exact)"""
    return (np.asarray(w, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _elements(n, seed, off):
    return words((n + 3) // 4, seed, off).reshape(-1)[:n]


# ---- 16-bit roundings --------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """float32 -> the bfloat16 bit pattern (uint16), round to nearest even; NaN stays a (quiet) NaN"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    return np.where(np.isnan(x), ((b >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16), r)


def bf16_round(x):
    """float32 -> the nearest bfloat16 value (ties to even), as float32"""
    return (bf16_bits(x).astype(np.uint32) << np.uint32(16)).view(np.float32)


def bf16_bits64(x):
    """float64 -> the bfloat16 bit pattern, ONE rounding: where the float32 on the way is an exact tie of two bfloat16 values, the side
    on which the float64 lies decides, not the even neighbour"""
    x = np.asarray(x, dtype=np.float64)
    f = x.astype(np.float32)
    b = f.view(np.uint32)
    tie = (b & np.uint32(0xFFFF)) == np.uint32(0x8000)
    down = (b >> np.uint32(16)).astype(np.uint16)                  # truncated: the neighbour towards zero
    away = np.abs(x) > np.abs(f.astype(np.float64))
    toward = np.abs(x) < np.abs(f.astype(np.float64))
    return np.where(tie & away, down + np.uint16(1), np.where(tie & toward, down, bf16_bits(f)))


def bits_value(bits):
    """bfloat16 bit pattern -> float64"""
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def ordinal(bits):
    """16-bit sign-magnitude pattern (bfloat16 or half) -> its position on the number line: neighbours differ by 1, -0 = +0"""
    b = np.asarray(bits, dtype=np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def fp16_bits(x):
    with np.errstate(over="ignore"):                # beyond 65504 the cast gives inf, as the device's conversion does
        return np.asarray(x, dtype=np.float32).astype(np.float16).view(np.uint16)


def fp16_round(x):
    """float32 -> the nearest IEEE half value (ties to even), as float32"""
    return fp16_bits(x).view(np.float16).astype(np.float32)


# ---- one function per consumer ---------------------------------------------------------------------------------------------------
def uniform(n, seed, off):
    """gank_rng_uniform_f32: float32 [n], exact"""
    return u01(_elements(n, seed, off))


def labels(n, n_labels, seed, off):
    """gank_rng_labels: int32 [n] = min(int(u * n_labels), n_labels - 1), the product in float32; exact"""
    lb = (u01(_elements(n, seed, off)) * np.float32(n_labels)).astype(np.int32)
    return np.minimum(lb, np.int32(n_labels - 1))


def normal64(n, seed, off):
    """gank_rng_normal_bf16 before its rounding, in float64 [n]: Box-Muller on the uniforms of a group, u1 = 1 - u01(x), u2 = u01(y)
    -> r1 cos(2 pi u2), r1 sin(2 pi u2); u3 = 1 - u01(z), u4 = u01(w) -> r3 cos(2 pi u4), r3 sin(2 pi u4); r = sqrt(-2 ln u)"""
    u = u01(words((n + 3) // 4, seed, off)).astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(1.0 - u[:, 0])), np.sqrt(-2.0 * np.log(1.0 - u[:, 2]))
    (ca, sa), (cb, sb) = cos_sin_2pi(u[:, 1]), cos_sin_2pi(u[:, 3])
    return np.stack([ra * ca, ra * sa, rb * cb, rb * sb], axis=1).reshape(-1)[:n]


def cos_sin_2pi(u):
    """(cos(2 pi u), sin(2 pi u)) in float64 for u = k * 2**-24 in [0, 1), accurate RELATIVE to the result next to the zeros too:
    the quarter turns are taken off exactly, where np.cos(2 * np.pi * u) rounds the angle first and returns 6e-17 at u = 1/4"""
    u = np.asarray(u, dtype=np.float64)
    q = np.rint(4.0 * u)                                 # nearest quarter turn, 0..4
    f = 2.0 * np.pi * (u - q / 4.0)                      # exact difference, |f| <= pi / 4
    c, s = np.cos(f), np.sin(f)
    q = q.astype(np.int64) & 3
    return np.choose(q, [c, -s, -c, s]), np.choose(q, [s, c, -s, -c])


def preprocess(data_u8, seed, off, rounding=bf16_round):
    """gank_preprocess_real / the real half of gank_critic_feed: uint8 CHW rows [B, 3072] -> [B, 32, 32, 3] (HWC), output element o
    (flattened) = rounding(float32(2 * (px / 256 - .5) + u01 * (1 / 128))) with the uniform of stream element o.  Exact: every product is by
    a power of two, so the float32 sum is the only rounding before the 16-bit one."""
    data_u8 = np.asarray(data_u8)
    b = data_u8.shape[0]
    assert data_u8.dtype == np.uint8 and data_u8.shape == (b, 3072)
    px = data_u8.reshape(b, 3, 1024).transpose(0, 2, 1).reshape(-1).astype(np.float32)      # o -> data[b, c * 1024 + hw]
    v = np.float32(2) * (px / np.float32(256) - np.float32(.5)) + uniform(b * 3072, seed, off) * np.float32(1 / 128)
    assert v.dtype == np.float32
    return rounding(v).reshape(b, 32, 32, 3)


def dropout(x, keep, seed, off, rounding=bf16_round):
    """gank_dropout_fwd: x holds 16-bit values (any float array) -> (y float32 of 16-bit values, mask uint8).  Element i takes word 0
    of Philox call i -- one call per ELEMENT, unlike the draws above."""
    x = np.asarray(x, dtype=np.float32)
    u = u01(words(x.size, seed, off)[:, 0]).reshape(x.shape)
    mask = u < np.float32(keep)
    y = np.where(mask, rounding(x * (np.float32(1) / np.float32(keep))), np.float32(0))
    return y.astype(np.float32), mask.astype(np.uint8)


# ---- offsets -----------------------------------------------------------------------------------------------------------------------
DRAW_ADVANCE = 1                    # rng_normal, rng_labels, rng_uniform, preprocess_real, critic_feed, dropout_fwd


def generator_feed_advance(with_labels):
    """labels at off and noise at off + 1, or the noise alone at off"""
    return 2 if with_labels else 1
