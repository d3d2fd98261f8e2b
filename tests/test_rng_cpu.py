"""The host reference of the device RNG (tests/philox_ref.py) checked on its own: the Random123 known-answer vectors of
Philox4x32-10, and the properties that the GPU comparisons (tests/test_rng_gpu.py) lean on."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref as P  # noqa: E402

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in P.philox4x32_10(ctr, key)) == want, (ctr, key)
    # vectorised over the counter: the three vectors as one call
    got = P.philox4x32_10([np.array([k[0][j] for k in KAT]) for j in range(4)], [np.array([k[1][j] for k in KAT]) for j in range(2)])
    assert np.array_equal(np.stack(got, 1), np.array([k[2] for k in KAT], dtype=np.uint32))


def test_stream_layout_is_the_known_answer_generator():
    """words(): counter (lo32 i, hi32 i, lo32 off, hi32 off), key (lo32 seed, hi32 seed) -- the third vector read as a stream"""
    ctr, key, want = KAT[2]
    i, off, seed = ctr[0] | ctr[1] << 32, ctr[2] | ctr[3] << 32, key[0] | key[1] << 32
    # call i of the stream is too far to enumerate: the layout is checked at i < 3 against the generator itself
    w = P.words(3, seed, off)
    for j in range(3):
        assert tuple(w[j]) == P.philox4x32_10((j, 0, ctr[2], ctr[3]), key)
    assert tuple(int(v) for v in P.philox4x32_10((i & 0xffffffff, i >> 32, off & 0xffffffff, off >> 32), (seed & 0xffffffff, seed >> 32))) == want
    # int64 state bits: a negative int64 is its 64-bit pattern
    assert np.array_equal(P.words(2, -1, -1), P.words(2, 2 ** 64 - 1, 2 ** 64 - 1))


def test_uniform_and_labels_ranges():
    u = P.uniform(100003, 5, 9)
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert P.u01(np.uint32(0xffffffff)) == np.float32(1 - 2.0 ** -24) and P.u01(np.uint32(0xff)) == 0.0
    for n_labels in (1, 10, 1000, 16777217):
        lb = P.labels(100003, n_labels, 5, 9)
        assert lb.dtype == np.int32 and lb.min() >= 0 and lb.max() <= n_labels - 1
    assert np.array_equal(np.bincount(P.labels(4096, 1, 1, 0)), [4096])


def test_normal_is_finite_where_the_uniform_is_zero(monkeypatch):
    """u01 = 0 -> u1 = 1 -> r = 0: the draw is 0, not NaN or inf; and the largest uniform gives the largest radius, 5.77"""
    for word, radius in ((0, 0.0), (0xffffffff, np.sqrt(-2 * np.log(2.0 ** -24)))):
        monkeypatch.setattr(P, "words", lambda n, seed, off, word=word: np.full((n, 4), word, dtype=np.uint32))
        z = P.normal64(7, 0, 0)
        assert z.shape == (7,) and np.isfinite(z).all()
        assert np.allclose(np.hypot(z[0], z[1]), radius, rtol=1e-12, atol=0) and np.abs(z).max() <= 5.8


def test_normal_moments_and_pairing():
    z = P.normal64(1 << 18, 3, 1)
    assert abs(z.mean()) < 0.01 and abs(z.std() - 1) < 0.01
    u = P.u01(P.words(4, 3, 1)).astype(np.float64)
    assert np.allclose(np.hypot(z[0], z[1]) ** 2, -2 * np.log(1 - u[0, 0])) and np.allclose(np.arctan2(z[1], z[0]) % (2 * np.pi), 2 * np.pi * u[0, 1])
    assert np.allclose(np.hypot(z[14], z[15]) ** 2, -2 * np.log(1 - u[3, 2])) and np.allclose(np.arctan2(z[15], z[14]) % (2 * np.pi), 2 * np.pi * u[3, 3])


def test_cos_sin_of_whole_turns_keep_their_zeros():
    u = np.concatenate([np.arange(0, 1 << 24, 4099), [1 << 22, 1 << 23, 3 << 22, (1 << 22) + 1, (1 << 23) - 1, (1 << 24) - 1]]) * 2.0 ** -24
    c, s = P.cos_sin_2pi(u)
    assert np.abs(c - np.cos(2 * np.pi * u)).max() < 1e-15 and np.abs(s - np.sin(2 * np.pi * u)).max() < 1e-15
    assert np.abs(c * c + s * s - 1).max() < 1e-15
    assert tuple(P.cos_sin_2pi(np.array([0, .25, .5, .75]))[0]) == (1, 0, -1, 0) and tuple(P.cos_sin_2pi(np.array([0, .25, .5, .75]))[1]) == (0, 1, 0, -1)
    # one step past a quarter turn: -sin(2 pi 2^-24), to full relative accuracy
    assert abs(P.cos_sin_2pi(np.array([.25 + 2.0 ** -24]))[0][0] / -np.sin(2 * np.pi * 2.0 ** -24) - 1) < 1e-15


def test_prefix_of_a_long_draw_is_the_short_draw():
    for n in (1, 2, 3, 4, 5, 7, 1027):
        assert np.array_equal(P.uniform(4099, 11, 2)[:n], P.uniform(n, 11, 2))
        assert np.array_equal(P.labels(4099, 10, 11, 2)[:n], P.labels(n, 10, 11, 2))
        assert np.array_equal(P.normal64(4099, 11, 2)[:n], P.normal64(n, 11, 2))


def test_offsets_and_seeds_share_no_output():
    base = P.words(4096, 7, 0)
    seen = set(base.reshape(-1).tolist())
    for seed, off in ((7, 1), (7, 2), (7, 1 << 32), (8, 0), (7 + (1 << 32), 0)):
        other = P.words(4096, seed, off)
        assert not (other == base).any()                                        # no word repeats in place
        assert len(seen & set(other.reshape(-1).tolist())) <= 2                 # 16384 of 2^32 values twice: 0.06 expected by chance


def test_bf16_rounding_matches_torch():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.normal(size=50000).astype(np.float32), (rng.normal(size=50000) * 10.0 ** rng.integers(-30, 30, 50000)).astype(np.float32),
                        rng.integers(0, 2 ** 32, 50000, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    # ties: exactly half way between two bfloat16 values, after an even and after an odd one; and the edges
    ties = (np.arange(0x3f80, 0x3f90, dtype=np.uint32) << 16 | 0x8000).view(np.float32)
    edge = np.array([0.0, -0.0, np.inf, -np.inf, 3.3895314e38, 3.4e38, 1e-45, 9.2e-41, 4.6e-41, -4.6e-41], dtype=np.float32)
    x = np.concatenate([x, ties, -ties, edge])
    x = x[~np.isnan(x)]
    want = torch.from_numpy(x).to(torch.bfloat16)
    assert np.array_equal(P.bf16_bits(x).view(np.int16), want.view(torch.int16).numpy())
    assert np.array_equal(P.bf16_round(x).view(np.uint32), want.to(torch.float32).numpy().view(np.uint32))
    assert np.isnan(P.bf16_round(np.array([np.nan], dtype=np.float32))).all()
    assert np.array_equal(P.fp16_bits(x).view(np.int16), torch.from_numpy(x).to(torch.float16).view(torch.int16).numpy())
    assert np.array_equal(P.fp16_round(x).view(np.uint32), torch.from_numpy(x).to(torch.float16).to(torch.float32).numpy().view(np.uint32))


def test_preprocess_layout_and_range():
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, (3, 3072), dtype=np.uint8)
    y = P.preprocess(data, 42, 0)
    assert y.shape == (3, 32, 32, 3) and y.dtype == np.float32
    base = 2 * (data.reshape(3, 3, 32, 32).transpose(0, 2, 3, 1) / 256.0 - .5)          # CHW rows -> HWC
    d = y - base
    assert d.min() >= -2.0 ** -9 and d.max() <= 1 / 128 + 2.0 ** -9                      # U[0, 1/128) and half a bf16 ulp at |x| <= 1
    assert np.array_equal(P.bf16_round(y), y)
    noise = (P.preprocess(data, 42, 0, rounding=lambda v: v) - base.astype(np.float32)).reshape(-1)
    assert np.allclose(noise, P.uniform(3 * 3072, 42, 0) / 128, atol=2.0 ** -24, rtol=0)


def test_dropout_takes_word_zero_of_one_call_per_element():
    x = np.linspace(-3, 3, 1027, dtype=np.float32)
    x = P.bf16_round(x)
    for keep in (0.5, 0.8, 1.0):
        y, m = P.dropout(x, keep, 9, 4)
        assert np.array_equal(m, (P.u01(P.words(1027, 9, 4)[:, 0]) < np.float32(keep)).astype(np.uint8))
        assert np.array_equal(y[m == 0], np.zeros(int((m == 0).sum()), np.float32)) and np.array_equal(P.bf16_round(y), y)
        assert np.allclose(y[m == 1], x[m == 1] / keep, rtol=2.0 ** -8)
        assert abs(m.mean() - keep) < 0.05
    assert P.dropout(x, 1.0, 9, 4)[1].all() and np.array_equal(P.dropout(x, 1.0, 9, 4)[0], x)


def test_documented_increments():
    assert P.DRAW_ADVANCE == 1 and P.generator_feed_advance(True) == 2 and P.generator_feed_advance(False) == 1
