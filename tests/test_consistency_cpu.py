"""Properties of tests/consistency_ref.py itself, the restatement the GPU tests of consistency regularisation compare against, and the
constructor checks of ACGANTrainer(consistency=...).  No GPU."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consistency_ref as R  # noqa: E402
import philox_ref as P  # noqa: E402

SEED, OFF = 0x1234_5678_9ABC_DEF0, 11          # the state of the GPU draw tests (tests/test_consistency_gpu.py)


def ramp(shape):
    return np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)


SHAPES = [(1, 32, 32, 3), (3, 32, 32, 3), (2, 8, 8, 3), (2, 5, 7, 4)]


@pytest.mark.parametrize("shape", SHAPES)
def test_zero_table_is_the_identity(shape):
    x = ramp(shape)
    assert np.array_equal(R.augment(x, np.zeros((shape[0], 3), np.int32)), x)


@pytest.mark.parametrize("shape", SHAPES)
def test_flipping_twice_is_the_identity(shape):
    x = ramp(shape)
    t = np.tile(np.array([[1, 0, 0]], np.int32), (shape[0], 1))
    once = R.augment(x, t)
    assert np.array_equal(once, x[:, :, ::-1]) and not np.array_equal(once, x)
    assert np.array_equal(R.augment(once, t), x)


@pytest.mark.parametrize("shape", SHAPES)
def test_shift_is_reflect_pad_then_crop(shape):
    """a shift by (dx, dy) is np.pad(mode='reflect') by s on every side and the window that starts at (s - dy, s - dx); with a flip, that
    window mirrored left to right (out[x] = in[R(W - 1 - x - dx)]: the shifted image, flipped -- which is the flipped image shifted by
    -dx, and dx is drawn symmetrically).  Every shift up to s = min(H, W) - 1 in both axes."""
    x = ramp(shape)
    b, h, w, _ = shape
    s = min(h, w) - 1
    padded = np.pad(x, ((0, 0), (s, s), (s, s), (0, 0)), mode='reflect')
    flipped = np.pad(x[:, :, ::-1], ((0, 0), (s, s), (s, s), (0, 0)), mode='reflect')
    for dx, dy in itertools.product(sorted({-s, -1, 0, 1, s}), repeat=2):
        window = padded[:, s - dy:s - dy + h, s - dx:s - dx + w]
        for flip, want in ((0, window), (1, window[:, :, ::-1])):
            t = np.tile(np.array([[flip, dx, dy]], np.int32), (b, 1))
            assert np.array_equal(R.augment(x, t), want), (flip, dx, dy)
        assert np.array_equal(window[:, :, ::-1], flipped[:, s - dy:s - dy + h, s + dx:s + dx + w])


def test_rows_of_a_batch_take_their_own_table_row():
    x = ramp((3, 5, 7, 2))
    t = np.array([[0, 2, -1], [1, 0, 0], [1, -3, 4]], np.int32)
    out = R.augment(x, t)
    for i in range(3):
        assert np.array_equal(out[i:i + 1], R.augment(x[i:i + 1], t[i:i + 1]))


def test_reflection_is_undefined_from_the_size_on():
    with pytest.raises(AssertionError):
        R.augment(ramp((1, 4, 6, 1)), np.array([[0, 0, 4]], np.int32))


@pytest.mark.parametrize("n,s", [(1, 1), (7, 4), (64, 4), (4096, 1)])
def test_draw_table_ranges_and_words(n, s):
    t = R.draw_table(n, s, SEED, OFF)
    assert t.shape == (n, 3) and t.dtype == np.int32
    assert set(np.unique(t[:, 0])) <= {0, 1} and int(t[:, 1:].min()) >= -s and int(t[:, 1:].max()) <= s
    w = P.words(n, SEED, OFF).astype(np.int64)
    m = 2 * s + 1
    assert np.array_equal(t[:, 0], w[:, 0] // 2 ** 31)
    assert np.array_equal(t[:, 1], w[:, 1] * m // 2 ** 32 - s) and np.array_equal(t[:, 2], w[:, 2] * m // 2 ** 32 - s)
    assert not np.array_equal(t, R.draw_table(n, s, SEED, OFF + R.DRAW_ADVANCE))


def test_every_outcome_occurs_in_4096_rows():
    """the condition of the GPU test: over 4096 rows at s = 1 each of the 2 (2 s + 1)^2 = 18 outcomes occurs, for the seed used there"""
    t = R.draw_table(4096, 1, SEED, OFF)
    assert len({tuple(r) for r in t.tolist()}) == 18


def test_multiply_high_map_is_unbiased_to_one_word():
    """of the 2^32 words either floor or ceil(2^32 / m) go to each value: the first word of value v is ceil(v 2^32 / m)"""
    for m in (3, 9, 63):
        first = np.array([-(-v * 2 ** 32 // m) for v in range(m + 1)], dtype=np.int64)
        assert np.array_equal(R.mulhi(first[:-1], m), np.arange(m)) and np.array_equal(R.mulhi(first[1:] - 1, m), np.arange(m))
        sizes = np.diff(first)
        assert int(sizes.max()) - int(sizes.min()) <= 1


@pytest.mark.parametrize("b,c", [(1, 1), (8, 1), (7, 10)])
def test_loss_gradients_agree_with_central_differences(b, c):
    rng = np.random.default_rng(b * 16 + c)
    a, bb = rng.normal(size=(b, c)), rng.normal(size=(b, c))
    w = 10.0
    loss, da, db = R.loss_and_grads(a, bb, w)
    assert loss == pytest.approx(w * ((a - bb) ** 2).sum(axis=1).mean(), rel=1e-14)
    assert np.array_equal(db, -da)
    h = 1e-6
    for which, g in ((0, da), (1, db)):
        num = np.empty_like(g)
        for idx in np.ndindex(*g.shape):
            hi, lo = [a.copy(), bb.copy()], [a.copy(), bb.copy()]
            hi[which][idx] += h
            lo[which][idx] -= h
            num[idx] = (R.loss_and_grads(*hi, w)[0] - R.loss_and_grads(*lo, w)[0]) / (2 * h)
        assert np.abs(num - g).max() <= 1e-8 * max(1.0, np.abs(g).max())          # (a quadratic: central differences are exact up to rounding)
    zero = R.loss_and_grads(a, a, w)
    assert zero[0] == 0.0 and not zero[1].any() and not zero[2].any()


def test_rounding_counts():
    assert R.loss_roundings(1) == R.loss_roundings(64) == R.loss_roundings(256) == 14
    assert R.loss_roundings(640) == 16 and R.GRAD_ROUNDINGS == 3
    assert R.gamma(16) < 17 * 2.0 ** -24


# ------------------------------------------------------------------ the constructor's checks (raised before any device work)
def test_check_consistency_errors_without_a_gpu():
    from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer, check_consistency
    assert check_consistency('none', None, None) == (0.0, 0.0)
    assert check_consistency('cr', 10.0, 4) == (10.0, 10.0) and check_consistency('bcr', (10, 5.0), 0) == (10.0, 5.0)
    for bad, match in ((dict(consistency='CR'), "one of none, cr, bcr"),
                       (dict(consistency='cr', consistency_weight=0.0), "positive weight"),
                       (dict(consistency='bcr', consistency_weight=(10.0, -1.0)), "positive weight"),
                       (dict(consistency='bcr', consistency_weight=(10.0,)), "positive weight"),
                       (dict(consistency='cr', consistency_weight=True), "positive weight"),
                       (dict(consistency='cr', consistency_weight=float('nan')), "positive weight"),
                       (dict(consistency='cr', consistency_shift=32), "consistency_shift 32"),
                       (dict(consistency='cr', consistency_shift=-1), "consistency_shift -1"),
                       (dict(consistency='bcr', consistency_shift=2.5), "consistency_shift 2.5")):
        with pytest.raises(ValueError, match=match):
            ACGANTrainer(device="cpu", **bad)
