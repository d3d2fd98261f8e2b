"""CPU: the float64 restatement tests/kid_ref.py against a direct double loop, the unbiasedness of the estimator, the subset
tables of common/kid.py, the argument errors of its host side, and the refusals of the two C entry points (csrc/kid.hip), which
are decided on the host before anything is launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kid_ref as R  # noqa: E402


def test_ref_block_sums_against_a_double_loop():
    rng = np.random.default_rng(0)
    m, d, gamma, coef0 = 3, 4, 0.25, 1.0
    x, y = rng.normal(size=(5, d)), rng.normal(size=(4, d))
    ix, iy = np.array([[4, 0, 2], [1, 4, 3]]), np.array([[3, 1, 0], [0, 2, 1]])
    for degree in (1, 2, 3):
        sums, absolute = R.block_sums(x, y, ix, iy, gamma, coef0, degree)
        for s in range(2):
            want, want_abs = np.zeros(3), np.zeros(3)
            for i in range(m):
                for j in range(m):
                    for blk, (a, b) in enumerate(((x[ix[s, i]], x[ix[s, j]]), (y[iy[s, i]], y[iy[s, j]]), (x[ix[s, i]], y[iy[s, j]]))):
                        if blk < 2 and i == j:
                            continue
                        want[blk] += (gamma * sum(a[k] * b[k] for k in range(d)) + coef0) ** degree
                        want_abs[blk] += (gamma * sum(abs(a[k]) * abs(b[k]) for k in range(d)) + abs(coef0)) ** degree
            np.testing.assert_allclose(sums[s], want, rtol=1e-13)
            np.testing.assert_allclose(absolute[s], want_abs, rtol=1e-13)
            assert np.all(np.abs(sums[s]) <= absolute[s])
    sums, _ = R.block_sums(x, y, ix, iy, gamma, coef0, 3)
    np.testing.assert_allclose(R.mmd2(sums, m), sums[:, 0] / 6 + sums[:, 1] / 6 - 2 * sums[:, 2] / 9, rtol=1e-15)


def test_mmd2_of_one_set_split_in_halves_is_unbiased():
    """Two halves of one sample: the unbiased estimator scatters around zero and takes both signs; the biased one (the diagonal
    kept, 1 / m^2 throughout) is a squared norm and never negative."""
    d, m = 16, 40
    values = []
    for seed in range(40):
        x = np.random.default_rng(seed).normal(size=(2 * m, d))
        ix, iy = np.arange(m)[None, :], np.arange(m, 2 * m)[None, :]
        mean, std, per, sums, _ = R.kernel_distance(x, x, ix, iy)
        assert std == 0.0 and per.shape == (1,) and mean == per[0]
        values.append(mean)
        a, b = x[:m], x[m:]
        k = lambda p, q: (p @ q.T / d + 1.0) ** 3  # noqa: E731
        assert k(a, a).mean() + k(b, b).mean() - 2 * k(a, b).mean() >= 0.0
    values = np.array(values)
    assert values.min() < 0.0 < values.max()
    assert abs(values.mean()) < 3 * values.std() / np.sqrt(len(values)) + 1e-12


def test_draw_subsets():
    from gan_lib_tensorflow_amd.common.kid import draw_subsets
    t = draw_subsets(50, 7, 20, np.random.RandomState(3))
    assert t.shape == (7, 20) and t.dtype == np.int32
    assert t.min() >= 0 and t.max() < 50
    assert all(len(set(row)) == 20 for row in t.tolist())
    assert len({tuple(row) for row in t.tolist()}) == 7
    assert np.array_equal(t, draw_subsets(50, 7, 20, np.random.RandomState(3)))
    assert not np.array_equal(t, draw_subsets(50, 7, 20, np.random.RandomState(4)))
    full = draw_subsets(5, 2, 5, np.random.RandomState(0))
    assert sorted(full[0].tolist()) == sorted(full[1].tolist()) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        draw_subsets(5, 2, 6, np.random.RandomState(0))


def test_argument_errors():
    from gan_lib_tensorflow_amd.common import kid
    one, many = np.zeros((1, 2048), np.float32), np.zeros((8, 2048), np.float32)
    with pytest.raises(ValueError, match="at least 2"):
        kid.kernel_distance(one, many)
    with pytest.raises(ValueError, match="at least 2"):
        kid.kernel_distance(many, one)
    with pytest.raises(ValueError, match="at least 2"):
        kid.calculate_kid(many, one)
    with pytest.raises(ValueError, match="subsets"):
        kid.kernel_distance(many, many, subsets=0)
    images = np.zeros((4, 32, 32, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        kid.calculate_kid(images, many)
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        kid.sample_features(lambda: None, 10, None)
    with pytest.raises(TypeError, match="calculate_kid"):
        kid.calculate_kid("features.npy", many)
    with pytest.raises(ValueError, match="multiple of 16"):
        kid.FeatureBank(24, 10, device='cpu')


def test_kid_num_tiles():
    from gan_lib_tensorflow_amd import kernels as K
    assert [K.kid_num_tiles(m) for m in (2, 64, 65, 128, 130, 1000)] == [3, 3, 10, 10, 21, 16 * 17 + 256]


def test_entry_points_refuse_bad_arguments_with_a_message():
    from gan_lib_tensorflow_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below is refused by argument checks

    def err():
        return lib.gank_last_error().decode()

    def sums(nx=100, ny=100, d=64, ix=fake, iy=fake, subsets=1, m=10, degree=3, x=fake, partial=fake):
        return lib.gank_kid_block_sums(x, nx, fake, ny, d, ix, iy, subsets, m, 1.0 / d, 1.0, degree, partial, None)

    assert sums(d=24) != 0 and "D = 24 unsupported" in err()
    assert sums(d=4112) != 0 and "unsupported" in err()
    assert sums(m=1) != 0 and "at least 2" in err()
    assert sums(nx=9) != 0 and "exceeds the feature banks" in err()
    assert sums(ny=9) != 0 and "exceeds the feature banks" in err()
    assert sums(degree=4) != 0 and "degree = 4" in err()
    assert sums(degree=0) != 0 and "degree = 0" in err()
    assert sums(subsets=0) != 0 and "subsets = 0" in err()
    assert sums(ix=None) != 0 and "null pointer" in err()
    assert sums(iy=None) != 0 and "null pointer" in err()
    assert sums(x=None) != 0 and "null pointer" in err()
    assert sums(partial=None) != 0 and "null pointer" in err()
    assert lib.gank_kid_finish(None, 1, 10, fake, None) != 0 and "null pointer" in err()
    assert lib.gank_kid_finish(fake, 0, 10, fake, None) != 0 and "subsets = 0" in err()
    assert lib.gank_kid_finish(fake, 1, 1, fake, None) != 0 and "m = 1" in err()
