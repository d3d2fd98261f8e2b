"""CPU: what the GPU tests of the sliced Wasserstein distance rest on, shown on the restatement tests/swd_ref.py alone -- the
pyramid of uint8 images is exact, the 4-bit statistics are exact, sorting is non-expansive, the derived key bound is far below
the values compared, and the cases have equal M and no constant channel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swd_ref as R  # noqa: E402

PYRAMID_SHAPES = [(2, 16, 16, 3), (2, 32, 32, 3), (2, 8, 12, 1), (2, 4, 4, 3)]


def uint8_images(shape, seed=1):
    return np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8)


@pytest.mark.parametrize("shape", PYRAMID_SHAPES)
def test_pyramid_of_uint8_is_exact(shape):
    """two levels against int64 scaled by 2^14: every value a multiple of 2^-14 below 256, so float64 is exact in any order"""
    x = uint8_images(shape)
    fine_int, coarse_int = R.pyramid_int(x)
    coarse = R.pyr_down(x)
    fine = x.astype(np.float64) - R.pyr_up(coarse)
    assert np.array_equal(coarse * 2.0 ** 14, coarse_int.astype(np.float64))
    assert np.array_equal(fine * 2.0 ** 14, fine_int.astype(np.float64))
    assert np.abs(coarse_int).max() < 256 * 2 ** 14 and np.abs(fine_int).max() < 512 * 2 ** 14
    if shape[1] >= 32:
        levels = R.laplacian_pyramid(x)
        assert len(levels) == 2 and np.array_equal(levels[0], fine) and np.array_equal(levels[1], coarse)


@pytest.mark.parametrize("shape", PYRAMID_SHAPES)
def test_pyramid_against_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    x = uint8_images(shape, 2).astype(np.float64)
    blurred = np.stack([np.stack([ndimage.convolve(x[n, :, :, c], R.WINDOW, mode='mirror') for c in range(shape[3])], axis=-1)
                        for n in range(shape[0])])
    assert np.array_equal(R.pyr_down(x), blurred[:, ::2, ::2, :])
    z = np.zeros((shape[0], 2 * shape[1], 2 * shape[2], shape[3]))
    z[:, ::2, ::2, :] = x
    up = np.stack([np.stack([ndimage.convolve(z[n, :, :, c], 4 * R.WINDOW, mode='mirror') for c in range(shape[3])], axis=-1)
                   for n in range(shape[0])])
    assert np.array_equal(R.pyr_up(x), up)


def test_level_sizes():
    assert R.level_sizes(32, 32) == [(32, 32), (16, 16)]
    assert R.level_sizes(64, 64) == [(64, 64), (32, 32), (16, 16)]
    assert R.level_sizes(16, 16) == [(16, 16)] and R.level_sizes(8, 12) == [(8, 12)] and R.level_sizes(4, 4) == [(4, 4)]


@pytest.mark.parametrize("i", range(len(R.PROJ)))
def test_four_bit_statistics_are_exact(i):
    """values 0..15: a sum of n squares is below n * 225, far inside 2^53, so sums and sums of squares are exact integers"""
    case = R.proj_case(i, True)
    n = len(case["cx"]) * case["nhood"] ** 2
    assert n * 15 * 15 < 2 ** 53 and np.log2(n * 225) < 20
    level = case["level"].astype(np.int64)
    assert np.array_equal(level.astype(np.float64), case["level"]) and level.min() >= 0 and level.max() <= 15
    p = R.patches(level, case["cx"], case["cy"], case["nhood"], R.PROJ_PER_IMAGE).astype(np.int64)
    exact = np.stack([p.sum(axis=(0, 2, 3)), (p * p).sum(axis=(0, 2, 3))], axis=1)
    assert np.array_equal(case["sums"], exact.astype(np.float64))


def test_sorting_is_non_expansive():
    rng = np.random.RandomState(3)
    for m in (1, 2, 17, 1000):
        for scale in (1e-12, 1e-3, 1.0):
            a = rng.randn(5, m)
            moved = a + scale * rng.uniform(-1, 1, size=a.shape)
            lhs = np.mean(np.abs(np.sort(moved, axis=1) - np.sort(a, axis=1)), axis=1)
            assert np.all(lhs <= np.abs(moved - a).max(axis=1) * (1 + 1e-12))


@pytest.mark.parametrize("i", R.cases())
def test_e2e_cases_and_their_bound(i):
    case = R.e2e_case(i)
    a, b, kw = case["a"], case["b"], case["kw"]
    assert a.shape == b.shape                                   # equal M on both sides
    for side in (a, b):
        for level in R.laplacian_pyramid(side):
            assert np.all(level.reshape(-1, level.shape[-1]).std(axis=0) > 0)
    _, ca, cb = R.draw_tables(*a.shape, kw["nhood_size"], kw["nhoods_per_image"], kw["dir_repeats"], kw["dirs_per_repeat"], 0)
    for side, centres in ((a, ca), (b, cb)):
        for level, (cx, cy) in zip(R.laplacian_pyramid(side), centres):
            assert len(cx) == len(cy) == a.shape[0] * kw["nhoods_per_image"]
            assert np.all(R.mean_std(R.patches(level, cx, cy, 7, kw["nhoods_per_image"]))[1] > 0)
    assert len(case["values"]) == len(R.level_sizes(a.shape[1], a.shape[2]))
    print("values", case["values"], "bounds", case["bounds"])
    assert np.all(case["values"] > 1.0)                         # the sides differ at every level
    # the bound cannot pass a wrong kernel.  It is a worst case over every order of summation, (n + 1) u with n = 12 544
    # elements per channel here: 10^-8 of the values, not 10^-9, is what such a bound can promise at this n
    assert np.all(case["bounds"] <= 1e-8 * case["values"])


@pytest.mark.parametrize("i", range(len(R.PROJ)))
def test_projection_cases_and_their_bound(i):
    case = R.proj_case(i)
    shape, nhood, ndirs = R.PROJ[i]
    half, (n, h, w, c) = nhood // 2, shape
    cx, cy = case["cx"], case["cy"]
    corners = {(half, half), (w - half - 1, half), (half, h - half - 1), (w - half - 1, h - half - 1)}
    assert corners <= set(zip(cx.tolist(), cy.tolist()))
    assert (cx[5], cy[5]) == (cx[6], cy[6]) and 5 // R.PROJ_PER_IMAGE == 6 // R.PROJ_PER_IMAGE
    assert np.all(case["std"] > 0) and case["keys"].shape == (ndirs, n * R.PROJ_PER_IMAGE)
    typical = np.abs(case["keys"]).mean()
    print("typical |key|", typical, "bound", case["key_bound"])
    assert case["key_bound"] <= 1e-9 * typical
    # a wrong mean by one part in 10^6, or one tap off, moves the keys by far more than the bound
    p = R.patches(case["level"], cx, cy, nhood, R.PROJ_PER_IMAGE)
    z = (p - (case["mean"] * (1 + 1e-6))[None, :, None, None]) / case["std"][None, :, None, None]
    assert np.abs((z.reshape(len(cx), -1) @ case["dirs"]).T - case["keys"]).max() > 1e3 * case["key_bound"]
