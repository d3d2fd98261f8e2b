"""CPU: the host side of NDB / JSD (gan_lib_tensorflow_amd/common/ndb.py: the bin statistics and the draws) on known answers,
the restatement tests/ndb_ref.py on a hand-checkable k-means, and the conditions on the inputs that the exact-equality claims
of tests/test_ndb_gpu.py rest on: at every case used there the reference alone leaves no row undecided."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndb_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def N():
    from gan_lib_tensorflow_amd.common import ndb
    return ndb


def test_equal_proportions(N):
    got = N.bin_statistics([10, 20, 30, 40], [20, 40, 60, 80])         # unequal totals, equal shares
    assert got["ndb"] == 0 and got["ndb_over_k"] == 0.0 and got["js"] == 0.0 and len(got["different_bins"]) == 0
    assert np.array_equal(got["bin_proportions_train"], [0.1, 0.2, 0.3, 0.4])
    assert np.array_equal(got["bin_proportions_samples"], got["bin_proportions_train"])


def test_disjoint_histograms(N):
    got = N.bin_statistics([5, 5, 0, 0], [0, 0, 8, 8])
    assert abs(got["js"] - math.log(2.0)) <= 1e-15
    # every bin: pooled P = 5 / 26 or 8 / 26, far from 0 and 1, and |p - q| = 1 / 2
    assert got["ndb"] == 4 and got["ndb_over_k"] == 1.0 and got["different_bins"].tolist() == [0, 1, 2, 3]


def test_one_z_value_by_hand(N):
    """N_r = 100, N_f = 200; bin 0 holds 30 training rows and 40 samples:
        p = 0.3, q = 0.2, pooled P = 70 / 300 = 7 / 30
        SE^2 = (7 / 30)(23 / 30)(1 / 100 + 1 / 200) = (161 / 900)(3 / 200) = 483 / 180000 = 0.00268333..
        SE = 0.0518009..,  z = 0.1 / SE = 1.930468..
        p-value = erfc(z / sqrt 2) = 0.05355..: different at 0.06, not at 0.05.
    Bin 1 is the complement (70 against 160): p - q = -0.1 and the same pooled variance, so the same |z|."""
    se = math.sqrt(483.0 / 180000.0)
    z = 0.1 / se
    assert abs(z - 1.930468) < 1e-6
    pvalue = math.erfc(z / math.sqrt(2.0))
    assert 0.05 < pvalue < 0.06 and abs(pvalue - 0.05355) < 1e-4
    assert N.bin_statistics([30, 70], [40, 160], 0.05)["ndb"] == 0
    got = N.bin_statistics([30, 70], [40, 160], 0.06)
    assert got["ndb"] == 2 and got["different_bins"].tolist() == [0, 1] and got["ndb_over_k"] == 1.0
    # JSD of (0.3, 0.7) against (0.2, 0.8), term by term
    want = 0.5 * (0.3 * math.log(0.3 / 0.25) + 0.7 * math.log(0.7 / 0.75)) + 0.5 * (0.2 * math.log(0.2 / 0.25) + 0.8 * math.log(0.8 / 0.75))
    assert abs(got["js"] - want) <= 1e-15


def test_bins_without_standard_error_are_not_different(N):
    got = N.bin_statistics([0, 50, 50], [0, 10, 90])                  # bin 0: P = 0, SE = 0
    assert 0 not in got["different_bins"].tolist() and got["different_bins"].tolist() == [1, 2]
    one = N.bin_statistics([7], [9])                                   # one bin: P = 1, SE = 0
    assert one["ndb"] == 0 and one["js"] == 0.0


def test_statistics_against_the_restatement_and_refusals(N):
    rng = np.random.RandomState(2)
    for _ in range(5):
        a, b = rng.randint(0, 50, 12), rng.randint(0, 80, 12)
        got, want = N.bin_statistics(a, b, 0.05), R.bin_statistics(a, b, 0.05)
        assert got["ndb"] == want["ndb"] and got["different_bins"].tolist() == want["different"]
        assert abs(got["js"] - want["js"]) <= 1e-15
        assert np.array_equal(got["bin_proportions_train"], want["p"]) and np.array_equal(got["bin_proportions_samples"], want["q"])
    with pytest.raises(ValueError, match="two equal"):
        N.bin_statistics([1, 2], [1, 2, 3])
    with pytest.raises(ValueError, match="not all zero"):
        N.bin_statistics([0, 0], [1, 2])


def test_draws(N):
    assert N.draw_dims(3072) is None and N.draw_dims(4096) is None and N.draw_dims(48, max_dims=48) is None
    dims = N.draw_dims(12288, seed=3)
    assert dims.dtype == np.int32 and dims.shape == (4096,)
    assert np.all(np.diff(dims) > 0) and dims[0] >= 0 and dims[-1] < 12288          # sorted, distinct, in range
    assert np.array_equal(dims, N.draw_dims(12288, seed=3)) and not np.array_equal(dims, N.draw_dims(12288, seed=4))
    assert np.array_equal(dims, R.draw_dims(12288, seed=3))
    small = N.draw_dims(100, max_dims=48, seed=1)
    assert small.shape == (48,) and np.array_equal(small, np.sort(np.random.RandomState(1).choice(100, 48, replace=False)))
    for bad in (15, 4097):
        with pytest.raises(ValueError, match="max_dims"):
            N.draw_dims(5000, max_dims=bad)
    init = N.draw_init(600, 12, seed=5)
    assert init.shape == (12,) and len(set(init.tolist())) == 12 and init.min() >= 0 and init.max() < 600
    assert np.array_equal(init, N.draw_init(600, 12, seed=5)) and np.array_equal(init, np.random.RandomState(5).choice(600, 12, replace=False))
    assert np.array_equal(init, R.draw_init(600, 12, seed=5)) and not np.array_equal(init, N.draw_init(600, 12, seed=6))
    with pytest.raises(ValueError, match="at least 13"):
        N.draw_init(12, 13)


def test_no_cpu_path(N):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.NDB(np.zeros((4, 4, 4, 3), dtype=np.uint8), number_of_bins=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        N.kmeans(torch.zeros((4, 16)), 2)


def test_restatement_kmeans_by_hand():
    """One dimension (15 zero columns beside it), rows 0, 1, 2, 10, 11, 12, 30, K = 2.  From the centroids (0, 1):
        iteration 1: |x - 0|^2 < |x - 1|^2 only for x = 0 -> labels 0 1 1 1 1 1 1, centroids 0 and 66 / 6 = 11
        iteration 2: 0, 1, 2 are nearer to 0 (2: 4 < 81), the rest to 11 -> labels 0 0 0 1 1 1 1, centroids 1 and 63 / 4 = 15.75
        iteration 3: 10 -> 81 against 33.06, no label moves: the last iteration.  inertia = 1 + 0 + 1 + 5.75^2 + 4.75^2 + 3.75^2 + 14.25^2"""
    col = np.array([0, 1, 2, 10, 11, 12, 30], dtype=np.float32)
    x = np.zeros((7, 16), dtype=np.float32)
    x[:, 0] = col
    seed = next(s for s in range(1000) if R.draw_init(7, 2, s).tolist() == [0, 1])
    fit = R.kmeans(x, 2, seed=seed)
    assert [l.tolist() for l in fit["labels"]] == [[0, 1, 1, 1, 1, 1, 1], [0, 0, 0, 1, 1, 1, 1], [0, 0, 0, 1, 1, 1, 1]]
    assert fit["iterations"] == 3 and fit["undecided"] == 0
    assert fit["centroids"][:, 0].tolist() == [1.0, 15.75] and not fit["centroids"][:, 1:].any()
    assert [c[:, 0].tolist() for c in fit["centroid_steps"]] == [[0.0, 1.0], [0.0, 11.0], [1.0, 15.75]]
    assert fit["inertia"] == 1 + 0 + 1 + 5.75 ** 2 + 4.75 ** 2 + 3.75 ** 2 + 14.25 ** 2
    assert R.kmeans(x, 2, seed=seed, max_iter=1)["iterations"] == 1
    # the stages by themselves: ties go to the lowest index, the grouping is stable, an empty cluster keeps its centroid
    label, d2, undecided, _ = R.assign(x, np.stack([x[1], x[1], x[6]]))
    assert label.tolist() == [0, 0, 0, 0, 0, 0, 2] and d2[:3].tolist() == [1.0, 0.0, 1.0]
    assert undecided[:6].all() and not undecided[6]               # the duplicated centroid ties six rows; row 6 is 29^2 clear
    count, offset, perm = R.group_rows(np.array([2, 0, 2, 0, 0]), 4)
    assert count.tolist() == [3, 0, 2, 0] and offset.tolist() == [0, 3, 3, 5] and perm.tolist() == [1, 3, 4, 0, 2]
    kept = R.centroids(x, np.arange(7), np.array([7, 0]), np.array([0, 7]), np.full((2, 16), 9, dtype=np.float32))
    assert kept[0, 0] == np.float32(66.0 / 7) and (kept[1] == 9).all()


@pytest.mark.parametrize("n,K,D", R.ASSIGN_SHAPES)
def test_no_row_of_the_assignment_cases_is_undecided(n, K, D):
    case = R.assign_case(n, K, D)
    assert int(case["undecided"].sum()) == 0
    assert len(np.unique(case["c"], axis=0)) == K
    if K > 3:
        assert (case["count"] == 0).any() or n >= 2 * K          # (the small-n cases have clusters without rows)
    assert (case["prev"] != case["label"]).sum() >= 1


def test_the_exact_case_has_ties():
    x, c, d, prev = R.integer_case()
    assert d.max() <= 16 * 36 and (c[5] == c[2]).all() and (c[41] == c[17]).all()
    tied = (d == d.min(axis=1, keepdims=True)).sum(axis=1)
    assert (tied >= 2).sum() >= 2                                # rows with more than one nearest centroid
    label = np.argmin(d, axis=1)
    assert 5 not in label and 41 not in label                    # the duplicates lose every tie to the lower index
    assert 0 < (label != prev).sum() <= 40


@pytest.mark.parametrize("K", [8, 12])
def test_no_row_of_the_mixture_fits_is_undecided(K):
    fit = R.mixture_case(K)["fit"]
    assert fit["undecided"] == 0 and 2 <= fit["iterations"] < 100
    assert np.array_equal(fit["labels"][-1], fit["labels"][-2])


def test_the_image_case_separates_the_two_sample_sets():
    case = R.image_case()
    a, b = case["ref_held_out"], case["ref_missing"]
    assert a["undecided"] == 0 and b["undecided"] == 0 and a["iterations"] < 100
    assert a["train_counts"].sum() == a["sample_counts"].sum() == b["sample_counts"].sum() == 600
    assert b["ndb"] > a["ndb"] and b["js"] > a["js"]
