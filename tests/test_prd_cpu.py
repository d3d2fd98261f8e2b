"""CPU: the float64 restatement tests/prd_ref.py against a direct double loop; the condition under which the GPU tests may
demand EQUAL counts (no comparison of a distance with a radius, and no choice of a k-th neighbour, lies within the derived error
bound: a cap of zero, checked on the reference alone); the ties of the exact integer case; the argument errors of
common/precision_recall.py; the refusals of the four C entry points (csrc/prd.hip), decided on the host before anything is
launched; and the segment heuristic."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prd_ref as R  # noqa: E402


def test_ref_against_a_double_loop():
    x, y = R.manifold_banks(7, 9, 16, seed=3)
    k = 2
    xd, yd = x.astype(np.float64), y.astype(np.float64)

    def dist(a, b):
        return sum((a[t] - b[t]) ** 2 for t in range(len(a)))

    want = np.array([[dist(a, b) for b in yd] for a in xd])
    np.testing.assert_allclose(R.d2(x, y), want, rtol=1e-14)
    assert np.all(R.d2_bound(x, y) > 0) and np.all(np.abs(R.d2(x, y) - want) <= R.d2_bound(x, y))
    radii = {}
    for name, bank in (("x", xd), ("y", yd)):
        radii[name] = np.array([sorted(dist(bank[i], bank[j]) for j in range(len(bank)) if j != i)[k - 1] for i in range(len(bank))])
        np.testing.assert_allclose(R.radii(bank.astype(np.float32), k), radii[name], rtol=1e-13)
    count, nearest = R.counts(y, x, radii["x"])
    want_count = [sum(dist(q, xd[j]) <= radii["x"][j] for j in range(len(xd))) for q in yd]
    assert count.tolist() == want_count
    np.testing.assert_allclose(nearest, [min(dist(q, b) for b in xd) for q in yd], rtol=1e-13)
    back, near_back = R.counts(x, y, radii["y"])
    got = R.prdc(x, y, k)
    assert got == dict(precision=float(np.mean(np.array(want_count) > 0)), recall=float(np.mean(back > 0)),
                       density=sum(want_count) / (k * len(yd)), coverage=float(np.mean(near_back <= radii["x"])))


def test_a_duplicate_is_a_neighbour_and_self_is_not():
    x = np.array([[0, 0], [3, 4], [0, 0], [6, 8]], np.float32)
    assert R.radii(x, 1).tolist() == [0.0, 25.0, 0.0, 25.0]
    assert R.radii(x, 2).tolist() == [25.0, 25.0, 25.0, 100.0]


@pytest.mark.parametrize("nx,ny,d,k", R.cases())
def test_no_comparison_is_undecided(nx, ny, d, k):
    """The cap that lets tests/test_prd_gpu.py compare counts with ==: zero undecided elements, zero undecided radii."""
    ref = R.reference(nx, ny, d, k)
    x, y = ref['x'], ref['y']
    undecided = [R.undecided_elements(y, x, ref['radii_x'], ref['radii_bound_x']),
                 R.undecided_elements(x, y, ref['radii_y'], ref['radii_bound_y']),
                 R.undecided_coverage(x, y, ref['radii_x'], ref['radii_bound_x'])]
    (rx, gap_x), (ry, gap_y) = R.undecided_radii(x, k), R.undecided_radii(y, k)
    print(f"({nx},{ny},{d}) k={k}: undecided elements {undecided}, undecided radii {rx} + {ry}, smallest radius gap / bound "
          f"{min(gap_x, gap_y):.3g}, {ref['prdc']}")
    assert undecided == [0, 0, 0]
    assert rx == 0 and ry == 0
    if nx >= 17:
        assert 0.0 < ref['prdc']['precision'] < 1.0
    assert all(0.0 <= ref['prdc'][name] <= 1.0 for name in ('precision', 'recall', 'coverage')) and ref['prdc']['density'] >= 0.0


def test_the_integer_case_has_ties_that_matter():
    """what the exact GPU case can catch: elements EQUAL to their radius (an exclusive comparison changes a count), rows whose
    k-th and (k+1)-th distances are equal, and a duplicated row (self-exclusion by value changes its radius)"""
    x, y = R.integer_banks()
    k = 3
    assert np.array_equal(x[40], x[7]) and R.integer_radii(x, 1)[7] == 0 and R.integer_radii(x, 1)[40] == 0
    assert R.integer_d2(x, y).max() <= 16 * 49 and R.integer_d2(x, x).max() <= 16 * 49
    rx = R.integer_radii(x, k)
    d = R.integer_d2(y, x)
    inclusive, exclusive = (d <= rx[None, :]).sum(axis=1), (d < rx[None, :]).sum(axis=1)
    assert (inclusive != exclusive).sum() >= 1
    n = len(x)
    s = np.sort(R.integer_d2(x, x)[~np.eye(n, dtype=bool)].reshape(n, n - 1), axis=1)
    assert (s[:, k - 1] == s[:, k]).sum() >= 1
    # the float64 restatement agrees with the integers exactly
    assert np.array_equal(R.radii(x.astype(np.float32), k), rx.astype(np.float64))
    assert np.array_equal(R.counts(y.astype(np.float32), x.astype(np.float32), rx)[0], inclusive)


def test_argument_errors():
    from gan_lib_tensorflow_amd.common import precision_recall as PR
    few, many = np.zeros((3, 2048), np.float32), np.zeros((8, 2048), np.float32)
    with pytest.raises(ValueError, match="at least 4"):
        PR.calculate_prdc(few, many)
    with pytest.raises(ValueError, match="at least 4"):
        PR.calculate_prdc(many, few)
    with pytest.raises(ValueError, match="at least 6"):
        PR.density_coverage(many, np.zeros((5, 2048), np.float32))
    with pytest.raises(ValueError, match="at least 4"):
        PR.precision_recall(few, many)
    with pytest.raises(ValueError, match="at least 4"):
        PR.knn_radii(few)
    with pytest.raises(ValueError, match="k = 9"):
        PR.calculate_prdc(np.zeros((20, 16), np.float32), np.zeros((20, 16), np.float32), k=9)
    with pytest.raises(ValueError, match="k = 0"):
        PR.knn_radii(many, k=0)
    images = np.zeros((8, 32, 32, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        PR.calculate_prdc(images, many)
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        PR.calculate_prdc(many, images)
    with pytest.raises(TypeError, match="calculate_prdc"):
        PR.calculate_prdc("features.npy", many)


def test_prd_default_segments():
    from gan_lib_tensorflow_amd import kernels as K
    # never more segments than column tiles, at least one
    assert [K.prd_default_segments(n) for n in (4, 64, 65, 130, 300)] == [1, 1, 2, 3, 5]
    # 10 000 rows: 157 strips, 16 workgroups per compute unit want ceil(4096 / 157) = 27 segments
    assert K.prd_default_segments(10000) == 27
    assert K.prd_default_segments(50000) == 6 and K.prd_default_segments(500000) == 1
    # few query rows against a long bank: the bank is cut finer
    assert K.prd_default_segments(10000, rows=64) == 157 and K.prd_default_segments(64, rows=10000) == 1
    assert K.prd_counts_partial_len(5, 3) == 15 + 8 and K.prd_counts_partial_len(4, 3) == 12 + 6


def test_entry_points_refuse_bad_arguments_with_a_message():
    from gan_lib_tensorflow_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below is refused by argument checks

    def err():
        return lib.gank_last_error().decode()

    def knn(x=fake, n=100, d=64, k=3, segments=1, part=fake):
        return lib.gank_prd_knn_partial(x, n, d, k, segments, part, None)

    assert knn(x=None) != 0 and "null pointer" in err()
    assert knn(part=None) != 0 and "null pointer" in err()
    assert knn(d=24) != 0 and "D = 24 unsupported" in err()
    assert knn(d=8) != 0 and "unsupported" in err()
    assert knn(d=4112) != 0 and "unsupported" in err()
    assert knn(k=0) != 0 and "k = 0" in err()
    assert knn(k=9) != 0 and "k = 9" in err()
    assert knn(n=3) != 0 and "at least 4" in err()
    assert knn(segments=0) != 0 and "segments = 0" in err()
    assert knn(segments=3) != 0 and "segments = 3" in err() and "2 column tiles" in err()
    assert knn(n=(1 << 24) + 1) != 0 and "at most" in err()
    assert lib.gank_prd_knn_finish(None, 100, 3, 1, fake, None) != 0 and "null pointer" in err()
    assert lib.gank_prd_knn_finish(fake, 100, 9, 1, fake, None) != 0 and "k = 9" in err()
    assert lib.gank_prd_knn_finish(fake, 3, 3, 1, fake, None) != 0 and "n = 3" in err()
    assert lib.gank_prd_knn_finish(fake, 100, 3, 0, fake, None) != 0 and "segments = 0" in err()

    def counts(q=fake, nq=100, r=fake, nr=100, d=64, radii2=fake, segments=1, part_count=fake, part_min=fake):
        return lib.gank_prd_counts_partial(q, nq, r, nr, d, radii2, segments, part_count, part_min, None)

    for name in ("q", "r", "radii2", "part_count", "part_min"):
        assert counts(**{name: None}) != 0 and "null pointer" in err()
    assert counts(d=24) != 0 and "D = 24 unsupported" in err()
    assert counts(nq=0) != 0 and "nq = 0" in err()
    assert counts(nr=0) != 0 and "nr = 0" in err()
    assert counts(segments=0) != 0 and "segments = 0" in err()
    assert counts(nq=1000, segments=3) != 0 and "segments = 3" in err()          # the BANK's tiles bound the segments
    assert counts(nq=(1 << 24) + 1) != 0 and "nq =" in err()
    assert lib.gank_prd_counts_finish(fake, fake, 100, 1, None, fake, None) != 0 and "null pointer" in err()
    assert lib.gank_prd_counts_finish(fake, fake, 0, 1, fake, fake, None) != 0 and "nq = 0" in err()
    assert lib.gank_prd_counts_finish(fake, fake, 100, 0, fake, fake, None) != 0 and "segments = 0" in err()
