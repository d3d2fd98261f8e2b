"""CPU: the host side of the FID (gan_lib_tensorflow_amd/common/fid.py) against the float64 restatement tests/fid_ref.py -- the
Frechet distance against its published sqrtm form and against known answers, rank-deficient statistics, the finalisation of the
device's sums, the statistics file -- and the argument checks of the two entry points of csrc/fid.hip (decided on the host)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def F():
    from gan_lib_tensorflow_amd.common import fid
    return fid


@pytest.mark.parametrize("d,n", [(64, 256), (128, 512)])
def test_frechet_distance_matches_the_sqrtm_form(F, d, n):
    """N = 4 D keeps the sqrtm reference itself well conditioned (at N < D its own result carries a 1e-6 imaginary part)."""
    xa, xb = R.feature_sets(d, n, seed=0)
    sa, sb = R.statistics(xa), R.statistics(xb)
    got, want = F.frechet_distance(*sa, *sb), R.frechet_sqrtm(*sa, *sb)
    rel = abs(got - want) / abs(want)
    print(f"D={d} N={n}: product {got!r} sqrtm form {want!r} relative difference {rel:.2e}")
    assert want > 0 and rel <= 1e-9
    assert abs(got - R.frechet_eigen(*sa, *sb)) <= 1e-9 * abs(want)


def test_frechet_distance_known_answers(F):
    rng = np.random.default_rng(1)
    d = 48
    xa, xb = R.feature_sets(d, 4 * d, seed=2)
    (mu1, s1), (mu2, s2) = R.statistics(xa), R.statistics(xb)
    assert abs(F.frechet_distance(mu1, s1, mu1, s1)) <= 1e-12 * np.trace(s1)                 # identical statistics
    shift = rng.normal(size=d)
    eye = np.eye(d)
    assert abs(F.frechet_distance(mu1, eye, mu1 + shift, eye) - shift @ shift) <= 1e-12 * (shift @ shift + 2 * d)
    a, b = rng.uniform(0.1, 2.0, size=d), rng.uniform(0.1, 2.0, size=d)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(F.frechet_distance(mu1, np.diag(a), mu1, np.diag(b)) - want) <= 1e-12 * (a.sum() + b.sum())
    c = 0.37
    want = (1 - np.sqrt(c)) ** 2 * np.trace(s1)
    assert abs(F.frechet_distance(mu1, s1, mu1, c * s1) - want) <= 1e-12 * (1 + c) * np.trace(s1)
    ab, ba = F.frechet_distance(mu1, s1, mu2, s2), F.frechet_distance(mu2, s2, mu1, s1)
    assert ab > 0 and abs(ab - ba) <= 1e-10 * ab


def test_frechet_distance_rank_deficient(F):
    d, n = 256, 48
    xa, xb = R.feature_sets(d, n, seed=3)
    (mu1, s1), (mu2, s2) = R.statistics(xa), R.statistics(xb)
    scale = np.trace(s1) + np.trace(s2)
    got = F.frechet_distance(mu1, s1, mu2, s2)
    assert np.isfinite(got) and got >= -1e-9 * scale
    assert abs(got - R.frechet_eigen(mu1, s1, mu2, s2)) <= 1e-9 * scale
    assert abs(F.frechet_distance(mu1, s1, mu1, s1)) <= 1e-12 * np.trace(s1)


def test_finalisation_of_the_device_sums(F):
    """(count, sum, upper triangle of the Gram matrix) -> mean and covariance; what lies below the diagonal is never read"""
    d, n = 80, 142
    x = R.feature_sets(d, n, seed=4, count=1)[0]
    gram = np.triu(x.T @ x) + np.tril(np.full((d, d), -7.0e300), -1)
    mu, sigma = F.moments_from_sums(n, x.sum(axis=0), gram)
    rmu, rsigma = R.statistics(x)
    assert np.abs(mu - rmu).max() <= 1e-12 * np.abs(rmu).max()
    assert np.abs(sigma - rsigma).max() <= 1e-12 * np.abs(rsigma).max()
    assert np.array_equal(sigma, sigma.T)
    with pytest.raises(ValueError):
        F.moments_from_sums(1, x[0], np.outer(x[0], x[0]))


def test_statistics_file_round_trip(F, tmp_path):
    d = 32
    x = R.feature_sets(d, 100, seed=5, count=1)[0]
    mom = F.FeatureMoments.__new__(F.FeatureMoments)         # the host half alone: no device buffers on a machine without a GPU
    mom.dim, mom.count, mom._stats = d, 100, R.statistics(x)
    path = str(tmp_path / "stats.npz")
    mom.save(path)
    with np.load(path) as f:
        assert {'mu', 'sigma'} <= set(f.files) and int(f['count']) == 100
    mu, sigma = F.FeatureMoments.load(path)
    assert mu.dtype == np.float64 and np.array_equal(mu, mom._stats[0]) and np.array_equal(sigma, mom._stats[1])
    assert F.calculate_fid(path, mom._stats) == F.frechet_distance(mu, sigma, mu, sigma)


def test_images_without_a_network_name_the_download(F):
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        F.calculate_fid(np.zeros((4, 32, 32, 3), np.uint8), np.zeros((4, 32, 32, 3), np.uint8))


def test_entry_points_reject_bad_arguments_with_a_message():
    """A non-zero return and a gank_last_error() message, decided on the host before any launch."""
    import ctypes as C
    from gan_lib_tensorflow_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)         # never dereferenced

    def err():
        return lib.gank_last_error().decode()

    assert lib.gank_moments_update(None, 1, 4, 64, fake, fake, None) != 0 and "null pointer" in err()
    assert lib.gank_moments_update(fake, 1, 4, 64, None, fake, None) != 0 and "null pointer" in err()
    assert lib.gank_moments_update(fake, 1, 4, 64, fake, None, None) != 0 and "null pointer" in err()
    assert lib.gank_moments_update(fake, 1, 4, 24, fake, fake, None) != 0 and "D = 24" in err()
    assert lib.gank_moments_update(fake, 1, 4, 8192, fake, fake, None) != 0 and "D = 8192" in err()
    assert lib.gank_moments_update(fake, 0, 0, 64, fake, fake, None) != 0 and "n = 0" in err()
    assert lib.gank_moments_update(fake, 2, 4, 64, fake, fake, None) != 0 and "dtype" in err()
    assert lib.gank_mean_hw_f32(None, fake, 2, 4, 16, None) != 0 and "null pointer" in err()
    assert lib.gank_mean_hw_f32(fake, None, 2, 4, 16, None) != 0 and "null pointer" in err()
    assert lib.gank_mean_hw_f32(fake, fake, 2, 4, 12, None) != 0 and "C=12" in err()
    assert lib.gank_mean_hw_f32(fake, fake, 0, 4, 16, None) != 0 and "empty" in err()
