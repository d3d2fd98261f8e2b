"""CPU: the host side of MS-SSIM (gan_lib_tensorflow_amd/common/msssim.py) against numbers recorded from the reference program
itself (tests/golden/msssim.npz, written by tests/golden/make_msssim_golden.py), and the argument checks of the C entry points
and of the Python interface.  Nothing here computes an SSIM map: there is no CPU path for that."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_cases as MC  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(MC.GOLDEN)


def test_fixture_is_small_and_complete(golden):
    assert os.path.getsize(MC.GOLDEN) <= 200 * 1024
    for name in MC.CASES:
        for key in ("levels", "pairs", "batch"):
            assert f"{name}/{key}" in golden, (name, key)


@pytest.mark.parametrize("name", list(MC.BASE))
def test_fixture_inputs_regenerate_to_the_recorded_sha256(golden, name):
    a, b, _ = MC.inputs(name, golden)           # raises "regenerate the fixture" on a mismatch
    h, w, c, n, _, _ = MC.BASE[name]
    assert a.shape == b.shape == (n, h, w, c) and a.dtype == b.dtype == np.uint8


def test_a_changed_input_is_reported_not_skipped(golden):
    fake = {k: golden[k] for k in ("s45_noisy/a", "s45_noisy/b")}
    fake["s45_noisy/sha256"] = np.array("0" * 64)
    with pytest.raises(AssertionError, match="regenerate the fixture"):
        MC.inputs("s45_noisy", fake)


def test_default_weights():
    from gan_lib_tensorflow_amd.common import msssim as M
    assert tuple(M.DEFAULT_WEIGHTS) == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    assert abs(sum(M.DEFAULT_WEIGHTS) - 1.0) > 1e-6          # they do not sum to 1, and stay so


@pytest.mark.parametrize("name", MC.CASES)
def test_combine_levels_reproduces_the_reference_scores(golden, name):
    """combine_levels on the reference's own per-level values gives the reference's per-pair and batch scores to 1e-12
    relative, NaN exactly where the reference has NaN."""
    from gan_lib_tensorflow_amd.common.msssim import combine_levels
    _, _, kwargs = MC.inputs(name, golden)
    weights = kwargs.get("weights")
    levels, pairs, batch = golden[f"{name}/levels"], golden[f"{name}/pairs"], float(golden[f"{name}/batch"])
    got = combine_levels(levels, weights)
    assert got.shape == pairs.shape and got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(pairs))
    ok = ~np.isnan(pairs)
    assert np.all(np.abs(got[ok] - pairs[ok]) <= 1e-12 * np.abs(pairs[ok]))
    got_batch = combine_levels(levels.mean(axis=0), weights)
    if np.isnan(batch):
        assert np.isnan(got_batch)
    else:
        assert abs(got_batch - batch) <= 1e-12 * abs(batch)


def test_the_fixture_has_nan_pairs_and_nan_free_batches(golden):
    """what the docstring of the module says about NaN, on the recorded reference values"""
    assert np.isnan(golden["s32_indep/pairs"]).mean() > 0.25
    assert not np.isnan(golden["s256_indep/pairs"]).any()
    for name in MC.BASE:
        assert np.isfinite(float(golden[f"{name}/batch"])), name


def test_gauss_taps_are_the_separable_factor_of_the_reference_window():
    from gan_lib_tensorflow_amd.common.msssim import gauss_taps
    for size in range(1, 12):
        k = gauss_taps(size, size * 1.5 / 11)
        assert k.shape == (size,) and abs(k.sum() - 1.0) < 1e-15 and np.allclose(k, k[::-1], rtol=0, atol=1e-17)
    k = gauss_taps(4, 1.0)                         # even size: half-integer offsets -1.5, -0.5, 0.5, 1.5
    e = np.exp(-np.array([1.5, 0.5, 0.5, 1.5]) ** 2 / 2.0)
    assert np.allclose(k, e / e.sum(), rtol=1e-15)


def test_entry_points_reject_bad_arguments_with_a_message():
    """gank_msssim_level refuses, on the host and before any launch (so without a GPU): null pointers, a window outside 1..11,
    C < 1, an image smaller than the window, an unknown dtype code."""
    from gan_lib_tensorflow_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)           # never dereferenced
    taps = (C.c_float * 11)(*([1.0 / 11] * 11))
    f = C.c_float

    def call(a=fake, b=fake, dtype=0, n=2, h=32, w=32, c=3, size=11, k=taps, part=fake, p1=None, p2=None):
        return lib.gank_msssim_level(a, b, dtype, n, h, w, c, size, k, f(6.5), f(58.5), f(127.5), part, p1, p2, None)

    def err():
        return lib.gank_last_error().decode()

    for kw in (dict(a=None), dict(b=None), dict(part=None), dict(k=None)):
        assert call(**kw) != 0 and "null pointer" in err(), kw
    assert call(p1=fake) != 0 and "both or neither" in err()
    assert call(size=0) != 0 and "outside 1..11" in err()
    assert call(size=12, h=64, w=64) != 0 and "outside 1..11" in err()
    assert call(c=0) != 0 and "at least one channel" in err()
    assert call(h=10) != 0 and "smaller than the window" in err()
    assert call(w=10) != 0 and "smaller than the window" in err()
    assert call(dtype=2) != 0 and "unknown input dtype" in err()
    assert call(n=0) != 0 and "empty batch" in err()
    assert lib.gank_msssim_level_parts(10, 32, 3, 11) == 0 and "unsupported" in err()
    assert lib.gank_msssim_level_parts(32, 32, 3, 11) == 1                    # a whole small image is one part
    assert lib.gank_msssim_level_parts(512, 512, 3, 11) == 32 * 16            # 16 x 32-pixel tiles of the 502 x 502 outputs
    assert lib.gank_msssim_level_parts(64, 64, 6, 11) == 4 * 2 * 2            # ... per chunk of 4 channels


def test_python_interface_checks_before_touching_the_device():
    import torch
    from gan_lib_tensorflow_amd.common import msssim as M
    a = np.zeros((2, 32, 32, 3), np.uint8)
    for fn in (M.MultiScaleSSIM, M._SSIMForMultiScale, M.msssim_levels):
        with pytest.raises(RuntimeError, match="same shape"):
            fn(a, a[:, :16])
        with pytest.raises(RuntimeError, match="four dimensions"):
            fn(a[0], a[0])
        with pytest.raises(NotImplementedError, match="102-107"):
            fn(a, a, filter_size=0)
        with pytest.raises(NotImplementedError, match="filter_size=13"):
            fn(a, a, filter_size=13)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            M.MultiScaleSSIM(torch.zeros(2, 32, 32, 3, dtype=torch.uint8), torch.zeros(2, 32, 32, 3, dtype=torch.uint8))
        with pytest.raises(RuntimeError, match="no CPU path"):
            M.MultiScaleSSIM(a, a)
    with pytest.raises(RuntimeError, match="do not fit"):
        M.combine_levels(np.ones((3, 4, 2)))


def test_trainers_expose_the_metric():
    from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
    from gan_lib_tensorflow_amd.Pix2Pix import train as P
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
    assert callable(SNGANTrainer.msssim_diversity) and callable(ACGANTrainer.msssim_diversity) and callable(P.msssim_score)
