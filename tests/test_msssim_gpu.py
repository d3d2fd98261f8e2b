"""GPU: MS-SSIM (csrc/msssim.hip behind gan_lib_tensorflow_amd/common/msssim.py) against numbers recorded from the reference
program itself (tests/golden/msssim.npz), its properties, and the trainers' diversity score.

Bounds.  5e-4 absolute on every per-pair per-level mean: a float32 NumPy emulation of the kernel's arithmetic (separable direct
form, pixels shifted by max_val / 2) stays within 6.1e-5 of the reference on near-saturated flat images -- where the
E[x^2] - mu^2 cancellation is worst -- and within 2.6e-7 on textured ones; 5e-4 leaves 8x for another summation order and
FMA contraction.  Scores: 1e-3 absolute where the reference score is >= 0.9 (noisy, bright); 2 % relative on the batch score of
independent pairs (the error of prod cs^w at cs ~ 0.03 under the 5e-4 bound is ~1.6 %).  Largest deviations measured on an MI355X:
DESIGN.md, section "MS-SSIM"."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import msssim_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu

LEVEL_TOL = 5e-4
SCORE_TOL = 1e-3
INDEP_REL_TOL = 0.02
BAND = 5e-4           # a reference base (cs before the last level, ssim at the last) this close to 0 may change sign on the GPU
BAND_CAP = 0.05       # ... for at most this share of a case's pairs


@pytest.fixture(scope="module")
def golden():
    return np.load(MC.GOLDEN)


@pytest.fixture(scope="module")
def M():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from gan_lib_tensorflow_amd.common import msssim
    return msssim


def _levels(M, name, golden):
    a, b, kwargs = MC.inputs(name, golden)
    weights = kwargs.pop("weights", None)
    n_levels = len(weights) if weights else 5
    return M.msssim_levels(a, b, levels=n_levels, **kwargs), weights


@pytest.mark.parametrize("name", MC.CASES)
def test_levels_match_the_reference(M, golden, name):
    got, _ = _levels(M, name, golden)
    ref = golden[f"{name}/levels"]
    assert got.shape == ref.shape and got.dtype == np.float64
    dev = np.abs(got - ref)
    print(f"{name}: max |levels - reference| = {dev.max():.3e} (ssim {dev[..., 0].max():.3e}, cs {dev[..., 1].max():.3e})")
    assert np.all(dev <= LEVEL_TOL), (name, dev.max())


@pytest.mark.parametrize("name", MC.CASES)
def test_scores_match_the_reference(M, golden, name):
    a, b, kwargs = MC.inputs(name, golden)
    ref_pairs, ref_batch = golden[f"{name}/pairs"], float(golden[f"{name}/batch"])
    got_pairs = M.MultiScaleSSIM(a, b, per_image=True, **kwargs)
    got_batch = M.MultiScaleSSIM(a, b, **kwargs)
    assert isinstance(got_batch, float) and got_pairs.shape == ref_pairs.shape and got_pairs.dtype == np.float64
    if MC.kind_of(name) in ("noisy", "bright"):
        assert ref_batch >= 0.9 and not np.isnan(ref_pairs).any()
        print(f"{name}: max |pair score - reference| = {np.abs(got_pairs - ref_pairs).max():.3e}, batch {abs(got_batch - ref_batch):.3e}")
        assert np.all(np.abs(got_pairs - ref_pairs) <= SCORE_TOL)
        assert abs(got_batch - ref_batch) <= SCORE_TOL
    else:
        # the batch means of the fixture's independent cases lie far outside the band (>= 1.8e-3), so NaN must agree
        assert np.isnan(got_batch) == np.isnan(ref_batch)
        if not np.isnan(ref_batch):
            print(f"{name}: batch score {got_batch:.6f} vs {ref_batch:.6f}: rel {abs(got_batch / ref_batch - 1):.3e}")
            assert abs(got_batch - ref_batch) <= INDEP_REL_TOL * abs(ref_batch)


@pytest.mark.parametrize("name", MC.CASES)
def test_nan_mask_matches_the_reference(M, golden, name):
    a, b, kwargs = MC.inputs(name, golden)
    ref_levels, ref_pairs = golden[f"{name}/levels"], golden[f"{name}/pairs"]
    got = M.MultiScaleSSIM(a, b, per_image=True, **kwargs)
    bases = np.concatenate([ref_levels[:, :-1, 1], ref_levels[:, -1:, 0]], axis=1)
    decided = (np.abs(bases) >= BAND).all(axis=1)
    assert (~decided).mean() <= BAND_CAP, (name, (~decided).mean())
    assert np.array_equal(np.isnan(got)[decided], np.isnan(ref_pairs)[decided])


def _smooth_pair(n, h, w, c, seed=7):
    rng = np.random.default_rng(seed)
    return MC.smooth(rng, n, h, w, c), MC.smooth(rng, n, h, w, c)


@pytest.mark.parametrize("shape", [(4, 32, 32, 3), (2, 45, 37, 1), (2, 96, 80, 3)])
def test_properties(M, shape):
    import torch
    a, b = _smooth_pair(*shape)
    noisy = np.clip(a.astype(np.int64) + np.random.default_rng(1).integers(-20, 21, size=a.shape), 0, 255).astype(np.uint8)
    same = M.msssim_levels(a, a)
    assert np.all(np.abs(same - 1.0) <= 1e-6)
    assert abs(M.MultiScaleSSIM(a, a) - 1.0) <= 1e-6
    ab, ba = M.MultiScaleSSIM(a, noisy, per_image=True), M.MultiScaleSSIM(noisy, a, per_image=True)
    assert np.all(np.abs(ab - ba) <= 1e-6)
    lv = M.msssim_levels(a, b)
    assert np.array_equal(lv, M.msssim_levels(a, b))                                        # two calls: the same bits
    assert np.array_equal(lv, M.msssim_levels(a.astype(np.float32), b.astype(np.float32)))  # uint8 and the same values as fp32
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    assert np.array_equal(lv, M.msssim_levels(ta, tb))                                      # device tensors and uploaded arrays
    batch = M.MultiScaleSSIM(a, noisy)
    assert batch == float(M.combine_levels(M.msssim_levels(a, noisy).mean(axis=0)))
    ssim, cs = M._SSIMForMultiScale(a, noisy)
    first = M.msssim_levels(a, noisy)[:, 0].mean(axis=0)
    assert (ssim, cs) == (float(first[0]), float(first[1]))


def test_channels_are_averaged_and_chunked_consistently(M):
    """the means run over the channels too: a 6-channel pair (two chunks of channels per tile) scores the mean of its channels
    scored alone, at a tiled size and at a whole-image size"""
    for n, h, w in ((2, 70, 50), (3, 24, 24)):
        a, b = _smooth_pair(n, h, w, 6, seed=11)
        whole = M.msssim_levels(a, b)
        single = np.mean([M.msssim_levels(a[..., c:c + 1].copy(), b[..., c:c + 1].copy()) for c in range(6)], axis=0)
        # the same per-pixel values, added in another order: fp32 tile sums of <= 2048 terms near 1 (per-thread runs of <= 8, then
        # a tree of 8 + 2 steps) are good to ~20 roundings of 6e-8
        assert np.all(np.abs(whole - single) <= 2e-6)


def test_a_batch_is_its_images_one_by_one(M):
    """many images per workgroup at the small levels and one launch per level for the batch change no image's numbers"""
    a, b = _smooth_pair(70, 32, 32, 3, seed=5)
    lv = M.msssim_levels(a, b)
    for i in (0, 1, 63, 64, 69):
        assert np.array_equal(lv[i], M.msssim_levels(a[i:i + 1], b[i:i + 1])[0])


def test_pix2pix_helper_scores_outputs_against_targets(M):
    import torch
    from gan_lib_tensorflow_amd.Pix2Pix.train import msssim_score
    a, _ = _smooth_pair(2, 64, 64, 3)
    b = np.clip(a.astype(np.int64) + np.random.default_rng(2).integers(-20, 21, size=a.shape), 0, 255).astype(np.uint8)
    ta, tb = torch.from_numpy(a).cuda().float() / 127.5 - 1.0, torch.from_numpy(b).cuda().float() / 127.5 - 1.0
    got = msssim_score(ta, tb)
    want = M.MultiScaleSSIM(a, b)                      # scale invariance: max_val scales with the pixels
    assert want > 0.9 and abs(got - want) <= 1e-5
    assert abs(msssim_score(ta, ta) - 1.0) <= 1e-6


def test_sngan_msssim_diversity(deterministic_stats):
    """(on the fixed-order batch-norm statistics: with the conv epilogues' float atomics two runs of the generator on the same
    noise differ in a few quantised pixels, and the comparison below is for equality)"""
    import torch
    from gan_lib_tensorflow_amd import kernels as K
    from gan_lib_tensorflow_amd.common import msssim as M
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
    torch.cuda.set_device(0)
    tr = SNGANTrainer(batch_size=8, seed=0, use_graphs=False)
    saved = tr.rng_state.clone()
    scores, mean = tr.msssim_diversity(n_pairs=20)
    assert sorted(scores) == list(range(10))
    vals = np.array([scores[k] for k in range(10)])
    assert np.all(np.isfinite(vals)) and np.all(vals > 0.0) and np.all(vals <= 1.0)
    assert mean == float(np.mean(vals))
    # by hand, on the same samples: the same draws after restoring the device RNG state, paired the same way
    tr.rng_state.copy_(saved)
    per_class = {k: [] for k in range(10)}
    while min(len(v) for v in per_class.values()) < 40:
        labels = K.rng_labels(100, 10, tr.rng_state)
        x = tr.sample(100, labels).float().cpu().numpy()
        imgs = ((x + 1.0) * (255.99 / 2)).astype('int32').reshape(-1, 32, 32, 3)     # the quantisation of the IS path
        assert imgs.min() >= 0 and imgs.max() <= 255
        for img, lab in zip(imgs.astype(np.uint8), labels.cpu().numpy()):
            if len(per_class[int(lab)]) < 40:
                per_class[int(lab)].append(img)
    for k in range(10):
        s = np.stack(per_class[k])
        assert M.MultiScaleSSIM(s[0::2], s[1::2]) == scores[k], k


def test_acgan_msssim_diversity():
    import torch
    from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
    torch.cuda.set_device(0)
    tr = ACGANTrainer(batch_size=64, seed=0, use_graphs=False)
    scores, mean = tr.msssim_diversity(n_pairs=8)
    vals = np.array([scores[k] for k in range(10)])
    # an untrained ACGAN generator's samples are close to unrelated noise images: with 8 pairs a class's mean cs can be negative
    # at a coarse level, and the score is then NaN as in the reference (module docstring) -- every other value is a score
    ok = np.isfinite(vals)
    assert sorted(scores) == list(range(10)) and ok.any() and np.all(vals[ok] > 0.0) and np.all(vals[ok] <= 1.0)
    assert np.array_equal(np.array(mean), np.mean(vals), equal_nan=True)
