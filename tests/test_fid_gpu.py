"""GPU: the FID statistics kernels (csrc/fid.hip) against NumPy float64, the fp32 pool_3 of the Inception trunk, and the metric end
to end (gan_lib_tensorflow_amd/common/fid.py, the trainers' `fid`) against the float64 restatement tests/fid_ref.py.

Bounds.  gank_moments_update: the inputs (fp32 or 16-bit) are exact in float64 and so is every product of two of them, so the
only error of an entry is that of its n additions: |G - G_ref| <= 4 n 2^-53 (|X|^T |X|) elementwise, likewise the sums with
sum |x|; the factor 4 covers the reference's own summation order.  gank_mean_hw_f32: HW additions and one division in fp32,
HW 2^-24 mean|x|.  End to end: 1e-9 (tr S1 + tr S2) -- the thresholded eigen form moves by ~1e-15 of that scale under another
summation order (N < D, the rank-deficient path)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref as R  # noqa: E402
from test_inception_gpu import random_params  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
SHAPES = [(1, 16), (3, 16), (4, 48), (5, 64), (37, 80), (130, 272), (100, 2048)]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from gan_lib_tensorflow_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def F(K):
    from gan_lib_tensorflow_amd.common import fid
    return fid


@pytest.fixture(scope="module")
def net(K):
    from gan_lib_tensorflow_amd.common.inception.inception_v3 import InceptionV3
    return InceptionV3(random_params(7))


def upper_tiles(d):
    t = np.arange(d) // 16
    return t[:, None] <= t[None, :]


def features(K, n, d, sixteen_bit, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, d, generator=g) * 0.5 + 0.3
    return (x.to(K.BF16) if sixteen_bit else x).cuda()


def fresh(d):
    """(sum, gram): zeros, with a sentinel in the tiles strictly below the diagonal"""
    gram = torch.zeros(d, d, dtype=torch.float64)
    gram[torch.from_numpy(~upper_tiles(d))] = SENTINEL
    return torch.zeros(d, dtype=torch.float64, device="cuda"), gram.cuda()


def check_moments(total, gram, xs):
    """the device's sums against NumPy float64 on the rows of `xs` (a list of the batches that went in)"""
    x = np.concatenate([b.double().cpu().numpy() for b in xs], axis=0)
    n, d = x.shape
    up = upper_tiles(d)
    g, s = gram.cpu().numpy(), total.cpu().numpy()
    gerr, gbound = np.abs(g - x.T @ x), 4 * n * 2.0 ** -53 * (np.abs(x).T @ np.abs(x))
    serr, sbound = np.abs(s - x.sum(axis=0)), 4 * n * 2.0 ** -53 * np.abs(x).sum(axis=0)
    print(f"n={n} D={d}: worst gram error / bound {np.max(gerr[up] / gbound[up]):.3f}, sum {np.max(serr / sbound):.3f}")
    assert np.all(gerr[up] <= gbound[up])
    assert np.all(serr <= sbound)
    assert np.all(g[~up] == SENTINEL)


@pytest.mark.parametrize("sixteen_bit", [False, True], ids=["f32", "act16"])
@pytest.mark.parametrize("n,d", SHAPES)
def test_moments_update_from_zero(K, n, d, sixteen_bit):
    x = features(K, n, d, sixteen_bit, seed=n * 10000 + d)
    total, gram = fresh(d)
    K.moments_update(x, total, gram)
    check_moments(total, gram, [x])


def test_moments_update_accumulates(K):
    d = 80
    xs = [features(K, n, d, n == 37, seed=n) for n in (5, 37, 100)]
    total, gram = fresh(d)
    for x in xs:
        K.moments_update(x, total, gram)
    check_moments(total, gram, xs)


def test_moments_update_is_deterministic(K):
    x = features(K, 130, 272, False, seed=11)
    runs = []
    for _ in range(2):
        total, gram = fresh(272)
        K.moments_update(x, total, gram)
        runs.append((total, gram))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("n,hw,c", [(2, 1, 16), (5, 9, 40), (3, 64, 2048)])
def test_mean_hw_f32(K, n, hw, c):
    g = torch.Generator().manual_seed(hw)
    x = (torch.randn(n, hw, c, generator=g) + 0.5).to(K.BF16)
    y = K.mean_hw_f32(x.cuda())
    assert y.dtype == torch.float32 and tuple(y.shape) == (n, c)
    xd = x.double()
    err = (y.double().cpu() - xd.mean(1)).abs()
    bound = hw * 2.0 ** -24 * xd.abs().mean(1)
    print(f"n={n} HW={hw} C={c}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


def test_features_f32_is_features_before_the_16_bit_rounding(net):
    rng = np.random.default_rng(2)
    images = torch.tensor(rng.uniform(-1, 1, size=(4, 32, 32, 3)).astype(np.float32))
    f32 = net.features_f32(images)
    f16 = net.features(images).float()
    assert f32.dtype == torch.float32 and tuple(f32.shape) == (4, 2048)
    assert float(f32.abs().mean()) > 1e-3
    assert bool(((f32 - f16).abs() <= 2.0 ** -8 * f32.abs() + 1e-6).all())


@pytest.fixture(scope="module")
def image_sets():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, size=(64, 32, 32, 3), dtype=np.uint8) for _ in range(2)]


@pytest.fixture(scope="module")
def ref_stats(net, image_sets):
    """np.cov statistics of the downloaded features_f32 of the two image sets, pixel values mapped as get_inception_score maps them"""
    out = []
    for imgs in image_sets:
        feats = net.features_f32((2 * (imgs / 255. - 0.5)).astype(np.float32))
        out.append(R.statistics(feats.cpu().numpy()))
    return out


@pytest.fixture(scope="module")
def real_moments(F, net, image_sets):
    return F.image_moments(image_sets[0], net)


def test_fid_end_to_end(F, net, image_sets, ref_stats, tmp_path):
    a, b = image_sets
    (mu1, s1), (mu2, s2) = ref_stats
    scale = np.trace(s1) + np.trace(s2)
    want = R.frechet_eigen(mu1, s1, mu2, s2)
    got = F.calculate_fid(a, b, net)
    print(f"FID (random weights, 64 vs 64 images): product {got!r} restatement {want!r}, scale {scale:.4g}")
    assert want > 0 and abs(got - want) <= 1e-9 * scale
    assert abs(F.calculate_fid(a, a, net)) <= 1e-9 * scale
    path = str(tmp_path / "b.npz")
    F.image_moments(b, net).save(path)
    assert abs(F.calculate_fid(a, path, net) - got) <= 1e-9 * scale
    assert F.image_moments(a, net, batch_size=24).count == 64          # two whole batches and a trailing partial one


def snapshot(tr):
    return {k: v['params'].clone() for k, v in tr.store.flat.items() if 'params' in v}


@pytest.mark.parametrize("which", ["sngan", "acgan"])
def test_trainer_fid_is_an_evaluation_only(F, net, real_moments, monkeypatch, which):
    if which == "sngan":
        from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
        tr, step = SNGANTrainer(batch_size=8, seed=0, use_graphs=False), 'iteration'
    else:
        from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
        tr, step = ACGANTrainer(batch_size=8, seed=0, use_graphs=False), 'global_step'
    real = real_moments
    traces = []
    distance = F.frechet_distance

    def recording(mu1, sigma1, mu2, sigma2):
        traces.append(np.trace(sigma1) + np.trace(sigma2))
        return distance(mu1, sigma1, mu2, sigma2)
    monkeypatch.setattr(F, "frechet_distance", recording)
    before, at = snapshot(tr), getattr(tr, step)
    assert before
    got = tr.fid(real=real, n=200, net=net)
    assert len(traces) == 1 and traces[0] > 0
    assert isinstance(got, float) and np.isfinite(got) and got >= -1e-9 * traces[0]
    assert getattr(tr, step) == at
    after = snapshot(tr)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        tr.fid(real=real, n=100)
