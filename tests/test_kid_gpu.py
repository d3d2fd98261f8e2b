"""GPU: the KID statistics kernels (csrc/kid.hip) against the NumPy float64 restatement tests/kid_ref.py, an exact integer case,
and the metric end to end (gan_lib_tensorflow_amd/common/kid.py, the trainers' `kid`).

Bound, derived and not measured.  The features are float32, so they and every product of two of them are exact in float64.  A
dot product over D features carries at most D roundings; the affine map and the power at most 8 more; each of them moves
t^degree by at most `degree` <= 3 times its relative size; a block sum of P addends carries at most P more in any order.  With
T_ij = gamma sum_k |a_ik| |b_jk| + |coef0| >= |t_ij|:
    |S - S_ref| <= 2 (3 D + 8 + P) 2^-53 sum_ij T_ij^degree,
the factor 2 for the reference's own rounding (kid_ref.sum_bound).  End to end a subset's MMD^2 is within the sum of the three
block bounds, each divided by its normaliser (the last one twice: it enters as -2 sxy / m^2)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kid_ref as R  # noqa: E402
from test_inception_gpu import random_params  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
SHAPES = [(2, 16), (3, 16), (17, 48), (64, 64), (65, 80), (130, 272), (100, 2048)]


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from gan_lib_tensorflow_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def KID(K):
    from gan_lib_tensorflow_amd.common import kid
    return kid


@pytest.fixture(scope="module")
def net(K):
    from gan_lib_tensorflow_amd.common.inception.inception_v3 import InceptionV3
    return InceptionV3(random_params(7))


def banks(m, d, seed):
    """float32 feature banks of different lengths, both longer than m"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(m + 7, d, generator=g) * 0.5 + 0.3
    y = torch.randn(m + 12, d, generator=g) * 0.5 + 0.3
    return x, y


def tables(nx, ny, subsets, m, seed):
    """unsorted row tables without repeats inside a row; later subsets reuse rows of the first"""
    rng = np.random.RandomState(seed)
    out = []
    for n in (nx, ny):
        t = np.stack([rng.permutation(n)[:m] for _ in range(subsets)]).astype(np.int32)
        for s in range(1, subsets):
            if t[0, 0] not in t[s]:
                t[s, -1] = t[0, 0]
        if m > 1 and t[0, 0] < t[0, 1]:
            t[0, :2] = t[0, 1], t[0, 0]
        assert all(len(set(row)) == m for row in t.tolist()) and t[0, 0] > t[0, 1]
        assert all(t[0, 0] in t[s] or t[0, 1] in t[s] for s in range(subsets))
        out.append(t)
    return out


def check_sums(got, x, y, ix, iy, gamma, coef0, degree, what):
    m, d = ix.shape[1], x.shape[1]
    want, absolute = R.block_sums(x.numpy(), y.numpy(), ix, iy, gamma, coef0, degree)
    err, bound = np.abs(got.cpu().numpy() - want), R.sum_bound(absolute, m, d, degree)
    print(f"{what}: worst block-sum error / bound {np.max(err / bound):.4f}")
    assert got.dtype == torch.float64 and tuple(got.shape) == want.shape
    assert np.all(err <= bound)


@pytest.mark.parametrize("subsets", [1, 3])
@pytest.mark.parametrize("m,d", SHAPES)
def test_block_sums(K, m, d, subsets):
    x, y = banks(m, d, seed=m * 10000 + d)
    ix, iy = tables(len(x), len(y), subsets, m, seed=m + d)
    got = K.kid_block_sums(x.cuda(), y.cuda(), ix, iy, 1.0 / d, 1.0, 3)
    check_sums(got, x, y, ix, iy, 1.0 / d, 1.0, 3, f"m={m} D={d} subsets={subsets}")


def test_block_sums_exact_integers(K):
    """Integers in -3..3, gamma = coef0 = 1, degree 3: |dot| <= 9 * 48 = 432, |t^3| <= 433^3 < 8.2e7, a sum of 65^2 of them
    < 3.5e11 -- every intermediate is an integer below 2^53, so the device must return NumPy's int64 sums exactly.  A wrong
    diagonal mask, a tile counted once instead of twice or a row read through the wrong table cannot hide in a tolerance."""
    m, d, subsets = 65, 48, 2
    rng = np.random.RandomState(5)
    x, y = rng.randint(-3, 4, size=(m + 7, d)), rng.randint(-3, 4, size=(m + 12, d))
    ix, iy = tables(len(x), len(y), subsets, m, seed=6)
    want = np.zeros((subsets, 3), np.int64)
    off = ~np.eye(m, dtype=bool)
    for s in range(subsets):
        a, b = x[ix[s]].astype(np.int64), y[iy[s]].astype(np.int64)
        want[s] = [((a @ a.T + 1) ** 3)[off].sum(), ((b @ b.T + 1) ** 3)[off].sum(), ((a @ b.T + 1) ** 3).sum()]
    assert np.abs(want).max() < 3.5e11
    got = K.kid_block_sums(torch.tensor(x, dtype=torch.float32).cuda(), torch.tensor(y, dtype=torch.float32).cuda(), ix, iy, 1.0, 1.0, 3)
    got = got.cpu().numpy()
    print("exact case, device - int64:", (got - want).tolist())
    assert np.array_equal(got, want.astype(np.float64))


def test_symmetric_blocks_from_upper_tiles_only(K):
    """m = 130 is a 3 x 3 tile grid of which XX owns the 6 upper tiles: its sum must be that of the full matrix less its diagonal"""
    m, d = 130, 64
    x, y = banks(m, d, seed=21)
    ix, iy = tables(len(x), len(y), 1, m, seed=22)
    got = K.kid_block_sums(x.cuda(), y.cuda(), ix, iy, 1.0 / d, 1.0, 3).cpu().numpy()
    a = x.double().numpy()[ix[0]]
    full = (a @ a.T / d + 1.0) ** 3
    want = full.sum() - np.trace(full)
    _, absolute = R.block_sums(x.numpy(), y.numpy(), ix, iy, 1.0 / d, 1.0, 3)
    bound = R.sum_bound(absolute, m, d)[0, 0]
    print(f"XX from upper tiles: error / bound {abs(got[0, 0] - want) / bound:.4f}")
    assert abs(got[0, 0] - want) <= bound


def test_buffers_are_written_inside_their_bounds(K):
    m, d, subsets = 65, 80, 3
    x, y = banks(m, d, seed=31)
    ix, iy = tables(len(x), len(y), subsets, m, seed=32)
    tiles = K.kid_num_tiles(m)
    partial = torch.full((subsets + 1, tiles), SENTINEL, dtype=torch.float64, device="cuda")
    out = torch.full((subsets + 1, 3), SENTINEL, dtype=torch.float64, device="cuda")
    got = K.kid_block_sums(x.cuda(), y.cuda(), ix, iy, 1.0 / d, 1.0, 3, partial=partial, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert bool((partial[subsets] == SENTINEL).all()) and bool((out[subsets] == SENTINEL).all())
    assert bool((partial[:subsets] != SENTINEL).all()) and bool((out[:subsets] != SENTINEL).all())
    check_sums(got, x, y, ix, iy, 1.0 / d, 1.0, 3, "caller's buffers")


def test_block_sums_are_deterministic(K):
    m, d = 130, 272
    x, y = banks(m, d, seed=41)
    ix, iy = tables(len(x), len(y), 3, m, seed=42)
    xg, yg = x.cuda(), y.cuda()
    first = K.kid_block_sums(xg, yg, ix, iy, 1.0 / d, 1.0, 3)
    second = K.kid_block_sums(xg, yg, ix, iy, 1.0 / d, 1.0, 3)
    assert torch.equal(first, second)


@pytest.mark.parametrize("degree", [1, 2])
def test_lower_degrees(K, degree):
    m, d = 17, 48
    x, y = banks(m, d, seed=50 + degree)
    ix, iy = tables(len(x), len(y), 3, m, seed=52)
    got = K.kid_block_sums(x.cuda(), y.cuda(), ix, iy, 0.07, 0.5, degree)
    check_sums(got, x, y, ix, iy, 0.07, 0.5, degree, f"degree {degree}")


def test_wrapper_refuses_what_the_kernel_cannot_check(K):
    x, y = banks(17, 48, seed=60)
    ix, iy = tables(len(x), len(y), 1, 17, seed=61)
    bad = ix.copy()
    bad[0, 3] = len(x)
    with pytest.raises(RuntimeError, match="names rows"):
        K.kid_block_sums(x.cuda(), y.cuda(), bad, iy, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.kid_block_sums(x, y.cuda(), ix, iy, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="float32 features"):
        K.kid_block_sums(x.cuda().double(), y.cuda(), ix, iy, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="int32 row tables"):
        K.kid_block_sums(x.cuda(), y.cuda(), ix.astype(np.int64), iy, 1.0, 1.0)


def test_polynomial_mmd2_defaults(KID):
    """gamma=None is 1 / D; without tables it is one subset of all rows in order"""
    m, d = 17, 48
    x, y = banks(m, d, seed=70)
    y = y[:len(x)]
    n = len(x)
    every = np.arange(n, dtype=np.int32)[None, :]
    want_sums, absolute = R.block_sums(x.numpy(), y.numpy(), every, every, 1.0 / d, 1.0, 3)
    bound = R.sum_bound(absolute, n, d)[0]
    tol = bound[0] / (n * (n - 1)) + bound[1] / (n * (n - 1)) + 2 * bound[2] / (n * n)
    got = KID.polynomial_mmd2(x.cuda(), y.numpy())
    assert got.dtype == np.float64 and got.shape == (1,)
    assert abs(got[0] - R.mmd2(want_sums, n)[0]) <= tol
    assert np.array_equal(got, KID.polynomial_mmd2(x.cuda(), y.cuda(), every, every, gamma=1.0 / d))
    with pytest.raises(ValueError, match="equally long"):
        KID.polynomial_mmd2(x.cuda(), y[:-1].cuda())


def test_feature_bank(K, KID):
    bank = KID.FeatureBank(48, 10)
    a = torch.randn(4, 48).to(K.BF16)
    b = np.random.default_rng(0).normal(size=(3, 48))
    bank.append(a.cuda()).append(b)
    assert bank.count == len(bank) == 7 and tuple(bank.features.shape) == (7, 48) and bank.features.dtype == torch.float32
    assert torch.equal(bank.features[:4].cpu(), a.float())
    assert np.array_equal(bank.features[4:].cpu().numpy(), b.astype(np.float32))
    bank.append(torch.zeros(3, 48, device="cuda"))
    with pytest.raises(RuntimeError, match="capacity"):
        bank.append(torch.zeros(1, 48, device="cuda"))
    with pytest.raises(RuntimeError, match="expected"):
        KID.FeatureBank(48, 10).append(torch.zeros(1, 32, device="cuda"))


@pytest.fixture(scope="module")
def image_sets():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, size=(64, 32, 32, 3), dtype=np.uint8) for _ in range(2)]


@pytest.fixture(scope="module")
def feature_banks(KID, net, image_sets):
    return [KID.image_features(imgs, net) for imgs in image_sets]


def test_kid_end_to_end(KID, net, image_sets, feature_banks):
    a, b = image_sets
    subsets, m, seed = 4, 32, 1
    feats = [net.features_f32((2 * (imgs / 255. - 0.5)).astype(np.float32)).cpu().numpy() for imgs in image_sets]
    assert all(torch.equal(bank.features.cpu(), torch.from_numpy(f)) for bank, f in zip(feature_banks, feats))
    rng = np.random.RandomState(seed)
    ix = KID.draw_subsets(64, subsets, m, rng)
    iy = KID.draw_subsets(64, subsets, m, rng)
    mean, std, per, _, absolute = R.kernel_distance(feats[0], feats[1], ix, iy)
    bound = R.sum_bound(absolute, m, 2048)
    tol = bound[:, 0] / (m * (m - 1)) + bound[:, 1] / (m * (m - 1)) + 2 * bound[:, 2] / (m * m)
    got_per = KID.polynomial_mmd2(feature_banks[0], feature_banks[1], ix, iy)
    print(f"MMD^2 per subset (random weights, 64 vs 64 images): product {got_per.tolist()} restatement {per.tolist()}, "
          f"worst error / bound {np.max(np.abs(got_per - per) / tol):.4f}")
    assert np.all(np.abs(got_per - per) <= tol)
    got = KID.calculate_kid(a, b, net, subsets=subsets, subset_size=m, seed=seed)
    assert isinstance(got, tuple) and len(got) == 2 and all(isinstance(v, float) for v in got)
    assert abs(got[0] - mean) <= tol.max() and abs(got[1] - std) <= tol.max()
    assert got == KID.calculate_kid(feature_banks[0], feats[1], subsets=subsets, subset_size=m, seed=seed)
    assert KID.image_features(a, net, batch_size=24).count == 64          # two whole batches and a trailing partial one
    # subset_size is clipped to the 64 rows there are: every subset is the whole sets in another order
    every = np.arange(64, dtype=np.int32)[None, :]
    whole_mean, _, _, _, absolute = R.kernel_distance(feats[0], feats[1], every, every)
    bound = R.sum_bound(absolute, 64, 2048)[0]
    tol = bound[0] / (64 * 63) + bound[1] / (64 * 63) + 2 * bound[2] / (64 * 64)
    clipped = KID.kernel_distance(feature_banks[0], feature_banks[1], subsets=2, subset_size=1000)
    assert abs(clipped[0] - whole_mean) <= tol and clipped[1] <= tol


def test_identical_sides_give_identical_blocks(K, KID, net, image_sets, feature_banks, monkeypatch):
    """a set against itself: with one row table for both sides the XX and YY sums are the same sum, to the bit (the two blocks
    stage the same rows and add in the same order); through calculate_kid(a, a) the two tables differ, both blocks are sums
    over rows of one bank and the distance is of the size of its own deviation"""
    bank = feature_banks[0]
    ix = KID.draw_subsets(64, 4, 32, np.random.RandomState(1))
    sums = K.kid_block_sums(bank.features, bank.features, ix, ix, 1.0 / 2048, 1.0, 3)
    assert torch.equal(sums[:, 0], sums[:, 1])
    seen = []
    block_sums = K.kid_block_sums

    def recording(x, y, *args, **kw):
        seen.append((x, y))
        return block_sums(x, y, *args, **kw)
    monkeypatch.setattr(K, "kid_block_sums", recording)
    mean, std = KID.calculate_kid(image_sets[0], image_sets[0], net, subsets=4, subset_size=32, seed=1)
    assert len(seen) == 1 and torch.equal(seen[0][0], seen[0][1])
    assert np.isfinite(mean) and std > 0


def snapshot(tr):
    return {k: v['params'].clone() for k, v in tr.store.flat.items() if 'params' in v}


@pytest.mark.parametrize("which", ["sngan", "acgan"])
def test_trainer_kid_is_an_evaluation_only(net, feature_banks, which):
    if which == "sngan":
        from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
        tr, step = SNGANTrainer(batch_size=8, seed=0, use_graphs=False), 'iteration'
    else:
        from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
        tr, step = ACGANTrainer(batch_size=8, seed=0, use_graphs=False), 'global_step'
    real = feature_banks[0]
    before, at = snapshot(tr), getattr(tr, step)
    assert before
    got = tr.kid(real=real, n=200, net=net, subsets=3, subset_size=50)
    assert isinstance(got, tuple) and len(got) == 2
    assert all(isinstance(v, float) and np.isfinite(v) for v in got) and got[1] >= 0
    assert getattr(tr, step) == at
    after = snapshot(tr)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        tr.kid(real=real, n=100)
