"""GPU: the per-sample score kernels (csrc/prd.hip: gank_prd_scores_*) and common/sample_scores.py against the NumPy float64
restatement tests/sample_scores_ref.py: integer cases that must agree bit for bit, invariance under the segment count, Gaussian
features within the derived bounds, consistency with the manifold counts of the same file, the refusals of the entry points, and
the trainers' `sample_scores`.  What the shared cases contain is asserted on the reference alone in
tests/test_sample_scores_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prd_ref  # noqa: E402
import sample_scores_ref as S  # noqa: E402
from test_inception_gpu import random_params  # noqa: E402
from test_sample_scores_cpu import entry_points_refuse  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from gan_lib_tensorflow_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def SS(K):
    from gan_lib_tensorflow_amd.common import sample_scores
    return sample_scores


@pytest.fixture(scope="module")
def net(K):
    from gan_lib_tensorflow_amd.common.inception.inception_v3 import InceptionV3
    return InceptionV3(random_params(7))


def dev(a, dtype=np.float32):
    return torch.tensor(np.asarray(a, dtype=dtype)).cuda()      # a copy: the reference's arrays are read-only


def host(pair):
    return tuple(t.cpu().numpy() for t in pair)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def segment_counts(nr):
    tiles = (nr + S.tile_width() - 1) // S.tile_width()
    return sorted({1, min(2, tiles), tiles})            # 1, 2 and the most the entry point allows: one tile a segment


@pytest.mark.parametrize("d,nq,nr,k", S.exact_cases())
def test_exact_integers(K, SS, d, nq, nr, k):
    """Integer features in -3..3: every d2 and radii2 is an exact integer and a ratio one correctly rounded division, so the
    kernel's values and the scores built on them must equal the restatement's bit for bit, whatever the segment count.  The
    cases hold duplicated bank rows (radius 0 at k = 1), queries copied from bank rows (+inf), pairs on a ball's boundary and,
    under prune = 0.5, a query whose nearest row is pruned (tests/test_sample_scores_cpu.py asserts all of it)."""
    e = S.exact_case(d, nq, nr, k)
    q, r = dev(e['q']), dev(e['r'])
    assert same_bits(K.prd_knn_radii(r, k).cpu().numpy(), e['radii2'])
    for radii2, ratio2, rare2 in ((e['radii2'], e['ratio2'], e['rare2']), (e['pruned2'], e['ratio2_pruned'], e['rare2_pruned'])):
        for segments in segment_counts(nr) + [None]:
            got = K.prd_sample_scores(q, r, dev(radii2, np.float64), segments=segments)
            assert got[0].dtype == got[1].dtype == torch.float64 and tuple(got[0].shape) == tuple(got[1].shape) == (nq,)
            got = host(got)
            print(f"({d},{nq},{nr}) k={k} segments={segments}: ratio2 differs in {int((got[0] != ratio2).sum())} rows, "
                  f"rare2 in {int((got[1] != rare2).sum())}")
            assert same_bits(got[0], ratio2) and same_bits(got[1], rare2)
    assert same_bits(SS.realism_scores(r, q, k=k), e['realism'])                      # prune = 0.5 is the default
    assert same_bits(SS.realism_scores(r, q, k=k, prune=0), e['realism_all'])
    score, inside = SS.rarity_scores(r, q, k=k)
    assert same_bits(score, e['rarity']) and same_bits(inside, e['inside'])
    both = SS.calculate_sample_scores(np.array(e['r']), np.array(e['q']), k=k)        # NumPy sides (copies: the case is read-only)
    want = S.sample_scores(e['r'], e['q'], k)
    assert sorted(both) == sorted(want)
    for name, value in want.items():
        if isinstance(value, np.ndarray):
            assert same_bits(both[name], value), name
        else:
            assert isinstance(both[name], float) and (both[name] == value or (np.isnan(value) and np.isnan(both[name]))), name


def test_pruning_leaves_the_callers_radii_alone(K, SS):
    e = S.exact_case(16, 65, 129, 1)
    radii2 = dev(e['radii2'], np.float64)
    pruned = SS.pruned_radii(radii2, 0.5)
    assert same_bits(radii2.cpu().numpy(), e['radii2']) and same_bits(pruned.cpu().numpy(), e['pruned2'])
    assert SS.pruned_radii(radii2, 0) is radii2
    all_pruned = K.prd_sample_scores(dev(e['q']), dev(e['r']), torch.full_like(radii2, -1.0))
    assert bool((all_pruned[0] == -np.inf).all()) and bool((all_pruned[1] == np.inf).all())


def test_segments_and_calls_do_not_change_a_bit(K):
    """max and min do not depend on the cut: 142 rows are 3 column tiles, the last of 14 columns; 257 rows 5 tiles, the last of
    1 column.  Every allowed segment count, the default, and a second call."""
    for nx, ny, d in ((130, 142, 272), (300, 257, 64)):
        ref = prd_ref.reference(nx, ny, d, 3)
        x, y = dev(ref['x']), dev(ref['y'])
        radii2 = K.prd_knn_radii(y, 3)
        base = K.prd_sample_scores(x, y, radii2, segments=1)
        tiles = (ny + S.tile_width() - 1) // S.tile_width()
        for segments in list(range(1, tiles + 1)) + [None, 1]:
            got = K.prd_sample_scores(x, y, radii2, segments=segments)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), segments
        with pytest.raises(RuntimeError, match=f"segments = {tiles + 1}"):
            K.prd_sample_scores(x, y, radii2, segments=tiles + 1)


def test_gaussian_features(K):
    """D = 2048, 130 queries against 200 bank rows, independent normal features; the kernel gets the restatement's radii2, so
    both sides compare and divide the same values.
    rare2: a row is set aside when one of its inclusion tests has a margin |d2_ij - radii2_j| within prd_ref.d2_bound (2 (D + 4)
    2^-53 sum_k (|a_ik| + |b_jk|)^2, the kernel's and the reference's roundings); on every other row each test has the
    reference's outcome and rare2, a copy of one radii2[j], must be EQUAL.  At most 1 % of the rows may be set aside; the seed
    sets aside none (tests/test_sample_scores_cpu.py).
    ratio2: relative error at most sample_scores_ref.ratio_rel_bound(D) = (4 (D + 4) + 4) 2^-53 = 9.12e-13 at D = 2048 -- a
    pair's d2 is off by at most the bound above, which is at most 4 (D + 4) 2^-53 d2_ij here because sum_k (|a_ik| + |b_jk|)^2
    <= 2 d2_ij on this data (asserted on the reference), two roundings of the divisions, and a maximum moves by no more than
    its elements."""
    g = S.gaussian_case()
    q, r = dev(g['q']), dev(g['r'])
    bound = S.ratio_rel_bound(S.GAUSS['d'])
    for name, radii2, ratio2, rare2 in (("all balls", g['radii2'], g['ratio2'], g['rare2']),
                                        ("prune = 0.5", g['pruned2'], g['ratio2_pruned'], g['rare2_pruned'])):
        aside = S.undecided_rows(g['q'], g['r'], radii2)
        got = host(K.prd_sample_scores(q, r, dev(radii2, np.float64)))
        rel = np.abs(got[0] - ratio2) / ratio2
        print(f"{name}: {int(aside.sum())} rows set aside, rare2 differs in {int((got[1][~aside] != rare2[~aside]).sum())} of the others, "
              f"worst relative ratio2 error {rel.max():.3g} (bound {bound:.3g})")
        assert aside.sum() <= len(aside) // 100
        assert np.array_equal(got[1][~aside], rare2[~aside])
        assert np.all(rel <= bound)


def test_consistent_with_the_manifold_counts(K, SS):
    """the same strips, the same d2 bits: a row is inside exactly when its count is positive, and without pruning its realism is
    >= 1 exactly then (radii2 / d2 rounds to >= 1 if and only if d2 <= radii2, and so does its square root)"""
    g = S.gaussian_case()
    ref = prd_ref.reference(130, 142, 272, 3)
    for real, fake in ((g['r'], g['q']), (ref['x'], ref['y'])):
        real, fake = dev(real), dev(fake)
        count, _ = K.prd_manifold_counts(fake, real, K.prd_knn_radii(real, 3))
        positive = count.cpu().numpy() > 0
        assert 0 < positive.sum() < len(positive)
        score, inside = SS.rarity_scores(real, fake, k=3)
        assert np.array_equal(inside, positive) and np.array_equal(score > 0, positive)
        assert np.array_equal(SS.realism_scores(real, fake, k=3, prune=0) >= 1.0, positive)
        pruned = SS.realism_scores(real, fake, k=3) >= 1.0
        assert np.all(positive[pruned]) and pruned.sum() <= positive.sum()        # fewer balls: a subset


def test_refusals(K):
    from gan_lib_tensorflow_amd import _lib
    entry_points_refuse(_lib.load())
    torch.cuda.synchronize()                      # nothing was launched: there is no error to surface
    e = S.exact_case(16, 65, 63, 3)
    q, r, radii2 = dev(e['q']), dev(e['r']), dev(e['radii2'], np.float64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.prd_sample_scores(q.cpu(), r, radii2)
    with pytest.raises(RuntimeError, match="float32 features"):
        K.prd_sample_scores(q, r.double(), radii2)
    with pytest.raises(RuntimeError, match="differ in the feature width"):
        K.prd_sample_scores(dev(np.zeros((4, 32))), r, radii2)
    with pytest.raises(RuntimeError, match=r"radii2 float64 \[63\]"):
        K.prd_sample_scores(q, r, radii2[:62])
    with pytest.raises(RuntimeError, match=r"radii2 float64 \[63\]"):
        K.prd_sample_scores(q, r, radii2.float())
    with pytest.raises(RuntimeError, match=r"radii2 float64 \[63\]"):
        K.prd_sample_scores(q, r, radii2.cpu())
    with pytest.raises(RuntimeError, match="segments = 0"):
        K.prd_sample_scores(q, r, radii2, segments=0)
    with pytest.raises(RuntimeError, match="misaligned"):
        K.prd_sample_scores(torch.zeros(4 * 16 + 2, device="cuda")[2:].view(4, 16), r, radii2)       # contiguous, 8 bytes off


def test_trainer_sample_scores(SS, net):
    from gan_lib_tensorflow_amd.common import kid
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
    rng = np.random.default_rng(3)
    real = kid.image_features(rng.integers(0, 256, size=(64, 32, 32, 3), dtype=np.uint8), net)
    tr = SNGANTrainer(batch_size=8, seed=0, use_graphs=False)
    before = {k: v['params'].clone() for k, v in tr.store.flat.items() if 'params' in v}
    n = 150                                      # a whole pass of 100 and one cut to 50
    got = tr.sample_scores(real=real, n=n, net=net)
    assert sorted(got) == ["inside", "mean_rarity", "mean_realism", "rarity", "realism", "realistic_fraction", "samples"]
    assert got['realism'].shape == got['rarity'].shape == got['inside'].shape == (n,)
    assert got['realism'].dtype == got['rarity'].dtype == np.float64 and got['inside'].dtype == np.bool_
    assert got['samples'].is_cuda and got['samples'].dtype == torch.uint8 and tuple(got['samples'].shape) == (n, 32, 32, 3)
    assert all(isinstance(got[name], float) for name in ("mean_rarity", "mean_realism", "realistic_fraction"))
    again = SS.calculate_sample_scores(real, got['samples'], net)
    for name in ("realism", "rarity", "inside"):
        assert same_bits(got[name], again[name]), name
    assert got['realistic_fraction'] == again['realistic_fraction'] == float(np.mean(got['realism'] >= 1.0))
    assert all(torch.equal(before[k], v['params']) for k, v in tr.store.flat.items() if 'params' in v)      # an evaluation only
    best = SS.rank_samples(got['realism'], 8)
    assert tuple(got['samples'][torch.from_numpy(best).cuda()].shape) == (8, 32, 32, 3)
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        tr.sample_scores(real=real, n=100)
