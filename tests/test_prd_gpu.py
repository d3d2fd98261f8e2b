"""GPU: the k-NN radii and manifold-count kernels (csrc/prd.hip) against the NumPy float64 restatement tests/prd_ref.py, an exact
integer case, and the metric end to end (gan_lib_tensorflow_amd/common/precision_recall.py, the trainers' `precision_recall`).

The bound on a squared distance is derived in prd_ref (|d2 - d2_ref| <= 2 (D + 4) 2^-53 sum_k (|a_ik| + |b_jk|)^2); a radius and
a nearest distance are order statistics of such values and move by at most the row's largest bound.  Counts are compared with
==: tests/test_prd_cpu.py shows on the reference alone that at every shape used here no comparison of a distance with a radius
and no choice of a k-th neighbour lies within that bound."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prd_ref as R  # noqa: E402
from test_inception_gpu import random_params  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from gan_lib_tensorflow_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def PR(K):
    from gan_lib_tensorflow_amd.common import precision_recall
    return precision_recall


@pytest.fixture(scope="module")
def net(K):
    from gan_lib_tensorflow_amd.common.inception.inception_v3 import InceptionV3
    return InceptionV3(random_params(7))


def dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float32)).cuda()      # a copy: the reference's arrays are read-only


@pytest.mark.parametrize("nx,ny,d,k", R.cases())
def test_knn_radii(K, nx, ny, d, k):
    ref = R.reference(nx, ny, d, k)
    for name in ("x", "y"):
        bank = ref[name]
        got = K.prd_knn_radii(dev(bank), k)
        assert got.dtype == torch.float64 and tuple(got.shape) == (len(bank),)
        err, bound = np.abs(got.cpu().numpy() - ref["radii_" + name]), ref["radii_bound_" + name]
        print(f"({nx},{ny},{d}) k={k} bank {name}: worst radius error / bound {np.max(err / bound):.4f}")
        assert np.all(err <= bound)


@pytest.mark.parametrize("nx,ny,d,k", R.cases())
def test_manifold_counts_and_the_four_values(K, PR, nx, ny, d, k):
    ref = R.reference(nx, ny, d, k)
    x, y = dev(ref["x"]), dev(ref["y"])
    for what, q, bank, radii, bound in (("fake_in_real", y, x, ref["radii_x"], ref["nearest_bound_fake"]),
                                        ("real_in_fake", x, y, ref["radii_y"], ref["nearest_bound_real"])):
        count, nearest = K.prd_manifold_counts(q, bank, torch.tensor(radii).cuda())
        want_count, want_nearest = ref[what]
        assert count.dtype == torch.int32 and nearest.dtype == torch.float64 and tuple(count.shape) == tuple(nearest.shape) == (len(q),)
        err = np.abs(nearest.cpu().numpy() - want_nearest)
        print(f"({nx},{ny},{d}) k={k} {what}: counts differ in {int((count.cpu().numpy() != want_count).sum())} rows, "
              f"worst nearest2 error / bound {np.max(err / bound):.4f}")
        assert np.array_equal(count.cpu().numpy(), want_count)
        assert np.all(err <= bound)
    got = PR.calculate_prdc(x, y, k=k)
    print(f"({nx},{ny},{d}) k={k}: product {got} restatement {ref['prdc']}")
    assert all(isinstance(v, float) for v in got.values())
    assert got == ref["prdc"]
    assert PR.precision_recall(x, y, k=k) == (got["precision"], got["recall"])
    assert PR.density_coverage(x, y, k=k) == (got["density"], got["coverage"])


def test_exact_integers(K):
    """Integer features: every d2 is an integer of at most 16 * 49, exact in float64 in any order, so radii, counts and nearest2
    must equal the int64 computation bit for bit.  The seed has elements equal to their radius, rows with equal k-th and
    (k+1)-th distances and a duplicated row (tests/test_prd_cpu.py asserts it): a non-inclusive comparison, a self-exclusion by
    value or a mask off by one column cannot hide."""
    xi, yi = R.integer_banks()
    x, y, k = dev(xi), dev(yi), 3
    for bank, ints in ((x, xi), (y, yi)):
        for kk in (1, k):
            got = K.prd_knn_radii(bank, kk).cpu().numpy()
            assert np.array_equal(got, R.integer_radii(ints, kk).astype(np.float64)), kk
    first = K.prd_knn_radii(x, 1).cpu().numpy()
    assert first[7] == 0.0 and first[40] == 0.0                 # rows 7 and 40 are copies of each other
    for q, qi, bank, bi in ((y, yi, x, xi), (x, xi, y, yi), (x, xi, x, xi)):
        radii = R.integer_radii(bi, k)
        d = R.integer_d2(qi, bi)
        count, nearest = K.prd_manifold_counts(q, bank, torch.from_numpy(radii.astype(np.float64)).cuda())
        print("exact case, counts device - int64:", (count.cpu().numpy() - (d <= radii[None, :]).sum(axis=1)).tolist())
        assert np.array_equal(count.cpu().numpy(), (d <= radii[None, :]).sum(axis=1))
        assert np.array_equal(nearest.cpu().numpy(), d.min(axis=1).astype(np.float64))


@pytest.mark.parametrize("nx,ny,d", [(130, 142, 272), (300, 257, 64)])
def test_segments_do_not_change_a_bit(K, nx, ny, d):
    """selection and integer sums do not depend on the cut.  142 rows are 3 column tiles, the last of 14 columns: with 3
    segments the last segment is that partial tile alone; 257 rows are 5 tiles, the last of 1 column."""
    k = 3
    ref = R.reference(nx, ny, d, k)
    x, y = dev(ref["x"]), dev(ref["y"])
    radii_y = K.prd_knn_radii(y, k, segments=1)
    base = K.prd_manifold_counts(x, y, radii_y, segments=1)
    for segments in (2, 3, None):
        assert torch.equal(K.prd_knn_radii(y, k, segments=segments), radii_y), segments
        count, nearest = K.prd_manifold_counts(x, y, radii_y, segments=segments)
        assert torch.equal(count, base[0]) and torch.equal(nearest, base[1]), segments
    assert K.prd_default_segments(ny) == (ny + 63) // 64       # the default is the finest cut here: one tile per segment
    with pytest.raises(RuntimeError, match="segments = 6"):
        K.prd_knn_radii(y, k, segments=6)


def test_buffers_are_written_inside_their_bounds(K):
    nx, ny, d, k, segments = 65, 77, 80, 3, 2
    ref = R.reference(nx, ny, d, k)
    x, y = dev(ref["x"]), dev(ref["y"])
    part = torch.full((nx + 1, segments * k), SENTINEL, dtype=torch.float64, device="cuda")
    out = torch.full((nx + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    radii = K.prd_knn_radii(x, k, segments=segments, part=part, out=out)
    assert radii.data_ptr() == out.data_ptr() and tuple(radii.shape) == (nx,)
    assert bool((part[nx] == SENTINEL).all()) and float(out[nx]) == SENTINEL
    assert bool((part[:nx] != SENTINEL).all()) and bool((out[:nx] != SENTINEL).all())
    assert np.all(np.abs(radii.cpu().numpy() - ref["radii_x"]) <= ref["radii_bound_x"])
    need = K.prd_counts_partial_len(ny, segments)
    partial = torch.full((need + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    counts = torch.full((ny + 1,), -7, dtype=torch.int32, device="cuda")
    nearest = torch.full((ny + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    got = K.prd_manifold_counts(y, x, radii, segments=segments, partial=partial, counts=counts, nearest=nearest)
    assert got[0].data_ptr() == counts.data_ptr() and got[1].data_ptr() == nearest.data_ptr()
    assert bool((partial[need:] == SENTINEL).all()) and int(counts[ny]) == -7 and float(nearest[ny]) == SENTINEL
    assert bool((partial[:ny * segments] != SENTINEL).all()) and bool((nearest[:ny] != SENTINEL).all()) and bool((counts[:ny] >= 0).all())
    assert np.array_equal(got[0].cpu().numpy(), ref["fake_in_real"][0])
    with pytest.raises(RuntimeError, match="part .* holds fewer"):
        K.prd_knn_radii(x, k, segments=segments, part=part.view(-1)[:nx * segments * k - 1])
    with pytest.raises(RuntimeError, match="out .* is smaller"):
        K.prd_knn_radii(x, k, out=out[:nx - 1])
    with pytest.raises(RuntimeError, match="partial .* holds fewer"):
        K.prd_manifold_counts(y, x, radii, segments=segments, partial=partial[:need - 1])
    with pytest.raises(RuntimeError, match="counts .* is smaller"):
        K.prd_manifold_counts(y, x, radii, counts=counts[:ny - 1])
    with pytest.raises(RuntimeError, match="nearest .* is smaller"):
        K.prd_manifold_counts(y, x, radii, nearest=nearest[:ny - 1])


def test_two_calls_return_the_same_bits(K):
    ref = R.reference(130, 142, 272, 3)
    x, y = dev(ref["x"]), dev(ref["y"])
    radii = K.prd_knn_radii(x, 3)
    assert torch.equal(radii, K.prd_knn_radii(x, 3))
    first, second = K.prd_manifold_counts(y, x, radii), K.prd_manifold_counts(y, x, radii)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_a_set_against_itself_and_against_a_distant_copy(PR):
    x = np.array(R.reference(130, 142, 272, 3)["x"])         # a copy: the reference's arrays are read-only
    assert len(np.unique(x, axis=0)) == len(x)
    same = PR.calculate_prdc(x, x)
    assert same["precision"] == same["recall"] == same["coverage"] == 1.0 and same["density"] >= 1.0 / 3
    far = PR.calculate_prdc(x, x + np.float32(100.0))
    assert far == dict(precision=0.0, recall=0.0, density=0.0, coverage=0.0)


def test_wrapper_refusals(K):
    ref = R.reference(17, 23, 48, 3)
    x, y = dev(ref["x"]), dev(ref["y"])
    radii = K.prd_knn_radii(x, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.prd_knn_radii(x.cpu(), 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.prd_manifold_counts(y.cpu(), x, radii)
    with pytest.raises(RuntimeError, match="float32 features"):
        K.prd_knn_radii(x.double(), 3)
    with pytest.raises(RuntimeError, match="float32 features"):
        K.prd_manifold_counts(y, x.double(), radii)
    with pytest.raises(RuntimeError, match="differ in the feature width"):
        K.prd_manifold_counts(y[:, :32].contiguous(), x, radii)
    with pytest.raises(RuntimeError, match=r"radii2 float64 \[17\]"):
        K.prd_manifold_counts(y, x, radii[:16])
    with pytest.raises(RuntimeError, match=r"radii2 float64 \[17\]"):
        K.prd_manifold_counts(y, x, radii.float())
    with pytest.raises(RuntimeError, match="k = 0"):
        K.prd_knn_radii(x, 0)
    with pytest.raises(RuntimeError, match="k = 9"):
        K.prd_knn_radii(x, 9)
    with pytest.raises(RuntimeError, match="at least 4"):
        K.prd_knn_radii(x[:3].contiguous(), 3)


@pytest.fixture(scope="module")
def image_sets():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, size=(64, 32, 32, 3), dtype=np.uint8) for _ in range(2)]


@pytest.fixture(scope="module")
def feature_banks(net, image_sets):
    from gan_lib_tensorflow_amd.common import kid
    return [kid.image_features(imgs, net) for imgs in image_sets]


def test_prdc_through_inception(PR, net, image_sets, feature_banks):
    """plumbing only: features of noise under random weights may be nearly tied, parity with the restatement is carried by the
    kernel tests above"""
    from gan_lib_tensorflow_amd.common import kid
    a, b = image_sets
    got = PR.calculate_prdc(a, b, net)
    print("random weights, 64 vs 64 noise images:", got)
    assert sorted(got) == ["coverage", "density", "precision", "recall"] and all(isinstance(v, float) for v in got.values())
    assert all(0.0 <= got[name] <= 1.0 for name in ("precision", "recall", "coverage")) and got["density"] >= 0.0
    assert got == PR.calculate_prdc(feature_banks[0], feature_banks[1].features.cpu().numpy())
    partial_batches = kid.image_features(a, net, batch_size=24)          # two whole batches and a trailing partial one
    assert partial_batches.count == 64
    again = PR.calculate_prdc(partial_batches, feature_banks[1])
    assert all(0.0 <= again[name] <= 1.0 for name in ("precision", "recall", "coverage")) and again["density"] >= 0.0
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        PR.calculate_prdc(a, feature_banks[1])


def snapshot(tr):
    return {k: v['params'].clone() for k, v in tr.store.flat.items() if 'params' in v}


@pytest.mark.parametrize("which", ["sngan", "acgan"])
def test_trainer_precision_recall_is_an_evaluation_only(net, feature_banks, which):
    if which == "sngan":
        from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
        tr, step = SNGANTrainer(batch_size=8, seed=0, use_graphs=False), 'iteration'
    else:
        from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
        tr, step = ACGANTrainer(batch_size=8, seed=0, use_graphs=False), 'global_step'
    real = feature_banks[0]
    before, at = snapshot(tr), getattr(tr, step)
    assert before
    got = tr.precision_recall(real=real, n=200, net=net)
    assert sorted(got) == ["coverage", "density", "precision", "recall"]
    assert all(isinstance(v, float) and np.isfinite(v) for v in got.values())
    assert getattr(tr, step) == at
    after = snapshot(tr)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        tr.precision_recall(real=real, n=100)
