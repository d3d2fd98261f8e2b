"""GPU: the sliced Wasserstein kernels (csrc/swd.hip) against the NumPy float64 restatement tests/swd_ref.py -- the pyramid of
uint8 images with ==, the sort with np.array_equal against np.sort, the sorted L1 on integers exactly, statistics and projection
within the bound derived in swd_ref (tests/test_swd_cpu.py shows it is far below the values) -- and the metric end to end
(gan_lib_tensorflow_amd/common/swd.py, the trainers' `swd`, Pix2Pix's `swd_score`)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from gan_lib_tensorflow_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def S(K):
    from gan_lib_tensorflow_amd.common import swd
    return swd


def dev(a, dtype=np.float64):
    return torch.tensor(np.asarray(a, dtype=dtype)).cuda()      # a copy: the reference's arrays are read-only


# ---- pyramid
@pytest.mark.parametrize("shape", [(2, 16, 16, 3), (2, 32, 32, 3), (2, 8, 12, 1), (2, 4, 4, 3)])
def test_pyramid_of_uint8_is_exact(K, shape):
    n, h, w, c = shape
    x = np.random.RandomState(1).randint(0, 256, size=shape).astype(np.uint8)
    coarse_ref = R.pyr_down(x)
    fine_ref = x.astype(np.float64) - R.pyr_up(coarse_ref)
    need = coarse_ref.size
    buf = torch.full((need + 64,), SENTINEL, dtype=torch.float64, device="cuda")
    coarse = K.swd_pyr_down(dev(x), out=buf)
    assert coarse.data_ptr() == buf.data_ptr() and tuple(coarse.shape) == (n, h // 2, w // 2, c)
    assert bool((buf[need:] == SENTINEL).all())
    assert np.array_equal(coarse.cpu().numpy(), coarse_ref)
    fine_buf = torch.full((x.size + 64,), SENTINEL, dtype=torch.float64, device="cuda")
    fine = fine_buf[:x.size].view(shape)
    fine.copy_(dev(x))
    assert K.swd_laplacian(fine, coarse).data_ptr() == fine.data_ptr()
    assert bool((fine_buf[x.size:] == SENTINEL).all()) and bool((buf[need:] == SENTINEL).all())
    assert np.array_equal(fine.cpu().numpy(), fine_ref)
    assert np.array_equal(coarse.cpu().numpy(), coarse_ref)          # the coarse level is only read


def test_pyramid_of_float32_within_a_25_term_dot(K, S):
    x = np.random.RandomState(2).uniform(-1, 1, size=(2, 32, 32, 3)).astype(np.float32)
    levels = S.laplacian_pyramid(x)
    ref = R.laplacian_pyramid(x)
    assert [tuple(lv.shape) for lv in levels] == [(2, 32, 32, 3), (2, 16, 16, 3)] and all(lv.dtype == torch.float64 for lv in levels)
    # 25 products of weights that sum to 1 (4 for pyr_up's non-zero taps: at most 1 as well) with |x| <= 1, in any order:
    # (25 + 1) u each for the product and the restatement; level 0 adds pyr_down's error carried through pyr_up and one subtraction
    u = 2.0 ** -53
    err1, err0 = np.abs(levels[1].cpu().numpy() - ref[1]).max(), np.abs(levels[0].cpu().numpy() - ref[0]).max()
    print(f"float32 pyramid: level 1 error {err1:.3e} (bound {2 * 26 * u:.3e}), level 0 error {err0:.3e} (bound {2 * (2 * 26 + 2) * u:.3e})")
    assert err1 <= 2 * 26 * u and err0 <= 2 * (2 * 26 + 2) * u


def test_pyramid_refusals(K):
    x = torch.zeros((2, 16, 16, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.swd_pyr_down(x.cpu())
    with pytest.raises(RuntimeError, match="float64 images"):
        K.swd_pyr_down(x.float())
    with pytest.raises(RuntimeError, match="cannot be halved"):
        K.swd_pyr_down(x[:, :, :5].contiguous())
    with pytest.raises(RuntimeError, match="cannot be halved"):
        K.swd_pyr_down(x[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="out .* holds fewer"):
        K.swd_pyr_down(x, out=torch.empty(2 * 8 * 8 * 3 - 1, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError, match="not the half-size level"):
        K.swd_laplacian(x, torch.zeros((2, 8, 4, 3), dtype=torch.float64, device="cuda"))


# ---- sort
def sort_contents(name, dirs, m, rng):
    if name == "normal":
        return rng.randn(dirs, m)
    if name == "ties":
        return rng.randint(-3, 4, size=(dirs, m)).astype(np.float64)
    if name == "equal":
        return np.full((dirs, m), 2.5)
    if name == "sorted":
        return np.sort(rng.randn(dirs, m), axis=1)
    if name == "reversed":
        return np.sort(rng.randn(dirs, m), axis=1)[:, ::-1].copy()
    pool = np.array([1e300, -1e300, 1e-300, -1e-300, 5e-324, -5e-324, 2.5e-310, -2.5e-310, 1.0, -1.0, 0.0, np.finfo(np.float64).tiny])
    return pool[rng.randint(0, len(pool), size=(dirs, m))]


SORT_SHAPES = [(1, 1), (3, 1), (1, 2), (3, 2), (3, 255), (3, 256), (128, 257), (1, 4099), (3, 4099), (1, 70001), (3, 70001)]


@pytest.mark.parametrize("dirs,m", SORT_SHAPES)
def test_sort_rows_equals_numpy(K, dirs, m):
    rng = np.random.RandomState(dirs * 100003 + m)
    for name in ("normal", "ties", "equal", "sorted", "reversed", "extremes"):
        keys = sort_contents(name, dirs, m, rng)
        assert np.all(np.isfinite(keys)) and not np.any(np.signbit(keys) & (keys == 0))       # the contract: no NaN, no -0.0
        want = np.sort(keys, axis=1)
        buf = torch.full((dirs * m + 64,), SENTINEL, dtype=torch.float64, device="cuda")
        tmp = torch.full((dirs * m + 64,), SENTINEL, dtype=torch.float64, device="cuda")
        hist = torch.full((K.swd_sort_ws_elems(dirs, m) + 64,), -7, dtype=torch.int32, device="cuda")
        view = buf[:dirs * m].view(dirs, m)
        view.copy_(dev(keys))
        got = K.swd_sort_rows(view, tmp=tmp, hist=hist)
        assert got.data_ptr() == buf.data_ptr()
        assert bool((buf[dirs * m:] == SENTINEL).all()) and bool((tmp[dirs * m:] == SENTINEL).all()) and bool((hist[-64:] == -7).all())
        got = got.cpu().numpy()
        assert np.array_equal(got, want), (name, int((got != want).sum()))      # equal to np.sort: a permutation, same multiset
        again = dev(keys)
        K.swd_sort_rows(again)
        assert np.array_equal(again.cpu().numpy().view(np.int64), got.view(np.int64)), name           # two calls, equal bits


def test_sort_refusals(K):
    limit = K.swd_sort_max_rows()
    assert limit == 1 << 24
    with pytest.raises(RuntimeError, match=f"M = {limit + 1} keys a row unsupported"):
        K.swd_sort_rows(torch.empty((1, limit + 1), dtype=torch.float64, device="cuda"))
    keys = torch.zeros((3, 300), dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.swd_sort_rows(keys.cpu())
    with pytest.raises(RuntimeError, match="float64 keys"):
        K.swd_sort_rows(keys.float())
    with pytest.raises(RuntimeError, match="float64 keys"):
        K.swd_sort_rows(keys.view(-1))
    with pytest.raises(RuntimeError, match="tmp .* holds fewer"):
        K.swd_sort_rows(keys, tmp=torch.empty(899, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError, match="hist .* holds fewer"):
        K.swd_sort_rows(keys, hist=torch.empty(3 * 256 - 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="same buffer"):
        K.swd_sort_rows(keys, tmp=keys)


# ---- sorted L1
@pytest.mark.parametrize("m", [257, 4099])
def test_sorted_l1_on_integers_is_exact(K, m):
    rng = np.random.RandomState(m)
    a, b = rng.randint(-1000, 1000, size=(3, m)), rng.randint(-1000, 1000, size=(3, m))
    parts = K.swd_sorted_l1_parts(m)
    buf = torch.full((3 * parts + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    got = K.swd_sorted_l1(dev(a), dev(b), part=buf)
    assert tuple(got.shape) == (3, parts) and bool((buf[3 * parts:] == SENTINEL).all())
    assert np.array_equal(got.cpu().numpy().sum(axis=1), np.abs(a - b).sum(axis=1).astype(np.float64))
    assert torch.equal(got, K.swd_sorted_l1(dev(a), dev(b)))
    with pytest.raises(RuntimeError, match="differ"):
        K.swd_sorted_l1(dev(a), dev(b[:, :-1]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.swd_sorted_l1(dev(a).cpu(), dev(b))
    with pytest.raises(RuntimeError, match="part .* holds fewer"):
        K.swd_sorted_l1(dev(a), dev(b), part=buf[:3 * parts - 1])


# ---- statistics and projection
@pytest.mark.parametrize("i", range(len(R.PROJ)))
def test_patch_stats_and_projection(K, S, i):
    case = R.proj_case(i)
    level, nhood, per = dev(case["level"]), case["nhood"], R.PROJ_PER_IMAGE
    m, c = len(case["cx"]), case["level"].shape[3]
    n_el = m * nhood * nhood
    u = 2.0 ** -53
    sums = K.swd_patch_stats(level, case["cx"], case["cy"], nhood, per)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (c, 2)
    # a float64 sum of n_el terms in any order, twice (the product and the restatement); the squares carry one rounding more
    p = R.patches(case["level"], case["cx"], case["cy"], nhood, per)
    tol = 2 * (n_el + 2) * u * np.stack([np.abs(p).sum(axis=(0, 2, 3)), np.square(p).sum(axis=(0, 2, 3))], axis=1)
    assert np.all(np.abs(sums.cpu().numpy() - case["sums"]) <= tol)
    mean, std = S.patch_mean_std(level, case["cx"], case["cy"], nhood, per)
    em = 2 * (n_el + 1) * u * np.abs(p).mean(axis=(0, 2, 3))
    rs = 2 * ((n_el + 8) * u + np.square(em + n_el * u * case["std"] * 1.01) / np.square(case["std"]))
    print(f"case {i}: mean error / bound {np.max(np.abs(mean - case['mean']) / em):.3f}, std error / bound "
          f"{np.max(np.abs(std - case['std']) / (rs * case['std'])):.3f}")
    assert np.all(np.abs(mean - case["mean"]) <= em) and np.all(np.abs(std - case["std"]) <= rs * case["std"])
    ndirs = case["dirs"].shape[1]
    buf = torch.full((ndirs * m + 64,), SENTINEL, dtype=torch.float64, device="cuda")
    keys = K.swd_project(level, case["cx"], case["cy"], nhood, per, mean, std, dev(case["dirs"]), out=buf)
    assert keys.data_ptr() == buf.data_ptr() and tuple(keys.shape) == (ndirs, m) and bool((buf[ndirs * m:] == SENTINEL).all())
    err = np.abs(keys.cpu().numpy() - case["keys"]).max()
    print(f"case {i}: worst key error {err:.3e}, bound {case['key_bound']:.3e}")
    assert err <= case["key_bound"]
    assert torch.equal(keys.clone(), K.swd_project(level, case["cx"], case["cy"], nhood, per, mean, std, dev(case["dirs"])))
    assert np.array_equal(keys.cpu().numpy()[:, 5], keys.cpu().numpy()[:, 6])          # the repeated centre


@pytest.mark.parametrize("i", range(len(R.PROJ)))
def test_four_bit_statistics_are_exact(K, i):
    case = R.proj_case(i, True)
    m, c = len(case["cx"]), case["level"].shape[3]
    part = torch.full((K.swd_patch_stats_parts(m) * c * 2 + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    out = torch.full((c * 2 + 8,), SENTINEL, dtype=torch.float64, device="cuda")
    sums = K.swd_patch_stats(dev(case["level"]), case["cx"], case["cy"], case["nhood"], R.PROJ_PER_IMAGE, part=part, out=out)
    assert bool((part[-8:] == SENTINEL).all()) and bool((out[c * 2:] == SENTINEL).all())
    assert np.array_equal(sums.cpu().numpy(), case["sums"])
    shifted = K.swd_patch_stats(dev(case["level"]), case["cx"], case["cy"], case["nhood"], R.PROJ_PER_IMAGE, shift=np.full(c, 3.0))
    p = R.patches(case["level"], case["cx"], case["cy"], case["nhood"], R.PROJ_PER_IMAGE) - 3.0
    assert np.array_equal(shifted.cpu().numpy(), np.stack([p.sum(axis=(0, 2, 3)), np.square(p).sum(axis=(0, 2, 3))], axis=1))


def test_stats_and_projection_refusals(K):
    case = R.proj_case(0)
    level, cx, cy, nhood, per = dev(case["level"]), case["cx"], case["cy"], case["nhood"], R.PROJ_PER_IMAGE
    dirs, mean, std = dev(case["dirs"]), case["mean"], case["std"]
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.swd_patch_stats(level.cpu(), cx, cy, nhood, per)
    with pytest.raises(RuntimeError, match="float64 images"):
        K.swd_patch_stats(level.float(), cx, cy, nhood, per)
    with pytest.raises(RuntimeError, match="int32 centre tables"):
        K.swd_patch_stats(level, cx.astype(np.int64), cy, nhood, per)
    for axis in (0, 1):
        for bad in (nhood // 2 - 1, 16 - nhood // 2):
            tables = [np.array(cx), np.array(cy)]
            tables[axis][9] = bad
            with pytest.raises(RuntimeError, match="is outside"):
                K.swd_patch_stats(level, tables[0], tables[1], nhood, per)
            with pytest.raises(RuntimeError, match="is outside"):
                K.swd_project(level, tables[0], tables[1], nhood, per, mean, std, dirs)
    with pytest.raises(RuntimeError, match="need more than the 3 images"):
        K.swd_patch_stats(level, cx, cy, nhood, per - 1)
    with pytest.raises(RuntimeError, match="nhood_size = 4"):
        K.swd_patch_stats(level, cx, cy, 4, per)
    with pytest.raises(RuntimeError, match="shift float64"):
        K.swd_patch_stats(level, cx, cy, nhood, per, shift=np.zeros(2))
    with pytest.raises(RuntimeError, match="out .* holds fewer"):
        K.swd_patch_stats(level, cx, cy, nhood, per, out=torch.empty(5, dtype=torch.float64, device="cuda"))
    with pytest.raises(RuntimeError, match="zero variance"):
        K.swd_project(level, cx, cy, nhood, per, mean, np.array([1.0, 0.0, 1.0]), dirs)
    with pytest.raises(RuntimeError, match="dirs float64"):
        K.swd_project(level, cx, cy, nhood, per, mean, std, dirs[:-1].contiguous())
    with pytest.raises(RuntimeError, match="out .* holds fewer"):
        K.swd_project(level, cx, cy, nhood, per, mean, std, dirs, out=torch.empty(3 * 15 - 1, dtype=torch.float64, device="cuda"))


# ---- end to end
@pytest.mark.parametrize("i", R.cases())
def test_calculate_swd_against_the_restatement(S, i):
    case = R.e2e_case(i)
    values, mean = S.calculate_swd(np.array(case["a"]), np.array(case["b"]), seed=0, **case["kw"])
    err = np.abs(values - case["values"])
    print(f"case {i}: product {values} restatement {case['values']} error {err} bound {case['bounds']}")
    assert values.dtype == np.float64 and values.shape == case["values"].shape and isinstance(mean, float)
    assert np.all(err <= case["bounds"])
    assert abs(mean - case["mean"]) <= case["bounds"].max()
    from_device = S.calculate_swd(torch.tensor(np.array(case["a"])).cuda(), torch.tensor(np.array(case["b"])).cuda(), seed=0, **case["kw"])
    assert np.array_equal(from_device[0], values) and from_device[1] == mean


def test_a_set_against_itself_is_exactly_zero(S):
    case = R.e2e_case(0)
    a, kw = np.array(case["a"]), case["kw"]
    dirs, centres, _ = S.draw_tables(*a.shape, kw["nhood_size"], kw["nhoods_per_image"], kw["dir_repeats"], kw["dirs_per_repeat"], seed=0)
    ref_dirs, ref_centres, _ = R.draw_tables(*a.shape, kw["nhood_size"], kw["nhoods_per_image"], kw["dir_repeats"], kw["dirs_per_repeat"], 0)
    assert np.array_equal(dirs, ref_dirs) and all(np.array_equal(x, y) for p, q in zip(centres, ref_centres) for x, y in zip(p, q))
    levels = S.laplacian_pyramid(a)
    assert len(levels) == 2
    for level, table in zip(levels, centres):
        assert S.sliced_wasserstein(level, level.clone(), table, table, dirs, kw["nhood_size"], kw["nhoods_per_image"]) == 0.0


def test_calculate_swd_refusals(S):
    a = np.array(R.e2e_case(0)["a"])
    kw = dict(nhoods_per_image=4, dir_repeats=1, dirs_per_repeat=4)
    with pytest.raises(ValueError, match="differ in shape"):
        S.calculate_swd(a, a[:8], **kw)
    with pytest.raises(RuntimeError, match="zero variance"):
        S.calculate_swd(a, np.full_like(a, 77), **kw)
    with pytest.raises(ValueError, match="does not fit"):
        S.calculate_swd(a[:, :4, :4], a[:, :4, :4], **kw)


# ---- trainers
def snapshot(tr):
    return {k: v['params'].clone() for k, v in tr.store.flat.items() if 'params' in v}


@pytest.mark.parametrize("which", ["sngan", "acgan", "pggan"])
def test_trainer_swd_is_an_evaluation_only(K, which):
    size = 32
    if which == "sngan":
        from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
        tr, step = SNGANTrainer(batch_size=8, seed=0, use_graphs=False), 'iteration'
    elif which == "acgan":
        from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
        tr, step = ACGANTrainer(batch_size=8, seed=0, use_graphs=False), 'global_step'
    else:
        from gan_lib_tensorflow_amd.PGGAN.train import PGGANTrainer, default_args
        size = 16
        tr, step = PGGANTrainer(default_args(batch_size=16, image_size=16, block_count=2, model='nvidia'), seed=0, use_graphs=False), 'step'
    real = np.random.RandomState(4).randint(0, 256, size=(64, size, size, 3)).astype(np.uint8)
    before, at = snapshot(tr), getattr(tr, step)
    assert before
    values, mean = tr.swd(real, n=64, nhoods_per_image=8, dir_repeats=1, dirs_per_repeat=8)
    assert values.shape == (len(R.level_sizes(size, size)),) and np.all(np.isfinite(values)) and isinstance(mean, float) and np.isfinite(mean)
    assert getattr(tr, step) == at
    after = snapshot(tr)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    with pytest.raises(ValueError, match="at least 65"):
        tr.swd(real, n=65)


def test_pggan_trainer_at_4x4_raises(K):
    from gan_lib_tensorflow_amd.PGGAN.train import PGGANTrainer, default_args
    tr = PGGANTrainer(default_args(batch_size=16), seed=0, use_graphs=False)
    with pytest.raises(ValueError, match="does not fit"):
        tr.swd(np.zeros((64, 4, 4, 3), dtype=np.uint8), n=64)


def test_pix2pix_swd_score(K):
    from gan_lib_tensorflow_amd.Pix2Pix.train import swd_score
    rng = np.random.RandomState(6)
    outputs = torch.tensor(rng.uniform(-1, 1, size=(2, 64, 64, 3)).astype(np.float32)).cuda()
    targets = torch.tensor(rng.uniform(-1, 1, size=(2, 64, 64, 3)).astype(np.float32)).cuda()
    values, mean = swd_score(outputs, targets, nhoods_per_image=16, dir_repeats=1, dirs_per_repeat=8)
    assert values.shape == (3,) and values.dtype == np.float64 and np.all(np.isfinite(values)) and mean == float(values.mean())
    half = swd_score(outputs.to(K.BF16), targets.to(K.BF16), nhoods_per_image=16, dir_repeats=1, dirs_per_repeat=8)
    assert half[0].shape == (3,) and np.all(np.isfinite(half[0]))
