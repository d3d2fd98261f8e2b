"""GPU: the k-means kernels of NDB / JSD (csrc/ndb.hip) against the NumPy float64 restatement tests/ndb_ref.py, an exact integer
case, the whole fit iteration by iteration, and the metric end to end (gan_lib_tensorflow_amd/common/ndb.py, the trainers' `ndb`).

The bound on a squared distance is prd_ref's (|d2 - d2_ref| <= 2 (D + 4) 2^-53 sum_k (|a_ik| + |b_jk|)^2).  Labels are compared
with ==: a label can differ from the reference's only on a row that the reference leaves undecided (ndb_ref's docstring), and
every test that compares labels asserts, on the reference alone, that its case has no such row (so does tests/test_ndb_cpu.py).
With equal labels the grouping is an integer computation and the centroids are one fixed order of float64 additions: those are
compared for equal bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ndb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from gan_lib_tensorflow_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def N(K):
    from gan_lib_tensorflow_amd.common import ndb
    return ndb


def dev(a, dtype=np.float32):
    return torch.tensor(np.asarray(a, dtype=dtype)).cuda()      # a copy: the reference's arrays are read-only


def host(t):
    return t.cpu().numpy()


# ---- 1. pixel features
@pytest.mark.parametrize("shape,ndims", [((5, 4, 4, 3), None), ((67, 8, 8, 3), 40), ((3, 40, 40, 3), 4096)])
def test_pixel_features(K, N, shape, ndims):
    images = np.random.RandomState(shape[0]).randint(0, 256, size=shape).astype(np.uint8)
    p = int(np.prod(shape[1:]))
    if ndims is None:
        dims = None
    elif ndims == 4096:
        dims = N.draw_dims(p, 4096, seed=2)
    else:
        dims = np.sort(np.random.RandomState(1).choice(p, ndims, replace=False)).astype(np.int32)
    want = R.pixel_features(images, dims)
    dsel = p if dims is None else len(dims)
    got = K.ndb_pixel_features(torch.from_numpy(images).cuda(), dims)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (shape[0], (dsel + 15) // 16 * 16)
    assert np.array_equal(host(got), want)
    assert not host(got)[:, dsel:].any()                           # the padding columns are exactly 0
    if dims is not None and ndims == 40:
        assert got.shape[1] == 48
        unsorted = dims[::-1].copy()                               # any order of positions is a gather
        assert np.array_equal(host(K.ndb_pixel_features(torch.from_numpy(images).cuda(), unsorted)), R.pixel_features(images, unsorted))


# ---- 2. assign, exact
def test_assign_exact_integers(K):
    """Integer features: every d2 is an integer of at most 16 * 36, exact in float64 in any order, so labels, d2 and the strip
    sums must equal the int64 computation bit for bit, with every tie (two duplicated centroids, and the ties integers bring) to
    the lowest index: a merge that prefers a later column class or a later tile cannot hide."""
    xi, ci, d, prev = R.integer_case()
    want = np.argmin(d, axis=1)
    label, d2, part_inertia, part_changed = K.ndb_assign(dev(xi), dev(ci), prev=dev(prev, np.int32))
    assert label.dtype == torch.int32 and d2.dtype == torch.float64 and part_inertia.dtype == torch.float64 and part_changed.dtype == torch.int32
    assert tuple(label.shape) == tuple(d2.shape) == (150,) and tuple(part_inertia.shape) == tuple(part_changed.shape) == (3,)
    print("exact case, rows whose label differs:", np.flatnonzero(host(label) != want).tolist())
    assert np.array_equal(host(label), want)
    assert np.array_equal(host(d2), d.min(axis=1).astype(np.float64))
    assert np.array_equal(host(part_inertia), [d.min(axis=1)[i:i + 64].sum() for i in (0, 64, 128)])
    assert np.array_equal(host(part_changed), [(want != prev)[i:i + 64].sum() for i in (0, 64, 128)])
    assert not host(K.ndb_assign(dev(xi), dev(ci))[3]).any()        # no prev: nothing changed


# ---- 3. assign, general shapes
@pytest.mark.parametrize("n,k,d", R.ASSIGN_SHAPES)
def test_assign(K, n, k, d):
    case = R.assign_case(n, k, d)
    assert int(case["undecided"].sum()) == 0                       # a condition on the inputs, not a tolerance on the kernel
    label, d2, part_inertia, part_changed = K.ndb_assign(dev(case["x"]), dev(case["c"]), prev=dev(case["prev"], np.int32))
    err = np.abs(host(d2) - case["d2"])
    print(f"({n},{k},{d}): labels differ in {int((host(label) != case['label']).sum())} rows, worst d2 error / bound "
          f"{np.max(err / case['bound']):.4f}")
    assert np.array_equal(host(label), case["label"])
    assert np.all(err <= case["bound"])
    strips = (n + 63) // 64
    assert tuple(part_inertia.shape) == tuple(part_changed.shape) == (strips,)
    want = R.strip_sums(case["d2"])
    bound = R.strip_sums(case["bound"]) + 2 * 64 * 2.0 ** -53 * want          # the elements' bounds and the strip's 64 additions
    assert np.all(np.abs(host(part_inertia) - want) <= bound)
    moved = case["label"] != case["prev"]
    assert np.array_equal(host(part_changed), [moved[i:i + 64].sum() for i in range(0, n, 64)])


# ---- 4. group_rows
def check_grouping(K, label, k):
    count, offset, perm = K.ndb_group_rows(dev(label, np.int32), k)
    assert count.dtype == offset.dtype == perm.dtype == torch.int32
    want_count, want_offset, want_perm = R.group_rows(np.asarray(label), k)
    assert np.array_equal(host(count), want_count) and np.array_equal(host(offset), want_offset)
    assert np.array_equal(host(perm), want_perm)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("k", [1, 7, 1024])
def test_group_rows(K, n, k):
    check_grouping(K, np.random.RandomState(n + k).randint(0, k, n), k)


def test_group_rows_special_labels(K):
    rng = np.random.RandomState(0)
    check_grouping(K, rng.choice([3, 40, 99], 1000), 100)          # clusters without rows
    check_grouping(K, np.full(1000, 5), 7)                         # all rows in one cluster
    check_grouping(K, np.full(65, 1023), 1024)
    check_grouping(K, rng.randint(0, 100, 5000), 100)              # three units of 2048 rows
    check_grouping(K, np.repeat(np.arange(10), 410)[::-1].copy(), 10)        # 4100 rows, descending labels, runs across the units


# ---- 5. centroids
@pytest.mark.parametrize("n,k,d", R.ASSIGN_SHAPES)
def test_centroids(K, n, k, d):
    case = R.assign_case(n, k, d)
    c = dev(case["c"])
    before = c.clone()
    got = K.ndb_centroids(dev(case["x"]), dev(case["perm"], np.int32), dev(case["count"], np.int32), dev(case["offset"], np.int32), c)
    assert got.data_ptr() == c.data_ptr()
    assert np.array_equal(host(c).view(np.uint32), case["new_c"].view(np.uint32))          # equal bits
    empty = np.flatnonzero(case["count"] == 0)
    assert torch.equal(c[empty], before[empty])                    # clusters without rows keep the bytes they came in with
    if k > n:
        assert len(empty) > 0


def test_centroids_keep_any_bytes_of_an_empty_cluster(K):
    x = dev(np.arange(32, dtype=np.float32).reshape(2, 16))
    c = torch.full((3, 16), float("nan"), device="cuda")
    K.ndb_centroids(x, dev([1, 0], np.int32), dev([0, 2, 0], np.int32), dev([0, 0, 2], np.int32), c)
    assert bool(torch.isnan(c[0]).all()) and bool(torch.isnan(c[2]).all())
    assert np.array_equal(host(c[1]), np.arange(8, 24, dtype=np.float32))       # (16 + j + j) / 2, the rows in the order 1, 0


# ---- 6. the whole fit
@pytest.mark.parametrize("k", [8, 12])
def test_fit_follows_the_restatement_iteration_by_iteration(K, N, k):
    case = R.mixture_case(k)
    fit = case["fit"]
    assert fit["undecided"] == 0                                   # in no iteration: a condition on the inputs
    x = dev(case["x"])
    c = x[torch.from_numpy(R.draw_init(600, k, seed=k)).cuda()].contiguous()
    prev = None
    for it, (want_label, want_c) in enumerate(zip(fit["labels"], fit["centroid_steps"])):
        assert np.array_equal(host(c).view(np.uint32), want_c.view(np.uint32)), it
        label, _, _, part_changed = K.ndb_assign(x, c, prev=prev)
        assert np.array_equal(host(label), want_label), it
        if prev is not None:
            assert int(host(part_changed).sum()) == int((want_label != fit["labels"][it - 1]).sum())
        count, offset, perm = K.ndb_group_rows(label, k)
        K.ndb_centroids(x, perm, count, offset, c)
        prev = label
    centroids, labels, inertia, iterations = N.kmeans(x, k, seed=k)
    print(f"K = {k}: {iterations} iterations, inertia {inertia!r}, restatement {fit['inertia']!r} +- {fit['inertia_bound']:.3g}")
    assert iterations == fit["iterations"]
    assert np.array_equal(host(labels), fit["labels"][-1])
    assert centroids.dtype == torch.float32 and np.array_equal(host(centroids).view(np.uint32), fit["centroids"].view(np.uint32))
    assert isinstance(inertia, float) and abs(inertia - fit["inertia"]) <= fit["inertia_bound"]
    again = N.kmeans(x, k, seed=k)
    assert torch.equal(again[0], centroids) and torch.equal(again[1], labels) and again[2:] == (inertia, iterations)
    capped = N.kmeans(x, k, seed=k, max_iter=2)
    assert capped[3] == 2 and np.array_equal(host(capped[1]), fit["labels"][1])
    assert np.array_equal(host(capped[0]).view(np.uint32), fit["centroid_steps"][1].view(np.uint32))


# ---- 7. the house checks
def test_buffers_are_written_inside_their_bounds(K):
    n, k, d = 65, 3, 48
    case = R.assign_case(n, k, d)
    x, c = dev(case["x"]), dev(case["c"])
    strips = 2
    label = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    d2 = torch.full((n + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    part_inertia = torch.full((strips + 1,), SENTINEL, dtype=torch.float64, device="cuda")
    part_changed = torch.full((strips + 1,), -7, dtype=torch.int32, device="cuda")
    got = K.ndb_assign(x, c, label=label, d2=d2, part_inertia=part_inertia, part_changed=part_changed)
    assert [g.data_ptr() for g in got] == [label.data_ptr(), d2.data_ptr(), part_inertia.data_ptr(), part_changed.data_ptr()]
    assert int(label[n]) == -7 and float(d2[n]) == SENTINEL and float(part_inertia[strips]) == SENTINEL and int(part_changed[strips]) == -7
    assert np.array_equal(host(got[0]), case["label"]) and bool((d2[:n] != SENTINEL).all()) and bool((part_inertia[:strips] != SENTINEL).all())
    assert not host(got[3]).any()
    count = torch.full((k + 1,), -7, dtype=torch.int32, device="cuda")
    offset = torch.full((k + 1,), -7, dtype=torch.int32, device="cuda")
    perm = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
    need = K.ndb_group_ws_elems(n, k)
    assert need == k
    ws = torch.full((need + 1,), -7, dtype=torch.int32, device="cuda")
    grouped = K.ndb_group_rows(got[0], k, count=count, offset=offset, perm=perm, ws=ws)
    assert int(count[k]) == -7 and int(offset[k]) == -7 and int(perm[n]) == -7 and int(ws[need]) == -7
    assert np.array_equal(host(grouped[2]), case["perm"]) and np.array_equal(host(grouped[0]), case["count"])
    cbuf = torch.full((k + 1, d), SENTINEL, dtype=torch.float32, device="cuda")
    cbuf[:k] = c
    K.ndb_centroids(x, grouped[2], grouped[0], grouped[1], cbuf[:k])
    assert bool((cbuf[k] == SENTINEL).all()) and np.array_equal(host(cbuf[:k]).view(np.uint32), case["new_c"].view(np.uint32))
    images = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(5, 40)).astype(np.uint8)).cuda()
    out = torch.full((5 * 48 + 16,), SENTINEL, dtype=torch.float32, device="cuda")
    feats = K.ndb_pixel_features(images, out=out)
    assert feats.data_ptr() == out.data_ptr() and bool((out[5 * 48:] == SENTINEL).all()) and bool((out[:5 * 48] != SENTINEL).all())
    for name, kw in (("label", dict(label=label[:n - 1])), ("d2", dict(d2=d2[:n - 1])), ("part_inertia", dict(part_inertia=part_inertia[:1])),
                     ("part_changed", dict(part_changed=part_changed[:1]))):
        with pytest.raises(RuntimeError, match=f"{name} .* holds fewer"):
            K.ndb_assign(x, c, **kw)
    with pytest.raises(RuntimeError, match="ws .* holds fewer"):
        K.ndb_group_rows(got[0], k, ws=ws[:need - 1])
    with pytest.raises(RuntimeError, match="perm .* holds fewer"):
        K.ndb_group_rows(got[0], k, perm=perm[:n - 1])
    with pytest.raises(RuntimeError, match="out .* holds fewer"):
        K.ndb_pixel_features(images, out=out[:5 * 48 - 1])


def test_two_calls_return_the_same_bits(K):
    case = R.assign_case(257, 100, 3072)
    x, c, prev = dev(case["x"]), dev(case["c"]), dev(case["prev"], np.int32)
    first, second = K.ndb_assign(x, c, prev=prev), K.ndb_assign(x, c, prev=prev)
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    g1, g2 = K.ndb_group_rows(first[0], 100), K.ndb_group_rows(first[0], 100)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    c1, c2 = c.clone(), c.clone()
    K.ndb_centroids(x, g1[2], g1[0], g1[1], c1)
    K.ndb_centroids(x, g1[2], g1[0], g1[1], c2)
    assert torch.equal(c1, c2)


def test_refusals_of_the_c_abi(K):
    """every refusal gank.h lists, through the library itself, with its error text: decided on the host before any launch"""
    from gan_lib_tensorflow_amd import _lib
    lib = _lib.load()
    P = C.c_void_p
    a, odd = P(0x1000), P(0x1004)          # never dereferenced: every call below is refused by the argument checks

    def refused(rc, text):
        assert rc != 0
        assert text in lib.gank_last_error().decode(), lib.gank_last_error().decode()

    def assign(x=a, n=64, c=a, k=4, d=32, label=a, d2=a, pi=a, pc=a):
        return lib.gank_ndb_assign(x, n, c, k, d, None, label, d2, pi, pc, None)

    for kw in (dict(x=None), dict(c=None), dict(label=None), dict(d2=None), dict(pi=None), dict(pc=None)):
        refused(assign(**kw), "ndb_assign: null pointer")
    for d in (0, 8, 24, 4112):
        refused(assign(d=d), f"ndb_assign: D = {d} unsupported")
    for k in (0, 1025):
        refused(assign(k=k), f"ndb_assign: K = {k} unsupported")
    for n in (0, (1 << 24) + 1):
        refused(assign(n=n), f"ndb_assign: n = {n} ")
    refused(assign(x=odd), "ndb_assign: misaligned pointer")
    refused(assign(c=odd), "ndb_assign: misaligned pointer")

    def group(label=a, n=64, k=4, count=a, offset=a, perm=a, ws=a):
        return lib.gank_ndb_group_rows(label, n, k, count, offset, perm, ws, None)

    for kw in (dict(label=None), dict(count=None), dict(offset=None), dict(perm=None), dict(ws=None)):
        refused(group(**kw), "ndb_group_rows: null pointer")
    refused(group(k=0), "ndb_group_rows: K = 0 unsupported")
    refused(group(k=1025), "ndb_group_rows: K = 1025 unsupported")
    refused(group(n=0), "ndb_group_rows: n = 0 ")
    refused(group(n=(1 << 24) + 1), "ndb_group_rows: n = 16777217 ")
    assert lib.gank_ndb_group_ws_elems(5000, 100) == 300 and lib.gank_ndb_group_ws_elems(0, 100) == 0 and lib.gank_ndb_group_ws_elems(10, 1025) == 0

    def cent(x=a, n=64, d=32, perm=a, count=a, offset=a, k=4, c=a):
        return lib.gank_ndb_centroids(x, n, d, perm, count, offset, k, c, None)

    for kw in (dict(x=None), dict(perm=None), dict(count=None), dict(offset=None), dict(c=None)):
        refused(cent(**kw), "ndb_centroids: null pointer")
    refused(cent(d=40), "ndb_centroids: D = 40 unsupported")
    refused(cent(d=8192), "ndb_centroids: D = 8192 unsupported")
    refused(cent(k=0), "ndb_centroids: K = 0 unsupported")
    refused(cent(k=1025), "ndb_centroids: K = 1025 unsupported")
    refused(cent(n=0), "ndb_centroids: n = 0 ")
    refused(cent(n=(1 << 24) + 1), "ndb_centroids: n = 16777217 ")
    refused(cent(x=odd), "ndb_centroids: misaligned pointer")
    refused(cent(c=odd), "ndb_centroids: misaligned pointer")

    def pix(img=a, n=4, p=48, dims=None, dsel=48, out=a):
        return lib.gank_ndb_pixel_features(img, n, p, dims, dsel, out, None)

    refused(pix(img=None), "ndb_pixel_features: null pointer")
    refused(pix(out=None), "ndb_pixel_features: null pointer")
    refused(pix(n=0), "ndb_pixel_features: n = 0 ")
    refused(pix(n=(1 << 24) + 1), "ndb_pixel_features: n = 16777217 ")
    refused(pix(p=0, dsel=1), "ndb_pixel_features: P = 0 ")
    refused(pix(dsel=0), "ndb_pixel_features: Dsel = 0 ")
    refused(pix(dsel=49), "ndb_pixel_features: Dsel = 49 ")
    refused(pix(p=5000, dsel=4097), "ndb_pixel_features: Dsel = 4097 ")
    refused(pix(out=odd), "ndb_pixel_features: misaligned pointer")


def test_wrapper_refusals(K, N):
    case = R.assign_case(65, 3, 48)
    x, c = dev(case["x"]), dev(case["c"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.ndb_assign(x.cpu(), c)
    with pytest.raises(RuntimeError, match="float32 features"):
        K.ndb_assign(x.double(), c)
    with pytest.raises(RuntimeError, match="differ in the feature width"):
        K.ndb_assign(x, c[:, :32].contiguous())
    with pytest.raises(RuntimeError, match=r"prev int32 \[65\]"):
        K.ndb_assign(x, c, prev=torch.zeros(64, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="D = 40 unsupported"):
        K.ndb_assign(x[:, :40].contiguous(), c[:, :40].contiguous())
    with pytest.raises(RuntimeError, match="K = 1025 unsupported"):
        K.ndb_group_rows(torch.zeros(8, dtype=torch.int32, device="cuda"), 1025)
    with pytest.raises(RuntimeError, match=r"label int32 \[n\]"):
        K.ndb_group_rows(torch.zeros(8, dtype=torch.int64, device="cuda"), 4)
    with pytest.raises(RuntimeError, match=r"count int32 \[3\]"):
        K.ndb_centroids(x, torch.zeros(65, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"),
                        torch.zeros(3, dtype=torch.int32, device="cuda"), c)
    images = torch.zeros((4, 4, 4, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match=r"outside \[0, 48\)"):
        K.ndb_pixel_features(images, np.array([0, 48], dtype=np.int32))
    with pytest.raises(RuntimeError, match=r"outside \[0, 48\)"):
        K.ndb_pixel_features(images, np.array([-1, 4], dtype=np.int32))
    with pytest.raises(RuntimeError, match="uint8 images"):
        K.ndb_pixel_features(images.float())
    with pytest.raises(RuntimeError, match=r"dims int32 \[Dsel\]"):
        K.ndb_pixel_features(images, np.array([0, 1], dtype=np.int64))
    with pytest.raises(ValueError, match="at least 66"):
        N.kmeans(x, 66)
    with pytest.raises(ValueError, match="not rows"):
        N.NDB(np.zeros((8, 4, 4, 3), dtype=np.uint8), number_of_bins=2).evaluate(np.zeros((8, 4, 4, 1), dtype=np.uint8))
    with pytest.raises(TypeError, match="multiple of 16"):
        N.NDB(np.zeros((8, 40), dtype=np.float32), number_of_bins=2)


# ---- 8. end to end on uint8 images
def test_calculate_ndb_on_images(N):
    case = R.image_case()
    bins = N.NDB(case["train"], number_of_bins=case["bins"])
    assert bins.dims is None and tuple(bins.centroids.shape) == (10, 3072) and bins.iterations == case["ref_held_out"]["iterations"]
    results = {}
    for name in ("held_out", "missing"):
        ref = case["ref_" + name]
        assert ref["undecided"] == 0
        got = N.calculate_ndb(case["train"], case[name], number_of_bins=case["bins"])
        print(f"{name}: product ndb {got['ndb']} js {got['js']!r}, restatement ndb {ref['ndb']} js {ref['js']!r}")
        assert sorted(got) == ["bin_proportions_samples", "bin_proportions_train", "different_bins", "js", "ndb", "ndb_over_k"]
        assert got["ndb"] == ref["ndb"] and got["different_bins"].tolist() == ref["different"] and got["ndb_over_k"] == ref["ndb"] / 10.0
        assert np.array_equal(got["bin_proportions_train"], ref["train_counts"] / 600.0)          # the bin counts, exactly
        assert np.array_equal(got["bin_proportions_samples"], ref["sample_counts"] / 600.0)
        assert abs(got["js"] - ref["js"]) <= 1e-12
        again = bins.evaluate(torch.from_numpy(np.array(case[name])).cuda())          # fitted once, a device tensor
        assert again["ndb"] == got["ndb"] and again["js"] == got["js"]
        results[name] = got
    assert np.array_equal(bins.train_counts, case["ref_held_out"]["train_counts"])
    assert results["missing"]["ndb"] > results["held_out"]["ndb"]


def test_ndb_on_features_and_chosen_dims(N):
    """float32 features go in as they are; images of more than max_dims values are read at the drawn positions"""
    case = R.mixture_case(8)
    x = np.array(case["x"])
    got = N.NDB(x, number_of_bins=8, seed=8)
    assert np.array_equal(got.train_counts, np.bincount(case["fit"]["labels"][-1], minlength=8))
    same = got.evaluate(x)
    assert same["ndb"] == 0 and same["js"] == 0.0
    rng = np.random.RandomState(9)
    images = rng.randint(0, 256, size=(40, 8, 8, 3)).astype(np.uint8)
    samples = rng.randint(0, 256, size=(30, 8, 8, 3)).astype(np.uint8)
    ref = R.calculate_ndb(images, samples, 4, max_dims=48, seed=1)
    assert ref["undecided"] == 0
    bins = N.NDB(images, number_of_bins=4, max_dims=48, seed=1)
    assert np.array_equal(bins.dims, R.draw_dims(192, 48, 1)) and tuple(bins.centroids.shape) == (4, 48)
    res = bins.evaluate(samples)
    assert np.array_equal(bins.train_counts, ref["train_counts"]) and np.array_equal(res["bin_proportions_samples"], ref["sample_counts"] / 30.0)
    assert res["ndb"] == ref["ndb"] and abs(res["js"] - ref["js"]) <= 1e-12


# ---- 9. the trainers
NDB_KW = dict(number_of_bins=8)


def make(which):
    torch.cuda.set_device(0)
    if which == "sngan":
        from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
        return SNGANTrainer(batch_size=8, seed=0, use_graphs=False), 'iteration', 32
    if which == "acgan":
        from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
        return ACGANTrainer(batch_size=8, seed=0, use_graphs=False), 'global_step', 32
    from gan_lib_tensorflow_amd.PGGAN.train import PGGANTrainer, default_args
    return PGGANTrainer(default_args(batch_size=16, image_size=64, block_count=4, model='nvidia'), seed=0, use_graphs=False), 'step', 64


def snapshot(tr):
    """every tensor of the flat buffers: parameters and, where the trainer keeps them there, the optimiser's moments"""
    return {(k, name): t.clone() for k, v in tr.store.flat.items() for name, t in v.items() if isinstance(t, torch.Tensor)}


@pytest.mark.parametrize("which", ["sngan", "acgan", "pggan"])
def test_trainer_ndb_is_the_hook_plus_calculate_ndb(N, which, deterministic_stats):
    n = 400
    a, step, size = make(which)
    b = make(which)[0]
    real = np.random.RandomState(4).randint(0, 256, size=(n, size, size, 3)).astype(np.uint8)
    assert torch.equal(a.rng_state, b.rng_state)
    before, at = snapshot(a), getattr(a, step)
    assert before and any(name == 'params' for _, name in before)
    got = a.ndb(real, n=n, **NDB_KW)
    assert getattr(a, step) == at
    after = snapshot(a)
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)
    batches, have = [], 0
    with torch.no_grad():
        while have < n:
            images, _ = b._metric_batch(b._metric_rows())
            batches.append(images)
            have += len(images)
    fake = torch.cat(batches)[:n]
    assert fake.dtype == torch.uint8 and tuple(fake.shape) == (n, size, size, 3) and fake.is_cuda
    bins = N.NDB(real, **NDB_KW)
    assert (bins.dims is not None) == (which == "pggan")          # 64 x 64 x 3 = 12 288 values: 4096 of them are drawn
    want = bins.evaluate(fake)
    assert got["ndb"] == want["ndb"] and got["js"] == want["js"] and got["different_bins"].tolist() == want["different_bins"].tolist()
    assert np.array_equal(got["bin_proportions_train"], want["bin_proportions_train"])
    assert np.array_equal(got["bin_proportions_samples"], want["bin_proportions_samples"])
    assert abs(got["bin_proportions_samples"].sum() - 1.0) < 1e-12 and 0 <= got["ndb"] <= 8
    assert torch.equal(a.rng_state, b.rng_state)                   # the RNG advanced exactly as the hook calls do
    fitted = a.ndb(bins, n=16)                                     # an NDB fitted before is taken as it is
    assert sorted(fitted) == sorted(got)
    with pytest.raises(TypeError, match="fitted already"):
        a.ndb(bins, n=16, number_of_bins=4)


def test_pix2pix_ndb_score(K):
    from gan_lib_tensorflow_amd.Pix2Pix.train import ndb_score
    rng = np.random.RandomState(6)
    outputs = torch.tensor(rng.uniform(-1, 1, size=(24, 16, 16, 3)).astype(np.float32)).cuda()
    targets = torch.tensor(rng.uniform(-1, 1, size=(24, 16, 16, 3)).astype(np.float32)).cuda()
    got = ndb_score(outputs, targets, number_of_bins=3)
    assert 0 <= got["ndb"] <= 3 and np.isfinite(got["js"]) and got["bin_proportions_train"].shape == (3,)
    same = ndb_score(targets, targets, number_of_bins=3)
    assert same["ndb"] == 0 and same["js"] == 0.0
    half = ndb_score(outputs.to(K.BF16), targets.to(K.BF16), number_of_bins=3)
    assert 0 <= half["ndb"] <= 3 and np.isfinite(half["js"])
