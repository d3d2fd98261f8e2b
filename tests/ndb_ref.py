"""NumPy float64 restatement of NDB / JSD for the tests (imports nothing from the product, no torch): the draws, the pixel
features, the nearest-centroid assignment with numpy.argmin's tie rule, the stable grouping, the ordered float64 centroid sums,
Lloyd's iteration with its whole trajectory, the bin statistics, and the "undecided" test that the exact-equality claims of the
GPU tests rest on.  Squared distances and their derived bound are prd_ref's (d2 by differences; |d2 - d2_ref| <= 2 (D + 4) 2^-53
sum_k (|a_ik| + |b_jk|)^2).

Undecided.  A row's label is an argmin over perturbed values; it can differ from the reference's only if the reference's gap
between its smallest and its second-smallest d2 is at most the sum of those two elements' bounds (any other centroid is further
still and its bound is of the same size: the test uses the row's LARGEST bound for the second term, which is no weaker).  The
rule is a condition on the inputs, not a tolerance on the kernel: the tests assert that it leaves no row undecided."""
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prd_ref  # noqa: E402

ASSIGN_SHAPES = [(4, 1, 16), (65, 3, 48), (130, 64, 272), (300, 65, 64), (100, 130, 2048), (257, 100, 3072)]     # (n, K, D)


# ---- the draws
def draw_dims(P, max_dims=4096, seed=0):
    if P <= max_dims:
        return None
    return np.sort(np.random.RandomState(seed).choice(P, max_dims, replace=False)).astype(np.int32)


def draw_init(n, K, seed=0):
    return np.random.RandomState(seed).choice(n, K, replace=False)


# ---- the stages
def pixel_features(images, dims=None):
    """uint8 [n, ...] -> float32 [n, Dp]: the flat image at dims (all positions when None), zero columns up to a multiple of 16"""
    flat = np.asarray(images).reshape(len(images), -1)
    if dims is not None:
        flat = flat[:, np.asarray(dims)]
    out = np.zeros((len(flat), (flat.shape[1] + 15) // 16 * 16), dtype=np.float32)
    out[:, :flat.shape[1]] = flat
    return out


def assign(x, c):
    """-> (label int64 [n], d2 float64 [n], undecided bool [n], bound float64 [n]): argmin over the centroids (numpy.argmin: the
    lowest index of a tie), its d2, whether a permitted error could move the label (module docstring), the bound on d2"""
    d, b = prd_ref.d2(x, c), prd_ref.d2_bound(x, c)
    label = np.argmin(d, axis=1)
    rows = np.arange(len(d))
    best = d[rows, label]
    if d.shape[1] == 1:
        undecided = np.zeros(len(d), dtype=bool)
    else:
        second = np.partition(d, 1, axis=1)[:, 1]
        undecided = second - best <= b[rows, label] + b.max(axis=1)
    return label, best, undecided, b[rows, label]


def group_rows(label, K):
    """-> (count [K], offset [K], perm [n]): bincount, its exclusive prefix sum, the stable argsort"""
    count = np.bincount(label, minlength=K)
    return count, np.cumsum(count) - count, np.argsort(label, kind='stable')


def centroids(x, perm, count, offset, c):
    """float32 [K, D]: per cluster with rows the float64 sum of its rows in perm order, one accumulator per feature, / count,
    rounded to float32; a cluster without rows keeps its centroid.  The explicit ordered loop."""
    out = np.array(c, dtype=np.float32)
    for k in range(len(count)):
        if count[k] > 0:
            s = np.zeros(x.shape[1], dtype=np.float64)
            for r in perm[offset[k]:offset[k] + count[k]]:
                s += x[r].astype(np.float64)
            out[k] = (s / float(count[k])).astype(np.float32)
    return out


def strip_sums(d2):
    """[ceil(n / 64)]: the sum of every strip of 64 rows (the order of the device's sum is its own: compare within `inertia_bound`)"""
    return np.array([d2[i:i + 64].sum() for i in range(0, len(d2), 64)])


def kmeans(x, K, seed=0, max_iter=100):
    """Lloyd's iteration as the product documents it -> dict(centroids float32 [K, D] (final), labels: the list of every
    iteration's labels, centroid_steps: the centroids every assignment used, inertia, inertia_bound (the summed element bounds
    plus the n additions of the sum itself), iterations, undecided: rows undecided in ANY iteration)"""
    x = np.asarray(x, dtype=np.float32)
    c = x[draw_init(len(x), K, seed)].copy()
    labels, steps, undecided, prev = [], [], 0, None
    while True:
        label, d2, und, bound = assign(x, c)
        labels.append(label)
        steps.append(c.copy())
        undecided += int(und.sum())
        inertia = float(d2.sum())
        inertia_bound = float(bound.sum() + 2 * len(x) * 2.0 ** -53 * d2.sum())
        if (prev is not None and np.array_equal(label, prev)) or len(labels) >= max_iter:
            return dict(centroids=c, labels=labels, centroid_steps=steps, inertia=inertia, inertia_bound=inertia_bound,
                        iterations=len(labels), undecided=undecided)
        count, offset, perm = group_rows(label, K)
        c = centroids(x, perm, count, offset, c)
        prev = label


def bin_statistics(train_counts, sample_counts, significance_level=0.05):
    """scalar arithmetic, bin by bin -> dict(ndb, js, p, q, different)"""
    nk, mk = [int(v) for v in train_counts], [int(v) for v in sample_counts]
    nr, nf = sum(nk), sum(mk)
    different, js, ps, qs = [], 0.0, [], []
    for n, m in zip(nk, mk):
        p, q = n / nr, m / nf
        pooled = (n + m) / (nr + nf)
        se = math.sqrt(pooled * (1 - pooled) * (1 / nr + 1 / nf))
        if se > 0:
            z = (p - q) / se
            pvalue = math.erfc(abs(z) / math.sqrt(2))           # = 2 (1 - Phi(|z|))
            if pvalue < significance_level:
                different.append(len(ps))
        mid = (p + q) / 2
        if p > 0:
            js += 0.5 * p * math.log(p / mid)
        if q > 0:
            js += 0.5 * q * math.log(q / mid)
        ps.append(p)
        qs.append(q)
    return dict(ndb=len(different), js=js, p=np.array(ps), q=np.array(qs), different=different)


def calculate_ndb(train, samples, number_of_bins, significance_level=0.05, max_dims=4096, seed=0, max_iter=100):
    """uint8 images both -> dict(ndb, js, p, q, different, train_counts, sample_counts, undecided, iterations)"""
    dims = draw_dims(int(np.prod(train.shape[1:])), max_dims, seed)
    x, y = pixel_features(train, dims), pixel_features(samples, dims)
    fit = kmeans(x, number_of_bins, seed, max_iter)
    label, _, und, _ = assign(y, fit["centroids"])
    train_counts = np.bincount(fit["labels"][-1], minlength=number_of_bins)
    sample_counts = np.bincount(label, minlength=number_of_bins)
    out = bin_statistics(train_counts, sample_counts, significance_level)
    out.update(train_counts=train_counts, sample_counts=sample_counts, undecided=fit["undecided"] + int(und.sum()),
               iterations=fit["iterations"])
    return out


# ---- the cases (computed once, read-only)
def _freeze(out):
    for v in out.values():
        for a in (v if isinstance(v, (tuple, list)) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def assign_case(n, K, D):
    """Rows around K centres, float32, the centroids K perturbed centres (no two equal), a `prev` that differs from the labels in
    every third row -> dict(x, c, prev, label, d2, undecided, bound, count, offset, perm, new_c); new_c from `centroids` on a c
    whose clusters without rows must keep their bytes"""
    rng = np.random.RandomState(n * 10000 + K * 10 + D)
    centres = rng.normal(size=(K, D))
    x = (centres[rng.randint(0, K, n)] + 0.3 * rng.normal(size=(n, D))).astype(np.float32)
    c = (centres + 0.05 * rng.normal(size=(K, D))).astype(np.float32)
    label, d2, und, bound = assign(x, c)
    prev = label.copy()
    prev[::3] = (prev[::3] + 1) % max(K, 2)
    count, offset, perm = group_rows(label, K)
    return _freeze(dict(x=x, c=c, prev=prev.astype(np.int32), label=label, d2=d2, undecided=und, bound=bound, count=count, offset=offset,
                        perm=perm, new_c=centroids(x, perm, count, offset, c)))


def integer_case():
    """The exact case: integer features in -3..3, [150, 16]; the centroids are 70 of those rows, rows 5 and 41 of them copies of
    rows 2 and 17 (two duplicated pairs: a tie at distance 0 for the rows they came from, and a tie for every other row).  Every
    d2 is an integer of at most 16 * 36, exact in float64 in any order.  -> (x int64, c int64, integer d2 [150, 70], prev)"""
    rng = np.random.RandomState(11)
    x = rng.randint(-3, 4, (150, 16)).astype(np.int64)
    c = x[rng.choice(150, 70, replace=False)].copy()
    c[5], c[41] = c[2], c[17]
    d = ((x[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    prev = np.argmin(d, axis=1).astype(np.int32)
    prev[rng.choice(150, 40, replace=False)] = 69
    return x, c, d, prev


@functools.lru_cache(maxsize=None)
def mixture_case(K):
    """8 well-separated Gaussians in 48 dimensions, n = 600, float32, and the reference fit at K bins"""
    rng = np.random.RandomState(100 + K)
    means = 6.0 * rng.normal(size=(8, 48))
    x = (means[rng.randint(0, 8, 600)] + rng.normal(size=(600, 48))).astype(np.float32)
    return _freeze(dict(x=x, fit=kmeans(x, K, seed=K)))


@functools.lru_cache(maxsize=None)
def image_case():
    """The end-to-end case on tests/synthetic_classes.py images as [N,32,32,3]: 600 training images of 10 classes; samples (a) a
    held-out draw of the same classes, (b) a draw with the classes 7, 8, 9 missing, 600 each; 10 bins"""
    import synthetic_classes
    def nhwc(rows):
        return np.ascontiguousarray(rows.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1))
    train = nhwc(synthetic_classes.make_dataset(60, 1)[0])
    held_out = nhwc(synthetic_classes.make_dataset(60, 2)[0])
    rows, labels = synthetic_classes.make_dataset(90, 3)
    missing = nhwc(rows[labels < 7][:600])
    assert len(missing) == 600
    return _freeze(dict(train=train, held_out=held_out, missing=missing, bins=10,
                        ref_held_out=calculate_ndb(train, held_out, 10), ref_missing=calculate_ndb(train, missing, 10)))
