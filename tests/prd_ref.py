"""NumPy float64 restatement of precision / recall and density / coverage for the tests (imports nothing from the product, no
torch): squared distances, k-NN radii (self excluded by index, via a sort), manifold counts, the four values, the derived bound
on a squared distance and the "undecided" tests that the exact-equality claims of the GPU tests rest on.

Bound, derived and not measured.  The features are float32, so they and every product of two of them are exact in float64.
Each of the two norms and the dot product carries at most D roundings, the combination (|a|^2 + |b|^2) - 2 <a, b> a few more;
every partial sum is at most A_ij = sum_k (|a_ik| + |b_jk|)^2 in size.  So
    |d2 - d2_ref| <= 2 (D + 4) 2^-53 A_ij,
the factor 2 for the reference's own rounding."""
import functools

import numpy as np

SHAPES = [(4, 6, 16), (17, 23, 48), (64, 64, 64), (65, 77, 80), (130, 142, 272), (100, 112, 2048), (300, 257, 64)]
KS = (1, 3, 5)


def cases():
    """(nx, ny, d, k) over SHAPES and KS where k < min(nx, ny)"""
    return [(nx, ny, d, k) for nx, ny, d in SHAPES for k in KS if k < min(nx, ny)]


def manifold_banks(nx, ny, d, seed):
    """two shifted 4-dimensional manifolds in d dimensions, float32: the four values are non-trivial"""
    rng = np.random.RandomState(seed)
    A = rng.normal(size=(4, d))
    x = (rng.normal(size=(nx, 4)) @ A + 0.05 * rng.normal(size=(nx, d))).astype(np.float32)
    y = ((1.3 * rng.normal(size=(ny, 4)) + 0.5) @ A + 0.05 * rng.normal(size=(ny, d))).astype(np.float32)
    return x, y


def shape_banks(nx, ny, d):
    return manifold_banks(nx, ny, d, nx * 10000 + d)


def integer_banks():
    """The exact case: integer features, 72 x 16 in -3..3 (row 40 a copy of row 7) against 77 x 16 in -2..4.  Every d2 is an
    integer of at most 16 * 49, so float64 is exact in any order of summation.  -> (x, y) int64"""
    rng = np.random.RandomState(5)
    x, y = rng.randint(-3, 4, (72, 16)), rng.randint(-2, 5, (77, 16))
    x[40] = x[7]
    return x.astype(np.int64), y.astype(np.int64)


def integer_d2(a, b):
    """int64 [na, nb]"""
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)


def integer_radii(x, k):
    n = len(x)
    return np.sort(integer_d2(x, x)[~np.eye(n, dtype=bool)].reshape(n, n - 1), axis=1)[:, k - 1]


def d2(a, b):
    """[na, nb] squared distances, float64, by differences (no cancellation of norms)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((len(a), len(b)))
    for i in range(len(a)):
        diff = b - a[i]
        out[i] = np.einsum('jk,jk->j', diff, diff)
    return out


def d2_bound(a, b):
    """[na, nb]: the bound on |d2 - d2_ref| of the module docstring"""
    a, b = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
    out = np.empty((len(a), len(b)))
    for i in range(len(a)):
        s = b + a[i]
        out[i] = np.einsum('jk,jk->j', s, s)
    return 2 * (a.shape[1] + 4) * 2.0 ** -53 * out


def _others(x):
    """d2(x, x) with the diagonal removed by index: [n, n - 1], and the same of the bound"""
    n = len(x)
    off = ~np.eye(n, dtype=bool)
    return d2(x, x)[off].reshape(n, n - 1), d2_bound(x, x)[off].reshape(n, n - 1)


def radii(x, k):
    """float64 [n]: the k-th smallest squared distance of every row to the OTHER rows (self excluded by index, via a sort)"""
    return np.sort(_others(x)[0], axis=1)[:, k - 1]


def radii_bound(x, k):
    """float64 [n]: a bound on a radius's error -- the row's largest element bound (the k-th smallest of perturbed values moves
    by at most the largest perturbation)"""
    return _others(x)[1].max(axis=1)


def counts(q, r, radii2):
    """-> (count int64 [nq], nearest2 float64 [nq]): #{j: d2_ij <= radii2[j]} (inclusive) and min_j d2_ij"""
    d = d2(q, r)
    return (d <= np.asarray(radii2)[None, :]).sum(axis=1), d.min(axis=1)


def prdc(real, fake, k):
    """dict(precision, recall, density, coverage), the definitions of Kynkaanniemi et al. and Naeem et al."""
    radii_real, radii_fake = radii(real, k), radii(fake, k)
    count_fake, _ = counts(fake, real, radii_real)
    count_real, nearest_real = counts(real, fake, radii_fake)
    return dict(precision=float(np.mean(count_fake > 0)),
                recall=float(np.mean(count_real > 0)),
                density=float(count_fake.sum(dtype=np.int64) / (k * len(count_fake))),
                coverage=float(np.mean(nearest_real <= radii_real)))


def undecided_elements(q, r, radii2, radii2_bound):
    """the number of (i, j) whose comparison d2_ij <= radii2[j] a permitted error could turn: |d2_ij - radii2_j| at most the
    sum of the element's bound and the radius's"""
    gap = np.abs(d2(q, r) - np.asarray(radii2)[None, :])
    return int((gap <= d2_bound(q, r) + np.asarray(radii2_bound)[None, :]).sum())


def undecided_coverage(real, fake, radii2_real, radii2_bound):
    """the same for coverage's comparison nearest2_i <= radii2_real[i]: the elements of row i against row i's own radius"""
    gap = np.abs(d2(real, fake) - np.asarray(radii2_real)[:, None])
    return int((gap <= d2_bound(real, fake) + np.asarray(radii2_bound)[:, None]).sum())


def undecided_radii(x, k):
    """(count, smallest gap / bound): the rows whose k-th smallest distance is within twice the row's largest bound of the
    (k-1)-th or the (k+1)-th -- where a permitted error could make another element the k-th"""
    d, b = _others(x)
    s = np.sort(d, axis=1)
    worst = 2 * b.max(axis=1)
    gaps = np.full(len(x), np.inf)
    if k >= 2:
        gaps = np.minimum(gaps, s[:, k - 1] - s[:, k - 2])
    if k < s.shape[1]:
        gaps = np.minimum(gaps, s[:, k] - s[:, k - 1])
    return int((gaps <= worst).sum()), float((gaps / worst).min())


@functools.lru_cache(maxsize=None)
def reference(nx, ny, d, k):
    """Everything the tests compare against at one case of `cases()`, computed once and read-only: the banks x (real) and y
    (fake), their radii and radius bounds, counts and nearest distances in both directions (`fake_in_real`: queries y, bank x;
    `real_in_fake`: queries x, bank y) and the four values"""
    x, y = shape_banks(nx, ny, d)
    out = dict(x=x, y=y, radii_x=radii(x, k), radii_y=radii(y, k), radii_bound_x=radii_bound(x, k), radii_bound_y=radii_bound(y, k))
    out['fake_in_real'] = counts(y, x, out['radii_x'])
    out['real_in_fake'] = counts(x, y, out['radii_y'])
    out['nearest_bound_fake'] = d2_bound(y, x).max(axis=1)
    out['nearest_bound_real'] = d2_bound(x, y).max(axis=1)
    out['prdc'] = prdc(x, y, k)
    for v in out.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out
