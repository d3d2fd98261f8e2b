"""NumPy float64 restatement of the Kernel Inception Distance for the tests (imports nothing from the product, no torch):
the three block sums of the polynomial kernel by brute force (full m x m matrices, the diagonal removed with a mask), the
unbiased MMD^2, the subset protocol, and the "absolute" sums that the tests' error bound needs."""
import numpy as np


def _kernel(a, b, gamma, coef0, degree):
    return (gamma * (a @ b.T) + coef0) ** degree


def block_sums(x, y, ix, iy, gamma, coef0, degree):
    """-> (sums, absolute), both float64 [subsets, 3]: per subset (sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j),
    sum_{i, j} k(x_i, y_j)) over the rows x[ix[s]], y[iy[s]], and the same sums of T_ij^degree with
    T_ij = gamma sum_k |a_ik| |b_jk| + |coef0|"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    ix, iy = np.asarray(ix), np.asarray(iy)
    subsets, m = ix.shape
    off = ~np.eye(m, dtype=bool)
    sums, absolute = np.zeros((subsets, 3)), np.zeros((subsets, 3))
    for s in range(subsets):
        a, b = x[ix[s]], y[iy[s]]
        for out, (p, q), g, c in ((sums, (a, b), gamma, coef0), (absolute, (np.abs(a), np.abs(b)), abs(gamma), abs(coef0))):
            out[s, 0] = _kernel(p, p, g, c, degree)[off].sum()
            out[s, 1] = _kernel(q, q, g, c, degree)[off].sum()
            out[s, 2] = _kernel(p, q, g, c, degree).sum()
    return sums, absolute


def mmd2(sums, m):
    """block sums [subsets, 3] -> the unbiased MMD^2 per subset"""
    sums = np.asarray(sums, np.float64)
    return sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2 * sums[:, 2] / (m * m)


def kernel_distance(x, y, ix, iy, degree=3, gamma=None, coef0=1.0):
    """-> (mean, std (ddof = 0), mmd2 per subset, block sums, absolute sums) on the given row tables"""
    x = np.asarray(x, np.float64)
    if gamma is None:
        gamma = 1.0 / x.shape[1]
    sums, absolute = block_sums(x, y, ix, iy, gamma, coef0, degree)
    per = mmd2(sums, np.asarray(ix).shape[1])
    return float(per.mean()), float(per.std()), per, sums, absolute


def sum_bound(absolute, m, d, degree=3):
    """The tests' bound on |S - S_ref| per block sum, [subsets, 3].  The products of two float32 values are exact in float64; a
    dot product carries at most D roundings, the affine map and the power at most 8 more, each scaling with T_ij^degree to
    first order `degree` times (3 D + 8 covers degree <= 3); a block sum of P addends carries at most P more in any order;
    the factor 2 covers the reference's own rounding."""
    p = np.array([m * (m - 1), m * (m - 1), m * m], np.float64)
    return 2 * (3 * d + 8 + p) * 2.0 ** -53 * np.asarray(absolute, np.float64)
