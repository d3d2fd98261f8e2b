"""NumPy float64 restatement of the sliced Wasserstein distance on Laplacian-pyramid patches (Karras et al., "Progressive
Growing of GANs", ICLR 2018, section 5) for the tests.  Imports nothing from the product and no torch.  It follows the paper
and its published evaluation program; that program is not at hand here, so PARITY WITH IT IS UNPINNED.  Known departures:
the directions stay float64 (there: cast to float32); the patch centres are one table per level and side (there: one per
minibatch, the same distribution); every array is float64 (there: float32 descriptors).

The draws, all from one numpy.random.RandomState(seed): the direction matrices first, one randn(K, dirs_per_repeat) per
repeat; then for side a, then side b, level by level, x = randint(h, W - h, M) and then y = randint(h, H - h, M).

Exactness of the pyramid.  For uint8 input a pyr_down value is a multiple of 2^-8 below 256, a second one of 2^-16, a pyr_up of
those a multiple of 2^-14 resp. 2^-22, and so is every partial sum of the stencils: at most 30 bits, so the float64 pyramid of
up to three levels is exact in any order of summation (`pyramid_int` proves it for two levels on integers scaled by 2^14).

Bound on a key, derived and not measured.  u = 2^-53; n = M nhood^2 elements per channel, A = mean |x|, K = C nhood^2.
  mean   m = fl(S / n), S a float64 sum of n terms in ANY order: |m - mu| <= (n + 1) u A =: em.
  std    the product forms D1 = sum (x - m), D2 = sum (x - m)^2 and var = D2 / n - (D1 / n)^2 (the restatement: np.std, which is
         D2 / n about its own mean).  The exact variance is D2 / n - (mu - m)^2.  A sum of n squares carries a relative error of
         at most (n + 2) u, the correction is at most q^2 with q = em + n u sqrt(D2 / n), the division, subtraction and root a
         few u more; a root halves a relative error, which pays for the second-order terms:  |s' - s| / s <= (n + 8) u + q^2 / var
         =: rs.
  key    sum_k z_k d_k with z_k = (x_k - m) / s and |d|_2 = 1.  A changed s scales z by 1 + rs: the key moves by at most
         rs |z|_2 (Cauchy-Schwarz).  A changed m moves every z_k of channel c by em_c (1 + rs) / s_c and sum_k |d_k| <= sqrt(K).
         The subtraction, the division, the product and the K - 1 additions (fused multiply-adds: fewer roundings) add at most
         (K + 3) u sum |z_k d_k| <= (K + 3) u |z|_2, 1.01 for second order.  With Zn = the largest |z|_2 of a patch:
         |key' - key| <= (rs + 1.01 (K + 3) u) Zn + sqrt(K) max_c em_c (1 + rs) / s_c          per computation,
         twice that between two computations (the product's and this restatement's).
Sorting is non-expansive, mean_r |sort(a')_r - sort(a)_r| <= max_r |a'_r - a_r|, so a level's value moves by at most the key
bound of side a plus that of side b (`level_bound`, in the x 1000 units of the result)."""
import functools

import numpy as np

WINDOW = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]) / 256.0
U = 2.0 ** -53


def level_sizes(h, w):
    sizes = [(h, w)]
    while min(h, w) >= 32:
        assert h % 2 == 0 and w % 2 == 0
        h, w = h // 2, w // 2
        sizes.append((h, w))
    return sizes


def _convolve(x, window):
    """[N,H,W,C] with a 5 x 5 window, NumPy's `reflect` boundary (-1 -> 1, H -> H - 2)"""
    n, h, w, c = x.shape
    p = np.pad(x, ((0, 0), (2, 2), (2, 2), (0, 0)), mode='reflect')
    out = np.zeros_like(x, dtype=np.float64)
    for a in range(5):
        for b in range(5):
            out += window[a, b] * p[:, a:a + h, b:b + w, :]
    return out


def pyr_down(x):
    x = np.asarray(x, np.float64)
    assert x.shape[1] % 2 == 0 and x.shape[2] % 2 == 0 and min(x.shape[1:3]) >= 4
    return _convolve(x, WINDOW)[:, ::2, ::2, :]


def pyr_up(x):
    x = np.asarray(x, np.float64)
    n, h, w, c = x.shape
    z = np.zeros((n, 2 * h, 2 * w, c))
    z[:, ::2, ::2, :] = x
    return _convolve(z, 4.0 * WINDOW)


def laplacian_pyramid(images):
    levels = [np.asarray(images, np.float64)]
    for _ in level_sizes(images.shape[1], images.shape[2])[1:]:
        levels.append(pyr_down(levels[-1]))
    return [levels[i] - pyr_up(levels[i + 1]) for i in range(len(levels) - 1)] + [levels[-1]]


def pyramid_int(images):
    """the two-level pyramid of uint8 images on int64 scaled by 2^14 -> (level0 * 2^14, level1 * 2^14)"""
    k = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1]).astype(np.int64)

    def conv(x):
        n, h, w, c = x.shape
        p = np.pad(x, ((0, 0), (2, 2), (2, 2), (0, 0)), mode='reflect')
        out = np.zeros_like(x)
        for a in range(5):
            for b in range(5):
                out += k[a, b] * p[:, a:a + h, b:b + w, :]
        return out
    x = images.astype(np.int64)
    down = conv(x)[:, ::2, ::2, :]                      # * 2^8
    z = np.zeros_like(x)
    z[:, ::2, ::2, :] = down
    up = conv(z)                                        # * 2^8 * 2^6 (the window times 4 is k / 64)
    return x * 2 ** 14 - up, down * 2 ** 6


def draw_tables(n, h, w, c, nhood_size, nhoods_per_image, dir_repeats, dirs_per_repeat, seed):
    rng = np.random.RandomState(seed)
    k, half, m = c * nhood_size ** 2, nhood_size // 2, n * nhoods_per_image
    dirs = []
    for _ in range(dir_repeats):
        d = rng.randn(k, dirs_per_repeat)
        dirs.append(d / np.sqrt(np.sum(np.square(d), axis=0, keepdims=True)))
    sides = []
    for _ in range(2):
        side = []
        for lh, lw in level_sizes(h, w):
            cx = rng.randint(half, lw - half, m).astype(np.int32)
            cy = rng.randint(half, lh - half, m).astype(np.int32)
            side.append((cx, cy))
        sides.append(side)
    return np.stack(dirs), sides[0], sides[1]


def patches(level, cx, cy, nhood_size, nhoods_per_image):
    """[M, C, nhood, nhood] float64"""
    half, m = nhood_size // 2, len(cx)
    img = np.arange(m) // nhoods_per_image
    off = np.arange(nhood_size) - half
    yy = np.asarray(cy)[:, None, None] + off[None, :, None]
    xx = np.asarray(cx)[:, None, None] + off[None, None, :]
    return np.asarray(level, np.float64)[img[:, None, None], yy, xx, :].transpose(0, 3, 1, 2)


def patch_sums(level, cx, cy, nhood_size, nhoods_per_image):
    """[C, 2]: sum x and sum x^2 per channel"""
    p = patches(level, cx, cy, nhood_size, nhoods_per_image)
    return np.stack([p.sum(axis=(0, 2, 3)), np.square(p).sum(axis=(0, 2, 3))], axis=1)


def mean_std(p):
    return p.mean(axis=(0, 2, 3)), p.std(axis=(0, 2, 3))


def keys(level, cx, cy, nhood_size, nhoods_per_image, dirs):
    """[ndirs, M]: the normalised descriptors projected on dirs [K, ndirs]"""
    p = patches(level, cx, cy, nhood_size, nhoods_per_image)
    mean, std = mean_std(p)
    z = (p - mean[None, :, None, None]) / std[None, :, None, None]
    return (z.reshape(len(cx), -1) @ dirs).T


def key_bound(level, cx, cy, nhood_size, nhoods_per_image):
    """the bound on |key' - key| between two float64 computations (module docstring)"""
    p = patches(level, cx, cy, nhood_size, nhoods_per_image)
    n, k = p.shape[0] * nhood_size ** 2, p.shape[1] * nhood_size ** 2
    mean, std = mean_std(p)
    rs, shift = 0.0, 0.0
    for c in range(p.shape[1]):
        em = (n + 1) * U * np.abs(p[:, c]).mean()
        q = em + n * U * std[c] * 1.01
        rs_c = (n + 8) * U + q * q / (std[c] ** 2)
        rs, shift = max(rs, rs_c), max(shift, em * (1 + rs_c) / std[c])
    z = (p - mean[None, :, None, None]) / std[None, :, None, None]
    zn = np.sqrt(np.square(z).sum(axis=(1, 2, 3))).max()
    return 2.0 * ((rs + 1.01 * (k + 3) * U) * zn + np.sqrt(k) * shift)


def sliced_wasserstein(level_a, level_b, centres_a, centres_b, dirs, nhood_size, nhoods_per_image):
    out = []
    for d in dirs:
        ka = np.sort(keys(level_a, centres_a[0], centres_a[1], nhood_size, nhoods_per_image, d), axis=1)
        kb = np.sort(keys(level_b, centres_b[0], centres_b[1], nhood_size, nhoods_per_image, d), axis=1)
        assert ka.shape == kb.shape
        out.append(np.mean(np.abs(ka - kb)))
    return float(np.mean(out))


def level_bound(level_a, level_b, centres_a, centres_b, nhood_size, nhoods_per_image):
    """the bound on a level's value, x 1000"""
    return 1e3 * (key_bound(level_a, centres_a[0], centres_a[1], nhood_size, nhoods_per_image) +
                  key_bound(level_b, centres_b[0], centres_b[1], nhood_size, nhoods_per_image))


def calculate_swd(a, b, nhood_size=7, nhoods_per_image=128, dir_repeats=4, dirs_per_repeat=128, seed=0):
    """-> (float64 [levels] x 1000, their mean, float64 [levels] bounds x 1000)"""
    assert a.shape == b.shape
    n, h, w, c = a.shape
    dirs, ca, cb = draw_tables(n, h, w, c, nhood_size, nhoods_per_image, dir_repeats, dirs_per_repeat, seed)
    pa, pb = laplacian_pyramid(a), laplacian_pyramid(b)
    values = np.array([sliced_wasserstein(la, lb, xa, xb, dirs, nhood_size, nhoods_per_image) for la, lb, xa, xb in zip(pa, pb, ca, cb)]) * 1e3
    bounds = np.array([level_bound(la, lb, xa, xb, nhood_size, nhoods_per_image) for la, lb, xa, xb in zip(pa, pb, ca, cb)])
    return values, float(values.mean()), bounds


# ---- the cases the GPU tests use
E2E = [dict(shape=(16, 32, 32, 3), nhoods_per_image=16, dir_repeats=2, dirs_per_repeat=8),
       dict(shape=(4, 64, 64, 3), nhoods_per_image=16, dir_repeats=2, dirs_per_repeat=8)]
# (level shape, nhood_size, ndirs) for the stats and projection kernels: N = 3, 5 patches per image
PROJ = [((3, 16, 16, 3), 7, 3), ((3, 16, 16, 3), 3, 128), ((3, 9, 8, 1), 7, 128), ((3, 9, 8, 1), 3, 3)]
PROJ_PER_IMAGE = 5


def cases():
    return list(range(len(E2E)))


@functools.lru_cache(maxsize=None)
def e2e_case(i):
    """two uint8 image sets of case i (a smooth field plus noise on one side, so the levels differ) and the restatement's
    result on seed 0, read-only"""
    cfg = E2E[i]
    rng = np.random.RandomState(100 + i)
    n, h, w, c = cfg['shape']
    a = rng.randint(0, 256, size=cfg['shape']).astype(np.uint8)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    smooth = 127 + 60 * np.sin(yy / 5.0)[None, :, :, None] * np.cos(xx / 7.0)[None, :, :, None]
    b = np.clip(smooth + rng.normal(0, 40, size=cfg['shape']), 0, 255).astype(np.uint8)
    kw = dict(nhood_size=7, nhoods_per_image=cfg['nhoods_per_image'], dir_repeats=cfg['dir_repeats'], dirs_per_repeat=cfg['dirs_per_repeat'])
    values, mean, bounds = calculate_swd(a, b, seed=0, **kw)
    out = dict(a=a, b=b, kw=kw, values=values, mean=mean, bounds=bounds)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def proj_case(i, four_bit=False):
    """a level, centre tables that hold all four extreme centres and a repeated one, directions, and the restatement's sums,
    mean / std, keys and key bound, read-only"""
    shape, nhood, ndirs = PROJ[i]
    n, h, w, c = shape
    rng = np.random.RandomState(200 + i)
    if four_bit:
        level = rng.randint(0, 16, size=shape).astype(np.float64)
    else:
        level = 127.0 + 50.0 * rng.randn(*shape)           # the coarsest level's range: a large mean
    half, m = nhood // 2, n * PROJ_PER_IMAGE
    cx = rng.randint(half, w - half, m).astype(np.int32)
    cy = rng.randint(half, h - half, m).astype(np.int32)
    cx[:4], cy[:4] = [half, w - half - 1, half, w - half - 1], [half, half, h - half - 1, h - half - 1]
    cx[6], cy[6] = cx[5], cy[5]                             # a repeated centre (the same image: 5 patches per image)
    d = rng.randn(c * nhood * nhood, ndirs)
    d /= np.sqrt(np.sum(np.square(d), axis=0, keepdims=True))
    p = patches(level, cx, cy, nhood, PROJ_PER_IMAGE)
    mean, std = mean_std(p)
    out = dict(level=level, cx=cx, cy=cy, nhood=nhood, dirs=d, sums=patch_sums(level, cx, cy, nhood, PROJ_PER_IMAGE), mean=mean, std=std,
               keys=keys(level, cx, cy, nhood, PROJ_PER_IMAGE, d), key_bound=key_bound(level, cx, cy, nhood, PROJ_PER_IMAGE))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
