"""Kernel Inception Distance on the GPU (Binkowski et al., "Demystifying MMD GANs"): the unbiased estimator of the squared
maximum mean discrepancy between the pool_3 features of two image sets under the polynomial kernel

    k(a, b) = (gamma <a, b> + coef0)^degree,      degree = 3, gamma = 1 / dim, coef0 = 1
    MMD^2 = sum_{i != j} k(x_i, x_j) / (m (m - 1)) + sum_{i != j} k(y_i, y_j) / (m (m - 1)) - 2 sum_{i, j} k(x_i, y_j) / m^2

averaged over `subsets` random subsets of `subset_size` rows a side (the standard protocol: 100 subsets of 1000), reported with
the standard deviation over the subsets.  Unlike FID (common/fid.py) it is unbiased in the sample count, defined for any
N >= 2 and needs no covariance of a thin sample: the number for a 10 000-image split or a single class.

Stages:  images -> `InceptionV3.features_f32` -> `FeatureBank.append`: the float32 features of a set stay on the device
         -> `draw_subsets`: int32 row tables from a seeded NumPy RandomState, uploaded once
         -> `K.kid_block_sums` (csrc/kid.hip): the three block sums of every subset in float64 on the f64 MFMA, gathered
            through the tables; no atomics, bit-reproducible
         -> `polynomial_mmd2`: one copy back of [subsets, 3], the normalisation in NumPy float64.
There is no CPU path for the first and third stages.  The real Inception weights are a download
(common/inception/inception_v3.py), so `net` is always the caller's, as for FID.
"""
import os

import numpy as np
import torch

from .. import kernels as K
from .fid import _NO_WEIGHTS, _unit_range, draw_until


class FeatureBank:
    """The features of a set, float32 [capacity, dim] on the device, filled by `append`; `count` rows are in, `features` is
    the filled view."""

    def __init__(self, dim, capacity, device='cuda'):
        if dim % 16 or not 16 <= dim <= 4096:
            raise ValueError(f"FeatureBank: dim = {dim}, needs a multiple of 16 in 16..4096 (gank_kid_block_sums)")
        if capacity < 1:
            raise ValueError(f"FeatureBank: capacity = {capacity}")
        self.dim, self.capacity, self.count = dim, int(capacity), 0
        self._buf = torch.empty((self.capacity, dim), dtype=torch.float32, device=device)

    @property
    def features(self):
        return self._buf[:self.count]

    def __len__(self):
        return self.count

    def append(self, features):
        """features [n, dim]: a GPU tensor in the 16-bit activation dtype or float32, or a NumPy array (uploaded as float32)"""
        if isinstance(features, np.ndarray):
            if not torch.cuda.is_available():
                raise RuntimeError("gank: the KID statistics run on the GPU (no CPU path exists)")
            features = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32))
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise RuntimeError(f"FeatureBank.append: features {tuple(features.shape)}, expected [n, {self.dim}]")
        if features.dtype not in (K.BF16, torch.float32):
            raise RuntimeError(f"FeatureBank.append: features in {K.BF16} or float32, got {features.dtype}")
        n = features.shape[0]
        if self.count + n > self.capacity:
            raise RuntimeError(f"FeatureBank.append: {self.count} + {n} rows exceed the capacity of {self.capacity}")
        self._buf[self.count:self.count + n].copy_(features)        # widens 16-bit features exactly
        self.count += n
        return self


def image_features(images, net, batch_size=100):
    """images [N,H,W,3] (NumPy or torch; integer pixel values, float pixel values (max of the first image > 1.01, the test of
    get_inception_score) or already in [-1, 1]) -> FeatureBank of their `net.features_f32`, whole and trailing partial batches:
    the pixel handling and the loop of fid.image_moments"""
    if net is None:
        raise NotImplementedError(_NO_WEIGHTS)
    assert images.ndim == 4 and images.shape[3] == 3, tuple(images.shape)
    if isinstance(images, np.ndarray):
        pixels = images.dtype.kind in 'iu' or float(np.max(images[0])) > 1.01
    else:
        pixels = not images.dtype.is_floating_point or float(images[0].max()) > 1.01
    bank = FeatureBank(2048, len(images), net.device)
    for i in range(0, len(images), batch_size):
        batch = images[i:i + batch_size]
        bank.append(net.features_f32(_unit_range(batch) if pixels else batch))
    return bank


def sample_features(draw, n, net):
    """FeatureBank of n generated samples: draw() -> uint8 images [b,H,W,3] on the device, quantised as for the Inception
    score (msssim.quantize_on_device), called until n are in; samples and features stay on the device (fid.sample_moments)"""
    if net is None:
        raise NotImplementedError(_NO_WEIGHTS)
    bank = FeatureBank(2048, n, net.device)
    for batch in draw_until(draw, n):
        bank.append(net.features_f32(_unit_range(batch)))
    return bank


def cifar10_features(data_dir, net, split='train'):
    """FeatureBank of a CIFAR-10 split (the python-version pickles of common/data/cifar10.py), as fid.cifar10_moments"""
    from .data.cifar10 import unpickle
    files = {'train': ['data_batch_%d' % i for i in range(1, 6)], 'test': ['test_batch']}[split]
    rows = np.concatenate([np.asarray(unpickle(os.path.join(data_dir, f))[0], dtype=np.uint8) for f in files], axis=0)
    return image_features(rows.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1), net)       # CHW-planar rows -> HWC


def draw_subsets(n, subsets, m, rng):
    """int32 [subsets, m]: row s is rng.choice(n, m, replace=False), rng a numpy.random.RandomState"""
    if not 1 <= m <= n:
        raise ValueError(f"draw_subsets: {m} rows out of {n}")
    if subsets < 1:
        raise ValueError(f"draw_subsets: subsets = {subsets}")
    return np.stack([rng.choice(n, m, replace=False) for _ in range(subsets)]).astype(np.int32)


def _device_features(side, name):
    if isinstance(side, FeatureBank):
        side = side.features
    if isinstance(side, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("gank: the KID statistics run on the GPU (no CPU path exists)")
        side = torch.from_numpy(np.ascontiguousarray(side, dtype=np.float32)).cuda()
    if side.dim() != 2:
        raise ValueError(f"polynomial_mmd2: {name} {tuple(side.shape)}, expected features [N, D]")
    if side.dtype != torch.float32:
        side = side.float()
    return side.contiguous()


def polynomial_mmd2(x, y, ix=None, iy=None, degree=3, gamma=None, coef0=1.0):
    """The unbiased MMD^2 (module docstring) of the rows x[ix[s]] against y[iy[s]] for every subset s -> float64 [subsets] on
    the host.  x, y: a FeatureBank or features [N, D] (device tensor or NumPy); ix, iy: int32 [subsets, m] (`draw_subsets`);
    without tables it is one subset of all rows and needs len(x) == len(y).  gamma=None means 1 / D."""
    x, y = _device_features(x, "x"), _device_features(y, "y")
    if (ix is None) != (iy is None):
        raise ValueError("polynomial_mmd2: give both row tables or neither")
    if ix is None:
        if len(x) != len(y):
            raise ValueError(f"polynomial_mmd2: without row tables the sides must be equally long, got {len(x)} and {len(y)}")
        ix = iy = np.arange(len(x), dtype=np.int32)[None, :]
    m = ix.shape[1]
    if m < 2:
        raise ValueError(f"polynomial_mmd2: {m} rows a side, the unbiased estimator needs at least 2")
    if gamma is None:
        gamma = 1.0 / x.shape[1]
    sums = K.kid_block_sums(x, y, ix, iy, gamma, coef0, degree).cpu().numpy()
    return sums[:, 0] / (m * (m - 1)) + sums[:, 1] / (m * (m - 1)) - 2 * sums[:, 2] / (m * m)


def kernel_distance(x, y, subsets=100, subset_size=1000, seed=0):
    """KID of two feature sets -> (mean, std) of `polynomial_mmd2` over `subsets` subsets of `subset_size` rows a side (clipped
    to the shorter side), drawn without replacement by RandomState(seed): first the table of x, then that of y.  std is
    NumPy's (ddof = 0)."""
    nx, ny = len(x), len(y)
    if nx < 2 or ny < 2:
        raise ValueError(f"kernel_distance: {nx} and {ny} rows, needs at least 2 on each side")
    if subsets < 1:
        raise ValueError(f"kernel_distance: subsets = {subsets}")
    m = min(int(subset_size), nx, ny)
    if m < 2:
        raise ValueError(f"kernel_distance: subset_size = {subset_size}, needs at least 2")
    rng = np.random.RandomState(seed)
    ix = draw_subsets(nx, subsets, m, rng)
    iy = draw_subsets(ny, subsets, m, rng)
    mmd2 = polynomial_mmd2(x, y, ix, iy)
    return float(mmd2.mean()), float(mmd2.std())


def _features(side, net):
    if isinstance(side, FeatureBank):
        return side
    ndim = getattr(side, 'ndim', 0)
    if ndim == 2:
        return side
    if ndim == 4:
        return image_features(side, net)
    raise TypeError(f"calculate_kid: a FeatureBank, features [N, D] or images [N,H,W,3], not {type(side).__name__}")


def calculate_kid(a, b, net=None, **kw):
    """KID between two sides, each a FeatureBank, features [N, D] (NumPy or device tensor) or images [N,H,W,3]; `net` (an
    InceptionV3) is needed only for images; **kw: subsets, subset_size, seed of `kernel_distance` -> (mean, std)"""
    return kernel_distance(_features(a, net), _features(b, net), **kw)
