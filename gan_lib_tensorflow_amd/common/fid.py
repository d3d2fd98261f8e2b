"""Frechet Inception Distance on the GPU: the FID column of the reference README's "Quantitative evaluation" table (3.2 for
CIFAR-10 train vs test) and the first entry of its TODO list.

    FID = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2),   (mu, S) = mean and covariance of the pool_3 features of a set

Stages:  images -> `InceptionV3.features_f32` (the HIP trunk of the Inception-score harness, pool_3 kept in fp32)
         -> `FeatureMoments.update`, one gank_moments_update launch per batch (csrc/fid.hip): running float64 sums and the upper
            tiles of the float64 Gram matrix on the f64 MFMA -- features never leave the device, no atomics, bit-reproducible
         -> `FeatureMoments.finalize`: one copy back, mean and covariance in float64
         -> `frechet_distance`: NumPy float64 on the host, as `preds2score` is for the Inception score.
There is no CPU path for the first two stages.  The real Inception weights are a download (common/inception/inception_v3.py), so
`net` is always the caller's: with random weights the number is a test quantity, not the published one.

The matrix square root.  tr sqrt(S1 S2) = sum of the square roots of the eigenvalues of S1^(1/2) S2 S1^(1/2), a symmetric PSD
matrix: two `eigh` calls and no general `sqrtm`.  In both spectra eigenvalues below D * 2^-52 * lambda_max are set to zero: they
are rounding noise of a rank-deficient covariance (N < D samples), and sqrt turns noise of size e into sqrt(e).  With the
threshold rank-deficient statistics are well defined and need no "add eps to the diagonal" branch.
"""
import os

import numpy as np
import torch

from .. import kernels as K

_NO_WEIGHTS = ('the Inception classifier needs downloaded weights (inception_score.py:29-47): pass '
               'net=InceptionV3.from_npz(path)')


def moments_from_sums(count, total, gram):
    """(count, sum_i x_i, upper triangle of sum_i x_i x_i^T; whatever lies below the diagonal is ignored) ->
    (mu float64 [D], sigma float64 [D, D]) with sigma = (G - s s^T / N) / (N - 1), np.cov's normalisation."""
    n = int(count)
    if n < 2:
        raise ValueError(f"FID statistics need at least 2 samples, got {n}")
    s = np.asarray(total, np.float64)
    g = np.asarray(gram, np.float64)
    g = np.triu(g) + np.triu(g, 1).T
    return s / n, (g - np.outer(s, s) / n) / (n - 1)


class FeatureMoments:
    """Running first and second moments of a feature set [*, dim]: `sum` float64 [dim] and `gram` float64 [dim, dim] live on the
    device (one buffer; of gram only the 16 x 16 tiles on and above the diagonal are maintained), `count` is the row count."""

    def __init__(self, dim, device='cuda'):
        if dim % 16 or not 16 <= dim <= 4096:
            raise ValueError(f"FeatureMoments: dim = {dim}, needs a multiple of 16 in 16..4096 (gank_moments_update)")
        self.dim, self.count = dim, 0
        self._buf = torch.zeros(dim + dim * dim, dtype=torch.float64, device=device)
        self.sum, self.gram = self._buf[:dim], self._buf[dim:].view(dim, dim)
        self._stats = None

    def update(self, features):
        """features [n, dim]: a GPU tensor in the 16-bit activation dtype or float32, or a NumPy array (uploaded as float32)"""
        if isinstance(features, np.ndarray):
            if not torch.cuda.is_available():
                raise RuntimeError("gank: the FID statistics run on the GPU (no CPU path exists)")
            features = torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(self._buf.device)
        if features.dim() != 2 or features.shape[1] != self.dim:
            raise RuntimeError(f"FeatureMoments.update: features {tuple(features.shape)}, expected [n, {self.dim}]")
        if features.shape[0]:
            K.moments_update(features.contiguous(), self.sum, self.gram)
            self.count += features.shape[0]
            self._stats = None
        return self

    def finalize(self):
        """-> (mu float64 [dim], sigma float64 [dim, dim]); one copy back, the rest in float64 on the host"""
        if self._stats is None:
            host = self._buf.cpu().numpy()
            self._stats = moments_from_sums(self.count, host[:self.dim], host[self.dim:].reshape(self.dim, self.dim))
        return self._stats

    def save(self, path):
        """.npz with `mu` and `sigma` (the layout of the precomputed-statistics files FID users have) plus `count`"""
        mu, sigma = self.finalize()
        np.savez(path, mu=mu, sigma=sigma, count=np.int64(self.count))

    @staticmethod
    def load(path):
        """-> (mu, sigma) float64 from an .npz with keys `mu` and `sigma`"""
        with np.load(path) as f:
            return np.asarray(f['mu'], np.float64), np.asarray(f['sigma'], np.float64)


def _psd_sqrt_spectrum(w, dim):
    """square roots of a PSD matrix's eigenvalues; those below dim * 2^-52 * lambda_max (noise, or negative) count as zero"""
    cut = max(dim * 2.0 ** -52 * float(w.max()), 0.0)
    return np.sqrt(np.where(w > cut, w, 0.0))


def frechet_distance(mu1, sigma1, mu2, sigma2):
    """|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrt(S1 S2), NumPy float64 (module docstring: the eigen form and its threshold)"""
    mu1, mu2 = np.asarray(mu1, np.float64).ravel(), np.asarray(mu2, np.float64).ravel()
    s1, s2 = np.asarray(sigma1, np.float64), np.asarray(sigma2, np.float64)
    d = mu1.size
    if mu2.size != d or s1.shape != (d, d) or s2.shape != (d, d):
        raise ValueError(f"frechet_distance: shapes {mu1.shape} {s1.shape} {mu2.shape} {s2.shape} do not fit")
    w1, v1 = np.linalg.eigh((s1 + s1.T) / 2)
    root = (v1 * _psd_sqrt_spectrum(w1, d)) @ v1.T                      # S1^(1/2)
    m = root @ s2 @ root
    tr_sqrt = _psd_sqrt_spectrum(np.linalg.eigvalsh((m + m.T) / 2), d).sum()
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * tr_sqrt)


def _unit_range(batch):
    """a batch of pixel values 0..255 -> [-1, 1] exactly as get_inception_score maps them (inception_score.py:72-73:
    `2 * (images / 255. - 0.5)` in float64, then float32); NumPy or torch, stays where it is"""
    if isinstance(batch, np.ndarray):
        return (2 * (batch / 255. - 0.5)).astype(np.float32)
    return (2 * (batch.double() / 255. - 0.5)).float()


def image_moments(images, net, batch_size=100):
    """images [N,H,W,3] (NumPy or torch; integer pixel values, float pixel values (max of the first image > 1.01, the test of
    get_inception_score) or already in [-1, 1]) -> FeatureMoments of their `net.features_f32`, whole and trailing partial batches"""
    if net is None:
        raise NotImplementedError(_NO_WEIGHTS)
    assert images.ndim == 4 and images.shape[3] == 3, tuple(images.shape)
    if isinstance(images, np.ndarray):
        pixels = images.dtype.kind in 'iu' or float(np.max(images[0])) > 1.01
    else:
        pixels = not images.dtype.is_floating_point or float(images[0].max()) > 1.01
    mom = FeatureMoments(2048, net.device)
    for i in range(0, len(images), batch_size):
        batch = images[i:i + batch_size]
        mom.update(net.features_f32(_unit_range(batch) if pixels else batch))
    return mom


def draw_until(draw, n):
    """The batches of n generated rows: draw() -> a batch [b >= 1, ...] is called while rows are missing and the last batch is
    cut to the rows still needed.  draw() is never called once n rows are in: a call advances the device RNG."""
    have = 0
    while have < n:
        batch = draw()[:n - have]
        have += len(batch)
        yield batch


def sample_moments(draw, n, net):
    """FeatureMoments of n generated samples: draw() -> uint8 images [b,H,W,3] on the device, quantised as for the Inception
    score (msssim.quantize_on_device), called until n are in (`draw_until`); samples and features stay on the device"""
    if net is None:
        raise NotImplementedError(_NO_WEIGHTS)
    mom = FeatureMoments(2048, net.device)
    for batch in draw_until(draw, n):
        mom.update(net.features_f32(_unit_range(batch)))
    return mom


def _statistics(side, net):
    if isinstance(side, FeatureMoments):
        return side.finalize()
    if isinstance(side, (str, os.PathLike)):
        return FeatureMoments.load(side)
    if isinstance(side, (tuple, list)) and len(side) == 2:
        return side
    if getattr(side, 'ndim', 0) == 4:
        return image_moments(side, net).finalize()
    raise TypeError(f"calculate_fid: a FeatureMoments, a (mu, sigma) pair, an .npz path or images [N,H,W,3], not {type(side).__name__}")


def calculate_fid(a, b, net=None):
    """FID between two sides, each a FeatureMoments, a (mu, sigma) pair, the path of an .npz with `mu` and `sigma`, or images
    [N,H,W,3]; `net` (an InceptionV3) is needed only for images"""
    return frechet_distance(*_statistics(a, net), *_statistics(b, net))


def cifar10_moments(data_dir, net, split='train'):
    """FeatureMoments of a CIFAR-10 split (the python-version pickles of common/data/cifar10.py); with `calculate_fid` on the
    two splits this is the reference README's "train vs test" protocol"""
    from .data.cifar10 import unpickle
    files = {'train': ['data_batch_%d' % i for i in range(1, 6)], 'test': ['test_batch']}[split]
    rows = np.concatenate([np.asarray(unpickle(os.path.join(data_dir, f))[0], dtype=np.uint8) for f in files], axis=0)
    return image_moments(rows.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1), net)       # CHW-planar rows -> HWC
