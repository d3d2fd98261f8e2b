"""NDB and JSD on the GPU (Richardson & Weiss, "On GANs and GMMs", NeurIPS 2018, section 2): which modes of the training data a
generator covers.  It needs no network and no downloaded weights; with the sliced Wasserstein distance (common/swd.py: local
texture) it is the evaluation this library can run from a clean checkout.

    bins         k-means of the training images in pixel space into K bins (Lloyd's iteration, K = 100 in the paper)
    assignment   every generated sample goes to the bin of its nearest centroid
    test         per bin a two-proportion z-test of the training share against the sample share; NDB = the Number of
                 statistically-Different Bins at the significance level, reported also as NDB / K
    JSD          the Jensen-Shannon divergence of the two bin histograms, natural logarithm

Pixel space.  A row is the flat uint8 image, P = H * W * C values, as float32 (0..255 are exact).  Up to `max_dims` = 4096 values
all of them are used (CIFAR-10: P = 3072, no randomness); above, `draw_dims` chooses max_dims of them once per NDB, sorted, and
training images and samples are read at the same positions.

The draws.  Two, each from its own numpy.random.RandomState(seed): `draw_dims` (choice(P, max_dims, replace=False), sorted) and
`draw_init` (choice(n, K, replace=False), in drawn order: the initial centroids are those training rows).

Stages:  images -> `K.ndb_pixel_features` (csrc/ndb.hip) -> per iteration `K.ndb_assign` (nearest centroid in float64 on the
         MFMA tile prd.hip uses, ties to the lowest index), one copy back of the per-strip inertia sums and change counts (the
         one sync of an iteration), `K.ndb_group_rows` (stable counting sort of the rows by label), `K.ndb_centroids` (float64
         means in that order; a cluster without rows keeps its centroid) -> the bin counts come back, the statistics are NumPy
         float64 (`bin_statistics`).
No atomics anywhere and every sum has a fixed order: the same inputs give the same bits.  There is no CPU path.

Not implemented: whitening of the pixel space, k-means++ seeding and multiple restarts (the paper's code uses the library
defaults of its k-means for these); the initial centroids are K distinct training rows and there is one run."""
import math
import os

import numpy as np
import torch

from .. import kernels as K
from .fid import draw_until


def draw_dims(P, max_dims=4096, seed=0):
    """The pixel positions an NDB reads: None when P <= max_dims (all of them, in order), else the sorted int32 [max_dims]
    numpy.random.RandomState(seed).choice(P, max_dims, replace=False).  max_dims: 16..4096."""
    P, max_dims = int(P), int(max_dims)
    if not 16 <= max_dims <= 4096:
        raise ValueError(f"ndb: max_dims = {max_dims} (16..4096)")
    if P < 1:
        raise ValueError(f"ndb: P = {P}")
    if P <= max_dims:
        return None
    return np.sort(np.random.RandomState(seed).choice(P, max_dims, replace=False)).astype(np.int32)


def draw_init(n, K, seed=0):
    """The training rows that are the initial centroids: numpy.random.RandomState(seed).choice(n, K, replace=False), in drawn order"""
    n, K = int(n), int(K)
    if not 1 <= K <= n:
        raise ValueError(f"ndb: {K} bins need at least {K} rows, got {n}")
    return np.random.RandomState(seed).choice(n, K, replace=False)


def kmeans(x, K_bins, seed=0, max_iter=100):
    """Lloyd's iteration on x float32 [n, D] on the device (D % 16 == 0) from the rows `draw_init(n, K_bins, seed)` ->
    (centroids float32 [K_bins, D] on the device, labels int32 [n] on the device, inertia float, iterations).
    An iteration assigns every row and copies back the per-strip inertia sums and change counts; it is the last one when no
    label changed (never the first) or at max_iter; otherwise the rows are grouped and the centroids recomputed.  labels and
    inertia are those of the last assignment; inertia is the sum of the strip sums in index order, NumPy float64."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("gank: x must live on the GPU (no CPU path exists)")
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError(f"ndb: kmeans takes float32 features [n, D], got {tuple(x.shape)} {x.dtype}")
    max_iter = int(max_iter)
    if max_iter < 1:
        raise ValueError(f"ndb: max_iter = {max_iter}")
    n, k = x.shape[0], int(K_bins)
    init = draw_init(n, k, seed)
    c = x[torch.from_numpy(init.astype(np.int64)).to(x.device)].contiguous()
    labels = [torch.empty(n, dtype=torch.int32, device=x.device) for _ in range(2)]
    d2 = torch.empty(n, dtype=torch.float64, device=x.device)
    strips = K.ndb_strips(n)
    part_inertia = torch.empty(strips, dtype=torch.float64, device=x.device)
    part_changed = torch.empty(strips, dtype=torch.int32, device=x.device)
    count, offset = (torch.empty(k, dtype=torch.int32, device=x.device) for _ in range(2))
    perm = torch.empty(n, dtype=torch.int32, device=x.device)
    ws = torch.empty(max(K.ndb_group_ws_elems(n, k), 1), dtype=torch.int32, device=x.device)
    prev, iterations = None, 0
    while True:
        label = labels[iterations % 2]
        K.ndb_assign(x, c, prev=prev, label=label, d2=d2, part_inertia=part_inertia, part_changed=part_changed)
        iterations += 1
        inertia = float(np.cumsum(part_inertia.cpu().numpy())[-1])          # cumsum: index order
        changed = int(part_changed.cpu().numpy().sum(dtype=np.int64))
        if (prev is not None and changed == 0) or iterations >= max_iter:
            return c, label, inertia, iterations
        K.ndb_group_rows(label, k, count=count, offset=offset, perm=perm, ws=ws)
        K.ndb_centroids(x, perm, count, offset, c)
        prev = label


def bin_statistics(train_counts, sample_counts, significance_level=0.05):
    """The test and the divergence on two bin histograms (counts per bin, of any totals), NumPy float64 ->
    dict(ndb, ndb_over_k, js, bin_proportions_train, bin_proportions_samples, different_bins).
    Per bin, p = n_k / N_r and q = m_k / N_f, the pooled P = (n_k + m_k) / (N_r + N_f), SE = sqrt(P (1 - P) (1 / N_r + 1 / N_f)),
    z = (p - q) / SE, the two-sided p-value erfc(|z| / sqrt 2); a bin is different when its p-value < significance_level, and
    never when SE == 0.  js = KL(p || m) / 2 + KL(q || m) / 2 with m = (p + q) / 2, natural logarithm, 0 log 0 = 0."""
    nk, mk = np.asarray(train_counts, dtype=np.float64), np.asarray(sample_counts, dtype=np.float64)
    if nk.ndim != 1 or nk.shape != mk.shape or len(nk) < 1:
        raise ValueError(f"ndb: bin counts {nk.shape} and {mk.shape}, expected two equal [K]")
    nr, nf = nk.sum(), mk.sum()
    if nr <= 0 or nf <= 0 or np.any(nk < 0) or np.any(mk < 0):
        raise ValueError("ndb: bin counts must be non-negative and not all zero")
    p, q = nk / nr, mk / nf
    pooled = (nk + mk) / (nr + nf)
    se = np.sqrt(pooled * (1.0 - pooled) * (1.0 / nr + 1.0 / nf))
    different = np.zeros(len(nk), dtype=bool)
    for i in range(len(nk)):
        if se[i] > 0.0:
            different[i] = math.erfc(abs((p[i] - q[i]) / se[i]) / math.sqrt(2.0)) < significance_level
    m = (p + q) / 2.0

    def kl(a):
        nz = a > 0
        return float(np.sum(a[nz] * np.log(a[nz] / m[nz])))
    ndb = int(different.sum())
    return dict(ndb=ndb, ndb_over_k=ndb / float(len(nk)), js=0.5 * kl(p) + 0.5 * kl(q), bin_proportions_train=p,
                bin_proportions_samples=q, different_bins=np.flatnonzero(different))


def _on_device(a, name):
    if isinstance(a, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("gank: NDB runs on the GPU (no CPU path exists)")
        a = torch.from_numpy(np.ascontiguousarray(a) if a.flags.writeable else a.copy()).cuda()      # (torch cannot wrap a read-only array)
    if not isinstance(a, torch.Tensor):
        raise TypeError(f"ndb: {name} must be a NumPy array or a tensor, got {type(a).__name__}")
    if not a.is_cuda:
        raise RuntimeError(f"gank: {name} must live on the GPU (no CPU path exists)")
    return a.contiguous()


class NDB:
    """The bins of one training set: NDB(train).evaluate(samples) as often as wanted.
    train: uint8 images [N,H,W,C] or float32 features [N,D] with D % 16 == 0 and D <= 4096, NumPy or device tensor.  The fit is
    `kmeans(features, number_of_bins, seed, max_iter)`; for images of more than max_dims values `draw_dims(P, max_dims, seed)`
    chooses the positions.  Kept: `centroids` float32 [K, D] on the device, `dims` (int32 NumPy or None), `train_counts` int64
    [K] (NumPy), `inertia`, `iterations`."""

    def __init__(self, train, number_of_bins=100, significance_level=0.05, max_dims=4096, seed=0, max_iter=100):
        train = _on_device(train, "train")
        self.number_of_bins, self.significance_level = int(number_of_bins), float(significance_level)
        self.is_images = train.dtype == torch.uint8
        if self.is_images:
            if train.dim() != 4:
                raise ValueError(f"ndb: train {tuple(train.shape)}, expected images [N,H,W,C]")
            self.row_shape = tuple(train.shape[1:])
            self.dims = draw_dims(train[0].numel(), max_dims, seed)
        else:
            if train.dim() != 2 or train.dtype != torch.float32 or train.shape[1] % 16 or not 16 <= train.shape[1] <= 4096:
                raise TypeError(f"ndb: train must be uint8 images [N,H,W,C] or float32 features [N,D] with D a multiple of 16 in "
                                f"16..4096, got {tuple(train.shape)} {train.dtype}")
            self.row_shape, self.dims = tuple(train.shape[1:]), None
        x = self._features(train, "train")
        self.centroids, labels, self.inertia, self.iterations = kmeans(x, self.number_of_bins, seed, max_iter)
        self.train_counts = self._counts(labels)

    def _features(self, a, name):
        if tuple(a.shape[1:]) != self.row_shape or a.dtype != (torch.uint8 if self.is_images else torch.float32):
            raise ValueError(f"ndb: {name} {tuple(a.shape)} {a.dtype} is not rows {self.row_shape} of the training set's type")
        return K.ndb_pixel_features(a, self.dims) if self.is_images else a

    def _counts(self, labels):
        return K.ndb_group_rows(labels, self.number_of_bins)[0].cpu().numpy().astype(np.int64)

    def assign(self, samples):
        """the bin of every sample -> int32 [n] on the device"""
        return K.ndb_assign(self._features(_on_device(samples, "samples"), "samples"), self.centroids)[0]

    def evaluate(self, samples):
        """samples of the training set's kind and row shape (NumPy or device tensor) -> `bin_statistics` of the training bin
        counts against the samples' bin counts"""
        return bin_statistics(self.train_counts, self._counts(self.assign(samples)), self.significance_level)


def calculate_ndb(train, samples, **kw):
    """NDB(train, **kw).evaluate(samples)"""
    return NDB(train, **kw).evaluate(samples)


def cifar10_bins(data_dir, split='train', **kw):
    """The bins of CIFAR-10's training images (split='train': data_batch_1..5) or test images ('test': test_batch) under
    data_dir, as [N,32,32,3] like the trainers' samples (common/data/cifar10.py reads the CHW-planar rows)."""
    from .data.cifar10 import unpickle
    files = {'train': [f'data_batch_{i}' for i in range(1, 6)], 'test': ['test_batch']}
    if split not in files:
        raise ValueError(f"ndb: split = {split!r} ('train' or 'test')")
    rows = np.concatenate([np.asarray(unpickle(os.path.join(data_dir, f))[0], dtype=np.uint8) for f in files[split]])
    return NDB(np.ascontiguousarray(rows.reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1)), **kw)


def sample_ndb(draw, ndb, n):
    """`ndb.evaluate` on n generated samples: draw() -> uint8 images [b,H,W,C] on the device, called until n are in
    (fid.draw_until); the samples stay on the device."""
    return ndb.evaluate(torch.cat(list(draw_until(draw, int(n)))))
