"""Precision / recall and density / coverage on the GPU: which of the two went wrong, sample quality or sample diversity, on
the pool_3 features that FID and KID use.

    improved precision and recall (Kynkaanniemi et al., "Improved Precision and Recall Metric for Assessing Generative
    Models", 2019): the manifold of a set is the union of the balls around its rows that reach to the row's k-th nearest
    neighbour inside the set.  precision = the share of fake rows inside the real manifold, recall = the share of real rows
    inside the fake manifold.
    density and coverage (Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models", 2020), robust to
    outliers: density = the number of real balls a fake row lies in, summed over the fake rows, / (k N_fake); coverage = the
    share of real rows whose own ball holds at least one fake row.

With count_i = #{j : d2(q_i, b_j) <= radius2(b_j)} and nearest2_i = min_j d2(q_i, b_j) for queries q against a bank b:

    precision = mean over fake i of count_i > 0            bank = real with the real radii
    density   = sum_i count_i / (k N_fake)                 the same launch
    recall    = mean over real i of count_i > 0            bank = fake with the fake radii
    coverage  = mean over real i of nearest2_i <= radius2_real[i]      that same second launch

k = 3 is the default of the precision / recall paper and the default here; the density / coverage paper uses k = 5.

Stages:  images -> `kid.image_features` / `kid.sample_features`: the float32 features of a set stay on the device in a `FeatureBank`
         -> `K.prd_knn_radii` (csrc/prd.hip) per side: squared k-NN radii, float64 on the f64 MFMA, self excluded by index
         -> `K.prd_manifold_counts` per direction: counts (int32) and nearest squared distances (float64)
         -> one copy back per side, the four fractions in NumPy.
Everything is float64 on the device because the comparisons are exact questions: a count changes when a distance crosses a
radius, and a radius IS one of the distances of its bank.  There is no CPU path; the real Inception weights are a download
(common/inception/inception_v3.py), so `net` is always the caller's, as for FID and KID.
"""
import numpy as np
import torch

from .. import kernels as K
from .fid import _NO_WEIGHTS
from .kid import FeatureBank, image_features


def _device_features(side, name):
    if isinstance(side, FeatureBank):
        side = side.features
    if getattr(side, 'ndim', 0) != 2:
        raise ValueError(f"precision_recall: {name} {tuple(getattr(side, 'shape', ()))}, expected features [N, D]")
    if isinstance(side, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("gank: the precision / recall statistics run on the GPU (no CPU path exists)")
        side = torch.from_numpy(np.ascontiguousarray(side, dtype=np.float32)).cuda()
    if side.dtype != torch.float32:
        side = side.float()
    return side.contiguous()


def _check_rows(n, k, name):
    if not 1 <= k <= 8:
        raise ValueError(f"precision_recall: k = {k} unsupported (1..8)")
    if n < k + 1:
        raise ValueError(f"precision_recall: {name} has {n} rows, the k = {k} nearest neighbours need at least {k + 1}")


def knn_radii(features, k=3):
    """features: a FeatureBank or [N, D] (device tensor or NumPy) -> float64 [N] on the device: the SQUARED distance of every
    row to its k-th nearest other row (self excluded by index: a duplicated row is a neighbour at distance 0)"""
    _check_rows(len(features), k, "features")
    return K.prd_knn_radii(_device_features(features, "features"), k)


def manifold_counts(queries, bank, radii2):
    """-> (count int32 [Nq], nearest2 float64 [Nq]) on the device: per query row the number of bank rows whose ball (squared
    radius radii2[j], `knn_radii(bank)`) holds it, boundary included, and the squared distance to the nearest bank row"""
    return K.prd_manifold_counts(_device_features(queries, "queries"), _device_features(bank, "bank"), radii2)


def _features(side, net):
    if isinstance(side, FeatureBank):
        return side
    ndim = getattr(side, 'ndim', 0)
    if ndim == 2:
        return side
    if ndim == 4:
        if net is None:
            raise NotImplementedError(_NO_WEIGHTS)
        return image_features(side, net)
    raise TypeError(f"calculate_prdc: a FeatureBank, features [N, D] or images [N,H,W,3], not {type(side).__name__}")


def calculate_prdc(real, fake, net=None, k=3):
    """Precision, recall, density and coverage (module docstring) of `fake` against `real`, each side a FeatureBank, features
    [N, D] (NumPy or device tensor) or images [N,H,W,3]; `net` (an InceptionV3) is needed only for images, as in
    `calculate_kid`.  k = 3 is the default of the precision / recall paper, k = 5 that of the density / coverage paper.
    -> dict(precision, recall, density, coverage) of Python floats.  Two radii passes and two counts passes on the device,
    one copy back of counts and minima per side."""
    real, fake = _features(real, net), _features(fake, net)
    _check_rows(len(real), k, "real")
    _check_rows(len(fake), k, "fake")
    real, fake = _device_features(real, "real"), _device_features(fake, "fake")
    radii_real, radii_fake = K.prd_knn_radii(real, k), K.prd_knn_radii(fake, k)
    count_fake, _ = K.prd_manifold_counts(fake, real, radii_real)
    count_real, nearest_real = K.prd_manifold_counts(real, fake, radii_fake)
    count_fake = count_fake.cpu().numpy()
    count_real, nearest_real, radii_real = count_real.cpu().numpy(), nearest_real.cpu().numpy(), radii_real.cpu().numpy()
    return dict(precision=float(np.mean(count_fake > 0)),
                recall=float(np.mean(count_real > 0)),
                density=float(count_fake.sum(dtype=np.int64) / (k * len(count_fake))),
                coverage=float(np.mean(nearest_real <= radii_real)))


def precision_recall(real, fake, net=None, k=3):
    """(precision, recall) of `calculate_prdc`; k = 3 is the paper's default"""
    out = calculate_prdc(real, fake, net, k)
    return out['precision'], out['recall']


def density_coverage(real, fake, net=None, k=5):
    """(density, coverage) of `calculate_prdc`; k = 5 is the paper's default"""
    out = calculate_prdc(real, fake, net, k)
    return out['density'], out['coverage']
