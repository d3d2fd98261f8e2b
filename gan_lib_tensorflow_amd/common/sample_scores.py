"""Per-sample realism and rarity scores on the GPU: WHICH samples are the good ones and which the unusual ones, on the k-NN
manifold of the pool_3 features that precision / recall (common/precision_recall.py) reduces to four fractions.

    realism score (Kynkaanniemi et al., "Improved Precision and Recall Metric for Assessing Generative Models", 2019, section
    5): R(q) = max_j r_j / |q - x_j| over the real rows x_j, r_j the k-NN radius of x_j inside the real set.  R >= 1 exactly
    when q lies in a real ball, and its size says how deep.  To keep outliers with huge balls from vouching for everything
    near them, the half of the real rows with the largest radii is dropped first (`prune` = 0.5, the paper's rule).
    rarity score (Han et al., "Rarity Score: A New Metric to Evaluate the Uncommonness of Synthesized Images", ICLR 2023): for
    a sample inside the real manifold the SMALLEST radius among the real balls that hold it -- large where the real data is
    sparse, an unusual sample; a sample in no ball scores 0.

Conventions.  A sample that coincides with a real row (d2 == 0) has realism +inf, also when that row's radius is 0 (a
duplicated real row).  A ball holds its boundary (d2 <= radius2, as the precision counts).  Pruning keeps the
ceil(N_real * (1 - prune)) real rows of smallest squared radius, ties to the lowest index (a stable argsort on the host); the
others get radii2 = -1 in a device COPY, which the kernel skips.  Rarity is never pruned.

Stages:  sides -> features on the device as for `calculate_prdc` -> `K.prd_knn_radii` of the real side
         -> `K.prd_sample_scores` (csrc/prd.hip: gank_prd_scores_*): per fake row max_j radii2_j / d2_ij and the smallest holding
            radii2_j, float64 on the f64 MFMA strips of the counts pass, one IEEE division a pair, no atomics, bit-identical
            for every segment count
         -> one copy back of the [N_fake] vectors (and of radii2, for the pruning), the square roots in NumPy.
Features never leave the device; there is no CPU path, and `net` is always the caller's (as for FID, KID and precision /
recall).
"""
import math

import numpy as np
import torch

from .. import kernels as K
from .precision_recall import _check_rows, _device_features, _features, knn_radii


def _sides(real, fake, net, k):
    real, fake = _features(real, net), _features(fake, net)
    _check_rows(len(real), k, "real")
    if len(fake) < 1:
        raise ValueError("sample_scores: fake has no rows")
    return _device_features(real, "real"), _device_features(fake, "fake")


def _check_prune(prune):
    if not 0.0 <= prune < 1.0:          # (refuses NaN too)
        raise ValueError(f"sample_scores: prune = {prune}, the share of real rows to drop lies in [0, 1)")


def pruned_radii(radii2, prune):
    """radii2 float64 [N] on the device -> a device copy in which all but the ceil(N * (1 - prune)) rows of smallest radii2
    (ties to the lowest index) are -1, the mark `K.prd_sample_scores` skips; radii2 itself when prune == 0"""
    _check_prune(prune)
    if prune == 0:
        return radii2
    n = len(radii2)
    keep = math.ceil(n * (1.0 - prune))
    drop = np.argsort(radii2.cpu().numpy(), kind='stable')[keep:]
    out = radii2.clone()
    out[torch.from_numpy(drop).to(out.device)] = -1.0
    return out


def _realism(ratio2):
    return np.sqrt(ratio2.cpu().numpy())


def _rarity(rare2):
    rare2 = rare2.cpu().numpy()
    inside = np.isfinite(rare2)
    return np.sqrt(np.where(inside, rare2, 0.0)), inside


def realism_scores(real, fake, net=None, k=3, prune=0.5):
    """Realism score (module docstring) of every row of `fake` against `real`, each side a FeatureBank, features [N, D] (NumPy
    or device tensor) or images [N,H,W,3] with `net` -> float64 [N_fake] (NumPy); >= 1: inside the (pruned) real manifold,
    +inf: on a real row.  prune in [0, 1): the share of real rows with the largest radii to drop, 0 keeps all."""
    _check_prune(prune)
    real, fake = _sides(real, fake, net, k)
    return _realism(K.prd_sample_scores(fake, real, pruned_radii(knn_radii(real, k), prune))[0])


def rarity_scores(real, fake, net=None, k=3):
    """Rarity score (module docstring) of every row of `fake` against `real`, sides as in `realism_scores` -> (score float64
    [N_fake], inside bool [N_fake]) (NumPy): the radius of the smallest real ball that holds the row, 0.0 where none does
    (inside == False)."""
    real, fake = _sides(real, fake, net, k)
    return _rarity(K.prd_sample_scores(fake, real, knn_radii(real, k))[1])


def calculate_sample_scores(real, fake, net=None, k=3, prune=0.5):
    """Both scores, the real radii computed once -> dict(realism float64 [N_fake], rarity float64 [N_fake], inside bool
    [N_fake], mean_realism, realistic_fraction (the share with realism >= 1), mean_rarity (over `inside` only, nan if none));
    the scalars are Python floats.  One scores pass with all balls (rarity) and, unless prune == 0, one with the pruned ones
    (realism)."""
    _check_prune(prune)
    real, fake = _sides(real, fake, net, k)
    radii2 = knn_radii(real, k)
    ratio2, rare2 = K.prd_sample_scores(fake, real, radii2)
    if prune != 0:
        ratio2, _ = K.prd_sample_scores(fake, real, pruned_radii(radii2, prune))
    realism = _realism(ratio2)
    rarity, inside = _rarity(rare2)
    return dict(realism=realism, rarity=rarity, inside=inside,
                mean_realism=float(realism.mean()), realistic_fraction=float(np.mean(realism >= 1.0)),
                mean_rarity=float(rarity[inside].mean()) if inside.any() else float('nan'))


def rank_samples(scores, n, largest=True):
    """-> int64 [n]: the indices of the n largest (or smallest) scores, best first, ties to the lowest index (a stable host
    sort): the rows of a sample sheet"""
    scores = np.asarray(scores, dtype=np.float64)
    if scores.ndim != 1:
        raise ValueError(f"rank_samples: scores {scores.shape}, expected [N]")
    if not 0 <= n <= len(scores):
        raise ValueError(f"rank_samples: n = {n} of {len(scores)} scores")
    if np.isnan(scores).any():
        raise ValueError("rank_samples: NaN among the scores")
    return np.argsort(-scores if largest else scores, kind='stable')[:n].astype(np.int64)
