"""NumPy float64 restatement of the per-sample realism and rarity scores for the tests (imports nothing from the product, no
torch).  Squared distances, radii and the derived bound on a squared distance are prd_ref's; on top of them

    ratio2_i = max over the unpruned j of radii2[j] / d2_ij      +inf where d2_ij == 0 (also for 0 / 0), -inf when all are pruned
    rare2_i  = min over the unpruned j with d2_ij <= radii2[j] of radii2[j]      (inclusive) +inf when no ball holds row i
    pruned   = radii2[j] < 0; `prune_radii` keeps the ceil(n (1 - prune)) smallest radii, ties to the lowest index (stable argsort)
    realism  = sqrt(ratio2), rarity = sqrt(rare2) where finite and 0.0 elsewhere, inside = isfinite(rare2)

and the cases the CPU and GPU tests share, each computed once and read-only."""
import functools
import math
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prd_ref  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gan_lib_tensorflow_amd", "csrc")


def tile_width():
    """the column tile of csrc/prd.hip (kPrdTile, resolved through f64_tile.h when it is a name)"""
    def constant(path, name):
        with open(os.path.join(CSRC, path)) as f:
            return re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*(\w+)\s*;", f.read()).group(1)
    value = constant("prd.hip", "kPrdTile")
    return int(value) if value.isdigit() else int(constant("f64_tile.h", value))


def prune_radii(radii2, prune):
    """a copy of radii2 in which all but the ceil(n (1 - prune)) smallest (ties to the lowest index) are -1"""
    radii2 = np.array(radii2, dtype=np.float64)
    keep = math.ceil(len(radii2) * (1.0 - prune))
    radii2[np.argsort(radii2, kind='stable')[keep:]] = -1.0
    return radii2


def scores2(q, r, radii2):
    """-> (ratio2 float64 [nq], rare2 float64 [nq]) of the module docstring"""
    d = prd_ref.d2(q, r)
    radii2 = np.asarray(radii2, np.float64)
    live = np.broadcast_to(radii2[None, :] >= 0, d.shape)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(d == 0, np.inf, radii2[None, :] / d)
    ratio2 = np.where(live, ratio, -np.inf).max(axis=1)
    rare2 = np.where(live & (d <= radii2[None, :]), radii2[None, :], np.inf).min(axis=1)
    return ratio2, rare2


def realism(real, fake, k, prune=0.5):
    return np.sqrt(scores2(fake, real, prune_radii(prd_ref.radii(real, k), prune))[0])


def rarity(real, fake, k):
    """-> (score, inside)"""
    rare2 = scores2(fake, real, prd_ref.radii(real, k))[1]
    inside = np.isfinite(rare2)
    return np.sqrt(np.where(inside, rare2, 0.0)), inside


def sample_scores(real, fake, k, prune=0.5):
    """the dict of common/sample_scores.calculate_sample_scores"""
    real_, (rare, inside) = realism(real, fake, k, prune), rarity(real, fake, k)
    return dict(realism=real_, rarity=rare, inside=inside, mean_realism=float(real_.mean()),
                realistic_fraction=float(np.mean(real_ >= 1.0)), mean_rarity=float(rare[inside].mean()) if inside.any() else float('nan'))


def undecided_rows(q, r, radii2):
    """bool [nq]: the rows with an unpruned j whose test d2_ij <= radii2[j] a permitted error of d2 could turn (the margin
    |d2_ij - radii2[j]| is within prd_ref.d2_bound; radii2 is the same array on both sides and carries no error)"""
    radii2 = np.asarray(radii2, np.float64)
    close = np.abs(prd_ref.d2(q, r) - radii2[None, :]) <= prd_ref.d2_bound(q, r)
    return (close & (radii2[None, :] >= 0)).any(axis=1)


def _freeze(out):
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


EXACT_D, EXACT_NQ, EXACT_K = (16, 48), (1, 63, 65), (1, 3)


def exact_nr():
    """one row short of a column tile, one row more than two column tiles"""
    return (tile_width() - 1, 2 * tile_width() + 1)


def exact_cases():
    return [(d, nq, nr, k) for d in EXACT_D for nq in EXACT_NQ for nr in exact_nr() for k in EXACT_K]


@functools.lru_cache(maxsize=None)
def exact_case(d, nq, nr, k):
    """Integer features in -3..3 as float32: every d2 and radii2 is an integer (at most 36 D), exact in float64 in any order, and
    a ratio is one correctly rounded division.  Bank rows 5 and nr - 1 (in the last column tile) are copies of row 2: radius 0 at
    k = 1.  Query 0 is a copy of bank row 2 (d2 == 0, at k = 1 against radius 0); with more than 8 queries, query 7 is a copy of
    the bank row of largest radius, which prune = 0.5 drops: its nearest row is in the pruned half.
    -> q, r float32; radii2 (all balls), pruned2 (prune = 0.5); ratio2 / rare2 against radii2, ratio2_pruned / rare2_pruned
    against pruned2; realism (prune = 0.5), realism_all (prune = 0), rarity, inside."""
    rng = np.random.RandomState(1000 * d + 10 * nr + nq + k)
    r, q = rng.randint(-3, 4, (nr, d)), rng.randint(-3, 4, (nq, d))
    r[5] = r[nr - 1] = r[2]
    q[0] = r[2]
    radii2 = prd_ref.integer_radii(r, k).astype(np.float64)
    if nq > 8:
        q[7] = r[int(np.argmax(radii2))]
    q, r = q.astype(np.float32), r.astype(np.float32)
    pruned2 = prune_radii(radii2, 0.5)
    out = dict(q=q, r=r, radii2=radii2, pruned2=pruned2)
    out['ratio2'], out['rare2'] = scores2(q, r, radii2)
    out['ratio2_pruned'], out['rare2_pruned'] = scores2(q, r, pruned2)
    out['realism'], out['realism_all'] = np.sqrt(out['ratio2_pruned']), np.sqrt(out['ratio2'])
    out['inside'] = np.isfinite(out['rare2'])
    out['rarity'] = np.sqrt(np.where(out['inside'], out['rare2'], 0.0))
    return _freeze(out)


GAUSS = dict(d=2048, nq=130, nr=200, k=3, seed=11)


@functools.lru_cache(maxsize=None)
def gaussian_case():
    """independent standard normal features, float32 -> q, r, radii2 = prd_ref.radii(r, k), pruned2 (prune = 0.5) and the
    restatement's ratio2 / rare2 against both"""
    rng = np.random.RandomState(GAUSS['seed'])
    r = rng.normal(size=(GAUSS['nr'], GAUSS['d'])).astype(np.float32)
    q = rng.normal(size=(GAUSS['nq'], GAUSS['d'])).astype(np.float32)
    radii2 = prd_ref.radii(r, GAUSS['k'])
    out = dict(q=q, r=r, radii2=radii2, pruned2=prune_radii(radii2, 0.5))
    out['ratio2'], out['rare2'] = scores2(q, r, radii2)
    out['ratio2_pruned'], out['rare2_pruned'] = scores2(q, r, out['pruned2'])
    return _freeze(out)


def ratio_rel_bound(d):
    """The bound on |ratio2 - ratio2_ref| / ratio2_ref where both sides divide the SAME radii2 and every pair has
    A_ij <= 2 d2_ij (A_ij = sum_k (|a_ik| + |b_jk|)^2; the tests assert it on the reference).  A pair's d2 differs from the
    reference's by at most B_ij = 2 (D + 4) 2^-53 A_ij (prd_ref), so r / d2 moves by the relative B_ij / (d2_ij - B_ij) <=
    4 (D + 4) 2^-53 (1 + 1e-9); each side's division rounds once more (2^-53 each, 2 with the cross terms to spare); and the
    maximum over j of values that each moved by at most a relative e moves by at most e.  -> (4 (D + 4) + 4) 2^-53, that is
    4 D 2^-53 and a little."""
    return (4 * (d + 4) + 4) * 2.0 ** -53
