"""GPU: the Inception score's statistics kernels (csrc/inception_score.hip) against the float64 restatement
tests/inception_score_ref.py, their order-exactness, and the device path end to end (InceptionScore, get_inception_score_device,
the three trainers' `inception_score(net=...)`).

Bound.  Every state element is a sum of at most N <= 1.3e5 float64 terms of one sign (probabilities, or p log p <= 0), so the
worst case of the summation is N 2^-53 ~ 1.5e-11 relative, whatever the order; a few ulp each for the device's exp and log come
on top.  1e-9 relative on every state element and on every split score."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inception_score_ref as R  # noqa: E402
from test_inception_gpu import random_params  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-9


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    from gan_lib_tensorflow_amd import kernels
    return kernels


@pytest.fixture(scope="module")
def S(K):
    from gan_lib_tensorflow_amd.common.inception import inception_score
    return inception_score


@pytest.fixture(scope="module")
def net(K):
    from gan_lib_tensorflow_amd.common.inception.inception_v3 import InceptionV3
    return InceptionV3(random_params(7))


def make_logits(n, ld, seed):
    """N(0, 3^2) float32 [n, ld]"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, ld, generator=g) * 3.0


def feed(S, logits, splits, chunks):
    """an InceptionScore of len(logits) rows fed in calls of the given sizes -> the object"""
    assert sum(chunks) == len(logits)
    score = S.InceptionScore(len(logits), splits)
    dev, at = logits.cuda(), 0
    for c in chunks:
        score.update(dev[at:at + c])
        at += c
    return score


def worst_relative(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.all(np.isfinite(got)), got
    return float(np.max(np.abs(got - want) / np.abs(want)))


def check_against_restatement(score, logits, splits, what):
    want_state, want_scores = R.state(logits.numpy(), splits), R.scores(logits.numpy(), splits)
    es = worst_relative(score.state.cpu().numpy(), want_state)
    ec = worst_relative(score.scores(), want_scores)
    print(f"{what}: worst relative error of a state element {es:.3e}, of a split score {ec:.3e} (bound {TOL:.0e})")
    assert es <= TOL and ec <= TOL
    mean, std = score.finalize()
    assert abs(mean - np.mean(want_scores)) <= TOL * np.mean(want_scores) and abs(std - np.std(want_scores)) <= TOL * np.mean(want_scores)


CASES = {"7rows_3splits_ld1008": (7, 3, 1008, (3, 3, 1)), "130rows_10splits_ld1000": (130, 10, 1000, (64, 64, 2))}


@pytest.mark.parametrize("case", list(CASES))
def test_kernel_against_the_float64_restatement(S, case):
    n, splits, ld, chunks = CASES[case]
    if n == 7:
        assert S.split_bounds(n, splits) == [0, 2, 4, 7]
    logits = make_logits(n, ld, seed=n)
    check_against_restatement(feed(S, logits, splits, chunks), logits, splits, case)


def test_order_exactness(S):
    """the same rows in one call, in 64 + 64 + 2 and in 130 calls of one row: the same bits; and twice the same run"""
    logits = make_logits(130, 1000, seed=130)
    whole = feed(S, logits, 10, (130,)).state
    assert torch.equal(whole, feed(S, logits, 10, (64, 64, 2)).state)
    assert torch.equal(whole, feed(S, logits, 10, (1,) * 130).state)
    assert torch.equal(whole, feed(S, logits, 10, (130,)).state)
    assert torch.equal(feed(S, logits, 10, (64, 64, 2)).state, feed(S, logits, 10, (64, 64, 2)).state)


def test_range(S):
    """logits shifted by +-85 (float32 exp overflows from 88.7) and a row whose winner is 800 above the rest (every other
    probability underflows to exactly 0): finite, and the restatement's number -- it uses the same log-softmax form"""
    logits = make_logits(7, 1008, seed=7)
    logits[0] += 85.0
    logits[1] -= 85.0
    logits[2] += 85.0
    logits[4] -= 85.0
    logits[5, 123] = logits[5, :1000].max() + 800.0
    with np.errstate(over='ignore'):
        assert not np.all(np.isfinite(np.exp(logits.numpy()[:, :1000])))          # what the host path's float32 exp makes of them
    assert np.count_nonzero(np.exp(R.log_softmax(logits.numpy())[5])) == 1
    score = feed(S, logits, 3, (3, 3, 1))
    assert bool(torch.isfinite(score.state).all())
    check_against_restatement(score, logits, 3, "shifted and one-hot rows")


def test_row_stride(S, K):
    """[b, 1000] values inside a [b, 1008] buffer whose last 8 columns hold 1e30 and nan: bit-identical state, no copy"""
    dense = make_logits(130, 1000, seed=130)
    wide = torch.empty(130, 1008)
    wide[:, :1000] = dense
    wide[:, 1000:1004] = 1e30
    wide[:, 1004:] = float('nan')
    want = feed(S, dense, 10, (64, 64, 2)).state
    assert torch.equal(want, feed(S, wide, 10, (64, 64, 2)).state)
    view = wide.cuda()[:, :1000]                                  # a view: row stride 1008, passed as ld
    assert not view.is_contiguous()
    state = torch.zeros(10, 1001, dtype=torch.float64, device="cuda")
    K.inception_score_update(view, 0, 130, 10, state)
    assert torch.equal(state, feed(S, dense, 10, (130,)).state)


def test_get_inception_score_device(S, net, monkeypatch):
    rng = np.random.default_rng(5)
    images = rng.uniform(-1, 1, size=(20, 32, 32, 3)).astype(np.float32)
    host_logits = net.logits(images[:16])
    assert torch.equal(net.logits_device(images[:16]).cpu(), torch.from_numpy(host_logits))
    fed = []
    update = S.InceptionScore.update

    def counting(self, logits):
        fed.append(logits.shape[0])
        return update(self, logits)
    monkeypatch.setattr(S.InceptionScore, "update", counting)
    mean, std = S.get_inception_score_device(images, net, splits=2, batch_size=8)
    mean_t, std_t = S.get_inception_score_device(torch.from_numpy(images).cuda(), net, splits=2, batch_size=8)
    assert fed == [8, 8, 8, 8]                                    # 16 rows each: whole batches only
    want_mean, want_std = R.score(host_logits, 2)
    print(f"device {mean!r} +- {std!r}, restatement {want_mean!r} +- {want_std!r}")
    assert abs(mean - want_mean) <= TOL * want_mean and abs(std - want_std) <= TOL * want_mean
    assert (mean_t, std_t) == (mean, std)


def test_sngan_device_path_against_the_host_path(S, net, deterministic_stats):
    """The same trainer state, the same draws: `net=` against `classifier=`.  The host path rounds its softmax in float32, so its
    own distance from the float64 restatement on the logits it saw is measured first; the device path must be within 4 x that
    of the host path (a factor of two for each of the two places the paths round differently).
    (On the fixed-order batch-norm statistics, as tests/test_msssim_gpu.py::test_sngan_msssim_diversity: with the conv epilogues'
    float atomics two runs of the generator on the same noise differ in their quantised pixels -- 46 399 of 307 200 between two
    trainers of the same seed, 1.9e-6 of this score, 35 x the host path's own error -- and the two paths are to see the same
    samples.  Measured: host path's own error 1.47e-8, device/host gap 1.47e-8, device against the restatement 1.9e-15.)"""
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
    seen = []

    def classifier(batch):
        seen.append(net.logits(batch))
        return seen[-1]
    host = SNGANTrainer(batch_size=8, seed=0, use_graphs=False).inception_score(n=200, classifier=classifier, splits=2)
    dev = SNGANTrainer(batch_size=8, seed=0, use_graphs=False).inception_score(n=200, net=net, splits=2)
    ref = R.score(np.concatenate(seen, 0), 2)
    assert len(seen) == 2 and all(np.isfinite(host)) and all(np.isfinite(dev))
    host_err = max(abs(host[0] - ref[0]), abs(host[1] - ref[1]))
    gap = max(abs(dev[0] - host[0]), abs(dev[1] - host[1]))
    dev_err = max(abs(dev[0] - ref[0]), abs(dev[1] - ref[1]))
    print(f"host {host!r} device {dev!r} restatement {ref!r}: host path's own error {host_err:.3e}, device/host gap {gap:.3e}, "
          f"device against the restatement {dev_err:.3e}")
    assert gap <= 4 * host_err


def test_sngan_refuses_classifier_and_net_together(net):
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
    tr = SNGANTrainer(batch_size=8, seed=0, use_graphs=False)
    with pytest.raises(ValueError, match="not both"):
        tr.inception_score(n=200, classifier=net.logits, net=net)
    assert tr.maybe_inception_score(net=net) is None                      # not due at iteration 0


@pytest.mark.parametrize("which", ["acgan", "pggan"])
def test_trainer_inception_score(net, which, deterministic_stats):
    """(on the fixed-order batch-norm statistics: the comparison of two trainers of the same seed is for equality, see above)"""
    def trainer():
        if which == "acgan":
            from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
            return ACGANTrainer(batch_size=8, seed=0, use_graphs=False)
        from gan_lib_tensorflow_amd.PGGAN.train import PGGANTrainer, default_args
        return PGGANTrainer(default_args(model='resnet', image_size=8, block_count=1, batch_size=16), seed=0, use_graphs=False)
    tr = trainer()
    first = tr.inception_score(n=200, net=net, splits=2)
    assert len(first) == 2 and all(isinstance(v, float) and np.isfinite(v) for v in first)
    assert 1.0 <= first[0] <= 1000.0
    again = trainer().inception_score(n=200, net=net, splits=2)
    print(f"{which}: {first!r}, a fresh trainer with the same seed {again!r}")
    assert tuple(again) == tuple(first)
    with pytest.raises(NotImplementedError, match="needs downloaded weights"):
        tr.inception_score(n=200)
