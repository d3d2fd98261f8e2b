"""CPU: the float64 restatements of the gradient penalties (tests/grad_penalty_ref.py) on hand-computed cases, the DRAGAN sigma against
np.std, the two new entry points in the header-derived binding, and the penalty arguments of the ACGAN trainer's constructor (checked
before any device work, so no GPU is needed)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_penalty_ref as G  # noqa: E402

F64 = torch.float64


def rows(a):
    return torch.tensor(np.asarray(a, np.float64))


@pytest.mark.parametrize("kind,loss,dg", [
    # one row (1.2, 1.6): norm 2, target 1, lam 10.  s - 1 = 1: 10 * 1^2; d/dg = 2 lam (s - 1) / s * g = 10 g
    ("two_sided", 10.0, [[12.0, 16.0]]),
    ("one_sided", 10.0, [[12.0, 16.0]]),
    # lam * |g|^2 = 40; d/dg = 2 lam g
    ("squared", 40.0, [[24.0, 32.0]]),
])
def test_restatement_row_of_norm_two(kind, loss, dg):
    """(the 1e-10 under the square root moves s by 2.5e-11: 1e-9 absolute covers it; the squared kind has none and is exact)"""
    got_loss, got_dg = G.grad_penalty_and_derivative(rows([[1.2, 1.6]]), 10.0, 1.0, kind)
    tol = 0.0 if kind == "squared" else 1e-9
    assert abs(float(got_loss) - loss) <= tol + 1e-12
    assert float((got_dg - rows(dg)).abs().max()) <= tol + 1e-12


def test_restatement_one_sided_below_the_target_is_exactly_zero():
    """a row of norm 0.5 under target 1: no loss, no derivative; beside a row of norm 2 only that row counts: 10 * (0 + 1) / 2"""
    loss, dg = G.grad_penalty_and_derivative(rows([[0.3, 0.4]]), 10.0, 1.0, "one_sided")
    assert float(loss) == 0.0 and bool((dg == 0).all())
    loss, dg = G.grad_penalty_and_derivative(rows([[0.3, 0.4], [1.2, 1.6]]), 10.0, 1.0, "one_sided")
    assert abs(float(loss) - 5.0) < 1e-9 and bool((dg[0] == 0).all()) and float((dg[1] - rows([6.0, 8.0])).abs().max()) < 1e-9
    # the two-sided kind does penalise it: 10 * (0.5 - 1)^2 = 2.5, d/dg = 2 * 10 * (-0.5) / 0.5 * g = -20 g
    loss, dg = G.grad_penalty_and_derivative(rows([[0.3, 0.4]]), 10.0, 1.0, "two_sided")
    assert abs(float(loss) - 2.5) < 1e-8 and float((dg - rows([[-6.0, -8.0]])).abs().max()) < 1e-7
    # ... and target 0.5 puts the row on the target: (sqrt(0.25 + 1e-10) - 0.5)^2 = 1e-20
    loss, _ = G.grad_penalty_and_derivative(rows([[0.3, 0.4]]), 10.0, 0.5, "two_sided")
    assert 0.0 <= float(loss) < 1e-18


def test_restatement_squared_zero_row_is_exactly_zero():
    """R1 takes no square root: value and derivative of an all-zero row are 0, not 0/0; the two-sided kind has a finite value there
    (10 * (1e-5 - 1)^2) and derivative 0"""
    loss, dg = G.grad_penalty_and_derivative(torch.zeros((1, 5), dtype=F64), 10.0, 1.0, "squared")
    assert float(loss) == 0.0 and bool((dg == 0).all()) and bool(torch.isfinite(dg).all())
    loss, dg = G.grad_penalty_and_derivative(rows([[0.0, 0.0], [3.0, 4.0]]), 0.5, 1.0, "squared")
    assert float(loss) == 0.5 * 25.0 / 2 and bool((dg[0] == 0).all()) and torch.equal(dg[1], rows([1.5, 2.0]))
    loss, dg = G.grad_penalty_and_derivative(torch.zeros((1, 5), dtype=F64), 10.0, 1.0, "two_sided")
    assert abs(float(loss) - 10.0 * (1e-5 - 1.0) ** 2) < 1e-12 and bool((dg == 0).all())


def test_restatement_two_sided_target_one_is_gploss():
    import functional2_ref as R
    g = torch.tensor(np.random.default_rng(0).normal(size=(5, 4, 3, 2)))
    assert float(G.GradPenalty(g, 10.0)) == float(R.GPLoss(g, 10.0))


def test_dragan_sigma_is_the_population_standard_deviation():
    x = np.random.default_rng(1).normal(size=(8, 32, 32, 3)) * 0.5 + 0.25
    sigma = float(G.dragan_sigma(torch.tensor(x)))
    assert abs(sigma - np.std(x)) < 1e-12 and abs(sigma - np.std(x, ddof=1)) > 1e-7      # ddof 0, and the test can tell
    u = np.random.default_rng(2).uniform(size=x.shape)
    out = G.dragan_perturb(torch.tensor(x), torch.tensor(u).reshape(-1))
    assert float((out - torch.tensor(x + 0.5 * np.std(x) * u)).abs().max()) < 1e-12
    assert float(G.dragan_sigma(torch.full((7, 3), 0.7, dtype=F64))) == 0.0


def test_the_binding_picks_up_the_two_entry_points():
    """nothing names them outside gank.h, csrc/ and kernels.py: the header-derived binding types them and the library exports them"""
    from gan_lib_tensorflow_amd import _lib, build
    import test_abi
    assert {"gank_grad_penalty", "gank_dragan_perturb"} <= set(test_abi.header_symbols())
    P, I = C.c_void_p, C.c_int
    assert _lib.PROTOTYPES["gank_grad_penalty"] == [P, P, P, P, I, C.c_long, C.c_float, C.c_float, I, P]
    assert _lib.PROTOTYPES["gank_dragan_perturb"] == [P, P, P, P, C.c_long, P]
    assert _lib.RESTYPES["gank_grad_penalty"] is I and _lib.RESTYPES["gank_dragan_perturb"] is I
    build.build(verbose=False)
    lib = _lib.load()
    fake = P(0x1000)      # never dereferenced: every call below is refused by argument checks, before any launch
    assert lib.gank_grad_penalty(fake, fake, fake, fake, 4, 16, 10.0, 1.0, 3, None) != 0 and "kind 3" in lib.gank_last_error().decode()
    assert lib.gank_grad_penalty(fake, fake, None, fake, 4, 16, 10.0, 1.0, 0, None) != 0 and "bad arguments" in lib.gank_last_error().decode()
    assert lib.gank_dragan_perturb(fake, fake, fake, fake, 0, None) != 0 and "bad arguments" in lib.gank_last_error().decode()
    assert lib.gank_dragan_perturb(fake, P(0x1004), fake, fake, 64, None) != 0 and "16-byte aligned" in lib.gank_last_error().decode()


@pytest.mark.parametrize("kw", [dict(penalty="wgan"), dict(penalty="R1"), dict(penalty=None), dict(penalty_every=0), dict(penalty_every=-2),
                                dict(penalty_every=1.5), dict(penalty_weight=0.0), dict(penalty_weight=-1.0),
                                dict(penalty="r1", penalty_weight=0.0), dict(penalty="none", penalty_every=0),
                                dict(penalty_every=None), dict(penalty_every="2"), dict(penalty_weight=None), dict(penalty_weight="10"),
                                dict(penalty_every=True)])
def test_trainer_refuses_bad_penalty_arguments(kw):
    from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
    with pytest.raises(ValueError, match="penalty"):
        ACGANTrainer(batch_size=8, **kw)


def test_trainer_penalty_table_and_names():
    from gan_lib_tensorflow_amd import kernels as K
    from gan_lib_tensorflow_amd.ACGAN import train
    assert train.PENALTIES == G.PENALTIES and list(train.PENALTIES) == ["wgan-gp", "wgan-lp", "dragan", "r1", "r2", "none"]
    assert K.GRAD_PENALTY_KINDS == {"two_sided": 0, "one_sided": 1, "squared": 2} and tuple(K.GRAD_PENALTY_KINDS) == G.KINDS
    train.check_penalty("none", 0.0, 1)               # a weight is only asked of a penalty that is switched on
    train.check_penalty("r1", 5.0, 16)
    train.check_penalty("r1", np.float32(5.0), np.int64(16))      # NumPy scalars are numbers too
    train.check_penalty("none", None, 2.0)
    with pytest.raises(ValueError, match="kind"):
        K.grad_penalty(torch.zeros((2, 8), dtype=torch.bfloat16), 10.0, 1.0, "both_sided")
