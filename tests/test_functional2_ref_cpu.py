"""tests/functional2_ref.py (the float64 restatements the GPU tests of functional2 compare against) pinned to facts that do
not depend on it: every (forward, gradient) pair is an adjoint pair to 1e-12, and the closed forms of the second-order
batch norm that csrc/acgan_ops.hip implements equal float64 autograd of the first backward to 1e-9.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import functional2_ref as R  # noqa: E402

F64 = torch.float64


def rnd(rng, *shape):
    return torch.tensor(rng.normal(size=shape), dtype=F64)


def dot(a, b):
    return float((a * b).detach().sum())


def close(a, b, tol):
    return abs(a - b) <= tol * max(abs(a), abs(b), 1.0)


@pytest.mark.parametrize("k,cin,cout,h,w,n", [(3, 3, 16, 8, 8, 2), (1, 8, 5, 4, 8, 3), (3, 7, 3, 4, 6, 1)])
def test_conv_adjointness(k, cin, cout, h, w, n):
    rng = np.random.default_rng(k * 100 + cin)
    x, W, dy = rnd(rng, n, h, w, cin), rnd(rng, k, k, cin, cout), rnd(rng, n, h, w, cout)
    a, b, c = dot(R.ConvF(x, W), dy), dot(x, R.ConvD(dy, W)), dot(W, R.ConvW(x, dy, W.shape))
    assert close(a, b, 1e-12) and close(a, c, 1e-12), (a, b, c)
    bias = rnd(rng, cout)
    assert torch.equal(R.ConvF(x, W, bias), R.ConvF(x, W) + bias)


@pytest.mark.parametrize("m,k,c", [(5, 128, 1), (8, 128, 10), (3, 7, 3)])
def test_linear_adjointness(m, k, c):
    rng = np.random.default_rng(m)
    x, W, dy = rnd(rng, m, k), rnd(rng, k, c), rnd(rng, m, c)
    a, b, d = dot(R.LinF(x, W), dy), dot(x, R.LinD(dy, W)), dot(W, R.LinW(x, dy))
    assert close(a, b, 1e-12) and close(a, d, 1e-12), (a, b, d)
    assert torch.allclose(R.LinD(dy, W), dy @ W.t(), rtol=0, atol=1e-12) and torch.allclose(R.LinW(x, dy), x.t() @ dy, rtol=0, atol=1e-12)


@pytest.mark.parametrize("scale", [0.25, 1.0])
def test_pool_adjointness(scale):
    rng = np.random.default_rng(3)
    x, g = rnd(rng, 2, 8, 4, 5), rnd(rng, 2, 4, 2, 5)
    a, b = dot(R.Pool2(x, scale), g), dot(x, R.Unpool2(g, scale))
    assert close(a, b, 1e-12), (a, b)
    # every pixel of a 2x2 block receives scale * g
    assert torch.equal(R.Unpool2(g, scale)[:, 1::2, ::2], g * scale)


@pytest.mark.parametrize("hw", [(1, 1), (8, 8), (4, 8)])
def test_sum_hw_adjointness(hw):
    rng = np.random.default_rng(4)
    x, g = rnd(rng, 3, hw[0], hw[1], 13), rnd(rng, 3, 13)
    scale = 1.0 / (hw[0] * hw[1])
    a, b = dot(R.SumHW(x, scale), g), dot(x, R.BcastHW(g, hw, scale))
    assert close(a, b, 1e-12), (a, b)
    assert torch.allclose(R.SumHW(x, scale), x.mean(dim=(1, 2)), rtol=0, atol=1e-14)


def test_lrelu_backward_is_a_mask():
    rng = np.random.default_rng(5)
    x, dy = rnd(rng, 2, 4, 4, 8), rnd(rng, 2, 4, 4, 8)
    for leak in (0.2, 0.0):
        assert torch.equal(R.LReluB(dy, x, leak), torch.where(x > 0, dy, leak * dy))


def test_helpers_stay_differentiable():
    """every gradient-valued helper can be differentiated again with respect to each of its operands"""
    rng = np.random.default_rng(6)
    x, dy = rnd(rng, 2, 4, 4, 3).requires_grad_(True), rnd(rng, 2, 4, 4, 5).requires_grad_(True)
    W = rnd(rng, 3, 3, 3, 5).requires_grad_(True)
    for out, wrt in ((R.ConvD(dy, W), (dy, W)), (R.ConvW(x, dy, W.shape), (x, dy))):
        assert all(g is not None and float(g.abs().max()) > 0 for g in torch.autograd.grad(out.sum(), wrt))
    x2, dy2, W2 = rnd(rng, 4, 7).requires_grad_(True), rnd(rng, 4, 3).requires_grad_(True), rnd(rng, 7, 3).requires_grad_(True)
    for out, wrt in ((R.LinD(dy2, W2), (dy2, W2)), (R.LinW(x2, dy2), (x2, dy2))):
        assert all(g is not None and float(g.abs().max()) > 0 for g in torch.autograd.grad((out ** 2).sum(), wrt))
    g = rnd(rng, 2, 2, 2, 5).requires_grad_(True)
    assert torch.autograd.grad(R.Unpool2(g, 0.25).sum(), g)[0] is not None
    gg = rnd(rng, 2, 5).requires_grad_(True)
    assert torch.autograd.grad(R.BcastHW(gg, (4, 4), 0.5).sum(), gg)[0] is not None
    gam = rnd(rng, 5).requires_grad_(True)
    dx, dgam, dbeta = R.BNB(dy, dy * 0.5 + 1.0, gam)
    assert dgam.shape == gam.shape and dbeta.shape == gam.shape
    assert all(t is not None for t in torch.autograd.grad((dx ** 2).sum(), (dy, gam)))


@pytest.mark.parametrize("rows,c,means", [(96, 8, (0.0, 0.0)), (257, 16, (1.0, -0.5)), (40, 8, (1.0, -0.5))])
def test_bn_second_order_closed_forms_vs_autograd(rows, c, means):
    """ggO, gI and gG as the comment heading csrc/acgan_ops.hip states them == float64 autograd of BNB's dx, to 1e-9 of the maximum"""
    rng = np.random.default_rng(rows)
    x = rnd(rng, rows, 1, 1, c) * 1.5 + 0.3
    a, dy = rnd(rng, rows, 1, 1, c) * 0.3 + means[0], rnd(rng, rows, 1, 1, c) * 0.3 + means[1]
    gamma = rnd(rng, c) * 0.3 + 1.0
    ref = R.bn_second_order_autograd(a, dy, x, gamma)
    got = R.bn_second_order_closed_forms(a, dy, x, gamma)
    for name, g, r in zip(("gI", "ggO", "gG"), got, ref):
        err = float((g.reshape(r.shape) - r).abs().max() / r.abs().max())
        assert err < 1e-9, (name, err)


def test_bn_first_backward_closed_form():
    """dx = gamma s (dy - mean(dy) - xh mean(dy xh)), dgamma = sum dy xh, dbeta = sum dy"""
    rng = np.random.default_rng(8)
    x, dy, gamma = rnd(rng, 3, 4, 4, 8) + 0.5, rnd(rng, 3, 4, 4, 8), rnd(rng, 8) * 0.3 + 1.0
    dx, dgamma, dbeta = R.BNB(dy, x, gamma)
    mu = x.mean(dim=(0, 1, 2))
    s = torch.rsqrt(((x - mu) ** 2).mean(dim=(0, 1, 2)) + 1e-5)
    xh = (x - mu) * s
    want = gamma * s * (dy - dy.mean(dim=(0, 1, 2)) - xh * (dy * xh).mean(dim=(0, 1, 2)))
    assert float((dx - want).abs().max()) < 1e-12
    assert float((dgamma - (dy * xh).sum(dim=(0, 1, 2))).abs().max()) < 1e-12 and float((dbeta - dy.sum(dim=(0, 1, 2))).abs().max()) < 1e-12


def test_gp_loss_value():
    g = torch.zeros(2, 2, 1, 2, dtype=F64)
    g[0, 0, 0, 0], g[0, 1, 0, 1] = 3.0, 4.0                   # slopes 5 and 1e-5
    want = 10.0 * ((np.sqrt(25 + 1e-10) - 1) ** 2 + (1e-5 - 1) ** 2) / 2
    assert abs(float(R.GPLoss(g, 10.0)) - want) < 1e-12
