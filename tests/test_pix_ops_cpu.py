"""CPU checks of tests/pix_ops_ref.py: a known answer for every restatement (index ramps and ones), float64 autograd for the three
backward functions, and the accept / reject behaviour of the two bounds on every operand set of tests/test_pix_ops_gpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pix_ops_ref as P  # noqa: E402

F64 = torch.float64


# ------------------------------------------------------------------ known answers
def test_blend_known_answers():
    a, b = np.array([1.0, 2.0, -4.0]), np.array([3.0, -2.0, 4.0])
    for mode, want, s_want in ((0, [1.5, 1.0, -2.0], [1.5, 2.0, 4.0]), (1, [0.75, 1.5, -3.0], [0.75, 1.5, 3.0]), (2, [0.25, 0.5, -1.0], [0.25, 0.5, 1.0])):
        y, S = P.blend(a, b if mode == 0 else None, 0.25, mode)
        assert y.tolist() == want and S.tolist() == s_want
    y, S = P.axpby(a, b, 2.0, -1.0)
    assert y.tolist() == [-1.0, 6.0, -12.0] and S.tolist() == [5.0, 6.0, 12.0]
    y, S = P.axpby(a, None, 0.5)
    assert y.tolist() == [0.5, 1.0, -2.0] and S.tolist() == [0.5, 1.0, 2.0]
    assert float(P.blend(a, b, 0.3, 2)[0][0]) == float(np.float32(0.3))          # alpha is the fp32 value


def test_minibatch_std_known_answers():
    """constant over the batch: s = sqrt(1e-8); x[b] = +-1: every position has variance 1, so s = sqrt(1 + 1e-8)"""
    y, S = P.minibatch_std_fwd(np.ones((3, 2, 2, 5)))
    assert y.shape == (3, 2, 2, 6) and np.all(y[..., :5] == 1.0) and np.allclose(y[..., 5], 1e-4, rtol=1e-12)
    assert np.all(S[..., :5] == 0.0) and np.all(S[..., 5] == y[..., 5])
    x = np.stack([np.ones((2, 2, 3)), -np.ones((2, 2, 3))])
    assert np.allclose(P.minibatch_std_fwd(x)[0][..., 3], np.sqrt(1 + 1e-8), rtol=1e-15)
    # backward on it: ds = sum of dy's last channel = 8, R B = 24, (x - m) / sd = +-1 / sqrt(1 + 1e-8)
    dy = np.ones((2, 2, 2, 4))
    dx, S = P.minibatch_std_bwd(dy, x)
    assert np.allclose(dx[0], 1 + 8 / 24 / np.sqrt(1 + 1e-8), rtol=1e-15) and np.allclose(dx[1], 1 - 8 / 24 / np.sqrt(1 + 1e-8), rtol=1e-15)
    assert np.allclose(S, 1 + 8 / 24 / np.sqrt(1 + 1e-8) * 2, rtol=1e-15)


def test_resize_known_answers():
    ramp = np.arange(16.0).reshape(1, 4, 4, 1)
    y, S = P.resize_bilinear(ramp, (8, 8))
    assert y[0, 0, 1, 0] == 0.5 and y[0, 1, 0, 0] == 2.0 and y[0, 7, 7, 0] == 15.0 and np.array_equal(y, S)     # src = dst / 2, far edge clamped
    y, S = P.resize_bilinear(-ramp, (4, 4))
    assert np.array_equal(y, -ramp) and np.array_equal(S, ramp)                                                # identity; S by magnitude
    y, S = P.resize_bilinear(np.array([1.0, -1.0]).reshape(1, 1, 2, 1), (1, 4))
    assert y.reshape(-1).tolist() == [1.0, 0.0, -1.0, -1.0] and S.reshape(-1).tolist() == [1.0, 1.0, 1.0, 1.0]
    y, S = P.resize_nearest_fwd(ramp, (2, 2))
    assert y.reshape(-1).tolist() == [0.0, 2.0, 8.0, 10.0] and not S.any()                 # the top-left pixel of each 2 x 2 cell
    y, _ = P.resize_nearest_fwd(ramp, (8, 8))
    assert np.array_equal(y[0, :, :, 0], np.repeat(np.repeat(ramp[0, :, :, 0], 2, 0), 2, 1))
    dx, S = P.resize_nearest_bwd(-np.ones((1, 8, 8, 1)), (1, 4, 4, 1))
    assert np.all(dx == -4.0) and np.all(S == 4.0)
    dx, S = P.resize_nearest_bwd(np.ones((1, 2, 2, 1)), (1, 4, 4, 1))                      # sources nobody reads get 0
    assert dx[0, :, :, 0].tolist() == [[1, 0, 1, 0], [0, 0, 0, 0], [1, 0, 1, 0], [0, 0, 0, 0]]


def test_concat_split_l1_dropout_known_answers():
    a, b = np.arange(6.0).reshape(3, 2), -np.arange(3.0).reshape(3, 1)
    y, S = P.concat(a, b)
    assert y.tolist() == [[0, 1, 0], [2, 3, -1], [4, 5, -2]] and not S.any()
    a2, b2 = P.split(y, 2)
    assert np.array_equal(a2, a) and np.array_equal(b2, b)
    loss, sum_abs, sign = P.l1(np.array([1.0, 5.0, 2.0, -1.0]), np.array([3.0, 5.0, 1.0, -4.0]))
    assert loss == 1.5 and sum_abs == 1.5 and sign.tolist() == [-1.0, 0.0, 1.0, 1.0]
    dx, S = P.dropout_bwd(np.array([1.0, -2.0, 3.0]), np.array([1, 0, 1], np.uint8), 0.5)
    assert dx.tolist() == [2.0, 0.0, 6.0] and S.tolist() == [2.0, 0.0, 6.0]
    assert P.dropout_bwd(np.array([1.0, -2.0]), np.array([1, 1]), 1.0)[0].tolist() == [1.0, -2.0]
    assert P.l1_chain(1) == 1 + 6 + 4 + 1 + 6 + 4 and P.l1_chain(2 * P.CAP_L1 + 5) == 3 + 6 + 4 + 4 + 6 + 4


def _pool_loops(x, k, stride, pad, out_hw, mode):
    """the definition, one output element at a time"""
    n, h, w, c = x.shape
    out = np.zeros((n, out_hw[0], out_hw[1], c))
    for i in np.ndindex(*out.shape):
        vals = [x[i[0], ih, iw, i[3]] for ih in range(i[1] * stride - pad, i[1] * stride - pad + k) if 0 <= ih < h
                for iw in range(i[2] * stride - pad, i[2] * stride - pad + k) if 0 <= iw < w]
        out[i] = max(vals) if mode == 'max' else sum(vals) / len(vals)
    return out


def test_pool2d_known_answers():
    """ones: SAME average pooling that does not count the padding is 1 everywhere, corners included; a ramp: the 3 x 3 stride-1
    average at a corner is the mean of its 2 x 2 in-image part; every configuration against the element-by-element definition and
    (where torch has the operation) torch's pooling with count_include_pad=False"""
    import torch.nn.functional as F
    ones = np.ones((1, 5, 5, 8))
    for k, s, p in P.POOL_CONFIGS:
        out_hw = (P.pool_out(5, k, s, p),) * 2
        for mode in ('max', 'avg'):
            y, S = P.pool2d(ones, k, s, p, out_hw, mode)
            assert np.all(y == 1.0) and np.all(S == (1.0 if mode == 'avg' else 0.0)), (k, s, p, mode)
    ramp = np.tile(np.arange(16.0).reshape(1, 4, 4, 1), (1, 1, 1, 8))
    y, S = P.pool2d(ramp, 3, 1, 1, (4, 4), 'avg')
    assert y[0, 0, 0, 0] == (0 + 1 + 4 + 5) / 4 and y[0, 0, 3, 0] == (2 + 3 + 6 + 7) / 4 and y[0, 3, 0, 0] == (8 + 9 + 12 + 13) / 4
    assert y[0, 3, 3, 0] == (10 + 11 + 14 + 15) / 4 and y[0, 1, 1, 0] == 5.0 and np.array_equal(y, S)
    assert P.pool2d(ramp, 3, 2, 1, (2, 2), 'max')[0][0, :, :, 0].tolist() == [[5.0, 7.0], [13.0, 15.0]]
    assert P.pool2d(ramp, 8, 1, 0, (1, 1), 'avg')[0][0, 0, 0, 0] == 7.5                  # the window is clipped to the image
    wide = np.full((1, 2, 2, 24), np.nan)
    y, S = P.pool2d(ramp, 2, 2, 0, (2, 2), 'max', out=wide, c_off=16)
    assert np.isnan(y[..., :16]).all() and y[0, :, :, 16].tolist() == [[5.0, 7.0], [13.0, 15.0]] and np.isnan(wide).all() and not S.any()
    for shape in P.POOL_INPUTS:
        x = P.pool_operands(shape)
        xc = torch.tensor(x).permute(0, 3, 1, 2)
        for k, s, p in P.POOL_CONFIGS:
            out_hw = (P.pool_out(shape[1], k, s, p), P.pool_out(shape[2], k, s, p))
            for mode in ('max', 'avg'):
                y, _ = P.pool2d(x, k, s, p, out_hw, mode)
                assert np.allclose(y, _pool_loops(x, k, s, p, out_hw, mode), rtol=1e-14, atol=1e-14), (shape, k, s, p, mode)
            if k <= min(shape[1], shape[2]) and 2 * p <= k and (shape[1] + 2 * p - k) % s == 0 and (shape[2] + 2 * p - k) % s == 0:
                assert np.allclose(P.pool2d(x, k, s, p, out_hw, 'avg')[0], F.avg_pool2d(xc, k, s, p, count_include_pad=False).permute(0, 2, 3, 1).numpy())
                assert np.array_equal(P.pool2d(x, k, s, p, out_hw, 'max')[0], F.max_pool2d(xc, k, s, p).permute(0, 2, 3, 1).numpy())


def test_relu_to_channels_known_answers():
    x = P.relu_operands((1, 1, 2, 8))
    y, S = P.relu_to_channels(x)
    assert y.reshape(-1)[:8].tolist() == [0.0, 0.0, 0.0, 3.3895313892515355e38, 0.0, 1.0, 0.0, 0.0] and not S.any()
    wide = np.full((1, 1, 2, 24), np.nan)
    y, _ = P.relu_to_channels(x, wide, 8)
    assert np.isnan(y[..., :8]).all() and np.isnan(y[..., 16:]).all() and np.array_equal(y[..., 8:16], np.maximum(x, 0))


def test_norm_known_answers():
    """pixel norm of ones is ones / sqrt(1 + eps), of a zero pixel 0 with dx = dy / sqrt(eps); layer norm of a +-1 pattern with
    gamma 2, beta 3 is 3 +- 2"""
    y, S = P.pixel_norm_fwd(np.ones((1, 2, 2, 8)))
    assert np.allclose(y, 1 / np.sqrt(1 + 1e-8), rtol=1e-15) and np.array_equal(S, y)
    dx, S = P.pixel_norm_bwd(np.ones((1, 1, 1, 8)), np.zeros((1, 1, 1, 8)))
    assert np.allclose(dx, 1e4, rtol=1e-12) and np.allclose(S, 1e4, rtol=1e-12)
    dx, S = P.pixel_norm_bwd(np.ones((1, 1, 1, 8)), np.ones((1, 1, 1, 8)))         # dy parallel to x: nothing but eps survives
    assert np.all(np.abs(dx) < 2e-8) and np.allclose(S, 2.0, rtol=1e-7)
    x = np.tile(np.array([1.0, -1.0]), 8).reshape(1, 1, 2, 8)
    y, S, cache = P.layer_norm_fwd(x, np.full(8, 2.0), np.full(8, 3.0))
    assert np.allclose(y, 3 + 2 * x, rtol=1e-11) and np.allclose(S, (1 + 1) * 2 + 3, rtol=1e-11)
    dx, Sdx, dg, dg_abs, db, db_abs = P.layer_norm_bwd(np.ones_like(x), x, np.full(8, 2.0), cache)
    assert np.all(np.abs(dx) < 1e-10) and np.allclose(Sdx, 2.0 + 2.0 + 2.0, rtol=1e-11)      # a constant gradient is projected out
    assert np.allclose(dg, [2, -2] * 4, rtol=1e-11) and np.allclose(dg_abs, 4.0, rtol=1e-11) and db.tolist() == [2.0] * 8 and db_abs.tolist() == [2.0] * 8
    assert P.layer_norm_param_chain(2, 256, 2) == 260


# ------------------------------------------------------------------ the three backward functions against float64 autograd
def test_minibatch_std_backward_matches_autograd():
    from oracle import ref_pggan as RG
    for shape in P.MBSTD_SHAPES[1:4]:
        x, dy = P.mbstd_operands(shape)
        xt = torch.tensor(x, requires_grad=True)
        RG.minibatch_std(xt).backward(torch.tensor(dy))
        dx, S = P.minibatch_std_bwd(dy, x)
        assert np.allclose(dx, xt.grad.numpy(), rtol=1e-10, atol=1e-12), shape
        assert np.all(S >= np.abs(dx) * (1 - 1e-12))


def test_pixel_norm_backward_matches_autograd():
    from oracle import ref_pggan as RG
    for c in (8, 512):
        x, dy = P.pixel_norm_operands((3, 4, 4), c)
        xt = torch.tensor(x, requires_grad=True)
        y = RG.pixel_norm(xt)
        y.backward(torch.tensor(dy))
        assert np.allclose(P.pixel_norm_fwd(x)[0], y.detach().numpy(), rtol=1e-12, atol=1e-14)
        dx, S = P.pixel_norm_bwd(dy, x)
        assert np.allclose(dx, xt.grad.numpy(), rtol=1e-9, atol=1e-9 * np.abs(xt.grad.numpy()).max())
        assert np.all(S >= np.abs(dx) * (1 - 1e-12))


def test_layer_norm_backward_matches_autograd():
    for (n, side, c), which in P.LAYER_NORM_RUNS:
        x, dy, gamma, beta = P.layer_norm_operands(n, side, c, which)
        xt, gt, bt = (torch.tensor(v, requires_grad=True) for v in (x, gamma, beta))
        mean = xt.mean(dim=(1, 2, 3), keepdim=True)
        var = ((xt - mean) ** 2).mean(dim=(1, 2, 3), keepdim=True)
        y = (xt - mean) * torch.rsqrt(var + 1e-12) * gt + bt
        y.backward(torch.tensor(dy))
        yr, S, cache = P.layer_norm_fwd(x, gamma, beta)
        dx, Sdx, dg, dg_abs, db, db_abs = P.layer_norm_bwd(dy, x, gamma, cache)
        assert np.allclose(yr, y.detach().numpy(), rtol=1e-9, atol=1e-9)
        scale = np.abs(xt.grad.numpy()).max()
        assert np.allclose(dx, xt.grad.numpy(), rtol=1e-7, atol=1e-9 * scale), (n, side, c, which)
        assert np.allclose(dg, gt.grad.numpy(), rtol=1e-9, atol=1e-9 * np.abs(dg).max()) and np.allclose(db, bt.grad.numpy(), rtol=1e-12)
        assert np.all(S >= np.abs(yr) * (1 - 1e-12)) and np.all(Sdx >= np.abs(dx) * (1 - 1e-9)) and np.all(dg_abs >= np.abs(dg) * (1 - 1e-12))


# ------------------------------------------------------------------ the two bounds on every operand set of the GPU file
def _two_ulps_off(got, ref, bound_scale):
    """`got` with one element moved by two bf16 ulps: the one where the bound, in ulps, is tightest"""
    nz = np.nonzero(ref.reshape(-1))[0]
    if nz.size == 0:
        return None
    ulp = P.bf16_ulp(ref.reshape(-1)[nz])
    j = nz[int(np.argmin(bound_scale.reshape(-1)[nz] / ulp))]
    moved = got.copy().reshape(-1)
    moved[j] += 2 * P.bf16_ulp(ref.reshape(-1)[j])
    return moved.reshape(got.shape)


def test_bounds_accept_the_rounded_reference_and_reject_small_errors():
    """On every operand set of tests/test_pix_ops_gpu.py: the float64 reference rounded to the output's format (bf16, or fp32 for the
    sums) is inside the bound, so the reference alone never fails a test; the same tensor with one element two bf16 ulps off is
    outside; so is the rounded reference against a reference shifted by one element along its last axis."""
    count = {"bf16": 0, "f32": 0}
    for label, kind, ref, S in P.bound_sets():
        ref = np.asarray(ref, np.float64)
        if kind == "bf16":
            got = P.bf16_round(ref)
            check = lambda g, r, S=S: P.within_bf16(g, r, np.broadcast_to(S, r.shape))       # noqa: E731
            scale = 2.0 ** -8 * np.abs(ref) + 2.0 ** -18 * np.broadcast_to(S, ref.shape)
        else:
            got = ref.astype(np.float32).astype(np.float64)
            check = lambda g, r, S=S: P.within_f32_sum(g, r, S[0], S[1])                     # noqa: E731
            scale = np.broadcast_to((S[1] + 8) * 2.0 ** -24 * S[0], ref.shape)
        count[kind] += 1
        ok, idx, ratio = check(got, ref)
        assert ok, ("the rounded reference misses its own bound", label, idx, ratio)
        moved = _two_ulps_off(got, ref, scale)
        if moved is not None:
            ok, idx, ratio = check(moved, ref)
            assert not ok and ratio > 1.0, ("two bf16 ulps pass", label, idx, ratio)
        shifted = np.roll(ref, 1, axis=-1)
        if ref.shape[-1] > 1 and not np.array_equal(shifted, ref):
            ok, idx, ratio = check(got, shifted)
            assert not ok, ("a reference shifted by one element passes", label, idx, ratio)
    assert count["bf16"] > 100 and count["f32"] == 6 + 4 + 5, count          # L1 losses, dgamma, dbeta


def test_bounds_reject_non_finite_and_report_the_worst_element():
    ref, S = np.array([[1.0, 2.0], [4.0, 0.0]]), np.array([[1.0, 2.0], [4.0, 0.0]])
    assert P.within_bf16(ref, ref, S) == (True, (0, 0), 0.0)
    got = ref.copy()
    got[1, 0] += 4.0 * 2.0 ** -7
    ok, idx, ratio = P.within_bf16(got, ref, S)
    assert not ok and idx == (1, 0) and ratio == pytest.approx(2.0 ** -7 / (2.0 ** -8 + 2.0 ** -18))
    got = ref.copy()
    got[0, 1] = np.nan
    assert P.within_bf16(got, ref, S)[:2] == (False, (0, 1))
    got = ref.copy()
    got[1, 1] = 1e-30                                  # a gather (S = 0) of a zero is exact or wrong
    assert P.within_bf16(got, ref, S)[:2] == (False, (1, 1))
    ok, idx, ratio = P.within_f32_sum(np.array([1.0 + 30 * 2.0 ** -24]), np.array([1.0]), np.array([1.0]), 22)
    assert ok and ratio == pytest.approx(1.0)
    assert not P.within_f32_sum(np.array([1.0 + 31 * 2.0 ** -24]), np.array([1.0]), np.array([1.0]), 22)[0]
