"""The small operators of the PGGAN, Pix2Pix and Inception-score paths (csrc/pggan_pix_ops.hip from axpby down to relu_to_channels,
the layer- and pixel-norm kernels of csrc/norms.hip) through kernels.py / functional.py on a real MI355X, each against the float64
restatement of tests/pix_ops_ref.py on shared bf16-rounded operands: at one element, at a ragged tail, past the grid cap of every
grid-stride loop (2 x cap + an odd remainder, the output filled with NaN first wherever the wrapper takes `out`), on every dispatch
arm and at every rejection.

Bounds (pix_ops_ref.py, checked on these operand sets by tests/test_pix_ops_cpu.py): bf16 outputs per element
|got - ref| <= 2^-8 |ref| + 2^-18 S, S the sum of the magnitudes of the terms of that element; fp32 sums
|got - ref| <= (chain + 8) 2^-24 sum_abs; operators that only move data (concat, split, nearest forward, relu_to_channels, max
pool, the copied channels of minibatch-std) bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pix_ops_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
NAN_BITS = 0x7FA5           # a NaN with a payload: an untouched element keeps exactly these bits


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gan_lib_tensorflow_amd import kernels
    kernels.lib()
    assert kernels.BF16 is torch.bfloat16
    return kernels


def bf(a):
    """-> (bf16-rounded float64 CPU tensor, bf16 cuda tensor)"""
    t = torch.as_tensor(np.asarray(a, np.float32)).to(torch.bfloat16)
    return t.to(F64), t.cuda().contiguous()


def f32(a):
    t = torch.as_tensor(np.asarray(a, np.float32))
    return t.to(F64), t.cuda().contiguous()


def host(t):
    return t.detach().to(F64).cpu().numpy()


def nan_fill(shape):
    return torch.full(tuple(shape), NAN_BITS, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def untouched(t):
    return bool((t.contiguous().view(torch.int16) == NAN_BITS).all())


def check_bf16(what, got, ref, S):
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == tuple(np.shape(ref)), (what, got.dtype, got.shape, np.shape(ref))
    ok, idx, ratio = P.within_bf16(host(got), ref, S)
    print(what, "worst |got - ref| / bound %.3f at %s" % (ratio, idx))
    assert ok, (what, idx, ratio)


def check_f32(what, got, ref, sum_abs, chain):
    assert got.dtype == torch.float32
    ok, idx, ratio = P.within_f32_sum(host(got), ref, sum_abs, chain)
    print(what, "chain", chain, "worst |got - ref| / bound %.3f at %s" % (ratio, idx))
    assert ok, (what, idx, ratio)


def check_equal(what, got, ref):
    """bit for bit: the values of a bf16 output against float64 (every operand is a bf16 value; -0.0 == +0.0)"""
    assert got.dtype == torch.bfloat16 and tuple(got.shape) == tuple(np.shape(ref)), (what, got.shape, np.shape(ref))
    g = host(got)
    assert np.array_equal(g, ref), (what, int((g != ref).sum()), "elements differ, the first at", tuple(np.argwhere(g != ref)[0]))


# ------------------------------------------------------------------ axpby / blend_dev
@pytest.mark.parametrize("n", P.BLEND_SIZES)
def test_axpby_and_blend_dev(K, n):
    """n = 1; 257 (two blocks, the second with one live thread); 2 x 4096 x 256 + 77 (every thread strides twice, 77 three times).
    axpby with and without b; blend_dev in its three modes at alpha 0, 1 and 0.3, alpha rewritten in the SAME device tensor between
    the calls (what a replayed graph sees)."""
    a, b, g = P.blend_operands(n)
    at, bt, gt = bf(a)[1], bf(b)[1], bf(g)[1]
    check_bf16("axpby b=None", K.axpby(at, None, 0.7), *P.axpby(a, None, 0.7))
    alpha = torch.full((1,), 0.5, dtype=torch.float32, device="cuda")
    for al in P.BLEND_ALPHAS:
        check_bf16("axpby %g" % al, K.axpby(at, bt, 1.0 - al, al), *P.axpby(a, b, 1.0 - al, al))
        alpha.fill_(al)
        for mode in (0, 1, 2):
            src, srct = (a, at) if mode == 0 else (g, gt)
            check_bf16("blend_dev alpha %g mode %d" % (al, mode), K.blend_dev(srct, bt if mode == 0 else None, alpha, mode), *P.blend(src, b, al, mode))
    alpha.fill_(0.0)
    y0 = K.blend_dev(at, bt, alpha, 0)
    alpha.fill_(1.0)
    y1 = K.blend_dev(at, bt, alpha, 0)
    check_equal("alpha 0 -> a", y0, a)
    check_equal("the same tensor rewritten to 1 -> b", y1, b)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_blend_function_value_and_both_gradients(K, kind):
    from gan_lib_tensorflow_amd import functional as Fn
    a, b, g = (v.reshape(1, 1, 257, 1) for v in P.blend_operands(257))
    at, bt, gt = bf(a)[1].requires_grad_(True), bf(b)[1].requires_grad_(True), bf(g)[1]
    alpha = 0.3 if kind == "host" else torch.full((1,), 0.3, dtype=torch.float32, device="cuda")
    y = Fn.blend(at, bt, alpha)
    y.backward(gt)
    if kind == "host":          # the wrapper passes fp32(1 - 0.3) and fp32(0.3)
        check_bf16("blend", y, *P.axpby(a, b, 1.0 - 0.3, 0.3))
        check_bf16("d/da", at.grad, *P.axpby(g, None, 1.0 - 0.3))
        check_bf16("d/db", bt.grad, *P.axpby(g, None, 0.3))
    else:
        check_bf16("blend", y, *P.blend(a, b, 0.3, 0))
        check_bf16("d/da", at.grad, *P.blend(g, None, 0.3, 1))
        check_bf16("d/db", bt.grad, *P.blend(g, None, 0.3, 2))


# ------------------------------------------------------------------ minibatch std
@pytest.mark.parametrize("shape", P.MBSTD_SHAPES)
def test_minibatch_std_value_and_gradient(K, shape):
    """(1,1,1,1): zero variance, s = sqrt(1e-8) = 1e-4 and dx = dy; (2,1,1,3); (5,4,4,24); (8,4,4,512) the workload's shape;
    (4,64,64,64): the concat passes its cap (1,064,960 outputs) and the one block of the mean averages 262,144 positions.
    The copied channels bit for bit, the statistic s (channel C) and the gradient within the bf16 bound."""
    from gan_lib_tensorflow_amd import functional as Fn
    x, dy = P.mbstd_operands(shape)
    c = shape[3]
    xt, dyt = bf(x)[1].requires_grad_(True), bf(dy)[1]
    out = Fn.minibatch_std(xt)
    y_ref, S = P.minibatch_std_fwd(x)
    assert tuple(out.shape) == y_ref.shape
    check_equal("copied channels", out[..., :c], x)
    check_bf16("s", out[..., c], y_ref[..., c], S[..., c])
    if shape == (1, 1, 1, 1):
        assert float(out.detach()[0, 0, 0, 1]) == float(torch.tensor(1e-4).to(torch.bfloat16))
    out.backward(dyt)
    check_bf16("dx", xt.grad, *P.minibatch_std_bwd(dy, x))


# ------------------------------------------------------------------ resize_bilinear
@pytest.mark.parametrize("shape,out_hw", P.BILINEAR_CASES)
def test_resize_bilinear(K, shape, out_hw):
    """one pixel; odd non-square down and up at once; 8 channels; 32 -> 299, the Inception harness's ratio; the identity, bit
    equal; 837 x 839 x 3 outputs, past the cap.  S is the sum of the four weighted magnitudes.

    The restatement computes the source coordinate dst * in / out in float64, the kernel in fp32, so at a coordinate that is an
    integer up to rounding the two may pick different cells.  Bilinear interpolation is continuous across a cell boundary (at
    weight 1 of one cell and weight 0 of the next both give the shared sample), so the bound holds whichever cell the kernel
    takes; no case here has such a coordinate other than the exact ones (0, and the power-of-two ratios)."""
    x = P.bilinear_operands(shape)
    y = K.resize_bilinear(bf(x)[1], out_hw)
    check_bf16("resize_bilinear", y, *P.resize_bilinear(x, out_hw))
    if tuple(out_hw) == shape[1:3]:
        check_equal("identity", y, x)


# ------------------------------------------------------------------ resize_nearest past its 2048-block cap
@pytest.mark.parametrize("shape,out_hw", P.NEAREST_CAP_CASES)
def test_resize_nearest_past_the_cap(K, shape, out_hw):
    """what RESIZE_CASES of tests/test_pggan_resnet_gpu.py lacks: more than 2 x 2048 x 256 threads forward (one per output, or per
    8 channels of it) and backward (one per source), on the 16-byte arm (C = 8) and on the element arm (C = 3)"""
    from gan_lib_tensorflow_amd import functional as Fn
    x, dy = P.nearest_operands(shape, out_hw)
    xt = bf(x)[1].requires_grad_(True)
    y = Fn.resize_nearest(xt, out_hw)
    check_equal("forward", y, P.resize_nearest_fwd(x, out_hw)[0])
    y.backward(bf(dy)[1])
    check_bf16("backward", xt.grad, *P.resize_nearest_bwd(dy, shape))


# ------------------------------------------------------------------ concat / split
@pytest.mark.parametrize("pixels,ca,cb", P.CONCAT_CASES)
def test_concat_split(K, pixels, ca, cb):
    """(8,8) and (64,24): 16 bytes per lane; (13,3), (1,7), (513,63): the element arm; 400,003 x (16,8) and 299,595 x (4,3): past the
    cap on either arm.  Forward and Fn.concat_channels' backward (the split) bit for bit; gank_split_channels with either output
    null writes the other one alone."""
    from gan_lib_tensorflow_amd import _lib, functional as Fn
    a, b, g = P.concat_operands(pixels, ca, cb)
    at, bt, gt = bf(a)[1].requires_grad_(True), bf(b)[1].requires_grad_(True), bf(g)[1]
    y = Fn.concat_channels(at, bt)
    check_equal("concat", y, P.concat(a, b)[0])
    y.backward(gt)
    ga, gb = P.split(g, ca)
    check_equal("d/da", at.grad, ga)
    check_equal("d/db", bt.grad, gb)
    for null in ("a", "b"):
        bufa, bufb = nan_fill((pixels + 1, ca)), nan_fill((pixels + 1, cb))            # one guard row behind each
        _lib.check(K.lib().gank_split_channels(K._p(gt), None if null == "a" else K._p(bufa), None if null == "b" else K._p(bufb),
                                               pixels, ca, cb, K._stream()), "split_channels")
        torch.cuda.synchronize()
        kept, want, other = (bufb, gb, bufa) if null == "a" else (bufa, ga, bufb)
        check_equal("split with %s null" % null, kept[:pixels], want)
        assert untouched(kept[pixels:]) and untouched(other), null


# ------------------------------------------------------------------ L1
@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("n", P.L1_SIZES)
def test_l1_loss_and_gradient(K, n, tied):
    """n = 1, 255 and 2 x 1024 x 256 + 5 (three grid-stride iterations, all 1024 partials); `tied`: a == b on every tenth element,
    whose gradient is exactly 0.  The loss within the fp32 sum bound, dl32 exactly +-fl32(1 / n) or 0, and Fn.l1_loss' gradient
    under an upstream scale of 100."""
    from gan_lib_tensorflow_amd import functional as Fn
    a, b = P.l1_operands(n, tied)
    at, bt = bf(a)[1].requires_grad_(True), bf(b)[1]
    loss_ref, sum_abs, sign = P.l1(a, b)
    loss, dl32 = K.l1_loss(at.detach(), bt)
    # chain: ceil(n / threads) iterations per thread + 6 shuffles + 4 waves per block, then the second launch over the block
    # partials: ceil(blocks / 256) iterations + 6 shuffles + 4 waves  (n = 524,293: 3 + 6 + 4 + 4 + 6 + 4 = 27; n <= 255: 22)
    chain = P.l1_chain(n)
    assert chain == {1: 22, 255: 22, 2 * P.CAP_L1 + 5: 27}[n]
    check_f32("l1 loss", loss, np.array([loss_ref]), np.array([sum_abs]), chain)
    inv = float(np.float32(1) / np.float32(n))
    got = host(dl32)
    assert np.array_equal(got, sign * inv), int((got != sign * inv).sum())
    if tied:
        assert np.all(got[::10] == 0.0)
    out = Fn.l1_loss(at, bt)
    out.backward(torch.full((1,), 100.0, dtype=torch.float32, device="cuda"))
    check_bf16("100 x gradient", at.grad, 100.0 * inv * sign, np.abs(100.0 * inv * sign))


# ------------------------------------------------------------------ dropout backward
@pytest.mark.parametrize("n,keep", P.DROPOUT_CASES)
def test_dropout_backward_on_the_forward_mask(K, n, keep):
    """dx = dy / keep where the forward's mask kept the element, 0 elsewhere: one element and past the cap, keep 0.5 and 1.0 (the
    forward's mask and values are pinned by tests/test_rng_gpu.py)"""
    dy = P.dropout_operands(n)
    dyt = bf(dy)[1]
    rs = K.new_rng_state(11, "cuda")
    _, mask = K.dropout_fwd(dyt, keep, rs)
    dx = K.dropout_bwd(dyt, mask, keep)
    m = mask.cpu().numpy()
    assert m.shape == dy.shape and (keep < 1.0 or m.all())
    check_bf16("dropout_bwd", dx, *P.dropout_bwd(dy, m, keep))


# ------------------------------------------------------------------ pool2d
def _pool_check(K, x, xt, k, s, p, out_hw, mode, cy, c_off):
    c = x.shape[-1]
    out = nan_fill((x.shape[0],) + tuple(out_hw) + (cy,))
    got = K.pool2d(xt, k, s, p, out_hw, mode, out=out, c_off=c_off)
    assert got is out
    ref, S = P.pool2d(x, k, s, p, out_hw, mode)
    what = "pool2d %s k%d s%d p%d %s -> [%d:%d] of %d" % (mode, k, s, p, x.shape, c_off, c_off + c, cy)
    if mode == 'max':
        check_equal(what, out[..., c_off:c_off + c], ref)
    else:
        check_bf16(what, out[..., c_off:c_off + c].contiguous(), ref, S)
    assert untouched(out[..., :c_off]) and untouched(out[..., c_off + c:]), what


@pytest.mark.parametrize("k,s,p", P.POOL_CONFIGS)
@pytest.mark.parametrize("mode", ["max", "avg"])
def test_pool2d_small(K, mode, k, s, p):
    """3x3 stride 2 without and with leading padding, 3x3 SAME, 2x2 stride 2, an 8-window clipped to the image (the global pool of
    5 x 8; 2 x 2 windows of 64 on 9 x 9) and the 1x1 identity, on a single pixel, a square and a non-square image: the whole
    output, the first, a middle and the last slice of an output 16 channels wider, whose other channels keep their NaN bits"""
    for shape in P.POOL_INPUTS:
        x = P.pool_operands(shape)
        xt = bf(x)[1]
        c = shape[3]
        out_hw = (P.pool_out(shape[1], k, s, p), P.pool_out(shape[2], k, s, p))
        for cy, c_off in ((c, 0), (c + 16, 0), (c + 16, 8), (c + 16, 16)):
            _pool_check(K, x, xt, k, s, p, out_hw, mode, cy, c_off)


@pytest.mark.parametrize("mode", ["max", "avg"])
@pytest.mark.parametrize("case", [P.POOL_BIG, P.POOL_CAP], ids=["stem_147", "past_cap"])
def test_pool2d_large(K, case, mode):
    """the Inception stem's 3x3 stride-2 pool of 4 x 147 x 147 x 128 to 73 x 73; 3x3 SAME on 1449 x 1449 x 8 into the second half
    of a 16-channel output: 2 x 4096 x 256 + 2449 lanes, every thread strides twice"""
    shape, (k, s, p), out_hw = case
    x = P.pool_operands(shape)
    cy, c_off = (shape[3], 0) if case is P.POOL_BIG else (16, 8)
    _pool_check(K, x, bf(x)[1], k, s, p, out_hw, mode, cy, c_off)


def test_pool2d_avg_divides_by_the_in_image_count_at_the_corners(K):
    """3x3 SAME average into channels [8, 24) of 32: each corner is the mean of its 2 x 2 in-image elements (not a ninth of their
    sum), an edge the mean of 6"""
    x = P.pool_operands((2, 9, 9, 16))
    out = nan_fill((2, 9, 9, 32))
    K.pool2d(bf(x)[1], 3, 1, 1, (9, 9), 'avg', out=out, c_off=8)
    got = host(out[..., 8:24])
    for (oh, ow), rows, cols in (((0, 0), (0, 2), (0, 2)), ((0, 8), (0, 2), (7, 9)), ((8, 0), (7, 9), (0, 2)), ((8, 8), (7, 9), (7, 9)),
                                 ((0, 4), (0, 2), (3, 6))):
        win = x[:, rows[0]:rows[1], cols[0]:cols[1]]
        ref, S = win.mean(axis=(1, 2)), np.abs(win).mean(axis=(1, 2))
        ok, idx, ratio = P.within_bf16(got[:, oh, ow], ref, S)
        assert ok, ((oh, ow), idx, ratio)


def test_pool2d_rejections(K):
    x = torch.ones((1, 5, 5, 16), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="multiples of 8"):
        K.pool2d(torch.ones((1, 5, 5, 12), dtype=torch.bfloat16, device="cuda"), 3, 1, 1, (5, 5), 'max')
    out = nan_fill((1, 5, 5, 16))
    with pytest.raises(RuntimeError, match="multiples of 8 inside the output"):
        K.pool2d(x, 3, 1, 1, (5, 5), 'max', out=out, c_off=8)                   # 8 + 16 > 16
    with pytest.raises(RuntimeError, match="reaches past"):
        K.pool2d(x, 3, 2, 0, (4, 4), 'max')                                     # the last window would start at row 6 of 5
    torch.cuda.synchronize()
    assert untouched(out)


# ------------------------------------------------------------------ relu_to_channels
@pytest.mark.parametrize("shape,cy,c_off", [((2, 3, 5, 16), 16, 0), ((2, 3, 5, 16), 40, 8), ((P.RELU_CAP_PIXELS, 8), 16, 8)],
                         ids=["whole", "slice", "past_cap"])
def test_relu_to_channels(K, shape, cy, c_off):
    """-0.0, the most negative and the largest finite bf16, a negative subnormal and zeros among the inputs; the whole output, a
    slice of a wider one, and 2 x 4096 x 256 + 77 lanes: the values of np.maximum(x, 0), the other channels untouched"""
    x = P.relu_operands(shape)
    c = shape[-1]
    out = nan_fill(shape[:-1] + (cy,))
    got = K.relu_to_channels(bf(x)[1], out, c_off)
    assert got is out
    check_equal("relu_to_channels", out[..., c_off:c_off + c], np.maximum(x, 0))
    assert untouched(out[..., :c_off]) and untouched(out[..., c_off + c:])
    if cy == c:
        check_equal("fresh output", K.relu_to_channels(bf(x)[1]), np.maximum(x, 0))


# ------------------------------------------------------------------ pixel norm
@pytest.mark.parametrize("c", P.PIXEL_NORM_C)
def test_pixel_norm_value_and_gradient(K, c):
    """C = 8 (one live lane of 64), 16 and 32 (PGGAN's high-resolution layers), 256, 512 (the kernel's limit, every lane live) at 1,
    9, 48 and 2048 pixels (9: the last block of 4 waves has one live wave).  The first pixel is all zero: a = rsqrt(eps), y = 0 and
    dx = 1e4 dy; the last holds values about 1e3."""
    from gan_lib_tensorflow_amd.common.ops import normalization as Nm
    for shape in P.PIXEL_NORM_SHAPES:
        x, dy = P.pixel_norm_operands(shape, c)
        xt = bf(x)[1].requires_grad_(True)
        y = Nm.pixel_norm(xt)
        y.backward(bf(dy)[1])
        check_bf16("pixel_norm %s x %d" % (shape, c), y, *P.pixel_norm_fwd(x))
        check_bf16("pixel_norm backward %s x %d" % (shape, c), xt.grad, *P.pixel_norm_bwd(dy, x))
        if x.size > c:
            assert not host(y).reshape(-1, c)[0].any()
            assert np.allclose(host(xt.grad).reshape(-1, c)[0], 1e4 * dy.reshape(-1, c)[0], rtol=2.0 ** -7, atol=0)


@pytest.mark.parametrize("c", [520, 12])
def test_pixel_norm_rejects_unsupported_channel_counts(K, c):
    from gan_lib_tensorflow_amd.common.ops import normalization as Nm
    x = torch.ones((1, 2, 2, c), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="C=%d unsupported" % c):
        Nm.pixel_norm(x)
    with pytest.raises(RuntimeError, match="C=%d unsupported" % c):
        K.pixel_norm_bwd(x, x)


# ------------------------------------------------------------------ layer norm
def _layer_norm_store():
    from gan_lib_tensorflow_amd.store import ParamStore, set_default_store
    return set_default_store(ParamStore("cuda", seed=0))


@pytest.mark.parametrize("case,which", P.LAYER_NORM_RUNS)
def test_layer_norm_value_and_gradients(K, case, which):
    """(1,1,8): one pixel, 1023 of 1024 threads idle through the three block reductions; (3,2,2048): the full LDS table, one row of 8
    per thread; (2,16,64): two rows per thread; (5,1,24).  "offset": mean 100, sigma 0.1.  The backward runs twice onto the same
    `main_grad` buffers, so the second run's atomics land on nonzero dgamma / dbeta: both against twice the reference."""
    from gan_lib_tensorflow_amd.common.ops import normalization as Nm
    n, side, c = case
    x, dy, gamma, beta = P.layer_norm_operands(n, side, c, which)
    store = _layer_norm_store()
    scope, gname, bname = 'Discriminator', 'Discriminator/D.Block.2.N1/gamma', 'Discriminator/D.Block.2.N1/beta'
    dyt = bf(dy)[1]
    with store.variable_scope(scope):
        Nm.layer_norm('D.Block.2.N1', [1, 2, 3], bf(x)[1])             # creates gamma / beta
    with torch.no_grad():
        store.vars[gname].copy_(f32(gamma)[1])
        store.vars[bname].copy_(f32(beta)[1])
    for name in (gname, bname):
        store.vars[name].main_grad = torch.zeros(c, dtype=torch.float32, device="cuda")
    for _ in range(2):
        xt = bf(x)[1].requires_grad_(True)
        with store.variable_scope(scope):
            y = Nm.layer_norm('D.Block.2.N1', [1, 2, 3], xt)
        y.backward(dyt)
    torch.cuda.synchronize()
    y_ref, S, cache = P.layer_norm_fwd(x, gamma, beta)
    dx_ref, Sdx, dg, dg_abs, db, db_abs = P.layer_norm_bwd(dy, x, gamma, cache)
    check_bf16("layer_norm", y, y_ref, S)
    check_bf16("layer_norm dx", xt.grad, dx_ref, Sdx)
    # chain: side^2 LDS atomics per channel and sample (one per pixel, any order) + one global atomic per sample and run = side^2 + 2 n
    chain = P.layer_norm_param_chain(n, side * side, 2)
    assert chain == side * side + 2 * n
    if which == "unit":         # at mean 100 every fp32 xhat is off by thousands of ulps of its term: no sum bound sees anything there
        check_f32("dgamma x 2", store.vars[gname].main_grad, 2 * dg, 2 * dg_abs, chain)
    check_f32("dbeta x 2", store.vars[bname].main_grad, 2 * db, 2 * db_abs, chain)
    assert store.vars[gname].grad is None and store.vars[bname].grad is None


def test_layer_norm_rejects_unsupported_channel_counts(K):
    x = torch.ones((1, 1, 1, 2056), dtype=torch.bfloat16, device="cuda")
    g = torch.ones(2056, device="cuda")
    with pytest.raises(RuntimeError, match="C=2056 unsupported"):
        K.layer_norm_fwd(x, g, g)
    with pytest.raises(RuntimeError, match="C=2056 unsupported"):
        K.layer_norm_bwd(x, x, g, torch.ones((1, 2), device="cuda"), g.clone(), g.clone())
