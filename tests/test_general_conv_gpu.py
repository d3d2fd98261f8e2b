"""The general convolution on a real MI355X against tests/general_conv_ref.py: the three ABI entry points on every row of
CASES (every filter size, stride, pad edge, ragged channel and pixel count, each tile route of the dispatchers), the
filter-gradient contract, functional.conv2d_general through autograd on the routes it picks itself, and Conv2D's derived
geometry.  Every element of every result is compared with the per-element allowance derived in general_conv_ref (one bf16
rounding of the result + the any-order fp32 accumulation bound, one more rounding term per bf16 store on the route); only
out_tanh results keep the suite's whole-tensor 1e-2."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import general_conv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
BF_TOL = 1e-2


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gan_lib_tensorflow_amd import kernels
    kernels.lib()
    return kernels


def dev16(t):
    return t.to(torch.bfloat16).cuda().contiguous()


def dev32(t):
    return t.to(torch.float32).cuda().contiguous()


def check(failures, name, got, ref, bnd):
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    ok, ratio, where = R.within(got, ref, bnd)
    print(f"{name}: worst |err| / allowance = {ratio:.3f} at {where}")
    if not ok:
        failures.append(f"{name}: |err| / allowance = {ratio:.3g} at {where}")


# ---------------------------------------------------------------------------------------------------------- ABI level
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.case_id)
def test_abi_entry_points_every_element_within_the_bound(K, i):
    r = R.reference(i)
    n, hin, win, cin, cout, k, s, pad, ho, wo, up, relu = r["case"]
    flags = (K.IN_UPSAMPLE2X if up else 0) | (K.IN_RELU if relu else 0)
    x, dy = dev16(r["x"]), dev16(r["dy"])
    wf, wd = K.prep_weights(dev32(r["w"]), True, s == 1)
    y = K.conv2d_general_fprop(x, wf, dev32(r["b"]), (ho, wo), cout, k, s, pad, flags)
    dw, db = dev32(r["dw0"]), dev32(r["db0"])
    K.conv2d_general_wgrad(x, dy, dw, k, s, pad, flags, dbias=db)
    fails = []
    check(fails, "y", y, r["y"], r["y_bound"])
    check(fails, "dw", dw, r["dw"], r["dw_bound"])
    check(fails, "db", db, r["db"], r["db_bound"])
    if s == 1:
        dxg = K.conv2d_general_dgrad(dy, wd, r["gathered_hw"], cin, k, pad, x if relu and not up else None)
        check(fails, "dx", dxg, r["dxg"], r["dxg_bound"])
    assert not fails, fails


# (the lean kernel, the generic per-tap kernel, the packed narrow-x and narrow-dy kernels, stride 2, the upsampled VALID case)
CONTRACT = [R.find_case(k=4, hin=8, hout=8, cin=64, stride=1), R.find_case(cout=33), R.find_case(cin=3, k=2), R.find_case(cout=3, k=2),
            R.find_case(hin=15, k=4, stride=2, pad=1, cin=64), R.find_case(hin=10, k=5, up=True, cin=64, relu=False)]


@pytest.mark.parametrize("i", CONTRACT, ids=R.case_id)
def test_filter_gradient_accumulates_and_leaves_a_null_dbias_alone(K, i):
    r = R.reference(i)
    n, hin, win, cin, cout, k, s, pad, ho, wo, up, relu = r["case"]
    flags = (K.IN_UPSAMPLE2X if up else 0) | (K.IN_RELU if relu else 0)
    x, dy = dev16(r["x"]), dev16(r["dy"])
    dw, db = dev32(r["dw0"]), dev32(r["db0"])
    K.conv2d_general_wgrad(x, dy, dw, k, s, pad, flags, dbias=db)
    dw1, db1 = dw.clone(), db.clone()
    fails = []
    check(fails, "dw after one call", dw1, r["dw"], r["dw_bound"])
    check(fails, "db after one call", db1, r["db"], r["db_bound"])
    K.conv2d_general_wgrad(x, dy, dw, k, s, pad, flags, dbias=db)
    # the second call starts from the first call's (fp32) result and adds the same sum again
    s1w, s1b = dw1.double().cpu(), db1.double().cpu()
    check(fails, "dw after two calls", dw, s1w + r["dw_sum"], R.bound_f32(r["dw_A"], r["M"], s1w))
    check(fails, "db after two calls", db, s1b + R.db(r["dy"]), R.bound_f32(r["db_A"], r["M"], s1b))
    # dbias = None: the filter gradient is the same and the bias buffer of the earlier calls keeps its bits
    dw3, keep = dev32(r["dw0"]), db.clone()
    K.conv2d_general_wgrad(x, dy, dw3, k, s, pad, flags, dbias=None)
    check(fails, "dw without dbias", dw3, r["dw"], r["dw_bound"])
    torch.cuda.synchronize()
    assert torch.equal(db, keep)
    assert not fails, fails


# --------------------------------------------------------------------------------------------- functional.conv2d_general
def run_general(K, x, w, b, dy, stride, pad, out_hw, up=False, relu=False, tanh=False, x_grad=True):
    from gan_lib_tensorflow_amd import functional as Fn
    xt = dev16(x).requires_grad_(x_grad)
    wt, bt = dev32(w).requires_grad_(True), dev32(b).requires_grad_(True)
    y = Fn.conv2d_general(xt, wt, bt, stride=stride, pad=pad, out_hw=out_hw, upsample=up, in_relu=relu, out_tanh=tanh)
    y.backward(dev16(dy))
    Fn.join_wgrad()
    torch.cuda.synchronize()
    return y.detach(), xt.grad, wt.grad, bt.grad


def compare_route(K, ref, got):
    fails = []
    for name, g in zip(("y", "dx", "dw", "db"), got):
        if g is not None or name != "dx":
            check(fails, name, g, ref[name], ref[name + "_bound"])
    assert not fails, fails


@pytest.mark.parametrize("cout,relu", [(1, False), (3, True), (4, False), (5, True)])
def test_few_output_route_and_its_neighbour(K, cout, relu):
    """Cout <= 4 behind an upsample (k*k*Cout <= 64, Cin % 64 == 0, out == 2*in) runs as a 1x1 conv to tap partials + a
    tap gather; Cout = 5 does not.  Same reference for both; the few-output allowance carries its extra bf16 stores."""
    n, h, w, cin, k, pad = 2, 5, 7, 64, 4, 1
    x, wt, b, dy, _, _ = R.draw((n, h, w, cin), (k, k, cin, cout), (n, 2 * h, 2 * w, cout), 7 + cout)
    few = cout <= 4
    ref = R.few_route(x, wt, b, dy, pad, relu) if few else R.general_route(x, wt, b, dy, 1, pad, (2 * h, 2 * w), True, relu)
    compare_route(K, ref, run_general(K, x, wt, b, dy, 1, pad, (2 * h, 2 * w), True, relu))


@pytest.mark.parametrize("cout", [3, 5])
def test_out_tanh_keeps_the_whole_tensor_tolerance(K, cout):
    """the kernel's tanh has no stated accuracy, so these two (few-output route and general gather) keep max-relative 1e-2
    on y and relative L2 1e-2 on the gradients -- every other test in this file is per element"""
    n, h, w, cin, k, pad = 2, 5, 7, 64, 4, 1
    x, wt, b, dy, _, _ = R.draw((n, h, w, cin), (k, k, cin, cout), (n, 2 * h, 2 * w, cout), 17 + cout)
    y = R.fprop(x, wt, b, 1, pad, (2 * h, 2 * w), True, True, tanh=True)
    g = dy * (1 - y * y)
    ref = dict(y=y, dx=R.dx(x, wt, g, 1, pad, True, True), dw=R.dw(x, g, k, 1, pad, True, True), db=R.db(g))
    got = run_general(K, x, wt, b, dy, 1, pad, (2 * h, 2 * w), True, True, tanh=True)
    for name, t in zip(("y", "dx", "dw", "db"), got):
        t = t.double().cpu()
        assert torch.isfinite(t).all(), name
        if name == "y":
            assert float((t - ref[name]).abs().max() / ref[name].abs().max()) < BF_TOL
        else:
            assert float((t - ref[name]).norm() / ref[name].norm()) < BF_TOL, name


@pytest.mark.parametrize("h,w", [(128, 128), (120, 128)])
def test_phase_stacked_form_at_its_threshold_and_one_step_below(K, h, w):
    """NN-upsample + 4x4 pad-1 conv with Cin % 64 == 0, Cout % 32 == 0, h % 8 == 0, w % 16 == 0 runs as one stacked 3x3 conv +
    depth_to_space from PHASE_STACK_MIN_PIXELS low-resolution pixels on: 128 x 128 = 16384 takes it, 120 x 128 = 15360 (the
    next size down that meets the divisibility conditions) runs the general gather.  Same reference function for both."""
    from gan_lib_tensorflow_amd import functional as Fn
    assert Fn.PHASE_STACK_MIN_PIXELS == 16384 and Fn.PHASE_STACK_UPCONV4
    stacked = h * w >= Fn.PHASE_STACK_MIN_PIXELS
    assert stacked == (h == 128)
    cin, cout, k, pad = 64, 32, 4, 1
    x, wt, b, dy, _, _ = R.draw((1, h, w, cin), (k, k, cin, cout), (1, 2 * h, 2 * w, cout), h)
    ref = R.general_route(x, wt, b, dy, 1, pad, (2 * h, 2 * w), True, True, stacked=stacked)
    compare_route(K, ref, run_general(K, x, wt, b, dy, 1, pad, (2 * h, 2 * w), True, True))


@pytest.mark.parametrize("n,cin", [(4, 3), (4, 6), (3, 6)])
def test_narrow_im2col_filter_gradient_route_at_its_threshold(K, n, cin):
    """kernels.conv2d_general_wgrad sends Cin < 32, k*k*Cin <= 128, Cout % 64 == 0, no flags through im2col + the 1x1 kernels
    from n*Hdy*Wdy >= 16384 output pixels on (IM2COL_NARROW_WGRAD): 4 x 64 x 64 = 16384 is the smallest that takes it (48 and
    96 im2col columns: both paddings), 3 x 64 x 64 stays on the general kernel"""
    assert K.IM2COL_NARROW_WGRAD
    k, s, pad, cout = 4, 2, 1, 64
    x, wt, b, dy, _, _ = R.draw((n, 128, 128, cin), (k, k, cin, cout), (n, 64, 64, cout), 31 * n + cin)
    ref = R.general_route(x, wt, b, dy, s, pad, (64, 64))
    got = run_general(K, x, wt, b, dy, s, pad, (64, 64), x_grad=False)
    assert got[1] is None
    compare_route(K, ref, got)


@pytest.mark.parametrize("k", [4, 3])
@pytest.mark.parametrize("hin,win", [(16, 16), (15, 15), (7, 7), (3, 3), (1, 1), (8, 6), (7, 12)])
def test_stride2_input_gradient(K, k, hin, win):
    """the stride-2 input gradient is the transposed conv by output phase, cropped for odd sizes; k = 4 with its SAME pad 1
    and k = 3 with pad 0 (its SAME pad on even sizes), out = ceil(in / 2)"""
    n, cin, cout, pad = 2, 64, 64, (k - 2) // 2
    oh, ow = -(-hin // 2), -(-win // 2)
    x, wt, b, dy, _, _ = R.draw((n, hin, win, cin), (k, k, cin, cout), (n, oh, ow, cout), 100 * k + 10 * hin + win)
    ref = R.general_route(x, wt, b, dy, 2, pad, (oh, ow), relu=True)
    compare_route(K, ref, run_general(K, x, wt, b, dy, 2, pad, (oh, ow), relu=True))


@pytest.mark.parametrize("k,pad,cout", [(2, 0, 64), (5, 1, 64), (7, 3, 64), (3, 1, 64), (4, 0, 64), (4, 2, 64), (4, 1, 32), (3, 0, 96)])
def test_unsupported_stride2_input_gradients_raise(K, k, pad, cout):
    """anything but a 3x3 / 4x4 filter with pad (k-2)//2 and Cout % 64 == 0 has no stride-2 input gradient: the backward must
    raise, and still serve a caller who does not ask for dx"""
    n, hin, cin = 2, 8, 64
    oh = hin // 2
    x, wt, b, dy, _, _ = R.draw((n, hin, hin, cin), (k, k, cin, cout), (n, oh, oh, cout), k + pad + cout)
    with pytest.raises(NotImplementedError):
        run_general(K, x, wt, b, dy, 2, pad, (oh, oh))
    ref = R.general_route(x, wt, b, dy, 2, pad, (oh, oh))
    got = run_general(K, x, wt, b, dy, 2, pad, (oh, oh), x_grad=False)
    assert got[1] is None
    compare_route(K, ref, got)


# ------------------------------------------------------------------------------------------------------------- Conv2D
@pytest.mark.parametrize("hin,win,k,stride,padding,pad_input", [
    (15, 15, 4, 2, 'SAME', 0),        # odd size: total pad 3, one in front, two behind
    (7, 9, 2, 2, 'SAME', 0),          # odd size, k = 2: total pad 1, all of it behind
    (9, 10, 4, 2, 'VALID', 1),        # tf.pad 1 + VALID, the last padded row / column is never read
])
def test_conv2d_derives_pad_and_output_size_like_the_reference_formula(K, hin, win, k, stride, padding, pad_input):
    from gan_lib_tensorflow_amd.common.ops import conv2d as C
    from gan_lib_tensorflow_amd.store import ParamStore, set_default_store
    from oracle import ref_pix2pix as X
    n, cin, cout = 2, 64, 64
    store = set_default_store(ParamStore("cuda", seed=1))
    x, _, _, _, _, _ = R.draw((n, hin, win, cin), (k, k, cin, cout), (1, 1, 1, cout), hin + win)
    xt = dev16(x)
    kw = dict(padding=padding, he_init=True, biases=True, pad_input=pad_input)
    C.Conv2D(xt, cin, cout, k, stride, 'L', **kw)
    W, b = store.vars['L/Filters'], store.vars['L/Biases']
    with torch.no_grad():
        W.copy_(W.to(torch.bfloat16).float())
        b.copy_(torch.linspace(-1, 1, cout))
    y = C.Conv2D(xt, cin, cout, k, stride, 'L', **kw)
    w64, b64 = W.detach().double().cpu(), b.detach().double().cpu()
    tf = X.conv2d_tf(x, w64, b64, stride, padding, pad_input)         # F.pad by TF's own SAME / tf.pad rule, then an unpadded conv
    assert tuple(y.shape) == tuple(tf.shape)
    oh, ow = tf.shape[1:3]
    pad = pad_input if padding == 'VALID' else R.same_pad(hin, k, stride)[1]
    A = R.fprop_abs(x, w64, b64, stride, pad, (oh, ow))
    assert float((R.fprop(x, w64, b64, stride, pad, (oh, ow)) - tf).abs().max()) < 1e-9
    fails = []
    check(fails, "y", y, tf, R.bound_bf16(tf, A, k * k * cin))
    assert not fails, fails
