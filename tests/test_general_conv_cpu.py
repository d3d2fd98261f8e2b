"""CPU checks of tests/general_conv_ref.py, the reference and allowance that test_general_conv_gpu.py holds the general
convolution to: the tap-loop reference against the oracle's two independent statements of the operation, the allowance
against a correct fp32 / bf16 implementation (it must admit it on every element of every case) and against seeded wrong
ones (each must be rejected by a named case), and the reason the per-element form exists: the whole-tensor metrics of
test_pix2pix_gpu.py let a corner fault through."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import general_conv_ref as R  # noqa: E402
from oracle import ref_pix2pix as X  # noqa: E402

ALL = range(len(R.CASES))


def tf_geometry(case):
    """(padding, pad_input) when tf.nn.conv2d behind an optional symmetric tf.pad is this case's gather, else None"""
    n, hin, win, cin, cout, k, s, pad, ho, wo, up, relu = case
    gh, gw = (2 * hin, 2 * win) if up else (hin, win)
    if (ho, pad) == R.same_pad(gh, k, s) and (wo, pad) == R.same_pad(gw, k, s):
        return 'SAME', 0
    if gh + 2 * pad >= k and gw + 2 * pad >= k and (ho, wo) == ((gh + 2 * pad - k) // s + 1, (gw + 2 * pad - k) // s + 1):
        return 'VALID', pad
    return None


@pytest.mark.parametrize("i", ALL, ids=R.case_id)
def test_reference_agrees_with_the_oracle(i):
    r = R.reference(i)
    n, hin, win, cin, cout, k, s, pad, ho, wo, up, relu = r["case"]
    xp = R.prepare(r["x"], up, relu)
    if ho * wo * k * k <= 4096:            # the plain loops take any geometry; the three largest grids are left to conv2d_tf below
        chk = torch.as_tensor(X.conv2d_numpy(xp.numpy(), r["w"].numpy(), r["b"].numpy(), s, pad, (ho, wo)))
        assert float((chk - r["y"]).abs().max()) < 1e-9
    geo = tf_geometry(r["case"])
    if geo is None:
        assert ho * wo * k * k <= 4096      # every case is checked by at least one of the two
        return
    xr, wr, br = r["x"].clone().requires_grad_(True), r["w"].clone().requires_grad_(True), r["b"].clone().requires_grad_(True)
    y = X.conv2d_tf(R.prepare(xr, up, relu), wr, br, s, geo[0], geo[1])
    assert tuple(y.shape) == tuple(r["y"].shape)
    assert float((y.detach() - r["y"]).abs().max()) < 1e-9
    y.backward(r["dy"])
    assert float((xr.grad - r["dx"]).abs().max()) < 1e-9
    assert float((wr.grad - r["dw_sum"]).abs().max()) < 1e-9 * max(1.0, r["M"] ** 0.5)
    assert float((br.grad + r["db0"] - r["db"]).abs().max()) < 1e-9 * max(1.0, r["M"] ** 0.5)
    if not up:
        g = xr.grad if not relu else R.dx_gathered(r["w"], r["dy"], s, pad, (hin, win)) * (r["x"] > 0)
        assert float((g - r["dxg"]).abs().max()) < 1e-9


def test_the_two_oracle_forms_together_cover_every_geometry_class():
    kinds = {(tf_geometry(c) or ('OTHER',))[0] for c in R.CASES}
    assert kinds == {'SAME', 'VALID', 'OTHER'}


def to_bf16(t):
    return t.to(torch.bfloat16).to(torch.float64)


@pytest.mark.parametrize("i", ALL, ids=R.case_id)
def test_the_bound_admits_a_correct_fp32_bf16_implementation(i):
    """stand-in kernel: the reference's own code run in torch fp32 on the bf16-rounded operands, bf16 results rounded to
    nearest, fp32 results added to the fp32 initial contents -- every element of every result of every case is inside"""
    r = R.reference(i)
    n, hin, win, cin, cout, k, s, pad, ho, wo, up, relu = r["case"]
    x, w, b, dy = (r[name].float() for name in ("x", "w", "b", "dy"))
    bad = []

    def check(name, got, ref, bnd):
        ok, ratio, where = R.within(got, ref, bnd)
        if not ok:
            bad.append((name, ratio, where))

    check("y", to_bf16(R.fprop(x, w, b, s, pad, (ho, wo), up, relu)), r["y"], r["y_bound"])
    g = R.dx_gathered(w, dy, s, pad, r["gathered_hw"])
    if relu and not up:
        g = g * (x > 0)
    check("dx (gathered size)", to_bf16(g), r["dxg"], r["dxg_bound"])
    if up:
        g = R.pool_sum(to_bf16(g).float())
        check("dx (stored size)", to_bf16(g * (x > 0) if relu else g), r["dx"], r["dx_bound"])
    check("dw", r["dw0"].float() + R.dw(x, dy, k, s, pad, up, relu), r["dw"], r["dw_bound"])
    check("db", r["db0"].float() + R.db(dy), r["db"], r["db_bound"])
    assert not bad, bad


def test_the_bound_admits_the_few_output_and_phase_stacked_routes():
    """the two routes with extra bf16 stores, as functional runs them, in the same fp32 / bf16 stand-in arithmetic"""
    n, h, wd, cin, cout, k, pad = 2, 5, 7, 64, 3, 4, 1
    x, w, b, dy, _, _ = R.draw((n, h, wd, cin), (k, k, cin, cout), (n, 2 * h, 2 * wd, cout), 5)
    ref = R.few_route(x, w, b, dy, pad, relu=True)
    xp = R.prepare(x.float(), True, True)
    acc = torch.zeros((n, 2 * h, 2 * wd, cout))
    for a, bb, oy, ox, iy, ix in R._taps(k, 1, pad, (2 * h, 2 * wd), (2 * h, 2 * wd)):
        acc[:, oy, ox, :] += to_bf16(xp[:, iy, ix, :] @ w[a, bb].float()).float()         # Z: one bf16 store per tap partial
    y = to_bf16(acc + b.float())
    assert R.within(y, ref["y"], ref["y_bound"])[0]
    # phase-stacked: the 4x4 filter's taps summed per output phase and low-resolution offset, rounded to bf16, applied at the low resolution
    cout = 32
    x, w, b, dy, _, _ = R.draw((n, 8, 16, cin), (k, k, cin, cout), (n, 16, 32, cout), 6)
    ref = R.general_route(x, w, b, dy, 1, pad, (16, 32), True, True, stacked=True)
    rows = {0: ((0,), (1, 2), (3,)), 1: ((), (0, 1), (2, 3))}      # output parity -> taps of w read at low-resolution offsets -1, 0, +1
    xl = torch.relu(x.float())
    y = torch.zeros((n, 16, 32, cout))
    for pa in (0, 1):
        for pb in (0, 1):
            w3 = torch.zeros((3, 3, cin, cout), dtype=torch.float64)
            for i3, ta in enumerate(rows[pa]):
                for j3, tb in enumerate(rows[pb]):
                    for a in ta:
                        for bb in tb:
                            w3[i3, j3] += w[a, bb]
            y[:, pa::2, pb::2, :] = R.gather(xl, to_bf16(w3).float(), 1, 1, (8, 16))
    y = to_bf16(y + b.float())
    assert float((R.general_route(x, w, b, dy, 1, pad, (16, 32), True, True)["y"] - ref["y"]).abs().max()) == 0
    assert R.within(y, ref["y"], ref["y_bound"])[0]


# ----------------------------------------------------------------------------------------------------------- mutants
def mutant(r, name):
    """(y, dw) of a wrong implementation in exact float64 arithmetic: only the named fault separates it from the reference"""
    n, hin, win, cin, cout, k, s, pad, ho, wo, up, relu = r["case"]
    x, w, b, dy = r["x"], r["w"], r["b"], r["dy"]
    xp = R.prepare(x, up, relu)
    gh, gw = r["gathered_hw"]
    dw0 = r["dw0"]
    if name == "corner_tap":                # the filter's last tap is skipped at each image's last output pixel
        y, dwv = R.gather(xp, w, s, pad, (ho, wo)) + b, R.dw(xp, dy, k, s, pad)
        iy, ix = (ho - 1) * s + k - 1 - pad, (wo - 1) * s + k - 1 - pad
        if iy < gh and ix < gw:
            y[:, -1, -1, :] -= xp[:, iy, ix, :] @ w[-1, -1]
            dwv[-1, -1] -= xp[:, iy, ix, :].t() @ dy[:, -1, -1, :]
        return y, dw0 + dwv
    if name == "pad_plus_one":
        pad = pad + 1
    elif name == "bound_from_output":       # taps bounded by dy's grid instead of x''s
        xp = xp.clone()
        xp[:, ho:, :, :] = 0
        xp[:, :, wo:, :] = 0
    elif name == "surplus_front":           # the larger half of the total pad in front
        pad = max((ho - 1) * s + k - gh, 0) - pad
    elif name == "swap_ab":
        w = w.transpose(0, 1)
    elif name == "skip_last_row_s2":
        if s == 2 and gh % 2 == 1:
            xp = xp.clone()
            xp[:, -1, :, :] = 0
    elif name == "relu_border":             # relu skipped on the outermost ring of the stored image (applied behind the border logic)
        xm = torch.relu(x) if relu else x.clone()
        if relu:
            xm[:, 0, :, :], xm[:, -1, :, :], xm[:, :, 0, :], xm[:, :, -1, :] = x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1]
        xp = R.prepare(xm, up, False)
    elif name == "dw_overwrite":
        dw0 = 0
    else:
        raise KeyError(name)
    dwv = R.dw(xp, dy, k, s, pad)
    if name == "swap_ab":
        dwv = dwv.transpose(0, 1)
    return R.gather(xp, w, s, pad, (ho, wo)) + b, dw0 + dwv


def rejected(r, y, dwv):
    return not (R.within(y, r["y"], r["y_bound"])[0] and R.within(dwv, r["dw"], r["dw_bound"])[0])


# mutant -> the case of CASES that catches it
CATCHERS = {
    "corner_tap": dict(hin=5, win=9, k=3, stride=1, pad=0),                      # VALID 5x9 -> 3x7: the last tap of the last pixel reads x[4, 8]
    "pad_plus_one": dict(hin=5, win=9, k=3, stride=1, pad=1),
    "bound_from_output": dict(hin=5, win=9, k=5, stride=1, pad=0),               # stride 1: 5x9 -> 1x5, rows 1..4 of x lie past dy's grid
    "surplus_front": dict(hin=8, hout=8, k=4, stride=1, pad=1, cin=64),          # total pad 3: 1 in front, 2 behind
    "swap_ab": dict(hin=5, win=9, k=3, stride=1, pad=0),                         # non-square
    "skip_last_row_s2": dict(hin=15, k=4, stride=2, pad=1, cin=64),
    "relu_border": dict(up=True, relu=True, k=4, hin=4, win=5),
    "dw_overwrite": dict(hin=5, win=9, k=1),
}
UP_CATCHER = dict(up=True, hin=10, k=5, cin=64, relu=False)                      # upsampled: 20 -> 16, rows / columns 16..19 of x' past dy's grid


@pytest.mark.parametrize("name", list(CATCHERS) + ["bound_from_output/upsampled"])
def test_the_bound_rejects_each_seeded_mutant_on_a_named_case(name):
    want = UP_CATCHER if "/" in name else CATCHERS[name]
    name = name.split("/")[0]
    i = R.find_case(**want)
    r = R.reference(i)
    assert not rejected(r, r["y"], r["dw"])
    y, dwv = mutant(r, name)
    assert rejected(r, y, dwv), (name, R.case_id(i))


def test_every_mutant_is_inert_somewhere_so_the_named_cases_matter():
    """out == 2*in hides the output-size bound, an even total pad hides the surplus side, an even input hides the last row"""
    for name, want in (("bound_from_output", dict(up=True, k=4, hin=4, win=5)), ("surplus_front", dict(hin=5, win=9, k=3, stride=1, pad=1)),
                       ("skip_last_row_s2", dict(hin=16, win=9, k=4, stride=2, pad=1))):
        r = R.reference(R.find_case(**want))
        assert not rejected(r, *mutant(r, name)), name


def test_whole_tensor_metrics_pass_a_corner_fault_that_the_bound_rejects():
    """The metrics of test_pix2pix_gpu.py on the gradients -- relative L2 < 1e-2 on dx, < 4e-3 on dw, the only checks the
    separate dgrad and wgrad kernels get there -- accept the corner-tap mutant on a 131x131 -> 128x128 image: one tap of one pixel is
    1 / (16 * 16384) of the terms (relative L2 about 1 / (k * Hout) = 2e-3 on either gradient).  The per-element allowance rejects it in y and in dx at that size, and in dw on the small
    case above (the fp32 allowance grows with M^2, which is why CASES keeps M small)."""
    n, hin, cin, cout, k, ho = 1, 131, 32, 32, 4, 128
    x, w, b, dy, _, _ = R.draw((n, hin, hin, cin), (k, k, cin, cout), (n, ho, ho, cout), 99)
    ref = R.general_route(x, w, b, dy, 1, 0, (ho, ho))
    y, dwv, dxv = ref["y"].clone(), ref["dw"].clone(), ref["dx"].clone()
    y[:, -1, -1, :] -= x[:, -1, -1, :] @ w[-1, -1]
    dwv[-1, -1] -= x[:, -1, -1, :].t() @ dy[:, -1, -1, :]
    dxv[:, -1, -1, :] -= dy[:, -1, -1, :] @ w[-1, -1].t()

    def l2(got, want):
        return float((got - want).norm() / want.norm())

    assert 0 < l2(dxv, ref["dx"]) < 1e-2 and 0 < l2(dwv, ref["dw"]) < 4e-3
    assert not R.within(dxv, ref["dx"], ref["dx_bound"])[0]
    assert not R.within(y, ref["y"], ref["y_bound"])[0]
    assert R.within(ref["dx"], ref["dx"], ref["dx_bound"])[0]
