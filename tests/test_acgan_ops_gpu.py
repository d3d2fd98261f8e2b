"""The kernels of csrc/acgan_ops.hip through kernels.py on a real MI355X, each against a float64 restatement of the same operation on
shared (bf16- or fp32-rounded) operands: the second-order batch norm at every block / grid-cap / channel-group regime, the moving
statistics update, the gradient-penalty reduction, the row interpolation past its grid cap, and the spatial sum / broadcast pair.
Single-launch bounds of tests/test_kernels_gpu.py: bf16 outputs 1e-2 of the maximum, fp32 outputs from bf16 operands 2e-3."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import functional2_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF_TOL = 1e-2
F32_FROM_BF_TOL = 2e-3
F64 = torch.float64


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


def relerr(got, ref):
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


# ------------------------------------------------------------------ bn_bwd_bwd
BN2_CASES = [(96, 128), (257, 64), (40, 8), (262149, 8), (2100, 2048)]
BN2_SETS = {"zero_mean": (0.0, 0.0, 1.0), "offset_means": (1.0, -0.5, 0.3)}      # mean of a, mean of dy, sigma of both


def bn2_operands(rows, c, which):
    ma, mg, sig = BN2_SETS[which]
    rng = np.random.default_rng(rows + c)
    x = bf(rng.normal(size=(rows, 1, 1, c)) * 1.5 + 0.3)
    dy = bf(rng.normal(size=(rows, 1, 1, c)) * sig + mg)
    a = bf(rng.normal(size=(rows, 1, 1, c)) * sig + ma)
    gamma = f32(rng.normal(size=c) * 0.3 + 1.0)
    return x, dy, a, gamma


@pytest.mark.parametrize("which", list(BN2_SETS))
@pytest.mark.parametrize("rows,c", BN2_CASES)
def test_bn_bwd_bwd_vs_float64_autograd(K, rows, c, which):
    """gank_bn_bwd_bwd against float64 autograd of the first backward (functional2_ref.BNB), the statistics computed in float64 and
    passed as fp32 so that only this kernel is under test: gI, ggO <= 1e-2 of the maximum, gG <= 2e-3, gG accumulated onto 0.5.

    (96, 128) one block; (257, 64) two blocks, the second ragged; (40, 8) one channel group on 256 row lanes; (262149, 8) past the
    1024-block cap of the sums launch; (2100, 2048) 256 channel groups on one row lane and past the 2048-block cap of the apply
    launch.  Each with zero-mean a, dy (sigma 1) and with means +1.0 / -0.5 (sigma 0.3), where AG - A0 G0 / M cancels.

    What float32 arithmetic alone costs on these operands (the closed forms of functional2_ref.bn_second_order_closed_forms
    evaluated in torch float32 on the CPU against float64; gI / ggO / gG, relative to the maximum) -- every figure is within a
    quarter of its bound, so a kernel that misses a bound is summing worse than float32 has to:
        (96, 128)     zero mean 1.7e-7 / 1.2e-7 / 9.2e-8     offset means 2.7e-6 / 1.3e-7 / 2.5e-6
        (257, 64)     zero mean 2.6e-7 / 1.8e-7 / 1.4e-7     offset means 3.8e-6 / 1.6e-7 / 6.5e-6
        (40, 8)       zero mean 9.0e-8 / 5.4e-8 / 8.2e-8     offset means 5.1e-7 / 7.4e-8 / 1.2e-6
        (262149, 8)   zero mean 3.4e-7 / 1.6e-7 / 1.1e-7     offset means 2.4e-4 / 2.5e-7 / 2.5e-4
        (2100, 2048)  zero mean 3.7e-7 / 1.5e-7 / 1.3e-7     offset means 2.1e-5 / 2.1e-7 / 2.0e-5"""
    (x, xt), (dy, dyt), (a, at), (gamma, gt) = bn2_operands(rows, c, which)
    gI_ref, ggO_ref, gG_ref = R.bn_second_order_autograd(a, dy, x, gamma)
    mu = x.mean(dim=(0, 1, 2))
    invstd = torch.rsqrt(((x - mu) ** 2).mean(dim=(0, 1, 2)) + 1e-5)
    stats = torch.cat([mu, invstd]).float().cuda()
    gG = torch.full((c,), 0.5, device="cuda")
    gI, ggO = K.bn_bwd_bwd(at, dyt, xt, gt, stats, gG)
    torch.cuda.synchronize()
    errs = dict(gI=relerr(gI, gI_ref), ggO=relerr(ggO, ggO_ref), gG=relerr(gG.double().cpu() - 0.5, gG_ref))
    print("bn_bwd_bwd", rows, c, which, {k: "%.2e" % v for k, v in errs.items()})
    assert errs["gI"] < 1e-2 and errs["ggO"] < 1e-2 and errs["gG"] < 2e-3, errs


@pytest.mark.parametrize("c", [24, 12, 4096])
def test_bn_bwd_bwd_rejects_unsupported_channel_counts(K, c):
    """C must be a multiple of 8, at most 2048, with C / 8 dividing 256: anything else is the library's error and no launch"""
    rows = 16
    x = torch.ones((rows, 1, 1, c), dtype=torch.bfloat16, device="cuda")
    gG = torch.full((c,), 0.5, device="cuda")
    stats = torch.ones(2 * c, device="cuda")
    with pytest.raises(RuntimeError, match="unsupported channel count %d" % c):
        K.bn_bwd_bwd(x, x, x, torch.ones(c, device="cuda"), stats, gG)
    torch.cuda.synchronize()
    assert bool((gG == 0.5).all())


# ------------------------------------------------------------------ bn_moving_update
@pytest.mark.parametrize("count", [1, 4096])
@pytest.mark.parametrize("step0", [0, 7])
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("c", [1, 100, 1000, 1024])
def test_bn_moving_update_vs_float64(K, c, groups, step0, count):
    """tf.contrib.layers.batch_norm's moving statistics with zero-debiased mean, towers applied in order (the recurrence stated above
    gank_bn_moving_update), in float64 on the same fp32 operands: 1e-5 of the maximum (about ten fp32 roundings and one powf);
    local_step exact.  Variances >= 1e-2, so 1 / invstd^2 - eps does not cancel."""
    rng = np.random.default_rng(c * 100 + groups * 10 + step0 + count)
    decay, eps = 0.9, 1e-5
    mean = rng.normal(size=(groups, c))
    var = rng.uniform(1e-2, 4.0, size=(groups, c))
    stats, statst = f32(np.stack([mean, 1.0 / np.sqrt(var + eps)], axis=1))            # [groups, 2, C]
    (mm, mmt), (mv, mvt), (b, bt) = f32(rng.normal(size=c)), f32(rng.uniform(0.5, 2.0, size=c)), f32(rng.normal(size=c) * 0.5)
    stept = torch.full((1,), float(step0), device="cuda")
    K.bn_moving_update(statst, mmt, mvt, bt, stept, count, decay, eps)
    torch.cuda.synchronize()
    unbias = count / (count - 1) if count > 1 else 1.0
    st = float(step0)
    for g in range(groups):
        mv = decay * mv + (1 - decay) * (1.0 / stats[g, 1] ** 2 - eps) * unbias
        b = decay * b + (1 - decay) * stats[g, 0]
        st += 1.0
        mm = b / (1.0 - decay ** st)
    assert float(stept) == step0 + groups
    errs = dict(moving_mean=relerr(mmt, mm), moving_variance=relerr(mvt, mv), biased=relerr(bt, b))
    assert all(e < 1e-5 for e in errs.values()), errs


def test_bn_moving_update_rejects_more_than_one_block(K):
    c = 1025
    mm, mv, b = (torch.full((c,), v, device="cuda") for v in (0.25, 1.5, 0.75))
    step = torch.full((1,), 3.0, device="cuda")
    with pytest.raises(RuntimeError, match="C = 1025 > 1024"):
        K.bn_moving_update(torch.ones((1, 2, c), device="cuda"), mm, mv, b, step, 64)
    torch.cuda.synchronize()
    assert float(step) == 3.0 and bool((mm == 0.25).all()) and bool((mv == 1.5).all()) and bool((b == 0.75).all())


# ------------------------------------------------------------------ gp_loss
def gp_rows(n, d, seed):
    """N rows of D: random ones, and (as far as N allows) one all-zero row and rows of norm 1 + 2^-7 and 1 - 2^-7"""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(n, d)) * (1.5 / np.sqrt(d))
    special = {}
    if n >= 4:
        special = {1: 0.0, 2: 1.0 + 2.0 ** -7, 4: 1.0 - 2.0 ** -7}
    for row, norm in special.items():
        g[row] = g[row] / np.linalg.norm(g[row]) * norm
    return g, special


def gp_reference(g, lam):
    gr = g.clone().requires_grad_(True)
    loss = R.GPLoss(gr, lam)
    (dg,) = torch.autograd.grad(loss, gr)
    return loss.detach(), dg


def check_gp(K, g, gt, lam, special=()):
    n = g.shape[0]
    loss_ref, dg_ref = gp_reference(g, lam)
    loss, dg = K.gp_loss(gt, lam)
    torch.cuda.synchronize()
    norms = g.reshape(n, -1).norm(dim=1)
    scale = float(lam * ((norms + 1.0) ** 2).mean())
    assert bool(torch.isfinite(loss).all()) and abs(float(loss) - float(loss_ref)) <= F32_FROM_BF_TOL * scale, (float(loss), float(loss_ref))
    assert dg.dtype == torch.float32 and relerr(dg, dg_ref) < F32_FROM_BF_TOL
    for row in special:                                         # each special row on its own maximum, not hidden behind the others
        if float(dg_ref[row].abs().max()) == 0.0:
            assert bool((dg[row] == 0).all())
        else:
            assert relerr(dg[row], dg_ref[row]) < F32_FROM_BF_TOL, row
    return dg_ref


@pytest.mark.parametrize("d", [1, 255, 3072])
@pytest.mark.parametrize("n", [1, 7])
def test_gp_loss_vs_float64(K, n, d):
    """lam * mean_n (sqrt(sum g^2 + 1e-10) - 1)^2 and its derivative against float64 autograd on the bf16-rounded rows: the loss at
    2e-3 of lam * mean (|g| + 1)^2, dg at 2e-3 of the maximum; an all-zero row gives dg == 0 exactly and a finite loss; rows of
    norm 1 +- 2^-7 (where slope - 1 cancels) hold the bound on their own maximum.  D = (3072, 1, 1) is the trainer's shape class,
    255 a ragged tail of the 256-thread row loop, 1 a single element."""
    lam = 10.0
    g, special = gp_rows(n, d, 10 * n + d)
    g, gt = bf(g.reshape(n, d, 1, 1) if d > 1 else g.reshape(n, 1))
    check_gp(K, g, gt, lam, special)
    if n == 1:                                                  # the special rows, one at a time
        for v in (np.zeros(d), np.full(d, (1.0 + 2.0 ** -7) / np.sqrt(d)), np.full(d, (1.0 - 2.0 ** -7) / np.sqrt(d))):
            g1, g1t = bf(v.reshape(1, d))
            check_gp(K, g1, g1t, lam, (0,))


def test_gp_loss_function_backward_scales_by_upstream(K):
    """functional2.GPLoss.backward: the saved fp32 derivative times an upstream scalar (3.0), rounded once to bf16: 1e-2 of the maximum"""
    from gan_lib_tensorflow_amd import functional2 as F2
    g, special = gp_rows(7, 255, 3)
    g, gt = bf(g.reshape(7, 255))
    _, dg_ref = gp_reference(g, 10.0)
    gt.requires_grad_(True)
    loss = F2.gradient_penalty(gt, 10.0)
    (loss * 3.0).sum().backward()
    torch.cuda.synchronize()
    assert gt.grad.dtype == torch.bfloat16 and relerr(gt.grad, 3.0 * dg_ref) < BF_TOL
    assert bool((gt.grad[1] == 0).all())


# ------------------------------------------------------------------ lerp_rows
@pytest.mark.parametrize("n,d,alpha", [(3, 200003, [0.0, 1.0, 0.37]), (5, 7, [0.0, 1.0, 0.25, 0.5, 0.9])])
def test_lerp_rows_vs_float64(K, n, d, alpha):
    """real + alpha[n] (fake - real): 3 x 200003 is 600009 elements, past one sweep of the capped grid (2048 blocks x 256 threads =
    524288) with an odd row length; alpha = 0 reproduces `real` to the bit, every other element is one bf16 rounding from the
    float64 value (|err| <= 2^-8 |ref| + 1e-6)."""
    rng = np.random.default_rng(d)
    (r, rt), (f, ft) = bf(rng.normal(size=(n, d))), bf(rng.normal(size=(n, d)))
    al, alt = f32(np.asarray(alpha))
    out = K.lerp_rows(rt, ft, alt)
    torch.cuda.synchronize()
    ref = r + al.reshape(-1, 1) * (f - r)
    got = out.double().cpu()
    assert torch.equal(out[0].cpu(), rt[0].cpu())
    bad = (got - ref).abs() > 2.0 ** -8 * ref.abs() + 1e-6
    assert not bool(bad.any()), (int(bad.sum()), torch.nonzero(bad)[:4].tolist())


# ------------------------------------------------------------------ sum_hw / bcast_hw
@pytest.mark.parametrize("n,hw,c", [(3, (1, 1), 13), (5, (8, 8), 128), (17, (16, 16), 257)])
def test_sum_hw_bcast_hw_vs_float64_and_adjoint(K, n, hw, c):
    """y[n, c] = scale sum_hw x and its adjoint y[n, hw, c] = scale g[n, c]; 17 x 256 x 257 is 1118464 output elements, past one sweep
    of bcast_hw's capped grid (4096 x 256 = 1048576).  bcast_hw is one bf16 rounding of the float64 value, sum_hw 1e-2 of the maximum,
    and <sum_hw(x), g> = <x, bcast_hw(g)> on float64 copies of the two kernel outputs to 1e-2 of |sum_hw(x)| |g| (each side carries
    one bf16 rounding per output element, 2^-9 relative, so the two differ by far less than that product of norms times 1e-2)."""
    rng = np.random.default_rng(n * c)
    scale = 1.0 / (hw[0] * hw[1])
    (x, xt), (g, gt) = bf(rng.normal(size=(n, hw[0], hw[1], c)) + 0.25), bf(rng.normal(size=(n, c)))
    s, b = K.sum_hw(xt, scale), K.bcast_hw(gt, hw, scale)
    torch.cuda.synchronize()
    assert s.shape == (n, c) and b.shape == (n, hw[0], hw[1], c)
    s_ref, b_ref = R.SumHW(x, float(np.float32(scale))), R.BcastHW(g, hw, float(np.float32(scale)))
    assert relerr(s, s_ref) < BF_TOL
    bad = (b.double().cpu() - b_ref).abs() > 2.0 ** -8 * b_ref.abs()
    assert not bool(bad.any()), int(bad.sum())
    s64, b64 = s.double().cpu(), b.double().cpu()
    lhs, rhs = float((s64 * g).sum()), float((x * b64).sum())
    assert abs(lhs - rhs) <= BF_TOL * float(s64.norm() * g.norm()), (lhs, rhs)
