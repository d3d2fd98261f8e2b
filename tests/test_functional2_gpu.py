"""Every autograd.Function of functional2 (the twice-differentiable operator set of the ACGAN critic) on its own, on a real MI355X:
the forward value and the vector-Jacobian product with respect to each differentiable input, with a random bf16 cotangent, against
the float64 restatements of tests/functional2_ref.py on shared bf16-rounded operands.  Each comparison is one kernel launch, so the
single-launch bounds of tests/test_kernels_gpu.py apply: bf16 outputs 1e-2 of the reference maximum, fp32 outputs from bf16 operands
2e-3; copies, selections and sums of two are bit-exact.  Then one small critic for how gradients are DELIVERED: returned to autograd,
accumulated in place into an existing `.grad`, under input_gradient_only() and under one_update() / prepare_batched()."""
import contextlib
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
def F2():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gan_lib_tensorflow_amd import kernels
    kernels.lib()
    assert kernels.BF16 is torch.bfloat16
    from gan_lib_tensorflow_amd import functional2
    return functional2


def pair(a, f32=False):
    """values rounded to bf16 -> (float64 CPU leaf, cuda leaf: bf16, or fp32 holding the same values), both requiring gradients"""
    t = torch.as_tensor(np.asarray(a, np.float32)).to(torch.bfloat16)
    dev = (t.float() if f32 else t).cuda().contiguous()
    return t.to(F64).requires_grad_(True), dev.requires_grad_(True)


def relerr(got, ref):
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def tol_of(t):
    return BF_TOL if t.dtype == torch.bfloat16 else F32_FROM_BF_TOL


def check(name, rng, out_dev, out_ref, ins_dev, ins_ref):
    """forward value, then the VJP with one random bf16 cotangent with respect to every input listed"""
    e = relerr(out_dev, out_ref)
    assert e < tol_of(out_dev), (name, "forward", e)
    ct = torch.as_tensor(rng.normal(size=tuple(out_ref.shape)).astype(np.float32)).to(torch.bfloat16)
    g_dev = torch.autograd.grad(out_dev, ins_dev, ct.to(out_dev.dtype).cuda())
    g_ref = torch.autograd.grad(out_ref, ins_ref, ct.to(F64))
    torch.cuda.synchronize()
    for i, (gd, gr, x) in enumerate(zip(g_dev, g_ref, ins_dev)):
        assert gd is not None and gd.shape == x.shape, (name, i)
        e = relerr(gd, gr)
        assert e < tol_of(gd), (name, "vjp of input %d" % i, e)


# ------------------------------------------------------------------ convolution
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("h,w", [(8, 8), (4, 8)])
@pytest.mark.parametrize("cin,cout", [(3, 128), (128, 128), (8, 64)])
@pytest.mark.parametrize("k", [3, 1])
def test_conv_functions(F2, k, cin, cout, h, w, n):
    """ConvF (with and without bias), ConvD and ConvW.  cin = 3 makes ConvD the penalty's gradient with respect to the image
    (3 output channels); ConvW's cotangent is an fp32 tensor that its backward uses as a filter."""
    rng = np.random.default_rng(1000 * k + 10 * cin + h + n)
    x, xt = pair(rng.normal(size=(n, h, w, cin)))
    dy, dyt = pair(rng.normal(size=(n, h, w, cout)))
    W, Wt = pair(rng.normal(size=(k, k, cin, cout)) / np.sqrt(k * k * cin), f32=True)
    b, bt = pair(rng.normal(size=cout), f32=True)
    check("ConvF+bias", rng, F2.ConvF.apply(xt, Wt, bt), R.ConvF(x, W, b), (xt, Wt, bt), (x, W, b))
    check("ConvF", rng, F2.ConvF.apply(xt, Wt, None), R.ConvF(x, W), (xt, Wt), (x, W))
    check("ConvD", rng, F2.ConvD.apply(dyt, Wt), R.ConvD(dy, W), (dyt, Wt), (dy, W))
    out = F2.ConvW.apply(xt, dyt, Wt.shape)
    assert out.dtype == torch.float32 and out.shape == Wt.shape
    check("ConvW", rng, out, R.ConvW(x, dy, W.shape), (xt, dyt), (x, dy))


@pytest.mark.parametrize("k,cin,cout", [(3, 8, 64), (1, 3, 128)])
def test_conv_functions_with_non_leaf_filter(F2, k, cin, cout):
    """Inside one_update() a filter that is itself a graph node -- the `g` ConvW.backward hands to ConvD / ConvF -- is prepared at
    the point of use, never cached: two different non-leaf filters in a row, each against float64, gradients reaching their leaves."""
    with F2.one_update():
        for seed in (1, 2):
            rng = np.random.default_rng(seed)
            x, xt = pair(rng.normal(size=(3, 4, 8, cin)))
            dy, dyt = pair(rng.normal(size=(3, 4, 8, cout)))
            W, Wt = pair(rng.normal(size=(k, k, cin, cout)) / np.sqrt(k * k * cin), f32=True)
            assert not (Wt * 1.0).is_leaf and (Wt * 1.0).dtype == torch.float32
            check("ConvD(non-leaf W)", rng, F2.ConvD.apply(dyt, Wt * 1.0), R.ConvD(dy, W), (dyt, Wt), (dy, W))
            check("ConvF(non-leaf W)", rng, F2.ConvF.apply(xt, Wt * 1.0, None), R.ConvF(x, W), (xt, Wt), (x, W))
            # ConvW.backward with a non-leaf cotangent as its filter
            g, gt = pair(rng.normal(size=(k, k, cin, cout)), f32=True)
            gd = torch.autograd.grad(F2.ConvW.apply(xt, dyt, Wt.shape), (xt, dyt), gt * 1.0)
            gr = torch.autograd.grad(R.ConvW(x, dy, W.shape), (x, dy), g.detach())
            assert relerr(gd[0], gr[0]) < BF_TOL and relerr(gd[1], gr[1]) < BF_TOL


# ------------------------------------------------------------------ linear
@pytest.mark.parametrize("m,k,c", [(5, 128, 1), (8, 128, 10), (3, 7, 3)])
def test_linear_functions(F2, m, k, c):
    rng = np.random.default_rng(m * k + c)
    x, xt = pair(rng.normal(size=(m, k)))
    dy, dyt = pair(rng.normal(size=(m, c)))
    W, Wt = pair(rng.normal(size=(k, c)) / np.sqrt(k), f32=True)
    b, bt = pair(rng.normal(size=c), f32=True)
    check("LinF+bias", rng, F2.LinF.apply(xt, Wt, bt), R.LinF(x, W, b), (xt, Wt, bt), (x, W, b))
    check("LinF", rng, F2.LinF.apply(xt, Wt, None), R.LinF(x, W), (xt, Wt), (x, W))
    check("LinD", rng, F2.LinD.apply(dyt, Wt), R.LinD(dy, W), (dyt, Wt), (dy, W))
    out = F2.LinW.apply(xt, dyt)
    assert out.dtype == torch.float32
    check("LinW", rng, out, R.LinW(x, dy), (xt, dyt), (x, dy))
    with F2.one_update():                                    # LinW.backward's call: a graph node as the weight
        check("LinF(non-leaf W)", rng, F2.LinF.apply(xt, Wt * 1.0, None), R.LinF(x, W), (xt, Wt), (x, W))


# ------------------------------------------------------------------ leaky relu
@pytest.mark.parametrize("leak", [0.2, 0.0])
def test_lrelu_functions(F2, leak):
    rng = np.random.default_rng(7)
    x, xt = pair(rng.normal(size=(3, 4, 8, 13)))
    dy, dyt = pair(rng.normal(size=(3, 4, 8, 13)))
    assert float(x.abs().min()) > 0
    check("LRelu", rng, F2.LRelu.apply(xt, leak), R.LRelu(x, leak), (xt,), (x,))
    out = F2.LReluB.apply(dyt, xt, leak)
    check("LReluB", rng, out, R.LReluB(dy, x, leak), (dyt,), (dy,))
    if leak == 0.0:                                          # a selection: to the bit, forward and backward
        zero = torch.zeros_like(dyt)
        assert torch.equal(F2.LRelu.apply(xt, leak).detach(), torch.where(xt > 0, xt, zero).detach())
        out = F2.LReluB.apply(dyt, xt, leak)
        assert torch.equal(out.detach(), torch.where(xt > 0, dyt, zero).detach())
        (g,) = torch.autograd.grad(out, dyt, xt.detach())
        assert torch.equal(g, torch.where(xt > 0, xt, zero).detach())


# ------------------------------------------------------------------ pooling
@pytest.mark.parametrize("scale", [0.25, 1.0])
@pytest.mark.parametrize("h,w", [(2, 2), (8, 4)])
@pytest.mark.parametrize("c", [8, 128])
def test_pool_functions(F2, c, h, w, scale):
    rng = np.random.default_rng(c + h)
    x, xt = pair(rng.normal(size=(3, h, w, c)))
    g, gt = pair(rng.normal(size=(3, h // 2, w // 2, c)))
    check("Pool2", rng, F2.Pool2.apply(xt, scale), R.Pool2(x, scale), (xt,), (x,))
    check("Unpool2", rng, F2.Unpool2.apply(gt, scale), R.Unpool2(g, scale), (gt,), (g,))


@pytest.mark.parametrize("hw", [(1, 1), (8, 8)])
@pytest.mark.parametrize("c", [3, 13, 128])
def test_sum_hw_functions(F2, c, hw):
    rng = np.random.default_rng(c)
    scale = 1.0 / (hw[0] * hw[1])
    x, xt = pair(rng.normal(size=(3, hw[0], hw[1], c)) + 0.25)
    g, gt = pair(rng.normal(size=(3, c)))
    s, b = F2.SumHW.apply(xt, scale), F2.BcastHW.apply(gt, hw, scale)
    check("SumHW", rng, s, R.SumHW(x, scale), (xt,), (x,))
    check("BcastHW", rng, b, R.BcastHW(g, hw, scale), (gt,), (g,))
    # the pair is adjoint: <SumHW x, g> = <x, BcastHW g> on float64 copies of the outputs, to 1e-2 of |SumHW x| |g|
    s64, b64 = s.detach().double().cpu(), b.detach().double().cpu()
    lhs, rhs = float((s64 * g.detach()).sum()), float((x.detach() * b64).sum())
    assert abs(lhs - rhs) <= BF_TOL * float(s64.norm() * g.detach().norm()), (lhs, rhs)


# ------------------------------------------------------------------ batch norm
@pytest.mark.parametrize("rows", [96, 257])
@pytest.mark.parametrize("c", [8, 128])
def test_batch_norm_functions(F2, c, rows):
    """BNF (value, statistics, VJP with respect to x, gamma, beta) and BNB (dx, dgamma, dbeta; the VJP of dx with respect to dy, x and
    gamma is the second-order kernel).  BNB gets float64 statistics as fp32, so that its comparisons are of its own launch only."""
    rng = np.random.default_rng(rows + c)
    x, xt = pair(rng.normal(size=(rows, 1, 1, c)) * 1.5 + 0.3)
    dy, dyt = pair(rng.normal(size=(rows, 1, 1, c)))
    gamma, gt = pair(rng.normal(size=(1, c)) * 0.3 + 1.0, f32=True)
    beta, bt = pair(rng.normal(size=(1, c)) * 0.2, f32=True)
    y, stats = F2.BNF.apply(xt, gt, bt)
    mu = x.detach().mean(dim=(0, 1, 2))
    invstd = torch.rsqrt(((x.detach() - mu) ** 2).mean(dim=(0, 1, 2)) + 1e-5)
    assert stats.shape == (2, c) and not stats.requires_grad
    assert relerr(stats[0], mu) < F32_FROM_BF_TOL and relerr(stats[1], invstd) < F32_FROM_BF_TOL
    check("BNF", rng, y, R.BNF(x, gamma, beta), (xt, gt, bt), (x, gamma, beta))

    st = torch.stack([mu, invstd]).float().cuda()
    dx, dgamma, dbeta = F2.BNB.apply(dyt, xt, gt, st, True)
    dx_ref, dgamma_ref, dbeta_ref = R.BNB(dy, x, gamma)
    assert dgamma.shape == gt.shape and dbeta.shape == gt.shape
    assert relerr(dgamma, dgamma_ref) < F32_FROM_BF_TOL and relerr(dbeta, dbeta_ref) < F32_FROM_BF_TOL
    check("BNB", rng, dx, dx_ref, (dyt, xt, gt), (dy, x, gamma))
    dx2, none_g, none_b = F2.BNB.apply(dyt, xt, gt, st, False)             # want_tables=False: the same dx, no table gradient
    assert none_g is None and none_b is None and torch.equal(dx2.detach(), dx.detach())
    check("BNB(want_tables=False)", rng, dx2, R.BNB(dy, x, gamma)[0], (dyt, xt, gt), (dy, x, gamma))


# ------------------------------------------------------------------ penalty, add, fork
@pytest.mark.parametrize("n,d", [(1, 1), (7, 255), (4, 3072)])
def test_gp_loss_function(F2, n, d):
    rng = np.random.default_rng(d)
    g, gt = pair(rng.normal(size=(n, d)) * (1.5 / np.sqrt(d)))
    out, ref = F2.GPLoss.apply(gt, 10.0), R.GPLoss(g, 10.0)
    assert out.dtype == torch.float32
    scale = float(10.0 * ((g.detach().norm(dim=1) + 1.0) ** 2).mean())
    assert abs(float(out) - float(ref)) <= F32_FROM_BF_TOL * scale
    (gd,) = torch.autograd.grad(out, gt, torch.full((1,), -0.75, device="cuda"))
    (gr,) = torch.autograd.grad(ref, g, torch.tensor(-0.75, dtype=F64))
    assert gd.dtype == torch.bfloat16 and relerr(gd, gr) < BF_TOL


def test_add_and_fork_functions(F2):
    rng = np.random.default_rng(11)
    a, at = pair(rng.normal(size=(3, 4, 8, 13)))
    b, bt = pair(rng.normal(size=(3, 4, 8, 13)))
    ct = torch.as_tensor(rng.normal(size=(2, 3, 4, 8, 13)).astype(np.float32)).to(torch.bfloat16).cuda()
    out = F2.AddF.apply(at, bt)
    assert torch.equal(out.detach().cpu(), (a.detach() + b.detach()).to(torch.bfloat16))      # one correctly rounded sum of two
    ga, gb = torch.autograd.grad(out, (at, bt), ct[0])
    assert torch.equal(ga, ct[0]) and torch.equal(gb, ct[0])                                  # AddF backward: copies
    u, v = F2.Fork.apply(at)
    assert torch.equal(u.detach(), at.detach()) and torch.equal(v.detach(), at.detach())
    (g,) = torch.autograd.grad((u, v), at, (ct[0], ct[1]), retain_graph=True)
    assert torch.equal(g.cpu(), (ct[0].double() + ct[1].double()).to(torch.bfloat16).cpu())   # both branches: one sum of two
    (g,) = torch.autograd.grad(u, at, ct[0], retain_graph=True)
    assert torch.equal(g, ct[0])                                                              # one branch: a copy
    (g,) = torch.autograd.grad(v, at, ct[1])
    assert torch.equal(g, ct[1])
    xng = at.detach()
    p, q = F2.fork(xng)
    assert p is xng and q is xng


# ------------------------------------------------------------------ gradient delivery
NAMES = ("w1", "b1", "g", "bt", "w2", "ws", "wl1", "bl1", "wl2", "bl2")
FILL = 0.125


class Critic:
    """conv3x3 + bias -> lrelu -> batch norm -> conv3x3 -> mean pool -> add(1x1 shortcut of the pooled input) -> lrelu -> spatial mean
    -> fork -> two dense heads; loss = gradient_penalty(d sum f / d x) + sum f.  n = 4, 8x8x8 input, 64 channels."""

    def __init__(self, F2):
        self.F2 = F2
        rng = np.random.default_rng(21)
        n, c = 4, 64
        shapes = dict(w1=(3, 3, 8, c), w2=(3, 3, c, c), ws=(1, 1, 8, c), wl1=(c, 1), wl2=(c, 10))
        self.ref, self.dev = {}, {}
        for k, shp in shapes.items():
            self.ref[k], self.dev[k] = pair(rng.normal(size=shp) / np.sqrt(np.prod(shp[:-1])) * 1.5, f32=True)
        for k, shp in dict(b1=(c,), g=(1, c), bt=(1, c), bl1=(1,), bl2=(10,)).items():
            self.ref[k], self.dev[k] = pair(rng.normal(size=shp) * 0.2 + (1.0 if k == "g" else 0.0), f32=True)
        self.x, self.xt = pair(rng.normal(size=(n, 8, 8, 8)))
        xr = self.x
        f1, f2 = self.net(R, self.ref, xr, lambda h, g, b: R.BNF(h, g, b))
        (gx,) = torch.autograd.grad([f1.sum() + f2.sum()], [xr], create_graph=True)
        self.gx_ref = gx.detach()
        loss = R.GPLoss(gx, 10.0) + f1.sum() + f2.sum()
        self.loss_ref = float(loss)
        self.g_ref = dict(zip(NAMES, torch.autograd.grad(loss, [self.ref[k] for k in NAMES])))

    @staticmethod
    def net(M, P, xin, bn):
        """M: functional2 (Function classes) or functional2_ref (float64 functions of the same names)"""
        ap = (lambda f, *a: f.apply(*a)) if M is not R else (lambda f, *a: f(*a))
        xs, xm = ap(M.Fork, xin)
        h = ap(M.ConvF, xm, P["w1"], P["b1"])
        h = ap(M.LRelu, h, 0.2)
        h = bn(h, P["g"], P["bt"])
        h = ap(M.Pool2, ap(M.ConvF, h, P["w2"], None), 0.25)
        h = ap(M.AddF, ap(M.ConvF, ap(M.Pool2, xs, 0.25), P["ws"], None), h)
        h = ap(M.SumHW, ap(M.LRelu, h, 0.2), 1.0 / 16)
        ha, hb = ap(M.Fork, h)
        return ap(M.LinF, ha, P["wl1"], P["bl1"]).reshape(-1), ap(M.LinF, hb, P["wl2"], P["bl2"])

    def params(self):
        return [self.dev[k] for k in NAMES]

    def set_grads(self, value):
        for p in self.params():
            p.grad = None if value is None else torch.full_like(p, value)

    def forward(self, hint=False):
        """-> (loss, the input gradient of the first backward)"""
        F2 = self.F2
        xd = self.xt.detach().clone().requires_grad_(True)
        f1, f2 = self.net(F2, self.dev, xd, lambda h, g, b: F2.BNF.apply(h, g, b)[0])
        with (F2.input_gradient_only() if hint else contextlib.nullcontext()):
            (gx,) = torch.autograd.grad([f1, f2], [xd], [torch.ones_like(f1), torch.ones_like(f2)], create_graph=True)
        return F2.gradient_penalty(gx, 10.0).sum() + f1.float().sum() + f2.float().sum(), gx

    def grads(self, minus=0.0):
        torch.cuda.synchronize()
        return {k: (self.dev[k].grad.detach().clone() - minus) for k in NAMES}

    def accumulated(self, fill=0.0, hint=False):
        """mode (b) / (c): loss.backward() into existing fp32 .grad buffers holding `fill`; -> gradients with the fill taken off"""
        self.set_grads(fill)
        loss, _ = self.forward(hint)
        loss.backward()
        out = self.grads(fill)
        self.set_grads(None)
        return out


@pytest.fixture(scope="module")
def critic(F2):
    c = Critic(F2)
    c.set_grads(None)
    loss, gx = c.forward()
    c.gx_a = gx.detach().clone()
    c.loss_a = float(loss)
    c.g_a = dict(zip(NAMES, torch.autograd.grad(loss, c.params())))         # (a): returned to autograd
    c.g_b = c.accumulated(0.0)                                              # (b): accumulated into zeroed .grad
    return c


def l2(got, ref):
    got, ref = got.detach().to(F64).cpu().flatten(), ref.detach().to(F64).flatten()
    assert bool(torch.isfinite(got).all())
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def cos(got, ref):
    got, ref = got.detach().to(F64).cpu().flatten(), ref.detach().to(F64).flatten()
    return float((got @ ref) / max(float(got.norm() * ref.norm()), 1e-300))


def within(got, ref, tol=F32_FROM_BF_TOL):
    """{name: max |got - ref| / max |ref|}, asserted below tol"""
    errs = {k: relerr(got[k], ref[k].cpu()) for k in NAMES}
    assert all(e < tol for e in errs.values()), errs
    return errs


@pytest.mark.parametrize("mode", ["a", "b"])
def test_delivery_returned_and_accumulated_vs_float64(critic, mode):
    """(a) torch.autograd.grad on parameters without .grad and (b) loss.backward() into zeroed fp32 .grad (the in-place path, with the
    bias sum riding on the filter-gradient launch), each against float64 at the network bounds of
    test_acgan_gpu.py::test_twice_differentiable_operators_vs_autograd: relative L2 <= 8e-2, cosine >= 0.995."""
    assert abs(critic.loss_a - critic.loss_ref) < 3e-2 * max(1.0, abs(critic.loss_ref)), (critic.loss_a, critic.loss_ref)
    assert l2(critic.gx_a, critic.gx_ref) < 5e-2
    got = critic.g_a if mode == "a" else critic.g_b
    errs = {k: (round(l2(got[k], critic.g_ref[k]), 4), round(cos(got[k], critic.g_ref[k]), 5)) for k in NAMES}
    print("delivery", mode, errs)
    assert all(e < 8e-2 and c > 0.995 for e, c in errs.values()), errs


def test_delivery_accumulated_equals_returned(critic):
    """(a) versus (b), per tensor: they differ in fp32 accumulation order only"""
    errs = {k: relerr(critic.g_b[k], critic.g_a[k].cpu()) for k in NAMES}
    print("delivery a-vs-b", {k: "%.2e" % e for k, e in errs.items()})
    assert all(e < F32_FROM_BF_TOL for e in errs.values()), errs      # largest measured: 8.9e-8 (b1, the fused bias sum); 0 elsewhere


def test_delivery_accumulates_onto_existing_values(critic):
    """(c) every .grad pre-filled with 0.125: the result minus the fill equals (b) -- accumulate, not overwrite"""
    within(critic.accumulated(FILL), critic.g_b)


def test_delivery_under_input_gradient_only(critic, monkeypatch):
    """(d) the first backward inside input_gradient_only(): the same input gradient to the bit, no filter / bias gradient launch and no
    change of any .grad during that pass, and the gradients of the following backward() match (b)."""
    F2 = critic.F2
    calls = []
    for name in ("conv2d_wgrad", "colsum"):
        monkeypatch.setattr(F2.K, name, (lambda fn, nm: lambda *a, **k: (calls.append(nm), fn(*a, **k))[1])(getattr(F2.K, name), name))
    lin = F2.K.linear_bwd
    monkeypatch.setattr(F2.K, "linear_bwd", lambda dy, x, w, want_dx=True, dw=None, dbias=None:
                        (calls.append("linear_bwd(dw)") if dw is not None or dbias is not None else None, lin(dy, x, w, want_dx, dw, dbias))[1])
    critic.set_grads(FILL)
    loss, gx = critic.forward(hint=True)
    torch.cuda.synchronize()
    assert calls == [], calls
    assert all(bool((p.grad == FILL).all()) for p in critic.params())
    assert torch.equal(gx.detach(), critic.gx_a)
    loss.backward()
    assert calls, "the differentiated backward computes the filter gradients"
    got = critic.grads(FILL)
    critic.set_grads(None)
    within(got, critic.g_b)


def test_delivery_inside_one_update_with_batched_preparation(critic):
    """(e) inside one_update() after prepare_batched(): both operand layouts equal K.prep_weights' bit for bit, so every gradient is
    bit-identical to (b); after the block a weight rewritten in place is what the next forward uses."""
    F2, K = critic.F2, critic.F2.K
    with F2.one_update():
        F2.prepare_batched(critic.params())
        for k in ("w1", "w2", "ws"):
            w = critic.dev[k]
            wf, wd = K.prep_weights(w.detach(), True, True)
            assert torch.equal(F2._wf(w), wf) and torch.equal(F2._wd(w), wd), k
        got = critic.accumulated(0.0)
    bad = [k for k in NAMES if not torch.equal(got[k], critic.g_b[k])]
    assert not bad, {k: relerr(got[k], critic.g_b[k].cpu()) for k in bad}
    w1, kept = critic.dev["w1"], critic.dev["w1"].detach().clone()
    x = critic.xt.detach()
    try:
        with torch.no_grad():
            before = F2.conv2d(x, w1)
            w1.zero_()
            after = F2.conv2d(x, w1)
            assert float(before.abs().max()) > 0 and float(after.abs().max()) == 0.0       # a stale operand would reproduce `before`
            with F2.one_update():
                F2.prepare_batched(critic.params())
                assert float(F2.conv2d(x, w1).abs().max()) == 0.0
    finally:
        with torch.no_grad():
            w1.copy_(kept)


def test_second_derivative_through_table_or_bias_gradient_raises(F2):
    """(f) dgamma, dbeta and a bias gradient are not differentiable again: NotImplementedError, never a number"""
    rng = np.random.default_rng(31)
    _, xt = pair(rng.normal(size=(6, 4, 4, 8)))
    _, ct = pair(rng.normal(size=(6, 4, 4, 8)))
    _, gt = pair(rng.normal(size=(1, 8)) * 0.3 + 1.0, f32=True)
    _, bt = pair(rng.normal(size=(1, 8)), f32=True)
    for which in (0, 1):
        y, _ = F2.BNF.apply(xt, gt, bt)
        (d,) = torch.autograd.grad(y, (gt, bt)[which], ct, create_graph=True)
        with pytest.raises(NotImplementedError):
            torch.autograd.grad(d.sum(), xt)
    _, Wt = pair(rng.normal(size=(3, 3, 8, 8)) / 8.5, f32=True)
    _, bias = pair(rng.normal(size=8), f32=True)
    (db,) = torch.autograd.grad(F2.ConvF.apply(xt, Wt, bias), bias, ct, create_graph=True)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(db.sum(), ct)
    _, x2 = pair(rng.normal(size=(5, 7)))
    _, c2 = pair(rng.normal(size=(5, 3)))
    _, W2 = pair(rng.normal(size=(7, 3)), f32=True)
    _, b2 = pair(rng.normal(size=3), f32=True)
    (db,) = torch.autograd.grad(F2.LinF.apply(x2, W2, b2), b2, c2, create_graph=True)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(db.sum(), c2)


def test_non_differentiated_grad_call_delivers_into_existing_grad(critic):
    """The module's statement about torch.autograd.grad(create_graph=False) on a parameter that already owns an fp32 .grad: the
    gradient is ADDED to that .grad and the call itself receives None (functional2's docstring, "Gradient delivery")."""
    critic.set_grads(FILL)
    loss, _ = critic.forward()
    got = torch.autograd.grad(loss, critic.params(), allow_unused=True)
    assert all(g is None for g in got)
    delivered = critic.grads(FILL)
    critic.set_grads(None)
    within(delivered, critic.g_b)
