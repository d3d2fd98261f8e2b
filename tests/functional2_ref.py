"""Plain torch float64 restatements of the forward of every functional2 Function, on NHWC tensors (no GPU import).

Each is built from oracle/ref_torch.py (conv2d_same, meanpool2x2, batch_norm_train, lrelu) and, where the Function is itself
a gradient, from `torch.autograd.grad(..., create_graph=True)`, so every helper stays differentiable: the vector-Jacobian
products the GPU tests compare against are float64 autograd of these.  tests/test_functional2_ref_cpu.py pins the helpers
to independent facts (adjoint identities, the closed forms of the second-order batch norm)."""
import torch

from oracle import ref_torch as T

F64 = torch.float64


def _leaf(shape):
    return torch.zeros(shape, dtype=F64, requires_grad=True)


def ConvF(x, W, b=None):
    return T.conv2d_same(x, W, b)


def ConvD(dy, W):
    """input gradient of conv2d_same (linear in x: taken at x = 0)"""
    x = _leaf(tuple(dy.shape[:3]) + (W.shape[2],))
    (dx,) = torch.autograd.grad(T.conv2d_same(x, W), x, dy, create_graph=True)
    return dx


def ConvW(x, dy, wshape):
    """filter gradient of conv2d_same (linear in W: taken at W = 0)"""
    W = _leaf(tuple(wshape))
    (dw,) = torch.autograd.grad(T.conv2d_same(x, W), W, dy, create_graph=True)
    return dw


def LinF(x, W, b=None):
    y = x @ W
    return y if b is None else y + b


def LinD(dy, W):
    x = _leaf((dy.shape[0], W.shape[0]))
    (dx,) = torch.autograd.grad(x @ W, x, dy, create_graph=True)
    return dx


def LinW(x, dy):
    W = _leaf((x.shape[1], dy.shape[1]))
    (dw,) = torch.autograd.grad(x @ W, W, dy, create_graph=True)
    return dw


def LRelu(x, leak=0.2):
    return T.lrelu(x, leak)


def LReluB(dy, x, leak=0.2):
    xr = x.detach().clone().requires_grad_(True)
    (dx,) = torch.autograd.grad(T.lrelu(xr, leak), xr, dy, create_graph=True)
    return dx


def Pool2(x, scale=0.25):
    return T.meanpool2x2(x) * (4.0 * scale)


def Unpool2(g, scale=0.25):
    n, h, w, c = g.shape
    x = _leaf((n, 2 * h, 2 * w, c))
    (dx,) = torch.autograd.grad(Pool2(x, scale), x, g, create_graph=True)
    return dx


def SumHW(x, scale):
    return x.sum(dim=(1, 2)) * scale


def BcastHW(g, hw, scale):
    x = _leaf((g.shape[0], hw[0], hw[1], g.shape[1]))
    (dx,) = torch.autograd.grad(SumHW(x, scale), x, g, create_graph=True)
    return dx


def BNF(x, gamma, beta):
    return T.batch_norm_train(x, gamma.reshape(-1), beta.reshape(-1))


def BNB(dy, x, gamma):
    """-> (dx, dgamma, dbeta) of train-mode batch norm; differentiable in dy, x and gamma"""
    xr = x if x.requires_grad else x.detach().clone().requires_grad_(True)
    gr = gamma if gamma.requires_grad else gamma.detach().clone().requires_grad_(True)
    beta = _leaf(gr.shape)
    return torch.autograd.grad(BNF(xr, gr, beta), [xr, gr, beta], dy, create_graph=True)


def GPLoss(g, lam=10.0):
    slopes = torch.sqrt((g.reshape(g.shape[0], -1) ** 2).sum(dim=1) + 1e-10)
    return lam * ((slopes - 1.0) ** 2).mean()


def AddF(a, b):
    return a + b


def Fork(x):
    return x, x


def bn_second_order_closed_forms(a, dy, x, gamma, eps=T.BN_EPS):
    """The formulas in the comment that heads csrc/acgan_ops.hip, as written there, in the dtype of the operands:
    a = dL/d(dx) -> (gI = dL/dx, ggO = dL/d(dy), gG = dL/dgamma).  Operands [rows, C] (or NHWC), gamma [C]."""
    c = x.shape[-1]
    a, dy, x = a.reshape(-1, c), dy.reshape(-1, c), x.reshape(-1, c)
    M = x.shape[0]
    mu = x.mean(dim=0)
    d = x - mu
    s = torch.rsqrt((d * d).mean(dim=0) + eps)
    A0, A1, G0, G1, AG = a.sum(0), (a * d).sum(0), dy.sum(0), (dy * d).sum(0), (a * dy).sum(0)
    s2, s3 = s * s, s * s * s
    ggO = gamma * s / M * (M * a - A0 - d * s2 * A1)
    gI = gamma * (d * s3 / M * (A0 * G0 / M - AG + 3 * s2 * G1 * A1 / M) + A1 * s3 / M * (G0 / M - dy) + G1 * s3 / M * (A0 / M - a))
    gG = s * (AG - A0 * G0 / M - s2 * A1 * G1 / M)
    return gI, ggO, gG


def bn_second_order_autograd(a, dy, x, gamma):
    """float64 autograd of BNB's dx: the reference the closed forms and the kernel are held to"""
    xr, dyr, gr = (t.detach().clone().requires_grad_(True) for t in (x, dy, gamma))
    dx, _, _ = BNB(dyr, xr, gr)
    return torch.autograd.grad(dx, [xr, dyr, gr], a)
