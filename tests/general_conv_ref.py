"""float64 reference, per-element error bound and case table of the general convolution
(gank_conv2d_general_fprop / _dgrad / _wgrad, functional.conv2d_general).

The operation is the plain gather

    y[n, oy, ox, :] = b + sum_{a, b < k}  x'[n, oy*s + a - pad, ox*s + b - pad, :] @ w[a, b]

with x' the stored input after the fused relu and the nearest-neighbour 2x upsample, and every tap outside x' read as zero (so
the trailing pad is implied by the output size).  The functions below loop over the k*k taps and treat all pixels of a tap as
one matrix product; they are written on torch tensors and follow the dtype of their operands, so the CPU test can run the very
same code in fp32 as a stand-in kernel.

ERROR BOUND (derived, not tuned).  u = 2^-24 is the fp32 unit roundoff; a bf16 store rounds by at most 2^-9 relative
(round-to-nearest), 2^-8 if it truncates.  Every allowance carries that factor 2.

  bf16 results (y, dx):   |got - ref| <= 2^-8 |ref| + K 2^-23 A
      K = length of the dot product (k*k*Cin for y, k*k*Cout for dx), A = the same sum taken over magnitudes
      (sum |x'| |w| + |b|).  The second term is the any-order fp32 accumulation bound K u A, doubled; the doubling also pays
      for the bias add (one more term) and for the second-order product of the two terms.
  fp32 results (dw, db):  |got - ref| <= M 2^-23 A + 2^-23 |initial|
      M = N*Hdy*Wdy pixels summed, A = sum |x'| |dy| (sum |dy| for db), initial = what the accumulated-into buffer held.

Roundings per route (one 2^-8 term for each bf16 store a value passes through, applied to the float64 magnitude of the value
stored there):
  general gather, fprop and stride-1 dgrad ......... 1: the result.
  upsampled-input dx (functional level) ............ 2: the gradient at the upsampled size, then its 2x2 sum (4 fp32 adds).
  few-output route (Cout <= 4 behind an upsample) .. y:  the tap partials Z (one 1x1 conv result per tap), then y.
                                                     dx: the gathered gradient `col` of Z (<= 4 fp32 adds), then dx.
                                                     dw: `col` (bf16) feeds an fp32 1x1 filter gradient.
  phase-stacked route (>= PHASE_STACK_MIN_PIXELS) .. y, dx: the stacked 3x3 filter holds SUMS of taps of w, rounded to bf16
                                                     once more (|sum w| <= sum |w|, so the term is 2^-8 A), then the result.
  stride-2 dx (transposed conv by phase) ........... 1: the result (the phase filters are single taps of w).
out_tanh results are not given a derived bound (the kernel's tanh has no stated accuracy): callers keep max-relative 1e-2."""
import functools

import torch

U8, U23 = 2.0 ** -8, 2.0 ** -23


# ----------------------------------------------------------------------------------------------------------- the gather
def prepare(x, up=False, relu=False):
    """x' : the stored input after the fused relu and NN-upsample"""
    if relu:
        x = torch.relu(x)
    if up:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return x


def _span(a, s, pad, nin, nout):
    """outputs [lo, hi) whose tap `a` reads an in-image index o*s + a - pad, and the index the first of them reads"""
    lo = max(0, -((a - pad) // s))
    hi = min(nout, (nin - 1 + pad - a) // s + 1)
    return lo, hi, lo * s + a - pad


def _taps(k, s, pad, in_hw, out_hw):
    for a in range(k):
        y0, y1, iy = _span(a, s, pad, in_hw[0], out_hw[0])
        if y1 <= y0:
            continue
        for b in range(k):
            x0, x1, ix = _span(b, s, pad, in_hw[1], out_hw[1])
            if x1 > x0:
                yield a, b, slice(y0, y1), slice(x0, x1), slice(iy, iy + (y1 - y0 - 1) * s + 1, s), slice(ix, ix + (x1 - x0 - 1) * s + 1, s)


def gather(xp, w, stride, pad, out_hw, per_tap_abs=False):
    """sum over taps of x'[tap window] @ w[tap]; per_tap_abs: sum of the magnitudes of the per-tap partial results"""
    n, h, wd, _ = xp.shape
    y = xp.new_zeros((n, out_hw[0], out_hw[1], w.shape[3]))
    for a, b, oy, ox, iy, ix in _taps(w.shape[0], stride, pad, (h, wd), out_hw):
        t = xp[:, iy, ix, :] @ w[a, b]
        y[:, oy, ox, :] += t.abs() if per_tap_abs else t
    return y


def scatter(dy, w, stride, pad, in_hw):
    """adjoint of gather in x': gx'[n, iy, ix, :] = sum dy[n, oy, ox, :] @ w[a, b]^T over the taps that read (iy, ix)"""
    n, oh, ow, _ = dy.shape
    g = dy.new_zeros((n, in_hw[0], in_hw[1], w.shape[2]))
    for a, b, oy, ox, iy, ix in _taps(w.shape[0], stride, pad, in_hw, (oh, ow)):
        g[:, iy, ix, :] += dy[:, oy, ox, :] @ w[a, b].t()
    return g


def pool_sum(g):
    n, h, w, c = g.shape
    return g.reshape(n, h // 2, 2, w // 2, 2, c).sum(dim=(2, 4))


def fprop(x, w, b, stride, pad, out_hw, up=False, relu=False, tanh=False):
    y = gather(prepare(x, up, relu), w, stride, pad, out_hw)
    if b is not None:
        y = y + b
    return torch.tanh(y) if tanh else y


def dx_gathered(w, dy, stride, pad, in_hw):
    """gradient in x' (the upsampled size for an upsampled-input conv), before any relu mask"""
    return scatter(dy, w, stride, pad, in_hw)


def dx(x, w, dy, stride, pad, up=False, relu=False):
    """gradient in the stored x"""
    n, h, wd, _ = x.shape
    g = scatter(dy, w, stride, pad, (2 * h, 2 * wd) if up else (h, wd))
    if up:
        g = pool_sum(g)
    return g * (x > 0).to(g.dtype) if relu else g


def dw(x, dy, k, stride, pad, up=False, relu=False):
    xp = prepare(x, up, relu)
    n, h, wd, cin = xp.shape
    out = xp.new_zeros((k, k, cin, dy.shape[3]))
    for a, b, oy, ox, iy, ix in _taps(k, stride, pad, (h, wd), dy.shape[1:3]):
        out[a, b] = xp[:, iy, ix, :].reshape(-1, cin).t() @ dy[:, oy, ox, :].reshape(-1, dy.shape[3])
    return out


def db(dy):
    return dy.sum(dim=(0, 1, 2))


# magnitude sums A: the same functions on |x'|, |w|, |b|, |dy|
def fprop_abs(x, w, b, stride, pad, out_hw, up=False, relu=False):
    return fprop(prepare(x, up, relu).abs(), w.abs(), None if b is None else b.abs(), stride, pad, out_hw)


def dx_gathered_abs(w, dy, stride, pad, in_hw):
    return scatter(dy.abs(), w.abs(), stride, pad, in_hw)


def dw_abs(x, dy, k, stride, pad, up=False, relu=False):
    return dw(prepare(x, up, relu).abs(), dy.abs(), k, stride, pad)


def db_abs(dy):
    return dy.abs().sum(dim=(0, 1, 2))


# ------------------------------------------------------------------------------------------------------------ the bound
def bound_bf16(ref, A, K, extra=None):
    """one bf16 store behind a K-term fp32 dot product; extra: the allowances of earlier stores on the way"""
    t = U8 * ref.abs() + K * U23 * A
    return t if extra is None else t + extra


def bound_f32(A, M, initial=None):
    t = M * U23 * A
    return t if initial is None else t + U23 * initial.abs()


def bound_dx_pooled(x, w, dy, pad, relu=False):
    """dx of an upsampled-input conv as functional computes it: bf16 gradient at the upsampled size, 2x2 sum, bf16, relu mask"""
    n, h, wd, _ = x.shape
    K = w.shape[0] ** 2 * w.shape[3]
    g = dx_gathered(w, dy, 1, pad, (2 * h, 2 * wd))
    first = bound_bf16(g, dx_gathered_abs(w, dy, 1, pad, (2 * h, 2 * wd)), K)
    ref = pool_sum(g)
    t = U8 * ref.abs() + pool_sum(first) + 4 * U23 * pool_sum(g.abs())
    return t * (x > 0).to(t.dtype) if relu else t


def few_route(x, w, b, dy, pad, relu=False):
    """references and allowances of the few-output route (upsampled input, out == 2*in): tap partials Z = 1x1 conv at the low
    resolution (bf16), y = bias + the taps gathered; backward through col = the gathered gradient of Z (bf16)"""
    k, _, cin, cout = w.shape
    n, h, wd, _ = x.shape
    out_hw, M = (2 * h, 2 * wd), n * 4 * h * wd
    xp = prepare(x, True, relu)
    xl = prepare(x, False, relu)
    y = fprop(x, w, b, 1, pad, out_hw, True, relu)
    zabs = gather(xp, w, 1, pad, out_hw, per_tap_abs=True) + (0 if b is None else b.abs())
    r = dict(y=y, y_bound=bound_bf16(y, fprop_abs(x, w, b, 1, pad, out_hw, True, relu), k * k * cin, (U8 + (k * k + 1) * U23) * zabs))
    dw_extra = torch.zeros_like(w)
    dx_extra = torch.zeros_like(x)
    for a, bb, oy, ox, iy, ix in _taps(k, 1, pad, out_hw, out_hw):
        G = torch.zeros_like(dy)
        G[:, iy, ix, :] = dy[:, oy, ox, :]
        ecol = U8 * pool_sum(G).abs() + 4 * U23 * pool_sum(G.abs())              # allowance of col[tap]
        dw_extra[a, bb] = xl.abs().reshape(-1, cin).t() @ ecol.reshape(-1, cout)
        dx_extra += ecol @ w[a, bb].abs().t()
    mask = (x > 0).to(torch.float64) if relu else 1.0
    r["dx"] = dx(x, w, dy, 1, pad, True, relu)
    r["dx_bound"] = (U8 * r["dx"].abs() + k * k * cout * U23 * pool_sum(dx_gathered_abs(w, dy, 1, pad, out_hw)) + dx_extra) * mask
    r["dw"] = dw(x, dy, k, 1, pad, True, relu)
    r["dw_bound"] = bound_f32(dw_abs(x, dy, k, 1, pad, True, relu), M) + dw_extra
    r["db"], r["db_bound"] = db(dy), bound_f32(db_abs(dy), M)
    return r


def general_route(x, w, b, dy, stride, pad, out_hw, up=False, relu=False, stacked=False):
    """references and allowances of conv2d_general through autograd from zero gradients.  stacked: the phase-stacked form,
    whose 3x3 filter holds sums of taps of w rounded to bf16 once more (allowance 2^-8 A on y and dx) and whose dx is one
    bf16 store at the low resolution"""
    k, _, cin, cout = w.shape
    n, h, wd, _ = x.shape
    M = n * out_hw[0] * out_hw[1]
    gh, gw = (2 * h, 2 * wd) if up else (h, wd)
    y = fprop(x, w, b, stride, pad, out_hw, up, relu)
    A = fprop_abs(x, w, b, stride, pad, out_hw, up, relu)
    r = dict(y=y, y_bound=bound_bf16(y, A, k * k * cin, U8 * A if stacked else None))
    r["dx"] = dx(x, w, dy, stride, pad, up, relu)
    mask = (x > 0).to(torch.float64) if relu else 1.0
    if stacked:
        Ad = pool_sum(dx_gathered_abs(w, dy, 1, pad, (gh, gw)))
        r["dx_bound"] = bound_bf16(r["dx"], Ad, 36 * cout, U8 * Ad) * mask
    elif up:
        r["dx_bound"] = bound_dx_pooled(x, w, dy, pad, relu)
    else:
        r["dx_bound"] = bound_bf16(r["dx"], dx_gathered_abs(w, dy, stride, pad, (gh, gw)), k * k * cout) * mask
    r["dw"] = dw(x, dy, k, stride, pad, up, relu)
    r["dw_bound"] = bound_f32(dw_abs(x, dy, k, stride, pad, up, relu), M)
    r["db"], r["db_bound"] = db(dy), bound_f32(db_abs(dy), M)
    return r


def within(got, ref, bnd):
    """(ok, worst ratio, index of the worst element); a non-finite value is never inside"""
    got = torch.as_tensor(got).detach().to(torch.float64).cpu()
    err = (got - ref).abs()
    bad = ~torch.isfinite(got) | (err > bnd)
    ratio = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    i = int(ratio.argmax())
    return not bool(bad.any()), float(ratio.flatten()[i]), tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))


# ------------------------------------------------------------------------------------------------------------ the cases
def same_pad(n_in, k, s):
    """TF SAME: (output size, leading pad) -- the smaller half of the total pad goes in front"""
    o = -(-n_in // s)
    return o, max((o - 1) * s + k - n_in, 0) // 2


def _build_cases():
    C = []

    def add(tag, n, hin, win, cin, cout, k, stride, pad, hout, wout, up=False, relu=False):
        assert 0 <= pad < k and hout > 0 and wout > 0 and not (up and stride == 2)
        row = (n, hin, win, cin, cout, k, stride, pad, hout, wout, up, relu)
        if row not in [r for _, r in C]:
            C.append((tag, row))

    # every filter size at stride 1 on a non-square 5x9 input: VALID (pad 0), SAME ((k-1)//2) and FULL (k-1) windows
    for k in range(1, 8):
        for j, pad in enumerate((0, (k - 1) // 2, k - 1)):
            if j == 0:
                ho, wo = max(5 - k + 1, 1), max(9 - k + 1, 1)       # VALID where the filter fits; one row / column where it does not
            elif j == 1:
                ho, wo = 5, 9
            else:
                ho, wo = 5 + k - 1, 9 + k - 1
            add("k", 2, 5, 9, 64, 32, k, 1, pad, ho, wo, relu=(k + j) % 2 == 1)
    # ragged Cout: the 32-, 64- and 128-wide tile routes and their ragged last tiles; M = 126 is ragged on every pixel tile
    for cout in (1, 3, 33, 64, 96, 128, 160):
        add("cout", 3, 6, 7, 64, cout, 4, 1, 1, 6, 7)
    add("cout", 3, 6, 7, 64, 3, 2, 1, 0, 6, 7)                      # taps * Cout <= 32: the packed narrow-dy filter gradient
    add("cout", 3, 6, 7, 128, 160, 3, 1, 2, 8, 9, relu=True)
    # either side of T128_MIN = 192 pixel tiles of 128 at Cout = 128 (conv_igemm.hip): 191 tiles run 64x64, 192 run 128x128
    add("t128", 1, 128, 191, 64, 128, 2, 1, 0, 128, 191)
    add("t128", 3, 64, 128, 64, 128, 2, 1, 0, 64, 128)
    # packed K (Cin % 64 != 0): an 8-element chunk spans several taps; the packed kernel takes stride / upsample / relu at run time
    for cin in (1, 3, 5, 6, 8, 12, 63, 65, 72):
        add("packed", 2, 5, 6, cin, 32, 2, 1, 0, 10, 12, up=True, relu=True)
        add("packed", 2, 5, 6, cin, 64, 4, 2, 1, 3, 3)
        add("packed", 2, 5, 6, cin, 32, 7, 1, 3, 5, 6, relu=cin % 2 == 1)
    add("packed", 2, 4, 4, 513, 32, 4, 1, 1, 4, 4)
    # Cin = 3, k = 3, Cout % 128 == 0 off the SAME pad: the streaming 3-channel filter-gradient kernel (pad fixed at 1) used to take
    # pads 0 and 2 as well
    add("packed", 2, 5, 9, 3, 128, 3, 1, 0, 5, 9)
    add("packed", 2, 5, 9, 3, 128, 3, 1, 1, 5, 9)
    add("packed", 2, 5, 9, 3, 128, 3, 1, 2, 5, 9)
    # stride 2: TF SAME, VALID behind pad_input 0 / 1, and k-1 in front, on even, odd, one-pixel and non-square inputs
    for k in (2, 3, 4, 5, 7):
        for hin, win in ((1, 1), (2, 3), (7, 12), (15, 15), (16, 9)):
            n = 1 if (hin, win) == (15, 15) else 2
            (oh, ph), (ow, pw) = same_pad(hin, k, 2), same_pad(win, k, 2)
            if ph == pw:                                            # (one pad for both axes is all the entry points take)
                add("s2", n, hin, win, 64, 64, k, 2, ph, oh, ow)
            for p in (0, 1):
                if p < k and hin + 2 * p >= k and win + 2 * p >= k:
                    add("s2", n, hin, win, 64, 64, k, 2, p, (hin + 2 * p - k) // 2 + 1, (win + 2 * p - k) // 2 + 1, relu=p == 1)
            add("s2", n, hin, win, 64, 64, k, 2, k - 1, (hin + k - 2) // 2 + 1, (win + k - 2) // 2 + 1)
    # upsampled input: out == 2*in, then out < 2*in (the window stops short of the upsampled image).  With a power-of-two dy grid,
    # M % 64 == 0, Cin, Cout >= 64 and no relu the out < 2*in rows used to reach the lean filter-gradient kernel, which bounds its
    # taps by dy's grid: every tap reading rows / columns >= Hdy of x' was dropped (dw off by 1e4 allowances).  The dispatcher
    # now keeps them on the per-tap kernel; the 5x5 -> 10 -> 8 row (M = 64) is the smallest that showed it.
    add("up", 2, 4, 5, 64, 64, 4, 1, 1, 8, 10, up=True, relu=True)
    add("up", 2, 4, 4, 64, 64, 2, 1, 0, 8, 8, up=True)
    add("up", 1, 9, 9, 64, 64, 3, 1, 0, 16, 16, up=True)            # k = 3 VALID: 18 -> 16
    add("up", 1, 10, 10, 64, 64, 5, 1, 0, 16, 16, up=True)          # k = 5 VALID: 20 -> 16, taps reach rows / columns 16..19 of x'
    add("up", 1, 5, 5, 64, 64, 3, 1, 1, 8, 8, up=True)              # pad 1 in front, 10 -> 8
    add("up", 1, 10, 10, 128, 128, 5, 1, 0, 16, 16, up=True)        # the same on 128-wide tiles
    add("up", 3, 5, 7, 64, 64, 3, 1, 0, 8, 12, up=True, relu=True)  # M = 288 ragged
    add("up", 1, 10, 10, 64, 64, 5, 1, 0, 16, 16, up=True, relu=True)
    # lean filter-gradient entry (power-of-two output grid, M % 64 == 0, Cin, Cout >= 64) and its M % 64 != 0 complements
    add("lean", 1, 8, 8, 64, 64, 4, 1, 1, 8, 8)
    add("lean", 1, 8, 8, 64, 64, 2, 1, 0, 8, 8, relu=True)
    add("lean", 1, 8, 8, 128, 128, 2, 1, 0, 8, 8)
    add("lean", 1, 4, 4, 64, 64, 4, 1, 1, 4, 4)
    add("lean", 1, 4, 4, 64, 64, 2, 1, 0, 4, 4, relu=True)
    add("lean", 3, 7, 7, 64, 64, 4, 2, 1, 4, 4)                     # stride 2 from an odd input, M = 48
    add("lean", 1, 15, 15, 128, 128, 4, 2, 1, 8, 8, relu=True)
    add("lean", 1, 9, 9, 64, 64, 4, 1, 1, 8, 8)                     # power-of-two dy grid but x on another grid: must stay off the lean kernel
    # 3x3, pad 1, stride 1 on a power-of-two dy grid through the general entry: the geometry tests of the filter-row (M < 16384)
    # and all-taps (M >= 16384) filter-gradient kernels, with x on dy's grid and off it (the all-taps kernel indexes x by dy's
    # pitch and used to be entered without that test: the two off-grid rows at n = 256 are the smallest that reach it)
    add("rows", 1, 8, 8, 64, 64, 3, 1, 1, 8, 8)
    add("rows", 1, 9, 10, 64, 64, 3, 1, 1, 8, 8)
    add("taps", 256, 8, 8, 64, 64, 3, 1, 1, 8, 8)
    add("taps", 256, 9, 9, 64, 64, 3, 1, 1, 8, 8)
    add("taps", 256, 5, 5, 64, 64, 3, 1, 1, 8, 8, up=True)          # 10 -> 8 behind the upsample
    return C


_TAGGED = _build_cases()
CASES = [row for _, row in _TAGGED]


def case_id(i):
    n, hin, win, cin, cout, k, s, pad, ho, wo, up, relu = CASES[i]
    return f"{i}-{_TAGGED[i][0]}-n{n}-{hin}x{win}x{cin}-k{k}s{s}p{pad}-{ho}x{wo}x{cout}" + ("-up" if up else "") + ("-relu" if relu else "")


def find_case(**want):
    """index of the first case whose named fields have the given values"""
    names = ("n", "hin", "win", "cin", "cout", "k", "stride", "pad", "hout", "wout", "up", "relu")
    for i, row in enumerate(CASES):
        if all(row[names.index(f)] == v for f, v in want.items()):
            return i
    raise KeyError(want)


def bf16(t):
    """fp32 draw -> nearest bf16, returned as float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def draw(shape_x, shape_w, shape_dy, seed):
    """operands as everywhere in the suite: drawn in fp32, x / w / dy rounded to bf16 first; the bias and the initial
    contents of dw / db stay fp32 (the kernels read them as fp32)"""
    g = torch.Generator().manual_seed(seed)
    k, _, cin, cout = shape_w
    x = bf16(torch.randn(shape_x, generator=g))
    w = bf16(torch.randn(shape_w, generator=g) / (k * k * cin) ** 0.5)
    b = torch.randn(cout, generator=g).to(torch.float64)
    dy = bf16(torch.randn(shape_dy, generator=g))
    dw0 = torch.randn(shape_w, generator=g).to(torch.float64)
    db0 = torch.randn(cout, generator=g).to(torch.float64)
    return x, w, b, dy, dw0, db0


@functools.lru_cache(maxsize=None)
def reference(i):
    """operands, float64 results and allowances of case i (computed once per process; treat as read-only)"""
    n, hin, win, cin, cout, k, s, pad, ho, wo, up, relu = CASES[i]
    x, w, b, dy, dw0, db0 = draw((n, hin, win, cin), (k, k, cin, cout), (n, ho, wo, cout), 1000 + i)
    gh, gw = (2 * hin, 2 * win) if up else (hin, win)
    M = n * ho * wo
    r = dict(case=CASES[i], x=x, w=w, b=b, dy=dy, dw0=dw0, db0=db0, M=M, gathered_hw=(gh, gw))
    r["y"] = fprop(x, w, b, s, pad, (ho, wo), up, relu)
    r["y_bound"] = bound_bf16(r["y"], fprop_abs(x, w, b, s, pad, (ho, wo), up, relu), k * k * cin)
    r["dw"] = dw0 + dw(x, dy, k, s, pad, up, relu)
    r["dw_sum"] = r["dw"] - dw0
    r["dw_A"] = dw_abs(x, dy, k, s, pad, up, relu)
    r["dw_bound"] = bound_f32(r["dw_A"], M, dw0)
    r["db"] = db0 + db(dy)
    r["db_A"] = db_abs(dy)
    r["db_bound"] = bound_f32(r["db_A"], M, db0)
    # gradient at the gathered size (what gank_conv2d_general_dgrad returns), masked by relu only where x' is the stored x
    g = dx_gathered(w, dy, s, pad, (gh, gw))
    gb = bound_bf16(g, dx_gathered_abs(w, dy, s, pad, (gh, gw)), k * k * cout)
    if relu and not up:
        mask = (x > 0).to(torch.float64)
        g, gb = g * mask, gb * mask
    r["dxg"], r["dxg_bound"] = g, gb
    r["dx"] = dx(x, w, dy, s, pad, up, relu)
    r["dx_bound"] = bound_dx_pooled(x, w, dy, pad, relu) if up else gb
    return r
