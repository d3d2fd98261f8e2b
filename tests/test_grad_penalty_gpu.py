"""The gradient penalties beside WGAN-GP on a real MI355X: gank_grad_penalty and gank_dragan_perturb through kernels.py against the
float64 restatements of tests/grad_penalty_ref.py (single-launch bounds of tests/test_acgan_ops_gpu.py: fp32 outputs from bf16
operands 2e-3, bf16 outputs 1e-2 of the maximum), functional2.gradient_penalty(kind=...), and ACGANTrainer(penalty=...) against the
float64 critic loss under each penalty, with the bounds of tests/test_acgan_gpu.py."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import grad_penalty_ref as G  # noqa: E402
from oracle import ref_torch as T  # noqa: E402

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


def relerr(got, ref):
    got, ref = got.detach().to(F64).cpu(), ref.detach().to(F64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "non-finite output"
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


# ------------------------------------------------------------------ grad_penalty
KIND_TARGETS = [("two_sided", 1.0), ("two_sided", 0.5), ("one_sided", 1.0), ("one_sided", 0.5), ("squared", 1.0)]
ZERO, ABOVE, BELOW = 1, 2, 4          # the special rows of a batch of 7


def gpen_rows(n, d, seed, target):
    """N rows of D: random ones of norm about 1.5 target, and (as far as N allows) an all-zero row and rows of norm target (1 +- 2^-7)"""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=(n, d)) * (1.5 * target / np.sqrt(d))
    special = {}
    if n >= 5:
        special = {ZERO: 0.0, ABOVE: target * (1.0 + 2.0 ** -7), BELOW: target * (1.0 - 2.0 ** -7)}
    for row, norm in special.items():
        g[row] = g[row] / np.linalg.norm(g[row]) * norm
    return g, special


def check_gpen(K, g, gt, lam, target, kind, special=()):
    """loss at 2e-3 of lam * mean (|g| + target)^2 (squared kind: of lam * mean |g|^2), dgrad at 2e-3 of its maximum and every special row
    on its own maximum; where float64 has a zero row of dgrad the kernel has exact zeros"""
    n = g.shape[0]
    loss_ref, dg_ref = G.grad_penalty_and_derivative(g, lam, target, kind)
    loss, dg = K.grad_penalty(gt, lam, target, kind)
    torch.cuda.synchronize()
    norms = g.reshape(n, -1).norm(dim=1)
    scale = float(lam * (norms ** 2).mean()) if kind == "squared" else float(lam * ((norms + target) ** 2).mean())
    assert loss.shape == (1,) and loss.dtype == torch.float32 and bool(torch.isfinite(loss).all())
    assert abs(float(loss) - float(loss_ref)) <= F32_FROM_BF_TOL * scale, (float(loss), float(loss_ref))
    assert dg.dtype == torch.float32 and dg.shape == gt.shape and relerr(dg, dg_ref) < F32_FROM_BF_TOL
    for row in special:
        if float(dg_ref[row].abs().max()) == 0.0:
            assert bool((dg[row] == 0).all()), row
        else:
            assert relerr(dg[row], dg_ref[row]) < F32_FROM_BF_TOL, row
    return loss, dg, loss_ref, dg_ref


@pytest.mark.parametrize("kind,target", KIND_TARGETS)
@pytest.mark.parametrize("d", [1, 255, 3072, 3 * 4096 + 5])
@pytest.mark.parametrize("n", [1, 7])
def test_grad_penalty_vs_float64(K, n, d, kind, target):
    """gank_grad_penalty against float64 autograd on the bf16-rounded rows.  D = 3072 is the trainer's row (read once into registers,
    384 vectors of 8 on 256 threads), 1 a single element and 255 a ragged tail (both on the looped path: no whole vector), 3 * 4096 + 5
    longer than the resident path holds and ragged.  The batch of 7 holds an all-zero row and rows of norm target (1 +- 2^-7), where
    s - target cancels (two-sided) and where the one-sided kind switches: the row below has dgrad == 0 exactly.  With N = 1 each
    special row is a batch of its own, so its share of the loss is the loss: exactly 0 for the squared kind on the zero row and for
    the one-sided kind on the row below."""
    lam = 10.0
    g, special = gpen_rows(n, d, 10 * n + d, target)
    g, gt = bf(g.reshape(n, d, 1, 1) if d > 1 else g.reshape(n, 1))
    if special:
        norms = g.reshape(n, -1).norm(dim=1)
        assert float(norms[ZERO]) == 0.0 and float(norms[BELOW]) < target < float(norms[ABOVE])      # also after the rounding to bf16
    _, dg, _, _ = check_gpen(K, g, gt, lam, target, kind, special)
    if special and kind == "one_sided":
        assert bool((dg[BELOW] == 0).all()) and bool((dg[ZERO] == 0).all()) and float(dg[ABOVE].abs().max()) > 0.0
    if special and kind == "squared":
        assert bool((dg[ZERO] == 0).all())
    if n == 1:                                                  # the special rows, one at a time
        for which, v in ((ZERO, np.zeros(d)), (ABOVE, np.full(d, target * (1.0 + 2.0 ** -7) / np.sqrt(d))),
                         (BELOW, np.full(d, target * (1.0 - 2.0 ** -7) / np.sqrt(d)))):
            g1, g1t = bf(v.reshape(1, d))
            # (equal elements all round the same way, by at most 2^-9 of the norm: the row stays on its side of the target)
            assert which == ZERO or (float(g1.norm()) < target if which == BELOW else float(g1.norm()) > target)
            loss, dg1, _, _ = check_gpen(K, g1, g1t, lam, target, kind, (0,))
            if which == ZERO:
                assert bool((dg1 == 0).all())
                assert float(loss) == 0.0 if kind == "squared" else np.isfinite(float(loss))
            if which == BELOW and kind == "one_sided":
                assert float(loss) == 0.0 and bool((dg1 == 0).all())


@pytest.mark.parametrize("d", [255, 3072])
def test_grad_penalty_one_sided_batch_below_the_target_is_exactly_zero(K, d):
    rng = np.random.default_rng(d)
    g, gt = bf(rng.normal(size=(7, d)) * (0.8 / np.sqrt(d)))
    assert float(g.norm(dim=1).max()) < 1.0
    loss, dg = K.grad_penalty(gt, 10.0, 1.0, "one_sided")
    torch.cuda.synchronize()
    assert float(loss) == 0.0 and bool((dg == 0).all())
    loss, dg = K.grad_penalty(gt, 10.0, 0.5, "one_sided")        # ... and the same rows over a target of 0.5 are penalised
    assert float(loss) > 0.0 and float(dg.abs().max()) > 0.0


@pytest.mark.parametrize("d", [1, 255, 3072, 3 * 4096 + 5])
def test_grad_penalty_two_sided_target_one_agrees_with_gp_loss(K, d):
    """kind 0 at target 1 states the arithmetic of gank_gp_loss: both within the single-launch bound of each other"""
    g, special = gpen_rows(7, d, 70 + d, 1.0)
    g, gt = bf(g)
    loss, dg = K.grad_penalty(gt, 10.0, 1.0, "two_sided")
    loss0, dg0 = K.gp_loss(gt, 10.0)
    torch.cuda.synchronize()
    scale = float(10.0 * ((g.norm(dim=1) + 1.0) ** 2).mean())
    assert abs(float(loss) - float(loss0)) <= F32_FROM_BF_TOL * scale
    assert relerr(dg, dg0.double().cpu()) < F32_FROM_BF_TOL
    for row in special:
        assert relerr(dg[row], dg0[row].double().cpu()) < F32_FROM_BF_TOL or bool((dg[row] == 0).all() and (dg0[row] == 0).all())


def test_grad_penalty_rejects_an_unknown_kind(K):
    g = torch.ones((2, 8), dtype=torch.bfloat16, device="cuda")
    from gan_lib_tensorflow_amd import _lib
    loss, dg, ws = torch.full((1,), 7.0, device="cuda"), torch.full((2, 8), 7.0, device="cuda"), torch.zeros(2, device="cuda")
    assert K.lib().gank_grad_penalty(g.data_ptr(), loss.data_ptr(), dg.data_ptr(), ws.data_ptr(), 2, 8, 10.0, 1.0, 5, None) != 0
    with pytest.raises(RuntimeError, match="kind 5"):
        _lib.check(1, "grad_penalty")
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and bool((dg == 7.0).all())


@pytest.mark.parametrize("kind,target", [("one_sided", 1.0), ("squared", 1.0), ("two_sided", 0.5)])
def test_gradient_penalty_function_backward_scales_by_upstream(K, kind, target):
    """functional2.GradPenalty.backward: the saved fp32 derivative times an upstream scalar (3.0), rounded once to bf16: 1e-2 of the
    maximum; the zero row stays exactly 0 (test_gp_loss_function_backward_scales_by_upstream is the model)"""
    from gan_lib_tensorflow_amd import functional2 as F2
    g, special = gpen_rows(7, 255, 3, target)
    g, gt = bf(g.reshape(7, 255))
    _, dg_ref = G.grad_penalty_and_derivative(g, 10.0, target, kind)
    gt.requires_grad_(True)
    loss = F2.gradient_penalty(gt, 10.0, kind=kind, target=target)
    (loss * 3.0).sum().backward()
    torch.cuda.synchronize()
    assert gt.grad.dtype == torch.bfloat16 and relerr(gt.grad, 3.0 * dg_ref) < BF_TOL
    assert bool((gt.grad[ZERO] == 0).all())
    if kind == "one_sided":
        assert bool((gt.grad[BELOW] == 0).all())


def test_gradient_penalty_without_new_arguments_is_gploss(K):
    """calls without the new arguments run the code they ran: the GPLoss node on gank_gp_loss, bit for bit"""
    from gan_lib_tensorflow_amd import functional2 as F2
    from gan_lib_tensorflow_amd.common import misc
    g, _ = gpen_rows(7, 3072, 5, 1.0)
    _, gt = bf(g)
    a, b = gt.clone().requires_grad_(True), gt.clone().requires_grad_(True)
    la, lb = F2.gradient_penalty(a, 10.0), misc.gradient_penalty(b, 10.0, kind="two_sided", target=1.0)
    assert type(la.grad_fn).__name__ == type(lb.grad_fn).__name__ == "GPLossBackward"
    assert type(F2.gradient_penalty(a, 10.0, kind="one_sided").grad_fn).__name__ == "GradPenaltyBackward"
    l0, _ = K.gp_loss(gt, 10.0)
    assert torch.equal(la.detach(), l0) and torch.equal(lb.detach(), l0)


# ------------------------------------------------------------------ dragan_perturb
def bf16_ulp(x):
    """the unit in the last place of bf16 (8 significant bits) at |x|"""
    return 2.0 ** (torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


@pytest.mark.parametrize("total", [1, 255, 8 * 3072])
def test_dragan_perturb(K, total):
    """out = real + 0.5 sigma u: u = 0 and a constant real (sigma == 0: the case where E[x^2] - E[x]^2 cancels) return `real` to the
    bit; a random batch is within one bf16 unit in the last place of |real| + 0.5 sigma of the float64 restatement rounded once to
    bf16; two runs give identical bits.  1: a single element; 255: no whole vector; 8 * 3072: the trainer's batch of the tests, six
    partials of 4096."""
    rng = np.random.default_rng(total)
    (r, rt), u = bf(rng.normal(size=total) * 0.5 + 0.1), torch.tensor(rng.uniform(size=total).astype(np.float32))
    ut = u.cuda()
    assert torch.equal(bits(K.dragan_perturb(rt, torch.zeros_like(ut))), bits(rt))
    c, ct = bf(np.full(total, 0.7))
    assert torch.equal(bits(K.dragan_perturb(ct, ut)), bits(ct))
    c, ct = bf(np.full(total, -1.0 / 3.0))
    assert torch.equal(bits(K.dragan_perturb(ct, torch.ones_like(ut))), bits(ct))
    out = K.dragan_perturb(rt, ut)
    out2 = K.dragan_perturb(rt, ut)
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and out.shape == rt.shape and torch.equal(bits(out), bits(out2))
    ref = G.dragan_perturb(r, u.double())
    sigma = float(G.dragan_sigma(r))
    ref_bf = ref.to(torch.bfloat16).to(F64)
    bad = (out.double().cpu() - ref_bf).abs() > bf16_ulp(r.abs() + 0.5 * sigma)
    assert not bool(bad.any()), (int(bad.sum()), torch.nonzero(bad)[:4].tolist())
    if total > 1:
        assert sigma > 0.1 and not torch.equal(bits(out), bits(rt))                   # the perturbation is there


def test_dragan_perturb_rejects_mismatched_u(K):
    r = torch.zeros(64, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="u has 63"):
        K.dragan_perturb(r, torch.zeros(63, device="cuda"))


# ------------------------------------------------------------------ the trainer
BATCH, SEED = 8, 4
LP_OUTPUT_SCALE = 8.0        # D.Output/W of the test state times this for 'wgan-lp': see test_acgan_penalty_losses_and_gradients_vs_oracle


def l2(got, ref):
    got, ref = got.detach().to(F64).cpu().flatten(), ref.detach().to(F64).flatten()
    assert torch.isfinite(got).all()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def cos(got, ref):
    got, ref = got.detach().to(F64).cpu().flatten(), ref.detach().to(F64).flatten()
    return float((got @ ref) / max(float(got.norm() * ref.norm()), 1e-300))


@pytest.fixture(scope="module")
def inputs(K):
    """the explicit inputs of every trainer test here, drawn once: (float64 CPU, device) pairs"""
    rng = np.random.default_rng(BATCH)
    real = bf(np.clip(rng.normal(size=(BATCH, 32, 32, 3)) * 0.5, -1, 1))
    rl = torch.tensor(rng.integers(0, 10, BATCH), dtype=torch.int32)
    z = bf(rng.normal(size=(BATCH, 128)))
    fl = torch.tensor(rng.integers(0, 10, BATCH), dtype=torch.int32)
    alpha = torch.tensor(rng.uniform(size=BATCH), dtype=torch.float32)
    u = torch.tensor(rng.uniform(size=BATCH * 3072), dtype=torch.float32)
    return dict(real=real, rl=rl, z=z, fl=fl, alpha=alpha, u=u, state=T.init_acgan_params(SEED))


def state_for(inputs, penalty):
    state = dict(inputs['state'])
    if penalty == 'wgan-lp':
        state['d_net/D.Output/W'] = state['d_net/D.Output/W'] * np.float32(LP_OUTPUT_SCALE)
    return state


def make(inputs, penalty=None, **kw):
    from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
    if penalty is not None:
        kw['penalty'] = penalty
    return ACGANTrainer(batch_size=BATCH, seed=SEED, state=state_for(inputs, penalty), **kw)


def device_d_loss(tr, inputs, **kw):
    tr.d_flat['grads'].zero_()
    loss = tr.d_loss(inputs['real'][1], inputs['rl'].cuda(), z=inputs['z'][1], fake_labels=inputs['fl'].cuda(), alpha=inputs['alpha'].cuda(),
                     u=inputs['u'].cuda(), **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss


def reference_d_loss(inputs, penalty, weight=10.0, storage=None):
    P = T.to_torch(state_for(inputs, penalty))
    T.STORE = storage
    try:
        loss, parts = G.acgan_d_loss(P, inputs['real'][0], inputs['rl'].long(), inputs['z'][0], inputs['fl'].long(), penalty, weight,
                                     inputs['alpha'].double(), inputs['u'].double())
        dn = T.trainable_names(P, 'd_net')
        grads = dict(zip(dn, torch.autograd.grad(loss, [P[k] for k in dn])))
    finally:
        T.STORE = None
    return loss.detach(), parts, grads


@pytest.mark.parametrize("penalty", ["wgan-lp", "dragan", "r1", "r2"])
def test_acgan_penalty_losses_and_gradients_vs_oracle(K, inputs, penalty, deterministic_stats):
    """ACGANTrainer(penalty=...).d_loss at batch 8 on explicit z, labels, alpha and u against the float64 restatement: the penalty term
    and the total within 3 % of max(1, |ref|); every critic weight gradient at most 1.5 x as far from float64 (relative L2) as the
    restatement's own bf16-storage pass, plus 0.05; conv biases under a batch norm (true gradient exactly zero) at most 2e-3 absolute.
    The absolute limits of test_acgan_losses_and_gradients_vs_oracle (cosine >= 0.975, L2 <= 0.25, measured for WGAN-GP) are applied
    where the kind's own bf16-storage floor, printed below, leaves them room: worst floor L2 <= 0.2 and cosine >= 0.98, that is the
    floor itself is inside the limits with a fifth of the L2 budget to spare.  The floors of the four kinds are L2 0.154-0.173 and
    cosine 0.985-0.988 (a CPU computation; WGAN-GP's own on these inputs 0.158 / 0.988): all four have that room, the test asserts
    that they do, and the absolute limits bind for all four.

    'wgan-lp': at the initial weights every slope at the interpolates is 0.22-0.25 and the one-sided term is identically zero, so
    D.Output/W is scaled by 8 (slopes 1.79-1.96 in float64, all above the target: the term is 7.5); asserted on the reference side.
    The term is steep in the slope there (a slope off by 0.3 % moves it by 1 %), and without `deterministic_stats` the generator's
    batch statistics, summed by float atomics in arrival order, move the fakes and with them the slopes at the interpolates by that
    much from run to run (at scale 6 two runs gave 1.586 and 1.639 against 1.615: most of the 3 % allowed), so the test runs on
    the fixed-order statistics: the bound is for the arithmetic, not for the arrival order.

    Measured on the MI355X (cosine min / L2 max over the critic's tensors, the floor of the same inputs after the bar; penalty term
    device vs float64; largest true-zero bias gradient):
        wgan-lp  0.9840 / 0.179 | 0.9878 / 0.156   term 7.4894 vs 7.5291   biases 3.8e-4
        dragan   0.9836 / 0.181 | 0.9849 / 0.173   term 4.0762 vs 4.0842   biases 5.8e-5
        r1       0.9864 / 0.165 | 0.9882 / 0.154   term 1.3072 vs 1.3016   biases 7.1e-5
        r2       0.9867 / 0.163 | 0.9880 / 0.154   term 0.2240 vs 0.2239   biases 4.2e-5
    All four have room for the absolute limits and hold them; the worst tensors are the batch-norm scales and the 3x3 filters right
    under a batch norm, as for WGAN-GP."""
    loss_ref, parts, gref = reference_d_loss(inputs, penalty)
    _, _, gfloor = reference_d_loss(inputs, penalty, storage=T.bf16_storage)
    if penalty == 'wgan-lp':
        assert int((parts['slopes'] > 1.0).sum()) * 2 >= BATCH, parts['slopes']
    assert float(parts['gp']) > 0.1                              # a vanishing term tests nothing
    tr = make(inputs, penalty, use_graphs=False)
    loss = device_d_loss(tr, inputs)
    gp, gp_ref = float(tr.losses['gradient_penalty']), float(parts['gp'])
    print("acgan", penalty, "d_loss", float(loss), float(loss_ref), "gp", gp, gp_ref)
    assert abs(gp - gp_ref) < 0.03 * max(1.0, gp_ref) and abs(float(loss) - float(loss_ref)) < 0.03 * max(1.0, abs(float(loss_ref)))
    hinge_plus_pen = float(tr.losses['d_loss_gan'])
    assert abs(hinge_plus_pen - float(parts['d_gan'] + parts['gp'])) < 0.03 * max(1.0, float(parts['d_gan'] + parts['gp']))
    dn = list(gref)
    errs = {k: (cos(tr.store.vars[k].grad, gref[k]), l2(tr.store.vars[k].grad, gref[k])) for k in dn}
    floors = {k: (cos(gfloor[k], gref[k]), l2(gfloor[k], gref[k])) for k in dn if float(gref[k].norm()) > 1e-9}
    room = max(f[1] for f in floors.values()) <= 0.2 and min(f[0] for f in floors.values()) >= 0.98
    assert room, "the bf16-storage floor of %s leaves the absolute limits no room any more: decide anew whether they apply" % penalty
    print("acgan", penalty, "D grads:", {k.split('/', 1)[1]: (round(c, 4), round(e, 3)) for k, (c, e) in errs.items()})
    print("acgan", penalty, "bf16-storage floor of the restatement:", {k.split('/', 1)[1]: (round(c, 4), round(e, 3)) for k, (c, e) in floors.items()})
    normed = [k for k in dn if not (k.endswith('.Conv1/Biases') and 'DownBlock.1' not in k)]
    print("acgan", penalty, "summary: device cosine min %.4f L2 max %.3f | floor cosine min %.4f L2 max %.3f | absolute limits %s | biases %.2e" % (
        min(errs[k][0] for k in normed), max(errs[k][1] for k in normed), min(f[0] for f in floors.values()), max(f[1] for f in floors.values()),
        "applied", max(float(tr.store.vars[k].grad.abs().max()) for k in dn if k not in normed)))
    bad = []
    for k, (c, e) in errs.items():
        if k not in normed:
            if float(tr.store.vars[k].grad.abs().max()) > 2e-3:
                bad.append((k, 'abs', float(tr.store.vars[k].grad.abs().max())))
        elif c < 0.975 or e > 0.25:
            bad.append((k, c, e))
        elif e > 1.5 * l2(gfloor[k], gref[k]) + 0.05:
            bad.append((k, 'floor', e, l2(gfloor[k], gref[k])))
    assert not bad, bad


def test_acgan_penalty_none(K, inputs):
    """penalty='none': hinge + class cross-entropy of the restatement (3 % of max(1, |ref|), as above), a zero penalty term, no third
    pass; d_loss(penalise=False) of a penalised trainer is the same form"""
    loss_ref, parts, _ = reference_d_loss(inputs, 'none')
    tr = make(inputs, 'none', use_graphs=False)
    loss = device_d_loss(tr, inputs)
    assert float(tr.losses['gradient_penalty']) == 0.0 and tr.losses['gradient_penalty'].shape == tr.losses['d_loss_gan'].shape
    assert abs(float(loss) - float(parts['d_gan'] + parts['d_ac'])) < 0.03 * max(1.0, abs(float(loss_ref)))
    assert abs(float(tr.losses['d_loss_gan']) - float(parts['d_gan'])) < 0.03 * max(1.0, float(parts['d_gan']))
    tr2 = make(inputs, 'r1', use_graphs=False)
    loss2 = device_d_loss(tr2, inputs, penalise=False)
    assert float(tr2.losses['gradient_penalty']) == 0.0 and abs(float(loss2) - float(loss)) < 0.03 * max(1.0, abs(float(loss_ref)))


def autograd_nodes(loss):
    """the names of every node type in the autograd graph behind `loss`"""
    seen, todo, names = set(), [loss.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names


def test_acgan_default_penalty_is_the_existing_path(K, inputs, deterministic_stats):
    """no new arguments, and penalty='wgan-gp', penalty_weight=10.0, penalty_every=1 spelled out: the same code on the same inputs.
    The route itself: the graph behind the returned loss holds the GPLoss node (gank_gp_loss) and no GradPenalty node, in both.  The
    four loss terms are fixed-order sums behind the fixed-order statistics of `deterministic_stats`: bitwise equal, between two runs of
    the default trainer and between it and the spelled-out one (kind 0 of the new kernel states the same arithmetic in another order
    of summation and would sit about 1e-7 away).  The gradient buffer sums through float atomics in arrival order (the filter
    gradients' split sums, the double-precision sums of gank_bn_bwd_bwd), so one trainer need not repeat it to the bit: where the
    default trainer does, the spelled-out one equals it bitwise; where it does not, the spelled-out one is held to that very noise,
    four times the largest difference between the two runs or, where that is larger, 1e-5 of the buffer's maximum (the last bits of
    float sums in arrival order: 170 units in the last place of fp32 there, and a four-hundredth of the one bf16 unit that another
    operand or another kernel would move it by).  Measured: the gradient buffers 7.5e-8 - 1.1e-7 (run 2 against run 1) and 8.9e-8 -
    1.0e-7 (spelled out against default) apart at a maximum of 0.59, one or two units in the last place."""
    a, b = make(inputs, use_graphs=False), make(inputs, 'wgan-gp', penalty_weight=10.0, penalty_every=1, use_graphs=False)
    assert (a.penalty, a.penalty_weight, a.penalty_every) == (b.penalty, b.penalty_weight, b.penalty_every) == ('wgan-gp', 10.0, 1)
    runs = []
    for tr in (a, a, b):
        loss = device_d_loss(tr, inputs)
        nodes = autograd_nodes(loss)
        assert 'GPLossBackward' in nodes and 'GradPenaltyBackward' not in nodes, sorted(nodes)
        runs.append((dict({k: float(v) for k, v in tr.losses.items()}, d_loss=float(loss)), tr.d_flat['grads'].clone()))
    (t1, g1), (t2, g2), (tb, gb) = runs
    assert set(t1) == set(tb) == {'d_loss', 'd_loss_gan', 'd_loss_acgan', 'gradient_penalty'}
    print("default path: |run2 - run1| max", float((g2 - g1).abs().max()), "|spelled - default| max", float((gb - g1).abs().max()), "of",
          float(g1.abs().max()), "| terms", t1, t2, tb)
    assert t1 == t2 == tb, (t1, t2, tb)
    if torch.equal(g1, g2):
        assert torch.equal(gb, g1)
    else:
        assert float((gb - g1).abs().max()) <= max(4 * float((g2 - g1).abs().max()), 1e-5 * float(g1.abs().max()))
    # ... and the other kinds do leave that route, DRAGAN excepted: its term is the two-sided one at target 1, GPLoss again
    for penalty, node in (('wgan-lp', 'GradPenaltyBackward'), ('r1', 'GradPenaltyBackward'), ('dragan', 'GPLossBackward')):
        nodes = autograd_nodes(make(inputs, penalty, use_graphs=False).d_loss(
            inputs['real'][1], inputs['rl'].cuda(), z=inputs['z'][1], fake_labels=inputs['fl'].cuda(), alpha=inputs['alpha'].cuda(), u=inputs['u'].cuda()))
        assert node in nodes and len(nodes & {'GPLossBackward', 'GradPenaltyBackward'}) == 1, (penalty, sorted(nodes))


def test_acgan_lazy_r1_two_graphs_and_saved_schedule(K, inputs, deterministic_stats):
    """penalty='r1', penalty_every=2 with captured graphs: five critic updates and one generator update.  Exactly the two forms of the
    critic update are captured, 'd' (carries the penalty: updates 0, 2, 4, at weight 2 * penalty_weight) and 'd_plain' (updates 1, 3; the
    generator update has run once, eagerly).  Every update is also run by a trainer with use_graphs=False from the same state and
    seed: before each update the eager trainer takes the captured one's critic weights and RNG state (both have the same generator;
    the loss does not read the optimiser's slots).  No test of this trainer holds eager against captured execution to the bit -- its
    gradients sum through float atomics in arrival order, and left to themselves two trajectories drift apart by 0.1 - 0.5 % of the
    term within four updates (measured; Adam at beta1 = 0 steps every element by about lr whatever its size, so an element at noise
    level may step the other way) -- but from the same weights the loss terms are fixed-order sums behind the fixed-order statistics
    of `deterministic_stats`, and every run so far gave identical bits: the three terms of every update are held bitwise, so that a
    captured form that read a stale buffer shows however small the effect.  The unpenalised
    updates report a zero term in both.  The first penalised update also equals that of a trainer with penalty_every=1 at twice the
    weight.  A trainer rebuilt from `state_dict()` after three updates continues on the schedule: plain, then penalised."""
    from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import synthetic_batches
    tr = make(inputs, 'r1', penalty_weight=5.0, penalty_every=2, use_graphs=True)
    eager = make(inputs, 'r1', penalty_weight=5.0, penalty_every=2, use_graphs=False)
    assert tr.graphs.enabled and not eager.graphs.enabled
    feed = synthetic_batches(BATCH, "cuda", seed=2)
    rows, saved = [], None
    for i in range(5):
        batch = next(feed)
        with torch.no_grad():
            eager.d_flat['params'].copy_(tr.d_flat['params'])
            eager.rng_state.copy_(tr.rng_state)
        tr.d_step(*batch)
        eager.d_step(*batch)
        rows.append(tuple(float(t.losses[k]) for t in (tr, eager) for k in ('gradient_penalty', 'd_loss', 'd_loss_gan')))
        assert all(np.isfinite(v) for v in rows[-1])
        if i == 2:
            saved = tr.state_dict()
    tr.g_step()
    torch.cuda.synchronize()
    assert tr.d_updates == eager.d_updates == 5 and int(tr.d_opt['t']) == 5 and int(tr.g_opt['t']) == 1
    assert set(tr.graphs.graphs) == {'d', 'd_plain'} and not eager.graphs.graphs
    print("lazy r1 (penalty term, d_loss, d_loss_gan) captured | eager:", rows)
    for i, (gp, dl, dg, gp_e, dl_e, dg_e) in enumerate(rows):
        if i % 2:
            assert gp == 0.0 and gp_e == 0.0, (i, gp, gp_e)
        else:
            assert gp > 0.0 and gp == gp_e, (i, gp, gp_e)
        assert dl == dl_e and dg == dg_e, (i, rows[i])
    every1 = make(inputs, 'r1', penalty_weight=10.0, penalty_every=1, use_graphs=False)
    every1.d_step(*next(synthetic_batches(BATCH, "cuda", seed=2)))
    assert float(every1.losses['gradient_penalty']) == rows[0][3]
    # the saved schedule
    assert int(saved['_d_updates']) == 3 and set(saved) - {'_d_updates'} == set(tr.store.vars)
    tr2 = ACGANTrainer(batch_size=BATCH, seed=SEED, state=saved, penalty='r1', penalty_weight=5.0, penalty_every=2, use_graphs=False)
    assert tr2.d_updates == 3
    feed = synthetic_batches(BATCH, "cuda", seed=3)
    tr2.d_step(*next(feed))
    assert float(tr2.losses['gradient_penalty']) == 0.0 and tr2.d_updates == 4
    tr2.d_step(*next(feed))
    assert float(tr2.losses['gradient_penalty']) > 0.0 and tr2.d_updates == 5
    assert int(ACGANTrainer(batch_size=BATCH, seed=SEED, state=inputs['state'], use_graphs=False).state_dict()['_d_updates']) == 0
    # the two captured graphs go here, outside any capture, not whenever a later test's collector pass finds them
    tr.graphs.clear()
    del tr, eager, every1, tr2
    gc.collect()
    torch.cuda.synchronize()
