"""Consistency regularisation (CR / bCR) on a real MI355X: gank_cr_draw, gank_cr_augment and gank_consistency_loss through kernels.py
against the host restatements of tests/consistency_ref.py (the draw and the gather exactly, the loss within the bound derived from the
kernel's order of summation), functional2.consistency_loss, and ACGANTrainer(consistency=...) against the float64 critic loss with the
limits of tests/test_grad_penalty_gpu.py."""
import collections
import gc
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consistency_ref as R  # noqa: E402
from oracle import ref_torch as T  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = torch.float64
SEED, OFF = 0x1234_5678_9ABC_DEF0, 11          # the state of the draw tests (tests/test_consistency_cpu.py checks the 18 outcomes for it)
U = 2.0 ** -24


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


# ------------------------------------------------------------------ cr_augment
def bf16_ramp(shape):
    """consecutive bfloat16 values from 2^-95 up, one per element: all distinct, so a wrong index cannot coincide -> (bits int16
    ndarray, bf16 cuda tensor)"""
    n = int(np.prod(shape))
    assert n < 0x6000
    bits = (np.arange(n, dtype=np.int32) + 0x1000).astype(np.int16).reshape(shape)
    return bits, torch.from_numpy(bits).view(torch.bfloat16).cuda()


@pytest.mark.parametrize("shape", [(1, 32, 32, 3), (3, 32, 32, 3), (2, 8, 8, 3), (2, 5, 7, 4)])
def test_cr_augment_is_the_gather_bit_for_bit(K, shape):
    """every flip x dx x dy of {-s, -1, 0, 1, s}^2 for s = 4 and s = min(H, W) - 1, dealt over the images of the batch, against the NumPy
    gather on the bit patterns.  32 x 32 x 3 and 8 x 8 x 3 take the kernel's 16-byte pieces (W C a multiple of 8; 3 x 32 x 32 x 3 more
    than one block a image and more than one image), 5 x 7 x 4 the one-element pieces (odd, not square, C != 3)."""
    b, h, w, _ = shape
    bits, xt = bf16_ramp(shape)
    for s in sorted({min(4, min(h, w) - 1), min(h, w) - 1}):
        combos = [(f, dx, dy) for f in (0, 1) for dx, dy in itertools.product(sorted({-s, -1, 0, 1, s}), repeat=2)]
        assert len(combos) == 2 * len({-s, -1, 0, 1, s}) ** 2
        for i in range(0, len(combos), b):
            table = np.array([combos[(i + j) % len(combos)] for j in range(b)], np.int32)
            out = K.cr_augment(xt, torch.from_numpy(table).cuda(), s)
            assert out.dtype == torch.bfloat16 and out.shape == xt.shape and out.data_ptr() != xt.data_ptr()
            got = out.cpu().view(torch.int16).numpy()
            assert np.array_equal(got, R.augment(bits, table)), (s, table.tolist())
    # the default bound admits every shift the reflection is defined for
    s = min(h, w) - 1
    table = np.tile(np.array([[1, -s, s]], np.int32), (b, 1))
    assert np.array_equal(K.cr_augment(xt, torch.from_numpy(table).cuda()).cpu().view(torch.int16).numpy(), R.augment(bits, table))


def test_cr_augment_rejects(K):
    """a table of the wrong shape or dtype and a shift >= min(H, W) raise ValueError before any launch; the C entry point refuses the
    shift too"""
    from gan_lib_tensorflow_amd import _lib
    from gan_lib_tensorflow_amd.common import misc
    x = torch.zeros((2, 5, 7, 4), dtype=torch.bfloat16, device="cuda")
    good = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    for table, match in ((torch.zeros((3, 3), dtype=torch.int32, device="cuda"), "table has shape"),
                         (torch.zeros((2, 2), dtype=torch.int32, device="cuda"), "table has shape"),
                         (torch.zeros(6, dtype=torch.int32, device="cuda"), "table has shape"),
                         (torch.zeros((2, 3), dtype=torch.int64, device="cuda"), "int32"),
                         (torch.zeros((2, 3), dtype=torch.float32, device="cuda"), "int32")):
        with pytest.raises(ValueError, match=match):
            K.cr_augment(x, table)
    for s in (5, 7, 100, -1, 2.5):
        with pytest.raises(ValueError, match="below min"):
            K.cr_augment(x, good, s)
    with pytest.raises(ValueError, match="below min"):
        misc.augment(x, good, 5)
    with pytest.raises(ValueError, match="NHWC"):
        K.cr_augment(x.reshape(2, 5, 28), good)
    out = torch.full_like(x, 7.0)
    assert K.lib().gank_cr_augment(x.data_ptr(), good.data_ptr(), out.data_ptr(), 2, 5, 7, 4, 5, None) != 0
    with pytest.raises(RuntimeError, match="shift 5 on 5 x 7"):
        _lib.check(1, "cr_augment")
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert torch.equal(K.cr_augment(x, good, 4), x)                 # ... and the largest shift that is defined passes


# ------------------------------------------------------------------ cr_draw
def state(off=OFF):
    return torch.tensor([SEED, off], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("s", [1, 4])
@pytest.mark.parametrize("n", [1, 7, 64])
def test_cr_draw_equals_the_host_philox_restatement(K, n, s):
    """the table to the integer, the state one draw further (DRAW_ADVANCE = 1: one Philox call of four words a row, three used), and
    the next draw is the restatement at that offset: another table"""
    st = state()
    first, second = K.cr_draw(n, s, st), K.cr_draw(n, s, st)
    torch.cuda.synchronize()
    assert first.dtype == torch.int32 and first.shape == (n, 3)
    assert st.tolist() == [SEED, OFF + 2 * R.DRAW_ADVANCE]
    assert np.array_equal(first.cpu().numpy(), R.draw_table(n, s, SEED, OFF))
    assert np.array_equal(second.cpu().numpy(), R.draw_table(n, s, SEED, OFF + R.DRAW_ADVANCE))
    assert not torch.equal(first, second)


def test_cr_draw_4096_rows_hold_every_outcome(K):
    """more rows than one pass of the block's 256 threads; all 2 (2 s + 1)^2 = 18 outcomes of s = 1 occur (the restatement's do: CPU test)"""
    st = state()
    t = K.cr_draw(4096, 1, st).cpu().numpy()
    assert np.array_equal(t, R.draw_table(4096, 1, SEED, OFF)) and st.tolist() == [SEED, OFF + 1]
    assert len({tuple(r) for r in t.tolist()}) == 18
    assert bool((K.cr_draw(5, 0, st)[:, 1:] == 0).all())            # no shift: flips alone
    for bad in (dict(n=0, shift=1), dict(n=4, shift=-1), dict(n=4, shift=1.5), dict(n=2.5, shift=1)):
        with pytest.raises(ValueError, match="cr_draw"):
            K.cr_draw(bad['n'], bad['shift'], st)
    assert st.tolist() == [SEED, OFF + 2]


# ------------------------------------------------------------------ consistency_loss
@pytest.mark.parametrize("b,c", [(1, 1), (8, 1), (64, 1), (7, 10), (64, 10)])
def test_consistency_loss_vs_float64(K, b, c):
    """gank_consistency_loss against float64 on the same fp32 inputs.  The bounds follow from the kernel's arithmetic, not from its
    output.  Every term (a - b)^2 is >= 0, so k roundings of relative size u = 2^-24 anywhere between the exact value and the result
    leave it within gamma_k = k u / (1 - k u) of the exact value, relatively.  The loss takes k = ceil(n / 256) + 13 for n = B C
    elements: 3 a term (the difference, which enters the square twice, and the product), ceil(n / 256) - 1 thread-serial additions (a
    thread adds elements t, t + 256, ...; the first addition is to 0), 6 steps of the 64-lane xor butterfly, 3 additions of the 4
    waves' sums, the quotient w / B and the product with it: 14 for n <= 256, 16 for n = 640.  The bound is gamma_k * w / B * sum (a -
    b)^2, 14 to 16 times 2^-24 of the term.  A derivative takes 3 (the difference, w / B, their product; the doubling is exact):
    |da - ref| <= gamma_3 |ref| per element, that is 3 units in the last place of fp32 at most.  (w = 10 is a float32; no operand comes
    near the subnormals.)  a == b gives exact zeros, db is -da to the bit (the sign turned), two runs are bit-identical."""
    rng = np.random.default_rng(100 * b + c)
    w = 10.0
    a = rng.normal(size=(b, c)).astype(np.float32)
    bb = (a + rng.normal(size=(b, c)) * 0.3).astype(np.float32)
    if b * c > 4:
        bb[0, 0], bb[-1, -1] = a[0, 0], a[-1, -1]                    # exact zeros among the others
    shape = (b,) if c == 1 else (b, c)                               # the logit comes as [B]
    at, bt = torch.from_numpy(a).reshape(shape).cuda(), torch.from_numpy(bb).reshape(shape).cuda()
    loss, da, db = K.consistency_loss(at, bt, w)
    loss2, da2, db2 = K.consistency_loss(at, bt, w)
    torch.cuda.synchronize()
    ref, da_ref, _ = R.loss_and_grads(a, bb, w)
    k = R.loss_roundings(b * c)
    assert k == -(-b * c // 256) + 13
    err = abs(float(loss.double()) - ref)
    print("consistency_loss", (b, c), "loss", float(loss), ref, "error %.2e of the term, bound %.2e" % (err / max(ref, 1e-300), R.gamma(k)))
    assert loss.shape == (1,) and loss.dtype == torch.float32 and da.shape == at.shape and db.shape == at.shape
    assert ref > 0.0 and err <= R.gamma(k) * ref
    g = da.double().cpu().numpy().reshape(b, c)
    assert bool((np.abs(g - da_ref) <= R.gamma(R.GRAD_ROUNDINGS) * np.abs(da_ref)).all()), float(np.abs(g - da_ref).max())
    assert bool((g[a == bb] == 0.0).all()) and int((a == bb).sum()) == (2 if b * c > 4 else 0)
    assert torch.equal(db.view(torch.int32), (-da).view(torch.int32))
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(da.view(torch.int32), da2.view(torch.int32)) \
        and torch.equal(db.view(torch.int32), db2.view(torch.int32))
    zl, za, zb = K.consistency_loss(at, at.clone(), w)
    assert float(zl) == 0.0 and not bool(za.any()) and not bool(zb.any())


def test_consistency_loss_rejects(K):
    a = torch.zeros((4, 2), device="cuda")
    with pytest.raises(ValueError, match="one shape"):
        K.consistency_loss(a, torch.zeros((4, 3), device="cuda"), 1.0)
    with pytest.raises(ValueError, match="one shape"):
        K.consistency_loss(a.reshape(2, 2, 2), a.reshape(2, 2, 2), 1.0)
    with pytest.raises(ValueError, match="finite"):
        K.consistency_loss(a, a, float('inf'))
    with pytest.raises(RuntimeError, match="float32"):
        K.consistency_loss(a.double(), a.double(), 1.0)


# ------------------------------------------------------------------ the Function
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_consistency_function_backward_scales_by_upstream(K, dtype):
    """functional2.ConsistencyLoss: the saved fp32 derivatives times an upstream scalar (3.0) reach BOTH inputs, in their dtype: fp32
    logits within gamma_4 of float64 (one more product), the critic's 16-bit logits rounded once more (2^-8 relative); equal logits
    keep an exact zero"""
    from gan_lib_tensorflow_amd import functional2 as F2
    from gan_lib_tensorflow_amd.common import misc
    rng = np.random.default_rng(5)
    (a, at), (b, bt) = bf(rng.normal(size=7)), bf(rng.normal(size=7))
    bt[3] = at[3]
    b[3] = a[3]
    at, bt = at.to(dtype).requires_grad_(True), bt.to(dtype).requires_grad_(True)
    loss = F2.consistency_loss(at, bt, 10.0)
    assert type(loss.grad_fn).__name__ == "ConsistencyLossBackward" and type(misc.consistency_loss(at, bt).grad_fn).__name__ == "ConsistencyLossBackward"
    ref, da_ref, db_ref = R.loss_and_grads(a.numpy(), b.numpy(), 10.0)
    assert abs(float(loss.detach()) - ref) <= R.gamma(R.loss_roundings(7)) * ref
    (loss * 3.0).sum().backward()
    torch.cuda.synchronize()
    tol = R.gamma(4) if dtype == torch.float32 else 2.0 ** -8 + R.gamma(4)
    for got, want in ((at.grad, da_ref), (bt.grad, db_ref)):
        assert got.dtype == dtype and got.shape == (7,)
        g = got.double().cpu().numpy()
        assert bool((np.abs(g - 3.0 * want) <= tol * np.abs(3.0 * want)).all()) and float(np.abs(g).max()) > 0.0
        assert g[3] == 0.0
    assert torch.equal(bt.grad, -at.grad)
    # one input without a gradient: the other still gets its own
    at2 = at.detach().clone().requires_grad_(True)
    F2.consistency_loss(at2, bt.detach(), 10.0).backward()
    assert at2.grad is not None and float(at2.grad.abs().max()) > 0.0
    with pytest.raises(ValueError, match="logits of"):
        F2.consistency_loss(at.detach().double(), bt.detach().double(), 1.0)


# ------------------------------------------------------------------ the trainer
BATCH, TSEED = 8, 4
OUTPUT_SCALE = 1.5           # D.Output/W of the test state times this: see test_acgan_consistency_losses_and_gradients_vs_oracle
WEIGHTS = (10.0, 5.0)


def l2(got, ref):
    got, ref = got.detach().to(F64).cpu().flatten(), ref.detach().to(F64).flatten()
    assert torch.isfinite(got).all()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def cos(got, ref):
    got, ref = got.detach().to(F64).cpu().flatten(), ref.detach().to(F64).flatten()
    return float((got @ ref) / max(float(got.norm() * ref.norm()), 1e-300))


@pytest.fixture(scope="module")
def inputs(K):
    """the explicit inputs of every trainer test here, drawn once (those of tests/test_grad_penalty_gpu.py, and two tables of shifts up
    to 4 from the restatement): (float64 CPU, device) pairs"""
    rng = np.random.default_rng(BATCH)
    real = bf(np.clip(rng.normal(size=(BATCH, 32, 32, 3)) * 0.5, -1, 1))
    rl = torch.tensor(rng.integers(0, 10, BATCH), dtype=torch.int32)
    z = bf(rng.normal(size=(BATCH, 128)))
    fl = torch.tensor(rng.integers(0, 10, BATCH), dtype=torch.int32)
    alpha = torch.tensor(rng.uniform(size=BATCH), dtype=torch.float32)
    state = dict(T.init_acgan_params(TSEED))
    scaled = dict(state)
    scaled['d_net/D.Output/W'] = state['d_net/D.Output/W'] * np.float32(OUTPUT_SCALE)
    return dict(real=real, rl=rl, z=z, fl=fl, alpha=alpha, state=state, scaled=scaled,
                table_real=R.draw_table(BATCH, 4, 99, 0), table_fake=R.draw_table(BATCH, 4, 99, 1))


def make(inputs, state='scaled', **kw):
    from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
    return ACGANTrainer(batch_size=BATCH, seed=TSEED, state=inputs[state], **kw)


def device_d_loss(tr, inputs, **kw):
    tr.d_flat['grads'].zero_()
    loss = tr.d_loss(inputs['real'][1], inputs['rl'].cuda(), z=inputs['z'][1], fake_labels=inputs['fl'].cuda(), alpha=inputs['alpha'].cuda(), **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss


def reference_d_loss(inputs, consistency, storage=None):
    P = T.to_torch(inputs['scaled'])
    T.STORE = storage
    try:
        loss, parts = R.acgan_d_loss(P, inputs['real'][0], inputs['rl'].long(), inputs['z'][0], inputs['fl'].long(), consistency, WEIGHTS,
                                     inputs['table_real'], inputs['table_fake'])
        dn = T.trainable_names(P, 'd_net')
        grads = dict(zip(dn, torch.autograd.grad(loss, [P[k] for k in dn])))
    finally:
        T.STORE = None
    return loss.detach(), parts, grads


def autograd_nodes(loss):
    """how often each node type occurs in the autograd graph behind `loss`"""
    seen, todo, names = set(), [loss.grad_fn], collections.Counter()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names[type(fn).__name__] += 1
        todo.extend(f for f, _ in fn.next_functions)
    return names


@pytest.mark.parametrize("consistency", ["bcr", "cr"])
def test_acgan_consistency_losses_and_gradients_vs_oracle(K, inputs, consistency, deterministic_stats):
    """ACGANTrainer(consistency=..., penalty='none', use_graphs=False).d_loss at batch 8 on explicit z, labels and tables against the
    float64 restatement, with the limits of test_acgan_penalty_losses_and_gradients_vs_oracle: the term and the total within 3 % of
    max(1, |ref|); per critic tensor cosine >= 0.975 and relative L2 <= 0.25, and L2 <= 1.5 x the restatement's own bf16-storage pass +
    0.05; conv biases under a batch norm (true gradient zero) <= 2e-3.  The absolute limits are applied where the bf16-storage floor
    leaves them room (worst floor L2 <= 0.2, cosine >= 0.98): asserted.

    The scale.  At the initial weights the logits are within 0.77 of zero and the float64 term on the real batch, at weight 10, is
    0.084: D.Output/W of the test's state is scaled by 1.5 (the terms grow by 2.25: real 0.19 at weight 10, fake 0.22 at weight 5),
    established from the restatement alone on the CPU and asserted on the reference side (each term that is on exceeds 0.1).  A larger
    scale would only push the hinge terms off their slopes.  `deterministic_stats` as in the penalty tests: the bound is for the
    arithmetic, not for the arrival order of the generator's statistics.

    'cr': the fake term is exactly zero and there is one ConsistencyLoss node, not two (the passes themselves are counted in
    test_acgan_cr_is_one_critic_pass_fewer_than_bcr).

    Measured on the MI355X (cosine min / L2 max over the critic's tensors, the floor of the same inputs after the bar; terms device vs
    float64; largest true-zero bias gradient):
        bcr  0.9837 / 0.180 | 0.9863 / 0.166   real 0.1922 vs 0.1889, fake 0.2145 vs 0.2218   biases 2.4e-4
        cr   0.9804 / 0.198 | 0.9852 / 0.173   real 0.1922 vs 0.1889, fake 0 vs 0             biases 2.1e-4
    Both floors leave the absolute limits room and both runs hold them; the worst tensors are the batch-norm scales of D.DownBlock.2."""
    loss_ref, parts, gref = reference_d_loss(inputs, consistency)
    _, _, gfloor = reference_d_loss(inputs, consistency, storage=T.bf16_storage)
    assert float(parts['cr_real']) > 0.1 and float(parts['cr']) > 0.1
    assert float(parts['cr_fake']) > 0.1 if consistency == 'bcr' else float(parts['cr_fake']) == 0.0
    tr = make(inputs, consistency=consistency, consistency_weight=WEIGHTS, penalty='none', use_graphs=False)
    tables = dict(table_real=torch.from_numpy(inputs['table_real']).cuda(), table_fake=torch.from_numpy(inputs['table_fake']).cuda())
    off = int(tr.rng_state[1])
    loss = device_d_loss(tr, inputs, **tables)
    assert int(tr.rng_state[1]) == off                       # every draw was given: none taken
    got = {k: float(tr.losses[k]) for k in ('consistency', 'consistency_real', 'consistency_fake')}
    want = dict(consistency=float(parts['cr']), consistency_real=float(parts['cr_real']), consistency_fake=float(parts['cr_fake']))
    print("acgan", consistency, "d_loss", float(loss), float(loss_ref), "terms", got, want)
    for k in got:
        assert abs(got[k] - want[k]) < 0.03 * max(1.0, want[k]), (k, got[k], want[k])
    assert abs(float(loss) - float(loss_ref)) < 0.03 * max(1.0, abs(float(loss_ref)))
    assert float(tr.losses['gradient_penalty']) == 0.0
    nodes = autograd_nodes(loss)
    if consistency == 'cr':
        assert got['consistency_fake'] == 0.0 and got['consistency'] == got['consistency_real']
    assert nodes['ConsistencyLossBackward'] == (2 if consistency == 'bcr' else 1)
    dn = list(gref)
    errs = {k: (cos(tr.store.vars[k].grad, gref[k]), l2(tr.store.vars[k].grad, gref[k])) for k in dn}
    floors = {k: (cos(gfloor[k], gref[k]), l2(gfloor[k], gref[k])) for k in dn if float(gref[k].norm()) > 1e-9}
    room = max(f[1] for f in floors.values()) <= 0.2 and min(f[0] for f in floors.values()) >= 0.98
    assert room, "the bf16-storage floor of %s leaves the absolute limits no room: decide anew whether they apply" % consistency
    normed = [k for k in dn if not (k.endswith('.Conv1/Biases') and 'DownBlock.1' not in k)]
    print("acgan", consistency, "D grads:", {k.split('/', 1)[1]: (round(c, 4), round(e, 3)) for k, (c, e) in errs.items()})
    print("acgan", consistency, "summary: device cosine min %.4f L2 max %.3f | floor cosine min %.4f L2 max %.3f | biases %.2e" % (
        min(errs[k][0] for k in normed), max(errs[k][1] for k in normed), min(f[0] for f in floors.values()), max(f[1] for f in floors.values()),
        max(float(tr.store.vars[k].grad.abs().max()) for k in dn if k not in normed)))
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


def test_acgan_cr_is_one_critic_pass_fewer_than_bcr(K, inputs):
    """counted on the autograd graph of the returned loss, with penalty='none': the critic is passed twice without the term, three times
    for 'cr', four times for 'bcr'.  Each pass ends in the logit's linear head (functional2.LinF); the class head is on the graph for
    the real pass alone, whose cross-entropy reads it: 3, 4 and 5 LinF nodes."""
    counts = {}
    for consistency in ('none', 'cr', 'bcr'):
        tr = make(inputs, consistency=consistency, penalty='none', use_graphs=False)
        nodes = autograd_nodes(tr.d_loss(inputs['real'][1], inputs['rl'].cuda(), z=inputs['z'][1], fake_labels=inputs['fl'].cuda()))
        counts[consistency] = nodes['LinFBackward']
    assert counts == dict(none=3, cr=4, bcr=5), counts


def test_acgan_consistency_none_is_the_existing_path(K, inputs, deterministic_stats):
    """consistency='none' spelled out against a trainer constructed without the argument, the default penalty, same inputs: the same
    nodes on the autograd graph, the same draws from the RNG stream, the same `state_dict()` keys, the same keys in `losses`, and a
    lookup of losses['consistency'] answers 0.  The loss terms are fixed-order sums: bitwise equal.  The gradient buffer sums through
    float atomics in arrival order (tests/test_grad_penalty_gpu.py, test_acgan_default_penalty_is_the_existing_path: one trainer does
    not always repeat its own buffer to the bit, 1-2 units in the last place), so the measure of that noise is a SECOND trainer
    constructed without the argument: where the two default trainers agree bitwise, the spelled-out one equals them bitwise; where
    they do not, the spelled-out one is held to that very noise (four times their largest difference, or 1e-5 of the buffer's
    maximum).  The three trainers have one seed, so each draws the same z, labels and alpha from its stream."""
    a, a2, b = make(inputs, 'state', use_graphs=False), make(inputs, 'state', use_graphs=False), make(inputs, 'state', consistency='none', use_graphs=False)
    assert a.consistency == b.consistency == 'none' and set(a.state_dict()) == set(b.state_dict()) == set(a.store.vars) | {'_d_updates'}
    runs = []
    for tr in (a, a2, b):
        off = int(tr.rng_state[1])
        tr.d_flat['grads'].zero_()
        loss = tr.d_loss(inputs['real'][1], inputs['rl'].cuda())                  # z, labels and alpha from the stream
        loss.backward()
        torch.cuda.synchronize()
        nodes = autograd_nodes(loss)
        assert 'ConsistencyLossBackward' not in nodes
        assert float(tr.losses['consistency']) == 0.0 and tr.losses['consistency'].shape == tr.losses['d_loss_gan'].shape
        assert set(tr.losses) == {'d_loss_gan', 'd_loss_acgan', 'gradient_penalty'}
        runs.append((dict({k: float(v) for k, v in tr.losses.items()}, d_loss=float(loss)), tr.d_flat['grads'].clone(), nodes, int(tr.rng_state[1]) - off))
    (t1, g1, n1, o1), (t2, g2, n2, o2), (tb, gb, nb, ob) = runs
    assert o1 == o2 == ob == 3 and n1 == n2 == nb
    print("none path: |default 2 - default 1| max", float((g2 - g1).abs().max()), "|spelled - default 1| max", float((gb - g1).abs().max()), "of",
          float(g1.abs().max()), "| terms", t1, t2, tb)
    assert t1 == t2 == tb, (t1, t2, tb)
    if torch.equal(g1, g2):
        assert torch.equal(gb, g1)
    else:
        assert float((gb - g1).abs().max()) <= max(4 * float((g2 - g1).abs().max()), 1e-5 * float(g1.abs().max()))


def run_steps(tr, n, seed=2):
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import synthetic_batches
    feed = synthetic_batches(BATCH, "cuda", seed=seed)
    rows = []
    for _ in range(n):
        off = int(tr.rng_state[1])
        tr.d_step(*next(feed))
        torch.cuda.synchronize()
        rows.append(dict(off=off, advance=int(tr.rng_state[1]) - off, losses={k: float(tr.losses[k]) for k in
                                                                               ('d_loss', 'd_loss_gan', 'd_loss_acgan', 'gradient_penalty', 'consistency', 'consistency_real', 'consistency_fake')},
                         tables={k: v.cpu().numpy().copy() for k, v in tr.consistency_tables.items()}))
    return rows


def test_acgan_bcr_captured_graph_draws_afresh_on_every_replay(K, inputs):
    """consistency='bcr' with the default penalty and captured graphs, three critic updates: eager, capture + replay, replay.  Every
    update advances the RNG stream by its six draws (dequantisation noise, z, labels, alpha, the two tables) and its tables are the
    host restatement at that update's offsets: the replays draw afresh.  The losses are finite and the term is there.  With
    penalty_every=4, nine updates: exactly two captured forms, 'd_bcr' (updates 0, 4, 8) and 'd_plain_bcr' (the others), the term in both."""
    tr = make(inputs, consistency='bcr', use_graphs=True)
    assert tr.graphs.enabled
    seed = int(tr.rng_state[0])
    rows = run_steps(tr, 3)
    assert set(tr.graphs.graphs) == {'d_bcr'} and tr.d_updates == 3
    for i, r in enumerate(rows):
        assert r['advance'] == 6, (i, r['advance'])
        assert np.array_equal(r['tables']['real'], R.draw_table(BATCH, 4, seed, r['off'] + 4)), i
        assert np.array_equal(r['tables']['fake'], R.draw_table(BATCH, 4, seed, r['off'] + 5)), i
        assert all(np.isfinite(v) for v in r['losses'].values()), r['losses']
        assert r['losses']['consistency_real'] > 0.0 and r['losses']['consistency_fake'] > 0.0 and r['losses']['gradient_penalty'] > 0.0
    assert not np.array_equal(rows[1]['tables']['real'], rows[2]['tables']['real']) and not np.array_equal(rows[1]['tables']['fake'], rows[2]['tables']['fake'])
    assert len({r['losses']['consistency'] for r in rows}) == 3
    print("bcr graphs:", [r['losses'] for r in rows])
    tr.graphs.clear()
    del tr
    lazy = make(inputs, consistency='bcr', penalty_every=4, use_graphs=True)
    rows = run_steps(lazy, 9)
    assert set(lazy.graphs.graphs) == {'d_bcr', 'd_plain_bcr'} and lazy.d_updates == 9
    for i, r in enumerate(rows):
        assert all(np.isfinite(v) for v in r['losses'].values()), (i, r['losses'])
        assert r['losses']['consistency'] > 0.0 and r['losses']['consistency_real'] > 0.0 and r['losses']['consistency_fake'] > 0.0, (i, r['losses'])
        assert (r['losses']['gradient_penalty'] > 0.0) == (i % 4 == 0) and r['advance'] == (6 if i % 4 == 0 else 5), (i, r)
    print("bcr lazy graphs:", [r['losses'] for r in rows])
    lazy.graphs.clear()
    del lazy
    gc.collect()
    torch.cuda.synchronize()
