"""The projection discriminator on a real MI355X: the three head kernels against the NumPy float64 head, the spectrally normalised
label table, the projection critic and its trainer against the float64 restatement (tests/projection_ref.py).

Bounds of the kernel tests are derived from the arithmetic (inputs are rounded to bf16 first, the reference gets the rounded
values): a logit is an fp32 sum rounded to bf16 once -- 2^-8 |ref| for the rounding (twice the half-ulp) plus 1e-5 * sum |x| |w + E|
for 128 fp32 additions (each 2^-24 relative) and the fp32 coefficient; dx is one product rounded once: 2^-8 relative; the fp32
gradient sums: 1e-5 * the sum of their absolute terms.  Model bounds are those of test_model_gpu.py, stated at each assertion."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_ref as R  # noqa: E402
from oracle import ref_torch as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gan_lib_tensorflow_amd import kernels
    kernels.lib()
    return kernels


def bf(a):
    """fp32 ndarray -> (bf16-rounded float64 ndarray, bf16 cuda tensor)"""
    t = torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16)
    return t.to(torch.float64).numpy(), t.cuda().contiguous()


def f32(a):
    t = torch.tensor(np.asarray(a, np.float32))
    return t.to(torch.float64).numpy(), t.cuda().contiguous()


def bf16r(a):
    return torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16)


def f64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def same_bits(a, b):
    return (a is None and b is None) or torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                                                    b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))


def head_inputs(rng, M, Kd, V, labels=None):
    x = bf(rng.normal(size=(M, Kd)))
    w = f32(rng.normal(size=Kd) * 0.3)
    b = f32(rng.normal(size=1))
    E = f32(rng.normal(size=(V, Kd)) * 0.3)
    labels = rng.integers(0, V, M) if labels is None else np.asarray(labels)
    return x, w, b, E, labels, torch.tensor(labels, dtype=torch.int32).cuda()


AB_CASES = {
    "128x128x10": dict(M=128, Kd=128, V=10),
    "6x128x10": dict(M=6, Kd=128, V=10),
    "7x64x3": dict(M=7, Kd=64, V=3),
    "1x128x10": dict(M=1, Kd=128, V=10),
    "one_label": dict(M=70, Kd=128, V=10, labels=[4] * 70),
    "absent_label_prior_grads": dict(M=7, Kd=64, V=3, labels=[2, 0, 2, 2, 0, 0, 2], prior=True),
    "no_bias": dict(M=6, Kd=128, V=10, use_b=False),
    "no_dx": dict(M=6, Kd=128, V=10, want_dx=False),
}


@pytest.mark.parametrize("case", list(AB_CASES))
def test_head_forward_and_backward_vs_float64(K, case):
    """gank_proj_head_fwd / gank_proj_head_bwd: logits, dx and the three accumulated sums against the closed form; accumulation onto
    prior content; a row of e_grad whose label does not occur keeps its bits; two launches give the same bits."""
    cfg = dict(AB_CASES[case])
    M, Kd, V = cfg["M"], cfg["Kd"], cfg["V"]
    rng = np.random.default_rng(M * 1000 + Kd + V)
    x, w, b, E, labels, lt = head_inputs(rng, M, Kd, V, cfg.get("labels"))
    use_b, want_dx, prior = cfg.get("use_b", True), cfg.get("want_dx", True), cfg.get("prior", False)
    dl = bf(rng.normal(size=M))
    ref = R.head_logits(x[0], w[0], b[0] if use_b else None, E[0], labels)
    rdx, rdw, rdb, rdE = R.head_grads(dl[0], x[0], w[0], E[0], labels)
    p_w, p_b, p_E = (f32(rng.normal(size=s)) if prior else f32(np.zeros(s)) for s in ((Kd,), (1,), (V, Kd)))
    runs = []
    for _ in range(2):
        gw, gb, gE = p_w[1].clone(), p_b[1].clone(), p_E[1].clone()
        logits = K.proj_head_fwd(x[1], w[1], b[1] if use_b else None, E[1], lt)
        dx = K.proj_head_bwd(dl[1], x[1], w[1], E[1], lt, want_dx, gw, gb, gE)
        torch.cuda.synchronize()
        runs.append((logits, dx, gw, gb, gE))
    logits, dx, gw, gb, gE = runs[0]
    tol = 2.0 ** -8 * np.abs(ref) + 1e-5 * R.head_abs_terms(x[0], w[0], E[0], labels)
    err = np.abs(f64(logits) - ref)
    print("logits: worst error / bound", float((err / tol).max()))
    assert (err <= tol).all(), (err, tol)
    if want_dx:
        assert dx.shape == (M, Kd) and (np.abs(f64(dx) - rdx) <= 2.0 ** -8 * np.abs(rdx)).all()
    else:
        assert dx is None
    terms = np.abs(dl[0])[:, None] * np.abs(x[0])
    absE = np.zeros((V, Kd))
    np.add.at(absE, labels, terms)
    assert (np.abs(f64(gw) - (p_w[0] + rdw)) <= 1e-5 * (terms.sum(axis=0) + np.abs(p_w[0]))).all()
    assert abs(float(gb) - (float(p_b[0][0]) + rdb)) <= 1e-5 * (np.abs(dl[0]).sum() + abs(float(p_b[0][0])))
    assert (np.abs(f64(gE) - (p_E[0] + rdE)) <= 1e-5 * (absE + np.abs(p_E[0]))).all()
    absent = [v for v in range(V) if v not in set(labels.tolist())]
    for v in absent:
        assert same_bits(gE[v], p_E[1][v])
    if prior:
        assert absent and float(np.abs(p_E[0][absent]).min()) > 0 and float(np.abs(f64(gE) - p_E[0])[labels[0]].max()) > 0
    for a, c in zip(runs[0], runs[1]):
        assert same_bits(a, c)


def test_head_treats_labels_out_of_range_like_the_embedding_kernels(K):
    """a label outside [0, V): a zero table row in the logit and in dx, no row of e_grad (gank_embedding_fwd / _bwd)"""
    rng = np.random.default_rng(1)
    x, w, b, E, _, _ = head_inputs(rng, 6, 128, 10)
    labels = np.array([3, -1, 10, 9, 0, 1 << 20])
    lt = torch.tensor(labels, dtype=torch.int32).cuda()
    dl = bf(rng.normal(size=6))
    gE = torch.zeros_like(E[1])
    logits = K.proj_head_fwd(x[1], w[1], b[1], E[1], lt)
    dx = K.proj_head_bwd(dl[1], x[1], w[1], E[1], lt, True, None, None, gE)
    torch.cuda.synchronize()
    ref = R.head_logits(x[0], w[0], b[0], E[0], labels)
    assert (np.abs(f64(logits) - ref) <= 2.0 ** -8 * np.abs(ref) + 1e-5 * R.head_abs_terms(x[0], w[0], E[0], labels)).all()
    rdx, _, _, rdE = R.head_grads(dl[0], x[0], w[0], E[0], labels)
    assert (np.abs(f64(dx) - rdx) <= 2.0 ** -8 * np.abs(rdx)).all()
    assert np.abs(f64(gE) - rdE).max() <= 1e-5 * np.abs(rdE).max() and not f64(gE)[[1, 2, 4, 5, 6, 7, 8]].any()


@pytest.mark.parametrize("loss_scale", [1.0, 1024.0])
@pytest.mark.parametrize("M,n_real", [(128, 64), (6, 2), (7, 0)])
@pytest.mark.parametrize("mode", [0, 1])
def test_fused_hinge_head_equals_the_three_launches(K, mode, M, n_real, loss_scale):
    """gank_proj_head_hinge_scaled: logits and dx bit-equal to proj_head_fwd -> hinge_*_loss (-> loss_grad_scale) -> proj_head_bwd;
    loss and the three accumulated gradients within 1e-6 of the sum of their absolute terms; the loss against float64 (hinge is
    1-Lipschitz per logit: the logits' own bound, averaged).  The critic loss with no real row (mode 0, n_real = 0) is a mean
    over nothing: refused, as gank_hinge_d_loss and gank_critic_head_hinge refuse it."""
    Kd, V = 128, 10
    rng = np.random.default_rng(100 * M + n_real + mode)
    x, w, b, E, labels, lt = head_inputs(rng, M, Kd, V)
    if mode == 0 and n_real == 0:
        with pytest.raises(RuntimeError, match="n_real must split the batch"):
            K.proj_head_hinge(x[1], w[1], b[1], E[1], lt, n_real, mode, loss_scale=loss_scale)
        with pytest.raises(RuntimeError, match="hinge_d_loss"):
            K.hinge_d_loss(K.proj_head_fwd(x[1], w[1], b[1], E[1], lt), n_real)
        return
    prior = [f32(rng.normal(size=s)) for s in ((Kd,), (1,), (V, Kd))]
    gw, gb, gE = (p[1].clone() for p in prior)
    loss, logits, dx = K.proj_head_hinge(x[1], w[1], b[1], E[1], lt, n_real, mode, True, gw, gb, gE, loss_scale=loss_scale)
    uw, ub, uE = (p[1].clone() for p in prior)
    ulogits = K.proj_head_fwd(x[1], w[1], b[1], E[1], lt)
    uloss, udl, udl32 = K.hinge_g_loss(ulogits) if mode else K.hinge_d_loss(ulogits, n_real)
    if loss_scale != 1.0:
        udl = K.loss_grad_scale(udl32, torch.tensor([loss_scale], dtype=torch.float32).cuda())
    udx = K.proj_head_bwd(udl, x[1], w[1], E[1], lt, True, uw, ub, uE)
    torch.cuda.synchronize()
    assert same_bits(logits, ulogits) and same_bits(dx, udx)
    dl = f64(udl)
    cnt = np.where(np.arange(M) < n_real, n_real, M - n_real) if mode == 0 else np.full(M, M)
    lterms = (1.0 + np.abs(f64(ulogits))) / cnt
    print("loss fused / unfused", float(loss), float(uloss))
    assert abs(float(loss) - float(uloss)) <= 1e-6 * lterms.sum()
    terms = np.abs(dl)[:, None] * np.abs(x[0])
    absE = np.zeros((V, Kd))
    np.add.at(absE, labels, terms)
    assert (np.abs(f64(gw) - f64(uw)) <= 1e-6 * (terms.sum(axis=0) + np.abs(prior[0][0]))).all()
    assert abs(float(gb) - float(ub)) <= 1e-6 * (np.abs(dl).sum() + abs(float(prior[1][0][0])))
    assert (np.abs(f64(gE) - f64(uE)) <= 1e-6 * (absE + np.abs(prior[2][0]))).all()
    # against float64: the loss, and the projection term is in the gradients (dl is exact: +-loss_scale / count or 0)
    ref = R.head_logits(x[0], w[0], b[0], E[0], labels)
    tol = 2.0 ** -8 * np.abs(ref) + 1e-5 * R.head_abs_terms(x[0], w[0], E[0], labels)
    rloss, _ = R.hinge(ref, n_real, mode)
    assert abs(float(loss) - rloss) <= (tol / cnt).sum() + 1e-6 * lterms.sum(), (float(loss), rloss)
    rdx, rdw, rdb, rdE = R.head_grads(dl, x[0], w[0], E[0], labels)
    assert (np.abs(f64(dx) - rdx) <= 2.0 ** -8 * np.abs(rdx)).all()
    assert (np.abs(f64(gE) - (prior[2][0] + rdE)) <= 1e-5 * (absE + np.abs(prior[2][0]))).all()
    assert (np.abs(f64(gw) - (prior[0][0] + rdw)) <= 1e-5 * (terms.sum(axis=0) + np.abs(prior[0][0]))).all()


def test_autograd_nodes_of_the_head(K):
    """Fn.projection_head is the two kernels (same bits); the fused node refuses a gradient seed of another scale"""
    from gan_lib_tensorflow_amd import functional as Fn
    rng = np.random.default_rng(9)
    M, Kd, V = 6, 128, 10
    x, w, b, E, labels, lt = head_inputs(rng, M, Kd, V)
    dl = bf(rng.normal(size=M))
    xt = x[1].clone().requires_grad_(True)
    Wt, bt, Et = w[1].reshape(Kd, 1).clone().requires_grad_(True), b[1].clone().requires_grad_(True), E[1].clone().requires_grad_(True)
    logits = Fn.projection_head(xt, Wt, bt, Et, lt)
    assert logits.shape == (M,) and same_bits(logits.detach(), K.proj_head_fwd(x[1], w[1], b[1], E[1], lt))
    logits.backward(dl[1])
    gw, gb, gE = torch.zeros_like(w[1]), torch.zeros_like(b[1]), torch.zeros_like(E[1])
    dx = K.proj_head_bwd(dl[1], x[1], w[1], E[1], lt, True, gw, gb, gE)
    torch.cuda.synchronize()
    assert same_bits(xt.grad, dx) and same_bits(Wt.grad.reshape(-1), gw) and same_bits(bt.grad, gb) and same_bits(Et.grad, gE)
    for scale, wrong in ((1.0, 1024.0), (1024.0, 1.0)):
        xt = x[1].clone().requires_grad_(True)
        loss = Fn.ProjectionHeadSpec(0, 2, lt, loss_scale=scale)(xt, Wt, bt, Et)
        assert loss.logits.shape == (M,)
        with pytest.raises(NotImplementedError, match="loss scale"):
            loss.backward(gradient=Fn.grad_seed(loss, wrong))
        loss = Fn.ProjectionHeadSpec(0, 2, lt, loss_scale=scale)(xt, Wt, bt, Et)
        loss.backward(gradient=Fn.grad_seed(loss, scale))
        _, _, dx = K.proj_head_hinge(x[1], w[1], b[1], E[1], lt, 2, 0, loss_scale=scale)
        torch.cuda.synchronize()
        assert same_bits(xt.grad, dx)


# ---------------------------------------------------------------------------------------------- embed_y(spectral_normed=True)
def test_embed_y_spectral_normed(K):
    """embed_y(..., spectral_normed=True): rows of E / sigma(E) (one bf16 rounding: 2^-8, on top of the fp32 normalisation's 1e-5);
    u overwritten with update_collection=None, untouched with NO_OPS; the table's gradient THROUGH the normalisation against
    float64 autograd at test_kernels_gpu.py's bound for the spectral norm's backward pass (2e-4 of the largest entry)."""
    from gan_lib_tensorflow_amd.common.ops import embedding as Emb
    from gan_lib_tensorflow_amd.common.ops.sn import NO_OPS
    from gan_lib_tensorflow_amd.store import ParamStore, set_default_store
    store = set_default_store(ParamStore('cuda', seed=3))
    labels = np.array([1, 7, 7, 0, 9, 3])
    lt = torch.tensor(labels, dtype=torch.int32).cuda()
    with store.variable_scope('Discriminator'):
        y0 = Emb.embed_y(lt, 10, 128, spectral_normed=True, update_collection=NO_OPS)
    assert sorted(store.vars) == [R.TABLE, R.TABLE_U] and store.trainable == {R.TABLE: True, R.TABLE_U: False}
    table, u = store.vars[R.TABLE], store.vars[R.TABLE_U]
    assert tuple(table.shape) == (10, 128) and tuple(u.shape) == (1, 128) and float(table.detach().abs().max()) <= 0.08
    Et = torch.tensor(f64(table), requires_grad=True)
    u0 = u.detach().clone()
    E_bar, u1, _ = T.spectral_normed_weight(Et, torch.tensor(f64(u0)))
    ref = E_bar.detach().numpy()[labels]
    torch.cuda.synchronize()
    assert (np.abs(f64(y0) - ref) <= (2.0 ** -8 + 1e-5) * np.abs(ref)).all()
    assert torch.equal(u, u0)                                            # NO_OPS: read, never written
    dy = bf(np.random.default_rng(4).normal(size=(6, 128)))
    with store.variable_scope('Discriminator'), pytest.warns(UserWarning, match="update_collection"):
        y1 = Emb.embed_y(lt, 10, 128, spectral_normed=True, update_collection=None)
    y1.backward(dy[1])
    torch.cuda.synchronize()
    assert same_bits(y1.detach(), y0.detach())
    assert float((u - u0).abs().max()) > 1e-3 and np.abs(f64(u) - u1.detach().numpy()).max() <= 1e-5      # None: u <- u_final
    (E_bar[torch.tensor(labels)] * torch.tensor(dy[0])).sum().backward()
    g, r = f64(table.grad), Et.grad.numpy()
    print("table gradient through the normalisation: max-rel", float(np.abs(g - r).max() / np.abs(r).max()))
    assert np.abs(g - r).max() <= 2e-4 * np.abs(r).max()
    # the switch off: bit for bit the plain lookup
    with store.variable_scope('Discriminator'):
        plain = Emb.embed_y(lt, 10, 128)
    assert same_bits(plain.detach(), K.embedding_fwd(table.detach(), lt))


# ---------------------------------------------------------------------------------------------- model
GRAD_LABELS = [3, 3, 7, 1]       # one label twice, six labels never


def make_trainer(seed, batch=4, **kw):
    from gan_lib_tensorflow_amd.SNGAN import gan_cifar_resnet as S
    state = R.init_projection_params(seed)
    kw.setdefault("use_graphs", False)
    return S, S.SNGANTrainer(batch_size=batch, seed=seed, projection=True, state=state, **kw), state


def step_inputs(rng, b, labels=None):
    z = bf16r(rng.normal(size=(b, 128)))
    labels = torch.tensor(rng.integers(0, 10, b) if labels is None else labels, dtype=torch.int32)
    real_u8 = torch.tensor(rng.integers(0, 256, (b, 3072)), dtype=torch.uint8)
    real_pre = bf16r(T.preprocess_real(real_u8, torch.zeros(b, 3072, dtype=torch.float64), torch.float64).numpy())
    return z, labels, real_pre


def grad_errors(tr, names, ref_g):
    out = {}
    for k in names:
        g, r = tr.store.vars[k].main_grad.double().cpu().flatten(), ref_g[k].flatten()
        out[k] = (float((g - r).abs().max() / r.abs().max()), float((g @ r) / (g.norm() * r.norm())), float((g - r).norm() / r.norm()))
    return out


def test_names_counts_and_logits_vs_restatement(K):
    S, tr, state = make_trainer(0)
    assert tr.projection is True and sorted(tr.store.vars) == sorted(state)
    assert not any('D.Embedding_y' in k for k in tr.store.vars)
    assert tr.store.param_count('Generator') == 7875587 and tr.store.param_count('Discriminator') == R.CRITIC_PARAMS
    us = [k for k in tr.store.vars if k.endswith('spectral_norm/u')]
    assert len(us) == 12 and R.TABLE_U in us and tr.sn_state is not None and tr.sn_state.n == 12
    assert tuple(tr.store.vars['Discriminator/D.Block.2.Conv1/Filters'].shape) == (3, 3, 128, 128)
    assert R.TABLE in tr.d_flat['offsets'] and tr.store.vars[R.TABLE].main_grad.shape == (10, 128)
    rng = np.random.default_rng(2)
    x = bf16r(rng.uniform(-1, 1, (8, 3072)))
    labels = torch.tensor(rng.integers(0, 10, 8), dtype=torch.int32)
    P = T.to_torch(state)
    with torch.no_grad():
        ref, new_u = R.discriminator_projection(P, x.to(torch.float64), labels.long())
    ref = ref.numpy()
    u_flat = tr.store.flat['Discriminator#state']['buf']
    u_before = u_flat.clone()
    with torch.no_grad():
        logits, aux = S.Discriminator(x.cuda(), labels.cuda(), update_collection=S.NO_OPS, projection=True)
    torch.cuda.synchronize()
    assert aux is None and torch.equal(u_flat, u_before)                                  # NO_OPS: never written
    d = np.abs(f64(logits) - ref)
    print("logits |d| max", float(d.max()), "ref", ref)
    assert (d <= 0.06 * np.maximum(1., np.abs(ref))).all(), (d, ref)
    with torch.no_grad():
        logits2, _ = S.Discriminator(x.cuda(), labels.cuda(), update_collection=None, projection=True)
    torch.cuda.synchronize()
    assert (np.abs(f64(logits2) - ref) <= 0.06 * np.maximum(1., np.abs(ref))).all()
    for k in (R.TABLE_U, 'Discriminator/D.Output/spectral_norm/u', 'Discriminator/D.Block.2.Conv1/filters/spectral_norm/u'):
        got, want = f64(tr.store.vars[k]), new_u[k].numpy()
        assert np.abs(got - want).max() <= 1e-4 * np.abs(want).max(), k               # None: overwritten with u_final


def test_d_and_g_gradients_vs_restatement(K):
    """_d_forward_backward / _g_forward_backward per tensor against float64 autograd at the bounds of
    test_model_gpu.py::test_d_and_g_gradients_vs_oracle without its 'mbedding' allowance: critic tensors max-rel 0.1, cosine 0.995,
    L2 0.08; generator tensors cosine 0.98, L2 0.2 (conv biases in front of a batch norm: |g| <= 1e-3, their true gradient is
    zero).  The gradient with respect to the NORMALISED table (the head's e_grad, before the spectral norm's backward pass
    spreads <G, W> d sigma / dW over every row) is exactly zero in the rows of labels that do not occur."""
    S, tr, state = make_trainer(5)
    rng = np.random.default_rng(7)
    b = 4
    z, labels, real_pre = step_inputs(rng, b, GRAD_LABELS)
    P = T.to_torch(state)
    loss, _, _ = R.d_loss_fn(P, None, labels.long(), z.to(torch.float64), None, real_pre=real_pre.to(torch.float64))
    dn = T.trainable_names(P, 'Discriminator')
    ref_g = dict(zip(dn, torch.autograd.grad(loss, [P[k] for k in dn])))
    tr.real_labels.copy_(labels)
    tr._d_forward_backward(real_pre=real_pre.cuda(), z=z.cuda())
    torch.cuda.synchronize()
    assert abs(float(tr.d_loss) - float(loss)) < 0.05
    errs = grad_errors(tr, dn, ref_g)
    print("D grad (max-rel, cos, l2):", {k.split('/', 1)[1]: tuple(round(e, 4) for e in v) for k, v in errs.items()})
    zero_ref = [k for k in dn if float(ref_g[k].abs().max()) < 1e-12]      # D.Output/b: the eight hinge derivatives cancel
    assert zero_ref == ['Discriminator/D.Output/b'] and float(tr.store.vars[zero_ref[0]].main_grad.abs().max()) <= 1e-6
    bad = [(k, v) for k, v in errs.items() if k not in zero_ref and not (v[0] <= 0.1 and v[1] >= 0.995 and v[2] <= 0.08)]
    assert not bad, bad
    from gan_lib_tensorflow_amd.common.ops import sn
    pairs = sn.sn_pairs(tr.store, 'Discriminator', with_names=True)
    assert pairs[-1][2] == R.TABLE
    off = sum(w.numel() for w, _, _ in pairs[:-1])
    e_grad = tr.d_flat['scratch'][off:off + 1280].view(10, 128)
    present = sorted(set(GRAD_LABELS))
    absent = [v for v in range(10) if v not in present]
    assert float(e_grad[absent].abs().max()) == 0.0
    assert all(float(e_grad[v].abs().max()) > 0 for v in present)
    # ---- generator (fresh oracle parameters: the D pass advanced u)
    P = T.to_torch(tr.store.state_dict())
    z2 = bf16r(rng.normal(size=(2 * b, 128)))
    fl = torch.tensor(GRAD_LABELS + [7, 0, 3, 3], dtype=torch.int32)
    loss, _ = R.g_loss_fn(P, z2.to(torch.float64), fl.long())
    gn = T.trainable_names(P, 'Generator')
    ref_g = dict(zip(gn, torch.autograd.grad(loss, [P[k] for k in gn])))
    tr._g_forward_backward(z=z2.cuda(), fake_labels=fl.cuda())
    torch.cuda.synchronize()
    assert abs(float(tr.g_loss) - float(loss)) < 0.05
    bad = []
    for k in gn:
        g, r = tr.store.vars[k].main_grad.double().cpu().flatten(), ref_g[k].flatten()
        if k.endswith('Biases') and 'G.Output' not in k:
            if g.abs().max() > 1e-3:
                bad.append((k, 'abs', float(g.abs().max())))
            continue
        cos, l2 = float((g @ r) / (g.norm() * r.norm())), float((g - r).norm() / r.norm())
        if cos < 0.98 or l2 > 0.2:
            bad.append((k, cos, l2))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------- trainer
def test_wgan_loss_goes_through_the_unfused_operator(K):
    """loss_type='WGAN': Fn.projection_head + wgan_d_loss / hinge_g_loss; losses and critic gradients against the restatement
    (bounds of test_d_and_g_gradients_vs_restatement)"""
    S, tr, state = make_trainer(6, loss_type='WGAN')
    rng = np.random.default_rng(17)
    b = 4
    z, labels, real_pre = step_inputs(rng, b, GRAD_LABELS)
    P = T.to_torch(state)
    lg, _ = R.d_logits_fn(P, None, labels.long(), z.to(torch.float64), None, real_pre=real_pre.to(torch.float64))
    loss, _ = T.sngan_losses(lg, b, None, 'WGAN', False)
    dn = T.trainable_names(P, 'Discriminator')
    ref_g = dict(zip(dn, torch.autograd.grad(loss, [P[k] for k in dn])))
    tr.real_labels.copy_(labels)
    tr._d_forward_backward(real_pre=real_pre.cuda(), z=z.cuda())
    torch.cuda.synchronize()
    assert abs(float(tr.d_loss) - float(loss)) < 0.05, (float(tr.d_loss), float(loss))
    zero_ref = [k for k in dn if float(ref_g[k].abs().max()) < 1e-12]      # D.Output/b: -1/b on b rows and +1/b on b rows cancel
    assert zero_ref == ['Discriminator/D.Output/b'] and float(tr.store.vars[zero_ref[0]].main_grad.abs().max()) <= 1e-6
    bad = [(k, v) for k, v in grad_errors(tr, dn, ref_g).items() if k not in zero_ref and not (v[1] >= 0.995 and v[2] <= 0.08)]
    assert not bad, bad
    P = T.to_torch(tr.store.state_dict())
    z2 = bf16r(rng.normal(size=(2 * b, 128)))
    fl = torch.tensor(rng.integers(0, 10, 2 * b), dtype=torch.int32)
    gloss, _ = R.g_loss_fn(P, z2.to(torch.float64), fl.long())
    tr._g_forward_backward(z=z2.cuda(), fake_labels=fl.cuda())
    torch.cuda.synchronize()
    assert abs(float(tr.g_loss) - float(gloss)) < 0.05


def test_train_iterations_eager_vs_captured(K):
    """the first two critic updates eager against hipGraph replay as test_model_gpu.py compares them (fixed-order batch-norm
    statistics; parameters equal up to the order of the filter gradients' fp32 atomics), then two whole iterations each way
    through the prefetched, captured path: sanity only"""
    from gan_lib_tensorflow_amd import functional as Fn
    stats_were, Fn.CONV_EPILOGUE_STATS = Fn.CONV_EPILOGUE_STATS, False
    try:
        S, tr_e, _ = make_trainer(11, 8, use_graphs=False)
        _, tr_g, _ = make_trainer(11, 8, use_graphs=True)
        feed_e, feed_g = S.synthetic_batches(8, "cuda", seed=1), S.synthetic_batches(8, "cuda", seed=1)
        for _ in range(2):
            tr_e.d_step(*next(feed_e))
            tr_g.d_step(*next(feed_g))
        torch.cuda.synchronize()
        assert tr_g.use_graphs and 'd' in tr_g._graphs
        assert torch.equal(tr_e.rng_state, tr_g.rng_state)
        d = (tr_e.d_flat["params"] - tr_g.d_flat["params"]).abs()
        assert (d > 2e-5).float().mean().item() < 5e-3 and d.mean().item() < 2e-6, ((d > 2e-5).float().mean().item(), d.mean().item())
        assert abs(float(tr_e.d_loss) - float(tr_g.d_loss)) < 1e-4
        o, n = tr_e.d_flat['offsets'][R.TABLE], 1280
        assert float((tr_e.d_flat["params"][o:o + n] - torch.tensor(R.init_projection_params(11)[R.TABLE]).cuda().reshape(-1)).abs().max()) > 1e-5
    finally:
        Fn.CONV_EPILOGUE_STATS = stats_were
    tr_e._graphs.clear()
    tr_g._graphs.clear()
    for _ in range(2):
        tr_e.train_iteration(feed_e)
        tr_g.train_iteration(feed_g)
    torch.cuda.synchronize()
    assert tr_g.use_graphs and 'd_pre' in tr_g._graphs
    for tr in (tr_e, tr_g):
        assert tr.iteration == 2 and int(tr.iteration_dev) == 2 and int(tr.d_opt.t) == 12 and int(tr.g_opt.t) == 1
        assert 0.0 <= float(tr.d_loss) < 4.0
    for net in ('Generator', 'Discriminator'):
        a, b = tr_e.store.flat[net]["params"], tr_g.store.flat[net]["params"]
        assert torch.isfinite(a).all() and torch.isfinite(b).all() and (a - b).abs().max().item() < 60 * 2e-4
    assert np.isfinite(f64(tr_g.sample(4))).all()


def test_dev_disc_cost_is_forward_only_and_advances_u(K):
    b = 8
    S, tr, state = make_trainer(61, b)
    rng = np.random.default_rng(5)
    z, labels, real_pre = step_inputs(rng, b)
    P = T.to_torch(state)
    with torch.no_grad():
        ref, new_u, _ = R.d_loss_fn(P, None, labels.long(), z.to(torch.float64), None, real_pre=real_pre.to(torch.float64))
    u0 = tr.store.vars[R.TABLE_U].clone()
    p0, m0 = tr.d_flat["params"].clone(), tr.d_flat["m"].clone()
    tr.d_flat["grads_all"].zero_()
    tr.d_flat["clean"] = True
    got = tr.dev_disc_cost(None, labels, z=z.cuda(), real_pre=real_pre.cuda())
    assert abs(got - float(ref)) < 0.02, (got, float(ref))
    u1 = tr.store.vars[R.TABLE_U].clone()
    assert float((u1 - u0).abs().max()) > 1e-3
    assert float((u1.double().cpu().reshape(-1) - new_u[R.TABLE_U].reshape(-1)).abs().max()) < 1e-4
    assert torch.equal(tr.d_flat["params"], p0) and torch.equal(tr.d_flat["m"], m0) and int(tr.d_opt.t) == 0
    assert float(tr.d_flat["grads_all"].abs().max()) == 0.0 and tr.d_flat["clean"] is True
    tr.dev_disc_cost(None, labels, z=z.cuda(), real_pre=real_pre.cuda())
    assert float((tr.store.vars[R.TABLE_U] - u1).abs().max()) > 0


def test_checkpoints_restore_the_table_its_u_and_its_adam_slots(K, tmp_path):
    """state_dict -> a differently initialised trainer -> load_state_dict, and the same through TF checkpoint files: the table, its u
    and its Adam slots come back exactly"""
    from gan_lib_tensorflow_amd.common import tf_checkpoint as C
    S, tr, _ = make_trainer(41)
    feed = S.synthetic_batches(4, "cuda", seed=3)
    for _ in range(2):
        tr.d_step(*next(feed))
    torch.cuda.synchronize()
    sd = tr.state_dict()
    assert sd[R.TABLE + '/Adam'].shape == (10, 128) and float(np.abs(sd[R.TABLE + '/Adam_1']).max()) > 0 and int(sd['Discriminator/adam_t']) == 2
    o, n = tr.d_flat['offsets'][R.TABLE], 1280
    prefix = str(tmp_path / "model.ckpt-1")
    C.write_checkpoint(prefix, C.checkpoint_from_trainer_state(sd))
    assert {R.TABLE, R.TABLE_U, R.TABLE + '/Adam', R.TABLE + '/Adam_1'} <= {nm for nm, _, _ in C.list_variables(prefix)}
    for how in ("state_dict", "tf_checkpoint"):
        tr2 = S.SNGANTrainer(batch_size=4, seed=99, use_graphs=False, projection=True)
        assert not torch.equal(tr2.store.vars[R.TABLE], tr.store.vars[R.TABLE])
        if how == "state_dict":
            tr2.load_state_dict(sd)
        else:
            assert len(C.optimistic_restore(tr2, prefix)) == len(tr.store.vars)
        for k in tr.store.vars:
            assert torch.equal(tr.store.vars[k], tr2.store.vars[k]), (how, k)
        assert tr2.d_flat['offsets'][R.TABLE] == o
        for slot in ('m', 'v'):
            assert torch.equal(tr.d_flat[slot][o:o + n], tr2.d_flat[slot][o:o + n]) and torch.equal(tr.d_flat[slot], tr2.d_flat[slot])
        assert int(tr2.d_opt.t) == 2
        tr2.d_step(*next(S.synthetic_batches(4, "cuda", seed=5)))                    # the restored trainer still steps
        assert bool(torch.isfinite(tr2.d_flat["params"]).all())


def test_default_trainer_in_the_same_process_keeps_the_concat_critic(K):
    S, tr_p, _ = make_trainer(3)
    tr = S.SNGANTrainer(batch_size=4, seed=3, use_graphs=False)
    assert tr.projection is False and tr_p.projection is True
    assert 'Discriminator/D.Embedding_y/W' in tr.store.vars and tr.store.param_count('Discriminator') == 1701689
    assert tuple(tr.store.vars['Discriminator/D.Block.2.Conv1/Filters'].shape) == (3, 3, 256, 256)
    assert tuple(tr.store.vars[R.TABLE].shape) == (10, 300) and R.TABLE_U not in tr.store.vars
    assert len([k for k in tr.store.vars if k.endswith('spectral_norm/u')]) == 12
    feed = S.synthetic_batches(4, "cuda", seed=2)
    for t in (tr, tr_p, tr):                   # interleaved: each trainer works on its own store
        t.d_step(*next(feed))
        t.g_step()
    torch.cuda.synchronize()
    g = tr.store.vars['Discriminator/D.Embedding_y/W']
    assert bool(torch.isfinite(tr.d_flat["params"]).all()) and bool(torch.isfinite(tr_p.d_flat["params"]).all())
    assert float((g - torch.tensor(np.asarray(tr.state_dict()['Discriminator/D.Embedding_y/W'])).cuda()).abs().max()) == 0.0
    assert int(tr.d_opt.t) == 2 and int(tr_p.d_opt.t) == 1


def test_data_parallel_path_with_a_world_size_one_group(K):
    """the projection critic through the data-parallel path (backend "nccl" = RCCL, world size 1): nothing there names the label
    branch -- same RNG consumption and step counts as the single-process trainer, parameters (the table among them) equal up to
    the order of fp32 atomics.  The body runs in tests/projection_rccl_worker.py, a process of its own (RCCL teardown)."""
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "projection_rccl_worker.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert "RCCL PATH OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.returncode == 0, f"projection_rccl_worker exited with {r.returncode}: {r.stderr[-3000:]}"
