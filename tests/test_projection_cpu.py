"""CPU: the projection discriminator without a device -- the float64 restatement (tests/projection_ref.py) against answers that
do not depend on it, the name rule that puts the label table into the critic's batched spectral norm, the pinned variable names
and parameter count, and every refusal that is decided on the host."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import projection_ref as R  # noqa: E402
from oracle import ref_ops  # noqa: E402
from oracle import ref_torch as T  # noqa: E402


@pytest.fixture(scope="module")
def small():
    """parameters and a batch of three images (labels 3, 3, 7) in float64"""
    P = T.to_torch(R.init_projection_params(2))
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.uniform(-1, 1, (3, 3072)))
    labels = torch.tensor([3, 3, 7])
    return P, x, labels


def test_all_zero_table_leaves_the_plain_critic(small):
    """E = 0: the logits are D.Output on the same trunk.  (sigma(0) = 0, so E / sigma is 0 / 0 in the reference's formula: the
    restatement is asked to use the stored table as E_bar.)"""
    P, x, labels = small
    Q = dict(P)
    Q[R.TABLE] = torch.zeros_like(P[R.TABLE])
    with torch.no_grad():
        logits, _ = R.discriminator_projection(Q, x, labels, normalise_table=False)
        c = T._Ctx(P, 'Discriminator', True)
        plain = c.linear(R.critic_features(c, x), 'D.Output', sn=True).reshape(-1)
    assert float((logits - plain).abs().max()) <= 1e-12
    assert float(plain.abs().max()) > 1e-3


def test_projection_term_is_one_hot_times_table_times_features(small):
    P, x, labels = small
    with torch.no_grad():
        parts = R.projection_parts(P, x, labels)
    onehot = torch.nn.functional.one_hot(labels, R.VOCAB).to(torch.float64)
    for n in range(x.shape[0]):
        want = onehot[n] @ parts['E_bar'] @ parts['h'][n]
        assert abs(float(parts['proj'][n] - want)) <= 1e-12
    assert float((parts['logits'] - parts['plain'] - parts['proj']).abs().max()) <= 1e-12
    assert float(parts['proj'].abs().max()) > 1e-4                      # the term is not trivially zero
    assert float((parts['proj'][0] - parts['proj'][1]).abs()) > 0       # same label, different features


def test_closed_form_head_gradients_equal_autograd():
    rng = np.random.default_rng(3)
    M, K, V = 7, 64, 3
    x, w, b, E = rng.normal(size=(M, K)), rng.normal(size=K), rng.normal(size=1), rng.normal(size=(V, K))
    labels = np.array([2, 0, 2, 2, 0, 2, 0])                            # label 1 never occurs
    dl = rng.normal(size=M)
    tx, tw, tb, tE = (torch.tensor(a, requires_grad=True) for a in (x, w, b, E))
    logits = (tx * (tw[None, :] + tE[torch.tensor(labels)])).sum(dim=1) + tb
    assert np.abs(logits.detach().numpy() - R.head_logits(x, w, b, E, labels)).max() <= 1e-12
    gx, gw, gb, gE = torch.autograd.grad(logits, [tx, tw, tb, tE], torch.tensor(dl))
    dx, dw, db, dE = R.head_grads(dl, x, w, E, labels)
    for got, ref in ((dx, gx), (dw, gw), (db, gb), (dE, gE)):
        assert np.abs(np.asarray(got) - ref.numpy().reshape(np.shape(got))).max() <= 1e-12
    assert not dE[1].any()
    for mode, n_real in ((0, 3), (1, 0)):
        tl = torch.tensor(logits.detach().numpy(), requires_grad=True)
        loss = -tl.mean() if mode else torch.relu(1 - tl[:n_real]).mean() + torch.relu(1 + tl[n_real:]).mean()
        val, d = R.hinge(tl.detach().numpy(), n_real, mode)
        assert abs(val - float(loss.detach())) <= 1e-12 and np.abs(d - torch.autograd.grad(loss, tl)[0].numpy()).max() <= 1e-12
    # a label outside [0, V): a zero row, no table gradient
    lab2 = np.array([2, 0, 5, 2, -1, 2, 0])
    ok = np.array([1, 1, 0, 1, 0, 1, 1], bool)
    assert np.abs(R.head_logits(x, w, b, E, lab2)[~ok] - (x[~ok] @ w + b)).max() <= 1e-12
    assert np.abs(R.head_grads(dl, x, w, E, lab2)[3] - R.head_grads(dl[ok], x[ok], w, E, lab2[ok])[3]).max() <= 1e-12


def test_table_sigma_and_new_u_equal_the_numpy_oracle(small):
    P, x, labels = small
    with torch.no_grad():
        parts = R.projection_parts(P, x, labels)
    E, u = P[R.TABLE].detach().numpy(), P[R.TABLE_U].numpy()
    W_bar, u1, sigma, _ = ref_ops.sn_forward(E, u)
    assert W_bar.shape == (R.VOCAB, R.DIM_D) and u1.shape == (1, R.DIM_D)
    assert np.abs(parts['E_bar'].numpy() - W_bar).max() <= 1e-12 * np.abs(W_bar).max()
    assert np.abs(parts['new_u'][R.TABLE_U].numpy() - u1).max() <= 1e-12
    _, _, sig_t = T.spectral_normed_weight(P[R.TABLE].detach(), P[R.TABLE_U])
    assert abs(float(sig_t) - sigma) <= 1e-12 * sigma


def _cpu_store(P):
    from gan_lib_tensorflow_amd.store import ParamStore
    store = ParamStore('cpu')
    for k, v in P.items():
        store.vars[k] = torch.tensor(np.asarray(v))
        store.trainable[k] = not T.is_state(k)
    return store


def test_sn_pairs_knows_the_table_and_keeps_the_old_pairs():
    from gan_lib_tensorflow_amd.common.ops import sn
    store = _cpu_store(R.init_projection_params(0))
    pairs = sn.sn_pairs(store, 'Discriminator', with_names=True)
    assert len(pairs) == 12
    by_name = {nm: (w, u) for w, u, nm in pairs}
    w, u = by_name[R.TABLE]
    assert w is store.vars[R.TABLE] and u is store.vars[R.TABLE_U]
    assert by_name['Discriminator/D.Output/W'][1] is store.vars['Discriminator/D.Output/spectral_norm/u']
    assert [nm for _, _, nm in pairs][-1] == R.TABLE                 # created behind D.Output
    # a concat-mode store: exactly the pairs of the two older rules
    P = T.init_sngan_params(0)
    store = _cpu_store(P)
    want = []
    for name in P:
        if not name.startswith('Discriminator/'):
            continue
        if name.endswith('/filters/spectral_norm/u'):
            want.append((name[:-len('/filters/spectral_norm/u')] + '/Filters', name))
        elif name.endswith('/spectral_norm/u'):
            want.append((name[:-len('/spectral_norm/u')] + '/W', name))
    got = sn.sn_pairs(store, 'Discriminator', with_names=True)
    assert len(got) == 12 and [nm for _, _, nm in got] == [w for w, _ in want]
    assert all(w is store.vars[wn] and u is store.vars[un] for (w, u, _), (wn, un) in zip(got, want))
    assert sn.sn_pairs(store, 'Generator') == []


def test_pinned_names_and_parameter_count():
    P = R.init_projection_params(0)
    d = [k for k in P if k.startswith('Discriminator/')]
    assert not any('D.Embedding_y' in k for k in d)
    assert P[R.TABLE].shape == (10, 128) and P[R.TABLE_U].shape == (1, 128)
    assert P['Discriminator/D.Block.2.Conv1/Filters'].shape == (3, 3, 128, 128)
    assert P['Discriminator/D.Block.2.Shortcut/Filters'].shape == (1, 1, 128, 128)
    assert P['Discriminator/D.Block.2.Conv2/Filters'].shape == (3, 3, 128, 128)
    assert len([k for k in d if k.endswith('spectral_norm/u')]) == 12
    assert sum(P[k].size for k in T.trainable_names(P, 'Discriminator')) == R.CRITIC_PARAMS == 1055105
    g = T.init_sngan_params(0)
    assert [k for k in P if k.startswith('Generator/')] == [k for k in g if k.startswith('Generator/')]
    assert all(np.array_equal(P[k], g[k]) for k in P if k.startswith('Generator/'))
    assert abs(float(np.abs(P[R.TABLE]).max()) - 0.08) < 0.002


def test_projection_without_labels_is_refused(monkeypatch):
    from gan_lib_tensorflow_amd.SNGAN import gan_cifar_resnet as S
    assert S.PROJECTION is False
    monkeypatch.setattr(S, 'CONDITIONAL', False)
    with pytest.raises(ValueError, match="CONDITIONAL"):
        S.Discriminator(None, None, projection=True)
    with pytest.raises(ValueError, match="CONDITIONAL"):
        S.SNGANTrainer(batch_size=4, device='cpu', projection=True)


def test_wrappers_refuse_bad_operands_on_the_host():
    from gan_lib_tensorflow_amd import kernels as K
    M, Kd, V = 4, 8, 3
    x = torch.zeros((M, Kd), dtype=K.BF16)
    w, b, E = torch.zeros(Kd), torch.zeros(1), torch.zeros((V, Kd))
    labels = torch.zeros(M, dtype=torch.int32)
    dl = torch.zeros(M, dtype=K.BF16)
    with pytest.raises(ValueError, match="E must be"):
        K.proj_head_fwd(x, w, b, torch.zeros((V, Kd + 1)), labels)
    with pytest.raises(ValueError, match="w must be"):
        K.proj_head_fwd(x, torch.zeros(Kd + 1), b, E, labels)
    with pytest.raises(ValueError, match="labels must be"):
        K.proj_head_hinge(x, w, b, E, labels[:-1], 2, 0)
    with pytest.raises(ValueError, match="x must be"):
        K.proj_head_fwd(x.reshape(-1), w, b, E, labels)
    with pytest.raises(ValueError, match="e_grad must be"):
        K.proj_head_bwd(dl, x, w, E, labels, e_grad=torch.zeros((V + 1, Kd)))
    with pytest.raises(RuntimeError, match="labels must be torch.int32"):
        K.proj_head_fwd(x, w, b, E, labels.long())
    with pytest.raises(RuntimeError, match="x must be"):
        K.proj_head_fwd(x.float(), w, b, E, labels)
    with pytest.raises(RuntimeError, match="dl must be"):
        K.proj_head_bwd(dl.float(), x, w, E, labels)
    with pytest.raises(RuntimeError, match="w_grad must be"):
        K.proj_head_hinge(x, w, b, E, labels, 2, 0, w_grad=torch.zeros(Kd, dtype=torch.float64))
    for call in (lambda: K.proj_head_fwd(x, w, b, E, labels), lambda: K.proj_head_bwd(dl, x, w, E, labels),
                 lambda: K.proj_head_hinge(x, w, b, E, labels, 2, 0)):
        with pytest.raises(RuntimeError, match="must live on the GPU"):
            call()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from gan_lib_tensorflow_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)          # never dereferenced: every call below is refused by the argument checks

    def err():
        return lib.gank_last_error().decode()

    assert lib.gank_proj_head_fwd(None, fake, None, fake, fake, fake, 4, 128, 10, None) != 0 and "null pointer" in err()
    assert lib.gank_proj_head_fwd(fake, fake, None, fake, fake, None, 4, 128, 10, None) != 0 and "null pointer" in err()
    for m, k, v in ((0, 128, 10), (1025, 128, 10), (4, 0, 10), (4, 1025, 10), (4, 128, 0), (4, 128, 257)):
        assert lib.gank_proj_head_fwd(fake, fake, None, fake, fake, fake, m, k, v, None) != 0 and "unsupported shape" in err()
    assert lib.gank_proj_head_bwd(None, fake, fake, fake, fake, fake, None, None, None, 4, 128, 10, None) != 0 and "null pointer" in err()
    assert lib.gank_proj_head_bwd(fake, fake, fake, None, fake, fake, None, None, None, 4, 128, 10, None) != 0 and "null pointer" in err()
    assert lib.gank_proj_head_bwd(fake, fake, fake, fake, fake, fake, None, None, None, 2000, 128, 10, None) != 0 and "unsupported shape" in err()
    one = C.c_float(1.0)
    args = (fake, fake, None, fake, fake, fake, fake, None, None, None, None)
    assert lib.gank_proj_head_hinge_scaled(*args, 8, 128, 10, 0, 0, one, None) != 0 and "n_real must split" in err()
    assert lib.gank_proj_head_hinge_scaled(*args, 8, 128, 10, 8, 0, one, None) != 0 and "n_real must split" in err()
    assert lib.gank_proj_head_hinge_scaled(*args, 8, 128, 10, 4, 2, one, None) != 0 and "mode" in err()
    assert lib.gank_proj_head_hinge_scaled(*args, 8, 128, 10, 4, 0, C.c_float(0.0), None) != 0 and "loss_scale" in err()
    assert lib.gank_proj_head_hinge_scaled(fake, fake, None, fake, fake, fake, None, None, None, None, None, 8, 128, 10, 4, 0, one, None) != 0
    assert "null pointer" in err()
