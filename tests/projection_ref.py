"""Float64 restatement of the projection discriminator (Miyato & Koyama, "cGANs with Projection Discriminator") on the
SNGAN critic, built from the oracle's pieces (oracle.ref_torch: _Ctx, meanpool2x2, spectral_normed_weight, _st), plus a NumPy
float64 projection head with its gradients in closed form.  Test instrument only: the product never imports it.

The critic:  OptimizedResBlockDisc1 -> D.Block.2 (128 -> 128, 'down', no label concat) -> D.Block.3 / D.Block.4 -> relu ->
reduce_mean over H and W (the reference's pooling, not the paper's sum) -> h;  logits = D.Output(h) + <E_bar[y], h> with
E = `Embedding.Label/embedding_map` [10, 128], E_bar = E / sigma(E) by the reference's spectral_normed_weight with
u = `Embedding.Label/embedding_map/spectral_norm/u` [1, 128].  No D.Embedding_y."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import ref_torch as T

DIM_D = T.DIM_D
VOCAB = T.N_LABELS
TABLE = 'Discriminator/Embedding.Label/embedding_map'
TABLE_U = TABLE + '/spectral_norm/u'
CRITIC_PARAMS = 1055105          # 1 701 689 of the concat critic - 646 584 (D.Embedding_y, the 300-wide table, half of D.Block.2's inputs)


def init_projection_params(seed=0):
    """The generator of oracle.ref_torch.init_sngan_params(seed), unchanged, and the critic's variables in projection mode, in
    creation order."""
    base = T.init_sngan_params(seed)
    P = OrderedDict((k, v) for k, v in base.items() if k.startswith('Generator/'))
    rng = np.random.default_rng(seed + 7919)
    d = 'Discriminator'

    def conv(name, k, cin, cout, he_init=True):
        P[f'{d}/{name}/Filters'] = T.conv_init(rng, k, cin, cout, he_init)
        P[f'{d}/{name}/filters/spectral_norm/u'] = T.trunc_normal(rng, (1, cout))
        P[f'{d}/{name}/Biases'] = np.zeros(cout, 'float32')

    conv('D.Block.1.Shortcut', 1, 3, DIM_D, he_init=False)
    conv('D.Block.1.Conv1', 3, 3, DIM_D)
    conv('D.Block.1.Conv2', 3, DIM_D, DIM_D)
    conv('D.Block.2.Shortcut', 1, DIM_D, DIM_D, he_init=False)
    conv('D.Block.2.Conv1', 3, DIM_D, DIM_D)
    conv('D.Block.2.Conv2', 3, DIM_D, DIM_D)
    for i in (3, 4):
        conv(f'D.Block.{i}.Conv1', 3, DIM_D, DIM_D)
        conv(f'D.Block.{i}.Conv2', 3, DIM_D, DIM_D)
    P[f'{d}/D.Output/W'] = T.linear_init(rng, DIM_D, 1)
    P[f'{d}/D.Output/spectral_norm/u'] = T.trunc_normal(rng, (1, 1))
    P[f'{d}/D.Output/b'] = np.zeros(1, 'float32')
    P[TABLE] = rng.uniform(-0.08, 0.08, (VOCAB, DIM_D)).astype('float32')          # embedding.py:33-36
    P[TABLE_U] = T.trunc_normal(rng, (1, DIM_D))
    return P


def critic_features(c, x):
    """the label-free trunk -> pooled features h [n, 128]; c: a T._Ctx on the 'Discriminator' scope"""
    _st = T._st
    x = x.reshape(-1, 32, 32, 3)
    shortcut = _st(c.conv(T.meanpool2x2(x), 'D.Block.1.Shortcut', sn=True), 'd')
    h = _st(c.conv(x, 'D.Block.1.Conv1', sn=True), 'd')
    h = T.meanpool2x2(c.conv(torch.relu(h), 'D.Block.1.Conv2', sn=True))
    out = _st(shortcut + h, 'd')
    shortcut = _st(T.meanpool2x2(c.conv(out, 'D.Block.2.Shortcut', sn=True)), 'd')
    h = _st(c.conv(torch.relu(out), 'D.Block.2.Conv1', sn=True), 'd')
    h = T.meanpool2x2(c.conv(torch.relu(h), 'D.Block.2.Conv2', sn=True))
    out = _st(shortcut + h, 'd')
    for i in (3, 4):
        h = _st(c.conv(torch.relu(out), f'D.Block.{i}.Conv1', sn=True), 'd')
        h = c.conv(torch.relu(h), f'D.Block.{i}.Conv2', sn=True)
        out = _st(out + h, 'd')
    return _st(torch.relu(out).mean(dim=(1, 2)), 'd')


def projection_parts(P, x, labels, normalise_table=True):
    """-> dict(h, plain, E_bar, proj, logits, new_u): pooled features, D.Output(h) [n], the normalised table, the projection term
    [n] and their sum.  normalise_table=False uses the stored table as E_bar (an all-zero table has sigma = 0: its normalised
    form is 0 / 0 in the reference's formula)."""
    c = T._Ctx(P, 'Discriminator', True)
    h = critic_features(c, x)
    plain = c.linear(h, 'D.Output', sn=True).reshape(-1)
    E = P[TABLE]
    if normalise_table:
        E_bar, u_new, _ = T.spectral_normed_weight(E, P[TABLE_U])
        c.new_u[TABLE_U] = u_new.detach()
    else:
        E_bar = E
    proj = (E_bar[labels] * h).sum(dim=1)
    return dict(h=h, plain=plain, E_bar=E_bar, proj=proj, logits=T._st(plain + proj, 'd'), new_u=c.new_u)


def discriminator_projection(P, x, labels, normalise_table=True):
    """-> (logits [n], {u name: new u})"""
    parts = projection_parts(P, x, labels, normalise_table)
    return parts['logits'], parts['new_u']


def d_logits_fn(P, real_u8, labels, z, deq_noise, towers=2, real_pre=None):
    """the critic's logits of one D step (the graph of T.d_loss_fn) -> (logits [2b], new_u)"""
    fake = T.generator(P, z, labels, groups=towers)
    real = T.preprocess_real(real_u8, deq_noise, z.dtype) if real_pre is None else real_pre
    return discriminator_projection(P, torch.cat([real, fake], 0), torch.cat([labels, labels], 0))


def d_loss_fn(P, real_u8, labels, z, deq_noise, towers=2, real_pre=None):
    """T.d_loss_fn with the projection critic -> (hinge loss, new_u, logits)"""
    logits, new_u = d_logits_fn(P, real_u8, labels, z, deq_noise, towers, real_pre)
    b = logits.shape[0] // 2
    return torch.relu(1. - logits[:b]).mean() + torch.relu(1. + logits[b:]).mean(), new_u, logits


def g_loss_fn(P, z, fake_labels, towers=2):
    """T.g_loss_fn with the projection critic (u read, never written) -> (loss, logits)"""
    fake = T.generator(P, z, fake_labels, groups=towers)
    logits, _ = discriminator_projection(P, fake, fake_labels)
    return -logits.mean(), logits


# ------------------------------------------------------------------ NumPy float64 head
def _rows(E, labels):
    """E[labels], a zero row for a label outside [0, V) (gank_embedding_fwd's convention)"""
    E, labels = np.asarray(E, np.float64), np.asarray(labels)
    ok = (labels >= 0) & (labels < E.shape[0])
    rows = np.zeros((labels.shape[0], E.shape[1]), np.float64)
    rows[ok] = E[labels[ok]]
    return rows, ok


def head_logits(x, w, b, E, labels):
    """logits[n] = sum_c x[n][c] (w[c] + E[y_n][c]) + b"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(-1)
    rows, _ = _rows(E, labels)
    return (x * (w[None, :] + rows)).sum(axis=1) + (0.0 if b is None else float(np.asarray(b).reshape(-1)[0]))


def head_abs_terms(x, w, E, labels):
    """sum_c |x[n][c]| |w[c] + E[y_n][c]|: the scale of a logit's fp32 accumulation error"""
    rows, _ = _rows(E, labels)
    return (np.abs(np.asarray(x, np.float64)) * np.abs(np.asarray(w, np.float64).reshape(-1)[None, :] + rows)).sum(axis=1)


def head_grads(dl, x, w, E, labels):
    """closed form -> (dx [M,K], dw [K], db, dE [V,K]) for an upstream dl [M]"""
    dl, x, w = np.asarray(dl, np.float64), np.asarray(x, np.float64), np.asarray(w, np.float64).reshape(-1)
    rows, ok = _rows(E, labels)
    dx = dl[:, None] * (w[None, :] + rows)
    dw = (dl[:, None] * x).sum(axis=0)
    dE = np.zeros(np.asarray(E).shape, np.float64)
    np.add.at(dE, np.asarray(labels)[ok], (dl[:, None] * x)[ok])
    return dx, dw, dl.sum(), dE


def hinge(logits, n_real, mode):
    """mode 0: mean(relu(1 - l[:n_real])) + mean(relu(1 + l[n_real:])); mode 1: -mean(l) -> (loss, d loss / d logits)"""
    l = np.asarray(logits, np.float64)
    if mode == 1:
        return -l.mean(), np.full(l.shape, -1.0 / l.size)
    real, fake = l[:n_real], l[n_real:]
    d = np.concatenate([-(1. - real > 0).astype(np.float64) / real.size, (1. + fake > 0).astype(np.float64) / fake.size])
    return np.maximum(1. - real, 0).mean() + np.maximum(1. + fake, 0).mean(), d
