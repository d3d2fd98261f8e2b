"""Host restatements of consistency regularisation (csrc/consistency.hip): the table draw on tests/philox_ref.py, the gather and the loss
with its gradients in NumPy (float64 where there is arithmetic), and the ACGAN critic loss with the term in float64 torch.

    L_cr  = w_real * mean_i (D(x_i) - D(T(x_i)))^2                         Zhang et al. 2020 (CR-GAN), eq. 7
    L_bcr = L_cr + w_fake * mean_i (D(G(z_i)) - D(T(G(z_i))))^2            Zhao et al. 2020 (bCR), eq. 1-2
    T: table row (flip, dx, dy) -> out[y, x] = in[R(y - dy, H), R(xf - dx, W)], xf = W - 1 - x where flip, R = np.pad(mode='reflect')
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref as P  # noqa: E402

DRAW_ADVANCE = 1                    # gank_cr_draw leaves offset + 1, as every other draw
WORDS_PER_ROW = 4                   # one Philox call a row: words 0, 1, 2 used, word 3 not


def mulhi(w, m):
    """floor(w * m / 2^32) of 32-bit words: the multiply-high map onto 0 .. m - 1"""
    return ((np.asarray(w, dtype=np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def draw_table(n, shift, seed, off):
    """gank_cr_draw: int32 [n, 3] = (word 0 >> 31, mulhi(word 1, 2 s + 1) - s, mulhi(word 2, 2 s + 1) - s) of Philox call i; exact"""
    w = P.words(n, seed, off)
    m = 2 * int(shift) + 1
    return np.stack([(w[:, 0] >> np.uint32(31)).astype(np.int64), mulhi(w[:, 1], m) - shift, mulhi(w[:, 2], m) - shift], axis=1).astype(np.int32)


def reflect(i, n):
    """R(i, n) for -n < i < 2 n - 1: the mirror that does not repeat the edge"""
    i = np.asarray(i, dtype=np.int64)
    assert n >= 1 and bool(((i > -n) & (i < 2 * n - 1)).all()), "the reflection is defined for shifts below the size"
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def augment(x, table):
    """gank_cr_augment on an array [B, H, W, C] of any dtype (a gather: the values are moved, never computed with)"""
    x, table = np.asarray(x), np.asarray(table)
    b, h, w, _ = x.shape
    assert table.shape == (b, 3)
    out = np.empty_like(x)
    for i, (flip, dx, dy) in enumerate(table.tolist()):
        xs = np.arange(w)
        cols = reflect((w - 1 - xs if flip else xs) - dx, w)
        rows = reflect(np.arange(h) - dy, h)
        out[i] = x[i][rows][:, cols]
    return out


def loss_and_grads(a, b, w):
    """float64: (w / B * sum (a - b)^2, dL/da = 2 w / B * (a - b), dL/db = -dL/da) for a, b of shape [B] or [B, C]"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = a - b
    k = float(w) / a.shape[0]
    return k * float((d * d).sum()), 2.0 * k * d, -2.0 * k * d


def loss_roundings(n):
    """fp32 roundings between the exact loss and the kernel's, for n = B C elements, by its order of summation: 3 a term (a - b, its
    square is two factors of it, the product), ceil(n / 256) - 1 thread-serial additions that round (the first adds to 0), 6 butterfly
    steps, 3 of the 4 wave additions, w / B and the product with it"""
    return 3 + (-(-n // 256) - 1) + 6 + 3 + 2


GRAD_ROUNDINGS = 3                  # a - b, w / B, their product (the doubling is exact)


def gamma(k):
    """Higham's gamma_k for fp32: k roundings of relative size 2^-24 compound to at most this"""
    u = 2.0 ** -24
    return k * u / (1.0 - k * u)


def acgan_d_loss(P_, real, real_labels, z, fake_labels, consistency, weights, table_real, table_fake=None, penalty='none', alpha=None, u=None):
    """grad_penalty_ref.acgan_d_loss plus the consistency term: every critic pass a call of its own (batch statistics of that batch)
    -> (total, parts); parts has cr_real, cr_fake, cr and the four sets of logits"""
    import torch
    import grad_penalty_ref as G
    from oracle import ref_torch as T
    total, parts = G.acgan_d_loss(P_, real, real_labels, z, fake_labels, penalty, 10.0, alpha, u)
    if consistency == 'none':
        return total, parts
    w_real, w_fake = weights
    d_real, _ = T.acgan_discriminator(P_, real)
    d_real_aug, _ = T.acgan_discriminator(P_, torch.from_numpy(augment(real.numpy(), table_real)))
    cr_real = w_real * ((d_real - d_real_aug) ** 2).mean()
    cr_fake = torch.zeros((), dtype=cr_real.dtype)
    parts.update(d_real=d_real.detach(), d_real_aug=d_real_aug.detach())
    if consistency == 'bcr':
        with torch.no_grad():
            x_fake = T.acgan_generator(P_, z, fake_labels)
        d_fake, _ = T.acgan_discriminator(P_, x_fake)
        d_fake_aug, _ = T.acgan_discriminator(P_, torch.from_numpy(augment(x_fake.numpy(), table_fake)))
        cr_fake = w_fake * ((d_fake - d_fake_aug) ** 2).mean()
        parts.update(d_fake=d_fake.detach(), d_fake_aug=d_fake_aug.detach())
    elif consistency != 'cr':
        raise ValueError(consistency)
    parts.update(cr_real=cr_real, cr_fake=cr_fake, cr=cr_real + cr_fake)
    return total + cr_real + cr_fake, parts
