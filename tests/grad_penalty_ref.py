"""Float64 restatements (torch CPU, autograd) of the gradient penalties of csrc/acgan_ops.hip and of the ACGAN critic loss under each of
them, in the style of functional2_ref.GPLoss: plain formulas, differentiated by autograd.

    two_sided  lam * mean_n (s_n - target)^2            s_n = sqrt(sum_d g[n,d]^2 + 1e-10)
               WGAN-GP at the interpolates (Gulrajani et al. 2017), DRAGAN at real + 0.5 std(real) U[0,1) (Kodali et al. 2017)
    one_sided  lam * mean_n max(0, s_n - target)^2      WGAN-LP (Petzka et al. 2018)
    squared    lam * mean_n sum_d g[n,d]^2              R1 at the real batch, R2 at the generated one (Mescheder et al. 2018)
"""
import torch
import torch.nn.functional as F

from oracle import ref_torch as T

KINDS = ('two_sided', 'one_sided', 'squared')
# penalty of ACGANTrainer -> (kind, penalised point)
PENALTIES = {'wgan-gp': ('two_sided', 'interpolates'), 'wgan-lp': ('one_sided', 'interpolates'), 'dragan': ('two_sided', 'perturbed'),
             'r1': ('squared', 'real'), 'r2': ('squared', 'fake'), 'none': (None, None)}


def slopes(g):
    return torch.sqrt((g.reshape(g.shape[0], -1) ** 2).sum(dim=1) + 1e-10)


def GradPenalty(g, lam, target=1.0, kind='two_sided'):
    if kind == 'squared':
        return lam * (g.reshape(g.shape[0], -1) ** 2).sum(dim=1).mean()
    e = slopes(g) - target
    if kind == 'one_sided':
        e = torch.clamp(e, min=0.0)
    elif kind != 'two_sided':
        raise ValueError(kind)
    return lam * (e ** 2).mean()


def grad_penalty_and_derivative(g, lam, target=1.0, kind='two_sided'):
    gr = g.clone().requires_grad_(True)
    loss = GradPenalty(gr, lam, target, kind)
    (dg,) = torch.autograd.grad(loss, gr)
    return loss.detach(), dg


def dragan_sigma(real):
    """x.std() of the original: the population standard deviation (ddof 0) of every element"""
    return torch.sqrt(((real - real.mean()) ** 2).mean())


def dragan_perturb(real, u):
    return real + 0.5 * dragan_sigma(real) * u.reshape(real.shape)


def acgan_d_loss(P, real, real_labels, z, fake_labels, penalty='wgan-gp', weight=10.0, alpha=None, u=None):
    """oracle.ref_torch.acgan_d_loss with the penalty term of `penalty`: hinge + weight * penalty at its point + class cross-entropy
    on the real batch -> (total, parts); parts['slopes'] are the slopes at the penalised point."""
    kind, point = PENALTIES[penalty]
    with torch.no_grad():
        x_fake = T.acgan_generator(P, z, fake_labels)
    disc_real, ac_real = T.acgan_discriminator(P, real)
    disc_fake, _ = T.acgan_discriminator(P, x_fake)
    d_gan = torch.relu(1. - disc_real).mean() + torch.relu(1. + disc_fake).mean()
    d_ac = F.cross_entropy(ac_real, real_labels.long())
    if kind is None:
        return d_gan + d_ac, dict(d_gan=d_gan, gp=torch.zeros((), dtype=d_gan.dtype), d_ac=d_ac)
    if point == 'interpolates':
        x = real + alpha.reshape(-1, 1, 1, 1) * (x_fake - real)
    elif point == 'perturbed':
        x = dragan_perturb(real, u)
    else:
        x = real if point == 'real' else x_fake
    x = x.detach().clone().requires_grad_(True)
    d_x, _ = T.acgan_discriminator(P, x)
    (grads,) = torch.autograd.grad(d_x.sum(), x, create_graph=True)
    gp = GradPenalty(grads, weight, 1.0, kind)
    return d_gan + gp + d_ac, dict(d_gan=d_gan, gp=gp, d_ac=d_ac, slopes=slopes(grads).detach(), grads=grads)
