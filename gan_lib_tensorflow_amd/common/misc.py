"""`get_loss` -- drop-in for common/misc.py:310-394 of the reference (the adversarial loss pair)."""
import torch

from .. import functional as Fn


def get_loss(disc_real, disc_fake, loss_type='HINGE'):
    """(d_loss, g_loss) for critic outputs on real / generated samples (misc.py:310-394).
      'HINGE'   (:326-335, the loss of the SNGAN and ACGAN scripts): mean(relu(1 - real)) + mean(relu(1 + fake)); -mean(fake)
      'WGAN'    (:328-336): -mean(real) + mean(fake); -mean(fake)
      'WGAN-GP' (:337-352): the same pair -- the reference leaves the penalty to the call site (ACGAN/train.py:99-107);
                use `gradient_penalty` below for it.
      'LSGAN'   (:353-360): (mean((1 - real)^2) + mean(fake^2)) / 2; mean((1 - fake)^2) / 2
      'CGAN'    (:361-372): sigmoid cross-entropy against ones / zeros; generator: against ones on the fakes
      'Modified_MiniMax' (:373-381): -mean(log sigmoid(real)) - mean(log(1 - sigmoid(fake))); -mean(log sigmoid(fake))
      'MiniMax' (:382-390): the same critic loss; generator mean(log(1 - sigmoid(fake)))
    One launch per loss computes the value and d loss / d logits (the sigmoid family through the stable softplus form)."""
    n_real = disc_real.reshape(-1).shape[0]
    fake = disc_fake.reshape(-1)
    both = Fn.concat_rows(disc_real.reshape(-1), fake)
    if loss_type == 'HINGE':
        return Fn.hinge_d_loss(both, n_real), Fn.hinge_g_loss(fake)
    if loss_type in ('WGAN', 'WGAN-GP'):
        return Fn.wgan_d_loss(both, n_real), Fn.hinge_g_loss(fake)        # -mean(disc_fake) in all three branches
    if loss_type == 'LSGAN':
        return Fn.gan_pointwise_loss(both, n_real, 0), Fn.gan_pointwise_loss(fake, 0, 1)
    if loss_type in ('CGAN', 'Modified_MiniMax'):
        return Fn.gan_pointwise_loss(both, n_real, 2), Fn.gan_pointwise_loss(fake, 0, 3)
    if loss_type == 'MiniMax':
        return Fn.gan_pointwise_loss(both, n_real, 2), Fn.gan_pointwise_loss(fake, 0, 4)
    raise NotImplementedError('loss_type %r (misc.py:310-394 knows HINGE, WGAN, WGAN-GP, LSGAN, CGAN, Modified_MiniMax, MiniMax)' % (loss_type,))


def gradient_penalty(gradients, weight=10.0, kind='two_sided', target=1.0):
    """weight * mean((sqrt(sum(g^2, axis=[1,2,3]) + 1e-10) - 1)^2)  -- the block the reference asks to paste at the call
    site (misc.py:341-349; ACGAN/train.py:104-106).  `gradients` must come from a critic built of `functional2` operators
    with create_graph=True so the penalty can be differentiated with respect to the critic's weights.
    With s = sqrt(sum(g^2) + 1e-10) per sample, `kind` selects the function of the slope, the caller the penalised point:
      'two_sided'  weight * mean((s - target)^2)          WGAN-GP at the interpolates; DRAGAN at real + 0.5 * std(real) * U[0, 1)
      'one_sided'  weight * mean(max(0, s - target)^2)    WGAN-LP at the interpolates
      'squared'    weight * mean(sum(g^2))                R1 at the real batch, R2 at the generated one; weight = gamma / 2"""
    from .. import functional2 as F2
    return F2.gradient_penalty(gradients, weight, kind, target)


def consistency_loss(logits, logits_aug, weight=10.0):
    """weight * mean_i ||D(x_i) - D(T(x_i))||^2  -- consistency regularisation (Zhang et al. 2020, CR-GAN, eq. 7): `logits` the critic's
    output on a batch, `logits_aug` its output on `augment` of the same batch, [B] or [B, C], 16-bit or float32.  On the real batch
    alone it is CR; with a second term on the generated batch (its own weight) bCR (Zhao et al. 2020).  Gradients flow into both
    passes; the term is differentiated once (it is no operand of a gradient penalty)."""
    from .. import functional2 as F2
    return F2.consistency_loss(logits, logits_aug, weight)


def augment(images, table, max_shift=None):
    """T of consistency_loss: NHWC 16-bit images and an int32 table [B, 3] = (flip, dx, dy), one row an image (kernels.cr_draw(B, shift,
    rng_state) draws one) -> out[b, y, x] = images[b, R(y - dy), R(xf - dx)], xf = W - 1 - x where flip != 0: each image shifted by
    (dx, dy) whole pixels, the pixels that come from outside mirrored as np.pad(mode='reflect') mirrors them (R), then flipped left to
    right where flip != 0.  A gather: exact, and no gradient flows through it (the
    augmented images are leaves of the critic update).  max_shift: the largest shift in the table, below min(H, W)."""
    from .. import kernels as K
    return K.cr_augment(images, table, max_shift)
