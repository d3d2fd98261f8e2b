"""ACGAN train step -- the loop body of ACGAN/train.py:89-201 of the reference (BASELINE.json config 3).

One step (train.py:194-204) = 1 generator update (skipped at step 0) + n_dis = 5 critic updates:
    critic loss    = hinge(D(real), D(G(z, fake_labels)))                                   (misc.get_loss, :96)
                   + 10 * mean((||grad_x D(x_hat)||_2 - 1)^2),  x_hat = real + alpha (fake - real)   (:99-107)
                   + mean softmax cross-entropy of the class head on the real batch          (:111-114)
    generator loss = -mean(D(G(z))) + acgan_scale_G * cross-entropy of the class head on the fakes (:117-121)
(the second term is the default of `ACGANTrainer(penalty=...)`: PENALTIES below has the one-sided, DRAGAN, R1 and R2 terms and 'none';
`ACGANTrainer(consistency='cr' | 'bcr')` adds consistency regularisation, CONSISTENCY below, to the critic loss)
both with tf.train.AdamOptimizer(beta1=0, beta2=0.9) at a learning rate that decays linearly from 4e-4 to 2e-4 over
max_iter / 2 generator steps (tf.train.polynomial_decay on `global_step`, :141-148).

Data parallel (config 3: global batch 256 over 8 GPUs): one process per GPU, each rank a replica with batch/world
samples and its own batch-norm statistics (as the reference's towers would have); flat gradient buffers summed with one
RCCL all-reduce per update, 1/world applied inside the Adam kernel.
"""
import numbers

import numpy as np
import torch

from .. import functional as Fn
from .. import functional2 as F2
from .. import kernels as K
from .. import trainer
from ..store import set_default_store
from .model import ACGAN


def polynomial_decay(step, lr0=0.0004, decay_steps=50000, lr_end=0.0002):
    """tf.train.polynomial_decay(power=1, cycle=False) with the script's values   (train.py:141)"""
    return trainer.polynomial_decay(step, lr0, decay_steps, lr_end)


BATCHED_PREP = True     # operand copies of the weights: one launch per network and update (False: per conv and layout on first use)


def _g_prep_kind(name, W):
    """operand layout per generator weight (kernels.prep_weights_batched), by the kernel its conv wrapper picks: the UpsampleConv
    3x3 layers run phase-decomposed, the 16x16 conv of G.2 on the image-resident kernel where its shape allows; a wrapper that
    wants another layout than the one attached prepares its own."""
    if W.dim() != 4:
        return None
    # (the same choices as the SNGAN generator's, whose blocks these are: SNGAN/gan_cifar_resnet.py _g_prep_kind)
    if Fn.RES8_CONV and name.endswith(('G.1.Conv1/Filters', 'G.1.Conv2/Filters')) and W.shape[0] == 3 and W.shape[2] in (128, 256) and W.shape[3] % 128 == 0:
        return 4                      # 8x8 images: LDS-resident kernel, fragment-major operands
    if Fn.PHASE_UPCONV and name.endswith('.Conv1/Filters') and W.shape[0] == 3:
        return 1
    if Fn.IMG16_CONV and name.endswith('G.2.Conv2/Filters') and W.shape[0] == 3 and W.shape[2] % 128 == 0 and W.shape[3] % 128 == 0:
        return 4                      # 16x16 image-resident conv
    return 0


# The critic's gradient regulariser: penalty -> (the function of the slope, kernels.GRAD_PENALTY_KINDS; the penalised point)
PENALTIES = {
    'wgan-gp': ('two_sided', 'interpolates'),     # Gulrajani et al. 2017: the reference's term (train.py:99-107)
    'wgan-lp': ('one_sided', 'interpolates'),     # Petzka et al. 2018
    'dragan': ('two_sided', 'perturbed'),         # Kodali et al. 2017: real + 0.5 * std(real) * U[0, 1)
    'r1': ('squared', 'real'),                    # Mescheder et al. 2018; penalty_weight = gamma / 2
    'r2': ('squared', 'fake'),
    'none': (None, None),
}


def check_penalty(penalty, penalty_weight, penalty_every):
    """the constructor's checks, before any device work"""
    if penalty not in PENALTIES:
        raise ValueError(f"penalty {penalty!r}: one of {', '.join(PENALTIES)}")
    if isinstance(penalty_every, bool) or not isinstance(penalty_every, numbers.Real) or int(penalty_every) != penalty_every or penalty_every < 1:
        raise ValueError(f"penalty_every {penalty_every!r}: a whole number of critic updates, at least 1")
    if penalty != 'none' and (isinstance(penalty_weight, bool) or not isinstance(penalty_weight, numbers.Real) or not penalty_weight > 0):
        raise ValueError(f"penalty_weight {penalty_weight!r} with penalty {penalty!r}: a positive weight (penalty='none' switches the term off)")


# Consistency regularisation of the critic, a further summand of its loss on every update:
#   'cr'   w_real * mean_i (D(x_i) - D(T(x_i)))^2                       Zhang et al. 2020 (CR-GAN), eq. 7
#   'bcr'  the same + w_fake * mean_i (D(G(z_i)) - D(T(G(z_i))))^2       Zhao et al. 2020 (bCR), eq. 1-2
# D the adversarial logit, T a random horizontal flip and a random shift by up to consistency_shift whole pixels in each axis with
# the outside mirrored (kernels.cr_draw / cr_augment).  The augmented images are leaves; gradients flow into both passes.
CONSISTENCY = ('none', 'cr', 'bcr')
IMAGE_SIZE = 32


def check_consistency(consistency, consistency_weight, consistency_shift):
    """the constructor's checks, before any device work -> (w_real, w_fake)"""
    if consistency not in CONSISTENCY:
        raise ValueError(f"consistency {consistency!r}: one of {', '.join(CONSISTENCY)}")
    if consistency == 'none':
        return 0.0, 0.0                  # (asks for no weight and no shift)
    pair = tuple(consistency_weight) if isinstance(consistency_weight, (tuple, list)) else (consistency_weight, consistency_weight)
    if len(pair) != 2 or any(isinstance(w, bool) or not isinstance(w, numbers.Real) or not 0 < w < float('inf') for w in pair):
        raise ValueError(f"consistency_weight {consistency_weight!r} with consistency {consistency!r}: a positive weight, or a pair "
                         "(w_real, w_fake) of them (consistency='none' switches the term off)")
    s = consistency_shift
    if isinstance(s, bool) or not isinstance(s, numbers.Real) or int(s) != s or not 0 <= s < IMAGE_SIZE:
        raise ValueError(f"consistency_shift {s!r}: a whole number of pixels, 0 .. {IMAGE_SIZE - 1} (the mirror rule ends at the image's size)")
    return float(pair[0]), float(pair[1])


class _Losses(dict):
    """the reported loss terms.  With consistency='none' the dict holds the terms it always held, and a lookup of a consistency term
    answers a zero constant without storing it."""
    ABSENT = ('consistency', 'consistency_real', 'consistency_fake')

    def __missing__(self, key):
        if key in self.ABSENT and 'd_loss_gan' in self:
            return Fn.constant_like(self['d_loss_gan'], 0.0)
        raise KeyError(key)


class ACGANTrainer(trainer.SampleMetrics, trainer.GraphTrainer):
    def __init__(self, batch_size=64, z_dim=128, acgan_scale_G=0.1, n_dis=5, max_iter=100000, device="cuda", seed=0,
                 process_group=None, state=None, use_graphs=True, allow_eager_fallback=False, penalty='wgan-gp', penalty_weight=10.0,
                 penalty_every=1, consistency='none', consistency_weight=10.0, consistency_shift=4):
        """penalty: the critic's gradient regulariser (PENALTIES), `penalty_weight` its weight.  penalty_every = k > 1 is the lazy
        regularisation of StyleGAN2 (Karras et al. 2020, appendix B): the term is added on the critic updates whose count is a
        multiple of k, with weight k * penalty_weight; the others run the 'none' form.  `state` may be a `state_dict()` of this
        trainer: the variables and the count of critic updates.
        consistency: 'cr' or 'bcr' adds consistency regularisation (CONSISTENCY) to every critic update, lazy or not, at
        `consistency_weight` (one weight, or (w_real, w_fake)) under flips and shifts of up to `consistency_shift` pixels."""
        check_penalty(penalty, penalty_weight, penalty_every)
        self.consistency_weights = check_consistency(consistency, consistency_weight, consistency_shift)
        super().__init__(device, seed, process_group, use_graphs, allow_eager_fallback)
        self.losses = _Losses()
        self.consistency_tables, self._d_tables = {}, {}       # the augmentations of the last critic update: 'real' (and 'fake') -> int32 [B, 3]
        self.consistency, self.consistency_shift = consistency, int(consistency_shift) if consistency != 'none' else 0
        self.batch, self.z_dim, self.scale_g, self.n_dis, self.max_iter = batch_size, z_dim, acgan_scale_G, n_dis, max_iter
        self.penalty, self.penalty_every = penalty, int(penalty_every)
        self.penalty_weight = float(penalty_weight) if isinstance(penalty_weight, numbers.Real) else 0.0      # ('none' asks for no weight)
        self.d_updates = 0               # critic updates taken: chooses the form of the next one on the host, outside any capture
        self._d_losses = {}              # graph key -> the loss tensors that form of the critic update writes
        if state is not None and '_d_updates' in state:
            state = dict(state)
            self.d_updates = int(state.pop('_d_updates'))
        self.model = ACGAN()
        self.global_step = 0
        # build once (variables are created by name on first use)
        with torch.no_grad():
            labels = torch.zeros(batch_size, dtype=torch.int32, device=self.device)
            z = torch.zeros((batch_size, z_dim), dtype=K.BF16, device=self.device)
            x = self.model.get_generator(z, labels)
            self.model.get_discriminator(x, labels)
        self._finish_build(state, g_adam=(0.0004, 0.0, 0.9), d_adam=(0.0004, 0.0, 0.9))
        self._g_convs = [(k, v) for k, v in self.store.vars.items() if k.startswith('g_net/') and k.endswith('/Filters') and v.dim() == 4]
        self._refresh_g_prep()
        # the static inputs of the captured updates
        self.real_u8 = torch.zeros((batch_size, 3072), dtype=torch.uint8, device=self.device)
        self.real_labels = torch.zeros(batch_size, dtype=torch.int32, device=self.device)

    def _flatten_nets(self, state, g_prefix, d_prefix):
        super()._flatten_nets(state, g_prefix, d_prefix)
        for p in self.d_params:
            p.grad = p.main_grad         # the twice-differentiable critic RETURNS weight gradients: autograd adds them in place here
            del p.main_grad

    def _apply(self, opt):
        """Adam without the gradient clear (_d_fwd_bwd / _g_fwd_bwd zero the buffers themselves), then the generator's operands"""
        f = opt['flat']
        K.adam_tf(f['params'], f['grads'], f['m'], f['v'], opt['hp'], opt['t'], None)
        if opt is self.g_opt:
            self._refresh_g_prep()

    def _refresh_g_prep(self):
        """The generator's MFMA operand copies, once per generator update in ONE launch (every pass until the next update -- the
        fakes of the critic updates, the generator's own forward / backward -- picks them up from the variables) instead of one
        or two launches per conv and pass."""
        if BATCHED_PREP and self._g_convs:
            K.prep_weights_batched([v for _, v in self._g_convs], want_d=True, kinds=[_g_prep_kind(k, v) for k, v in self._g_convs])

    def _learning_rate(self):
        return polynomial_decay(self.global_step, decay_steps=self.max_iter // 2)

    # ---- the two losses (eager; explicit inputs override the device RNG for parity tests) -----------------------------
    def d_loss(self, real, real_labels, z=None, fake_labels=None, alpha=None, u=None, penalise=True, table_real=None, table_fake=None):
        """penalise=False: the form of an update that carries no penalty (`penalty='none'`, and the updates lazy regularisation skips).
        table_real, table_fake: the augmentations of the consistency term, int32 [B, 3] (drawn behind the other draws when not given)"""
        set_default_store(self.store)
        b = real.shape[0]
        m = self.model
        kind, point = PENALTIES[self.penalty if penalise else 'none']
        if z is None:
            z = K.rng_normal((b, self.z_dim), self.rng_state)
        if fake_labels is None:
            fake_labels = K.rng_labels(b, 10, self.rng_state)
        if alpha is None and point == 'interpolates':
            alpha = K.rng_uniform(b, self.rng_state)
        if u is None and point == 'perturbed':
            u = K.rng_uniform(real.numel(), self.rng_state)
        if table_real is None and self.consistency != 'none':
            table_real = K.cr_draw(b, self.consistency_shift, self.rng_state)
        if table_fake is None and self.consistency == 'bcr':
            table_fake = K.cr_draw(b, self.consistency_shift, self.rng_state)
        with torch.no_grad():            # d_train_op differentiates w.r.t. d_vars only (train.py:148)
            x_fake = m.get_generator(z, fake_labels)
        disc_real, ac_real = m.get_discriminator(real, real_labels, update_collection=None)
        disc_fake, _ = m.get_discriminator(x_fake, fake_labels, update_collection='NO_OPS', reuse=True)
        d_gan = Fn.hinge_d_loss(Fn.concat_rows(disc_real, disc_fake), b)
        cons = self._consistency_terms(real, real_labels, disc_real, table_real, x_fake, fake_labels, disc_fake, table_fake)
        if kind is None:
            d_ac = Fn.softmax_xent(ac_real, real_labels)
            self.losses.update(d_loss_gan=d_gan.detach(), d_loss_acgan=d_ac.detach(), gradient_penalty=Fn.constant_like(d_gan.detach(), 0.0))
            return Fn.weighted_sum([d_gan, d_ac] + cons)
        # the penalised point: a third pass over the critic, differentiated twice
        if point == 'interpolates':
            x_pen, pen_labels = K.lerp_rows(real, x_fake, alpha), real_labels
        elif point == 'perturbed':
            x_pen, pen_labels = K.dragan_perturb(real, u), real_labels
        elif point == 'real':
            x_pen, pen_labels = real.detach(), real_labels           # (an alias: `real` itself stays without a gradient)
        else:
            x_pen, pen_labels = x_fake.detach(), fake_labels         # detached from the generator (it was run without a graph)
        interp = x_pen.requires_grad_(True)
        d_int, _ = m.get_discriminator(interp, pen_labels, 'NO_OPS', reuse=True)
        ones = Fn.constant_like(d_int, 1.0)                 # tf.gradients(D(x_hat), [x_hat]): d(sum of logits)/d(x_hat); a persistent buffer
        with F2.input_gradient_only():       # the filter / bias / table gradients of this pass are not part of the penalty
            (grads,) = torch.autograd.grad([d_int], [interp], [ones], create_graph=True)
        if self.penalty == 'wgan-gp':
            gp = F2.gradient_penalty(grads, self.penalty_weight * self.penalty_every)      # the reference's term, on its own kernel
        else:
            gp = F2.gradient_penalty(grads, self.penalty_weight * self.penalty_every, kind, 1.0)
        d_ac = Fn.softmax_xent(ac_real, real_labels)
        self.losses.update(d_loss_gan=K.weighted_sum_f32([d_gan.detach(), gp.detach()], [1.0, 1.0]), d_loss_acgan=d_ac.detach(), gradient_penalty=gp.detach())
        return Fn.weighted_sum([d_gan, gp, d_ac] + cons)

    def _consistency_terms(self, real, real_labels, disc_real, table_real, x_fake, fake_labels, disc_fake, table_fake):
        """-> [] ('none': nothing is launched or reported) or [the term]: one more critic pass over the augmented real batch, for 'bcr'
        another over the augmented fakes; each a call of its own, so the critic's batch norm sees that batch by itself, and 'NO_OPS'
        with reuse, so the spectral norm's u is not advanced again"""
        if self.consistency == 'none':
            return []
        w_real, w_fake = self.consistency_weights
        m = self.model
        aug_real, _ = m.get_discriminator(K.cr_augment(real, table_real, self.consistency_shift), real_labels, 'NO_OPS', reuse=True)
        c_real = F2.consistency_loss(disc_real, aug_real, w_real)
        self.consistency_tables = dict(real=table_real) if self.consistency == 'cr' else dict(real=table_real, fake=table_fake)
        if self.consistency == 'cr':
            self.losses.update(consistency=c_real.detach(), consistency_real=c_real.detach(), consistency_fake=Fn.constant_like(c_real.detach(), 0.0))
            return [c_real]
        aug_fake, _ = m.get_discriminator(K.cr_augment(x_fake, table_fake, self.consistency_shift), fake_labels, 'NO_OPS', reuse=True)
        c_fake = F2.consistency_loss(disc_fake, aug_fake, w_fake)
        cons = Fn.weighted_sum([c_real, c_fake])
        self.losses.update(consistency=cons.detach(), consistency_real=c_real.detach(), consistency_fake=c_fake.detach())
        return [cons]

    def g_loss(self, z=None, fake_labels=None):
        set_default_store(self.store)
        b = self.batch
        m = self.model
        if z is None:
            z = K.rng_normal((b, self.z_dim), self.rng_state)
        if fake_labels is None:
            fake_labels = K.rng_labels(b, 10, self.rng_state)
        x_fake = m.get_generator(z, fake_labels)
        with self.critic_frozen():       # g_train_op differentiates w.r.t. g_vars only (train.py:146)
            disc_fake, ac_fake = m.get_discriminator(x_fake, fake_labels, update_collection='NO_OPS', reuse=True)
            g_gan = Fn.hinge_g_loss(disc_fake)
            g_ac = Fn.softmax_xent(ac_fake, fake_labels)
            total = Fn.weighted_sum([g_gan, g_ac], [1.0, self.scale_g])
        self.losses.update(g_loss_gan=g_gan.detach(), g_loss_acgan=g_ac.detach())
        return total

    # ---- updates --------------------------------------------------------------------------------------------------
    def _d_fwd_bwd(self, penalise=True):
        with F2.one_update():            # every pass over the critic in this update shares one preparation of its weights
            if BATCHED_PREP:
                F2.prepare_batched(self.d_params)
            real = K.preprocess_real(self.real_u8, self.rng_state)         # [B, 32, 32, 3] bf16   (train.py:80-83)
            K.zero_(self.d_flat['grads'])
            loss = self.d_loss(real, self.real_labels, penalise=penalise)
            loss.backward(gradient=Fn.unit_seed(loss))
            self.losses['d_loss'] = loss.detach()
        # (runs on the eager and on the capturing call of a form, not on a replay: d_step puts these back after every update)
        self._d_losses[self._d_key(penalise)] = {k: self.losses[k] for k in ('d_loss', 'd_loss_gan', 'd_loss_acgan', 'gradient_penalty') + (
            _Losses.ABSENT if self.consistency != 'none' else ())}
        self._d_tables[self._d_key(penalise)] = self.consistency_tables

    def _d_key(self, penalise):
        """the captured form of a critic update: 'd' / 'd_plain' as ever, with the consistency term in it 'd_cr' / 'd_plain_cr' (or _bcr)"""
        return ('d' if penalise else 'd_plain') + ('' if self.consistency == 'none' else '_' + self.consistency)

    def _d_fwd_bwd_plain(self):
        self._d_fwd_bwd(penalise=False)

    def _g_fwd_bwd(self):
        with F2.one_update():
            if BATCHED_PREP:
                F2.prepare_batched(self.d_params)
            self.store.zero_grads('g_net')
            loss = self.g_loss()
            loss.backward(gradient=Fn.unit_seed(loss))
            self.losses['g_loss'] = loss.detach()

    def d_step(self, real_u8, labels):
        """one critic update on a uint8 [B, 3072] CHW-planar batch + int labels (train.py:199-204).  Two forms, each a captured graph
        of its own: 'd' carries the penalty, 'd_plain' does not (penalty='none'; under lazy regularisation every update whose count
        is no multiple of penalty_every).  The count lives on the host and picks the form outside any capture.  The consistency term is
        part of both forms (their keys then end in '_cr' / '_bcr')."""
        self.real_u8.copy_(real_u8, non_blocking=True)
        self.real_labels.copy_(labels, non_blocking=True)
        penalise = self.penalty != 'none' and self.d_updates % self.penalty_every == 0
        key = self._d_key(penalise)
        self._update(key, self._d_fwd_bwd if penalise else self._d_fwd_bwd_plain, self.d_opt)
        self.d_updates += 1
        self.losses.update(self._d_losses[key])          # a replay wrote the tensors of ITS form, whichever form ran last in Python
        self.consistency_tables = self._d_tables[key]
        return self.losses['d_loss']

    def state_dict(self):
        """the variables by name (`store.state_dict()`) and `_d_updates`, the count of critic updates that schedules the lazy penalty;
        the constructor's `state` takes it back.  Not a full checkpoint: `global_step` (the learning-rate decay), the Adam moments and
        step counts and the RNG state are not in it, so a trainer rebuilt from it keeps its weights and the penalty schedule and starts
        those afresh."""
        sd = self.store.state_dict()
        sd['_d_updates'] = np.asarray(self.d_updates, dtype=np.int64)
        return sd

    def g_step(self):
        self._update('g', self._g_fwd_bwd, self.g_opt)
        self.global_step += 1            # minimize(..., global_step=global_step) on the generator's optimiser (train.py:146)
        return self.losses['g_loss']

    def train_iteration(self, batches, step=None):
        step = self.global_step_counter if step is None else step
        if step > 0:
            self.g_step()
        for _ in range(self.n_dis):
            data, labels = next(batches)
            self.d_step(data, labels)
        self.global_step_counter = step + 1

    global_step_counter = 0

    # ---- evaluation: the metrics of trainer.SampleMetrics over this hook --------------------------------------------
    def _metric_rows(self):
        return self.batch                # the draws of g_loss; the Inception score draws 100 (train.py:159-171)

    def _metric_batch(self, b):
        """b samples on fresh normal noise, then fresh uniform labels (the order of g_loss), quantised as get_inception_score
        quantises them (train.py:159-171) -> (uint8 [b, 32, 32, 3], labels [b])"""
        from ..common.msssim import quantize_on_device
        set_default_store(self.store)
        z = K.rng_normal((b, self.z_dim), self.rng_state)
        labels = K.rng_labels(b, 10, self.rng_state)
        return quantize_on_device(self.model.get_generator(z, labels)).reshape(-1, 32, 32, 3), labels
