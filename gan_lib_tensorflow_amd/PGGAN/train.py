"""PGGAN train step -- the loop body of PGGAN/train.py:61-219 of the reference (BASELINE.json config 4).

One step (train.py:185-193) = 1 generator update + n_dis = 5 critic updates at fade-in weight alpha = step / max_iter:
    real images : CIFAR-10 rows -> 2 (x/256 - .5) + U[0, 1/128) -> NHWC -> bilinear resize to image_size (through
                  image_size/2 first while a new block fades in, :88-92)
    critic loss : mean(relu(1 - D(real))) + mean(relu(1 + D(G(z))))       (:104-106)   D(real) updates the spectral-norm u
    gen loss    : -mean(D(G(z)))                                           (:107)       (D(fake) runs with NO_OPS, :102)
both with tf.train.AdamOptimizer(1e-4, beta1=0, beta2=0.9)               (:130-134).
`args` is any object with the reference's flag names (batch_size, image_size, block_count, trans, inputs_norm, z_dim, n_dis,
max_iter, model).  `model` = 'nvidia' (model_nvidia.py) | 'resnet' (model_resnet.py, the reference's default; the generator's
batch-norm moving statistics are non-trainable state and stay out of the optimiser's buffers).  Data parallel: flat gradient buffers, one RCCL all-reduce per update, 1/world inside the Adam kernel.
"""
import types

import torch

from .. import functional as Fn
from .. import kernels as K
from ..store import set_default_store
from ..trainer import GraphTrainer, SampleMetrics


def model_class(name):
    """the `--model` switch of train.py:62-67"""
    if name == 'nvidia':
        from .model_nvidia import PGGAN
    elif name == 'resnet':
        from .model_resnet import PGGAN
    else:
        raise NotImplementedError('Not supported model!')
    return PGGAN


def default_args(**over):
    """the argparse defaults of train.py:24-57"""
    a = dict(batch_size=16, image_size=4, max_iter=100000, n_dis=5, z_dim=512, image_dim=3072, model='nvidia', block_count=0,
             trans=False, inputs_norm=False)
    a.update(over)
    return types.SimpleNamespace(**a)


class PGGANTrainer(SampleMetrics, GraphTrainer):
    def __init__(self, args, device="cuda", seed=0, process_group=None, state=None, use_graphs=True, allow_eager_fallback=False):
        assert args.image_size == 4 * 2 ** args.block_count, "image_size must be 4 * 2**block_count (train.py:52-54)"
        super().__init__(device, seed, process_group, use_graphs, allow_eager_fallback)
        self.args = args
        self.model = model_class(args.model)(args)
        self.step = 0
        with torch.no_grad():            # build once: variables are created by name on first use
            z = torch.zeros((args.batch_size, args.z_dim), dtype=K.BF16, device=self.device)
            x = self.model.get_generator(z, 0.0)
            self.model.get_discriminator(x, 0.0, update_collection='NO_OPS')
        self._finish_build(state, g_adam=(0.0001, 0.0, 0.9), d_adam=(0.0001, 0.0, 0.9))
        # the static inputs of the captured updates: the input rows, the fade-in weight in device memory (written before a replay)
        self.real_u8 = torch.zeros((args.batch_size, args.image_dim), dtype=torch.uint8, device=self.device)
        self.alpha_dev = torch.zeros(1, dtype=torch.float32, device=self.device)

    def alpha(self, step=None):
        return float(self.step if step is None else step) / float(self.args.max_iter)        # feed_dict alpha (:186)

    # ---- inputs ---------------------------------------------------------------------------------------------------
    def real_images(self, real_u8):
        """uint8 [B, 3072] CHW-planar rows -> bf16 [B, image_size, image_size, 3]   (:81-92)"""
        a = self.args
        x = K.preprocess_real(real_u8, self.rng_state)                          # [B, 32, 32, 3]
        if a.trans and a.block_count:
            x = K.resize_bilinear(x, (a.image_size // 2, a.image_size // 2))
        if x.shape[1] != a.image_size:
            x = K.resize_bilinear(x, (a.image_size, a.image_size))
        return x

    # ---- the two losses (explicit inputs override the device RNG for parity tests) -------------------------------
    def d_loss(self, real, z=None, alpha=None):
        set_default_store(self.store)
        b = real.shape[0]
        alpha = self.alpha() if alpha is None else alpha
        if z is None:
            z = K.rng_normal((b, self.args.z_dim), self.rng_state)
        with torch.no_grad():            # d_train_op differentiates w.r.t. d_vars only (:134)
            x_fake = self.model.get_generator(z, alpha, reuse=True)
        disc_real = self.model.get_discriminator(real, alpha, update_collection=None, reuse=True)
        disc_fake = self.model.get_discriminator(x_fake, alpha, update_collection='NO_OPS', reuse=True)
        return Fn.hinge_d_loss(Fn.concat_rows(disc_real, disc_fake), b)

    def g_loss(self, z=None, alpha=None):
        set_default_store(self.store)
        alpha = self.alpha() if alpha is None else alpha
        if z is None:
            z = K.rng_normal((self.args.batch_size, self.args.z_dim), self.rng_state)
        x_fake = self.model.get_generator(z, alpha, reuse=True)
        with self.critic_frozen():       # g_train_op differentiates w.r.t. g_vars only (:132)
            disc_fake = self.model.get_discriminator(x_fake, alpha, update_collection='NO_OPS', reuse=True)
            return Fn.hinge_g_loss(disc_fake)

    # ---- updates --------------------------------------------------------------------------------------------------
    def _d_fwd_bwd(self):
        loss = self.d_loss(self.real_images(self.real_u8), alpha=self.alpha_dev)
        self._backward(loss)
        self.losses['d_loss'] = loss.detach()

    def _g_fwd_bwd(self):
        loss = self.g_loss(alpha=self.alpha_dev)
        self._backward(loss)
        self.losses['g_loss'] = loss.detach()

    def d_step(self, real_u8, alpha=None):
        self.real_u8.copy_(real_u8, non_blocking=True)
        self.alpha_dev.fill_(self.alpha() if alpha is None else float(alpha))
        self._update('d', self._d_fwd_bwd, self.d_opt)
        return self.losses['d_loss']

    def g_step(self, alpha=None):
        self.alpha_dev.fill_(self.alpha() if alpha is None else float(alpha))
        self._update('g', self._g_fwd_bwd, self.g_opt)
        return self.losses['g_loss']

    def train_iteration(self, batches):
        """one pass of the loop at train.py:185-193"""
        a = self.alpha()
        self.g_step(a)
        for _ in range(self.args.n_dis):
            data, _labels = next(batches)
            self.d_step(data, a)
        self.step += 1

    @torch.no_grad()
    def sample(self, n=100, z=None, alpha=None):
        """fixed-noise samples (:138-145)"""
        set_default_store(self.store)
        if z is None:
            z = K.rng_normal((n, self.args.z_dim), self.rng_state)
        return self.model.get_generator(z, self.alpha() if alpha is None else alpha, reuse=True)

    def _metric_batch(self, b, alpha=None):
        """the hook of trainer.SampleMetrics: `sample(b)` on fresh noise at `alpha` (default: the current fade-in weight), at the
        stage's image_size, quantised as get_inception_score quantises (:150-162) -> (uint8 [b, size, size, 3], None: no labels)"""
        from ..common.msssim import quantize_on_device
        size = self.args.image_size
        return quantize_on_device(self.sample(b, alpha=alpha)).reshape(-1, size, size, 3), None

    @torch.no_grad()
    def inception_score(self, n=50000, net=None, splits=10, alpha=None):
        """get_inception_score(n, alpha) of the training script (:150-162, every evaluation_interval steps at the step's fade-in
        weight, :195-198): `SampleMetrics.inception_score` on samples at `alpha` -- the classifier's own bilinear resize takes
        them from the stage's image_size to 299 x 299."""
        from ..common.inception.inception_score import sample_inception_score
        return sample_inception_score(self._metric_draw(100, alpha=alpha), int(n / 100), 100, net, splits)

    @torch.no_grad()
    def swd(self, real, n=8192, alpha=None, seed=0, **kw):
        """The metric of the progressive-GAN paper's tables: `SampleMetrics.swd` on samples at `alpha`, `real` already at the
        stage's size; one value per pyramid level from image_size down to 16.  At image_size 4 it raises: a 7 x 7 patch does
        not fit."""
        from ..common.swd import sample_swd
        return sample_swd(self._metric_draw(alpha=alpha), real, n, seed, **kw)
