"""Pix2Pix train step -- create_model and the loop body of Pix2Pix/train.py:447-568,700-730 of the reference (config 5).

    outputs       = G(inputs)                                             U-Net, SAME padding, dropout in the decoder
    discrim_loss  = mean(relu(1 - D(inputs, targets))) + mean(relu(1 + D(inputs, outputs)))     (misc.get_loss 'HINGE')
    gen_loss      = gan_weight * (-mean(D(inputs, outputs))) + l1_weight * mean(|targets - outputs|)
both critic passes run with update_collection=None (the spectral-norm `u` advances in each, train.py:458-475); one step =
n_dis critic updates then one generator update (:704-730); tf.train.AdamOptimizer(beta1=0, beta2=0.9) at a learning rate
decaying linearly from initial_lr to end_lr over max_steps generator steps (polynomial_decay on global_step, :521-541).
`args`: any object with the reference's flag names (batch_size, ngf, ndf, l1_weight, gan_weight, initial_lr, end_lr,
max_steps, n_dis, conv_type, upsampe_method).

The input pipeline of the same script (train.py:95-444, 601-660) is here too, under the reference's names: load_data reads a
folder of side-by-side frames; load_examples turns a batch of raw uint8 frames into (inputs, targets) in ONE launch of
gank_pix2pix_load_examples (csrc/pix_input.hip) -- split, preprocess or Lab, flip, AREA resize, crop; convert / save_images /
append_index turn tensors back into 8-bit PNGs and an index.html.  There is no CPU path: NumPy arrays are uploaded.
"""
import collections
import io
import math
import pathlib
import types

import numpy as np
import torch

from .. import functional as Fn
from .. import kernels as K
from ..store import set_default_store
from ..trainer import GraphTrainer, polynomial_decay  # noqa: F401  (polynomial_decay: part of this module's surface)
from .model import Pix2Pix


def default_args(**over):
    """the argparse defaults of train.py:29-80"""
    a = dict(batch_size=64, ngf=64, ndf=64, l1_weight=100.0, gan_weight=1.0, initial_lr=0.0002, end_lr=0.0001, beta1=0., beta2=0.9,
             max_steps=100000, n_dis=5, conv_type='conv2d', channel_multiplier=0, net_type='UNet', upsampe_method='depth_to_space',
             loss_type='HINGE', crop_size=256, scale_size=None, flip=True, which_direction='AtoB', lab_colorization=False, multiple_A=False,
             aspect_ratio=1.0)
    a.update(over)
    if a['scale_size'] is None:      # the reference's own default (286, under its crop_size of 512) raises at train.py:421-422
        a['scale_size'] = a['crop_size']
    return types.SimpleNamespace(**a)


Examples = collections.namedtuple("Examples", "paths, inputs, targets, count, steps_per_epoch")     # train.py:88


# ---- the input pipeline (train.py:95-444) ----------------------------------------------------------------------------------
def load_data(data_dir=None):
    """train.py:95-132: every *.jpg of data_dir (else every *.png), sorted by number when every stem is a number, read with PIL
    as RGB -> (uint8 [M,H,W,3], paths).  Frames of different sizes raise (the reference's np.asarray would give an object array
    that its [768, 4080, 3] placeholder then refuses)."""
    from PIL import Image
    folder = None if data_dir is None else pathlib.Path(data_dir)
    if folder is None or not folder.is_dir():
        raise Exception(f"load_data: the input directory {data_dir!r} does not exist")
    frames = next((found for found in (list(folder.glob("*" + ext)) for ext in (".jpg", ".png")) if found), None)
    if frames is None:
        raise Exception(f"load_data: {data_dir!r} contains no image files (*.jpg, else *.png)")
    by_number = all(f.stem.isdigit() for f in frames)
    frames.sort(key=(lambda f: int(f.stem)) if by_number else str)
    images = []
    for f in frames:
        with Image.open(f) as im:
            images.append(np.asarray(im.convert("RGB"), dtype=np.uint8))
        if images[-1].shape != images[0].shape:
            raise Exception(f"load_data: images differ in size: {f} is {images[-1].shape}, {frames[0]} is {images[0].shape}")
    return np.stack(images), np.asarray([str(f) for f in frames])


def _gpu(x, dtype=None):
    """a device tensor; NumPy arrays are uploaded (float64 as float32), as common/msssim.py does"""
    if isinstance(x, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("gank: the Pix2Pix input pipeline runs on the GPU (no CPU path exists)")
        x = torch.from_numpy(np.ascontiguousarray(x.astype(np.float32) if x.dtype == np.float64 else x)).cuda()
    if not x.is_cuda:
        raise RuntimeError("gank: the Pix2Pix input pipeline runs on the GPU (no CPU path exists)")
    return (x if dtype is None else x.to(dtype)).contiguous()


def preprocess(image):
    """[0, 1] => [-1, 1] (train.py:135-138)"""
    return _gpu(image) * 2 - 1


def deprocess(image):
    """[-1, 1] => [0, 1] (train.py:141-144)"""
    return (_gpu(image) + 1) / 2


def preprocess_lab(lab):
    """train.py:147-153: lab [..., 3] -> [L / 50 - 1, a / 110, b / 110]"""
    L_chan, a_chan, b_chan = torch.unbind(_gpu(lab), dim=-1)
    return [L_chan / 50 - 1, a_chan / 110, b_chan / 110]


def deprocess_lab(L_chan, a_chan, b_chan):
    """train.py:156-159"""
    return torch.stack([(_gpu(L_chan) + 1) / 2 * 100, _gpu(a_chan) * 110, _gpu(b_chan) * 110], dim=-1)


def rgb_to_lab(srgb):
    """train.py:178-218 (gank_rgb_to_lab): sRGB in [0, 1], [..., 3] -> CIE Lab, fp32"""
    return K.rgb_to_lab(_gpu(srgb, torch.float32))


def lab_to_rgb(lab):
    """train.py:221-262 (gank_lab_to_rgb)"""
    return K.lab_to_rgb(_gpu(lab, torch.float32))


def augment(image, brightness):
    """train.py:265-271: (a, b) colour channels [N,H,W,2] + brightness [N,H,W,1], both in [-1, 1] -> RGB in [0, 1]"""
    image, brightness = _gpu(image, torch.float32), _gpu(brightness, torch.float32)
    a_chan, b_chan = torch.unbind(image, dim=3)
    return lab_to_rgb(deprocess_lab(brightness.squeeze(3), a_chan, b_chan))


def pix_mode(args):
    return 2 if getattr(args, "lab_colorization", False) else (1 if getattr(args, "multiple_A", False) else 0)


def draw_transform(n, args, rng=None, training=True):
    """The randoms of `transform` (train.py:405-420) for n images: int32 [n, 3] rows (flip, offset_y, offset_x), ONE row per
    image, used for its input and its target alike.  Per image: one flip bit if args.flip, then (offset_y, offset_x) uniform in
    [0, scale_size - crop_size].  training=False is the validation setting of :756-757 (scale_size = crop_size, no flip): all
    zeros.  -> (table, scale_size)"""
    scale = args.scale_size if training else args.crop_size
    if scale < args.crop_size:
        raise Exception("scale size cannot be less than crop size")
    rng = np.random if rng is None else rng
    table = np.zeros((n, 3), np.int32)
    for i in range(n):
        if training and args.flip:
            table[i, 0] = rng.randint(0, 2)
        if scale > args.crop_size:
            table[i, 1:] = rng.randint(0, scale - args.crop_size + 1, size=2)
    return table, scale


def load_examples(raw_input, input_paths, args, rng=None, training=True, out=None, dtype=None):
    """train.py:326-444 for a batch: raw_input uint8 [N,H,W,3] (NumPy or device tensor; one [H,W,3] frame is a batch of one)
    -> Examples(paths, inputs [N,crop,crop,Ca], targets [N,crop,crop,Cb], count, steps_per_epoch), one kernel launch.
    args: scale_size, crop_size, flip, which_direction, lab_colorization, multiple_A (and batch_size for steps_per_epoch).
    rng: a numpy.random.RandomState (default: NumPy's global one) -- see draw_transform.  The reference seeds two TensorFlow
    ops with one Python integer; TensorFlow's op-seeded stream cannot be reproduced here, so the draws have the reference's
    distribution and sharing between input and target, not its values.
    out=(inputs, targets) writes in place (their dtype); otherwise `dtype` (default: the 16-bit activation type).
    count and steps_per_epoch come from the data (the reference hard-codes 118, :436-442)."""
    raw = _gpu(raw_input)
    if raw.dim() == 3:
        raw = raw.unsqueeze(0)
    if raw.dim() != 4 or raw.shape[3] != 3 or raw.dtype != torch.uint8:
        raise Exception(f"image does not have 3 channels (uint8 [N,H,W,3] expected, got {raw.dtype} {tuple(raw.shape)})")
    if args.which_direction not in ("AtoB", "BtoA"):
        raise Exception("invalid direction")
    n = raw.shape[0]
    table, scale = draw_transform(n, args, rng, training)
    inputs, targets = out if out is not None else (None, None)
    inputs, targets = K.pix2pix_load_examples(raw, table, pix_mode(args), 0 if args.which_direction == "AtoB" else 1,
                                              scale, scale, args.crop_size, inputs, targets, dtype)
    return Examples(paths=input_paths, inputs=inputs, targets=targets, count=n,
                    steps_per_epoch=int(math.ceil(n / float(getattr(args, "batch_size", n) or n))))


# ---- back to viewable images (train.py:274-323, 601-660) ----------------------------------------------------------------------
def _check_aspect(args):
    if args is not None and getattr(args, "aspect_ratio", 1.0) != 1.0:
        raise NotImplementedError("aspect_ratio != 1 (the bicubic upscale of train.py:628-631) is not implemented")


def convert(image, args=None):
    """train.py:627-633: a deprocessed image in [0, 1] -> uint8, tf.image.convert_image_dtype(saturate=True): scaled by 255.5,
    saturated, truncated."""
    _check_aspect(args)
    image = _gpu(image)
    return K.pix2pix_convert_u8(image if image.dtype in (K.BF16, torch.float32) else image.float(), deprocess=False)


def encode_png(image):
    """PNG bytes of a uint8 [H,W,1] or [H,W,3] image (tf.image.encode_png, :657-659), through PIL"""
    from PIL import Image
    a = image.cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (1, 3):
        raise RuntimeError(f"gank: encode_png takes uint8 [H,W,1] or [H,W,3], got {a.dtype} {a.shape}")
    buf = io.BytesIO()
    Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(buf, format="PNG")
    return buf.getvalue()


def display_images(inputs, outputs, targets, args):
    """train.py:601-652: the three uint8 [N,H,W,1|3] tensors written to disk, each ONE launch of gank_pix2pix_convert_u8 --
    deprocess + convert; with lab_colorization the colour side goes through augment (deprocess_lab, lab_to_rgb) in the same
    launch; with multiple_A the inputs show their second panel (tf.split(...)[1])."""
    _check_aspect(args)
    if getattr(args, "lab_colorization", False):
        if args.which_direction == "AtoB":
            return K.pix2pix_convert_u8(inputs), K.pix2pix_convert_u8(outputs, brightness=inputs), K.pix2pix_convert_u8(targets, brightness=inputs)
        return K.pix2pix_convert_u8(inputs, brightness=targets), K.pix2pix_convert_u8(outputs), K.pix2pix_convert_u8(targets)
    c = inputs.shape[-1]
    shown = K.pix2pix_convert_u8(inputs, c0=c // 2, cw=c // 2) if getattr(args, "multiple_A", False) else K.pix2pix_convert_u8(inputs)
    return shown, K.pix2pix_convert_u8(outputs), K.pix2pix_convert_u8(targets)


KINDS = ("inputs", "outputs", "targets")


def save_images(fetches, output_dir, step=None):
    """train.py:274-298: fetches = {"paths": path or paths, "inputs" / "outputs" / "targets": PNG bytes per path} ->
    <output_dir>/images/[<step, 8 digits>-]<stem>-<kind>.png; returns the filesets for append_index."""
    images = pathlib.Path(output_dir, "images")
    images.mkdir(parents=True, exist_ok=True)
    prefix = "" if step is None else f"{step:08d}-"
    filesets = []
    for i, source in enumerate(np.atleast_1d(np.asarray(fetches["paths"])).tolist()):
        stem = pathlib.PurePath(str(source)).stem
        files = {kind: f"{prefix}{stem}-{kind}.png" for kind in KINDS}
        for kind, filename in files.items():
            (images / filename).write_bytes(fetches[kind][i])
        filesets.append(dict(files, name=stem, step=step))
    return filesets


def _index_row(cells, tag="td"):
    return "<tr>" + "".join(f"<{tag}>{cell}</{tag}>" for cell in cells) + "</tr>"


def append_index(filesets, output_dir, step=False):
    """train.py:301-323: one table row per fileset appended to <output_dir>/index.html (the header when the file is new)"""
    index = pathlib.Path(output_dir, "index.html")
    lead = ["step"] if step else []
    text = "" if index.exists() else "<html><body><table>" + _index_row(lead + ["name", "input", "output", "target"], "th")
    for fileset in filesets:
        cells = [format(fileset["step"], "d")] if step else []
        text += _index_row(cells + [fileset["name"]] + [f"<img src='images/{fileset[kind]}'>" for kind in KINDS])
    with index.open("a") as f:
        f.write(text)
    return str(index)


class Pix2PixTrainer(GraphTrainer):
    def __init__(self, args, device="cuda", seed=0, process_group=None, state=None, in_channels=3, out_channels=3, use_graphs=True, allow_eager_fallback=False):
        if args.loss_type != 'HINGE':
            raise NotImplementedError('loss_type HINGE (the reference default, train.py:38)')
        super().__init__(device, seed, process_group, use_graphs, allow_eager_fallback)
        self.args = args
        self.model = Pix2Pix()
        self.out_channels = out_channels
        self.global_step = 0
        with torch.no_grad():            # build once: variables are created by name on first use
            s = args.crop_size
            a = torch.zeros((args.batch_size, s, s, in_channels), dtype=K.BF16, device=self.device)
            out = self._generator(a, reuse=False)
            self._critic(a, out, 'NO_OPS', reuse=False)
        adam = (args.initial_lr, args.beta1, args.beta2)
        self._finish_build(state, g_adam=adam, d_adam=adam)
        # the static inputs of the captured updates
        self.inputs = torch.zeros((args.batch_size, args.crop_size, args.crop_size, in_channels), dtype=K.BF16, device=self.device)
        self.targets = torch.zeros((args.batch_size, args.crop_size, args.crop_size, out_channels), dtype=K.BF16, device=self.device)

    def _generator(self, inputs, reuse=True):
        a = self.args
        return self.model.get_generator(inputs, self.out_channels, ngf=a.ngf, conv_type=a.conv_type, channel_multiplier=a.channel_multiplier,
                                        padding='SAME', net_type=a.net_type, reuse=reuse, upsampe_method=a.upsampe_method, rng_state=self.rng_state)

    def _critic(self, inputs, targets, update_collection, reuse=True):
        a = self.args
        return self.model.get_discriminator(inputs, targets, ndf=a.ndf, spectral_normed=True, update_collection=update_collection,
                                            conv_type=a.conv_type, channel_multiplier=a.channel_multiplier, padding='VALID',
                                            net_type=a.net_type, reuse=reuse)

    def _learning_rate(self):
        a = self.args
        return polynomial_decay(self.global_step, a.initial_lr, a.max_steps, a.end_lr)

    # ---- losses ---------------------------------------------------------------------------------------------------
    def d_loss(self, inputs, targets):
        """discrim_loss (train.py:477-483); the generator is not differentiated (var_list=discrim_tvars, :546)"""
        set_default_store(self.store)
        with torch.no_grad():
            outputs = self._generator(inputs)
        predict_real = self._critic(inputs, targets, None)
        predict_fake = self._critic(inputs, outputs, None)
        n = predict_real.numel()
        return Fn.hinge_d_loss(Fn.concat_rows(predict_real.reshape(-1), predict_fake.reshape(-1)), n)

    def g_loss(self, inputs, targets):
        """gen_loss (train.py:504-512); the critic's variables are not differentiated (var_list=gen_tvars, :552).  The
        generator update's graph contains BOTH critic passes with update_collection=None (:452-475), so `u` advances twice."""
        set_default_store(self.store)
        outputs, outputs_l1 = Fn.fork(self._generator(inputs))     # read by the critic and by the L1 term: one add launch backward
        with self.critic_frozen():
            with torch.no_grad():
                self._critic(inputs, targets, None)            # predict_real: only its u update is observable here
            predict_fake = self._critic(inputs, outputs, None)
            gan = Fn.hinge_g_loss(predict_fake.reshape(-1))
            l1 = Fn.l1_loss(outputs_l1, targets)
        self.losses.update(gen_loss_GAN=gan.detach(), gen_loss_L1=l1.detach())
        return Fn.weighted_sum([gan, l1], [self.args.gan_weight, self.args.l1_weight])

    # ---- updates --------------------------------------------------------------------------------------------------
    def _d_fwd_bwd(self):
        loss = self.d_loss(self.inputs, self.targets)
        self._backward(loss)
        self.losses['discrim_loss'] = loss.detach()

    def _g_fwd_bwd(self):
        loss = self.g_loss(self.inputs, self.targets)
        self._backward(loss)
        self.losses['gen_loss'] = loss.detach()

    def _feed(self, inputs, targets):
        if inputs.data_ptr() != self.inputs.data_ptr():
            self.inputs.copy_(inputs, non_blocking=True)
        if targets.data_ptr() != self.targets.data_ptr():
            self.targets.copy_(targets, non_blocking=True)

    def d_step(self, inputs, targets):
        self._feed(inputs, targets)
        self._update('d', self._d_fwd_bwd, self.d_opt)
        return self.losses['discrim_loss']

    def g_step(self, inputs, targets):
        self._feed(inputs, targets)
        self._update('g', self._g_fwd_bwd, self.g_opt)
        self.global_step += 1            # apply_gradients(..., global_step=global_step) on the generator's optimiser (:554)
        return self.losses['gen_loss']

    def train_step(self, inputs, targets):
        """train.py:704-730: n_dis critic updates, then the generator update, on one batch of pairs"""
        for _ in range(self.args.n_dis):
            self.d_step(inputs, targets)
        return self.g_step(inputs, targets)

    # ---- data (train.py:585-588, 694-699, 753-770) ---------------------------------------------------------------------------
    def load_examples(self, raw_input, rng=None, training=True):
        """raw uint8 [batch_size,H,W,3] -> (self.inputs, self.targets): the kernel writes the static buffers the captured graphs
        read, so train_step(*tr.load_examples(raw)) copies nothing in _feed."""
        ex = load_examples(raw_input, None, self.args, rng=rng, training=training, out=(self.inputs, self.targets))
        return ex.inputs, ex.targets

    def fit_epoch(self, train_data, rng=None):
        """One epoch over train_data (uint8 [M,H,W,3], NumPy or device tensor): one shuffle (train.py:695-699), batches of
        args.batch_size, the ragged tail dropped; yields the losses of every train_step as a dict of device scalars.
        A NumPy train_data is uploaded WHOLE, once: M x H x W x 3 bytes of device memory (the reference's 118 frames of
        768 x 4080 are 1.1 GB).  A folder that does not fit there has to be fed in parts, one fit_epoch call per part, or batch by
        batch through load_examples.  Each step also uploads its 3-integer-per-image table from pageable host memory, a small
        synchronous copy."""
        rng = np.random if rng is None else rng
        data = _gpu(train_data)
        bs = self.args.batch_size
        order = torch.from_numpy(rng.permutation(np.arange(len(data)))).to(data.device)
        for b in range(len(data) // bs):
            self.train_step(*self.load_examples(data[order[b * bs:(b + 1) * bs]], rng=rng))
            yield dict(self.losses)

    @torch.no_grad()
    def evaluate(self, val_data, val_paths, output_dir):
        """train.py:753-769: the generator on every validation frame (scale_size = crop_size, no flip), three PNGs per frame
        under <output_dir>/images and one row each in <output_dir>/index.html; returns the index path.  A last batch shorter
        than batch_size is filled up with its last frame (the buffers are static); only the real frames are written."""
        set_default_store(self.store)
        data, bs = _gpu(val_data), self.args.batch_size
        index_path = None
        for b in range(0, len(data), bs):
            k = min(bs, len(data) - b)
            idx = torch.clamp(torch.arange(b, b + bs, device=data.device), max=len(data) - 1)
            inputs, targets = self.load_examples(data[idx], training=False)
            outputs = self._generator(inputs)
            shown = [t[:k].cpu() for t in display_images(inputs, outputs, targets, self.args)]
            fetches = {"paths": list(val_paths[b:b + k])}
            for kind, t in zip(("inputs", "outputs", "targets"), shown):
                fetches[kind] = [encode_png(im) for im in t]
            index_path = append_index(save_images(fetches, output_dir), output_dir)
        return index_path


@torch.no_grad()
def msssim_score(outputs, targets, weights=None, per_image=False):
    """MS-SSIM (common/msssim.py of the reference) of generator outputs against their targets, both [N,H,W,C] in [-1, 1] as the
    model produces / is fed them (any 16-bit or fp32 dtype, any size up to the 512 x 512 crops): scored as fp32 with max_val = 2
    after the shift to [0, 2].  One float with the reference's batch semantics, or float64 [N] with per_image=True."""
    from ..common.msssim import MultiScaleSSIM
    return MultiScaleSSIM(outputs.float() + 1.0, targets.float() + 1.0, max_val=2.0, weights=weights, per_image=per_image)


@torch.no_grad()
def swd_score(outputs, targets, **kw):
    """Sliced Wasserstein distance on Laplacian-pyramid patches (common/swd.py) of generator outputs against their targets, both
    [N,H,W,C] in [-1, 1] as the model produces / is fed them (any 16-bit or fp32 dtype), scored as float64 ->
    (float64 [levels], their mean), x 1000.  **kw: nhood_size, nhoods_per_image, dir_repeats, dirs_per_repeat, seed."""
    from ..common.swd import calculate_swd
    return calculate_swd(outputs.float(), targets.float(), **kw)


@torch.no_grad()
def ndb_score(outputs, targets, **kw):
    """NDB and JSD (common/ndb.py) of generator outputs against their targets, both [N,H,W,C] in [-1, 1] as the model produces /
    is fed them (any 16-bit or fp32 dtype): both are quantised to uint8 as the sample metrics quantise
    (msssim.quantize_on_device), the bins are fitted on the targets -> dict(ndb, ndb_over_k, js, bin_proportions_train,
    bin_proportions_samples, different_bins).  **kw: number_of_bins, significance_level, max_dims, seed, max_iter."""
    from ..common.msssim import quantize_on_device
    from ..common.ndb import calculate_ndb
    if tuple(outputs.shape) != tuple(targets.shape) or outputs.dim() != 4:
        raise ValueError(f"ndb_score: outputs {tuple(outputs.shape)} and targets {tuple(targets.shape)}, expected two equal [N,H,W,C]")
    return calculate_ndb(quantize_on_device(targets), quantize_on_device(outputs), **kw)
