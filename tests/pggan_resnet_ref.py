"""torch-CPU float64 restatement of the PGGAN ResNet graph (the reference's default `--model resnet`) and its train-step
losses, with autograd.

TEST INFRASTRUCTURE ONLY: a literal restatement of common/resnet_block.py:100-156 (ResidualBlock), :188-349 (get_dim,
Generator_PGGAN, Discriminator_PGGAN) and PGGAN/train.py:101-111 (the two losses) of the reference -- not a port of the
product code, and nothing under gan_lib_tensorflow_amd/ imports it.  Parameters live in a dict keyed by the TF variable
names the reference's scopes produce (`g_net/...`, `d_net/...`); the operators shared with the other restatements (SAME
convolution, spectral norm with the full gradient, train-mode batch norm, NN upsampling, 2x2 mean pool, the initialisers,
the bf16-storage hook `_st`) come from oracle/ref_torch.py.

Normalize (:32-50) on this path: `labels` is None everywhere, so every `G.` layer is tf.contrib.layers.batch_norm in training
mode (batch statistics; the moving statistics are state no output depends on) and every `D.` layer, called with
spectral_normed=True, is the identity.  The nonlinearity behind an identity Normalize still runs: the critic's fromRGB blocks
feed relu(image) to their first convolution and the raw image to their 1x1 shortcut.
"""
import numpy as np
import torch

from oracle import ref_torch as T


def get_dim(stage):
    """:188-189 (a float under Python 3; the channel counts are its integer values)"""
    return int(min(2048 / (2 ** stage), 512))


def resize_nearest(x, out_hw):
    """tf.image.resize_nearest_neighbor(x, size) of TF 1.5 (align_corners=False): source index = min(floor(dst * scale), in - 1)
    with scale = in / out computed in float32, as the TF kernel does.  x [N,H,W,C] torch tensor; differentiable (index_select)."""
    hi, wi = x.shape[1], x.shape[2]
    ho, wo = out_hw

    def src(n_in, n_out):
        scale = np.float32(n_in) / np.float32(n_out)
        idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
        return torch.as_tensor(np.minimum(idx, n_in - 1))
    return x.index_select(1, src(hi, ho)).index_select(2, src(wi, wo))


# ------------------------------------------------------------------ parameters
def _blocks(bc, trans):
    """[(scope, block name, cin, cout, resample)] in creation order (:223-252, :283-336)"""
    g, d = [], []
    c = 1024
    for i in range(bc - 1):
        g.append((f'G.UpBlock.{i + 1}', c, get_dim(i), 'up'))
        c = get_dim(i)
    top = get_dim(bc - 1)
    if trans:
        g.append((f'G.UpBlock.{bc}', c, top, 'up'))
        g.append((f'G.{bc}_toRGB1', top, top, None))
        g.append((f'G.{bc}_toRGB2', c, top, None))
    else:
        if bc > 0:
            g.append((f'G.UpBlock.{bc}', c, top, 'up'))
            c = top
        g.append((f'G.{bc}_toRGB', c, top, None))
    if trans:
        d.append((f'D.{bc}_fromRGB1', 3, top, None))
        d.append((f'D.DownBlock.{bc}', top, top, 'down'))
        d.append((f'D.{bc}_fromRGB2', 3, top, None))
    else:
        d.append((f'D.{bc}_fromRGB', 3, top, None))
        if bc > 0:
            d.append((f'D.DownBlock.{bc}', top, top, 'down'))
    c = top
    for i in range(1, bc):
        d.append((f'D.DownBlock.{bc - i}', c, get_dim(bc - 1 - i), 'down'))
        c = get_dim(bc - 1 - i)
    d.append(('D.NoneBlock', c, get_dim(0), None))
    return g, d


def init_params(seed, bc, trans, z_dim=512):
    """Variables of Generator_PGGAN / Discriminator_PGGAN for block_count bc, by name, with the initialisers of conv2d.py:83-140 /
    linear.py:76-80 / sn.py:32 and the batch-norm variables of tf.contrib.layers.batch_norm(zero_debias_moving_mean=True)."""
    if trans and bc == 0:
        raise ValueError('trans needs block_count >= 1')
    rng = np.random.default_rng(seed)
    P = {}

    def conv(scope, name, k, cin, cout, he_init=True, sn=False):
        P[f'{scope}/{name}/Filters'] = T.conv_init(rng, k, cin, cout, he_init)
        if sn:
            P[f'{scope}/{name}/filters/spectral_norm/u'] = T.trunc_normal(rng, (1, cout))
        P[f'{scope}/{name}/Biases'] = np.zeros(cout, 'float32')

    def bn(scope, name, c):
        P[f'{scope}/{name}/BatchNorm/beta'] = np.zeros((1, c), 'float32')
        P[f'{scope}/{name}/BatchNorm/gamma'] = np.ones((1, c), 'float32')
        P[f'{scope}/{name}/BatchNorm/moving_mean'] = np.zeros(c, 'float32')
        P[f'{scope}/{name}/BatchNorm/moving_variance'] = np.ones(c, 'float32')
        P[f'{scope}/{name}/BatchNorm/moving_mean/biased'] = np.zeros(c, 'float32')
        P[f'{scope}/{name}/BatchNorm/moving_mean/local_step'] = np.zeros(1, 'float32')

    def block(scope, name, cin, cout, resample, sn, norm):
        if not (cin == cout and resample is None):
            conv(scope, name + '.Shortcut', 1, cin, cout, he_init=False, sn=sn)
        mid = cin if resample == 'down' else cout
        if norm:
            bn(scope, name + '.N1', cin)
        conv(scope, name + '.Conv1', 3, cin, mid, sn=sn)
        if norm:
            bn(scope, name + '.N2', mid)
        conv(scope, name + '.Conv2', 3, mid, cout, sn=sn)

    g, d = _blocks(bc, trans)
    P['g_net/G.Input/W'] = T.linear_init(rng, z_dim, 4 * 4 * 1024)
    P['g_net/G.Input/b'] = np.zeros(4 * 4 * 1024, 'float32')
    bn('g_net', 'G.N0', 1024)
    conv('g_net', 'G.Conv', 3, 1024, 1024)
    for name, cin, cout, resample in g:
        block('g_net', name, cin, cout, resample, False, True)
    bn('g_net', 'G.Output_Normalize', get_dim(bc - 1))
    conv('g_net', 'G.Output', 3, get_dim(bc - 1), 3, he_init=False)
    for name, cin, cout, resample in d:
        block('d_net', name, cin, cout, resample, True, False)
    P['d_net/D.Output/W'] = T.linear_init(rng, get_dim(0), 1)
    P['d_net/D.Output/spectral_norm/u'] = T.trunc_normal(rng, (1, 1))
    P['d_net/D.Output/b'] = np.zeros(1, 'float32')
    return P


# ------------------------------------------------------------------ model
class _Ctx(T._Ctx):
    """SN `u` write policy of the train step: update_u=True hands back u_final (update_collection=None); False leaves u"""

    def conv(self, x, name, sn=False):
        W = self.P[f'{self.scope}/{name}/Filters']
        if sn:
            key = f'{self.scope}/{name}/filters/spectral_norm/u'
            W, u_new, _ = T.spectral_normed_weight(W, self.P[key])
            if self.update_u:
                self.new_u[key] = u_new.detach()
        return T.conv2d_same(x, W, self.P[f'{self.scope}/{name}/Biases'])

    def linear(self, x, name, sn=False):
        W = self.P[f'{self.scope}/{name}/W']
        if sn:
            key = f'{self.scope}/{name}/spectral_norm/u'
            W, u_new, _ = T.spectral_normed_weight(W, self.P[key])
            if self.update_u:
                self.new_u[key] = u_new.detach()
        return x @ W + self.P[f'{self.scope}/{name}/b']

    def norm(self, x, name, sn):
        """Normalize (:32-50) with labels=None"""
        if 'D.' in name:
            assert sn, 'every critic block of the PGGAN path is spectrally normalised'
            return x
        return T.batch_norm_train(x, self.P[f'{self.scope}/{name}/BatchNorm/gamma'], self.P[f'{self.scope}/{name}/BatchNorm/beta'])


def residual_block(c, x, cin, cout, name, sn=False, resample=None):
    """:100-156"""
    if resample == 'down':
        def conv_1(h): return c.conv(h, name + '.Conv1', sn)                              # cin -> cin
        def conv_2(h): return T.meanpool2x2(c.conv(h, name + '.Conv2', sn))               # ConvMeanPool (:53-64)
        def conv_shortcut(h): return T.meanpool2x2(c.conv(h, name + '.Shortcut', sn))
    elif resample == 'up':
        def conv_1(h): return c.conv(T.upsample_nn2x(h), name + '.Conv1', sn)             # UpsampleConv (:83-97)
        def conv_shortcut(h): return c.conv(T.upsample_nn2x(h), name + '.Shortcut', sn)
        def conv_2(h): return c.conv(h, name + '.Conv2', sn)
    elif resample is None:
        def conv_shortcut(h): return c.conv(h, name + '.Shortcut', sn)
        def conv_1(h): return c.conv(h, name + '.Conv1', sn)
        def conv_2(h): return c.conv(h, name + '.Conv2', sn)
    else:
        raise Exception('invalid resample value')
    shortcut = x if (cout == cin and resample is None) else T._st(conv_shortcut(x))
    h = T._st(torch.relu(c.norm(x, name + '.N1', sn)))
    h = T._st(conv_1(h))
    h = T._st(torch.relu(c.norm(h, name + '.N2', sn)))
    return T._st(shortcut + conv_2(h))


def generator(P, z, alpha, bc, trans):
    """:192-263 -> [N, 4 * 2**bc, 4 * 2**bc, 3]"""
    c = _Ctx(P, 'g_net', False)
    out = T._st(c.linear(z.reshape(z.shape[0], -1), 'G.Input')).reshape(-1, 4, 4, 1024)
    out = T._st(torch.relu(c.norm(out, 'G.N0', True)))
    out = T._st(c.conv(out, 'G.Conv'))
    for i in range(bc - 1):
        out = residual_block(c, out, out.shape[-1], get_dim(i), f'G.UpBlock.{i + 1}', resample='up')
    if trans:
        rgb1 = residual_block(c, out, out.shape[-1], get_dim(bc - 1), f'G.UpBlock.{bc}', resample='up')
        rgb1 = residual_block(c, rgb1, rgb1.shape[-1], get_dim(bc - 1), f'G.{bc}_toRGB1')
        rgb2 = T._st(resize_nearest(out, (rgb1.shape[1], rgb1.shape[2])))
        rgb2 = residual_block(c, rgb2, rgb2.shape[-1], get_dim(bc - 1), f'G.{bc}_toRGB2')
        rgb = T._st((1.0 - alpha) * rgb2 + alpha * rgb1)
    else:
        rgb = residual_block(c, out, out.shape[-1], get_dim(bc - 1), f'G.UpBlock.{bc}', resample='up') if bc > 0 else out
        rgb = residual_block(c, rgb, rgb.shape[-1], get_dim(bc - 1), f'G.{bc}_toRGB')
    out = T._st(torch.relu(c.norm(rgb, 'G.Output_Normalize', True)))
    return T._st(torch.tanh(c.conv(out, 'G.Output')))


def discriminator(P, x, alpha, bc, trans, update_u=False):
    """:266-349 -> (logits [N], {u name: u_final} when update_u)"""
    c = _Ctx(P, 'd_net', update_u)
    top = get_dim(bc - 1)
    if trans:
        f1 = residual_block(c, x, 3, top, f'D.{bc}_fromRGB1', sn=True)
        f1 = residual_block(c, f1, top, top, f'D.DownBlock.{bc}', sn=True, resample='down')
        f2 = T._st(resize_nearest(x, (f1.shape[1], f1.shape[2])))
        f2 = residual_block(c, f2, 3, top, f'D.{bc}_fromRGB2', sn=True)
        h = T._st((1.0 - alpha) * f2 + alpha * f1)
    else:
        h = residual_block(c, x, 3, top, f'D.{bc}_fromRGB', sn=True)
        if bc > 0:
            h = residual_block(c, h, top, top, f'D.DownBlock.{bc}', sn=True, resample='down')
    for i in range(1, bc):
        h = residual_block(c, h, h.shape[-1], get_dim(bc - 1 - i), f'D.DownBlock.{bc - i}', sn=True, resample='down')
    h = residual_block(c, h, h.shape[-1], get_dim(0), 'D.NoneBlock', sn=True)
    h = T._st(torch.relu(h))
    h = T._st(h.mean(dim=(1, 2)))
    return T._st(c.linear(h, 'D.Output', sn=True)).reshape(-1), c.new_u


def d_loss(P, real, z, alpha, bc, trans):
    """PGGAN/train.py:101-110: D(real) with update_collection=None (u advances), then D(G(z)) with NO_OPS reading the new u.
    Returns (loss, new_u)."""
    with torch.no_grad():
        x_fake = generator(P, z, alpha, bc, trans)
    disc_real, new_u = discriminator(P, real, alpha, bc, trans, update_u=True)
    P2 = dict(P)
    P2.update(new_u)
    disc_fake, _ = discriminator(P2, x_fake, alpha, bc, trans)
    return torch.relu(1. - disc_real).mean() + torch.relu(1. + disc_fake).mean(), new_u


def g_loss(P, z, alpha, bc, trans):
    """train.py:111"""
    disc_fake, _ = discriminator(P, generator(P, z, alpha, bc, trans), alpha, bc, trans)
    return -disc_fake.mean()
