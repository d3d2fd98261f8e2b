"""CPU: the PGGAN ResNet model (the reference's default `--model resnet`) without a device -- the float64 restatement
(tests/pggan_resnet_ref.py) against known answers that do not depend on it, the variable names pinned to the reference's scopes
(common/resnet_block.py:188-349), the generator's output shapes, and the argument checks of the two new C entry points (refused
on the host, before any launch)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pggan_resnet_ref as R  # noqa: E402
from oracle import ref_torch as T  # noqa: E402


# ---- tf.image.resize_nearest_neighbor (TF 1.5, align_corners=False) -----------------------------------------------------------
def test_resize_nearest_known_answers():
    x = torch.arange(16, dtype=torch.float64).reshape(1, 4, 4, 1)
    down = R.resize_nearest(x, (2, 2))[0, :, :, 0]
    assert down.tolist() == [[0., 2.], [8., 10.]]                       # the top-left pixel of each 2x2 cell, not its mean
    up = R.resize_nearest(x, (8, 8))[0, :, :, 0]
    assert torch.equal(up, x[0, :, :, 0].repeat_interleave(2, 0).repeat_interleave(2, 1))     # each source pixel as a 2x2 block
    assert torch.equal(R.resize_nearest(x, (8, 8)), T.upsample_nn2x(x))
    line = torch.arange(5, dtype=torch.float64).reshape(1, 5, 1, 1)
    assert R.resize_nearest(line, (3, 1)).flatten().tolist() == [0., 1., 3.]                  # floor(0, 1.67, 3.33)
    assert R.resize_nearest(line.reshape(1, 1, 5, 1), (1, 3)).flatten().tolist() == [0., 1., 3.]


def test_resize_nearest_down_gradient_lands_on_even_even_pixels():
    x = torch.zeros(2, 4, 6, 3, dtype=torch.float64, requires_grad=True)
    g = torch.arange(2 * 2 * 3 * 3, dtype=torch.float64).reshape(2, 2, 3, 3) + 1.
    R.resize_nearest(x, (2, 3)).backward(g)
    assert torch.equal(x.grad[:, ::2, ::2, :], g)
    mask = torch.ones(4, 6, dtype=torch.bool)
    mask[::2, ::2] = False
    assert float(x.grad[:, mask, :].abs().max()) == 0.0


# ---- variable names ---------------------------------------------------------------------------------------------------------------
_BN = ['BatchNorm/beta', 'BatchNorm/gamma', 'BatchNorm/moving_mean', 'BatchNorm/moving_variance', 'BatchNorm/moving_mean/biased',
       'BatchNorm/moving_mean/local_step']


def _g_block(name, shortcut):
    out = []
    for part in ((['Shortcut'] if shortcut else []) + ['Conv1', 'Conv2']):
        out += [f'g_net/{name}.{part}/Filters', f'g_net/{name}.{part}/Biases']
    for part in ('N1', 'N2'):
        out += [f'g_net/{name}.{part}/{v}' for v in _BN]
    return out


def _d_block(name, shortcut):
    out = []
    for part in ((['Shortcut'] if shortcut else []) + ['Conv1', 'Conv2']):
        out += [f'd_net/{name}.{part}/Filters', f'd_net/{name}.{part}/Biases', f'd_net/{name}.{part}/filters/spectral_norm/u']
    return out


def _g_common():
    return (['g_net/G.Input/W', 'g_net/G.Input/b', 'g_net/G.Conv/Filters', 'g_net/G.Conv/Biases', 'g_net/G.Output/Filters',
             'g_net/G.Output/Biases'] + [f'g_net/G.N0/{v}' for v in _BN] + [f'g_net/G.Output_Normalize/{v}' for v in _BN])


_D_OUT = ['d_net/D.Output/W', 'd_net/D.Output/b', 'd_net/D.Output/spectral_norm/u']


def test_variable_names_with_a_block_fading_in():
    """bc = 1, trans: the scopes of common/resnet_block.py:207-257 and :283-345"""
    P = R.init_params(0, 1, True)
    want = (_g_common() + _g_block('G.UpBlock.1', True) + _g_block('G.1_toRGB1', False) + _g_block('G.1_toRGB2', True)
            + _d_block('D.1_fromRGB1', True) + _d_block('D.DownBlock.1', True) + _d_block('D.1_fromRGB2', True)
            + _d_block('D.NoneBlock', False) + _D_OUT)
    assert sorted(P) == sorted(want), set(P) ^ set(want)
    assert P['g_net/G.Input/W'].shape == (512, 4 * 4 * 1024)
    assert P['g_net/G.UpBlock.1.Conv1/Filters'].shape == (3, 3, 1024, 512) and P['g_net/G.UpBlock.1.Shortcut/Filters'].shape == (1, 1, 1024, 512)
    assert P['g_net/G.1_toRGB1.Conv1/Filters'].shape == (3, 3, 512, 512)                      # 512 -> 512: identity shortcut
    assert P['g_net/G.1_toRGB2.Shortcut/Filters'].shape == (1, 1, 1024, 512)                  # 1024 -> 512
    assert P['g_net/G.1_toRGB2.N1/BatchNorm/gamma'].shape == (1, 1024) and P['g_net/G.1_toRGB2.N2/BatchNorm/gamma'].shape == (1, 512)
    assert P['g_net/G.Output/Filters'].shape == (3, 3, 512, 3)
    assert P['d_net/D.1_fromRGB1.Shortcut/Filters'].shape == (1, 1, 3, 512) and P['d_net/D.1_fromRGB1.Conv1/Filters'].shape == (3, 3, 3, 512)
    assert P['d_net/D.DownBlock.1.Conv2/Filters'].shape == (3, 3, 512, 512)
    assert P['d_net/D.Output/W'].shape == (512, 1)


def test_variable_names_at_the_first_stage():
    """bc = 0, no fade-in: G.0_toRGB is a residual block 1024 -> get_dim(-1) = 512 at 4x4; the critic is fromRGB + NoneBlock"""
    P = R.init_params(0, 0, False)
    want = _g_common() + _g_block('G.0_toRGB', True) + _d_block('D.0_fromRGB', True) + _d_block('D.NoneBlock', False) + _D_OUT
    assert sorted(P) == sorted(want), set(P) ^ set(want)
    assert P['g_net/G.0_toRGB.Shortcut/Filters'].shape == (1, 1, 1024, 512)
    with pytest.raises(ValueError):
        R.init_params(0, 0, True)


def test_get_dim():
    assert [R.get_dim(s) for s in range(-1, 7)] == [512, 512, 512, 512, 256, 128, 64, 32]
    from gan_lib_tensorflow_amd.common import resnet_block as blocks
    assert [blocks.get_dim(s) for s in range(-1, 7)] == [512, 512, 512, 512, 256, 128, 64, 32]


@pytest.mark.parametrize("bc,trans", [(0, False), (1, True), (2, False), (3, True)])
def test_generator_output_shape(bc, trans):
    n = 2
    P = T.to_torch(R.init_params(1, bc, trans, z_dim=16), requires_grad=False)
    z = torch.tensor(np.random.default_rng(bc).normal(size=(n, 16)))
    with torch.no_grad():
        img = R.generator(P, z, 0.25, bc, trans)
        logits, new_u = R.discriminator(P, img, 0.25, bc, trans, update_u=True)
    assert img.shape == (n, 4 * 2 ** bc, 4 * 2 ** bc, 3) and float(img.abs().max()) <= 1.0
    assert logits.shape == (n,) and bool(torch.isfinite(logits).all())
    assert sorted(new_u) == sorted(k for k in P if k.endswith('spectral_norm/u'))


# ---- the product's host side ------------------------------------------------------------------------------------------------------
def test_model_switch():
    from gan_lib_tensorflow_amd.PGGAN import model_nvidia, model_resnet
    from gan_lib_tensorflow_amd.PGGAN.train import default_args, model_class
    assert default_args().model == 'nvidia'
    assert model_class('nvidia') is model_nvidia.PGGAN and model_class('resnet') is model_resnet.PGGAN
    with pytest.raises(NotImplementedError, match='Not supported model!'):
        model_class('stylegan')


def test_entry_points_reject_bad_arguments_with_a_message():
    """null pointers and non-positive sizes are refused on the host with a gank_last_error() message, before anything launches"""
    from gan_lib_tensorflow_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below is refused by the argument checks
    for fn, what in ((lib.gank_resize_nearest_fwd, 'resize_nearest_fwd'), (lib.gank_resize_nearest_bwd, 'resize_nearest_bwd')):
        assert fn(None, fake, 1, 4, 4, 2, 2, 3, None) != 0
        assert what in lib.gank_last_error().decode()
        assert fn(fake, None, 1, 4, 4, 2, 2, 3, None) != 0
        assert what in lib.gank_last_error().decode()
        for sizes in ((0, 4, 4, 2, 2, 3), (1, 0, 4, 2, 2, 3), (1, 4, 0, 2, 2, 3), (1, 4, 4, 0, 2, 3), (1, 4, 4, 2, 0, 3), (1, 4, 4, 2, 2, 0),
                      (1, 4, 4, 2, -2, 3)):
            assert fn(fake, fake, *sizes, None) != 0, sizes
            assert what in lib.gank_last_error().decode()
