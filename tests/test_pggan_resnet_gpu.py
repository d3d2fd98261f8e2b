"""PGGAN ResNet model (the reference's default `--model resnet`: PGGAN/model_resnet.py, common/resnet_block.py:188-349) on a real
MI355X against the float64 restatement (tests/pggan_resnet_ref.py): the nearest-neighbour resize kernels, the generator and the
critic at three stages of the progression, both losses with their gradients, the spectral-norm `u` policy of the two critic
passes, training steps on the captured-graph path and the trainer's model switch.  bf16 activations / fp32 accumulate;
tolerances stated at each assertion."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pggan_resnet_ref as R  # noqa: E402
from oracle import ref_torch as T  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gan_lib_tensorflow_amd import kernels
    kernels.lib()
    return torch.device("cuda")


def bf(a):
    t = torch.tensor(np.asarray(a, np.float32)).to(torch.bfloat16)
    return t.to(torch.float64), t.cuda().contiguous()


def rel(got, ref):
    got = got.detach().to(torch.float64).cpu()
    ref = torch.as_tensor(ref, dtype=torch.float64)
    assert torch.isfinite(got).all()
    return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def l2(got, ref):
    got, ref = got.detach().to(torch.float64).cpu().flatten(), ref.detach().to(torch.float64).flatten()
    assert torch.isfinite(got).all()
    return float((got - ref).norm() / max(float(ref.norm()), 1e-300))


def cos(got, ref):
    got, ref = got.detach().to(torch.float64).cpu().flatten(), ref.detach().to(torch.float64).flatten()
    return float((got @ ref) / max(float(got.norm() * ref.norm()), 1e-300))


# image 2x down (scalar path, zeros in the gradient); vector path 2x up; non-integer ratios both ways with C % 8 != 0; identity
RESIZE_CASES = [((2, 4, 4, 3), (2, 2)), ((3, 8, 8, 3), (4, 4)), ((2, 4, 4, 512), (8, 8)), ((2, 5, 7, 20), (3, 4)), ((2, 5, 7, 20), (8, 9)),
                ((1, 2, 2, 8), (2, 2))]


@pytest.mark.parametrize("shape,out_hw", RESIZE_CASES)
def test_resize_nearest_value_and_gradient(gpu, shape, out_hw):
    """tf.image.resize_nearest_neighbor (TF 1.5, align_corners=False): the forward pass is a copy and must be exact; the backward
    pass sums at most a handful of bf16 values in fp32 and rounds once: relative error <= 1e-2 (the bound of the blend test)."""
    from gan_lib_tensorflow_amd import functional as Fn
    rng = np.random.default_rng(sum(shape) + out_hw[0])
    x, xt = bf(rng.normal(size=shape))
    xr = x.clone().requires_grad_(True)
    ref = R.resize_nearest(xr, out_hw)
    xt.requires_grad_(True)
    out = Fn.resize_nearest(xt, out_hw)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    assert torch.equal(out.detach().double().cpu(), ref.detach())
    dy, dyt = bf(rng.normal(size=ref.shape))
    ref.backward(dy)
    out.backward(dyt)
    assert xt.grad.shape == xr.grad.shape
    e = rel(xt.grad, xr.grad)
    print("resize_nearest", shape, "->", out_hw, "gradient rel err", e)
    assert e <= 1e-2
    untouched = xr.grad == 0
    if out_hw[0] < shape[1]:
        assert bool(untouched.any())                                     # sources no destination reads ...
    assert float(xt.grad.double().cpu()[untouched].abs().max() if bool(untouched.any()) else 0.0) == 0.0       # ... get exact zeros


def make(bc, trans, batch, seed=3, model='resnet'):
    from gan_lib_tensorflow_amd.PGGAN.train import PGGANTrainer, default_args
    args = default_args(batch_size=batch, block_count=bc, image_size=4 * 2 ** bc, trans=trans, max_iter=1000, model=model)
    tr = PGGANTrainer(args, seed=seed)
    return tr, tr.store.state_dict()


def _bad_grads(tr, names, gref, l2_max, cos_min):
    """tensors outside cosine >= cos_min / relative L2 <= l2_max; a gradient that is ~0 in the restatement (the last layer's bias
    when every hinge margin is active: -1/n per real + 1/n per fake) is bounded absolutely instead"""
    bad, worst = [], [1.0, 0.0]
    gmax = max(float(g.abs().max()) for g in gref.values())
    for k in names:
        g, r = tr.store.vars[k].main_grad, gref[k]
        if float(r.abs().max()) < 1e-6 * gmax:
            if float(g.abs().max()) > 1e-3 * gmax:
                bad.append((k, 'abs', float(g.abs().max())))
            continue
        c, e = cos(g, r), l2(g, r)
        worst = [min(worst[0], c), max(worst[1], e)]
        if c < cos_min or e > l2_max:
            bad.append((k, c, e))
    print("   worst cosine", worst[0], "worst relative L2", worst[1])
    return bad


# Bounds of the model tests.  Base: those of tests/test_pggan_gpu.py, whose path has no batch statistics -- images 2e-2 of the range,
# logits 3e-2 and losses 2e-2 of max(1, |ref|), gradients cosine >= 0.99 and relative L2 <= 0.1 per tensor.  This path normalises with
# batch statistics over as few as 8 * 16 values per channel, which amplifies what bf16 storage does.  That amplification was measured
# on the CPU, without the product: the restatement with bf16 storage emulation (oracle.ref_torch.STORE = bf16_storage on every tensor
# the product path stores) against the float64 restatement, init_params seeds 3 and 4, the inputs of this test, the larger of the two
# runs.  Rule, fixed before any GPU run: bound = max(base, 2 x that emulated error) (a cosine c counts as the error 1 - c).  Measured
# emulation errors (they are what the bounds are derived from; logits <= 1.3e-4 and losses <= 4.6e-5 stay far inside their base):
#   (0, False): image 0.0141; critic gradients cos 0.99945 / L2 0.0332; generator gradients cos 0.98635 / L2 0.1647
#   (1, True):  image 0.0216; critic gradients cos 0.99836 / L2 0.0572; generator gradients cos 0.98556 / L2 0.1705
#   (2, True):  image 0.0294; critic gradients cos 0.99930 / L2 0.0374; generator gradients cos 0.98127 / L2 0.1932
#   (3, True), forward only, batch 4: image 0.0397 (mean 0.0047), logits 6.1e-5
BOUNDS = {
    (0, False): dict(img=2 * 0.0141, logit=3e-2, loss=2e-2, d_cos=0.99, d_l2=0.1, g_cos=1 - 2 * (1 - 0.98635), g_l2=2 * 0.1647),
    (1, True): dict(img=2 * 0.0216, logit=3e-2, loss=2e-2, d_cos=0.99, d_l2=2 * 0.0572, g_cos=1 - 2 * (1 - 0.98556), g_l2=2 * 0.1705),
    (2, True): dict(img=2 * 0.0294, logit=3e-2, loss=2e-2, d_cos=0.99, d_l2=0.1, g_cos=1 - 2 * (1 - 0.98127), g_l2=2 * 0.1932),
}
FWD32_IMG, FWD32_LOGIT = 2 * 0.0397, 3e-2


@pytest.mark.parametrize("bc,trans", [(0, False), (1, True), (2, True)])
def test_pggan_resnet_model_losses_gradients_vs_restatement(gpu, bc, trans):
    """Generator images and critic logits, the two losses and their gradients w.r.t. every trainable variable, and the `u`
    vectors after a critic update's two passes (real: written; fake: NO_OPS), against the float64 restatement from the same
    parameters, noise and fade-in weight.  The real images have negative pixels: the fromRGB blocks' main branch sees
    relu(image), their shortcut the raw image."""
    batch, alpha = 8, 0.37
    B = BOUNDS[(bc, trans)]
    tr, state = make(bc, trans, batch)
    names = sorted(state)
    assert names == sorted(R.init_params(0, bc, trans)), set(names) ^ set(R.init_params(0, bc, trans))      # the reference's variable names
    P = T.to_torch(state)
    rng = np.random.default_rng(bc)
    z, zt = bf(rng.normal(size=(batch, 512)))
    size = 4 * 2 ** bc
    real, realt = bf(np.clip(rng.normal(size=(batch, size, size, 3)) * 0.5, -1, 1))
    assert float(real.min()) < -0.5
    with torch.no_grad():
        img = tr.model.get_generator(zt, alpha, reuse=True)
        lg = tr.model.get_discriminator(realt, alpha, update_collection='NO_OPS', reuse=True)
        img_ref = R.generator(P, z, alpha, bc, trans)
        lg_ref, _ = R.discriminator(P, real, alpha, bc, trans)
    assert img.shape == (batch, size, size, 3)
    scale = max(1.0, float(img_ref.abs().max()))
    e_img = float((img.double().cpu() - img_ref).abs().max()) / scale
    e_lg = float((lg.double().cpu() - lg_ref).abs().max()) / max(1.0, float(lg_ref.abs().max()))
    print("pggan resnet", (bc, trans), "image", e_img, "logits", e_lg)
    assert e_img < B['img']
    assert e_lg < B['logit']
    # critic loss: values, gradients, u policy
    loss_ref, new_u = R.d_loss(P, real, z, alpha, bc, trans)
    dn = T.trainable_names(P, 'd_net')
    gref = dict(zip(dn, torch.autograd.grad(loss_ref, [P[k] for k in dn])))
    loss = tr.d_loss(realt, z=zt, alpha=alpha)
    tr._backward(loss)
    torch.cuda.synchronize()
    print("   d loss", float(loss), "ref", float(loss_ref.detach()))
    assert abs(float(loss) - float(loss_ref)) < B['loss'] * max(1.0, abs(float(loss_ref)))
    assert _bad_grads(tr, dn, gref, B['d_l2'], B['d_cos']) == []
    assert sorted(new_u) == sorted(k for k in names if k.endswith('spectral_norm/u'))
    for k, u in new_u.items():
        assert rel(tr.store.vars[k], u) < 1e-3, k                   # written once, by the real pass
    tr.d_flat['grads'].zero_()
    # generator loss
    P = T.to_torch(tr.store.state_dict())                            # u has advanced
    loss_ref = R.g_loss(P, z, alpha, bc, trans)
    gn = T.trainable_names(P, 'g_net')
    assert not any('moving_' in k for k in gn) and sorted(gn) == sorted(tr.g_flat['names'])
    gref = dict(zip(gn, torch.autograd.grad(loss_ref, [P[k] for k in gn])))
    loss = tr.g_loss(z=zt, alpha=alpha)
    tr._backward(loss)
    torch.cuda.synchronize()
    print("   g loss", float(loss), "ref", float(loss_ref.detach()))
    assert abs(float(loss) - float(loss_ref)) < B['loss'] * max(1.0, abs(float(loss_ref)))
    assert _bad_grads(tr, gn, gref, B['g_l2'], B['g_cos']) == []
    assert all(float(tr.store.vars[k].main_grad.abs().max()) == 0.0 for k in dn)     # gen_cost moves g_vars only (train.py:115,133)


def test_pggan_resnet_forward_at_32_fading_vs_restatement(gpu):
    """32 x 32 with the fourth block fading in (channels 1024, 512, 512, 512 -> 256), batch 4: generator images and critic logits
    against the float64 restatement (forward only: the float64 backward pass of this size takes too long for the suite)."""
    bc, trans, batch, alpha = 3, True, 4, 0.37
    tr, state = make(bc, trans, batch, seed=9)
    P = T.to_torch(state, requires_grad=False)
    rng = np.random.default_rng(6)
    z, zt = bf(rng.normal(size=(batch, 512)))
    real, realt = bf(np.clip(rng.normal(size=(batch, 32, 32, 3)) * 0.5, -1, 1))
    with torch.no_grad():
        img = tr.model.get_generator(zt, alpha, reuse=True)
        img_ref = R.generator(P, z, alpha, bc, trans)
        lg = tr.model.get_discriminator(realt, alpha, update_collection='NO_OPS', reuse=True)
        lg_ref, _ = R.discriminator(P, real, alpha, bc, trans)
    assert img.shape == (batch, 32, 32, 3)
    scale = max(1.0, float(img_ref.abs().max()))
    d = (img.double().cpu() - img_ref).abs()
    e_lg = float((lg.double().cpu() - lg_ref).abs().max()) / max(1.0, float(lg_ref.abs().max()))
    print("pggan resnet 32x32 image max |delta|", float(d.max()), "mean", float(d.mean()), "range", scale, "logits", e_lg)
    assert float(d.max()) < FWD32_IMG * scale
    assert e_lg < FWD32_LOGIT


def test_pggan_resnet_training_steps(gpu, deterministic_stats):
    """train.py:185-193 with `--model resnet` at the 16x16 stage with a block fading in, batch 16, on the captured-graph path: 1
    generator + 5 critic updates per step; parameters move by at most ~lr per update and stay finite; the generator's batch-norm
    moving statistics advance but are no optimiser state."""
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import synthetic_batches
    tr, _ = make(2, True, 16, seed=5)
    assert tr.graphs.enabled
    feed = synthetic_batches(16, "cuda", seed=2)
    x = tr.real_images(next(feed)[0])
    assert x.shape == (16, 16, 16, 3) and float(x.abs().max()) <= 1.01
    assert not any('moving_' in k for k in tr.g_flat['names']) and not any('spectral_norm/u' in k for k in tr.d_flat['names'])
    p0d, p0g = tr.d_flat['params'].clone(), tr.g_flat['params'].clone()
    for _ in range(3):
        tr.train_iteration(feed)
    torch.cuda.synchronize()
    assert set(tr.graphs.graphs) == {'d', 'g'}                       # both updates were captured and replayed
    assert tr.step == 3 and int(tr.d_opt['t']) == 15 and int(tr.g_opt['t']) == 3 and abs(tr.alpha() - 0.003) < 1e-12
    for flat, p0, n in ((tr.d_flat, p0d, 15), (tr.g_flat, p0g, 3)):
        assert bool(torch.isfinite(flat['params']).all()) and float(flat['grads'].abs().max()) == 0.0     # cleared by the Adam launch
        moved = (flat['params'] - p0).abs()
        assert 1e-5 < float(moved.max()) < n * 1e-4 * 3      # beta1 = 0: a step is lr * g / rms(g history), above lr when a gradient outgrows its history
    assert all(np.isfinite(float(v)) for v in tr.losses.values())
    mm = [v for k, v in tr.store.vars.items() if k.startswith('g_net/') and k.endswith('BatchNorm/moving_mean')]
    assert len(mm) == 2 + 2 * 4 and all(bool(torch.isfinite(v).all()) and float(v.abs().max()) > 0.0 for v in mm)      # has left zero
    img = tr.sample(10)
    assert img.shape == (10, 16, 16, 3) and bool(torch.isfinite(img.float()).all())


def test_pggan_trainer_model_switch(gpu):
    """`args.model` (train.py:62-67): 'resnet' builds model_resnet.PGGAN, 'nvidia' model_nvidia.PGGAN, anything else raises; a
    fade-in without a block to fade in raises (the reference graph would ask for G.UpBlock.0)."""
    from gan_lib_tensorflow_amd.PGGAN import model_nvidia, model_resnet
    from gan_lib_tensorflow_amd.PGGAN.train import PGGANTrainer, default_args
    tr, state = make(0, False, 2)
    assert type(tr.model) is model_resnet.PGGAN and 'g_net/G.0_toRGB.Conv1/Filters' in state
    tr, state = make(0, False, 2, model='nvidia')
    assert type(tr.model) is model_nvidia.PGGAN and 'g_net/G.0_toRGB/Filters' in state
    with pytest.raises(NotImplementedError, match='Not supported model!'):
        PGGANTrainer(default_args(batch_size=2, model='dcgan'))
    with pytest.raises(ValueError):
        PGGANTrainer(default_args(batch_size=2, model='resnet', trans=True))
