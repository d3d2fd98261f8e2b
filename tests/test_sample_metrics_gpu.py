"""GPU: `trainer.SampleMetrics` is its hook plus the functions under common/ and nothing else -- a trainer's `swd` against
`_metric_batch` + `common.swd.calculate_swd` on a second trainer of the same seed, for equality of the values and of the device
RNG state afterwards, and the hook's first batch against the draw sequence it documents, written out by hand.  SWD needs no
network weights.  (On the fixed-order batch-norm statistics: with the conv epilogues' float atomics two runs of the generator
on the same noise differ in a few quantised pixels, and the comparisons are for equality.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SWD_KW = dict(nhoods_per_image=8, dir_repeats=1, dirs_per_repeat=8)


def make(which):
    torch.cuda.set_device(0)
    if which == "sngan":
        from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
        return SNGANTrainer(batch_size=8, seed=0, use_graphs=False)
    from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
    return ACGANTrainer(batch_size=8, seed=0, use_graphs=False)


@pytest.mark.parametrize("which", ["sngan", "acgan"])
def test_swd_is_the_hook_plus_calculate_swd(which, deterministic_stats):
    from gan_lib_tensorflow_amd.common.swd import calculate_swd
    real = np.random.RandomState(4).randint(0, 256, size=(64, 32, 32, 3)).astype(np.uint8)
    a, b = make(which), make(which)
    assert torch.equal(a.rng_state, b.rng_state)
    values, mean = a.swd(real, n=64, **SWD_KW)
    batches, have = [], 0
    with torch.no_grad():
        while have < 64:
            images, _ = b._metric_batch(b._metric_rows())
            batches.append(images)
            have += len(images)
    fake = torch.cat(batches)[:64]
    assert fake.dtype == torch.uint8 and tuple(fake.shape) == (64, 32, 32, 3) and fake.is_cuda
    want_values, want_mean = calculate_swd(fake, real, **SWD_KW)
    assert np.array_equal(values, want_values) and mean == want_mean
    assert torch.equal(a.rng_state, b.rng_state)


@pytest.mark.parametrize("which", ["sngan", "acgan"])
def test_the_hook_draws_in_the_documented_order(which, deterministic_stats):
    from gan_lib_tensorflow_amd import kernels as K
    from gan_lib_tensorflow_amd.common.msssim import quantize_on_device
    from gan_lib_tensorflow_amd.store import set_default_store
    tr = make(which)
    rows = tr._metric_rows()
    assert rows == (100 if which == "sngan" else 8)
    saved = tr.rng_state.clone()
    with torch.no_grad():
        images, labels = tr._metric_batch(rows)
        after = tr.rng_state.clone()
        tr.rng_state.copy_(saved)
        if which == "sngan":           # labels, then sample(100, labels): the draws of sample(100)
            want_labels = K.rng_labels(100, 10, tr.rng_state)
            x = tr.sample(100, want_labels)
        else:                          # noise, then labels, then the generator
            set_default_store(tr.store)
            z = K.rng_normal((8, tr.z_dim), tr.rng_state)
            want_labels = K.rng_labels(8, 10, tr.rng_state)
            x = tr.model.get_generator(z, want_labels)
    assert torch.equal(labels, want_labels)
    assert torch.equal(images, quantize_on_device(x).reshape(-1, 32, 32, 3))
    assert torch.equal(tr.rng_state, after) and not torch.equal(after, saved)
