"""Every consumer of the device RNG against the host reference tests/philox_ref.py ("Device RNG contract"), on a real
MI355X: never one launch against another.  Uniforms, labels, the dequantised reals and the dropout mask / output are integer work
plus float32 products by powers of two (and one correctly rounded product or sum), so they are compared BIT FOR BIT; the normal draw
goes through log, sqrt, sin and cos in float32 and is bounded against the float64 Box-Muller instead.

Sizes: 1..7 (tails of the 4-element group), 1027, and one element count past TWO sweeps of the capped grid (2048 blocks x 256 threads
x 4 elements = 2,097,152 per sweep; dropout: 4096 x 256 x 1 = 1,048,576)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

SWEEP = 2048 * 256 * 4                      # elements that one pass of rgrid's capped grid covers
SIZES = [1, 2, 3, 4, 5, 7, 1027, 2 * SWEEP + 3]
DROPOUT_SWEEP = 4096 * 256                  # g1's cap, one element per thread: one past a full sweep is 1,048,577 < 8M
DROPOUT_SIZES = [1, 2, 3, 4, 5, 7, 1027, DROPOUT_SWEEP + 1]
SEED, OFF = 0x1234_5678_9ABC, 3             # the state of the size sweeps: both key words in use
SEEDS = [0, 2 ** 32 + 12345, 2 ** 63 - 1]
OFFSETS = [0, 2 ** 32 - 1, 2 ** 32 + 7]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from gan_lib_tensorflow_amd import kernels
    kernels.lib()
    assert kernels.BF16 is torch.bfloat16
    return kernels


def state(seed, off):
    return torch.tensor([seed, off], dtype=torch.int64, device="cuda")


def assert_state(st, seed, off):
    assert st.tolist() == [seed, off], (st.tolist(), [seed, off])


def bits16(t):
    """16-bit float tensor -> CPU int16 tensor of its bit patterns"""
    return t.reshape(-1).view(torch.int16).cpu()


def want16(a):
    """float32 array of bf16 values -> CPU int16 tensor of their bit patterns"""
    return torch.from_numpy(P.bf16_bits(np.asarray(a, np.float32).reshape(-1)).view(np.int16))


def f32bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.int32))


def assert_uniform(got, n, seed, off):
    assert got.dtype == torch.float32 and got.shape == (n,)
    assert torch.equal(got.view(torch.int32).cpu(), f32bits(P.uniform(n, seed, off)))


def assert_labels(got, n, n_labels, seed, off):
    assert got.dtype == torch.int32 and got.shape == (n,)
    assert torch.equal(got.cpu(), torch.from_numpy(P.labels(n, n_labels, seed, off)))


def assert_preprocess(got, data_u8, seed, off):
    assert torch.equal(bits16(got), want16(P.preprocess(data_u8.cpu().numpy(), seed, off)))


def assert_dropout(y, mask, x, keep, seed, off):
    ry, rm = P.dropout(x.float().cpu().numpy(), keep, seed, off)
    assert mask.dtype == torch.uint8 and torch.equal(mask.cpu(), torch.from_numpy(rm))
    assert torch.equal(bits16(y), want16(ry))


def assert_normal(got, n, seed, off):
    """|got - ref64| <= 2^-8 |ref64| + 1e-5 for every element (half a bf16 ulp, and slack for the float32 log / sqrt / sin / cos), and
    an element that is not bf16(ref64) is its NEIGHBOUR.  Returns the largest |got - ref64| - 2^-8 |ref64| and the number of neighbours."""
    assert got.dtype == torch.bfloat16 and got.numel() == n
    ref = P.normal64(n, seed, off)
    gb = bits16(got).numpy().view(np.uint16)
    g = P.bits_value(gb)
    assert np.isfinite(g).all()
    slack = float((np.abs(g - ref) - 2.0 ** -8 * np.abs(ref)).max())
    dist = np.abs(P.ordinal(gb) - P.ordinal(P.bf16_bits64(ref)))
    worst = int(dist.argmax())
    print(f"rng_normal n={n} seed={seed:#x} off={off:#x}: max(|got-ref64| - 2^-8|ref64|) = {slack:.3e}; {int((dist > 0).sum())} elements are not "
          f"bf16(ref64), the farthest by {int(dist.max())} (ref64 {ref[worst]:.6e}, got {g[worst]:.6e})")
    assert slack <= 1e-5, slack
    assert dist.max() <= 1, (worst, ref[worst], g[worst], int((dist > 1).sum()))
    return slack, int((dist > 0).sum())


def bf16_input(n, seed=0):
    """bf16 values with every exponent that activations take, both signs, zeros included"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.tensor(10.0) ** torch.randint(-3, 3, (n,), generator=g)
    x[::97] = 0.0
    return x.to(torch.bfloat16).cuda()


# ---- exact outputs, every size -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_uniform_is_the_reference_bit_for_bit(K, n):
    st = state(SEED, OFF)
    assert_uniform(K.rng_uniform(n, st), n, SEED, OFF)
    assert_state(st, SEED, OFF + 1)


@pytest.mark.parametrize("n", SIZES)
def test_labels_are_the_reference(K, n):
    """n_labels 1 (every label 0), 10 (the CIFAR classes) and 1000 (a product that float32 rounds)"""
    st = state(SEED, OFF)
    for j, n_labels in enumerate((1, 10, 1000)):
        assert_labels(K.rng_labels(n, n_labels, st), n, n_labels, SEED, OFF + j)
    assert_state(st, SEED, OFF + 3)


@pytest.mark.parametrize("n", SIZES)
def test_normal_is_box_muller_of_the_reference_stream(K, n):
    """Measured on an MI355X: max(|got - ref64| - 2^-8 |ref64|) = 0.0 at n = 4,194,307 (attained where both are exactly 0; negative
    everywhere else, -2.8e-10 at the next offset) and <= -2.7e-7 at n = 1027 over every seed and offset of this file: the float32
    evaluation never uses the 1e-5 that the bound allows.  34 to 42 of the 4,194,307 elements are the neighbour of bf16(ref64),
    none is farther.  (With the angle as 6.2831853f * u2, rounded before the reduction, a float32 restatement on the host leaves
    about 30 elements of |z| < 1.1e-4 two to eighty bf16 values away from bf16(ref64), within the 1e-5 all the same:
    csrc/loss_opt.hip, box_muller.)"""
    st = state(SEED, OFF)
    assert_normal(K.rng_normal((n,), st), n, SEED, OFF)
    assert_state(st, SEED, OFF + 1)


@pytest.mark.parametrize("n", [5, 2 * SWEEP + 3])
def test_generator_feed_draws_labels_then_noise(K, n):
    """the fused launch has block ranges and grid strides of its own: labels at off, noise at off + 1, the fill zeroed; without
    labels the noise at off"""
    st = state(SEED, OFF)
    lab, z, zb = K.generator_feed(st, (n,), 1027, n, 10)
    assert_labels(lab, n, 10, SEED, OFF)
    assert_normal(z, n, SEED, OFF + 1)
    assert zb.shape == (1027,) and float(zb.abs().max()) == 0.0
    assert_state(st, SEED, OFF + 2)
    lab, z, zb = K.generator_feed(st, (n,), 0, 0, 10)
    assert lab is None and zb is None
    assert_normal(z, n, SEED, OFF + 2)
    assert_state(st, SEED, OFF + 3)


@pytest.mark.parametrize("b", [1, 3, 700])
def test_preprocess_real_is_the_reference_bit_for_bit(K, b):
    """B = 700: 537,600 groups, past the 2048 x 256 of one sweep (B >= 683)"""
    g = torch.Generator().manual_seed(b)
    data = torch.randint(0, 256, (b, 3072), generator=g, dtype=torch.uint8)
    data[0, :256] = torch.arange(256, dtype=torch.uint8)            # every pixel value
    st = state(SEED, OFF)
    y = K.preprocess_real(data.cuda(), st)
    assert y.shape == (b, 32, 32, 3)
    assert_preprocess(y, data, SEED, OFF)
    assert_state(st, SEED, OFF + 1)


def _feed_ring(b, slots, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    real_all = torch.randint(0, 256, (slots, b, 3072), generator=g, dtype=torch.uint8)
    labels_all = torch.randint(0, 10, (slots, b), generator=g, dtype=torch.int32)
    fake_all = torch.randn((slots, b, 3072), generator=g).to(torch.bfloat16)
    return real_all, labels_all, fake_all


def test_critic_feed_real_half_is_the_reference(K):
    """B = 8, three slots, once round the ring and one step more: slot s at offset OFF + step"""
    b, slots = 8, 3
    real_all, labels_all, fake_all = _feed_ring(b, slots, 3)
    dev = [t.cuda() for t in (real_all, labels_all, fake_all)]
    both = torch.zeros((2 * b, 3072), dtype=torch.bfloat16, device="cuda")
    labels2 = torch.zeros(2 * b, dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = state(SEED, OFF)
    for step in range(slots + 1):
        i = step % slots
        K.critic_feed(*dev, both, labels2, slot, st, done)
        assert_preprocess(both[:b], real_all[i], SEED, OFF + step)
        assert torch.equal(bits16(both[b:]), bits16(fake_all[i]))
        assert torch.equal(labels2.cpu(), torch.cat([labels_all[i], labels_all[i]]))
        assert int(slot) == (i + 1) % slots and int(done) == 0
        assert_state(st, SEED, OFF + step + 1)


def test_critic_feed_inside_the_spectral_norm_launch_is_the_reference(K):
    """the feed as a block range of the second spectral-norm launch (K.defer_critic_feed with the power iteration in hand): the same
    reals at the same offsets, and the offset advances once per pass"""
    b, slots = 64, 2
    real_all, labels_all, fake_all = _feed_ring(b, slots, 4)
    dev = [t.cuda() for t in (real_all, labels_all, fake_all)]
    shapes = [(3, 3, 3, 128), (3, 3, 128, 128), (300, 128), (1, 1, 256, 128), (128, 1)]
    kinds = [0, 4, None, 0, None]
    gg = torch.Generator(device="cpu").manual_seed(8)
    Ws = [(torch.randn(sh, generator=gg) * 0.05).cuda() for sh in shapes]
    u_flat = torch.randn(sum(sh[-1] for sh in shapes), generator=gg).cuda()
    us, o = [], 0
    for sh in shapes:
        us.append(u_flat[o:o + sh[-1]].view(1, sh[-1]))
        o += sh[-1]
    sn = K.SnState(Ws, us, u_flat)
    both = torch.zeros((2 * b, 3072), dtype=torch.bfloat16, device="cuda")
    labels2 = torch.zeros(2 * b, dtype=torch.int32, device="cuda")
    slot = torch.zeros(1, dtype=torch.int32, device="cuda")
    done = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = state(SEED, OFF)
    for step in range(slots + 1):
        sn.refresh()
        assert sn.valid
        batch = K.SnBatch(Ws, us, snapshot=True, inplace=True, state=sn)
        batch.prep = (kinds, True)
        K.defer_critic_feed(*dev, both, labels2, slot, st, done)
        batch.forward()
        assert not K.deferred_critic_feed_pending()
        i = step % slots
        assert_preprocess(both[:b], real_all[i], SEED, OFF + step)
        assert torch.equal(bits16(both[b:]), bits16(fake_all[i]))
        assert int(slot) == (i + 1) % slots and int(done) == 0
        assert_state(st, SEED, OFF + step + 1)


@pytest.mark.parametrize("keep", [0.5, 0.8, 1.0])
@pytest.mark.parametrize("n", DROPOUT_SIZES)
def test_dropout_mask_and_output_are_the_reference(K, n, keep):
    x = bf16_input(n, seed=n)
    st = state(SEED, OFF)
    y, mask = K.dropout_fwd(x, keep, st)
    assert_dropout(y, mask, x, keep, SEED, OFF)
    if keep == 1.0:
        assert bool(mask.all()) and torch.equal(bits16(y), bits16(x))
    assert_state(st, SEED, OFF + 1)


# ---- state edges --------------------------------------------------------------------------------------------------------------
def run_sequence(K, st, seed, off, n=1027, x=None, data=None):
    """normal, labels, uniform, dropout, preprocess_real, generator_feed with labels, generator_feed without -- through ONE state;
    each result is the reference at its offset.  Returns the offset the state must hold afterwards."""
    x = bf16_input(n) if x is None else x
    data = torch.randint(0, 256, (2, 3072), generator=torch.Generator().manual_seed(5), dtype=torch.uint8) if data is None else data
    assert_normal(K.rng_normal((n,), st), n, seed, off)
    off += P.DRAW_ADVANCE
    assert_labels(K.rng_labels(n, 10, st), n, 10, seed, off)
    off += P.DRAW_ADVANCE
    assert_uniform(K.rng_uniform(n, st), n, seed, off)
    off += P.DRAW_ADVANCE
    y, mask = K.dropout_fwd(x, 0.8, st)
    assert_dropout(y, mask, x, 0.8, seed, off)
    off += P.DRAW_ADVANCE
    assert_preprocess(K.preprocess_real(data.cuda(), st), data, seed, off)
    off += P.DRAW_ADVANCE
    lab, z, _ = K.generator_feed(st, (n,), 0, 37, 10)
    assert_labels(lab, 37, 10, seed, off)
    assert_normal(z, n, seed, off + 1)
    off += P.generator_feed_advance(True)
    lab, z, _ = K.generator_feed(st, (n,), 0, 0, 10)
    assert lab is None
    assert_normal(z, n, seed, off)
    off += P.generator_feed_advance(False)
    return off


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("seed", SEEDS)
def test_state_edges(K, seed, off):
    """seed 0, a seed with the high key word in use, the largest seed; offset 0, 2^32 - 1 (the second draw sees the carry into the
    high counter word) and an offset beyond it"""
    st = state(seed, off)
    end = run_sequence(K, st, seed, off)
    assert end == off + 8
    assert_state(st, seed, end)


# ---- stream discipline ----------------------------------------------------------------------------------------------------------
def test_every_consumer_advances_the_one_stream_by_its_documented_increment(K):
    seed, k = 20240229, 11
    st = state(seed, k)
    end = run_sequence(K, st, seed, k)
    assert end == k + 5 * 1 + 2 + 1
    assert_state(st, seed, end)
    # 40 draws in a row: more than the 32 ticket words that the launches rotate through
    for j in range(40):
        z = K.rng_normal((5,), st)
        assert_normal(z, 5, seed, end + j)
        assert_state(st, seed, end + j + 1)


# ---- replay -----------------------------------------------------------------------------------------------------------------------
def test_a_captured_graph_draws_fresh_numbers_on_every_replay(K):
    """normal, labels, uniform and dropout on one state in ONE graph (a single stream: no parallel branches): an eager run on a side
    stream as the trainers do, the capture (which executes nothing), three replays -- each at the next four offsets"""
    from gan_lib_tensorflow_amd import graphs
    seed, start, n = 77, 2 ** 32 - 6, 1027               # the first replay crosses the carry into the high counter word
    st = state(seed, start)
    x = bf16_input(n)
    out = {}

    def step():
        out["z"] = K.rng_normal((n,), st)
        out["lab"] = K.rng_labels(n, 10, st)
        out["u"] = K.rng_uniform(n, st)
        out["y"], out["mask"] = K.dropout_fwd(x, 0.8, st)

    def check(off):
        torch.cuda.synchronize()
        assert_normal(out["z"], n, seed, off)
        assert_labels(out["lab"], n, 10, seed, off + 1)
        assert_uniform(out["u"], n, seed, off + 2)
        assert_dropout(out["y"], out["mask"], x, 0.8, seed, off + 3)
        assert_state(st, seed, off + 4)

    graphs.eager_on_side_stream(step)
    check(start)
    with graphs.capture() as g:
        step()
    torch.cuda.synchronize()
    assert_state(st, seed, start + 4)
    for r in range(1, 4):
        g.replay()
        check(start + 4 * r)
    assert_state(st, seed, start + 4 * (1 + 3))
