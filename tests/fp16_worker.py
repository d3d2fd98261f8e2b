"""Runs in its own process with GANK_DTYPE=fp16 (libgank_f16.so: the same kernels built for IEEE-half buffers and
v_mfma_f32_32x32x16_f16): convolution kernels of every family, conditional batch norm, and the SNGAN networks with both
losses and their gradients against the float64 oracle on fp16-rounded inputs.  Every check is a SECTION of its own: a failure
is recorded (traceback) and the remaining sections still run; the results go to the JSON file named by argv[1] as
{section: "ok" | traceback} and one `ok ...` / `FAILED ...` line per section to stdout; exit status 1 if any failed.
Started once per session by tests/test_fp16_gpu.py, which turns each section into its own test id."""
import json
import os
import sys
import traceback

assert os.environ.get("GANK_DTYPE") == "fp16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gan_lib_tensorflow_amd import _lib, kernels as K  # noqa: E402
from gan_lib_tensorflow_amd import functional as Fn  # noqa: E402
from oracle import ref_ops as R  # noqa: E402
from oracle import ref_torch as T  # noqa: E402

assert K.BF16 is torch.float16 and _lib.load().gank_act_dtype() == 1 and _lib.LIB_PATH.endswith("libgank_f16.so")
HALF_TOL, F32_TOL = 2e-3, 5e-4          # half: 11-bit significand (bf16: 8): tighter than the bf16 tests' 1e-2 / 2e-3


def h(a):
    t = torch.tensor(np.asarray(a, np.float32)).to(torch.float16)
    return t.to(torch.float64).numpy(), t.cuda().contiguous()


def relerr(got, ref):
    got = got.detach().to(torch.float64).cpu().numpy()
    assert np.isfinite(got).all()
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)



SECTIONS = {}


def section(name):
    def reg(fn):
        SECTIONS[name] = fn
        return fn
    return reg


CONV_SHAPES = {"two-group": (64, 32, 256, 256, 3), "patch": (8, 16, 256, 128, 3), "generic 8x8": (4, 8, 128, 128, 3),
               "1x1": (4, 8, 256, 128, 1), "narrow input": (4, 32, 3, 128, 3)}


# ---- convolution engines: two-group LDS-DMA kernel, LDS-patch kernel, generic, narrow input, phase form, all-taps / filter-row wgrad
def _conv(name):
    n, hw, cin, cout, k = CONV_SHAPES[name]
    rng = np.random.default_rng(sorted(CONV_SHAPES).index(name))
    x, xt = h(rng.normal(size=(n, hw, hw, cin)))
    w, _ = h(rng.normal(size=(k, k, cin, cout)) / np.sqrt(k * k * cin))
    b = rng.normal(size=cout).astype(np.float32)
    wt = torch.tensor(w, dtype=torch.float32).cuda()
    wf, wd = K.prep_weights(wt, True, True)
    K.prof_enable(True); K.prof_reset()
    y = K.conv2d_fprop(xt, wf, torch.tensor(b).cuda(), (hw, hw), cout, k)
    torch.cuda.synchronize()
    ran = [r[0] for r in K.prof_kernels(0)]
    K.prof_enable(False)
    if n * hw * hw <= 4096:
        ref = R.conv2d_same(x, w, b.astype(np.float64))
        assert relerr(y, ref) < HALF_TOL, (name, relerr(y, ref))
        dy, dyt = h(rng.normal(size=ref.shape))
        rdx, rdw, _ = R.conv2d_same_grads(x, w, dy)
        assert relerr(K.conv2d_dgrad(dyt, wd, (hw, hw), cin, k), rdx) < HALF_TOL, name
        dw = K.conv2d_wgrad(xt, dyt, torch.zeros_like(wt), (hw, hw), k)
        assert relerr(dw, rdw) < F32_TOL, (name, relerr(dw, rdw))
    else:       # the large shape: against torch-CPU float64 conv on a slice of the batch
        ref = T.conv2d_same(torch.tensor(x[:2]), torch.tensor(w), torch.tensor(b.astype(np.float64))).numpy()
        assert relerr(y[:2], ref) < HALF_TOL, (name, relerr(y[:2], ref))
    return str(ran[:1])


for _name in CONV_SHAPES:
    section("conv " + _name)(lambda _name=_name: _conv(_name))


@section("upconv phase form")
def _upconv():
    rng = np.random.default_rng(10)
    x, xt = h(rng.normal(size=(4, 8, 8, 128)))
    w, _ = h(rng.normal(size=(3, 3, 128, 256)) / 34.)
    wph, _ = K.upconv3x3_prep(torch.tensor(w, dtype=torch.float32).cuda())
    assert relerr(K.upconv3x3_fprop(xt, wph, None, 256), R.conv2d_same(R.upsample_nn2x(x), w)) < 2 * HALF_TOL     # the summed taps are rounded once more


@section("wgrad all-taps")
def _wgrad_taps():
    rng = np.random.default_rng(11)
    x, xt = h(rng.normal(size=(64, 16, 16, 256)))
    dy, dyt = h(rng.normal(size=(64, 16, 16, 256)))
    dw = K.conv2d_wgrad(xt, dyt, torch.zeros((3, 3, 256, 256), dtype=torch.float32, device="cuda"), (16, 16), 3)
    xr, dyr = torch.tensor(x), torch.tensor(dy)
    wr = torch.zeros(3, 3, 256, 256, dtype=torch.float64, requires_grad=True)
    (T.conv2d_same(xr, wr) * dyr).sum().backward()
    assert relerr(dw, wr.grad.numpy()) < F32_TOL


@section("cond_batchnorm")
def _cbn():
    # ---- conditional batch norm (statistics in fp32)
    rng = np.random.default_rng(12)
    x, xt = h(rng.normal(size=(8, 8, 8, 256)) * 2 + 0.5)
    labels = rng.integers(0, 10, 8)
    gamma = (1 + 0.2 * rng.normal(size=(10, 256))).astype(np.float32)
    beta = (0.1 * rng.normal(size=(10, 256))).astype(np.float32)
    y, stats = K.cbn_fwd(xt, torch.tensor(labels, dtype=torch.int32).cuda(), torch.tensor(gamma).cuda(), torch.tensor(beta).cuda(), 2, True)
    ry, _ = R.cond_batchnorm_forward(x, labels, gamma.astype(np.float64), beta.astype(np.float64), 2)
    assert relerr(y, R.relu(ry)) < HALF_TOL


# ---- the SNGAN networks, both losses, every gradient (batch 8: two towers of 4), and training iterations
@section("SNGAN critic loss + gradients")
def _critic():
    from gan_lib_tensorflow_amd.SNGAN import gan_cifar_resnet as S
    rng = np.random.default_rng(13)
    tr = S.SNGANTrainer(batch_size=4, seed=11, use_graphs=False)
    P = T.to_torch(tr.store.state_dict())
    b = 4
    z, zt = h(rng.normal(size=(b, 128)))
    labels = torch.tensor(rng.integers(0, 10, b), dtype=torch.int32)
    real_u8 = torch.tensor(rng.integers(0, 256, (b, 3072)), dtype=torch.uint8)
    real_pre = T.preprocess_real(real_u8, torch.zeros(b, 3072, dtype=torch.float64), torch.float64)
    real_pre = real_pre.to(torch.float16).to(torch.float64)
    loss_ref, _, _ = T.d_loss_fn(P, None, labels.long(), torch.tensor(z), None, towers=2, real_pre=real_pre)
    dn = T.trainable_names(P, 'Discriminator')
    gref = dict(zip(dn, torch.autograd.grad(loss_ref, [P[k] for k in dn])))
    tr.real_labels.copy_(labels)
    tr._d_forward_backward(real_pre=real_pre.to(torch.float16).cuda(), z=zt)
    torch.cuda.synchronize()
    assert abs(float(tr.d_loss) - float(loss_ref)) < 0.02, (float(tr.d_loss), float(loss_ref))
    worst = 1.0
    for k in dn:
        g, r = tr.store.vars[k].main_grad.double().cpu().flatten(), gref[k].flatten()
        if float(r.norm()) > 0:
            worst = min(worst, float((g @ r) / (g.norm() * r.norm())))
    assert worst > 0.99, worst
    return f"worst cosine {worst:.4f}"


@section("SNGAN generator loss + gradients")
def _generator():
    from gan_lib_tensorflow_amd.SNGAN import gan_cifar_resnet as S
    rng = np.random.default_rng(14)
    b = 4
    tr = S.SNGANTrainer(batch_size=b, seed=11, use_graphs=False)
    P = T.to_torch(tr.store.state_dict())
    z2, z2t = h(rng.normal(size=(2 * b, 128)))
    fl = torch.tensor(rng.integers(0, 10, 2 * b), dtype=torch.int32)
    loss_ref, _ = T.g_loss_fn(P, torch.tensor(z2), fl.long())
    gn = T.trainable_names(P, 'Generator')
    gref = dict(zip(gn, torch.autograd.grad(loss_ref, [P[k] for k in gn])))
    tr._g_forward_backward(z=z2t, fake_labels=fl.cuda())
    torch.cuda.synchronize()
    assert abs(float(tr.g_loss) - float(loss_ref)) < 0.02
    worst = 1.0
    for k in gn:
        if k.endswith('Biases') and 'G.Output' not in k:
            continue                                     # exactly-zero true gradient (feeds a batch norm)
        g, r = tr.store.vars[k].main_grad.double().cpu().flatten(), gref[k].flatten()
        worst = min(worst, float((g @ r) / (g.norm() * r.norm())))
    assert worst > 0.98, worst
    return f"worst cosine {worst:.4f}"


@section("SNGAN training iterations under hipGraph replay")
def _training():
    from gan_lib_tensorflow_amd.SNGAN import gan_cifar_resnet as S
    tr2 = S.SNGANTrainer(batch_size=16, seed=3, use_graphs=True)
    feed = S.synthetic_batches(16, "cuda", seed=1)
    for _ in range(4):
        tr2.train_iteration(feed)
    torch.cuda.synchronize()
    assert tr2.use_graphs and all(bool(torch.isfinite(tr2.store.flat[n]["params"]).all()) for n in ("Generator", "Discriminator"))
    assert np.isfinite(float(tr2.d_loss)) and np.isfinite(float(tr2.g_loss))
    hl = tr2.health()
    assert hl is not None and hl['G'][0] == 0 and hl['D'][0] == 0, hl
    return f"d_loss {float(tr2.d_loss):.3f}, g_loss {float(tr2.g_loss):.3f}, health {hl}"


@section("Adam skips non-finite gradients")
def _adam_guard():
    """A loss-scale overflow must not poison the optimiser state: elements with a non-finite gradient keep p, m, v and are counted
    (vector body AND the n % 4 tail); finite elements move; the gradient buffer is cleared."""
    n = 4 * 300 + 3
    g = torch.Generator().manual_seed(2)
    p0 = torch.randn(n, generator=g)
    grad = torch.randn(n, generator=g)
    bad = [5, 777, n - 1, n - 2]                # two in the vector body, two in the tail
    grad[bad[0]] = float('inf'); grad[bad[1]] = float('nan'); grad[bad[2]] = float('-inf'); grad[bad[3]] = float('nan')
    flat = {"params": p0.clone().cuda(), "grads": grad.clone().cuda(), "m": torch.zeros(n).cuda(), "v": torch.zeros(n).cuda()}
    flat["grads_all"] = flat["grads"]
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import AdamTF
    it = torch.zeros(1, dtype=torch.int64, device="cuda")
    opt = AdamTF(flat, it, grad_scale=1.0 / 1024.0, health=True)
    opt.apply()
    torch.cuda.synchronize()
    p1 = flat["params"].cpu()
    assert torch.isfinite(p1).all() and torch.isfinite(flat["m"]).all() and torch.isfinite(flat["v"]).all()
    assert all(float(p1[i]) == float(p0[i]) and float(flat["m"][i]) == 0.0 and float(flat["v"][i]) == 0.0 for i in bad)
    moved = (p1 != p0)
    assert int(moved.sum()) == n - len(bad)
    assert float(flat["grads"].abs().max()) == 0.0
    assert int(opt.health[0]) == len(bad), opt.health.tolist()


@section("device RNG against the host Philox reference")
def _rng():
    """rng_normal at n = 1027 against the float64 Box-Muller of tests/philox_ref.py: |got - ref64| <= 2^-11 |ref64| + 1e-5 (half an ulp
    of IEEE half, and the slack of the float32 log / sqrt / sin / cos); preprocess_real bit for bit under the half rounding.
    Measured on an MI355X: max(|got - ref64| - 2^-11 |ref64|) = -1.1e-7 (never beyond half an ulp)."""
    import philox_ref as P
    seed, off, n = 0x1234_5678_9ABC, 3, 1027
    st = torch.tensor([seed, off], dtype=torch.int64, device="cuda")
    z = K.rng_normal((n,), st)
    assert z.dtype == torch.float16
    ref = P.normal64(n, seed, off)
    got = z.to(torch.float64).cpu().numpy()
    slack = float((np.abs(got - ref) - 2.0 ** -11 * np.abs(ref)).max())
    print(f"rng_normal (half) n={n}: max(|got-ref64| - 2^-11|ref64|) = {slack:.3e}", flush=True)
    assert np.isfinite(got).all() and slack <= 1e-5, slack
    data = torch.randint(0, 256, (3, 3072), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    y = K.preprocess_real(data.cuda(), st)
    want = P.fp16_bits(P.preprocess(data.numpy(), seed, off + 1, rounding=P.fp16_round).reshape(-1)).view(np.int16)
    assert torch.equal(y.reshape(-1).view(torch.int16).cpu(), torch.from_numpy(want))
    assert st.tolist() == [seed, off + 2]
    return f"normal slack {slack:.3e}"


# ---- the headline batch (64 = two towers of 32; generator update on 2 x 64 fakes) with the STATIC LOSS SCALE (default 1024 for
# this build): generator gradients against the float64 oracle at 0.25 / 0.30 / 0.29 / 0.31 of the bfloat16 build's limits
# (tests/test_model_gpu.py::test_headline_batch_64...: 0.02 / 0.10 / 0.13 / 0.22 relative L2 by depth; measured here 0.0006 /
# 0.026 (a batch-norm scale table; filters 0.020) / 0.030 / 0.054, the same for every scale from 2^8 to 2^16: scratch/fp16_scale_sweep.py) -- fp16 keeps 3 more
# significand bits in every stored activation, and oracle/ref_torch.py's attribution (scratch/attribution.py) puts the whole
# generator-gradient error of a 16-bit build on the stored VALUES.  Without the scale the activation gradients underflow.
@section("SNGAN batch-64 generator gradients, loss scale 1024")
def _headline():
    from gan_lib_tensorflow_amd.SNGAN import gan_cifar_resnet as S
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    # statistics from the batch-norm kernels' fixed-order reduction (the GANK_EPILOGUE_STATS=0 option): the conv epilogue's float
    # atomics alone move single CBN-table gradients by a quarter of these limits from run to run
    Fn.CONV_EPILOGUE_STATS = False
    b = 64
    res = {}
    for scale in (1024.0, 1.0):
        tr = S.SNGANTrainer(batch_size=b, seed=21, use_graphs=False, loss_scale=scale)
        assert tr.loss_scale == scale and (tr.g_opt.health is not None) == (scale != 1.0)
        rng2 = np.random.default_rng(64)
        z2, z2t = h(rng2.normal(size=(2 * b, 128)))
        fl = torch.tensor(rng2.integers(0, 10, 2 * b), dtype=torch.int32)
        if scale == 1024.0:
            P = T.to_torch(tr.store.state_dict())
            loss_ref, _ = T.g_loss_fn(P, torch.tensor(z2), fl.long())
            gn = T.trainable_names(P, 'Generator')
            gref = dict(zip(gn, torch.autograd.grad(loss_ref, [P[k] for k in gn])))
        tr._g_forward_backward(z=z2t, fake_labels=fl.cuda())
        torch.cuda.synchronize()
        assert abs(float(tr.g_loss) - float(loss_ref)) < 5e-3
        errs = {}
        for k in gn:
            if k.endswith('Biases') and 'G.Output' not in k:
                continue
            g, r = tr.store.vars[k].main_grad.double().cpu().flatten() / scale, gref[k].flatten()
            errs[k] = (float((g @ r) / (g.norm() * r.norm())), float((g - r).norm() / r.norm()))
        res[scale] = errs
        if scale == 1024.0:
            tr.g_opt.apply()                      # the optimiser divides the scale out and counts non-finite / zero gradients
            torch.cuda.synchronize()
            hl = tr.health()
            assert hl['G'][0] == 0, hl            # no overflow at 2^10
        del tr
    bad = []
    for k, (cos, l2) in res[1024.0].items():
        lim = 0.005 if 'G.Output' in k else 0.03 if 'G.Block.3' in k else 0.0375 if 'G.Block.2' in k else 0.068
        if cos < 0.998 or l2 > lim:
            bad.append((k, cos, l2, lim))
    assert not bad, bad
    worst = max(v[1] for v in res[1024.0].values())
    worst1 = max(v[1] for v in res[1.0].values())
    by_depth = {k.split('/', 1)[1]: round(v[1], 4) for k, v in res[1024.0].items() if k.endswith(('Filters', '/W'))}
    return f"worst relative L2 {worst:.4f} (unscaled fp16: {worst1:.4f}; bf16 limit 0.22); by depth (scaled): {by_depth}"


if __name__ == "__main__":
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    only = sys.argv[2:]                     # optional: section names to run
    results = {}
    for name, fn in SECTIONS.items():
        if only and name not in only:
            continue
        try:
            note = fn()
            torch.cuda.synchronize()
            results[name] = "ok"
            print("ok", name, note or "", flush=True)
        except Exception:  # noqa: BLE001
            results[name] = traceback.format_exc()
            print("FAILED", name, "\n" + results[name], flush=True)
        if out_path:
            with open(out_path, "w") as f:
                json.dump(results, f)
    if all(v == "ok" for v in results.values()):
        print("FP16 PATH OK", flush=True)
        sys.exit(0)
    sys.exit(1)
