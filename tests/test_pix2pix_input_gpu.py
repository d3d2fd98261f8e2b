"""GPU: the Pix2Pix input pipeline (csrc/pix_input.hip, Pix2Pix/train.py) against the float64 restatement of
tests/pix2pix_input_ref.py, which tests/test_pix2pix_input_cpu.py pins by known answers.  Every test prints the figure it
measured before it asserts.  Raw frames are at most 96 x 390 except in the trainer test."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pix2pix_input_cases as PC  # noqa: E402
import pix2pix_input_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _K():
    from gan_lib_tensorflow_amd import kernels as K
    return K


def _f64(t):
    return t.to(torch.float64).cpu().numpy()


def _grid():
    g = np.arange(0, 256, 5) / 255.0
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


# ---- 1. placement --------------------------------------------------------------------------------------------------------
def _placed_source_pixels(raw, table, panels, wp, crop):
    """the uint8 source pixel behind every output pixel when scale == source size: per panel, flipped, cropped -> list of [N,crop,crop,3]"""
    out = []
    for k in range(panels):
        pan = [img[:, k * wp:(k + 1) * wp] for img in raw]
        pan = [p[:, ::-1] if flip else p for p, (flip, _, _) in zip(pan, table)]
        out.append(np.stack([p[oy:oy + crop, ox:ox + crop] for p, (_, oy, ox) in zip(pan, table)]))
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("direction", [0, 1])
def test_placement_is_nearly_exact(mode, direction):
    """scale == source size: every output is ONE source pixel, so the fp32 output is x * 2 / 255 - 1 of the right pixel within
    2^-22 (a few fp32 ulp between the two ways of writing the affine map); neighbouring 8-bit levels are 7.8e-3 apart, so a wrong
    panel, a mirrored axis or swapped offsets fail.  Modes 0 and 1 compare with the affine map written here.  Mode 2 (Lab) is not
    an affine map of one byte, so it is compared twice: with the restatement at the Lab bound of test 3, and -- independent of
    the restatement -- with preprocess_lab of gank_rgb_to_lab of the source pixel that belongs at (y, x), gathered here, within
    the same 2^-22 (the same fp32 function of the same fp32 argument; L / 50 - 1 and a / 110 are one division and one
    subtraction, each correctly rounded on both sides, and 2^-22 is 2 ulp below 1).  Flips on and off, offset_y != offset_x."""
    K = _K()
    h, wp, crop, panels = 80, 72, 48, {0: 2, 1: 3, 2: 1}[mode]
    rng = np.random.RandomState(10 * mode + direction)
    raw = rng.randint(0, 256, size=(4, h, wp * panels, 3)).astype(np.uint8)
    table = np.array([[0, 5, 17], [1, 31, 2], [1, 0, 24], [0, 32, 23]], np.int32)
    ins, tgs = K.pix2pix_load_examples(torch.from_numpy(raw).cuda(), torch.from_numpy(table).cuda(), mode, direction, h, wp, crop, dtype=torch.float32)
    ins, tgs = _f64(ins), _f64(tgs)
    src = _placed_source_pixels(raw, table, panels, wp, crop)
    bound = 2.0 ** -22
    if mode == 2:
        ri, rt = R.load_examples(raw, mode, direction, h, wp, crop, table)
        dev = max(np.abs(ins - ri).max(), np.abs(tgs - rt).max())
        print(f"placement mode 2 direction {direction} against the restatement: max deviation {dev:.3e} (bound {LAB_BOUND:.3e})")
        assert ins.shape == ri.shape and tgs.shape == rt.shape and dev <= LAB_BOUND
        lab = K.rgb_to_lab(torch.from_numpy(src[0].astype(np.float32) * np.float32(1.0 / 255.0)).cuda())
        a, b = _f64(lab[..., :1] / 50 - 1), _f64(lab[..., 1:] / 110)
    else:
        x = [p.astype(np.float64) * 2 / 255 - 1 for p in src]
        a, b = np.concatenate(x[:-1], axis=3), x[-1]
    ri, rt = (a, b) if direction == 0 else (b, a)
    dev = max(np.abs(ins - ri).max(), np.abs(tgs - rt).max())
    print(f"placement mode {mode} direction {direction}: max deviation {dev:.3e} (bound {bound:.3e})")
    assert ins.shape == ri.shape and tgs.shape == rt.shape and dev <= bound


def test_out_of_range_table_rows():
    """A DEVICE table cannot be refused on the host: the kernel clamps offset_y / offset_x into [0, scale - crop] and takes any
    non-zero flip as 1, so rows far outside (negative, huge, INT_MIN / INT_MAX) give bit for bit what the clamped rows give --
    every value a real source pixel's, nothing read outside the frame -- in all three modes, with a resize and without.  The raw
    buffer's size is no multiple of 4, so the last dword of the last row is the kernel's guarded tail.  The same rows in a HOST
    table raise before any launch."""
    K = _K()
    big = np.iinfo(np.int32)
    wild = np.array([[7, -5, 1000], [-1, 99999, -3], [0, big.min, big.max], [1, big.max, big.min], [0, 30, -30]], np.int32)
    for mode, panels in ((0, 2), (1, 3), (2, 1)):
        for h, wp, sh, sw, crop in ((41, 37, 41, 37, 29), (50, 45, 40, 36, 32)):
            raw = np.random.RandomState(mode).randint(0, 256, size=(5, h, wp * panels, 3)).astype(np.uint8)
            assert raw.size % 4 != 0 or h == 50
            tame = np.stack([(wild[:, 0] != 0).astype(np.int32), np.clip(wild[:, 1], 0, sh - crop), np.clip(wild[:, 2], 0, sw - crop)], axis=1).astype(np.int32)
            rawd = torch.from_numpy(raw).cuda()
            got = K.pix2pix_load_examples(rawd, torch.from_numpy(wild).cuda(), mode, 0, sh, sw, crop, dtype=torch.float32)
            want = K.pix2pix_load_examples(rawd, torch.from_numpy(tame).cuda(), mode, 0, sh, sw, crop, dtype=torch.float32)
            ri, rt = R.load_examples(raw, mode, 0, sh, sw, crop, tame)
            for g, w, r in zip(got, want, (ri, rt)):
                assert torch.equal(g.view(torch.int32), w.view(torch.int32)), (mode, h)
                assert np.abs(_f64(g) - r).max() <= PC.F32_BOUND + (LAB_BOUND if mode == 2 else 0), (mode, h)
            with pytest.raises(RuntimeError, match=r"outside \[0, scale - crop\]"):
                K.pix2pix_load_examples(rawd, wild, mode, 0, sh, sw, crop, dtype=torch.float32)
            assert all(torch.equal(a, b) for a, b in zip(K.pix2pix_load_examples(rawd, tame, mode, 0, sh, sw, crop, dtype=torch.float32), want))


# ---- 2. AREA ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.AREA_CASES))
@pytest.mark.parametrize("mode", [0, 1])
def test_area_against_the_restatement(name, mode):
    """fp32 within 2e-5 absolute, the 16-bit output of the bf16 library within 2^-9 + 2e-5; no element is excluded"""
    K = _K()
    dev = PC.run_area_case(name, torch.float32, mode, direction=mode)
    print(f"AREA {name} mode {mode} fp32: max deviation {dev:.3e} (bound {PC.F32_BOUND:.1e})")
    assert dev <= PC.F32_BOUND
    assert K.BF16 is torch.bfloat16
    dev = PC.run_area_case(name, K.BF16, mode, direction=mode)
    print(f"AREA {name} mode {mode} bf16: max deviation {dev:.3e} (bound {PC.BF16_BOUND:.3e})")
    assert dev <= PC.BF16_BOUND


def test_area_fp16_library(tmp_path):
    """the same cases with the fp16 library in a process of its own (GANK_DTYPE is per process): 2^-12 + 2e-5"""
    out = tmp_path / "results.json"
    env = dict(os.environ, GANK_DTYPE="fp16")
    env.pop("GANK_LIB_NAME", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pix2pix_input_fp16_worker.py"), str(out)], env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-3000:])
    results = json.loads(out.read_text()) if out.exists() else {}
    assert r.returncode == 0 and sorted(results) == sorted(PC.AREA_CASES), r.stdout[-2000:] + r.stderr[-3000:]
    assert all(v.startswith("ok") for v in results.values()), results


# ---- 3. Lab ----------------------------------------------------------------------------------------------------------------
LAB_BOUND = 1e-5        # about 10x the float32-emulation floor (4.2e-7 / 9.8e-7 / 4.2e-7); see the module docstring of the CPU tests


def test_lab_mode_against_the_restatement():
    """mode 2, fp32: preprocessed L / a / b within 1e-5 of the restatement -- on the colour grid (every 5th 8-bit level, 52^3
    colours as 52 frames of 52 x 52, scale == size) and on a resized noise frame."""
    K = _K()
    raw = np.round(_grid() * 255).astype(np.uint8).reshape(52, 52, 52, 3)        # the crop is square: 52 frames of 52 x 52
    table = np.zeros((52, 3), np.int32)
    ins, tgs = K.pix2pix_load_examples(torch.from_numpy(raw).cuda(), torch.from_numpy(table).cuda(), 2, 0, 52, 52, 52, dtype=torch.float32)
    ri, rt = R.load_examples(raw, 2, 0, 52, 52, 52, table)
    dl, dab = np.abs(_f64(ins) - ri).max(), np.abs(_f64(tgs) - rt).max(axis=(0, 1, 2))
    print(f"Lab grid: max deviation L {dl:.3e}  a {dab[0]:.3e}  b {dab[1]:.3e} (bound {LAB_BOUND:.0e})")
    assert dl <= LAB_BOUND and (dab <= LAB_BOUND).all()
    dev = max(PC.run_area_case(name, torch.float32, mode=2, direction=d) for name in PC.AREA_CASES for d in (0, 1))
    print(f"Lab resized noise: max deviation {dev:.3e} (bound {LAB_BOUND + PC.F32_BOUND:.1e})")
    assert dev <= LAB_BOUND + PC.F32_BOUND


def test_rgb_to_lab_and_back_against_the_restatement():
    """gank_rgb_to_lab on the colour grid: L, a, b within 50 / 110 / 110 x 1e-5 (the bound of the preprocessed values, undone);
    gank_lab_to_rgb on those Lab values within 1e-5 of its restatement; the Python names agree with the kernels."""
    from gan_lib_tensorflow_amd.Pix2Pix import train as P
    x = _grid()
    lab = P.rgb_to_lab(x.reshape(-1, 1, 3).astype(np.float32))
    ref = R.rgb_to_lab(x.astype(np.float32).astype(np.float64)).reshape(-1, 1, 3)
    dev = np.abs(_f64(lab) - ref).max(axis=(0, 1))
    print(f"rgb_to_lab grid: max deviation L {dev[0]:.3e} a {dev[1]:.3e} b {dev[2]:.3e} (bounds 5e-4 / 1.1e-3 / 1.1e-3)")
    assert dev[0] <= 50 * LAB_BOUND and dev[1] <= 110 * LAB_BOUND and dev[2] <= 110 * LAB_BOUND
    lab32 = ref.astype(np.float32)
    back = P.lab_to_rgb(lab32)
    dev = np.abs(_f64(back) - R.lab_to_rgb(lab32.astype(np.float64))).max()
    print(f"lab_to_rgb grid: max deviation {dev:.3e} (bound {LAB_BOUND:.0e})")
    assert dev <= LAB_BOUND
    assert np.abs(_f64(back).reshape(-1, 3) - x).max() < 3.6e-5 + 2 * LAB_BOUND          # the round trip's own floor


NEAR = 1e-6 * 127.75


# ---- 4. convert_u8 ---------------------------------------------------------------------------------------------------------
def test_convert_u8_is_the_integer_formula():
    """fp32 inputs on a grid of 200 001 values over [-1.5, 1.5], without the x within 1e-6 of a truncation boundary (its
    (x+1)/2 * 255.5 within 1e-6 * 127.75 of an integer), where fp32 and float64 may truncate differently: about 0.03 % of the
    grid, printed and required to stay under 1 %.  Inputs outside [-1, 1] saturate to 0 / 255."""
    K = _K()
    x = np.linspace(-1.5, 1.5, 200001).astype(np.float32)
    y = (x.astype(np.float64) + 1) / 2 * 255.5
    keep = np.abs(y - np.round(y)) > NEAR
    dropped = 1 - keep.mean()
    got = K.pix2pix_convert_u8(torch.from_numpy(x).cuda().reshape(1, 1, -1, 1)).cpu().numpy().reshape(-1)
    ref = R.convert_u8(x)
    print(f"convert_u8: {dropped:.4%} of the grid dropped; mismatches on the rest: {(got != ref)[keep].sum()}")
    assert dropped < 0.01 and np.array_equal(got[keep], ref[keep])
    assert got[x <= -1].max() == 0 and got[x >= 1].min() == 255 and got[0] == 0 and got[-1] == 255
    # bf16 inputs and the [0, 1] form of convert()
    from gan_lib_tensorflow_amd.Pix2Pix import train as P
    xb = torch.from_numpy(x[::7].copy()).cuda().to(K.BF16).reshape(1, -1, 1, 3)
    yb = (_f64(xb) + 1) / 2 * 255.5
    kb = np.abs(yb - np.round(yb)) > NEAR
    assert np.array_equal(K.pix2pix_convert_u8(xb).cpu().numpy()[kb], R.convert_u8(_f64(xb))[kb])
    x01 = np.linspace(-0.2, 1.2, 30000).astype(np.float32).reshape(1, 100, 100, 3)
    k01 = np.abs(x01.astype(np.float64) * 255.5 - np.round(x01.astype(np.float64) * 255.5)) > NEAR
    assert np.array_equal(P.convert(x01).cpu().numpy()[k01], R.convert01(x01)[k01])


def test_convert_u8_augment_and_channel_window():
    K = _K()
    rng = np.random.RandomState(5)
    raw = rng.randint(0, 256, size=(2, 40, 40, 3)).astype(np.uint8)
    table = np.zeros((2, 3), np.int32)
    L, ab = R.load_examples(raw, 2, 0, 40, 40, 40, table)
    L32, ab32 = np.ascontiguousarray(L, np.float32), np.ascontiguousarray(ab, np.float32)
    got = K.pix2pix_convert_u8(torch.from_numpy(ab32).cuda(), brightness=torch.from_numpy(L32).cuda()).cpu().numpy().astype(int)
    ref = R.convert01(R.augment(ab32.astype(np.float64), L32.astype(np.float64))).astype(int)
    off = np.abs(got - ref).max()
    print(f"augment: max |level difference| {off}; against the source frame {np.abs(got - raw.astype(int)).max()}")
    assert got.shape == (2, 40, 40, 3) and off <= 1
    x = rng.uniform(-1, 1, size=(2, 16, 16, 6)).astype(np.float32)
    got = K.pix2pix_convert_u8(torch.from_numpy(x).cuda(), c0=3, cw=3).cpu().numpy()
    y = (x[..., 3:].astype(np.float64) + 1) / 2 * 255.5
    keep = np.abs(y - np.round(y)) > NEAR
    assert got.shape == (2, 16, 16, 3) and np.array_equal(got[keep], R.convert_u8(x[..., 3:])[keep])       # tf.split(...)[1]: the second panel


# ---- 5. determinism and batching ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 2])
def test_determinism_and_batching(mode):
    from gan_lib_tensorflow_amd.Pix2Pix import train as P
    K = _K()
    raw, table, kw = PC.area_case("96x130->80x72 crop 64", mode, n=4)
    rawd, tabd = torch.from_numpy(raw).cuda(), torch.from_numpy(table).cuda()
    call = lambda r, t: K.pix2pix_load_examples(r, t, mode, 0, kw["scale_h"], kw["scale_w"], kw["crop"], dtype=K.BF16)     # noqa: E731
    a, b = call(rawd, tabd), call(rawd, tabd)
    assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(a, b))
    for i in range(4):
        one = call(rawd[i:i + 1].contiguous(), tabd[i:i + 1].contiguous())
        assert all(torch.equal(x[0].view(torch.int16), y[i].view(torch.int16)) for x, y in zip(one, a)), i
    args = P.default_args(crop_size=64, scale_size=72, lab_colorization=mode == 2, batch_size=2)
    ex_np = P.load_examples(raw, ["a"] * 4, args, rng=np.random.RandomState(1))
    ex_dev = P.load_examples(rawd, ["a"] * 4, args, rng=np.random.RandomState(1))
    assert ex_np.count == 4 and ex_np.steps_per_epoch == 2 and ex_np.inputs.dtype == K.BF16 and ex_np.inputs.is_cuda
    assert torch.equal(ex_np.inputs.view(torch.int16), ex_dev.inputs.view(torch.int16)) and torch.equal(ex_np.targets.view(torch.int16), ex_dev.targets.view(torch.int16))
    t, scale = P.draw_transform(4, args, np.random.RandomState(1))
    ri, rt = R.load_examples(raw, mode, 0, scale, scale, 64, t)
    dev = max(np.abs(_f64(ex_np.inputs) - ri).max(), np.abs(_f64(ex_np.targets) - rt).max())
    assert dev <= PC.BF16_BOUND + (LAB_BOUND if mode == 2 else 0), dev


# ---- 6. through the trainer --------------------------------------------------------------------------------------------------
def test_through_the_trainer(tmp_path):
    """one construction of the 512 x 512 network: load_examples writes tr.inputs / tr.targets in place and matches the restatement
    under the bf16 bound of test 2; train_step on them captures its graphs and replays once with finite losses; evaluate writes
    N x 3 PNGs that decode to the convert of what was fed; msssim_score(targets, targets) is 1."""
    from PIL import Image
    from gan_lib_tensorflow_amd.Pix2Pix import train as P
    K = _K()
    args = P.default_args(batch_size=2, crop_size=512, scale_size=544, n_dis=1, max_steps=10)
    tr = P.Pix2PixTrainer(args, seed=0)
    rng = np.random.RandomState(0)
    small = rng.randint(0, 256, size=(3, 64, 128, 3)).astype(np.uint8)
    raw = np.ascontiguousarray(np.repeat(np.repeat(small, 8, axis=1), 8, axis=2))            # 512 x 1024 frames with structure
    raw = np.clip(raw.astype(int) + rng.randint(-20, 21, size=raw.shape), 0, 255).astype(np.uint8)
    ins, tgs = tr.load_examples(raw[:2], rng=np.random.RandomState(7))
    assert ins.data_ptr() == tr.inputs.data_ptr() and tgs.data_ptr() == tr.targets.data_ptr()
    table, scale = P.draw_transform(2, args, np.random.RandomState(7))
    assert scale == 544 and table[:, 1:].any()
    ri, rt = R.load_examples(raw[:2], 0, 0, 544, 544, 512, table)
    dev = max(np.abs(_f64(tr.inputs) - ri).max(), np.abs(_f64(tr.targets) - rt).max())
    print(f"trainer load_examples: max deviation {dev:.3e} (bound {PC.BF16_BOUND:.3e})")
    assert dev <= PC.BF16_BOUND
    assert abs(P.msssim_score(tr.targets, tr.targets) - 1.0) < 1e-6
    for _ in range(2):                                   # capture, then one replay
        loss = tr.train_step(*tr.load_examples(raw[:2], rng=np.random.RandomState(7)))
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and all(np.isfinite(float(v)) for v in tr.losses.values()), tr.losses
    losses = list(tr.fit_epoch(raw, np.random.RandomState(3)))
    assert len(losses) == 1 and all(np.isfinite(float(v)) for v in losses[0].values())       # 3 frames, batch 2: the tail is dropped
    paths = ["/val/3.png", "/val/1.png", "/val/2.png"]
    index = tr.evaluate(raw, paths, str(tmp_path))
    files = sorted(os.listdir(tmp_path / "images"))
    assert len(files) == 9 and index == str(tmp_path / "index.html") and open(index).read().count("<tr>") == 1 + 3
    ri, rt = R.load_examples(raw, 0, 0, 512, 512, 512, np.zeros((3, 3), np.int32))          # validation: scale_size = crop_size, no flip
    for b, stems in ((0, ("3", "1")), (2, ("2",))):
        fed = [_f64(t) for t in tr.load_examples(raw[[b, min(b + 1, 2)]], training=False)]      # what evaluate fed: the bf16 tensors
        for i, stem in enumerate(stems):
            for kind, t, ref in (("inputs", fed[0], ri), ("targets", fed[1], rt)):
                png = np.asarray(Image.open(tmp_path / "images" / f"{stem}-{kind}.png"))
                assert np.abs(t[i] - ref[b + i]).max() <= PC.BF16_BOUND
                assert png.shape == (512, 512, 3) and np.array_equal(png, R.convert_u8(t[i])), (stem, kind)
            assert np.asarray(Image.open(tmp_path / "images" / f"{stem}-outputs.png")).shape == (512, 512, 3)
