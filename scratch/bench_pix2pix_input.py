"""The Pix2Pix input pipeline on the GPU (Pix2Pix/train.py -> csrc/pix_input.hip): ms per batch of 16 raw frames of 512x1024 and
768x4080 (the reference's placeholder, train.py:585) in pair, multiple_A and Lab mode, to 512x512 bf16 inputs / targets, against
  - the compulsory traffic: the raw bytes read once + the output bytes written once, as GB/s and as a fraction of a plain device
    copy (torch copy_) of the same number of bytes, timed in the same run;
  - a host baseline: the same maths in NumPy float32 (separable AREA weights as two matrix products per image, PIL load excluded),
    on the CPUs this process may use.
Also display_images' gank_pix2pix_convert_u8 on 16x512x512x3 bf16.  Device times are hipEvent times over REPS launches after
WARM warm-up launches, median of 5 such windows; REPS is several hundred, so that a window lasts tens of milliseconds and not a
fraction of one.  A figure below ENQUEUE_US per launch is marked: back-to-back launches from Python cannot be issued much
faster than that, so such a figure may be the host's enqueue rate and not the kernel's run time (a kernel trace of its own
would tell).  Writes profiles/pix2pix_input_bench.txt."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_lib_tensorflow_amd import kernels as K  # noqa: E402

N, CROP, WARM, REPS = 16, 512, 20, 400
ENQUEUE_US = 20.0
FRAMES = {"512x1024": (512, 1024), "768x4080": (768, 4080)}
MODES = {"pair": 0, "multiple_A": 1, "lab": 2}
PANELS = {0: 2, 1: 3, 2: 1}


def event_ms(fn):
    for _ in range(WARM):
        fn()
    windows = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        windows.append(a.elapsed_time(b) / REPS)
    return sorted(windows)[2], min(windows), max(windows)


def mark(ms):
    return " [may be bound by the enqueue rate]" if ms * 1e3 < ENQUEUE_US else ""


def area_matrix(n_in, n_out):
    w = np.zeros((n_out, n_in), np.float32)
    for y in range(n_out):
        a, b = y * n_in, (y + 1) * n_in
        for i in range(a // n_out, -(-b // n_out)):
            w[y, i] = (min(b, (i + 1) * n_out) - max(a, i * n_out)) / n_in
    return w


def host_lab(x):
    f = np.float32
    rgb = np.where(x <= f(0.04045), x / f(12.92), ((x + f(0.055)) / f(1.055)) ** f(2.4))
    m = np.array([[0.412453, 0.212671, 0.019334], [0.357580, 0.715160, 0.119193], [0.180423, 0.072169, 0.950227]], f)
    xyz = (rgb @ m) * np.array([1 / 0.950456, 1.0, 1 / 1.088754], f)
    eps = 6 / 29
    t = np.where(xyz <= f(eps ** 3), xyz / f(3 * eps ** 2) + f(4 / 29), np.cbrt(xyz))
    return np.stack([(t[..., 1] * f(116) - f(16)) / f(50) - f(1), (t[..., 0] - t[..., 1]) * f(500) / f(110), (t[..., 1] - t[..., 2]) * f(200) / f(110)], axis=-1)


def host_batch(raw, mode, table):
    h, wraw = raw.shape[1:3]
    wp = wraw // PANELS[mode]
    wy, wx = area_matrix(h, CROP), area_matrix(wp, CROP)
    outs = []
    for img, (flip, _, _) in zip(raw, table):
        x = img.astype(np.float32) * np.float32(1 / 255.0)
        pans = [host_lab(x)] if mode == 2 else [x[:, k * wp:(k + 1) * wp] * 2 - 1 for k in range(PANELS[mode])]
        for p in pans:
            p = p[:, ::-1] if flip else p
            outs.append(np.einsum("xj,yjc->yxc", wx, np.tensordot(wy, p, axes=(1, 0)), optimize=True))
    return outs


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_pix2pix_input.py needs a GPU")
    lines = [f"Pix2Pix input pipeline, batch {N}, crop {CROP}, bf16 outputs; device: {torch.cuda.get_device_name(0)}; "
             f"event timing, {WARM} warm-up + 5 windows of {REPS} launches (median, min..max)"]
    rng = np.random.RandomState(0)
    for fname, (h, w) in FRAMES.items():
        for mname, mode in MODES.items():
            wraw = w - w % PANELS[mode]
            raw_np = rng.randint(0, 256, size=(N, h, wraw, 3)).astype(np.uint8)
            raw = torch.from_numpy(raw_np).cuda()
            table_np = np.stack([rng.randint(0, 2, size=N), np.zeros(N, int), np.zeros(N, int)], axis=1).astype(np.int32)
            table = torch.from_numpy(table_np).cuda()
            ca, cb = K.PIX_CHANNELS[mode]
            ins = torch.empty((N, CROP, CROP, ca), dtype=K.BF16, device="cuda")
            tgs = torch.empty((N, CROP, CROP, cb), dtype=K.BF16, device="cuda")
            med, lo, hi = event_ms(lambda: K.pix2pix_load_examples(raw, table, mode, 0, CROP, CROP, CROP, ins, tgs))
            nbytes = raw.numel() + 2 * (ins.numel() + tgs.numel())
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            cmed, _, _ = event_ms(lambda: dst.copy_(src))                    # nbytes / 2 read + nbytes / 2 written = nbytes moved
            t = time.perf_counter()
            host_batch(raw_np, mode, table_np)
            host_ms = (time.perf_counter() - t) * 1e3
            lines.append(f"{fname} {mname}: raw {N}x{h}x{wraw}x3 -> {ca}+{cb} channels: {med:.3f} ms ({lo:.3f}..{hi:.3f}); compulsory traffic "
                         f"{nbytes / 1e6:.1f} MB -> {nbytes / med / 1e6:.0f} GB/s{mark(med)}; device copy of the same bytes {cmed:.3f} ms{mark(cmed)} -> kernel at "
                         f"{cmed / med:.2f} of the copy rate; host NumPy float32 ({os.cpu_count()} CPUs visible, OMP_NUM_THREADS="
                         f"{os.environ.get('OMP_NUM_THREADS', 'unset')}) {host_ms:.0f} ms = {host_ms / med:.0f}x")
            print(lines[-1], flush=True)
    x = torch.empty((N, CROP, CROP, 3), dtype=K.BF16, device="cuda").uniform_(-1, 1)
    med, lo, hi = event_ms(lambda: K.pix2pix_convert_u8(x))
    nbytes = x.numel() * 3
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    cmed, _, _ = event_ms(lambda: dst.copy_(src))
    lines.append(f"convert_u8 {N}x{CROP}x{CROP}x3 bf16 -> uint8 (with its output allocation): {med:.4f} ms ({lo:.4f}..{hi:.4f}); {nbytes / 1e6:.1f} MB -> "
                 f"{nbytes / med / 1e6:.0f} GB/s{mark(med)}; device copy of the same bytes {cmed:.4f} ms{mark(cmed)} -> {cmed / med:.2f} of the copy rate")
    print(lines[-1], flush=True)
    out = os.path.join(ROOT, sys.argv[1] if len(sys.argv) > 1 else "profiles/pix2pix_input_bench.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
