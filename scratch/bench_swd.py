"""Wall clock of the sliced Wasserstein distance (common/swd.py -> csrc/swd.hip) at the CIFAR protocol on seeded random uint8
images: n = 8192 images of 32 x 32 x 3, 128 patches per image (M = 1 048 576 per side and level), 4 x 128 directions.  Every kernel
between device events, 1 warm-up call and 3 timed ones, on the finest level; then `calculate_swd` end to end under a host clock.
The sort's bytes are its own traffic model (csrc/swd.hip: 8 passes x (two reads + one write) x 8 bytes = 192 bytes a key, the
histograms left out).  As a yardstick for the sort only, `torch.sort` on the same key buffer is timed in the same process,
interleaved call by call with ours; the ratio is reported, not gated.

    python scratch/bench_swd.py [--out profiles/swd_bench.txt] [--n 8192]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_lib_tensorflow_amd import kernels as K  # noqa: E402
from gan_lib_tensorflow_amd.common import swd  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def timed(fn, warmup=1, reps=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return [event_ms(fn) for _ in range(reps)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=8192)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n, size, c, nhood, per, repeats, ndirs = args.n, 32, 3, 7, 128, 4, 128
    rng = np.random.RandomState(0)
    a = torch.from_numpy(rng.randint(0, 256, size=(n, size, size, c)).astype(np.uint8)).cuda()
    b = torch.from_numpy(rng.randint(0, 200, size=(n, size, size, c)).astype(np.uint8)).cuda()
    m = n * per
    lines = [f"n = {n} images of {size} x {size} x {c}, {per} patches per image: M = {m} per side and level, {repeats} x {ndirs} directions"]

    def report(name, times, note=""):
        med = float(np.median(times))
        lines.append(f"{name}: ms {['%.2f' % t for t in times]} median {med:.2f} ms{note(med) if callable(note) else note}")
        print(lines[-1], flush=True)
        return med

    x64 = a.to(torch.float64)
    coarse = torch.empty((n, size // 2, size // 2, c), dtype=torch.float64, device="cuda")
    report("swd_pyr_down 32 -> 16", timed(lambda: K.swd_pyr_down(x64, out=coarse)))
    fine = x64.clone()
    report("swd_laplacian at 32", timed(lambda: K.swd_laplacian(fine, coarse)))
    level = swd.laplacian_pyramid(a)[0]
    dirs, centres, _ = swd.draw_tables(n, size, size, c, nhood, per, repeats, ndirs, seed=0)
    cx, cy = (torch.from_numpy(t).cuda() for t in centres[0])      # device tables: the host check is not part of a kernel's time
    cxh, cyh = centres[0]
    K.swd_patch_stats(level, cxh, cyh, nhood, per)                  # the host check, once
    report("swd_patch_stats (one of the two calls)", timed(lambda: K.swd_patch_stats(level, cx, cy, nhood, per)))
    mean, std = swd.patch_mean_std(level, cxh, cyh, nhood, per)
    d0 = torch.from_numpy(np.ascontiguousarray(dirs[0])).cuda()
    keys = torch.empty((ndirs, m), dtype=torch.float64, device="cuda")
    flop = 2.0 * m * ndirs * c * nhood * nhood
    report("swd_project, one repeat", timed(lambda: K.swd_project(level, cx, cy, nhood, per, mean, std, d0, out=keys)),
           lambda med: f", {flop / 1e9:.1f} GFLOP -> {flop / med / 1e9:.2f} TFLOP/s")
    unsorted = keys.clone()
    work, tmp = torch.empty_like(keys), torch.empty_like(keys)
    hist = torch.empty(K.swd_sort_ws_elems(ndirs, m), dtype=torch.int32, device="cuda")
    ours, theirs = [], []
    for i in range(4):                                              # interleaved; the first round is the warm-up
        work.copy_(unsorted)
        t = event_ms(lambda: K.swd_sort_rows(work, tmp=tmp, hist=hist))
        u = event_ms(lambda: torch.sort(unsorted, dim=1))
        if i:
            ours.append(t)
            theirs.append(u)
    assert torch.equal(work, torch.sort(unsorted, dim=1).values)
    traffic = 192.0 * ndirs * m
    ours_med = report(f"swd_sort_rows, {ndirs} rows of {m} keys", ours,
                      lambda med: f", model traffic {traffic / 1e9:.1f} GB -> {traffic / med / 1e9:.2f} TB/s")
    theirs_med = report("torch.sort on the same keys (yardstick)", theirs)
    lines.append(f"swd_sort_rows / torch.sort = {ours_med / theirs_med:.2f}")
    print(lines[-1], flush=True)
    other = torch.sort(unsorted.flip(1), dim=1).values
    part = torch.empty((ndirs, K.swd_sorted_l1_parts(m)), dtype=torch.float64, device="cuda")
    report("swd_sorted_l1", timed(lambda: K.swd_sorted_l1(work, other, part=part)),
           lambda med: f", {16.0 * ndirs * m / med / 1e9:.2f} TB/s")
    swd.calculate_swd(a[:256], b[:256], nhoods_per_image=per, dir_repeats=1, dirs_per_repeat=ndirs)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    values, mean_value = swd.calculate_swd(a, b, nhood_size=nhood, nhoods_per_image=per, dir_repeats=repeats, dirs_per_repeat=ndirs)
    t1 = time.perf_counter()
    lines.append(f"calculate_swd({n} vs {n}): {(t1 - t0) * 1e3:.0f} ms wall clock end to end (2 levels x 2 sides x {repeats} repeats, host draws "
                 f"and checks, copies back), levels {values.tolist()} mean {mean_value}")
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
