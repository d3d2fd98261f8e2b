"""Wall clock of the KID statistics stage (common/kid.py -> csrc/kid.hip) on seeded random features, Inception excluded:
`K.kid_block_sums` (both launches) between device events at the standard protocol -- 100 subsets of 1000 + 1000 rows out of
10 000, D = 2048 -- and at two smaller problems, 2 warm-up calls and 7 timed ones each; then one `kernel_distance` end to end
under a host clock (tables drawn and uploaded, kernels, copy back).  FLOP are the executed ones: 64 x 64 x D x 2 per tile that
has a workgroup (the symmetric blocks' lower tiles have none; edge tiles count whole).

    python scratch/bench_kid.py [--out profiles/kid_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_lib_tensorflow_amd import kernels as K  # noqa: E402
from gan_lib_tensorflow_amd.common import kid  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(10000, 2048, generator=g) * 0.5 + 0.3).cuda()
    y = (torch.randn(10000, 2048, generator=g) * 0.5 + 0.3).cuda()
    rng = np.random.RandomState(0)
    lines = []
    for subsets, m in ((100, 1000), (10, 1000), (100, 500)):
        ix = torch.from_numpy(kid.draw_subsets(10000, subsets, m, rng)).cuda()
        iy = torch.from_numpy(kid.draw_subsets(10000, subsets, m, rng)).cuda()
        partial = torch.empty(subsets * K.kid_num_tiles(m), dtype=torch.float64, device="cuda")
        res = torch.empty(subsets, 3, dtype=torch.float64, device="cuda")
        for _ in range(2):
            K.kid_block_sums(x, y, ix, iy, 1 / 2048, 1.0, 3, partial=partial, out=res)
        torch.cuda.synchronize()
        times = []
        for _ in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            K.kid_block_sums(x, y, ix, iy, 1 / 2048, 1.0, 3, partial=partial, out=res)
            b.record()
            torch.cuda.synchronize()
            times.append(a.elapsed_time(b))
        flop = subsets * K.kid_num_tiles(m) * 64 * 64 * 2048 * 2
        med = float(np.median(times))
        lines.append(f"subsets={subsets} m={m}: ms {['%.2f' % t for t in times]} median {med:.2f} ms, "
                     f"executed {flop / 1e12:.3f} TFLOP -> {flop / med / 1e9:.1f} TFLOP/s")
        print(lines[-1], flush=True)
    t0 = time.perf_counter()
    mean, std = kid.kernel_distance(x, y)
    t1 = time.perf_counter()
    lines.append(f"kernel_distance(10000 vs 10000, 100 x 1000): {(t1 - t0) * 1e3:.1f} ms wall clock end to end "
                 f"(tables, upload, kernels, copy back), mean {mean!r} std {std!r}")
    print(lines[-1])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
