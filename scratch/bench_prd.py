"""Wall clock of the precision / recall statistics stage (common/precision_recall.py -> csrc/prd.hip) on seeded random features,
Inception excluded: the two radii passes (`K.prd_knn_radii`, k = 3) and the two counts passes (`K.prd_manifold_counts`) at
10 000 x 10 000 x 2048, each between device events (both launches of a pass), 1 warm-up call and 3 timed ones; then
`calculate_prdc` end to end under a host clock.  FLOP are the executed ones of the distance matrix: 64 x 64 x D x 2 per tile that a
workgroup walks (edge tiles count whole; norms and selection are not counted).  For comparison the KID tile loop (the same
contraction, `K.kid_block_sums` at 100 subsets of 1000) is timed in the same process, as scratch/bench_kid.py times it.

    python scratch/bench_prd.py [--out profiles/prd_bench.txt] [--n 10000] [--segments S ...]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_lib_tensorflow_amd import kernels as K  # noqa: E402
from gan_lib_tensorflow_amd.common import kid, precision_recall  # noqa: E402


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--segments", type=int, nargs="*", default=[], help="further segment counts to time the real radii pass at")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n, d, k = args.n, 2048, 3
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(n, d, generator=g) * 0.5 + 0.3).cuda()
    y = (torch.randn(n, d, generator=g) * 0.5 + 0.35).cuda()
    tiles = (n + 63) // 64
    flop = tiles * tiles * 64 * 64 * d * 2
    lines = []

    def report(name, times, flop):
        med = float(np.median(times))
        lines.append(f"{name}: ms {['%.1f' % t for t in times]} median {med:.1f} ms, executed {flop / 1e12:.3f} TFLOP -> "
                     f"{flop / med / 1e9:.1f} TFLOP/s")
        print(lines[-1], flush=True)

    segments = K.prd_default_segments(n)
    lines.append(f"n = {n} a side, D = {d}, k = {k}, default segments {segments}: {tiles} x {segments} workgroups per pass")
    radii = {}
    for name, bank in (("real", x), ("fake", y)):
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        radii[name] = out
        report(f"radii pass, {name} bank", timed(lambda: K.prd_knn_radii(bank, k, out=out), 1, 3), flop)
    for name, q, bank, r in (("fake in real manifold", y, x, radii["real"]), ("real in fake manifold", x, y, radii["fake"])):
        report(f"counts pass, {name}", timed(lambda: K.prd_manifold_counts(q, bank, r), 1, 3), flop)
    for s in args.segments:
        report(f"radii pass, real bank, segments = {s}", timed(lambda: K.prd_knn_radii(x, k, segments=s), 1, 2), flop)
    t0 = time.perf_counter()
    got = precision_recall.calculate_prdc(x, y, k=k)
    t1 = time.perf_counter()
    lines.append(f"calculate_prdc({n} vs {n}): {(t1 - t0) * 1e3:.0f} ms wall clock end to end (four passes, copies back), {got}")
    print(lines[-1], flush=True)

    rng = np.random.RandomState(0)
    subsets, m = 100, min(1000, n)
    ix = torch.from_numpy(kid.draw_subsets(n, subsets, m, rng)).cuda()
    iy = torch.from_numpy(kid.draw_subsets(n, subsets, m, rng)).cuda()
    times = timed(lambda: K.kid_block_sums(x, y, ix, iy, 1 / d, 1.0, 3), 2, 7)
    report(f"for comparison, kid_block_sums subsets={subsets} m={m}", times, subsets * K.kid_num_tiles(m) * 64 * 64 * d * 2)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
