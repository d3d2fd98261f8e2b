"""Wall clock of the per-sample scores pass (common/sample_scores.py -> csrc/prd.hip: `K.prd_sample_scores`) next to the counts
pass it mirrors (`K.prd_manifold_counts`) on the seeded random features of scratch/bench_prd.py, Inception excluded: 10 000 x
10 000 x 2048, each between device events (both launches of a pass), 2 warm-up calls and 5 timed ones, the two alternating over
two rounds; then `calculate_sample_scores` (one radii pass, two scores passes at prune = 0.5) and `calculate_prdc` (two radii
passes, two counts passes) end to end under a host clock.  FLOP are the executed ones of the distance matrix, as in bench_prd.py.

    python scratch/bench_sample_scores.py [--out profiles/sample_scores_bench.txt] [--n 10000]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_prd import timed  # noqa: E402
from gan_lib_tensorflow_amd import kernels as K  # noqa: E402
from gan_lib_tensorflow_amd.common import precision_recall, sample_scores  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=10000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n, d, k = args.n, 2048, 3
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(n, d, generator=g) * 0.5 + 0.3).cuda()
    y = (torch.randn(n, d, generator=g) * 0.5 + 0.35).cuda()
    tiles = (n + 63) // 64
    flop = tiles * tiles * 64 * 64 * d * 2
    lines = [f"n = {n} a side, D = {d}, k = {k}, default segments {K.prd_default_segments(n)}"]

    def report(name, times):
        med = float(np.median(times))
        lines.append(f"{name}: ms {['%.2f' % t for t in times]} median {med:.2f} ms, executed {flop / 1e12:.3f} TFLOP -> "
                     f"{flop / med / 1e9:.1f} TFLOP/s")
        print(lines[-1], flush=True)

    radii2 = K.prd_knn_radii(x, k)
    pruned2 = sample_scores.pruned_radii(radii2, 0.5)
    for round_ in (1, 2):
        report(f"counts pass, fake in real manifold, round {round_}", timed(lambda: K.prd_manifold_counts(y, x, radii2), 2, 5))
        report(f"scores pass, all balls, round {round_}", timed(lambda: K.prd_sample_scores(y, x, radii2), 2, 5))
        report(f"scores pass, prune = 0.5, round {round_}", timed(lambda: K.prd_sample_scores(y, x, pruned2), 2, 5))
    for name, fn in (("calculate_sample_scores", lambda: sample_scores.calculate_sample_scores(x, y, k=k)),
                     ("calculate_prdc", lambda: precision_recall.calculate_prdc(x, y, k=k))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = fn()
        t1 = time.perf_counter()
        got = {key: value for key, value in got.items() if isinstance(value, float)}
        lines.append(f"{name}({n} vs {n}): {(t1 - t0) * 1e3:.0f} ms wall clock end to end (copies back included), {got}")
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
