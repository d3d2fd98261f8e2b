"""Times of one Lloyd iteration of NDB's k-means (common/ndb.py -> csrc/ndb.hip) at the metric's own size, 50 000 x 3072 float32
rows (CIFAR-10's training set in pixel space) and K = 100, on seeded synthetic pixel rows (100 centres + noise, rounded to
0..255): `K.ndb_assign` and `K.ndb_group_rows` + `K.ndb_centroids`, each between device events, 2 warm-up calls and 7 timed
ones, alternating with the yardstick in the tree for the same tile loop, gank_prd_counts_partial at (nq, nr, D) = (n, K, D) and
one segment.  FLOP are the executed ones of the distance matrix: 64 x 64 x D x 2 per tile that a workgroup walks (edge tiles
count whole: K_padded = 128).  Bytes of the centroid pass: the n x D x 4 of the rows, each read once.  Then `ndb.kmeans` end to
end under a host clock.

    python scratch/bench_ndb.py [--out profiles/ndb_bench.txt] [--n 50000] [--k 100] [--d 3072]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_lib_tensorflow_amd import _lib  # noqa: E402
from gan_lib_tensorflow_amd import kernels as K  # noqa: E402
from gan_lib_tensorflow_amd.common import ndb  # noqa: E402


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
    ap.add_argument("--n", type=int, default=50000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--d", type=int, default=3072)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    n, k, d = args.n, args.k, args.d
    g = torch.Generator().manual_seed(0)
    centres = torch.rand(k, d, generator=g) * 255.0
    member = torch.randint(0, k, (n,), generator=g)
    x = (centres[member] + 40.0 * torch.randn(n, d, generator=g)).round_().clamp_(0, 255).cuda()
    c = x[torch.from_numpy(ndb.draw_init(n, k, 0)).cuda()].contiguous()
    strips, tiles = (n + 63) // 64, (k + 63) // 64
    flop = strips * tiles * 64 * 64 * d * 2
    lines = [f"n = {n}, K = {k} ({tiles} tiles), D = {d}: {strips} workgroups per assignment"]

    def report(name, times, flop=None, nbytes=None):
        med = float(np.median(times))
        rate = f", executed {flop / 1e9:.1f} GFLOP -> {flop / med / 1e9:.1f} TFLOP/s" if flop else ""
        rate += f", {nbytes / 1e6:.0f} MB -> {nbytes / med / 1e9:.2f} TB/s" if nbytes else ""
        lines.append(f"{name}: ms {['%.3f' % t for t in times]} median {med:.3f} ms{rate}")
        print(lines[-1], flush=True)

    label, d2, part_inertia, part_changed = K.ndb_assign(x, c)
    prev = label.clone()
    radii2 = torch.ones(k, dtype=torch.float64, device="cuda")
    part_count = torch.empty(n, dtype=torch.int32, device="cuda")
    part_min = torch.empty(n, dtype=torch.float64, device="cuda")

    def assign():
        K.ndb_assign(x, c, prev=prev, label=label, d2=d2, part_inertia=part_inertia, part_changed=part_changed)

    def prd():
        _lib.check(K.lib().gank_prd_counts_partial(K._p(x), n, K._p(c), k, d, K._p(radii2), 1, K._p(part_count), K._p(part_min), K._stream()),
                   "prd_counts_partial")

    for round_ in range(2):                 # the two alternate: a drift of the clock shows in both
        report(f"ndb_assign, round {round_}", timed(assign, 2, 7), flop=flop)
        report(f"prd_counts_partial at the same (n, K, D), 1 segment, round {round_}", timed(prd, 2, 7), flop=flop)

    count, offset, perm = K.ndb_group_rows(label, k)
    ws = torch.empty(K.ndb_group_ws_elems(n, k), dtype=torch.int32, device="cuda")
    sizes = count.cpu().numpy()
    lines.append(f"cluster sizes after the first assignment: min {sizes.min()} median {int(np.median(sizes))} max {sizes.max()}")
    cnew = c.clone()
    report("ndb_group_rows (4 launches)", timed(lambda: K.ndb_group_rows(label, k, count=count, offset=offset, perm=perm, ws=ws), 2, 7))
    report("ndb_centroids", timed(lambda: K.ndb_centroids(x, perm, count, offset, cnew), 2, 7), nbytes=n * d * 4)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, _, inertia, iterations = ndb.kmeans(x, k, seed=0, max_iter=100)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    lines.append(f"ndb.kmeans: {iterations} iterations in {(t1 - t0) * 1e3:.1f} ms wall clock ({(t1 - t0) * 1e3 / iterations:.2f} ms an "
                 f"iteration, copies back included), inertia {inertia!r}")
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
