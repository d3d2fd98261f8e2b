"""MS-SSIM on the GPU (common/msssim.py -> csrc/msssim.hip): ms per MultiScaleSSIM call and achieved GB/s against the compulsory
traffic (both inputs read once per level + the pooled pair written once) for
  - 25 000 pairs of 32x32x3 uint8 (one Inception-score-sized sample set, paired), and
  - 64 pairs of 512x512x3 uint8,
plus the time SNGANTrainer.sample needs for the 50 000 images behind the first one.  `--once NAME` runs one warm-up and one call of
a single workload, for `rocprofv3 --kernel-trace --stats -- python scratch/bench_msssim.py --once small|large` (one kernel per level)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gan_lib_tensorflow_amd.common import msssim as M  # noqa: E402

WORKLOADS = {'small': (25000, 32, 32, 3), 'large': (64, 512, 512, 3)}


def make(n, h, w, c):
    g = torch.Generator(device='cuda').manual_seed(0)
    a = torch.randint(0, 256, (n, h, w, c), generator=g, dtype=torch.uint8, device='cuda')
    noise = torch.randint(-20, 21, (n, h, w, c), generator=g, dtype=torch.int16, device='cuda')
    return a, (a.to(torch.int16) + noise).clamp_(0, 255).to(torch.uint8)


def traffic_bytes(n, h, w, c, levels=5):
    total = 0
    for lvl in range(levels):
        total += 2 * n * h * w * c * (1 if lvl == 0 else 4)
        h, w = (h + 1) // 2, (w + 1) // 2
        if lvl + 1 < levels:
            total += 2 * n * h * w * c * 4
    return total


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    if '--once' in sys.argv:
        a, b = make(*WORKLOADS[sys.argv[sys.argv.index('--once') + 1]])
        for _ in range(2):
            score = M.MultiScaleSSIM(a, b)
        print('score', score)
        return
    for name, shape in WORKLOADS.items():
        a, b = make(*shape)
        for _ in range(3):
            score = M.MultiScaleSSIM(a, b)
        med, lo, hi = wall(lambda: M.MultiScaleSSIM(a, b), 20)
        gb = traffic_bytes(*shape) / 1e9
        print(f'{name}: {shape[0]} pairs {shape[1]}x{shape[2]}x{shape[3]} uint8: {med:.3f} ms per call (min {lo:.3f}, max {hi:.3f}; 20 calls, wall clock '
              f'with the copy of the partial sums back and the float64 combine), compulsory traffic {gb * 1e3:.1f} MB -> {gb / med * 1e3:.1f} GB/s, '
              f'score {score:.6f}')
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer
    tr = SNGANTrainer(batch_size=64, seed=0, use_graphs=False)
    for _ in range(5):
        tr.sample(100)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(500):
        tr.sample(100)
    torch.cuda.synchronize()
    print(f'SNGANTrainer.sample(100) x 500 = 50 000 images: {(time.perf_counter() - t) * 1e3:.1f} ms')
    t = time.perf_counter()
    scores, mean = tr.msssim_diversity(n_pairs=500)
    print(f'SNGANTrainer.msssim_diversity(n_pairs=500) (10 000 samples drawn and sorted by class, 10 calls of 500 pairs): '
          f'{(time.perf_counter() - t) * 1e3:.1f} ms, mean score {mean:.4f}')


if __name__ == '__main__':
    main()
