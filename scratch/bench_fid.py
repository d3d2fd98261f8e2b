"""FID statistics stage (common/fid.py -> csrc/fid.hip), Inception excluded: the time of one FeatureMoments.update at (100, 2048)
and of the whole 50 000-sample stage (500 updates and finalize), beside the host time of the same sums as `X.T @ X` in NumPy
float64 on the same features.  Information only: there is no earlier GPU figure to compare with.

    python scratch/bench_fid.py [--out profiles/fid_bench.txt]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_lib_tensorflow_amd.common import fid as F  # noqa: E402

N, BATCH, DIM = 50000, 100, 2048


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
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'fid_bench.txt')
    g = torch.Generator(device='cuda').manual_seed(0)
    feats = torch.randn(N, DIM, generator=g, device='cuda') * 0.2 + 1.0          # float32, mean 1 and spread 0.2
    lines = [f'FID statistics stage, {torch.cuda.get_device_name(0)}; features float32 [{N}, {DIM}] in batches of {BATCH}; wall clock, ms']
    mom = F.FeatureMoments(DIM)
    batch = feats[:BATCH]
    for _ in range(5):
        mom.update(batch)
    med, lo, hi = wall(lambda: mom.update(batch), 50)
    rmw = DIM * (DIM + 16) / 2 * 8 * 2            # the upper tiles of gram read and written once
    lines.append(f'one update ({BATCH}, {DIM}): median {med:.4f} (min {lo:.4f}, max {hi:.4f}; 50 calls, each synchronised); '
                 f'gram read-modify-write {rmw / 1e6:.1f} MB -> {rmw / med / 1e6:.1f} GB/s')

    def stage():
        m = F.FeatureMoments(DIM)
        for i in range(0, N, BATCH):
            m.update(feats[i:i + BATCH])
        return m
    stage()
    med, lo, hi = wall(stage, 5)
    lines.append(f'moment stage of {N} samples ({N // BATCH} updates, one synchronisation): median {med:.2f} (min {lo:.2f}, max {hi:.2f}; 5 runs) '
                 f'= {med / (N // BATCH):.4f} per update')
    m = stage()
    torch.cuda.synchronize()
    t = time.perf_counter()
    mu, sigma = m.finalize()
    lines.append(f'finalize (one copy back of {(DIM + DIM * DIM) * 8 / 1e6:.1f} MB, mirror, covariance in float64 on the host): '
                 f'{(time.perf_counter() - t) * 1e3:.1f}')

    host = feats.cpu().numpy()
    hb = host[:BATCH].astype(np.float64)
    ts = []
    for _ in range(10):
        t = time.perf_counter()
        hb.T @ hb
        ts.append((time.perf_counter() - t) * 1e3)
    lines.append(f'host, NumPy float64 X.T @ X at ({BATCH}, {DIM}): median {sorted(ts)[5]:.3f} ({os.environ.get("OMP_NUM_THREADS", "all")} threads)')
    t = time.perf_counter()
    gram = np.zeros((DIM, DIM))
    total = np.zeros(DIM)
    for i in range(0, N, BATCH):
        xb = host[i:i + BATCH].astype(np.float64)
        gram += xb.T @ xb
        total += xb.sum(axis=0)
    host_ms = (time.perf_counter() - t) * 1e3
    lines.append(f'host, the same {N // BATCH} batches accumulated in NumPy float64 (features already on the host): {host_ms:.1f}')
    rsigma = (gram - np.outer(total, total) / N) / (N - 1)
    lines.append(f'device vs host covariance: largest difference {np.abs(sigma - rsigma).max():.3e} of largest entry {np.abs(rsigma).max():.3e}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
