"""Inception score of 5000 SNGAN samples, both paths on the same trainer and the same random-weight InceptionV3: the host path
`inception_score(n, classifier=net.logits)` (samples to the host, quantised there, batches uploaded again, logits copied back,
float32 softmax and preds2score in NumPy) and the device path `inception_score(n, net=net)` (common/inception/inception_score.py
-> csrc/inception_score.hip).  The host path is untouched by the device path's arrival, so its time is the earlier state's.  Also
the Inception forward alone on the same 50 batches, to say what share of the device path lies outside it, and the statistics
stage alone.  Information only, not a gate.

    python scratch/bench_inception_score.py [--out profiles/inception_score_bench.txt]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from gan_lib_tensorflow_amd.common.inception import inception_score as IS  # noqa: E402
from gan_lib_tensorflow_amd.common.inception.inception_v3 import InceptionV3  # noqa: E402
from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import SNGANTrainer  # noqa: E402
from test_inception_gpu import random_params  # noqa: E402

N, REPS = 5000, 5


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def spread(ts):
    ts = sorted(ts)
    return f'median {ts[len(ts) // 2]:.1f} (min {ts[0]:.1f}, max {ts[-1]:.1f}; {len(ts)} runs)'


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'inception_score_bench.txt')
    torch.cuda.set_device(0)
    net = InceptionV3(random_params(7))
    tr = SNGANTrainer(batch_size=64, seed=0, use_graphs=False)
    lines = [f'Inception score of {N} SNGAN samples (50 generator passes of 100, 50 Inception batches of 100 at 299 x 299, 10 splits), '
             f'{torch.cuda.get_device_name(0)}; random-weight InceptionV3; wall clock around a device synchronise, ms; the two paths alternate']
    host = lambda: tr.inception_score(n=N, classifier=net.logits)      # noqa: E731
    dev = lambda: tr.inception_score(n=N, net=net)                     # noqa: E731
    wall(lambda: tr.inception_score(n=200, classifier=net.logits, splits=2))         # warm-up: every shape of the timed window
    wall(lambda: tr.inception_score(n=200, net=net, splits=2))
    th, td, last = [], [], None
    for _ in range(REPS):
        ms, hs = wall(host)
        th.append(ms)
        ms, ds = wall(dev)
        td.append(ms)
        last = (hs, ds)
    lines.append(f'host path   inception_score(n={N}, classifier=net.logits): {spread(th)}')
    lines.append(f'device path inception_score(n={N}, net=net):               {spread(td)}')
    lines.append(f'last scores (different draws, random weights): host {last[0][0]:.6f} +- {last[0][1]:.6f}, device {last[1][0]:.6f} +- {last[1][1]:.6f}')

    g = torch.Generator(device='cuda').manual_seed(0)
    images = (torch.rand(100, 32, 32, 3, generator=g, device='cuda') * 2 - 1)
    tf = [wall(lambda: [net.logits_device(images) for _ in range(N // 100)])[0] for _ in range(REPS)]
    lines.append(f'Inception forward alone, {N // 100} x logits_device([100, 32, 32, 3]): {spread(tf)}')
    med_d, med_f = sorted(td)[REPS // 2], sorted(tf)[REPS // 2]
    lines.append(f'device path outside the Inception forward (sampling, quantisation, statistics, finalize): {med_d - med_f:.1f} = '
                 f'{100 * (med_d - med_f) / med_d:.1f} % of the path')

    logits = net.logits_device(images)

    def stage():
        s = IS.InceptionScore(N, 10)
        for _ in range(N // 100):
            s.update(logits)
        return s
    stage()
    ts = [wall(stage)[0] for _ in range(REPS)]
    lines.append(f'statistics stage alone, {N // 100} x InceptionScore.update([100, 1008]) (two launches each): {spread(ts)}')
    s = stage()
    ms, _ = wall(s.finalize)
    lines.append(f'finalize (one copy back of {10 * 1001 * 8} bytes, NumPy float64): {ms:.2f}')
    hl = logits.cpu().numpy()
    t = time.perf_counter()
    for _ in range(N // 100):
        e = np.exp(hl[:, :1000])
        e / e.sum(axis=1, keepdims=True)
    lines.append(f'host, the float32 softmax of the same {N // 100} batches in NumPy (logits already on the host): {(time.perf_counter() - t) * 1e3:.1f}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
