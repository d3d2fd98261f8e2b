"""The projection discriminator beside the concat critic on one GPU, interleaved in one process: the captured critic update
(graph replay of `d_pre`), the whole training iteration at batch 64 (1 generator + 5 critic updates, bench.py's unit), and the
head launch gank_proj_head_hinge_scaled alone beside gank_critic_head_hinge_scaled at the critic's shape (128 x 128, 10 labels),
as back-to-back launches of one graph.  Information only: bench.py and its headline measure the default (concat) mode.

    python scratch/bench_projection.py [--out profiles/projection_bench.txt] [--rounds 7]
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gan_lib_tensorflow_amd import kernels as K  # noqa: E402
from gan_lib_tensorflow_amd.SNGAN import gan_cifar_resnet as S  # noqa: E402

BATCH, ITERS, UPDATES, HEADS = 64, 20, 100, 200


def timed(fn, n):
    """n calls between two synchronisations -> time per call, seconds"""
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def graph_of(fn, n):
    """n back-to-back launches of fn as one hipGraph (what a launch costs inside a captured update, not the host's enqueue)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    return g


def stat(xs, scale, unit):
    xs = sorted(x * scale for x in xs)
    return f'median {xs[len(xs) // 2]:.1f} {unit} (min {xs[0]:.1f}, max {xs[-1]:.1f}; {len(xs)} rounds)'


def main():
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'projection_bench.txt')
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 7
    trainers, feeds = {}, {}
    for name, proj in (('concat', False), ('projection', True)):
        trainers[name] = S.SNGANTrainer(batch_size=BATCH, seed=0, use_graphs=True, projection=proj)
        feeds[name] = S.synthetic_batches(BATCH, 'cuda', seed=1)
        for _ in range(4):                       # eager first pass, capture, replays: every graph of the iteration exists and is warm
            trainers[name].train_iteration(feeds[name])
        assert trainers[name].use_graphs and 'd_pre' in trainers[name]._graphs and 'g' in trainers[name]._graphs
    g = torch.Generator(device='cuda').manual_seed(0)
    M, Kd, V = 2 * BATCH, 128, 10
    x = torch.randn(M, Kd, generator=g, device='cuda').to(K.BF16)
    w, b, E = torch.randn(Kd, generator=g, device='cuda') * 0.1, torch.zeros(1, device='cuda'), torch.randn(V, Kd, generator=g, device='cuda') * 0.1
    labels = torch.randint(0, V, (M,), generator=g, device='cuda', dtype=torch.int32)
    gw, gb, gE, loss = torch.zeros(Kd, device='cuda'), torch.zeros(1, device='cuda'), torch.zeros(V, Kd, device='cuda'), torch.zeros(1, device='cuda')
    heads = {'projection': lambda: K.proj_head_hinge(x, w, b, E, labels, BATCH, 0, True, gw, gb, gE, loss),
             'concat': lambda: K.critic_head_hinge(x, w, b, BATCH, 0, True, gw, gb, loss)}
    head_graphs = {name: graph_of(fn, HEADS) for name, fn in heads.items()}
    for hg in head_graphs.values():
        timed(hg.replay, 3)
    res = {(what, name): [] for what in ('iteration', 'update', 'head') for name in trainers}
    for _ in range(rounds):
        for name, tr in trainers.items():
            res['iteration', name].append(timed(lambda: tr.train_iteration(feeds[name]), ITERS))
            update = lambda: tr._run('d_pre', tr._d_forward_backward_prefetched, tr.d_opt, tr.d_flat)  # noqa: E731  (replay: the ring of the last iteration)
            res['update', name].append(timed(update, UPDATES))
            res['head', name].append(timed(head_graphs[name].replay, 5) / HEADS)
    lines = [f'projection discriminator beside the concat critic, {torch.cuda.get_device_name(0)}; batch {BATCH}, hipGraph replay, {rounds} interleaved rounds; '
             f'wall clock between two synchronisations']
    for name, tr in trainers.items():
        lines.append(f'{name}: critic parameters {tr.store.param_count("Discriminator")}')
        lines.append(f'  captured critic update ({UPDATES} replays per round): ' + stat(res['update', name], 1e6, 'us'))
        lines.append(f'  whole iteration, 1 G + {S.N_CRITIC} D updates ({ITERS} per round): ' + stat(res['iteration', name], 1e3, 'ms'))
        lines.append(f'  head launch alone, {M} x {Kd} (a graph of {HEADS} back-to-back launches, 5 replays per round): ' + stat(res['head', name], 1e6, 'us'))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
