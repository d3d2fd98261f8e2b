"""hipGraph capture-and-replay of a train-step piece (torch.cuda.CUDAGraph = hipGraph on ROCm): the one place that creates and
captures graphs.

A GAN update at the reference's batch sizes is a few hundred kernel launches of 5-50 us; issued eagerly from Python they
cost ~100 us of host time each and the GPU idles between them (ACGAN at 32 samples per GPU: 69 ms per step eager).  Each
piece runs eagerly once (allocator warm-up, lazy initialisation; this IS the step), is captured and replayed from then on.
What a captured piece may depend on: device memory at fixed addresses only -- inputs are copied into static buffers, step
counters / learning rates / fade-in weights / RNG state live on the device and are updated OUTSIDE the captured region.

Three primitives -- `eager_on_side_stream`, `capture`, `capture_failed` -- and two protocols built on them:
  * `GraphRunner` (owned by `trainer.GraphTrainer`, the base of the ACGAN, PGGAN and Pix2Pix trainers, whose `_update` is its
    only caller): first call of a key eager, second call capture + one replay, later calls replay;
  * `SNGANTrainer` (SNGAN/gan_cifar_resnet.py): first call eager AND captured (nothing replayed), later calls replay; its
    updates may hold their collectives, and the ranks agree on that.
The two differ in which call consumes RNG state and advances Adam's step count, so they stay apart.
"""
import contextlib
import gc
import sys

import torch

from . import parallel


def eager_on_side_stream(fn):
    """fn() on a fresh side stream (so that lazily created state is not tied to a capture), joined and synchronised"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    return out


@contextlib.contextmanager
def capture(pool=None):
    """with capture() as g: ...launches...  -- g is the CUDAGraph that holds them (nothing is executed).  `pool`: a
    torch.cuda.graph_pool_handle() shared by graphs that read each other's tensors.
    The Python garbage collector is paused: a cyclic-GC pass in the middle of a capture can destroy an older trainer's
    CUDAGraph / return its pool memory while the stream is capturing, which aborts the process (torch only collects once, on
    entry).  The pause spans the whole `with torch.cuda.graph`, its exit included: the stream is still capturing inside
    capture_end, and a collector switched back on before it ran its pass right there.  No eager collective is left on the RCCL
    watchdog's list when the capture starts, and thread_local because that watchdog's thread polls events concurrently under data
    parallel."""
    g = torch.cuda.CUDAGraph()
    was = gc.isenabled()
    parallel.drain_collective_watchdog()
    gc.disable()                         # (torch's own gc.collect() on entry is an explicit call: it still runs)
    try:
        with torch.cuda.graph(g, pool=pool, capture_error_mode="thread_local"):
            yield g
    finally:
        if was:
            gc.enable()


def capture_failed(what, e, allow_eager_fallback):
    """The eager first execution already WAS this step, so nothing is lost either way: raise (default: a run that asked for
    graphs must not silently become a 10x slower eager run), or return after a message on stderr -- the caller then runs
    eagerly for the rest of the run."""
    torch.cuda.synchronize()
    if not allow_eager_fallback:
        raise RuntimeError(f"hipGraph capture of {what} failed ({e}); pass allow_eager_fallback=True (or use_graphs=False) "
                           f"to run eagerly") from e
    print(f"[gank] hipGraph capture of {what} failed ({e}); running eagerly", file=sys.stderr)


class GraphRunner:
    def __init__(self, enabled=True, allow_eager_fallback=False):
        self.enabled = enabled and torch.cuda.is_available()
        self.allow_eager_fallback = allow_eager_fallback
        self.graphs = {}
        self._seen = set()

    def run(self, key, fn):
        """fn(): enqueues kernels only (no host synchronisation, no host-dependent control flow that changes between calls)"""
        if not self.enabled:
            return fn()
        g = self.graphs.get(key)
        if g is not None:
            g.replay()
            return None
        if key not in self._seen:
            self._seen.add(key)
            return eager_on_side_stream(fn)
        try:
            with capture() as g:
                fn()
            self.graphs[key] = g
            g.replay()                   # capture executed nothing: this is the step
        except Exception as e:  # noqa: BLE001
            capture_failed(repr(key), e, self.allow_eager_fallback)
            self.enabled = False
            return fn()
        return None

    def update(self, key, fwd_bwd, apply, grads, pg, world):
        """fwd_bwd (graph) -> [RCCL all-reduce of `grads`] -> apply (graph): one graph when there is nothing to exchange"""
        if world == 1:
            self.run(key, lambda: (fwd_bwd(), apply()))
        else:
            self.run(key, fwd_bwd)
            parallel.allreduce_sum_(grads, pg)
            self.run(key + '/adam', apply)

    def clear(self):
        self.graphs.clear()
        self._seen.clear()
