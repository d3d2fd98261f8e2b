"""What the ACGAN, PGGAN and Pix2Pix trainers share: the store / process-group / RNG / GraphRunner set-up, the flat buffers and
their Adam state, and one update = forward-backward -> [all-reduce] -> Adam through `graphs.GraphRunner.update`.  A subclass
builds its model once between `__init__` and `_finish_build`, and supplies the losses, `_d_fwd_bwd` / `_g_fwd_bwd` and the steps.
(`SNGANTrainer` has its own capture protocol -- see graphs.py -- and stays apart.)"""
import contextlib

import torch

from . import functional as Fn
from . import kernels as K
from . import parallel
from .graphs import GraphRunner
from .store import ParamStore, adam_state, set_default_store


def polynomial_decay(step, lr0, decay_steps, lr_end):
    """tf.train.polynomial_decay(power=1, cycle=False)"""
    s = min(step, decay_steps)
    return (lr0 - lr_end) * (1.0 - s / float(decay_steps)) + lr_end


class GraphTrainer:
    def __init__(self, device, seed, process_group, use_graphs, allow_eager_fallback):
        self.device = torch.device(device)
        self.store = set_default_store(ParamStore(self.device, seed=seed))
        self.pg = process_group
        self.world, self.rank = parallel.world_and_rank(process_group)
        # data-side RNG differs per rank; parameter init (store seed) is identical on all ranks
        self.rng_state = K.new_rng_state(parallel.data_seed(seed, self.rank), self.device)
        self.losses = {}
        # the two updates as captured hipGraphs: they read static buffers and device-side scalars written outside the capture
        self.graphs = GraphRunner(use_graphs, allow_eager_fallback)     # a failed hipGraph capture raises unless the caller allows eager execution

    def _flatten_nets(self, state, g_prefix, d_prefix):
        if state is not None:
            self.store.load_state_dict(state)
        self.g_flat = self.store.flatten(g_prefix)
        self.d_flat = self.store.flatten(d_prefix)
        self.g_params = [self.store.vars[k] for k in self.g_flat['names']]
        self.d_params = [self.store.vars[k] for k in self.d_flat['names']]

    def _finish_build(self, state, g_adam, d_adam, g_prefix='g_net', d_prefix='d_net'):
        """after the build pass has created every variable: flat buffers, then Adam state from (lr, beta1, beta2)"""
        self._flatten_nets(state, g_prefix, d_prefix)
        self.g_opt = adam_state(self.g_flat, *g_adam, self.world)
        self.d_opt = adam_state(self.d_flat, *d_adam, self.world)

    def _apply(self, opt):
        f = opt['flat']
        K.adam_tf(f['params'], f['grads'], f['m'], f['v'], opt['hp'], opt['t'], None, zero_grads=True)

    def _learning_rate(self):
        """the learning rate of the coming update, or None to leave the optimisers' value alone"""
        return None

    def _update(self, key, fwd_bwd, opt):
        """the learning rate, written outside the captured region, then GraphRunner.update: fwd_bwd (graph) -> [RCCL
        all-reduce] -> Adam (graph)"""
        lr = self._learning_rate()
        if lr is not None:
            opt['hp'][0:1].fill_(lr)
        self.graphs.update(key, fwd_bwd, lambda: self._apply(opt), opt['flat']['grads'], self.pg, self.world)

    def _backward(self, loss):
        Fn.reset_deferred()
        try:
            loss.backward(gradient=Fn.unit_seed(loss))
            Fn.join_wgrad()
        finally:
            Fn.reset_deferred()

    @contextlib.contextmanager
    def critic_frozen(self):
        """the generator's loss differentiates w.r.t. the generator's variables only"""
        for p in self.d_params:
            p.requires_grad_(False)
        try:
            yield
        finally:
            for p in self.d_params:
                p.requires_grad_(True)
