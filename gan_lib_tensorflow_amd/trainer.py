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


class SampleMetrics:
    """The evaluation metrics of a trainer's own samples, once for every trainer (a mixin: `SNGANTrainer` is no `GraphTrainer`).
    All of them sit over one hook of the trainer,

        _metric_batch(b, **kw) -> (uint8 images [b,H,W,3] on the device, int labels [b] or None)

    one generator pass of b samples on fresh draws from the trainer's device RNG, quantised as the training scripts quantise
    for the Inception score (`msssim.quantize_on_device`: `((x + 1) * (255.99 / 2))` truncated to uint8).  The hook is called
    until a metric has its rows and never once more (`fid.draw_until`): every call advances the RNG.  A pass has
    `_metric_rows()` samples, 100 unless the trainer says otherwise; the Inception score always draws 100, as the scripts do.
    Samples, features and logits never leave the device; no parameter, optimiser state or step counter moves.  `net` is an
    `InceptionV3` (the frozen graph's weights are a download): without one the metrics that need it raise NotImplementedError."""

    def _metric_batch(self, b, **kw):
        raise NotImplementedError(f"{type(self).__name__} supplies no _metric_batch")

    def _metric_rows(self):
        return 100

    def _metric_draw(self, b=None, **kw):
        """draw() of the sampling loops under common/: the images of one hook call of b rows (default `_metric_rows()`)"""
        b = self._metric_rows() if b is None else b
        return lambda: self._metric_batch(b, **kw)[0]

    @torch.no_grad()
    def msssim_diversity(self, n_pairs=500, weights=None):
        """Per-class sample diversity, the mode-collapse measure of the ACGAN paper: MS-SSIM (common/msssim.py) between pairs of
        same-class samples.  Passes are drawn until every class has 2 * n_pairs samples; consecutive same-class samples are
        paired.  -> ({class: batch MultiScaleSSIM of its n_pairs pairs}, mean over classes).  Low = diverse.  A trainer whose
        samples carry no labels raises TypeError."""
        from .common.msssim import class_pair_diversity

        def draw():
            images, labels = self._metric_batch(self._metric_rows())
            if labels is None:
                raise TypeError(f"{type(self).__name__}.msssim_diversity: the score pairs samples of one class, and this trainer's "
                                "samples carry no labels")
            return images, labels
        return class_pair_diversity(draw, n_pairs, 10, weights)

    @torch.no_grad()
    def fid(self, real, n=50000, net=None):
        """Frechet Inception Distance (common/fid.py) between n samples and `real`: a FeatureMoments, a (mu, sigma) pair, the
        path of an .npz with `mu` and `sigma`, or images [N,H,W,3].  The samples are mapped back to [-1, 1] and fed to
        `net.features_f32`."""
        from .common.fid import calculate_fid, sample_moments
        return calculate_fid(sample_moments(self._metric_draw(), n, net), real, net)

    @torch.no_grad()
    def kid(self, real, n=50000, net=None, subsets=100, subset_size=1000, seed=0):
        """Kernel Inception Distance (common/kid.py: the unbiased polynomial-kernel MMD^2 of the pool_3 features) between n
        samples and `real`: a FeatureBank, features [N, 2048] or images [N,H,W,3] -> (mean, std) over `subsets` subsets of
        `subset_size` rows a side."""
        from .common.kid import calculate_kid, sample_features
        return calculate_kid(sample_features(self._metric_draw(), n, net), real, net, subsets=subsets, subset_size=subset_size, seed=seed)

    @torch.no_grad()
    def precision_recall(self, real, n=10000, net=None, k=3):
        """Precision, recall, density and coverage (common/precision_recall.py: k-NN manifolds of the pool_3 features) of n
        samples against `real`: a FeatureBank, features [N, 2048] or images [N,H,W,3] -> dict(precision, recall, density,
        coverage).  The default n is 10 000, not 50 000: in float64 a distance matrix costs 2 n^2 D FLOP per pass and there are
        four passes, 0.41 TFLOP a pass at 10 000 and 10 TFLOP at 50 000 (25 times the time and, for the n samples, five times the
        Inception forwards)."""
        from .common.kid import sample_features
        from .common.precision_recall import calculate_prdc
        return calculate_prdc(real, sample_features(self._metric_draw(), n, net), net, k)

    @torch.no_grad()
    def sample_scores(self, real, n=10000, net=None, k=3, prune=0.5):
        """Per-sample realism and rarity scores (common/sample_scores.py: which samples lie deep in the k-NN manifold of the real
        pool_3 features, and which in its sparse regions) of n samples against `real`, drawn and batched as for
        `precision_recall` -> the dict of `calculate_sample_scores` (realism, rarity, inside [n] and their summary scalars)
        plus `samples`: the n drawn images, uint8 [n,H,W,3] on the device, row i the sample of score i -- index them with
        `sample_scores.rank_samples` for a sheet of the best and the worst."""
        from .common.kid import sample_features
        from .common.sample_scores import calculate_sample_scores
        draw, drawn = self._metric_draw(), []

        def keep():
            drawn.append(draw())
            return drawn[-1]
        out = calculate_sample_scores(real, sample_features(keep, n, net), net, k, prune)
        out['samples'] = torch.cat(drawn)[:n]           # the last pass is cut to the rows that were scored
        return out

    @torch.no_grad()
    def swd(self, real, n=8192, seed=0, **kw):
        """Sliced Wasserstein distance on Laplacian-pyramid patches (common/swd.py; Karras et al. 2018, section 5: no network,
        no downloaded weights) between n samples and the first n images of `real` [N >= n,H,W,3] at the samples' size (uint8 or
        float32, NumPy or device tensor) -> (float64 [levels], their mean), x 1000.  A `real` that is too short or too small for
        a patch raises before anything is drawn.  **kw: nhood_size, nhoods_per_image, dir_repeats, dirs_per_repeat."""
        from .common.swd import sample_swd
        return sample_swd(self._metric_draw(), real, n, seed, **kw)

    @torch.no_grad()
    def ndb(self, real, n=10000, **kw):
        """NDB and JSD (common/ndb.py; Richardson & Weiss 2018, section 2: k-means bins of the training images in pixel space, no
        network, no downloaded weights) of n samples against `real`: an `NDB` (the bins of a training set, fitted once) or
        training images uint8 [N,H,W,3] at the samples' size, fitted here -> dict(ndb, ndb_over_k, js, bin_proportions_train,
        bin_proportions_samples, different_bins).  **kw: number_of_bins, significance_level, max_dims, seed, max_iter of `NDB`
        when `real` is images."""
        from .common.ndb import NDB, sample_ndb
        if isinstance(real, NDB):
            if kw:
                raise TypeError(f"{type(self).__name__}.ndb: {sorted(kw)} belong to the fit, and `real` is fitted already")
        else:
            real = NDB(real, **kw)
        return sample_ndb(self._metric_draw(), real, n)

    @torch.no_grad()
    def inception_score(self, n=50000, net=None, splits=10, batch_size=100):
        """get_inception_score(n) of the training scripts, on the device throughout (common/inception/inception_score.py):
        n / 100 passes of 100 samples, mapped back to [-1, 1], `net.logits_device` in batches of `batch_size`, the float64
        statistics in `splits` splits; only their final state comes back.  -> (mean, std)"""
        from .common.inception.inception_score import sample_inception_score
        return sample_inception_score(self._metric_draw(100), int(n / 100), 100, net, splits, batch_size)


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
