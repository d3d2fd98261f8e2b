"""Host side of the sampling / Inception-score harness: the statistics of
common/inception/inception_score.py:59-90 and the quantisation of SNGAN/gan_cifar_resnet.py:536-551.

The classifier itself (tfgan's frozen Inception graph, inception_score.py:29-47) needs downloaded weights, which this
environment does not have: `get_inception_score` takes it as a callable instead of building it.

The score on the device.  `get_inception_score` moves every batch to the host and back and keeps all n x 1000 probabilities
there.  The score does not need them: for one split of n_s rows, with lse_x = logsumexp(l_x) and p_xy = exp(l_xy - lse_x),

    mean_x KL(p_x || m) = (1/n_s) sum_x sum_y p_xy (l_xy - lse_x)  -  sum_y m_y log m_y,      m_y = (1/n_s) sum_x p_xy,

so 1000 float64 class sums and one float64 scalar per split are the whole running state.  `InceptionScore` keeps them on the
device (gank_inception_score_update, csrc/inception_score.hip: float64 from the float32 logits, no atomics, every element
summed in global row order so that the batching never changes a bit), `InceptionV3.logits_device` feeds it, and only the
[splits, 1001] state comes back, once, to be finished in NumPy float64 -- as `frechet_distance` finishes the FID.
sum p (l - lse) is the log-softmax form of the reference's sum p log p: the same number wherever the reference's is finite, and
finite where a probability underflows to 0 (0 * -inf = nan there) or a logit passes 88.7 (float32 exp overflows there)."""
import numpy as np

N_CLASSES = 1000          # of the frozen graph's 1008 logits the reference keeps the first 1000 (inception_score.py:55)


def quantize_samples(samples, for_score=False):
    """Generator output in [-1, 1] -> int32 pixel values, as the reference does it on the host:
    `(x + 1) * (255 / 2)` for the sample grid (:538) and `(x + 1) * (255.99 / 2)` for the score (:551);
    `.astype('int32')` truncates toward zero."""
    s = np.asarray(samples, dtype=np.float32)
    return ((s + 1.) * ((255.99 if for_score else 255.) / 2)).astype('int32')


def preds2score(preds, splits):
    """exp(mean_x KL(p(y|x) || p(y))) per split of the class-probability rows, then (mean, std) over the splits
    (inception_score.py:59-66)."""
    preds = np.asarray(preds)
    n = preds.shape[0]
    scores = []
    for i in range(splits):
        part = preds[(i * n // splits):((i + 1) * n // splits), :]
        marginal = part.mean(axis=0, keepdims=True)
        kl = (part * (np.log(part) - np.log(marginal))).sum(axis=1).mean()
        scores.append(np.exp(kl))
    return np.mean(scores), np.std(scores)


def get_inception_score(images, splits=10, classifier=None, batch_size=64):
    """images: [N,H,W,3], either pixel values (max > 1.01: mapped to [-1,1] as :72-73) or already in [-1,1].
    `classifier(batch[-1,1] NHWC float32) -> logits [b, >=1000]` stands in for the Inception graph of :29-47;
    whole batches only, first 1000 logits, softmax, `preds2score` (:49-56, :86)."""
    images = np.asarray(images)
    if np.max(images[0]) > 1.01:
        images = 2 * (images / 255. - 0.5)
    assert images.ndim == 4 and images.shape[3] == 3, images.shape          # [batch, height, width, channel]
    assert np.max(images[0]) <= 1 and np.min(images[0]) >= -1
    if classifier is None:
        raise NotImplementedError('the Inception classifier needs downloaded weights (inception_score.py:29-47): pass '
                                  'classifier=callable returning logits')
    preds = []
    for i in range(len(images) // batch_size):
        logits = np.asarray(classifier(images[i * batch_size:(i + 1) * batch_size].astype(np.float32)))[:, :1000]
        e = np.exp(logits)
        preds.append(e / e.sum(axis=1, keepdims=True))
    return preds2score(np.concatenate(preds, 0), splits)


def split_bounds(n, splits):
    """[b_0 .. b_splits]: split i of n rows is rows b_i .. b_{i+1} - 1, the slices of `preds2score` (uneven ones included)"""
    return [i * n // splits for i in range(splits + 1)]


def state_scores(state, n):
    """state float64 [splits, 1001] (per split: the 1000 class-probability sums, then sum_x sum_y p (l - lse)) of n rows
    -> float64 [splits], exp(state[j, 1000] / n_j - sum_y m_y log m_y) with m_y = state[j, y] / n_j; m_y == 0 contributes 0"""
    state = np.asarray(state, np.float64)
    bounds = split_bounds(n, state.shape[0])
    scores = np.empty(state.shape[0], np.float64)
    for j in range(state.shape[0]):
        n_j = bounds[j + 1] - bounds[j]
        m = state[j, :N_CLASSES] / n_j
        pos = m > 0
        scores[j] = np.exp(state[j, N_CLASSES] / n_j - np.sum(m[pos] * np.log(m[pos])))
    return scores


class InceptionScore:
    """The running statistics of the Inception score of exactly n rows in `splits` splits: `state` float64 [splits, 1001] on the
    device (allocated by the first `update`), `count` the rows fed so far.  Rows are taken in the order they arrive: row i of
    the stream is row i of `preds2score`."""

    def __init__(self, n, splits=10, device='cuda'):
        n, splits = int(n), int(splits)
        if splits < 1 or splits > n:
            raise ValueError(f"InceptionScore: splits = {splits} for n = {n} rows, needs 1 <= splits <= n (an empty split has no score)")
        self.n, self.splits, self.count, self.device = n, splits, 0, device
        self.state = self._scratch = self._scores = None

    def update(self, logits):
        """logits: device float32 [b, >= 1000] (the first 1000 columns count; [b, 1008] is taken as it is, not copied)"""
        from ... import kernels as K
        if logits.dim() != 2 or logits.shape[1] < N_CLASSES:
            raise RuntimeError(f"InceptionScore.update: logits {tuple(logits.shape)}, expected [b, >= {N_CLASSES}]")
        b = logits.shape[0]
        if self.count + b > self.n:
            raise RuntimeError(f"InceptionScore.update: {self.count} + {b} rows, more than the n = {self.n} this score was set up for")
        if b:
            import torch
            if self.state is None:
                self.state = torch.zeros((self.splits, N_CLASSES + 1), dtype=torch.float64, device=self.device)
            if self._scratch is None or self._scratch.shape[0] < b:
                self._scratch = torch.empty((b, 2), dtype=torch.float64, device=self.device)
            K.inception_score_update(logits, self.count, self.n, self.splits, self.state, self._scratch)
            self.count += b
            self._scores = None
        return self

    def scores(self):
        """-> float64 [splits], the per-split exp(mean KL); one copy back of the state, the rest in float64 on the host"""
        if self.count < self.n:
            raise RuntimeError(f"InceptionScore: {self.count} of n = {self.n} rows fed; the split bounds are those of n rows")
        if self._scores is None:
            self._scores = state_scores(self.state.cpu().numpy(), self.n)
        return self._scores

    def finalize(self):
        """-> (mean, std) over the splits, as `preds2score` returns them"""
        s = self.scores()
        return np.mean(s), np.std(s)


def get_inception_score_device(images, net, splits=10, batch_size=100):
    """`get_inception_score` with the classifier's logits, the softmax and the statistics kept on the device: images [N,H,W,3],
    a device tensor or a NumPy array, either pixel values (max of the first image > 1.01: mapped to [-1, 1] as :72-73) or
    already in [-1, 1]; whole batches only (N // batch_size * batch_size rows); `net.logits_device` -> `InceptionScore`.
    net: an `InceptionV3`.  Only the final [splits, 1001] state leaves the device.  -> (mean, std)"""
    from ..fid import _NO_WEIGHTS, _unit_range
    if net is None:
        raise NotImplementedError(_NO_WEIGHTS)
    assert images.ndim == 4 and images.shape[3] == 3, tuple(images.shape)          # [batch, height, width, channel]
    first = images[0]
    pixels = float(first.max()) > 1.01
    if not pixels:
        assert float(first.max()) <= 1 and float(first.min()) >= -1
    batches = len(images) // batch_size
    score = InceptionScore(batches * batch_size, splits, net.device)
    for i in range(batches):
        batch = images[i * batch_size:(i + 1) * batch_size]
        score.update(net.logits_device(_unit_range(batch) if pixels else batch))
    return score.finalize()


def sample_inception_score(draw, calls, per_call, net, splits=10, batch_size=100):
    """The score of generated samples, on the device: draw() -> uint8 images [per_call,H,W,3] on the device, quantised as the
    training scripts quantise them (msssim.quantize_on_device), called `calls` times; the rows are mapped back to [-1, 1] as
    `get_inception_score` maps pixel values and scored in whole batches of `batch_size` in the order they were drawn (rows
    past the last whole batch are dropped, as there).  Samples, logits and probabilities stay on the device.  -> (mean, std)"""
    import torch
    from ..fid import _NO_WEIGHTS, _unit_range
    if net is None:
        raise NotImplementedError(_NO_WEIGHTS)
    score = InceptionScore(calls * per_call // batch_size * batch_size, splits, net.device)
    held = None
    for _ in range(calls):
        rows = draw()
        assert rows.shape[0] == per_call, tuple(rows.shape)
        held = rows if held is None or not held.shape[0] else torch.cat([held, rows], 0)
        while held.shape[0] >= batch_size:
            score.update(net.logits_device(_unit_range(held[:batch_size])))
            held = held[batch_size:]
    return score.finalize()
