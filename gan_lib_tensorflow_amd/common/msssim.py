"""MS-SSIM on the GPU: the reference's common/msssim.py (NumPy / SciPy, from the TensorFlow models tree; listed as an evaluation
TODO in its README and never called) with the same names, signatures and numbers.

The arithmetic of every level -- the Gaussian-windowed moments, the ssim and cs maps, their per-image sums and the 2x2 mean
pooling in front of the next level -- is one launch of gank_msssim_level (csrc/msssim.hip) for the whole batch.  The host adds
each image's per-tile partial sums in float64 in a fixed order and applies the closing formula (:184-185) in float64.  There is
no CPU path: NumPy inputs are uploaded, the compute is on the GPU.

NaN.  The reference raises a level's mean cs (and the last level's mean ssim) to a fractional power.  For weakly related image
pairs the mean cs of a small level is often NEGATIVE, and the score is then NaN in the reference -- and here, on purpose.  On
independent random pairs about half of single 32x32 pairs, a few percent of 128x128 pairs and no 256x256 pair come out NaN; a
BATCH call is NaN-free on the same data, because the reference averages every level over the whole batch before the power and
the batch mean of cs is positive.  That is the form to use for a diversity score (`msssim_diversity` of the trainers).
"""
import numpy as np
import torch

from .. import kernels as K

DEFAULT_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)     # :169; they do not sum to 1 (the paper's / MATLAB's values)
MAX_FILTER_SIZE = 11                                            # the window the kernel holds in registers


def _check_pair(img1, img2):
    """(:78-83, :160-165) -- before anything touches the device"""
    if tuple(img1.shape) != tuple(img2.shape):
        raise RuntimeError('Input images must have the same shape (%s vs. %s).' % (tuple(img1.shape), tuple(img2.shape)))
    if img1.ndim != 4:
        raise RuntimeError('Input images must have four dimensions, not %d' % img1.ndim)


def _check_filter(filter_size):
    if not filter_size:
        raise NotImplementedError("filter_size=0 (the no-blur branch of common/msssim.py:102-107) is not implemented")
    if filter_size < 0 or filter_size > MAX_FILTER_SIZE or int(filter_size) != filter_size:
        raise NotImplementedError(f"filter_size={filter_size}: the kernel holds windows of 1..{MAX_FILTER_SIZE} taps "
                                  "(common/msssim.py:50 defaults to 11)")


def _to_device(img):
    """uint8 / float32 [N,H,W,C] on the GPU.  NumPy arrays are uploaded (other dtypes than uint8 as float32)."""
    if isinstance(img, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("gank: MS-SSIM runs on the GPU (no CPU path exists)")
        img = torch.from_numpy(np.ascontiguousarray(img if img.dtype == np.uint8 else img.astype(np.float32))).cuda()
    return img.contiguous()


def gauss_taps(size, sigma):
    """The 1-D factor of _FSpecialGauss (:36-47): its 2-D window is exactly the outer product of this normalised vector.
    Even sizes sample at half-integer offsets."""
    x = np.arange(size, dtype=np.float64) - size // 2 + (0.5 if size % 2 == 0 else 0.0)
    g = np.exp(-(x ** 2) / (2.0 * sigma ** 2))
    return g / g.sum()


def msssim_levels(img1, img2, max_val=255, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, levels=5):
    """float64 [N, levels, 2]: per image pair and pyramid level the mean ssim ([..., 0]) and mean cs ([..., 1]) that
    _SSIMForMultiScale (:50-123) returns for that single pair at that level of MultiScaleSSIM's pyramid (:175-183).
    All images of a batch share a shape, so the reference's batch values are the mean over N of these."""
    _check_pair(img1, img2)
    _check_filter(filter_size)
    a, b = _to_device(img1), _to_device(img2)
    n, h, w, c = a.shape
    c1, c2, offset = (k1 * max_val) ** 2, (k2 * max_val) ** 2, max_val / 2.0
    shapes = []
    for _ in range(levels):                       # (:181-183) sizes halve, rounding up: a 1-pixel level stays 1 pixel
        size = min(filter_size, h, w)             # (:90)
        shapes.append((h, w, size, K.msssim_level_parts(h, w, c, size)))
        h, w = (h + 1) // 2, (w + 1) // 2
    parts = torch.empty(sum(n * s[3] * 2 for s in shapes), dtype=torch.float32, device=a.device)
    at = 0
    for lvl, (h, w, size, tiles) in enumerate(shapes):
        taps = gauss_taps(size, size * filter_sigma / filter_size)      # (:93)
        a, b = K.msssim_level(a, b, taps, c1, c2, offset, parts[at:at + n * tiles * 2], pool=lvl + 1 < levels)
        at += n * tiles * 2
    host = parts.cpu().numpy().astype(np.float64)                       # the one copy back; float64, fixed order from here on
    out = np.empty((n, levels, 2), dtype=np.float64)
    at = 0
    for lvl, (h, w, size, tiles) in enumerate(shapes):
        p = host[at:at + n * tiles * 2].reshape(n, tiles, 2)
        tot = np.zeros((n, 2), dtype=np.float64)
        for t in range(tiles):
            tot += p[:, t]
        out[:, lvl] = tot / float((h - size + 1) * (w - size + 1) * c)
        at += n * tiles * 2
    return out


def combine_levels(levels, weights=None):
    """(:184-185) prod(cs[:L-1] ** w[:L-1]) * ssim[L-1] ** w[L-1] in float64 on the host.  levels: [..., L, 2] (ssim, cs).
    A negative base under a fractional weight is NaN, as in the reference."""
    w = np.asarray(weights if weights is not None and len(weights) else DEFAULT_WEIGHTS, dtype=np.float64)
    lv = np.asarray(levels, dtype=np.float64)
    n_lv = w.size
    if lv.shape[-2] != n_lv or lv.shape[-1] != 2:
        raise RuntimeError(f"combine_levels: levels {lv.shape} do not fit {n_lv} weights")
    with np.errstate(invalid='ignore'):
        return np.prod(lv[..., :n_lv - 1, 1] ** w[:n_lv - 1], axis=-1) * lv[..., n_lv - 1, 0] ** w[n_lv - 1]


def _SSIMForMultiScale(img1, img2, max_val=255, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """(:50-123) -> (ssim, cs): the means of the two maps over every axis, batch included."""
    lv = msssim_levels(img1, img2, max_val, filter_size, filter_sigma, k1, k2, levels=1).mean(axis=0)
    return float(lv[0, 0]), float(lv[0, 1])


def MultiScaleSSIM(img1, img2, max_val=255, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03, weights=None, per_image=False):
    """(:126-185) the MS-SSIM score of two image batches [N,H,W,C] (uint8 or float32; GPU tensors or NumPy arrays).

    per_image=False: one float, the reference's batch semantics -- every level's ssim / cs is averaged over the whole batch
    before the weights are applied.  per_image=True: float64 [N], entry i is what the reference returns for
    img1[i:i+1], img2[i:i+1] -- NaN included wherever a level's mean cs (or the last level's mean ssim) of that pair is
    negative (see the module docstring: common for small, weakly related images; not an error and not "fixed" here)."""
    w = weights if weights is not None and len(weights) else DEFAULT_WEIGHTS
    lv = msssim_levels(img1, img2, max_val, filter_size, filter_sigma, k1, k2, levels=len(w))
    if per_image:
        return combine_levels(lv, w)
    return float(combine_levels(lv.mean(axis=0), w))


def quantize_on_device(x):
    """Generator output in [-1, 1] -> uint8 as the Inception-score path quantises it (gan_cifar_resnet.py:551:
    `((x + 1) * (255.99 / 2)).astype('int32')`), on the device."""
    return ((x.float() + 1.0) * (255.99 / 2)).clamp_(0, 255).to(torch.uint8)


def class_pair_diversity(draw, n_pairs, n_classes=10, weights=None):
    """The ACGAN paper's diversity score: MS-SSIM between pairs of samples of the SAME class.  draw() -> (uint8 images
    [b,H,W,C] on the device, int labels [b]); it is called until every class has 2 * n_pairs samples.  Consecutive samples of
    a class form a pair.  -> ({class: batch MultiScaleSSIM of that class's n_pairs pairs}, their mean)"""
    need = 2 * n_pairs
    kept, have = [[] for _ in range(n_classes)], [0] * n_classes
    while min(have) < need:
        imgs, labels = draw()
        labels = labels.cpu().numpy()
        for k in range(n_classes):
            if have[k] < need:
                idx = np.nonzero(labels == k)[0]
                if idx.size:
                    kept[k].append(imgs[torch.as_tensor(idx, device=imgs.device)])
                    have[k] += idx.size
    scores = {}
    for k in range(n_classes):
        s = torch.cat(kept[k], 0)[:need]
        scores[k] = MultiScaleSSIM(s[0::2].contiguous(), s[1::2].contiguous(), weights=weights)
    return scores, float(np.mean(list(scores.values())))
