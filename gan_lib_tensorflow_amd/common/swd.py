"""Sliced Wasserstein distance on the GPU (Karras et al., "Progressive Growing of GANs for Improved Quality, Stability, and
Variation", ICLR 2018, section 5): the metric of that paper's tables.  It needs no network and no downloaded weights, and it
compares two image sets at every resolution of a Laplacian pyramid separately.

    pyramid      levels H, H/2, .. while the side is >= 16 (a smaller image is one level); every level but the last is
                 level - pyr_up(next level), the last the plain downsampled image; 5 x 5 binomial window, mirror boundaries
    descriptors  per level and side `nhoods_per_image` patches of nhood_size x nhood_size x C per image, centres uniform in
                 [h, W - h) x [h, H - h), h = nhood_size // 2; each channel normalised to mean 0 and population standard
                 deviation 1 over all patches of the level and side; a descriptor is the patch in (channel, y, x) order
    slices       dir_repeats x dirs_per_repeat unit directions; both sides projected, every direction's M projections sorted,
                 mean |sorted_a - sorted_b| over rows and directions, then over repeats
    result       one value per level and their mean, both x 1000 as the paper prints them

Departures from the published evaluation program, none of which changes a distribution: the directions stay float64 (there
they are cast to float32); the centres are one table per level and side (there one per minibatch); everything is float64.

The draws.  All come from one numpy.random.RandomState(seed), in this order: the direction matrices, one randn(K,
dirs_per_repeat) per repeat; then for side a, then for side b, level by level, x = randint(h, W - h, M) and then
y = randint(h, H - h, M), M = N * nhoods_per_image.

Stages:  images -> float64 on the device (a torch cast) -> `K.swd_pyr_down` / `K.swd_laplacian` (csrc/swd.hip)
         -> `K.swd_patch_stats` twice (the mean, then the squares about the mean); mean and std finished here in float64
         -> per repeat `K.swd_project` (patches gathered straight from the level: no descriptor bank), `K.swd_sort_rows` (the
            library's own radix sort), `K.swd_sorted_l1` -> one copy back of the workgroup partials, the rest in NumPy float64.
Keys are processed one repeat at a time: two buffers of dirs_per_repeat x M doubles plus one of work space.  No atomics
anywhere: the same inputs give the same bits.  There is no CPU path."""
import numpy as np
import torch

from .. import kernels as K
from .fid import draw_until


def level_sizes(h, w):
    """[(h, w), (h/2, w/2), ..] while the smaller side is >= 16; an image smaller than 16 is a single level.  A side that is
    halved must be even and >= 4."""
    h, w = int(h), int(w)
    sizes = [(h, w)]
    while min(h, w) >= 32:
        if h % 2 or w % 2:
            raise ValueError(f"level_sizes: a {h} x {w} level cannot be halved (odd side)")
        h, w = h // 2, w // 2
        sizes.append((h, w))
    return sizes


def _device_images(images, name):
    if isinstance(images, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("gank: the sliced Wasserstein distance runs on the GPU (no CPU path exists)")
        images = torch.from_numpy(np.ascontiguousarray(images)).cuda()
    if not images.is_cuda:
        raise RuntimeError(f"gank: {name} must live on the GPU (no CPU path exists)")
    if images.dim() != 4:
        raise ValueError(f"swd: {name} {tuple(images.shape)}, expected images [N,H,W,C]")
    if images.dtype not in (torch.uint8, torch.float32, torch.float64):
        raise TypeError(f"swd: {name} must be uint8 or float32 images, got {images.dtype}")
    return images


def laplacian_pyramid(images):
    """images [N,H,W,C] uint8 or float32 (NumPy or device tensor) -> list of float64 device tensors, finest first"""
    images = _device_images(images, "images")
    sizes = level_sizes(images.shape[1], images.shape[2])
    levels = [images.to(torch.float64).contiguous()]          # a copy: the levels are changed in place below
    if levels[0].data_ptr() == images.data_ptr():
        levels[0] = levels[0].clone()
    for _ in sizes[1:]:
        levels.append(K.swd_pyr_down(levels[-1]))
    for i in range(len(levels) - 1):
        K.swd_laplacian(levels[i], levels[i + 1])
    return levels


def draw_directions(k, dir_repeats, dirs_per_repeat, rng):
    """float64 [dir_repeats, k, dirs_per_repeat]: per repeat randn(k, dirs_per_repeat), every column scaled to unit length"""
    out = []
    for _ in range(dir_repeats):
        d = rng.randn(k, dirs_per_repeat)
        out.append(d / np.sqrt(np.sum(np.square(d), axis=0, keepdims=True)))
    return np.stack(out)


def draw_centres(n, h, w, nhood_size, nhoods_per_image, rng):
    """(cx, cy) int32 [n * nhoods_per_image]: x = randint(half, w - half, M), then y = randint(half, h - half, M)"""
    half, m = nhood_size // 2, n * nhoods_per_image
    if nhood_size % 2 == 0 or nhood_size > min(h, w):
        raise ValueError(f"swd: a {nhood_size} x {nhood_size} patch does not fit a {h} x {w} level (odd sizes only)")
    cx = rng.randint(half, w - half, m).astype(np.int32)
    cy = rng.randint(half, h - half, m).astype(np.int32)
    return cx, cy


def draw_tables(n, h, w, c, nhood_size=7, nhoods_per_image=128, dir_repeats=4, dirs_per_repeat=128, seed=0):
    """Every draw of `calculate_swd` for two sides of n images [h, w, c], in the order of the module docstring ->
    (dirs float64 [dir_repeats, K, dirs_per_repeat], centres_a, centres_b), centres_x a list over levels of (cx, cy) int32 [M]"""
    rng = np.random.RandomState(seed)
    dirs = draw_directions(c * nhood_size * nhood_size, dir_repeats, dirs_per_repeat, rng)
    sizes = level_sizes(h, w)
    sides = [[draw_centres(n, lh, lw, nhood_size, nhoods_per_image, rng) for lh, lw in sizes] for _ in range(2)]
    return dirs, sides[0], sides[1]


def _table(t):
    """a centre table as a tensor (a read-only NumPy array is copied: torch cannot wrap it)"""
    return torch.as_tensor(t.copy() if isinstance(t, np.ndarray) and not t.flags.writeable else t)


def patch_mean_std(level, cx, cy, nhood_size, nhoods_per_image):
    """(mean, std) float64 [C] of the level's patches per channel, population standard deviation: `K.swd_patch_stats` for
    the sum, then again about the mean it gives (no cancellation of a large mean against the squares), finished in float64
    here.  A channel with zero variance raises RuntimeError."""
    m = len(cx)
    count = float(m * nhood_size * nhood_size)
    cx, cy = _table(cx), _table(cy)
    mean = K.swd_patch_stats(level, cx, cy, nhood_size, nhoods_per_image).cpu().numpy()[:, 0] / count
    about = K.swd_patch_stats(level, cx, cy, nhood_size, nhoods_per_image, shift=mean).cpu().numpy()
    var = about[:, 1] / count - np.square(about[:, 0] / count)
    if not np.all(np.isfinite(var)) or np.any(var <= 0.0):
        raise RuntimeError(f"swd: a channel of the patches has zero variance (variances {var.tolist()}): a constant image set?")
    return mean, np.sqrt(var)


def sliced_wasserstein(level_a, level_b, centres_a, centres_b, dirs, nhood_size=7, nhoods_per_image=128):
    """One level: level_x float64 [N,H,W,C] on the device, centres_x = (cx, cy) int32 [M], dirs float64 [dir_repeats, K,
    dirs_per_repeat] (NumPy) -> float, the mean over repeats of mean |sort(proj_a) - sort(proj_b)|, NOT yet x 1000."""
    if tuple(level_a.shape) != tuple(level_b.shape):
        raise ValueError(f"swd: the sides differ in shape, {tuple(level_a.shape)} and {tuple(level_b.shape)}")
    dirs = np.asarray(dirs, dtype=np.float64)
    if dirs.ndim != 3:
        raise ValueError(f"swd: dirs {dirs.shape}, expected [dir_repeats, K, dirs_per_repeat]")
    m = len(centres_a[0])
    if len(centres_b[0]) != m:
        raise ValueError(f"swd: the sides differ in their number of patches, {m} and {len(centres_b[0])}")
    sides = []
    for level, (cx, cy) in ((level_a, centres_a), (level_b, centres_b)):
        cx, cy = _table(cx), _table(cy)
        sides.append((level, cx, cy) + patch_mean_std(level, cx, cy, nhood_size, nhoods_per_image))
    ndirs, dev = dirs.shape[2], level_a.device
    keys = [torch.empty((ndirs, m), dtype=torch.float64, device=dev) for _ in range(2)]
    tmp = torch.empty((ndirs, m), dtype=torch.float64, device=dev)
    hist = torch.empty(K.swd_sort_ws_elems(ndirs, m), dtype=torch.int32, device=dev)
    part = torch.empty((ndirs, K.swd_sorted_l1_parts(m)), dtype=torch.float64, device=dev)
    repeats = []
    for d in dirs:
        d_dev = torch.from_numpy(np.ascontiguousarray(d)).to(dev)
        for (level, cx, cy, mean, std), buf in zip(sides, keys):
            K.swd_project(level, cx, cy, nhood_size, nhoods_per_image, mean, std, d_dev, out=buf)
            K.swd_sort_rows(buf, tmp=tmp, hist=hist)
        sums = K.swd_sorted_l1(keys[0], keys[1], part=part).cpu().numpy()
        repeats.append(sums.sum(axis=1).sum() / (float(m) * ndirs))
    return float(np.mean(repeats))


def calculate_swd(a, b, nhood_size=7, nhoods_per_image=128, dir_repeats=4, dirs_per_repeat=128, seed=0):
    """SWD between two image sets of equal shape [N,H,W,C] (uint8 or float32, NumPy or device tensor) ->
    (float64 [levels], their mean), both x 1000.  The draws are those of `draw_tables(seed=seed)`."""
    a, b = _device_images(a, "a"), _device_images(b, "b")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"calculate_swd: the sides differ in shape, {tuple(a.shape)} and {tuple(b.shape)}")
    n, h, w, c = a.shape
    if nhood_size > min(level_sizes(h, w)[-1]):
        raise ValueError(f"calculate_swd: a {nhood_size} x {nhood_size} patch does not fit the {h} x {w} images' coarsest level")
    dirs, centres_a, centres_b = draw_tables(n, h, w, c, nhood_size, nhoods_per_image, dir_repeats, dirs_per_repeat, seed)
    pyr_a, pyr_b = laplacian_pyramid(a), laplacian_pyramid(b)
    values = [sliced_wasserstein(la, lb, ca, cb, dirs, nhood_size, nhoods_per_image)
              for la, lb, ca, cb in zip(pyr_a, pyr_b, centres_a, centres_b)]
    values = np.asarray(values, dtype=np.float64) * 1e3
    return values, float(values.mean())


def sample_swd(draw, real, n, seed=0, nhood_size=7, **kw):
    """SWD of n generated samples against the first n images of `real` [N >= n,H,W,C]: draw() -> uint8 images [b,H,W,C] on the
    device, called until n are in (fid.draw_until); the samples stay on the device.  A patch that does not fit
    the images raises before anything is drawn.  **kw: nhoods_per_image, dir_repeats, dirs_per_repeat of `calculate_swd`."""
    if getattr(real, 'ndim', 0) != 4:
        raise ValueError(f"swd: real {tuple(getattr(real, 'shape', ()))}, expected images [N,H,W,C]")
    if len(real) < n:
        raise ValueError(f"swd: real has {len(real)} images, needs at least {n}")
    if nhood_size > min(level_sizes(real.shape[1], real.shape[2])[-1]):
        raise ValueError(f"swd: a {nhood_size} x {nhood_size} patch does not fit {real.shape[1]} x {real.shape[2]} images")
    fake = torch.cat(list(draw_until(draw, n)))
    if tuple(fake.shape[1:]) != tuple(real.shape[1:]):
        raise ValueError(f"swd: real {tuple(real.shape)} is not at the samples' size {tuple(fake.shape[1:])}")
    return calculate_swd(fake, real[:n], nhood_size=nhood_size, seed=seed, **kw)
