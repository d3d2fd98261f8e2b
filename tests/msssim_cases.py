"""The MS-SSIM fixture cases (tests/golden/msssim.npz): shared by the script that records the reference's numbers
(tests/golden/make_msssim_golden.py) and by the tests that replay them.  Inputs larger than 64 KB per case are not stored: they
are regenerated here from the recorded seed and checked against the recorded SHA-256."""
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "msssim.npz")
STORE_RAW_BYTES = 64 * 1024

# name -> (height, width, channels, pairs, kind, seed)
BASE = {
    "s32_indep": (32, 32, 3, 64, "indep", 3201),
    "s32_noisy": (32, 32, 3, 64, "noisy", 3202),
    "s32_bright": (32, 32, 3, 64, "bright", 3203),
    "s45_indep": (45, 37, 1, 16, "indep", 4501),
    "s45_noisy": (45, 37, 1, 16, "noisy", 4502),
    "s128_indep": (128, 128, 3, 8, "indep", 12801),
    "s128_noisy": (128, 128, 3, 8, "noisy", 12802),
    "s128_bright": (128, 128, 3, 8, "bright", 12803),
    "s256_indep": (256, 256, 3, 2, "indep", 25601),
    "s256_noisy": (256, 256, 3, 2, "noisy", 25602),
    "s512_noisy": (512, 512, 3, 1, "noisy", 51202),
}
# name -> (base case, pairs taken from its front, keyword arguments, inputs as float32 in [0, 1])
VARIANTS = {}
for _kind in ("indep", "noisy"):
    VARIANTS[f"s32_{_kind}_w2"] = (f"s32_{_kind}", 16, dict(weights=[0.5, 0.5]), False)
    VARIANTS[f"s32_{_kind}_f32"] = (f"s32_{_kind}", 16, dict(max_val=1.0), True)
    VARIANTS[f"s32_{_kind}_fs7"] = (f"s32_{_kind}", 16, dict(filter_size=7), False)
CASES = list(BASE) + list(VARIANTS)


def kind_of(name):
    return BASE[VARIANTS[name][0] if name in VARIANTS else name][4]


def smooth(rng, n, h, w, c):
    """standard-normal noise at 1/4 resolution, replicated 4x per axis, plus 0.3 x standard-normal pixel noise, min-max
    scaled to uint8"""
    low = rng.standard_normal((n, (h + 3) // 4, (w + 3) // 4, c))
    x = np.repeat(np.repeat(low, 4, axis=1), 4, axis=2)[:, :h, :w]
    x = x + 0.3 * rng.standard_normal((n, h, w, c))
    x = (x - x.min()) / (x.max() - x.min())
    return np.round(x * 255.0).astype(np.uint8)


def generate(name):
    """-> (a, b) uint8 [N,H,W,C] of a BASE case"""
    h, w, c, n, kind, seed = BASE[name]
    rng = np.random.default_rng(seed)
    if kind == "indep":
        return smooth(rng, n, h, w, c), smooth(rng, n, h, w, c)
    if kind == "noisy":
        a = smooth(rng, n, h, w, c)
        b = np.clip(a.astype(np.int64) + rng.integers(-20, 21, size=a.shape), 0, 255).astype(np.uint8)
        return a, b
    a = (250 + rng.integers(-2, 3, size=(n, h, w, c))).astype(np.uint8)
    return a, np.roll(a, 1, axis=0)


def digest(a, b):
    return hashlib.sha256(a.tobytes() + b.tobytes()).hexdigest()


def inputs(name, golden):
    """-> (img1, img2, kwargs) of any case, as the reference was fed them.  Raises if regenerated inputs are not the recorded ones."""
    if name in VARIANTS:
        base, take, kwargs, as_float = VARIANTS[name]
        a, b, _ = inputs(base, golden)
        a, b = a[:take], b[:take]
        if as_float:
            a, b = (a / 255.0).astype(np.float32), (b / 255.0).astype(np.float32)
        return a, b, dict(kwargs)
    if f"{name}/a" in golden:
        a, b = golden[f"{name}/a"], golden[f"{name}/b"]
    else:
        a, b = generate(name)
    if digest(a, b) != str(golden[f"{name}/sha256"]):
        raise AssertionError(f"{name}: the inputs do not hash to the recorded SHA-256: regenerate the fixture "
                             "(tests/golden/make_msssim_golden.py)")
    return a, b, {}
