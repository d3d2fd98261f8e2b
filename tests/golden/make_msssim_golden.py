"""Records tests/golden/msssim.npz from the REFERENCE program itself: common/msssim.py of watsonyanghx/GAN_Lib_Tensorflow, which
runs on a CPU with NumPy + SciPy (TensorFlow is imported there for command-line flags only, so a stub module stands in).

    python tests/golden/make_msssim_golden.py /path/to/GAN_Lib_Tensorflow

Never run by a test.  Per case (tests/msssim_cases.py) it stores
  <case>/levels   float64 [N, L, 2]  per pair and level (ssim, cs): what the reference's MultiScaleSSIM got from its own
                                     _SSIMForMultiScale at each level of its own pyramid, called on that single pair
  <case>/pairs    float64 [N]        the reference's MultiScaleSSIM of each single pair (NaN where the reference gives NaN)
  <case>/batch    float64            the reference's MultiScaleSSIM of the whole batch
and per base case the SHA-256 of the input bytes, plus the inputs themselves where they are at most 64 KB.
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msssim_cases as MC  # noqa: E402

BAND = 5e-4          # tests/test_msssim_gpu.py leaves pairs with a reference base inside +-BAND out of the NaN-mask comparison
BAND_CAP = 0.05      # ... and at most this share of a case's pairs


def load_reference(root):
    tf = types.ModuleType("tensorflow")
    tf.flags = types.SimpleNamespace(DEFINE_string=lambda *a, **k: None, FLAGS=None)
    tf.app = types.SimpleNamespace(run=lambda *a, **k: None)
    sys.modules["tensorflow"] = tf
    spec = importlib.util.spec_from_file_location("reference_msssim", os.path.join(root, "common", "msssim.py"))
    mod = importlib.util.module_from_spec(spec)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", DeprecationWarning)
        spec.loader.exec_module(mod)
    return mod


def record(ref, a, b, kwargs):
    """the reference on every single pair (its per-level values seen through a recording wrapper around its own
    _SSIMForMultiScale) and on the batch"""
    inner = ref._SSIMForMultiScale
    seen = []

    def spy(*args, **kw):
        out = inner(*args, **kw)
        seen.append(out)
        return out

    levels, pairs = [], []
    ref._SSIMForMultiScale = spy
    try:
        with np.errstate(invalid="ignore"):
            for i in range(a.shape[0]):
                del seen[:]
                pairs.append(ref.MultiScaleSSIM(a[i:i + 1], b[i:i + 1], **kwargs))
                levels.append(np.array(seen, dtype=np.float64))
    finally:
        ref._SSIMForMultiScale = inner
    with np.errstate(invalid="ignore"):
        batch = ref.MultiScaleSSIM(a, b, **kwargs)
    return np.stack(levels), np.array(pairs, dtype=np.float64), np.float64(batch)


def main():
    ref = load_reference(sys.argv[1])
    out = {}
    for name in MC.BASE:
        a, b = MC.generate(name)
        out[f"{name}/sha256"] = np.array(MC.digest(a, b))
        if a.nbytes + b.nbytes <= MC.STORE_RAW_BYTES:
            out[f"{name}/a"], out[f"{name}/b"] = a, b
    for name in MC.CASES:
        a, b, kwargs = MC.inputs(name, out)
        levels, pairs, batch = record(ref, a, b, kwargs)
        out[f"{name}/levels"], out[f"{name}/pairs"], out[f"{name}/batch"] = levels, pairs, batch
        bases = np.concatenate([levels[:, :-1, 1], levels[:, -1:, 0]], axis=1)
        in_band = (np.abs(bases) < BAND).any(axis=1).mean()
        print(f"{name:16s} pairs {a.shape[0]:3d}  batch {batch:.6f}  NaN pairs {np.isnan(pairs).mean():5.1%}  inside the band {in_band:5.1%}")
        assert in_band <= BAND_CAP, f"{name}: {in_band:.1%} of the pairs lie inside the NaN band; pick another seed"
    np.savez_compressed(MC.GOLDEN, **out)
    print(f"{MC.GOLDEN}: {os.path.getsize(MC.GOLDEN)} bytes")
    assert os.path.getsize(MC.GOLDEN) <= 200 * 1024


if __name__ == "__main__":
    main()
