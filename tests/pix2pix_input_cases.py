"""Shared by tests/test_pix2pix_input_gpu.py and its fp16 child (tests/pix2pix_input_fp16_worker.py): the AREA cases and how one
is run and measured against the float64 restatement."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pix2pix_input_ref as R  # noqa: E402

# name -> (H, panel width, scale_h, scale_w, crop): anisotropic non-integer, integer, upscaling
AREA_CASES = {"96x130->64x64": (96, 130, 64, 64, 64), "128->64": (128, 128, 64, 64, 64), "48->64": (48, 48, 64, 64, 64),
              "96x130->80x72 crop 64": (96, 130, 80, 72, 64)}
F32_BOUND = 2e-5            # a convex combination of at most 100 values in [-1, 1], accumulated in fp32
BF16_BOUND = 2.0 ** -9 + 2e-5       # half an ulp below 1
FP16_BOUND = 2.0 ** -12 + 2e-5


def area_case(name, mode=0, n=3, seed=0):
    """-> raw uint8 [n,H,P*Wp,3], table, kwargs of the kernel call"""
    h, wp, sh, sw, crop = AREA_CASES[name]
    rng = np.random.RandomState(seed + len(name))
    raw = rng.randint(0, 256, size=(n, h, wp * {0: 2, 1: 3, 2: 1}[mode], 3)).astype(np.uint8)
    table = np.stack([rng.randint(0, 2, size=n), rng.randint(0, sh - crop + 1, size=n), rng.randint(0, sw - crop + 1, size=n)], axis=1).astype(np.int32)
    return raw, table, dict(mode=mode, scale_h=sh, scale_w=sw, crop=crop)


def run_area_case(name, dtype, mode=0, direction=0):
    """the largest |kernel - restatement| over inputs and targets, every element counted"""
    import torch
    from gan_lib_tensorflow_amd import kernels as K
    raw, table, kw = area_case(name, mode)
    got = K.pix2pix_load_examples(torch.from_numpy(raw).cuda(), torch.from_numpy(table).cuda(), kw["mode"], direction, kw["scale_h"], kw["scale_w"],
                                  kw["crop"], dtype=dtype)
    ref = R.load_examples(raw, kw["mode"], direction, kw["scale_h"], kw["scale_w"], kw["crop"], table)
    dev = 0.0
    for g, r in zip(got, ref):
        g = g.to(torch.float64).cpu().numpy()
        assert g.shape == r.shape and np.isfinite(g).all()
        dev = max(dev, float(np.abs(g - r).max()))
    return dev
