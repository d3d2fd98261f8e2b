"""Runs in its own process with GANK_DTYPE=fp16 (libgank_f16.so), in the pattern of tests/fp16_worker.py: the AREA cases of
tests/test_pix2pix_input_gpu.py with the 16-bit output of the fp16 library, against the float64 restatement at 2^-12 + 2e-5.
Writes {case: "ok <deviation>" | traceback} as JSON to argv[1]; exit status 1 if any case failed."""
import json
import os
import sys
import traceback

assert os.environ.get("GANK_DTYPE") == "fp16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

from gan_lib_tensorflow_amd import _lib, kernels as K  # noqa: E402
import pix2pix_input_cases as PC  # noqa: E402

assert K.BF16 is torch.float16 and _lib.load().gank_act_dtype() == 1 and _lib.LIB_PATH.endswith("libgank_f16.so")

if __name__ == "__main__":
    results = {}
    for name in PC.AREA_CASES:
        try:
            dev = PC.run_area_case(name, K.BF16)
            print(f"fp16 AREA {name}: max deviation {dev:.3e} (bound {PC.FP16_BOUND:.3e})", flush=True)
            assert dev <= PC.FP16_BOUND, dev
            results[name] = f"ok {dev:.3e}"
        except Exception:
            results[name] = traceback.format_exc()
            print(f"FAILED {name}\n{results[name]}", flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(results, f)
    sys.exit(0 if all(v.startswith("ok") for v in results.values()) else 1)
