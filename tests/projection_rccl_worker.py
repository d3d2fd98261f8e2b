"""Worker of tests/test_projection_gpu.py::test_data_parallel_path_with_a_world_size_one_group: the projection critic through the
data-parallel update path (a world-size-1 RCCL group: bucketed generator update, critic update with its all-reduce call) against
the single-process path, in a process of its own with the ordered teardown of tests/rccl_worker.py -- `RCCL PATH OK` is printed
only after destroy_process_group(), and the parent fails on any non-zero exit code."""
import gc
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import projection_ref as R  # noqa: E402
from gan_lib_tensorflow_amd import functional as Fn  # noqa: E402
from gan_lib_tensorflow_amd import parallel  # noqa: E402
from gan_lib_tensorflow_amd.SNGAN import gan_cifar_resnet as S  # noqa: E402

s = socket.socket()
s.bind(("127.0.0.1", 0))
port = s.getsockname()[1]
s.close()
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
stats_were, Fn.CONV_EPILOGUE_STATS = Fn.CONV_EPILOGUE_STATS, False          # (fixed-order statistics: see tests/rccl_worker.py)
parallel.disable_collective_event_cache()
dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
ok = False
try:
    results = {}
    for name, pg in (("plain", None), ("data_parallel", dist.group.WORLD)):
        tr = S.SNGANTrainer(batch_size=8, seed=17, use_graphs=True, process_group=pg, projection=True, state=R.init_projection_params(17))
        assert tr.projection and tr.dp == (pg is not None) and tr.bucketed == (pg is not None)
        assert tr.store.param_count('Discriminator') == R.CRITIC_PARAMS
        feed = S.synthetic_batches(8, "cuda", seed=5)
        for _ in range(3):
            tr.train_iteration(feed)
        torch.cuda.synchronize()
        assert tr.use_graphs
        o = tr.d_flat['offsets'][R.TABLE]
        results[name] = (tr.g_flat["params"].clone(), tr.d_flat["params"].clone(), float(tr.g_loss), tr.rng_state.clone(), int(tr.g_opt.t),
                         int(tr.d_opt.t), tr.d_flat["params"][o:o + 1280].clone())
        del tr, feed
        gc.collect()
    ref, got = results["plain"], results["data_parallel"]
    assert torch.equal(got[3], ref[3]) and got[4] == ref[4] == 2 and got[5] == ref[5] == 15
    for a, b_ in ((got[0], ref[0]), (got[1], ref[1]), (got[6], ref[6])):
        d = (a - b_).abs()
        # (three iterations of TF-Adam with beta1 = 0 on trajectories that differ by atomics ordering: tests/rccl_worker.py's bound)
        assert torch.isfinite(a).all() and d.max().item() < 40 * 2e-4 and d.mean().item() < 3e-4, (d.max().item(), d.mean().item())
    assert abs(got[2] - ref[2]) < 0.5
    init = torch.tensor(R.init_projection_params(17)[R.TABLE]).cuda().reshape(-1)
    assert float((got[6] - init).abs().max()) > 1e-4                      # the table is trained under data parallel
    ok = True
finally:
    Fn.CONV_EPILOGUE_STATS = stats_were
    results = ref = got = init = None
    gc.collect()
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    dist.destroy_process_group()
if ok:
    print("RCCL PATH OK", flush=True)
