#!/usr/bin/env python
"""bench.py -- images/sec of the SNGAN-ResNet CIFAR-10 train iteration on N MI355X (BASELINE.json).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = one reference iteration (SNGAN/gan_cifar_resnet.py:599-620): 1 generator update on 2x64
fakes + N_CRITIC=5 critic updates on 64 real + 64 fake each, i.e. 320 real images per GPU.
Weak scaling: every rank processes its own 64-image batches; G/D gradients are summed with one RCCL
all-reduce per update.  Inputs are synthetic CIFAR-10-shaped uint8 batches already resident in HBM.

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times --steps iterations and reports them; the keys
below stay in the line but are null unless --full asks for them (each takes runs of its own after the timed steps):
  roofline      -- dominant MFMA kernel family, algorithmic FLOPs / HIP-event time of its launches over one
                   eagerly executed iteration (events recorded on the launch stream by libgank's profiler)
  cpu_baseline  -- the oracle's torch-CPU fp32 restatement of the same iteration, timed on this box's host
                   cores on a bounded sample (rank 0, N=1 only; --no-cpu-baseline skips it)
  fp16, other_configs -- present with --full on one bf16 rank: the headline with IEEE-half activations (a child process;
                   --no-fp16 skips it) and the ACGAN / PGGAN / Pix2Pix step times (--no-other-configs skips them)

--dump-outputs DIR writes what the last timed step computed (rank 0) as DIR/<name>.npy, float32: see dump_outputs().  That step
then starts from the seeded weights, Adam state and RNG state (restore_seeded_state), so its outputs repeat from run to run.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA peak (MI355X_MICROARCH.md, chip-level parameters)
GFLOP_PER_REAL_IMAGE = 13.77   # 4406.0 GFLOP per iteration / 320 real images


def host_cores():
    """Physical cores this process may run on: the box's share of the host (scheduler affinity / cgroup), not the
    machine's total; hyper-thread siblings count once."""
    try:
        allowed = len(os.sched_getaffinity(0))
    except AttributeError:
        allowed = os.cpu_count() or 1
    try:
        import psutil
        phys, logical = psutil.cpu_count(logical=False) or allowed, psutil.cpu_count(logical=True) or allowed
        if logical > phys:                      # SMT: the affinity mask counts logical CPUs
            allowed = max(1, allowed * phys // logical)
    except Exception:  # noqa: BLE001
        pass
    # the container's CPU bandwidth quota (cgroup v2 cpu.max / v1 cfs quota): a GPU box shows all 256 logical CPUs of its host
    # in the affinity mask but may run 16 of them at a time -- 128 threads on that share ran the baseline 4x slower than 16
    try:
        quota = None
        if os.path.exists("/sys/fs/cgroup/cpu.max"):
            q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
            quota = None if q == "max" else float(q) / float(per)
        elif os.path.exists("/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            quota = None if q <= 0 else q / per
        if quota is not None:
            allowed = min(allowed, max(1, int(quota)))
    except Exception:  # noqa: BLE001
        pass
    return max(1, allowed)


def traffic_per_launch(tj, tag):
    """HBM bytes per launch of a launcher tag from a pmc_bench_traffic.sh table.  A tag may name a kernel plus its follow-up
    launch ("a + b": the parts add) and leaves out trailing template arguments the launcher chooses at run time (the
    statistics epilogue: `<0, 32>` covers rocprofv3's `<0, 32, true>` and `<0, 32, false>`, weighted by launches)."""
    per, total = tj.get("per_kernel", {}), 0.0
    for part in tag.split(" + "):
        hits = [v for k, v in per.items() if k == part or (part.endswith(">") and k.startswith(part[:-1] + ", ") and k.count(",") == part.count(",") + 1)]
        if not hits:
            return None
        n = sum(v["launches"] for v in hits)
        total += sum(v["bytes_per_launch"] * v["launches"] for v in hits) / max(n, 1)
    return total


def cpu_baseline(budget_s=40.0):
    """Oracle ("port") leg: torch-CPU fp32 restatement of the reference graph; the timed sample is one whole
    iteration (5 D updates + 1 G update), at batch 64 when that fits budget_s, else at a smaller batch scaled up."""
    import numpy as np
    from oracle import ref_torch as T
    cores = host_cores()
    torch.set_num_threads(cores)
    P = T.to_torch(T.init_sngan_params(0), dtype=torch.float32)
    tr = T.Trainer(P)
    rng = np.random.default_rng(0)

    def one_d(b):
        z = torch.tensor(rng.normal(size=(b, 128)), dtype=torch.float32)
        labels = torch.tensor(rng.integers(0, 10, b))
        real = torch.tensor(rng.integers(0, 256, (b, 3072)))
        deq = torch.tensor(rng.uniform(0, 1 / 128, (b, 3072)), dtype=torch.float32)
        t0 = time.perf_counter()
        tr.d_step(0, real, labels, z, deq)
        return time.perf_counter() - t0

    def one_g(b):
        z2 = torch.tensor(rng.normal(size=(2 * b, 128)), dtype=torch.float32)
        fl = torch.tensor(rng.integers(0, 10, 2 * b))
        t0 = time.perf_counter()
        tr.g_step(0, z2, fl)
        return time.perf_counter() - t0

    def one(b):
        return one_d(b), one_g(b)

    one(2)                                  # warm-up (thread pool, oneDNN primitives)
    td, tg = one(8)
    per_img = (5 * td + tg) / 8
    b = 64
    while b > 8 and per_img * b > budget_s:
        b //= 2
    # the timed sample: one whole iteration (5 D updates + 1 G update) at batch b
    t0 = time.perf_counter()
    tds = [one_d(b) for _ in range(5)]
    tg = one_g(b)
    t_iter = (time.perf_counter() - t0) * (64.0 / b)
    return {"value": round(320.0 / t_iter, 3), "unit": "images/sec", "cores": cores, "kind": "port",
            "sample": f"one full iteration (5 D updates + 1 G update) at batch {b} of the torch-CPU fp32 restatement of the "
                      f"reference graph (oracle/ref_torch.py){'' if b == 64 else ', scaled linearly to batch 64'}: "
                      f"{t_iter:.2f}s (D {sum(tds) / 5:.2f}s each, G {tg:.2f}s)"}


def other_configs(steps=5):
    """BASELINE.json configs 3-5 at their per-GPU sizes, in this process AFTER the headline measurement (outside its timed region):
    a few captured steps each -> {ms_per_step, gflop_as_run, mfma_frac}.  ACGAN at 32 samples (config 3's share of 256 over 8
    GPUs; ACGAN/train.py:89-121), PGGAN model_nvidia at 64x64 while the block fades in (PGGAN/train.py:83-136), Pix2Pix U-Net at
    512x512, batch 16 (Pix2Pix/train.py:704-729; the reference graph does not run at 256x256).  The conv
    FLOPs are the ones the kernels executed (counted by the launchers over one eager step of the same configuration)."""
    from gan_lib_tensorflow_amd import kernels as K
    from gan_lib_tensorflow_amd.SNGAN.gan_cifar_resnet import synthetic_batches
    out = {}

    def measure(name, make, step, workload):
        try:
            tr = make(False)                      # eager: FLOPs as run
            step(tr)
            torch.cuda.synchronize()
            K.prof_reset()
            K.prof_enable(True)
            step(tr)
            torch.cuda.synchronize()
            K.prof_enable(False)
            fl = sum(K.prof_collect(f)[2] for f in (0, 1))
            K.prof_reset()
            del tr
            tr = make(True)                       # captured
            for _ in range(3):                    # eager first execution, capture, one replay
                step(tr)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step(tr)
            torch.cuda.synchronize()
            t = (time.perf_counter() - t0) / steps
            out[name] = {"workload": workload, "ms_per_step": round(1e3 * t, 3), "steps": steps, "gflop_as_run": round(fl / 1e9, 1),
                         "mfma_frac": round(fl / t / (PEAK_BF16_TFLOPS * 1e12), 4)}
            del tr
        except Exception as e:  # noqa: BLE001 -- the headline line must not depend on the other configurations
            out[name] = {"workload": workload, "error": f"{type(e).__name__}: {e}"[:300]}
        import gc
        gc.collect()
        torch.cuda.synchronize()

    from gan_lib_tensorflow_amd.ACGAN.train import ACGANTrainer
    feed = synthetic_batches(32, "cuda", seed=2)
    it = [0]

    def acgan_step(trn):
        it[0] += 1
        trn.train_iteration(feed, it[0])
    measure("acgan_bs32", lambda g: ACGANTrainer(batch_size=32, seed=1, use_graphs=g), acgan_step,
            "ACGAN ResNet CIFAR-10, 32 samples per GPU (bs=256 over 8 GPUs): 1 G + 5 D updates, WGAN-GP double backward")
    from gan_lib_tensorflow_amd.PGGAN.train import PGGANTrainer, default_args as pg_args
    feed16 = synthetic_batches(16, "cuda", seed=2)
    measure("pggan_64_fading", lambda g: PGGANTrainer(pg_args(batch_size=16, block_count=4, image_size=64, trans=True), seed=1, use_graphs=g),
            lambda trn: trn.train_iteration(feed16), "PGGAN model_nvidia 64x64, block fading in, batch 16: 1 G + 5 D updates")
    from gan_lib_tensorflow_amd.Pix2Pix.train import Pix2PixTrainer, default_args as px_args
    g = torch.Generator().manual_seed(3)
    a = (torch.rand(16, 512, 512, 3, generator=g) * 2 - 1).to(K.BF16).cuda()
    b = (torch.rand(16, 512, 512, 3, generator=g) * 2 - 1).to(K.BF16).cuda()
    measure("pix2pix_512_bs16", lambda gr: Pix2PixTrainer(px_args(batch_size=16, crop_size=512), seed=1, use_graphs=gr),
            lambda trn: trn.train_step(a, b), "Pix2Pix U-Net + PatchGAN 512x512, batch 16: 5 D + 1 G updates")
    return out


def fp16_child(steps, warmup):
    """The same headline measurement with IEEE-half activations (libgank_f16.so, static loss scale 1024), in a process of its own --
    the element type is a per-process choice -- started BEFORE this process touches the GPU and finished before it does."""
    import subprocess
    env = dict(os.environ, GANK_DTYPE="fp16", GANK_BENCH_CHILD="1")
    env.pop("GANK_LIB_NAME", None)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                            "--no-cpu-baseline", "--no-other-configs", "--no-fp16"], env=env, capture_output=True, text=True, timeout=300)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not line:
            return {"error": f"exit {r.returncode}: {r.stderr[-300:]}"}
        d = json.loads(line[-1])
        return {"value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"], "median_ms_per_step_hip_events": d["median_ms_per_step_hip_events"],
                "steps": d["steps"], "dtype": d["dtype"], "loss_scale": 1024, "finite": d["config"]["finite"]}
    except Exception as e:  # noqa: BLE001
        return {"error": f"{type(e).__name__}: {e}"[:300]}


DUMP_LIMIT_BYTES = 64 << 20


def seeded_state(tr):
    """--dump-outputs: the trainer's numeric state as the seed made it (weights, spectral-norm u vectors, Adam slots and step
    counts, device RNG state), taken before the first iteration."""
    return {"vars": {k: v.detach().clone() for k, v in tr.store.vars.items()},
            "slots": {(net, key): tr.store.flat[net][key].clone() for net in ("Generator", "Discriminator") for key in ("m", "v")},
            "adam_t": [opt.t.clone() for opt in (tr.g_opt, tr.d_opt)],
            "rng": tr.rng_state.clone()}


def restore_seeded_state(tr, snap):
    """Write seeded_state() back IN PLACE (the captured graphs keep their addresses), as tests/test_timed_path_gpu.py's
    _sync_trainers does.  The iteration counters (which updates run, the learning-rate decay) stay, so the step that follows does
    the work of any other timed step; Adam's own step counts restart with its empty slots, as in a first step.  Why: the
    statistics, filter-gradient and table-gradient sums add fp32 atomics in arrival order, and TF-Adam with beta1 = 0 turns the
    last-bit differences of ~0 gradients into whole steps, so after a few dozen iterations two runs of one build hold different
    weights.  From the seeded state, one step's outputs are a function of the arguments, up to rounding."""
    with torch.no_grad():
        for k, v in snap["vars"].items():
            tr.store.vars[k].copy_(v)
        for (net, key), v in snap["slots"].items():
            tr.store.flat[net][key].copy_(v)
        for opt, t in zip((tr.g_opt, tr.d_opt), snap["adam_t"]):
            opt.t.copy_(t)
        tr.rng_state.copy_(snap["rng"])
        for flat in (tr.g_flat, tr.d_flat):
            flat["grads_all"].zero_()
            flat["clean"] = True
    tr._refresh_g_prep()
    tr.sn_state_changed()           # the critic's weights and u were written behind the trainer's back


def dump_outputs(tr, out_dir):
    """What the timed path (SNGANTrainer.train_iteration) computed in its last step, as float32 DIR/<name>.npy: the two losses,
    the critic logits of the last critic update, the fakes the generator made for the step's critic updates and both networks'
    parameters after the updates (flat buffers in store order).  That step starts from the seeded state (restore_seeded_state)
    and takes the batches the step count selects from the seeded synthetic feed, so two builds run with the same arguments
    can be compared array for array."""
    import numpy as np
    arrays = {"d_loss": tr.d_loss, "g_loss": tr.g_loss, "critic_logits": tr.last_logits, "critic_fakes": tr.fake_all,
              "generator_params": tr.g_flat["params"], "discriminator_params": tr.d_flat["params"]}
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items() if v is not None}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise RuntimeError(f"--dump-outputs: {total} bytes exceed the {DUMP_LIMIT_BYTES}-byte limit")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def roofline_pass(tr, feed, rank):
    """--full: the roofline object of the result line (None on ranks other than 0)."""
    from gan_lib_tensorflow_amd import kernels as K
    graphs_used = tr.use_graphs
    # ---- roofline leg: one iteration executed eagerly with a HIP event pair around every MFMA conv launch.
    # EVERY rank runs the two eager iterations (they contain the gradient all-reduces: a rank that skipped them
    # would leave the others waiting in the collective); only rank 0 records and reports.
    roofline = None
    tr.use_graphs = False
    tr.train_iteration(feed)          # untimed eager warm-up of the non-graph path
    torch.cuda.synchronize()
    if rank == 0:
        K.prof_reset()
        K.prof_enable(True)
    tr.train_iteration(feed)
    torch.cuda.synchronize()
    if rank == 0:
        K.prof_enable(False)
        fam = {}
        alg_bytes = {}
        for f, name in ((0, "conv_igemm_kernel (fprop+dgrad)"), (1, "conv_wgrad_kernel")):
            n, ms, fl = K.prof_collect(f)
            fam[name] = (n, ms, fl)
            alg_bytes[name] = K.prof_bytes(f)
        # the dominant KERNEL (one symbol, as rocprofv3 lists it) over both conv families, by total time
        kernels = [(nm, n_, ms_, fl_, by_, fname) for f, fname in ((0, "conv_igemm_kernel (fprop+dgrad)"), (1, "conv_wgrad_kernel"))
                   for nm, n_, ms_, fl_, by_ in K.prof_kernels(f)]
        K.prof_reset()
        pair_us = 1e3 * K.prof_calibrate(200)      # what an event pair around an EMPTY kernel reads
        # Ranked on event totals LESS the event-pair floor per launch: that fixed cost (an empty kernel reads ~7.5 us)
        # is not kernel time, and with it a 46-launch 10-us kernel outranks the 200-us one that rocprofv3's kernel-only
        # durations (profiles/) put first.  `achieved` below still uses the raw event time of the chosen kernel.
        kernels.sort(key=lambda t: -(t[2] - t[1] * pair_us * 1e-3))
        dom, n, ms, fl, by, dom_family = kernels[0]
        achieved = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        # HBM traffic per launch: rocprofv3 PMC passes cannot run inside this process; the committed measurement of
        # scratch/pmc_bench_traffic.sh over this same workload is reported when it covers the dominant kernel
        traffic, traffic_src, tj = None, None, None
        import glob
        for tpath in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")), reverse=True):   # latest round first
            cand = json.load(open(tpath))
            traffic = traffic_per_launch(cand, dom)
            if traffic is not None:
                tj = cand                      # only a file that covers the dominant kernel feeds the ratios below
                traffic_src = f"profiles/{os.path.basename(tpath)} (" + tj["method"] + ")"
                break
        roofline = {"bound": "mfma", "kernel": dom, "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_TFLOPS, 4), "traffic": traffic,
                    "traffic_unit": "HBM bytes per launch", "traffic_source": traffic_src,
                    "algorithmic_bytes_per_launch": round(by / max(n, 1)),
                    "launches_per_iteration": n, "avg_launch_us": round(1e3 * ms / max(n, 1), 2),
                    # an event pair reads the kernel plus a fixed few microseconds (measured on an empty kernel,
                    # whose own run time is part of it): rocprofv3's kernel-only durations are shorter by about that
                    "event_pair_floor_us": round(pair_us, 2),
                    "avg_launch_gflop": round(fl / max(n, 1) / 1e9, 3),
                    "conv_gflop_per_iteration_as_run": round(sum(v[2] for v in fam.values()) / 1e9, 1),
                    "families": {k: {"launches": v[0], "ms": round(v[1], 3),
                                     "tflops": round(v[2] / (v[1] * 1e-3) / 1e12, 2) if v[1] > 0 else 0.0} for k, v in fam.items()},
                    "kernels": [{"kernel": t[0], "launches": t[1], "ms": round(t[2], 3),
                                 "tflops": round(t[3] / (t[2] * 1e-3) / 1e12, 1) if t[2] > 0 else 0.0} for t in kernels[:8]],
                    # every conv kernel of the iteration: measured HBM bytes per launch (the committed PMC passes) over its
                    # algorithmic bytes (operands read once + result written once, summed by the launchers)
                    "traffic_ratio": {t[0]: round(tr_b / (t[4] / max(t[1], 1)), 2) for t in kernels
                                      for tr_b in [traffic_per_launch(tj, t[0]) if tj else None] if tr_b and t[4] > 0}}
        # the same over ALL conv launches of the iteration: a kernel's PMC bytes include dirty lines of its predecessors that
        # the L2 / Infinity Cache evict while it runs, so only the sum is attribution-free
        cov = [(traffic_per_launch(tj, t[0]) if tj else None, t) for t in kernels]
        cov = [(b, t) for b, t in cov if b and t[4] > 0]
        if cov:
            roofline["traffic_ratio_all_conv_kernels"] = round(sum(b * t[1] for b, t in cov) / sum(t[4] for _, t in cov), 3)
    tr.use_graphs = graphs_used            # every rank (the eager roofline pass above switched it off)
    return roofline


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)     # ~1 s timed: long enough for clocks to settle
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-graphs", action="store_true")
    ap.add_argument("--strong", action="store_true",
                    help="strong scaling (the reference's semantics, gan_cifar_resnet.py:324,330): the global batch of 64 is split over the ranks")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for --gpus > 1 (nccl = RCCL; gloo for rehearsals)")
    ap.add_argument("--force-dp", action="store_true",
                    help="one GPU, but through the data-parallel path: a world-size-1 RCCL group, bucketed generator gradients on the "
                         "communication stream, the all-reduces captured inside the update graphs -- what N > 1 ranks run, minus the wire")
    ap.add_argument("--grad-wire", default=None, choices=[None, "bf16"], help="16-bit gradient buckets on the wire (data parallel)")
    ap.add_argument("--no-capture-collectives", action="store_true", help="data parallel: collectives eagerly between graph replays (the round-2 form)")
    ap.add_argument("--capture-collectives", action="store_true",
                    help="data parallel, world > 1: RCCL all-reduces INSIDE the update graphs (default there: between graphs, until a "
                         "multi-GPU run has verified replayed collectives; a world-size-1 group captures by default)")
    ap.add_argument("--no-other-configs", action="store_true", help="skip the ACGAN / PGGAN / Pix2Pix step times behind the headline line (key other_configs)")
    ap.add_argument("--no-fp16", action="store_true", help="skip the fp16 child process (key fp16)")
    ap.add_argument("--set", action="append", default=[], metavar="module.NAME=value",
                    help="A/B runs: set a module constant of the package before the trainer is built, e.g. functional.RES8_CONV=False")
    ap.add_argument("--full", action="store_true",
                    help="after the headline: the roofline pass, the CPU baseline, the fp16 child and the other configurations "
                         "(keys roofline, whole_step_mfma_frac_as_run, cpu_baseline, fp16, other_configs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32, rank 0); that step starts from the seeded state")
    args = ap.parse_args()
    for kv in args.set:
        import ast
        import importlib
        target, value = kv.split("=", 1)
        modname, attr = target.rsplit(".", 1)
        mod = importlib.import_module("gan_lib_tensorflow_amd." + modname)
        if not hasattr(mod, attr):
            raise SystemExit(f"--set {kv}: gan_lib_tensorflow_amd.{modname} has no {attr}")
        setattr(mod, attr, ast.literal_eval(value))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    extras = args.full and world == 1 and not args.set and not args.no_graphs and not args.force_dp and os.environ.get("GANK_DTYPE", "bf16").lower() == "bf16" \
        and "GANK_LIB_NAME" not in os.environ and os.environ.get("GANK_BENCH_EXTRAS", "1") != "0"      # (measurement scripts: headline only)
    fp16 = None
    if extras and not args.no_fp16:
        fp16 = fp16_child(min(args.steps, 100), min(max(args.warmup, 2), 10))       # before this process touches the GPU
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {args.gpus}"
                         " (one rank per GPU)")
    if local_rank >= torch.cuda.device_count():     # rehearsal of the N > 1 path on fewer GPUs than ranks (gloo only)
        assert args.backend != "nccl", "RCCL needs one GPU per rank"
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    rccl_log = None
    if world > 1 and args.backend == "nccl":
        # which algorithm / protocol / channel count RCCL picks over the xGMI mesh is part of the result: log the
        # communicator setup (not every collective) and summarise it in the JSON line
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        rccl_log = os.path.join(ROOT, "gpurun_out", f"rccl_n{world}_rank{rank}.log")
        os.environ.setdefault("NCCL_DEBUG", "INFO")
        os.environ.setdefault("NCCL_DEBUG_SUBSYS", "INIT,GRAPH,TUNING")
        os.environ.setdefault("NCCL_DEBUG_FILE", rccl_log)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    from gan_lib_tensorflow_amd import kernels as K
    from gan_lib_tensorflow_amd import parallel
    from gan_lib_tensorflow_amd.SNGAN import gan_cifar_resnet as S
    pg, rank, world = parallel.init_from_env(backend=args.backend, device=device, force=args.force_dp)   # nccl = RCCL over xGMI; None for 1 rank

    per_gpu = S.BATCH_SIZE // world if args.strong else S.BATCH_SIZE
    assert per_gpu >= 2 and per_gpu * world == (S.BATCH_SIZE if args.strong else S.BATCH_SIZE * world), "batch 64 must split evenly"
    # allow_eager_fallback: a capture failure on SOME ranks must not leave the others waiting in a collective -- every rank
    # finishes its warm-up, then all of them agree (MIN over ranks) whether to go on
    tr = S.SNGANTrainer(batch_size=per_gpu, device=device, seed=0, use_graphs=not args.no_graphs, process_group=pg,
                        allow_eager_fallback=True, capture_collectives=(False if args.no_capture_collectives else True if args.capture_collectives else None), grad_wire_dtype=args.grad_wire)
    feed = S.synthetic_batches(per_gpu, device, seed=rank)
    seeded = seeded_state(tr) if args.dump_outputs else None

    def barrier():
        if world > 1:
            import torch.distributed as dist
            dist.barrier(group=pg)
        torch.cuda.synchronize()

    warm = max(args.warmup, 2)    # iterations 0 and 1 run eagerly and capture the D and G graphs
    for _ in range(warm):
        tr.train_iteration(feed)
    graphs_ok = torch.tensor([1 if (args.no_graphs or tr.use_graphs) else 0], dtype=torch.int32, device=device)
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(graphs_ok, op=dist.ReduceOp.MIN, group=pg)
    if not int(graphs_ok.item()):
        # capture fell back to eager execution during warm-up (on at least one rank): a line that says "graphs" must not
        # describe eager runs.  Every rank takes this branch together and tears its process group down.
        if world > 1:
            dist.destroy_process_group()
        print("[bench] hipGraph capture failed during warm-up; refusing to report an eager run as a graph run "
              "(use --no-graphs to measure eager execution)", file=sys.stderr, flush=True)
        sys.exit(3)
    barrier()
    # per-step HIP events on the launch stream (graph replays and eager kernels both go to torch's current stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    starts = ev[:-1]
    t0 = time.perf_counter()
    ev[0].record()
    for i in range(args.steps):
        if seeded is not None and i == args.steps - 1:
            # --dump-outputs: the last step starts from the seeded state (restore_seeded_state); the restore is not timed
            torch.cuda.synchronize()
            t_restore = time.perf_counter()
            restore_seeded_state(tr, seeded)
            torch.cuda.synchronize()
            t0 += time.perf_counter() - t_restore
            starts[i] = torch.cuda.Event(enable_timing=True)
            starts[i].record()
        tr.train_iteration(feed)
        ev[i + 1].record()
    torch.cuda.synchronize()
    t_local = time.perf_counter() - t0
    barrier()
    step_ms = sorted(starts[i].elapsed_time(ev[i + 1]) for i in range(args.steps))
    median_ms = step_ms[len(step_ms) // 2]
    graphs_used = bool(tr.use_graphs)
    t = torch.tensor([t_local], dtype=torch.float64, device=device)
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=pg)
    elapsed = float(t)
    finite = bool(torch.isfinite(tr.g_flat["params"]).all() and torch.isfinite(tr.d_flat["params"]).all())
    if args.dump_outputs and rank == 0:
        dump_outputs(tr, args.dump_outputs)     # before the roofline pass, whose eager iterations move the state on

    roofline = roofline_pass(tr, feed, rank) if args.full else None

    if rank == 0:
        images = 5.0 * per_gpu * world * args.steps
        value = images / elapsed
        out = {
            # images = real images through the critic: 5 critic batches of 64 per step (and per GPU)
            "metric": "images/sec (G+D step) SNGAN-ResNet CIFAR-10 bs=64", "value": round(value, 2), "unit": "images/sec",
            "n_gpus": world, "steps": args.steps, "warmup": warm, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
            "median_ms_per_step_hip_events": round(median_ms, 3), "min_ms_per_step_hip_events": round(step_ms[0], 3),
            "higher_is_better": True, "scaling": "strong" if args.strong else "weak", "vs_baseline": None, "dtype": os.environ.get("GANK_DTYPE", "bf16").lower(), "data": "synthetic",
            "config": {"workload": "SNGAN ResNet CIFAR-10 32x32 bs=64 hinge: 1 G update (2x64 fakes) + 5 D updates (64 real + 64 fake) per step",
                       "global_batch": per_gpu * world, "per_gpu_batch": per_gpu, "parallelism": f"dp{world}",
                       "images_per_step": "5 critic batches x 64 real images per GPU",
                       "graphs": graphs_used, "finite": finite,
                       "data_parallel_path": bool(pg is not None), "collectives_in_graphs": bool(pg is not None and tr.capture_collectives),
                       "grad_wire": args.grad_wire or "fp32"},
            # reference algorithm (9-tap upsample convs, SURVEY 8d: 13.77 GFLOP per real image) and the algorithm as run
            # (UpsampleConv 3x3 as a 4-tap-per-output transposed conv; conv FLOPs counted by the kernels themselves)
            "whole_step_mfma_frac": round(value / world * GFLOP_PER_REAL_IMAGE * 1e9 / (PEAK_BF16_TFLOPS * 1e12), 4),
            "whole_step_mfma_frac_as_run": (round(roofline["conv_gflop_per_iteration_as_run"] * 1e9 * (value / world / (5.0 * per_gpu))
                                                  / (PEAK_BF16_TFLOPS * 1e12), 4) if roofline else None),
            "roofline": roofline,
        }
        if rccl_log and os.path.exists(rccl_log):
            import re
            txt = open(rccl_log, errors="replace").read()
            out["config"]["rccl"] = {
                "log": os.path.relpath(rccl_log, ROOT),
                "version": (re.findall(r"(?:RCCL|NCCL) version ([^\s]+)", txt) or [None])[0],
                "channels": sorted(set(re.findall(r"(\d+) coll channels", txt))),
                "rings_or_trees": sorted(set(re.findall(r"\b(Ring|Tree|CollNet|NVLS|PAT)\b", txt))),
                "xgmi_or_p2p_lines": len(re.findall(r"via P2P|XGMI|xGMI", txt)),
                "gradient_exchange": "generator: 4 fp32 buckets (G.OutputNorm+G.Output, G.Block.3, G.Block.2, G.Input+G.Block.1) all-reduced "
                                     "on a communication stream beside the segmented backward pass; critic: one fp32 all-reduce of 6.8 MB per update",
            }
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        else:
            out["cpu_baseline"] = None
        if fp16 is not None:
            out["fp16"] = fp16
        if extras and not args.no_other_configs:
            del tr, feed
            import gc
            gc.collect()
            torch.cuda.synchronize()
            out["other_configs"] = other_configs()
            tr = feed = None
        print(json.dumps(out), flush=True)
    if pg is not None:
        # ordered teardown: the captured graphs (they may hold collective nodes) and the bucket views go before the communicator,
        # and nothing is in flight when it is destroyed
        import gc
        import torch.distributed as dist
        del tr, feed
        gc.collect()
        torch.cuda.synchronize()
        dist.barrier(group=pg)
        torch.cuda.synchronize()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
