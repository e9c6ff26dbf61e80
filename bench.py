#!/usr/bin/env python3
"""bench.py -- images/sec of the fused int8 conv3x3+relu+conv1x1(+relu) block.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload res2a] [--dst s32]
                    [--full] [--dump-outputs DIR]

A "step" is one pass of the hot path (one dfx_conv_submit) over one batch of
synthetic input already resident in HBM.  Default workload = BASELINE.json
configs[2], the configuration the metric is quoted on: ResNet-50 res2a-style
block, N=128 per GPU, 56x56, 64->64->256, u8 x s8, s32 output.  With N>1 GPUs
(launched by torch.distributed.run, one rank per GPU) every rank processes its
own 128 images -- images are independent, so the conv path has no collective --
and the value is the whole-job aggregate ("scaling": "weak").  The RCCL
all-gather + op_concat exchange of configs[3] is measured after the timed region
(with --full) and reported beside it (key "concat_allgather"), never inside `value`.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps,
writes the last step's output if asked (--dump-outputs) and prints the line:
  roofline     dominant kernel vs its binding roof (HBM for s32/f32 output),
               achieved = algorithmic bytes per launch / mean launch duration
               measured with HIP events on the launching stream
Everything else runs after the timed region only with --full:
  cpu_baseline the CPU oracle's AVX-512-VNNI/OpenMP port (or its scalar OpenMP
               form) timed on this host's cores on a bounded sample; the oracle
               output of that sample also checks what the timed path wrote
  u8_out       the default workload's block with 1-byte output (and a second
               conv1 scale), timed and checked the same way
  concat_allgather  (N > 1) the configs[3] exchange

--dump-outputs DIR writes what the last timed step computed as DIR/dst.npy
(float64 for s32 output, float32 otherwise; outputs over DUMP_BYTES as a fixed
seeded sample of flat indices).  Inputs are seeded, so two builds run with the
same arguments can be compared output for output.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured copy)
INT8_PEAK_TOPS = 5033.0    # dense: 2048 op/clk/SIMD (v_mfma_i32_32x32x32_i8 in 32 clk) x 1024 SIMDs x 2.4 GHz
DUMP_BYTES = 48 << 20      # --dump-outputs: largest file written whole (the option promises at most 64 MB in all)
DUMP_SEED = 20240607       # --dump-outputs: fixed seed of the sample of a larger output


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def dump_output(dirname, name, t):
    """Write tensor `t` (what the timed path handed its caller) as dirname/<name>.npy: float64 for
    32-bit integers (exact), float32 for the 1-byte types and f32.  An output larger than DUMP_BYTES
    is written as its values at a sorted sample of flat indices drawn with DUMP_SEED: the sample depends
    on the output's size only, so runs with the same arguments write the same elements.  Returns what
    was written, for the result line."""
    import torch
    f64 = t.dtype == torch.int32
    es = 8 if f64 else 4
    n = t.numel()
    desc = {"file": name + ".npy", "dtype": "float64" if f64 else "float32", "shape": list(t.shape)}
    if n * es <= DUMP_BYTES:
        vals = t.cpu().numpy()
    else:
        idx = np.unique(np.random.default_rng(DUMP_SEED).integers(0, n, DUMP_BYTES // es))
        vals = t.reshape(-1)[torch.from_numpy(idx).to(t.device)].cpu().numpy()
        desc["sample"] = "%d of %d elements at sorted flat indices np.unique(default_rng(%d).integers(0, %d, %d))" % (
            idx.size, n, DUMP_SEED, n, DUMP_BYTES // es)
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, name + ".npy"), vals.astype(np.float64 if f64 else np.float32))
    return desc


def workloads():
    import cases as C
    return {
        # name: (case at per-GPU batch, description)
        "res2a": (C.ConvCase("res2a", 128, 64, 56, 56, 64, 256, dst_dt=C.S32),
                  "BASELINE configs[2]: N=128 56x56 64->64->256 u8xs8"),
        "vgg": (C.ConvCase("vgg", 64, 64, 224, 224, 64, 128, dst_dt=C.F32),
                "BASELINE configs[4]: N=64 224x224 64->64->128 u8xs8"),
        "bringup": (C.ConvCase("bringup", 1, 32, 28, 28, 32, 64, dst_dt=C.U8),
                    "BASELINE configs[1]: N=1 28x28 32->32->64 u8xs8"),
        # SURVEY 8(f) rank 3 (general shapes, streamed-weight MFMA kernel): deeper ResNet-50 stages
        "res3": (C.ConvCase("res3", 128, 128, 28, 28, 128, 512, dst_dt=C.U8),
                 "ResNet-50 res3-style block: N=128 28x28 128->128->512 u8xs8"),
        "res4": (C.ConvCase("res4", 128, 256, 14, 14, 256, 1024, dst_dt=C.U8),
                 "ResNet-50 res4-style block: N=128 14x14 256->256->1024 u8xs8"),
        "res5": (C.ConvCase("res5", 128, 512, 7, 7, 512, 2048, dst_dt=C.U8),
                 "ResNet-50 res5-style block: N=128 7x7 512->512->2048 u8xs8"),
        "pw256": (C.ConvCase("pw256", 128, 256, 56, 56, 64, 0, k=(1, 1), pad=(0, 0), dst_dt=C.U8),
                  "ResNet-50 res2 reduce-style unfused 1x1 conv: N=128 56x56 256->64 u8xs8"),
        "pw1024": (C.ConvCase("pw1024", 128, 1024, 14, 14, 256, 0, k=(1, 1), pad=(0, 0), dst_dt=C.U8),
                   "ResNet-50 res4 reduce-style unfused 1x1 conv: N=128 14x14 1024->256 u8xs8"),
        "vgg3": (C.ConvCase("vgg3", 64, 256, 56, 56, 256, 0, dst_dt=C.U8),
                 "VGG conv3-style unfused conv: N=64 56x56 256->256 u8xs8"),
        "vgg5": (C.ConvCase("vgg5", 64, 512, 14, 14, 512, 0, dst_dt=C.U8),
                 "VGG conv5-style unfused conv: N=64 14x14 512->512 u8xs8"),
        "vggpool": (C.ConvCase("vggpool", 64, 64, 224, 224, 64, 0, dst_dt=C.U8),
                    "VGG conv1_2-style unfused conv: N=64 224x224 64->64 u8xs8 (with --fuse-pool: + relu + 2x2/2 max pool, "
                    "the reference's roadmap op, test_conv_relu_pooling.cc:315-316)"),
        "res3s2": (C.ConvCase("res3s2", 128, 128, 56, 56, 128, 512, stride=(2, 2), dst_dt=C.U8),
                   "ResNet-50 res3a-style stride-2 block: N=128 56x56 128->128->512 s2 u8xs8"),
    }


def cpu_baseline(case, data, threads, gpu_out, budget_s=12.0, fuse_pool=0, max_images=32):
    """Oracle port timed on the host cores on a bounded sample of the workload.  This leg
    is the only place bench.py touches oracle/: it also uses the sample's oracle output as
    the checker of what the timed GPU path wrote (never as something measured or shipped)."""
    from dataclasses import replace
    from oracle import oracle as orc
    import hipref
    orc.set_num_threads(threads)
    impl = "avx512" if orc.have_avx512_vnni() else "scalar_mt"
    n = min(case.bs, max_images if impl == "avx512" else 4, len(gpu_out))
    sub = dict(data, src=data["src"][:n])
    c = replace(case, bs=n)
    def run_oracle():
        r = hipref.oracle_conv(orc, c, sub, impl)
        return orc.maxpool(r, (2, 2), (2, 2), (0, 0), (r.shape[1] // 2, r.shape[2] // 2)) if fuse_pool else r
    ref = run_oracle()                                        # warm-up + checker
    hipref.assert_bit_equal(gpu_out[:n], ref, "bench output vs oracle")
    t0 = time.perf_counter()
    reps = 0
    while True:
        run_oracle()
        reps += 1
        el = time.perf_counter() - t0
        if el > budget_s or reps >= 100:
            break
    cpu_model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            cpu_model = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), "unknown")
    except OSError:
        pass
    return {"value": round(n * reps / el, 2), "unit": "images/sec", "cores": orc.num_threads(),
            "cpu_model": cpu_model, "host_cpus": os.cpu_count(),
            "kind": "port", "gpu_output_matches_oracle": True,
            "sample": "%d images x %d reps of the same workload, oracle impl=%s (%s)" % (
                n, reps, impl,
                "AVX-512 VNNI intrinsics mirroring the reference JIT, OpenMP over (n,oh)"
                if impl == "avx512" else "scalar C, OpenMP over (n,oh)")}


def socket_cores():
    """(physical cores of socket 0, CPUs this process may run on): the second cpu_baseline leg runs on one
    full socket's physical cores, or on as many as the box lets this process use"""
    cores = set()
    try:
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for l in f:
                if l.startswith("physical id"):
                    phys = int(l.split(":")[1])
                elif l.startswith("core id"):
                    core = int(l.split(":")[1])
                elif not l.strip():
                    if phys == 0 and core is not None:
                        cores.add(core)
                    phys = core = None
    except (OSError, ValueError):
        pass
    try:
        usable = len(os.sched_getaffinity(0))
    except AttributeError:
        usable = os.cpu_count() or 1
    return (len(cores) or usable), usable


def calibrated_peak(hbm_bound):
    """measured roofs of the gpurun MI355X (write stream in the kernel's store shape; back-to-back
    int8 MFMA), see profiles/calibration.json; None if the file is missing"""
    try:
        with open(os.path.join(ROOT, "profiles", "calibration.json")) as f:
            c = json.load(f)
        return float(c["hbm_write_GBps"] if hbm_bound else c["int8_mfma_TOPs"])
    except (OSError, KeyError, ValueError):
        return None


def load_traffic(workload, dst):
    """HBM bytes per launch from the COMMITTED rocprofv3 PMC passes of this workload (profiles/traffic.json,
    collected with profiles/collect_pmc.sh), or None.  Counters of an earlier profiled run of the same
    command, not of this run: the line says so in roofline.traffic_source."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        t = json.load(open(path))
        return t.get("%s-%s" % (workload, dst))
    except Exception:
        return None


TRAFFIC_SOURCE = ("profiles/traffic.json: (2*FETCH_SIZE + WRITE_SIZE) of separate rocprofv3 --pmc passes of this "
                  "command (profiles/collect_pmc.sh); a committed profile, not counters of this run")


def cpu_grant():
    """what the box lets this process use: CPUs in the affinity mask and the cgroup CPU quota (CPUs' worth of
    time per period; None = unlimited / unreadable)"""
    try:
        nproc = len(os.sched_getaffinity(0))
    except AttributeError:
        nproc = os.cpu_count() or 1
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:           # cgroup v2: "<quota|max> <period>"
            q, per = f.read().split()[:2]
            quota = None if q == "max" else round(int(q) / int(per), 2)
    except (OSError, ValueError):
        try:                                                # cgroup v1
            with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
                q = int(f.read())
            with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
                per = int(f.read())
            quota = None if q <= 0 else round(q / per, 2)
        except (OSError, ValueError):
            pass
    return nproc, quota


def launch_ranks(n):
    """`python bench.py --gpus N` without torchrun: run N ranks as children of
    `python -m torch.distributed.run` (one per GPU, rendezvous on 127.0.0.1), relay what they
    print (rank 0 prints the JSON line) and return their exit status."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("bench.py: launching %d ranks: %s" % (n, " ".join(cmd)))
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="res2a")
    ap.add_argument("--dst", default=None, help="override dst dtype: u8|s8|s32|f32")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also run the CPU baseline and oracle check, the u8-output leg of "
                         "the default workload and (N > 1) the all-gather + concat exchange")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32/float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-u8-out", action="store_true", help="with --full: skip the u8-output leg of the default workload")
    ap.add_argument("--fuse-pool", action="store_true",
                    help="unfused conv workloads: 2x2/2 max pooling fused into the conv kernel (conv+relu+pool roadmap op)")
    ap.add_argument("--device-ramp-ms", type=float, default=150.0,
                    help="untimed set-up launches for this long before the warm-up steps (GPU clock ramp); 0 = off")
    ap.add_argument("--launch-stats", type=int, default=0,
                    help="after the timed region, time N more launches one by one and report min/median/p90")
    ap.add_argument("--variant", type=int, default=-1, help="-1 auto, 0 generic, 1/2 resident-weight mfma, 3 streamed-weight mfma")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="OpenMP threads of the CPU baseline (default: min(host cpus, 16) = one GPU's CPU share)")
    ap.add_argument("--rehearse-launch", action="store_true",
                    help="testing aid: stop right after the process group is up (exercises the --gpus N "
                         "launcher and rendezvous without touching a GPU; with DFX_BENCH_BACKEND=gloo)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    # ---- N > 1 typed as `python bench.py --gpus N`: start the ranks ourselves.  Decided BEFORE
    #      torch is imported or any HIP call is made: the parent never touches the GPU, the ranks
    #      are fresh child processes (never an exec of a process that initialised the GPU). ----
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch_ranks(args.gpus))
    world = int(env_world or "1")
    if world != args.gpus:
        log("bench.py: WORLD_SIZE=%d but --gpus %d; launch with --nproc-per-node %d or drop WORLD_SIZE"
            % (world, args.gpus, args.gpus))
        sys.exit(2)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))

    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        backend = os.environ.get("DFX_BENCH_BACKEND", "nccl")   # "gloo": rehearsal of the N>1 path
        if backend == "nccl":
            local_rank = local_rank % max(torch.cuda.device_count(), 1)
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
            if not args.rehearse_launch:
                torch.cuda.set_device(local_rank % max(torch.cuda.device_count(), 1))
    if args.rehearse_launch:
        if world > 1:
            t = torch.tensor([float(rank)])
            dist.all_reduce(t)
            dist.barrier()
            total = float(t[0])
        else:
            total = 0.0
        if rank == 0:
            print(json.dumps({"rehearsal": True, "n_gpus": world, "rank_sum": total,
                              "backend": os.environ.get("DFX_BENCH_BACKEND", "nccl")}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return
    if world == 1:
        torch.cuda.set_device(0)

    import cases as C
    import hipref
    dfa = importlib.import_module("deep-fusion_amd")
    from dataclasses import replace

    if args.workload == "concat":
        return bench_concat(args, torch, dist, dfa, C, world, rank)

    case, desc = workloads()[args.workload]
    if args.dst:
        case = replace(case, dst_dt={"u8": C.U8, "s8": C.S8, "s32": C.S32, "f32": C.F32}[args.dst])
    dst_name = C.NAME_OF[case.dst_dt]
    case = replace(case, seed=1234 + rank)
    data = C.generate(case)

    op = hipref.make_conv(case, data, force_variant=args.variant, fuse_pool=2 if args.fuse_pool else 0)
    info = op.info()
    tdt = {C.F32: torch.float32, C.S32: torch.int32, C.S8: torch.int8, C.U8: torch.uint8}[case.dst_dt]
    # rotate over a few src/dst pairs so no step is served from the 256 MiB Infinity Cache
    dst_bytes = int(np.prod(op.dst_shape)) * torch.empty(0, dtype=tdt).element_size()
    nbuf = max(2, min(4, int(1.5e9 // max(dst_bytes, 1))))
    srcs = [torch.from_numpy(np.roll(data["src"], i, axis=0)).cuda() for i in range(nbuf)]
    dsts = [torch.empty(op.dst_shape, dtype=tdt, device="cuda") for _ in range(nbuf)]

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    # device ramp (set-up, reported as config.device_ramp_ms): a freshly started process finds the GPU in a low
    # power state, and the W warm-up steps of a short run (the driver uses W=5: 0.4 ms) end before the clocks are
    # up -- the same launches measure 2-3 % slower there than a few hundred launches later.  Untimed; the W
    # warm-up steps and the K timed steps follow unchanged.
    ramp_t0 = time.perf_counter()
    i = 0
    while args.device_ramp_ms > 0 and (time.perf_counter() - ramp_t0) * 1e3 < args.device_ramp_ms:
        for _ in range(16):
            op.submit(srcs[i % nbuf], dsts[i % nbuf])
            i += 1
        torch.cuda.synchronize()
    for i in range(args.warmup):
        op.submit(srcs[i % nbuf], dsts[i % nbuf])
    barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(args.steps):
        op.submit(srcs[i % nbuf], dsts[i % nbuf])      # launches on torch's current stream
    e1.record()
    barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    kern_ms = e0.elapsed_time(e1) / args.steps        # mean launch duration, HIP events
    if world > 1:
        tt = torch.tensor([elapsed, kern_ms], dtype=torch.float64,
                          device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed, kern_ms = float(tt[0]), float(tt[1])

    extra = {}
    if args.dump_outputs and rank == 0:  # before anything else reuses the buffers
        extra["dump_outputs"] = [dump_output(args.dump_outputs, "dst", dsts[(args.steps - 1) % nbuf])]
    if args.launch_stats:  # outside the timed region: per-launch durations (their spread, not the mean)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.launch_stats)]
        for i, (a0, a1) in enumerate(evs):
            a0.record()
            op.submit(srcs[i % nbuf], dsts[i % nbuf])
            a1.record()
        torch.cuda.synchronize()
        ds = sorted(a0.elapsed_time(a1) for a0, a1 in evs)
        extra["launch_ms"] = {"n": len(ds), "min": round(ds[0], 5), "median": round(ds[len(ds) // 2], 5),
                              "p90": round(ds[int(len(ds) * 0.9)], 5), "max": round(ds[-1], 5)}
    # the same block with 1-byte output: the variant north_star's ">= 40 % of int8-MFMA peak" is about (the s32
    # headline is bound by its 411 MB output stream, cap 15.7 % of the MFMA peak).  Measured after the timed
    # region, same protocol (rotating buffers, HIP events on the launching stream), checked against the oracle.
    if args.full and args.workload == "res2a" and case.dst_dt == C.S32 and not args.no_u8_out:
        try:
            extra["u8_out"] = bench_u8_out(torch, hipref, C, case, data, args, world, dist, rank)
        except Exception as ex:  # never lose the main line
            extra["u8_out"] = {"error": repr(ex)[:300]}
    if world > 1:  # proof that N ranks ran: an all-reduce of ones over the job's own backend
        ones = torch.ones(1, dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(ones)
        extra["ranks_seen"] = int(round(float(ones[0])))
    else:
        extra["ranks_seen"] = 1
    # configs[3]: op_concat + RCCL all-gather, measured outside the timed region
    if args.full and world > 1 and dist.get_backend() == "nccl":
        try:
            extra["concat_allgather"] = bench_concat_allgather(dfa, torch, dist, dsts[0], world, rank)
        except Exception as ex:  # never lose the main line
            extra["concat_allgather"] = {"error": repr(ex)[:200]}

    if rank == 0:
        images = case.bs * world * args.steps
        value = images / elapsed
        alg_bytes, alg_ops = int(info.algorithmic_bytes), int(info.algorithmic_ops)
        achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
        tops = alg_ops / (kern_ms * 1e-3) / 1e12
        hbm_bound = case.dst_dt in (C.S32, C.F32)
        out = {
            "metric": "fused conv3x3+relu+conv1x1 int8 images/sec",
            "value": round(value, 1), "unit": "images/sec", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 5),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "u8*s8->s32 (int8 MFMA), f32 requant, %s out" % dst_name, "data": "synthetic",
            "config": {"workload": "%s (%s), %s out" % (args.workload, desc, dst_name),
                       "per_gpu_batch": case.bs, "global_batch": case.bs * world,
                       "parallelism": "batch-sharded x%d, no data-path collective" % world,
                       "device_ramp_ms": args.device_ramp_ms, "fuse_pool": bool(args.fuse_pool),
                       "full": bool(args.full),
                       "kernel": info.kernel_name.decode(), "grid": info.grid,
                       "split": False,  # one launch (the two-launch execution of small fused ops was removed in round 3)
                       "lds_bytes": info.lds_bytes, "rows_per_unit": info.rows_per_unit},
            "roofline": {"bound": "hbm" if hbm_bound else "mfma",
                         "achieved": round(achieved if hbm_bound else tops, 2),
                         "peak": HBM_PEAK_GBS if hbm_bound else INT8_PEAK_TOPS,
                         "unit": "GB/s" if hbm_bound else "TOP/s",
                         "frac": round((achieved / HBM_PEAK_GBS) if hbm_bound else (tops / INT8_PEAK_TOPS), 4),
                         "traffic": load_traffic(args.workload, dst_name),
                         "traffic_source": TRAFFIC_SOURCE if load_traffic(args.workload, dst_name) else None,
                         # nominal AND calibrated denominators (profiles/calibration.json)
                         "peak_calibrated": calibrated_peak(hbm_bound),
                         "frac_of_calibrated": round((achieved if hbm_bound else tops) / calibrated_peak(hbm_bound), 4)
                         if calibrated_peak(hbm_bound) else None,
                         "kernel_ms": round(kern_ms, 5),
                         "algorithmic_bytes_per_launch": alg_bytes,
                         "algorithmic_ops_per_launch": alg_ops,
                         "hbm_GBps": round(achieved, 2), "hbm_frac_of_8TBps": round(achieved / HBM_PEAK_GBS, 4),
                         "int8_TOPs": round(tops, 2), "mfma_frac_of_int8_peak": round(tops / INT8_PEAK_TOPS, 4)},
        }
        out.update(extra)
        if args.full and world == 1 and not args.no_cpu_baseline:
            gpu_head = dsts[0][:128].cpu().numpy()
            out["cpu_baseline"] = cpu_baseline(case, data, args.cpu_threads or min(os.cpu_count() or 1, 16), gpu_head,
                                               fuse_pool=args.fuse_pool)
            # second leg: more threads -- one socket's physical cores, or as many CPUs as this process may use.
            # Whether that is a "full socket" number depends on what the box grants: the affinity mask and the
            # cgroup CPU quota are printed next to it.
            sock, usable = socket_cores()
            nproc, quota = cpu_grant()
            n_wide = max(1, min(sock, usable))
            leg = cpu_baseline(case, data, n_wide, gpu_head, budget_s=8.0, fuse_pool=args.fuse_pool,
                               max_images=128)  # (a larger sample: 32 images do not feed that many threads)
            granted = min(nproc, quota) if quota else nproc
            out["cpu_baseline"]["nproc"] = nproc
            out["cpu_baseline"]["cgroup_cpu_quota"] = quota
            out["cpu_baseline"]["more_threads"] = {
                "value": leg["value"], "unit": leg["unit"], "cores": leg["cores"],
                "socket_physical_cores": sock, "nproc": nproc, "cgroup_cpu_quota": quota,
                "is_full_socket": bool(leg["cores"] >= sock and granted >= sock),
                "note": None if granted >= leg["cores"] else
                "the box grants this process about %s CPUs' worth of time: %d threads share them" % (granted, leg["cores"]),
                "sample": leg["sample"]}
        else:
            out["cpu_baseline"] = None
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def bench_u8_out(torch, hipref, C, case, data, args, world, dist, rank):
    """res2a block with u8 output, per rank; returns a roofline-shaped object (rank 0's view, launch time = max
    over ranks).  Algorithmic ops / bytes from dfx_conv_query."""
    from dataclasses import replace
    ucase = replace(case, dst_dt=C.U8)
    op = hipref.make_conv(ucase, data, force_variant=args.variant)
    info = op.info()
    nbuf = 4
    srcs = [torch.from_numpy(np.roll(data["src"], i, axis=0)).cuda() for i in range(nbuf)]
    dsts = [torch.empty(op.dst_shape, dtype=torch.uint8, device="cuda") for _ in range(nbuf)]
    steps = max(args.steps, 50)
    # the same untimed device ramp as the headline leg (config.device_ramp_ms): building this op's weights on the
    # host left the GPU idle long enough to drop its clocks -- without the ramp this leg read 35.7 us where the
    # same kernel measures 28.8 us as its own bench.py --dst u8 run (profiles/bench_r03_res2a_s32*.json)
    import time as _time
    ramp_t0 = _time.perf_counter()
    i = 0
    while args.device_ramp_ms > 0 and (_time.perf_counter() - ramp_t0) * 1e3 < args.device_ramp_ms:
        for _ in range(16):
            op.submit(srcs[i % nbuf], dsts[i % nbuf])
            i += 1
        torch.cuda.synchronize()
    for i in range(max(args.warmup, 20)):
        op.submit(srcs[i % nbuf], dsts[i % nbuf])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(steps):
        op.submit(srcs[i % nbuf], dsts[i % nbuf])
    e1.record()
    torch.cuda.synchronize()
    kern_ms = e0.elapsed_time(e1) / steps
    if world > 1:
        tt = torch.tensor([kern_ms], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        kern_ms = float(tt[0])
    checked = None
    if rank == 0 and not args.no_cpu_baseline:   # (the oracle is only ever the checker)
        from oracle import oracle as orc
        n = 8
        ref = hipref.oracle_conv(orc, replace(ucase, bs=n), dict(data, src=data["src"][:n]))
        hipref.assert_bit_equal(dsts[0][:n].cpu().numpy(), ref, "u8-out leg vs oracle")
        checked = "%d images bit-exact vs oracle" % n
    op.close()
    # The synthetic conv1 scale of this workload is a power of two (60 / (6 * 40 * sqrt(64)) = 2^-5), which admits
    # the role-specialised kernel's one-instruction "fma" requant route; an arbitrary scale takes the "magic" route
    # (one more vector instruction per output value).  Timed as well, so that the line does not rest on the lucky one.
    other = None
    try:
        data2 = dict(data, scales1=(data["scales1"] * np.float32(1.37)).astype(np.float32))
        op2 = hipref.make_conv(ucase, data2, force_variant=args.variant)
        ramp_t0 = _time.perf_counter()   # (building op2's weights on the host let the clocks drop again)
        i = 0
        while args.device_ramp_ms > 0 and (_time.perf_counter() - ramp_t0) * 1e3 < args.device_ramp_ms:
            for _ in range(16):
                op2.submit(srcs[i % nbuf], dsts[i % nbuf])
                i += 1
            torch.cuda.synchronize()
        for i in range(max(args.warmup, 20)):
            op2.submit(srcs[i % nbuf], dsts[i % nbuf])
        torch.cuda.synchronize()
        e0.record()
        for i in range(steps):
            op2.submit(srcs[i % nbuf], dsts[i % nbuf])
        e1.record()
        torch.cuda.synchronize()
        ms2 = e0.elapsed_time(e1) / steps
        if world > 1:
            tt = torch.tensor([ms2], dtype=torch.float64, device="cuda" if dist.get_backend() == "nccl" else "cpu")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            ms2 = float(tt[0])
        other = {"conv1_scale": "x 1.37 (not a power of two)", "kernel": op2.info().kernel_name.decode(),
                 "kernel_ms": round(ms2, 5),
                 "frac": round(int(info.algorithmic_ops) / (ms2 * 1e-3) / 1e12 / INT8_PEAK_TOPS, 4)}
        op2.close()
    except Exception as e:  # (never lose the headline line over the extra leg)
        other = {"error": str(e)[:200]}
    ops, byts = int(info.algorithmic_ops), int(info.algorithmic_bytes)
    tops = ops / (kern_ms * 1e-3) / 1e12
    gbs = byts / (kern_ms * 1e-3) / 1e9
    return {"bound": "mfma", "achieved": round(tops, 2), "peak": INT8_PEAK_TOPS, "unit": "TOP/s",
            "frac": round(tops / INT8_PEAK_TOPS, 4), "traffic": load_traffic("res2a", "u8"),
            "traffic_source": TRAFFIC_SOURCE if load_traffic("res2a", "u8") else None,
            "kernel_ms": round(kern_ms, 5), "steps": steps, "kernel": info.kernel_name.decode(),
            "images_per_sec_per_gpu": round(case.bs / (kern_ms * 1e-3), 1),
            "algorithmic_ops_per_launch": ops, "algorithmic_bytes_per_launch": byts,
            "hbm_GBps": round(gbs, 2), "hbm_frac_of_8TBps": round(gbs / HBM_PEAK_GBS, 4),
            # which roof binds this op: the larger of the two floor times.  With 1-byte output the block moves
            # 128.5 MB for 42.7 GOP = 333 op/B, below the ridge (int8 peak / HBM peak = 629 op/B): the HBM floor
            # is the higher one, and 40 % of the int8 peak would be 76 % of the HBM peak
            "floors_us": {"hbm": round(byts / (HBM_PEAK_GBS * 1e9) * 1e6, 2),
                          "mfma": round(ops / (INT8_PEAK_TOPS * 1e12) * 1e6, 2)},
            "binding_roof": "hbm" if byts / (HBM_PEAK_GBS * 1e9) > ops / (INT8_PEAK_TOPS * 1e12) else "mfma",
            "conv1_scale": "2^-5 (the synthetic workload's)", "other_scale": other,
            "checked": checked}


def bench_concat(args, torch, dist, dfa, C, world, rank):
    """--workload concat: the reference's default bench_concat case
    (/root/reference/benchmark/bench_concat.cc:226-242: {4,128,244,244}+{4,256,244,244}, post_relu)
    in --dst s8|s32|f32|u8 (default s8), device resident.  Rotates over enough src/dst sets that
    the working set exceeds the 256 MiB Infinity Cache.  HBM-bound: algorithmic bytes = read
    every input once + write dst once = 2 x dst bytes."""
    np_dt = {"s8": np.int8, "u8": np.uint8, "s32": np.int32, "f32": np.float32}[args.dst or "s8"]
    t_dt = {np.int8: torch.int8, np.uint8: torch.uint8, np.int32: torch.int32, np.float32: torch.float32}[np_dt]
    bs, h, w, chans = 4, 244, 244, [128, 256]
    es = np.dtype(np_dt).itemsize
    dst_bytes = bs * h * w * sum(chans) * es
    nbuf = max(3, int(np.ceil(600e6 / (2 * dst_bytes))) + 1)
    rng = np.random.default_rng(77 + rank)
    op = dfa.Concat(bs, h, w, chans, np_dt, True)
    sets = []
    for b in range(nbuf):
        if np_dt == np.float32:
            srcs = [torch.from_numpy(rng.standard_normal((bs, h, w, c)).astype(np.float32)).cuda() for c in chans]
        else:
            lo, hi = (0, 256) if np_dt == np.uint8 else (-100, 100)
            srcs = [torch.from_numpy(rng.integers(lo, hi, (bs, h, w, c)).astype(np_dt)).cuda() for c in chans]
        sets.append((srcs, torch.empty(op.dst_shape, dtype=t_dt, device="cuda")))

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    ramp_t0 = time.perf_counter()  # device ramp (set-up): see the conv path above
    i = 0
    while args.device_ramp_ms > 0 and (time.perf_counter() - ramp_t0) * 1e3 < args.device_ramp_ms:
        for _ in range(16):
            op.submit(*sets[i % nbuf])
            i += 1
        torch.cuda.synchronize()
    for i in range(args.warmup):
        op.submit(*sets[i % nbuf])
    barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for i in range(args.steps):
        op.submit(*sets[i % nbuf])
    e1.record()
    barrier()
    elapsed = time.perf_counter() - t0
    kern_ms = e0.elapsed_time(e1) / args.steps
    if world > 1:
        tt = torch.tensor([elapsed, kern_ms], dtype=torch.float64,
                          device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed, kern_ms = float(tt[0]), float(tt[1])
    # with --full: checker + CPU baseline (oracle = restatement of op_concat.cc:22-72, pinned by test_concat.cc:31-87)
    cpu = None
    dumped = None
    if rank == 0 and args.dump_outputs:
        dumped = [dump_output(args.dump_outputs, "dst", sets[(args.steps - 1) % nbuf][1])]
    if rank == 0 and args.full:
        from oracle import oracle as orc
        srcs, dst = sets[(args.steps - 1) % nbuf]
        h_srcs = [s_.cpu().numpy() for s_ in srcs]
        ref = orc.concat(h_srcs, True)
        got = dst.cpu().numpy()
        assert np.array_equal(got.view(np.uint8), ref.view(np.uint8)), "concat output differs from the oracle"
        if world == 1 and not args.no_cpu_baseline:
            t1 = time.perf_counter()
            reps = 0
            while time.perf_counter() - t1 < 5.0 and reps < 50:
                orc.concat(h_srcs, True)
                reps += 1
            el = time.perf_counter() - t1
            cpu = {"value": round(bs * reps / el, 2), "unit": "images/sec", "cores": 1, "kind": "port",
                   "sample": "%d reps of the same {4,384,244,244} concat+relu, scalar C oracle" % reps}
    if rank == 0:
        achieved = 2 * dst_bytes / (kern_ms * 1e-3) / 1e9
        out = {"metric": "concat+relu images/sec", "value": round(bs * world * args.steps / elapsed, 1),
               "unit": "images/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
               "ms_per_step": round(elapsed / args.steps * 1e3, 5), "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": np.dtype(np_dt).name, "data": "synthetic",
               "config": {"workload": "concat+relu {4,128,244,244}+{4,256,244,244} NHWC %s "
                                      "(reference benchmark/bench_concat.cc:226-242)" % np.dtype(np_dt).name,
                          "buffer_sets_rotated": nbuf, "working_set_bytes": 2 * dst_bytes * nbuf,
                          "device_ramp_ms": args.device_ramp_ms, "full": bool(args.full)},
               "roofline": {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": round(achieved / HBM_PEAK_GBS, 4),
                            "traffic": load_traffic("concat", np.dtype(np_dt).name),
                            "traffic_source": TRAFFIC_SOURCE if load_traffic("concat", np.dtype(np_dt).name) else None,
                            "kernel_ms": round(kern_ms, 5), "algorithmic_bytes_per_launch": 2 * dst_bytes},
               "cpu_baseline": cpu}
        if dumped:
            out["dump_outputs"] = dumped
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def bench_concat_allgather(dfa, torch, dist, conv_out, world, rank, images=16, iters=5):
    """Every rank contributes the conv output of its first `images` images as one
    channel branch; all-gather (RCCL) + concat+relu kernel -> {images,h,w,world*C}."""
    ddist = importlib.import_module("deep-fusion_amd.dist")
    local = conv_out[:images].contiguous()
    bs, h, w, c = local.shape
    np_dt = {torch.int32: np.int32, torch.float32: np.float32, torch.int8: np.int8,
             torch.uint8: np.uint8}[local.dtype]
    op = dfa.Concat(bs, h, w, [c] * world, np_dt, True)
    offs, total = ddist.gathered_offsets(bs, h, w, [c] * world, local.element_size())
    dst = torch.empty((bs, h, w, c * world), dtype=local.dtype, device=local.device)
    times = []
    for it in range(iters + 2):
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        g = ddist.allgather_shards(local, [c] * world)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        op.submit_gathered(g, offs, dst)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if it >= 2:
            times.append((t1 - t0, t2 - t1))
    # correctness of the exchange: channel block r of dst == relu(rank r's shard)
    mine = dst[..., rank * c:(rank + 1) * c]
    ok = bool(torch.equal(mine, torch.clamp(local, min=0) if local.dtype != torch.uint8 else local))
    tt = torch.tensor([sum(t[0] for t in times) / len(times), sum(t[1] for t in times) / len(times),
                       0.0 if ok else 1.0], dtype=torch.float64, device="cuda")
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    return {"shard_bytes_per_rank": int(local.numel() * local.element_size()),
            "allgather_ms": round(float(tt[0]) * 1e3, 4), "concat_relu_ms": round(float(tt[1]) * 1e3, 4),
            "allgather_GBps_per_rank_in": round(total * (world - 1) / world / float(tt[0]) / 1e9, 2),
            "correct": float(tt[2]) == 0.0}


if __name__ == "__main__":
    main()
