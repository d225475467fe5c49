#!/usr/bin/env python3
"""Benchmark of the matching hot path: matched stereo image-pairs/sec (4096 kpts, 1080p) on N MI355X.

    python bench.py --gpus N --steps K --warmup W            (N > 1: the parent spawns one process per GPU, see `spawn`)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...

--config 2 (default, the headline; BASELINE.json configs[1]): one step = one synthetic 1080x1920 stereo pair, gray uint8
    already resident in HBM -> SuperPoint on both images -> LightGlue (9 layers) -> matches + the pair's match-table record
    on the device. A small pool of pairs is cycled.
--config 3 (configs[2]): the same step over a sequence of DISTINCT epochs (default 256 steps; seeds 1234+2e / 1235+2e).
--config 4 (configs[3]): config 3's step over 2048 epochs in total, sharded e = rank (mod N) over --gpus N ranks (2048 / N steps per
    rank by default), 98 KB records that carry the keypoints of both images, one RCCL all-gather of the tables at the
    end. A pool of --pool distinct synthetic pairs per rank is cycled (host synthesis of 2048 pairs would take minutes).
--config 5 (configs[4], not the headline): one step = one 3000x4000 pair, 16384 keypoints, SuperPoint (nms 3) + SuperGlue
    (18 layers, 20 Sinkhorn iterations); with --full, roofline objects for the Sinkhorn sweeps (HBM) and the attention kernel (MFMA).
Every rank processes its own steps (weak scaling, epochs sharded round-robin); the timed region ends with the job's single
collective, one all-gather of the per-rank match tables (RCCL). Prints ONE JSON line on rank 0.
--steps K: the timed region is exactly K steps; `ms_per_step` is its time / K.
--dump-outputs DIR: after the timed region, the last timed step's match-table records as DIR/<name>.npy (`dump_outputs`).
--full: after the timed region, also what the headline does not need (rank 0): the per-launch roofline pass (`roofline*`,
    `kernel_ms_per_pair`, the pair-level utilisation figures), the default line's `side_measurements` (other configurations, launch
    modes and calls, each in runs of its own) and the oracle's `cpu_baseline` (over a minute of CPU work). Without it a run sets up,
    warms up, times its steps, writes its outputs and prints the line: the same headline, the same timed steps.
--dry-run: no GPU work at all (fabricated records): exercises spawn, rendezvous (gloo), sharding, the table all-gather and the
    JSON contract on a CPU-only machine (tests/test_host_cpu.py).
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

H, W, KPTS = 1080, 1920, 4096
H5, W5, KPTS5 = 3000, 4000, 16384
PEAK_F32_MFMA_TFLOPS = 157.3   # /opt/skills/guides/MI355X_MICROARCH.md: dense fp32 matrix peak
PEAK_BF16_MFMA_TFLOPS = 2500.0 # same guide: dense bf16 matrix peak (the 5 PFLOP/s headline includes 2:1 sparsity)
# The attention kernel (csrc/attention_bx.hip) computes every fp32 product as SIX bf16 products on the bf16 matrix cores (fp32 operands cut
# into three bf16 values, fp32 accumulation: error at or below the f32-input MFMA chain's, profiles/r05_bf16x_probe.txt). Its roofline is
# the bf16 peak divided by the six products an algorithmic fp32 FLOP costs.
ATTN_BF16_PRODUCTS = 6
PEAK_ATTN_F32_EQUIVALENT_TFLOPS = PEAK_BF16_MFMA_TFLOPS / ATTN_BF16_PRODUCTS
ATTN_F32_FORM = os.environ.get("IM_ATTN_F32", "0") not in ("", "0")   # the f32-input MFMA kernel of rounds 1-5 (csrc/attention.hip), for A/B
ATTN_KERNEL = "im::flash_attn_f32_kernel" if ATTN_F32_FORM else "im::flash_attn_bx_kernel"
PEAK_ATTN_TFLOPS = PEAK_F32_MFMA_TFLOPS if ATTN_F32_FORM else PEAK_ATTN_F32_EQUIVALENT_TFLOPS
CONV_F32_FORM = os.environ.get("IM_CONV_F32", "0") not in ("", "0")   # the f32-input MFMA Winograd kernel of rounds 2-5 (csrc/conv_wino.hip, !BX), for A/B
PEAK_CONV_TFLOPS = PEAK_F32_MFMA_TFLOPS if CONV_F32_FORM else PEAK_ATTN_F32_EQUIVALENT_TFLOPS
SPEC_CLOCK_MHZ = 2400.0        # the clock the spec peaks are quoted at (MI355X_MICROARCH.md)
BX_ARITHMETIC = ("six bf16 products per fp32 product (v_mfma_f32_32x32x16_bf16, fp32 accumulation): every fp32 operand is the exact sum of three bf16 "
                 "values, the products h l, l h, m m, h m, m h, h h are added small terms first")
DTYPE_NOTE = ("fp32 end to end, as the reference. Every large contraction - SuperPoint's 3 x 3 convolutions (Winograd F(2x2, 3x3), since round 6) and the "
              "matchers' attention, feed-forward and K = 256 / score GEMMs (since round 5) - computes each fp32 product as six bf16 products on the bf16 "
              "matrix cores with fp32 accumulation (every fp32 operand is the exact sum of three bf16 values; error at or below the f32-input MFMA chain's: "
              "profiles/r05_bf16x_probe.txt, profiles/r06_bf16_stress.txt, tests/test_gpu_bf16_stress.py); SuperPoint's 1 x 1 heads stay on the f32-input MFMA")
PEAK_HBM_GBS = 8000.0          # same guide: HBM3E spec peak (6.3 TB/s is what a copy kernel reaches)
# Pairs per launch of the timed region (`--batch`): the batch dimension over pairs inside the kernels. Re-measured on the round-6 build
# (profiles/r06_sweep_launch_mode.txt, one MI355X, `--steps 20 --warmup 5`), pairs/s by launch groups in flight x pairs per launch:
#   1 group :  1 -> 143.7   2 -> 156.7   4 -> 160.4   5 -> 161.0   10 -> 162.2   20 -> 163.3
#   2 groups:  1 -> 156.2   2 -> 162.4   4 -> 164.5   5 -> 165.9   10 -> 166.0   20 -> 162.8      <- the default (two groups, ten pairs)
#   3 groups:  1 -> 150.3   2 -> 159.5   4 -> 164.4   5 -> 163.2   10 -> 162.8   20 -> 162.9
# (round 3, three boxes: 2 -> 105.8, 4 -> 107.3, 5 -> 107.5, 8 -> 108.1, 10 -> 107.0-108, 16 -> 106.6, 25 -> 106.3: the same shape.)
# 10 divides the default 50 steps and the driver's 20. tests/test_gpu_fullsize.py checks this very mode against one pair per launch.
DEFAULT_PAIRS_PER_LAUNCH = 10
SIDE_CONFIG3_EPOCHS = 60         # distinct epochs of the default line's `side_measurements.config3_distinct_epochs`
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "traffic.json")   # PMC-derived HBM bytes per launch (latest round)


def conv_flops(h, w, cin, cout):
    return 2.0 * 9 * cin * cout * h * w


def kernel_flops(name, n_images=2, n0=KPTS, n1=KPTS, h=H, w=W, superglue=False):
    """Algorithmic FLOPs (2 x MAC) of ONE launch of a kernel class at the benchmark shape."""
    h2, w2, h4, w4, h8, w8 = h // 2, w // 2, h // 4, w // 4, h // 8, w // 8
    conv = {"conv1b": (h, w, 64, 64), "conv2a": (h2, w2, 64, 64), "conv2b": (h2, w2, 64, 64), "conv3a": (h4, w4, 64, 128),
            "conv3b": (h4, w4, 128, 128), "conv4a": (h8, w8, 128, 128), "conv4b": (h8, w8, 128, 128),
            "convPa": (h8, w8, 128, 256), "convDa": (h8, w8, 128, 256)}
    if name in conv:
        return n_images * conv_flops(*conv[name])
    if name == "flash_attn_self":   # per image 4 n^2 256 (QK^T and PV over 4 heads x 64)
        return 4.0 * 256 * (n0 * n0 + n1 * n1)
    if name == "flash_attn_cross":
        if superglue:               # SuperGlue: two independent cross attentions, own q/k/v each (`superglue.py:143-147`)
            return 8.0 * 256 * n0 * n1
        return 6.0 * 256 * n0 * n1  # LightGlue, algorithmic: one similarity matrix (2MN 256) + two PV products (4MN 256)
    return None


_REAL_STDOUT = None


def emit(line: str) -> None:
    """The one JSON line, on the process's ORIGINAL stdout (see main)."""
    sys.stdout.flush()
    os.write(_REAL_STDOUT if _REAL_STDOUT is not None else 1, (line + "\n").encode())


def spawn(args) -> None:
    """`python bench.py --gpus N` typed as is: this parent (which never touches a GPU) starts N ranks through
    torch.distributed.run and relays their output; rank 0 prints the JSON line."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def _make_pair(job):
    kind, epoch, h, w = job
    from icepy4d_amd import synthetic
    import numpy as np
    if kind == "translated":
        a, b = synthetic.translated_pair(epoch, h, w, 40, 8)
    else:
        a, b = synthetic.stereo_pair(epoch, h, w)
    return np.stack([a, b])


def make_pairs(jobs, world):
    """Host-side synthesis of the input pairs, jobs = [(kind, epoch, h, w)] (about 1-2 s each at 1080p, ~10 s at 12 MP). MUST run
    before this process initialises the GPU: the workers are forked."""
    jobs = list(jobs)
    workers = max(1, min(len(jobs), 32, (os.cpu_count() or 1) // max(world, 1)))
    if workers == 1:
        return [_make_pair(j) for j in jobs]
    import multiprocessing as mp
    order = sorted(range(len(jobs)), key=lambda i: -jobs[i][2] * jobs[i][3])     # the 12 MP pair first: it is the longest job
    with mp.get_context("fork").Pool(workers) as pool:
        made = pool.map(_make_pair, [jobs[i] for i in order], chunksize=1)
    out = [None] * len(jobs)
    for i, m in zip(order, made):
        out[i] = m
    return out


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 4, 5))
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: roofline pass, side measurements, "
                                                        "CPU baseline (see the module docstring)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--pool", type=int, default=None, help="configs 2 / 4: distinct synthetic pairs per rank (cycled; default 4 / 32)")
    ap.add_argument("--pairs", default="stereo", choices=("stereo", "translated"),
                    help="stereo = SURVEY §8d homography-warped pair (seeded weights find almost no matches on it: full-depth worst "
                         "case); translated = pure translation by (40, 8) px, ~2500 matches per pair")
    ap.add_argument("--no-graph", action="store_true", help="enqueue launches directly instead of replaying a HIP graph")
    ap.add_argument("--streams", type=int, default=2, help="launch groups in flight per GPU (independent contexts on separate HIP streams)")
    ap.add_argument("--batch", type=int, default=DEFAULT_PAIRS_PER_LAUNCH,
                    help="pairs per launch (batch dimension over pairs inside the kernels); see DEFAULT_PAIRS_PER_LAUNCH for the measured sweep")
    ap.add_argument("--no-side-measurements", action="store_true", help="with --full: skip the short untimed-side runs (other launch mode, translated pairs)")
    ap.add_argument("--dry-run", action="store_true", help="no GPU work: spawn / rendezvous / sharding / gather / JSON only")
    ap.add_argument("--fail-epochs", default="", help="test hook for the failure isolation of the sharded driver: comma-separated epochs whose "
                    "input pair is replaced by an array of the wrong shape; their records come out as n_matches = -1, the rank goes on, "
                    "the all-gather happens and the line lists them in `failed_epochs`")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the match-table records of the last timed step (one per rank) as DIR/<name>.npy "
                         "(see `dump_outputs`); the inputs are seeded, so two builds run with the same arguments can be compared array by array")
    args = ap.parse_args()
    if args.steps is None:
        args.steps = {2: 50, 3: 256, 4: max(1, 2048 // max(args.gpus, 1)), 5: 5}[args.config]
    if args.warmup is None:
        args.warmup = {2: 6, 3: 6, 4: 6, 5: 2}[args.config]
    if args.pool is None:
        args.pool = 32 if args.config == 4 else 4

    if args.config == 5:
        args.batch = 1
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn(args)   # does not return
    # the contract is ONE JSON line on stdout: native libraries write there too (RCCL prints a version banner when its first
    # communicator is made, gloo its connection notes), so file descriptor 1 is pointed at stderr for the whole run and the line goes
    # out through a duplicate of the original descriptor (`emit`)
    global _REAL_STDOUT
    sys.stdout.flush()
    _REAL_STDOUT = os.dup(1)
    os.dup2(2, 1)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # IM_BENCH_ISOLATE_DEVICES=1 (default off; the fallback if a plain N > 1 run faults on a device index other than 0): every rank
    # sees ONLY its own GPU, as device 0 - i.e. it runs exactly the single-GPU path every test exercises. Decided here, before
    # anything in this process has touched the HIP runtime (torch is not even imported yet); never by re-executing the process.
    isolate = os.environ.get("IM_BENCH_ISOLATE_DEVICES") == "1" and world > 1
    if isolate:
        seen = [d for d in os.environ.get("HIP_VISIBLE_DEVICES", "").split(",") if d.strip() != ""]
        mine = seen[local_rank] if seen else str(local_rank)       # index into a list the launcher may already have narrowed
        os.environ["HIP_VISIBLE_DEVICES"] = mine
        local_rank = 0

    from icepy4d_amd.sequence import shard_epochs
    total = args.warmup + args.steps
    epochs = shard_epochs(total * world, rank, world)           # this rank's epochs: e = rank (mod world)
    cfg5 = args.config == 5
    h, w, kpts = (H5, W5, KPTS5) if cfg5 else (H, W, KPTS)
    # side measurements of the default line (--full, rank 0 of a one-rank run, headline config only): their inputs are synthesised here
    # too, BEFORE the GPU is initialised (forked workers)
    side_on = args.full and world == 1 and args.config == 2 and not args.no_side_measurements and not args.dry_run
    side_inputs = {}
    if args.dry_run:
        host_pairs = []
    elif args.config == 3:
        host_pairs = make_pairs([(args.pairs, e, h, w) for e in epochs], world)            # every epoch distinct
    else:
        jobs = [("translated" if cfg5 else args.pairs, e, h, w) for e in epochs[:min(args.pool, total)]]
        n_main = len(jobs)
        if side_on:
            g_side = max(1, args.batch * args.streams)
            n_c3 = ((SIDE_CONFIG3_EPOCHS + g_side - 1) // g_side) * g_side                  # whole launch groups only
            jobs += [("stereo", e, H, W) for e in range(n_c3)]                              # configs[2]: distinct epochs 0 .. n_c3 - 1
            jobs += [("translated", j, H, W) for j in range(2)]
            jobs += [("translated", 0, H5, W5)]                                             # configs[4]: one 12 MP pair
        made = make_pairs(jobs, world)
        host_pairs = made[:n_main]
        if side_on:
            side_inputs = {"config3": made[n_main:n_main + n_c3], "translated": made[n_main + n_c3:n_main + n_c3 + 2], "config5": made[-1]}

    import numpy as np
    import torch
    import torch.distributed as dist
    # debugging aid only: IM_BENCH_ONE_DEVICE=1 runs every rank on cuda:0 with a gloo group (1-GPU box rehearsal of N > 1)
    one_dev = os.environ.get("IM_BENCH_ONE_DEVICE") == "1"
    cpu_group = one_dev or args.dry_run
    if one_dev:
        local_rank = 0
    if not args.dry_run:
        torch.cuda.set_device(local_rank)
    # IM_BENCH_FORCE_DIST=1: initialise the process group even for one rank (RCCL rehearsal on a 1-GPU box: the same
    # init / all-gather / barrier calls the N > 1 run makes, through the nccl backend)
    force_dist = os.environ.get("IM_BENCH_FORCE_DIST") == "1" and "RANK" in os.environ
    if world > 1 or force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # a bounded collective timeout: a rank that died without reaching the all-gather must not hold the others for the default
        # 10 (nccl) / 30 (gloo) minutes; torch.distributed.run additionally ends every rank as soon as one exits non-zero
        import datetime
        tmo = datetime.timedelta(seconds=int(os.environ.get("IM_BENCH_COLLECTIVE_TIMEOUT_S", "300")))
        if cpu_group:
            dist.init_process_group("gloo", timeout=tmo)
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank), timeout=tmo)

    from icepy4d_amd.sequence import all_gather_tables, new_table
    if args.dry_run:
        return dry_run(args, rank, world, epochs, kpts, dist)

    from icepy4d_amd import synthetic
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.sequence import PairPipeline

    sp_sd = synthetic.superpoint_state_dict(0)
    if cfg5:
        m_sd, m_name = synthetic.superglue_state_dict(0, "passthrough"), "superglue"
    else:
        m_sd, m_name = synthetic.lightglue_state_dict(0, "passthrough"), "lightglue"

    def make_engine():
        e = Engine(local_rank)
        e.load_state_dict("superpoint", sp_sd)
        e.load_state_dict(m_name, m_sd)
        return e

    n_streams = 1 if cfg5 else args.streams
    with_kp = args.config == 4                     # 98 KB records: keypoints of both images ride along
    sm = PairPipeline(make_engine, h, w, kpts, n_streams=n_streams, use_graph=not args.no_graph, matcher=m_name,
                      pairs_per_launch=args.batch, with_keypoints=with_kp)
    eng = sm.slots[0][0]
    pool = [torch.from_numpy(p).cuda().contiguous() for p in host_pairs]
    fail_epochs = {int(x) for x in args.fail_epochs.split(",") if x.strip()}
    bad_pair = torch.zeros((2, 8, 8), dtype=torch.uint8, device=pool[0].device)      # --fail-epochs: a pair of the wrong shape
    table = new_table(args.steps, kpts, eng.device, with_kp)
    scratch = new_table(max(args.warmup, 2), kpts, eng.device, with_kp)   # >= 2 rows: the untimed gather below must load torch's sort kernels

    def barrier():
        sm.synchronize()
        torch.cuda.synchronize()
        if world > 1 or force_dist:
            dist.barrier()
        torch.cuda.synchronize()

    # untimed warm-up: at least W steps, then batches of >= 16 pairs (whole launch groups) until the batch time stops falling (two consecutive
    # batches within 2 %) or 20 s have passed. A cold MI355X needs seconds of sustained load, not milliseconds, to
    # settle its clocks: the first process on a fresh box measured 62-67 pairs/s after a 3 s warm-up and 83-85 in every
    # later process, with identical per-kernel durations at the end of both.
    i = 0
    while i < args.warmup:
        sm.match_pair(pool[i % len(pool)], epochs[i % len(epochs)], scratch, i % scratch.shape[0])
        i += 1
    sm.flush()                                  # an odd W must not leave a parked pair behind: it would join the first timed group
    sm.synchronize()
    t_w = time.perf_counter()
    prev, stable = None, 0
    g_ = max(1, args.batch * n_streams)
    nb = 2 if cfg5 else ((16 + g_ - 1) // g_) * g_      # whole launch groups: a partial group runs directly, not as the timed mode does
    while time.perf_counter() - t_w < 20.0 and stable < 2:
        t_b = time.perf_counter()
        for _ in range(nb):
            sm.match_pair(pool[i % len(pool)], epochs[i % len(epochs)], scratch, i % scratch.shape[0])
            i += 1
        sm.flush()
        sm.synchronize()
        cur = time.perf_counter() - t_b
        stable = stable + 1 if prev is not None and abs(cur - prev) < 0.02 * prev else 0
        prev = cur
    warm_pairs = i
    sm.synchronize()
    # the gather / sort of the match tables is part of the timed region: run it once untimed as well, so that the lazy
    # loading of torch's indexing and sort kernels (100+ ms in a fresh process) is not billed to the timed steps
    all_gather_tables(scratch.cpu() if one_dev else scratch)
    # The timed region: EXACTLY `steps` steps bracketed by barrier + synchronize, ending with the job's one collective. `--steps` is the
    # number of timed steps and `ms_per_step` this region's time over it: callers size later runs from it.
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ep = epochs[args.warmup + i]
        sm.match_pair(bad_pair if ep in fail_epochs else pool[(args.warmup + i) % len(pool)], ep, table, i)
    sm.flush()
    t_enq = time.perf_counter() - t0            # host time to enqueue every step (graph launches are asynchronous)
    sm.synchronize()
    t_own = time.perf_counter() - t0            # this rank's own pairs done (before the collective)
    t_g = time.perf_counter()
    full = all_gather_tables(table.cpu() if one_dev else table)
    torch.cuda.synchronize()
    t_gather = time.perf_counter() - t_g
    barrier()
    dt = time.perf_counter() - t0
    if world > 1 or force_dist:                 # the slowest rank's clock is the region's
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if one_dev else "cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, full, kpts, world)
    ranks = None
    if world > 1 or force_dist:
        dev_ = "cpu" if one_dev else "cuda"
        # what lets a reader verify that N ranks really took part: every rank reports its own pair count, its own time to finish
        # them and its time inside the all-gather (one more tiny all-gather, outside the timed region)
        ranks = rank_report(dist, rank, world, args, t_own, t_gather, torch.cuda.current_device(), dev_, table, full, cpu_group)
        ranks["device_names"] = sorted({torch.cuda.get_device_name(torch.cuda.current_device())})
    n_pairs = args.steps * world
    assert full.shape[0] == n_pairs, (full.shape, n_pairs)
    # failure isolation: a pair that could not be matched carries n_matches = -1 in the gathered table, whichever rank owned it
    ok_rows = full[full[:, 3] >= 0]
    failed_epochs = sorted(int(e) for e in full[full[:, 3] < 0, 0].tolist())
    nm = ok_rows[:, 3].float().mean().item() if len(ok_rows) else 0.0
    n0 = ok_rows[:, 1].float().mean().item() if len(ok_rows) else 0.0
    n1 = ok_rows[:, 2].float().mean().item() if len(ok_rows) else 0.0

    if cfg5:
        metric = "matched stereo image-pairs/sec (16384 kpts, 12 MP, SuperGlue)"
        workload = ("configs[4]: one 3000x4000 gray pair per step, SuperPoint (16384 kpts, nms 3, threshold 0.001) + SuperGlue (18 "
                    "layers, 20 Sinkhorn iterations, match threshold 0.3), seeded weights")
    else:
        metric = "matched stereo image-pairs/sec (4096 kpts, 1080p)"
        workload = (f"configs[{args.config - 1}]: one 1080x1920 gray stereo pair per step"
                    + (" over a sequence of distinct epochs" if args.config == 3 else f" (pool of {len(pool)} pairs cycled)")
                    + (f", {n_pairs} epochs in total sharded over {world} rank(s), 98 KB records with the keypoints of both images" if args.config == 4 else "")
                    + ", SuperPoint (4096 kpts, nms 4) + LightGlue (9 layers, CPU-path semantics: pruning evaluated every layer), "
                      "seeded weights; epochs sharded round-robin, one all-gather of match tables at the end")
    result = {
        "metric": metric, "value": len(ok_rows) / dt, "unit": "pairs/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "dtype_note": DTYPE_NOTE, "data": "synthetic",
        "config": {"workload": workload, "height": h, "width": w, "max_keypoints": kpts, "pairs_per_step": 1,
                   "pair_synthesis": args.pairs if not cfg5 else "translated", "hip_graph": not args.no_graph,
                   "launch_groups_in_flight": n_streams, "pairs_per_launch": args.batch,
                   "attention": ("f32-input MFMA (IM_ATTN_F32=1)" if ATTN_F32_FORM else BX_ARITHMETIC),
                   "convolutions": "Winograd F(2x2, 3x3), " + ("f32-input MFMA (IM_CONV_F32=1)" if CONV_F32_FORM else BX_ARITHMETIC),
                   "mean_keypoints": n0, "mean_matches": nm},
        "host_enqueue_ms_per_step": 1e3 * t_enq / args.steps, "untimed_pairs_before_timing": warm_pairs,
        "all_gather_ms": 1e3 * t_gather,
        "failed_epochs": failed_epochs, "full": args.full,
    }
    if failed_epochs:
        result["failed_epochs_note"] = (f"{len(failed_epochs)} of the {n_pairs} timed pairs have a record with n_matches = -1 (this rank's own: "
                                        f"{sm.failed}); `value` counts the {len(ok_rows)} matched pairs only, `ms_per_step` all {n_pairs} steps")
    if ranks is not None:
        result["ranks"] = ranks

    def quick_rate(pipe, inputs, n, host=False, epoch0=0, keep=None):
        """Untimed-warm, short side measurement on this rank: pairs/s of `pipe` over n pairs of `inputs` (whole launch groups of
        warm-up first). `keep`: a table that receives the timed records."""
        side = keep if keep is not None else new_table(n, kpts, eng.device, with_kp)
        feed = pipe.match_host_pair if host else pipe.match_pair
        for j in range(min(n, len(pipe.slots) * pipe.slots[0][2].P)):
            feed(inputs[j % len(inputs)], epoch0 + j, side, j)
        pipe.flush(); pipe.synchronize()
        t = time.perf_counter()
        for j in range(n):
            feed(inputs[j % len(inputs)], epoch0 + j, side, j)
        pipe.flush(); pipe.synchronize()
        return n / (time.perf_counter() - t), side[:, 3].float().mean().item()

    if rank == 0 and side_on:
        # side measurements (not `value`): the other launch mode, and a pool of pairs on which the seeded weights DO find matches
        t_side = time.perf_counter()
        alt_b, alt_s = (1, 3) if args.batch > 1 else (2, 2)
        n_side = ((48 + args.batch * n_streams - 1) // (args.batch * n_streams)) * args.batch * n_streams   # whole launch groups only
        alt = PairPipeline(make_engine, h, w, kpts, n_streams=alt_s, use_graph=not args.no_graph, matcher=m_name, pairs_per_launch=alt_b,
                           with_keypoints=with_kp)
        r_alt, _ = quick_rate(alt, pool, 48)
        alt.close()
        tr_pool = [torch.from_numpy(p).cuda().contiguous() for p in side_inputs["translated"]]
        r_tr, m_tr = quick_rate(sm, tr_pool, n_side)
        # the same pairs handed over in HOST memory (what the reference's epoch loop holds after imread): page-locked staging
        # ring + asynchronous upload on the launch stream, PCIe inside the measured time
        r_host, _ = quick_rate(sm, host_pairs, n_side, host=True)
        # configs[2]: the timed launch mode over DISTINCT epochs (seeds 1234 + 2e / 1235 + 2e, slowly varying homography), whole
        # launch groups; inputs resident in HBM like the headline's
        c3_pool = [torch.from_numpy(p).cuda().contiguous() for p in side_inputs["config3"]]
        c3_table = new_table(len(c3_pool), kpts, eng.device, with_kp)
        r_c3, m_c3 = quick_rate(sm, c3_pool, len(c3_pool), keep=c3_table)
        c3_epochs = c3_table[:, 0].tolist()
        del c3_pool
        adaptive = adaptive_side(args, local_rank, sp_sd, tr_pool, n_side, n_streams, h, w, kpts, eng)
        result["side_measurements"] = {
            "adaptive_depth_and_width": adaptive,
            "other_launch_mode": {"pairs_per_launch": alt_b, "launch_groups_in_flight": alt_s, "pairs_per_s": r_alt, "pairs": 48},
            "host_inputs_pairs_per_s": {"pairs_per_s": r_host, "pairs": n_side,
                                        "note": "PCIe-inclusive: every pair starts as a numpy uint8 array in pageable host memory, is copied "
                                                "into a page-locked staging ring and uploaded asynchronously on its launch group's stream "
                                                "(`PairPipeline.match_host_pair`; one group's upload runs beside the other group's "
                                                "kernels); never `value`"},
            "translated_pairs": {"pairs_per_s": r_tr, "mean_matches": m_tr, "pairs": n_side,
                                 "note": "pairs related by a pure (40, 8) px translation: the seeded weights match ~1000 keypoints "
                                         "per pair on them (8 on the homography-warped pairs of `value`); same launches, no pruning or "
                                         "early exit triggers with seeded weights either way"},
            "config3_distinct_epochs": {"pairs_per_s": r_c3, "ms_per_pair": 1e3 / r_c3, "pairs": len(c3_epochs), "mean_matches": m_c3,
                                        "epochs_distinct_and_in_order": c3_epochs == list(range(len(c3_epochs))),
                                        "note": "BASELINE configs[2] at reduced length: the timed launch mode of `value` over "
                                                f"{len(c3_epochs)} DISTINCT synthetic epochs (SURVEY 8d config 3 seeds), every pair "
                                                "computed once after one launch group per stream of warm-up; `python bench.py --config 3` "
                                                "runs all 256"}}
        result["side_measurements"]["config5"] = config5_side(args, local_rank, sp_sd, side_inputs["config5"])
        result["side_measurements"]["match_call_ms"] = match_call_side(local_rank, sp_sd, m_sd, host_pairs[0])
        result["side_measurements"]["production_call_ms"] = production_call_side(local_rank, sp_sd, m_sd)
        result["side_measurements"]["seconds_spent"] = round(time.perf_counter() - t_side, 1)

    if rank == 0 and args.full:
        # ---- roofline of the dominant kernel: HIP events around every launch (library-side, on the launch stream); during the same isolated pass the
        # two matrix-core kernel classes report the shader clock they hold inside their main loops (im_debug_clock_probe: cycles / 100 MHz reference ticks)
        prof_steps = 1 if cfg5 else 4
        clocks = (ctypes.c_double * 4)()
        eng0 = sm.slots[0][0]
        eng0.ctx.call("im_debug_clock_probe", 1, None, eng0.stream_ptr())
        prof, ev_overhead_ms = event_profile(sm.slots[0], pool, epochs, scratch, 1 if cfg5 else 3, prof_steps)
        eng0.ctx.call("im_debug_clock_probe", 0, clocks, eng0.stream_ptr())
        clock_mhz = {"attention": clocks[0] if clocks[1] > 0 else None, "convolutions": clocks[2] if clocks[3] > 0 else None}
        tot = sum(v["total_ms"] for v in prof.values())
        try:
            with open(TRAFFIC_FILE) as fh:
                traffic_db = json.load(fh)
        except (OSError, ValueError):
            traffic_db = {}
        how = ("HIP events around each launch, minus the duration of an empty event pair measured on the same stream, in an "
               "isolated pass with ONE pair in flight (with several pairs in flight kernels of different pairs share the chip and "
               "per-launch durations are not kernel properties); rocprofv3 --stats of `bench.py --streams 1` in profiles/ agrees")
        # group the launch classes by kernel symbol, as rocprofv3 --stats does; `roofline` is the class with the largest time, the other class is
        # always emitted next to it (`roofline_attention` / `roofline_convolutions`)
        CONV_SYM = "im::conv3x3_wino_kernel<POOL, FUSE1A, UREG, BX> (all instantiations)"
        if cfg5:
            groups = {ATTN_KERNEL: ["flash_attn_self", "flash_attn_cross"]}
        else:
            groups = {ATTN_KERNEL: ["flash_attn_self", "flash_attn_cross"],
                      CONV_SYM: ["conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convDa"]}
        gstat = {}
        for sym, names in groups.items():
            ms = sum(prof[k]["total_ms"] for k in names if k in prof)
            cnt = sum(prof[k]["count"] for k in names if k in prof)
            fl = sum(kernel_flops(k, 2, n0, n1, h, w, cfg5) * prof[k]["count"] for k in names if k in prof)
            if sym == CONV_SYM:
                fl /= 2.25     # the Winograd F(2x2, 3x3) kernels execute 16 multiplies per 2 x 2 outputs where the direct form has 36: a utilisation prices what runs
            if cnt:
                gstat[sym] = (ms, cnt, fl)

        def class_roofline(sym):
            ms_, cnt_, fl_ = gstat[sym]
            is_attn = sym == ATTN_KERNEL
            peak_ = PEAK_ATTN_TFLOPS if is_attn else PEAK_CONV_TFLOPS
            ach_ = fl_ / (ms_ * 1e-3) / 1e12
            mhz = clock_mhz["attention" if is_attn else "convolutions"]
            out = {"bound": "mfma", "kernel": sym, "achieved": ach_, "peak": peak_, "unit": "TFLOP/s", "frac": ach_ / peak_,
                   "avg_launch_ms": ms_ / cnt_, "launches_per_pair": cnt_ / prof_steps, "algorithmic_gflop_per_launch": fl_ / cnt_ / 1e9,
                   "share_of_pair_time": ms_ / tot,
                   "sustained_clock_mhz": mhz,
                   "frac_at_sustained_clock": (ach_ / (peak_ * mhz / SPEC_CLOCK_MHZ)) if mhz else None,
                   "sustained_clock_is": "median over the blocks of one isolated pass of (shader cycles / 100 MHz reference ticks) x 100 MHz inside the kernel's "
                                         "main loop (s_memtime / s_memrealtime of the first wave, im_debug_clock_probe); `frac_at_sustained_clock` = achieved / "
                                         f"(peak x that clock / {SPEC_CLOCK_MHZ:.0f} MHz): how well the kernel uses the matrix-pipe cycles the chip actually gives it"}
            bx_form = not (ATTN_F32_FORM if is_attn else CONV_F32_FORM)
            if bx_form:
                out["peak_is"] = (f"{PEAK_BF16_MFMA_TFLOPS:.0f} TFLOP/s dense bf16 MFMA (MI355X_MICROARCH.md) / {ATTN_BF16_PRODUCTS}: the kernel computes every fp32 FLOP "
                                  "it executes as six bf16 products on the bf16 matrix cores (fp32 operands as exact sums of three bf16 values, fp32 accumulation; "
                                  "accuracy at or below the f32-input MFMA chain's: profiles/r05_bf16x_probe.txt, profiles/r06_bf16_stress.txt)")
                out["vs_f32_input_mfma_peak"] = ach_ / PEAK_F32_MFMA_TFLOPS
            if not is_attn:
                out["flops_are"] = ("EXECUTED fp32 FLOPs of the Winograd F(2x2, 3x3) form = SURVEY 8d's direct-form count / 2.25 (against the direct-form count the "
                                    "rate is `achieved` x 2.25: not a utilisation)")
            return out

        dom = max(gstat, key=lambda k: gstat[k][0])
        ms, cnt, fl = gstat[dom]
        ach = fl / (ms * 1e-3) / 1e12
        tkey = dom + ("<2>" if dom == "im::flash_attn_f32_kernel" else "<true, true>" if dom == ATTN_KERNEL else "")   # the instantiation rocprofv3 names
        result["roofline"] = class_roofline(dom)
        result["roofline"].update({
            "traffic": traffic_db.get(tkey + ("@16384" if cfg5 else ""), {}).get("traffic_bytes"),
            "traffic_source": "profiles/traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of a builder run, "
                              "FETCH_SIZE doubled per the gfx950 correction; NOT measured by this run)",
            "event_pair_overhead_us": round(1e3 * ev_overhead_ms, 2), "measured": how})
        for key, sym in (("roofline_attention", ATTN_KERNEL), ("roofline_convolutions", CONV_SYM)):
            if sym in gstat:
                result[key] = class_roofline(sym)
        if dom == ATTN_KERNEL and not ATTN_F32_FORM:
            result["roofline"].update({
                "executed_bf16_tflops": ach * ATTN_BF16_PRODUCTS * (4.0 * 256 * (n0 * n0 + n1 * n1) * prof.get("flash_attn_self", {}).get("count", 0)
                                                                   + 8.0 * 256 * n0 * n1 * prof.get("flash_attn_cross", {}).get("count", 0)) / fl,
                "vs_f32_input_mfma_peak_is": "the same algorithmic rate against the 157.3 TFLOP/s of the f32-input MFMA, the roofline of rounds 1-5's "
                                             "kernel (csrc/attention.hip, IM_ATTN_F32=1: 0.745 there). A ratio, not a utilisation: this kernel does "
                                             "not run on that pipe"})
        if dom == ATTN_KERNEL:
            # the two launch kinds of the class apart: self-attention (4 . 256 . n^2 per image) and the cross block, whose two
            # launches execute 8 . 256 . n^2 for an algorithmic 6 . 256 . n^2 (S = Q0 Q1^T is computed once per direction)
            for kname in ("flash_attn_self", "flash_attn_cross"):
                if kname in prof and prof[kname]["count"]:
                    f1 = kernel_flops(kname, 2, n0, n1, h, w, cfg5)
                    result["roofline"]["frac_" + kname.split("_")[-1]] = f1 / (prof[kname]["total_ms"] / prof[kname]["count"] * 1e-3) / 1e12 / PEAK_ATTN_TFLOPS
        if cfg5 and "sinkhorn" in prof:
            # Sinkhorn: (2 x iterations) sweeps over the (M+1)(N+1) fp32 couplings, one "launch" here = the whole 20-iteration
            # solve of one pair (41 kernel launches of three symbols; rocprofv3 lists them separately)
            sk = prof["sinkhorn"]
            alg = 20.0 * (n0 + 1) * (n1 + 1) * 4          # ONE read of the couplings per iteration: what a single-read kernel must move
            gbs = alg * sk["count"] / (sk["total_ms"] * 1e-3) / 1e9
            result["roofline_sinkhorn"] = {"bound": "hbm", "kernel": "im::sinkhorn_fused4_kernel + its combine kernel (20 iterations)", "achieved": gbs, "peak": PEAK_HBM_GBS,
                                           "unit": "GB/s", "frac": gbs / PEAK_HBM_GBS,
                                           "traffic": (20 * sum(v.get("traffic_bytes", 0) for k, v in traffic_db.items()
                                                                if isinstance(v, dict) and "sinkhorn_fused" in k and k.endswith("@16384"))) or None,
                                           "avg_solve_ms": sk["total_ms"] / sk["count"], "algorithmic_bytes_per_solve": alg,
                                           "survey_8d_bytes_per_solve": 2 * alg,
                                           "note": "algorithmic bytes = 20 iterations x one read of the (M+1)(N+1) fp32 couplings: the kernel keeps each "
                                                   "row in registers for both the row and the column update, so one read per iteration is all the "
                                                   "algorithm needs. SURVEY 8d counted two reads per iteration (row sweep + column sweep, "
                                                   "`survey_8d_bytes_per_solve`); against that count the same time would read as twice this "
                                                   "fraction, which is not a utilisation and is not emitted"}
        result["kernel_ms_per_pair"] = {k: round(v["total_ms"] / prof_steps, 4) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"])}
        pair_flops = (2 * 2035e9 + 10818e9) if cfg5 else (2 * 351.7e9 + 734.4e9)  # algorithmic FLOPs per pair
        # speed of light by ALGORITHMIC FLOPs (direct-form convolutions): the 3x3 layers run as Winograd F(2x2, 3x3), which executes
        # 1 / 2.25 of those multiplies, so this figure is not a utilisation and may exceed 1; the executed-FLOP figure is next to it
        result["pair_algorithmic_tflops"] = pair_flops * (n_pairs / dt) / world / 1e12
        result["pair_algorithmic_tflops_is"] = ("SURVEY 8d's algorithmic fp32 FLOPs per pair x pairs/s. Not a utilisation of anything: the 3x3 convolutions run as "
                                                "Winograd F(2x2, 3x3) (1 / 2.25 of the multiplies), they and the matchers' contractions on the bf16 matrix cores at "
                                                "six products per fp32 product; `pair_matrix_pipe_time_at_peak_frac` is the utilisation figure")
        if not cfg5:
            conv3 = 2 * sum(conv_flops(*d) for d in ((h, w, 64, 64), (h // 2, w // 2, 64, 64), (h // 2, w // 2, 64, 64), (h // 4, w // 4, 64, 128),
                                                     (h // 4, w // 4, 128, 128), (h // 8, w // 8, 128, 128), (h // 8, w // 8, 128, 128),
                                                     (h // 8, w // 8, 128, 256), (h // 8, w // 8, 128, 256)))
            attn_exec = 9 * (4.0 * 256 * (n0 * n0 + n1 * n1) + 8.0 * 256 * n0 * n1)   # executed fp32-equivalent FLOPs of the 18 attention launches
            attn_alg = 9 * (4.0 * 256 * (n0 * n0 + n1 * n1) + 6.0 * 256 * n0 * n1)
            # executed fp32-equivalent FLOPs by pipe: the bf16 cores at six products per fp32 product (Winograd convolutions at 1 / 2.25 of their direct-form
            # count, LightGlue's attention as executed, its feed-forward and GEMMs), the f32-input MFMA for what is left of SuperPoint (1 x 1 heads)
            bx_exec = (0.0 if CONV_F32_FORM else conv3 / 2.25) + (734.4e9 - attn_alg) + attn_exec
            f32_exec = (2 * 351.7e9 - conv3) + (conv3 / 2.25 if CONV_F32_FORM else 0.0)
            pipe_s = bx_exec / (PEAK_ATTN_F32_EQUIVALENT_TFLOPS * 1e12) + f32_exec / (PEAK_F32_MFMA_TFLOPS * 1e12)
            # seconds the matrix pipes need for the executed work of one pair at their spec peaks / seconds a pair takes
            result["pair_matrix_pipe_time_at_peak_frac"] = pipe_s * (n_pairs / dt) / world
            result["pair_executed_mfma_utilisation"] = result["pair_matrix_pipe_time_at_peak_frac"]     # the name of rounds 3-5, same meaning

        # ---- CPU baseline: the oracle (torch-CPU fp32 restatement of the reference path) on this box's host cores
        if world == 1 and not args.no_cpu_baseline and not cfg5:
            result["cpu_baseline"] = cpu_baseline(epochs)
    if rank == 0:
        emit(json.dumps(result))
    if world > 1 or force_dist:
        dist.barrier()
        dist.destroy_process_group()


def adaptive_side(args, local_rank, sp_sd, tr_pool, n_side, n_streams, h, w, kpts, eng):
    """`side_measurements.adaptive_depth_and_width`: the timed launch mode with seeded weights under which LightGlue's adaptive
    machinery is at work in EVERY layer, as it is with trained weights on the reference's CPU path (pruning evaluated after every
    layer, `lightglue.py:326-331, 495-510`; stop test `:571-579`): `prune_gradual` (~30 % of the live points go per layer, the pair
    stops by itself once the pruned points lift the confident ratio over 0.95; its one-channel weights are scaled with the channel
    statistics of one image's keypoint descriptors, read from the device) and `earlystop_late` (full width, stop at layer 7). These
    are the variants tests/test_gpu_adaptive.py pins against the reference (G9) and the oracle (from pixels, live counts per layer).
    `matches_equal_to_direct_launches`: the records of the timed mode (pairs share launches, HIP-graph replay, two launch groups)
    are bit-identical to one pair per direct launch."""
    import torch
    from icepy4d_amd import synthetic
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.sequence import PairPipeline, new_table
    eng.superpoint(tr_pool[0], 4, 0.0005, 4, kpts)
    torch.cuda.synchronize()
    d0 = eng.desc[0, :int(eng.n[0])].float().cpu()
    stats = (d0.mean(0), d0.std(0))
    out = {}
    for variant in ("prune_gradual", "earlystop_late"):
        v_sd = synthetic.lightglue_state_dict(0, variant, channel_stats=stats if variant == "prune_gradual" else None)

        def make_variant_engine():
            e = Engine(local_rank)
            e.load_state_dict("superpoint", sp_sd)
            e.load_state_dict("lightglue", v_sd)
            return e
        vp = PairPipeline(make_variant_engine, h, w, kpts, n_streams=n_streams, use_graph=not args.no_graph, matcher="lightglue",
                          pairs_per_launch=args.batch)
        side = new_table(n_side, kpts, eng.device)
        for j in range(args.batch * n_streams):
            vp.match_pair(tr_pool[j % 2], j, side, j)
        vp.flush(); vp.synchronize()
        t_v = time.perf_counter()
        for j in range(n_side):
            vp.match_pair(tr_pool[j % 2], j, side, j)
        vp.flush(); vp.synchronize()
        rate = n_side / (time.perf_counter() - t_v)
        vp.close()
        direct = PairPipeline(make_variant_engine, h, w, kpts, n_streams=1, use_graph=False, matcher="lightglue", pairs_per_launch=1)
        ref = new_table(2, kpts, eng.device)
        for j in range(2):
            direct.match_pair(tr_pool[j], j, ref, j)
        direct.flush(); direct.synchronize()
        prune = direct.slots[0][0].prune[:2].cpu().numpy()
        stop = int(ref[1, 4])
        live = [[int((prune[0] > l).sum()), int((prune[1] > l).sum())] for l in range(stop)]
        direct.close()
        same = all(bool(torch.equal(side[j, 1:], ref[j % 2, 1:])) for j in range(n_side))
        out[variant] = {"pairs_per_s": rate, "mean_stop_layer": side[:, 4].float().mean().item(), "mean_matches": side[:, 3].float().mean().item(),
                        "pairs": n_side, "live_points_per_layer_of_one_pair": live, "matches_equal_to_direct_launches": same}
    out["note"] = ("the launches of `value` with seeded weights under which early stop (`lightglue.py:571-579`) and point pruning (`:563-568`, evaluated "
                   "after every layer as on the reference's CPU path) are at work in every layer of the translated pairs: the device-side stop flag "
                   "skips the remaining layers' kernels, pruned images run on their live rows only (attention with device-side split-KV below 2048 "
                   "live queries); parity of exactly these variants: tests/test_gpu_adaptive.py")
    return out


def production_call_side(local_rank, sp_sd, lg_sd):
    """`side_measurements.production_call_ms`: the call of the reference's driver with its own parameters (`main_dev.py:115-132`:
    LightGlueMatcher.match(..., quality=HIGH, tile_selection=PRESELECTION, grid=[2, 2], overlap=200, min_matches_per_tile=3,
    max_keypoints=8196, geometric_verification=PYDEGENSAC, threshold=2, confidence=0.9999)) on a synthetic 24 MP RGB pair whose texture
    survives the two pyramid levels of the preselection pass (a translated 1000 x 1500 pair, every pixel blown up to a 4 x 4 block):
    host arrays in, numpy results out; median of 3 calls after 1, with the matcher's own timer split."""
    import statistics
    import numpy as np
    from icepy4d_amd import matching, synthetic
    ha, hb = synthetic.translated_pair(3, 1000, 1500, 24, 8, noise=0.0)
    a3 = np.repeat(np.kron(ha, np.ones((4, 4), np.uint8))[:, :, None], 3, 2)
    b3 = np.repeat(np.kron(hb, np.ones((4, 4), np.uint8))[:, :, None], 3, 2)
    m = matching.LightGlueMatcher({"state_dicts": {"superpoint": sp_sd, "lightglue": lg_sd}, "device": local_rank})
    ts, splits = [], []
    for r in range(4):
        t = time.perf_counter()
        m.match(a3, b3, quality=matching.Quality.HIGH, tile_selection=matching.TileSelection.PRESELECTION, grid=[2, 2], overlap=200,
                origin=[0, 0], min_matches_per_tile=3, max_keypoints=8196,
                geometric_verification=matching.GeometricVerification.PYDEGENSAC, threshold=2, confidence=0.9999)
        ts.append(1e3 * (time.perf_counter() - t))
        splits.append({k: round(1e3 * v, 1) for k, v in m.timer.times.items()})
    k = sorted(range(1, 4), key=lambda i: ts[i])[1]
    return {"median": statistics.median(ts[1:]), "calls_ms": [round(t, 1) for t in ts[1:]], "first_call_ms": round(ts[0], 1),
            "split_ms_of_the_median_call": splits[k], "matched_points": int(len(m.mkpts0)), "image": "4000x6000x3 uint8 (24 MP RGB), synthetic",
            "note": "main_dev.py:115-132 call: PRESELECTION (two pyramid levels + one low-resolution match), 2 x 2 tiles with overlap 200, "
                    "8196 keypoints per tile, device LO-RANSAC + DEGENSAC check at 2 px; the first call (workspace growth, graph captures) is "
                    "listed apart"}


def config5_side(args, local_rank, sp_sd, host_pair):
    """`side_measurements.config5` of the default line: BASELINE configs[4] (12 MP pair, 16384 keypoints, SuperPoint nms 3 +
    SuperGlue with 20 Sinkhorn iterations) on three pairs - pairs/s, the attention kernel against the fp32 MFMA peak and the
    Sinkhorn solve against HBM. `python bench.py --config 5` is the full line."""
    import torch
    from icepy4d_amd import synthetic
    from icepy4d_amd.engine import Engine
    from icepy4d_amd.sequence import PairPipeline, new_table
    sg_sd = synthetic.superglue_state_dict(0, "passthrough")

    def make_engine5():
        e = Engine(local_rank)
        e.load_state_dict("superpoint", sp_sd)
        e.load_state_dict("superglue", sg_sd)
        return e
    p5 = PairPipeline(make_engine5, H5, W5, KPTS5, n_streams=1, use_graph=not args.no_graph, matcher="superglue", pairs_per_launch=1)
    dev = p5.device
    pair = torch.from_numpy(host_pair).to(dev).contiguous()
    side = new_table(3, KPTS5, dev)
    p5.match_pair(pair, 0, side, 0)
    p5.flush(); p5.synchronize()
    t = time.perf_counter()
    for j in range(3):
        p5.match_pair(pair, j, side, j)
    p5.flush(); p5.synchronize()
    dt = time.perf_counter() - t
    n0, n1 = side[:, 1].float().mean().item(), side[:, 2].float().mean().item()
    prof, _ = event_profile(p5.slots[0], [pair], [0], side, 1, 1)
    out = {"pairs_per_s": 3 / dt, "ms_per_pair": 1e3 * dt / 3, "pairs": 3, "mean_keypoints": n0, "mean_matches": side[:, 3].float().mean().item(),
           "workload": "configs[4]: 3000x4000 gray pair (the same pair three times), SuperPoint (16384 kpts, nms 3, threshold 0.001) + "
                       "SuperGlue (18 layers, 20 Sinkhorn iterations, match threshold 0.3), seeded weights, one pair per launch"}
    ms = sum(prof[k]["total_ms"] for k in ("flash_attn_self", "flash_attn_cross") if k in prof)
    cnt = sum(prof[k]["count"] for k in ("flash_attn_self", "flash_attn_cross") if k in prof)
    fl = sum(kernel_flops(k, 2, n0, n1, H5, W5, True) * prof[k]["count"] for k in ("flash_attn_self", "flash_attn_cross") if k in prof)
    if cnt:
        out["attention"] = {"avg_launch_ms": ms / cnt, "achieved_tflops": fl / (ms * 1e-3) / 1e12, "peak_tflops": PEAK_ATTN_TFLOPS,
                            "frac_of_peak": fl / (ms * 1e-3) / 1e12 / PEAK_ATTN_TFLOPS,
                            "vs_f32_input_mfma_peak": fl / (ms * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS,
                            "peak_is": "see roofline.peak_is: bf16 dense MFMA peak / 6 products per fp32 product (157.3 with IM_ATTN_F32=1)"}
    if "sinkhorn" in prof and prof["sinkhorn"]["count"]:
        sk = prof["sinkhorn"]
        solve_ms = sk["total_ms"] / sk["count"]
        moved = 20.0 * (n0 + 1) * (n1 + 1) * 4      # the fused kernel reads the couplings ONCE per iteration
        out["sinkhorn"] = {"solve_ms": solve_ms, "bytes_moved_per_solve": moved, "moved_gb_per_s": moved / (solve_ms * 1e-3) / 1e9,
                           "frac_of_hbm_peak_moved": moved / (solve_ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                           "survey_8d_bytes_per_solve": 2 * moved, "survey_8d_gb_per_s": 2 * moved / (solve_ms * 1e-3) / 1e9,
                           "note": "bytes moved = 20 iterations x one read of the (M+1)(N+1) fp32 couplings (u, v and partials "
                                   "are < 4 % more: profiles/traffic.json); SURVEY 8d counts two reads per iteration"}
    out["kernel_ms_per_pair"] = {k: round(v["total_ms"], 3) for k, v in sorted(prof.items(), key=lambda kv: -kv[1]["total_ms"])[:8]}
    p5.close()
    return out


def match_call_side(local_rank, sp_sd, lg_sd, host_pair):
    """`side_measurements.match_call_ms`: ONE `matcher.match(image0, image1)` at 1080p / 4096 keypoints through the plugin API -
    numpy uint8 arrays in (pageable host memory), numpy results out, upload / graph replay / download and the host code of
    `match()` inside the measured time (`matchers.py:139-261`, the call of `main_dev.py:115-132` without tiles)."""
    import statistics
    from icepy4d_amd import matching
    m = matching.LightGlueMatcher({"state_dicts": {"superpoint": sp_sd, "lightglue": lg_sd}, "device": local_rank})
    a, b = host_pair[0], host_pair[1]
    ts = []
    for r in range(13):
        t = time.perf_counter()
        m.match(a, b, quality=matching.Quality.HIGH, tile_selection=matching.TileSelection.NONE, max_keypoints=KPTS,
                geometric_verification=matching.GeometricVerification.NONE)
        ts.append(1e3 * (time.perf_counter() - t))
    ts = ts[3:]     # the first calls capture the HIP graph and size the workspace
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "calls": len(ts),
            "keypoints": int(len(m.mkpts0)), "note": "LightGlueMatcher.match(image0, image1, quality=HIGH, tile_selection=NONE, "
            "max_keypoints=4096, geometric_verification=NONE), host arrays in / numpy out, 10 calls after 3 untimed ones"}


def event_profile(slot, inputs, epochs, scratch, warm, steps):
    """Per-launch durations of one launch group's kernels: HIP events recorded by the library around every launch on the launch
    stream (`im_profile_begin / end`), direct launches with ONE pair in flight. Returns ({launch class: {count, total_ms}}, the
    duration of an empty event pair in ms - already subtracted per launch)."""
    import torch
    eng, pstream, psm = slot
    lib = eng.ctx
    psm.use_graph = False  # per-launch events need direct launches (same kernels, same stream, one pair in flight)
    psm.P = 1
    with torch.cuda.stream(pstream):
        # untimed pairs in this launch mode first: the side measurements end with an idle gap, and directly launched
        # kernels (host-paced, unlike the graph replays of the timed region) need a moment to bring the clocks back up
        for i in range(warm):
            psm.match_pair(inputs[i % len(inputs)], epochs[i % len(epochs)], scratch, 0)
        pstream.synchronize()
        lib.call("im_profile_begin")
        for i in range(steps):
            psm.match_pair(inputs[i % len(inputs)], epochs[i % len(epochs)], scratch, 0)
        pstream.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    lib.call("im_profile_end", buf, len(buf))
    prof = json.loads(buf.value.decode())
    # an event pair around nothing still reads a few microseconds (two packets for the command processor): the library
    # measures that on the same stream and it is subtracted per launch, so the durations are the kernels' own
    cal = prof.pop("_empty_event_pair", None)
    ev_overhead_ms = cal["total_ms"] / cal["count"] if cal and cal["count"] else 0.0
    for v in prof.values():
        v["total_ms"] = max(v["total_ms"] - v["count"] * ev_overhead_ms, 0.0)
    return prof, ev_overhead_ms


def rank_report(dist, rank, world, args, t_own, t_gather, device_index, dev_, table, full, cpu_group):
    """The `ranks` object of an N > 1 line: every rank reports its own pair count, its own time to finish them and its time inside
    the table all-gather (one more tiny all-gather, outside the timed region), so that a reader can verify that N ranks on N
    devices took part and that the gathered table holds every epoch."""
    import torch
    from icepy4d_amd.sequence import shard_epochs
    vis = os.environ.get("HIP_VISIBLE_DEVICES", "")
    vis_id = float(vis) if vis.strip().lstrip("-").isdigit() else -1.0          # a single index (IM_BENCH_ISOLATE_DEVICES=1), else -1
    mine = torch.tensor([float(rank), float(args.steps), t_own, t_gather, float(device_index), vis_id], dtype=torch.float64, device=dev_)
    every = [torch.zeros_like(mine) for _ in range(world)]
    dist.all_gather(every, mine)
    every = sorted((e.tolist() for e in every), key=lambda r: r[0])
    nccl_version = None
    if not cpu_group:
        try:
            nccl_version = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            pass
    total = args.warmup + args.steps
    want = sorted(e for r in range(world) for e in shard_epochs(total * world, r, world)[args.warmup:])
    return {"world": dist.get_world_size(), "backend": dist.get_backend(), "nccl_version": nccl_version,
            "pairs_per_rank": [int(r[1]) for r in every], "device_per_rank": [int(r[4]) for r in every],
            "devices_isolated": os.environ.get("IM_BENCH_ISOLATE_DEVICES") == "1",
            "hip_visible_device_per_rank": [int(r[5]) for r in every],
            "per_rank_pairs_per_s": [r[1] / max(r[2], 1e-9) for r in every], "all_gather_ms": [1e3 * r[3] for r in every],
            "record_bytes": int(table.shape[1]) * 4, "gathered_table_bytes": int(full.numel()) * 4,
            "epochs_in_gathered_table": int(full.shape[0]), "epochs_complete_and_sorted": bool(full[:, 0].tolist() == want)}


def cpu_baseline(epochs):
    """SURVEY §8d / BASELINE.md §3: the oracle on the host cores of the GPU box, same synthetic pairs, one warm-up pair, then
    variant B (weights built once; the denominator of the >= 50x target) as the median of 5 pairs, and variant A (the
    reference rebuilds both models and reloads their weights inside every call, `matchers.py:1256-1258`: here the state
    dicts are rebuilt per call) as the median of 2 pairs. About 70-90 s of CPU work."""
    import statistics
    import torch
    from icepy4d_amd import synthetic
    from oracle import ref_cpu
    # 32 threads: measured fastest on the 2 x 64-core host of the GPU box (16/32/64 threads tie at ~2.5 s per
    # SuperPoint image; all 256 hardware threads are 20x slower through oversubscription)
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    sp_sd = synthetic.superpoint_state_dict(0)
    lg_sd = synthetic.lightglue_state_dict(0, "passthrough")
    pairs = [synthetic.stereo_pair(epochs[i % len(epochs)], H, W) for i in range(6)]
    ref_cpu.match_images_lightglue(*pairs[5], sp_sd, lg_sd, max_keypoints=KPTS)       # warm-up pair (untimed)
    tb = []
    for a, b in pairs[:5]:
        t = time.perf_counter()
        ref_cpu.match_images_lightglue(a, b, sp_sd, lg_sd, max_keypoints=KPTS)
        tb.append(time.perf_counter() - t)
    ta = []
    for a, b in pairs[:2]:
        t = time.perf_counter()
        sp2 = {k: v.clone() for k, v in synthetic.superpoint_state_dict(0).items()}
        lg2 = {k: v.clone() for k, v in synthetic.lightglue_state_dict(0, "passthrough").items()}
        ref_cpu.match_images_lightglue(a, b, sp2, lg2, max_keypoints=KPTS)
        ta.append(time.perf_counter() - t)
    med_b, med_a = statistics.median(tb), statistics.median(ta)
    return {"value": 1.0 / med_b, "unit": "pairs/s", "cores": cores, "kind": "port",
            "sample": f"variant B (weights built once): median of 5 pairs 1080x1920 / 4096 kpts after 1 warm-up pair, "
                      f"{med_b:.2f} s per pair (min {min(tb):.2f}, max {max(tb):.2f}); torch {torch.__version__} CPU fp32, "
                      f"{cores} threads on {os.cpu_count()} logical CPUs, {cpu_model()}",
            "variant_A": {"value": 1.0 / med_a, "unit": "pairs/s",
                          "sample": f"weights rebuilt inside every call: median of 2 pairs, {med_a:.2f} s per pair"}}


def dump_outputs(out_dir, full, kpts, world):
    """`--dump-outputs DIR`: what the timed path handed its caller in its last step - the match-table record of that step on every rank,
    i.e. the last `world` rows of the gathered table (sorted by epoch; layout in icepy4d_amd/sequence.py) - decoded into one .npy per
    field. Integer fields as float64 (exact for int32), scores and keypoints as float32: under 0.25 MB per rank in every
    configuration (12 bytes per keypoint, 28 with the keypoints of configs[3])."""
    import numpy as np
    from icepy4d_amd.sequence import HEADER
    rec = full[-world:].cpu().numpy()
    K = kpts
    out = {"epoch": rec[:, 0], "n_keypoints": rec[:, 1:3], "n_matches": rec[:, 3], "stop_layer": rec[:, 4],
           "matches0": rec[:, HEADER:HEADER + K], "matching_scores0": rec[:, HEADER + K:HEADER + 2 * K].view(np.float32)}
    if rec.shape[1] == HEADER + 6 * K:          # configs[3]: the records carry the keypoints of both images
        out["keypoints"] = rec[:, HEADER + 2 * K:].view(np.float32).reshape(-1, 2, K, 2)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64))


def dry_run(args, rank, world, epochs, kpts, dist):
    """No GPU: every rank fabricates the records of its epochs (n_matches = epoch), the tables are all-gathered over gloo and
    rank 0 prints a JSON line with the contract's fields (value = records per second of this fake work: NOT a measurement)."""
    import torch
    from icepy4d_amd.sequence import all_gather_tables, new_table
    from icepy4d_amd.sequence import mark_failed
    table = new_table(args.steps, kpts, "cpu", args.config == 4)
    fail_epochs = {int(x) for x in args.fail_epochs.split(",") if x.strip()}
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        e = epochs[args.warmup + i]
        if e in fail_epochs:
            mark_failed(table, i, e, kpts)
            continue
        table[i, 0] = e
        table[i, 1] = kpts
        table[i, 2] = kpts
        table[i, 3] = e
    t_own = time.perf_counter() - t0
    t_g = time.perf_counter()
    full = all_gather_tables(table)
    t_gather = time.perf_counter() - t_g
    if world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    n_pairs = args.steps * world
    assert full.shape[0] == n_pairs, (full.shape, n_pairs)
    want = sorted(e for r in range(world) for e in range(r, (args.warmup + args.steps) * world, world)[args.warmup:])
    assert full[:, 0].tolist() == want and full[:, 3].tolist() == [(-1 if e in fail_epochs else e) for e in want]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, full, kpts, world)
    ranks = rank_report(dist, rank, world, args, t_own, t_gather, -1, "cpu", table, full, True) if world > 1 else None
    if rank == 0:
        emit(json.dumps({"ranks": ranks, "metric": "matched stereo image-pairs/sec (4096 kpts, 1080p)", "value": n_pairs / dt, "unit": "pairs/s",
                          "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * dt / args.steps,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "dtype_note": DTYPE_NOTE, "data": "synthetic",
                          "config": {"workload": "DRY RUN: fabricated records, no GPU work"}, "dry_run": True,
                          "failed_epochs": sorted(int(e) for e in full[full[:, 3] < 0, 0].tolist()),
                          "roofline": None, "cpu_baseline": None}))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def abort_rank(exc) -> None:
    """An error nothing could isolate (the device is gone, the library failed outside a pair): say so, try to leave the process group
    for a bounded time so that the other ranks' collective fails fast instead of waiting for its timeout, and exit non-zero -
    torch.distributed.run then ends the remaining ranks. Never re-executes: this process has touched the GPU."""
    import threading
    import traceback
    traceback.print_exc()
    sys.stderr.write(f"bench.py rank {os.environ.get('RANK', '0')}: unrecoverable error, leaving the process group and exiting 3\n")
    sys.stderr.flush()
    dist = sys.modules.get("torch.distributed")
    if dist is not None and dist.is_available() and dist.is_initialized():
        t = threading.Thread(target=dist.destroy_process_group, daemon=True)
        t.start()
        t.join(20.0)
    os._exit(3)


if __name__ == "__main__":
    try:
        main()
    except SystemExit:
        raise
    except BaseException as exc:      # noqa: BLE001
        abort_rank(exc)
