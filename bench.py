#!/usr/bin/env python3
"""bench.py -- poses/sec of the batched absolute-pose SDP solver on N MI355X.

Contract (driver):  python bench.py --gpus N --steps K --warmup W   prints ONE JSON line.
A "step" is one pass of the hot path (assembly -> SDP solve -> pose) over one batch of
synthetic problems already resident in HBM.  The default workload is BASELINE config 2
("10k PnP problems, N=10 points each"); with --gpus N every rank solves its own batch
(weak scaling) and the per-step results are gathered over RCCL (north-star config 4).

A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, higher_is_better, dtype,
ms_per_step, plus what the timed region itself yields: launch-time roofline, solver statistics of the last step).
--dump-outputs DIR writes the last timed step's outputs as DIR/<name>.npy.  Every other measurement and check below
(and the extra legs named in the code) runs with --full only.

Extra objects in the JSON line:
  roofline      HBM roofline of the solve kernel: algorithmic bytes per launch
                (8*(5 n_p + 10 n_l) + 100 per problem) / mean launch duration
                measured with HIP events on the launch stream; peak 8000 GB/s.  Measured traffic
                and VALU issue (rocprofv3 --pmc child passes): --full.
  cpu_baseline  (--full) this solver's algorithm built for the host (tests/hostsim: solver_core.h under g++, OpenMP over
                problems), timed on a bounded sample of the same workload on this box's host cores (rank 0,
                N=1 only); cpu_baseline_reference_path_port: the CPU oracle (restated reference path) likewise.
  value / dtype the timed region runs at the REFERENCE's precision: float64 throughout (opts.f32_sweeps_until = 0; the reference is
                float64 end to end, cvxpnpl.py:475-513).  value_mixed (--full): the same K steps with the library's default, which runs the
                Jacobi sweeps of young solves on single-precision columns (--precision mixed makes that the timed region instead).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

# More hardware queues than ROCm's default of 4, before the HIP runtime starts: with four, the side stream that packs and
# exchanges the results of a finished step (--gpus > 1) lands on the solve stream's own queue and every step waits behind it
# (measured with a one-rank RCCL group: 0.231 -> 0.208 ms per step; no effect on the single-GPU run).
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (n_p, n_l, batch per GPU, sigma)
    "pnp_n10_10k": (10, 0, 10_000, 2.0),     # BASELINE config 2 (the metric's config)
    "pnpl_5p5l_100k": (5, 5, 100_000, 2.0),  # BASELINE config 3
    "pnp_n10_125k": (10, 0, 125_000, 2.0),   # BASELINE config 4 per-GPU shard
    "pnp_n4_50k": (4, 0, 50_000, 0.0),       # 50 k INDEPENDENT noise-free four-point problems (not config 5: see ransac_n4_50k)
    "ransac_n4_50k": (4, 0, 50_000, 0.5),    # BASELINE config 5 as SURVEY.md 8(d) defines it: ONE scene of 100 correspondences, 30 % of the
                                             # 2D points replaced by uniform clutter, 50 000 random 4-subsets (synth.make_ransac); `value` times
                                             # the solve, `ransac_frame` the whole frame (solve + score + arg-max + refit)
    "pnp_scal": (0, 0, 0, 2.0),                # --n N: one point of the reference's scalability grid (benchmarks/scalability/pnp.py:26-40,
                                               # N = 4...10 and 200...10 000 points per problem); problems per step chosen so that a step
                                               # streams ~1e7 points (at least 1 000, at most 125 000 problems)
    "pnp_n10000_1k": (10_000, 0, 1_000, 2.0),  # the reference's scalability regime (benchmarks/scalability/pnp.py:37-40): the
                                               # blocked, bandwidth-shaped assembly (400 KB per problem) + the solve at the cost seam
}


def algorithmic_bytes(n_p, n_l):
    return 8 * (5 * n_p + 10 * n_l) + 100


def model_flops(n_p, n_l, iters, sweeps):
    """SURVEY.md 8(d), the secondary roofline: flops of one solve from its COUNTED iterations and Jacobi sweeps,
    F = F_setup + iters (F_aff + F_rec + F_vec) + sweeps F_sweep + F_recover, nominal constants F_setup = 160 m + 400 (m correspondence
    records), F_aff = 1 200 (structured affine projection), F_rec = 1 100 (W+ from the eigen columns), F_vec = 550 (the update),
    F_sweep = 9 000 (45 rotations x 200), F_recover = 2 000.  Certificate attempts (polish, dual recovery, LDL^T) are NOT in the model:
    the figure is a lower bound on the arithmetic actually executed."""
    m = n_p + 2 * n_l
    return (160.0 * m + 400.0) + iters * (1200.0 + 1100.0 + 550.0) + sweeps * 9000.0 + 2000.0


FP64_VECTOR_PEAK_TFLOPS = 78.6  # MI355X public datasheet (the local guide lists FP32 vector 157.3)
REFERENCE_PYTHON_OVERHEAD_US = 224.0  # measured per-pose cost of the reference's Python side with the solve stubbed out


def _cpu_quota():
    """CPUs the container may use per scheduling period (cgroup v2 cpu.max or v1 cfs quota), or None when unlimited / unknown: with a quota,
    short bursts of many threads run at the box's full width and are then throttled for the rest of the period -- a sustained rate is the quota's."""
    try:
        if os.path.exists("/sys/fs/cgroup/cpu.max"):
            q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
            return None if q == "max" else float(q) / float(per)
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except Exception:
        return None


def _host_link(dev_index):
    """What the transfer-inclusive rate depends on outside this code (round-5 verdict: 31-58 M poses/s across boxes): the PCIe link of the
    device as the kernel driver reports it, the NUMA node it hangs off, and where this process's threads may run."""
    import glob
    info = {}
    try:
        import torch
        bus = None
        props = torch.cuda.get_device_properties(dev_index)
        if hasattr(props, "pci_bus_id"):
            bus = f"{getattr(props, 'pci_domain_id', 0):04x}:{props.pci_bus_id:02x}:{getattr(props, 'pci_device_id', 0):02x}.0"
        cands = [f"/sys/bus/pci/devices/{bus}"] if bus else []
        cands += sorted(glob.glob("/sys/class/drm/card*/device"))
        for c in cands:
            if os.path.exists(os.path.join(c, "current_link_speed")):
                rd = lambda n: open(os.path.join(c, n)).read().strip() if os.path.exists(os.path.join(c, n)) else None  # noqa: E731
                info.update({"sysfs": c, "current_link_speed": rd("current_link_speed"), "current_link_width": rd("current_link_width"),
                             "max_link_speed": rd("max_link_speed"), "max_link_width": rd("max_link_width"), "numa_node": rd("numa_node")})
                break
    except Exception as e:  # diagnostics only
        info["error"] = str(e)[:120]
    try:
        aff = sorted(os.sched_getaffinity(0))
        # (with OMP_PROC_BIND set -- main() does, for the host baselines -- the OpenMP runtime binds the calling thread to its first place when it
        #  starts: a two-cpu answer here is that binding of THIS thread, not a limit of the box; os.cpu_count() is the box)
        info["main_thread_affinity"] = f"{len(aff)} cpus, {aff[0]}..{aff[-1]}"
        info["host_cpus"] = os.cpu_count()
        nodes = sorted(glob.glob("/sys/devices/system/node/node[0-9]*"))
        info["host_numa_nodes"] = len(nodes)
    except Exception:
        pass
    return info


def _kernel_name(layout, batch, blocked=False, n_corr=10):
    """kernels of one step (AUTO policy of cvxpnpl_solve_batch: by launch size; four-correspondence problems stay in the quad schedule)"""
    if blocked:
        return "assemble_large_kernel (dominant: timed on its own) + assemble_finish_kernel + solve_wave_kernel"
    if layout == 0:
        layout = 2 if batch < 2560 else (3 if (batch < 20000 or n_corr <= 4) else 1)
    return {1: "solve_lane2_kernel + resume_wave_kernel (+ rescue_wave_kernel / ipm_quad_kernel: problems beyond opts.rescue_from iterations)",
            2: "solve_wave_kernel (+ rescue_wave_kernel: problems beyond opts.rescue_from iterations)",
            3: "solve_quad_kernel (+ rescue_wave_kernel, or ipm_quad_kernel + resume_wave_kernel for at most five correspondences: planar scenes and problems beyond opts.rescue_from iterations)",
            4: "solve_quad_kernel<12 lanes per problem> (+ rescue_wave_kernel: planar scenes and problems beyond opts.rescue_from iterations)"}.get(layout, f"experimental layout {layout}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="pnp_n10_10k", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="override problems per GPU per step")
    ap.add_argument("--n", type=int, default=0, help="points per problem of --workload pnp_scal")
    ap.add_argument("--blocked", default="auto", choices=("auto", "0", "1"), help="assembly path: 1 = cvxpnpl_assemble_large_batch + cost-seam solve, "
                    "0 = in-kernel assembly, auto = the product's rule (cvxpnpl_amd.api.use_blocked_assembly: 768 correspondence records, 384 in batches of >= 2 048)")
    ap.add_argument("--precision", default="f64", choices=("f64", "mixed"), help="arithmetic of the timed region: f64 = every Jacobi sweep in float64 "
                    "like the reference (opts.f32_sweeps_until = 0; the headline), mixed = the library's default (single-precision sweeps while a "
                    "solve is young); with --full the other mode is measured beside it (value_mixed / value_all_f64)")
    ap.add_argument("--no-f64-ab", action="store_true", help="skip the extra measurement in the other precision mode (value_mixed / value_all_f64)")
    ap.add_argument("--collective", default="all_gather", choices=("all_gather", "gather"), help="--gpus N exchange: all_gather = every rank ends with "
                    "every shard's records (north-star config 4 as written); gather = rank 0 only (one consumer: 1/N of the bytes per rank)")
    ap.add_argument("--sigma", type=float, default=None, help="pixel noise of the synthetic problems")
    ap.add_argument("--seed", type=int, default=42, help="seed of the synthetic problems (diagnostics: the default is the judged workload)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-overlap", action="store_true", help="skip the extra two-stream (overlapped batches) measurement")
    ap.add_argument("--cpu-sample", type=int, default=0, help="problems in the CPU baseline sample (0 = auto)")
    ap.add_argument("--layout", type=int, default=0, help="kernel layout (0 auto, 1 lane/hybrid, 2 wave, 3 quad/hybrid, 4 penta: quad schedule with 12 lanes per problem)")
    ap.add_argument("--no-gather", action="store_true", help="skip the RCCL gather of results when --gpus > 1")
    ap.add_argument("--force-dist", action="store_true", help="diagnostics: run the RCCL path (process group, packed all_gather) "
                    "even with one rank, to measure / smoke-test it on a 1-GPU box")
    ap.add_argument("--events-per-step", action="store_true", help="record a HIP event after every launch (per-launch durations) instead of "
                    "one before the first and one after the last (their span / K)")
    ap.add_argument("--opt", action="append", default=[], help="solver option override name=value (diagnostics)")
    ap.add_argument("--streams", type=int, default=1, help="HIP streams the steps are issued round-robin on (1 = the contract's "
                    "back-to-back steps; >1 lets independent batches overlap, reported in config)")
    ap.add_argument("--pmc", default="auto", choices=("auto", "run", "off"), help="roofline.traffic: auto = measure with rocprofv3 --pmc child passes "
                    "when rocprofv3 is on PATH, else a hash-matched committed profile; run = measure or nothing; off = committed profile only")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)  # the profiled child of --pmc: solve steps + calibration copies only
    ap.add_argument("--scaling", default="weak", choices=("weak", "strong"), help="--gpus N: weak = every rank solves its own batch of the "
                    "workload's size (the default contract); strong = --total problems split over the ranks (config 4 proper: --total 1000000)")
    ap.add_argument("--total", type=int, default=0, help="problems of the whole job with --scaling strong (default: the workload's batch)")
    ap.add_argument("--no-transfer", action="store_true", help="skip the transfer-inclusive measurement (pinned host buffers, H2D / D2H overlapped)")
    ap.add_argument("--backend", default="auto", choices=("auto", "nccl", "gloo"), help="process-group backend for --gpus > 1: nccl (= RCCL) when "
                    "every rank has a GPU of its own; auto falls back to gloo when ranks have to share a device (diagnostics on a 1-GPU box)")
    ap.add_argument("--full", action="store_true", help="everything beside the headline as well: per-launch median, the other precision mode, "
                    "transfer-inclusive, two-stream and graph-replay rates, the RANSAC frame, the cost and check of the exchange (--gpus N), "
                    "PMC traffic, B = 1 latency, CPU baselines (the --no-* switches still skip single legs).  Without it a run sets up, "
                    "warms up, times the K steps and prints the line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed to DIR/<name>.npy "
                    "(float64; a fixed, seeded sample of rows when the arrays exceed 64 MB)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return _spawn_ranks(args.gpus)
    if "WORLD_SIZE" not in os.environ and not args.no_cpu_baseline:
        # the host baselines (cpu_baseline, its single_core entry) want their OpenMP threads bound one per core; the runtime reads these
        # when it loads, i.e. before torch / the host libraries are imported.  Single-process runs only: ranks sharing a node would
        # all bind to the same cores.  (Set without --full too: the timed region runs in the same process environment either way.)
        os.environ.setdefault("OMP_PROC_BIND", "close")
        os.environ.setdefault("OMP_PLACES", "cores")
        # ... and no more threads than the container may run: under a cgroup CPU quota (the round-6 GPU boxes: 16 CPUs of a 256-cpu host)
        # 128 threads burst for two milliseconds and are throttled for the rest of every 100 ms period
        q = _cpu_quota()
        if q and q < (os.cpu_count() or 1):
            os.environ.setdefault("OMP_NUM_THREADS", str(max(1, int(q))))

    import torch
    import torch.distributed as dist

    from cvxpnpl_amd import _lib, synth
    from cvxpnpl_amd.api import pnpl_batch  # noqa: F401  (import check: the product path)

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with {args.gpus} ranks, or without a launcher (bench.py starts them)")
    assert torch.cuda.is_available(), "bench.py needs a GPU; cvxpnpl_amd has no CPU fallback"
    n_dev = torch.cuda.device_count()
    shared = world > n_dev  # more ranks than GPUs (diagnostics on a small box): ranks share devices, RCCL cannot run
    torch.cuda.set_device(local_rank % n_dev)
    dev = torch.device("cuda", local_rank % n_dev)
    dist_on = world > 1 or args.force_dist
    backend = None
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        backend = args.backend if args.backend != "auto" else ("gloo" if shared else "nccl")
        # rendezvous + a tiny all_reduce and all_gather under a 60 s watchdog: a rank that cannot reach the others says so in one line and
        # exits (code 3) instead of hanging the run (cvxpnpl_amd.dist.init_with_preflight)
        from cvxpnpl_amd.dist import init_with_preflight
        preflight = init_with_preflight(backend, rank, world, device=dev, timeout_s=float(os.environ.get("CVXPNPL_PREFLIGHT_TIMEOUT", "60")))

    n_p, n_l, batch, sigma = WORKLOADS[args.workload]
    if args.workload == "pnp_scal":
        if args.n < 3:
            raise SystemExit("--workload pnp_scal needs --n N (points per problem, N >= 3)")
        n_p = args.n
        batch = int(min(125_000, max(1_000, 10_000_000 // n_p)))
    batch = args.batch or batch
    total_job = batch * world
    if args.scaling == "strong":  # total work fixed: contiguous, balanced shards (cvxpnpl_amd.dist.shard_range), ragged by at most one
        from cvxpnpl_amd.dist import shard_range
        total_job = args.total or batch
        lo_, hi_ = shard_range(total_job, rank, world)
        batch = hi_ - lo_
        if batch < 1:
            raise SystemExit(f"--scaling strong: {total_job} problems leave rank {rank} of {world} without work")
    sigma = sigma if args.sigma is None else args.sigma
    L = _lib.lib()

    # synthetic inputs, resident in HBM before the timed region (distinct per rank)
    ransac = args.workload == "ransac_n4_50k"
    if ransac:
        d = synth.make_ransac(batch, n_corr=100, outlier_frac=0.3, sigma=sigma, seed=46 + args.seed - 42 + 1000 * rank)
    else:
        d = synth.make_pnpl(batch, n_p, n_l, sigma, seed=args.seed + 1000 * rank)
    tt = lambda x: torch.as_tensor(x, device=dev).contiguous()  # noqa: E731
    p2, p3 = (tt(d["pts_2d"]), tt(d["pts_3d"])) if n_p else (None, None)
    l2, l3 = (tt(d["line_2d"]), tt(d["line_3d"])) if n_l else (None, None)
    K = tt(d["K"])
    R = torch.empty((batch, 3, 3), dtype=torch.float64, device=dev)
    t = torch.empty((batch, 3), dtype=torch.float64, device=dev)
    status = torch.empty((batch,), dtype=torch.int32, device=dev)
    iters = torch.empty((batch,), dtype=torch.int32, device=dev)
    cost = torch.empty((batch, 2), dtype=torch.float64, device=dev)
    work = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    over = {}
    for kv in args.opt:
        k, v = kv.split("=")
        over[k] = float(v) if k in ("eps", "rho", "alpha", "res_tol", "jacobi_tol", "rho_tail", "adapt_mu", "adapt_tau", "stall_lam", "stall_res", "stall_drop", "dual_shift") else int(v)
    if args.precision == "f64" and "f32_sweeps_until" not in over:
        over["f32_sweeps_until"] = 0  # the reference's precision (cvxpnpl.py:475-513: numpy float64 throughout) is the headline
    opts = _lib.default_opts(layout=args.layout, **over)
    ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else C.c_void_p(0)  # noqa: E731
    stream = torch.cuda.current_stream(dev)
    sh = C.c_void_p(stream.cuda_stream)

    from cvxpnpl_amd import dist as cdist

    gather = dist_on and not args.no_gather
    # records per rank in the exchange: the largest shard (strong scaling: shards differ by at most one problem and the short ones are
    # padded with zero records, so that the exchange stays ONE all_gather_into_tensor of equal slices)
    batch_pad = batch if args.scaling == "weak" else -(-total_job // world)
    to_root = args.collective == "gather"   # one consumer: only rank 0 receives (1/N of the all_gather's bytes per rank; none at all for N - 1 ranks)
    # TWO receive buffers: the exchange of step k may still be in flight when that of step k + 1 is enqueued (a step of config 4 is
    # ~0.45 ms, 91 MB arrive per rank per step: the exchange is of the order of the solve and must not be serialised behind its predecessor)
    gathered2 = [torch.empty((world * batch_pad, cdist.PACK), dtype=torch.float64, device=dev) if (gather and (rank == 0 or not to_root)) else None
                 for _ in range(2)]
    gathered = gathered2[0]
    MAX_IN_FLIGHT = 2
    gather_on = [True]  # (switched off for the second timed region that prices the exchange: config.collective.gather_ms_per_step)
    nstreams = max(1, args.streams)
    streams = [stream] + [torch.cuda.Stream(dev) for _ in range(nstreams - 1)]
    # one output set per stream so that overlapping steps do not write the same buffers; with the gather, two sets per stream:
    # the records of step k are packed and exchanged on a side stream while step k + 1 is already being solved into the other set
    nsets = nstreams * (2 if gather else 1)
    outs = [(R, t, status, iters, cost, work)] + [tuple(torch.empty_like(x) for x in (R, t, status, iters, cost, work))
                                                   for _ in range(nsets - 1)]
    step_no = [0]
    pending = []  # (work, packed) of the gather in flight: overlapped with the next batch's solve
    side = torch.cuda.Stream(dev) if gather else None   # pack + all_gather of the finished step, off the solve stream
    packed_done = [None] * nsets                         # event: the records of this output set have been packed (it may be overwritten)
    blocked = ((n_p + 2 * n_l >= 768) or (n_p + 2 * n_l >= 384 and batch >= 2048)) if args.blocked == "auto" else args.blocked == "1"  # cvxpnpl_amd.api.use_blocked_assembly: blocked assembly + cost-seam solve
    if blocked:
        nb = L.cvxpnpl_assemble_large_scratch_bytes(batch, n_p, n_l)
        asm_scratch = torch.empty((nb,), dtype=torch.uint8, device=dev)
        Bt = torch.empty((batch, 27), dtype=torch.float64, device=dev)
        Qt = torch.empty((batch, 45), dtype=torch.float64, device=dev)
    mid_events = []  # (event after the assembly) per timed step of the blocked path

    # Hand-over of a finished step from the solve stream to the side stream: a flag in device memory (cvxpnpl_stream_write_value /
    # cvxpnpl_stream_wait_value), not an event -- an event recorded between two solves costs the solve stream ~17 us per step
    # (rocprofv3 trace of --force-dist: the next solve kernel starts 17.6 us after the previous step's last kernel, 2 us without)
    step_flag = torch.zeros(2, dtype=torch.int64, device=dev) if gather else None  # [flag, "the wait gave up"]
    # The flag must only grow and a wait must be checked: with several solve streams the write kernels of different streams can complete
    # out of order (the library's store is an atomic max, so the flag never moves backwards -- but a wait for step n could then pass on
    # the strength of step n + 1): the flag hand-over is used with ONE solve stream only, events otherwise.  A wait that gave up (~0.25 s:
    # the two streams share a hardware queue, or a step took longer than that) sets step_flag[1]; it is checked after the warm-up AND
    # after the timed region -- a timed region in which a wait gave up is thrown away and repeated with events (round-3 advisor).
    handover = ["flag" if nstreams == 1 else "event"]

    def step():
        k = step_no[0] % nstreams
        oset = step_no[0] % nsets
        step_no[0] += 1
        sR, st_, sst, sit, sco, swk = outs[oset]
        with torch.cuda.stream(streams[k]):
            shk = C.c_void_p(streams[k].cuda_stream)
            if gather and packed_done[oset] is not None and not packed_done[oset].query():
                # the records of this set (two steps old) are normally packed long ago: a device-side wait only if they are not --
                # an event dependency on the solve stream costs ~10 us of bubble per step (measured)
                streams[k].wait_event(packed_done[oset])
            if blocked:
                rc = L.cvxpnpl_assemble_large_batch(batch, n_p, ptr(p2), ptr(p3), n_l, ptr(l2), ptr(l3), ptr(K), 0, ptr(Bt), ptr(Qt),
                                                    ptr(asm_scratch), nb, shk)
                if rc == 0 and timing[0]:
                    em = L.cvxpnpl_event_create()
                    L.cvxpnpl_event_record(em, shk)
                    mid_events.append(em)
                if rc == 0:
                    rc = L.cvxpnpl_solve_cost_batch(batch, ptr(Qt), ptr(Bt), C.byref(opts), ptr(sR), ptr(st_), ptr(sst), ptr(sit), ptr(sco),
                                                    C.c_void_p(0), ptr(swk), shk)
            else:
                rc = L.cvxpnpl_solve_batch(batch, n_p, ptr(p2), ptr(p3), n_l, ptr(l2), ptr(l3), ptr(K), 0, C.byref(opts),
                                           ptr(sR), ptr(st_), ptr(sst), ptr(sit), ptr(sco), C.c_void_p(0), ptr(swk), shk)
            if rc != 0:
                raise RuntimeError(_lib.last_error())
            if gather and gather_on[0]:  # north-star config 4: results of every shard on every rank (RCCL over xGMI)
                if handover[0] == "flag":
                    rc = L.cvxpnpl_stream_write_value(ptr(step_flag), step_no[0], shk)
                    if rc != 0:
                        raise RuntimeError(_lib.last_error())
                else:
                    solved = torch.cuda.Event()
                    solved.record(streams[k])
        if gather and gather_on[0]:
            # On the side stream: pack this step's records and all-gather them, while the solve stream goes on with the next
            # batch -- the exchange of step k runs under the solve of step k + 1 and nothing of it sits on the solve stream.
            with torch.cuda.stream(side):
                if handover[0] == "flag":
                    # (the EXPLICITLY fail-open wait: this script checks the give-up word after the warm-up and after the timed region
                    #  and repeats a region in which a wait gave up; cvxpnpl_stream_wait_value itself holds its stream until acknowledged)
                    rc = L.cvxpnpl_stream_wait_value_bounded(ptr(step_flag), step_no[0], 1 << 18, C.c_void_p(side.cuda_stream))
                    if rc != 0:
                        raise RuntimeError(_lib.last_error())
                else:
                    side.wait_event(solved)
                while len(pending) >= MAX_IN_FLIGHT:  # at most two exchanges in flight (one receive buffer each)
                    pending.pop(0)[0].wait()
                packed = cdist.pack_results(sR, st_, sst)
                if batch_pad != batch:
                    packed = torch.cat([packed, packed.new_zeros((batch_pad - batch, cdist.PACK))])
                ev_p = torch.cuda.Event()
                ev_p.record(side)
                packed_done[oset] = ev_p
                gbuf = gathered2[step_no[0] % 2]
                if to_root:
                    work_h = cdist.gather_to_root(packed, world * batch_pad, out=gbuf, async_op=True)[1]
                else:
                    _, work_h = cdist.gather_results(packed, world * batch_pad, out=gbuf, async_op=True)
                pending.append((work_h, packed))
        return k

    timing = [False]

    def barrier():
        if gather:
            with torch.cuda.stream(side):
                while pending:
                    pending.pop()[0].wait()
        while pending:
            pending.pop()[0].wait()
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def any_rank_gave_up():
        """has a flag wait given up on ANY rank?  The decision to switch the hand-over mode / to repeat a timed region changes the sequence of
        collectives a rank issues, so it must be the same on every rank: all_reduce(MAX) of the local flag (round-4 advisor)"""
        f = step_flag[1:2].to(torch.float64)
        if dist_on:
            dist.all_reduce(f, op=dist.ReduceOp.MAX)
        return int(f.item()) != 0

    for _ in range(args.warmup):
        step()
    barrier()
    if gather and (args.warmup == 0 or any_rank_gave_up()):
        # no warm-up to check the flag hand-over on, or a wait gave up on some rank (the solve and the side stream share a hardware
        # queue): events, on every rank
        handover[0] = "event"
        step()
        barrier()
    # timed region: exactly K steps; HIP events on the launch stream give the per-launch time
    handover_retries = 0
    while True:
        ev = [L.cvxpnpl_event_create() for _ in range(args.steps + 1)]
        del mid_events[:]
        timing[0] = True
        t0 = time.perf_counter()
        L.cvxpnpl_event_record(ev[0], sh)
        per_step_events = args.events_per_step or blocked or nstreams > 1
        for k in range(args.steps):
            ks = step()
            if per_step_events or k == args.steps - 1:
                L.cvxpnpl_event_record(ev[k + 1], C.c_void_p(streams[ks].cuda_stream))
        enqueue_s = time.perf_counter() - t0  # host time to enqueue the K steps (close to `elapsed` = the host, not the device, sets the pace)
        barrier()
        elapsed = time.perf_counter() - t0
        timing[0] = False
        if gather and handover[0] == "flag" and any_rank_gave_up():
            # a wait gave up inside the timed region of some rank: its side stream may have packed records the solve had not finished --
            # the run is invalid; every rank repeats it with event hand-over (the decision is collective: see any_rank_gave_up)
            handover[0] = "event"
            handover_retries += 1
            for e in ev + mid_events:
                L.cvxpnpl_event_destroy(e)
            continue
        break
    # (One event before the first and one after the last launch: the K launches run back to back and their average duration is the
    # events' span / K.  An event after EVERY launch puts a marker between two kernels of the stream: rocprofv3 shows the next
    # solve kernel starting 6 us after the previous step's last kernel instead of 2 -- 2-3 % of a 10 k step.  --events-per-step
    # brings them back; the blocked-assembly workloads keep them, they time the assembly kernel alone.)
    ms = C.c_float()
    launch_ms = []
    if nstreams == 1 and per_step_events:
        for k in range(args.steps):
            L.cvxpnpl_event_elapsed_ms(ev[k], ev[k + 1], C.byref(ms))
            launch_ms.append(ms.value)
    else:  # overlapping launches: only the aggregate span is meaningful
        L.cvxpnpl_event_elapsed_ms(ev[0], ev[args.steps], C.byref(ms))
        launch_ms = [ms.value / args.steps]
    asm_ms = []
    if blocked and nstreams == 1:  # duration of the assembly (the bandwidth-shaped, dominant kernel) alone
        for k in range(args.steps):
            L.cvxpnpl_event_elapsed_ms(ev[k], mid_events[k], C.byref(ms))
            asm_ms.append(ms.value)
    for e in ev + mid_events:
        L.cvxpnpl_event_destroy(e)
    elapsed_own = elapsed
    if dist_on:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())

    # ---- what the last timed step computed, copied off before anything else runs on these buffers: the arrays a caller of
    # cvxpnpl_solve_batch (cvxpnpl_solve_cost_batch on the blocked path) receives, and with the exchange the records it gathered
    if args.dump_outputs and rank == 0:
        last_out = outs[(step_no[0] - 1) % nsets]
        arrays = {k: x.cpu().numpy() for k, x in zip(("R", "t", "status", "iters", "cost", "work"), last_out)}
        if gather and gathered2[step_no[0] % 2] is not None:
            arrays["gathered_records"] = gathered2[step_no[0] % 2].cpu().numpy()
        _dump_outputs(args.dump_outputs, arrays)

    # ---- per-launch durations: >= 10 launches, each bracketed by its own pair of HIP events on the launch stream (SURVEY.md 8(d):
    # "median of >= 10 launches"; the reference reports mean AND median of its per-call wall times, benchmarks/toolkit/suites/
    # synth.py:183,221).  The events between launches cost the stream a few microseconds each, so `ms_per_step` (no events inside the
    # timed region) stays the judged figure and the median is reported beside it.
    per_launch = None
    if args.full and nstreams == 1 and not args.pmc_child:
        gather_on[0] = False
        nl = max(10, min(args.steps, 50))
        evs = [L.cvxpnpl_event_create() for _ in range(2 * nl)]
        for k in range(nl):
            L.cvxpnpl_event_record(evs[2 * k], sh)
            step()
            L.cvxpnpl_event_record(evs[2 * k + 1], sh)
        barrier()
        dur = []
        for k in range(nl):
            L.cvxpnpl_event_elapsed_ms(evs[2 * k], evs[2 * k + 1], C.byref(ms))
            dur.append(ms.value)
        for e in evs:
            L.cvxpnpl_event_destroy(e)
        dur = np.sort(np.array(dur))
        per_launch = {"n": nl, "median": float(np.median(dur)), "min": float(dur[0]), "p10": float(dur[int(0.1 * (nl - 1))]),
                      "p90": float(dur[int(round(0.9 * (nl - 1)))]), "max": float(dur[-1]), "mean": float(dur.mean()), "unit": "ms",
                      "how": "one HIP event before and one after every launch of a step, on the launch stream; no exchange"}
        gather_on[0] = True

    # ---- what the exchange costs a step: the same K steps without it (everything else identical), and the pack + all_gather alone
    gather_cost = None
    if gather and args.full:
        gather_on[0] = False
        for _ in range(min(args.warmup, 3)):
            step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        el_nog = time.perf_counter() - t0
        tm = torch.tensor([el_nog], dtype=torch.float64, device=dev)
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        el_nog = float(tm.item())
        gather_on[0] = True
        # the exchange alone, back to back on the side stream (pack + one all_gather_into_tensor of world x batch_pad records)
        ng = max(5, min(args.steps, 20))
        g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            sR, st_, sst = outs[0][0], outs[0][1], outs[0][2]
            for i in range(ng + 1):
                if i == 1:
                    g0.record(side)
                pk = cdist.pack_results(sR, st_, sst)
                if batch_pad != batch:
                    pk = torch.cat([pk, pk.new_zeros((batch_pad - batch, cdist.PACK))])
                if to_root:
                    cdist.gather_to_root(pk, world * batch_pad, out=gathered)
                else:
                    cdist.gather_results(pk, world * batch_pad, out=gathered)
            g1.record(side)
        barrier()
        alone = g0.elapsed_time(g1) / ng
        tm = torch.tensor([alone], dtype=torch.float64, device=dev)
        dist.all_reduce(tm, op=dist.ReduceOp.MAX)
        alone = float(tm.item())
        exposed = max(0.0, 1e3 * (elapsed - el_nog) / args.steps)
        gather_cost = {"alone": alone, "exposed": exposed, "hidden": max(0.0, alone - exposed), "unit": "ms per step",
                       "ms_per_step_without_exchange": 1e3 * el_nog / args.steps,
                       "bytes_received_per_rank_per_step": int(world * batch_pad * cdist.PACK * 8) if not to_root else {"rank 0": int(world * batch_pad * cdist.PACK * 8), "other ranks": 0},
                       "in_flight": MAX_IN_FLIGHT,
                       "how": "alone: pack + all_gather_into_tensor back to back on the side stream (events); exposed: ms_per_step minus the same "
                              "K steps without the exchange (both max over ranks); hidden = alone - exposed: what runs under the next step's solve. "
                              "With N ranks every rank receives N x the records of one shard: the exposed share grows with N."}

    # ---- the same K steps in the OTHER precision mode.  The timed region above runs at the reference's precision by default (float64
    # throughout, cvxpnpl.py:475-513; opts.f32_sweeps_until = 0); the library's default runs the sweeps of the first iterations of a
    # solve on single-precision columns.  Both are reported: value_all_f64 and value_mixed.
    other_mode = None
    if args.full and world == 1 and not dist_on and nstreams == 1 and not args.pmc_child and not args.no_f64_ab and not any(kv.startswith("f32_sweeps_until=") for kv in args.opt):
        opts_d = opts
        over_o = dict(over)
        over_o["f32_sweeps_until"] = -1 if args.precision == "f64" else 0
        opts = _lib.default_opts(layout=args.layout, **over_o)
        st_d, it_d = status.clone(), iters.clone()
        R_d = R.clone()
        for _ in range(args.warmup):
            step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        dto = time.perf_counter() - t0
        sto, ito = status.cpu().numpy(), iters.cpu().numpy()
        cert = (sto == 0) & (st_d.cpu().numpy() == 0)
        other_mode = {"value": batch * args.steps / dto, "unit": "poses/s", "ms_per_step": 1e3 * dto / args.steps,
                      "opts": f"f32_sweeps_until={over_o['f32_sweeps_until']}" + (" (the library's default: 64)" if over_o["f32_sweeps_until"] < 0 else ""),
                      "certified_frac": float((sto == 0).mean()), "mean_iters": float(ito.mean()), "max_iters_seen": int(ito.max()),
                      "status_equal_to_timed_region_frac": float((sto == st_d.cpu().numpy()).mean()),
                      "max_rot_diff_vs_timed_region_rad": float(synth.geodesic(R.cpu().numpy()[cert], R_d.cpu().numpy()[cert]).max()) if cert.any() else None}
        opts = opts_d
        step()  # (the outputs read below are those of the timed region's mode again)
        barrier()

    if args.pmc_child:
        # known-size copies with 4, 8 and 16 bytes per lane: what FETCH_SIZE / WRITE_SIZE report for them calibrates the
        # counters for this access width (MI355X guide, HBM section: only the wide streaming read is calibrated there)
        nbytes = 64 << 20
        src = torch.ones(nbytes // 8, dtype=torch.float64, device=dev)
        dst = torch.empty_like(src)
        for width in (4, 8, 16):
            rc = L.cvxpnpl_calibration_copy(ptr(src), ptr(dst), nbytes, width, sh)
            if rc != 0:
                raise RuntimeError(_lib.last_error())
        if ransac:  # the scoring kernel of the frame, so that the byte counters of the same passes see it too
            from cvxpnpl_amd.api import score_hypotheses
            for _ in range(8):
                score_hypotheses(R, t, K, tt(d["scene_2d"]), tt(d["scene_3d"]), 2.0, status=status, usable=(0, 2))
        torch.cuda.synchronize(dev)
        return None

    # ---- transfer-inclusive rate ("also with H2D/D2H included"; the reference times the whole call on the wall clock,
    # benchmarks/toolkit/suites/suite.py:75-85).  The boundary hands over device pointers, so a host caller pays PCIe both ways: inputs
    # from PINNED host buffers on a copy stream into one of two device input sets (the copy of step k + 1 runs under the solve of step
    # k), solve, pack, and the 13-double records back to pinned host memory on a third stream.  Never `value`.
    transfer = None
    if args.full and nstreams == 1 and world == 1 and not args.no_transfer and not blocked and not dist_on:
        # one pinned host buffer and one device buffer per input set: [pts_2d | pts_3d | line_2d | line_3d] back to back, so that a step
        # is ONE H2D copy (the C ABI takes the four device pointers separately: views into the buffer); events are created once
        parts = [np.ascontiguousarray(d[k]).ravel() for k, n_ in (("pts_2d", n_p), ("pts_3d", n_p), ("line_2d", n_l), ("line_3d", n_l)) if n_]
        offs = np.cumsum([0] + [x.size for x in parts])
        h_all = torch.from_numpy(np.concatenate(parts)).pin_memory()
        d_all = [torch.empty_like(h_all, device=dev) for _ in range(2)]

        def views(buf):
            out_, j = [], 0
            for n_ in (n_p, n_p, n_l, n_l):
                if n_:
                    out_.append(buf[int(offs[j]):int(offs[j + 1])]); j += 1
                else:
                    out_.append(None)
            return out_
        d_in = [views(x) for x in d_all]
        h_in = [h_all]
        d_pk = [torch.empty((batch, cdist.PACK), dtype=torch.float64, device=dev) for _ in range(2)]
        h_pk = [torch.empty((batch, cdist.PACK), dtype=torch.float64).pin_memory() for _ in range(2)]
        # Two streams, each with its own input set, output set and pinned record buffer, steps issued alternately; a step is H2D -> solve
        # -> pack -> D2H IN ORDER on its stream, so that nothing has to be synchronised across streams (measured on this stack: the
        # three-stream version with event hand-overs between a copy-in, a solve and a copy-out stream took 0.9-1.4 ms per 10 k step
        # against 0.31 ms for the plain one-stream sequence -- cross-stream events cost more than the copies they were to hide).
        t_streams = [stream, torch.cuda.Stream(dev)]
        t_outs = [outs[0], tuple(torch.empty_like(x) for x in (R, t, status, iters, cost, work))]

        def tstep(k, nst=2):
            b_ = k % nst
            with torch.cuda.stream(t_streams[b_]):
                shb = C.c_void_p(t_streams[b_].cuda_stream)
                d_all[b_].copy_(h_all, non_blocking=True)
                q2, q3, m2, m3 = d_in[b_]
                sR, st_, sst, sit, sco, swk = t_outs[b_]
                rc = L.cvxpnpl_solve_batch(batch, n_p, ptr(q2), ptr(q3), n_l, ptr(m2), ptr(m3), ptr(K), 0, C.byref(opts), ptr(sR), ptr(st_), ptr(sst),
                                           ptr(sit), ptr(sco), C.c_void_p(0), ptr(swk), shb)
                if rc == 0:
                    rc = L.cvxpnpl_pack_results(batch, ptr(sR), ptr(st_), ptr(sst), ptr(d_pk[b_]), shb)
                if rc != 0:
                    raise RuntimeError(_lib.last_error())
                h_pk[b_].copy_(d_pk[b_], non_blocking=True)

        def timed(nst):
            for k in range(4):
                tstep(k, nst)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for k in range(args.steps):
                tstep(k, nst)
            torch.cuda.synchronize(dev)
            return time.perf_counter() - t1
        # Both schedules are measured, twice each and interleaved (boxes differ: on the round-4 driver box the two-stream schedule was
        # 39 % SLOWER than the plain sequence, on the builder's box equal); `value` is the better one and says which -- a caller should
        # measure the same way before choosing.
        dt1 = min(timed(1), timed(1))
        dt2 = timed(2)
        dt1 = min(dt1, timed(1))
        dt2 = min(dt2, timed(2))
        # Round 6 (profiles/r06/xfer_numa.txt): on ONE box the two-stream schedule is bimodal -- 62-64 M poses/s in eight of ten processes, 43 M in
        # the other two, whatever NUMA node the feeding thread runs on (the one-stream figure is 33 M in all ten; PCIe Gen5 x16 every time).  The
        # slow mode belongs to the PAIR of streams a process happened to get (both repeats of a process agree): how the runtime maps the second
        # stream's copies and kernels onto hardware queues / copy engines.  So a pair that does not overlap is replaced: up to two fresh second
        # streams, the best pair counts, and the line says how many were tried.
        pair_ms = [1e3 * dt2 / args.steps]
        while dt2 > 0.62 * dt1 and len(pair_ms) < 3:
            t_streams[1] = torch.cuda.Stream(dev)
            d_new = min(timed(2), timed(2))
            pair_ms.append(1e3 * d_new / args.steps)
            dt2 = min(dt2, d_new)
        best_two = dt2 < dt1
        dtt = min(dt1, dt2)
        # the records that arrived on the host are those of the device-resident run (same inputs, same options)
        last = (args.steps - 1) % 2
        same = bool(torch.equal(torch.nan_to_num(h_pk[last]), torch.nan_to_num(cdist.pack_results(R, t, status).cpu())))
        bytes_in = int(h_all.numel()) * 8
        bytes_out = batch * cdist.PACK * 8
        transfer = {"value": batch * args.steps / dtt, "unit": "poses/s", "ms_per_step": 1e3 * dtt / args.steps,
                    "schedule": "two_streams" if best_two else "one_stream",
                    "one_stream": {"value": batch * args.steps / dt1, "ms_per_step": 1e3 * dt1 / args.steps},
                    "two_streams": {"value": batch * args.steps / dt2, "ms_per_step": 1e3 * dt2 / args.steps, "stream_pairs_tried_ms_per_step": pair_ms},
                    "h2d_bytes_per_step": int(bytes_in), "d2h_bytes_per_step": int(bytes_out),
                    "pcie_GBps_both_ways": (bytes_in + bytes_out) * args.steps / dtt / 1e9, "records_equal_device_run": same,
                    "host_link": _host_link(dev.index),
                    "how": "pinned host inputs (one buffer) -> H2D -> cvxpnpl_solve_batch -> cvxpnpl_pack_results -> D2H of the [batch][13] records to "
                           "pinned memory, in order on a stream; one_stream: a single stream, nothing overlapped; two_streams: steps alternate between "
                           "two such streams (each with its own buffers), so that one step's copies can run under the other's solve; wall clock over the "
                           "K steps, best of two interleaved runs each; `value` = the faster schedule (named in `schedule`), the other is the loser"}

    # ---- BASELINE config 5 as a frame: sample 4-subsets -> solve -> score every hypothesis against the scene (cvxpnpl_score_hypotheses) ->
    # arg-max -> refit on the consensus set.  `value` above is the solve alone (the metric's unit); this is the consumer's rate.
    ransac_frame = None
    if args.full and ransac and world == 1 and nstreams == 1:
        from cvxpnpl_amd import ransac as cr
        from cvxpnpl_amd.api import score_hypotheses

        sx, sX = tt(d["scene_2d"]), tt(d["scene_3d"])
        cnt = score_hypotheses(R, t, K, sx, sX, 2.0, status=status, usable=(0, 2))
        best = int(torch.argmax(cnt))
        # scoring alone, K launches, events on the stream
        e0, e1 = L.cvxpnpl_event_create(), L.cvxpnpl_event_create()
        score_hypotheses(R, t, K, sx, sX, 2.0, status=status, usable=(0, 2))
        L.cvxpnpl_event_record(e0, sh)
        for _ in range(args.steps):
            score_hypotheses(R, t, K, sx, sX, 2.0, status=status, usable=(0, 2))
        L.cvxpnpl_event_record(e1, sh)
        L.cvxpnpl_event_elapsed_ms(e0, e1, C.byref(ms))
        score_ms = ms.value / args.steps
        L.cvxpnpl_event_destroy(e0); L.cvxpnpl_event_destroy(e1)
        nf = max(3, min(args.steps, 20))
        kw = dict(n_hyp=batch, thresh=2.0, max_iters=opts.max_iters, eps=opts.eps, device=dev)
        fr = cr.ransac_pnp(sx, sX, K, seed=1, **kw)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for i in range(nf):
            fr = cr.ransac_pnp(sx, sX, K, seed=2 + i, **kw)
        torch.cuda.synchronize(dev)
        dtf = (time.perf_counter() - t1) / nf
        M_ = int(sx.shape[0])
        ransac_frame = {
            "frames_per_s": 1.0 / dtf, "ms_per_frame": 1e3 * dtf, "hypotheses_per_s_whole_frame": batch / dtf, "frames": nf,
            "what": "cvxpnpl_amd.ransac.ransac_pnp: draw 4-subsets on the device, cvxpnpl_solve_batch, cvxpnpl_score_hypotheses (2 px), arg-max, "
                    "refit on the consensus set assembled on the device from scene + inlier mask (cvxpnpl_assemble_subsets -> cvxpnpl_solve_cost_batch -> one "
                    "more scoring launch), reference defaults eps / max_iters; wall clock, one host synchronisation per frame (at its end)",
            "score_kernel": {"ms": score_ms, "hypotheses_per_s": batch / (1e-3 * score_ms), "scene_correspondences": M_,
                             "bound": "compute: H x M x ~30 flop (projection + divide + compare) against 100 B per hypothesis -- "
                                      f"{batch * M_ * 30 / (1e-3 * score_ms) / 1e12:.2f} TFLOP/s f64 of 78.6; HBM {batch * 104 / (1e-3 * score_ms) / 1e9:.1f} GB/s"},
            "last_frame": {"n_inliers": int(fr["n_inliers"]), "true_inliers": int(d["inlier"].sum()), "status": int(fr["status"]),
                           "rot_err_vs_gt_rad": float(synth.geodesic(fr["R"].cpu().numpy(), d["R_gt"])), "n_certified_hypotheses": int(fr["n_certified"])},
            "fixed_subsets": {"best_hypothesis_inliers": int(cnt[best]), "true_inliers": int(d["inlier"].sum()),
                              "best_rot_err_vs_gt_rad": float(synth.geodesic(R[best].cpu().numpy(), d["R_gt"])),
                              "all_inlier_subsets": int(d["inlier"][d["idx"]].all(axis=1).sum())},
        }

    overlapped = None
    if args.full and nstreams == 1 and world == 1 and not args.no_overlap and not blocked:
        # same K steps issued round-robin on two HIP streams: independent batches overlap, which
        # hides the few slow problems at the end of every launch (reported beside `value`)
        s2 = torch.cuda.Stream(dev)
        o2 = tuple(torch.empty_like(x) for x in (R, t, status, iters, cost, work))
        pair = [(stream, outs[0]), (s2, o2)]
        def step2(k):
            sk, (sR, st_, sst, sit, sco, swk) = pair[k % 2]
            rc = L.cvxpnpl_solve_batch(batch, n_p, ptr(p2), ptr(p3), n_l, ptr(l2), ptr(l3), ptr(K), 0, C.byref(opts),
                                       ptr(sR), ptr(st_), ptr(sst), ptr(sit), ptr(sco), C.c_void_p(0), ptr(swk),
                                       C.c_void_p(sk.cuda_stream))
            if rc != 0:
                raise RuntimeError(_lib.last_error())
        for k in range(4):
            step2(k)
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for k in range(args.steps):
            step2(k)
        torch.cuda.synchronize(dev)
        dt2 = time.perf_counter() - t1
        overlapped = {"streams": 2, "value": batch * args.steps / dt2, "unit": "poses/s", "ms_per_step": 1e3 * dt2 / args.steps}

    graph_replay = None
    if args.full and nstreams == 1 and world == 1 and not args.no_overlap and not blocked:
        # the same step captured once into a hipGraph and replayed K times on one stream (the launches of a step -- first
        # kernel + resume kernel -- become one graph launch); reported beside `value`
        gs = torch.cuda.Stream(dev)
        try:
            with torch.cuda.stream(gs):
                for _ in range(2):  # warm-up on the capture stream (its workspace is allocated here, not during capture)
                    rc = L.cvxpnpl_solve_batch(batch, n_p, ptr(p2), ptr(p3), n_l, ptr(l2), ptr(l3), ptr(K), 0, C.byref(opts), ptr(R), ptr(t), ptr(status),
                                               ptr(iters), ptr(cost), C.c_void_p(0), ptr(work), C.c_void_p(gs.cuda_stream))
            gs.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=gs):
                rc = L.cvxpnpl_solve_batch(batch, n_p, ptr(p2), ptr(p3), n_l, ptr(l2), ptr(l3), ptr(K), 0, C.byref(opts), ptr(R), ptr(t), ptr(status),
                                           ptr(iters), ptr(cost), C.c_void_p(0), ptr(work), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            for _ in range(3):
                g.replay()
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            for _ in range(args.steps):
                g.replay()
            torch.cuda.synchronize(dev)
            dtg = time.perf_counter() - t1
            graph_replay = {"value": batch * args.steps / dtg, "unit": "poses/s", "ms_per_step": 1e3 * dtg / args.steps}
        except Exception as e:  # diagnostics only: never fail the bench line over it
            graph_replay = {"error": str(e)[:200]}

    gather_check = None
    if gather and args.full:
        # the gathered records against the local results (all ranks solved a step into the same output set last): this rank's
        # slice must be its own records bit for bit, every other rank's slice finite rotations with an integer status
        barrier()
        last = (step_no[0] - 1) % nsets
        mine = cdist.pack_results(outs[last][0], outs[last][1], outs[last][2])
        glast = gathered  # (last written by the exchange-alone loop above: the records of output set 0, identical to every other set's)
        if glast is not None:
            sl_ = glast[rank * batch_pad:rank * batch_pad + batch]
            own = bool(torch.equal(torch.nan_to_num(sl_), torch.nan_to_num(mine)))
            stc = glast[:, 12]
            others = bool(((stc == stc.round()) & (stc >= 0) & (stc <= 4)).all().item())
        else:  # --collective gather: this rank only sends
            own = others = True
        flag = torch.tensor([1.0 if (own and others) else 0.0], dtype=torch.float64, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        gather_check = {"own_slice_bit_equal": own, "all_slices_valid_status": others, "all_ranks_ok": bool(flag.item() == 1.0),
                        "records": int(world * batch_pad), "held_by": "rank 0" if to_root else "every rank"}

    st = status.cpu().numpy()
    it = iters.cpu().numpy()
    wk = work.cpu().numpy()
    total = total_job * args.steps  # (weak: batch x world per step; strong: --total per step)
    value = total / elapsed         # elapsed = the SLOWEST rank's wall time over the K steps (all_reduce MAX above)
    coll = None
    if dist_on:
        # the line proves what it ran on: ranks counted by a collective, every rank's device, the slowest rank's time
        ones = torch.ones(1, dtype=torch.float64, device=dev)
        dist.all_reduce(ones)
        import socket as _so
        props = torch.cuda.get_device_properties(dev)
        mine_desc = {"rank": rank, "local_rank": local_rank, "host": _so.gethostname(), "pid": os.getpid(), "device_index": dev.index,
                     "device": props.name, "gcn_arch": getattr(props, "gcnArchName", None), "problems_per_step": batch,
                     "own_ms_per_step": 1e3 * elapsed_own / args.steps}
        descs = [None] * world
        dist.all_gather_object(descs, mine_desc)
        coll = {"backend": backend + (" (RCCL)" if backend == "nccl" else " (ranks share a device: diagnostics, not RCCL)"),
                "ranks": dist.get_world_size(), "ranks_seen": int(round(float(ones.item()))), "devices": min(world, n_dev),
                "distinct_devices": len({(x["host"], x["device_index"]) for x in descs}), "per_rank": descs,
                "preflight": preflight,  # rendezvous + tiny all_reduce / all_gather under a watchdog, before anything else (ms per stage)
                "value_is": "problems of all ranks over the K steps / the slowest rank's wall time (all_reduce MAX)",
                "handover": (("device flag (cvxpnpl_stream_write_value / _wait_value_bounded, checked)" if handover[0] == "flag" else "event") +
                             (f"; {handover_retries} timed region(s) discarded because a flag wait gave up" if handover_retries else "")) if gather else None,
                "exchange": ((f"one gather to rank 0 of {world} x {batch_pad} records of 13 doubles per step" if to_root else
                              f"one all_gather_into_tensor of {world} x {batch_pad} records of 13 doubles per step") +
                             f", on a side stream under the next steps' solves, up to {MAX_IN_FLIGHT} in flight" if gather else None)}
    mean_launch_s = float(np.mean(asm_ms if asm_ms else launch_ms)) * 1e-3  # the dominant kernel's launch
    bytes_per_launch = algorithmic_bytes(n_p, n_l) * batch
    achieved = bytes_per_launch / mean_launch_s / 1e9
    out = {
        "metric": "poses/sec (batched 10x10 SDP solves/sec)", "value": value, "unit": "poses/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True,
        "scaling": args.scaling, "vs_baseline": None,
        "dtype": ("f64" if opts.f32_sweeps_until == 0 else "f64 (f32 Jacobi sweeps)"),  # what the timed region ran; the other mode beside it
        "data": "synthetic",
        "config": {"workload": args.workload, "n_points": n_p, "n_lines": n_l, "problems_per_gpu_per_step": batch,
                   "layout_effective": {0: None, 1: "lane-hybrid", 2: "wave", 3: "quad-hybrid", 4: "penta"}.get(int(L.cvxpnpl_last_layout()) if hasattr(L, "cvxpnpl_last_layout") else 0),
                   "pixel_noise_sigma": sigma, "eps": opts.eps, "max_iters": opts.max_iters,
                   "precision": ("f64 throughout, as the reference (opts.f32_sweeps_until = 0); value_mixed is the same run with the library's default "
                                 "(single-precision Jacobi sweeps while a solve is younger than 64 iterations)" if opts.f32_sweeps_until == 0 else
                                 "f64: inputs, Gram sums, iterate, Newton polish, dual certificate, outputs; the Jacobi sweeps of the PSD projection "
                                 "(and the product (W + sigma I) V that starts them) run on f32 columns while a solve is younger than "
                                 f"opts.f32_sweeps_until = {opts.f32_sweeps_until if opts.f32_sweeps_until >= 0 else 64} iterations -- all of "
                                 "the quad / lane phases -- and in f64 afterwards; value_all_f64 is the same run with every sweep in f64"),
                   "streams": nstreams,
                   "parallelism": f"batch-sharded x{world}" + (", RCCL all_gather of results" if gather else "") +
                                  (f", strong scaling: {total_job} problems per step over the ranks" if args.scaling == "strong" else ""),
                   "collective": coll},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": 8000.0, "unit": "GB/s", "frac": achieved / 8000.0,
                     "traffic": None, "kernel": _kernel_name(opts.layout, batch, blocked, n_p + n_l), "mean_launch_ms": 1e3 * mean_launch_s,
                     "mean_step_ms": float(np.mean(launch_ms)), "host_enqueue_ms_per_step": 1e3 * enqueue_s / args.steps,
                     "algorithmic_bytes_per_problem": algorithmic_bytes(n_p, n_l),
                     "note": ("HBM-bound stage: 40 B read per point against 60 FMAs; the roofline is that of assemble_large_kernel, the solve "
                              "behind it is in mean_step_ms" if blocked else
                              "VALU/latency-bound by construction (~500 B and ~1e5-1e6 flop per pose), see DESIGN.md")},
        "solver": {"certified_frac": float((st == 0).mean()), "status_hist": np.bincount(st, minlength=5).tolist(),
                   "mean_iters": float(it.mean()), "max_iters_seen": int(it.max()),
                   "mean_jacobi_sweeps": float(wk[:, 1].mean())},
    }
    if not blocked:
        # the honest roofline of this path: counted iterations and sweeps of THIS step through the flop model, against the
        # FP64 vector peak
        fl = float(model_flops(n_p, n_l, it.astype(np.float64), wk[:, 1].astype(np.float64)).sum())
        out["roofline"]["flops"] = {"achieved": fl / mean_launch_s / 1e12, "peak": FP64_VECTOR_PEAK_TFLOPS, "unit": "TFLOP/s",
                                    "frac": fl / mean_launch_s / 1e12 / FP64_VECTOR_PEAK_TFLOPS, "flops_per_pose": fl / batch,
                                    "model": "SURVEY.md 8(d): 160 m + 400 + iters x 2 850 + sweeps x 9 000 + 2 000 per solve, iterations and sweeps "
                                             "counted by the kernels (status / iters / work outputs of this step); certificate attempts not modelled"}
    # HBM bytes and VALU instructions per launch: measured in THIS run (rocprofv3 --pmc child passes of this very
    # command, a few steps each) when rocprofv3 is there; otherwise a committed profile of the same library build
    # (profiles/pmc_traffic.json entries are stamped with the library's hash; a stale entry is refused).
    if args.full and rank == 0 and world == 1 and not args.pmc_child:
        pmc = None
        if args.pmc != "off":
            pmc = _measure_pmc(args)
        if pmc is None and args.pmc != "run":
            pmc = _pmc_from_profile(f"{args.workload}:{batch}")
        if pmc:
            out["roofline"]["traffic"] = pmc["hbm_bytes_per_launch"]
            out["roofline"]["traffic_source"] = pmc["source"]
            out["roofline"]["traffic_detail"] = {k: pmc[k] for k in ("fetch_bytes", "write_bytes", "by_kernel", "calibration") if k in pmc}
            if pmc.get("valu_insts_per_launch"):
                # what actually binds: VALU issue.  One wave64 VALU instruction occupies a SIMD for 4 cycles
                # (fp64 FMA is full rate on gfx950); 256 CUs x 4 SIMDs at the 2.4 GHz peak engine clock.
                n = pmc["valu_insts_per_launch"]
                out["roofline"]["valu"] = {"insts_per_launch": n, "insts_per_pose": n / batch,
                                           "issue_frac": n * 4.0 / (1024 * 2.4e9 * mean_launch_s), "source": "SQ_INSTS_VALU, same PMC passes"}
        else:
            out["roofline"]["traffic_source"] = "none: rocprofv3 not available and no profile of this library build committed"
    if gather_check:
        out["config"]["collective"]["gather_check"] = gather_check
    if gather_cost:
        out["config"]["collective"]["gather_ms_per_step"] = gather_cost
    if per_launch:
        out["median_ms_per_step"] = per_launch["median"]
        out["roofline"]["per_launch_ms"] = per_launch
    if transfer:
        out["transfer_inclusive"] = transfer
    if ransac_frame:
        out["ransac_frame"] = ransac_frame
        out["solver"]["rank_gt1_frac"] = float((st == 1).mean())
        out["solver"]["uncertified_frac"] = float(((st == 2) | (st == 4)).mean())
    f64_run = opts.f32_sweeps_until == 0
    if f64_run:
        out["value_all_f64"] = value  # (= value: the timed region is the all-float64 run)
    if other_mode:
        if f64_run:
            out["value_mixed"] = other_mode["value"]
            out["mixed"] = other_mode
        else:
            out["value_all_f64"] = other_mode["value"]
            out["all_f64"] = other_mode
    if overlapped:
        out["overlapped"] = overlapped
    if graph_replay:
        out["graph_replay"] = graph_replay
    if args.full and sigma == 0.0:
        geo = synth.geodesic(R.cpu().numpy(), d["R_gt"])
        out["solver"]["max_rot_err_vs_gt_rad"] = float(geo[st == 0].max())

    if args.full and rank == 0 and world == 1 and not args.pmc_child and not args.no_cpu_baseline:
        # the reference's own unit of timing: wall clock of ONE estimate_pose call (benchmarks/toolkit/suites/suite.py:75-85) -- here the drop-in
        # pnp() on the problem of the reference's examples/pnp.py, host arrays in, host poses out (H2D, one-problem launch, D2H, recovery)
        import cvxpnpl_amd as ca

        ex = synth.example_pnp()
        for _ in range(20):
            poses = ca.pnp(ex["pts_2d"], ex["pts_3d"], ex["K"])
        lat = []
        for _ in range(200):
            t0 = time.perf_counter()
            poses = ca.pnp(ex["pts_2d"], ex["pts_3d"], ex["K"])
            lat.append(time.perf_counter() - t0)
        lat = np.array(lat) * 1e6
        out["latency_b1_us"] = {"median": float(np.median(lat)), "p90": float(np.percentile(lat, 90)), "calls": len(lat),
                                "rot_err_vs_literal_rad": float(synth.geodesic(poses[0][0][None], ex["R_gt"][None])[0]), "n_poses": len(poses),
                                "what": "cvxpnpl_amd.pnp(pts_2d, pts_3d, K) on the six-point problem of the reference's examples/pnp.py, numpy in, "
                                        "[(R, t)] out: the reference's unit of timing (one estimate_pose call, suite.py:75-85)"}

    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        import oracle  # the checker, timed beside the product; never on the product path

        oracle.build()
        nthreads = oracle.num_threads()
        sample = args.cpu_sample or max(nthreads * 64, 512)  # ~10 s of CPU work on this box
        sample = min(sample, batch)
        sl = slice(0, sample)
        t0 = time.perf_counter()
        o = oracle.pnpl_batch(d["pts_2d"][sl] if n_p else None, d["line_2d"][sl] if n_l else None, d["pts_3d"][sl] if n_p else None,
                              d["line_3d"][sl] if n_l else None, d["K"], eps=1e-9, max_iters=2500)
        dt = time.perf_counter() - t0
        Rg = R[:sample].cpu().numpy()
        both = (st[:sample] == 0) & (o["n_poses"] == 1) & (o["iters"] < 2500)
        out["cpu_baseline_reference_path_port"] = {
            "value": sample / dt, "unit": "poses/s", "cores": nthreads, "kind": "port",
            "sample": f"first {sample} problems of the same batch, reference defaults eps=1e-9 max_iters=2500, "
                      f"OpenMP over problems, {dt:.1f} s",
            "max_rot_diff_vs_gpu_rad": float(synth.geodesic(Rg, o["R"][:, 0])[both].max()) if both.any() else None,
            "converged_frac": float((o["iters"] < 2500).mean()),
            "what": "the oracle: the reference's path restated (explicit C, N, A; SCS's published HSDE-ADMM, dense, no equilibration / "
                    "acceleration): a stand-in for cvxpnpl + scs, which is not installable here; real SCS is likely 10-100x faster than this port",
        }
        # beside it: THIS solver's algorithm (solver_core.h compiled for the host with g++, OpenMP over problems) on all
        # host cores -- the ratio to `value` isolates what the GPU adds over the same arithmetic on the host
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import hostsim

        hostsim.build()
        hs_n = min(batch, max(sample * 16, 8192))
        hsl = slice(0, hs_n)
        hargs = (d["pts_2d"][hsl] if n_p else None, d["pts_3d"][hsl] if n_p else None, d["line_2d"][hsl] if n_l else None,
                 d["line_3d"][hsl] if n_l else None, d["K"])
        # Repeatability (round-5 verdict: 0.28-0.44 M poses/s across boxes): the OpenMP threads are pinned one per core (OMP_PROC_BIND /
        # OMP_PLACES, set in main() before any OpenMP runtime loads), half a second of untimed passes brings the clocks up and touches every
        # thread's stack, and the figure is the MEDIAN pass, with the spread beside it.
        t_w = time.perf_counter()
        warm = []
        while time.perf_counter() - t_w < 0.5:
            t0 = time.perf_counter()
            h = hostsim.solve_batch(*hargs)
            warm.append(time.perf_counter() - t0)
        # A pass over 10 k problems takes ~2 ms on 128 threads, and passes that short are bimodal (2 ms, or 90 ms when threads had gone to
        # sleep between two parallel regions: profiles/r06, 2.0-4.6 M poses/s from one box to the next).  So the timed passes run the sample
        # TILED until one pass is >= 50 ms of work: the wake-up of a thread is then 1 % of a pass instead of all of it -- and, where the container
        # has a cgroup CPU quota (cpu_quota_cores in the record), a pass spans several scheduling periods, so that the figure is the SUSTAINED
        # rate the quota allows and not the burst of a period's first two milliseconds (round 6: 4.6 M poses/s in bursts, 0.5 M sustained).
        tile = int(min(64, max(1, np.ceil(0.05 / max(min(warm), 1e-4)))))
        targs = tuple(np.concatenate([a] * tile) if (a is not None and a.ndim > 2) else a for a in hargs)
        hostsim.solve_batch(*targs)
        passes = []
        while sum(passes) < 1.5 and len(passes) < 100:  # at least a second and a half of work
            t0 = time.perf_counter()
            hostsim.solve_batch(*targs)
            passes.append(time.perf_counter() - t0)
        reps = len(passes)
        dth = float(np.median(passes)) / tile
        spread = [float(np.percentile(passes, 10)) / tile, float(np.percentile(passes, 90)) / tile]
        bothh = (st[:hs_n] == 0) & (h["status"] == 0)
        # (ii) of SURVEY.md 8(d): the same build on ONE pinned core
        prev_threads = hostsim.set_threads(1)
        one_n = min(hs_n, 2048)
        oargs = tuple(a[:one_n] if (a is not None and a.ndim > 2) else a for a in hargs)
        hostsim.solve_batch(*oargs)
        singles = []
        while sum(singles) < 1.5 and len(singles) < 50:
            t0 = time.perf_counter()
            hostsim.solve_batch(*oargs)
            singles.append(time.perf_counter() - t0)
        hostsim.set_threads(prev_threads)
        single = {"value": one_n / float(np.median(singles)), "unit": "poses/s", "cores": 1,
                  "sample": f"first {one_n} problems, one OpenMP thread (bound: OMP_PROC_BIND={os.environ.get('OMP_PROC_BIND')}), median of {len(singles)} passes"}
        # THIS is `cpu_baseline` (round-2 verdict): the honest host number.  The restated reference path above is a dense,
        # un-equilibrated restatement of SCS and says nothing about the real SCS; it stays in the line as a labelled extra.
        out["cpu_baseline"] = {
            "value": hs_n / dth, "unit": "poses/s", "cores": nthreads, "kind": "port",
            "what": "this solver's own algorithm (cvxpnpl_amd/csrc/solver_core.h, the scalar statement the lane kernel instantiates) compiled "
                    "for the host with g++ -O2, float64 throughout, OpenMP over problems on all host threads: the same arithmetic without the GPU. "
                    "(cvxpnpl + scs itself cannot be installed or timed in this image: SURVEY.md section 0.2; the restated reference path with "
                    "SCS's published algorithm is cpu_baseline_reference_path_port)",
            "sample": f"first {hs_n} problems of the same batch, same options, g++ -O2 host build of the device algorithm header, "
                      f"OpenMP over problems (threads bound one per core), tiled x{tile} per timed pass, {1e3 * dth:.2f} ms per {hs_n} problems, median of {reps} passes",
            "pass_ms_p10_p90": [1e3 * spread[0], 1e3 * spread[1]],
            "burst": {"value": hs_n / float(min(warm)), "unit": "poses/s", "what": f"the fastest single pass over the {hs_n} problems (~{1e3 * min(warm):.1f} ms): all threads "
                      "running before any cgroup CPU quota of the scheduling period is used up -- not a sustainable rate where there is a quota"},
            "cpu_quota_cores": _cpu_quota(), "host_cpus": os.cpu_count(),
            "single_core": single,
            "reference_python_overhead_us": REFERENCE_PYTHON_OVERHEAD_US,
            "reference_python_overhead_note": "measured in SURVEY.md section 6 with the reference imported in the build container and scs stubbed out: "
                                              "what cvxpnpl.pnp spends per pose in Python around the solve (constraint assembly, vech, recovery); it EXCLUDES "
                                              "the SDP solve, so 1e6 / 224 = 4 464 poses/s per core is an upper bound on the reference's rate, not a measurement of it",
            "max_rot_diff_vs_gpu_rad": float(synth.geodesic(R[:hs_n].cpu().numpy(), h["R"])[bothh].max()) if bothh.any() else None,
            "certified_frac": float((h["status"] == 0).mean()),
        }
    if dist_on:
        dist.destroy_process_group()
    return out if rank == 0 else None


DUMP_LIMIT_BYTES = 64 * 10**6


def _dump_outputs(dirname, arrays):
    """--dump-outputs: every array as DIR/<name>.npy in float64 (the integer outputs convert exactly).  Over DUMP_LIMIT_BYTES the files
    hold the same fixed, seeded sample of rows of every array with that many rows, and DIR/rows_<n>.npy the sampled row indices."""
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arrays.items()}
    row_bytes = {}  # rows -> bytes per row over the arrays with that many rows
    for a in arrays.values():
        row_bytes[len(a)] = row_bytes.get(len(a), 0) + a.nbytes // max(len(a), 1)
    if sum(n * b for n, b in row_bytes.items()) > DUMP_LIMIT_BYTES:
        # (+ 8: the index file of each row count; 1 KB per file for the .npy headers)
        frac = (DUMP_LIMIT_BYTES - 1024 * (len(arrays) + len(row_bytes))) / sum(n * (b + 8) for n, b in row_bytes.items())
        rows = {}
        for n in row_bytes:
            rows[n] = np.sort(np.random.default_rng(n).choice(n, size=int(n * frac), replace=False))
            np.save(os.path.join(dirname, f"rows_{n}.npy"), rows[n].astype(np.float64))
        arrays = {k: a[rows[len(a)]] for k, a in arrays.items()}
    for k, a in arrays.items():
        np.save(os.path.join(dirname, f"{k}.npy"), a)


def _lib_hash():
    import hashlib

    from cvxpnpl_amd import _lib
    return hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]


def _pmc_from_profile(key):
    path = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if not os.path.exists(path):
        return None
    e = json.load(open(path)).get(key)
    if not e or e.get("lib_sha16") != _lib_hash():
        return None  # no entry, or one measured on another build of the kernels
    return e


def _kname(raw):
    """kernel name without return type, anonymous-namespace prefix and argument list (template arguments kept)"""
    n = raw.replace("(anonymous namespace)::", "").replace("void ", "")
    return n.split("(")[0].strip()


def _pmc_pass(counters, child_args, tmp):
    """one rocprofv3 --pmc pass over a child run of this script; {kernel: {counter: [value per dispatch]}}"""
    import collections
    import csv
    import glob
    import subprocess

    out_dir = os.path.join(tmp, "_".join(counters))
    cmd = ["rocprofv3", "--pmc"] + counters + ["--output-format", "csv", "-d", out_dir, "-o", "p", "--",
           sys.executable, os.path.abspath(__file__)] + child_args
    env = dict(os.environ, TMPDIR=tmp)
    r = subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=600)
    files = glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True)
    if r.returncode != 0 or not files:
        print(f"bench.py: rocprofv3 pass {counters} failed ({r.returncode}): {r.stderr[-400:]}", file=sys.stderr)
        return None
    per = collections.defaultdict(lambda: collections.defaultdict(float))
    for f in files:
        for row in csv.DictReader(open(f)):
            per[(_kname(row["Kernel_Name"]), row["Dispatch_Id"])][row["Counter_Name"]] += float(row["Counter_Value"])
    acc = collections.defaultdict(lambda: collections.defaultdict(list))
    for (k, _), d in per.items():
        for c, v in d.items():
            acc[k][c].append(v)
    return acc


def _measure_pmc(args):
    """HBM bytes (FETCH_SIZE + WRITE_SIZE, separate passes: they do not fit one on gfx950) and VALU instructions per
    launch of the solve kernels, from rocprofv3 --pmc passes over a short child run of the same workload; counter
    calibration from known-size copies in the same passes.  None when rocprofv3 is not available."""
    import shutil
    import tempfile

    if not shutil.which("rocprofv3"):
        return None
    steps, warm = 6, 2
    child = ["--pmc-child", "--steps", str(steps), "--warmup", str(warm), "--workload", args.workload, "--layout", str(args.layout),
             "--seed", str(args.seed), "--no-cpu-baseline", "--no-overlap", "--pmc", "off", "--precision", args.precision]
    if args.batch:
        child += ["--batch", str(args.batch)]
    if args.n:
        child += ["--n", str(args.n)]
    if args.blocked != "auto":
        child += ["--blocked", args.blocked]
    if args.sigma is not None:
        child += ["--sigma", str(args.sigma)]
    for kv in args.opt:
        child += ["--opt", kv]
    tmp = tempfile.mkdtemp(prefix="cvxpnpl_pmc_")
    try:
        res = {}
        for counters in (["FETCH_SIZE"], ["WRITE_SIZE"], ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_WAVES"]):
            acc = _pmc_pass(counters, child, tmp)
            if acc is None:
                return None
            for k, d in acc.items():
                res.setdefault(k, {}).update(d)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    solve = {k: v for k, v in res.items() if "solve_" in k or "resume_" in k or "rescue_" in k or "assemble_" in k or "ipm_quad_" in k}
    extra = {k: v for k, v in res.items() if "score_kernel" in k}  # (reported in by_kernel, not part of a solve step)
    calib = {k: v for k, v in res.items() if "calibration_copy" in k}
    if not solve:
        return None

    def per_step(name):  # sum over the kernels of one step of the mean per launch (warm-up launches included: same work)
        return sum(sum(v[name]) / len(v[name]) for v in solve.values() if name in v)

    # calibration: a copy of B bytes must show B bytes fetched and B written (rocprofv3 reports KB)
    nbytes = float(64 << 20)
    cal = {}
    for k, v in calib.items():
        w = "4" if "<4>" in k else ("16" if "<16>" in k else "8")
        cal[w] = {"fetch_reported_over_true": (sum(v["FETCH_SIZE"]) / len(v["FETCH_SIZE"])) * 1024 / nbytes if "FETCH_SIZE" in v else None,
                  "write_reported_over_true": (sum(v["WRITE_SIZE"]) / len(v["WRITE_SIZE"])) * 1024 / nbytes if "WRITE_SIZE" in v else None}
    ref = cal.get("8", {})
    ff = ref.get("fetch_reported_over_true") or 1.0
    wf = ref.get("write_reported_over_true") or 1.0
    fetch, write = per_step("FETCH_SIZE") * 1024 / ff, per_step("WRITE_SIZE") * 1024 / wf
    by_kernel = {k: {"fetch_bytes": (sum(v["FETCH_SIZE"]) / len(v["FETCH_SIZE"])) * 1024 / ff if "FETCH_SIZE" in v else None,
                     "write_bytes": (sum(v["WRITE_SIZE"]) / len(v["WRITE_SIZE"])) * 1024 / wf if "WRITE_SIZE" in v else None,
                     "valu_insts": sum(v["SQ_INSTS_VALU"]) / len(v["SQ_INSTS_VALU"]) if "SQ_INSTS_VALU" in v else None,
                     "waves": sum(v["SQ_WAVES"]) / len(v["SQ_WAVES"]) if "SQ_WAVES" in v else None} for k, v in list(solve.items()) + list(extra.items())}
    return {"hbm_bytes_per_launch": fetch + write, "fetch_bytes": fetch, "write_bytes": write,
            "valu_insts_per_launch": per_step("SQ_INSTS_VALU"), "salu_insts_per_launch": per_step("SQ_INSTS_SALU"),
            "lds_insts_per_launch": per_step("SQ_INSTS_LDS"), "waves_per_launch": per_step("SQ_WAVES"), "by_kernel": by_kernel,
            "calibration": {"bytes_per_lane": cal, "applied": "8 (the width of this path's global accesses): reported / true",
                            "fetch_factor": ff, "write_factor": wf},
            "lib_sha16": _lib_hash(),
            "source": f"measured in this run: rocprofv3 --pmc FETCH_SIZE | WRITE_SIZE | SQ_INSTS_* (3 separate child passes of this command, "
                      f"{steps + warm} launches each), KB*1024, divided by the factor the same passes report for a known 64 MiB copy "
                      "with 8-byte accesses, summed over the kernels of one step"}


def _spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves -- the same command under
    torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1 at a free port) -- and hand rank 0's
    JSON line through.  Returns the parsed line."""
    import socket
    import subprocess

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=sys.stderr, env=env, text=True)
    line = None
    for ln in proc.stdout.splitlines():
        if ln.startswith("{"):
            line = ln
        else:
            print(ln, file=sys.stderr)
    if proc.returncode != 0 or line is None:
        raise SystemExit(f"bench.py: the {n}-rank run failed (exit {proc.returncode})")
    return json.loads(line)


def _only_json_on_stdout():
    """The contract is ONE JSON line on stdout.  Libraries print there too (RCCL writes its version banner
    to stdout through C stdio, which a pipe flushes at exit, i.e. AFTER the JSON line): everything the run
    prints goes to stderr, and only the final line is written to the real stdout."""
    sys.stdout.flush()
    real = os.dup(1)
    os.dup2(2, 1)
    try:
        out = main()
    finally:
        sys.stdout.flush()
        try:
            C.CDLL(None).fflush(None)  # C stdio buffers (the RCCL banner) -> stderr, before stdout is restored
        except OSError:
            pass
        os.dup2(real, 1)
        os.close(real)
    if out is not None:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    _only_json_on_stdout()
