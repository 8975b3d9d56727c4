#!/usr/bin/env python3
"""bench.py — k-mers scanned/sec of the MI355X SPeQ scan path (BASELINE.json `metric`).

One "step" = one pass of the hot path (exact search of every k-mer window + unique-to-one-group tally) over this
rank's batch of synthetic 150-bp reads already resident in HBM; the K steps of a timed region are one job whose summed
G + 2 counters are all-reduced over RCCL once at its end, inside the region (N > 1). Default workload = BASELINE config 2 (10 variants x 50 kb, 1M reads per GPU, k = 21, global
mode) -> `value`.

A plain run (`bench.py --gpus 1 --steps K --warmup W`) sets up, warms up, times ONE region of K steps pipelined over the
streams, scans batch 0 once more for the line's `check`, writes --dump-outputs DIR if given (dump_outputs) and prints
the line: `value`, `ms_per_step` (the region's time / K) and `check`; `roofline`, `one_stream`, `overlap`,
`cpu_baseline` are null and `lines` is empty. Everything else is behind --full: five regions (`value` their median), each
also timed on one stream and with per-launch HIP events (roofline), the checks of every stream's counters, the
instrumented twin, the LF-step and k-mer-table kernels, the PCIe-inclusive scan, the CPU baselines and the secondary
lines (compact objects under "lines" in the JSON):
  * "local_mode": config 2 in the reference's default Phred-weighted mode (fixed_accuracy 0, arg_parse.h:23);
  * "k31": BASELINE config 3 (50 variants x 3 isolates, k = 31) at its full 10 M reads per GPU — at N = 8 the
    per-rank shard of config 4 (100 M reads over 8 GPUs, 12.5 M each);
  * "cli_e2e" (N = 1): `bin/speq index` + `bin/speq scan` processes on config 3's 10 M reads written as FASTQ
    (reference defaults but k = 31: Phred-weighted, .dat pass, EM loop; src/main.cpp:25-31 -> fm_scanner.cpp:309-545);
    median of 3 cached-.dat scans each started on an idle GPU, and one started right after another (back_to_back);
  * "k70_reference_defaults": config 2's reads at the reference CLI's defaults (k = 70, Phred-weighted);
  * "k70_err05": the same at 0.5 % sequencing errors (the upper end of Illumina error rates);
  * "local_varq" (N = 1): config 2, Phred-weighted, with Illumina-like per-base qualities (synth "variable");
  * "cfg5_paired" / "cfg5_paired_local": BASELINE config 5's index (200 variants x 5 isolates), paired 2 x 150 bp,
    k = 31, on a per-GPU sample of the config's pairs (--cfg5-pairs);
  * "fastq_e2e" (N = 1): speq_scan_fastq on config 2's reads written as a FASTQ file (page cache warm).
Weak scaling: every rank scans its own shard of the deterministic read stream.

stdout: ONE compact JSON line on rank 0 (< 8 KB; `compact_result`); the full per-line detail (work counters, U
vectors, paths) goes to --detail (default with --full: profiles/r06/bench_detail_n<N>.json; without: not written).
Launch: python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR]. N > 1 under torch.distributed.run (WORLD_SIZE must equal N),
or without a launcher: bench.py then starts torch.distributed.run over N local ranks itself (launch_plan).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level parameters)
OCC_ENTRY_BYTES = 64   # algorithmic bytes per k-mer = k LF steps x 2 occ loads x 64 B
LINE_LIMIT = 8000      # bytes of the stdout line (the driver parsed 9.3 KB in round 2, not 22.8 KB in round 3)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1,
                   help="ranks (one process per GPU); N > 1 without a launcher starts torch.distributed.run itself")
    p.add_argument("--transport", default=os.environ.get("SPEQ_BENCH_TRANSPORT", "auto"),
                   help="N > 1 collective: rccl (one GPU per rank), host (gloo + host sockets; ranks may share a "
                        "GPU), auto (rccl when every rank has its own GPU)")
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--config", type=int, default=2, help="BASELINE.json config number (1-5) of the headline")
    p.add_argument("--reads", type=int, default=0, help="override reads per GPU")
    p.add_argument("--k", type=int, default=0, help="override k")
    p.add_argument("--err", type=float, default=0.001, help="substitution error rate of the headline reads")
    p.add_argument("--prefix-q", type=int, default=12)
    p.add_argument("--pair-steps", type=int, default=1)
    p.add_argument("--label-table", default="auto", help="auto|0|1 (auto: only for >= 4 M-symbol indexes)")
    p.add_argument("--mode", choices=["global", "local"], default="global")
    p.add_argument("--qual", default="q40", help="quality profile of the headline reads (speq_amd.synth.QUALITY_PROFILES)")
    p.add_argument("--ilp", type=int, default=0, help="windows per lane of the LF-step kernel (1|2; 0 = default)")
    p.add_argument("--gpu-build", type=int, default=1, help="build the index on the GPU (1) or host SA-IS (0)")
    p.add_argument("--triple-steps", type=int, default=1, help="three-symbol occ planes (1) or not (0)")
    p.add_argument("--kmer-table", type=int, default=1,
                   help="per-k interval table (1, default) or LF steps for every window (0)")
    p.add_argument("--tune", action="append", default=[],
                   help="extra launch tuning key=value (speq_device_set_tuning), e.g. ilp_kt=2; repeatable")
    p.add_argument("--no-lf-compare", action="store_true",
                   help="skip timing the LF-step kernel beside the table kernel")
    p.add_argument("--streams", type=int, default=2,
                   help="HIP streams the timed steps alternate between (each with its own counters): consecutive "
                        "batches overlap, the next scan's workgroups taking the CUs the previous one's drain leaves "
                        "(default 2; 1 = every step on one stream, each waiting for the one before)")
    p.add_argument("--full", action="store_true",
                   help="everything beside the headline: five timed regions (their median is `value`), each also "
                        "timed on one stream and with per-launch events (roofline), the result checks, the LF-step / "
                        "k-mer-table kernels, the PCIe-inclusive scan, the CPU baselines and the secondary lines. "
                        "Without it: set-up, warm-up, one timed region of --steps steps, the result line")
    p.add_argument("--dump-outputs", default="", metavar="DIR",
                   help="after the timed steps, write the counters the last timed step's scan left in its caller's "
                        "arrays as DIR/<name>.npy (float64; see dump_outputs)")
    p.add_argument("--regions", type=int, default=0,
                   help="timed regions of K steps per line (0 = default: 1, or with --full 5, SURVEY §8(d): the median "
                        "of 5 after warm-up); with --full each region times the pipelined steps, the same steps on one "
                        "stream, and one stream with per-launch events")
    p.add_argument("--allreduce", choices=["job", "step"], default="job",
                   help="N > 1 (or --transport rccl): job = the K steps of a timed region are one job whose summed "
                        "counters are all-reduced once at its end (default; SURVEY 8(d)); step = every step's "
                        "counters zeroed and all-reduced after its scan (diagnostic)")
    p.add_argument("--no-extra", action="store_true", help="skip the secondary lines")
    p.add_argument("--only", default="", help="comma-separated secondary lines to run (default: all)")
    p.add_argument("--k31-reads", type=int, default=0, help="reads per GPU of the k=31 line (0 = config 3/4)")
    p.add_argument("--cfg5-pairs", type=int, default=4_000_000, help="pairs per GPU of the config-5 lines (0: skip)")
    p.add_argument("--no-fastq", action="store_true", help="skip the FASTQ end-to-end lines (fastq_e2e, cli_e2e)")
    p.add_argument("--cpu-seconds", type=float, default=15.0, help="target CPU-baseline sample duration (headline)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-pcie", action="store_true", help="skip the PCIe-inclusive host-buffer measurement")
    p.add_argument("--detail", default="",
                   help="full-detail JSON path (default: with --full profiles/r06/bench_detail_n<N>.json, else none)")
    return p.parse_args(argv)


def host_cpu_info() -> dict:
    """The CPUs this process may use: affinity mask, machine count and the cgroup CPU quota (the GPU box gives
    each job a share of a larger machine: its nproc shows every CPU, the quota says how many it may keep busy)."""
    aff = len(os.sched_getaffinity(0))
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = int(q) / int(per)
    except (OSError, ValueError):
        pass
    threads = aff if quota is None else max(1, min(aff, int(quota)))
    return {"threads": threads, "affinity_cpus": aff, "nproc": os.cpu_count(), "cgroup_cpu_quota": quota,
            "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS"), "cpu_model": cpu_model(),
            "rule": "threads = min(affinity CPUs, cgroup CPU quota) (all CPUs this job may keep busy)"}


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


class LaunchError(RuntimeError):
    pass


def launch_plan(gpus: int, env) -> str:
    """What `python bench.py --gpus N` does in this process (decided before anything touches a GPU):
      "relaunch": N > 1 and no launcher around us (WORLD_SIZE unset) -> start N ranks under torch.distributed.run
                  as a child process and exit with its status;
      "run":      this process is one rank of a launcher whose WORLD_SIZE equals --gpus, or the only process (N = 1).
    A launcher whose WORLD_SIZE differs from --gpus is an error (the line would report the wrong n_gpus)."""
    if gpus < 1:
        raise LaunchError(f"--gpus {gpus}: at least one GPU")
    ws = env.get("WORLD_SIZE")
    if ws is None or ws == "":
        return "relaunch" if gpus > 1 else "run"
    if int(ws) != gpus:
        raise LaunchError(f"WORLD_SIZE={ws} from the launcher but --gpus {gpus}: they must agree")
    return "run"


def pick_transport(requested: str, world: int, n_devices: int) -> str:
    """The ranks' collective transport. "rccl": ncclAllReduce over xGMI, one rank per GPU (the product path the
    driver's 8-GPU run measures); "host": torch.distributed over gloo plus the product's host-socket transport
    (speq_comm_connect, SPEQ_COMM_HOST), so N ranks can share fewer GPUs (RCCL refuses two ranks on one GPU).
    "auto": rccl when every rank has its own GPU, else host."""
    if requested not in ("auto", "rccl", "host"):
        raise LaunchError(f"--transport {requested}: auto, rccl or host")
    if world <= 1:
        # one rank: no collective, unless RCCL is asked for explicitly (a one-member communicator: the N > 1 code
        # path — process group, RCCL streams, per-step all-reduce on the communication stream — on one GPU)
        return "rccl" if requested == "rccl" and n_devices >= 1 else "none"
    if requested == "auto":
        return "rccl" if n_devices >= world else "host"
    return requested


def free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def relaunch_cmd(gpus: int, argv: list, port: int) -> list:
    """torch.distributed.run over N local ranks (rendezvous on 127.0.0.1), each running this file with the same
    arguments; WORLD_SIZE then equals --gpus in every rank."""
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={gpus}",
            "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + list(argv)


_PIPE_STREAMS = {}  # device -> the bench's extra HIP streams (created first, in Ctx; used by run_workload)


class Ctx:
    def __init__(self, a):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.a = torch, dist, a
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        n_dev = self.n_dev = torch.cuda.device_count()
        self.transport = pick_transport(a.transport, self.world, n_dev)
        # ranks beyond the visible GPUs share them round-robin (host transport only: RCCL needs one GPU per rank)
        self.device = self.local_rank % max(1, n_dev)
        torch.cuda.set_device(self.device)
        self.dev_t = torch.device(f"cuda:{self.device}")
        # The pipeline's HIP streams (run_workload) are created FIRST, before torch's NCCL process group and the
        # product's RCCL communicator create theirs: HIP gives a new stream a hardware queue of its own until
        # GPU_MAX_HW_QUEUES (4) are in use and then shares the least used one, so streams created after RCCL's could
        # share a queue with each other and the batches would run one after the other. The one-stream
        # vs pipelined ratio of every line ("overlap") shows whether they did.
        n_extra = max(0, int(getattr(a, "streams", 1)) - 1) + (1 if self.transport in ("rccl", "host") else 0)
        _PIPE_STREAMS[self.device] = [torch.cuda.Stream(self.dev_t) for _ in range(n_extra)]
        # HIP binds a stream to its hardware queue at the stream's first command, not at its creation: without one
        # before RCCL's init the pipeline's streams came to share a queue with each other (one-member RCCL test:
        # pipelined 0.98x the one-stream rate). So every stream, the current one included, runs a command now.
        for s in [torch.cuda.current_stream(self.dev_t)] + _PIPE_STREAMS[self.device]:
            with torch.cuda.stream(s):
                torch.zeros(1, device=self.dev_t).add_(1)
        torch.cuda.synchronize(self.dev_t)
        if self.transport == "rccl":
            if self.world == 1:  # forced at one rank (tests): a one-member group over the loopback rendezvous
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", str(free_port()))
                os.environ.setdefault("RANK", "0")
                os.environ.setdefault("WORLD_SIZE", "1")
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{self.device}"))
        elif self.transport == "host":
            dist.init_process_group("gloo")
        self.comm = None
        from speq_amd import Comm
        if self.transport == "rccl":
            # the product's own collective (C ABI speq_allreduce_*, ncclAllReduce over xGMI): rank 0's 128-byte
            # RCCL id reaches the other ranks through torch.distributed, which keeps only the barrier and timing
            uid = torch.zeros(Comm.ID_BYTES, dtype=torch.uint8, device=self.dev_t)
            if self.rank == 0:
                uid.copy_(torch.frombuffer(bytearray(Comm.unique_id()), dtype=torch.uint8))
            dist.broadcast(uid, 0)
            self.comm = Comm(self.world, self.rank, bytes(uid.cpu().numpy().tobytes()))
        elif self.transport == "host":
            # the same C ABI calls (speq_allreduce_u64/_f64 on the device counters) over the product's host-socket
            # transport; the rendezvous file is keyed by this launch (torch.distributed.run's port and run id)
            rdzv = os.path.join(os.environ.get("TMPDIR", "/tmp"),
                                "speq_bench_rdzv_%s_%s" % (os.environ.get("MASTER_PORT", "0"),
                                                           os.environ.get("TORCHELASTIC_RUN_ID", "none")))
            self.comm = Comm.connect(self.world, self.rank, rdzv, device=self.device, transport=Comm.HOST)

    def barrier(self):
        if self.world > 1:
            self.dist.barrier()

    def allreduce_max(self, x: float) -> float:
        if self.world <= 1:
            return float(x)
        dev = self.dev_t if self.transport == "rccl" else "cpu"
        t = self.torch.tensor([x], dtype=self.torch.float64, device=dev)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())


def ax_request_bytes(st: dict, k: int, n_reads: int, local: bool) -> dict:
    """Bytes k_scan_ax REQUESTS per launch (L1/L2 requests, not fabric bytes), from the work counters of its
    instrumented twin (speq_scan_reads_device_stats, same scan, same results), by kind at the size it issues it:
      read offsets 8 B per read; staging 16 B of bases + 16 B of qualities per 16-base chunk;
      anchor buckets 64 B per lookup (phase 1 and phase 2); run granules 16 B each (counted);
      Bloom-filter words 8 B per deferred window; candidate granules ceil(k/32) + 1 x 16 B per phase-2 verification;
      local mode: single quality bytes."""
    hw = (k + 31) // 32
    parts = {
        "offsets": 8.0 * n_reads,
        "staging": 32.0 * st["chunks"],
        "anchor_buckets": 64.0 * (st["lookup_lanes"] + st["p2_probes"]),
        "run_granules": 16.0 * st["run_granules"],
        "filter": 8.0 * st["deferred"],
        "verify_granules": 16.0 * (hw + 1) * st["p2_verify"],
        "quality_bytes": float(st["qual_bytes"]) if local else 0.0,
    }
    return {"total": sum(parts.values()), "parts": parts}


def workload_key(cfg: int, k: int, mode: str, n_reads: int, kernel: str, qual_profile: str = "q40",
                 err: float = 0.001) -> str:
    """profiles/traffic.json key of one workload + kernel (scripts/summarize_profile.py --traffic-key)."""
    return (f"cfg{cfg}_k{k}_{mode}_reads{n_reads}_{kernel}" + ("" if qual_profile == "q40" else f"_{qual_profile}")
            + ("" if abs(err - 0.001) < 1e-12 else f"_err{err:g}"))


def traffic_lookup(key: str) -> dict | None:
    """Measured FABRIC bytes per launch of this exact workload and kernel, or None. Only round-4 entries count: they
    carry `fabric_bytes_per_launch`, computed from the L2's memory-side request counters with the request sizes
    calibrated on gfx950 (scripts/calibrate_counters.sh); earlier entries were raw FETCH_SIZE."""
    prof = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        tj = json.load(open(prof))
    except (OSError, ValueError):
        return None
    e = tj.get(key)
    if not e or "fabric_bytes_per_launch" not in e:
        return None
    e = dict(e)
    e["source"] = os.path.normpath(os.path.join("profiles", e["source"]))
    return e


def roofline_of(key: str, avg_kernel_s: float, request_bytes: float | None, compulsory_bytes: float, k: int,
                kmers: int) -> dict:
    """The roofline object of one line. frac = fabric bytes per launch (PMC, calibrated; profiles/traffic.json) ÷ the
    launch's mean duration (HIP events, this run) ÷ 8 TB/s. Beside it: l2_request_frac (bytes the kernel requests,
    mostly L2 hits), compulsory_frac (the read stream that must cross the fabric once: bases + qualities + offsets)
    and survey_model_frac (SURVEY §8(d)'s 2·k·64 B per k-mer: k uncached LF steps, not what this kernel does)."""
    tr = traffic_lookup(key)
    t = max(avg_kernel_s, 1e-12)
    gbs = lambda b: b / t / 1e9  # noqa: E731
    if tr:
        traffic, basis, source = tr["fabric_bytes_per_launch"], "fabric", tr["source"]
    else:
        traffic, basis, source = None, "compulsory", "no PMC profile of this workload: compulsory read bytes"
    achieved = gbs(traffic if traffic is not None else compulsory_bytes)
    return {
        "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
        "traffic": traffic, "traffic_frac": (gbs(traffic) / HBM_PEAK_GBS) if traffic is not None else None,
        "frac_basis": basis, "traffic_source": source, "avg_kernel_ms": t * 1e3,
        "traffic_rocprof_kernel_ms": (tr.get("kernel_steady_state_ns_rocprof") or 0) / 1e6 if tr else None,
        "l2_hit_rate": tr.get("l2_hit_rate") if tr else None,
        "l2_request_frac": (gbs(request_bytes) / HBM_PEAK_GBS) if request_bytes else None,
        "compulsory_frac": gbs(compulsory_bytes) / HBM_PEAK_GBS,
        "survey_model_frac": gbs(kmers * 2 * k * OCC_ENTRY_BYTES) / HBM_PEAK_GBS,
        "kernel": None,
    }


KERNEL_TAG = {0: "lf", 1: "kt", 2: "kt", 3: "ax"}  # speq_device_get_tuning("last_kernel")
KERNEL_NAME = {0: "k_scan<KT=false> (LF steps)", 1: "k_scan<KT> (k-mer table)", 2: "k_scan_kt (k-mer table)",
               3: "k_scan_ax (anchor-and-extend)"}


def u_sha1(u) -> str:
    return hashlib.sha1(np.asarray(u, dtype=np.int64).tobytes()).hexdigest()[:16]


def timed_outputs(snap, snap_job, ran, last_stream: int) -> dict:
    """name -> float64 array: what the scans of the last timed region left in the arrays their caller handed to
    speq_scan_reads_device, read back after the last timed step. `counts` = [T, ambiguous, U[0..G)] of the stream the
    last step ran on (the kernel adds into them: with --allreduce job the sum of that stream's scans of the region;
    64-bit integers, exact in float64 below 2^53), `weights` = its W[0..G) (Phred-weighted mode only), and
    `counts_stream<i>` / `weights_stream<i>` the same of every stream that ran a step; with a communicator
    `job_counts` / `job_weights`, the streams' sums all-reduced over the ranks."""
    out = {}

    def put(name, c):
        out["counts" + name] = c[0].astype(np.float64)
        if c[1] is not None:
            out["weights" + name] = c[1].astype(np.float64)

    put("", snap[last_stream])
    for i, c in enumerate(snap):
        if ran[i]:
            put(f"_stream{i}", c)
    if snap_job is not None:
        out["job_counts"] = snap_job[0].astype(np.float64)
        if snap_job[1] is not None:
            out["job_weights"] = snap_job[1].astype(np.float64)
    return out


DUMP_LIMIT = 64 << 20  # bytes of one --dump-outputs directory


def dump_outputs(path: str, arrays: dict) -> list:
    """Writes every array as <path>/<name>.npy (a few KB here: G + 2 counters and G weights per stream; nothing is
    sampled). Returns the names."""
    if sum(v.nbytes for v in arrays.values()) > DUMP_LIMIT:
        raise RuntimeError("--dump-outputs: the timed outputs exceed 64 MB")
    os.makedirs(path, exist_ok=True)
    for name, v in arrays.items():
        np.save(os.path.join(path, name + ".npy"), v)
    return sorted(arrays)


def run_workload(ctx: Ctx, cfg_no: int, k: int, n_reads: int, mode: str, steps: int, warmup: int,
                 with_lf: bool, with_pcie: bool, with_cpu: bool, cpu_seconds: float, prepared=None,
                 qual_profile: str = "q40", err: float = 0.001, cpu_extra_ports: bool = False) -> dict:
    """Builds the index of BASELINE config `cfg_no` (or reuses `prepared`), stages this rank's reads in HBM, times
    `steps` scans and returns the measurement (plus the objects for reuse). qual_profile: synth.QUALITY_PROFILES;
    err: substitution rate (the reads of `prepared` are regenerated when either differs)."""
    torch, a = ctx.torch, ctx.a
    from speq_amd import DeviceIndex, FmIndex, synth

    c = dict(synth.CONFIGS[cfg_no])
    paired, G = c["paired"], c["n_variants"]
    if prepared is None:
        ref = synth.make_reference(c["n_variants"], c["n_isolates"], c["length"])
        t0 = time.time()
        idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=a.prefix_q, pair_steps=bool(a.pair_steps),
                            label_table="auto" if a.label_table == "auto" else bool(int(a.label_table)),
                            threads=16, gpu_device=ctx.device if a.gpu_build else None,
                            triple_steps=bool(a.triple_steps))
        build_s = time.time() - t0
        dev = DeviceIndex(idx, ctx.device)
        if a.ilp:
            dev.tune(ilp=a.ilp)
        dev.tune(kmer_table=a.kmer_table)
        for kv in a.tune:
            key, val = kv.split("=")
            dev.tune(**{key: int(val)})
        prepared = dict(ref=ref, idx=idx, dev=dev, build_s=build_s, reads_key=None, cfg=cfg_no)
    if prepared.get("reads_key") != (qual_profile, err, n_reads):
        prepared.update(d_seq=None, d_qual=None, d_off=None)
        reads = synth.make_reads(prepared["ref"], n_reads, start_index=ctx.rank * n_reads, paired=paired,
                                 err_rate=err)
        reads = synth.apply_quality_profile(reads, qual_profile)
        prepared.update(reads=reads, reads_key=(qual_profile, err, n_reads),
                        d_seq=torch.from_numpy(reads.seq).to(ctx.dev_t),
                        d_qual=torch.from_numpy(reads.qual).to(ctx.dev_t),
                        d_off=torch.from_numpy(reads.offsets.astype(np.int64)).to(ctx.dev_t))
    ref, idx, dev, reads = prepared["ref"], prepared["idx"], prepared["dev"], prepared["reads"]
    d_seq, d_qual, d_off = prepared["d_seq"], prepared["d_qual"], prepared["d_off"]
    ktab = dev.prepare(k)  # per-k index structure (like the .dat cache): built once, outside the timed region
    lens = np.diff(reads.offsets).astype(np.int64)
    kmers_per_step = int(np.maximum(lens - k + 1, 0).sum())
    read_bytes = int(reads.offsets[-1])
    d_counts = torch.zeros(G + 2, dtype=torch.int64, device=ctx.dev_t)
    d_w = torch.zeros(G, dtype=torch.float64, device=ctx.dev_t)
    local = mode == "local"
    stream = torch.cuda.current_stream(ctx.dev_t).cuda_stream
    # --streams S: step i runs on stream i % S, each stream with its own batch of reads (stream 0: `reads`; stream
    # s > 0: the reads after every rank's batch 0, so no batch's reads are another's) and its own counters, so the
    # scans of consecutive batches overlap: the next scan's workgroups take the CUs the previous one's drain leaves
    # (a pipeline of S batches in flight). The scans add into their stream's counters; with more ranks the job's
    # summed counters are all-reduced once at its end (finish_job; --allreduce step: after every step, on one
    # communication stream in step order). Every stream's counters of the last timed job are checked against its
    # batch scanned alone on one stream; the per-launch kernel time (events) is taken with S = 1.
    n_str = max(1, int(getattr(a, "streams", 1)))
    xkey = (qual_profile, err, n_reads, n_str)
    if prepared.get("x_key") != xkey:
        xb = []
        for si in range(1, n_str):
            r = synth.make_reads(prepared["ref"], n_reads, start_index=(si * ctx.world + ctx.rank) * n_reads,
                                 paired=paired, err_rate=err)
            r = synth.apply_quality_profile(r, qual_profile)
            xb.append(dict(reads=r, seq=torch.from_numpy(r.seq).to(ctx.dev_t),
                           qual=torch.from_numpy(r.qual).to(ctx.dev_t),
                           off=torch.from_numpy(r.offsets.astype(np.int64)).to(ctx.dev_t)))
        prepared.update(x_key=xkey, x_batches=xb)
    # The extra streams (and the communication stream) were created once per process, before any other (Ctx): HIP
    # maps a new stream to a hardware queue of its own until GPU_MAX_HW_QUEUES (4) are in use, then shares the least
    # used one — a stream created per line (or after RCCL's) would sooner or later share another's queue, and the
    # batches would run one after the other (scripts/overlap_probe.py).
    ps = _PIPE_STREAMS.setdefault(ctx.device, [])
    while len(ps) < n_str - 1 + (ctx.comm is not None):
        ps.append(torch.cuda.Stream(ctx.dev_t))

    def kmers_at_k(offsets) -> int:  # windows of every read at THIS call's k (never cached across k)
        return int(np.maximum(np.diff(offsets).astype(np.int64) - k + 1, 0).sum())

    bufs = [dict(seq=d_seq, qual=d_qual, off=d_off, n=reads.n, kmers=kmers_per_step, cnt=d_counts, w=d_w,
                 stream=torch.cuda.current_stream(ctx.dev_t))]
    for si, b in enumerate(prepared["x_batches"]):
        bufs.append(dict(seq=b["seq"], qual=b["qual"], off=b["off"], n=b["reads"].n, kmers=kmers_at_k(b["reads"].offsets),
                         cnt=torch.zeros(G + 2, dtype=torch.int64, device=ctx.dev_t),
                         w=torch.zeros(G, dtype=torch.float64, device=ctx.dev_t), stream=ps[si]))
    comm_stream = ps[n_str - 1] if ctx.comm is not None and n_str > 1 else None
    ev_scan = [torch.cuda.Event() for _ in bufs]
    ev_comm = [torch.cuda.Event() for _ in bufs]
    rot = {"i": 0, "n": 1, "kmers": 0, "ran": [0] * len(bufs)}
    # --allreduce job (default): the K steps of a timed region are ONE job over K batches — every scan adds into its
    # stream's counters (the kernel's atomics accumulate), and the job ends with one all-reduce of the summed G + 2
    # counters (+ G weights) inside the timed region, as `speq scan` ends a shard ("to completion of the
    # final ncclAllReduce"; replaces the future.get() sums of /root/reference/src/fm_scanner.cpp:224-233).
    # --allreduce step: every step zeroes its counters and all-reduces them after its scan (diagnostic).
    per_step = getattr(a, "allreduce", "job") == "step"
    job_cnt = torch.zeros(G + 2, dtype=torch.int64, device=ctx.dev_t)
    job_w = torch.zeros(G, dtype=torch.float64, device=ctx.dev_t)

    def allreduce(cnt, w, st):
        ctx.comm.allreduce_u64(cnt.data_ptr(), G + 2, st)  # RCCL all-reduce of the G+2 counters over xGMI
        if local:
            ctx.comm.allreduce_f64(w.data_ptr(), G, st)

    def zero(b):
        b["cnt"].zero_()
        if local:
            b["w"].zero_()

    def step():
        i = rot["i"] % rot["n"]
        rot["i"] += 1
        b, s = bufs[i], bufs[i]["stream"]
        rot["kmers"] += b["kmers"]
        rot["ran"][i] += 1
        with torch.cuda.stream(s):
            if per_step:
                zero(b)
            dev.scan_device(b["seq"].data_ptr(), b["qual"].data_ptr(), b["off"].data_ptr(), b["n"], k,
                            b["cnt"].data_ptr(), b["w"].data_ptr(), paired=paired, local=local,
                            stream=s.cuda_stream)
        if ctx.comm is not None and per_step:
            if rot["n"] == 1:  # one stream: the all-reduce follows the scan on it
                allreduce(b["cnt"], b["w"], s.cuda_stream)
            else:
                ev_scan[i].record(s)
                comm_stream.wait_event(ev_scan[i])
                allreduce(b["cnt"], b["w"], comm_stream.cuda_stream)
                ev_comm[i].record(comm_stream)
                s.wait_event(ev_comm[i])  # the stream's next step zeroes these counters after their all-reduce

    def finish_job():
        """(job mode) the end of the timed job: the streams' counters summed and all-reduced once."""
        if ctx.comm is None or per_step:
            return
        cs = comm_stream if (comm_stream is not None and rot["n"] > 1) else bufs[0]["stream"]
        for i in range(rot["n"]):
            if cs is not bufs[i]["stream"]:
                ev_scan[i].record(bufs[i]["stream"])
                cs.wait_event(ev_scan[i])
        with torch.cuda.stream(cs):
            job_cnt.copy_(bufs[0]["cnt"])
            for b in bufs[1:rot["n"]]:
                job_cnt.add_(b["cnt"])
            if local:
                job_w.copy_(bufs[0]["w"])
                for b in bufs[1:rot["n"]]:
                    job_w.add_(b["w"])
        allreduce(job_cnt, job_w, cs.cuda_stream)

    def timed_run(n_steps, n_warm, events=True, pipelined=False):
        rot["i"], rot["n"] = 0, n_str if pipelined else 1
        for _ in range(n_warm):
            step()
        torch.cuda.synchronize()
        rot["kmers"] = 0  # k-mers of the timed steps only
        rot["ran"] = [0] * len(bufs)
        for b in bufs:
            zero(b)
        ctx.barrier()
        torch.cuda.synchronize()
        dev.timing(events)
        if events:
            dev.timing_read()  # reset
        t0 = time.perf_counter()
        for _ in range(n_steps):
            step()
        t_enq = time.perf_counter() - t0
        finish_job()
        torch.cuda.synchronize()
        ctx.barrier()
        elapsed = time.perf_counter() - t0
        kernel_ms, launches = dev.timing_read() if events else (0.0, 0)
        dev.timing(False)
        expect = sum(bufs[i % rot["n"]]["kmers"] for i in range(n_steps))
        if rot["kmers"] != expect:  # the timed k-mers are the steps' batches' windows at this k
            raise RuntimeError(f"timed k-mers {rot['kmers']} != {expect} of the {n_steps} steps' batches at k={k}")
        rot["enqueue_s"] = t_enq
        return ctx.allreduce_max(elapsed), kernel_ms, launches

    def counters(cnt, w):
        return cnt.cpu().numpy().copy(), (w.cpu().numpy().copy() if local else None)

    def times(x, n):  # n x a batch's counters (the job's sum of n scans of that batch)
        return x[0] * n, (x[1] * n if local else None)

    def same(x, y, rtol=1e-12) -> bool:
        return np.array_equal(x[0], y[0]) and (not local or np.allclose(x[1], y[1], rtol=rtol, atol=0))

    def scan_once(b, reduce):  # batch b scanned alone on the current stream (+ all-reduced over the ranks)
        cnt = torch.zeros(G + 2, dtype=torch.int64, device=ctx.dev_t)
        w = torch.zeros(G, dtype=torch.float64, device=ctx.dev_t)
        dev.scan_device(b["seq"].data_ptr(), b["qual"].data_ptr(), b["off"].data_ptr(), b["n"], k, cnt.data_ptr(),
                        w.data_ptr(), paired=paired, local=local, stream=stream)
        if reduce and ctx.comm is not None:
            allreduce(cnt, w, stream)
        torch.cuda.synchronize()
        return counters(cnt, w)

    # the median of `regions` timed regions of K steps after one warm-up. Each region times
    #   (p) the K steps as a job runs them (step i on stream i % S): `value`;
    #   (1) the same K steps on one stream, each waiting for the one before: `one_stream` and the overlap ratio
    #       (p) / (1) in k-mers/s — near 1.0 the streams ran one after the other (e.g. shared hardware queues);
    #   (e) (1) again with HIP events around every launch: the per-launch kernel time of the roofline (the events
    #       cost 6-10 µs per step, scripts/step_overhead.py, so (p) and (1) run without them).
    # Without --full: (p) alone, in one region of exactly K timed steps, and of the checks below only `counts`.
    full = bool(getattr(a, "full", False))
    with_lf, with_pcie, with_cpu = with_lf and full, with_pcie and full, with_cpu and full
    n_reg = max(1, int(getattr(a, "regions", 0)) or (5 if full else 1))
    el_p, el_1, el_e, kms, enq = [], [], [], [], []
    snap_p = snap_job = None
    ran_p = [0] * len(bufs)
    for r_i in range(n_reg):
        e, _, _ = timed_run(steps, warmup if r_i == 0 else 0, events=False, pipelined=True)
        el_p.append(e)
        enq.append(rot["enqueue_s"])
        timed_kmers = rot["kmers"]
        ran_p = list(rot["ran"])
        if r_i == n_reg - 1:  # every stream's counters of the last pipelined job (checked below; --dump-outputs)
            snap_p = [counters(b["cnt"], b["w"]) for b in bufs]
            snap_job = counters(job_cnt, job_w) if (ctx.comm is not None and not per_step) else None
            last_stream = (rot["i"] - 1) % rot["n"]  # the stream of the last timed step
        if not full:
            continue
        if n_str > 1:
            el_1.append(timed_run(steps, 0, events=False)[0])
            kmers_1 = rot["kmers"]
        e, kmsum, launches = timed_run(steps, 0, events=True)
        el_e.append(e)
        kms.append(kmsum / max(1, launches))
    elapsed = float(np.median(el_p))
    elapsed_ev = float(np.median(el_e)) if el_e else None
    kernel_med = float(np.median(kms)) if kms else None
    prepared["last_outputs"] = timed_outputs(snap_p, snap_job, ran_p, last_stream)
    # Checks of the last pipelined job: every stream's counters equal (scans of that stream) x its batch scanned
    # alone on one stream (per step mode: one scan, all-reduced); the job's all-reduced total equals the sum over
    # the streams of the same, all-reduced. `counts`: batch 0 scanned alone and all-reduced (the line's check, and
    # what the CPU baseline is compared with).
    alone_local = [scan_once(b, reduce=False) if (full and ran_p[i]) else None for i, b in enumerate(bufs)]
    counts_t = scan_once(bufs[0], reduce=True)
    for i, b in enumerate(bufs):
        if not ran_p[i] or not full:
            continue  # (fewer timed steps than streams: this stream's batch never ran)
        want = (scan_once(b, reduce=True) if ctx.comm is not None else alone_local[i]) if per_step else \
            times(alone_local[i], ran_p[i])
        if not same(snap_p[i], want, rtol=1e-11):
            raise RuntimeError(f"the pipelined scans of stream {i} disagree with its batch scanned alone")
    if snap_job is not None and full:
        tot = None
        for i, b in enumerate(bufs):
            if ran_p[i]:
                x = times(scan_once(b, reduce=True), ran_p[i])
                tot = x if tot is None else (tot[0] + x[0], (tot[1] + x[1]) if local else None)
        if not same(snap_job, tot, rtol=1e-11):
            raise RuntimeError("the job's all-reduced counters disagree with its batches scanned alone")
    # batch 0's counters after a one-stream timed run: `steps` scans summed (job), or one scan (+ all-reduced) per step
    job1 = ((counts_t[0] if ctx.comm is not None else alone_local[0][0]) if per_step else
            alone_local[0][0] * steps) if full else None
    d_counts.copy_(torch.from_numpy(counts_t[0]).to(ctx.dev_t))
    if local:
        d_w.copy_(torch.from_numpy(counts_t[1]).to(ctx.dev_t))
    timing = {
        "regions": n_reg, "steps_per_region": steps, "allreduce": "step" if per_step else "job",
        "value_median": timed_kmers * ctx.world / elapsed,
        "value_min": timed_kmers * ctx.world / max(el_p), "value_max": timed_kmers * ctx.world / min(el_p),
        "ms_per_step": [round(x / steps * 1e3, 5) for x in el_p],
        "host_enqueue_ms_per_step": [round(x / steps * 1e3, 5) for x in enq],
    }
    if kms:
        timing.update({
            "avg_kernel_ms": [round(x, 5) for x in kms],
            "avg_kernel_ms_median": kernel_med, "avg_kernel_ms_min": min(kms), "avg_kernel_ms_max": max(kms)})
    if el_1:
        e1 = float(np.median(el_1))
        timing["one_stream"] = {"value": kmers_1 * ctx.world / e1, "ms_per_step": e1 / steps * 1e3,
                                "ms_per_step_all": [round(x / steps * 1e3, 5) for x in el_1]}
        # k-mers/s pipelined over k-mers/s on one stream (equal-length reads: one-stream ms per step / pipelined)
        timing["overlap"] = (timed_kmers / elapsed) / (kmers_1 / e1)
    counts = d_counts.cpu().numpy()
    weights = d_w.cpu().numpy() if local else None
    table_on = bool(ktab["table_bytes"])
    hot_kernel = dev.tuning("last_kernel")

    lf = prev = None
    if with_lf and a.kmer_table and table_on and hot_kernel == 3:
        # the previous hot path (k-mer-table kernel for k <= 31, else LF steps) on the same reads
        dev.tune(ax_scan=0)
        pv_el, pv_ms, pv_n = timed_run(steps, 1)
        pv_counts = d_counts.cpu().numpy()  # (the sum of the `steps` scans of batch 0 on this rank)
        kind = dev.tuning("last_kernel")
        dev.tune(ax_scan=1)
        if not np.array_equal(pv_counts, job1):
            raise RuntimeError("k-mer-table scan disagrees with the anchor-and-extend scan")
        prev = {"value": kmers_per_step * ctx.world * steps / pv_el, "unit": "k-mers/s",
                "avg_kernel_ms": pv_ms / max(1, pv_n), "path": KERNEL_NAME.get(kind, str(kind))}
    if with_lf and a.kmer_table and table_on:
        dev.tune(kmer_table=0, ax_scan=0)
        lf_el, lf_ms, lf_n = timed_run(steps, 1)
        lf_counts = d_counts.cpu().numpy()
        dev.tune(kmer_table=1, ax_scan=1)
        if not np.array_equal(lf_counts, job1):
            raise RuntimeError("LF-step scan disagrees with the hot path")
        lf = {"value": kmers_per_step * ctx.world * steps / lf_el, "unit": "k-mers/s",
              "avg_kernel_ms": lf_ms / max(1, lf_n),
              "path": "k_scan<..., KT = false>: q-mer table + three-base LF steps + label-run classification"}

    total_kmers = timed_kmers * ctx.world
    value = total_kmers / elapsed
    ax_stats = req = None
    if full and hot_kernel == 3 and not os.environ.get("SPEQ_BENCH_NO_STATS"):
        # one untimed launch of the instrumented twin: the same scan (checked equal), plus its work counters
        d_counts.zero_()
        if local:
            d_w.zero_()
        ax_stats = dev.scan_device_stats(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), reads.n, k,
                                         d_counts.data_ptr(), d_w.data_ptr(), paired=paired, local=local)
        if not np.array_equal(d_counts.cpu().numpy(), alone_local[0][0]):  # (this rank's, not all-reduced)
            raise RuntimeError("instrumented anchor-and-extend scan disagrees with the timed scan")
        req = ax_request_bytes(ax_stats, k, reads.n, local)
    compulsory = 2.0 * read_bytes + 8.0 * (reads.n + 1)  # bases + qualities + read offsets
    key = workload_key(cfg_no, k, mode, n_reads, KERNEL_TAG.get(hot_kernel, "lf"), qual_profile, err)
    roofline = None  # (needs the per-launch kernel time of the runs with events: --full)
    if kernel_med is not None:
        roofline = roofline_of(key, kernel_med / 1e3, req["total"] if req else None, compulsory, k, kmers_per_step)
        roofline["kernel"] = KERNEL_NAME.get(hot_kernel, str(hot_kernel))
        roofline["launches_timed"] = steps

    pcie = None
    if with_pcie:
        seq_b, qual_b = reads.seq.tobytes(), reads.qual.tobytes()
        dev.scan(seq_b, qual_b, reads.offsets[:3], k=k, paired=paired, local=local)  # pipeline warm-up
        best = None
        for _ in range(3):
            t0 = time.perf_counter()
            r = dev.scan(seq_b, qual_b, reads.offsets, k=k, paired=paired, local=local)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        if ctx.world == 1:  # (at N > 1 the timed counters are the all-reduced sums of every rank)
            same = (r.total, r.ambiguous, r.unique.tolist()) == (int(counts[0]), int(counts[1]),
                                                                  [int(x) for x in counts[2:]])
            if same and local:
                same = bool(np.allclose(r.weights, weights, rtol=1e-10, atol=0))
            if not same:
                raise RuntimeError("host-buffer scan disagrees with the HBM-resident scan (T, ambiguous, U, W)")
        pcie = {"value": kmers_per_step / best, "unit": "k-mers/s", "per_gpu": True,
                "path": "speq_scan_reads: pageable host arrays -> pinned slots -> H2D (copy stream) || scan",
                "host_GB_per_s": 2 * len(seq_b) / best / 1e9}

    cpu = None
    if with_cpu and ctx.rank == 0:
        # rank 0 only, at any N (the other ranks wait at the next barrier); at N > 1 the timed counters are the
        # all-reduced sums of every rank's shard, so only the sample check (`checked`) applies there
        cpu = cpu_baseline(prepared, reads, k, G, cpu_seconds, local, paired, extra_ports=cpu_extra_ports,
                           timed_counts=(counts, weights) if ctx.world == 1 else None)
        cpu["ranks_waiting"] = ctx.world - 1

    check = {"T": int(counts[0]), "ambiguous": int(counts[1]), "U_sha1": u_sha1(counts[2:]),
             **({"W_sum": float(weights.sum())} if weights is not None else {})}
    out = {
        "value": value, "ms_per_step": elapsed / steps * 1e3, "avg_kernel_ms": kernel_med,
        "ms_per_step_with_events": elapsed_ev / steps * 1e3 if elapsed_ev is not None else None, "k": k,
        "streams": n_str,
        "mode": mode,
        "workload": f"BASELINE config {cfg_no}: {c['n_variants']} variants x {c['n_isolates']} isolates x "
                    f"{c['length']} bp, {n_reads} x 150 bp {'pairs' if paired else 'reads'} per GPU, k={k}, {mode}"
                    + (f", qualities '{qual_profile}'" if qual_profile != "q40" else "")
                    + (f", {err * 100:g} % substitutions" if abs(err - 0.001) > 1e-12 else ""),
        "reads_per_gpu": n_reads, "kmers_per_step_per_gpu": kmers_per_step, "paired": paired,
        "index_build_s": round(prepared["build_s"], 3), "fm_text_len": int(idx.info().n),
        "kmer_table": {"on": table_on, "distinct_kmers": ktab["distinct_kmers"], "bytes": ktab["table_bytes"],
                       "build_s": round(ktab["build_ms"] / 1e3, 4)},
        "roofline": roofline, "traffic_key": key, "cpu_baseline": cpu, "lf_steps": lf, "kmer_table_kernel": prev,
        "pcie_inclusive": pcie, "check": check, "timing": timing,
        "detail": {"U": [int(x) for x in counts[2:]], "W": weights.tolist() if weights is not None else None,
                   "ax_work": ax_stats, "request_bytes_by_kind": req["parts"] if req else None},
    }
    return out, prepared


def compact_cpu(cpu: dict | None) -> dict | None:
    if not cpu:
        return None
    return {k: cpu[k] for k in ("value", "unit", "cores", "kind", "sample", "checked", "checked_timed") if k in cpu}


def compact_line(r: dict) -> dict:
    """One secondary line in the stdout JSON: rate, times, roofline fractions and the result check (no vectors)."""
    rf = r.get("roofline") or {}
    out = {"value": r["value"]}
    for key in ("ms_per_step", "avg_kernel_ms", "seconds", "unit", "back_to_back_value"):
        if key in r:
            out[key] = r[key]
    tm = r.get("timing") or {}
    if tm:
        out["value_min"], out["value_max"] = tm["value_min"], tm["value_max"]
        if "one_stream" in tm:
            out["one_stream_value"] = tm["one_stream"]["value"]
            out["overlap"] = round(tm["overlap"], 4)
    if rf:
        out.update(frac=rf.get("frac"), traffic_frac=rf.get("traffic_frac"), l2_request_frac=rf.get("l2_request_frac"),
                   frac_basis=rf.get("frac_basis"))
    if "check" in r:
        out["check"] = {k: v for k, v in r["check"].items() if k != "U"}
    if r.get("cpu_baseline"):
        out["cpu_baseline"] = {k: r["cpu_baseline"][k] for k in ("value", "cores", "kind", "checked", "checked_timed")
                               if k in r["cpu_baseline"]}
    return out


def compact_result(head: dict, lines: dict, meta: dict) -> dict:
    """The ONE stdout JSON line (BASELINE keys + roofline + cpu_baseline + compact secondary lines), < LINE_LIMIT
    bytes; everything else goes to the detail file."""
    rf = dict(head["roofline"] or {})  # (None without --full, like one_stream, overlap and the kernel times)
    tm = head["timing"]
    roof = {k: rf.get(k) for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_frac",
                                   "frac_basis", "avg_kernel_ms", "traffic_source", "traffic_rocprof_kernel_ms",
                                   "l2_hit_rate", "l2_request_frac", "compulsory_frac", "survey_model_frac",
                                   "kernel")}
    out = {
        "metric": meta["metric"], "value": head["value"], "unit": "k-mers/s", "n_gpus": meta["n_gpus"],
        "steps": meta["steps"], "warmup": meta["warmup"], "ms_per_step": head["ms_per_step"],
        "ms_per_step_with_events": head.get("ms_per_step_with_events"),
        "streams": head.get("streams", 1),
        "full": bool(meta.get("full", True)),
        "timing": f"value: the median of {tm['regions']} timed regions of K steps without per-launch events" + (
            f", step i on HIP stream i % {head.get('streams')} (consecutive batches overlap)"
            if head.get("streams", 1) > 1 else "") + (
            "; one_stream: the same steps on one stream in each region (overlap = value / one_stream.value)"
            if "one_stream" in tm else "") + (
            "; roofline.avg_kernel_ms: the median over the regions of the same K steps on one stream with HIP events "
            "around every launch" if rf else ""),
        "value_min": tm["value_min"], "value_max": tm["value_max"],
        "one_stream": {k2: tm["one_stream"][k2] for k2 in ("value", "ms_per_step")} if "one_stream" in tm else None,
        "overlap": tm.get("overlap"),
        "avg_kernel_ms_min_max": [tm.get("avg_kernel_ms_min"), tm.get("avg_kernel_ms_max")],
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u32",
        "data": "synthetic (splitmix64 references/reads, SURVEY.md §8(d))",
        "config": meta["config"],
        "roofline": roof if rf else None,
        "cpu_baseline": compact_cpu(head.get("cpu_baseline")),
        "check": head["check"],
        "lines": {name: compact_line(r) for name, r in lines.items() if r},
        "detail_file": meta.get("detail_file"),
    }
    if meta.get("dumped") is not None:
        out["dumped"] = meta["dumped"]
    s = json.dumps(out)
    if len(s) > LINE_LIMIT:  # never let the line outgrow what the driver parses: drop the optional fields first
        for r in out["lines"].values():
            for key in ("l2_request_frac", "frac_basis", "unit"):
                r.pop(key, None)
        out["config"].pop("kmer_table", None)
    return out


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    a = parse_args(argv)
    try:
        plan = launch_plan(a.gpus, os.environ)
    except LaunchError as e:
        print(f"bench.py: {e}", file=sys.stderr, flush=True)
        sys.exit(2)
    if plan == "relaunch":
        # nothing has touched a GPU in this process: start the N ranks as a child and exit with its status
        sys.exit(subprocess.call(relaunch_cmd(a.gpus, argv, free_port())))
    ctx = Ctx(a)  # (creates the pipeline's streams before any collective's: Ctx.__init__)
    from speq_amd import synth

    c = dict(synth.CONFIGS[a.config])
    k = a.k or c["k"]
    n_reads = a.reads or (c["n_reads"] if a.config <= 3 else c["n_reads"] // 8)
    head, prep = run_workload(ctx, a.config, k, n_reads, a.mode, a.steps, a.warmup, with_lf=not a.no_lf_compare,
                              with_pcie=not a.no_pcie, with_cpu=not a.no_cpu_baseline, cpu_seconds=a.cpu_seconds,
                              qual_profile=a.qual, err=a.err, cpu_extra_ports=True)
    dev = prep["dev"]
    # every rank writes what its own last timed step computed (rank r > 0 into DIR/rank<r>)
    dumped = dump_outputs(a.dump_outputs if ctx.rank == 0 else os.path.join(a.dump_outputs, f"rank{ctx.rank}"),
                          prep["last_outputs"]) if a.dump_outputs else None
    lines = {}
    only = set(x for x in a.only.split(",") if x)
    want = lambda name: not only or name in only  # noqa: E731
    cpu_on = not a.no_cpu_baseline
    short_cpu = max(4.0, a.cpu_seconds / 2)
    if a.full and not a.no_extra and a.config == 2 and not a.k and not a.reads and a.qual == "q40" and a.err == 0.001:
        other = "local" if a.mode == "global" else "global"
        if want(f"{other}_mode"):
            lines[f"{other}_mode"], _ = run_workload(ctx, 2, k, n_reads, other, a.steps, a.warmup, with_lf=False,
                                                     with_pcie=False, with_cpu=False, cpu_seconds=0, prepared=prep)
        if want("k31") or want("cli_e2e"):
            n31 = a.k31_reads or (10_000_000 if ctx.world == 1 else synth.CONFIGS[4]["n_reads"] // 8)
            lines["k31"], p31 = run_workload(ctx, 3, 31, n31, "global", max(20, a.steps), max(3, a.warmup),
                                             with_lf=False, with_pcie=False, with_cpu=cpu_on, cpu_seconds=short_cpu)
            lines["k31"]["note"] = ("config 3 (10 M reads on one GPU); with 8 ranks each scans config 4's 12.5 M-read "
                                    "shard of the same index")
            if ctx.world == 1 and not a.no_fastq and want("cli_e2e"):
                lines["cli_e2e"] = cli_e2e(p31, 31, lines["k31"]["check"])
            p31["dev"].close()
            del p31
        # the reference CLI's defaults: k = 70 (include/arg_parse.h:21), Phred-weighted local mode (:23)
        if want("k70_reference_defaults"):
            lines["k70_reference_defaults"], _ = run_workload(ctx, 2, 70, n_reads, "local", a.steps, a.warmup,
                                                              with_lf=False, with_pcie=False, with_cpu=cpu_on,
                                                              cpu_seconds=short_cpu, prepared=prep)
        if ctx.world == 1:
            if not a.no_fastq and want("fastq_e2e"):
                lines["fastq_e2e"] = fastq_e2e(ctx, prep, k)
            # the reference's default (Phred-weighted) mode on reads whose qualities vary base by base
            if want("local_varq"):
                lines["local_varq"], _ = run_workload(ctx, 2, k, n_reads, "local", a.steps, a.warmup, with_lf=False,
                                                      with_pcie=False, with_cpu=False, cpu_seconds=0, prepared=prep,
                                                      qual_profile="variable")
        if want("k70_err05"):  # (after the lines that reuse config 2's 0.1 %-error reads)
            lines["k70_err05"], _ = run_workload(ctx, 2, 70, n_reads, "local", a.steps, a.warmup, with_lf=False,
                                                 with_pcie=False, with_cpu=False, cpu_seconds=0, prepared=prep,
                                                 err=0.005)
        if a.cfg5_pairs and (want("cfg5_paired") or want("cfg5_paired_local")):
            # BASELINE config 5 (the north_star's scaling config): paired, k = 31, on a per-GPU sample of its pairs
            lines["cfg5_paired"], p5 = run_workload(ctx, 5, 31, a.cfg5_pairs, "global", max(20, a.steps),
                                                    max(3, a.warmup), with_lf=False, with_pcie=False,
                                                    with_cpu=cpu_on, cpu_seconds=short_cpu)
            lines["cfg5_paired"]["note"] = (f"config 5 lists 500 M pairs (a node's job); each GPU scans a "
                                            f"{a.cfg5_pairs}-pair shard of the same deterministic pair stream")
            if want("cfg5_paired_local"):
                lines["cfg5_paired_local"], _ = run_workload(ctx, 5, 31, a.cfg5_pairs, "local", max(20, a.steps),
                                                             max(3, a.warmup), with_lf=False, with_pcie=False,
                                                             with_cpu=False, cpu_seconds=0, prepared=p5)
            p5["dev"].close()

    if ctx.rank == 0:
        # the detail file: where --detail says; with --full by default profiles/r06/bench_detail_n<N>.json
        detail_path = a.detail or (os.path.join(ROOT, "profiles", "r06", f"bench_detail_n{ctx.world}.json")
                                   if a.full else "")
        config = {
            "workload": head["workload"],
            "k": k, "reads_per_gpu": n_reads, "paired": head["paired"], "mode": a.mode,
            "parallelism": f"dp{ctx.world} (reads sharded, index replicated)",
            "collective": {"rccl": "speq_allreduce_u64/_f64 (C ABI; RCCL ncclAllReduce of the G + 2 counters, once per timed job of K steps)",
                           "host": "speq_allreduce_u64/_f64 (C ABI; host-socket transport, ranks share GPUs)",
                           "none": "none (one GPU)"}[ctx.transport],
            "gpus_visible": ctx.n_dev, "ranks_per_gpu": -(-ctx.world // max(1, min(ctx.world, ctx.n_dev))),
            "index_build_s": head["index_build_s"], "index_builder": "gpu" if a.gpu_build else "host",
            "fm_text_len": head["fm_text_len"],
            "kmer_table": {"bytes": head["kmer_table"]["bytes"], "build_s": head["kmer_table"]["build_s"]},
        }
        meta = {"metric": "k-mers scanned/sec (whole node) at k=%d, 150 bp reads" % k, "n_gpus": ctx.world,
                "steps": a.steps, "warmup": a.warmup, "config": config, "full": a.full, "dumped": dumped,
                "detail_file": (os.path.relpath(detail_path, ROOT) if detail_path.startswith(ROOT) else detail_path)
                or None}
        out = compact_result(head, lines, meta)
        try:
            if detail_path:
                write_detail(detail_path, {
                    "compact": out, "head": head, "lines": lines,
                    "tuning": {"blocks_per_cu": dev.tuning("blocks_per_cu"),
                               "grid_blocks": dev.tuning("grid_blocks"), "prefix_q": a.prefix_q,
                               "pair_steps": a.pair_steps, "triple_steps": a.triple_steps,
                               "label_table": int(prep["idx"].info().label_table)},
                    "host": host_cpu_info()})
        except OSError as e:
            out["detail_file"] = f"not written: {e}"
        print(json.dumps(out), flush=True)
    if ctx.comm is not None:
        ctx.comm.close()
    if ctx.world > 1:
        ctx.dist.destroy_process_group()


def write_detail(path: str, detail: dict) -> None:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(detail, f, indent=1, default=str)


def write_fastq(path: str, reads, chunk: int = 1_000_000) -> int:
    """Writes equal-length reads as four-line FASTQ records (@r<9-digit index>), vectorised in chunks; returns the
    bytes."""
    lens = np.diff(reads.offsets)
    L = int(lens[0]) if len(lens) else 0
    if not len(lens) or np.any(lens != L):
        raise ValueError("write_fastq: equal-length reads only")
    n = len(lens)
    total = 0
    with open(path, "wb") as f:
        for r0 in range(0, n, chunk):
            m = min(chunk, n - r0)
            digits = ((np.arange(r0, r0 + m, dtype=np.int64)[:, None] // (10 ** np.arange(8, -1, -1))[None, :]) % 10
                      + ord("0"))
            rec = np.empty((m, 2 + 9 + 1 + L + 3 + L + 1), dtype=np.uint8)
            rec[:, 0:2] = np.frombuffer(b"@r", dtype=np.uint8)
            rec[:, 2:11] = digits.astype(np.uint8)
            rec[:, 11] = ord("\n")
            rec[:, 12:12 + L] = reads.seq[r0 * L:(r0 + m) * L].reshape(m, L)
            rec[:, 12 + L:15 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
            rec[:, 15 + L:15 + 2 * L] = reads.qual[r0 * L:(r0 + m) * L].reshape(m, L)
            rec[:, 15 + 2 * L] = ord("\n")
            rec.tofile(f)
            total += rec.size
    return total


def fastq_e2e(ctx: Ctx, prep: dict, k: int) -> dict:
    """The drop-in input path (speq_scan_fastq: reader thread + parser threads -> pinned slots -> H2D || scan) on the
    workload's reads written as one FASTQ file on local disk; best of 3 passes with the page cache warm. Checked
    against the HBM-resident scan of the same reads."""
    reads, dev = prep["reads"], prep["dev"]
    threads = host_cpu_info()["threads"]
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as td:
        path = os.path.join(td, "reads.fq")
        nbytes = write_fastq(path, reads)
        ref_res = dev.scan(reads.seq.tobytes(), reads.qual.tobytes(), reads.offsets, k=k)
        best, res = None, None
        for _ in range(3):
            t0 = time.perf_counter()
            res, st = dev.scan_fastq(path, k=k, threads=threads)
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        if (res.total, res.ambiguous, res.unique.tolist()) != (ref_res.total, ref_res.ambiguous,
                                                              ref_res.unique.tolist()):
            raise RuntimeError("FASTQ scan disagrees with the in-memory scan")
    lens = np.diff(reads.offsets).astype(np.int64)
    kmers = int(np.maximum(lens - k + 1, 0).sum())
    return {"value": kmers / best, "unit": "k-mers/s", "file_GB_per_s": nbytes / best / 1e9, "seconds": best,
            "file_bytes": nbytes, "threads": threads, "k": k,
            "check": {"T": int(res.total), "ambiguous": int(res.ambiguous), "U_sha1": u_sha1(res.unique)},
            "path": "speq_scan_fastq: plain FASTQ on local disk (page cache warm), parallel record-aligned cut, "
                    "raw text to pinned slots -> H2D (copy stream) || GPU record parsing + k_scan_ax",
            "workload": f"{reads.n} x 150 bp reads of BASELINE config 2, global mode"}


def cli_e2e(prep: dict, k: int, check: dict) -> dict:
    """The user-visible path end to end (SURVEY §8(d) secondary metric): `bin/speq index` then `bin/speq scan` as
    processes on files — config 3's references + groupings, its 10 M reads as one FASTQ on local disk — at the
    reference's defaults (Phred-weighted, phred cutoff 30; src/main.cpp:25-31 -> fm_scanner.cpp:309-545) with
    k = 31: FASTQ stream + scan, the .dat pass (first scan only), unique_to_percent and the EM loop. T and the
    ambiguous count on stderr are checked against the HBM-resident scan of the same reads (`check`)."""
    ref, reads = prep["ref"], prep["reads"]
    threads = host_cpu_info()["threads"]
    speq = os.path.join(ROOT, "bin", "speq")
    work = tempfile.mkdtemp(prefix="speq_cli_", dir=os.environ.get("TMPDIR", "/tmp"))
    env = dict(os.environ, SPEQ_CLI_TIMING="1")
    res = {"unit": "k-mers/s", "threads": threads, "k": k}
    try:
        with open(os.path.join(work, "refs.fa"), "w") as f:
            f.write(ref.fasta_text())
        with open(os.path.join(work, "groups.txt"), "w") as f:
            f.write(ref.groupings_text())
        t0 = time.perf_counter()
        fq_bytes = write_fastq(os.path.join(work, "r1.fq"), reads)
        res["fastq_write_s"] = round(time.perf_counter() - t0, 2)
        lens = np.diff(reads.offsets).astype(np.int64)
        kmers = int(np.maximum(lens - k + 1, 0).sum())

        def run(args):
            t0 = time.perf_counter()
            p = subprocess.run([speq] + args, cwd=work, capture_output=True, text=True, env=env, timeout=300)
            dt = time.perf_counter() - t0
            if p.returncode != 0:
                raise RuntimeError(f"speq {args[0]} failed ({p.returncode}): {p.stderr[-400:]}")
            phases = {}
            for ln in p.stderr.splitlines():
                if ln.startswith("speq: ") and ln.endswith(" s"):
                    name, sec = ln[6:-2].rsplit(None, 1)
                    try:
                        phases[name.strip()] = float(sec)
                    except ValueError:
                        pass
            return dt, p.stderr, phases

        res["index_s"], _, res["index_phases"] = run(["index", "-r", "refs.fa", "-g", "groups.txt", "-x", "ref",
                                                      "-t", str(threads)])
        scan = ["scan", "-1", "r1.fq", "-x", "ref", "-k", str(k), "-t", str(threads)]
        res["first_scan_s"], _, res["first_scan_phases"] = run(scan + ["-o", "out.txt"])  # + the .dat pass (new index)
        # .dat cached (the reference's steady state: fm_scanner.cpp:79-135); -o must be a new file (arg_parse.cpp:37).
        # Three runs, each started 1 s after the previous process ended: the driver's teardown of a GPU process
        # (0.1-0.2 s after its exit) delays the runtime start of the next one, which a single invocation does not pay
        # (tools/module_load_probe.cpp: runtime start 59 ms on an idle GPU, 170-230 ms right after another process);
        # the median is `value`. One more run started right after the third is reported as `back_to_back_s`.
        runs = []
        for i in range(3):
            time.sleep(1.0)
            runs.append(run(scan + ["-o", f"out_cached{i}.txt"]))
        b2b = run(scan + ["-o", "out_b2b.txt"])
        dts = sorted(r[0] for r in runs)
        dt, err, phases = next(r for r in runs if r[0] == dts[1])
        for _, e, _ in runs + [b2b]:
            tl = [ln for ln in e.splitlines() if ln.count("\t") == 1 and ln.replace("\t", "").isdigit()]
            T, amb = (int(x) for x in tl[0].split("\t"))
            if (T, amb) != (check["T"], check["ambiguous"]):
                raise RuntimeError(f"speq scan stderr T/ambiguous {(T, amb)} != HBM-resident scan "
                                   f"{(check['T'], check['ambiguous'])}")
        res.update(value=kmers / dt, seconds=dt, seconds_runs=[round(x, 4) for x in dts],
                   back_to_back_s=round(b2b[0], 4), back_to_back_value=kmers / b2b[0], phases=phases, kmers=kmers,
                   fastq_bytes=fq_bytes,
                   em_iterations=err.count("Percent of each group"),
                   check={"T": T, "ambiguous": amb, "matches_hbm_scan": True},
                   timing_rule="median of 3 runs, each started 1 s after the previous process ended",
                   path="bin/speq scan process: index load || HIP init, FASTQ stream (parallel cut, GPU parsing) + "
                        "k_scan_ax, cached .dat, unique_to_percent, EM loop over the interval histogram, -o write",
                   workload=f"BASELINE config 3 references, {reads.n} x 150 bp reads (FASTQ on local disk), k={k}, "
                            f"Phred-weighted (reference default mode)")
    finally:
        subprocess.run(["rm", "-rf", work])
    return res


_SEQAN_LIKE = {}


def cpu_baseline(prep, reads, k, G, target_s, local, paired=False, extra_ports=False, timed_counts=None):
    """CPU baseline on this host's cores over a bounded sample of the same reads (rank 0, N = 1 only).

    value: oracle/seqan_like.c — the reference's ALGORITHM restated (backward search on a wavelet structure, locate of
    every hit through SA samples every 16 rows, sorted hit lists, first-hit rule), the SURVEY.md 8(d) stand-in for
    the SeqAn3 binary, which cannot be built here (8(c)). Its counts on the sample are checked against the GPU scan of
    the same sample (`checked`); when the sample is the whole shard, also against the TIMED scan's own counters
    (`timed_counts` = (counts, weights) of speq_scan_reads_device: T, ambiguous, every U[g], W; `checked_timed`).
    extra_ports (headline): also oracle/kmer_oracle.c (hash map, no FM-index) and oracle/fm_cpu.c (this build's
    label-run search on host cores)."""
    from oracle.oracle import Oracle, SeqanLike
    ref, idx, dev = prep["ref"], prep["idx"], prep["dev"]
    hw = host_cpu_info()
    threads = hw["threads"]
    t0 = time.perf_counter()
    cfg = prep.get("cfg")
    sl = _SEQAN_LIKE.get(cfg)
    if sl is None:
        # the product index's suffix array of the same text spares the stand-in its O(n log n) doubling sort
        # (minutes at config 5); a suffix array is unique (tests/test_seqan_like.py checks the two builds agree)
        sl = _SEQAN_LIKE[cfg] = SeqanLike(ref.records, ref.groups, G, sa=idx.array("sa", np.uint32))
    sl_build = time.perf_counter() - t0
    units = reads.n // 2 if paired else reads.n

    def timed(fn, target):
        def run(nu, reps=1):
            nr = 2 * nu if paired else nu
            b = int(reads.offsets[nr])
            t0 = time.perf_counter()
            for _ in range(reps):
                r = fn(reads.seq[:b], reads.qual[:b], reads.offsets[:nr + 1])
            return time.perf_counter() - t0, r

        n = min(units, 500)
        t, r = run(n)
        while t < target / 2 and n < units:  # grow the sample first, repeat passes only over the whole shard
            n = int(min(units, n * min(8.0, 1.2 * target / max(t, 1e-3))))
            t, r = run(n)
        reps = 1
        if t < target / 2:
            reps = max(1, int(target / max(t, 1e-3)))
            t, r = run(n, reps)
        nr = 2 * n if paired else n
        lens = np.diff(reads.offsets[:nr + 1]).astype(np.int64)
        km = int(np.maximum(lens - k + 1, 0).sum()) * reps
        return km / t, n, reps, km, t, r

    v, n, reps, km, t, r = timed(lambda s, q, o: sl.scan(s, q, o, k=k, paired=paired, local=local, threads=threads),
                                 target_s)
    # the same sample through the product (host buffers -> GPU): the baseline computed the same answer
    nr = 2 * n if paired else n
    b = int(reads.offsets[nr])
    g = dev.scan(reads.seq[:b].tobytes(), reads.qual[:b].tobytes(), reads.offsets[:nr + 1], k=k, paired=paired,
                 local=local)
    checked = (r[0], r[1], r[2].tolist()) == (g.total, g.ambiguous, g.unique.tolist())
    if checked and local:
        checked = bool(np.allclose(r[3], g.weights, rtol=1e-9, atol=0))
    if not checked:
        raise RuntimeError("CPU baseline (seqan_like) disagrees with the GPU scan on its sample")
    checked_timed = None
    if timed_counts is not None and n == units:
        tc, tw = timed_counts
        checked_timed = (r[0], r[1], r[2].tolist()) == (int(tc[0]), int(tc[1]), [int(x) for x in tc[2:]])
        if checked_timed and local:
            checked_timed = bool(np.allclose(r[3], tw, rtol=1e-9, atol=0))
        if not checked_timed:
            raise RuntimeError("CPU baseline (seqan_like) over the whole shard disagrees with the timed "
                               "speq_scan_reads_device counters")
    unit = "pairs" if paired else "reads"
    out = {"value": v, "unit": "k-mers/s", "cores": threads, "kind": "port", "checked": True,
           "checked_timed": checked_timed,
           "sample": f"first {n} {unit} x {reps} ({km} k-mers, {t:.1f} s), oracle/seqan_like.c (wavelet backward "
                     f"search + SA-sample-16 locate of every hit + first-hit rule), {threads} threads",
           "host": hw, "index_build_s_untimed": round(sl_build, 1)}
    if extra_ports:
        orc = Oracle(ref.records, ref.groups, G, k)
        hv, hn, hreps, hkm, ht, _ = timed(lambda s, q, o: orc.scan(s, q, o, paired=paired, local=local,
                                                                   threads=threads), target_s / 3)
        out["hash_port"] = {"value": hv, "unit": "k-mers/s", "cores": threads,
                            "sample": f"first {hn} {unit} x {hreps} passes ({hkm} k-mers, {ht:.1f} s), "
                                      f"oracle/kmer_oracle.c (hash map k-mer -> group label: no FM-index, no locate)"}
        if k <= 32 and not local:  # the build's own algorithm on CPU cores (oracle/fm_cpu.c)
            from oracle.oracle import FmCpu
            fc = FmCpu(idx)
            lv, ln, lreps, lkm, lt, _ = timed(lambda s, q, o: fc.scan(s, q, o, k=k, paired=paired, threads=threads),
                                              target_s / 3)
            out["label_run_port"] = {"value": lv, "unit": "k-mers/s", "cores": threads,
                                     "sample": f"first {ln} x {lreps} passes ({lkm} k-mers, {lt:.1f} s), "
                                               f"oracle/fm_cpu.c (this build's label-run FM-index search on host "
                                               f"cores, same index arrays as the GPU)"}
    return out


if __name__ == "__main__":
    main()
