#!/usr/bin/env python3
"""Cost of the duplicate-read pass beside the scan and the per-unit report, on bench.py's headline input (config 2: 10
variants of 50 kb, 1 M reads of 150 bp resident in HBM, k = 21, global mode, the bench's index options).

Times speq_scan_reads_device, speq_report_reads_device, speq_dedup_add_reads_device (the fingerprints),
speq_dedup_mask_device and speq_scan_reads_device over the masked qualities on the same buffers and stream with HIP
events: per entry point a warm-up launch, then five timed regions of about `--region-ms` of back-to-back launches each,
the entry points alternating; the median region per launch is the figure, and the five regions are printed beside it.
The timed adds go to a handle that is never finalized (every launch rewrites the same fingerprints). The finalize (two
radix sorts, the mark pass, blocking) is timed as wall time of the blocking call on an idle device, five times on a
handle whose first finalize has been made. One JSON line on stdout.

    python scripts/dedup_cost.py [--reads 1000000] [--region-ms 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before speq_amd: one HIP runtime per process (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speq_amd import Dedup, DeviceIndex, FmIndex, synth  # noqa: E402


def region(fn, reps: int) -> float:
    """Milliseconds per launch of `reps` back-to-back launches between two events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def calibrate(fn, region_ms: float) -> int:
    """Warm-up launch, then the launches a region of about region_ms needs."""
    fn()
    torch.cuda.synchronize()
    return max(1, min(1000, int(np.ceil(region_ms / max(region(fn, 1), 1e-3)))))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--region-ms", type=float, default=200.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = synth.CONFIGS[2]
    G = c["n_variants"]
    ref = synth.make_reference(G, c["n_isolates"], c["length"])
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=12, pair_steps=True, label_table="auto", threads=16,
                        triple_steps=True)
    dev = DeviceIndex(idx, 0)
    dev.prepare(a.k)  # the scan's per-k structures, outside the timed regions (as bench.py does)
    reads = synth.make_reads(ref, a.reads)
    d_seq = torch.from_numpy(reads.seq).cuda()
    d_qual = torch.from_numpy(reads.qual).cuda()
    d_off = torch.from_numpy(reads.offsets.astype(np.int64)).cuda()
    cnt = torch.zeros(G + 2, dtype=torch.int64, device="cuda")
    W = (G + 63) // 64
    rep = torch.zeros(reads.n * 4, dtype=torch.int32, device="cuda")
    sets = torch.zeros(reads.n * W, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    args = (d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), reads.n, a.k)
    # the handle that is finalized: one add, a first finalize (the new file's code object, the allocations), then timed
    dd = Dedup(dev)
    dd.add_device(d_seq.data_ptr(), d_off.data_ptr(), reads.n, stream=stream)
    stats = dd.finalize()
    t_fin = [wall_ms(dd.finalize)[1] for _ in range(5)]
    d_masked = d_qual.clone()
    dd.mask_device(d_masked.data_ptr(), d_off.data_ptr(), reads.n, stream=stream)
    torch.cuda.synchronize()
    timed = Dedup(dev)  # never finalized

    def scan():
        dev.scan_device(*args, cnt.data_ptr(), stream=stream)

    def report():
        dev.report_device(*args, rep.data_ptr(), sets.data_ptr(), stream=stream)

    def add():
        timed.add_device(d_seq.data_ptr(), d_off.data_ptr(), reads.n, stream=stream)

    def mask():
        dd.mask_device(d_masked.data_ptr(), d_off.data_ptr(), reads.n, stream=stream)

    def masked_scan():
        dev.scan_device(d_seq.data_ptr(), d_masked.data_ptr(), d_off.data_ptr(), reads.n, a.k, cnt.data_ptr(),
                        stream=stream)

    fns = {"scan": scan, "report": report, "add": add, "mask": mask, "masked_scan": masked_scan}
    reps = {name: calibrate(fn, a.region_ms) for name, fn in fns.items()}
    scan_kernel = dev.tuning("last_kernel")
    t = {name: [] for name in fns}
    for _ in range(5):
        for name, fn in fns.items():
            t[name].append(region(fn, reps[name]))
    # what the passes count: the masked scan sees the kept units' windows only
    cnt.zero_()
    scan()
    torch.cuda.synchronize()
    plain = cnt.cpu().numpy().copy()
    cnt.zero_()
    masked_scan()
    torch.cuda.synchronize()
    kept = cnt.cpu().numpy().copy()
    assert stats.units == reads.n and int(stats.mult_hist.sum()) == stats.distinct
    assert (kept <= plain).all()
    med = {name: statistics.median(v) for name, v in t.items()}
    line = {"config": 2, "reads": reads.n, "bases": int(reads.offsets[-1]), "k": a.k, "scan_kernel": scan_kernel,
            "units": stats.units, "distinct": stats.distinct, "max_multiplicity": stats.max_multiplicity,
            "windows": int(plain[0]), "windows_dedup": int(kept[0]),
            "finalize_ms": round(statistics.median(t_fin), 3), "finalize_calls_ms": [round(x, 3) for x in t_fin],
            "launches_per_region": reps, "device": torch.cuda.get_device_name(0)}
    for name in fns:
        line[name + "_ms"] = round(med[name], 4)
        line[name + "_regions_ms"] = [round(x, 4) for x in t[name]]
    line["add_over_report"] = round(med["add"] / med["report"], 4)
    line["add_over_scan"] = round(med["add"] / med["scan"], 3)
    line["masked_scan_over_scan"] = round(med["masked_scan"] / med["scan"], 3)
    line["add_gbytes_per_s"] = round(line["bases"] / med["add"] / 1e6, 1)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    timed.close()
    dd.close()
    dev.close()


if __name__ == "__main__":
    main()
