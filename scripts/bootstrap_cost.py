#!/usr/bin/env python3
"""Cost of the read-bootstrap pass beside the per-unit report, on bench.py's headline input (config 2: 10 variants of
50 kb, 1 M reads of 150 bp resident in HBM, k = 21, the bench's index options).

Times speq_report_reads_device and speq_bootstrap_add_reads_device on the same buffers and stream with HIP events: per
entry point a warm-up launch, then five timed regions of about `--region-ms` of back-to-back launches each, the entry
points alternating; the median region per launch is the figure, and the five regions are printed beside it. The
bootstrap is timed in three shapes: B = 200 global and local (both accumulate per block in LDS here) and B = 1024
global (12 * 1025 cells do not fit: device atomics throughout). Row 0 of every handle is checked against the scan. One
JSON line on stdout.

    python scripts/bootstrap_cost.py [--reads 1000000] [--region-ms 200] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # before speq_amd: one HIP runtime per process (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from marker_cost import calibrate, region  # noqa: E402
from speq_amd import Bootstrap, DeviceIndex, FmIndex, synth  # noqa: E402

SHAPES = [("b200_global", 200, False), ("b200_local", 200, True), ("b1024_global", 1024, False)]


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
    dev.prepare(a.k)
    reads = synth.make_reads(ref, a.reads)
    d_seq = torch.from_numpy(reads.seq).cuda()
    d_qual = torch.from_numpy(reads.qual).cuda()
    d_off = torch.from_numpy(reads.offsets.astype(np.int64)).cuda()
    W = (G + 63) // 64
    rep = torch.zeros(reads.n * 4, dtype=torch.int32, device="cuda")
    sets = torch.zeros(reads.n * W, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    args = (d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), reads.n)
    handles = {name: Bootstrap(dev, a.k, B, 1, local=local) for name, B, local in SHAPES}

    def report():
        dev.report_device(*args, a.k, rep.data_ptr(), sets.data_ptr(), stream=stream)

    fns = {"report": report}
    for name, h in handles.items():
        fns[name] = (lambda h=h: h.add_device(*args, stream=stream))
    reps = {name: calibrate(fn, a.region_ms) for name, fn in fns.items()}
    times = {name: [] for name in fns}
    for _ in range(5):
        for name, fn in fns.items():
            times[name].append(region(fn, reps[name]))
    med = {name: statistics.median(t) for name, t in times.items()}
    sc = dev.scan(reads.seq.tobytes(), reads.qual.tobytes(), reads.offsets, k=a.k)
    line = {"config": 2, "reads": reads.n, "k": a.k, "groups": G, "windows": sc.total,
            "report_ms": round(med["report"], 4), "report_regions_ms": [round(x, 4) for x in times["report"]],
            "launches_per_region": reps, "device": torch.cuda.get_device_name(0)}
    for name, B, local in SHAPES:
        h = handles[name]
        launches = 2 + 5 * reps[name]  # calibrate's two, then the regions
        counts, _ = h.finalize()
        assert counts[0].tolist() == [sc.total * launches, sc.ambiguous * launches] + (sc.unique * launches).tolist()
        line[name] = {"ms": round(med[name], 4), "regions_ms": [round(x, 4) for x in times[name]],
                      "over_report": round(med[name] / med["report"], 3), "lds_path": h.info()["lds_path"]}
        h.close()
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    dev.close()


if __name__ == "__main__":
    main()
