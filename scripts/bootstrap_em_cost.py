#!/usr/bin/env python3
"""Cost of filling one EM histogram per bootstrap replicate (speq_bootstrap_attach_em), by the method of
scripts/bootstrap_cost.py on the same input (config 2: 10 related variants of 50 kb, 1 M reads of 150 bp resident in
HBM, k = 21, B = 200): most passing windows of these reads lie in several groups (the share is printed).

Times speq_bootstrap_add_reads_device on the same buffers and stream with HIP events, in global and local mode, each
with a plain handle (the figures of §4p, re-measured in this run) and with a handle that has the finalized histogram of
the same reads attached: per handle a warm-up launch, then five timed regions of about `--region-ms` of back-to-back
launches each, the handles alternating; the median region per launch is the figure, and the five regions are printed
beside it. Row 0 of every handle is checked against the scan, row 0 of the multiplicities against the histogram, and
`missed` against 0. One JSON line on stdout.

    python scripts/bootstrap_em_cost.py [--reads 1000000] [--replicates 200] [--region-ms 200] [--out FILE]
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
from speq_amd import Bootstrap, DeviceIndex, EmHistogram, FmIndex, synth  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--replicates", type=int, default=200)
    ap.add_argument("--region-ms", type=float, default=200.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = synth.CONFIGS[2]
    G, B = c["n_variants"], a.replicates
    ref = synth.make_reference(G, c["n_isolates"], c["length"])
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=12, pair_steps=True, label_table="auto", threads=16,
                        triple_steps=True)
    dev = DeviceIndex(idx, 0)
    dev.prepare(a.k)
    reads = synth.make_reads(ref, a.reads)
    host = (reads.seq.tobytes(), reads.qual.tobytes(), reads.offsets)
    em = EmHistogram(dev)
    sc = em.scan(*host, k=a.k)
    em.finalize()
    row_mult, _, _, _ = em.rows_csr()
    n_intervals, _, multi_windows = em.info()
    d_seq = torch.from_numpy(reads.seq).cuda()
    d_qual = torch.from_numpy(reads.qual).cuda()
    d_off = torch.from_numpy(reads.offsets.astype(np.int64)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    args = (d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), reads.n)
    shapes = [("global", False, False), ("global_em", False, True), ("local", True, False), ("local_em", True, True)]
    handles = {}
    for name, local, with_em in shapes:
        handles[name] = Bootstrap(dev, a.k, B, 1, local=local)
        if with_em:
            handles[name].attach_em(em)
    fns = {name: (lambda h=h: h.add_device(*args, stream=stream)) for name, h in handles.items()}
    reps = {name: calibrate(fn, a.region_ms) for name, fn in fns.items()}
    times = {name: [] for name in fns}
    for _ in range(5):
        for name, fn in fns.items():
            times[name].append(region(fn, reps[name]))
    med = {name: statistics.median(t) for name, t in times.items()}
    line = {"config": 2, "reads": reads.n, "k": a.k, "groups": G, "replicates": B, "windows": sc.total,
            "multi_group_windows": multi_windows, "intervals": n_intervals, "rows": len(row_mult),
            "top_row_share": round(float(row_mult.max()) / max(multi_windows, 1), 4) if len(row_mult) else 0.0,
            "launches_per_region": reps, "device": torch.cuda.get_device_name(0)}
    for name, local, with_em in shapes:
        h = handles[name]
        launches = 2 + 5 * reps[name]  # calibrate's two, then the regions
        counts, _ = h.finalize()
        assert counts[0].tolist() == [sc.total * launches, sc.ambiguous * launches] + (sc.unique * launches).tolist()
        line[name] = {"ms": round(med[name], 4), "regions_ms": [round(x, 4) for x in times[name]],
                      "lds_path": h.info()["lds_path"]}
        if with_em:
            mult, missed = h.finalize_em()
            assert missed == 0 and mult[0].tolist() == (row_mult * np.uint64(launches)).tolist()
            line[name]["lds_rows"] = h.em_info()["lds_rows"]
            line[name]["over_plain"] = round(med[name] / med[name[:-3]], 3)
        h.close()
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    em.close()
    dev.close()


if __name__ == "__main__":
    main()
