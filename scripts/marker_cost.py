#!/usr/bin/env python3
"""Cost of the marker-coverage read pass beside the scan and the per-unit report, on bench.py's headline input
(config 2: 10 variants of 50 kb, 1 M reads of 150 bp resident in HBM, k = 21, global mode, the bench's index options).

Times speq_scan_reads_device, speq_report_reads_device and speq_markers_add_reads_device on the same buffers and
stream with HIP events: per entry point a warm-up launch, then five timed regions of about `--region-ms` of
back-to-back launches each, the three entry points alternating; the median region per launch is the figure, and the
five regions are printed beside it. The marker pass (speq_markers_create: allocation, clear, one search per text
window, blocking) and the fold (speq_markers_finalize: blocking, the copy of G records included) are timed once each,
as wall time of the blocking call on an idle device. One JSON line on stdout.

    python scripts/marker_cost.py [--reads 1000000] [--region-ms 200] [--out FILE]
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
from speq_amd import DeviceIndex, FmIndex, Markers, synth  # noqa: E402


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
    Markers(dev, a.k).close()  # the new file's code object and the first allocation, outside the timed create
    mk, create_ms = wall_ms(lambda: Markers(dev, a.k))

    def scan():
        dev.scan_device(*args, cnt.data_ptr(), stream=stream)

    def report():
        dev.report_device(*args, rep.data_ptr(), sets.data_ptr(), stream=stream)

    def markers():
        mk.add_device(*args[:4], stream=stream)

    n_scan, n_rep, n_mk = calibrate(scan, a.region_ms), calibrate(report, a.region_ms), calibrate(markers, a.region_ms)
    scan_kernel = dev.tuning("last_kernel")
    t_scan, t_rep, t_mk = [], [], []
    for _ in range(5):
        t_scan.append(region(scan, n_scan))
        t_rep.append(region(report, n_rep))
        t_mk.append(region(markers, n_mk))
    launches = 2 + 5 * n_mk  # calibrate's two, then the regions
    cov, fold_ms = wall_ms(mk.finalize)
    # the three passes agree on what they all count
    cnt.zero_()
    scan()
    torch.cuda.synchronize()
    cn = cnt.cpu().numpy()
    r = rep.cpu().numpy().view(np.uint32).reshape(-1, 4)
    assert int(r[:, 1].sum()) == int(cn[2:].sum()), "report and scan disagree"
    assert cov.hits.tolist() == (cn[2:] * launches).tolist(), "marker depths and scan disagree"
    assert (cov.depth_hist.sum(axis=1) == cov.markers).all()
    m_scan, m_rep, m_mk = statistics.median(t_scan), statistics.median(t_rep), statistics.median(t_mk)
    line = {"config": 2, "reads": reads.n, "k": a.k, "windows": int(cn[0]), "unique_windows": int(cn[2:].sum()),
            "scan_kernel": scan_kernel, "sa_positions": int(idx.info().n),
            "scan_ms": round(m_scan, 4), "scan_regions_ms": [round(x, 4) for x in t_scan],
            "report_ms": round(m_rep, 4), "report_regions_ms": [round(x, 4) for x in t_rep],
            "markers_ms": round(m_mk, 4), "markers_regions_ms": [round(x, 4) for x in t_mk],
            "markers_over_report": round(m_mk / m_rep, 3), "markers_over_scan": round(m_mk / m_scan, 2),
            "report_over_scan": round(m_rep / m_scan, 2), "launches_per_region": [n_scan, n_rep, n_mk],
            "marker_pass_create_ms": round(create_ms, 3), "fold_finalize_ms": round(fold_ms, 3),
            "markers_total": int(cov.markers.sum()), "observed_total": int(cov.observed.sum()),
            "device": torch.cuda.get_device_name(0)}
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    mk.close()
    dev.close()


if __name__ == "__main__":
    main()
