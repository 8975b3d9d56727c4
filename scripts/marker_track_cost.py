#!/usr/bin/env python3
"""Cost of the marker track (speq_markers_track) beside the marker pass of speq_markers_create, in one process, on
bench.py's headline index (config 2: 10 variants of 50 kb, 1.0 M text positions, k = 21, the bench's index options).

Both are blocking calls that run once per `speq scan` run, so the figure is the wall time of the call on an idle
device: per entry point one warm-up call (code object load, first allocation), then five timed calls, create and the
two tracks alternating; the median is the figure and the five are printed beside it. The handle holds the depths of
`--reads` reads of config 2, so the track folds real depths. One JSON line on stdout.

    python scripts/marker_track_cost.py [--reads 200000] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # before speq_amd: one HIP runtime per process (tests/conftest.py)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speq_amd import DeviceIndex, FmIndex, Markers, synth  # noqa: E402
from speq_amd.api import TRACK_DTYPE  # noqa: E402
from speq_amd._lib import check, lib  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=200_000)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    c = synth.CONFIGS[2]
    G = c["n_variants"]
    ref = synth.make_reference(G, c["n_isolates"], c["length"])
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=12, pair_steps=True, label_table="auto", threads=16,
                        triple_steps=True)
    dev = DeviceIndex(idx, 0)
    reads = synth.make_reads(ref, a.reads)
    mk = Markers(dev, a.k)
    mk.add(reads.seq.tobytes(), reads.qual.tobytes(), reads.offsets)
    cov = mk.finalize()
    bufs = {}
    for bin in (100, 1):
        t = mk.track(bin)  # warm-up, and the answer to check
        assert int(t.bins["hits"].sum()) >= int(cov.hits.sum()) > 0
        assert int(t.bins["markers"].sum()) * 2 >= int(cov.markers.sum())
        bufs[bin] = np.zeros(len(t.bins), dtype=TRACK_DTYPE)

    def track(bin):
        check(lib().speq_markers_track(mk._h, bin, bufs[bin].ctypes.data))

    t_create, t_100, t_1 = [], [], []
    for _ in range(5):
        m2, ms = wall_ms(lambda: Markers(dev, a.k))
        m2.close()
        t_create.append(ms)
        t_100.append(wall_ms(lambda: track(100))[1])
        t_1.append(wall_ms(lambda: track(1))[1])
    line = {"config": 2, "k": a.k, "reads": reads.n, "sa_positions": int(idx.info().n),
            "loci": int(idx.track_loci(a.k).sum()), "bins_100": len(bufs[100]), "bins_1": len(bufs[1]),
            "create_ms": round(statistics.median(t_create), 3), "create_runs_ms": [round(x, 3) for x in t_create],
            "track_bin100_ms": round(statistics.median(t_100), 3), "track_bin100_runs_ms": [round(x, 3) for x in t_100],
            "track_bin1_ms": round(statistics.median(t_1), 3), "track_bin1_runs_ms": [round(x, 3) for x in t_1],
            "timing": "wall time of the blocking call, idle device, median of 5",
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
