"""Child process of tests/test_gpu_sproof_knob.py: a few scans with the library SPEQ_LIB_PATH names (the build without
the substitution proofs) against the CPU oracle; tuning ax_sproof = 1 must then change nothing either. Prints one JSON
line; exits non-zero on any mismatch."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.oracle import Oracle  # noqa: E402
from speq_amd import DeviceIndex, FmIndex, synth  # noqa: E402
from speq_amd import _lib  # noqa: E402


def main():
    _lib.lib()
    want = os.path.realpath(_lib.LIB_PATH)
    if want not in open("/proc/self/maps").read():
        raise AssertionError(f"{want} is not the library this process loaded")
    ref = synth.make_reference(4, 2, 6_000, ref_n_rate=0.002)
    idx = FmIndex.build(ref.records, ref.groups, 4, prefix_q=8, pair_steps=True, triple_steps=True)
    dev = DeviceIndex(idx)
    reads = synth.make_reads(ref, 1_500, err_rate=0.01, n_rate=0.002, lowq_rate=0.01, short_frac=0.05)
    cases = 0
    for k in (21, 70):
        orc = Oracle(ref.records, ref.groups, 4, k)
        for local in (False, True):
            T, amb, U, W = orc.scan(reads.seq, reads.qual, reads.offsets, local=local)
            for sproof in (2, 1):
                dev.tune(ax_sproof=sproof)
                got = dev.scan(reads.seq.tobytes(), reads.qual.tobytes(), reads.offsets, k=k, local=local)
                if dev.tuning("last_kernel") != 3:
                    raise AssertionError("k_scan_ax did not take the scan")
                if (got.total, got.ambiguous, got.unique.tolist()) != (T, amb, U.tolist()):
                    raise AssertionError(f"k={k} local={local} ax_sproof={sproof}")
                if local:
                    np.testing.assert_allclose(got.weights, W, rtol=1e-10, atol=0)
                cases += 1
    dev.close()
    print(json.dumps({"lib": want, "cases": cases, "ok": True}), flush=True)


if __name__ == "__main__":
    main()
