"""GPU: k_scan_ax built without the substitution proofs (SPEQ_AX_SPROOF=0, the `kv4` build of `make axknobs`) still
gives the oracle's counts: tests/sproof_knob_child.py in a child process with SPEQ_LIB_PATH pointing at that build
(one library per process), a few scans of both modes at k = 21 and 70. With the switch off the kernel is the one the
rest of the knob builds run through tests/ax_knob_suite.py."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = "-DSPEQ_AX_SPROOF=0"


def test_makefile_builds_the_variant():
    mk = open(os.path.join(ROOT, "Makefile")).read()
    assert f"AXKNOB_kv4 := {FLAGS}\n" in mk
    assert "kv4" in mk.split("AXKNOBS    :=")[1].splitlines()[0].split()
    src = open(os.path.join(ROOT, "speq_amd", "csrc", "ax_common.hpp")).read()
    assert "#if !defined(SPEQ_AX_SPROOF)\n#define SPEQ_AX_SPROOF 1\n" in src  # the default is on


@pytest.mark.gpu
def test_build_without_proofs_matches_oracle():
    lib = os.path.join(ROOT, "build", "axknobs", "kv4", "libspeq_scan.so")
    assert os.path.exists(lib), f"{lib} missing: run `make axknobs` (build() does)"
    env = dict(os.environ, SPEQ_LIB_PATH=lib)
    p = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "sproof_knob_child.py")], env=env,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["ok"] and out["cases"] == 8 and out["lib"] == os.path.realpath(lib)
