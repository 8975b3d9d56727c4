"""No GPU: the phase-1 arithmetic of k_scan_ax that SPEQ_AX_LEAN put in speq_amd/csrc/ax_phase1.hpp.

tests/ax_phase1_check.cpp includes nothing but that header and is compiled here with plain g++ and no ROCm include path
(the header's host side states v_alignbit_b32, v_ffbl_b32 of zero and the saturating add in plain C++), once plain and
once with -fsanitize=address,undefined, and run as its own program:
  first mismatch   axp_first_mismatch against a base-by-base loop over byte arrays: every text offset s5 0..31 x every
                   read shift 0..15 x a mismatch at every base 0..159 and none (cl = 160, cl just before and just past
                   the mismatch, a random cl, and random bases from cl on), and 64 pairs of mismatches per (s5, shift)
The program counts its cases; the counts are checked here so that a loop that shrinks is noticed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (160 mismatch positions x 5 compares - the one skipped at base 0) + 4 without a mismatch + 64 pairs x 2, per (s5, shift)
MISMATCH_CASES = 32 * 16 * (161 * 5 - 2 + 64 * 2)


def compile_check(exe, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(ROOT, "speq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ax_phase1_check.cpp"), "-o", exe], check=True)


def run_part(exe, part):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-500:], p.stderr[-2000:])
    m = re.fullmatch(part + r" cases=(\d+) fail=(\d+)\n", p.stdout)
    assert m, p.stdout
    return int(m.group(1)), int(m.group(2))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ax_phase1") / "ax_phase1_check")
    compile_check(path)
    return path


def test_first_mismatch_equals_base_by_base_loop(exe):
    assert run_part(exe, "mismatch") == (MISMATCH_CASES, 0)


def test_sanitized_build_runs_clean(tmp_path):
    exe = str(tmp_path / "ax_phase1_check_san")
    compile_check(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert run_part(exe, "mismatch") == (MISMATCH_CASES, 0)
