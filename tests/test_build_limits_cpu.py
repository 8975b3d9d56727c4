"""No GPU: the size and memory decisions of the library (speq_amd/csrc/build_limits.hpp) on both sides of their edges.

tests/build_limits_check.cpp includes nothing of the project but build_limits.hpp and is compiled here with plain g++
and no ROCm include path: that it compiles is the proof that the header is host-only. It checks

* every free-memory decision (the three of build_ax, ensure_ax_em's, the two of build_ktab) at the smallest free_b that
  passes, worked out as ten times the tenths needed, and at the 12 values on either side (the truncation of
  free_b / 10 * 9 included), and that the bytes each compares are at least the bytes allocated after it;
* every 32-bit offset decision of build_ax at limit - 64 and one less, at the real 2^32 and at lowered limits: the
  m-mer filter goes before the table is refused, the bitmap has room or is dropped, and over a sweep of (n, k,
  distinct, n_texts, load) x limits every offset the kernel forms from the layout, and the descriptor length it builds,
  is exact in 32 bits and below the limit;
* the plane predicate at nb = 4,194,303 / 4,194,304 (three-symbol planes) and 16,777,215 / 16,777,216 (two-symbol
  planes) against the device's own 32-bit arithmetic, restated;
* that build_ktab's second (compact) check fires on its own at the default tuning.

The second build runs the same program under the address and undefined-behaviour sanitizers (a stand-alone program:
nothing is preloaded)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "sanitized"])
def test_every_decision_on_both_sides_of_its_edge(flags, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "build_limits_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags,
                    "-I", os.path.join(ROOT, "speq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "build_limits_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout[-4000:], run.stderr[-2000:])
    m = re.fullmatch(r"ok layouts=(\d+) compact_check_alone=(\d+)", run.stdout.strip())
    assert m, run.stdout[-2000:]
    assert int(m.group(1)) > 5000 and int(m.group(2)) > 0


def test_the_library_asks_for_free_memory_in_one_place():
    """dev_mem.cpp's free_bytes() is the only hipMemGetInfo of the library, so the test switch sees every query."""
    src = os.path.join(ROOT, "speq_amd", "csrc")
    users = sorted(f for f in os.listdir(src) if "hipMemGetInfo(" in open(os.path.join(src, f)).read())
    assert users == ["dev_mem.cpp"]
