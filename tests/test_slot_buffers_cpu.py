"""No GPU: the buffers of a pipeline slot (speq_amd/csrc/slot_buffers.hpp) over malloc and free.

tests/slot_buffers_check.cpp includes nothing of the project but slot_buffers.hpp and dev_mem.hpp and defines the four
functions they are written against itself (device and pinned allocation and release), with counters and a fail-the-nth
switch; it is compiled here with plain g++ and no ROCm include path: that it compiles is the proof that the header is
host-only. For ensure (fresh, growing, adding qualities), ensure_parse (fresh and growing, with and without scratch),
full and the moves it fails every allocation of the operation once and checks field by field that the set is then
exactly as it was or empty, that the same call then succeeds, and that every allocation was freed exactly once, the way
it was obtained. It includes the case the type exists for: a quality buffer whose device half fails. The second build
runs the same program under the address and undefined-behaviour sanitizers (a stand-alone program: nothing is
preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "sanitized"])
def test_a_failed_allocation_leaves_the_set_whole_or_empty(flags, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "slot_buffers_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags,
                    "-I", os.path.join(ROOT, "speq_amd", "csrc"), os.path.join(ROOT, "tests", "slot_buffers_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr[-2000:])
