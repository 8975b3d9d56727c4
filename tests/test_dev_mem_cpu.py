"""No GPU: the owner of device memory (speq_amd/csrc/dev_mem.hpp) over malloc and free.

tests/dev_mem_check.cpp includes nothing of the project but dev_mem.hpp and defines the two functions the header is
written against itself, with counters and a fail-the-nth switch; it is compiled here with plain g++ and no ROCm include
path: that it compiles is the proof that the header is host-only. It checks that a destructor frees once, that a move
and a move assignment empty their source, that release() hands the pointer over, that reset() frees once, that no
request is below 16 bytes, that a failing nth allocation among several owners frees exactly the ones already made, and
that DevTemp grows, keeps its buffer for a smaller request and frees once. The second build runs the same program under
the address and undefined-behaviour sanitizers (a stand-alone program: nothing is preloaded)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "sanitized"])
def test_owner_frees_once_and_moves(flags, tmp_path):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = str(tmp_path / "dev_mem_check")
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags,
                    "-I", os.path.join(ROOT, "speq_amd", "csrc"), os.path.join(ROOT, "tests", "dev_mem_check.cpp"),
                    "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr[-2000:])
