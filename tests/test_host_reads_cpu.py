"""No GPU: the host entry points' batch cut and array checks (speq_amd/csrc/host_reads.hpp).

tests/host_reads_check.cpp includes nothing but host_reads.hpp and is compiled here with plain g++ and no ROCm include
path: that it compiles is the proof that the header is host-only. The expected cuts are worked out by hand below, at
limits of 4 records and 10 bases, and by `rule`, the cut stated in Python; neither comes from the header."""
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    """lines of the program's input -> its output lines."""
    exe = str(tmp_path_factory.mktemp("host_reads") / "host_reads_check")
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "speq_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host_reads_check.cpp"),
                    "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(x + "\n" for x in lines), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out

    return run


def cut_line(step, max_records, max_bytes, lengths):
    return " ".join(str(x) for x in ["cut", step, max_records, max_bytes, len(lengths), *lengths])


def rule(lengths, step, max_records, max_bytes):
    """The batch ends: a batch takes its first unit of `step` reads whatever its size, then whole units while it holds
    at most max_records reads and max_bytes bases."""
    ends, r0 = [], 0
    while r0 < len(lengths):
        r1 = r0 + step
        while r1 < len(lengths) and r1 + step - r0 <= max_records and sum(lengths[r0:r1 + step]) <= max_bytes:
            r1 += step
        ends.append(r1)
        r0 = r1
    return ends


# name: (step, lengths, the batch ends), all at 4 records / 10 bases
CASES = {
    "record-cap-exact": (1, [1, 1, 1, 1], [4]),
    "record-cap-one-more": (1, [1, 1, 1, 1, 1], [4, 5]),
    "byte-cap-exact": (1, [5, 5, 1], [2, 3]),           # 5 + 5 = 10 stays, the third read would make 11
    "byte-cap-one-more": (1, [5, 6, 1], [1, 3]),        # 5 + 6 = 11: the first read alone, then 6 + 1
    "oversize-first": (1, [11, 1, 1], [1, 3]),
    "oversize-middle": (1, [1, 11, 1], [1, 2, 3]),      # 1 | 11 alone (11 + 1 > 10) | 1
    "pairs-whole": (2, [3, 3, 3, 5], [2, 4]),           # 3 + 3 + 3 = 9 would fit, the pair (3, 5) makes 14 ...
    "pairs-whole-as-reads": (1, [3, 3, 3, 5], [3, 4]),  # ... and single reads do take the third
    "pairs-record-cap": (2, [1, 1, 1, 1, 1, 1], [4, 6]),
    "oversize-pair": (2, [7, 8, 1, 1], [2, 4]),
    "zero-length": (1, [0, 0, 0, 0, 0], [4, 5]),
    "zero-length-after-full": (1, [10, 0, 0, 0, 1], [4, 5]),  # 10 bases and four records: both caps hit exactly
    "zero-length-around-oversize": (1, [0, 11, 0], [1, 2, 3]),
    "one-read": (1, [7], [1]),
    "one-pair": (2, [7, 8], [2]),
    "one-empty-read": (1, [0], [1]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_hand_worked_cuts(name, check):
    step, lengths, ends = CASES[name]
    assert rule(lengths, step, 4, 10) == ends, "the rule as stated in this file"
    (line,) = check([cut_line(step, 4, 10, lengths)])
    assert [int(x) for x in line.split()] == ends


def test_random_cuts_partition_within_caps_and_maximal(check):
    rng = random.Random(20)
    cases = []
    for _ in range(300):
        step = rng.choice([1, 2])
        max_records = step * rng.randint(1, 4)  # (every caller's record cap is a multiple of its unit)
        max_bytes = rng.randint(1, 12)
        n = step * rng.randint(1, 12)
        lengths = [rng.choice([0, 0, 1, 2, 3, 5, max_bytes, max_bytes + 1]) for _ in range(n)]
        cases.append((step, max_records, max_bytes, lengths))
    out = check([cut_line(*c) for c in cases])
    for (step, max_records, max_bytes, lengths), line in zip(cases, out):
        ends = [int(x) for x in line.split()]
        ctx = f"step {step}, {max_records} records / {max_bytes} bases, lengths {lengths}: ends {ends}"
        assert ends == rule(lengths, step, max_records, max_bytes), ctx
        assert ends[-1] == len(lengths) and all(b > a for a, b in zip([0] + ends, ends)), ctx  # a partition of [0, n)
        for r0, r1 in zip([0] + ends, ends):
            assert (r1 - r0) % step == 0, ctx
            within = r1 - r0 <= max_records and sum(lengths[r0:r1]) <= max_bytes
            assert within or r1 - r0 == step, ctx  # within the caps, or a single unit
            if r1 < len(lengths):  # maximal: one more unit would break a cap
                assert r1 + step - r0 > max_records or sum(lengths[r0:r1 + step]) > max_bytes, ctx


def test_check_host_reads_messages(check):
    assert check(["check 0 3 0 5 5 9",    # non-decreasing, with an empty read
                  "check 0 2 0 5 3",      # decreasing
                  "check 0 2 7 5 9",      # decreasing at the first read, though the last offset is the largest
                  "check 1 2 0 5 9",      # bases and no buffers
                  "check 1 2 4 4 4",      # no bases: the buffers may be null
                  "check 1 0 0"]) == ["ok", "who: offsets must be non-decreasing", "who: offsets must be non-decreasing",
                                      "who: null read buffer", "ok", "ok"]


def test_check_report_k_message(check):
    bad = "who: k must be in [1, 1024]"
    assert check(["k 0", "k 1", "k 21", "k 1024", "k 1025", "k 4294967295"]) == [bad, "ok", "ok", "ok", bad, bad]
