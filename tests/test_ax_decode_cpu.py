"""No GPU: the staging decode of one 16-base chunk (speq_amd/csrc/ax_decode.hpp), the formulas k_scan_ax's refill runs.

tests/ax_decode_check.cpp includes nothing but ax_decode.hpp and is compiled here with plain g++ and no ROCm include
path (the header's host side stands in plain C++ for v_perm_b32 and v_dot4_u32_u8). The contract is stated below in
numpy, byte by byte, not taken from the header:
  code    ((b | 0x20) >> 1 ^ (b | 0x20) >> 2) & 3 of every byte, base j at bits 2 j of the code word
  bad     bit j: byte j is none of ACGTUacgtu, or clamp(q - 33, 0, 41) <= cutoff (a quality byte of 128 or more
          counts as 41; from cutoff 41 on every base is bad)
  change  bit j: quality byte j differs from byte j - 1 (bit 0: from the byte before the chunk); 0 in global mode
Inputs: every base byte x every quality byte in each of the 16 chunk positions, the chunk's other bytes random (a chunk
holds 16 such pairs, drawn by an independent permutation per position), at each cutoff of CUTOFFS; uniform chunks; a
previous quality byte equal and unequal to byte 0."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTOFFS = (0, 1, 29, 30, 31, 40, 41, 42, 93, 94, 222)


def compile_check(exe, extra=()):
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                    "-I", os.path.join(ROOT, "speq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "ax_decode_check.cpp"), "-o", exe], check=True)


def run_blocks(exe, blocks):
    """blocks: [(cutoff, bases [n, 16] u8, quals [n, 16] u8, prev [n] u8)] -> per block (cw, bad, chg) of the local-mode
    decode, after checking that the global-mode decode gives the same code word and bad bits and no change bits."""
    payload = bytearray()
    for cutoff, b, q, prev in blocks:
        rec = np.concatenate([b, q, prev[:, None]], axis=1).astype(np.uint8)
        payload += struct.pack("<II", len(rec), cutoff) + rec.tobytes()
    p = subprocess.run([exe], input=bytes(payload), capture_output=True, check=True)
    assert p.stderr == b"", p.stderr[-2000:]
    out = np.frombuffer(p.stdout, dtype="<u4").reshape(-1, 4)
    assert len(out) == sum(len(b) for _, b, _, _ in blocks)
    assert np.array_equal(out[:, 0], out[:, 2]) and np.array_equal(out[:, 1] & 0xFFFF, out[:, 3])
    res, at = [], 0
    for _, b, _, _ in blocks:
        o = out[at:at + len(b)]
        at += len(b)
        res.append((o[:, 0], o[:, 1] & 0xFFFF, o[:, 1] >> 16))
    return res


def contract(cutoff, b, q, prev):
    x = (b | 0x20).astype(np.uint32)
    code = ((x >> 1) ^ (x >> 2)) & 3
    sh2 = (2 * np.arange(16)).astype(np.uint32)
    sh1 = np.arange(16).astype(np.uint32)
    cw = (code << sh2).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    letter = np.isin(b, np.frombuffer(b"ACGTUacgtu", dtype=np.uint8))
    qi = q.astype(np.int64)
    rank = np.where(qi >= 128, 41, np.clip(qi - 33, 0, 41))
    badb = ~letter | (rank <= cutoff)
    bad = (badb.astype(np.uint32) << sh1).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    before = np.concatenate([prev[:, None], q[:, :15]], axis=1)
    chg = ((q != before).astype(np.uint32) << sh1).sum(axis=1, dtype=np.uint64).astype(np.uint32)
    return cw, bad, chg


def check_blocks(exe, blocks):
    for (cutoff, b, q, prev), (cw, bad, chg) in zip(blocks, run_blocks(exe, blocks)):
        ecw, ebad, echg = contract(cutoff, b, q, prev)
        for name, got, exp in (("code", cw, ecw), ("bad", bad, ebad), ("change", chg, echg)):
            ne = np.flatnonzero(got != exp)
            assert ne.size == 0, (name, cutoff, bytes(b[ne[0]]), bytes(q[ne[0]]), int(prev[ne[0]]),
                                  hex(int(got[ne[0]])), hex(int(exp[ne[0]])))


def all_pairs_block(rng):
    """65,536 chunks in which every (base byte, quality byte) pair stands once at each of the 16 positions."""
    b = np.empty((65536, 16), dtype=np.uint8)
    q = np.empty((65536, 16), dtype=np.uint8)
    for pos in range(16):
        pair = rng.permutation(65536)
        b[:, pos] = pair >> 8
        q[:, pos] = pair & 0xFF
    prev = rng.integers(0, 256, 65536).astype(np.uint8)
    prev[::2] = q[::2, 0]  # half the chunks: the byte before equals byte 0
    return b, q, prev


def uniform_blocks():
    """all-N, all-u, all-0xFF (and clean all-A) chunks at every quality byte, the byte before equal and not."""
    qs = np.arange(256, dtype=np.uint8)
    out = []
    for base in (ord("N"), ord("u"), 0xFF, ord("A")):
        b = np.full((512, 16), base, dtype=np.uint8)
        q = np.repeat(np.concatenate([qs, qs])[:, None], 16, axis=1)
        prev = np.concatenate([qs, qs + np.uint8(1)])
        out.append((b, q, prev))
    # all-0xFF qualities too, and runs of equal qualities with one step at every position
    b = np.full((17, 16), ord("C"), dtype=np.uint8)
    q = np.full((17, 16), 0xFF, dtype=np.uint8)
    for j in range(16):
        q[j, j:] = 50
    out.append((b, q, np.full(17, 0xFF, dtype=np.uint8)))
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("ax_decode") / "ax_decode_check")
    compile_check(path)
    return path


def test_every_base_and_quality_byte_at_every_position(exe):
    rng = np.random.default_rng(409)
    check_blocks(exe, [(cutoff, *all_pairs_block(rng)) for cutoff in CUTOFFS])


def test_uniform_chunks_and_previous_quality(exe):
    check_blocks(exe, [(cutoff, *blk) for cutoff in CUTOFFS for blk in uniform_blocks()])


def test_hand_worked_chunk(exe):
    # ACGTUacgtuNn.-Rx at quality I (40) except a '#' (2) under the first G and a 0x80 under the last a
    b = np.frombuffer(b"ACGTUacgtuNn.-Rx", dtype=np.uint8)[None, :].copy()
    q = np.full((1, 16), ord("I"), dtype=np.uint8)
    q[0, 2] = ord("#")
    q[0, 5] = 0x80
    (cw, bad, chg), = run_blocks(exe, [(30, b, q, np.array([ord("I")], dtype=np.uint8))])
    assert int(cw[0]) & 0xFFFFF == sum(c << (2 * j) for j, c in enumerate([0, 1, 2, 3, 3, 0, 1, 2, 3, 3]))
    assert int(bad[0]) == 0b1111110000000100  # the low-quality G and the six non-bases; 0x80 passes as rank 41
    assert int(chg[0]) == 0b0000000001101100  # steps into and out of positions 2 and 5
    (_, bad41, _), = run_blocks(exe, [(41, b, q, np.array([0], dtype=np.uint8))])
    assert int(bad41[0]) == 0xFFFF


def test_sanitized_build_runs_clean(tmp_path):
    exe = str(tmp_path / "ax_decode_check_san")
    compile_check(exe, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rng = np.random.default_rng(7)
    check_blocks(exe, [(30, *all_pairs_block(rng))] + [(cutoff, *blk) for cutoff in (0, 41) for blk in uniform_blocks()])
