"""Inputs of the per-unit report tests (tests/test_read_report_cpu.py validates them against the oracle without a GPU,
tests/test_gpu_read_report.py runs them): synthetic reads plus hand-made reads aimed at the kernel's tile edges."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import em_reference as er
from speq_amd import synth

CUTOFF = 30
KS = [3, 8, 21, 32, 33, 70, 128, 151, 1024]  # below / at the index's prefix_q = 8, packed and LDS searches, many tiles
GOOD = ord("I")  # Phred 40


@lru_cache(maxsize=None)
def base_ref():
    return synth.make_reference(3, 1, 10_000)


@lru_cache(maxsize=None)
def _synth_reads():
    return synth.make_reads(base_ref(), 2_000, n_rate=0.002, lowq_rate=0.01)


def _private_start(rec: int, k: int, length: int, first: bool, lo: int = 100) -> int:
    """A start a (a multiple of 50) such that the first (or last) k-window of records[rec][a:a + length] differs from
    the other two records at the same coordinates; for k < 21 any start will do (nothing is expected of it)."""
    recs = base_ref().records
    if k < 21:
        return lo
    for a in range(lo, len(recs[rec]) - length, 50):
        w0 = a if first else a + length - k
        if all(recs[o][w0:w0 + k] != recs[rec][w0:w0 + k] for o in range(3) if o != rec):
            return a
    raise AssertionError("no private window")


def chimera(k: int) -> bytes:
    """Group 0's sequence joined to group 2's at the same coordinate: the first window is private to group 0, the last
    to group 2, and no window can be unique to group 1."""
    recs = base_ref().records
    H = k + 40
    for a in range(100, len(recs[0]) - 2 * H, 50):
        if k < 21 or (a == _private_start(0, k, H, True, a) and a + H == _private_start(2, k, H, False, a + H)):
            return recs[0][a:a + H] + recs[2][a + H:a + 2 * H]
    raise AssertionError("no chimera")


def _with(read: bytes, qual: bytearray, pos: int, base=None, q=None):
    s = bytearray(read)
    qq = bytearray(qual)
    if base is not None:
        s[pos] = base
    if q is not None:
        qq[pos] = q
    return bytes(s), bytes(qq)


@lru_cache(maxsize=None)
def base_read_list(k: int):
    """(seqs, quals): the 2,000 synthetic reads, then the hand-made ones; an even count, the split pair last."""
    recs = base_ref().records
    rd = _synth_reads()
    seqs = [rd.seq[int(a):int(b)].tobytes() for a, b in zip(rd.offsets[:-1], rd.offsets[1:])]
    quals = [rd.qual[int(a):int(b)].tobytes() for a, b in zip(rd.offsets[:-1], rd.offsets[1:])]

    def add(s: bytes, q: bytes = None):
        seqs.append(s)
        quals.append(bytes([GOOD]) * len(s) if q is None else q)

    # one tile against two tiles, no window, one window, many tiles; a pair with one empty mate (0, then k + 64 ... )
    for i, L in enumerate([0, k + 64, k - 1, k, k + 62, k + 63, 1_000, 151, 152, 1_100]):
        add(recs[1][200 + 37 * i:200 + 37 * i + L])
    # N / a quality equal to the cutoff at the last window start of a tile and the first of the next, and at the last
    # staged position of tile 0 and the first position only tile 1 stages
    long = recs[1][3_000:3_000 + 2 * k + 130]
    for pos in (63, 64, 64 + k - 2, 64 + k - 1):
        add(*_with(long, bytes([GOOD]) * len(long), pos, base=ord("N")))
        add(*_with(long, bytes([GOOD]) * len(long), pos, q=33 + CUTOFF))
        add(*_with(long, bytes([GOOD]) * len(long), pos, q=33 + CUTOFF + 1))  # passes
    low = recs[0][5_000:5_000 + k + 70]
    add(low.lower())
    add(low.replace(b"T", b"U"))
    add(low.lower().replace(b"t", b"u"))
    add(*_with(low, bytes([GOOD]) * len(low), k // 2, q=20))    # a quality byte below 33
    add(*_with(low, bytes([GOOD]) * len(low), len(low) - 1, q=0))
    add(low, bytes([33 + 41 + 5]) * len(low))                  # above the clamp
    c = chimera(k)
    add(c)
    add(er.revcomp(c))
    if len(seqs) % 2:
        add(b"")
    # a pair whose mates each hit one group: ambiguous only as a pair, first_group from mate 1
    L = k + 20
    a0, a1 = _private_start(0, k, L, True, 6_000), _private_start(1, k, L, True, 7_000)
    add(recs[0][a0:a0 + L])
    add(er.revcomp(recs[1][a1:a1 + L]))
    return seqs, quals


def split_pair_unit(k: int) -> int:
    return len(base_read_list(k)[0]) // 2 - 1


def pack(seqs, quals):
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    return b"".join(seqs), b"".join(quals), off


def base_reads(k: int, paired: bool = False):
    """(seq, qual, offsets) of base_read_list(k); paired: consecutive records are mates."""
    return pack(*base_read_list(k))


def tiled(seq: bytes, qual: bytes, off: np.ndarray, n: int):
    """(seq, qual, offsets) of n records: the read set repeated end to end, the last repeat cut after a record."""
    n0 = len(off) - 1
    i = np.arange(n + 1, dtype=np.int64)
    off_t = ((i // n0) * int(off[n0]) + off[i % n0].astype(np.int64)).astype(np.uint64)
    nb = int(off_t[n])
    return (np.resize(np.frombuffer(seq, np.uint8), nb).tobytes(), np.resize(np.frombuffer(qual, np.uint8), nb).tobytes(),
            off_t)


# ---- more than 64 groups: 70 groups of one random 300-bp record ----
MANY_K = 21


@lru_cache(maxsize=None)
def many_ref():
    rng = np.random.default_rng(70)
    records = [bytes(b"ACGT"[c] for c in rng.integers(0, 4, 300)) for _ in range(70)]
    return records, list(range(70))


@lru_cache(maxsize=None)
def many_reads():
    recs, _ = many_ref()
    seqs = [recs[g][10:110] for g in (0, 63, 64, 69)]
    seqs += [er.revcomp(recs[g][150:250]) for g in (0, 63, 64, 69)]
    seqs.append(recs[63][0:80] + recs[64][80:160])             # bits 63 and 64: the two words of the set
    seqs.append(recs[69][0:80] + recs[0][80:160])
    seqs.append(recs[1][0:60] + recs[65][60:120] + recs[33][120:180])
    seqs.append(b"ACGT" * 30)
    return pack(seqs, [bytes([GOOD]) * len(s) for s in seqs])
