"""Inputs of the duplicate-read tests (tests/test_dedup_cpu.py checks them against the model without a GPU,
tests/test_gpu_dedup.py runs them): hand-made units aimed at the fingerprint kernel's lane stride and at what must and
must not count as a duplicate, classes of every histogram bin, and real reads with a known subset repeated.

A unit list holds (mate 1, quality 1) for the single flavour; the paired flavour gives every unit the mate
mate_of(mate 1), a function of the converted bases alone, so that duplicates stay duplicates, and appends the cases that
only pairs have."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import em_reference as er
import read_report_inputs as ri

EDGE_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129, 150, 1000]  # both sides of every 64-lane stride
CLASS_SIZES = [1, 2, 4, 5, 7, 8, 9, 4096]                      # the histogram's bin edges (with the classes of 3 and 6
                                                               # below every bin is filled), and one large class
REPEATED = list(range(0, 500, 10))                             # the real reads that get a second copy
GOOD = ri.GOOD


def _rand(rng, n: int) -> bytes:
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, n))


def _q(rng, n: int) -> bytes:
    """Qualities of both sides of the tests' cutoff of 30."""
    return bytes(rng.choice(np.array([GOOD, GOOD, GOOD, 33 + 30, 33 + 12], dtype=np.uint8), n).tolist())


def _q1(rng, n: int) -> bytes:
    """Good qualities but for one position, which differs from copy to copy."""
    q = bytearray([GOOD]) * n
    if n:
        q[int(rng.integers(0, n))] = 33 + 12
    return bytes(q)


def mate_of(s: bytes, q: bytes):
    """Mate 2 of a unit of the paired flavour: the reverse complement of the converted mate 1 without its first three
    bases (in the index, like mate 1), with mate 1's qualities reversed."""
    return er.revcomp(er.dna5(s))[3:], q[::-1][3:]


@lru_cache(maxsize=None)
def unit_list(k: int):
    """[(seq, qual)]: an opener of one base, the edge block in order (every edge read behind a filler whose length makes
    the read start at an odd offset), then everything else in a fixed shuffled order. Returns (units, edge_index):
    edge_index[L] is the position of the read of EDGE_LENGTHS entry L."""
    rng = np.random.default_rng(4096)
    recs = ri.base_ref().records
    units = [(b"G", bytes([GOOD]))]
    at = 1
    edge_index = {}
    for L in EDGE_LENGTHS:
        fill = 7 if (at + 7) % 2 else 8
        units.append((_rand(rng, fill), bytes([GOOD]) * fill))
        at += fill
        edge_index[L] = len(units)
        units.append((recs[0][2_000:2_000 + L], bytes([GOOD]) * L))
        at += L
    rest = []
    # a second copy of every edge read (two empty units among them)
    for L in EDGE_LENGTHS:
        rest.append((recs[0][2_000:2_000 + L], _q(rng, L)))
    x = recs[1][4_000:4_150]
    other = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
    rest += [(x, bytes([GOOD]) * 150),
             (other[x[0]] + x[1:], bytes([GOOD]) * 150),          # differs in the first base only
             (x[:-1] + other[x[-1]], bytes([GOOD]) * 150),        # in the last base only
             (x[:-1], bytes([GOOD]) * 149), (x[:64], bytes([GOOD]) * 64), (x[1:], bytes([GOOD]) * 149)]  # prefixes, a shift
    # one read in every spelling the scan converts alike: a class of 6
    y = bytearray(recs[2][6_000:6_120])
    y[40] = ord("N")
    y = bytes(y)
    assert b"T" in y
    for v in (y, y.lower(), y.replace(b"T", b"U"), y.lower().replace(b"t", b"u"), y.replace(b"N", b"R"),
              y.replace(b"N", b".")):
        rest.append((v, bytes([GOOD]) * len(v)))
    # copies that differ in their qualities only: a class of 3
    z = recs[0][7_000:7_151]
    rest += [(z, bytes([GOOD]) * 151), (z, _q(rng, 151)), (z, b"!" * 151)]
    # classes of every bin edge; the large one is a short read of the reference, so its copies carry windows at k = 21
    for size in CLASS_SIZES:
        s = recs[2][1_234:1_234 + 60] if size == 4096 else recs[size % 3][3_000 + 200 * size:3_000 + 200 * size + 90 + size]
        for _ in range(size):
            rest.append((s, _q1(rng, len(s))))
    # real reads, and a known subset of them once more with qualities of their own
    seqs, quals = ri.base_read_list(k)
    rest += list(zip(seqs, quals))
    rest += [(seqs[i], bytes([GOOD]) * len(seqs[i])) for i in REPEATED]
    order = rng.permutation(len(rest))
    units += [rest[i] for i in order]
    return units, edge_index


PAIR_CASES = [  # mate 1, mate 2
    (b"ACGTACGTAC", b"TTGACCA"), (b"ACGTACGTAC", b"TTGACCC"),  # same mate 1, another mate 2
    (b"TTGACCA", b"ACGTACGTAC"),                               # the first pair with its mates swapped
    (b"AC", b"G"), (b"A", b"CG"),
    (b"GATTACA", b""), (b"", b"GATTACA"),
    (b"ACGTACGTAC", b"TTGACCA"), (b"acgtacguac", b"UUGACCA"),   # true duplicates of the first pair
    (b"", b""), (b"", b""),
]


@lru_cache(maxsize=None)
def reads(k: int, paired: bool):
    """(seq, qual, offsets) of the flavour's records."""
    units, _ = unit_list(k)
    seqs, quals = [], []
    for s, q in units:
        seqs.append(s)
        quals.append(q)
        if paired:
            s2, q2 = mate_of(s, q)
            seqs.append(s2)
            quals.append(q2)
    if paired:
        for a, b in PAIR_CASES:
            seqs += [a, b]
            quals += [bytes([GOOD]) * len(a), bytes([GOOD]) * len(b)]
    return ri.pack(seqs, quals)


def n_units(k: int, paired: bool) -> int:
    return len(unit_list(k)[0]) + (len(PAIR_CASES) if paired else 0)


# ---- more units than one storage chunk of the handle (65,536) ----
@lru_cache(maxsize=None)
def chunk_reads():
    """66,000 single-end units of 1 to 9 bases over ACGN: many small classes and a few thousand singletons, cheap to
    fingerprint, and the units 65,535 / 65,536 lie on both sides of the handle's first chunk boundary."""
    rng = np.random.default_rng(65_536)
    lens = rng.integers(1, 10, 66_000)
    seqs = [bytes(b"ACGN"[c] for c in rng.integers(0, 4, n)) for n in lens.tolist()]
    return ri.pack(seqs, [bytes([GOOD]) * len(s) for s in seqs])


# ---- files ----
def _mutated(rng, s: bytes) -> bytes:
    b = bytearray(s)
    for p in rng.integers(0, len(b), 3).tolist():
        b[p] = b"ACGT"[(b"ACGT".find(bytes([b[p]]).upper()) + 1) % 4]
    return bytes(b)


@lru_cache(maxsize=None)
def fastq_records(name: str, n: int = 40_000):
    """(seqs, quals, paired) of n records (more than one of the sequential reader's 32,768-record blocks, so that a
    block's first record index matters) made from the golden case's reads: each record (pair) is a read (pair)
    of the case with three bases changed at random, and every fifth unit is a copy of an earlier one, with qualities of
    its own, so that classes of several sizes arise."""
    from golden_io import Case
    c = Case(name)
    rng = np.random.default_rng(len(name))
    off = [int(x) for x in c.offsets]
    per = 2 if c.paired else 1
    src = [[(c.seq[off[r]:off[r + 1]], c.qual[off[r]:off[r + 1]]) for r in range(per * u, per * u + per)]
           for u in range((len(off) - 1) // per)]
    units = []
    for i in range(n // per):
        if i % 5 == 4:
            j = int(rng.integers(0, min(len(units), 200)))
            units.append([(s, _q1(rng, len(s))) for s, _ in units[j]])
        else:
            u = src[int(rng.integers(0, len(src)))]
            units.append([(_mutated(rng, s) if len(s) else s, q) for s, q in u])
    seqs = [s for u in units for s, _ in u]
    quals = [q for u in units for _, q in u]
    return seqs, quals, c.paired


@lru_cache(maxsize=None)
def cli_records(name: str):
    """(uniq, dup, paired): `uniq` the units of the golden case, each once (the case's own duplicates taken out by exact
    comparison of the converted bases), as lists of (seq, qual) per unit; `dup` the same with copies of every third unit
    inserted two units later (other qualities), and one unit seven times more at the end."""
    from golden_io import Case
    c = Case(name)
    rng = np.random.default_rng(7)
    off = [int(x) for x in c.offsets]
    per = 2 if c.paired else 1
    seen, uniq = set(), []
    for u in range((len(off) - 1) // per):
        unit = [(c.seq[off[r]:off[r + 1]], c.qual[off[r]:off[r + 1]]) for r in range(per * u, per * u + per)]
        key = tuple(er.dna5(s) for s, _ in unit)
        if key not in seen:
            seen.add(key)
            uniq.append(unit)
    dup, pending = [], {}
    for i, unit in enumerate(uniq):
        dup.append(unit)
        if i % 3 == 0:
            pending[i + 2] = [(s, _q1(rng, len(s))) for s, _ in unit]
        if i in pending:
            dup.append(pending.pop(i))
    dup += list(pending.values())
    dup += [[(s, _q1(rng, len(s))) for s, _ in uniq[1]] for _ in range(7)]
    return uniq, dup, c.paired


def flatten(units):
    """(seq, qual, offsets) of a list of units of (seq, qual) records."""
    return ri.pack([s for u in units for s, _ in u], [q for u in units for _, q in u])


def write_fastq(path: str, seqs, quals, start: int = 0, step: int = 1, gz: bool = False):
    import gzip
    data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, seqs[i], quals[i]) for i in range(start, len(seqs), step))
    with (gzip.open(path, "wb", compresslevel=1) if gz else open(path, "wb")) as f:
        f.write(data)


def split(rd, r0: int, r1: int):
    """(seq, qual, offsets from 0) of records r0 .. r1 - 1."""
    seq, qual, off = rd
    a, b = int(off[r0]), int(off[r1])
    return seq[a:b], qual[a:b], off[r0:r1 + 1] - off[r0]
