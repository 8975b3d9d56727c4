"""Exact pure-Python reference of the EM histogram (no GPU, no C; shares nothing with oracle/kmer_oracle.c).

The histogram of a read set is integers: for every passing window whose k-mer occurs in the texts of two or more
groups, the k-mer's per-group occurrence counts and how many such windows there were. So it is stated here exactly,
from a dictionary of every k-mer of every record and of its reverse complement, and the GPU's rows are compared with
it entry by entry (tests/test_gpu_em_rows.py); tests/test_em_reference_cpu.py checks this file against the C oracle.

Window filter, as oracle/kmer_oracle.c:321-325 states it: bases go through dna5 (ACGT/acgt, U/u -> T, anything else
N), qualities are byte - 33 clamped to 0..41, and a window passes iff each of its k qualities is > cutoff and none of
its k bases is N.
"""
from __future__ import annotations

from collections import Counter
from dataclasses import dataclass, field
from fractions import Fraction
from math import lcm

import numpy as np

_DNA5 = bytearray(b"N" * 256)
for _a, _b in zip(b"ACGTacgtUu", b"ACGTACGTTT"):
    _DNA5[_a] = _b
_DNA5 = bytes(_DNA5)
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
_N = ord("N")


def dna5(s: bytes) -> bytes:
    return bytes(s).translate(_DNA5)


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def _n_free_windows(text: bytes, k: int) -> list[int]:
    """Starts of the windows of text that hold no N."""
    if len(text) < k:
        return []
    bad = np.concatenate([[0], np.cumsum(np.frombuffer(text, dtype=np.uint8) == _N)])
    return np.flatnonzero(bad[k:] == bad[:-k]).tolist()


def build_index(records, groups, G: int, k: int) -> dict:
    """{k-mer: ((group, occurrences), ...) by ascending group} over every record and its reverse complement. Every
    occurrence counts (a k-mer equal to its own reverse complement counts twice per place it lies in a record);
    windows with an N, or past a record's end, do not exist."""
    acc: dict = {}
    for rec, g in zip(records, groups):
        assert 0 <= g < G
        fwd = dna5(rec)
        for text in (fwd, revcomp(fwd)):
            for i in _n_free_windows(text, k):
                w = text[i:i + k]
                d = acc.get(w)
                if d is None:
                    acc[w] = {g: 1}
                else:
                    d[g] = d.get(g, 0) + 1
    shared: dict = {}  # equal contents share one tuple
    return {w: shared.setdefault(c, c) for w, c in ((w, tuple(sorted(d.items()))) for w, d in acc.items())}


def passing_windows(seq: np.ndarray, qual: np.ndarray, k: int, cutoff: int) -> np.ndarray:
    """Starts of the passing windows of one read (seq after dna5, qual raw Phred+33 bytes)."""
    if len(seq) < k:
        return np.zeros(0, dtype=np.int64)
    q = np.clip(qual.astype(np.int32) - 33, 0, 41)
    bad = np.concatenate([[0], np.cumsum((q <= cutoff) | (seq == _N))])
    return np.flatnonzero(bad[k:] == bad[:-k])


@dataclass
class Histogram:
    """What a scan of one read set must produce."""
    G: int
    k: int
    total: int = 0                                   # passing windows (T)
    absent: int = 0                                  # passing windows whose k-mer is in no text
    unique: list = field(default_factory=list)       # single-group windows per group (U)
    multi: dict = field(default_factory=dict)        # k-mer -> (content, multiplicity) of the multi-group windows
    multi_at: list = field(default_factory=list)     # per read: starts of its multi-group windows

    @property
    def n_windows(self) -> int:
        return sum(m for _, m in self.multi.values())

    @property
    def n_intervals(self) -> int:
        return len(self.multi)  # (a k-mer and its reverse complement are two intervals)

    @property
    def n_entries(self) -> int:
        return sum(len(c) for c, _ in self.multi.values())

    @property
    def unmerged(self) -> Counter:
        """Multiset of (content, multiplicity), one per distinct k-mer."""
        return Counter(self.multi.values())

    @property
    def merged(self) -> dict:
        out: dict = {}
        for c, m in self.multi.values():
            out[c] = out.get(c, 0) + m
        return out


def scan(index: dict, G: int, k: int, seq, qual, offsets, cutoff: int = 30, paired: bool = False) -> Histogram:
    """Classifies every passing window of the reads (arguments as Oracle.scan takes them; mates share nothing that
    the histogram sees, so `paired` only asks for an even record count)."""
    seq_b = seq.tobytes() if isinstance(seq, np.ndarray) else bytes(seq)
    qual_b = qual.tobytes() if isinstance(qual, np.ndarray) else bytes(qual)
    off = [int(x) for x in offsets]
    if paired and (len(off) - 1) % 2:
        raise ValueError("paired scan needs an even record count")
    s5 = dna5(seq_b)
    s_arr = np.frombuffer(s5, dtype=np.uint8)
    q_arr = np.frombuffer(qual_b, dtype=np.uint8)
    h = Histogram(G, k, unique=[0] * G)
    mult: dict = {}
    for r in range(len(off) - 1):
        a, b = off[r], off[r + 1]
        at = []
        for j in passing_windows(s_arr[a:b], q_arr[a:b], k, cutoff).tolist():
            h.total += 1
            w = s5[a + j:a + j + k]
            c = index.get(w)
            if c is None:
                h.absent += 1
            elif len(c) == 1:
                h.unique[c[0][0]] += 1
            else:
                mult[w] = mult.get(w, 0) + 1
                at.append(j)
        h.multi_at.append(at)
    h.multi = {w: (index[w], m) for w, m in mult.items()}
    return h


def _tree_sum(xs: list) -> Fraction:
    """Exact sum; pairwise, so that the big denominators meet late."""
    if not xs:
        return Fraction(0)
    while len(xs) > 1:
        xs = [xs[i] + xs[i + 1] if i + 1 < len(xs) else xs[i] for i in range(0, len(xs), 2)]
    return xs[0]


def exact_step(percent, counts, unique, merged: dict) -> list:
    """next[g] = sum over windows of (c_g p_g / n_g) / sum_j (c_j p_j / n_j), windows with a non-positive sum skipped,
    single-group windows (unique[g] of them, c = 1 or more: the ratio is 1) included; exact rationals over the binary
    values of percent. merged: {content: multiplicity} of the multi-group windows."""
    G = len(counts)
    w = [Fraction(float(percent[g])) / int(counts[g]) for g in range(G)]
    den = lcm(*[x.denominator for x in w])
    wi = [int(x * den) for x in w]  # p_g / n_g over one denominator: only the ratios matter
    terms: list = [dict() for _ in range(G)]
    for content, m in merged.items():
        norm = sum(c * wi[g] for g, c in content)
        if norm <= 0:
            continue
        for g, c in content:
            t = terms[g]
            t[norm] = t.get(norm, 0) + m * c * wi[g]
    out = []
    for g in range(G):
        single = int(unique[g]) if wi[g] > 0 else 0
        out.append(single + _tree_sum([Fraction(n, d) for d, n in terms[g].items()]))
    return out


def max_relative_deviation(got, exact: list) -> float:
    """max_g |got_g - exact_g| / exact_g (0 where both are 0, inf where only exact is 0), computed exactly."""
    worst = Fraction(0)
    for x, e in zip(got, exact):
        d = abs(Fraction(float(x)) - e)
        if d == 0:
            continue
        if e == 0:
            return float("inf")
        worst = max(worst, d / abs(e))
    return float(worst)
