"""Exact pure-Python model of the per-unit report (speq_report_reads): no GPU, no C, nothing shared with the oracle.

A unit is a read, or the pair (2i, 2i+1). Over em_reference.build_index's dictionary {k-mer: ((group, count), ...)}:
a passing window whose k-mer maps to a content of length 1 is unique to that group, of length 2 or more is shared, and
a missing k-mer is absent. Bases go through em_reference.dna5 and the window filter is em_reference.passing_windows.
"""
from __future__ import annotations

from collections import Counter
from dataclasses import dataclass, field

import numpy as np

import em_reference as er


@dataclass
class Report:
    G: int
    passing: list = field(default_factory=list)      # per unit
    unique: list = field(default_factory=list)
    shared: list = field(default_factory=list)
    first_group: list = field(default_factory=list)  # -1: no unique window
    sets: list = field(default_factory=list)         # frozenset of groups per unit
    per_group: list = field(default_factory=list)    # unique windows per group over all units (the scan's U[g])

    @property
    def n_units(self) -> int:
        return len(self.passing)

    @property
    def W(self) -> int:
        return (self.G + 63) // 64

    @property
    def ambiguous(self) -> int:
        return sum(len(s) >= 2 for s in self.sets)

    def words(self) -> np.ndarray:
        """The sets as [n_units, W] uint64 (bit g % 64 of word g // 64)."""
        out = np.zeros((self.n_units, self.W), dtype=np.uint64)
        for u, s in enumerate(self.sets):
            for g in s:
                out[u, g // 64] |= np.uint64(1 << (g % 64))
        return out

    def histogram(self) -> dict:
        """{group set: units}: what a file-level summary holds."""
        return dict(Counter(self.sets))

    def totals(self) -> dict:
        return {"units": self.n_units, "passing": sum(self.passing), "unique": sum(self.unique),
                "shared": sum(self.shared)}

    def head(self, n_units: int) -> "Report":
        """The report of the first n_units units alone (units are independent)."""
        return Report(self.G, self.passing[:n_units], self.unique[:n_units], self.shared[:n_units],
                      self.first_group[:n_units], self.sets[:n_units], [])


def report(index: dict, G: int, k: int, seq, qual, offsets, cutoff: int = 30, paired: bool = False) -> Report:
    seq_b = seq.tobytes() if isinstance(seq, np.ndarray) else bytes(seq)
    qual_b = qual.tobytes() if isinstance(qual, np.ndarray) else bytes(qual)
    off = [int(x) for x in offsets]
    n = len(off) - 1
    if paired and n % 2:
        raise ValueError("a paired report needs an even record count")
    s5 = er.dna5(seq_b)
    s_arr = np.frombuffer(s5, dtype=np.uint8)
    q_arr = np.frombuffer(qual_b, dtype=np.uint8)
    per = 2 if paired else 1
    rep = Report(G, per_group=[0] * G)
    for u in range(n // per):
        passing = unique = shared = 0
        first, groups = -1, set()
        for r in range(per * u, per * u + per):  # mate 1 before mate 2, windows by ascending start
            a, b = off[r], off[r + 1]
            for j in er.passing_windows(s_arr[a:b], q_arr[a:b], k, cutoff).tolist():
                passing += 1
                c = index.get(s5[a + j:a + j + k])
                if c is None:
                    continue
                if len(c) == 1:
                    g = c[0][0]
                    unique += 1
                    rep.per_group[g] += 1
                    groups.add(g)
                    if first < 0:
                        first = g
                else:
                    shared += 1
        rep.passing.append(passing)
        rep.unique.append(unique)
        rep.shared.append(shared)
        rep.first_group.append(first)
        rep.sets.append(frozenset(groups))
    return rep


def sorted_sets(hist: dict) -> list:
    """The histogram's entries in the library's order: ascending by the set read as one integer."""
    return sorted(hist.items(), key=lambda e: sum(1 << g for g in e[0]))
