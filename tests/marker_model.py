"""Exact pure-Python model of marker coverage (speq_markers_*): no GPU, no C, nothing shared with the oracle.

Over em_reference.build_index's dictionary {k-mer: ((group, count), ...)}: a marker of group g is a k-mer whose content
is ((g, c),), its depth the number of passing read windows (em_reference.passing_windows over em_reference.dna5 bases)
equal to it. A k-mer and its reverse complement are two dictionary keys, so two markers. Per group: markers, observed
(depth >= 1), hits (the sum of depths: the scan's U[g]), max_depth and eight depth bins (exactly j for j < 7, >= 7 for
j = 7). `paired` does not matter: mates are reads like any other.
"""
from __future__ import annotations

import math
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

import em_reference as er

BINS = 8
HEADER = "name\tmarkers\tobserved\tbreadth\thits\tmean_depth\texpected_breadth\tmax_depth\t" + \
    "\t".join(f"d{j}" for j in range(BINS)) + "\n"


@dataclass
class Coverage:
    G: int
    group_of: dict = field(default_factory=dict)     # marker k-mer -> group
    depth: Counter = field(default_factory=Counter)  # marker k-mer -> depth (absent: 0)

    @property
    def markers(self) -> list:
        out = [0] * self.G
        for g in self.group_of.values():
            out[g] += 1
        return out

    def _over_observed(self, fn, start=0) -> list:
        out = [start] * self.G
        for w, d in self.depth.items():
            if d:
                g = self.group_of[w]
                out[g] = fn(out[g], d)
        return out

    @property
    def observed(self) -> list:
        return self._over_observed(lambda a, d: a + 1)

    @property
    def hits(self) -> list:
        return self._over_observed(lambda a, d: a + d)

    @property
    def max_depth(self) -> list:
        return self._over_observed(max)

    @property
    def depth_hist(self) -> list:
        out = [[0] * BINS for _ in range(self.G)]
        for w, g in self.group_of.items():
            out[g][min(self.depth.get(w, 0), BINS - 1)] += 1
        return out

    def records(self) -> np.ndarray:
        """[G, 12] uint64, the layout of speq_marker_cov."""
        cols = [self.markers, self.observed, self.hits, self.max_depth]
        return np.concatenate([np.array(cols, dtype=np.uint64).T.reshape(self.G, 4),
                               np.array(self.depth_hist, dtype=np.uint64).reshape(self.G, BINS)], axis=1)

    def marker_depths(self) -> dict:
        """{marker k-mer: (group, depth)}, depth 0 included: what speq_markers_list holds."""
        return {w: (g, self.depth.get(w, 0)) for w, g in self.group_of.items()}

    def added(self, other: "Coverage") -> "Coverage":
        """The coverage after the reads of `other` are added to this one's (same index)."""
        assert other.group_of == self.group_of
        return Coverage(self.G, self.group_of, self.depth + other.depth)

    def tsv_lines(self, names) -> list:
        """The lines of `speq scan --marker-coverage FILE` after the header, one per group."""
        rec = self.records().tolist()
        out = []
        for g, name in enumerate(names):
            m, o, h, mx = rec[g][:4]
            if m:
                ratios = [f"{o / m:.6f}", f"{h / m:.6f}", f"{1.0 - math.exp(-(h / m)):.6f}"]
            else:
                ratios = ["-"] * 3
            out.append("\t".join([name, str(m), str(o), ratios[0], str(h), ratios[1], ratios[2], str(mx)] +
                                 [str(x) for x in rec[g][4:]]) + "\n")
        return out


def marker_groups(index: dict) -> dict:
    return {w: c[0][0] for w, c in index.items() if len(c) == 1}


def coverage(index: dict, G: int, k: int, seq, qual, offsets, cutoff: int = 30) -> Coverage:
    seq_b = seq.tobytes() if isinstance(seq, np.ndarray) else bytes(seq)
    qual_b = qual.tobytes() if isinstance(qual, np.ndarray) else bytes(qual)
    off = [int(x) for x in offsets]
    s5 = er.dna5(seq_b)
    s_arr = np.frombuffer(s5, dtype=np.uint8)
    q_arr = np.frombuffer(qual_b, dtype=np.uint8)
    cov = Coverage(G, marker_groups(index))
    for r in range(len(off) - 1):
        a, b = off[r], off[r + 1]
        for j in er.passing_windows(s_arr[a:b], q_arr[a:b], k, cutoff).tolist():
            w = s5[a + j:a + j + k]
            if w in cov.group_of:
                cov.depth[w] += 1
    return cov


# ---- the feature's point: equal hits, different breadth ----
def two_samples(records, index: dict, group: int, k: int, n: int = 4096):
    """(copies, spread): two read sets of n reads of k bases, every read one window that is a marker of `group`.
    copies: n times the same read. spread: n distinct markers, one read each. Both as (seq, qual, offsets)."""
    own = []
    seen = set()
    for rec in records:
        fwd = er.dna5(rec)
        for text in (fwd, er.revcomp(fwd)):
            for i in range(len(text) - k + 1):
                w = text[i:i + k]
                c = index.get(w)
                if c is not None and len(c) == 1 and c[0][0] == group and w not in seen:
                    seen.add(w)
                    own.append(w)
                    if len(own) == n:
                        break
            if len(own) == n:
                break
        if len(own) == n:
            break
    assert len(own) == n, "not enough markers"
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(k)
    qual = b"I" * (n * k)
    return (own[0] * n, qual, off), (b"".join(own), qual, off)
