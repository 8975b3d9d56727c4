"""Exact pure-Python model of the marker track (speq_markers_track): no GPU, no C.

Built on marker_model.Coverage (marker status from the group sets of em_reference.build_index's dictionary, depths from
the reads through the scan's filter). A locus (r, p) is a window start p of the forward text of record r,
0 <= p < max(len - k + 1, 0); it is a marker locus when its k-mer x holds no N and is a marker. Its depth is
depth(x) + depth(rc(x)), or depth(x) alone when x is its own reverse complement. The depth belongs to the k-mer: every
locus of a repeated marker carries it in full. Record r has ceil(loci / bin) bins; per bin: marker loci, those of depth
>= 1, the sum of depths, the largest depth.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import em_reference as er
import marker_model as mm

DTYPE = np.dtype([("markers", np.uint64), ("observed", np.uint64), ("hits", np.uint64), ("max_depth", np.uint64)])
HEADER = "record\tgroup\tstart\tend\tmarkers\tobserved\tbreadth\thits\tmean_depth\tmax_depth\n"


def loci_of(records, k: int) -> list:
    return [max(len(r) - k + 1, 0) for r in records]


def layout(records, k: int, bin: int) -> np.ndarray:
    """first_bin[R + 1]"""
    first = np.zeros(len(records) + 1, dtype=np.uint64)
    first[1:] = np.cumsum([-(-n // bin) for n in loci_of(records, k)])
    return first


def locus_depths(records, groups, k: int, cov: mm.Coverage) -> list:
    """Per record, per locus: None (no marker there) or the locus depth."""
    out = []
    for rec, g in zip(records, groups):
        fwd = er.dna5(rec)
        row = []
        for p in range(max(len(fwd) - k + 1, 0)):
            x = fwd[p:p + k]
            if b"N" in x or x not in cov.group_of:
                row.append(None)
                continue
            assert cov.group_of[x] == g, "a marker lies in texts of its own group only"
            rc = er.revcomp(x)
            assert rc in cov.group_of, "marker status is symmetric under reverse complement"
            row.append(cov.depth.get(x, 0) + (cov.depth.get(rc, 0) if rc != x else 0))
        out.append(row)
    return out


@dataclass
class Track:
    first_bin: np.ndarray
    bins: np.ndarray  # DTYPE
    bin: int
    k: int
    loci: list

    def record(self, r: int) -> np.ndarray:
        return self.bins[int(self.first_bin[r]):int(self.first_bin[r + 1])]

    def group_hits(self, groups, G: int) -> list:
        out = [0] * G
        for r, g in enumerate(groups):
            out[g] += int(self.record(r)["hits"].sum())
        return out

    def tsv_lines(self, groups, names) -> list:
        """The lines of `speq scan --marker-track FILE` after the header."""
        out = []
        for r, g in enumerate(groups):
            for b, row in enumerate(self.record(r).tolist()):
                m, o, h, mx = row
                ratios = [f"{o / m:.6f}", f"{h / m:.6f}"] if m else ["-", "-"]
                out.append("\t".join([str(r), names[g], str(b * self.bin), str(min((b + 1) * self.bin, self.loci[r])),
                                      str(m), str(o), ratios[0], str(h), ratios[1], str(mx)]) + "\n")
        return out


def track(records, groups, k: int, cov: mm.Coverage, bin: int) -> Track:
    first = layout(records, k, bin)
    bins = np.zeros(int(first[-1]), dtype=DTYPE)
    for r, row in enumerate(locus_depths(records, groups, k, cov)):
        for p, d in enumerate(row):
            if d is None:
                continue
            i = int(first[r]) + p // bin
            bins["markers"][i] += np.uint64(1)
            if d:
                bins["observed"][i] += np.uint64(1)
                bins["hits"][i] += np.uint64(d)
                bins["max_depth"][i] = max(int(bins["max_depth"][i]), d)
    return Track(first, bins, bin, k, loci_of(records, k))


def model(records, groups, G: int, k: int, reads, bin: int, cutoff: int = 30):
    """(Coverage, Track) of the reads (seq, qual, offsets)."""
    cov = mm.coverage(er.build_index(records, groups, G, k), G, k, *reads, cutoff)
    return cov, track(records, groups, k, cov, bin)
