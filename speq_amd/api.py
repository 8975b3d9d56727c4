"""Python host mirror of the SPeQ scan path (thin layer over the C ABI in include/speq_scan.h).

Names follow the reference (``/root/reference``):

* :func:`file_to_map`       — ``speq::file_to_map``                      src/file_to_map.cpp:20-119
* :class:`FmIndex`          — ``seqan3::fm_index`` built by ``speq::fm::generate_fm_index``
                              src/fm_indexer.cpp:8-52 (texts [fwd_r, rc_r], :25-33)
* :meth:`DeviceIndex.scan`  — ``search`` + ``do_a_count`` over all reads  src/fm_scanner.cpp:137-236
* :meth:`DeviceIndex.count_unique_kmers_per_group`
                            — ``_async_count_unique_kmers_per_group``     src/fm_scanner.cpp:1476-1576
* :func:`unique_to_percent` — ``speq::scan::unique_to_percent``          src/fm_scanner.cpp:1455-1474

Every compute call runs on the GPU through libspeq_scan.so; nothing here computes counts on the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from ._lib import (MARKER_BINS, SPEQ_MODE_GLOBAL, SPEQ_MODE_LOCAL, BootstrapCI, BuildOpts, IndexInfo,  # noqa: F401
                   DedupStatsRecord, ScanParams, Slot, SpeqError, StreamStats, check, lib)

__all__ = ["FmIndex", "DeviceIndex", "Node", "Pipeline", "ScanResult", "ReadReport", "Markers", "MarkerCoverage", "MarkerTrack", "Bootstrap",
           "Dedup", "DedupStats", "dedup_fingerprint", "bootstrap_summary", "bootstrap_summary_percent", "em_rows_step", "em_rows_refine", "Groupings", "EmHistogram", "Comm", "file_to_map", "unique_to_percent",
           "em_refine", "pack_records", "SpeqError", "SPEQ_MODE_GLOBAL", "SPEQ_MODE_LOCAL"]


def debug_allocs() -> tuple[int, int]:
    """Test seam (dev_mem.cpp): device allocations of the library (alive now, made since the process started)."""
    live, made = C.c_uint64(), C.c_uint64()
    lib().speq_debug_allocs(C.byref(live), C.byref(made))
    return live.value, made.value


def debug_free_queries() -> int:
    """Test seam: free-memory queries the library has made since the process started."""
    made = C.c_uint64()
    lib().speq_debug_free_queries(C.byref(made))
    return made.value


def debug_free_bytes(nth: int, nbytes: int = 0) -> None:
    """Test seam: the nth free-memory query from now answers min(real, nbytes); one-shot, nth 0 disarms."""
    lib().speq_debug_free_bytes(nth, nbytes)


def debug_offset_limit(limit: int = 0) -> None:
    """Test seam: the host's offset decisions take `limit` for 2^32 until it is set again; 0 restores 2^32."""
    lib().speq_debug_offset_limit(limit)


def _u64p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def pack_records(records: Sequence[bytes | str]) -> tuple[bytes, np.ndarray]:
    """Concatenates sequences into one byte buffer + (n+1) u64 offsets."""
    bs = [r.encode() if isinstance(r, str) else bytes(r) for r in records]
    off = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return b"".join(bs), off


def fastq_parse_block(raw1: bytes, raw2: Optional[bytes] = None, n_records: int = 0, pad_byte: int = 0x0A,
                      poison: int = 0, device: int = 0):
    """Test accessor (speq_fastq_parse_block): one run of the GPU FASTQ parser over file 1's text (and file 2's when
    raw2 is not None), n_records per file. Returns (seq, qual, offsets, err, total_bases): seq / qual are all
    len(raw1) + len(raw2) bytes of the output buffers, `poison` wherever the parser wrote nothing."""
    paired = raw2 is not None
    raw = bytes(raw1) + (bytes(raw2) if paired else b"")
    n_slots = n_records * (2 if paired else 1)
    seq = np.empty(len(raw), dtype=np.uint8)
    qual = np.empty(len(raw), dtype=np.uint8)
    off = np.zeros(n_slots + 1, dtype=np.uint64)
    err, total = C.c_uint32(), C.c_uint64()
    check(lib().speq_fastq_parse_block(device, raw, len(raw1), len(raw2) if paired else 0, n_records, int(paired),
                                       pad_byte, poison, seq.ctypes.data, qual.ctypes.data, _u64p(off),
                                       C.byref(err), C.byref(total)))
    return seq, qual, off, err.value, total.value


@dataclass
class Groupings:
    names: list[str]
    scaffolds: list[int]
    counts: list[int]
    errors: str


def file_to_map(path: str) -> Groupings:
    """Parses a genome_groupings file exactly as speq::file_to_map does (file_to_map.cpp:20-119)."""
    L = lib()
    h = C.c_void_p()
    check(L.speq_groupings_parse(path.encode(), C.byref(h)))
    try:
        n = L.speq_groupings_n_groups(h)
        names = [L.speq_groupings_name(h, i).decode() for i in range(n)]
        counts = [int(L.speq_groupings_count(h, i)) for i in range(n)]
        m = L.speq_groupings_n_entries(h)
        p = L.speq_groupings_scaffolds(h)
        scaff = [int(p[i]) for i in range(m)] if m else []
        errs = L.speq_groupings_errors(h).decode()
    finally:
        L.speq_groupings_free(h)
    return Groupings(names, scaff, counts, errs)


def unique_to_percent(unique_in_reads, total_in_reads, unique_in_refs, total_in_refs) -> list[float]:
    """P_i = 100 * u_i / T / (U_ref_i / Tot_ref_i) when Tot_ref_i > 0, else 0 (fm_scanner.cpp:1455-1474)."""
    out = []
    for u, ur, tr in zip(unique_in_reads, unique_in_refs, total_in_refs):
        if float(tr) > 0.0:
            pu = float(ur) / float(tr)
            with np.errstate(all="ignore"):
                out.append(float(np.float64(100.0) * np.float64(u) / np.float64(total_in_reads) / np.float64(pu)))
        else:
            out.append(0.0)
    return out


class FmIndex:
    """Immutable FM-index of the grouped reference collection (host side)."""

    def __init__(self, handle: C.c_void_p, header: bytes = b""):
        self._h = handle
        self.header = header

    @classmethod
    def build(cls, records: Sequence[bytes | str], group_of_record: Sequence[int], n_groups: int,
              prefix_q: int = 0, threads: int = 0, pair_steps: bool = False,
              label_table: bool | str = False, gpu_device: Optional[int] = None,
              triple_steps: bool | str = False) -> "FmIndex":
        """label_table: True/False or "auto" (only for collections of >= 4 M symbols).
        gpu_device: build the suffix array and planes on that GPU (None = host SA-IS); identical results."""
        seq, off = pack_records(records)
        grp = np.asarray(group_of_record, dtype=np.int32)
        h = C.c_void_p()
        opts = BuildOpts(prefix_q, threads, int(pair_steps), 2 if label_table == "auto" else int(bool(label_table)),
                         int(gpu_device is not None),
                         gpu_device if gpu_device is not None else 0,
                         2 if triple_steps == "auto" else int(bool(triple_steps)))
        check(lib().speq_index_build(seq, _u64p(off), len(records), grp.ctypes.data_as(C.POINTER(C.c_int32)),
                                     len(grp), n_groups, C.byref(opts), C.byref(h)))
        return cls(h)

    @classmethod
    def load(cls, path: str) -> "FmIndex":
        h, hdr, hl = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(lib().speq_index_load(path.encode(), C.byref(h), C.byref(hdr), C.byref(hl)))
        header = C.string_at(hdr, hl.value) if hl.value else b""
        lib().speq_free(hdr)
        return cls(h, header)

    def save(self, path: str, header: bytes = b"") -> None:
        check(lib().speq_index_save(self._h, path.encode(), header if header else None, len(header)))

    def info(self) -> IndexInfo:
        info = IndexInfo()
        check(lib().speq_index_get_info(self._h, C.byref(info)))
        return info

    def array(self, name: str, dtype) -> np.ndarray:
        """Copy of a host array of the index (layout: DESIGN.md §3)."""
        p, nb = C.c_void_p(), C.c_uint64()
        check(lib().speq_index_array(self._h, name.encode(), C.byref(p), C.byref(nb)))
        if nb.value == 0:
            return np.zeros(0, dtype=dtype)
        return np.frombuffer(C.string_at(p, nb.value), dtype=dtype).copy()

    def track_layout(self, k: int, bin: int = 100) -> np.ndarray:
        """first_bin[R + 1] of the marker track at scan length k (speq_index_track_layout; host only)."""
        first = np.zeros(self.info().n_records + 1, dtype=np.uint64)
        check(lib().speq_index_track_layout(self._h, k, bin, None, _u64p(first)))
        return first

    def track_loci(self, k: int) -> np.ndarray:
        """Loci per record at scan length k: the bins of width 1."""
        return np.diff(self.track_layout(k, 1))

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().speq_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@dataclass
class ReadReport:
    """Per-unit report (speq_report_reads): one row per read, or per pair."""
    passing: np.ndarray      # passing windows (int64)
    unique: np.ndarray       # windows unique to one group (int64)
    shared: np.ndarray       # passing windows whose k-mer lies in >= 2 groups (int64)
    first_group: np.ndarray  # group of the first unique window, -1 for none (int64)
    sets: np.ndarray         # [n_units, W] uint64: bit g % 64 of word g // 64 <=> a window unique to group g

    def groups(self, unit: int) -> frozenset:
        """The group set of one unit."""
        return _set_groups(self.sets[unit])


def _set_groups(words) -> frozenset:
    return frozenset(64 * w + b for w, x in enumerate(words) for b in range(64) if (int(x) >> b) & 1)


@dataclass
class MarkerCoverage:
    """Per-group marker coverage (speq_markers_finalize): a marker of group g is a distinct k-mer of the texts found
    in g alone, its depth the number of passing read windows equal to it."""
    markers: np.ndarray      # markers of the group (uint64)
    observed: np.ndarray     # markers of depth >= 1 (uint64)
    hits: np.ndarray         # sum of depths: the scan's U[g] (uint64)
    max_depth: np.ndarray    # largest depth (uint64)
    depth_hist: np.ndarray   # [G, 8] uint64: markers of depth exactly j for j < 7, of depth >= 7 for j = 7

    @classmethod
    def from_records(cls, rec: np.ndarray) -> "MarkerCoverage":
        """rec: [G, 12] uint64, the speq_marker_cov records."""
        return cls(rec[:, 0].copy(), rec[:, 1].copy(), rec[:, 2].copy(), rec[:, 3].copy(), rec[:, 4:].copy())

    @property
    def breadth(self) -> np.ndarray:
        """observed / markers (nan for a group without markers)."""
        with np.errstate(all="ignore"):
            return np.where(self.markers > 0, self.observed / np.maximum(self.markers, 1).astype(np.float64), np.nan)

    @property
    def mean_depth(self) -> np.ndarray:
        with np.errstate(all="ignore"):
            return np.where(self.markers > 0, self.hits / np.maximum(self.markers, 1).astype(np.float64), np.nan)

    @property
    def expected_breadth(self) -> np.ndarray:
        """1 - exp(-hits / markers): the breadth that uniform sampling at this depth would give; the figure to hold
        `breadth` against (nan for a group without markers)."""
        return 1.0 - np.exp(-self.mean_depth)


TRACK_DTYPE = np.dtype([("markers", np.uint64), ("observed", np.uint64), ("hits", np.uint64), ("max_depth", np.uint64)])


@dataclass
class MarkerTrack:
    """The marker track (speq_markers_track): per record, bins of `bin` loci (window starts of the forward text), and
    per bin the marker loci, those covered, the sum of their depths and the largest. A locus's depth is its k-mer's
    plus its reverse complement's (once when the two are one k-mer)."""
    first_bin: np.ndarray    # [R + 1] uint64: record r's rows are bins[first_bin[r]:first_bin[r + 1]]
    bins: np.ndarray         # structured (TRACK_DTYPE), one row per bin, record after record
    bin: int
    k: int
    loci: np.ndarray         # [R] uint64: loci of each record, max(len - k + 1, 0)

    @property
    def n_records(self) -> int:
        return len(self.first_bin) - 1

    def record(self, r: int) -> np.ndarray:
        """The rows of record r (none for a record shorter than k)."""
        return self.bins[int(self.first_bin[r]):int(self.first_bin[r + 1])]

    def start(self, r: int, b: int) -> int:
        """First locus of bin b of record r."""
        if not 0 <= b < len(self.record(r)):
            raise IndexError(f"record {r} has no bin {b}")
        return b * self.bin

    def end(self, r: int, b: int) -> int:
        """One past the last locus of bin b of record r."""
        if not 0 <= b < len(self.record(r)):
            raise IndexError(f"record {r} has no bin {b}")
        return min((b + 1) * self.bin, int(self.loci[r]))

    def breadth(self) -> np.ndarray:
        """observed / markers per bin (nan for a bin without marker loci)."""
        m = self.bins["markers"]
        with np.errstate(all="ignore"):
            return np.where(m > 0, self.bins["observed"] / np.maximum(m, 1).astype(np.float64), np.nan)

    def mean_depth(self) -> np.ndarray:
        m = self.bins["markers"]
        with np.errstate(all="ignore"):
            return np.where(m > 0, self.bins["hits"] / np.maximum(m, 1).astype(np.float64), np.nan)


@dataclass
class ScanResult:
    total: int               # T: passing windows
    ambiguous: int           # reads (or pairs) whose counted windows name >= 2 groups
    unique: np.ndarray       # U[g] (u64)
    weights: Optional[np.ndarray]  # W[g] (f64, local mode only)


class DeviceIndex:
    """A replica of an FmIndex in one GPU's HBM."""

    def __init__(self, index: FmIndex, device: int = 0):
        self.index = index
        self.n_groups = index.info().n_groups
        h = C.c_void_p()
        check(lib().speq_device_open(index.handle, device, C.byref(h)))
        self._h = h

    @property
    def handle(self):
        return self._h

    def scan(self, seq: bytes, qual: bytes, offsets: np.ndarray, k: int, phred_cutoff: int = 30,
             paired: bool = False, local: bool = False) -> ScanResult:
        """Scans host reads (staged to HBM in batches)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(off) - 1
        G = self.n_groups
        counts = np.zeros(G + 2, dtype=np.uint64)
        w = np.zeros(G, dtype=np.float64) if local else None
        p = ScanParams(k, phred_cutoff, int(paired), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        check(lib().speq_scan_reads(self._h, seq, qual, _u64p(off), n, C.byref(p), _u64p(counts),
                                    w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None))
        return ScanResult(int(counts[0]), int(counts[1]), counts[2:].copy(), w)

    def scan_device(self, d_seq: int, d_qual: int, d_offsets: int, n_reads: int, k: int, d_counts: int,
                    d_weights: int = 0, phred_cutoff: int = 30, paired: bool = False, local: bool = False,
                    stream: int = 0) -> None:
        """Hot path on HBM-resident buffers (raw device pointers, e.g. torch tensor.data_ptr()).

        `stream` is a raw hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); 0 = the null stream."""
        p = ScanParams(k, phred_cutoff, int(paired), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        check(lib().speq_scan_reads_device(self._h, d_seq, d_qual, d_offsets, n_reads, C.byref(p), d_counts,
                                           d_weights or None, stream or None))

    def report(self, seq: bytes, qual: bytes, offsets: np.ndarray, k: int, phred_cutoff: int = 30,
               paired: bool = False) -> ReadReport:
        """Per-read (or per-pair) report of host reads (speq_report_reads): window counts, the first unique window's
        group and the set of groups the unit's windows are unique to. A diagnostic pass, far slower than scan()."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(off) - 1
        n_units = n // 2 if paired else n
        W = (self.n_groups + 63) // 64
        rec = np.zeros((n_units, 4), dtype=np.uint32)
        sets = np.zeros((n_units, W), dtype=np.uint64)
        p = ScanParams(k, phred_cutoff, int(paired), SPEQ_MODE_GLOBAL)
        check(lib().speq_report_reads(self._h, seq, qual, _u64p(off), n, C.byref(p), rec.ctypes.data, _u64p(sets)))
        first = rec[:, 3].astype(np.int64)
        first[first == 0xFFFFFFFF] = -1
        return ReadReport(rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64), first,
                          sets)

    def report_device(self, d_seq: int, d_qual: int, d_offsets: int, n_reads: int, k: int, d_reports: int,
                      d_sets: int, phred_cutoff: int = 30, paired: bool = False, stream: int = 0) -> None:
        """report() on HBM-resident buffers (raw device pointers, like scan_device): n_units records of four u32
        {passing, unique, shared, first_group (0xFFFFFFFF: none)} at d_reports (16-byte aligned) and n_units * W u64
        set words at d_sets are overwritten, asynchronously on `stream`."""
        p = ScanParams(k, phred_cutoff, int(paired), SPEQ_MODE_GLOBAL)
        check(lib().speq_report_reads_device(self._h, d_seq, d_qual, d_offsets, n_reads, C.byref(p), d_reports, d_sets,
                                             stream or None))

    def report_fastq(self, path1: str, path2: Optional[str] = None, k: int = 21, phred_cutoff: int = 30,
                     threads: int = 4):
        """The report of FASTQ(.gz) file(s) as a summary (speq_report_fastq; paired when path2 is given). Returns
        ({frozenset(groups): units}, totals) with totals = {"units", "passing", "unique", "shared"}; the sets of two or
        more groups are the fusion map."""
        p = ScanParams(k, phred_cutoff, int(path2 is not None), SPEQ_MODE_GLOBAL)
        h = C.c_void_p()
        check(lib().speq_report_fastq(self._h, path1.encode(), path2.encode() if path2 else None, C.byref(p), threads,
                                      C.byref(h), None))
        try:
            W = (self.n_groups + 63) // 64
            words = np.zeros(W, dtype=np.uint64)
            units = C.c_uint64()
            out = {}
            for i in range(lib().speq_group_sets_count(h)):
                check(lib().speq_group_sets_get(h, i, _u64p(words), C.byref(units)))
                out[_set_groups(words)] = units.value
            t = [C.c_uint64() for _ in range(4)]
            check(lib().speq_group_sets_totals(h, *[C.byref(x) for x in t]))
            totals = dict(zip(("units", "passing", "unique", "shared"), (x.value for x in t)))
        finally:
            lib().speq_group_sets_free(h)
        return out, totals

    def marker_coverage(self, seq: bytes, qual: bytes, offsets: np.ndarray, k: int,
                        phred_cutoff: int = 30) -> MarkerCoverage:
        """Marker coverage of host reads (speq_markers_*): one handle, one add, one finalize. A diagnostic pass, far
        slower than scan()."""
        m = Markers(self, k, phred_cutoff)
        try:
            m.add(seq, qual, offsets)
            return m.finalize()
        finally:
            m.close()

    def marker_coverage_fastq(self, path1: str, path2: Optional[str] = None, k: int = 21, phred_cutoff: int = 30,
                              threads: int = 4) -> MarkerCoverage:
        """Marker coverage of FASTQ(.gz) file(s) (speq_markers_fastq; both files' records when path2 is given)."""
        p = ScanParams(k, phred_cutoff, int(path2 is not None), SPEQ_MODE_GLOBAL)
        rec = np.zeros((self.n_groups, 4 + MARKER_BINS), dtype=np.uint64)
        check(lib().speq_markers_fastq(self._h, path1.encode(), path2.encode() if path2 else None, C.byref(p), threads,
                                       rec.ctypes.data, None))
        return MarkerCoverage.from_records(rec)

    def marker_track_fastq(self, path1: str, path2: Optional[str] = None, k: int = 21, phred_cutoff: int = 30,
                           bin: int = 100, threads: int = 4) -> tuple[MarkerCoverage, "MarkerTrack"]:
        """Marker coverage and the marker track of FASTQ(.gz) file(s) from one pass (speq_markers_track_fastq)."""
        p = ScanParams(k, phred_cutoff, int(path2 is not None), SPEQ_MODE_GLOBAL)
        rec = np.zeros((self.n_groups, 4 + MARKER_BINS), dtype=np.uint64)
        first = np.zeros(self.index.info().n_records + 1, dtype=np.uint64)
        rows, n = C.c_void_p(), C.c_uint64()
        check(lib().speq_markers_track_fastq(self._h, path1.encode(), path2.encode() if path2 else None, C.byref(p),
                                             threads, bin, rec.ctypes.data, _u64p(first), C.byref(rows), C.byref(n), None))
        try:
            bins = np.frombuffer(C.string_at(rows, n.value * TRACK_DTYPE.itemsize), dtype=TRACK_DTYPE).copy() \
                if n.value else np.zeros(0, dtype=TRACK_DTYPE)
        finally:
            lib().speq_free(rows)
        return MarkerCoverage.from_records(rec), MarkerTrack(first, bins, bin, k, self.index.track_loci(k))

    def bootstrap(self, seq: bytes, qual: bytes, offsets: np.ndarray, k: int, replicates: int = 200, seed: int = 1,
                  phred_cutoff: int = 30, paired: bool = False, local: bool = False, first_unit: int = 0):
        """The read bootstrap of host reads (speq_bootstrap_*): one handle, one add, one finalize. Returns (counts
        [B + 1, G + 2] u64, weights [B + 1, G] f64 or None); row 0 is the scan's own result. A diagnostic pass, far
        slower than scan()."""
        b = Bootstrap(self, k, replicates, seed, phred_cutoff, paired, local)
        try:
            b.add(seq, qual, offsets, first_unit)
            return b.finalize()
        finally:
            b.close()

    def bootstrap_fastq(self, path1: str, path2: Optional[str] = None, k: int = 21, replicates: int = 200,
                        seed: int = 1, phred_cutoff: int = 30, local: bool = False, threads: int = 4):
        """The read bootstrap of FASTQ(.gz) file(s) (speq_bootstrap_fastq; paired when path2 is given): the same
        (counts, weights) as bootstrap() of the files' records in file order, for any `threads`."""
        G = self.n_groups
        counts = np.zeros((replicates + 1, G + 2), dtype=np.uint64)
        w = np.zeros((replicates + 1, G), dtype=np.float64) if local else None
        p = ScanParams(k, phred_cutoff, int(path2 is not None), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        check(lib().speq_bootstrap_fastq(self._h, path1.encode(), path2.encode() if path2 else None, C.byref(p),
                                         replicates, seed, threads, _u64p(counts),
                                         w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None, None))
        return counts, w

    def bootstrap_em_fastq(self, em: "EmHistogram", path1: str, path2: Optional[str] = None, k: int = 21,
                           replicates: int = 200, seed: int = 1, phred_cutoff: int = 30, local: bool = False,
                           threads: int = 4):
        """bootstrap_fastq with the finalized histogram `em` attached (speq_bootstrap_em_fastq): (counts, weights,
        mult [B + 1, n_rows] u64, missed)."""
        G = self.n_groups
        counts = np.zeros((replicates + 1, G + 2), dtype=np.uint64)
        w = np.zeros((replicates + 1, G), dtype=np.float64) if local else None
        mult = np.zeros((replicates + 1, em.n_rows()), dtype=np.uint64)
        missed = C.c_uint64()
        p = ScanParams(k, phred_cutoff, int(path2 is not None), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        check(lib().speq_bootstrap_em_fastq(self._h, em._h, path1.encode(), path2.encode() if path2 else None,
                                            C.byref(p), replicates, seed, threads, _u64p(counts),
                                            w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None,
                                            _u64p(mult), C.byref(missed), None))
        return counts, w, mult, missed.value

    def dedup_fastq(self, path1: str, path2: Optional[str] = None, k: int = 21, phred_cutoff: int = 30,
                    local: bool = False, threads: int = 4, em: Optional["EmHistogram"] = None):
        """The scan of FASTQ(.gz) file(s) with every distinct read (pair, when path2 is given) counted once
        (speq_dedup_fastq): two passes, fingerprints and then the masked scan. Returns (DedupStats, ScanResult), the
        same for any `threads`; with `em` the scan also fills that histogram."""
        G = self.n_groups
        counts = np.zeros(G + 2, dtype=np.uint64)
        w = np.zeros(G, dtype=np.float64) if local else None
        p = ScanParams(k, phred_cutoff, int(path2 is not None), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        r = DedupStatsRecord()
        check(lib().speq_dedup_fastq(self._h, em._h if em is not None else None, path1.encode(),
                                     path2.encode() if path2 else None, C.byref(p), threads, C.byref(r),
                                     _u64p(counts), w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None,
                                     None))
        return DedupStats.from_record(r), ScanResult(int(counts[0]), int(counts[1]), counts[2:].copy(), w)

    AX_STATS_KEYS = ("wave_iters", "lookup_lanes", "run_lanes", "lookup_waves", "run_waves", "run_windows",
                     "deferred", "filter_pass", "p2_probes", "p2_verify", "chunks", "segments", "qual_bytes",
                     "run_tallied", "run_granules", "refills", "busy_1_4", "busy_5_16", "busy_17_32", "busy_33_64",
                     "cyc_refill", "cyc_lookup", "cyc_run", "cyc_phase2", "cyc_total", "p2_passes",
                     "cyc_p2_filter", "p2_rounds", "cyc_ref_pre", "cyc_ref_stage", "cyc_wave_max", "waves",
                     "cyc_gen0", "cyc_gen1", "cyc_gen2", "cyc_gen3", "cyc_gen4",
                     "sproof_probes", "sproof_windows", "sproof_partial", "stage_slots")

    def scan_device_stats(self, d_seq: int, d_qual: int, d_offsets: int, n_reads: int, k: int, d_counts: int,
                          d_weights: int = 0, phred_cutoff: int = 30, paired: bool = False,
                          local: bool = False) -> dict:
        """scan_device through the instrumented anchor-and-extend kernel (speq_scan_reads_device_stats, synchronous):
        the same counters, plus the kernel's work counts by kind (keys AX_STATS_KEYS)."""
        p = ScanParams(k, phred_cutoff, int(paired), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        st = np.zeros(len(self.AX_STATS_KEYS), dtype=np.uint64)
        check(lib().speq_scan_reads_device_stats(self._h, d_seq, d_qual, d_offsets, n_reads, C.byref(p), d_counts,
                                                 d_weights or None, _u64p(st)))
        return {key: int(v) for key, v in zip(self.AX_STATS_KEYS, st)}

    def scan_fastq(self, path1: str, path2: Optional[str] = None, k: int = 21, phred_cutoff: int = 30,
                   local: bool = False, threads: int = 4, em: Optional["EmHistogram"] = None):
        """Streams FASTQ(.gz) file(s) through pinned slots to the GPU (speq_scan_fastq). Paired when path2 is given.
        Returns (ScanResult, stats dict)."""
        G = self.n_groups
        counts = np.zeros(G + 2, dtype=np.uint64)
        w = np.zeros(G, dtype=np.float64) if local else None
        p = ScanParams(k, phred_cutoff, int(path2 is not None), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        st = StreamStats()
        check(lib().speq_scan_fastq(self._h, path1.encode(), path2.encode() if path2 else None, C.byref(p),
                                    em._h if em is not None else None, threads, _u64p(counts),
                                    w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None,
                                    C.byref(st)))
        stats = {"records": st.records, "bases": st.bases, "batches": st.batches, "seconds": st.seconds}
        return ScanResult(int(counts[0]), int(counts[1]), counts[2:].copy(), w), stats

    def scan_fastq_shard(self, path1: str, path2: Optional[str], k: int, shard: int, n_shards: int, cut: int = 0,
                         phred_cutoff: int = 30, local: bool = False, threads: int = 4,
                         em: Optional["EmHistogram"] = None):
        """One rank's share of a FASTQ scan (speq_scan_fastq_shard): the blocks b % n_shards == shard of the cut every
        rank makes. cut 1 (parallel cut) raises SpeqError with code SPEQ_E_RETRY when the input does not fit it."""
        G = self.n_groups
        counts = np.zeros(G + 2, dtype=np.uint64)
        w = np.zeros(G, dtype=np.float64) if local else None
        p = ScanParams(k, phred_cutoff, int(path2 is not None), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        st = StreamStats()
        check(lib().speq_scan_fastq_shard(self._h, em._h if em is not None else None, path1.encode(),
                                          path2.encode() if path2 else None, C.byref(p), threads, shard, n_shards,
                                          cut, _u64p(counts),
                                          w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None,
                                          C.byref(st)))
        stats = {"records": st.records, "bases": st.bases, "batches": st.batches, "seconds": st.seconds}
        return ScanResult(int(counts[0]), int(counts[1]), counts[2:].copy(), w), stats

    def count_unique_kmers_per_group_shard(self, k: int, shard: int, n_shards: int):
        """This shard's partial (U_ref, Tot_ref) of the .dat pass (speq_ref_unique_shard)."""
        G = self.n_groups
        u = np.zeros(G, dtype=np.uint64)
        t = np.zeros(G, dtype=np.uint64)
        check(lib().speq_ref_unique_shard(self._h, k, shard, n_shards, _u64p(u), _u64p(t)))
        return u, t

    def count_unique_kmers_per_group(self, k: int) -> tuple[np.ndarray, np.ndarray]:
        """(U_ref[G], Tot_ref[G]) of the reference-uniqueness pass."""
        G = self.n_groups
        u = np.zeros(G, dtype=np.uint64)
        t = np.zeros(G, dtype=np.uint64)
        check(lib().speq_ref_unique(self._h, k, _u64p(u), _u64p(t)))
        return u, t

    def tune(self, **kw) -> None:
        """Launch tuning (blocks_per_cu=..., grid_blocks=...); never changes results."""
        for k, v in kw.items():
            check(lib().speq_device_set_tuning(self._h, k.encode(), int(v)))

    def tuning(self, key: str) -> int:
        v = C.c_int64()
        check(lib().speq_device_get_tuning(self._h, key.encode(), C.byref(v)))
        return v.value

    def prepare(self, k: int) -> dict:
        """Builds the k-mer interval table of k now (speq_device_prepare); returns its size and build time."""
        n, b, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        check(lib().speq_device_prepare(self._h, k, C.byref(n), C.byref(b), C.byref(ms)))
        return {"distinct_kmers": n.value, "table_bytes": b.value, "build_ms": ms.value}

    def sproof_bitmap(self, k: int) -> np.ndarray:
        """Test accessor (speq_device_sproof_bitmap): the substitution bitmap S of the prepared k, one bool per text
        position (S[x]: no single-base substitution at x in any of the k windows over x gives an indexed k-mer)."""
        n = int(self.index.info().n)
        words = np.zeros((n + 63) // 64, dtype=np.uint64)
        check(lib().speq_device_sproof_bitmap(self._h, k, _u64p(words), len(words)))
        return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)

    BUILD_FACTS = ("ax", "nb", "nf", "m", "nmf", "s_off", "s_words", "sa_reps", "em_arrays", "distinct", "planes",
                   "ktab", "n", "n_texts")

    def build_facts(self, k: int) -> dict:
        """Test accessor (speq_device_build_facts): what the replica holds for k, building nothing. "ax": 0 not asked
        for, 1 built, 2 deferred (free memory was short), 3 refused; "planes": bit 0 / 1 / 2 the one- / two- /
        three-symbol planes it published; "ktab": 0 not asked for, 1 wide, 2 compact, 3 none."""
        f = np.zeros(len(self.BUILD_FACTS), dtype=np.uint64)
        check(lib().speq_device_build_facts(self._h, k, _u64p(f), len(f)))
        return {name: int(x) for name, x in zip(self.BUILD_FACTS, f)}

    def timing(self, on: bool) -> None:
        check(lib().speq_timing_enable(self._h, int(on)))

    def timing_read(self) -> tuple[float, int]:
        ms, n = C.c_double(), C.c_uint64()
        check(lib().speq_timing_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def close(self):
        if self._h:
            lib().speq_device_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Markers:
    """Depth of every marker of a replica at one k (speq_markers_*): create marks the markers, add / add_device count
    the reads' windows on them, finalize folds the depths per group and may be called again after more adds."""

    def __init__(self, dev: DeviceIndex, k: int, phred_cutoff: int = 30):
        self.dev = dev
        self.n_groups = dev.n_groups
        self.k = k
        p = ScanParams(k, phred_cutoff, 0, SPEQ_MODE_GLOBAL)
        h = C.c_void_p()
        check(lib().speq_markers_create(dev.handle, C.byref(p), C.byref(h)))
        self._h = h

    def add(self, seq: bytes, qual: bytes, offsets: np.ndarray) -> None:
        """Host reads (staged to HBM in batches; synchronous)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        check(lib().speq_markers_add_reads(self._h, seq, qual, _u64p(off), len(off) - 1))

    def add_device(self, d_seq: int, d_qual: int, d_offsets: int, n_reads: int, stream: int = 0) -> None:
        """HBM-resident reads (raw device pointers, like DeviceIndex.scan_device); asynchronous on `stream`."""
        check(lib().speq_markers_add_reads_device(self._h, d_seq, d_qual, d_offsets, n_reads, stream or None))

    def finalize(self) -> MarkerCoverage:
        rec = np.zeros((self.n_groups, 4 + MARKER_BINS), dtype=np.uint64)
        check(lib().speq_markers_finalize(self._h, rec.ctypes.data))
        return MarkerCoverage.from_records(rec)

    def track(self, bin: int = 100) -> MarkerTrack:
        """The marker track of everything added so far (speq_markers_track); the handle stays usable."""
        first = np.zeros(self.dev.index.info().n_records + 1, dtype=np.uint64)
        n = C.c_uint64()
        check(lib().speq_markers_track_layout(self._h, bin, C.byref(n), _u64p(first)))
        bins = np.zeros(n.value, dtype=TRACK_DTYPE)
        if n.value:
            check(lib().speq_markers_track(self._h, bin, bins.ctypes.data))
        return MarkerTrack(first, bins, bin, self.k, self.dev.index.track_loci(self.k))

    def list(self) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Test accessor (speq_markers_list): (lo, group, depth) of every marker, ascending SA position."""
        n = C.c_uint64()
        check(lib().speq_markers_list(self._h, C.byref(n), None, None, None))
        lo, grp, dep = (np.zeros(n.value, dtype=np.uint32) for _ in range(3))
        u32p = C.POINTER(C.c_uint32)
        check(lib().speq_markers_list(self._h, None, lo.ctypes.data_as(u32p), grp.ctypes.data_as(u32p),
                                      dep.ctypes.data_as(u32p)))
        return lo, grp, dep

    def close(self):
        if self._h:
            lib().speq_markers_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bootstrap:
    """B Poisson(1) resamplings of the reads' units in one pass (speq_bootstrap_*): add / add_device accumulate B + 1
    counter vectors on the GPU, each call with the index of its first unit in the input; finalize returns them and
    may be called again after more adds."""

    def __init__(self, dev: DeviceIndex, k: int, replicates: int = 200, seed: int = 1, phred_cutoff: int = 30,
                 paired: bool = False, local: bool = False):
        self.dev = dev
        self.n_groups = dev.n_groups
        self.replicates = replicates
        self.local = local
        p = ScanParams(k, phred_cutoff, int(paired), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        h = C.c_void_p()
        check(lib().speq_bootstrap_create(dev.handle, C.byref(p), replicates, seed, C.byref(h)))
        self._h = h

    def add(self, seq: bytes, qual: bytes, offsets: np.ndarray, first_unit: int = 0) -> None:
        """Host reads (staged to HBM in batches; synchronous); first_unit counts units (pairs of a paired handle)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        check(lib().speq_bootstrap_add_reads(self._h, seq, qual, _u64p(off), len(off) - 1, first_unit))

    def add_device(self, d_seq: int, d_qual: int, d_offsets: int, n_reads: int, first_unit: int = 0,
                   stream: int = 0) -> None:
        """HBM-resident reads (raw device pointers, like DeviceIndex.scan_device); asynchronous on `stream`."""
        check(lib().speq_bootstrap_add_reads_device(self._h, d_seq or None, d_qual or None, d_offsets or None, n_reads,
                                                    first_unit, stream or None))

    def finalize(self):
        """(counts [B + 1, G + 2] u64, weights [B + 1, G] f64 or None) of everything added so far."""
        counts = np.zeros((self.replicates + 1, self.n_groups + 2), dtype=np.uint64)
        w = np.zeros((self.replicates + 1, self.n_groups), dtype=np.float64) if self.local else None
        check(lib().speq_bootstrap_finalize(self._h, _u64p(counts),
                                            w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None))
        return counts, w

    def attach_em(self, em: "EmHistogram") -> None:
        """One EM histogram per replicate (speq_bootstrap_attach_em): before the first add, with the finalized
        histogram of the same replica; the adds then also fill the multiplicities finalize_em returns."""
        check(lib().speq_bootstrap_attach_em(self._h, em._h))

    def em_info(self) -> dict:
        """{"n_rows", "lds_rows" (the most frequent rows, accumulated per block in LDS)}."""
        n, h = C.c_uint64(), C.c_uint32()
        check(lib().speq_bootstrap_em_info(self._h, C.byref(n), C.byref(h)))
        return {"n_rows": n.value, "lds_rows": h.value}

    def finalize_em(self):
        """(mult [B + 1, n_rows] u64 in EmHistogram.rows() order, missed) of everything added so far."""
        n = self.em_info()["n_rows"]
        mult = np.zeros((self.replicates + 1, n), dtype=np.uint64)
        missed = C.c_uint64()
        check(lib().speq_bootstrap_finalize_em(self._h, _u64p(mult), C.byref(missed)))
        return mult, missed.value

    def info(self) -> dict:
        """{"replicates", "lds_path" (the last add accumulated in LDS), "units_added"}."""
        r, l, u = C.c_uint32(), C.c_uint32(), C.c_uint64()
        check(lib().speq_bootstrap_info(self._h, C.byref(r), C.byref(l), C.byref(u)))
        return {"replicates": r.value, "lds_path": bool(l.value), "units_added": u.value}

    def close(self):
        if self._h:
            lib().speq_bootstrap_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bootstrap_summary(counts: np.ndarray, weights: Optional[np.ndarray], u_ref, tot_ref, unique_scale: float = 1.0,
                      level: float = 0.95) -> list[dict]:
    """Per group {"estimate", "mean", "se", "lo", "hi", "used"} of a bootstrap's matrices (speq_bootstrap_summary; host
    only): the percentage of the sample and the spread of the replicates' percentages."""
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    B, G = c.shape[0] - 1, c.shape[1] - 2
    w = np.ascontiguousarray(weights, dtype=np.float64) if weights is not None else None
    ur = np.ascontiguousarray(u_ref, dtype=np.uint64)
    tr = np.ascontiguousarray(tot_ref, dtype=np.uint64)
    out = (BootstrapCI * max(G, 1))()
    check(lib().speq_bootstrap_summary(_u64p(c), w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None, B,
                                       G, _u64p(ur), _u64p(tr), unique_scale, level, out))
    return [{f: getattr(out[g], f) for f in ("estimate", "mean", "se", "lo", "hi", "used")} for g in range(G)]


def bootstrap_summary_percent(percent: np.ndarray, used, estimate=None, level: float = 0.95) -> list[dict]:
    """bootstrap_summary's statistics over a percentage matrix [B + 1, G] (speq_bootstrap_summary_percent; host only):
    used[b] says whether replicate b counts, estimate replaces row 0 as the sample's vector."""
    p = np.ascontiguousarray(percent, dtype=np.float64)
    B, G = p.shape[0] - 1, p.shape[1]
    u = np.ascontiguousarray(used, dtype=np.uint8)
    if u.shape != (B + 1,):
        raise ValueError("used has one entry per row of percent")
    e = np.ascontiguousarray(estimate, dtype=np.float64) if estimate is not None else None
    if e is not None and e.shape != (G,):
        raise ValueError("estimate has one entry per group")
    dp = C.POINTER(C.c_double)
    out = (BootstrapCI * max(G, 1))()
    check(lib().speq_bootstrap_summary_percent(p.ctypes.data_as(dp), e.ctypes.data_as(dp) if e is not None else None,
                                               u.ctypes.data_as(C.POINTER(C.c_uint8)), B, G, level, out))
    return [{f: getattr(out[g], f) for f in ("estimate", "mean", "se", "lo", "hi", "used")} for g in range(G)]


@dataclass
class DedupStats:
    units: int                 # N
    distinct: int              # classes of equal fingerprint
    max_multiplicity: int      # units of the largest class
    mult_hist: np.ndarray      # [8] u64: classes of exactly j + 1 units (j < 7), of 8 or more (j = 7)

    @classmethod
    def from_record(cls, r: DedupStatsRecord) -> "DedupStats":
        return cls(int(r.units), int(r.distinct), int(r.max_multiplicity),
                   np.array(list(r.mult_hist), dtype=np.uint64))

    @property
    def duplicates(self) -> int:
        return self.units - self.distinct


def dedup_fingerprint(seq1: bytes, seq2: Optional[bytes] = None) -> tuple[int, int]:
    """(F_0, F_1) of the unit (seq1, seq2) as the fingerprint kernel computes it (speq_dedup_fingerprint; host only)."""
    out = (C.c_uint64 * 2)()
    s2 = bytes(seq2) if seq2 is not None else None
    lib().speq_dedup_fingerprint(bytes(seq1), len(seq1), s2, len(s2) if s2 is not None else 0, out)
    return int(out[0]), int(out[1])


class Dedup:
    """Duplicate units of the reads (speq_dedup_*): add / add_device fingerprint units on the GPU, each call with the
    index of its first unit in the input; finalize sorts them and marks, per class of equal fingerprint, the lowest
    unit as the one that is kept; mask_device and scan then leave the others out of a scan."""

    def __init__(self, dev: DeviceIndex, paired: bool = False):
        self.dev = dev
        self.n_groups = dev.n_groups
        self.paired = paired
        h = C.c_void_p()
        check(lib().speq_dedup_create(dev.handle, int(paired), C.byref(h)))
        self._h = h

    def add(self, seq: bytes, offsets: np.ndarray, first_unit: int = 0) -> None:
        """Host reads (staged to HBM in batches; synchronous); first_unit counts units (pairs of a paired handle)."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        check(lib().speq_dedup_add_reads(self._h, seq, _u64p(off), len(off) - 1, first_unit))

    def add_device(self, d_seq: int, d_offsets: int, n_reads: int, first_unit: int = 0, stream: int = 0) -> None:
        """HBM-resident reads (raw device pointers, like DeviceIndex.scan_device); asynchronous on `stream`."""
        check(lib().speq_dedup_add_reads_device(self._h, d_seq or None, d_offsets or None, n_reads, first_unit,
                                                stream or None))

    def finalize(self) -> DedupStats:
        """Waits, checks that the units added so far are 0 .. N - 1 each once, and marks the representatives."""
        r = DedupStatsRecord()
        check(lib().speq_dedup_finalize(self._h, C.byref(r)))
        return DedupStats.from_record(r)

    def representatives(self, first_unit: int, n_units: int) -> np.ndarray:
        """rep[first_unit : first_unit + n_units] (u32): the lowest unit of each unit's class."""
        rep = np.zeros(n_units, dtype=np.uint32)
        check(lib().speq_dedup_representatives(self._h, first_unit, n_units,
                                               rep.ctypes.data_as(C.POINTER(C.c_uint32))))
        return rep

    def mask_device(self, d_qual: int, d_offsets: int, n_reads: int, first_unit: int = 0, stream: int = 0) -> None:
        """Writes '!' over the qualities of the records of units that are not kept; asynchronous on `stream`."""
        check(lib().speq_dedup_mask_device(self._h, d_qual or None, d_offsets or None, n_reads, first_unit,
                                           stream or None))

    def scan(self, seq: bytes, qual: bytes, offsets: np.ndarray, k: int, phred_cutoff: int = 30, local: bool = False,
             first_unit: int = 0, em: Optional["EmHistogram"] = None) -> ScanResult:
        """DeviceIndex.scan of the reads with every unit that is not kept left out (speq_dedup_scan_reads); with `em`
        the scan also fills that histogram."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        G = self.n_groups
        counts = np.zeros(G + 2, dtype=np.uint64)
        w = np.zeros(G, dtype=np.float64) if local else None
        p = ScanParams(k, phred_cutoff, int(self.paired), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        check(lib().speq_dedup_scan_reads(self._h, em._h if em is not None else None, seq, qual, _u64p(off),
                                          len(off) - 1, first_unit, C.byref(p), _u64p(counts),
                                          w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None))
        return ScanResult(int(counts[0]), int(counts[1]), counts[2:].copy(), w)

    def close(self):
        if self._h:
            lib().speq_dedup_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """One communicator of a one-process-per-GPU job (speq_comm_* / speq_allreduce_*): RCCL (ncclAllReduce over
    xGMI) or host sockets when ranks share a GPU.

    Replaces the host `future.get()` sums of per-thread count vectors (/root/reference/src/fm_scanner.cpp:224-233):
    every rank scans its own read shard and one all-reduce sums the G + 2 counters (and the G weights). Either rank 0
    makes the 128-byte RCCL id with `Comm.unique_id()` and hands it to the other ranks out of band (bench.py broadcasts
    it with torch.distributed), or `Comm.connect` runs the rendezvous through a file (as `speq scan` does)."""

    ID_BYTES = 128
    AUTO, RCCL, HOST = 0, 1, 2

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(Comm.ID_BYTES)
        check(lib().speq_comm_unique_id(buf))
        return buf.raw

    def __init__(self, nranks: int, rank: int, uid: bytes):
        if len(uid) != Comm.ID_BYTES:
            raise ValueError("the RCCL unique id is 128 bytes")
        h = C.c_void_p()
        check(lib().speq_comm_init(nranks, rank, C.create_string_buffer(uid, Comm.ID_BYTES), C.byref(h)))
        self._h, self.nranks, self.rank = h, nranks, rank

    @classmethod
    def connect(cls, nranks: int, rank: int, rendezvous: str, device: int = -1, transport: int = 0,
                timeout_s: int = 120) -> "Comm":
        """speq_comm_connect: file rendezvous at `rendezvous`; transport AUTO (RCCL when every rank has its own GPU),
        RCCL or HOST (loopback sockets; device may be -1)."""
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(lib().speq_comm_connect(nranks, rank, device, rendezvous.encode(), transport, timeout_s, C.byref(h)))
        self._h, self.nranks, self.rank = h, nranks, rank
        return self

    @property
    def transport(self) -> int:
        return lib().speq_comm_transport(self._h)

    def allreduce_host(self, buf: np.ndarray, device: int = -1) -> None:
        """In-place sum over the ranks of a host u64 or f64 array (speq_allreduce_host)."""
        if buf.dtype not in (np.uint64, np.float64) or not buf.flags.c_contiguous:
            raise TypeError("allreduce_host takes a contiguous uint64 or float64 array")
        check(lib().speq_allreduce_host(self._h, device, buf.ctypes.data, buf.size, int(buf.dtype == np.float64)))

    def allreduce_u64(self, d_buf: int, count: int, stream: int = 0) -> None:
        """In-place sum of `count` u64 at device pointer d_buf, enqueued on `stream` (raw hipStream_t)."""
        check(lib().speq_allreduce_u64(self._h, d_buf, count, stream or None))

    def allreduce_f64(self, d_buf: int, count: int, stream: int = 0) -> None:
        check(lib().speq_allreduce_f64(self._h, d_buf, count, stream or None))

    def close(self):
        if self._h:
            lib().speq_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipeline:
    """Pinned-slot streaming scan (include/speq_scan.h, speq_pipeline_*): fill a slot on the host, submit it, and
    its copy to HBM overlaps the previous slot's kernel."""

    def __init__(self, dev: DeviceIndex, k: int, phred_cutoff: int = 30, paired: bool = False, local: bool = False,
                 slot_bytes: int = 8 << 20, slot_records: int = 1 << 15, n_slots: int = 3,
                 em: Optional["EmHistogram"] = None):
        self.dev, self.local, self.paired = dev, local, paired
        self.n_groups = dev.n_groups
        p = ScanParams(k, phred_cutoff, int(paired), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        h = C.c_void_p()
        check(lib().speq_pipeline_create(dev.handle, C.byref(p), em._h if em is not None else None, slot_bytes,
                                         slot_records, n_slots, C.byref(h)))
        self._h = h

    def put(self, seq: bytes, qual: bytes, offsets: np.ndarray) -> None:
        """Copies whole records into a free slot (growing it if needed) and submits it."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(off) - 1
        nb = int(off[-1] - off[0])
        s = Slot()
        check(lib().speq_pipeline_acquire(self._h, C.byref(s)))
        try:
            if nb > s.cap_bytes or n > s.cap_records:
                check(lib().speq_pipeline_reserve(self._h, C.byref(s), nb, n))
            base = int(off[0])
            C.memmove(s.seq, bytes(seq[base:base + nb]), nb)
            C.memmove(s.qual, bytes(qual[base:base + nb]), nb)
            rel = (off - off[0]).astype(np.uint64)
            C.memmove(s.offsets, rel.ctypes.data, (n + 1) * 8)
        except BaseException:
            lib().speq_pipeline_submit(self._h, s.slot, 0)
            raise
        check(lib().speq_pipeline_submit(self._h, s.slot, n))

    def finish(self) -> ScanResult:
        G = self.n_groups
        counts = np.zeros(G + 2, dtype=np.uint64)
        w = np.zeros(G, dtype=np.float64) if self.local else None
        check(lib().speq_pipeline_finish(self._h, _u64p(counts),
                                         w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None))
        return ScanResult(int(counts[0]), int(counts[1]), counts[2:].copy(), w)

    def close(self):
        if self._h:
            lib().speq_pipeline_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EmHistogram:
    """{multi-group SA interval -> multiplicity} of the passing windows of a read set (include/speq_scan.h, EM).

    Replaces the reference's re-scan of every read in every EM iteration (fm_scanner.cpp:1069-1453): one GPU scan
    fills the histogram, then every iteration is a host sweep over it (step)."""

    def __init__(self, dev: "DeviceIndex"):
        self.dev = dev
        self.n_groups = dev.n_groups
        h = C.c_void_p()
        check(lib().speq_em_create(dev.index.handle, dev.handle, C.byref(h)))
        self._h = h

    def scan(self, seq: bytes, qual: bytes, offsets: np.ndarray, k: int, phred_cutoff: int = 30,
             paired: bool = False, local: bool = False) -> ScanResult:
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        G = self.n_groups
        counts = np.zeros(G + 2, dtype=np.uint64)
        w = np.zeros(G, dtype=np.float64) if local else None
        p = ScanParams(k, phred_cutoff, int(paired), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        check(lib().speq_em_scan_reads(self._h, seq, qual, _u64p(off), len(off) - 1, C.byref(p), _u64p(counts),
                                       w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None))
        return ScanResult(int(counts[0]), int(counts[1]), counts[2:].copy(), w)

    def allreduce(self, comm: "Comm", stream: int = 0) -> None:
        """Sums the unfinalized histogram over the ranks of comm (speq_em_allreduce)."""
        check(lib().speq_em_allreduce(self._h, comm._h, stream or None))

    def finalize(self, threads: int = 0) -> None:
        check(lib().speq_em_finalize(self._h, threads))

    def info(self) -> tuple[int, int, int]:
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(lib().speq_em_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def rows(self) -> list[tuple[int, tuple[tuple[int, int], ...]]]:
        """Test accessor (speq_em_rows): the finalized rows, in order, as (multiplicity, ((group, count), ...))."""
        nr, ne = C.c_uint64(), C.c_uint64()
        check(lib().speq_em_rows(self._h, C.byref(nr), C.byref(ne), None, None, None, None))
        mult = np.zeros(nr.value, dtype=np.uint64)
        ptr = np.zeros(nr.value + 1, dtype=np.uint64)
        grp = np.zeros(ne.value, dtype=np.uint32)
        cnt = np.zeros(ne.value, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        check(lib().speq_em_rows(self._h, None, None, _u64p(mult), _u64p(ptr), grp.ctypes.data_as(u32p),
                                 cnt.ctypes.data_as(u32p)))
        p, g, c = ptr.tolist(), grp.tolist(), cnt.tolist()
        return [(int(mult[r]), tuple(zip(g[p[r]:p[r + 1]], c[p[r]:p[r + 1]]))) for r in range(nr.value)]

    def n_rows(self) -> int:
        nr = C.c_uint64()
        check(lib().speq_em_rows(self._h, C.byref(nr), None, None, None, None, None))
        return nr.value

    def rows_csr(self) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """(row_mult, row_ptr, col_group, col_count) as speq_em_rows returns them: what em_rows_step takes."""
        nr, ne = C.c_uint64(), C.c_uint64()
        check(lib().speq_em_rows(self._h, C.byref(nr), C.byref(ne), None, None, None, None))
        mult = np.zeros(nr.value, dtype=np.uint64)
        ptr = np.zeros(nr.value + 1, dtype=np.uint64)
        grp = np.zeros(ne.value, dtype=np.uint32)
        cnt = np.zeros(ne.value, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        check(lib().speq_em_rows(self._h, None, None, _u64p(mult), _u64p(ptr), grp.ctypes.data_as(u32p),
                                 cnt.ctypes.data_as(u32p)))
        return mult, ptr, grp, cnt

    def intervals(self) -> tuple[np.ndarray, np.ndarray]:
        """Test accessor (speq_em_intervals): (lo, row) of every recorded interval, lo ascending; row indexes
        rows()."""
        n = C.c_uint64()
        check(lib().speq_em_intervals(self._h, C.byref(n), None, None))
        lo, row = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
        u32p = C.POINTER(C.c_uint32)
        check(lib().speq_em_intervals(self._h, None, lo.ctypes.data_as(u32p), row.ctypes.data_as(u32p)))
        return lo, row

    def step(self, percent, group_counts, unique) -> np.ndarray:
        p = np.ascontiguousarray(percent, dtype=np.float64)
        gc = np.ascontiguousarray(group_counts, dtype=np.int32)
        u = np.ascontiguousarray(unique, dtype=np.uint64)
        nxt = np.zeros(self.n_groups, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        check(lib().speq_em_step(self._h, p.ctypes.data_as(dp), gc.ctypes.data_as(C.POINTER(C.c_int32)), _u64p(u),
                                 nxt.ctypes.data_as(dp)))
        return nxt

    def close(self):
        if self._h:
            lib().speq_em_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Node:
    """Replicas of one FmIndex on several GPUs of this process (or logical shards on one GPU): SURVEY.md 8(e).

    Reads shard across the replicas (speq_scan_fastq_multi), the .dat pass splits the reference windows
    (speq_ref_unique_multi), and per-replica EM histograms fold into the first one (speq_em_merge)."""

    def __init__(self, index: FmIndex, devices: Sequence[int]):
        if not devices:
            raise ValueError("Node needs at least one device")
        self.index = index
        self.devices = [DeviceIndex(index, d) for d in devices]
        self.n_groups = self.devices[0].n_groups
        n = len(self.devices)
        self._arr = (C.c_void_p * n)(*[d.handle.value for d in self.devices])

    def __len__(self):
        return len(self.devices)

    def em_histograms(self) -> list["EmHistogram"]:
        return [EmHistogram(d) for d in self.devices]

    def scan_fastq(self, path1: str, path2: Optional[str] = None, k: int = 21, phred_cutoff: int = 30,
                   local: bool = False, threads: int = 4, ems: Optional[Sequence["EmHistogram"]] = None):
        """speq_scan_fastq over every replica; returns (ScanResult, stats dict) of the whole node."""
        G = self.n_groups
        n = len(self.devices)
        counts = np.zeros(G + 2, dtype=np.uint64)
        w = np.zeros(G, dtype=np.float64) if local else None
        p = ScanParams(k, phred_cutoff, int(path2 is not None), SPEQ_MODE_LOCAL if local else SPEQ_MODE_GLOBAL)
        st = StreamStats()
        em_arr = (C.c_void_p * n)(*[e._h.value for e in ems]) if ems is not None else None
        check(lib().speq_scan_fastq_multi(self._arr, em_arr, n, path1.encode(), path2.encode() if path2 else None,
                                          C.byref(p), threads, _u64p(counts),
                                          w.ctypes.data_as(C.POINTER(C.c_double)) if w is not None else None,
                                          C.byref(st)))
        stats = {"records": st.records, "bases": st.bases, "batches": st.batches, "seconds": st.seconds}
        return ScanResult(int(counts[0]), int(counts[1]), counts[2:].copy(), w), stats

    def count_unique_kmers_per_group(self, k: int) -> tuple[np.ndarray, np.ndarray]:
        G = self.n_groups
        u = np.zeros(G, dtype=np.uint64)
        t = np.zeros(G, dtype=np.uint64)
        check(lib().speq_ref_unique_multi(self._arr, len(self.devices), k, _u64p(u), _u64p(t)))
        return u, t

    @staticmethod
    def merge_em(ems: Sequence["EmHistogram"]) -> "EmHistogram":
        """Folds ems[1:] into ems[0] (which is returned; the others accept only close())."""
        for e in ems[1:]:
            check(lib().speq_em_merge(ems[0]._h, e._h))
        return ems[0]

    def close(self):
        for d in self.devices:
            d.close()


def _csr(n_groups: int, row_ptr, col_group, col_count):
    ptr = np.ascontiguousarray(row_ptr, dtype=np.uint64)
    grp = np.ascontiguousarray(col_group, dtype=np.uint32)
    cnt = np.ascontiguousarray(col_count, dtype=np.uint32)
    if ptr.ndim != 1 or len(ptr) < 1 or len(grp) != len(cnt) or (len(ptr) > 0 and int(ptr[-1]) != len(grp)):
        raise ValueError("row_ptr must end at the number of (group, count) entries")
    u32p = C.POINTER(C.c_uint32)
    return ptr, grp, cnt, (n_groups, len(ptr) - 1, _u64p(ptr), grp.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p))


def em_rows_step(n_groups: int, row_ptr, col_group, col_count, mult, percent, group_counts, unique) -> np.ndarray:
    """EmHistogram.step over given CSR rows with the multiplicities `mult` (speq_em_rows_step; host only)."""
    ptr, grp, cnt, args = _csr(n_groups, row_ptr, col_group, col_count)
    m = np.ascontiguousarray(mult, dtype=np.uint64)
    p = np.ascontiguousarray(percent, dtype=np.float64)
    gc = np.ascontiguousarray(group_counts, dtype=np.int32)
    u = np.ascontiguousarray(unique, dtype=np.uint64)
    if m.shape != (len(ptr) - 1,) or p.shape != (n_groups,) or gc.shape != (n_groups,) or u.shape != (n_groups,):
        raise ValueError("mult has one entry per row; percent, group_counts and unique one per group")
    nxt = np.zeros(n_groups, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    check(lib().speq_em_rows_step(*args, _u64p(m), p.ctypes.data_as(dp), gc.ctypes.data_as(C.POINTER(C.c_int32)),
                                  _u64p(u), nxt.ctypes.data_as(dp)))
    return nxt


def em_rows_refine(n_groups: int, row_ptr, col_group, col_count, mult, counts, weights, u_ref, tot_ref, group_counts,
                   unique_scale: float = 1.0, precision: float = 1e-6, max_iterations: int = 1000):
    """The refinement loop for every row of a bootstrap's matrices (speq_em_rows_refine; host only): mult [B + 1,
    n_rows], counts [B + 1, G + 2], weights [B + 1, G] or None. Returns (percent [B + 1, G] f64, iterations [B + 1])."""
    ptr, grp, cnt, args = _csr(n_groups, row_ptr, col_group, col_count)
    G, n_rows = n_groups, len(ptr) - 1
    c = np.ascontiguousarray(counts, dtype=np.uint64)
    B = c.shape[0] - 1
    m = np.ascontiguousarray(mult, dtype=np.uint64)
    w = np.ascontiguousarray(weights, dtype=np.float64) if weights is not None else None
    ur = np.ascontiguousarray(u_ref, dtype=np.uint64)
    tr = np.ascontiguousarray(tot_ref, dtype=np.uint64)
    gc = np.ascontiguousarray(group_counts, dtype=np.int32)
    if c.ndim != 2 or B < 0 or c.shape[1] != G + 2 or m.shape != (B + 1, n_rows) or \
            (w is not None and w.shape != (B + 1, G)) or ur.shape != (G,) or tr.shape != (G,) or gc.shape != (G,):
        raise ValueError("shapes: mult [B + 1, n_rows], counts [B + 1, G + 2], weights [B + 1, G], G-vectors")
    out = np.zeros((B + 1, G), dtype=np.float64)
    its = np.zeros(B + 1, dtype=np.uint32)
    dp = C.POINTER(C.c_double)
    check(lib().speq_em_rows_refine(*args, B, _u64p(m), _u64p(c), w.ctypes.data_as(dp) if w is not None else None,
                                    unique_scale, _u64p(ur), _u64p(tr), gc.ctypes.data_as(C.POINTER(C.c_int32)),
                                    precision, max_iterations, out.ctypes.data_as(dp),
                                    its.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out, its


def em_refine(step, unique_totals, total, percent0, precision: float = 1e-6, max_iterations: int = 1000):
    """The reference's refinement loop (fm_scanner.cpp:248-279): starting from diff = 1.0 per group, while
    max(diff) > precision: next_tkpg = step(percent); percent' = unique_to_percent(unique_totals, total,
    unique_totals, next_tkpg); diff = |percent' - percent|. Returns [(percent', next_tkpg), ...] per iteration."""
    percent = list(percent0)
    out = []
    diff = [1.0] * len(percent)
    while _max_element(diff) > precision and len(out) < max_iterations:
        nxt = step(np.asarray(percent, dtype=np.float64))
        new = unique_to_percent(unique_totals, total, unique_totals, nxt)
        diff = [abs(x - y) for x, y in zip(new, percent)]
        percent = new
        out.append((list(new), [float(x) for x in nxt]))
    return out


def _max_element(v):
    """std::max_element with operator< (NaN never compares greater, so a leading NaN wins)."""
    best = v[0]
    for x in v[1:]:
        if best < x:
            best = x
    return best
