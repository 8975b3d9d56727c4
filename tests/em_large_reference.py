"""The EM histogram of a read set over an index of any size, by numpy from the index's own arrays (no FM search, no
GPU): what tests/test_gpu_em_large.py compares speq_em_finalize with on an index of more than 1,024 tiles.

The suffix array lists the text's suffixes in order, so the rows whose suffix starts with the same valid k-mer (k
symbols of ACGT: a window over a separator or an N does not exist) are one run of rows: the k-mer's SA interval
[lo, hi). The groups of the run's rows, counted, are the interval's (group, count) entries; it is recorded when they
name two groups or more and a passing read window (every base ACGT, every quality above the cutoff) holds the k-mer,
with the number of such windows as its multiplicity. k <= 31: a k-mer is packed into 62 bits."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

SYM_A, SYM_T = 2, 5        # text codes: # $ A C G T N = 0..6
EM_TILE = 4096             # speq_em_finalize: positions per workgroup
SCAN_TILES = 1024          # k_em_scan: tiles per trip of its one workgroup


@dataclass
class Expected:
    n: int                 # text positions
    lo: np.ndarray         # starts of the recorded intervals, ascending
    mult: np.ndarray       # their multiplicities
    ptr: np.ndarray        # CSR over lo: the entries of interval i are [ptr[i], ptr[i + 1])
    grp: np.ndarray        # groups ascending within an interval
    cnt: np.ndarray
    total: int = 0         # passing windows (T)
    unique: np.ndarray = None  # windows whose k-mer lies in one group only (U[g])

    @property
    def info(self):
        return len(self.lo), len(self.grp), int(self.mult.sum())

    def conditions(self):
        """What makes the index worth its size: an interval on either side of k_em_scan's second trip, a tile with no
        interval among those with some, and an interval in n's last, partial tile."""
        tiles = (self.n + EM_TILE - 1) // EM_TILE
        per_tile = np.bincount(self.lo // EM_TILE, minlength=tiles)
        return {"tiles": tiles, "beyond_first_trip": int((self.lo >= SCAN_TILES * EM_TILE).sum()),
                "within_first_trip": int((self.lo < SCAN_TILES * EM_TILE).sum()),
                "empty_tiles": int((per_tile == 0).sum()), "empty_tiles_beyond": int((per_tile[SCAN_TILES:] == 0).sum()),
                "in_last_partial_tile": int(per_tile[-1]) if self.n % EM_TILE else -1}


def _pack(codes2: np.ndarray, k: int) -> np.ndarray:
    """The k-mer starting at every position (the last k - 1 are garbage), two bits per base, first base highest."""
    out = np.zeros(len(codes2), dtype=np.uint64)
    for j in range(k):
        out[:len(codes2) - j] |= codes2[j:].astype(np.uint64) << np.uint64(2 * (k - 1 - j))
    return out


def _valid(bad: np.ndarray, k: int) -> np.ndarray:
    """valid[p]: positions p .. p + k - 1 exist and none is bad."""
    c = np.concatenate([[0], np.cumsum(bad, dtype=np.int64)])
    v = np.zeros(len(bad), dtype=bool)
    if len(bad) >= k:
        v[:len(bad) - k + 1] = c[k:] == c[:-k]
    return v


def expected(text, sa, text_start, text_group, n_groups, k, seq, qual, offsets, cutoff=30) -> Expected:
    assert 1 <= k <= 31
    text = np.asarray(text, dtype=np.uint8)
    sa = np.asarray(sa, dtype=np.int64)
    n = len(text)
    assert len(sa) == n
    acgt = (text >= SYM_A) & (text <= SYM_T)
    key_at = _pack(np.where(acgt, text - SYM_A, 0).astype(np.uint8), k)
    ok_row = _valid(~acgt, k)[sa]
    key_row = key_at[sa]
    rows = np.flatnonzero(ok_row)                       # valid rows, ascending: their k-mers ascend with them
    keys = key_row[rows]
    assert (keys[1:] >= keys[:-1]).all()
    first = np.concatenate([[True], keys[1:] != keys[:-1]])
    run_of = np.cumsum(first) - 1                       # run index of every valid row
    run_lo = rows[first]
    run_key = keys[first]
    n_runs = len(run_lo)
    # a run's rows are adjacent: no other row lies between two suffixes that start with the same k symbols
    run_last = rows[np.concatenate([first[1:], [True]])]
    assert (run_last - run_lo + 1 == np.bincount(run_of, minlength=n_runs)).all()
    ts = np.asarray(text_start, dtype=np.int64)
    grp_row = np.asarray(text_group, dtype=np.int64)[np.searchsorted(ts, sa[rows], side="right") - 1]
    per = np.bincount(run_of * n_groups + grp_row, minlength=n_runs * n_groups).reshape(n_runs, n_groups)
    multi_run = (per > 0).sum(axis=1) >= 2
    # the reads' passing windows
    seq = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)
    qual = np.frombuffer(qual, dtype=np.uint8) if isinstance(qual, (bytes, bytearray)) else np.asarray(qual, np.uint8)
    code = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        code[ch] = i
        code[ch + 32] = i
    code[ord("U")] = code[ord("u")] = 3
    c = code[seq]
    q = np.clip(qual.astype(np.int32) - 33, 0, 41)
    bad = (c == 4) | (q <= cutoff)
    passing = _valid(bad, k)
    off = np.asarray(offsets, dtype=np.int64)
    inside = np.zeros(len(seq), dtype=bool)             # the window must end within its read
    for a, b in zip(off[:-1].tolist(), off[1:].tolist()):
        if b - a >= k:
            inside[a:b - k + 1] = True
    wkeys = _pack(np.where(c == 4, 0, c).astype(np.uint8), k)[passing & inside]
    at = np.searchsorted(run_key, wkeys)
    hit = (at < n_runs) & (run_key[np.minimum(at, n_runs - 1)] == wkeys)
    m_run = np.bincount(at[hit], minlength=n_runs)
    single = np.flatnonzero(~multi_run)
    unique = np.bincount(per[single].argmax(axis=1), weights=m_run[single], minlength=n_groups).astype(np.int64)
    rec = np.flatnonzero(multi_run & (m_run > 0))
    sub = per[rec]
    g_idx = np.nonzero(sub)
    ptr = np.concatenate([[0], np.cumsum((sub > 0).sum(axis=1))])
    return Expected(n, run_lo[rec].astype(np.int64), m_run[rec].astype(np.int64), ptr.astype(np.int64),
                    g_idx[1].astype(np.int64), sub[g_idx].astype(np.int64), int(len(wkeys)), unique)


# ---------------------------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_em_large.py (checked without a GPU by tests/test_em_large_reference_cpu.py)
# ---------------------------------------------------------------------------------------------------------------
LARGE_K = 21
LARGE_G = 2
LARGE_LEN = 530_000        # 4 records and their reverse complements, a separator each, the terminator: n = 4,240,009
POLY_AT, POLY_LEN = 100_000, 12_000


@lru_cache(maxsize=None)
def large_inputs():
    """(reference, index, reads, Expected): 2 variants x 2 isolates of 530,000 bases, n = 4,240,009 text positions in
    1,036 tiles of 4,096, so k_em_scan's one workgroup makes a second trip for the last 12. Both isolates of variant 0
    hold 12,000 C in a row: the interval of C^21 (and of G^21, the other strand) spans several whole tiles and belongs
    to one group, so those tiles record nothing. 4,000 reads of 150 bases with 0.3 % errors."""
    from speq_amd import FmIndex, synth
    ref = synth.make_reference(LARGE_G, 2, LARGE_LEN)
    records = list(ref.records)
    for r in (0, 1):  # variant 0's isolates
        assert ref.groups[r] == 0
        records[r] = records[r][:POLY_AT] + b"C" * POLY_LEN + records[r][POLY_AT + POLY_LEN:]
    ref = synth.Reference(records, list(ref.groups), LARGE_G, 2, LARGE_LEN)
    idx = FmIndex.build(ref.records, ref.groups, LARGE_G, prefix_q=10, pair_steps=True, triple_steps=True,
                        label_table=True)
    reads = synth.make_reads(ref, 4_000, read_len=150, err_rate=0.003)
    exp = expected(idx.array("text", np.uint8), idx.array("sa", np.uint32), idx.array("text_start", np.uint64),
                   idx.array("text_group", np.int32), LARGE_G, LARGE_K, reads.seq, reads.qual, reads.offsets)
    return ref, idx, reads, exp
