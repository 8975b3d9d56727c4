"""Inputs and reference answers of the scans past the anchor kernel's k (tests/test_big_k_cpu.py validates them against
the oracle without a GPU, tests/test_gpu_big_k.py runs them).

Above k = 128 (AX_MAX_K) every scan is k_scan with LF steps. KS holds the first k past the anchor kernel (129), the
three residues of the one/two/three-symbol leftover step (129, 130, 131), the edges of the 64-bit bad-mask words that
a window spans (192, 193, 257), both sides of the report's limit (1024, 1025) and MAX_K (4096).

`reference(k)`: three 12,000-base variants, a record holding two N (a piece of variant 2 filed under group 1, so its
N-free windows lie in two groups) and contigs of k - 1, k and k + 1 bases, each a piece of one variant filed under
another group (no window; one and two windows that two groups share). Everything a test names "the fragmented
reference" is this list: frag_refs.fragmented cuts 4,000-base genomes into contigs of at most 700 bases, so past
k = 700 it holds no window at all.

`reads(k)`, in this order (the order matters: with tuning "grid_blocks" 1 a scan is four waves that take a quarter of
the units each, so the first and the last 71 reads sit in one wave):
  70 reads of exactly k bases (one window each: more reads with a window than a wave has lanes, while the staging
     buffer of 2 (64 * 2 + k) bytes admits two or three of them per pass);
  synthetic reads of k + 400 bases with substitution errors, N bases and low qualities, the other qualities 31..41;
  reads of 0, k - 1, k, k + 1, k + 63, k + 64, k + 65 and 2k + 130 bases;
  one read of 3 (64 * 2 + k) bases (several passes);
  an N, and a quality equal to the cutoff, at positions 63, 64, k - 1, k and k + 63 of a 2k + 130 read;
  chimeras of two groups and their reverse complements; pairs whose mates name different groups;
  70 reads of k - 1 bases (the kernel's "the next 64 reads hold no window" skip), then one read that has windows.
The count is even and the same records serve as pairs (2i, 2i + 1).

The replicas of more than three groups hold the same records under other labels (group g becomes LABELS[G][g]), so
their answers are the three-group oracle's with U and W moved to those labels: the labels are names, nothing else
(test_big_k_cpu.py checks one relabelled oracle outright)."""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

import numpy as np

import em_reference as er
from oracle.oracle import Oracle
from speq_amd import synth

KS = [129, 130, 131, 192, 193, 257, 1024, 1025, 4096]
K_EM = [129, 1024, 4096]            # EM rows and the index variants
CUTOFF = 30
LENGTH = 12_000
N_SYNTH = 120
RUN = 70                            # consecutive reads of k, and of k - 1, bases
GOOD = ord("I")                     # Phred 40
LABELS = {3: (0, 1, 2), 2048: (0, 1024, 2047), 2049: (0, 1024, 2048)}   # the LDS tally's last G; the first past it

# (k, phred_cutoff, the quality whose window weight overflows, the next one, which stays finite): the weight of a
# window of k bases of quality q is (1 - 10^(-q/10))^-k. q = 3: 2.0047^1024 > 2^1027; q = 4: 1.6610^1024 = 5.9e225.
# q = 7: 1.2494^4096 = e^912; q = 8: 1.1883^4096 = e^706.7 = 8e306 (DBL_MAX = e^709.78). test_big_k_cpu.py confirms
# both pairs with the oracle.
OVERFLOW = [(1024, 2, 3, 4), (4096, 6, 7, 8)]


class Reads(NamedTuple):
    seq: np.ndarray
    qual: np.ndarray
    offsets: np.ndarray

    @property
    def n(self) -> int:
        return len(self.offsets) - 1

    def prefix(self, n: int) -> "Reads":
        end = int(self.offsets[n])
        return Reads(self.seq[:end], self.qual[:end], self.offsets[:n + 1])


def pack(seqs, quals) -> Reads:
    assert all(len(s) == len(q) for s, q in zip(seqs, quals))
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return Reads(np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(),
                 np.frombuffer(b"".join(quals), dtype=np.uint8).copy(), off)


@lru_cache(maxsize=None)
def base_ref() -> synth.Reference:
    return synth.make_reference(3, 1, LENGTH)


class Ref(NamedTuple):
    records: tuple
    groups: tuple       # labels 0..2


@lru_cache(maxsize=None)
def reference(k: int) -> Ref:
    v = base_ref().records
    with_n = bytearray(v[2][500:500 + 2 * k + 300])
    with_n[k + 10] = with_n[k + 150] = ord("N")
    records = list(v) + [bytes(with_n), v[0][100:100 + k - 1], v[1][200:200 + k], v[2][300:300 + k + 1]]
    return Ref(tuple(records), (0, 1, 2, 1, 1, 2, 0))


def groups_of(k: int, G: int) -> list:
    return [LABELS[G][g] for g in reference(k).groups]


def groupings_text(k: int) -> str:
    """The reference's groups as a genome_groupings file."""
    gs = reference(k).groups
    return "".join(f"V{g}({g + 1}): {', '.join(str(i) for i, x in enumerate(gs) if x == g)}\n" for g in range(3))


def fasta_text(k: int) -> str:
    out = []
    for i, s in enumerate(reference(k).records):
        out.append(f">rec{i}")
        out += [s[p:p + 80].decode() for p in range(0, len(s), 80)]
    return "\n".join(out) + "\n"


def private_start(rec: int, k: int, length: int, first: bool, lo: int) -> int:
    """A start a >= lo such that the first (or last) k-window of variant rec's [a, a + length) differs from both other
    variants at the same coordinates."""
    v = base_ref().records
    for a in range(lo, LENGTH - length, 50):
        w0 = a if first else a + length - k
        if all(v[o][w0:w0 + k] != v[rec][w0:w0 + k] for o in range(3) if o != rec):
            return a
    raise AssertionError("no private window")


def chimera(k: int, a_rec: int, b_rec: int, lo: int) -> bytes:
    """Variant a_rec joined to variant b_rec at the same coordinate: the first window names a_rec's group alone, the
    last b_rec's."""
    v = base_ref().records
    H = k + 40
    for a in range(lo, LENGTH - 2 * H, 50):
        if a == private_start(a_rec, k, H, True, a) and a + H == private_start(b_rec, k, H, False, a + H):
            return v[a_rec][a:a + H] + v[b_rec][a + H:a + 2 * H]
    raise AssertionError("no chimera")


def _synthetic(k: int):
    """N_SYNTH reads of k + 400 bases: about half of the windows hold an N or a quality of 10 (both at 0.35 / k per
    base) and about a quarter of the rest an error; the other qualities are 31..41, so the weights of the windows
    differ."""
    rd = synth.make_reads(base_ref(), N_SYNTH, read_len=k + 400, err_rate=0.3 / k, n_rate=0.35 / k, lowq_rate=0.35 / k)
    q = rd.qual.copy()
    keep = q == GOOD
    q[keep] = (33 + 31 + (synth.rand_u64(0xB16 + k, 0, q.size) % np.uint64(11)).astype(np.uint8))[keep]
    off = [int(x) for x in rd.offsets]
    return ([rd.seq[a:b].tobytes() for a, b in zip(off, off[1:])], [q[a:b].tobytes() for a, b in zip(off, off[1:])])


@lru_cache(maxsize=None)
def read_list(k: int):
    v = base_ref().records
    seqs, quals = [], []

    def add(s: bytes, q: bytes = None):
        seqs.append(bytes(s))
        quals.append(bytes([GOOD]) * len(s) if q is None else bytes(q))

    for i in range(RUN):
        add(v[i % 3][50 * i:50 * i + k])
    s, q = _synthetic(k)
    seqs += s
    quals += q
    for i, L in enumerate([0, k - 1, k, k + 1, k + 63, k + 64, k + 65, 2 * k + 130]):
        add(v[1][200 + 37 * i:200 + 37 * i + L])
    n_long = 3 * (64 * 2 + k)
    add((v[1] + er.revcomp(v[2]))[500:500 + n_long])
    long = v[1][3_000:3_000 + 2 * k + 130]
    for pos in (63, 64, k - 1, k, k + 63):
        s = bytearray(long)
        s[pos] = ord("N")
        add(s)
        q = bytearray([GOOD]) * len(long)
        q[pos] = 33 + CUTOFF
        add(long, q)
    for a_rec, b_rec, lo in ((0, 2, 100), (1, 0, 1_000), (2, 1, 2_000)):
        c = chimera(k, a_rec, b_rec, lo)
        add(c)
        add(er.revcomp(c))
    if len(seqs) % 2:
        add(b"")
    L = k + 20
    for a_rec, b_rec, lo in ((0, 1, 4_000), (2, 0, 5_000), (1, 2, 6_000)):
        a0, a1 = private_start(a_rec, k, L, True, lo), private_start(b_rec, k, L, True, lo + 500)
        add(v[a_rec][a0:a0 + L])
        add(er.revcomp(v[b_rec][a1:a1 + L]))
    if len(seqs) % 2 == 0:
        add(b"")            # (the run below and its last read are 71 records)
    for i in range(RUN):
        add(v[(i + 1) % 3][60 * i:60 * i + k - 1])
    add(v[2][7_000:7_000 + k + 100])
    assert len(seqs) % 2 == 0
    return seqs, quals


@lru_cache(maxsize=None)
def reads(k: int) -> Reads:
    return pack(*read_list(k))


def overflow_reads(k: int, q: int) -> Reads:
    """One error-free read of k + 2 bases per group (three windows that name it alone), every quality q."""
    v = base_ref().records
    seqs = [v[g][a:a + k + 2] for g in range(3) for a in [private_start(g, k, k + 2, True, 1_000 + 2_000 * g)]]
    seqs[1] = er.revcomp(seqs[1])
    return pack(seqs, [bytes([33 + q]) * len(s) for s in seqs])


# ---------------------------------------------------------------- reference answers
_ORACLE: dict = {}


def oracle(k: int) -> Oracle:
    """The three-group oracle of k; one at a time (callers go k by k)."""
    if k not in _ORACLE:
        _ORACLE.clear()
        r = reference(k)
        _ORACLE[k] = Oracle(r.records, r.groups, 3, k)
    return _ORACLE[k]


@lru_cache(maxsize=None)
def oracle_scan3(k: int, paired: bool, local: bool, n_reads: int = -1):
    rd = reads(k) if n_reads < 0 else reads(k).prefix(n_reads)
    return oracle(k).scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=CUTOFF, paired=paired, local=local)


def relabel(x: np.ndarray, G: int) -> np.ndarray:
    out = np.zeros(G, dtype=x.dtype)
    out[list(LABELS[G])] = x
    return out


def oracle_scan(k: int, G: int, paired: bool, local: bool, n_reads: int = -1):
    """(T, ambiguous, U[G], W[G] or None) of the C oracle under the labels of a G-group replica."""
    T, amb, U, W = oracle_scan3(k, paired, local, n_reads)
    return T, amb, relabel(U, G), relabel(W, G) if W is not None else None


@lru_cache(maxsize=None)
def ref_unique3(k: int):
    return oracle(k).ref_unique()


def ref_unique(k: int, G: int):
    u, t = ref_unique3(k)
    return relabel(u, G), relabel(t, G)


@lru_cache(maxsize=None)
def windows(k: int) -> int:
    """Windows of reads(k), passing or not."""
    lens = np.diff(reads(k).offsets).astype(np.int64)
    return int(np.maximum(lens - k + 1, 0).sum())


_HIST: dict = {}


def histogram(k: int, paired: bool) -> er.Histogram:
    """The exact EM histogram of reads(k) (tests/em_reference.py); the dictionary of one k at a time."""
    if ("index", k) not in _HIST:
        _HIST.clear()
        r = reference(k)
        _HIST[("index", k)] = er.build_index(r.records, r.groups, 3, k)
    if (k, paired) not in _HIST:
        rd = reads(k)
        _HIST[(k, paired)] = er.scan(_HIST[("index", k)], 3, k, rd.seq, rd.qual, rd.offsets, cutoff=CUTOFF,
                                     paired=paired)
    return _HIST[(k, paired)]
