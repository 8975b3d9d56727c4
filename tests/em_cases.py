"""Inputs of the EM-histogram row tests (tests/test_em_reference_cpu.py validates the pure-Python reference on every
one of them; tests/test_gpu_em_rows.py runs the kernels on them). Everything is deterministic and cached per
process: references, read sets, the reference's k-mer dictionaries (a few at a time: they are large), its histogram
of every input set, the oracle's answers and the exact EM steps."""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import numpy as np

import em_reference as er
from oracle.oracle import Oracle
from speq_amd import synth

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
CUTOFF = 30
LOWCX_K = 22  # even: a k-mer can equal its own reverse complement


@dataclass(frozen=True)
class RefSet:
    name: str
    records: tuple
    groups: tuple
    G: int
    counts: tuple            # the "(count)" of each groupings line: any positive integers
    synth_ref: object = None
    marks: object = None     # named k-mers / segments that a test looks up


@dataclass(frozen=True)
class Inputs:
    """One read set: which reference, which generator, read length, paired."""
    ref: str
    kind: str
    read_len: int = 150
    paired: bool = False

    @property
    def id(self) -> str:
        return f"{self.ref}-{self.kind}{self.read_len}{'-pe' if self.paired else ''}"


@dataclass(frozen=True)
class Reads:
    seq: np.ndarray
    qual: np.ndarray
    offsets: np.ndarray
    has_error: Optional[np.ndarray] = None   # deferred: the read differs from its error-free twin (or is random)
    stop_lo: Optional[np.ndarray] = None     # stops: windows with start + k <= stop_lo lie before the stop,
    stop_hi: Optional[np.ndarray] = None     # windows with start >= stop_hi after it

    @property
    def n(self) -> int:
        return len(self.offsets) - 1


def _pack(reads: list, qual_char: bytes = b"I", **kw) -> Reads:
    seq = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return Reads(seq, np.full(seq.size, qual_char[0], dtype=np.uint8), off, **kw)


def _rand_dna(rng, n: int) -> bytes:
    return bytes(rng.choice(ACGT, size=n))


def _counts(G: int) -> tuple:
    return tuple(g % 3 + 1 for g in range(G))


# ---------------------------------------------------------------- references
def _synth_ref(name, V, I, L, n_rate=0.0) -> RefSet:
    r = synth.make_reference(V, I, L, ref_n_rate=n_rate)
    return RefSet(name, tuple(r.records), tuple(r.groups), V, _counts(V), synth_ref=r)


def _lowcx_ref() -> RefSet:
    """Occurrence counts above 1: poly-A stretches of different lengths and a CAG tandem repeat shared by groups 0 and
    1, a k-mer equal to its own reverse complement in a record of each of them (two occurrences per record: one per
    strand), and, in group 2 only, a segment that its records hold twice (count 2, but one group: never a row)."""
    rng = np.random.default_rng(2201)
    k = LOWCX_K
    half = _rand_dna(rng, k // 2)
    pal = half + er.revcomp(half)
    assert pal == er.revcomp(pal)
    shared = _rand_dna(rng, 400)          # in every record: plain multi-group windows
    twice = _rand_dna(rng, 90)            # group 2 only, two copies per record
    recs, groups = [], []
    for g, polya, cag in ((0, 80, 30), (0, 80, 30), (1, 95, 24), (1, 95, 24)):
        recs.append(b"".join([_rand_dna(rng, 200), b"C", b"A" * polya, b"G", _rand_dna(rng, 60), shared, b"CAG" * cag,
                              _rand_dna(rng, 60), pal, _rand_dna(rng, 150)]))
        groups.append(g)
    for _ in range(2):
        recs.append(b"".join([_rand_dna(rng, 150), twice, _rand_dna(rng, 100), shared, _rand_dna(rng, 80), twice,
                              _rand_dna(rng, 150)]))
        groups.append(2)
    return RefSet("lowcx", tuple(recs), tuple(groups), 3, (2, 3, 1), marks={"pal": pal, "twice": twice})


@lru_cache(maxsize=None)
def ref(name: str) -> RefSet:
    if name == "std":
        return _synth_ref(name, 5, 3, 6_000, 0.001)
    if name == "g1":
        return _synth_ref(name, 1, 3, 6_000, 0.001)
    if name == "g2":
        return _synth_ref(name, 2, 3, 6_000, 0.001)
    if name == "g300":
        return _synth_ref(name, 300, 1, 600)
    if name == "lowcx":
        return _lowcx_ref()
    raise KeyError(name)


# ---------------------------------------------------------------- read sets
def _from_synth(r: synth.Reads, **kw) -> Reads:
    return Reads(r.seq, r.qual, r.offsets, **kw)


def _stops(rs: RefSet, L: int) -> Reads:
    """Reads whose run of equal bases in the index's text meets a stop. Chimeric: the tail of one text joined to the
    head of another, directly or over an 'A' (the text codes a separator as A), half of them texts that are
    neighbours in the index (fwd_r | rc_r | fwd_r+1); and reads over a reference N (coded as A too) that hold 'A' or a
    random base there. The stop lies 75..L-76 bases into the read, so windows of up to 70 bases fit on either side."""
    rng = np.random.default_rng(77)
    texts = []
    for rec in rs.records:
        texts += [rec, er.revcomp(rec)]
    reads, lo, hi = [], [], []
    for i in range(300):
        t = int(rng.integers(75, L - 75))
        a = int(rng.integers(len(texts) - 1))
        b = a + 1 if i % 2 else int(rng.integers(len(texts)))
        join = b"A" if i % 4 < 2 else b""
        tail = texts[a][-t:].replace(b"N", b"A")
        head = texts[b][:L - t - len(join)].replace(b"N", b"A")
        reads.append(tail + join + head)
        lo.append(t)
        hi.append(t + len(join))
    n_at = [(ti, p) for ti, tx in enumerate(texts) for p in range(len(tx)) if tx[p] == ord("N")]
    for i in range(300):
        ti, p = n_at[int(rng.integers(len(n_at)))]
        t = int(rng.integers(75, L - 75))
        s0 = p - t
        if s0 < 0 or s0 + L > len(texts[ti]):
            continue
        r = bytearray(texts[ti][s0:s0 + L])
        for x in range(L):
            if r[x] == ord("N"):
                r[x] = ord("A") if i % 2 else int(ACGT[int(rng.integers(4))])
        reads.append(bytes(r))
        lo.append(t)
        hi.append(t + 1)
    return _pack(reads, stop_lo=np.array(lo), stop_hi=np.array(hi))


def _lowcx_reads(rs: RefSet, L: int) -> Reads:
    rng = np.random.default_rng(2202)
    reads = []
    for _ in range(900):
        r = rs.records[int(rng.integers(len(rs.records)))]
        p = int(rng.integers(0, len(r) - L + 1))
        s = r[p:p + L]
        reads.append(er.revcomp(s) if rng.random() < 0.5 else s)
    reads += [b"A" * L, b"T" * L, (b"CAG" * L)[:L], (b"CTG" * L)[:L], b"A" * 60 + b"C" * (L - 60)]
    return _pack(reads)


@lru_cache(maxsize=None)
def reads(inp: Inputs) -> Reads:
    rs, L = ref(inp.ref), inp.read_len
    n = 300 if inp.paired else 600
    if L >= 400:
        n = 150
    if inp.ref == "g300":
        n = 200
    if inp.kind == "mixed":
        return _from_synth(synth.make_reads(rs.synth_ref, n, read_len=L, paired=inp.paired, err_rate=0.004,
                                            n_rate=0.002, lowq_rate=0.01, fragment=max(300, L)))
    if inp.kind == "clean":
        return _from_synth(synth.make_reads(rs.synth_ref, n, read_len=L, paired=inp.paired, err_rate=0.0,
                                            fragment=max(300, L)))
    if inp.kind == "deferred":  # (the mix of test_random_and_error_heavy_reads_overflow_the_deferred_list)
        noisy = synth.make_reads(rs.synth_ref, 640, read_len=L, err_rate=0.03)
        twin = synth.make_reads(rs.synth_ref, 640, read_len=L, err_rate=0.0)
        rnd = np.random.default_rng(5).choice(ACGT, size=160 * L)
        seq = np.concatenate([rnd, noisy.seq])
        err = np.concatenate([np.ones(160, dtype=bool), (noisy.seq != twin.seq).reshape(640, L).any(axis=1)])
        return Reads(seq, np.full(seq.size, ord("I"), dtype=np.uint8), np.arange(0, seq.size + 1, L, dtype=np.uint64),
                     has_error=err)
    if inp.kind == "stops":
        return _stops(rs, L)
    if inp.kind == "lowcx":
        return _lowcx_reads(rs, L)
    if inp.kind == "repeat":  # one error-free read 5,000 times: every add lands on the same intervals
        one = synth.make_reads(rs.synth_ref, 1, read_len=L, err_rate=0.0)
        return _pack([one.seq.tobytes()] * 5_000)
    raise KeyError(inp.kind)


# ---------------------------------------------------------------- cached answers
_INDEX: OrderedDict = OrderedDict()


def index(ref_name: str, k: int) -> dict:
    """The reference's dictionary of (reference, k); the last few are kept (tests are ordered by it)."""
    key = (ref_name, k)
    if key in _INDEX:
        _INDEX.move_to_end(key)
        return _INDEX[key]
    rs = ref(ref_name)
    d = er.build_index(rs.records, rs.groups, rs.G, k)
    _INDEX[key] = d
    while len(_INDEX) > 3:
        _INDEX.popitem(last=False)
    return d


@lru_cache(maxsize=None)
def histogram(inp: Inputs, k: int) -> er.Histogram:
    rs, rd = ref(inp.ref), reads(inp)
    return er.scan(index(inp.ref, k), rs.G, k, rd.seq, rd.qual, rd.offsets, cutoff=CUTOFF, paired=inp.paired)


@lru_cache(maxsize=4)
def oracle(ref_name: str, k: int) -> Oracle:
    rs = ref(ref_name)
    return Oracle(rs.records, rs.groups, rs.G, k)


@lru_cache(maxsize=None)
def oracle_scan(inp: Inputs, k: int, local: bool):
    rd = reads(inp)
    return oracle(inp.ref, k).scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=CUTOFF, paired=inp.paired, local=local)


def percents(G: int) -> dict:
    """The three percentage vectors of every case: uniform, random, and one with zeros (all non-negative, finite)."""
    rnd = np.random.default_rng(1000 + G).uniform(0.0, 50.0, G)
    zeros = rnd.copy()
    zeros[::2] = 0.0
    return {"uniform": np.full(G, 100.0 / G), "random": rnd, "zeros": zeros}


@lru_cache(maxsize=None)
def oracle_em_pass(inp: Inputs, k: int, local: bool, which: str) -> np.ndarray:
    rs, rd = ref(inp.ref), reads(inp)
    return oracle(inp.ref, k).em_pass(rd.seq, rd.qual, rd.offsets, percents(rs.G)[which], rs.counts,
                                      phred_cutoff=CUTOFF, paired=inp.paired, local=local)


@lru_cache(maxsize=None)
def exact_step(inp: Inputs, k: int, which: str) -> tuple:
    rs, h = ref(inp.ref), histogram(inp, k)
    return tuple(er.exact_step(percents(rs.G)[which], rs.counts, h.unique, h.merged))


# ---------------------------------------------------------------- the matrix
AX, KT, LF, FB = "ax", "kt", "lf", "fallback"  # (fallback: default tuning at a k that k_scan_ax does not take)
TUNE = {AX: {}, KT: dict(ax_scan=0), LF: dict(ax_scan=0, kmer_table=0), FB: {}}
KERNEL_CODES = {AX: (3,), KT: (1, 2), LF: (0,), FB: (0,)}  # speq_device_get_tuning("last_kernel")


@dataclass(frozen=True)
class Case:
    inp: Inputs
    k: int
    local: bool
    kernel: str = AX
    tune: tuple = ()          # extra (key, value) tuning pairs

    @property
    def id(self) -> str:
        t = "".join(f"-{a}{b}" for a, b in self.tune)
        return f"{self.inp.id}-k{self.k}-{'local' if self.local else 'global'}-{self.kernel}{t}"


def _matrix() -> list:
    cs = []

    def add(ref_name, kind, k, local, paired=False, kernel=AX, tune=(), read_len=None):
        L = read_len or (200 if k >= 96 else 150)
        cs.append(Case(Inputs(ref_name, kind, L, paired), k, local, kernel, tune))

    # every k of k_scan_ax's compare widths (HW = 1..4: k <= 32, 64, 96, 128) in both modes, single and paired
    for k in (21, 31, 32, 33, 64, 65, 70, 96, 97, 128):
        add("std", "mixed", k, False)
        add("std", "mixed", k, True, paired=True)
    for k in (21, 70):
        add("std", "mixed", k, False, paired=True)
        add("std", "mixed", k, True)
    add("std", "mixed", 21, False, tune=(("ax_sproof", 0),))
    add("std", "mixed", 21, True, paired=True, tune=(("ax_sproof", 0),))
    for kernel, ks in ((KT, (21, 31)), (LF, (21, 70))):
        for k in ks:
            add("std", "mixed", k, False, kernel=kernel)
            add("std", "mixed", k, True, paired=True, kernel=kernel)
    add("std", "mixed", 140, False, kernel=FB)   # k > 128: LF steps
    add("std", "mixed", 140, True, paired=True, kernel=FB)
    # the run-loop site: error-free reads, and reads of more than one chunk / segment
    add("std", "clean", 21, False)
    add("std", "clean", 31, True, paired=True)
    add("std", "clean", 70, False)
    for L in (191, 192, 193):
        add("std", "clean", 21, False, read_len=L)
    add("std", "clean", 70, True, read_len=400)
    add("std", "clean", 21, True, read_len=1000)
    add("std", "clean", 128, False, read_len=1000)
    # the deferred-window site
    for k in (21, 31, 70):
        add("std", "deferred", k, False)
        add("std", "deferred", k, True)
    # stops
    for k in (21, 31, 70):
        add("std", "stops", k, False, read_len=200)
    add("std", "stops", 21, True, read_len=200)
    add("std", "stops", 21, False, kernel=KT, read_len=200)
    add("std", "stops", 21, False, kernel=LF, read_len=200)
    # occurrence counts above 1
    add("lowcx", "lowcx", LOWCX_K, False)
    add("lowcx", "lowcx", LOWCX_K, True)
    add("lowcx", "lowcx", LOWCX_K, False, kernel=KT)
    add("lowcx", "lowcx", LOWCX_K, False, kernel=LF)
    # group-count edges
    add("g1", "mixed", 21, False)
    add("g1", "mixed", 21, True, paired=True)
    add("g2", "mixed", 21, False)
    add("g2", "mixed", 70, True, paired=True)
    add("g300", "mixed", 21, False)
    add("g300", "mixed", 21, True, paired=True)
    # contention and tiny grids
    add("std", "repeat", 21, False)
    add("std", "mixed", 21, False, tune=(("grid_blocks_ax", 1),))
    add("std", "mixed", 70, True, paired=True, tune=(("grid_blocks_ax", 3),))
    return sorted(cs, key=lambda c: (c.inp.ref, c.k, c.inp.id, c.local, c.kernel, c.tune))


CASES = _matrix()
INPUT_SETS = sorted({(c.inp, c.k) for c in CASES}, key=lambda x: (x[0].ref, x[1], x[0].id))
EM_SETS = sorted({(c.inp, c.k, c.local) for c in CASES}, key=lambda x: (x[0].ref, x[1], x[0].id, x[2]))
