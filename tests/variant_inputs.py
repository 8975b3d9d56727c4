"""Inputs and reference answers of the scan-kernel ledger (tests/variant_table.py, tests/test_gpu_variants.py).

Two references, the smallest shapes at which the instantiations can still go wrong: "g5" (5 groups of 2 records, some
reference N) for the LDS tally and "g2049" (2049 groups of one 220-base record) for the global-atomic tally, one group
past the threshold. Per (reference, paired, read length) one read set of 336 units, more than one wave of the anchor
kernel so that lanes refill:

  256 units of synth.make_reads with substitution errors, N bases and low-quality bases;
   64 chimeric units: a single read is the first half of one group's record joined to the second half of another
      group's at the same coordinates (the windows over the join exist in the texts wherever the two records agree),
      a pair has its mates from two groups. The records of "g2049" differ in 1 % of their bases and share most of
      those with some other group, so plain reads of it almost never name two groups; these do;
   16 error-free units from the last 16 records (the highest groups: the far end of the tally).

What the references alone must find on every set (asserted without a GPU by tests/test_variant_table_cpu.py, so that
no instantiation is compared on counters that are all zero): >= 2 ambiguous units, >= min(64, G) groups with U[g] > 0,
on "g2049" one of them among the last 64 groups, and >= 100 multi-group histogram rows.

Everything is deterministic and cached per process; the answers come from the C oracle (oracle/kmer_oracle.c) and the
pure-Python references (tests/em_reference.py, tests/read_report_model.py), never from the library under test."""
from __future__ import annotations

from functools import lru_cache
from typing import NamedTuple

import numpy as np

import em_reference as er
import read_report_model as rm
import variant_table as vt
from oracle.oracle import Oracle
from speq_amd import synth

CUTOFF = 30
N_PLAIN, N_CHIMERIC, N_CLEAN = 256, 64, 16
SEED = 20


class Reads(NamedTuple):
    seq: np.ndarray
    qual: np.ndarray
    offsets: np.ndarray

    @property
    def n(self) -> int:
        return len(self.offsets) - 1


@lru_cache(maxsize=None)
def ref(name: str) -> synth.Reference:
    s = vt.REFS[name]
    return synth.make_reference(s.n_variants, s.n_isolates, s.length, ref_n_rate=s.ref_n_rate)


def counts(name: str) -> tuple:
    """The "(count)" of each groupings line (what an EM step divides by): any positive integers."""
    return tuple(g % 3 + 1 for g in range(vt.REFS[name].G))


@lru_cache(maxsize=None)
def reads(name: str, paired: bool, read_len: int) -> Reads:
    r = ref(name)
    L, Lrec, nrec = read_len, r.length, len(r.records)
    plain = synth.make_reads(r, N_PLAIN, read_len=L, paired=paired, err_rate=0.004, n_rate=0.002, lowq_rate=0.01,
                             fragment=min(300, Lrec))
    rng = np.random.default_rng(SEED + 2 * L + int(paired))
    extra = []
    for _ in range(N_CHIMERIC):
        a = int(rng.integers(nrec))
        b = int(rng.integers(nrec))
        while r.groups[b] == r.groups[a]:
            b = int(rng.integers(nrec))
        p = int(rng.integers(0, Lrec - L + 1))
        flip = bool(rng.integers(2))
        if paired:
            q = int(rng.integers(0, Lrec - L + 1))
            extra += [r.records[a][p:p + L], er.revcomp(r.records[b][q:q + L])]
        else:
            s = r.records[a][p:p + L // 2] + r.records[b][p + L // 2:p + L]
            extra.append(er.revcomp(s) if flip else s)
    for i in range(N_CLEAN):
        rec = r.records[nrec - 1 - i % min(16, nrec)]
        p = int(rng.integers(0, Lrec - L + 1))
        if paired:
            q = int(rng.integers(0, Lrec - L + 1))
            extra += [rec[p:p + L], er.revcomp(rec[q:q + L])]
        else:
            extra.append(rec[p:p + L])
    assert all(len(s) == L for s in extra)
    seq = np.concatenate([plain.seq, np.frombuffer(b"".join(extra), dtype=np.uint8)])
    qual = np.concatenate([plain.qual, np.full(len(extra) * L, ord("I"), dtype=np.uint8)])
    return Reads(seq, qual, np.arange(0, seq.size + 1, L, dtype=np.uint64))


def reads_of(name: str, k: int, paired: bool) -> Reads:
    return reads(name, paired, vt.read_len(k))


# ---------------------------------------------------------------- reference answers
@lru_cache(maxsize=None)
def oracle(name: str, k: int) -> Oracle:
    r = ref(name)
    return Oracle(r.records, r.groups, vt.REFS[name].G, k)


@lru_cache(maxsize=None)
def oracle_scan(name: str, k: int, paired: bool, local: bool):
    """(T, ambiguous, U, W or None) of the C oracle."""
    rd = reads_of(name, k, paired)
    return oracle(name, k).scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=CUTOFF, paired=paired, local=local)


@lru_cache(maxsize=None)
def ref_unique(name: str, k: int):
    return oracle(name, k).ref_unique()


_INDEX: dict = {}


def index(name: str, k: int) -> dict:
    """em_reference's dictionary of (reference, k); one at a time (callers go k by k)."""
    if (name, k) not in _INDEX:
        _INDEX.clear()
        r = ref(name)
        _INDEX[(name, k)] = er.build_index(r.records, r.groups, vt.REFS[name].G, k)
    return _INDEX[(name, k)]


class Rows(NamedTuple):
    """The EM histogram a scan must leave, in the form the comparison takes: a row is its (group, count) entries as
    the bytes of two u32 arrays."""
    info: tuple          # (n_intervals, n_entries, n_windows)
    unmerged: dict       # {(row, multiplicity): how many such rows}
    merged: dict         # {row: multiplicity}
    exact: er.Histogram


def row_key(groups, cnts) -> bytes:
    return np.asarray(groups, dtype=np.uint32).tobytes() + np.asarray(cnts, dtype=np.uint32).tobytes()


@lru_cache(maxsize=None)
def histogram(name: str, k: int, paired: bool) -> Rows:
    rd = reads_of(name, k, paired)
    h = er.scan(index(name, k), vt.REFS[name].G, k, rd.seq, rd.qual, rd.offsets, cutoff=CUTOFF, paired=paired)
    keys = {}

    def key(content):
        b = keys.get(id(content))
        if b is None:
            b = keys[id(content)] = row_key([g for g, _ in content], [c for _, c in content])
        return b

    unmerged = {(key(c), m): n for (c, m), n in h.unmerged.items()}
    merged = {key(c): m for c, m in h.merged.items()}
    assert len(merged) == len(h.merged)
    return Rows((h.n_intervals, h.n_entries, h.n_windows), unmerged, merged, h)


def percent(name: str) -> np.ndarray:
    """The percentage vector of the EM-step check: random, non-negative, finite."""
    G = vt.REFS[name].G
    return np.random.default_rng(1000 + G).uniform(0.0, 50.0, G)


@lru_cache(maxsize=None)
def oracle_em_pass(name: str, k: int, paired: bool, local: bool) -> np.ndarray:
    rd = reads_of(name, k, paired)
    return oracle(name, k).em_pass(rd.seq, rd.qual, rd.offsets, percent(name), counts(name), phred_cutoff=CUTOFF,
                                   paired=paired, local=local)


@lru_cache(maxsize=None)
def exact_step(name: str, k: int, paired: bool) -> tuple:
    h = histogram(name, k, paired).exact
    return tuple(er.exact_step(percent(name), counts(name), h.unique, h.merged))


@lru_cache(maxsize=None)
def report(name: str, k: int, paired: bool) -> rm.Report:
    rd = reads_of(name, k, paired)
    return rm.report(index(name, k), vt.REFS[name].G, k, rd.seq, rd.qual, rd.offsets, cutoff=CUTOFF, paired=paired)
