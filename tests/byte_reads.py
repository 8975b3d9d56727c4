"""Reads over the whole byte range, for the tests of the raw read-byte contract (DESIGN.md §4e "Exactness").

The contract every scan path implements (restated in oracle/kmer_oracle.c: dna5, phred42): a base byte is one of
``ACGT`` / ``acgt``, ``U`` / ``u`` (read as T), or N (every other byte); a quality byte is ``byte - 33`` clamped to
[0, 41]; a window passes iff none of its bases is N and every clamped quality is ``> cutoff``.

`byte_reads` is the one generator of the tests: synth.make_reads, then soft-masked lower case, RNA ``U``, junk bytes
chosen next to the accepted letters, and quality bytes at the cutoff's edge, above ``J`` and above 0x7F. Every draw
comes from synth's counter-based streams, so the bytes depend on the arguments alone. The other helpers here cut reads
to given lengths and run a scan on device-resident torch tensors of the raw bytes.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from speq_amd import synth

ACCEPTED = b"ACGTUacgtu"
IUPAC = b"RYSWKMBDHVNryswkmbdhvn"

# Per-base rates. Lower case and U are common in real data; the junk and failing-quality rates are set so that a
# window of 70 bases still passes more often than not ((1 - 0.0035 - 0.005)^70 = 0.55): the tests require T above
# half of all windows at k = 70, so that a decoder which fails too much is seen as well as one that passes too much.
LOWER_RATE, U_RATE, JUNK_RATE, FAILQ_RATE = 0.30, 0.15, 0.0035, 0.005


# The inputs of the GPU tests (tests/test_gpu_bytes.py), which the CPU suite checks for non-vacuity with the oracle
N_READS, SEED, G = 1_500, 3, 4


def reference() -> synth.Reference:
    return synth.make_reference(G, 2, 3_000, ref_n_rate=0.002)


def rank(byte: int) -> int:
    """phred42 rank of a quality byte."""
    return min(41, max(0, byte - 33))


def junk_bytes(fastq_safe: bool = False) -> list[int]:
    """Bytes that are N although they look like a base to a sloppy decoder: every byte one bit away from an accepted
    letter (``@`` `````, ``E``, ``Q``, ``5``, 0xC1, ...), the IUPAC codes in both cases, 0x00 and 0xFF. fastq_safe:
    the ASCII letters among those, and ``* - .`` (what a four-line FASTQ base line can hold)."""
    near = {a ^ (1 << b) for a in ACCEPTED for b in range(8)}
    junk = (near | set(IUPAC) | {0x00, 0xFF}) - set(ACCEPTED)
    if fastq_safe:
        junk = {b for b in junk if chr(b).isascii() and chr(b).isalpha()} | set(b"*-.")
    return sorted(junk)


def quality_bytes(cutoff: int, fastq_safe: bool = False) -> tuple[list[int], list[int]]:
    """(passing, failing) quality bytes for a cutoff: the two bytes just above the cutoff, the neighbours of ``J``
    (ranks 40, 41, 41), of ``~`` and of 0x80, 200 and 255; and 0, 10, blank, ``!`` and the two bytes at the cutoff.
    fastq_safe keeps 33..126. When nothing can pass (cutoff >= 41) the first list holds the same candidates, which all
    fail then."""
    lo, hi = (33, 126) if fastq_safe else (0, 255)
    cand = [b for b in (34 + cutoff, 35 + cutoff, 73, 74, 75, 126, 127, 128, 200, 255) if lo <= b <= hi]
    passing = sorted({b for b in cand if rank(b) > cutoff}) or sorted(set(cand))
    failing = sorted({b for b in (0, 10, 32, 33, 33 + cutoff, 32 + cutoff) if lo <= b <= hi and rank(b) <= cutoff})
    return passing, failing


@dataclass
class Masks:
    """Per-base classes of byte_reads' output (a junk byte belongs to no other class)."""
    lower: np.ndarray   # lower-case accepted letters (acgtu)
    u: np.ndarray       # U or u
    junk: np.ndarray    # junk_bytes()


def byte_reads(ref, n: int, cutoff: int, seed: int, paired: bool = False, read_len: int = 150,
               fastq_safe: bool = False):
    """(Reads, Masks): n reads (or pairs) of synth.make_reads(ref, n, err_rate=0.003) with
    bases: ~30 % lower case, ~15 % of T/t as U/u, ~0.35 % junk_bytes();
    qualities: half of the reads one passing byte throughout (windows of one quality), the others a fresh passing
    byte per base (neighbours that differ as bytes but share rank 41 included); ~0.5 % failing bytes."""
    reads = synth.make_reads(ref, n, read_len=read_len, err_rate=0.003, paired=paired)
    seq = reads.seq.copy()
    nb, nr = seq.size, reads.n
    s = 0xB17E00 + 16 * seed
    lower = synth.rand_unit(s, 0, nb) < LOWER_RATE
    seq[lower] |= 0x20
    u = ((seq | 0x20) == ord("t")) & (synth.rand_unit(s + 1, 0, nb) < U_RATE)
    seq[u] += 1  # T -> U, t -> u
    junk = synth.rand_unit(s + 2, 0, nb) < JUNK_RATE
    jset = np.array(junk_bytes(fastq_safe), dtype=np.uint8)
    seq[junk] = jset[(synth.rand_u64(s + 3, 0, nb)[junk] % np.uint64(len(jset))).astype(np.int64)]
    lower &= ~junk
    u &= ~junk

    passing, failing = quality_bytes(cutoff, fastq_safe)
    pset, fset = np.array(passing, dtype=np.uint8), np.array(failing, dtype=np.uint8)
    lens = np.diff(reads.offsets).astype(np.int64)
    read_of = np.repeat(np.arange(nr), lens)
    uniform = (synth.rand_u64(s + 4, 0, nr) & np.uint64(1)).astype(bool)
    per_read = pset[(synth.rand_u64(s + 5, 0, nr) % np.uint64(len(pset))).astype(np.int64)]
    per_base = pset[(synth.rand_u64(s + 6, 0, nb) % np.uint64(len(pset))).astype(np.int64)]
    qual = np.where(uniform[read_of], per_read[read_of], per_base).astype(np.uint8)
    failq = synth.rand_unit(s + 7, 0, nb) < FAILQ_RATE
    qual[failq] = fset[(synth.rand_u64(s + 8, 0, nb)[failq] % np.uint64(len(fset))).astype(np.int64)]
    return synth.Reads(seq, qual, reads.offsets, reads.variant), Masks(lower, u, junk)


def cut(reads, lens) -> synth.Reads:
    """reads with record i cut to its first lens[i] bytes (lens[i] <= its length)."""
    lens = np.asarray(lens, dtype=np.int64)
    old = np.diff(reads.offsets).astype(np.int64)
    assert lens.shape == old.shape and (lens <= old).all() and (lens >= 0).all()
    pos = np.arange(reads.seq.size, dtype=np.int64) - np.repeat(reads.offsets[:-1].astype(np.int64), old)
    keep = pos < np.repeat(lens, old)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return synth.Reads(np.ascontiguousarray(reads.seq[keep]), np.ascontiguousarray(reads.qual[keep]), off,
                       reads.variant)


def gather(reads_list, order) -> synth.Reads:
    """The records order[j] = (i, r) (record r of reads_list[i]) concatenated in that order."""
    segs, quals, var = [], [], []
    for i, r in order:
        rd = reads_list[i]
        a, b = int(rd.offsets[r]), int(rd.offsets[r + 1])
        segs.append(rd.seq[a:b])
        quals.append(rd.qual[a:b])
        var.append(int(rd.variant[r]))
    off = np.zeros(len(segs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in segs], dtype=np.uint64)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, np.uint8)  # noqa: E731
    return synth.Reads(cat(segs), cat(quals), off, np.asarray(var, dtype=np.int32))


def device_scan(dev, reads, k: int, cutoff: int = 30, paired: bool = False, local: bool = False):
    """speq_scan_reads_device on torch tensors of the raw bytes (base pointers as torch allocates them). Returns
    (T, ambiguous, U[G] u64, W[G] f64 or None)."""
    import torch
    G = dev.n_groups
    # an input without bytes still gets one-byte buffers: the entry point takes no null read buffer (and torch wants
    # writable arrays)
    pad = lambda a: (a if a.flags.writeable else a.copy()) if a.size else np.zeros(1, np.uint8)  # noqa: E731
    d_seq = torch.from_numpy(pad(reads.seq)).cuda()
    d_qual = torch.from_numpy(pad(reads.qual)).cuda()
    d_off = torch.from_numpy(reads.offsets.astype(np.int64)).cuda()
    d_counts = torch.zeros(G + 2, dtype=torch.int64, device="cuda")
    d_w = torch.zeros(G, dtype=torch.float64, device="cuda")
    dev.scan_device(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), reads.n, k, d_counts.data_ptr(),
                    d_w.data_ptr() if local else 0, phred_cutoff=cutoff, paired=paired, local=local,
                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    c = d_counts.cpu().numpy().astype(np.uint64)
    return int(c[0]), int(c[1]), c[2:].copy(), d_w.cpu().numpy() if local else None
