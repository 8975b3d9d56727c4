"""References of short, empty and tiny contigs, and reads over their breaks (DESIGN.md §4e "Exactness").

Every other scan test indexes a handful of equal-length records far longer than k and than a read. Draft assemblies
hold contigs shorter than k, shorter than a 32-position granule, and empty records, and the code that depends on where
texts start and end (the END classes and granule padding of the anchor structures, the text lookups by binary search,
the flattened reference windows of the .dat pass, the label search of the GPU build) sees none of that otherwise.

`fragmented(k)`: four 4,000-base genomes cut left to right into consecutive contigs (so reads drawn from the uncut
genomes span the breaks), plus a fifth group whose records are all shorter than k (no reference window at all).
`reads(k)`: reads from the uncut genomes, splice reads that equal the index's 2-bit text across separators (a separator
is coded as A there, so only the END classes stop a run), and the contigs themselves as reads.
`TINY`: whole collections below one granule (32), one occ block (96), 160 and 256 symbols.

numpy only, deterministic (synth's counter-based streams), no library load. tests/test_frag_refs_cpu.py asserts the
properties of these inputs that the GPU tests rely on."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from speq_amd import synth

GENOMES, LENGTH, N_RATE = 4, 4_000, 0.001
LONG = (150, 300, 700)
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s: bytes) -> bytes:
    return s.translate(COMP)[::-1]


def short_lengths(k: int) -> list[int]:
    """Contig lengths around every boundary of the structures: nothing, a few bases, half a granule, a granule, two
    16-B staging chunks, an occ block, k_scan_ax's word widths, and k itself (k - 1: no window; k: one; 2k - 2: the
    windows of both ends overlap in every base)."""
    return sorted({0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, k - 1, k, k + 1,
                   2 * k - 2, 2 * k - 1})


def planted(k: int) -> list[int]:
    """One run of contig lengths in every genome: a read over it spans at least six texts."""
    return [1, 0, 2, 0, 0, 3, k - 1, k, k + 1]


def _cut(genome: bytes, lengths) -> list[bytes]:
    """Consecutive contigs of the given lengths; the last contig is what remains (lengths past the end are unused)."""
    out, p = [], 0
    for n in lengths:
        if p + n >= len(genome):
            break
        out.append(genome[p:p + n])
        p += n
    out.append(genome[p:])
    return out


@dataclass(frozen=True)
class Fragmented:
    records: tuple
    groups: tuple
    G: int
    uncut: synth.Reference      # the four genomes the contigs of groups 0..3 were cut from (reads come from these)
    n_cut: int                  # records of groups 0..3 (the fifth group's records follow)


@lru_cache(maxsize=None)
def fragmented(k: int, seed: int = 0, length: int = LENGTH, n_rate: float = N_RATE) -> Fragmented:
    five = synth.make_reference(GENOMES + 1, 1, length, ref_n_rate=n_rate)
    uncut = synth.make_reference(GENOMES, 1, length, ref_n_rate=n_rate)
    assert five.records[:GENOMES] == uncut.records
    short = short_lengths(k)
    records, groups = [], []
    for g in range(GENOMES):
        draw = synth.rand_u64(0xF4A6 + 64 * seed + g, 0, 400)
        lengths = []
        for c in range(200):
            if c == 1 + g:  # (a different place in every genome)
                lengths += planted(k)
            lengths.append(LONG[int(draw[2 * c]) % 3] if c % 3 == 2 else short[int(draw[2 * c + 1]) % len(short)])
        contigs = _cut(uncut.records[g], lengths)
        assert b"".join(contigs) == uncut.records[g]
        records += contigs
        groups += [g] * len(contigs)
    n_cut = len(records)
    # the fifth group: every record shorter than k, every other one of k - 1 bases
    below = [n for n in short if n < k]
    draw = synth.rand_u64(0xF4A6 + 64 * seed + GENOMES, 0, 2 * length)
    lengths = [k - 1 if c % 2 else below[int(draw[c]) % len(below)] for c in range(2 * length)]
    pieces = _cut(five.records[GENOMES], lengths)  # (what remains at the end is shorter than the length it cut short)
    assert all(len(p) < k for p in pieces)
    records += pieces
    groups += [GENOMES] * len(pieces)
    return Fragmented(tuple(records), tuple(groups), GENOMES + 1, uncut, n_cut)


def texts_of(records) -> list[bytes]:
    """The index's texts in its order: [fwd_r, rc_r, fwd_r+1, ...]."""
    out = []
    for r in records:
        out += [bytes(r), revcomp(bytes(r))]
    return out


def text_starts(records) -> np.ndarray:
    """Start of every text in the FM text (each text is followed by one separator)."""
    lens = np.array([len(t) + 1 for t in texts_of(records)], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(lens)[:-1]])


def splice_reads(records, n: int, read_len: int = 150, seed: int = 0):
    """(reads, texts spanned by each): the tail of text i, then 'A', then texts i + 1, i + 2, ... joined by 'A' until
    read_len bases: the bases of the index's 2-bit text over the separators between them. Reads that hold an N are
    dropped (an N is coded as A too, but it is no text end)."""
    texts = texts_of(records)
    draw = synth.rand_u64(0x5B11CE + seed, 0, 2 * n)
    reads, spans = [], []
    for j in range(n):
        i = int(draw[2 * j]) % (len(texts) - 1)
        if not texts[i]:
            continue
        tail = 1 + int(draw[2 * j + 1]) % min(len(texts[i]), read_len - 1)
        r, t = texts[i][len(texts[i]) - tail:], i
        while len(r) < read_len and t + 1 < len(texts):
            t += 1
            r += b"A" + texts[t]
        if len(r) < read_len or b"N" in r[:read_len]:
            continue
        # texts touched by the first read_len bases
        used, span = tail, 1
        for u in range(i + 1, t + 1):
            if used + 1 > read_len:
                break
            used += 1 + len(texts[u])
            span += 1
        reads.append(r[:read_len])
        spans.append(span)
    return reads, spans


def contig_reads(records, k: int, read_len: int = 150) -> list[bytes]:
    """Every N-free contig of k .. read_len bases, followed by its reverse complement."""
    out = []
    for r in records:
        if k <= len(r) <= read_len and b"N" not in r:
            out += [bytes(r), revcomp(bytes(r))]
    return out


def pack(seqs, qual: bytes = b"I") -> synth.Reads:
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8).copy()
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return synth.Reads(seq, np.full(seq.size, qual[0], dtype=np.uint8), off, np.zeros(len(seqs), np.int32))


def concat(parts) -> synth.Reads:
    lens = np.concatenate([np.diff(p.offsets) for p in parts])
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return synth.Reads(np.concatenate([p.seq for p in parts]), np.concatenate([p.qual for p in parts]), off,
                       np.concatenate([p.variant for p in parts]))


N_GENOME_READS, N_SPLICE = 2_000, 600  # (about 500 splice reads stay after those with an N are dropped)


@lru_cache(maxsize=None)
def reads(k: int, paired: bool = False, read_len: int = 150, length: int = LENGTH, n_genome: int = N_GENOME_READS,
          n_splice: int = N_SPLICE) -> synth.Reads:
    """(a) reads (or pairs) from the uncut genomes, which span the breaks; (b) splice reads; (c) the contigs of k ..
    read_len bases and their reverse complements. paired: (b) two by two, (c) contig and reverse complement as mates.
    Qualities are 'I' apart from what make_reads adds."""
    fr = fragmented(k, length=length)
    a = synth.make_reads(fr.uncut, n_genome // 2 if paired else n_genome, read_len=read_len, err_rate=0.002,
                         lowq_rate=0.005, paired=paired, fragment=min(length, max(300, 2 * read_len)))
    b, _ = splice_reads(fr.records, n_splice, read_len)
    if paired and len(b) % 2:
        b = b[:-1]
    c = contig_reads(fr.records, k, read_len)
    return concat([a, pack(b), pack(c)])


# ---------------------------------------------------------------- tiny collections
def fm_length(records) -> int:
    """Symbols of the FM text: both strands of every record, a separator each, one terminator."""
    return sum(2 * (len(r) + 1) for r in records) + 1


def _tiny_reads(records, k: int) -> synth.Reads:
    """A few short strings: every text and its neighbours spliced over 'A' (the whole 2-bit text, then poly-A: longer
    than the collection, so a run from any position would read past n), poly-A and poly-T of 300, the records
    themselves, every text cut to k and to k - 1 bases, strings of other bases of 48, k and k - 1 bases, and an empty
    read."""
    texts = texts_of(records)
    whole = b"A".join(t.replace(b"N", b"A") for t in texts)
    seqs = [whole + b"A" * 40, (whole + b"A" + b"A" * 200)[:300], whole[1:] + b"AA", b"A" * 300, b"T" * 300,
            b"ACGT" * 12, (b"GATC" * 40)[:k], (b"GATC" * 40)[:k - 1], b""]
    for t in texts:
        seqs += [t, t[:k], t[:k - 1], t[-k:] + b"A"]
    return pack(seqs)


def _tiny() -> list:
    rng = np.random.default_rng(20)
    dna = lambda n: bytes(rng.choice(synth.ACGT, size=n))  # noqa: E731
    cases = [
        ([b"ACGTA"], [0], 1, 3),                                         # n = 13: below one granule
        ([b"AC", b"", b"G", b"ACGTACGTAC"], [0, 1, 2, 3], 4, 3),         # n = 35
        ([dna(20), dna(20)], [0, 1], 2, 7),                              # n = 85: below one occ block
        ([b"A" * 5, b"C" * 4], [0, 1], 2, 5),                            # n = 23: group 1 has no window
        ([dna(6), dna(6)], [0, 1], 2, 9),                                # n = 29: no window anywhere
        ([dna(25), b"", dna(12) + b"N" + dna(17)], [0, 1, 1], 2, 11),    # n = 117: below 160
        ([dna(40), dna(3), dna(50), b"G"], [0, 1, 1, 0], 2, 21),         # n = 197: below 256
    ]
    out = []
    for records, groups, G, k in cases:
        out.append((records, groups, G, k, _tiny_reads(records, k)))
    return out


TINY = _tiny()
TINY_IDS = [f"n{fm_length(c[0])}-k{c[3]}" for c in TINY]
