"""A plain, slow restatement of the FASTQ grammar and the inputs that pin the GPU parser (fastq_gpu.hip) to it.

Two statements of what a block of text means:

* general(data): the sequential reader's grammar (get_line / scan_record / parse_record in fastq_stream.cpp) — the
  contract. Returns the records or raises GrammarError(kind).
* four_line(data, n): what k_records makes of the same text when it is told that it holds n four-line records: the
  error bits of every record (1 header, 2 separator, 4 length, 8 lines) and the records, a flagged one empty.

Where four_line flags nothing and n is the text's line count / 4, both give the same records (checked on the CPU by
test_fastq_grammar_cpu.py, which also ties general() to the host reader through speq_fastq_checksum); where it flags
something, the stream hands the file to the sequential reader, so general() decides.

The cases (single_cases, paired_cases, error_cases, big_cases) are shared by the CPU and the GPU tests."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

M64 = (1 << 64) - 1
BLANKS = b" \t\n\v\f\r"
DIGITS = b"0123456789"
ERR_HEADER, ERR_PLUS, ERR_LENGTH, ERR_LINES = 1, 2, 4, 8
NL_WIN, NL_SPAN, SCAN_TILE = 16, 4096, 2048  # fastq_gpu.hip: bytes per thread and per workgroup; items per scan tile


# ---- the digest of speq_fastq_checksum ----
def mix(z):
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def digest(records):
    acc = 0
    for s, q in records:
        h = 0x9e3779b97f4a7c15 ^ len(s)
        for a, b in zip(s, q):
            h = ((h ^ (a << 8 | b)) * 0x100000001b3) & M64
        acc = (acc + mix(h)) & M64
    return acc


def digest_by_length(records):
    """digest(), the records of one length hashed side by side (u64 wrap-around arithmetic is numpy's)."""
    groups = {}
    for s, q in records:
        groups.setdefault(len(s), []).append((s, q))
    acc = 0
    with np.errstate(over="ignore"):
        for n, rs in groups.items():
            S = np.frombuffer(b"".join(s for s, _ in rs), np.uint8).reshape(len(rs), n).astype(np.uint64)
            Q = np.frombuffer(b"".join(q for _, q in rs), np.uint8).reshape(len(rs), n).astype(np.uint64)
            h = np.full(len(rs), 0x9e3779b97f4a7c15 ^ n, dtype=np.uint64)
            for j in range(n):
                h = (h ^ (S[:, j] << np.uint64(8) | Q[:, j])) * np.uint64(0x100000001b3)
            for x in h.tolist():
                acc = (acc + mix(x)) & M64
    return acc


# ---- the general grammar ----
class GrammarError(Exception):
    """kind: 'header' (a record does not open with '@'), 'fasta' (it opens with '>'), 'truncated' (no '+' line),
    'mismatch' (base and quality counts differ)."""

    def __init__(self, kind):
        super().__init__(kind)
        self.kind = kind


# what the host reader's message says for each kind
MESSAGES = {"header": "malformed FASTQ record header", "fasta": "qualities are required", "truncated": "truncated",
            "mismatch": "mismatch"}


def bases_of(line: bytes) -> bytes:
    return line.translate(None, BLANKS + DIGITS)


def quals_of(line: bytes) -> bytes:
    return line.translate(None, BLANKS)


def lines_of(data: bytes):
    """get_line: lines end at '\\n'; a last line without one counts; trailing '\\r's are trimmed."""
    lines = data.split(b"\n")
    if lines[-1] == b"":
        lines.pop()  # nothing after the last '\n' (or empty input)
    return [ln.rstrip(b"\r") for ln in lines]


def general(data: bytes):
    lines = lines_of(data)
    i, out = 0, []
    while True:
        while i < len(lines) and lines[i] == b"":  # blank lines before a header
            i += 1
        if i == len(lines):
            return out
        if lines[i][:1] != b"@":
            raise GrammarError("fasta" if lines[i][:1] == b">" else "header")
        i += 1
        seq = b""
        while True:  # base lines up to the first line that opens with '+'
            if i == len(lines):
                raise GrammarError("truncated")
            ln = lines[i]
            i += 1
            if ln[:1] == b"+":
                break
            seq += bases_of(ln)
        qual = b""
        while len(qual) < len(seq) and i < len(lines):  # quality lines until the counts match
            qual += quals_of(lines[i])
            i += 1
        if len(qual) != len(seq):
            raise GrammarError("mismatch")
        out.append((seq, qual))


# ---- the four-line contract of k_records ----
def four_line(data: bytes, n: int):
    """(bits per record, records) of n four-line records read from data; a flagged record is (b'', b'')."""
    end = len(data)
    nl = np.flatnonzero(np.frombuffer(data, np.uint8) == 10).tolist()
    total = len(nl)
    bits, recs = [], []

    def line_end(j):
        return nl[j] if j < total else end  # the last line may be open

    for r in range(n):
        if 4 * r + 2 >= total:  # fewer than three newlines before the quality line
            bits.append(ERR_LINES)
            recs.append((b"", b""))
            continue
        h = 0 if r == 0 else nl[4 * r - 1] + 1
        s0, s1 = nl[4 * r] + 1, nl[4 * r + 1]
        p0 = s1 + 1
        q0, q1 = nl[4 * r + 2] + 1, line_end(4 * r + 3)
        sline, qline = data[s0:s1].rstrip(b"\r"), data[q0:q1].rstrip(b"\r")
        e = 0
        if h >= end or data[h:h + 1] != b"@":
            e |= ERR_HEADER
        # the third line opens with '+', and the second must not (the general grammar takes it for the separator)
        if p0 >= end or data[p0:p0 + 1] != b"+" or data[s0:s1][:1] == b"+":
            e |= ERR_PLUS
        s, q = bases_of(sline), quals_of(qline)
        # no bases: the general grammar ends the record at '+' and reads a quality line that is not empty (blanks
        # included) as the next header
        if len(s) != len(q) or (len(s) == 0 and qline):
            e |= ERR_LENGTH
        bits.append(e)
        recs.append((b"", b"") if e else (s, q))
    return bits, recs


def nl_groups(begin: int, end: int) -> int:
    """Workgroups of the newline scan over [begin, end), as launch_fastq_parse counts them."""
    a0 = begin & ~(NL_WIN - 1)
    return (end - a0 + NL_SPAN - 1) // NL_SPAN + (1 if end == a0 else 0)


# ---- inputs ----
@dataclass
class Case:
    name: str
    raw1: bytes
    n: int                                # records per file handed to the parser
    raw2: Optional[bytes] = None          # paired when not None
    reads1: Optional[list] = None         # the generator's own (seq, qual) per record, for clean blocks
    reads2: Optional[list] = None
    bits: Optional[int] = None            # error cases: the OR of the flags the issue's table expects
    bad: list = field(default_factory=list)  # error cases: the slots that must come out empty
    big: bool = False

    @property
    def paired(self):
        return self.raw2 is not None

    def expected(self):
        """(records per slot, OR of the error bits) by the four-line contract."""
        b1, r1 = four_line(self.raw1, self.n)
        b2, r2 = four_line(self.raw2, self.n) if self.paired else ([], [])
        recs = [x for pair in zip(r1, r2) for x in pair] if self.paired else r1  # slot 2r + f
        err = 0
        for b in b1 + b2:
            err |= b
        return recs, err


_ALPHA = np.frombuffer(b"ACGTN", np.uint8)


def read(rng, n, qlo=35, qhi=74):
    """(seq, qual) of n random bases (A C G T N) with quality bytes in [qlo, qhi)."""
    return _ALPHA[rng.integers(0, 5, n)].tobytes(), rng.integers(qlo, qhi, n).astype(np.uint8).tobytes()


def text(records, nl=b"\n", final_newline=True, headers=None, plus=b"+"):
    parts = []
    for i, (s, q) in enumerate(records):
        h = headers[i] if headers else b"@r%d" % i
        parts += [h, nl, s, nl, plus, nl, q, nl]
    data = b"".join(parts)
    return data if final_newline else data[:len(data) - len(nl)]


def single_cases():
    rng = np.random.default_rng(20260)
    out = []
    # one record of every length around the 16-byte window, the 64-lane step and two steps
    for L in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300):
        for fin in (True, False):
            r = [read(rng, L)]
            out.append(Case(f"one_L{L}_{'nl' if fin else 'open'}", text(r, final_newline=fin), 1, reads1=r))
    r = [read(rng, 40)]
    t = text(r, headers=[b"@r"])
    t = text(r, headers=[b"@r" + b"x" * (-len(t) % 16)])
    assert len(t) % 16 == 0
    out.append(Case("one_len_multiple_of_16", t, 1, reads1=r))
    t = text(r, headers=[b"@r"], final_newline=False)
    t = text(r, headers=[b"@r" + b"x" * (-len(t) % 16)], final_newline=False)
    assert len(t) % 16 == 0
    out.append(Case("one_open_len_multiple_of_16", t, 1, reads1=r))
    r = [read(rng, 1900)]
    t = text(r, headers=[b"@r"], final_newline=False)
    t = text(r, headers=[b"@r" + b"x" * (4096 - len(t))], final_newline=False)
    assert len(t) == 4096
    out.append(Case("one_open_len_4096", t, 1, reads1=r))
    # line endings
    r = [read(rng, int(n)) for n in rng.integers(1, 90, 9)]
    out.append(Case("crlf", text(r, nl=b"\r\n"), 9, reads1=r))
    out.append(Case("crlf_open", text(r, nl=b"\r\n", final_newline=False), 9, reads1=r))
    out.append(Case("crcrlf", text(r, nl=b"\r\r\n"), 9, reads1=r))
    out.append(Case("cr_base_lines", text([(s + b"\r", q) for s, q in r]), 9, reads1=r))
    out.append(Case("cr_quality_lines", text([(s, q + b"\r") for s, q in r]), 9, reads1=r))
    # compaction: one dropped character at lane 0, lane 63, the second step's lane 0 and 63, and the end, with the
    # quality line's blank somewhere else; then all of them at once
    raw, reads = [], []
    for drop in (b" ", b"\t", b"7"):
        for pos in (0, 63, 64, 127, 200):
            s, q = read(rng, 200)
            qpos = {0: 200, 63: 0, 64: 63, 127: 64, 200: 127}[pos]
            raw.append((s[:pos] + drop + s[pos:], q[:qpos] + b" " + q[qpos:]))
            reads.append((s, q))
    s, q = read(rng, 195)
    rs, rq = bytearray(s), bytearray(q)
    for pos, c in ((0, b"\x0b"), (63, b" "), (64, b"0"), (127, b"\t"), (199, b"9")):  # their places in the raw line
        rs[pos:pos] = c
    for pos in (0, 1, 62, 64, 128):
        rq[pos:pos] = b" "
    raw.append((bytes(rs), bytes(rq)))
    reads.append((s, q))
    raw.append((b"AC7G", b"II I"))
    reads.append((b"ACG", b"III"))
    raw.append((b"ACGT", b"I\tI I\x0cI"))  # lines of different raw lengths whose filtered counts agree
    reads.append((b"ACGT", b"IIII"))
    raw.append((b"A 1C 2G 3T", b"IIII"))
    reads.append((b"ACGT", b"IIII"))
    full = read(rng, 130)
    raw.insert(5, full)  # a straight-copy record between compacted ones
    reads.insert(5, full)
    out.append(Case("compaction", text(raw), len(raw), reads1=reads))
    # quality bytes
    allq = bytes(range(33, 127))
    r = [(read(rng, 94)[0], allq), (read(rng, 94)[0], allq[::-1]), (b"ACGTAC", b"@IIII+"), (b"ACGTAC", b"+IIII@"),
         (b"A", b"@"), (b"C", b"+"), read(rng, 20)]
    out.append(Case("quality_bytes", text(r), len(r), reads1=r))
    out.append(Case("plus_description", text(r, plus=b"+r desc 12 @x"), len(r), reads1=r))
    # empty reads between full ones, first and last
    r = [(b"", b""), read(rng, 30), (b"", b""), (b"", b""), read(rng, 70), (b"", b"")]
    out.append(Case("empty_reads", text(r), len(r), reads1=r))
    out.append(Case("empty_reads_open", text(r, final_newline=False), len(r), reads1=r))
    out.append(Case("empty_reads_crlf", text(r, nl=b"\r\n"), len(r), reads1=r))
    # record counts around the tile of the u64 scan of the lengths (n + 1 items)
    for n in (2047, 2048, 2049, 4097):
        r = [read(rng, int(L)) for L in rng.integers(1, 4, n)]
        out.append(Case(f"records_{n}", text(r), n, reads1=r))
    return out


def sweep_case(p: int):
    """70 records of 61 bases (three 4 KiB spans), the first header p bytes longer."""
    rng = np.random.default_rng(61)
    r = [read(rng, 61) for _ in range(70)]
    heads = [b"@r%02d" % i for i in range(70)]
    heads[0] += b"p" * p
    return Case(f"sweep_p{p}", text(r, headers=heads), 70, reads1=r)


def _pad_to_residue(records, residue, final_newline):
    """text() of the records with the last header lengthened until len % 16 == residue."""
    heads = [b"@m%d" % i for i in range(len(records))]
    t = text(records, headers=heads, final_newline=final_newline)
    heads[-1] += b"h" * ((residue - len(t)) % 16)
    t = text(records, headers=heads, final_newline=final_newline)
    assert len(t) % 16 == residue
    return t


def paired_cases():
    rng = np.random.default_rng(20261)
    out = []
    r1 = [read(rng, int(n)) for n in rng.integers(1, 50, 5)]
    r2 = [read(rng, int(n)) for n in rng.integers(1, 50, 5)]
    for res in range(16):
        for fin in (True, False):
            out.append(Case(f"len1_mod16_{res}_{'nl' if fin else 'open'}", _pad_to_residue(r1, res, fin), 5,
                            raw2=text(r2), reads1=r1, reads2=r2))
    # file 2 opens on a '\n'-free window edge: file 1 ends one byte into a window, file 2's first line is short
    out.append(Case("short_first_header_2", _pad_to_residue(r1, 1, False), 5,
                    raw2=text(r2, headers=[b"@", b"@b", b"@c", b"@d", b"@e"]), reads1=r1, reads2=r2))
    a = [read(rng, 33), (b"", b""), read(rng, 1), (b"", b""), read(rng, 129), read(rng, 64)]
    b = [(b"", b""), read(rng, 77), (b"", b""), (b"", b""), read(rng, 2), read(rng, 200)]
    out.append(Case("mates_differ", text(a), 6, raw2=text(b), reads1=a, reads2=b))
    out.append(Case("mates_differ_open_crlf", text(a, final_newline=False), 6, raw2=text(b, nl=b"\r\n"), reads1=a,
                    reads2=b))
    small = [read(rng, int(n)) for n in rng.integers(1, 12, 3)]
    large = [read(rng, int(n)) for n in rng.integers(5000, 7000, 3)]
    out.append(Case("file2_much_longer", text(small), 3, raw2=text(large), reads1=small, reads2=large))
    out.append(Case("file2_much_shorter", text(large), 3, raw2=text(small), reads1=large, reads2=small))
    m1 = [read(rng, int(n)) for n in rng.integers(0, 6, 1100)]
    m2 = [read(rng, int(n)) for n in rng.integers(0, 6, 1100)]
    out.append(Case("slots_2200", text(m1), 1100, raw2=text(m2), reads1=m1, reads2=m2))
    return out


# the faulty record of an error case: (name, its four lines, the bits the parser must report)
FAULTS = [
    ("header", (b"#r", b"ACGT", b"+", b"IIII"), ERR_HEADER),
    ("separator", (b"@r", b"ACGT", b"-", b"IIII"), ERR_PLUS),
    ("plus_base_line", (b"@r", b"+CGT", b"+", b"IIII"), ERR_PLUS),
    ("filtered_mismatch", (b"@r", b"ACGT7", b"+", b"IIIII"), ERR_LENGTH),
    # a base line of blanks or digits only, with a quality line that is not empty: no bases, so the general grammar
    # ends the record at '+' and takes the quality line for a header
    ("blank_base_line", (b"@r", b" ", b"+", b" "), ERR_LENGTH),
    ("blank_base_line_3", (b"@r", b" \t ", b"+", b"   "), ERR_LENGTH),
    ("digit_base_line", (b"@r", b"7", b"+", b" "), ERR_LENGTH),
    ("empty_base_blank_quality", (b"@r", b"", b"+", b" "), ERR_LENGTH),
]


def _faulty_block(rng, lines):
    good = [read(rng, int(n)) for n in rng.integers(20, 90, 4)]
    recs = [b"@g%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(good)]
    recs.insert(2, b"\n".join(lines) + b"\n")
    reads = good[:2] + [(b"", b"")] + good[2:]
    return b"".join(recs), reads


def error_cases():
    rng = np.random.default_rng(20262)
    out = []
    clean = [read(rng, int(n)) for n in rng.integers(20, 90, 5)]
    for name, lines, bits in FAULTS:
        t, reads = _faulty_block(rng, lines)
        out.append(Case(f"err_{name}", t, 5, reads1=reads, bits=bits, bad=[2]))
        out.append(Case(f"err_{name}_file1", t, 5, raw2=text(clean), reads1=reads, reads2=clean, bits=bits, bad=[4]))
        out.append(Case(f"err_{name}_file2", text(clean), 5, raw2=t, reads1=clean, reads2=reads, bits=bits, bad=[5]))
    # one record more than the text holds: the last one has no lines
    gone = clean + [(b"", b"")]
    six = clean + [read(rng, 25)]
    out.append(Case("err_count_plus_one", text(clean), 6, reads1=gone, bits=ERR_LINES, bad=[5]))
    out.append(Case("err_count_plus_one_open", text(clean, final_newline=False), 6, reads1=gone, bits=ERR_LINES,
                    bad=[5]))
    out.append(Case("err_count_plus_one_file1", text(clean), 6, raw2=text(six), reads1=gone, reads2=six,
                    bits=ERR_LINES, bad=[10]))
    out.append(Case("err_count_plus_one_file2", text(six), 6, raw2=text(clean), reads1=six, reads2=gone,
                    bits=ERR_LINES, bad=[11]))
    out.append(Case("err_empty_text", b"", 1, reads1=[(b"", b"")], bits=ERR_LINES, bad=[0]))
    out.append(Case("err_empty_text_paired", b"", 1, raw2=b"", reads1=[(b"", b"")], reads2=[(b"", b"")],
                    bits=ERR_LINES, bad=[0, 1]))
    out.append(Case("err_empty_file2", text(clean[:1]), 1, raw2=b"", reads1=clean[:1], reads2=[(b"", b"")],
                    bits=ERR_LINES, bad=[1]))
    return out


def _big(name, target_len, seed):
    """Records of 4,700 bases, the last one cut so that the text is exactly target_len bytes."""
    rng = np.random.default_rng(seed)
    per = len(b"@r0000\n") + 4700 + len(b"\n+\n") + 4700 + 1
    n = target_len // per
    rest = target_len - (n - 1) * per - len(b"@r0000\n\n+\n\n")
    odd = rest % 2  # one more header byte
    rest -= odd
    assert rest >= 0
    lens = [4700] * (n - 1) + [rest // 2]
    S = _ALPHA[rng.integers(0, 5, sum(lens))].tobytes()
    Q = rng.integers(35, 74, sum(lens)).astype(np.uint8).tobytes()
    r, o = [], 0
    for L in lens:
        r.append((S[o:o + L], Q[o:o + L]))
        o += L
    heads = [b"@r%04d" % i for i in range(n)]
    heads[-1] += b"x" * odd
    t = text(r, headers=heads)
    assert len(t) == target_len
    return Case(name, t, n, reads1=r, big=True)


def big_cases():
    """Blocks whose newline scan (one count per 4 KiB span, groups + 1 items) fills one tile exactly, spills one item
    into a second tile, and runs well into it."""
    return [_big("big_2048_items", 2047 * NL_SPAN, 1), _big("big_2049_items", 2047 * NL_SPAN + 1, 2),
            _big("big_8_5_MiB", 8912896 + 1234, 3)]
