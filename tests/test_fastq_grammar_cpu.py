"""CPU: the Python grammar of fastq_grammar.py against the host reader (speq_fastq_checksum), over every input the
GPU parser's tests use (test_gpu_fastq_parse.py), and the two halves of that grammar against each other. This ties
the reference of the GPU tests to the sequential reader, which is the contract."""
import ctypes as C
import functools

import pytest

import fastq_grammar as fg
from speq_amd import SpeqError
from speq_amd._lib import SPEQ_E_IO, check, lib


def checksum(p1, p2=None, threads=3):
    r, b, d = C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(lib().speq_fastq_checksum(str(p1).encode(), str(p2).encode() if p2 else None, threads, C.byref(r),
                                    C.byref(b), C.byref(d)))
    return r.value, b.value, d.value


SMALL = {c.name: c for c in fg.single_cases() + [fg.sweep_case(p) for p in range(33)] + fg.paired_cases() +
         fg.error_cases()}
BIG = ["big_2048_items", "big_2049_items", "big_8_5_MiB"]


@functools.lru_cache(maxsize=None)
def big():
    return {c.name: c for c in fg.big_cases()}


def case_of(name):
    return SMALL[name] if name in SMALL else big()[name]


def by_general(case):
    """The records of the case's file(s) by the general grammar (pairs zipped to the shorter file), or the error."""
    try:
        r1 = fg.general(case.raw1)
        if not case.paired:
            return r1
        return [x for pair in zip(r1, fg.general(case.raw2)) for x in pair]
    except fg.GrammarError as e:
        return e


def test_digest_by_length_is_the_digest():
    recs = [(b"", b""), (b"A", b"I"), (b"ACGTN", b"I#5~!"), (b"TTTTT", b"+@IIJ"), (b"", b""),
            (b"G" * 70, bytes(range(40, 110)))]
    assert fg.digest_by_length(recs) == fg.digest(recs)
    assert fg.digest_by_length([]) == fg.digest([]) == 0


@pytest.mark.parametrize("name", list(SMALL) + BIG)
def test_host_reader_matches_general_grammar(tmp_path, monkeypatch, name):
    case = case_of(name)
    p1, p2 = tmp_path / "1.fq", None
    p1.write_bytes(case.raw1)
    if case.paired:
        p2 = tmp_path / "2.fq"
        p2.write_bytes(case.raw2)
    exp = by_general(case)
    for split_cut in ("1",) if case.big else ("1", "0"):
        monkeypatch.setenv("SPEQ_SPLIT_CUT", split_cut)
        if isinstance(exp, fg.GrammarError):
            with pytest.raises(SpeqError, match=fg.MESSAGES[exp.kind]) as ei:
                checksum(p1, p2)
            assert ei.value.code == SPEQ_E_IO
        else:
            want = (len(exp), sum(len(s) for s, _ in exp), fg.digest_by_length(exp))
            assert checksum(p1, p2) == want


@pytest.mark.parametrize("name", list(SMALL) + BIG)
def test_four_line_contract_agrees_with_general_grammar(name):
    """Where k_records' checks flag nothing and the record count is the text's, the four-line reading and the general
    grammar give the same records; where the generator knows the reads, both give those; where they flag something
    the general grammar rejects the file or (too few lines) holds fewer records."""
    case = case_of(name)
    recs, err = case.expected()
    if case.bits is not None:
        assert err == case.bits
        assert [i for i, r in enumerate(recs) if r == (b"", b"")] == case.bad
    else:
        assert err == 0
    if case.reads1 is not None:
        want = ([x for pair in zip(case.reads1, case.reads2) for x in pair] if case.paired else case.reads1)
        assert recs == want
    gen = by_general(case)
    if err == 0:
        assert gen == recs
    elif err == fg.ERR_LINES:
        assert len(gen) < len(recs) and gen == recs[:len(gen)]  # (pairs are zipped to the shorter file)
    else:
        assert isinstance(gen, fg.GrammarError)


@pytest.mark.parametrize("base,qual,ok", [(b" ", b" ", False), (b"7", b" ", False), (b" \t", b"  ", False),
                                          (b"12", b"II", False), (b"", b" ", False), (b" ", b"", True),
                                          (b"\r", b"\r", True), (b"", b"", True)])
def test_base_line_without_bases(tmp_path, monkeypatch, base, qual, ok):
    """A base line of blanks and digits gives no bases, so the record ends at its '+' line; a quality line that is
    not empty is then read as the next header and refused. The four-line cut (fast_record) must not take such a record
    for an empty read: same error with the parallel cut, the sequential cutter, one thread or several."""
    full = b"@a\nACGT\n+\nIIII\n"
    data = full + b"@r\n" + base + b"\n+\n" + qual + b"\n" + full
    p = tmp_path / "b.fq"
    p.write_bytes(data)
    bits, _ = fg.four_line(data, 3)
    for split_cut in ("1", "0"):
        monkeypatch.setenv("SPEQ_SPLIT_CUT", split_cut)
        for threads in (1, 4):
            if ok:
                assert bits == [0, 0, 0]
                assert checksum(p, threads=threads) == (3, 8, fg.digest(fg.general(data)))
            else:
                assert bits[1] & fg.ERR_LENGTH
                with pytest.raises(SpeqError, match="malformed FASTQ record header|mismatch"):
                    checksum(p, threads=threads)
                with pytest.raises(fg.GrammarError):
                    fg.general(data)


def test_parse_block_accessor_checks_its_arguments():
    """speq_fastq_parse_block refuses bad shapes on the host, and n_records = 0 launches nothing (no GPU needed)."""
    from speq_amd._lib import SPEQ_E_ARG
    from speq_amd.api import fastq_parse_block
    seq, qual, off, err, total = fastq_parse_block(b"@r\nA\n+\nI\n", None, 0)
    assert off.tolist() == [0] and err == 0 and total == 0
    seq, qual, off, err, total = fastq_parse_block(b"", b"", 0)
    assert off.tolist() == [0] and len(seq) == len(qual) == 0
    L = lib()
    o, e, t = (C.c_uint64 * 3)(), C.c_uint32(), C.c_uint64()
    buf = (C.c_uint8 * 16)()
    raw = b"@r\nA\n+\nI\n"
    bad = [
        (0, raw, len(raw), 0, 1, 0, buf, buf, None, C.byref(e), C.byref(t)),     # no offsets
        (0, raw, len(raw), 0, 1, 0, buf, buf, o, None, C.byref(t)),              # no err
        (0, raw, len(raw), 0, 1, 0, buf, buf, o, C.byref(e), None),              # no total
        (0, None, len(raw), 0, 1, 0, buf, buf, o, C.byref(e), C.byref(t)),       # no text
        (0, raw, len(raw), 0, 1, 0, None, buf, o, C.byref(e), C.byref(t)),       # no seq
        (0, raw, len(raw), 0, 1, 0, buf, None, o, C.byref(e), C.byref(t)),       # no qual
        (-1, raw, len(raw), 0, 1, 0, buf, buf, o, C.byref(e), C.byref(t)),       # device
        (0, raw, len(raw), 0, 1, 2, buf, buf, o, C.byref(e), C.byref(t)),        # paired not 0 / 1
        (0, raw, 5, 4, 1, 0, buf, buf, o, C.byref(e), C.byref(t)),               # len2 without paired
        (0, raw, 1 << 32, 0, 1, 0, buf, buf, o, C.byref(e), C.byref(t)),         # 4 GiB
        (0, raw, (1 << 31) + 5, 1 << 31, 1, 1, buf, buf, o, C.byref(e), C.byref(t)),
        (0, raw, len(raw), 0, 1 << 28, 0, buf, buf, o, C.byref(e), C.byref(t)),  # records
    ]
    for dev, r, l1, l2, n, paired, s, q, off_p, e_p, t_p in bad:
        rc = L.speq_fastq_parse_block(dev, r, l1, l2, n, paired, 0x0A, 0, s, q, off_p, e_p, t_p)
        assert rc == SPEQ_E_ARG, (dev, l1, l2, n, paired)
