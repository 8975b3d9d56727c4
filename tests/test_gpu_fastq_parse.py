"""GPU: the records of the FASTQ parser (fastq_gpu.hip), byte for byte, against the grammar of fastq_grammar.py.

One parse per call through the test accessor speq_fastq_parse_block: offsets, the bases and qualities up to
offsets[-1], the error flags and the base total are compared exactly; every output byte at or past offsets[-1] must
still hold the poison the buffers were filled with; and each input runs with the scratch, the offsets and the outputs
poisoned with 0x00 and with 0xFF (a slot's scratch is whatever the block before left there), with identical results.
The text is padded with '\\n', so a read past its end shows as extra newlines. For clean generated blocks the expected
records are the generator's own; for the others they come from the four-line contract, which
test_fastq_grammar_cpu.py ties to the general grammar and to the host reader on the same inputs."""
import time

import numpy as np
import pytest

import fastq_grammar as fg
from speq_amd.api import fastq_parse_block

pytestmark = pytest.mark.gpu

SINGLE = {c.name: c for c in fg.single_cases()}
PAIRED = {c.name: c for c in fg.paired_cases()}
ERRORS = {c.name: c for c in fg.error_cases()}


def generated(case):
    """The generator's own records, in slot order."""
    return [x for pair in zip(case.reads1, case.reads2) for x in pair] if case.paired else list(case.reads1)


def parse_and_compare(case, recs, err):
    """Runs the case under both poisons; returns the (identical) offsets."""
    exp_seq = np.frombuffer(b"".join(s for s, _ in recs), np.uint8)
    exp_qual = np.frombuffer(b"".join(q for _, q in recs), np.uint8)
    exp_off = np.concatenate([[0], np.cumsum([len(s) for s, _ in recs])]).astype(np.uint64)
    end = int(exp_off[-1])
    n_raw = len(case.raw1) + (len(case.raw2) if case.paired else 0)
    for poison in (0x00, 0xFF):
        seq, qual, off, got_err, total = fastq_parse_block(case.raw1, case.raw2, case.n, pad_byte=0x0A, poison=poison)
        assert len(seq) == len(qual) == n_raw and len(off) == len(recs) + 1
        assert np.array_equal(off, exp_off), (case.name, poison, np.flatnonzero(off != exp_off)[:8])
        assert got_err == err, (case.name, poison)
        assert total == end
        for name, got, exp in (("seq", seq, exp_seq), ("qual", qual, exp_qual)):
            bad = np.flatnonzero(got[:end] != exp)
            assert bad.size == 0, (case.name, name, poison, bad[:8], got[bad[:8]], exp[bad[:8]])
            tail = np.flatnonzero(got[end:] != poison)
            assert tail.size == 0, (case.name, name, poison, "written past offsets[-1]", tail[:8] + end)
    return exp_off


@pytest.mark.parametrize("name", list(SINGLE))
def test_single_end_blocks(name):
    case = SINGLE[name]
    recs, err = case.expected()
    assert err == 0 and recs == generated(case)  # (the contract agrees with the generator: also checked on the CPU)
    parse_and_compare(case, generated(case), 0)


def test_alignment_sweep():
    """70 records of 61 bases over three 4 KiB spans, the first header 0..32 bytes longer: every newline meets every
    residue mod 16, and the span edges 4095 / 4096 / 4097."""
    at_4095 = at_0 = False
    for p in range(33):
        case = fg.sweep_case(p)
        assert fg.nl_groups(0, len(case.raw1)) == 3
        nl = np.flatnonzero(np.frombuffer(case.raw1, np.uint8) == 10)
        at_4095 |= bool(np.any(nl % 4096 == 4095))
        at_0 |= bool(np.any((nl % 4096 == 0) & (nl > 0)))
        parse_and_compare(case, generated(case), 0)
    assert at_4095 and at_0


@pytest.mark.parametrize("name", list(PAIRED))
def test_paired_blocks(name):
    case = PAIRED[name]
    if name.startswith("len1_mod16_"):
        assert len(case.raw1) % 16 == int(name.split("_")[2])
        assert (case.raw1[-1:] == b"\n") == name.endswith("_nl")
    off = parse_and_compare(case, generated(case), 0)
    lens = np.diff(off.astype(np.int64)).tolist()
    assert lens[0::2] == [len(s) for s, _ in case.reads1] and lens[1::2] == [len(s) for s, _ in case.reads2]


@pytest.mark.parametrize("name", list(ERRORS))
def test_error_flags(name):
    """One faulty record among good ones: exactly the expected bits, the flagged record empty, the others byte-exact,
    offsets non-decreasing, nothing written past the end."""
    case = ERRORS[name]
    recs, err = case.expected()
    assert err == case.bits and recs == generated(case)
    assert [i for i, r in enumerate(recs) if r == (b"", b"")] == case.bad
    off = parse_and_compare(case, recs, case.bits)
    assert np.all(np.diff(off.astype(np.int64)) >= 0)
    for slot in case.bad:
        assert off[slot + 1] == off[slot]


@pytest.fixture(scope="module")
def big_cases():
    return {c.name: c for c in fg.big_cases()}


@pytest.mark.parametrize("name,items", [("big_2048_items", 2048), ("big_2049_items", 2049), ("big_8_5_MiB", None)])
def test_newline_scan_second_tile(big_cases, name, items):
    """Blocks of 4,700-base records whose newline scan has groups + 1 = 2,048 items (one full tile), 2,049 (one item
    in a second tile) and about 2,180: the sums of the tiles before must reach every later tile's offsets."""
    case = big_cases[name]
    n_items = fg.nl_groups(0, len(case.raw1)) + 1
    if items is None:
        assert len(case.raw1) > 8.5 * 2 ** 20 and n_items > fg.SCAN_TILE + 100
    else:
        assert n_items == items
    assert (n_items + fg.SCAN_TILE - 1) // fg.SCAN_TILE == (1 if n_items <= fg.SCAN_TILE else 2)
    t0 = time.perf_counter()
    parse_and_compare(case, generated(case), 0)
    print(f"{name}: {len(case.raw1)} bytes, {case.n} records, {n_items} scan items, "
          f"{time.perf_counter() - t0:.2f} s for both parses and their comparison")
