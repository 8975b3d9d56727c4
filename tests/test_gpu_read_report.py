"""GPU: the per-unit report (speq_report_reads[_device], speq_report_fastq, `speq --group-sets`) against the exact
pure-Python model (tests/read_report_model.py; validated against the C oracle by tests/test_read_report_cpu.py).

The report is integers, so every comparison is exact: each unit's record and group set equal the model's, and the
report's sums equal what the scan kernels count on the same reads (T, sum of U[g], ambiguous units) and what the EM
histogram records (multi-group windows). Inputs (tests/read_report_inputs.py): synthetic reads plus hand-made ones at
the kernel's tile edges, for k below and at the index's q-mer length, across the packed / LDS search lengths and up
to SPEQ_REPORT_MAX_K; 70 groups (two set words); every index variant; the golden FASTQ cases, plain and gzip."""
import gzip
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import em_reference as er
import read_report_inputs as ri
import read_report_model as rm
from golden_io import CASES, Case
from speq_amd import DeviceIndex, EmHistogram, FmIndex, file_to_map

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")

VARIANTS = {
    "full": dict(pair_steps=True, triple_steps=True, label_table=True),
    "single_steps": dict(pair_steps=False, triple_steps=False, label_table=False),
    "pairs": dict(pair_steps=True, triple_steps=False, label_table=False),
    "pairs_label": dict(pair_steps=True, triple_steps=False, label_table=True),
    "triples_no_label": dict(pair_steps=True, triple_steps=True, label_table=False),
}


@lru_cache(maxsize=None)
def base_index(variant: str = "full") -> FmIndex:
    ref = ri.base_ref()
    return FmIndex.build(ref.records, ref.groups, 3, prefix_q=8, **VARIANTS[variant])


@lru_cache(maxsize=None)
def base_model(k: int, paired: bool) -> rm.Report:
    return rm.report(_base_dict(k), 3, k, *ri.base_reads(k), ri.CUTOFF, paired)


@lru_cache(maxsize=2)
def _base_dict(k: int) -> dict:
    ref = ri.base_ref()
    return er.build_index(ref.records, ref.groups, 3, k)


def assert_equal(got, exp: rm.Report):
    assert len(got.passing) == exp.n_units
    assert got.passing.tolist() == exp.passing
    assert got.unique.tolist() == exp.unique
    assert got.shared.tolist() == exp.shared
    assert got.first_group.tolist() == exp.first_group
    assert got.sets.shape == (exp.n_units, exp.W) and got.sets.dtype == np.uint64
    np.testing.assert_array_equal(got.sets, exp.words())
    assert [got.groups(u) for u in range(exp.n_units)] == exp.sets


def head(seq, qual, off, n):
    e = int(off[n])
    return seq[:e], qual[:e], off[:n + 1]


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("k", ri.KS)
def test_report_equals_the_model_and_the_scan_counters(k, paired):
    seq, qual, off = ri.base_reads(k)
    exp = base_model(k, paired)
    dev = DeviceIndex(base_index())
    got = dev.report(seq, qual, off, k=k, phred_cutoff=ri.CUTOFF, paired=paired)
    assert_equal(got, exp)
    if k >= 21:  # the hand-made chimeras and the split pair do what they were made for
        seqs, _ = ri.base_read_list(k)
        i = seqs.index(ri.chimera(k))
        if not paired:
            assert (got.groups(i), got.first_group[i]) == (frozenset({0, 2}), 0)
            assert (got.groups(i + 1), got.first_group[i + 1]) == (frozenset({0, 2}), 2)
            assert [len(got.groups(u)) for u in (len(seqs) - 2, len(seqs) - 1)] == [1, 1]
        else:
            u = ri.split_pair_unit(k)
            assert (got.groups(u), got.first_group[u]) == (frozenset({0, 1}), 0)
    # a few units alone (units are independent), and none
    per = 2 if paired else 1
    for n_units in (0, 1, 5):
        part = dev.report(*head(seq, qual, off, n_units * per), k=k, phred_cutoff=ri.CUTOFF, paired=paired)
        assert_equal(part, exp.head(n_units))
    # the scan kernels' counters on the same reads
    sc = dev.scan(seq, qual, off, k=k, phred_cutoff=ri.CUTOFF, paired=paired)
    assert int(got.passing.sum()) == sc.total
    assert int(got.unique.sum()) == int(sc.unique.sum())
    assert sum(len(got.groups(u)) >= 2 for u in range(exp.n_units)) == sc.ambiguous
    # the EM histogram's multi-group windows
    em = EmHistogram(dev)
    em.scan(seq, qual, off, k=k, phred_cutoff=ri.CUTOFF, paired=paired)
    em.finalize()
    assert int(got.shared.sum()) == em.info()[2]
    em.close()
    dev.close()


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_host_report_across_a_batch_edge(paired):
    """speq_report_reads stages at most 2^20 records per batch: 2^20 + 3 reads, or 2^20 + 4 as pairs (one pair starts
    exactly at the cut), of the base read set repeated end to end give the model's records and sets repeated the same
    way. The count is no multiple of the set's size, so a record sits at another place in every repeat."""
    k = 21
    n = (1 << 20) + (4 if paired else 3)
    seq, qual, off = ri.base_reads(k)
    n0 = len(off) - 1
    assert n0 % 2 == 0 and n % n0 != 0
    exp = base_model(k, paired)
    n_units = n // 2 if paired else n
    dev = DeviceIndex(base_index())
    got = dev.report(*ri.tiled(seq, qual, off, n), k=k, phred_cutoff=ri.CUTOFF, paired=paired)
    for name in ("passing", "unique", "shared", "first_group"):
        np.testing.assert_array_equal(getattr(got, name), np.resize(np.array(getattr(exp, name), np.int64), n_units),
                                      err_msg=name)
    np.testing.assert_array_equal(got.sets, np.resize(exp.words(), (n_units, exp.W)))
    dev.close()


def test_odd_paired_count_is_refused():
    from speq_amd import SpeqError
    dev = DeviceIndex(base_index())
    seq, qual, off = head(*ri.base_reads(21), 3)
    with pytest.raises(SpeqError) as e:
        dev.report(seq, qual, off, k=21, paired=True)
    assert e.value.code == -1
    with pytest.raises(SpeqError):
        dev.report(seq, qual, off, k=1025)
    dev.close()


def test_more_than_64_groups():
    records, groups = ri.many_ref()
    seq, qual, off = ri.many_reads()
    exp = rm.report(er.build_index(records, groups, 70, ri.MANY_K), 70, ri.MANY_K, seq, qual, off, ri.CUTOFF)
    idx = FmIndex.build(records, groups, 70, prefix_q=6, pair_steps=True, triple_steps=True, label_table=True)
    dev = DeviceIndex(idx)
    got = dev.report(seq, qual, off, k=ri.MANY_K, phred_cutoff=ri.CUTOFF)
    assert_equal(got, exp)
    assert got.sets.shape[1] == 2
    i = exp.sets.index(frozenset({63, 64}))
    assert got.sets[i].tolist() == [1 << 63, 1] and got.first_group[i] == 63
    for g in (0, 63, 64, 69):
        assert frozenset({g}) in [got.groups(u) for u in range(exp.n_units)]
    sc = dev.scan(seq, qual, off, k=ri.MANY_K, phred_cutoff=ri.CUTOFF)
    assert sum(len(s) >= 2 for s in exp.sets) == sc.ambiguous and int(got.unique.sum()) == int(sc.unique.sum())
    dev.close()


@pytest.mark.parametrize("variant", [v for v in VARIANTS if v != "full"])
def test_index_variants_give_equal_reports(variant):
    for k, paired in ((8, False), (21, True), (70, False)):
        seq, qual, off = ri.base_reads(k)
        dev = DeviceIndex(base_index(variant))
        assert_equal(dev.report(seq, qual, off, k=k, phred_cutoff=ri.CUTOFF, paired=paired), base_model(k, paired))
        dev.close()


@lru_cache(maxsize=None)
def golden_model(name: str, k: int) -> rm.Report:
    c = Case(name)
    return rm.report(er.build_index(c.records, c.groups, c.G, k), c.G, k, c.seq, c.qual, c.offsets, c.cutoff, c.paired)


def test_scattered_groups_reads():
    c = Case("scattered_groups")
    for label in (False, True):
        idx = FmIndex.build(c.records, c.groups, c.G, prefix_q=4, pair_steps=True, triple_steps=label,
                            label_table=label)
        dev = DeviceIndex(idx)
        for k in c.ks:
            got = dev.report(c.seq, c.qual, c.offsets, k=k, phred_cutoff=c.cutoff)
            assert_equal(got, golden_model(c.name, k))
        dev.close()


def _device_report(dev, seq, qual, off, k, paired, stream):
    """speq_report_reads_device on torch buffers one row longer than needed, pre-filled with 0xA5."""
    import torch
    n = len(off) - 1
    n_units = n // 2 if paired else n
    W = (dev.n_groups + 63) // 64
    d_seq = torch.from_numpy(np.frombuffer(seq, np.uint8).copy()).cuda()
    d_qual = torch.from_numpy(np.frombuffer(qual, np.uint8).copy()).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    rep = torch.full(((n_units + 1) * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    sets = torch.full(((n_units + 1) * W * 8,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    if stream is None:
        dev.report_device(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), n, k, rep.data_ptr(),
                          sets.data_ptr(), phred_cutoff=ri.CUTOFF, paired=paired)
        torch.cuda.synchronize()
    else:
        dev.report_device(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), n, k, rep.data_ptr(),
                          sets.data_ptr(), phred_cutoff=ri.CUTOFF, paired=paired, stream=stream.cuda_stream)
        stream.synchronize()
    r = rep.cpu().numpy()
    s = sets.cpu().numpy()
    assert (r[n_units * 16:] == 0xA5).all() and (s[n_units * W * 8:] == 0xA5).all(), "wrote past its rows"
    return r[:n_units * 16].view(np.uint32).reshape(n_units, 4), s[:n_units * W * 8].view(np.uint64).reshape(n_units, W)


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_device_entry_point_overwrites_its_rows_and_nothing_else(paired):
    import torch
    k = 21
    seq, qual, off = ri.base_reads(k)
    dev = DeviceIndex(base_index())
    host = dev.report(seq, qual, off, k=k, phred_cutoff=ri.CUTOFF, paired=paired)
    for stream in (None, torch.cuda.Stream()):
        rec, sets = _device_report(dev, seq, qual, off, k, paired, stream)
        first = rec[:, 3].astype(np.int64)
        first[first == 0xFFFFFFFF] = -1
        assert rec[:, 0].tolist() == host.passing.tolist() and rec[:, 1].tolist() == host.unique.tolist()
        assert rec[:, 2].tolist() == host.shared.tolist() and first.tolist() == host.first_group.tolist()
        np.testing.assert_array_equal(sets, host.sets)
    assert_equal(host, base_model(k, paired))
    dev.close()


def test_device_entry_point_two_set_words():
    records, groups = ri.many_ref()
    seq, qual, off = ri.many_reads()
    idx = FmIndex.build(records, groups, 70, prefix_q=6, pair_steps=True)
    dev = DeviceIndex(idx)
    host = dev.report(seq, qual, off, k=ri.MANY_K, phred_cutoff=ri.CUTOFF)
    rec, sets = _device_report(dev, seq, qual, off, ri.MANY_K, False, None)
    np.testing.assert_array_equal(sets, host.sets)
    assert rec[:, 1].tolist() == host.unique.tolist()
    dev.close()


@pytest.mark.parametrize("name", CASES)
def test_report_fastq_equals_the_model(name, tmp_path):
    c = Case(name)
    idx = FmIndex.build(c.records, c.groups, c.G, prefix_q=4, pair_steps=True, triple_steps=True, label_table=True)
    dev = DeviceIndex(idx)
    p1 = os.path.join(c.dir, "reads_1.fq")
    p2 = os.path.join(c.dir, "reads_2.fq") if c.paired else None
    k = c.ks[0]
    exp = golden_model(name, k)
    hist, totals = dev.report_fastq(p1, p2, k=k, phred_cutoff=c.cutoff, threads=3)
    assert hist == exp.histogram() and totals == exp.totals()
    assert list(hist.items()) == rm.sorted_sets(exp.histogram()), "entries ascending by the set as an integer"
    sc, _ = dev.scan_fastq(p1, p2, k=k, phred_cutoff=c.cutoff)
    assert sum(n for s, n in hist.items() if len(s) >= 2) == sc.ambiguous and totals["passing"] == sc.total
    # one gzip copy
    gz = []
    for p in (p1, p2):
        if p:
            gz.append(str(tmp_path / (os.path.basename(p) + ".gz")))
            with open(p, "rb") as f, gzip.open(gz[-1], "wb") as g:
                g.write(f.read())
    hist_gz, totals_gz = dev.report_fastq(gz[0], gz[1] if c.paired else None, k=k, phred_cutoff=c.cutoff, threads=2)
    assert hist_gz == hist and totals_gz == totals
    dev.close()


def test_cli_group_sets_file(tmp_path):
    """`speq all --group-sets FILE`: stderr and -o are byte-identical to a run without the option, and FILE holds the
    model's set histogram under the groupings file's names; its lines of two or more groups sum to the ambiguous
    count the run prints."""
    c = Case("tiny_paired")
    k = c.ks[0]
    outs = {}
    for tag in ("plain", "sets"):
        d = tmp_path / tag
        d.mkdir()
        for f in os.listdir(c.dir):
            shutil.copy(os.path.join(c.dir, f), d / f)
        args = ["all", "-r", "refs.fa", "-g", "groups.txt", "-1", "reads_1.fq", "-2", "reads_2.fq", "-x", "ref", "-k",
                str(k), "--phred-cutoff", str(c.cutoff), "--prefix-q", "4", "-o", "p.txt"]
        if tag == "sets":
            args += ["--group-sets", "sets.tsv"]
        r = subprocess.run([SPEQ] + args, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[tag] = (r.stderr, r.stdout, (d / "p.txt").read_bytes())
    assert outs["plain"] == outs["sets"]
    assert not (tmp_path / "plain" / "sets.tsv").exists()
    names = file_to_map(os.path.join(c.dir, "groups.txt")).names
    exp = golden_model(c.name, k)
    want = "".join(f"{n}\t{len(s)}\t{','.join(names[g] for g in sorted(s)) if s else '-'}\n"
                   for s, n in rm.sorted_sets(exp.histogram()))
    got = (tmp_path / "sets" / "sets.tsv").read_text()
    assert got == want
    amb = int([ln for ln in outs["sets"][0].split("\n") if "\t" in ln][0].split("\t")[1])
    assert sum(int(ln.split("\t")[0]) for ln in got.splitlines() if int(ln.split("\t")[1]) >= 2) == amb == exp.ambiguous


def test_cli_fusion_map_of_ambiguous_pairs(tmp_path):
    """Pairs that do hit two groups (the synthetic reads taken as mates): the lines of two or more groups sum to the
    ambiguous count on stderr, and the reference's degenerate fusion-map line is still printed beside them."""
    from speq_amd import synth
    k = 21
    ref = ri.base_ref()
    rd = synth.make_reads(ref, 2_000, n_rate=0.002, lowq_rate=0.01)
    exp = rm.report(_base_dict(k), 3, k, rd.seq, rd.qual, rd.offsets, ri.CUTOFF, paired=True)
    assert exp.ambiguous > 100
    (tmp_path / "refs.fa").write_text(ref.fasta_text())
    (tmp_path / "groups.txt").write_text(ref.groupings_text())
    for m in (0, 1):
        with open(tmp_path / f"reads_{m + 1}.fq", "w") as f:
            for i in range(m, rd.n, 2):
                f.write(rd.fastq_text(i, i + 1))
    r = subprocess.run([SPEQ, "all", "-r", "refs.fa", "-g", "groups.txt", "-1", "reads_1.fq", "-2", "reads_2.fq", "-x",
                        "ref", "-k", str(k), "--phred-cutoff", str(ri.CUTOFF), "--prefix-q", "8", "-o", "p.txt",
                        "--group-sets", "sets.tsv"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    names = ["V0", "V1", "V2"]
    want = "".join(f"{n}\t{len(s)}\t{','.join(names[g] for g in sorted(s)) if s else '-'}\n"
                   for s, n in rm.sorted_sets(exp.histogram()))
    got = (tmp_path / "sets.tsv").read_text()
    assert got == want
    lines = r.stderr.split("\n")
    tl = [ln for ln in lines if "\t" in ln][0]
    assert tl == f"{sum(exp.passing)}\t{exp.ambiguous}"
    assert lines[lines.index(tl) + 1] == f"[([],{exp.ambiguous})]"
    assert sum(int(ln.split("\t")[0]) for ln in got.splitlines() if int(ln.split("\t")[1]) >= 2) == exp.ambiguous
