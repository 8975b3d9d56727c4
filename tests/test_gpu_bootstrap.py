"""GPU: the read bootstrap (speq_bootstrap_*, `speq scan --bootstrap`) against the pure-Python model
(tests/bootstrap_model.py; validated against the C oracle by tests/test_bootstrap_cpu.py).

The counts are integers, so every comparison of them is exact equality with the model. The local weights are compared
within (3 k + n + 2) 2^-53 relative, n the windows that contribute to the cell: 3 k 2^-53 is the project's per-window
bound of the scan's Phred weight (tests/test_gpu_ax.py), n + 2 the first-order bound of rounding w x and summing n
positive terms in any order. Inputs: tests/read_report_inputs.py (empty reads, reads shorter than k, tile edges at
63 / 64, a pair with an empty mate, chimeras, a pair ambiguous only as a pair; 70 groups), and the golden FASTQ cases
through the CLI."""
import gzip
import os
import shutil
import subprocess
from functools import lru_cache

import numpy as np
import pytest

import bootstrap_model as bm
import em_reference as er
import read_report_inputs as ri
from golden_io import Case
from oracle.oracle import Oracle
from speq_amd import Bootstrap, DeviceIndex, FmIndex, file_to_map

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")
FULL = dict(pair_steps=True, triple_steps=True, label_table=True)
BS = [1, 63, 64, 65, 129]  # both sides of every 64-lane stride over the B + 1 rows
SEED = 7

# the accumulation path as include/speq_scan.h and DESIGN.md §4p state it: a block's (B + 1)(G + 2) u64 cells, plus
# (B + 1) G f64 cells in local mode, go to LDS when they fit 64 KiB together with the tile search's four wave regions
LDS_BUDGET = 64 << 10


def takes_lds(B: int, G: int, local: bool, k: int) -> bool:
    wave_bytes = (3 * (64 + k) + 15) & ~15
    return 8 * (B + 1) * (G + 2 + (G if local else 0)) + 4 * wave_bytes <= LDS_BUDGET


# ---- inputs, model, comparison ----
@lru_cache(maxsize=None)
def base_index() -> FmIndex:
    ref = ri.base_ref()
    return FmIndex.build(ref.records, ref.groups, 3, prefix_q=8, **FULL)


@pytest.fixture(scope="module")
def dev():
    d = DeviceIndex(base_index())
    yield d
    d.close()


@lru_cache(maxsize=None)
def base_units(k: int, paired: bool) -> bm.Units:
    ref = ri.base_ref()
    return bm.units(er.build_index(ref.records, ref.groups, 3, k), 3, k, *ri.base_reads(k), ri.CUTOFF, paired, True)


def model(un: bm.Units, B: int, local: bool, seed: int = SEED, first_unit: int = 0, n_total: int = None):
    counts, w = bm.replicates(un, seed, B, first_unit, n_total)
    return counts, (w if local else None)


def assert_equal(got, exp, k: int):
    (gc, gw), (ec, ew) = got, exp
    assert gc.dtype == np.uint64 and gc.shape == ec.shape
    np.testing.assert_array_equal(gc, ec)
    assert (gw is None) == (ew is None)
    if ew is not None:
        assert gw.shape == ew.shape
        err = np.abs(gw - ew)
        tol = bm.weights_bound(k, ec) * ew
        assert (err <= tol).all(), (float((err / np.maximum(ew, 1e-300)).max()), float(bm.weights_bound(k, ec).min()))


def run(dev, k, reads, B, paired, local, seed=SEED, first_unit=0):
    b = Bootstrap(dev, k, B, seed, ri.CUTOFF, paired, local)
    b.add(*reads, first_unit)
    out, info = b.finalize(), b.info()
    b.close()
    return out, info


def _to_device(reads):
    import torch
    seq, qual, off = reads
    return (torch.from_numpy(np.frombuffer(seq, np.uint8).copy()).cuda(),
            torch.from_numpy(np.frombuffer(qual, np.uint8).copy()).cuda(),
            torch.from_numpy(np.asarray(off).astype(np.int64)).cuda())


def _split(reads, n0: int, n1: int):
    seq, qual, off = reads
    a, b = int(off[n0]), int(off[n1])
    return seq[a:b], qual[a:b], off[n0:n1 + 1] - off[n0]


# ---- the base input ----
@pytest.mark.parametrize("local", [False, True], ids=["global", "local"])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("k", [8, 21, 70, 151])
def test_base_reads_equal_the_model_and_row_0_the_scan(dev, k, paired, local):
    reads = ri.base_reads(k)
    un = base_units(k, paired)
    sc = dev.scan(*reads, k=k, phred_cutoff=ri.CUTOFF, paired=paired, local=local)
    for B in BS:
        got, info = run(dev, k, reads, B, paired, local)
        assert_equal(got, model(un, B, local), k)
        assert info == {"replicates": B, "lds_path": takes_lds(B, 3, local, k), "units_added": un.n}
        counts, w = got
        assert counts[0].tolist() == [sc.total, sc.ambiguous] + sc.unique.tolist()
        if local:  # two sums of the same windows' weights
            tol = bm.weights_bound(k, counts)[0]
            assert (np.abs(w[0] - sc.weights) <= tol * sc.weights).all()
    if k == 21:
        assert counts[0, 1] > 0 and (counts[0, 2:] > 0).all() and (counts[1:] != counts[0]).any()


def test_70_groups():
    records, groups = ri.many_ref()
    reads = ri.many_reads()
    k = ri.MANY_K
    un = bm.units(er.build_index(records, groups, 70, k), 70, k, *reads, ri.CUTOFF, False, True)
    d = DeviceIndex(FmIndex.build(records, groups, 70, prefix_q=8, **FULL))
    for local in (False, True):
        got, info = run(d, k, reads, 65, False, local)
        assert_equal(got, model(un, 65, local), k)
        assert info["lds_path"] == takes_lds(65, 70, local, k) == (not local)
    assert np.flatnonzero(got[0][0, 2:]).tolist() == [0, 1, 33, 63, 64, 65, 69]
    # B = 1024 cannot fit LDS: device atomics throughout
    assert not takes_lds(1024, 70, False, k)
    got, info = run(d, k, reads, 1024, False, False)
    assert_equal(got, model(un, 1024, False), k)
    assert info["lds_path"] is False
    d.close()


def test_both_accumulation_paths_by_shape(dev):
    k = 21
    reads = ri.base_reads(k)
    un = base_units(k, False)
    assert takes_lds(3, 3, True, k)
    got, info = run(dev, k, reads, 3, False, True)
    assert_equal(got, model(un, 3, True), k)
    assert info["lds_path"] is True
    # B = 1024, local: 1025 * 8 * 8 bytes do not fit beside the tile search
    assert not takes_lds(1024, 3, True, k)
    got, info = run(dev, k, reads, 1024, False, True)
    assert_equal(got, model(un, 1024, True), k)
    assert info["lds_path"] is False


def test_the_lds_limit_at_k_1024(dev):
    """At k = 1024 the tile search takes 4 * 3,264 = 13,056 bytes, which leaves 52,480 for the accumulators: in local
    mode with G = 3 a row of (5 + 3) cells is 64 bytes, so 820 rows, B = 819, is the most LDS takes."""
    k = 1024
    assert takes_lds(819, 3, True, k) and not takes_lds(820, 3, True, k)
    reads = ri.base_reads(k)
    un = base_units(k, False)
    assert un.c.sum() > 0
    for B, lds in ((819, True), (820, False)):
        got, info = run(dev, k, reads, B, False, True)
        assert_equal(got, model(un, B, True), k)
        assert info["lds_path"] is lds


# ---- unit indices ----
def test_first_unit(dev):
    import torch
    k, B = 21, 65
    reads = ri.base_reads(k)
    n = len(reads[2]) - 1
    for paired in (False, True):
        un = base_units(k, paired)
        per = 2 if paired else 1
        cut_unit = 777  # an odd unit
        whole = _to_device(reads)
        parts = [_to_device(_split(reads, 0, cut_unit * per)), _to_device(_split(reads, cut_unit * per, n))]
        torch.cuda.synchronize()
        one = Bootstrap(dev, k, B, SEED, ri.CUTOFF, paired, True)
        one.add_device(whole[0].data_ptr(), whole[1].data_ptr(), whole[2].data_ptr(), n)
        a = one.finalize()
        two = Bootstrap(dev, k, B, SEED, ri.CUTOFF, paired, True)
        for (s, q, o), first in zip(parts, (0, cut_unit)):
            two.add_device(s.data_ptr(), q.data_ptr(), o.data_ptr(), len(o) - 1, first_unit=first)
        b = two.finalize()
        exp = model(un, B, True)
        assert_equal(a, exp, k)
        assert_equal(b, exp, k)
        np.testing.assert_array_equal(a[0], b[0])
        assert one.info()["units_added"] == two.info()["units_added"] == un.n
        # the second part at first_unit 0 draws other weights
        wrong = Bootstrap(dev, k, B, SEED, ri.CUTOFF, paired, False)
        for s, q, o in parts:
            wrong.add_device(s.data_ptr(), q.data_ptr(), o.data_ptr(), len(o) - 1)
        assert (wrong.finalize()[0] != exp[0]).any()
        for h in (one, two, wrong):
            h.close()
        # an index past 2^32 (a 32-bit unit index would wrap to 5)
        big = (1 << 40) + 5
        got, _ = run(dev, k, reads, B, paired, False, first_unit=big)
        assert_equal(got, model(un, B, False, first_unit=big), k)
        assert (got[0] != model(un, B, False, first_unit=5)[0]).any()


def test_host_add_equals_device_add_and_seeds(dev):
    import torch
    k, B = 21, 64
    reads = ri.base_reads(k)
    n = len(reads[2]) - 1
    un = base_units(k, True)
    host, _ = run(dev, k, reads, B, True, True)
    d_reads = _to_device(reads)
    torch.cuda.synchronize()
    b = Bootstrap(dev, k, B, SEED, ri.CUTOFF, True, True)
    b.add_device(d_reads[0].data_ptr(), d_reads[1].data_ptr(), d_reads[2].data_ptr(), n)
    device = b.finalize()
    b.close()
    np.testing.assert_array_equal(host[0], device[0])
    assert_equal(host, model(un, B, True), k)
    assert_equal(device, model(un, B, True), k)
    again, _ = run(dev, k, reads, B, True, False)
    other, _ = run(dev, k, reads, B, True, False, seed=SEED + 1)
    np.testing.assert_array_equal(again[0], host[0])
    np.testing.assert_array_equal(other[0][0], host[0][0])  # the sample itself does not depend on the seed
    assert (other[0][1:] != host[0][1:]).any()
    assert_equal(other, model(un, B, False, seed=SEED + 1), k)


def test_finalize_twice_with_an_add_in_between_and_no_reads(dev):
    k, B = 21, 65
    reads = ri.base_reads(k)
    n = len(reads[2]) - 1
    un = base_units(k, False)
    half = n // 2 + 1
    b = Bootstrap(dev, k, B, SEED, ri.CUTOFF, False, True)
    # 0 reads: nothing is launched, finalize returns zeros
    b.add(b"", b"", np.zeros(1, dtype=np.uint64))
    b.add_device(0, 0, 0, 0)
    counts, w = b.finalize()
    assert not counts.any() and not w.any() and b.info()["units_added"] == 0
    b.add(*_split(reads, 0, half))
    first = b.finalize()
    head = bm.Units(3, un.P[:half], un.amb[:half], un.c[:half], un.x[:half])
    assert_equal(first, model(head, B, True), k)
    b.add(*_split(reads, half, n), first_unit=half)
    assert_equal(b.finalize(), model(un, B, True), k)
    assert b.info()["units_added"] == n
    b.close()


# ---- files ----
def _write_fastq(path, seq, qual, off, start: int, step: int):
    with open(path, "wb") as f:
        f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (i, seq[int(off[i]):int(off[i + 1])], qual[int(off[i]):int(off[i + 1])])
                         for i in range(start, len(off) - 1, step)))


def test_fastq_equals_the_model_for_any_thread_count(dev, tmp_path):
    """70,000 records: more than two of the reader's 32,768-record blocks, so a block's first record index matters."""
    k, B, n = 21, 65, 70_000
    seq, qual, off = ri.tiled(*ri.base_reads(k), n)
    single = str(tmp_path / "reads.fq")
    _write_fastq(single, seq, qual, off, 0, 1)
    exp = model(base_units(k, False), B, True, n_total=n)
    for threads in (1, 4):
        got = dev.bootstrap_fastq(single, None, k=k, replicates=B, seed=SEED, phred_cutoff=ri.CUTOFF, local=True,
                                  threads=threads)
        assert_equal(got, exp, k)
    gz = single + ".gz"
    with open(single, "rb") as f, gzip.open(gz, "wb", compresslevel=1) as g:
        g.write(f.read())
    got = dev.bootstrap_fastq(gz, None, k=k, replicates=B, seed=SEED, phred_cutoff=ri.CUTOFF, local=True, threads=3)
    assert_equal(got, exp, k)
    # two files: records 2i and 2i + 1 are mates
    p1, p2 = str(tmp_path / "reads_1.fq"), str(tmp_path / "reads_2.fq")
    _write_fastq(p1, seq, qual, off, 0, 2)
    _write_fastq(p2, seq, qual, off, 1, 2)
    assert base_units(k, True).n * 2 == len(ri.base_reads(k)[2]) - 1
    exp = model(base_units(k, True), B, False, n_total=n // 2)
    for threads in (1, 4):
        got = dev.bootstrap_fastq(p1, p2, k=k, replicates=B, seed=SEED, phred_cutoff=ri.CUTOFF, threads=threads)
        assert_equal(got, exp, k)
    # the host add of the same records, first_unit = 0
    host, _ = run(dev, k, (seq, qual, off), B, True, False)
    np.testing.assert_array_equal(host[0], exp[0])


@pytest.mark.parametrize("name,accuracy", [("tiny_single", None), ("tiny_paired", "0.99")])
def test_cli_bootstrap_file(name, accuracy, tmp_path):
    """`speq all --bootstrap FILE`: stderr, stdout and -o are byte-identical to a run without the option, and FILE is
    the model's table: every number within 1e-6 of the model's value (the print precision)."""
    c = Case(name)
    k = c.ks[0]
    local = accuracy is None
    outs = {}
    for tag in ("plain", "bootstrap"):
        d = tmp_path / tag
        d.mkdir()
        for f in os.listdir(c.dir):
            shutil.copy(os.path.join(c.dir, f), d / f)
        args = ["all", "-r", "refs.fa", "-g", "groups.txt", "-1", "reads_1.fq"]
        if c.paired:
            args += ["-2", "reads_2.fq"]
        args += ["-x", "ref", "-k", str(k), "--phred-cutoff", str(c.cutoff), "--prefix-q", "4", "-o", "p.txt"]
        if accuracy:
            args += ["--fixed-accuracy", accuracy]
        if tag == "bootstrap":
            args += ["--bootstrap", "ci.tsv", "--bootstrap-replicates", "64", "--bootstrap-seed", "7"]
        r = subprocess.run([SPEQ] + args, cwd=d, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        outs[tag] = (r.stderr, r.stdout, (d / "p.txt").read_bytes())
    assert outs["plain"] == outs["bootstrap"]
    assert not (tmp_path / "plain" / "ci.tsv").exists()
    un = bm.units(er.build_index(c.records, c.groups, c.G, k), c.G, k, c.seq, c.qual, c.offsets, c.cutoff, c.paired,
                  local)
    counts, w = bm.replicates(un, 7, 64)
    u_ref, tot_ref = Oracle(c.records, c.groups, c.G, k).ref_unique()
    cis = bm.summary(counts, w, u_ref, tot_ref, 1.0 if local else 1.0 / float(accuracy) ** k, 0.95)
    names = file_to_map(os.path.join(c.dir, "groups.txt")).names
    got = (tmp_path / "bootstrap" / "ci.tsv").read_text().splitlines(keepends=True)
    assert got[0] == bm.HEADER and len(got) == c.G + 1
    assert any(ci["se"] > 0 for ci in cis)
    for line, nm, ci in zip(got[1:], names, cis):
        f = line.rstrip("\n").split("\t")
        assert len(f) == 7 and f[0] == nm and int(f[6]) == ci["used"] == 64
        for text, key in zip(f[1:6], ("estimate", "mean", "se", "lo", "hi")):
            assert len(text.split(".")[1]) == 6 and abs(float(text) - ci[key]) <= 1e-6, (nm, key, text, ci[key])
