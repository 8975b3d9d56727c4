"""GPU: every window path for k above 128 against the oracle (inputs: tests/big_k_inputs.py; their properties:
tests/test_big_k_cpu.py).

The scan entry points take k up to 4096, the report and marker passes up to 1024; past the anchor kernel's 128 a scan
is k_scan with LF steps (search_lds over the bases staged in LDS). For every k of big_k_inputs.KS:

  dispatch   "last_kernel" is 0 and "last_variant" is the k_scan instantiation tests/variant_table.py predicts;
  counters   T, the ambiguous units and U[g] equal the C oracle exactly and W[g] is within (3k + 2 n_g + 2) * 2^-53
             relative (the bound of tests/test_gpu_variants.py), over {global, local} x {single, paired} x "ilp" =
             "ilp_local" in {1, 2}, on a 3-group replica (the tally in LDS) and on a 2049-group one (global atomics),
             and once more as four waves ("grid_blocks" 1), where a wave holds the runs of 70 reads of k and of k - 1
             bases whole;
  the pass   count_unique_kmers_per_group and the sum of its shards equal Oracle.ref_unique();
  prefixes   the first 0, 1 and 71 units scanned alone give the oracle's counts for them.

At k = 129, 1024 and 4096 also: the index variants (single, pair and triple steps, with and without the label table,
prefix_q 0 and 8) and the EM rows against tests/em_reference.py. At 1024 the FASTQ stream and the pipeline; at 129 the
CLI; at 4096 the largest LDS request (local, G = 2048, "ilp_kt" 4: 120,960 B); and the limits of k at every entry point.

Not here: a window weight that passes DBL_MAX (k = 1024 at quality 3, k = 4096 at quality 7: big_k_inputs.OVERFLOW, which
tests/test_big_k_cpu.py confirms with the oracle). The oracle gives +inf there and k_scan gives NaN (div_rn's residual
is inf - inf); neither the correction nor its test is part of this file yet.

Every test is parametrised in increasing k and its ids name the k."""
import gzip
import os
import subprocess
from collections import Counter
from itertools import product

import numpy as np
import pytest

import big_k_inputs as bk
import variant_table as vt
from speq_amd import DeviceIndex, EmHistogram, FmIndex, Markers, Pipeline, SpeqError, unique_to_percent
from speq_amd._lib import SPEQ_E_ARG

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPEQ = os.path.join(ROOT, "bin", "speq")
FULL = dict(prefix_q=8, pair_steps=True, triple_steps=True)   # the build of tests/test_gpu_variants.py's replicas
OBSERVED: set = set()   # (k, instantiation) of every launch checked here


@pytest.fixture(scope="module")
def replica():
    """(k, G, build options) -> a replica of reference(k) under the labels of G groups; those of one k at a time."""
    made = {}

    def get(k: int, G: int = 3, **build) -> DeviceIndex:
        build = build or FULL
        key = (k, G, tuple(sorted(build.items())))
        for other in [x for x in made if x[0] != k]:
            made.pop(other).close()
        if key not in made:
            made[key] = DeviceIndex(FmIndex.build(bk.reference(k).records, bk.groups_of(k, G), G, **build))
        made[key].tune(**vt.DEFAULTS)
        return made[key]

    yield get
    for dev in made.values():
        dev.close()


def recipe(k, G, paired, local, entry, **tune) -> vt.Recipe:
    return vt.Recipe(f"big{G}", k, paired, local, entry, tuple(tune.items()))


def dispatched(dev: DeviceIndex, r: vt.Recipe) -> vt.Variant:
    """The last launch was k_scan with LF steps, in the instantiation the table predicts for r."""
    dev_kernel, got, exp = dev.tuning("last_kernel"), vt.unpack(dev.tuning("last_variant")), vt.predict(r)
    # ("last_kernel" is the last read scan's: the pass leaves it as it was, -1 on a fresh replica)
    assert dev_kernel in ((-1, 0) if r.entry == vt.REF else (0,)), f"{r.id}: last_kernel {dev_kernel}"
    assert got == exp, f"{r.id}: launched {got}, the table predicts {exp}"
    t = dict(vt.DEFAULTS, **dict(r.tune))
    width = 1 if r.entry == vt.EM else 2 if t["ilp_local" if r.local else "ilp"] >= 2 else 1
    mode = "ref" if r.entry == vt.REF else "local" if r.local else "global"
    assert got == vt.Variant(vt.K_SCAN, mode, r.paired, vt.BIG_K_REFS[r.ref].G <= 2048, r.entry == vt.EM, width), r.id
    OBSERVED.add((r.k, got))
    return got


def check_counters(tag, k, G, paired, local, got, n_reads=-1):
    T, amb, Uo, Wo = bk.oracle_scan(k, G, paired, local, n_reads)
    assert got.total == T, f"{tag}: T {got.total} != {T}"
    assert got.ambiguous == amb, f"{tag}: ambiguous {got.ambiguous} != {amb}"
    bad = np.flatnonzero(np.asarray(got.unique, dtype=np.uint64) != Uo)
    assert bad.size == 0, f"{tag}: U differs at groups {bad[:8].tolist()}: {got.unique[bad[:8]]} != {Uo[bad[:8]]}"
    if local:
        check_weights(tag, k, got.weights, Uo, Wo)


def check_weights(tag, k, W, Uo, Wo):
    assert not np.isnan(W).any(), f"{tag}: NaN in W: {W[np.isnan(W)][:8]}"
    tol = (3 * k + 2 * Uo.astype(np.float64) + 2) * U53 * Wo
    off = np.flatnonzero(~(np.abs(W - Wo) <= tol))
    assert off.size == 0, f"{tag}: W out of bound at groups {off[:8].tolist()}: {W[off[:8]]} vs {Wo[off[:8]]}"


def scan(dev, rd, k, paired, local, cutoff=bk.CUTOFF):
    return dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, phred_cutoff=cutoff, paired=paired,
                    local=local)


KG = [(k, G) for k in bk.KS for G in (3, 2049)]


@pytest.mark.parametrize("k,G", KG, ids=[f"k{k}-g{G}" for k, G in KG])
def test_scan_matrix_equals_the_oracle(k, G, replica):
    dev, rd = replica(k, G), bk.reads(k)
    for local, paired, ilp in product((False, True), (False, True), (1, 2)):
        dev.tune(ilp=ilp, ilp_local=ilp)
        r = recipe(k, G, paired, local, vt.SCAN, ilp=ilp, ilp_local=ilp)
        got = scan(dev, rd, k, paired, local)
        v = dispatched(dev, r)
        check_counters(f"{r.id} [{v}]", k, G, paired, local, got)


@pytest.mark.parametrize("k,G", KG, ids=[f"k{k}-g{G}" for k, G in KG])
def test_scan_as_four_waves_equals_the_oracle(k, G, replica):
    """A scan gives a wave four units or so; with "grid_blocks" 1 it is four waves of a quarter of the units each:
    the first holds the 70 reads of k bases whole (two or three of them fit a pass), the last the 70 reads of k - 1
    bases (the skip of 64 reads without a window) and the read after them."""
    dev, rd = replica(k, G), bk.reads(k)
    before = dev.tuning("grid_blocks")
    try:
        dev.tune(grid_blocks=1)
        for local, paired, ilp in ((True, False, 1), (True, True, 2), (False, True, 1), (False, False, 2)):
            dev.tune(ilp=ilp, ilp_local=ilp)
            r = recipe(k, G, paired, local, vt.SCAN, ilp=ilp, ilp_local=ilp)
            got = scan(dev, rd, k, paired, local)
            v = dispatched(dev, r)
            check_counters(f"{r.id} four waves [{v}]", k, G, paired, local, got)
    finally:
        dev.tune(grid_blocks=before)


@pytest.mark.parametrize("k,G", KG, ids=[f"k{k}-g{G}" for k, G in KG])
def test_reference_pass_equals_the_oracle(k, G, replica):
    dev = replica(k, G)
    ou, ot = bk.ref_unique(k, G)
    for ilp in (1, 2):
        dev.tune(ilp=ilp)
        r = recipe(k, G, False, False, vt.REF, ilp=ilp)
        u, t = dev.count_unique_kmers_per_group(k)
        v = dispatched(dev, r)
        assert np.array_equal(u, ou) and np.array_equal(t, ot), f"{r.id} [{v}]: (U_ref, Tot_ref) differ"
        for n_shards in (1, 3):
            parts = [dev.count_unique_kmers_per_group_shard(k, s, n_shards) for s in range(n_shards)]
            dispatched(dev, r)
            assert np.array_equal(sum(p[0] for p in parts), ou), f"{r.id}: U_ref of {n_shards} shards"
            assert np.array_equal(sum(p[1] for p in parts), ot), f"{r.id}: Tot_ref of {n_shards} shards"


@pytest.mark.parametrize("k", bk.KS, ids=[f"k{k}" for k in bk.KS])
def test_prefixes_scanned_alone_equal_the_oracle(k, replica):
    """0, 1 and 71 units (reads; then pairs): 71 reads of k bases are 71 units with one window each."""
    dev, rd = replica(k), bk.reads(k)
    for paired, local in ((False, True), (True, False)):
        for units in (0, 1, bk.RUN + 1):
            n = units * (2 if paired else 1)
            got = scan(dev, rd.prefix(n), k, paired, local)
            if units:
                dispatched(dev, recipe(k, 3, paired, local, vt.SCAN))
            check_counters(f"k {k} first {units} units paired {paired}", k, 3, paired, local, got, n)


STEPS = {"single": dict(), "pairs": dict(pair_steps=True), "triples": dict(pair_steps=True, triple_steps=True)}
KS_STEPS = [(k, s) for k in bk.K_EM for s in STEPS]


@pytest.mark.parametrize("k,steps", KS_STEPS, ids=[f"k{k}-{s}" for k, s in KS_STEPS])
def test_index_variants_equal_the_oracle(k, steps, replica):
    """search_lds takes another road per index: one, two or three symbols per step, the label table or the run
    bitvector, the q-mer prefix table or none."""
    rd = bk.reads(k)
    ou, ot = bk.ref_unique(k, 3)
    for label, q in product((False, True), (0, 8)):
        dev = replica(k, 3, prefix_q=q, label_table=label, **STEPS[steps])
        tag = f"k {k} {steps} label {label} prefix_q {q}"
        for local in (False, True):
            got = scan(dev, rd, k, False, local)
            dispatched(dev, recipe(k, 3, False, local, vt.SCAN))
            check_counters(tag, k, 3, False, local, got)
        u, t = dev.count_unique_kmers_per_group(k)
        dispatched(dev, recipe(k, 3, False, False, vt.REF))
        assert np.array_equal(u, ou) and np.array_equal(t, ot), tag


KP = [(k, p) for k in bk.K_EM for p in (False, True)]


@pytest.mark.parametrize("k,paired", KP, ids=[f"k{k}-{'pe' if p else 'se'}" for k, p in KP])
def test_em_rows_equal_the_exact_reference(k, paired, replica, monkeypatch):
    dev, rd, h = replica(k), bk.reads(k), bk.histogram(k, paired)
    # one row per interval (global mode), then merged (the default; local mode)
    for local, merge in ((False, False), (True, True)):
        if merge:
            monkeypatch.delenv("SPEQ_EM_MERGE_ROWS", raising=False)
        else:
            monkeypatch.setenv("SPEQ_EM_MERGE_ROWS", "0")
        em = EmHistogram(dev)
        got = em.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, phred_cutoff=bk.CUTOFF, paired=paired,
                      local=local)
        v = dispatched(dev, recipe(k, 3, paired, local, vt.EM))
        check_counters(f"EM k {k} [{v}]", k, 3, paired, local, got)
        em.finalize()
        assert em.info() == (h.n_intervals, h.n_entries, h.n_windows)
        rows = em.rows()
        assert all(len(c) >= 2 and [g for g, _ in c] == sorted({g for g, _ in c}) for _, c in rows)
        if merge:
            assert len({c for _, c in rows}) == len(rows), "equal rows left unmerged"
            assert {c: m for m, c in rows} == h.merged
        else:
            assert Counter((c, m) for m, c in rows) == h.unmerged
        em.close()


def test_largest_lds_request_k4096_local_2048_groups(replica):
    """k = 4096, local, G = 2048 (the last G with the tally in LDS), "ilp_kt" 4 (the widest staging buffer): 120,960 B
    of dynamic LDS (tests/test_big_k_cpu.py works the figure out)."""
    k, G = 4096, 2048
    dev, rd = replica(k, G), bk.reads(k)
    for paired, ilp in ((False, 2), (True, 1)):
        dev.tune(ilp_kt=4, ilp_local=ilp)
        r = recipe(k, G, paired, True, vt.SCAN, ilp_kt=4, ilp_local=ilp)
        got = scan(dev, rd, k, paired, True)
        v = dispatched(dev, r)
        check_counters(f"{r.id} [{v}]", k, G, paired, True, got)


# ---------------------------------------------------------------- files, the pipeline, the CLI
def write_fastq(path, seqs, quals, gz):
    data = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, s, q) for i, (s, q) in enumerate(zip(seqs, quals)))
    with (gzip.open(path, "wb", compresslevel=1) if gz else open(path, "wb")) as f:
        f.write(data)


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_files_and_pipeline_equal_the_in_memory_scan_k1024(paired, replica, tmp_path):
    k = 1024
    dev, rd = replica(k), bk.reads(k)
    seqs, quals = bk.read_list(k)
    for local in (False, True):
        mem = scan(dev, rd, k, paired, local)
        check_counters(f"k {k} in memory", k, 3, paired, local, mem)
        for gz in (False, True):
            ext = ".fq.gz" if gz else ".fq"
            p1, p2 = str(tmp_path / ("r1" + ext)), str(tmp_path / ("r2" + ext)) if paired else None
            if paired:
                write_fastq(p1, seqs[0::2], quals[0::2], gz)
                write_fastq(p2, seqs[1::2], quals[1::2], gz)
            else:
                write_fastq(p1, seqs, quals, gz)
            got, st = dev.scan_fastq(p1, p2, k=k, phred_cutoff=bk.CUTOFF, local=local, threads=2)
            dispatched(dev, recipe(k, 3, paired, local, vt.SCAN))
            assert (st["records"], st["bases"]) == (rd.n, int(rd.offsets[-1]))
            assert (got.total, got.ambiguous, got.unique.tolist()) == (mem.total, mem.ambiguous, mem.unique.tolist())
            check_counters(f"k {k} scan_fastq gz {gz}", k, 3, paired, local, got)
        pl = Pipeline(dev, k=k, phred_cutoff=bk.CUTOFF, paired=paired, local=local, slot_bytes=64 << 10,
                      slot_records=256, n_slots=3)
        seq, qual = rd.seq.tobytes(), rd.qual.tobytes()
        cuts = [0, 2, 100, rd.n]   # (the last slot holds more bytes than a slot has: it grows)
        for a, b in zip(cuts, cuts[1:]):
            pl.put(seq, qual, rd.offsets[a:b + 1])
        got = pl.finish()
        pl.close()
        dispatched(dev, recipe(k, 3, paired, local, vt.SCAN))
        assert (got.total, got.ambiguous, got.unique.tolist()) == (mem.total, mem.ambiguous, mem.unique.tolist())
        check_counters(f"k {k} pipeline", k, 3, paired, local, got)


def _parse_vec(line):
    assert line.startswith("[") and line.endswith("]"), line
    return [float(x) for x in line[1:-1].split(",")] if line[1:-1] else []


@pytest.mark.parametrize("mode", ["global", "local"])
def test_cli_scan_k129_prints_the_api_percentages(mode, replica, tmp_path):
    k, acc = 129, 0.99
    dev, rd = replica(k), bk.reads(k)
    (tmp_path / "refs.fa").write_text(bk.fasta_text(k))
    (tmp_path / "groups.txt").write_text(bk.groupings_text(k))
    write_fastq(tmp_path / "r1.fq", *bk.read_list(k), gz=False)

    def run(args):
        return subprocess.run([SPEQ] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)

    r = run(["index", "-r", "refs.fa", "-g", "groups.txt", "-x", "ref", "-o", "i.txt"])
    assert r.returncode == 0, r.stderr
    args = ["scan", "-1", "r1.fq", "-x", "ref", "-k", str(k), "--phred-cutoff", str(bk.CUTOFF), "-o", "p.txt"]
    r = run(args + (["--fixed-accuracy", str(acc)] if mode == "global" else []))
    assert r.returncode == 0, r.stderr
    lines = r.stderr.strip().split("\n")
    u_ref, t_ref = dev.count_unique_kmers_per_group(k)
    assert np.array_equal(u_ref, bk.ref_unique(k, 3)[0])
    assert _parse_vec(lines[0]) == u_ref.tolist() and _parse_vec(lines[1]) == t_ref.tolist()
    api = scan(dev, rd, k, False, mode == "local")
    ut = api.weights if mode == "local" else [u / acc ** k for u in api.unique]
    np.testing.assert_allclose(_parse_vec(lines[2]), unique_to_percent(ut, api.total, u_ref, t_ref), rtol=1e-5)
    assert [ln for ln in lines if "\t" in ln][0] == f"{api.total}\t{api.ambiguous}"
    assert api.total == bk.oracle_scan3(k, False, False)[0]


# ---------------------------------------------------------------- the limits of k
def test_limits_of_k(replica):
    import torch
    k = 1025
    dev, rd = replica(k), bk.reads(k)
    seq, qual = rd.seq.tobytes(), rd.qual.tobytes()
    d_seq, d_qual = torch.from_numpy(rd.seq.copy()).cuda(), torch.from_numpy(rd.qual.copy()).cuda()
    d_off = torch.from_numpy(rd.offsets.astype(np.int64)).cuda()
    cnt = torch.zeros(5, dtype=torch.int64, device="cuda")

    def refused(call, *a, code=SPEQ_E_ARG, **kw):
        with pytest.raises(SpeqError, match=r"k must be in \[1, 4096\]") as e:
            call(*a, **kw)
        assert code is None or e.value.code == code

    before = dev.tuning("last_variant")
    # (speq_scan_reads and speq_ref_unique hand on an inner call's refusal, message and all, but as SPEQ_E_DEVICE:
    # the code of these two is not asserted until they check k themselves)
    refused(dev.scan, seq, qual, rd.offsets, k=4097, code=None)
    refused(dev.scan_device, d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), rd.n, 4097, cnt.data_ptr())
    refused(dev.count_unique_kmers_per_group, 4097, code=None)
    refused(dev.count_unique_kmers_per_group_shard, 4097, 0, 1)
    refused(dev.prepare, 0)
    refused(dev.prepare, 4097)
    torch.cuda.synchronize()
    assert not cnt.any().item() and dev.tuning("last_variant") == before, "a refused call launched a scan"
    # 1025 scans (the matrix above checks it in full); the report and the marker pass stop at 1024
    got = scan(dev, rd, k, False, False)
    dispatched(dev, recipe(k, 3, False, False, vt.SCAN))
    check_counters("k 1025", k, 3, False, False, got)
    for call in (lambda: dev.report(seq, qual, rd.offsets, k=k), lambda: Markers(dev, k)):
        with pytest.raises(SpeqError, match=r"k must be in \[1, 1024\]") as e:
            call()
        assert e.value.code == SPEQ_E_ARG
    dev.prepare(4096)   # the limits themselves are taken (no table past k = 31: nothing is built)
    dev.prepare(1)


def test_the_instantiations_observed():
    """Runs last: the matrix, the pass and the EM scans reported, per k, every k_scan instantiation with LF steps that
    their parameters reach."""
    B = (False, True)
    for k in bk.KS:
        want = {vt.Variant(vt.K_SCAN, m, p, lds, False, w) for m, p, lds, w in product(("global", "local"), B, B, (1, 2))}
        want |= {vt.Variant(vt.K_SCAN, "ref", False, lds, False, w) for lds, w in product(B, (1, 2))}
        if k in bk.K_EM:
            want |= {vt.Variant(vt.K_SCAN, m, p, True, True, 1) for m, p in product(("global", "local"), B)}
        got = {v for kk, v in OBSERVED if kk == k}
        assert want <= got <= vt.ALL_VARIANTS, f"k {k}: never launched: {sorted(str(v) for v in want - got)}"
    for k, v in sorted(OBSERVED, key=lambda x: (x[0], str(x[1]))):
        print(f"k {k}: {v}")
