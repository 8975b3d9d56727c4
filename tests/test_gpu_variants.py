"""GPU: the ledger of scan-kernel instantiations ("Kernel inventory").

The read-scan kernels k_scan, k_scan_kt and k_scan_ax are templates; the dispatcher picks one of 208 separately
compiled instantiations, each with its own registers, launch bounds, LDS layout and, in places, code. This module
runs every recipe of tests/variant_table.py's PLAN on two module-scoped replicas (5 groups: the tally in LDS; 2049
groups: global atomics) and asserts, per recipe:

  (a) the replica reports the instantiation the hand-written table predicts (tuning key "last_variant"): a recipe
      that silently lands on another instantiation fails;
  (b) T, the ambiguous units and U[g] equal the C oracle bit for bit;
  (c) in local mode W[g] is within (3k + 2 n_g + 2) * 2^-53 relative of the oracle's (the documented bound:
      tests/test_gpu_ax.py);
  (d) EM recipes: EmHistogram.info() and the rows, unmerged and merged, equal tests/em_reference.py exactly; em.step
      is within rtol 1e-9 of the oracle's literal pass and, once per read set, within (n_intervals + 2 G + 80) * 2^-53
      of the exact rational step (the bounds of tests/test_gpu_em_rows.py; the step reads nothing but the rows, so
      the other recipes of a read set must return the same bits);
  (e) the reference-uniqueness pass equals Oracle.ref_unique();
  (f) the instrumented twin leaves the plain scan's counters, ran (waves > 0) and tallied no more windows than T.

The last test asserts that the instantiations reported, all recipes together, are exactly ALL_VARIANTS. The inputs
(tests/variant_inputs.py) hold ambiguous units, counted groups at the far end of the tally and multi-group rows on
every read set, by the references alone (tests/test_variant_table_cpu.py). Every k_scan and k_scan_kt recipe then runs
once more with its dynamic LDS padded to 160 KiB (the grant made at device open). On the 2049-group replica the per-unit
report (33 set words), the FASTQ stream (2051 counters, GPU parser) and the instrumented twin's refusal are pinned
too."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import em_reference as er
import variant_inputs as vi
import variant_table as vt
from speq_amd import DeviceIndex, EmHistogram, FmIndex, SpeqError
from speq_amd._lib import SPEQ_E_ARG, check, lib

pytestmark = pytest.mark.gpu
U53 = 2.0 ** -53
RTOL_STEP = 1e-9     # em.step against the oracle's literal pass (tests/test_gpu_em_rows.py)

REPORTED: dict = {}  # (family, reference) -> {recipe id: reported variant}; read by the coverage test
_EXACT_DONE: dict = {}  # (reference, k, paired, local) -> the step of the first recipe (checked against the exact one)


@pytest.fixture(scope="module")
def replica():
    """name -> the module's one replica of that reference (built on first use)."""
    made = {}

    def get(name: str) -> DeviceIndex:
        if name not in made:
            r = vi.ref(name)
            idx = FmIndex.build(r.records, r.groups, vt.REFS[name].G, prefix_q=8, pair_steps=True, triple_steps=True)
            made[name] = DeviceIndex(idx)
        return made[name]

    yield get
    for dev in made.values():
        dev.close()


def set_tuning(dev: DeviceIndex, r: vt.Recipe):
    dev.tune(**vt.DEFAULTS)
    dev.tune(**dict(r.tune))


def reported(dev: DeviceIndex, r: vt.Recipe) -> vt.Variant:
    """(a): the instantiation the last launch took is the predicted one."""
    got, exp = dev.tuning("last_variant"), vt.predict(r)
    assert got == exp.pack(), f"{r.id}: launched {vt.unpack(got)}, the table predicts {exp}"
    return exp


def check_counters(r: vt.Recipe, v: vt.Variant, total, ambiguous, unique, weights):
    """(b) and (c)."""
    T, amb, Uo, Wo = vi.oracle_scan(r.ref, r.k, r.paired, r.local)
    tag = f"{r.id} [{v}]"
    assert total == T, f"{tag}: T {total} != {T}"
    assert ambiguous == amb, f"{tag}: ambiguous {ambiguous} != {amb}"
    bad = np.flatnonzero(np.asarray(unique, dtype=np.uint64) != Uo)
    assert bad.size == 0, f"{tag}: U differs at groups {bad[:8].tolist()}: {unique[bad[:8]]} != {Uo[bad[:8]]}"
    if r.local:
        tol = (3 * r.k + 2 * Uo.astype(np.float64) + 2) * U53 * Wo
        off = np.flatnonzero(~(np.abs(weights - Wo) <= tol))
        assert off.size == 0, f"{tag}: W out of bound at groups {off[:8].tolist()}: {weights[off[:8]]} vs {Wo[off[:8]]}"


def raw_rows(em: EmHistogram):
    """speq_em_rows as arrays: (multiplicity[r], [row key]) with a row's key as variant_inputs.row_key makes it."""
    nr, ne = C.c_uint64(), C.c_uint64()
    check(lib().speq_em_rows(em._h, C.byref(nr), C.byref(ne), None, None, None, None))
    mult = np.zeros(nr.value, dtype=np.uint64)
    ptr = np.zeros(nr.value + 1, dtype=np.uint64)
    grp = np.zeros(ne.value, dtype=np.uint32)
    cnt = np.zeros(ne.value, dtype=np.uint32)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    check(lib().speq_em_rows(em._h, None, None, mult.ctypes.data_as(u64p), ptr.ctypes.data_as(u64p),
                             grp.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p)))
    p = ptr.tolist()
    assert p[0] == 0 and p[-1] == ne.value and all(b - a >= 2 for a, b in zip(p, p[1:])), "a row of fewer than 2 groups"
    if ne.value:
        inner = np.ones(ne.value, dtype=bool)
        inner[ptr[:-1].astype(np.int64)] = False
        assert (np.diff(grp.astype(np.int64))[inner[1:]] > 0).all(), "groups ascending within a row, each once"
    keys = [grp[a:b].tobytes() + cnt[a:b].tobytes() for a, b in zip(p, p[1:])]
    return mult.tolist(), keys


def em_scan(dev, r: vt.Recipe, rd):
    em = EmHistogram(dev)
    got = em.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=r.k, phred_cutoff=vi.CUTOFF, paired=r.paired,
                  local=r.local)
    return em, got


def run_em(dev, r: vt.Recipe, rd, monkeypatch) -> vt.Variant:
    """(a) to (d) for one EM recipe."""
    h = vi.histogram(r.ref, r.k, r.paired)
    monkeypatch.setenv("SPEQ_EM_MERGE_ROWS", "0")   # one row per interval
    em, got = em_scan(dev, r, rd)
    v = reported(dev, r)
    check_counters(r, v, got.total, got.ambiguous, got.unique, got.weights)
    em.finalize()
    assert em.info() == h.info, f"{r.id} [{v}]: info {em.info()} != {h.info}"
    mult, keys = raw_rows(em)
    assert Counter(zip(keys, mult)) == h.unmerged, f"{r.id} [{v}]: unmerged rows differ"
    em.close()
    monkeypatch.delenv("SPEQ_EM_MERGE_ROWS")        # merged (the default)
    em, got = em_scan(dev, r, rd)
    reported(dev, r)
    check_counters(r, v, got.total, got.ambiguous, got.unique, got.weights)
    em.finalize()
    assert em.info() == h.info
    mult, keys = raw_rows(em)
    assert len(set(keys)) == len(keys), f"{r.id} [{v}]: equal rows left unmerged"
    assert dict(zip(keys, mult)) == h.merged, f"{r.id} [{v}]: merged rows differ"
    step = em.step(vi.percent(r.ref), vi.counts(r.ref), got.unique)
    np.testing.assert_allclose(step, vi.oracle_em_pass(r.ref, r.k, r.paired, r.local), rtol=RTOL_STEP, atol=0,
                               err_msg=r.id)
    key = (r.ref, r.k, r.paired)
    if key not in _EXACT_DONE:
        bound = (h.info[0] + 2 * vt.REFS[r.ref].G + 80) * U53
        dev_rel = er.max_relative_deviation(step, vi.exact_step(r.ref, r.k, r.paired))
        print(f"{r.id}: deviation from the exact step {dev_rel:.3e}, bound {bound:.3e}")
        assert dev_rel <= bound, (r.id, dev_rel, bound)
        _EXACT_DONE[key] = step
    else:
        np.testing.assert_array_equal(step, _EXACT_DONE[key], err_msg=f"{r.id}: the step of equal rows differs")
    em.close()
    return v


def run_stats(dev, r: vt.Recipe, rd) -> vt.Variant:
    """(a), (b), (c) and (f) for one recipe of the instrumented twin."""
    import torch
    G = vt.REFS[r.ref].G
    d_seq = torch.from_numpy(rd.seq.copy()).cuda()
    d_qual = torch.from_numpy(rd.qual.copy()).cuda()
    d_off = torch.from_numpy(rd.offsets.astype(np.int64)).cuda()
    out = []
    for stats in (True, False):
        cnt = torch.zeros(G + 2, dtype=torch.int64, device="cuda")
        w = torch.zeros(G, dtype=torch.float64, device="cuda")
        fn = dev.scan_device_stats if stats else dev.scan_device
        st = fn(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), rd.n, r.k, cnt.data_ptr(),
                w.data_ptr() if r.local else 0, phred_cutoff=vi.CUTOFF, paired=r.paired, local=r.local)
        torch.cuda.synchronize()
        if stats:
            v = reported(dev, r)
            work = st
        else:
            plain = vt.unpack(dev.tuning("last_variant"))
            assert plain == v._replace(stats=False), f"{r.id}: the plain scan took {plain}"
        out.append((cnt.cpu().numpy().astype(np.uint64), w.cpu().numpy()))
    (c, wt), (c0, wt0) = out
    check_counters(r, v, int(c[0]), int(c[1]), c[2:], wt)
    assert c.tolist() == c0.tolist(), f"{r.id} [{v}]: the twin's counters differ from the plain scan's"
    if r.local:
        check_counters(r, v, int(c0[0]), int(c0[1]), c0[2:], wt0)
    assert work["waves"] > 0 and work["wave_iters"] > 0, (r.id, work)
    assert 0 < work["run_tallied"] <= int(c[0]), (r.id, work["run_tallied"], int(c[0]))
    return v


def run_recipe(dev, r: vt.Recipe, monkeypatch) -> vt.Variant:
    set_tuning(dev, r)
    if r.entry == vt.REF:
        u, t = dev.count_unique_kmers_per_group(r.k)
        v = reported(dev, r)
        ou, ot = vi.ref_unique(r.ref, r.k)
        assert np.array_equal(u, ou) and np.array_equal(t, ot), f"{r.id} [{v}]: (U_ref, Tot_ref) differ"   # (e)
        return v
    rd = vi.reads_of(r.ref, r.k, r.paired)
    if r.entry == vt.EM:
        return run_em(dev, r, rd, monkeypatch)
    if r.entry == vt.STATS:
        return run_stats(dev, r, rd)
    got = dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=r.k, phred_cutoff=vi.CUTOFF, paired=r.paired,
                   local=r.local)
    v = reported(dev, r)
    check_counters(r, v, got.total, got.ambiguous, got.unique, got.weights)
    return v


LEDGER = [(family, name) for family in vt.FAMILIES for name in vt.REFS]


@pytest.mark.parametrize("family,name", LEDGER, ids=[f"{f}-{n}" for f, n in LEDGER])
def test_every_recipe_launches_the_predicted_instantiation_and_matches_the_references(family, name, replica,
                                                                                       monkeypatch):
    dev = replica(name)
    mine = sorted((r for r in vt.PLAN if r.ref == name and vt.predict(r).family == family),
                  key=lambda r: (r.k, r.paired))   # (the reference dictionaries are built k by k)
    assert mine
    seen = REPORTED.setdefault((family, name), {})
    for r in mine:
        seen[r.id] = run_recipe(dev, r, monkeypatch)
    dev.tune(**vt.DEFAULTS)
    print(f"{family} on {name}: {len(mine)} recipes, {len(set(seen.values()))} instantiations")


def test_the_recipes_reported_every_instantiation():
    """Runs after the six ledger tests (same module, definition order): together they reported ALL_VARIANTS."""
    assert set(REPORTED) == set(LEDGER), "a ledger test did not run"
    assert sum(len(s) for s in REPORTED.values()) == len(vt.PLAN), "a recipe did not run"
    got = {v for s in REPORTED.values() for v in s.values()}
    unreached = sorted(str(v) for v in vt.ALL_VARIANTS - got)
    assert unreached == [], f"{len(unreached)} instantiations never launched: {unreached}"
    assert got == vt.ALL_VARIANTS


# ---------------------------------------------------------------- more than 64 KiB of dynamic LDS
@pytest.mark.parametrize("name", list(vt.REFS))
def test_every_k_scan_and_k_scan_kt_instantiation_runs_with_160_kib_of_lds(name, replica):
    """The grant of more than 64 KiB of dynamic LDS, made at device open for the set of compiled k_scan and k_scan_kt
    instantiations: with "blocks_per_cu" and "blocks_per_cu_kt" at 1 every launch pads its LDS to 160 KiB, which a
    kernel left out of the grant refuses. Every recipe of the plan that the anchor kernel does not take, once more:
    (a) and (b), (c) in local mode, the counters alone for EM recipes, (e) for the pass."""
    dev = replica(name)
    mine = [r for r in vt.PLAN if r.ref == name and vt.predict(r).family != vt.K_SCAN_AX]
    assert {vt.predict(r) for r in mine} == {v for v in vt.ALL_VARIANTS if v.family != vt.K_SCAN_AX
                                             and v.lds_hist == (name == "g5")}
    keys = ("blocks_per_cu", "blocks_per_cu_kt")
    before = {key: dev.tuning(key) for key in keys}
    try:
        for r in mine:
            set_tuning(dev, r)
            dev.tune(**dict.fromkeys(keys, 1))
            if r.entry == vt.REF:
                u, t = dev.count_unique_kmers_per_group(r.k)
                v = reported(dev, r)
                ou, ot = vi.ref_unique(r.ref, r.k)
                assert np.array_equal(u, ou) and np.array_equal(t, ot), f"{r.id} [{v}]: (U_ref, Tot_ref) differ"
                continue
            rd = vi.reads_of(r.ref, r.k, r.paired)
            if r.entry == vt.EM:
                em, got = em_scan(dev, r, rd)
                em.close()
            else:
                got = dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=r.k, phred_cutoff=vi.CUTOFF,
                               paired=r.paired, local=r.local)
            v = reported(dev, r)
            check_counters(r, v, got.total, got.ambiguous, got.unique, got.weights)
    finally:
        dev.tune(**before)
        dev.tune(**vt.DEFAULTS)


# ---------------------------------------------------------------- the other entry points at G = 2049
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_report_of_2049_groups_equals_the_model(paired, replica):
    """33 set words per unit; its ambiguous count is the scan's."""
    name, k = "g2049", vt.K_COMPACT
    dev, rd, exp = replica(name), vi.reads_of(name, k, paired), vi.report(name, k, paired)
    dev.tune(**vt.DEFAULTS)
    got = dev.report(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, phred_cutoff=vi.CUTOFF, paired=paired)
    assert got.sets.shape == (exp.n_units, 33) and exp.W == 33
    assert got.passing.tolist() == exp.passing and got.unique.tolist() == exp.unique
    assert got.shared.tolist() == exp.shared and got.first_group.tolist() == exp.first_group
    np.testing.assert_array_equal(got.sets, exp.words())
    n_bits = np.unpackbits(got.sets.view(np.uint8), axis=1).sum(axis=1)
    T, amb, Uo, _ = vi.oracle_scan(name, k, paired, False)
    assert int((n_bits >= 2).sum()) == exp.ambiguous == amb >= 2
    assert (got.sets[:, 32] >> np.uint64(1)).max() == 0, "bits past group 2048"
    assert got.sets[:, 31].any() or got.sets[:, 32].any(), "no unit names a group of the last words"
    sc = dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, phred_cutoff=vi.CUTOFF, paired=paired)
    assert (sc.total, sc.ambiguous) == (int(got.passing.sum()), int((n_bits >= 2).sum()))
    assert sc.unique.tolist() == exp.per_group == Uo.tolist()


def write_fastq(path, rd, lo: int, step: int):
    L = int(rd.offsets[1])
    with open(path, "wb") as f:
        for i in range(lo, rd.n, step):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, rd.seq[i * L:(i + 1) * L].tobytes(), rd.qual[i * L:(i + 1) * L].tobytes()))


@pytest.mark.parametrize("local", [False, True], ids=["global", "local"])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_fastq_stream_of_2049_groups_equals_the_in_memory_scan(paired, local, replica, tmp_path):
    """Plain FASTQ through the GPU parser, 2051 counters, with an EM histogram: the in-memory scan's results."""
    name, k = "g2049", vt.K_COMPACT
    dev, rd, h = replica(name), vi.reads_of(name, k, paired), vi.histogram(name, k, paired)
    dev.tune(**vt.DEFAULTS)
    assert dev.tuning("fastq_gpu_parse") == 1
    r = vt.Recipe(name, k, paired, local, vt.EM)
    if paired:
        write_fastq(tmp_path / "r1.fq", rd, 0, 2)
        write_fastq(tmp_path / "r2.fq", rd, 1, 2)
        p1, p2 = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")
    else:
        write_fastq(tmp_path / "r1.fq", rd, 0, 1)
        p1, p2 = str(tmp_path / "r1.fq"), None
    em = EmHistogram(dev)
    got, st = dev.scan_fastq(p1, p2, k=k, phred_cutoff=vi.CUTOFF, local=local, threads=2, em=em)
    v = reported(dev, r)
    assert (st["records"], st["bases"]) == (rd.n, int(rd.offsets[-1]))
    check_counters(r, v, got.total, got.ambiguous, got.unique, got.weights)
    em.finalize()
    assert em.info() == h.info
    mult, keys = raw_rows(em)
    assert dict(zip(keys, mult)) == h.merged
    em2, mem = em_scan(dev, r, rd)
    assert (got.total, got.ambiguous, got.unique.tolist()) == (mem.total, mem.ambiguous, mem.unique.tolist())
    if local:
        np.testing.assert_allclose(got.weights, mem.weights, rtol=1e-12, atol=0)  # (batches may differ: re-associated)
    em2.finalize()
    np.testing.assert_array_equal(em.step(vi.percent(name), vi.counts(name), got.unique),
                                  em2.step(vi.percent(name), vi.counts(name), mem.unique))
    em.close()
    em2.close()


def test_instrumented_twin_refuses_more_than_2048_groups(replica):
    """speq_scan_reads_device_stats on the 2049-group replica: SPEQ_E_ARG naming the limit, before anything is
    launched (the counters, the weights and the work counts stay as they were)."""
    import torch
    name, k = "g2049", vt.K_COMPACT
    dev, rd = replica(name), vi.reads_of(name, k, False)
    dev.tune(**vt.DEFAULTS)
    G = vt.REFS[name].G
    d_seq = torch.from_numpy(rd.seq.copy()).cuda()
    d_qual = torch.from_numpy(rd.qual.copy()).cuda()
    d_off = torch.from_numpy(rd.offsets.astype(np.int64)).cuda()
    plain = dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, phred_cutoff=vi.CUTOFF)
    before = dev.tuning("last_variant")
    for local in (False, True):
        cnt = torch.zeros(G + 2, dtype=torch.int64, device="cuda")
        w = torch.zeros(G, dtype=torch.float64, device="cuda")
        with pytest.raises(SpeqError, match="2048") as e:
            dev.scan_device_stats(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), rd.n, k, cnt.data_ptr(),
                                  w.data_ptr(), phred_cutoff=vi.CUTOFF, local=local)
        assert e.value.code == SPEQ_E_ARG and "2049" in str(e.value)
        torch.cuda.synchronize()
        assert not cnt.any().item() and not w.any().item(), "the refused call wrote counters"
        assert dev.tuning("last_variant") == before, "the refused call launched a scan kernel"
    # (the raw call: the caller's stats buffer stays untouched too)
    from speq_amd._lib import SPEQ_MODE_GLOBAL, ScanParams
    st = np.full(len(DeviceIndex.AX_STATS_KEYS), 7, dtype=np.uint64)
    cnt = torch.zeros(G + 2, dtype=torch.int64, device="cuda")
    p = ScanParams(k, vi.CUTOFF, 0, SPEQ_MODE_GLOBAL)
    rc = lib().speq_scan_reads_device_stats(dev.handle, d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), rd.n,
                                            C.byref(p), cnt.data_ptr(), None,
                                            st.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == SPEQ_E_ARG and (st == 7).all() and not cnt.any().item()
    assert plain.total == vi.oracle_scan(name, k, False, False)[0]
