"""GPU: fingerprint collisions and full-bucket chains of the anchor table, constructed (tests/ax_collision_inputs.py)
instead of hoped for, through k_scan_ax (both phases, global / local, single-end / paired, with the absence proofs and
without), its EM instantiation and k_ax_sbitmap.

Expected results come from oracle.Oracle, tests/em_reference.py and the brute-force bitmap of tests/test_gpu_sproof.py.
The numpy model (tests/ax_model.py) only states premises, which FAIL (never skip) when the inputs no longer collide:
the replica's distinct k-mer count equals the model's D (else nb differs), and the instrumented kernel's counters show
the collisions: exactly for class-A reads of k bases whose chain stays in one bucket that is neither full nor receives
overflow, as lower bounds elsewhere (which key sits in which slot of a chain is a race of k_ax_insert), with control
sets of the same shape strictly below. Every chain loop these inputs enter ends because ax_load <= 90 keeps 8 nb > D.
Raw device buffers and the varying-quality variant are compared on the mixed set, which holds every class three times
among ordinary reads: a failure there does not name the class; the per-class host scans do.
A collision at slot 7 of a full bucket (the resumed probe slot becoming 8) cannot be forced: slot order is a race."""
from functools import lru_cache

import numpy as np
import pytest

import ax_collision_inputs as ci
import em_reference as er
from oracle.oracle import Oracle
from speq_amd import DeviceIndex, EmHistogram, FmIndex
from test_gpu_em_rows import check_rows_merged
from test_gpu_parity import W_RTOL
from test_gpu_sproof import brute_force

pytestmark = pytest.mark.gpu
IDS = [f"k{k}-load{load}" for k, load in ci.CONFIGS]
U53 = 2.0 ** -53


@lru_cache(maxsize=None)
def fm_index(k, load):
    d = ci.design(k, load)
    return FmIndex.build(d.records, d.groups, ci.G, prefix_q=8, pair_steps=True, triple_steps=True)


@lru_cache(maxsize=4)
def oracle(k, load):
    d = ci.design(k, load)
    return Oracle(d.records, d.groups, ci.G, k)


def device(k, load, proofs=True):
    dev = DeviceIndex(fm_index(k, load))
    dev.tune(ax_load=load)
    if not proofs:
        dev.tune(ax_mproof=0, ax_sproof=0)
    D = ci.design(k, load).model.D
    got = dev.prepare(k)["distinct_kmers"]
    assert got == D, f"the replica indexes {got} distinct {k}-mers, the model {D}: nb differs, the inputs do not collide"
    return dev


def check_scan(dev, orc, rd, k, paired, local, tag, vary=False):
    got = dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, paired=paired, local=local)
    assert dev.tuning("last_kernel") == 3, tag
    T, amb, U, W = orc.scan(rd.seq, rd.qual, rd.offsets, paired=paired, local=local)
    assert (got.total, got.ambiguous, got.unique.tolist()) == (T, amb, U.tolist()), tag
    if local and not vary:
        np.testing.assert_allclose(got.weights, W, rtol=W_RTOL, atol=0, err_msg=str(tag))
    elif local:  # the bound of test_varying_quality_weights_within_the_documented_bound (tests/test_gpu_ax.py)
        for g in range(ci.G):
            tol = (3 * k + 2 * int(U[g]) + 2) * U53 * W[g]
            assert abs(got.weights[g] - W[g]) <= tol, (tag, g, got.weights[g], W[g], tol)


def check_device_buffers(dev, orc, rd, k, paired, local, tag, stats=False):
    import torch
    d_seq = torch.from_numpy(rd.seq).cuda()
    d_qual = torch.from_numpy(rd.qual).cuda()
    d_off = torch.from_numpy(rd.offsets.astype(np.int64)).cuda()
    cnt = torch.zeros(ci.G + 2, dtype=torch.int64, device="cuda")
    w = torch.zeros(ci.G, dtype=torch.float64, device="cuda")
    fn = dev.scan_device_stats if stats else dev.scan_device
    st = fn(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), rd.n, k, cnt.data_ptr(),
            w.data_ptr() if local else 0, paired=paired, local=local)
    torch.cuda.synchronize()
    assert dev.tuning("last_kernel") == 3, tag
    c = cnt.cpu().numpy()
    T, amb, U, W = orc.scan(rd.seq, rd.qual, rd.offsets, paired=paired, local=local)
    assert (int(c[0]), int(c[1]), c[2:].tolist()) == (T, amb, U.tolist()), tag
    if local:
        np.testing.assert_allclose(w.cpu().numpy(), W, rtol=W_RTOL, atol=0, err_msg=str(tag))
    return st


@pytest.mark.parametrize("proofs", [True, False], ids=["proofs", "noproofs"])
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("cfg", ci.CONFIGS, ids=IDS)
def test_every_class_equals_the_oracle(cfg, paired, proofs):
    k, load = cfg
    dev, orc = device(k, load, proofs), oracle(k, load)
    sets = {name: s[0] + s[1] for name, s in ci.read_sets(k, load).items()}  # constructed and control reads
    sets["all"] = ci.all_reads(k, load)
    for name, reads in sets.items():
        reads = ci.as_pairs(reads, k) if paired else reads
        rd = ci.pack(reads)
        for local in (False, True):
            check_scan(dev, orc, rd, k, paired, local, (name, cfg, paired, proofs, local))
        if name == "all":
            for local in (False, True):
                check_device_buffers(dev, orc, rd, k, paired, local, (name, cfg, paired, proofs, local, "device"))
            check_scan(dev, orc, ci.pack(reads, "vary", seed=k + load), k, paired, True,
                       (name, cfg, paired, proofs, "vary"), vary=True)
    dev.close()


def stats_of(dev, orc, reads, k, tag):
    return check_device_buffers(dev, orc, ci.pack(reads), k, False, False, tag, stats=True)


@pytest.mark.parametrize("cfg", ci.CONFIGS, ids=IDS)
def test_counters_show_the_collisions(cfg):
    k, load = cfg
    d, km, rs = ci.design(k, load), ci.kmers(k, load), ci.read_sets(k, load)
    M = d.model
    dev, orc = device(k, load, proofs=False), oracle(k, load)
    # A, reads of k bases, chains inside one bucket that holds exactly its home keys: exact
    n, want = len(km.A), int(M.collisions(km.A).sum())
    a, c = stats_of(dev, orc, rs["A_k"][0], k, "A_k"), stats_of(dev, orc, rs["A_k"][1], k, "A_k control")
    assert want >= n
    assert (a["run_lanes"], a["lookup_lanes"]) == (want, n + want), \
        f"A: run_lanes {a['run_lanes']} lookup_lanes {a['lookup_lanes']}, model {want} colliding slots of {n} reads"
    assert (c["run_lanes"], c["lookup_lanes"]) == (0, n), f"A control: {c['run_lanes']} {c['lookup_lanes']}"
    # B in phase 1: every key verifies itself, and in each pair one key is reached past the other
    n = len(rs["B_k"][0])
    b, c = stats_of(dev, orc, rs["B_k"][0], k, "B_k"), stats_of(dev, orc, rs["B_k"][1], k, "B_k control")
    assert b["run_lanes"] >= n + ci.H > c["run_lanes"] >= n, \
        f"B: run_lanes {b['run_lanes']}, control {c['run_lanes']}, {n} reads, {ci.H} colliding pairs"
    # B behind a mid-read error, in phase 1: the reads that end with the window against the same reads one base
    # shorter (no such window, everything before it the same). The difference is the window's own lookup: its
    # verification, and in each pair one more past the other key. A window deferred to phase 2 would add nothing.
    if 2 * k + 5 <= 192:  # (a run, the error and the window inside one 192-base piece: not at k = 128)
        diff = []
        for which in (0, 1):
            w, wo = ci.after_error_premise(k, load, which)
            tag = "B_after" + " control" * which
            diff.append(stats_of(dev, orc, w, k, tag)["run_lanes"] - stats_of(dev, orc, wo, k, tag + " cut")["run_lanes"])
        assert diff[0] >= n + ci.H > diff[1] >= n, \
            f"B after an error: {diff[0]} run_lanes for the windows, control {diff[1]}, {n} reads, {ci.H} pairs"
    # B in phase 2: the windows are deferred, found there, and one of each pair past the other
    b = stats_of(dev, orc, rs["B_deferred"][0], k, "B_deferred")
    c = stats_of(dev, orc, rs["B_deferred"][1], k, "B_deferred control")
    assert min(b["p2_verify"], b["p2_probes"]) >= n + ci.H > c["p2_verify"] >= n and b["filter_pass"] >= n, \
        f"B deferred: p2_verify {b['p2_verify']} (control {c['p2_verify']}) p2_probes {b['p2_probes']} " \
        f"filter_pass {b['filter_pass']}, {n} reads, {ci.H} colliding pairs"
    # C: deferred, not ruled out by the Bloom filter, verified against each colliding slot
    n, want = len(km.C), int(M.collisions(km.C).sum())
    a, c = stats_of(dev, orc, rs["C"][0], k, "C"), stats_of(dev, orc, rs["C"][1], k, "C control")
    assert a["filter_pass"] >= n and a["p2_probes"] >= n and a["p2_verify"] >= want > c["p2_verify"], \
        f"C: filter_pass {a['filter_pass']} p2_probes {a['p2_probes']} p2_verify {a['p2_verify']} " \
        f"(control {c['p2_verify']}), model {want} colliding slots of {n} k-mers"
    if load >= 90:
        home = lambda W: M.pair_of(W)[1]  # noqa: E731
        for name, W in (("D_abs_full", km.D_abs_full), ("D_abs_wrap", km.D_abs_wrap)):
            n, want = len(W), int(M.chain[home(W)].sum())
            a = stats_of(dev, orc, rs[name][0][:n], k, name)       # (the reads of k bases come first)
            c = stats_of(dev, orc, rs[name][1][:n], k, name + " control")
            assert want >= 2 * n
            assert a["lookup_lanes"] >= want > c["lookup_lanes"] == n, \
                f"{name}: lookup_lanes {a['lookup_lanes']} (control {c['lookup_lanes']}), model {want} buckets"
        # the keys homed in the last bucket: at least all but 8 of them live in bucket 0 or later (how many slots
        # keys of earlier buckets hold there is a race)
        n = len(km.D_keys_last)
        spilled = n - 8
        a = stats_of(dev, orc, rs["D_keys_last"][0][:n], k, "D_keys_last")
        c = stats_of(dev, orc, rs["D_keys_last"][1][:n], k, "D_keys_last control")
        assert spilled >= 1 and a["lookup_lanes"] >= n + spilled > c["lookup_lanes"] >= n, \
            f"D last bucket: lookup_lanes {a['lookup_lanes']} (control {c['lookup_lanes']}), {n} keys, {spilled} spilled"
    dev.close()


@lru_cache(maxsize=2)
def em_index(k, load):
    d = ci.design(k, load)
    return er.build_index(d.records, d.groups, ci.G, k)


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("cfg", ci.EM_CONFIGS, ids=[f"k{k}-load{load}" for k, load in ci.EM_CONFIGS])
def test_em_rows_of_classes_b_and_c(cfg, paired):
    """The EM instantiation records the interval of the position a lookup ended on: behind a collision that must be
    the verified key's, in both phases. Rows, info and one step against the exact reference, as test_gpu_em_rows."""
    k, load = cfg
    d, rs = ci.design(k, load), ci.read_sets(k, load)
    reads = [r for name, s in sorted(rs.items()) if name[0] in "BC" for r in s[0] + s[1]] + list(ci.ordinary(k, 300))
    rd = ci.pack(ci.as_pairs(reads, k) if paired else reads)
    h = er.scan(em_index(k, load), ci.G, k, rd.seq, rd.qual, rd.offsets, paired=paired)
    dev = device(k, load)
    em = EmHistogram(dev)
    r = em.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, paired=paired)
    assert dev.tuning("last_kernel") == 3
    T, amb, U, _ = oracle(k, load).scan(rd.seq, rd.qual, rd.offsets, paired=paired)
    assert (r.total, r.ambiguous, r.unique.tolist()) == (T, amb, U.tolist()) and (T, U.tolist()) == (h.total, h.unique)
    em.finalize()
    assert h.n_intervals > 0 and em.info() == (h.n_intervals, h.n_entries, h.n_windows)
    check_rows_merged(em, h)
    counts = np.bincount(d.groups, minlength=ci.G)
    percent = np.linspace(5.0, 30.0, ci.G)
    got = em.step(percent, counts, r.unique)
    dev_rel = er.max_relative_deviation(got, er.exact_step(percent, counts, h.unique, h.merged))
    bound = (h.n_intervals + 2 * ci.G + 80) * U53
    assert dev_rel <= bound, (dev_rel, bound)
    em.close()
    dev.close()


@pytest.mark.parametrize("cfg", ci.BITMAP_CONFIGS, ids=[f"k{k}-load{load}" for k, load in ci.BITMAP_CONFIGS])
def test_substitution_bitmap_sound_and_complete_on_the_designed_references(cfg):
    """k_ax_sbitmap walks the same chains: a wrong resume after a colliding slot, or a chain cut at a full bucket,
    sets a bit where a substituted k-mer is indexed (unsound) or clears provable ones."""
    k, load = cfg
    idx = fm_index(k, load)
    dev = device(k, load)
    S = dev.sproof_bitmap(k)
    all_valid, provable = brute_force(idx.array("text", np.uint8), k)
    assert not (S & ~all_valid).any(), "S = 1 within k - 1 of a text end or an N"
    assert not (S & ~provable).any(), "S = 1 where a substituted k-mer is indexed"
    assert provable.sum() > 0.3 * len(S) and not (provable & ~S).any(), "S = 0 at a provable position"
    dev.close()
