"""GPU: substitution-bitmap proofs in the anchor-and-extend scan (k_scan_ax lane state 7).

S[x] = 1 says that no k-mer of the texts equals one of the k text windows over position x with another base at x.
A run that breaks at read base e against text position x leaves the first window over e to be looked up; when that
finds nothing and S[x] = 1, the windows over e are dropped without a deferral and the run goes on behind e, as far as
the read equals the text there. A wrong 1 in S, or a window dropped on anything but compared bases, is a wrong count,
so the bitmap is checked against a brute-force set of the indexed k-mers (no false 1, and no missing 1 either: an
all-zero bitmap would pass every parity test) and the scans against the oracle and against the scan without the
proofs (tuning ax_sproof = 0) bit for bit: error-dense reads (second mismatches within k, deferred-list overflow),
mismatches near read and segment ends, N in reads and references, SNP sites whose substituted k-mers occur, paired
and local scans, EM histograms."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from speq_amd import DeviceIndex, EmHistogram, FmIndex, synth

pytestmark = pytest.mark.gpu


def scan(dev, reads, k, paired=False, local=False, sproof=1):
    dev.tune(ax_sproof=sproof)
    got = dev.scan(reads.seq.tobytes(), reads.qual.tobytes(), reads.offsets, k=k, paired=paired, local=local)
    assert dev.tuning("last_kernel") == 3
    return got


def same(a, b, local):
    assert (a.total, a.ambiguous, a.unique.tolist()) == (b.total, b.ambiguous, b.unique.tolist())
    if local:
        np.testing.assert_allclose(a.weights, b.weights, rtol=1e-12, atol=0)


def against_oracle(got, want, local, tag):
    T, amb, U, W = want
    assert (got.total, got.ambiguous, got.unique.tolist()) == (T, amb, U.tolist()), tag
    if local:
        np.testing.assert_allclose(got.weights, W, rtol=1e-10, atol=0)


def build(ref, G):
    return FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=True, triple_steps=True)


@pytest.fixture(scope="module")
def small():
    ref = synth.make_reference(4, 2, 6_000, ref_n_rate=0.002)
    idx = build(ref, 4)
    dev = DeviceIndex(idx)
    yield ref, idx, dev
    dev.close()


# ---- the bitmap against brute force

def brute_force(text, k):
    """(all_valid, provable) per text position x, from the FM text (A C G T = 2..5; N, separators, terminator other):
    all_valid: each of the k windows over x lies in one text and holds no N; provable: that, and no such window with
    another base at x is a k-mer of the texts (either strand: the texts hold both)."""
    n = len(text)
    acgt = (text >= 2) & (text <= 5)
    code = np.where(acgt, text - 2, 0).astype(np.uint64)
    nwin = n - k + 1
    bad = np.concatenate([[0], np.cumsum(~acgt)])
    valid = (bad[k:] - bad[:nwin]) == 0  # window s: all of text[s, s + k) is ACGT
    # a window's key: its first 32 bases in `a`, the rest in `b` (exact: 2 bits per base, k <= 64)
    a = np.zeros(nwin, dtype=np.uint64)
    b = np.zeros(nwin, dtype=np.uint64)
    for i in range(k):
        (a if i < 32 else b)[:] |= code[i:i + nwin] << np.uint64(2 * (i % 32))
    ia, ib = a[valid], b[valid]
    groups = {int(v): np.unique(ia[ib == v]) for v in np.unique(ib)}

    def member(qa, qb):
        out = np.zeros(len(qa), dtype=bool)
        for v in np.unique(qb):
            m = qb == v
            if int(v) in groups:
                out[m] = np.isin(qa[m], groups[int(v)])
        return out

    hit = np.zeros(n, dtype=bool)  # some valid window over x with another base at x is indexed
    starts = np.nonzero(valid)[0]
    for i in range(k):
        sh = np.uint64(2 * (i % 32))
        for sub in (1, 2, 3):
            qa, qb = a[starts].copy(), b[starts].copy()
            (qa if i < 32 else qb)[:] ^= np.uint64(sub) << sh
            hit[starts[member(qa, qb)] + i] = True
    cover = np.zeros(n + 1, dtype=np.int64)  # valid windows over x
    np.add.at(cover, starts, 1)
    np.add.at(cover, starts + k, -1)
    all_valid = np.cumsum(cover)[:n] == k
    return all_valid, all_valid & ~hit


@pytest.fixture(scope="module", params=[0.002, 0.0], ids=["refN", "noN"])
def bitmap_case(request):
    ref = synth.make_reference(4, 2, 3_000, ref_n_rate=request.param)
    idx = build(ref, 4)
    dev = DeviceIndex(idx)
    text = idx.array("text", np.uint8)
    out = {}
    for k in (21, 33):
        dev.prepare(k)
        out[k] = (dev.sproof_bitmap(k),) + brute_force(text, k)
    dev.close()
    return out


@pytest.mark.parametrize("k", [21, 33])
def test_bitmap_sound(bitmap_case, k):
    S, all_valid, provable = bitmap_case[k]
    assert not (S & ~all_valid).any(), "S = 1 within k - 1 of a text end or an N"
    assert not (S & ~provable).any(), "S = 1 where a substituted k-mer is indexed"


@pytest.mark.parametrize("k", [21, 33])
def test_bitmap_complete(bitmap_case, k):
    S, all_valid, provable = bitmap_case[k]
    assert provable.sum() > 0.5 * len(S)  # (the fixture is not degenerate)
    assert not (provable & ~S).any(), "S = 0 at a provable position"


# ---- the scans

@pytest.mark.parametrize("k", [21, 24, 31, 32, 33, 64, 65, 70])
@pytest.mark.parametrize("err", [0.003, 0.03])
def test_counts_match_oracle_and_no_proofs(small, k, err):
    """0.3 % errors: mostly single mismatches; 3 %: second mismatches within k and deferred-list overflow."""
    ref, idx, dev = small
    reads = synth.make_reads(ref, 2_000, err_rate=err, n_rate=0.002, lowq_rate=0.01, short_frac=0.05)
    orc = Oracle(ref.records, ref.groups, 4, k)
    for local in (False, True):
        on = scan(dev, reads, k, local=local)
        against_oracle(on, orc.scan(reads.seq, reads.qual, reads.offsets, local=local), local, (k, err, local))
        same(on, scan(dev, reads, k, local=local, sproof=0), local)


@pytest.mark.parametrize("k", [21, 31, 70])
@pytest.mark.parametrize("paired", [False, True])
def test_paired_and_local_variable_qualities(small, k, paired):
    ref, idx, dev = small
    reads = synth.apply_quality_profile(synth.make_reads(ref, 1_500, err_rate=0.01, paired=paired, n_rate=0.001),
                                        "variable")
    orc = Oracle(ref.records, ref.groups, 4, k)
    for local in (False, True):
        on = scan(dev, reads, k, paired=paired, local=local)
        against_oracle(on, orc.scan(reads.seq, reads.qual, reads.offsets, paired=paired, local=local), local,
                       (k, paired, local))
        same(on, scan(dev, reads, k, paired=paired, local=local, sproof=0), local)


@pytest.mark.parametrize("paired", [False, True])
def test_em_histogram_equal_with_and_without_proofs(paired):
    ref = synth.make_reference(5, 3, 8_000, ref_n_rate=0.0005)
    idx = FmIndex.build(ref.records, ref.groups, 5, prefix_q=9, pair_steps=True, triple_steps=True)
    reads = synth.make_reads(ref, 6_000, paired=paired, n_rate=0.001, lowq_rate=0.005, err_rate=0.01)
    for k in (21, 31):
        res = []
        for sproof in (1, 0):
            dev = DeviceIndex(idx)
            dev.tune(ax_sproof=sproof)
            em = EmHistogram(dev)
            r = em.scan(reads.seq.tobytes(), reads.qual.tobytes(), reads.offsets, k=k, paired=paired)
            em.finalize()
            res.append((r.total, r.ambiguous, r.unique.tolist(), em.info(),
                        em.step(np.linspace(5.0, 30.0, 5), [3] * 5, r.unique).tolist()))
            dev.close()
        assert res[0] == res[1], k


@pytest.mark.parametrize("read_len", [60, 191, 193, 400])
def test_read_and_segment_ends(small, read_len):
    """Short reads (the continued run reaches the piece's end before k - 1 bases) and reads longer than a lane's
    192-base segment (mismatches next to the segment boundary), at 2 % errors."""
    ref, idx, dev = small
    reads = synth.make_reads(ref, 800, read_len=read_len, err_rate=0.02)
    for k in (21, 31, 58):
        want = Oracle(ref.records, ref.groups, 4, k).scan(reads.seq, reads.qual, reads.offsets)
        on = scan(dev, reads, k)
        against_oracle(on, want, False, (k, read_len))
        same(on, scan(dev, reads, k, sproof=0), False)


def test_snp_alleles_of_another_variant_are_counted():
    """SNP-dense reference: reads of one variant that carry another variant's allele at the sites where the two
    differ. A window over such a site equals the other variant's text when no other difference lies in it, so it is
    indexed and S is 0 there: it must be looked up and counted as the oracle counts it, not dropped."""
    G, L, n_reads, rl = 24, 3_000, 3_000, 150
    ref = synth.make_reference(G, 1, L)
    idx = build(ref, G)
    dev = DeviceIndex(idx)
    gen = np.stack([np.frombuffer(r, dtype=np.uint8) for r in ref.records])
    rng = np.random.default_rng(11)
    v = rng.integers(0, G, n_reads)
    u = (v + 1 + rng.integers(0, G - 1, n_reads)) % G  # another variant
    s0 = rng.integers(0, L - rl + 1, n_reads)
    cols = s0[:, None] + np.arange(rl)[None, :]
    own, other = gen[v[:, None], cols], gen[u[:, None], cols]
    take = (own != other) & (rng.random((n_reads, rl)) < 0.5)  # half of the differing sites take the other allele
    assert take.sum() > n_reads  # more than one such site per read on average
    seq = np.where(take, other, own)
    rc = rng.random(n_reads) < 0.5
    seq[rc] = synth.COMP[seq[rc][:, ::-1]]
    reads = synth.Reads(np.ascontiguousarray(seq.reshape(-1)), np.full(n_reads * rl, ord("I"), dtype=np.uint8),
                        np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(rl), v.astype(np.int32))
    for k in (21, 31, 70):
        T, amb, U, W = Oracle(ref.records, ref.groups, G, k).scan(reads.seq, reads.qual, reads.offsets)
        on = scan(dev, reads, k)
        against_oracle(on, (T, amb, U, W), False, k)
        same(on, scan(dev, reads, k, sproof=0), False)
        assert int(U.sum()) > 0
    dev.close()


def test_not_vacuous():
    """N-free reference, Q40 reads, k = 21, 0.3 % errors: the instrumented twin drops windows on proofs, and defers
    fewer than half of what it defers without them (what remains: errors in a read's first window, whose text
    position is unknown, SNP sites, and second errors within k)."""
    import torch

    ref = synth.make_reference(4, 2, 6_000)
    idx = build(ref, 4)
    dev = DeviceIndex(idx)
    k, G = 21, 4
    reads = synth.make_reads(ref, 2_000, err_rate=0.003)
    T, amb, U, _ = Oracle(ref.records, ref.groups, G, k).scan(reads.seq, reads.qual, reads.offsets)
    d_seq = torch.from_numpy(reads.seq).cuda()
    d_qual = torch.from_numpy(reads.qual).cuda()
    d_off = torch.from_numpy(reads.offsets.astype(np.int64)).cuda()
    st = {}
    for sproof in (1, 0):
        dev.tune(ax_sproof=sproof)
        cnt = torch.zeros(G + 2, dtype=torch.int64, device="cuda")
        st[sproof] = dev.scan_device_stats(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), reads.n, k,
                                           cnt.data_ptr())
        c = cnt.cpu().numpy()
        assert (int(c[0]), int(c[1]), c[2:].tolist()) == (T, amb, U.tolist()), sproof
    print("sproof on:", {key: st[1][key] for key in ("deferred", "sproof_probes", "sproof_windows", "sproof_partial")},
          "off: deferred", st[0]["deferred"])
    assert st[0]["sproof_probes"] == 0 and st[0]["sproof_windows"] == 0
    assert st[1]["sproof_windows"] > 0
    assert st[1]["deferred"] < 0.5 * st[0]["deferred"], (st[1]["deferred"], st[0]["deferred"])
    dev.close()
