"""GPU: odd read shapes in the middle of ordinary reads, on every scan path, against the CPU oracle.

Trimmed data holds empty reads, reads of k - 1, k and k + 1 bases, and mates of unequal length next to full-length
reads. The persistent-lane kernel takes "the next piece" of a unit (a second mate after a first mate without windows,
an empty mate, a read that fits no window) in a branch of its own, which must also work when the other lanes of the
wave are busy with ordinary reads. Reads are upper case at Q40 with 0.3 % errors, so only the shape is under test.
Every case runs on raw device buffers (base pointers as torch allocates them) and through speq_scan_reads, on the four
kernel variants, global and local: integers bit-exact, W to rtol 1e-10."""
import numpy as np
import pytest

import byte_reads as br
from oracle.oracle import Oracle
from speq_amd import DeviceIndex, FmIndex, synth
from test_gpu_parity import VARIANTS, W_RTOL

pytestmark = pytest.mark.gpu

G, UNITS = br.G, 3_000
KS = [21, 33, 70]


@pytest.fixture(scope="module")
def env():
    ref = br.reference()
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=True, triple_steps=True)
    return ref, DeviceIndex(idx)


def check_all(dev, orc, reads, k, paired):
    """Both entry points, four kernels, both modes; returns the oracle's global (T, ambiguous, U, None)."""
    out = None
    try:
        for local in (False, True):
            exp = orc.scan(reads.seq, reads.qual, reads.offsets, paired=paired, local=local)
            out = out or exp
            for v in VARIANTS:
                dev.tune(ilp=v["ilp"], ilp_local=v["ilp"], kmer_table=v["kmer_table"], ax_scan=v["ax_scan"])
                host = dev.scan(reads.seq.tobytes(), reads.qual.tobytes(), reads.offsets, k=k, paired=paired,
                                local=local)
                for what, got in (("device", br.device_scan(dev, reads, k, 30, paired, local)),
                                  ("host", (host.total, host.ambiguous, host.unique, host.weights))):
                    assert (got[0], got[1], got[2].tolist()) == (exp[0], exp[1], exp[2].tolist()), (what, v, local)
                    if local:
                        assert np.isfinite(got[3]).all()
                        np.testing.assert_allclose(got[3], exp[3], rtol=W_RTOL, atol=0, err_msg=f"{what} {v}")
    finally:
        dev.tune(ilp=1, ilp_local=1, kmer_table=1, ax_scan=1)
    return out


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("ends_empty", [False, True])
def test_single_end_odd_lengths_mid_stream(env, k, ends_empty):
    """150-base reads shuffled with reads of 0, 1, k - 1, k, k + 1, 16, 17 (a staging chunk and a byte more) and 191,
    192, 193 bases (a lane's staging segment and its neighbours); once with an empty first and last read."""
    ref, dev = env
    full = synth.make_reads(ref, 2 * UNITS // 3, err_rate=0.003)
    odd = synth.make_reads(ref, UNITS // 3, read_len=193, err_rate=0.003, start_index=10_000)
    lengths = [0, 1, k - 1, k, k + 1, 16, 17, 191, 192, 193]
    odd = br.cut(odd, [lengths[i % len(lengths)] for i in range(odd.n)])
    order = [(0, i) for i in range(full.n)] + [(1, i) for i in range(odd.n)]
    order = [order[i] for i in np.random.default_rng(k).permutation(len(order))]
    if ends_empty:
        empties = [j for j, (s, i) in enumerate(order) if s == 1 and i % len(lengths) == 0]
        for end, j in ((0, empties[0]), (len(order) - 1, empties[-1])):
            order[end], order[j] = order[j], order[end]
    reads = br.gather([full, odd], order)
    lens = np.diff(reads.offsets).astype(np.int64)
    assert reads.n == UNITS and set(lengths) <= set(lens.tolist())
    assert not ends_empty or (lens[0] == 0 and lens[-1] == 0)
    exp = check_all(dev, Oracle(ref.records, ref.groups, G, k), reads, k, False)
    assert exp[0] == int(np.maximum(lens - k + 1, 0).sum()) - _windows_over_n(reads, k) and exp[2].sum() > 0


def _windows_over_n(reads, k):
    """Windows of the reads that hold a base other than ACGT (none at Q40 otherwise fails)."""
    bad = np.concatenate([[0], np.cumsum(~np.isin(reads.seq, np.frombuffer(b"ACGT", dtype=np.uint8)))])
    n = 0
    for i in range(reads.n):
        a, b = int(reads.offsets[i]), int(reads.offsets[i + 1])
        if b - a >= k:
            n += int(((bad[a + k:b + 1] - bad[a:b - k + 1]) > 0).sum())
    return n


@pytest.mark.parametrize("k", KS)
def test_paired_unequal_mates(env, k):
    """Mate lengths drawn independently from {0, k - 1, k, 37, 150}: first and second mates without windows, empty
    mates, pairs empty on both sides, next to ordinary pairs."""
    ref, dev = env
    reads = synth.make_reads(ref, UNITS, err_rate=0.003, paired=True)
    lens = np.random.default_rng(100 + k).choice([0, k - 1, k, 37, 150], size=reads.n)
    pl = lens.reshape(-1, 2)
    assert ((pl[:, 0] == 0) & (pl[:, 1] == 0)).any()
    for m in (0, 1):  # each mate without a window while the other has some, and the reverse
        assert ((pl[:, m] < k) & (pl[:, 1 - m] >= k)).any() and ((pl[:, m] == 0) & (pl[:, 1 - m] == 150)).any()
    reads = br.cut(reads, lens)
    exp = check_all(dev, Oracle(ref.records, ref.groups, G, k), reads, k, True)
    assert exp[0] > 0 and exp[2].sum() > 0


def chimeric_pairs(ref, n, rng):
    """Mate 1 from variant v, mate 2 (reverse complement) from variant u != v, over a position where the two differ."""
    recs = [np.frombuffer(r, dtype=np.uint8) for r in ref.records]
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    segs = []
    for _ in range(n):
        v, u = rng.choice(ref.n_variants, size=2, replace=False)
        a, b = recs[int(v) * ref.n_isolates], recs[int(u) * ref.n_isolates]
        d = int(rng.choice(np.flatnonzero(a != b)))
        s = min(max(d - 75, 0), a.size - 150)
        segs += [a[s:s + 150], synth.COMP[b[s:s + 150][::-1]]]
    seq = np.concatenate(segs)
    err = np.flatnonzero((rng.random(seq.size) < 0.003) & (seq != ord("N")))
    seq[err] = acgt[(np.searchsorted(acgt, seq[err]) + rng.integers(1, 4, size=err.size)) % 4]
    off = np.arange(0, seq.size + 1, 150, dtype=np.uint64)
    return synth.Reads(seq, np.full(seq.size, ord("I"), dtype=np.uint8), off, np.zeros(2 * n, np.int32))


@pytest.mark.parametrize("k", KS)
def test_chimeric_pairs_combine_their_mates(env, k):
    """A pair's mates share one read state: mates from two variants make the pair ambiguous. The oracle calls many of
    these pairs ambiguous; with one mate of each pair cut to k - 1 bases or to none, that mate has no window, and the
    ambiguity falls to what single mates show. The scans must give both counts."""
    ref, dev = env
    orc = Oracle(ref.records, ref.groups, G, k)
    reads = chimeric_pairs(ref, UNITS, np.random.default_rng(200 + k))
    full = check_all(dev, orc, reads, k, True)
    assert full[1] >= 100, full[1]
    rng = np.random.default_rng(300 + k)
    lens = np.full(reads.n, 150, dtype=np.int64)
    which = 2 * np.arange(UNITS) + rng.integers(0, 2, size=UNITS)  # either mate, first or second
    lens[which] = rng.choice([k - 1, 0], size=UNITS)
    cut = check_all(dev, orc, br.cut(reads, lens), k, True)
    assert cut[1] < full[1] // 2 and cut[2].sum() > 0, (cut[1], full[1])
