"""CPU: the C oracle against the pure-Python brute force of tests/golden/make_golden.py on fresh random cases
(the brute force replays the reference's loops literally over sorted (text_id, pos) hit lists)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden as bf  # noqa: E402

import byte_reads  # noqa: E402

from oracle.oracle import Oracle  # noqa: E402
from speq_amd import synth  # noqa: E402


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("paired", [False, True])
def test_oracle_equals_bruteforce(seed, paired):
    rng = np.random.default_rng(seed)
    V, I = int(rng.integers(1, 4)), int(rng.integers(1, 3))
    ref = synth.make_reference(V, I, 300, ref_n_rate=0.01 * (seed % 2))
    reads = synth.make_reads(ref, 25, read_len=45, fragment=100, paired=paired, n_rate=0.01, lowq_rate=0.03,
                             short_frac=0.0 if paired else 0.1, start_index=1000 * seed)
    recs = [r.decode() for r in ref.records]
    texts = bf.texts_of(recs)
    dgs = [g for g in ref.groups for _ in (0, 1)]
    rs, qs = bf.reads_lists(reads)
    k = int(rng.integers(5, 14))
    cutoff = int(rng.integers(5, 35))
    orc = Oracle(ref.records, ref.groups, V, k)
    u, t = orc.ref_unique()
    bu, bt = bf.ref_unique(recs, texts, dgs, ref.groups, V, k)
    assert u.tolist() == bu and t.tolist() == bt
    for local in (False, True):
        T, amb, U, W = orc.scan(reads.seq, reads.qual, reads.offsets, phred_cutoff=cutoff, paired=paired,
                                local=local)
        bT, bamb, bU, bW = bf.scan(texts, dgs, V, rs, qs, k, cutoff, local, paired)
        assert (T, amb, U.tolist()) == (bT, bamb, bU)
        if local:
            np.testing.assert_allclose(W, bW, rtol=1e-12)


@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("paired", [False, True])
def test_oracle_equals_bruteforce_on_byte_reads(seed, paired):
    """The whole byte range (byte_reads: lower case, U, junk bytes, qualities at the cutoff, above 'J' and above
    0x7F), with tails cut so that mates are unequal, shorter than k and empty. Bytes >= 0x80 travel to the brute force
    as latin-1 characters."""
    V, k, cutoff, L = 3, 9, 20, 45
    ref = synth.make_reference(V, 2, 300, ref_n_rate=0.01 * (seed % 2))
    reads, _ = byte_reads.byte_reads(ref, 25, cutoff, seed, paired=paired, read_len=L)
    rng = np.random.default_rng(seed)
    lens = rng.choice([L, L, L - 1, 10, 9, 8, 0], size=reads.n)
    reads = byte_reads.cut(reads, lens)
    if paired:
        pl = lens.reshape(-1, 2)
        assert (pl[:, 0] != pl[:, 1]).any() and (lens == 0).any() and (lens == k - 1).any()
    assert reads.seq.max() >= 0x80 and reads.qual.max() >= 0x80
    recs = [r.decode() for r in ref.records]
    texts = bf.texts_of(recs)
    dgs = [g for g in ref.groups for _ in (0, 1)]
    rs, qs = [], []
    for i in range(reads.n):
        a, b = int(reads.offsets[i]), int(reads.offsets[i + 1])
        rs.append(reads.seq[a:b].tobytes().decode("latin-1"))
        qs.append(reads.qual[a:b].tobytes().decode("latin-1"))
    orc = Oracle(ref.records, ref.groups, V, k)
    for local in (False, True):
        T, amb, U, W = orc.scan(reads.seq, reads.qual, reads.offsets, phred_cutoff=cutoff, paired=paired,
                                local=local)
        bT, bamb, bU, bW = bf.scan(texts, dgs, V, rs, qs, k, cutoff, local, paired)
        assert (T, amb, U.tolist()) == (bT, bamb, bU)
        assert T > 0 and sum(bU) > 0
        if local:
            np.testing.assert_allclose(W, bW, rtol=1e-12)


@pytest.mark.parametrize("cutoff", [0, 30, 40])
@pytest.mark.parametrize("k", [21, 70])
def test_byte_reads_are_not_vacuous(k, cutoff):
    """The inputs of tests/test_gpu_bytes.py, with the oracle alone: most windows pass and many are counted, and every
    byte class carries passing windows, since reading any one class wrongly lowers T: lower case as N, U as N, quality
    bytes above 'J' as rank 0, quality bytes >= 0x80 as rank 0. (Conditions on the input: a decoder that gets one of
    these classes wrong cannot give the oracle's T on them.)"""
    ref = byte_reads.reference()
    reads, m = byte_reads.byte_reads(ref, byte_reads.N_READS, cutoff, byte_reads.SEED)
    orc = Oracle(ref.records, ref.groups, byte_reads.G, k)
    T, _, U, W = orc.scan(reads.seq, reads.qual, reads.offsets, phred_cutoff=cutoff, local=True)
    windows = int(np.maximum(np.diff(reads.offsets).astype(np.int64) - k + 1, 0).sum())
    assert T > windows / 2, (T, windows)
    assert U.sum() > 0 and np.isfinite(W).all()
    assert m.junk.sum() > 0 and (reads.qual[~m.junk] <= 33).any()
    broken = {}
    for name, sel, on_seq in (("lower", m.lower, True), ("u", m.u, True), ("above_J", reads.qual > 74, False),
                              ("high_bit", reads.qual >= 128, False)):
        seq, qual = reads.seq.copy(), reads.qual.copy()
        if on_seq:
            seq[sel] = ord("N")
        else:
            qual[sel] = ord("!")
        broken[name] = orc.scan(seq, qual, reads.offsets, phred_cutoff=cutoff)[0]
        assert broken[name] < T, (name, broken[name], T)
    print(f"k={k} cutoff={cutoff}: T={T} of {windows}, U={int(U.sum())}, broken={broken}")
