"""GPU: the raw read-byte contract on every scan path (DESIGN.md §4e "Exactness"), against the CPU oracle.

dna5 (ACGT / acgt, U / u as T, every other byte N) and phred42 (byte - 33 clamped to [0, 41]; a window passes iff no
base is N and every quality > cutoff) are decoded by separate code in the LF-step kernel, the k-mer-table kernel, the
anchor-and-extend kernel (a SWAR decode and, in local mode, a factor table indexed by the byte), the host packers
(scalar and AVX2), the unpack kernels behind them, the GPU FASTQ parser and the index builds. These tests feed each
of them byte_reads.byte_reads (lower case, U, junk bytes one bit from a base, qualities at the cutoff, above 'J',
above 0x7F) and compare with oracle/kmer_oracle.c: integers bit-exact, W to rtol 1e-10 and finite.
tests/test_oracle_bruteforce.py shows with the oracle alone that each byte class carries passing windows."""
import numpy as np
import pytest

import byte_reads as br
from oracle.oracle import Oracle
from speq_amd import DeviceIndex, EmHistogram, FmIndex, SpeqError, synth
from test_gpu_build import ARRAYS
from test_gpu_parity import VARIANTS, W_RTOL

pytestmark = pytest.mark.gpu

G = br.G


@pytest.fixture(scope="module")
def env():
    ref = br.reference()
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=True, triple_steps=True)
    return ref, DeviceIndex(idx)


_reads, _oracles, _expected = {}, {}, {}


def reads_of(ref, cutoff=30, paired=False, fastq_safe=False):
    key = (cutoff, paired, fastq_safe)
    if key not in _reads:
        _reads[key] = br.byte_reads(ref, br.N_READS, cutoff, br.SEED, paired=paired, fastq_safe=fastq_safe)[0]
    return _reads[key]


def oracle_of(ref, k):
    if k not in _oracles:
        _oracles[k] = Oracle(ref.records, ref.groups, G, k)
    return _oracles[k]


def expected(ref, k, cutoff=30, paired=False, local=False, fastq_safe=False):
    """The oracle's (T, ambiguous, U, W) on reads_of(...): computed once, shared, never changed."""
    key = (k, cutoff, paired, local, fastq_safe)
    if key not in _expected:
        rd = reads_of(ref, cutoff, paired, fastq_safe)
        _expected[key] = oracle_of(ref, k).scan(rd.seq, rd.qual, rd.offsets, phred_cutoff=cutoff, paired=paired,
                                                local=local)
    return _expected[key]


def same(got, exp, local, what=None):
    """got: (T, amb, U, W) or a ScanResult."""
    if not isinstance(got, tuple):
        got = (got.total, got.ambiguous, got.unique, got.weights)
    T, amb, U, W = exp
    assert (got[0], got[1], np.asarray(got[2]).tolist()) == (T, amb, U.tolist()), what
    if local:
        assert np.isfinite(got[3]).all(), (what, got[3])
        np.testing.assert_allclose(got[3], W, rtol=W_RTOL, atol=0, err_msg=str(what))


def tune(dev, v):
    dev.tune(ilp=v["ilp"], ilp_local=v["ilp"], kmer_table=v["kmer_table"], ax_scan=v["ax_scan"])


def kernel_of(v, k):
    """last_kernel of a variant: 3 anchor-and-extend, 2 the k-mer table (k <= 31), 0 LF steps."""
    return 3 if v["ax_scan"] else (2 if v["kmer_table"] and k <= 31 else 0)


DEFAULT = VARIANTS[0]


@pytest.mark.parametrize("k", [21, 31, 33, 70])  # compact table, wide table; the anchor kernel's HW = 1, 2, 3
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("local", [False, True])
def test_raw_device_buffers_every_kernel(env, k, paired, local):
    """speq_scan_reads_device on the raw bytes: each kernel decodes them itself."""
    ref, dev = env
    rd = reads_of(ref, 30, paired)
    exp = expected(ref, k, 30, paired, local)
    assert exp[0] > 0 and exp[2].sum() > 0
    try:
        for v in VARIANTS:
            tune(dev, v)
            got = br.device_scan(dev, rd, k, 30, paired, local)
            assert dev.tuning("last_kernel") == kernel_of(v, k), v
            same(got, exp, local, v)
    finally:
        tune(dev, DEFAULT)


@pytest.mark.parametrize("cutoff", [0, 1, 29, 30, 31, 40, 41, 42, 93, 94, 222])
@pytest.mark.parametrize("local", [False, True])
def test_cutoff_sweep(env, cutoff, local):
    """Qualities regenerated per cutoff, so that bytes sit at 33 + cutoff and 34 + cutoff: an off-by-one in the
    threshold byte or in the comparison moves T. Cutoffs >= 41 pass nothing (the clamp stops at 41). Raw device
    buffers on the anchor kernel, the k-mer table and LF steps, and the host path; were a cutoff rejected, every entry
    point would have to reject it alike."""
    ref, dev = env
    k = 21
    rd = reads_of(ref, cutoff)
    exp = expected(ref, k, cutoff, False, local)
    if cutoff >= 41:
        assert exp[0] == 0 and not exp[2].any() and (not local or not exp[3].any())
    else:
        assert exp[0] > 0 and exp[2].sum() > 0
    got, errs = [], []
    try:
        for v in VARIANTS[:3]:
            tune(dev, v)
            try:
                got.append((v, br.device_scan(dev, rd, k, cutoff, False, local)))
                assert dev.tuning("last_kernel") == kernel_of(v, k)
            except SpeqError as e:
                errs.append(e.code)
    finally:
        tune(dev, DEFAULT)
    try:
        got.append(("host", dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, phred_cutoff=cutoff,
                                     local=local)))
    except SpeqError as e:
        errs.append(e.code)
    if errs:
        assert not got and len(set(errs)) == 1 and len(errs) == 4, (errs, [g[0] for g in got])
        return
    for what, g in got:
        same(g, exp, local, what)
        if cutoff >= 41:
            g = g if isinstance(g, tuple) else (g.total, g.ambiguous, g.unique, g.weights)
            assert g[0] == 0 and g[1] == 0 and not np.asarray(g[2]).any()
            assert not local or (g[3] == 0.0).all()


# (k, spacing of the failing bases): at spacing 40 windows of k <= 39 pass between two failing bases and end next to
# one, and no window of 70 passes; at spacing 97 windows of 70 do
@pytest.mark.parametrize("k,spacing", [(8, 40), (12, 40), (21, 40), (33, 40), (70, 40), (70, 97)])
def test_rank0_qualities_next_to_passing_windows(k, spacing):
    """Local mode on the anchor kernel: qualities vary base by base in 31..41 (the product path) and every 40th base
    is '!' (rank 0: its factor is 1 / 0 = inf) or byte 10 (below '!'). Blocks of eight windows are weighed together,
    so a rank-0 factor sits in products of windows outside the block's mask; it must never reach a sum. The bound is
    the one of test_varying_quality_weights_within_the_documented_bound: |W_gpu - W_ref| <= (3k + 2 n_g + 2) 2^-53
    W_ref per group. Group 0's texts are A/T only and group 1's C/G only, so every passing window is counted."""
    rng = np.random.default_rng(1000 * k + spacing)
    recs = [bytes(rng.choice(np.frombuffer(a, dtype=np.uint8), size=1_500)) for a in (b"AT", b"AT", b"CG", b"CG")]
    groups = [0, 0, 1, 1]
    dev = DeviceIndex(FmIndex.build(recs, groups, 2, prefix_q=6, pair_steps=True, triple_steps=True))
    orc = Oracle(recs, groups, 2, k)
    n, L = 300, 150
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seqs = []
    for _ in range(n):
        r = recs[int(rng.integers(0, 4))]
        a = int(rng.integers(0, len(r) - L))
        x = r[a:a + L]
        seqs.append(x.translate(comp)[::-1] if rng.random() < 0.5 else x)
    seq = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    off = np.arange(0, L * n + 1, L, dtype=np.uint64)
    qual = (rng.integers(31, 42, size=seq.size) + 33).astype(np.uint8)
    pos = np.arange(seq.size) % L
    fail = (pos + np.repeat(np.arange(n), L)) % spacing == spacing - 1  # the phase moves from read to read
    qual[fail] = rng.choice(np.array([33, 10], dtype=np.uint8), size=int(fail.sum()))
    reads = synth.Reads(seq, qual, off, np.zeros(n, np.int32))
    T, amb, U, W = orc.scan(seq, qual, off, local=True)
    got = br.device_scan(dev, reads, k, 30, False, True)
    assert dev.tuning("last_kernel") == 3
    assert (got[0], got[1], got[2].tolist()) == (T, amb, U.tolist())
    assert np.isfinite(got[3]).all(), got[3]
    if spacing < k:
        assert T == 0 and (got[3] == 0.0).all()
        return
    assert int(U.sum()) == T and T > 2_000  # enough windows counted for the bound to mean something
    u = 2.0 ** -53
    for g in range(2):
        tol = (3 * k + 2 * int(U[g]) + 2) * u * W[g]
        assert abs(got[3][g] - W[g]) <= tol, (g, got[3][g], W[g], tol)
    host = dev.scan(seq.tobytes(), qual.tobytes(), off, k=k, local=True)
    assert (host.total, host.unique.tolist()) == (T, U.tolist()) and np.isfinite(host.weights).all()
    for g in range(2):
        assert abs(host.weights[g] - W[g]) <= (3 * k + 2 * int(U[g]) + 2) * u * W[g]


@pytest.mark.parametrize("pack", [None, "0", "1"])
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("local", [False, True])
def test_host_path_packers(env, monkeypatch, pack, paired, local):
    """speq_scan_reads: the host packers (3 bits per base in global mode, a byte per base in local mode or with
    SPEQ_HOST_PACK=1; AVX2 bodies with scalar tails) and the unpack kernels behind them, or the raw bytes
    (SPEQ_HOST_PACK=0). Inputs of 31 and 33 bytes are all tail, or one vector and one byte."""
    ref, dev = env
    if pack is None:
        monkeypatch.delenv("SPEQ_HOST_PACK", raising=False)
    else:
        monkeypatch.setenv("SPEQ_HOST_PACK", pack)
    k = 21
    rd = reads_of(ref, 30, paired)
    assert rd.seq.size % 32 != 0
    exp = expected(ref, k, 30, paired, local)
    same(dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, paired=paired, local=local), exp, local)
    if pack is None and not paired:  # the EM histogram's entry point, once in each mode
        em = EmHistogram(dev)
        same(em.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=k, local=local), exp, local, "em")
    orc = oracle_of(ref, k)
    # the first read whose first 33 bytes hold passing windows, cut to 31 and 33 bytes (as two mates: 21 + the rest)
    one = orc.scan(rd.seq[:33], rd.qual[:33], np.array([0, 33], np.uint64))
    r0 = 0
    while one[0] == 0:
        r0 += 1
        a = int(rd.offsets[r0])
        one = orc.scan(rd.seq[a:a + 33], rd.qual[a:a + 33], np.array([0, 33], np.uint64))
    a = int(rd.offsets[r0])
    for nbytes in (31, 33):
        s, q = rd.seq[a:a + nbytes], rd.qual[a:a + nbytes]
        off = np.array([0, 21, nbytes] if paired else [0, nbytes], dtype=np.uint64)
        small = orc.scan(s, q, off, paired=paired, local=local)
        same(dev.scan(s.tobytes(), q.tobytes(), off, k=k, paired=paired, local=local), small, local, nbytes)


def write_fastq(path, reads, lo, step):
    with open(path, "wb") as f:
        for i in range(lo, reads.n, step):
            a, b = int(reads.offsets[i]), int(reads.offsets[i + 1])
            f.write(b"@r%d\n" % i + reads.seq[a:b].tobytes() + b"\n+\n" + reads.qual[a:b].tobytes() + b"\n")


@pytest.mark.parametrize("pack", ["0", "1"])
@pytest.mark.parametrize("paired", [False, True])
def test_fastq_path(env, tmp_path, monkeypatch, pack, paired):
    """speq_scan_fastq: the GPU parser hands the file's text to the kernels, or (SPEQ_FASTQ_PACK=1) the host packs the
    records. Bytes a four-line FASTQ record can hold: letters and * - . as bases, qualities 33..126 ('@' and '!'
    among them, also at the start of a line)."""
    monkeypatch.setenv("SPEQ_FASTQ_PACK", pack)
    ref, dev = env
    rd = reads_of(ref, 30, paired, fastq_safe=True)
    assert rd.seq.min() > 32 and 33 <= rd.qual.min() and rd.qual.max() <= 126
    first = rd.qual[rd.offsets[:-1].astype(np.int64)]
    assert (first == ord("@")).any()  # a quality line that opens like a header
    # a base line with a byte below 'A' sends its block to the general parser; with * - . written as letters every
    # record is a clean four-line record, which the four-line parser and the host's append packers take
    letters = rd.seq.copy()
    for a, b in zip(b"*-.", b"XxZ"):
        letters[letters == a] = b
    assert (letters != rd.seq).any() and letters.min() >= ord("A")
    rd2 = synth.Reads(letters, rd.qual, rd.offsets, rd.variant)
    for tag, r in (("punct", rd), ("letters", rd2)):
        if paired:
            write_fastq(tmp_path / f"{tag}1.fq", r, 0, 2)
            write_fastq(tmp_path / f"{tag}2.fq", r, 1, 2)
            p1, p2 = str(tmp_path / f"{tag}1.fq"), str(tmp_path / f"{tag}2.fq")
        else:
            write_fastq(tmp_path / f"{tag}1.fq", r, 0, 1)
            p1, p2 = str(tmp_path / f"{tag}1.fq"), None
        for local in (False, True):
            # (* - . and X x Z are all N: both files have the same expected counts)
            exp = expected(ref, 21, 30, paired, local, fastq_safe=True)
            assert exp[0] > 0 and exp[2].sum() > 0
            got, st = dev.scan_fastq(p1, p2, k=21, local=local, threads=3)
            same(got, exp, local, (tag, local))
            assert st["records"] == rd.n and st["bases"] == int(rd.offsets[-1])


def test_reference_bytes_host_and_gpu_build(env):
    """References with soft-masked stretches, U / u, IUPAC letters and a '*': the host build and the GPU build read
    them alike (array by array), the .dat pass and a read scan on that index equal the oracle's."""
    ref, _ = env
    rng = np.random.default_rng(17)
    recs = []
    for r in ref.records:
        s = np.frombuffer(r, dtype=np.uint8).copy()
        for _ in range(6):  # lower-case stretches
            a = int(rng.integers(0, s.size - 200))
            s[a:a + int(rng.integers(20, 200))] |= 0x20
        t = ((s | 0x20) == ord("t")) & (rng.random(s.size) < 0.2)
        s[t] += 1  # T -> U, t -> u
        iupac = rng.random(s.size) < 0.002
        s[iupac] = rng.choice(np.frombuffer(br.IUPAC, dtype=np.uint8), size=int(iupac.sum()))
        s[int(rng.integers(0, s.size))] = ord("*")
        recs.append(s.tobytes())
    assert any(c in b"".join(recs) for c in b"u") and b"U" in b"".join(recs)
    kw = dict(prefix_q=8, pair_steps=True, triple_steps=True)
    host = FmIndex.build(recs, ref.groups, G, **kw)
    gpu = FmIndex.build(recs, ref.groups, G, gpu_device=0, **kw)
    for name, dt in ARRAYS:
        x, y = host.array(name, dt), gpu.array(name, dt)
        assert x.shape == y.shape and np.array_equal(x, y), name
    dev = DeviceIndex(gpu)
    for k in (11, 21, 33):
        orc = Oracle(recs, ref.groups, G, k)
        u, t = dev.count_unique_kmers_per_group(k)
        ou, ot = orc.ref_unique()
        assert np.array_equal(u, ou) and np.array_equal(t, ot), (k, u, ou, t, ot)
        assert ou.sum() > 0
    rd = reads_of(ref, 30)
    orc = Oracle(recs, ref.groups, G, 21)
    for local in (False, True):
        exp = orc.scan(rd.seq, rd.qual, rd.offsets, local=local)
        assert exp[2].sum() > 0
        same(br.device_scan(dev, rd, 21, 30, False, local), exp, local)
        same(dev.scan(rd.seq.tobytes(), rd.qual.tobytes(), rd.offsets, k=21, local=local), exp, local)
