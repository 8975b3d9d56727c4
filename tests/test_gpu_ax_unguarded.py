"""GPU: k_scan_ax's phase-1 reads of a lane's own slot without bounds guards (SPEQ_AX_LEAN).

A run reads 11 code rows from the row of its slot position whatever the piece's length, and 6 valid-window dwords from
its window's; what lies past the piece is the previous pieces' codes in the same slot, and past the slot's rows the
wave's other arrays (valid-window words, the deferred list). The result must not depend on any of it: the first
mismatch is clamped to the bases left, the windows are masked to the run, the valid-bit searches stop at the piece's
last window. The launches here put such content next to short pieces on purpose.

tuning grid_blocks_ax = 1: one workgroup of four waves, wave w's pool the units [m w, m (w + 1)) of 4 m. Reads follow
each other without gaps, so a read's 16-byte phase (its first base's slot position) is set by the lengths before it:
reads shorter than k and empty reads fill up to the phase wanted, and empty reads pad every wave's block to m units.
  wave 0  64 reads of 192 bases of one locus at slot position 15 (every lane of the first refill stages one; they are
          equal, so all 64 lanes finish in the same iteration), then reads of k .. k + 3 bases that are prefixes of the
          same locus at the same phase: whichever lane takes one, the rows past its end hold the text's continuation
  wave 1  the same with the short reads from another locus: the stale rows differ from the text
  wave 2  reads of 191, 192 and 193 bases (193: a second segment of one window, first and last at once), clean and with
          one substitution that makes a run start at the piece's last window, at the window after the segment boundary,
          or after a broken first window
  wave 3  error-dense reads with N and failing qualities in neighbouring lanes (deferred list and the words after the
          valid-window words not zero while the unguarded reads run), reads shorter than k and empty ones between them
Paired: the blocks' reads are taken two by two (wave 0 and 1: a 192-base first mate, then its short prefix as the second
mate in the same lane). Every case equals the CPU oracle and the scan without the anchor kernel (tuning ax_scan = 0) bit
for bit; W to rtol 1e-10 against the oracle (floating-point atomics in an order that varies)."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from speq_amd import DeviceIndex, EmHistogram, FmIndex, synth

pytestmark = pytest.mark.gpu

G = 4
LONG = 192
SHORTS = 16  # short reads after the long ones, per block
# name: (k, paired, local)
SHAPES = {"global-k5": (5, False, False), "global-k21": (21, False, False), "global-k33": (33, False, False),
          "global-k70": (70, False, False), "global-k128": (128, False, False), "local-k21-varq": (21, False, True),
          "paired-k33": (33, True, False)}


@pytest.fixture(scope="module")
def world():
    ref = synth.make_reference(G, 2, 6_000)
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=True, triple_steps=True)
    return ref, idx, {}


def oracle_for(world, k):
    ref, _, oracles = world
    if k not in oracles:
        oracles[k] = Oracle(ref.records, ref.groups, G, k)
    return oracles[k]


class Block:
    """The reads of one wave's pool: (bases, qualities) in order, and the byte at which the next read starts."""

    def __init__(self, at):
        self.reads, self.at = [], at

    def add(self, seq, qual=None):
        seq = np.asarray(seq, dtype=np.uint8)
        self.reads.append((seq, np.full(len(seq), ord("I"), dtype=np.uint8) if qual is None else qual))
        self.at += len(seq)

    def fill_to(self, phase, k, rng):
        """Reads shorter than k (random bases) and an empty one, so that the next read starts at `phase` mod 16."""
        gap = (phase - self.at) % 16
        while gap:
            n = min(gap, k - 1)
            self.add(synth.ACGT[rng.integers(0, 4, n)])
            gap -= n
        self.add([])

    def even(self):
        if len(self.reads) % 2:
            self.add([])


def locus(ref, rng, n):
    rec = np.frombuffer(ref.records[int(rng.integers(len(ref.records)))], dtype=np.uint8)
    p = int(rng.integers(0, len(rec) - n))
    return rec[p:p + n].copy()


def other_base(b, rng):
    return synth.ACGT[(int(np.flatnonzero(synth.ACGT == b)[0]) + 1 + int(rng.integers(3))) % 4]


def stale_block(at, ref, rng, k, paired, same_locus):
    b = Block(at)
    b.fill_to(15, k, rng)
    b.even()
    long_read = locus(ref, rng, LONG)
    src = long_read if same_locus else locus(ref, rng, LONG)
    shorts = [src[:k + (i % 4)] for i in range(SHORTS)]
    if paired:  # (192-base first mate, short second mate): the next pair starts at phase 15 again
        for s in shorts:
            b.add(long_read)
            b.add(s)
            b.fill_to(15, k, rng)
            b.even()
        return b
    for _ in range(64):
        b.add(long_read)  # (192 bases: the phase stays 15)
    for s in shorts:
        b.add(s)
        b.fill_to(15, k, rng)
    return b


def boundary_block(at, ref, rng, k):
    b = Block(at)
    b.fill_to(15, k, rng)
    for L in (191, 192, 193):
        for rep in range(3):
            base = locus(ref, rng, L)
            # a substitution at base x breaks the windows x - k + 1 .. x: the next run starts at window x + 1
            for x in (None, L - k - 1, LONG - k, 0, k - 1):
                r = base.copy()
                if x is not None and 0 <= x < L:
                    r[x] = other_base(r[x], rng)
                b.add(r)
            if rep == 1:
                b.fill_to(int(rng.integers(16)), k, rng)
    return b


def dense_block(at, ref, rng, k, seed):
    b = Block(at)
    reads = synth.make_reads(ref, 72, read_len=150, start_index=1000 * seed, err_rate=0.06, n_rate=0.01, lowq_rate=0.03,
                             short_frac=0.1)
    off = reads.offsets.astype(np.int64)
    for r in range(reads.n):
        b.add(reads.seq[off[r]:off[r + 1]], reads.qual[off[r]:off[r + 1]].copy())
        if r % 6 == 5:
            b.fill_to(int(rng.integers(16)), k, rng)
    return b


def launch_input(ref, k, paired, local, seed):
    rng = np.random.default_rng(seed)
    blocks = [stale_block(0, ref, rng, k, paired, True)]  # (a block starts at the byte the one before ends at)
    blocks.append(stale_block(blocks[-1].at, ref, rng, k, paired, False))
    blocks.append(boundary_block(blocks[-1].at, ref, rng, k))
    blocks.append(dense_block(blocks[-1].at, ref, rng, k, seed))
    m = max(len(b.reads) for b in blocks)
    m += m % 2  # (paired: whole pairs per pool)
    for b in blocks:  # empty reads up to m units: no byte more
        while len(b.reads) < m:
            b.add([])
    reads = []
    for b in blocks:
        reads += b.reads
    seq = np.concatenate([s for s, _ in reads])
    qual = np.concatenate([q for _, q in reads])
    if local:  # runs of other passing qualities: windows that are not of one quality
        for p in rng.integers(0, seq.size - 8, seq.size // 40):
            keep = qual[p:p + 7] == ord("I")
            qual[p:p + 7][keep] = ord("F")
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s, _ in reads])
    return seq, qual, off, m


def check_layout(seq, off, k, paired, m):
    """The layout is what the docstring says: wave 0's and 1's long reads and short prefixes stand at slot position 15."""
    starts, lens = off[:-1].astype(np.int64), np.diff(off.astype(np.int64))
    for w in (0, 1):
        lo, hi = w * m, (w + 1) * m
        long_at = [r for r in range(lo, hi) if lens[r] == LONG]
        short_at = [r for r in range(lo, hi) if k <= lens[r] <= k + 3]
        assert len(long_at) == (SHORTS if paired else 64) and len(short_at) == SHORTS
        assert all(starts[r] % 16 == 15 for r in long_at + short_at)
        if paired:
            assert all(r % 2 == 0 and lens[r + 1] in range(k, k + 4) for r in long_at)
        else:
            assert long_at == list(range(long_at[0], long_at[0] + 64)) and min(short_at) > long_at[-1]
        if w == 0:  # prefixes of the long read's locus
            assert all(bytes(seq[starts[r]:starts[r] + lens[r]]) == bytes(seq[starts[long_at[0]]:starts[long_at[0]] + lens[r]])
                       for r in short_at)
    assert (lens == 0).sum() > 0 and ((lens > 0) & (lens < k)).sum() > 0


@pytest.mark.parametrize("shape", list(SHAPES))
def test_stale_rows_and_short_pieces(world, shape):
    import torch
    ref, idx, _ = world
    k, paired, local = SHAPES[shape]
    orc = oracle_for(world, k)
    seq, qual, off, m = launch_input(ref, k, paired, local, 4100 + k + paired + 2 * local)
    check_layout(seq, off, k, paired, m)
    assert len(off) - 1 == 4 * m and len(off) - 1 <= 800
    T, amb, U, W = orc.scan(seq, qual, off, paired=paired, local=local)
    assert T > 0 and (k == 5 or int(U.sum()) > 0)  # (every 5-mer occurs in every group: T alone counts)
    dev = DeviceIndex(idx)
    d_seq, d_qual = torch.from_numpy(seq).cuda(), torch.from_numpy(qual).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    got = {}
    for ax in (1, 0):
        dev.tune(ax_scan=ax, grid_blocks_ax=1)
        cnt = torch.zeros(G + 2, dtype=torch.int64, device="cuda")
        w = torch.zeros(G, dtype=torch.float64, device="cuda")
        dev.scan_device(d_seq.data_ptr(), d_qual.data_ptr(), d_off.data_ptr(), len(off) - 1, k, cnt.data_ptr(),
                        w.data_ptr() if local else 0, paired=paired, local=local)
        torch.cuda.synchronize()
        assert (dev.tuning("last_kernel") == 3) == (ax == 1)
        c = cnt.cpu().numpy()
        got[ax] = (int(c[0]), int(c[1]), c[2:].tolist())
        assert got[ax] == (T, amb, U.tolist()), (shape, ax)
        if local:
            np.testing.assert_allclose(w.cpu().numpy(), W, rtol=1e-10, atol=0)
    assert got[1] == got[0]
    dev.close()


def test_em_scan(world):
    """The EM histogram of the same launch (k = 21): counts equal the oracle's, and counts, histogram and one EM step
    equal those of the scan without the anchor kernel."""
    ref, idx, _ = world
    k = 21
    seq, qual, off, m = launch_input(ref, k, False, False, 4200)
    T, amb, U, _ = oracle_for(world, k).scan(seq, qual, off)
    res = []
    for ax in (1, 0):
        dev = DeviceIndex(idx)
        dev.tune(ax_scan=ax, grid_blocks_ax=1)
        em = EmHistogram(dev)
        r = em.scan(seq.tobytes(), qual.tobytes(), off, k=k)
        em.finalize()
        assert (dev.tuning("last_kernel") == 3) == (ax == 1)
        assert (r.total, r.ambiguous, r.unique.tolist()) == (T, amb, U.tolist()), ax
        res.append((em.info(), em.step(np.linspace(10.0, 40.0, G), [2] * G, r.unique).tolist()))
        dev.close()
    assert res[0] == res[1]
