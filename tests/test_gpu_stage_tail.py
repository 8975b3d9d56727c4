"""GPU: the last batch of a refill group in k_scan_ax's staging at every group size around a stream
instruction's 64 chunks.

A refill lays the refilling lanes' read pieces end to end as one stream of 16-base chunks and stages it in batches of
SU stream instructions of 64 chunks; the group's last batch executes only the instructions that hold a chunk. With
tuning grid_blocks_ax = 1 there is one workgroup of four waves and wave w's pool is the units [m w, m (w + 1)) of
4 m units: for m <= 64 its first refill stages exactly its m reads (the first mates, when paired) as one group. Every
read here starts at a multiple of 16 bases and is a multiple of 16 long, so a read of 16 c bases is c chunks and the
group's size is chosen exactly: 64 j - 1, 64 j and 64 j + 1 chunks for j = 1 .. 2 SU + 1, four sizes per launch (one
per wave), plus pools of 64 units and of 64 + 8 (a full first group and a second refill). The last chunk before each
multiple of 64 in the stream, the first after it and the group's last chunk each carry an N and a quality below the
cutoff (and, around the boundary, a step in the qualities), so a chunk that is dropped, staged twice or given to the
wrong lane changes T or U. Expected values come from the CPU oracle; the counters also equal those of the scan without
the anchor kernel (tuning ax_scan = 0) bit for bit. W is compared with the oracle to rtol 1e-10 under both tunings and
not bitwise between them: both kernels add it up with floating-point atomics, in an order that varies from run to
run."""
import numpy as np
import pytest

from oracle.oracle import Oracle
from speq_amd import DeviceIndex, FmIndex, synth

pytestmark = pytest.mark.gpu

G = 4
WAVES = 4       # waves of the one workgroup
CMAX = 12       # chunks of the longest read (192 bases: one staging segment)
# name: (k, paired, local, SU)
MODES = {"global-k21": (21, False, False, 3), "global-k70": (70, False, False, 2),
         "paired-k33": (33, True, False, 2), "local-k21": (21, False, True, 3)}


@pytest.fixture(scope="module")
def world():
    ref = synth.make_reference(G, 2, 6_000)
    idx = FmIndex.build(ref.records, ref.groups, G, prefix_q=8, pair_steps=True, triple_steps=True)
    return ref, idx, {}


def chunk_plan(rng, total, n, cmin):
    """n chunk counts in [cmin, CMAX] that sum to total."""
    assert n * cmin <= total <= n * CMAX, (total, n, cmin)
    c = np.full(n, cmin)
    for _ in range(total - n * cmin):
        c[rng.choice(np.flatnonzero(c < CMAX))] += 1
    rng.shuffle(c)
    return c


def launch_input(rng, ref, k, paired, local, totals, m, extra=0):
    """Reads of WAVES pools of m + extra units whose first m units' (first mates') chunks sum to totals[w]."""
    cmin = -(-k // 16)
    step = 2 if paired else 1
    chunks, marks = [], []  # chunks per read; (read, chunk) to plant
    for w, total in enumerate(totals):
        first = chunk_plan(rng, total, m, cmin)
        unit_chunks = np.concatenate([first, rng.integers(cmin, CMAX + 1, extra)])
        r0 = len(chunks)
        for c in unit_chunks:
            chunks.append(int(c))
            if paired:
                chunks.append(int(rng.integers(cmin, CMAX + 1)))
        ends = np.cumsum(first)
        at = sorted({total - 1} | {x for b in range(64, total + 1, 64) for x in (b - 1, b) if x < total})
        for x in at:
            u = int(np.searchsorted(ends, x, side="right"))
            marks.append((r0 + step * u, x - (int(ends[u - 1]) if u else 0), x))
    lens = 16 * np.asarray(chunks, dtype=np.int64)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    seq = np.empty(int(off[-1]), dtype=np.uint8)
    for r, L in enumerate(lens):
        rec = ref.records[int(rng.integers(len(ref.records)))]
        p = int(rng.integers(0, len(rec) - L))
        seq[int(off[r]):int(off[r + 1])] = np.frombuffer(rec[p:p + L], dtype=np.uint8)
    qual = np.full(seq.size, ord("I"), dtype=np.uint8)
    if local:  # runs of other passing qualities: weights of windows that are not of one quality
        for p in rng.integers(0, seq.size - 8, seq.size // 40):
            qual[p:p + int(rng.integers(1, 8))] = ord("F")
    for r, c, x in marks:
        b = int(off[r]) + 16 * c
        seq[b + 3] = ord("N")
        qual[b + 11] = ord("#")
        if x % 64 == 63:
            qual[b + 15] = ord("G")  # a step between this chunk's last quality and the next chunk's first
        if x % 64 == 0:
            qual[b] = ord("H")
    return seq, qual, off


def launches(k, su):
    """(totals per wave, m, extra) of every launch of a mode."""
    out = []
    tiers = ((8, [63, 64, 65]), (20, [127, 128, 129, 191, 192, 193]), (40, [64 * j + d for j in range(4, 2 * su + 2)
                                                                            for d in (-1, 0, 1)]))
    for m, totals in tiers:
        for i in range(0, len(totals), WAVES):
            t = totals[i:i + WAVES]
            out.append((t + t[:WAVES - len(t)], m, 0))
    j = max(2 * su, -(-k // 16) + 1)  # (64 reads of at least k bases hold 64 ceil(k / 16) chunks)
    full = [64 * j - 1, 64 * j, 64 * j + 1, 64 * (j + 1) + 1]
    out.append((full, 64, 0))    # every lane of the first refill stages a read
    out.append((full, 64, 8))    # ... and the pool goes on: a second group
    return out


@pytest.mark.parametrize("mode", list(MODES))
def test_group_sizes_around_a_stream_instruction(world, mode):
    import torch
    ref, idx, oracles = world
    k, paired, local, su = MODES[mode]
    if k not in oracles:
        oracles[k] = Oracle(ref.records, ref.groups, G, k)
    orc = oracles[k]
    dev = DeviceIndex(idx)
    rng = np.random.default_rng(900 + k + paired + 2 * local)
    plan = launches(k, su)
    sizes = {t for totals, _, _ in plan for t in totals}
    assert {64 * j + d for j in range(1, 2 * su + 2) for d in (-1, 0, 1)} <= sizes
    for totals, m, extra in plan:
        seq, qual, off = launch_input(rng, ref, k, paired, local, totals, m, extra)
        T, amb, U, W = orc.scan(seq, qual, off, paired=paired, local=local)
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
            assert got[ax] == (T, amb, U.tolist()), (mode, totals, m, extra, ax)
            if local:
                np.testing.assert_allclose(w.cpu().numpy(), W, rtol=1e-10, atol=0)
        assert got[1] == got[0], (mode, totals, m, extra)
    dev.close()
