"""Pure-Python / numpy model of the duplicate-read pass (speq_dedup_*): integers only, uint64 wrap-around.

A unit is a record, or the pair of records (2i, 2i + 1). Base code c: A C G T/U in either case 0..3, every other byte 4
(the scan's dna5 conversion). Fingerprint (F_0, F_1):
    F_s = sum over mates m and positions i of mix(S_s + g (1 + c + 5 i + (m << 40)))   (mod 2^64)
with mix splitmix64's finaliser. Two units are duplicates iff their fingerprints are equal; rep[u] is the lowest unit of
u's class and u is kept iff rep[u] == u. classes_exact groups the units by their converted sequences instead, and
tests/test_dedup_cpu.py checks that both agree on every input of the suite."""
from __future__ import annotations

import numpy as np

G64 = np.uint64(0x9E3779B97F4A7C15)
S = (np.uint64(0x243F6A8885A308D3), np.uint64(0x13198A2E03707344))
BINS = 8

_CODE = np.full(256, 4, dtype=np.uint64)
for _ch, _c in zip(b"ACGTUacgtu", (0, 1, 2, 3, 3, 0, 1, 2, 3, 3)):
    _CODE[_ch] = _c


def codes(seq) -> np.ndarray:
    """Base codes (u64) of a byte string or u8 array."""
    a = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)
    return _CODE[a]


def mix(z: np.ndarray) -> np.ndarray:
    """splitmix64's finaliser on a u64 array (wrap-around multiplies)."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _terms(code: np.ndarray, pos: np.ndarray, mate: np.ndarray):
    """The per-base terms of both streams (two u64 arrays)."""
    with np.errstate(over="ignore"):
        x = G64 * (np.uint64(1) + code + np.uint64(5) * pos + (mate << np.uint64(40)))
        return mix(S[0] + x), mix(S[1] + x)


def fingerprint(seq1: bytes, seq2: bytes = None) -> tuple[int, int]:
    f = [0, 0]
    for m, s in enumerate((seq1, seq2)):
        if not s:
            continue
        n = len(s)
        t = _terms(codes(s), np.arange(n, dtype=np.uint64), np.full(n, m, dtype=np.uint64))
        for j in (0, 1):
            f[j] = (f[j] + int(t[j].sum(dtype=np.uint64))) & (2 ** 64 - 1)
    return f[0], f[1]


def fingerprints(seq: bytes, offsets, paired: bool) -> np.ndarray:
    """[n_units, 2] u64 of packed records (all units at once: one segmented sum per stream)."""
    off = np.asarray(offsets, dtype=np.int64)
    n_rec = len(off) - 1
    per = 2 if paired else 1
    assert n_rec % per == 0
    n_units = n_rec // per
    base, total = int(off[0]), int(off[-1] - off[0])
    out = np.zeros((n_units, 2), dtype=np.uint64)
    if total == 0:
        return out
    lens = np.diff(off)
    rec_of = np.repeat(np.arange(n_rec, dtype=np.int64), lens)
    pos = (np.arange(total, dtype=np.int64) - (off[:-1] - base)[rec_of]).astype(np.uint64)
    mate = (rec_of % per).astype(np.uint64)
    c = codes(np.frombuffer(seq, dtype=np.uint8)[base:base + total])
    t0, t1 = _terms(c, pos, mate)
    unit_of = rec_of // per
    # segmented wrap-around sums: the units' bases are contiguous, so cumulative sums at the unit ends
    ends = np.searchsorted(unit_of, np.arange(n_units), side="right")
    for j, t in enumerate((t0, t1)):
        with np.errstate(over="ignore"):
            cs = np.concatenate([[np.uint64(0)], np.cumsum(t, dtype=np.uint64)])
            starts = np.concatenate([[0], ends[:-1]])
            out[:, j] = cs[ends] - cs[starts]
    return out


def unit_keys(seq: bytes, offsets, paired: bool) -> list:
    """Per unit, the tuple of its mates' dna5-coded sequences: equal keys are equal units, exactly."""
    off = [int(x) for x in offsets]
    per = 2 if paired else 1
    c = codes(seq).astype(np.uint8).tobytes()
    recs = [c[off[r]:off[r + 1]] for r in range(len(off) - 1)]
    return [tuple(recs[per * u:per * u + per]) for u in range(len(recs) // per)]


def _rep_of(keys) -> np.ndarray:
    first: dict = {}
    rep = np.zeros(len(keys), dtype=np.uint32)
    for u, key in enumerate(keys):
        rep[u] = first.setdefault(key, u)
    return rep


def rep_exact(seq: bytes, offsets, paired: bool) -> np.ndarray:
    """rep[] with classes by exact comparison of the converted sequences."""
    return _rep_of(unit_keys(seq, offsets, paired))


def rep_fingerprint(seq: bytes, offsets, paired: bool) -> np.ndarray:
    """rep[] with classes by fingerprint: the definition."""
    return _rep_of([(int(a), int(b)) for a, b in fingerprints(seq, offsets, paired)])


def stats(rep: np.ndarray) -> dict:
    n = len(rep)
    sizes = np.bincount(rep, minlength=1)[np.unique(rep)] if n else np.zeros(0, dtype=np.int64)
    hist = np.zeros(BINS, dtype=np.uint64)
    for s in sizes.tolist():
        hist[min(s, BINS) - 1] += 1
    return {"units": n, "distinct": int(len(sizes)), "max_multiplicity": int(sizes.max()) if n else 0,
            "mult_hist": hist}


def mask(qual: bytes, offsets, rep: np.ndarray, paired: bool) -> bytes:
    """qual with '!' over every record of a unit that is not kept."""
    off = [int(x) for x in offsets]
    per = 2 if paired else 1
    q = bytearray(qual)
    for r in range(len(off) - 1):
        u = r // per
        if rep[u] != u:
            q[off[r]:off[r + 1]] = b"!" * (off[r + 1] - off[r])
    return bytes(q)


def remove(seq: bytes, qual: bytes, offsets, rep: np.ndarray, paired: bool):
    """(seq, qual, offsets) of the kept units only."""
    off = [int(x) for x in offsets]
    per = 2 if paired else 1
    keep = [r for r in range(len(off) - 1) if rep[r // per] == r // per]
    new = np.zeros(len(keep) + 1, dtype=np.uint64)
    new[1:] = np.cumsum([off[r + 1] - off[r] for r in keep])
    return (b"".join(seq[off[r]:off[r + 1]] for r in keep), b"".join(qual[off[r]:off[r + 1]] for r in keep), new)
