"""The anchor table's arithmetic in numpy (speq_amd/csrc/ax_common.hpp and build_ax of ax_scan.hip).

Used only to CHOOSE inputs and to STATE PREMISES (tests/ax_collision_inputs.py): which k-mers share home bucket and
fingerprint, which buckets are full, how far a chain runs, which k-mers pass the Bloom filter. It never produces an
expected result: those come from oracle.Oracle and tests/em_reference.py, which share nothing with it.

Restated here:
  * 2-bit packing: base i of a k-mer at bits 2 (i mod 32) of word i / 32, A C G T = 0 1 2 3;
  * ax_fmix (murmur3 fmix64), ax_hash (seed 0x9E3779B97F4A7C15 * (k + 1), one fmix per word, the partial last word
    masked, words past the k-mer ignored), ax_bucket (the hash's high 32 bits scaled to nb), ax_fp (its low 16 bits),
    ax_fword / ax_fbits (one 64-bit filter word per key, three bits in it);
  * the sizing nb = floor(D * 100 / (8 * load)) + 1 buckets of 8 slots and nf = max(1, D * 16 / 64) filter words, D
    the distinct N-free k-mers of all texts (every record forward and reverse-complemented);
  * the occupancy of every bucket under linear probing over buckets without deletions. The SET of occupied slots
    does not depend on the order of insertion, so the model knows which buckets are full, which receive keys homed
    in earlier buckets, and after how many buckets a chain from any home bucket meets an empty slot.

What the model cannot know: WITHIN a chain, which key sits in which slot. k_ax_insert places keys with atomicCAS in
whatever order the threads arrive, so of two keys with equal home bucket and fingerprint either may come first, and
which of nine keys homed in the last bucket spills into bucket 0 differs from build to build. No test may depend on
it; inputs cover both loci of a colliding pair, and premises are lower bounds except where a bucket is neither full
nor receives overflow (then its slots are exactly its home keys and counts are exact). For the same reason a
collision at slot 7 of a full bucket (the probe slot becoming 8) cannot be forced.
"""
from __future__ import annotations

import numpy as np

U64 = np.uint64
SEED = 0x9E3779B97F4A7C15
FILTER_BITS = 16
SLOTS = 8
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[ord(chr(_c).lower())] = _i
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def codes_of(seq) -> np.ndarray:
    """ASCII -> 0..3, 4 for anything else (N)."""
    return _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]


def n_words(k: int) -> int:
    return (k + 31) // 32


def window_words(codes: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """(words [n_windows, ceil(k / 32)] u64, valid [n_windows]) of every window of a code array (N coded as A in the
    words, such windows not valid)."""
    nwin = len(codes) - k + 1
    if nwin <= 0:
        return np.zeros((0, n_words(k)), dtype=U64), np.zeros(0, dtype=bool)
    c = np.where(codes < 4, codes, 0).astype(U64)
    out = np.zeros((nwin, n_words(k)), dtype=U64)
    for i in range(k):
        out[:, i // 32] |= c[i:i + nwin] << U64(2 * (i % 32))
    bad = np.concatenate([[0], np.cumsum(codes >= 4)])
    return out, (bad[k:] - bad[:nwin]) == 0


def kmer_words(kmers, k: int) -> np.ndarray:
    """Words of a list of ASCII k-mers (all ACGT)."""
    out = np.zeros((len(kmers), n_words(k)), dtype=U64)
    for r, s in enumerate(kmers):
        c = codes_of(s)
        assert len(c) == k and (c < 4).all()
        out[r] = window_words(c, k)[0][0]
    return out


def words_to_ascii(words: np.ndarray, k: int) -> bytes:
    return bytes(ACGT[[(int(words[i // 32]) >> (2 * (i % 32))) & 3 for i in range(k)]])


def random_words(rng, n: int, k: int) -> np.ndarray:
    """n uniformly random k-mers as words (bits past the k-mer zero)."""
    w = rng.integers(0, 1 << 64, size=(n, n_words(k)), dtype=U64)
    rem = k - 32 * (n_words(k) - 1)
    if rem < 32:
        w[:, -1] &= U64((1 << (2 * rem)) - 1)
    return w


def ax_fmix(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> U64(33))
    x = x * U64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> U64(33))
    x = x * U64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> U64(33))


def ax_hash(words: np.ndarray, k: int) -> np.ndarray:
    """Hash of k-mers given as rows of 2-bit words; columns past ceil(k / 32) are ignored."""
    words = np.asarray(words, dtype=U64)
    h = np.full(words.shape[0], (SEED * (k + 1)) & 0xFFFFFFFFFFFFFFFF, dtype=U64)
    for i in range(words.shape[1]):
        if 32 * i < k:
            rem = k - 32 * i
            x = words[:, i]
            if rem < 32:
                x = x & U64((1 << (2 * rem)) - 1)
            h = ax_fmix(h ^ x)
    return h


def ax_bucket(h: np.ndarray, nb: int) -> np.ndarray:
    return ((h >> U64(32)) * U64(nb)) >> U64(32)


def ax_fp(h: np.ndarray) -> np.ndarray:
    return h & U64(0xFFFF)


def ax_fword(h: np.ndarray, nf: int) -> np.ndarray:
    return (((h >> U64(24)) & U64(0xFFFFFFFF)) * U64(nf)) >> U64(32)


def ax_fbits(h: np.ndarray) -> np.ndarray:
    one = U64(1)
    return (one << (h & U64(63))) | (one << ((h >> U64(6)) & U64(63))) | (one << ((h >> U64(12)) & U64(63)))


def sizing(D: int, load: int) -> tuple[int, int]:
    """(nb, nf) as build_ax computes them (the division in double, truncated)."""
    return max(1, int(float(D) * 100.0 / (8.0 * load)) + 1), max(1, D * FILTER_BITS // 64)


def revcomp(s: bytes) -> bytes:
    return bytes(s).translate(bytes.maketrans(b"ACGTNacgtn", b"TGCANTGCAN"))[::-1]


def text_windows(records, k: int):
    """Words, text index (2 r: record r forward, 2 r + 1: its reverse complement) and start of every N-free window
    of every text."""
    ws, ts, ps = [], [], []
    for r, rec in enumerate(records):
        for strand, s in enumerate((bytes(rec), revcomp(rec))):
            w, valid = window_words(codes_of(s), k)
            at = np.flatnonzero(valid)
            ws.append(w[at])
            ts.append(np.full(len(at), 2 * r + strand, dtype=np.int64))
            ps.append(at)
    return np.concatenate(ws), np.concatenate(ts), np.concatenate(ps)


def occupancy(home_count: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(occupied slots, keys received from earlier buckets) per bucket, from the number of keys homed in each: a key
    that finds its bucket full goes to the next one (bucket nb - 1 to bucket 0). Needs sum < 8 * nb."""
    nb = len(home_count)
    assert int(home_count.sum()) < SLOTS * nb
    cnt = home_count.tolist()
    occ, cin = [0] * nb, [0] * nb
    carry = 0
    for _ in range(3):  # the carry into bucket 0 is final after one round (some bucket has room)
        start = carry
        for b in range(nb):
            cin[b] = carry
            have = cnt[b] + carry
            occ[b] = min(SLOTS, have)
            carry = have - occ[b]
        if carry == start:
            break
    else:
        raise AssertionError("occupancy did not settle")
    return np.asarray(occ, dtype=np.int64), np.asarray(cin, dtype=np.int64)


class Model:
    """The anchor table of (records, k, load) as far as it is determined."""

    def __init__(self, records, k: int, load: int):
        assert 1 <= load <= 90, "ax_load is capped at 90: 8 * nb > D, so every chain meets an empty slot"
        self.k, self.load = k, load
        words, text, pos = text_windows(records, k)
        self.n_windows = len(words)
        self.keys, first = np.unique(words, axis=0, return_index=True)
        self.key_text, self.key_pos = text[first], pos[first]  # one occurrence of every key
        self.D = len(self.keys)
        self.nb, self.nf = sizing(self.D, load)
        self.h = ax_hash(self.keys, k)
        self.home = ax_bucket(self.h, self.nb).astype(np.int64)
        self.fp = ax_fp(self.h).astype(np.int64)
        self.pair = self.home * 65536 + self.fp
        self.pair_sorted = np.sort(self.pair)
        self.filt = np.zeros(self.nf, dtype=U64)
        np.bitwise_or.at(self.filt, ax_fword(self.h, self.nf).astype(np.int64), ax_fbits(self.h))
        self.home_count = np.bincount(self.home, minlength=self.nb)
        self.occ, self.carry_in = occupancy(self.home_count)
        self.full = self.occ == SLOTS
        # buckets a lookup homed in b loads before it meets an empty slot (if no slot stops it earlier)
        self.chain = np.ones(self.nb, dtype=np.int64)
        for _ in range(2):
            for b in range(self.nb - 1, -1, -1):
                if self.full[b]:
                    self.chain[b] = 1 + self.chain[(b + 1) % self.nb]
        self._set = None

    def contains(self, words: np.ndarray) -> np.ndarray:
        if self._set is None:
            self._set = {r.tobytes() for r in self.keys}
        return np.asarray([np.ascontiguousarray(r).tobytes() in self._set for r in np.asarray(words, dtype=U64)],
                          dtype=bool)

    def pair_of(self, words: np.ndarray):
        h = ax_hash(words, self.k)
        return h, ax_bucket(h, self.nb).astype(np.int64), ax_fp(h).astype(np.int64)

    def collisions_h(self, h: np.ndarray) -> np.ndarray:
        """Keys with the home bucket and the fingerprint of each hash (a key's own hash counts the key itself)."""
        q = ax_bucket(h, self.nb).astype(np.int64) * 65536 + ax_fp(h).astype(np.int64)
        return np.searchsorted(self.pair_sorted, q, side="right") - np.searchsorted(self.pair_sorted, q, side="left")

    def collisions(self, words: np.ndarray) -> np.ndarray:
        return self.collisions_h(ax_hash(words, self.k))

    def bloom_pass_h(self, h: np.ndarray) -> np.ndarray:
        bits = ax_fbits(h)
        return (self.filt[ax_fword(h, self.nf).astype(np.int64)] & bits) == bits

    def bloom_pass(self, words: np.ndarray) -> np.ndarray:
        return self.bloom_pass_h(ax_hash(words, self.k))

    def simple(self, bucket: np.ndarray) -> np.ndarray:
        """Buckets that are not full and receive no key from an earlier bucket: their slots are exactly their home
        keys, and every chain that starts in them ends in them."""
        return ~self.full[bucket] & (self.carry_in[bucket] == 0)
