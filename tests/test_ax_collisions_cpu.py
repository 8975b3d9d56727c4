"""No GPU: the numpy model of the anchor table (tests/ax_model.py) is self-consistent, every constructed input of
tests/ax_collision_inputs.py satisfies its premise under the model, and the inputs are not vacuous for the oracle: a
lookup that went wrong on them would change T-independent counts (U) or leave absent windows counted."""
import numpy as np
import pytest

import ax_collision_inputs as ci
import ax_model as am
from oracle.oracle import Oracle

ALL = tuple(dict.fromkeys(ci.CONFIGS + ci.BITMAP_CONFIGS))
IDS = [f"k{k}-load{load}" for k, load in ALL]


def brute_distinct(records, k):
    seen = set()
    for r in records:
        for s in (bytes(r), am.revcomp(r)):
            for i in range(len(s) - k + 1):
                w = s[i:i + k]
                if b"N" not in w:
                    seen.add(w)
    return seen


@pytest.mark.parametrize("k", [1, 21, 32, 33, 64, 70, 96, 97, 128])
def test_model_hash_ignores_words_past_k_and_ranges_hold(k):
    rng = np.random.default_rng(k)
    w = am.random_words(rng, 2_000, k)
    junk = rng.integers(0, 1 << 64, size=(2_000, 4), dtype=np.uint64)
    wide = junk.copy()
    wide[:, :w.shape[1]] = w
    rem = k - 32 * (w.shape[1] - 1)
    if rem < 32:  # junk above the k-mer inside its last word too
        wide[:, w.shape[1] - 1] |= junk[:, 0] << np.uint64(2 * rem)
    h = am.ax_hash(w, k)
    assert np.array_equal(h, am.ax_hash(wide, k))
    assert len(np.unique(h)) == len(np.unique(w, axis=0))  # (fmix is a bijection; a k-mer's words are its identity)
    for nb in (1, 7, 5_551, 14_272, (1 << 26) - 1):
        b = am.ax_bucket(h, nb)
        assert int(b.max()) < nb
        assert int(am.ax_fword(h, nb).max()) < nb
    assert int(am.ax_fp(h).max()) < 1 << 16 and np.array_equal(am.ax_fp(h), h & np.uint64(0xFFFF))
    bits = am.ax_fbits(h)
    pop = np.array([bin(int(x)).count("1") for x in bits[:200]])
    assert ((pop >= 1) & (pop <= 3)).all()


def test_model_packing_and_seed():
    w = am.kmer_words([b"ACGT" * 9], 36)  # base i at bits 2 (i mod 32) of word i / 32
    assert int(w[0, 0]) == int("11100100" * 8, 2) and int(w[0, 1]) == 0b11100100
    assert am.words_to_ascii(w[0], 36) == b"ACGT" * 9
    # fmix64 in Python integers, and the seed of an empty key
    def fmix(x):
        m = 2 ** 64 - 1
        x ^= x >> 33
        x = x * 0xFF51AFD7ED558CCD & m
        x ^= x >> 33
        x = x * 0xC4CEB9FE1A85EC53 & m
        return x ^ (x >> 33)
    for x in (1, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF):
        assert int(am.ax_fmix(np.array([x], dtype=np.uint64))[0]) == fmix(x)
    assert int(am.ax_hash(np.zeros((1, 1), dtype=np.uint64), 21)[0]) == int(
        am.ax_fmix(np.array([(am.SEED * 22) & (2 ** 64 - 1)], dtype=np.uint64))[0])
    assert am.sizing(40_000, 35) == (14_286, 10_000) and am.sizing(3, 90) == (1, 1)


def test_occupancy_by_insertion():
    """The closed form against inserting the keys one by one, in two different orders."""
    rng = np.random.default_rng(3)
    nb = 50
    home = np.concatenate([rng.integers(0, nb, 300), np.full(20, nb - 1)])
    occ, cin = am.occupancy(np.bincount(home, minlength=nb))
    for order in (home, home[::-1]):
        slots = [0] * nb
        for b in order.tolist():
            while slots[b] == 8:
                b = (b + 1) % nb
            slots[b] += 1
        assert slots == occ.tolist()
    assert occ.sum() == len(home) and cin[0] > 0


@pytest.fixture(scope="module", params=ALL, ids=IDS)
def cfg(request):
    k, load = request.param
    return ci.design(k, load), ci.kmers(k, load), ci.read_sets(k, load)


def test_distinct_count_and_occupancy(cfg):
    d, km, _ = cfg
    M = d.model
    brute = brute_distinct(d.records, d.k)
    assert M.D == len(brute) == d.D_planned, "the designed windows are not all new: nb differs from the planned one"
    assert {am.words_to_ascii(w, d.k) for w in M.keys[::97]} <= brute
    assert (M.nb, M.nf) == am.sizing(M.D, d.load) and 8 * M.nb > M.D
    assert int(M.occ.sum()) == M.D and int(M.home.max()) < M.nb
    assert ((M.occ == 8) == M.full).all() and (M.chain[~M.full] == 1).all() and (M.chain[M.full] >= 2).all()


def test_designed_windows_are_new_distinct_and_collide(cfg):
    d, km, _ = cfg
    M, k = d.model, d.k
    backbone = brute_distinct(d.records[:d.n_backbone], k)
    designed = [w for r in d.records[d.n_backbone:] for s in (bytes(r), am.revcomp(r))
                for w in (s[i:i + k] for i in range(len(s) - k + 1))]
    assert not backbone & set(designed)
    assert len(set(designed)) == 2 * ci.H * (ci.LD + 1)  # the two alleles share all but the 2 k windows over the SNP
    for dl, bl in d.pairs:
        wd, wb = d.window(dl), d.window(bl)
        assert wb in backbone and wd not in backbone and dl[1] <= ci.FLANK < dl[1] + k
        _, b, f = M.pair_of(am.kmer_words([wd, wb], k))
        assert b[0] == b[1] and f[0] == f[1]
        assert M.collisions(am.kmer_words([wd], k))[0] >= 2
    for dl, bl in km.B_ctrl:
        assert (M.collisions(am.kmer_words([d.window(dl), d.window(bl)], k)) == 1).all()


def test_constructed_kmers_satisfy_their_premises(cfg):
    d, km, _ = cfg
    M, k = d.model, d.k
    brute = brute_distinct(d.records, k)
    asc = lambda W: [am.words_to_ascii(w, k) for w in W]  # noqa: E731
    for name in ("A", "A_ctrl", "C", "C_ctrl"):
        assert not set(asc(getattr(km, name))) & brute, name
    home = lambda W: M.pair_of(W)[1]  # noqa: E731
    assert (M.collisions(km.A) >= 1).all() and M.simple(home(km.A)).all()
    assert (M.collisions(km.A_ctrl) == 0).all() and M.simple(home(km.A_ctrl)).all()
    assert (M.collisions(km.C) >= 1).all() and M.bloom_pass(km.C).all()
    assert (M.collisions(km.C_ctrl) == 0).all() and M.bloom_pass(km.C_ctrl).all()
    assert M.bloom_pass(M.keys).all()  # (the filter holds every key)
    assert len(km.A_sub) >= 1 and len(km.A_sub) == len(km.A_sub_ctrl)
    for (i, base), want in [(x, True) for x in km.A_sub] + [(x, False) for x in km.A_sub_ctrl]:
        q = am.words_to_ascii(M.keys[i], k)[:-1] + b"ACGT"[base:base + 1]
        assert q not in brute and (M.collisions(am.kmer_words([q], k))[0] > 0) == want
    if d.load >= 90:
        last = M.nb - 1
        assert len(km.D_keys_last) >= 9 and (M.home[km.D_keys_last] == last).all() and M.full[last]
        assert M.carry_in[0] >= len(km.D_keys_last) - 8 >= 1  # the last bucket spills into bucket 0
        assert M.full[M.home[km.D_keys_full]].all() and not M.full[M.home[km.D_keys_ctrl]].any()
        assert not set(asc(km.D_abs_full) + asc(km.D_abs_wrap) + asc(km.D_abs_ctrl)) & brute
        assert M.full[home(km.D_abs_full)].all() and (M.chain[home(km.D_abs_full)] >= 2).all()
        assert (home(km.D_abs_wrap) == last).all() and M.chain[last] >= 2
        assert not M.full[home(km.D_abs_ctrl)].any()


def test_inputs_are_not_vacuous_for_the_oracle(cfg):
    d, km, rs = cfg
    k = d.k
    orc = Oracle(d.records, d.groups, ci.G, k)

    def scan(reads):
        r = ci.pack(reads)
        return orc.scan(r.seq, r.qual, r.offsets)

    # A and C: the k-mer is a passing window that no group counts
    for q in [am.words_to_ascii(w, k) for w in np.concatenate([km.A, km.C])]:
        T, amb, U, _ = scan([q])
        assert T == 1 and int(U.sum()) == 0 and orc.lookup(q) < 0
    for name in ("A_k", "A_first", "A_sub", "C"):
        for r in rs[name][0]:
            assert len(r) >= k and b"N" not in r[:k]
    # B: the designed window is unique to its allele's group (a missed lookup changes U)
    for (dl, bl) in d.pairs:
        rec = dl[0] // 2
        T, amb, U, _ = scan([d.window(dl)])
        assert T == 1 and U.tolist() == [int(g == d.groups[rec]) for g in range(ci.G)]
    # every set and its control have the same size (reads near a text end are shorter)
    for name, (a, b) in rs.items():
        assert len(a) == len(b) and all(len(x) >= k for x in a + b), name


def test_read_forms_put_the_window_where_they_say(cfg):
    d, km, rs = cfg
    k, L = d.k, d.k + 10
    loci = [l for pr in d.pairs for l in pr]
    behind = 0
    for l, full in zip(loci, rs["B_after"][0]):
        w, wo = ci.after_error_read(d, l, 0), ci.after_error_read(d, l, -1)
        assert w.endswith(d.window(l)) and wo == w[:-1] and full.startswith(w)
        if len(w) > k:  # one substitution at index k + 4 >= k - 1: window 0 is clean, the window follows the error
            t, p = l
            texts = [d.texts[u][p - k - 5:p + k] for u in range(t % 2, len(d.texts), 2)]  # (aligned copies)
            assert len(w) == 2 * k + 5 and b"N" not in w
            assert any([i for i in range(len(w)) if w[i] != x[i]] == [k + 4] for x in texts if len(x) == len(w))
            behind += 1
    assert behind >= ci.H  # (every designed locus lies deep inside its record)
    # chimeric reads: no backbone record continues the piece with the window's first base
    for name in ("B_deferred", "C"):
        for r in rs[name][0] + rs[name][1]:
            at = [(i, rec.find(r[:L])) for i, rec in enumerate(d.records[:d.n_backbone]) if r[:L] in rec]
            assert at and all(rec[at[0][1] + L] != r[L] for rec in d.records[:d.n_backbone]), name
