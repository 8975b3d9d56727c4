"""Deterministic inputs that put fingerprint collisions and full-bucket chains of the anchor table
where k_scan_ax, k_ax_sbitmap and the EM instantiation must handle them. Chosen with tests/ax_model.py, which restates
the table's hash and sizing; expected results never come from here (oracle.Oracle, tests/em_reference.py).

Per (k, load) of CONFIGS one reference: a backbone like the suite's small references (4 variants x 2 isolates x 2,500
bases, a few N) plus H designed pairs of records. A pair is one random sequence of LD bases in two alleles that differ
at the central base, in two different groups, so the k windows over that base (and their reverse complements) are
unique to their allele's group. H and LD are fixed first: D = D(backbone) + 2 H (LD + 1) is known before any search,
hence nb and nf. The central 2 k - 1 bases of a pair are searched so that one window over the SNP has home bucket and
fingerprint of a backbone key; at load 90 the flanks are searched so that each holds a window homed in the last bucket.

Input classes (each with a control set of the same shape and size that has no collision under the model):
  A  absent k-mers with home bucket and fingerprint of a key, looked up in phase 1: as a read of k bases (their home
     bucket neither full nor receiving overflow: the exact premise), as the first window of a full-length read, and
     as the first window over a substitution in mid-read (a text window with another last base);
  B  the two keys of each designed collision (both loci: which of them sits behind the other is a race): as a read's
     first window, as the window looked up behind a mid-read error (k <= 70; at k = 128 a run, an error and the
     window do not fit one 192-base piece), as a window deferred to phase 2 (a chimeric read:
     reference bases of another place, then the window: the first window over the junction is absent, so those behind
     it that share the run's first mismatch are deferred, and this one is found there), and for k > 64 as window k of
     a read with a substitution in its first k bases (local mode: the speculative run starts from this candidate;
     k = 128 has no speculative run in a 192-base piece, 2 k > 192, the read is kept for the oracle comparison);
  C  read = reference bases, then an absent k-mer that passes the Bloom filter and collides: deferred, then probed
     and verified in phase 2;
  D  (load 90) keys and absent k-mers whose home bucket is full, every key homed in the last bucket (at least 9, so
     one of them lives in bucket 0), absent k-mers homed in the full last bucket (their chain ends in bucket 0 or
     later).
Paired forms put the constructed read in one mate and an ordinary read in the other; a local-mode variant has
qualities 31..41 varying base by base.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import ax_model as am
from speq_amd import synth

CONFIGS = ((21, 35), (21, 90), (70, 35), (70, 90), (33, 35), (128, 35))  # HW = 1..4, sproof k <= 32, SPEC k > 64
BITMAP_CONFIGS = ((21, 35), (21, 90), (31, 35))
EM_CONFIGS = ((21, 35), (21, 90), (70, 35), (70, 90))
G = 4
H = 5            # designed pairs
FLANK = 300      # bases either side of a pair's SNP
LD = 2 * FLANK + 1
N_A = 5          # class-A k-mers, class-C k-mers
N_D = 10         # class-D k-mers per kind


def read_len(k: int) -> int:
    return 150 if k <= 70 else 2 * k + 22


@lru_cache(maxsize=None)
def backbone():
    return synth.make_reference(4, 2, 2_500, ref_n_rate=0.002)


def _piece_windows(pieces: np.ndarray, k: int):
    """Words, piece and offset of every window of every row of a code matrix."""
    n, L = pieces.shape
    flat = np.full((n, L + 1), 4, dtype=np.uint8)
    flat[:, :L] = pieces
    w, valid = am.window_words(flat.reshape(-1), k)
    at = np.flatnonzero(valid)
    return w[at], at // (L + 1), at % (L + 1)


@dataclass
class Design:
    k: int
    load: int
    records: list
    groups: list
    model: am.Model
    n_backbone: int                      # records of the backbone (they come first)
    pairs: list                          # per designed pair: ((text, pos) of its window, (text, pos) of the key)
    D_planned: int
    texts: list = field(default_factory=list)  # text 2 r: record r, 2 r + 1: its reverse complement

    def window(self, locus) -> bytes:
        t, p = locus
        return self.texts[t][p:p + self.k]


@lru_cache(maxsize=None)
def design(k: int, load: int) -> Design:
    bb = backbone()
    bm = am.Model(bb.records, k, load)  # (for its key set; the table's size comes from the planned D)
    D = bm.D + 2 * H * (LD + 1)
    nb, _ = am.sizing(D, load)
    bpair = am.ax_bucket(bm.h, nb).astype(np.int64) * 65536 + am.ax_fp(bm.h).astype(np.int64)
    order = np.argsort(bpair, kind="stable")
    bsorted = bpair[order]
    rng = np.random.default_rng(1_000 * k + load)
    cores = []  # (codes of allele 0, other base, allele, strand, offset, backbone key)
    while len(cores) < H:
        cand = rng.integers(0, 4, size=(256 if k > 64 else 2048, 2 * k - 1), dtype=np.uint8)
        alt = ((cand[:, k - 1] + rng.integers(1, 4, size=len(cand))) % 4).astype(np.uint8)
        other = cand.copy()
        other[:, k - 1] = alt
        hits = {}
        for allele, c in enumerate((cand, other)):
            for strand, p in enumerate((c, (3 - c[:, ::-1]).astype(np.uint8))):
                w, pi, off = _piece_windows(p, k)
                h = am.ax_hash(w, k)
                q = am.ax_bucket(h, nb).astype(np.int64) * 65536 + am.ax_fp(h).astype(np.int64)
                at = np.minimum(np.searchsorted(bsorted, q), len(bsorted) - 1)
                for i in np.flatnonzero(bsorted[at] == q).tolist():
                    hits.setdefault(int(pi[i]), (allele, strand, int(off[i]), int(order[at[i]])))
        for pi in sorted(hits):
            if len(cores) < H:
                cores.append((cand[pi], int(alt[pi])) + hits[pi])

    def flank():
        Lf = FLANK - k + 1
        cand = rng.integers(0, 4, size=(400, Lf), dtype=np.uint8)
        if load < 90:
            return cand[0]
        good = set()
        for p in (cand, (3 - cand[:, ::-1]).astype(np.uint8)):
            w, pi, _ = _piece_windows(p, k)
            good |= set(pi[am.ax_bucket(am.ax_hash(w, k), nb).astype(np.int64) == nb - 1].tolist())
        assert good, "no flank with a window homed in the last bucket"
        return cand[min(good)]

    records, groups = list(bb.records), list(bb.groups)
    pairs = []
    for i, (core, alt, allele, strand, off, key) in enumerate(cores):
        left, right = flank(), flank()
        a = np.concatenate([left, core, right])
        b = a.copy()
        b[FLANK] = alt
        assert len(a) == LD and a[FLANK] != alt
        r0 = len(records)
        records += [bytes(am.ACGT[a]), bytes(am.ACGT[b])]
        groups += [i % G, (i + 1) % G]
        pairs.append(((2 * (r0 + allele) + strand, FLANK - k + 1 + off), (int(bm.key_text[key]), int(bm.key_pos[key]))))
    d = Design(k, load, records, groups, am.Model(records, k, load), len(bb.records), pairs, D)
    d.texts = [s for r in records for s in (bytes(r), am.revcomp(r))]
    return d


# ---------------------------------------------------------------------------------------------------- k-mer searches

def _search(M: am.Model, rng, pred, n: int, batch: int = 1 << 20, max_batches: int = 400) -> np.ndarray:
    """n random k-mers that are absent from the texts and whose hashes satisfy pred."""
    out = []
    for _ in range(max_batches):
        w = am.random_words(rng, batch, M.k)
        sel = np.flatnonzero(pred(am.ax_hash(w, M.k)))
        for i in sel.tolist():
            if not M.contains(w[i:i + 1])[0]:
                out.append(w[i].copy())
                if len(out) == n:
                    return np.asarray(out)
    raise AssertionError(f"search found {len(out)} of {n} k-mers")


def _home(M, h):
    return am.ax_bucket(h, M.nb).astype(np.int64)


@dataclass
class Kmers:
    """The constructed k-mers of one design and their controls, as 2-bit words."""
    A: np.ndarray          # absent, collide, home bucket simple
    A_ctrl: np.ndarray     # absent, no collision, home bucket simple
    A_sub: list            # (key index, base): the key with this last base is absent and collides
    A_sub_ctrl: list       # ... is absent and does not collide
    C: np.ndarray          # absent, pass the Bloom filter, collide
    C_ctrl: np.ndarray     # absent, pass the Bloom filter, no collision
    B_ctrl: list           # pairs of loci (a designed SNP window, a backbone key), neither colliding
    D_keys_full: np.ndarray = None   # key indices whose home bucket is full
    D_keys_last: np.ndarray = None   # key indices homed in bucket nb - 1
    D_keys_ctrl: np.ndarray = None   # key indices in simple buckets, alone with their fingerprint
    D_abs_full: np.ndarray = None    # absent, home bucket full (not the last)
    D_abs_wrap: np.ndarray = None    # absent, homed in the full last bucket
    D_abs_ctrl: np.ndarray = None    # absent, home bucket simple, no collision


@lru_cache(maxsize=None)
def kmers(k: int, load: int) -> Kmers:
    d = design(k, load)
    M = d.model
    rng = np.random.default_rng(7_000 * k + load)
    simple = lambda h: M.simple(_home(M, h))  # noqa: E731
    A = _search(M, rng, lambda h: (M.collisions_h(h) > 0) & simple(h), N_A)
    A_ctrl = _search(M, rng, lambda h: (M.collisions_h(h) == 0) & simple(h), N_A)
    # every key with another last base
    sh = am.U64(2 * ((k - 1) % 32))
    col = (k - 1) // 32
    A_sub, A_sub_ctrl = [], []
    for sub in (1, 2, 3):
        w = M.keys.copy()
        w[:, col] ^= am.U64(sub) << sh
        c = M.collisions(w)
        for i in np.flatnonzero(c > 0).tolist():
            if not M.contains(w[i:i + 1])[0]:
                A_sub.append((i, int((int(w[i, col]) >> int(sh)) & 3)))
    A_sub = sorted(A_sub)[:8]
    i = 0
    while len(A_sub_ctrl) < len(A_sub):
        w = M.keys[i:i + 1].copy()
        w[:, col] ^= am.U64(1) << sh
        if M.collisions(w)[0] == 0 and not M.contains(w)[0]:
            A_sub_ctrl.append((i, int((int(w[0, col]) >> int(sh)) & 3)))
        i = (i + 997) % M.D
    C = _search(M, rng, lambda h: M.bloom_pass_h(h) & (M.collisions_h(h) > 0), N_A)
    C_ctrl = _search(M, rng, lambda h: M.bloom_pass_h(h) & (M.collisions_h(h) == 0), N_A)
    # controls of B: a SNP window of each pair and a backbone key, each alone with its (home bucket, fingerprint)
    own = M.collisions_h(M.h)
    is_bb = M.key_text < 2 * d.n_backbone
    B_ctrl = []
    bb_alone = np.flatnonzero((own == 1) & is_bb)
    for i, (dl, _) in enumerate(d.pairs):
        t = dl[0]
        for off in range(k):
            w = am.kmer_words([d.texts[t][FLANK - k + 1 + off:FLANK + 1 + off]], k)
            if M.collisions(w)[0] == 1:
                break
        else:
            raise AssertionError("no control window")
        j = int(bb_alone[(i + 1) * len(bb_alone) // (H + 2)])
        B_ctrl.append(((t, FLANK - k + 1 + off), (int(M.key_text[j]), int(M.key_pos[j]))))
    out = Kmers(A, A_ctrl, A_sub, A_sub_ctrl, C, C_ctrl, B_ctrl)
    if load >= 90:
        last = M.nb - 1
        assert M.full[last] and M.home_count[last] >= 9
        out.D_keys_last = np.flatnonzero(M.home == last)
        full_keys = np.flatnonzero(M.full[M.home] & (M.home != last))
        out.D_keys_full = full_keys[:: max(1, len(full_keys) // (2 * N_D))][:2 * N_D]
        ctrl = np.flatnonzero(M.simple(M.home) & (own == 1))
        out.D_keys_ctrl = ctrl[:: max(1, len(ctrl) // (2 * N_D))][:2 * N_D]
        out.D_abs_full = _search(M, rng, lambda h: M.full[_home(M, h)] & (_home(M, h) != last), N_D)
        out.D_abs_wrap = _search(M, rng, lambda h: _home(M, h) == last, N_D // 2)
        out.D_abs_ctrl = _search(M, rng, lambda h: (M.collisions_h(h) == 0) & simple(h), N_D)
    return out


# ---------------------------------------------------------------------------------------------------- reads

def _sub(b: int) -> int:
    """Another base."""
    return b"CGTA"[b"ACGT".index(bytes([b]))] if bytes([b]) in b"ACGT" else ord("C")


def _prefixes(d: Design, nexts: list) -> list:
    """Per k-mer of `nexts` an N-free piece of k + 10 reference bases (backbone, forward) behind which no backbone
    record goes on with that k-mer's first base (the records are aligned): whichever of them represents the piece's
    k-mers, a run over piece + k-mer meets its first mismatch at the k-mer's first base, so of the windows deferred for
    it only the k-mer itself lies outside the piece."""
    out, L, p = [], d.k + 10, 37
    bb = d.records[:d.n_backbone]
    while len(out) < len(nexts):
        s = d.texts[2 * (len(out) % d.n_backbone)][p:p + L]
        after = {r[p + L] for r in bb}
        if len(s) == L and b"N" not in s and after <= set(b"ACGT") and nexts[len(out)][0] not in after:
            out.append(s)
        p = (p + 211) % (len(d.texts[0]) - L - 1)
    return out


def _tails(d: Design, n: int, L: int) -> list:
    """n N-free pieces of L reference bases (backbone, reverse complement)."""
    out, p = [], 53
    while len(out) < n:
        s = d.texts[2 * (len(out) % d.n_backbone) + 1][p:p + L]
        if len(s) == L and b"N" not in s:
            out.append(s)
        p = (p + 173) % (len(d.texts[0]) - L)
    return out


def first_window_read(d: Design, locus, L=None) -> bytes:
    t, p = locus
    return d.texts[t][p:p + (L or read_len(d.k))]


def after_error_read(d: Design, locus, cut=None) -> bytes:
    """The window is the first one behind a substituted base at read index e = k + 4: window 0 and a run of five
    windows come before the error, the first window over it is looked up and found absent with the mismatch known, and
    the next phase-1 lookup is this window (unless a proof skips it). cut = 0: the read ends with the window; cut = -1:
    one base earlier, so the window does not exist and everything before it is the same. A locus within k + 5 bases of
    its text's start, or with an N before it in every record that holds it, gives the window as the read's first.
    (k = 128: a run, the error and the window need 2 k + 5 bases, more than one 192-base piece; the read is kept for
    the oracle comparison.)"""
    t, p = locus
    k = d.k
    e = k + 4
    if p - 1 >= e:
        # the backbone's records are aligned copies: any of them that holds the window at p and no N before it will do
        same = [t] + [u for u in range(t % 2, 2 * d.n_backbone, 2) if t < 2 * d.n_backbone and u != t]
        for u in same:
            s = bytearray(d.texts[u][p - 1 - e:p - 1 - e + (read_len(k) if cut is None else e + 1 + k + cut)])
            if d.texts[u][p:p + k] == d.texts[t][p:p + k] and b"N" not in s[:e + 1 + k]:
                s[e] = _sub(s[e])
                return bytes(s)
    return first_window_read(d, locus, None if cut is None else k + cut)


def after_error_premise(k: int, load: int, which: int) -> tuple:
    """(reads that end with the window, the same reads one base shorter) of the class-B loci (which = 0) or their
    controls (1): the difference of the two scans' counters is the window's own lookup."""
    d, km = design(k, load), kmers(k, load)
    loci = [l for pr in (d.pairs if which == 0 else km.B_ctrl) for l in pr]
    return [after_error_read(d, l, 0) for l in loci], [after_error_read(d, l, -1) for l in loci]


def spec_read(d: Design, locus) -> bytes:
    """The window is window k of the read; a substitution inside the first k bases."""
    t, p = locus
    if p < d.k:
        return first_window_read(d, locus)
    s = bytearray(d.texts[t][p - d.k:p - d.k + read_len(d.k)])
    s[d.k // 2] = _sub(s[d.k // 2])
    return bytes(s)


def sub_read(d: Design, key: int, base: int) -> bytes:
    """A read whose first window over its one substitution is the key with `base` as its last base."""
    M, k = d.model, d.k
    t, p = int(M.key_text[key]), int(M.key_pos[key])
    e = min(read_len(k) // 2, p + k - 1)
    s = bytearray(d.texts[t][p + k - 1 - e:p + k - 1 - e + read_len(k)])
    s[e] = b"ACGT"[base]
    return bytes(s)


@lru_cache(maxsize=None)
def read_sets(k: int, load: int) -> dict:
    """{class: (constructed reads, control reads)}; each a list of bytes."""
    d, km = design(k, load), kmers(k, load)
    M = d.model
    asc = lambda W: [am.words_to_ascii(w, k) for w in W]  # noqa: E731
    locus = lambda i: (int(M.key_text[i]), int(M.key_pos[i]))  # noqa: E731
    out = {}
    tails = _tails(d, 4 * N_D, read_len(k) - k)
    with_tail = lambda ks: [q + tails[i % len(tails)] for i, q in enumerate(ks)]  # noqa: E731
    out["A_k"] = (asc(km.A), asc(km.A_ctrl))
    out["A_first"] = (with_tail(asc(km.A)), with_tail(asc(km.A_ctrl)))
    out["A_sub"] = ([sub_read(d, i, b) for i, b in km.A_sub], [sub_read(d, i, b) for i, b in km.A_sub_ctrl])
    loci = [l for pr in d.pairs for l in pr]
    cloci = [l for pr in km.B_ctrl for l in pr]

    def chim(ls):
        pre = _prefixes(d, [d.window(l) for l in ls])
        # (k > 70: piece + window exceed one 192-base piece; nothing behind the window, so that whatever the
        # pieces are, every other window over the junction is absent and the window is the only deferred one found)
        L = read_len(k) - len(pre[0]) if k <= 70 else k
        return [pre[i] + first_window_read(d, l, L) for i, l in enumerate(ls)]

    out["B_k"] = ([d.window(l) for l in loci], [d.window(l) for l in cloci])
    out["B_first"] = ([first_window_read(d, l) for l in loci], [first_window_read(d, l) for l in cloci])
    out["B_after"] = ([after_error_read(d, l) for l in loci], [after_error_read(d, l) for l in cloci])
    out["B_deferred"] = (chim(loci), chim(cloci))
    if k > 64:
        out["B_spec"] = ([spec_read(d, l) for l in loci], [spec_read(d, l) for l in cloci])
    out["C"] = tuple([p + q for p, q in zip(_prefixes(d, qs), qs)] for qs in (asc(km.C), asc(km.C_ctrl)))
    if load >= 90:
        ctrl_keys = [locus(i) for i in km.D_keys_ctrl]
        n_last = len(km.D_keys_last)
        out["D_keys_full"] = ([d.window(locus(i)) for i in km.D_keys_full] +
                              [first_window_read(d, locus(i)) for i in km.D_keys_full],
                              [d.window(l) for l in ctrl_keys] + [first_window_read(d, l) for l in ctrl_keys])
        rep = [ctrl_keys[i % len(ctrl_keys)] for i in range(n_last)]
        out["D_keys_last"] = ([d.window(locus(i)) for i in km.D_keys_last] +
                              [first_window_read(d, locus(i)) for i in km.D_keys_last],
                              [d.window(l) for l in rep] + [first_window_read(d, l) for l in rep])
        out["D_abs_full"] = (asc(km.D_abs_full) + with_tail(asc(km.D_abs_full)),
                             asc(km.D_abs_ctrl) + with_tail(asc(km.D_abs_ctrl)))
        n_wrap = len(km.D_abs_wrap)
        out["D_abs_wrap"] = (asc(km.D_abs_wrap) + with_tail(asc(km.D_abs_wrap)),
                             asc(km.D_abs_ctrl[:n_wrap]) + with_tail(asc(km.D_abs_ctrl[:n_wrap])))
    return out


def pack(reads: list, qual: str = "uniform", seed: int = 0) -> synth.Reads:
    """uniform: Q40 everywhere; vary: qualities 31..41 changing base by base."""
    seq = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
    off = np.zeros(len(reads) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    if qual == "uniform":
        q = np.full(seq.size, ord("I"), dtype=np.uint8)
    else:
        q = (np.random.default_rng(seed).integers(31, 42, size=seq.size) + 33).astype(np.uint8)
    return synth.Reads(seq, q, off, np.zeros(len(reads), dtype=np.int32))


@lru_cache(maxsize=None)
def ordinary(k: int, n: int) -> tuple:
    """n ordinary reads of the backbone (1 % errors, a few N), as bytes."""
    r = synth.make_reads(backbone(), n, read_len=read_len(k), err_rate=0.01, n_rate=0.001)
    return tuple(r.seq[int(a):int(b)].tobytes() for a, b in zip(r.offsets[:-1], r.offsets[1:]))


def as_pairs(reads: list, k: int) -> list:
    """Mate pairs (records 2 i, 2 i + 1): the constructed read as one mate, alternately the first or the second, an
    ordinary read as the other."""
    other = ordinary(k, 2_000)
    out = []
    for i, r in enumerate(reads):
        out += [r, other[i % len(other)]] if i % 2 == 0 else [other[i % len(other)], r]
    return out


def all_reads(k: int, load: int, which: int = 0) -> list:
    """Every class's constructed (which = 0) or control (1) reads, three times over, among 2,000 ordinary reads."""
    mine = [r for _, sets in sorted(read_sets(k, load).items()) for r in sets[which]]
    other = list(ordinary(k, 2_000))
    step = max(1, len(other) // (3 * len(mine) + 1))
    out = []
    it = iter(mine * 3)
    for i, o in enumerate(other):
        out.append(o)
        if i % step == 0:
            nxt = next(it, None)
            if nxt is not None:
                out.append(nxt)
    out += list(it)
    return out
