"""Pure Python / numpy model of the bootstrap's per-replicate EM histograms (speq_bootstrap_attach_em / _finalize_em,
speq_em_rows_refine): over em_reference and bootstrap_model only, nothing shared with the library.

Per unit (a read, or the pair 2i, 2i + 1) the multiset of contents of its multi-group windows: em_reference.scan's
multi_at gives the starts, the dictionary the content ((group, occurrences), ...) of each start's k-mer. Replicate b's
histogram is M[b][content] = sum_u w(u, b) n_u(content), w being bootstrap_model's weights; row 0 (every weight 1) is
the scan's merged histogram. A replicate is refined by api.em_refine with em_reference.exact_step rounded to f64 as
its step."""
from __future__ import annotations

from collections import Counter
from dataclasses import dataclass

import numpy as np

import bootstrap_model as bm
import em_reference as er
from speq_amd import em_refine, unique_to_percent


@dataclass
class MultiUnits:
    """Per unit, what the histogram sees of it."""
    n: int                  # units
    by_content: list        # per unit: Counter {content: windows}
    by_kmer: list           # per unit: Counter {k-mer: windows} (one interval per k-mer: the unmerged rows)
    content_of: dict        # k-mer -> content
    hist: er.Histogram      # em_reference.scan of the same reads


def multi_units(index: dict, G: int, k: int, seq, qual, offsets, cutoff: int = 30, paired: bool = False) -> MultiUnits:
    h = er.scan(index, G, k, seq, qual, offsets, cutoff, paired)
    s5 = er.dna5(seq.tobytes() if isinstance(seq, np.ndarray) else bytes(seq))
    off = [int(v) for v in offsets]
    per = 2 if paired else 1
    nu = (len(off) - 1) // per
    by_content, by_kmer, content_of = [], [], {}
    for u in range(nu):
        kc: Counter = Counter()
        for r in range(per * u, per * u + per):
            a = off[r]
            for j in h.multi_at[r]:
                kc[s5[a + j:a + j + k]] += 1
        cc: Counter = Counter()
        for w, n in kc.items():
            c = index[w]
            content_of[w] = c
            cc[c] += n
        by_content.append(cc)
        by_kmer.append(kc)
    return MultiUnits(nu, by_content, by_kmer, content_of, h)


def tile_profiles(index: dict, k: int, seq, offsets, h: er.Histogram) -> set:
    """{(multi-group windows, distinct k-mers among them, distinct contents among them)} over every tile of 64 window
    starts of every read: what the kernel's slot rounds see of a tile."""
    s5 = er.dna5(seq.tobytes() if isinstance(seq, np.ndarray) else bytes(seq))
    off = [int(v) for v in offsets]
    out = set()
    for r, at in enumerate(h.multi_at):
        tiles: dict = {}
        for j in at:
            tiles.setdefault(j // 64, []).append(s5[off[r] + j:off[r] + j + k])
        for ws in tiles.values():
            out.add((len(ws), len(set(ws)), len({index[w] for w in ws})))
    return out


def _matrix(per_unit: list, col_of: dict, n_cols: int, seed: int, B: int, first_unit: int, n_total):
    """([B + 1, n_cols] uint64 with cell (b, col_of[key]) = sum_u w(u, b) n_u(key), windows whose key has no column)."""
    n0 = len(per_unit)
    n_total = n0 if n_total is None else n_total
    wsum = np.zeros((B + 1, n0), dtype=np.int64)  # per unit of the list, the summed weights of its copies
    copies = np.zeros(n0, dtype=np.int64)
    for start in range(0, n_total, n0):
        m = min(n0, n_total - start)
        idx = np.arange(m, dtype=np.uint64) + np.uint64((first_unit + start) & bm.M64)
        wsum[:, :m] += bm.weights(seed, idx, B)
        copies[:m] += 1
    us, cols, ns = [], [], []
    missed = 0
    for u, c in enumerate(per_unit):
        for key, n in c.items():
            col = col_of.get(key)
            if col is None:
                missed += n * int(copies[u])
                continue
            us.append(u)
            cols.append(col)
            ns.append(n)
    M = np.zeros((B + 1, n_cols), dtype=np.int64)
    if us:
        us, cols, ns = np.array(us), np.array(cols), np.array(ns, dtype=np.int64)
        order = np.argsort(cols, kind="stable")
        us, cols, ns = us[order], cols[order], ns[order]
        starts = np.flatnonzero(np.concatenate([[True], cols[1:] != cols[:-1]]))
        M[:, cols[starts]] = np.add.reduceat(wsum[:, us] * ns[None, :], starts, axis=1)
    return M.astype(np.uint64), missed


def mult(mu: MultiUnits, contents: list, seed: int, B: int, first_unit: int = 0, n_total: int = None):
    """(M [B + 1, len(contents)] uint64 in the order of `contents` (the merged rows' contents), missed): missed counts
    the multi-group windows whose content is not among `contents` (unweighted, as the library counts them)."""
    return _matrix(mu.by_content, {c: i for i, c in enumerate(contents)}, len(contents), seed, B, first_unit, n_total)


def mult_by_kmer(mu: MultiUnits, seed: int, B: int):
    """The unmerged histogram as a multiset: Counter of (content, tuple of the k-mer's B + 1 multiplicities)."""
    kmers = sorted(mu.content_of)
    M, _ = _matrix(mu.by_kmer, {w: i for i, w in enumerate(kmers)}, len(kmers), seed, B, 0, None)
    return Counter((mu.content_of[w], tuple(M[:, i].tolist())) for i, w in enumerate(kmers))


def mult_in_table(mu: MultiUnits, table: MultiUnits, contents: list, seed: int, B: int):
    """mult() when the attached histogram is `table`'s (a subset of the reads): a window counts iff its k-mer, that is
    its interval, is one of the table's; every other multi-group window is missed."""
    col_of = {c: i for i, c in enumerate(contents)}
    known = {w: col_of[c] for w, c in table.content_of.items()}
    return _matrix(mu.by_kmer, known, len(contents), seed, B, 0, None)


def csr(contents: list):
    """(row_ptr u64, col_group u32, col_count u32) of rows with these contents, as speq_em_rows lays them out."""
    ptr = np.zeros(len(contents) + 1, dtype=np.uint64)
    ptr[1:] = np.cumsum([len(c) for c in contents])
    grp = np.array([g for c in contents for g, _ in c], dtype=np.uint32)
    cnt = np.array([n for c in contents for _, n in c], dtype=np.uint32)
    return ptr, grp, cnt


def exact_step_f64(contents: list, m_row, group_counts, unique):
    """percent -> em_reference.exact_step over {content: multiplicity}, each component rounded to f64."""
    merged = {c: int(m) for c, m in zip(contents, m_row) if int(m)}

    def step(percent):
        return np.array([float(x) for x in er.exact_step(percent, group_counts, unique, merged)], dtype=np.float64)
    return step


def refine_row(contents, m_row, counts_row, weights_row, u_ref, tot_ref, group_counts, unique_scale, precision,
               max_iterations, step=None):
    """(percent [G], iterations) of one replicate: the CLI's loop (api.em_refine) from unique_to_percent of the row. A
    row without a passing window is zeros and 0 iterations."""
    G = len(group_counts)
    total = int(counts_row[0])
    if total == 0:
        return [0.0] * G, 0
    unique = [int(x) for x in counts_row[2:]]
    ut = [float(x) for x in weights_row] if weights_row is not None else \
        [float(np.float64(x) * np.float64(unique_scale)) for x in unique]
    p0 = unique_to_percent(ut, total, [float(int(x)) for x in u_ref], [float(int(x)) for x in tot_ref])
    step = step or exact_step_f64(contents, m_row, group_counts, unique)
    its = em_refine(step, ut, total, p0, precision, max_iterations)
    return (its[-1][0] if its else p0), len(its)


def tsv_lines(names, cis) -> list:
    return bm.tsv_lines(names, cis)
