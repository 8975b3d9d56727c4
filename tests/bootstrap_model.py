"""Pure Python / numpy model of the read bootstrap (speq_bootstrap_*): no GPU, no C, nothing shared with the library.

Per unit (a read, or the pair 2i, 2i + 1) over em_reference.build_index's dictionary: P passing windows, c[g] windows
unique to group g, amb = two or more non-zero c[g], and in local mode x[g], the sum over those windows of the Phred
weight prod_i 1 / (1 - 10^(-q_i / 10)) (each window's product in extended precision, a unit's windows summed with
math.fsum). The weight function is restated from its definition, its thresholds recomputed with decimals. replicates()
gives the two matrices the library must return; summary() restates speq_bootstrap_summary."""
from __future__ import annotations

import math
from dataclasses import dataclass
from decimal import ROUND_FLOOR, Decimal, getcontext
from functools import lru_cache

import numpy as np

import em_reference as er

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
N_THRESHOLDS = 21
HEADER = "name\tpercent\tmean\tse\tlo\thi\tused\n"
LD = np.longdouble


# ---- the weight function ----
@lru_cache(maxsize=None)
def thresholds() -> tuple:
    """C_j = floor(2^64 e^-1 sum_{i <= j} 1 / i!), j = 0 .. 20, from 80-digit decimals."""
    getcontext().prec = 80
    e_inv = 1 / Decimal(1).exp()
    out, s, f = [], Decimal(0), Decimal(1)
    for j in range(N_THRESHOLDS):
        if j:
            f *= j
        s += 1 / f
        out.append(int((Decimal(2) ** 64 * e_inv * s).to_integral_value(rounding=ROUND_FLOOR)))
    assert all(0 < c <= M64 for c in out) and sorted(set(out)) == out
    return tuple(out)


def mix_int(z: int) -> int:
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_int(seed: int, unit: int, b: int) -> int:
    """h(seed, unit, b) with Python integers."""
    x = mix_int((seed + GAMMA * (unit + 1)) & M64)
    return mix_int((x + GAMMA * b) & M64)


def weight_int(seed: int, unit: int, b: int) -> int:
    if b == 0:
        return 1
    h = draw_int(seed, unit, b)
    return sum(h >= c for c in thresholds())


def _mix(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def weights(seed: int, units: np.ndarray, B: int) -> np.ndarray:
    """[B + 1, len(units)] int64: row b holds replicate b's weight of every unit index (u64) in `units`."""
    u = np.asarray(units, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = _mix(np.uint64(seed & M64) + np.uint64(GAMMA) * (u + np.uint64(1)))
        b = np.arange(1, B + 1, dtype=np.uint64)
        h = _mix(x[None, :] + np.uint64(GAMMA) * b[:, None])
    w = np.searchsorted(np.array(thresholds(), dtype=np.uint64), h, side="right").astype(np.int64)  # #{j: C_j <= h}
    return np.concatenate([np.ones((1, len(u)), dtype=np.int64), w], axis=0)


# ---- the units ----
@dataclass
class Units:
    G: int
    P: np.ndarray    # [n] int64
    amb: np.ndarray  # [n] int64, 0 / 1
    c: np.ndarray    # [n, G] int64
    x: np.ndarray    # [n, G] float64, or None (global mode)

    @property
    def n(self) -> int:
        return len(self.P)


def units(index: dict, G: int, k: int, seq, qual, offsets, cutoff: int = 30, paired: bool = False,
          local: bool = False) -> Units:
    seq_b = seq.tobytes() if isinstance(seq, np.ndarray) else bytes(seq)
    qual_b = qual.tobytes() if isinstance(qual, np.ndarray) else bytes(qual)
    off = [int(v) for v in offsets]
    n = len(off) - 1
    per = 2 if paired else 1
    if n % per:
        raise ValueError("a paired bootstrap needs an even record count")
    s5 = er.dna5(seq_b)
    s_arr = np.frombuffer(s5, dtype=np.uint8)
    q_arr = np.frombuffer(qual_b, dtype=np.uint8)
    # ln(1 / (1 - 10^(-q / 10))) in extended precision; a passing window holds only q > cutoff >= 0
    qs = np.arange(42, dtype=LD)
    log_inv = np.zeros(42, dtype=LD)
    log_inv[1:] = -np.log1p(-np.power(LD(10), -qs[1:] / LD(10)))
    nu = n // per
    P = np.zeros(nu, dtype=np.int64)
    c = np.zeros((nu, G), dtype=np.int64)
    x = np.zeros((nu, G), dtype=np.float64) if local else None
    for u in range(nu):
        terms = [[] for _ in range(G)]
        for r in range(per * u, per * u + per):
            a, b = off[r], off[r + 1]
            wins = er.passing_windows(s_arr[a:b], q_arr[a:b], k, cutoff).tolist()
            P[u] += len(wins)
            if not wins:
                continue
            if local:
                q = np.clip(q_arr[a:b].astype(np.int64) - 33, 0, 41)
                cs = np.concatenate([np.zeros(1, dtype=LD), np.cumsum(log_inv[q])])
                xw = np.exp(cs[k:] - cs[:-k]).astype(np.float64)  # every window's weight (used where it passes)
            for j in wins:
                hit = index.get(s5[a + j:a + j + k])
                if hit is None or len(hit) != 1:
                    continue
                g = hit[0][0]
                c[u, g] += 1
                if local:
                    terms[g].append(float(xw[j]))
        if local:
            for g in range(G):
                x[u, g] = math.fsum(terms[g])
    amb = ((c > 0).sum(axis=1) >= 2).astype(np.int64)
    return Units(G, P, amb, c, x)


def replicates(un: Units, seed: int, B: int, first_unit: int = 0, n_total: int = None):
    """(counts [B + 1, G + 2] uint64, weights [B + 1, G] float64 or None) of the units first_unit .. first_unit +
    n_total - 1, unit first_unit + i being un's unit i % un.n (n_total = None: un's units once; larger: the read set
    repeated end to end, the last repeat cut after a unit)."""
    n0 = un.n
    n_total = n0 if n_total is None else n_total
    wsum = np.zeros((B + 1, n0), dtype=np.int64)  # per unit of un, the summed weights of its copies
    for start in range(0, n_total, n0):
        m = min(n0, n_total - start)
        idx = (np.arange(m, dtype=np.uint64) + np.uint64((first_unit + start) & M64))
        with np.errstate(over="ignore"):
            wsum[:, :m] += weights(seed, idx, B)
    counts = np.zeros((B + 1, un.G + 2), dtype=np.int64)
    counts[:, 0] = wsum @ un.P
    counts[:, 1] = wsum @ un.amb
    counts[:, 2:] = wsum @ un.c
    w = None
    if un.x is not None:
        w = (wsum.astype(LD) @ un.x.astype(LD)).astype(np.float64)  # products exact, sums to 2^-64 per term
    return counts.astype(np.uint64), w


# ---- the summary ----
def _percent(counts, wts, b, g, u_ref, tot_ref, scale) -> float:
    """unique_to_percent (fm_scanner.cpp:1455-1474) of row b, in f64 like the library."""
    if not float(tot_ref[g]) > 0.0:
        return 0.0
    ur = np.float64(wts[b][g]) if wts is not None else np.float64(int(counts[b][2 + g])) * np.float64(scale)
    pu = np.float64(int(u_ref[g])) / np.float64(int(tot_ref[g]))
    with np.errstate(all="ignore"):
        return float(np.float64(100.0) * ur / np.float64(int(counts[b][0])) / pu)


def summary(counts, wts, u_ref, tot_ref, scale: float = 1.0, level: float = 0.95) -> list:
    """Per group {"estimate", "mean", "se", "lo", "hi", "used"}."""
    B, G = len(counts) - 1, len(counts[0]) - 2
    out = []
    for g in range(G):
        v = [_percent(counts, wts, b, g, u_ref, tot_ref, scale) for b in range(1, B + 1) if int(counts[b][0]) != 0]
        n = len(v)
        ci = {"estimate": _percent(counts, wts, 0, g, u_ref, tot_ref, scale), "mean": 0.0, "se": 0.0, "lo": 0.0,
              "hi": 0.0, "used": n}
        if n:
            s = 0.0
            for t in v:
                s += t
            ci["mean"] = s / n
            if n >= 2:
                q = 0.0
                for t in v:
                    q += (t - ci["mean"]) * (t - ci["mean"])
                ci["se"] = math.sqrt(q / (n - 1))
            sv = sorted(v)
            t = int(math.floor(n * (1.0 - level) / 2.0))
            ci["lo"], ci["hi"] = sv[t], sv[n - 1 - t]
        out.append(ci)
    return out


def tsv_lines(names, cis) -> list:
    return [HEADER] + ["%s\t%.6f\t%.6f\t%.6f\t%.6f\t%.6f\t%d\n" % (nm, c["estimate"], c["mean"], c["se"], c["lo"],
                                                                  c["hi"], c["used"]) for nm, c in zip(names, cis)]


def weights_bound(k: int, counts: np.ndarray) -> np.ndarray:
    """[B + 1, G] relative tolerance of the library's local weights: (3 k + n + 2) 2^-53 with n the windows that
    contribute to the cell (the counts cell itself)."""
    return (3.0 * k + counts[:, 2:].astype(np.float64) + 2.0) * 2.0 ** -53
