"""The scan kernels' dispatch, restated by hand: which template instantiation every scan must launch.

The three read-scan kernels are templates and the host dispatcher (plan_scan and compiled() in scan_plan.hpp, from
the facts launch_scan in scan_kernels.hip and ax_facts in ax_scan.hip gather) picks one of about 200 separately
compiled instantiations from the scan's parameters. This file reads nothing from the library: `predict` is the rules
written down again, `ALL_VARIANTS` the set the rules can produce, enumerated on its own, and `PLAN` one recipe or more
per variant. tests/test_variant_table_cpu.py holds the three against each other without a GPU and
tests/test_scan_plan_cpu.py holds the library's plan against them, also without one;
tests/test_gpu_variants.py runs every recipe, asserts that the replica reports the predicted instantiation (tuning key
"last_variant") and compares its results with the references.

One thing the rules do not state: a replica keeps the k-mer table of a k in the form it had when it was first built
(compact or wide), so "kt_compact" set afterwards changes nothing for that k. The plan therefore never sets it: the
compact form is reached at k = 21 and the wide form at k = 25.
"""
from __future__ import annotations

from itertools import product
from typing import NamedTuple

K_SCAN, K_SCAN_KT, K_SCAN_AX = "k_scan", "k_scan_kt", "k_scan_ax"
FAMILIES = (K_SCAN, K_SCAN_KT, K_SCAN_AX)
MODES = ("global", "local", "ref")
LDS_HIST_MAX_G = 2048


class Variant(NamedTuple):
    family: str          # K_SCAN, K_SCAN_KT, K_SCAN_AX
    mode: str            # "global", "local", "ref" (the reference-uniqueness pass)
    paired: bool
    lds_hist: bool       # the tally in LDS (G <= 2048), else global atomics
    em: bool
    width: int           # NWIN (k_scan), NW (k_scan_kt), HW (k_scan_ax)
    kt: bool = False     # k_scan reads a (wide) k-mer table
    compact: bool = False  # k_scan_kt reads the compact table (CK)
    sproof: bool = False   # k_scan_ax with the substitution-bitmap path (SP)
    stats: bool = False    # k_scan_ax's instrumented twin

    def pack(self) -> int:
        """The value of tuning key "last_variant" (the layout include/speq_scan.h documents)."""
        return (FAMILIES.index(self.family) | MODES.index(self.mode) << 2 | int(self.paired) << 4 |
                int(self.lds_hist) << 5 | int(self.em) << 6 | self.width << 7 | int(self.kt) << 10 |
                int(self.compact) << 11 | int(self.sproof) << 12 | int(self.stats) << 13)

    def __str__(self) -> str:
        flags = [self.mode, "paired" if self.paired else "single", "lds" if self.lds_hist else "atomics"]
        flags += ["EM"] if self.em else []
        flags.append({K_SCAN: "NWIN", K_SCAN_KT: "NW", K_SCAN_AX: "HW"}[self.family] + str(self.width))
        flags += [n for n, on in (("KT", self.kt), ("CK", self.compact), ("SP", self.sproof), ("STATS", self.stats))
                  if on]
        return f"{self.family}<{', '.join(flags)}>"


def unpack(x: int) -> Variant:
    return Variant(FAMILIES[x & 3], MODES[x >> 2 & 3], bool(x >> 4 & 1), bool(x >> 5 & 1), bool(x >> 6 & 1),
                   x >> 7 & 7, bool(x >> 10 & 1), bool(x >> 11 & 1), bool(x >> 12 & 1), bool(x >> 13 & 1))


# ---------------------------------------------------------------- the two references (tests/variant_inputs.py)
class RefShape(NamedTuple):
    n_variants: int
    n_isolates: int
    length: int
    ref_n_rate: float

    @property
    def G(self) -> int:
        return self.n_variants

    @property
    def text_len(self) -> int:
        """Symbols of the index's text: every record and its reverse complement, a separator each, one terminator."""
        return 2 * self.n_variants * self.n_isolates * (self.length + 1) + 1


REFS = {"g5": RefShape(5, 2, 3000, 0.001),      # the LDS plane
        "g2049": RefShape(2049, 1, 220, 0.0)}   # the smallest G past LDS_HIST_MAX_G: global atomics
# The replicas of tests/test_gpu_big_k.py (k past the anchor kernel and every table): `predict` takes recipes on them,
# the plan and ALL_VARIANTS do not. Only G enters the rules at those k (their texts are not of this shape: three
# records of tests/big_k_inputs.py under labels up to G - 1).
BIG_K_REFS = {"big3": RefShape(3, 1, 12000, 0.0), "big2048": RefShape(2048, 1, 12000, 0.0),
              "big2049": RefShape(2049, 1, 12000, 0.0)}


# ---------------------------------------------------------------- recipes
SCAN, EM, STATS, REF = "scan", "em", "stats", "ref"   # DeviceIndex.scan, EmHistogram.scan, scan_device_stats,
#                                                       count_unique_kmers_per_group


class Recipe(NamedTuple):
    ref: str
    k: int
    paired: bool
    local: bool
    entry: str
    tune: tuple = ()     # (key, value) pairs set on top of DEFAULTS

    @property
    def id(self) -> str:
        t = "".join(f"-{a}{b}" for a, b in self.tune)
        return f"{self.ref}-k{self.k}-{'pe' if self.paired else 'se'}-{'local' if self.local else 'global'}-" \
               f"{self.entry}{t}"


# The tuning a replica of either reference opens with (both indexes have fewer than 4 M symbols: "ilp" 2). The ledger
# sets all of them before every recipe, so a recipe's own keys never leak into the next.
DEFAULTS = dict(ax_scan=1, ax_sproof=2, kmer_table=1, kt_pipeline=1, kt_compact=1, ilp_kt=0, ilp=2, ilp_local=1)


def mfilter_m(text_len: int, k: int) -> int:
    """m of the anchor structures' m-mer filter: the smallest m >= 12 with 4^m >= 200 n, kept only when one probe
    covers 12 windows or more (k - m + 1 >= 12); 0: no filter."""
    m = 12
    while m < 32 and 4 ** m < 200 * text_len:
        m += 1
    return m if k + 1 >= m + 12 else 0


def read_len(k: int) -> int:
    return 200 if k >= 96 else 150


def predict(r: Recipe) -> Variant:
    shape = REFS[r.ref] if r.ref in REFS else BIG_K_REFS[r.ref]
    assert r.ref in REFS or r.k > 128, "the shapes of BIG_K_REFS state G alone"
    t = dict(DEFAULTS)
    t.update(dict(r.tune))
    k = r.k
    lds = shape.G <= LDS_HIST_MAX_G
    table = bool(t["kmer_table"]) and 1 <= k <= 31
    compact = table and k <= 23 and bool(t["kt_compact"])
    wide = table and not compact
    if r.entry == REF:  # never paired, never EM, never the anchor or the pipelined kernel; a compact table is not read
        assert not r.paired and not r.local
        ilp = (t["ilp_kt"] or 2) if wide else t["ilp"]
        return Variant(K_SCAN, "ref", False, lds, False, 2 if ilp >= 2 else 1, kt=wide)
    mode = "local" if r.local else "global"
    em = r.entry == EM
    if t["ax_scan"] and 1 <= k <= 128:
        hw = 1 if k <= 32 else 2 if k <= 64 else 3 if k <= 96 else 4
        sp = k <= 32 and (t["ax_sproof"] == 1 or (t["ax_sproof"] == 2 and mfilter_m(shape.text_len, k) == 0))
        if r.entry == STATS and not lds:
            raise ValueError("the instrumented twin takes at most 2048 groups")
        return Variant(K_SCAN_AX, mode, r.paired, lds, em, hw, sproof=sp, stats=r.entry == STATS)
    if r.entry == STATS:
        raise ValueError("the instrumented twin exists for k_scan_ax only")
    if table and t["kt_pipeline"] and t["ilp_kt"] <= 2:
        nw = 1 if em else (t["ilp_kt"] or (1 if compact else 2))
        return Variant(K_SCAN_KT, mode, r.paired, lds, em, nw, compact=compact)
    # k_scan: with the wide table if there is one (a compact table is read by the pipelined kernel only: LF steps)
    if em:
        nwin = 1
    elif wide:
        ilp = t["ilp_kt"] or 2
        nwin = 4 if (mode == "global" and ilp == 4) else 2 if ilp >= 2 else 1
    else:
        nwin = 2 if (t["ilp_local"] if r.local else t["ilp"]) >= 2 else 1
    return Variant(K_SCAN, mode, r.paired, lds, em, nwin, kt=wide)


# ---------------------------------------------------------------- every instantiation the rules can produce
def _all_variants() -> list:
    out = []
    B = (False, True)
    for mode, paired, lds in product(("global", "local"), B, B):
        # k_scan_ax: EM or not, HW 1..4 and HW 1 with SP: 2 x 5 each (80); STATS with the LDS tally, no EM (20)
        for em in B:
            out += [Variant(K_SCAN_AX, mode, paired, lds, em, hw) for hw in (1, 2, 3, 4)]
            out.append(Variant(K_SCAN_AX, mode, paired, lds, em, 1, sproof=True))
        if lds:
            out += [Variant(K_SCAN_AX, mode, paired, True, False, hw, stats=True) for hw in (1, 2, 3, 4)]
            out.append(Variant(K_SCAN_AX, mode, paired, True, False, 1, sproof=True, stats=True))
        # k_scan_kt: compact or wide, EM (NW 1) or NW 1, 2 (48)
        for ck in B:
            out.append(Variant(K_SCAN_KT, mode, paired, lds, True, 1, compact=ck))
            out += [Variant(K_SCAN_KT, mode, paired, lds, False, nw, compact=ck) for nw in (1, 2)]
        # k_scan: LF or KT, EM (NWIN 1) or NWIN 1, 2 (24 + 24); NWIN 4 for KT in global mode only (4)
        for kt in B:
            out.append(Variant(K_SCAN, mode, paired, lds, True, 1, kt=kt))
            out += [Variant(K_SCAN, mode, paired, lds, False, n, kt=kt) for n in (1, 2)]
        if mode == "global":
            out.append(Variant(K_SCAN, mode, paired, lds, False, 4, kt=True))
    # the reference-uniqueness pass: k_scan, never paired, never EM, LF or KT, NWIN 1 or 2 (8)
    out += [Variant(K_SCAN, "ref", False, lds, False, n, kt=kt) for lds, kt, n in product(B, B, (1, 2))]
    return out


ALL_VARIANTS = frozenset(_all_variants())
COUNTS = {K_SCAN_AX: 100, K_SCAN_KT: 48, K_SCAN: 60}


# ---------------------------------------------------------------- the plan: a recipe or more for every variant
K_COMPACT, K_WIDE, K_LF = 21, 25, 140     # compact table and HW 1; wide table; past every table and the anchor kernel
K_HW = {2: 40, 3: 70, 4: 128}             # (70 is the reference's default k)


def _plan() -> list:
    out = []
    B = (False, True)
    noax = (("ax_scan", 0),)
    for ref in REFS:
        for local, paired in product(B, B):
            def add(k, entry, *tune):
                out.append(Recipe(ref, k, paired, local, entry, tuple(tune)))

            for entry in (SCAN, EM) + ((STATS,) if REFS[ref].G <= LDS_HIST_MAX_G else ()):
                add(K_COMPACT, entry, ("ax_sproof", 1))
                add(K_COMPACT, entry, ("ax_sproof", 0))
                for k in K_HW.values():
                    add(k, entry)
            # the pipelined table kernel: compact (ilp_kt auto: 1) and wide (auto: 2)
            add(K_COMPACT, EM, *noax)
            add(K_COMPACT, SCAN, *noax)
            add(K_COMPACT, SCAN, *noax, ("ilp_kt", 2))
            add(K_WIDE, EM, *noax)
            add(K_WIDE, SCAN, *noax, ("ilp_kt", 1))
            add(K_WIDE, SCAN, *noax)
            # k_scan with the wide table
            add(K_WIDE, EM, *noax, ("kt_pipeline", 0))
            add(K_WIDE, SCAN, *noax, ("kt_pipeline", 0), ("ilp_kt", 1))
            add(K_WIDE, SCAN, *noax, ("kt_pipeline", 0))
            if not local:
                add(K_WIDE, SCAN, *noax, ("ilp_kt", 4))
            # k_scan with LF steps: k past every table and the anchor kernel
            ilp = "ilp_local" if local else "ilp"
            add(K_LF, EM)
            add(K_LF, SCAN, (ilp, 1))
            add(K_LF, SCAN, (ilp, 2))
        # the reference-uniqueness pass: a compact table is not read (LF steps), a wide one is
        for k, key in ((K_COMPACT, "ilp"), (K_WIDE, "ilp_kt")):
            out.append(Recipe(ref, k, False, False, REF, ((key, 1),)))
            out.append(Recipe(ref, k, False, False, REF, ((key, 2),)))
        # other roads to the same instantiations, one rule each
        out += [
            Recipe(ref, K_COMPACT, False, False, SCAN),                      # ax_sproof 2: no m-mer filter at k = 21
            Recipe(ref, K_WIDE, True, True, EM),                             # ax_sproof 2: a filter at k = 25
            Recipe(ref, K_COMPACT, True, False, SCAN, noax + (("kt_pipeline", 0),)),  # compact, not pipelined: LF
            Recipe(ref, K_COMPACT, False, True, EM, noax + (("ilp_kt", 4),)),         # compact, ilp_kt 4: LF
            Recipe(ref, K_COMPACT, True, True, SCAN, noax + (("kmer_table", 0), ("ilp_local", 2))),
            Recipe(ref, K_HW[3], False, False, EM, noax),                    # no table past k = 31: LF
            Recipe(ref, K_WIDE, False, True, SCAN, noax + (("ilp_kt", 4),)),  # NWIN 4 is global only: local takes 2
            Recipe(ref, K_WIDE, False, False, REF),                          # ilp_kt auto: 2 for the wide table
            Recipe(ref, K_HW[3], False, False, REF),                         # no table: "ilp" (2)
            Recipe(ref, K_WIDE, False, False, REF, (("ilp_kt", 4),)),        # NWIN 4 is not for the pass: 2
        ]
    return out


PLAN = _plan()
INPUT_SETS = sorted({(r.ref, r.k, r.paired) for r in PLAN if r.entry != REF})
