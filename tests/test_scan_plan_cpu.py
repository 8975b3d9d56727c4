"""No GPU: the scan dispatcher's decision (speq_amd/csrc/scan_plan.hpp) against the hand-written table.

tests/scan_plan_check.cpp includes nothing of the project but scan_plan.hpp and is compiled here with plain g++ and no
ROCm include path: that it compiles is the proof that the header is host-only. The program prints the set of compiled
instantiations, which must be ALL_VARIANTS, and the plan of every line of facts it is given: one per recipe of
variant_table.PLAN, with the facts derived from the recipe alone, must give predict(recipe); and one per quirk of the
launch shape, with the expected figures worked out by hand below."""
import os
import shutil
import subprocess

import pytest

import variant_table as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOBAL, LOCAL, REF = 0, 1, 2
NONE, WIDE, COMPACT = 0, 1, 2
FIELDS = ("mode paired em stats k G units ilp ilp_local ilp_kt kt_pipeline blocks_per_cu blocks_per_cu_kt "
          "blocks_per_cu_ax grid_blocks grid_blocks_kt grid_blocks_ax ax_generations n_cus ax_usable sproof_active "
          "table ax_wpb ax_wave_bytes").split()
# a replica of fewer than 4 M symbols as it opens (variant_table.DEFAULTS), on 256 CUs; the anchor kernel's workgroup
# with a round figure per wave
BASE = dict(mode=GLOBAL, paired=0, em=0, stats=0, k=21, G=5, units=300, ilp=2, ilp_local=1, ilp_kt=0, kt_pipeline=1,
            blocks_per_cu=0, blocks_per_cu_kt=0, blocks_per_cu_ax=0, grid_blocks=16384, grid_blocks_kt=8192,
            grid_blocks_ax=65535, ax_generations=1, n_cus=256, ax_usable=0, sproof_active=0, table=NONE, ax_wpb=4,
            ax_wave_bytes=8000)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    """facts (a list of dicts over FIELDS) -> (the compiled set, one tuple of the program's figures per facts)."""
    exe = str(tmp_path_factory.mktemp("scan_plan") / "scan_plan_check")
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "speq_amd", "csrc"),
                    os.path.join(ROOT, "tests", "scan_plan_check.cpp"), "-o", exe], check=True)

    def run(facts):
        text = "".join(" ".join(str(int(f[name])) for name in FIELDS) + "\n" for f in facts)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == 1 + len(facts)
        return {int(x) for x in out[0].split()}, [tuple(int(x) for x in line.split()) for line in out[1:]]

    return run


def test_compiled_set_is_the_enumeration(plan_check):
    compiled, _ = plan_check([])
    expected = {v.pack() for v in vt.ALL_VARIANTS}
    assert len(expected) == 208
    assert sorted(str(vt.unpack(x)) for x in compiled - expected) == [], "compiled, not in the table"
    assert sorted(str(vt.unpack(x)) for x in expected - compiled) == [], "in the table, not compiled"


def facts_of(r: vt.Recipe) -> dict:
    """What a replica of the recipe's reference holds for its k under its tuning, by the recipe alone."""
    t = dict(vt.DEFAULTS)
    t.update(dict(r.tune))
    shape = vt.REFS[r.ref]
    table = bool(t["kmer_table"]) and 1 <= r.k <= 31
    compact = table and r.k <= 23 and bool(t["kt_compact"])
    ax = bool(t["ax_scan"]) and 1 <= r.k <= 128
    bitmap = ax and r.k <= 32 and (t["ax_sproof"] == 1 or
                                   (t["ax_sproof"] == 2 and vt.mfilter_m(shape.text_len, r.k) == 0))
    return dict(BASE, mode=REF if r.entry == vt.REF else LOCAL if r.local else GLOBAL, paired=r.paired,
                em=r.entry == vt.EM, stats=r.entry == vt.STATS, k=r.k, G=shape.G,
                units=5000 if r.entry == vt.REF else 600 if r.paired else 300,
                ilp=t["ilp"], ilp_local=t["ilp_local"], ilp_kt=t["ilp_kt"], kt_pipeline=t["kt_pipeline"],
                ax_usable=ax, sproof_active=bitmap, table=COMPACT if compact else WIDE if table else NONE)


def test_every_recipe_plans_the_predicted_instantiation(plan_check):
    assert len(vt.PLAN) == 228
    _, plans = plan_check([facts_of(r) for r in vt.PLAN])
    for r, (packed, last_kernel, *_rest) in zip(vt.PLAN, plans):
        exp = vt.predict(r)
        assert packed == exp.pack(), f"{r.id}: planned {vt.unpack(packed)}, the table predicts {exp}"
        # 3 k_scan_ax, 2 k_scan_kt, 1 k_scan with a table, 0 LF steps
        assert last_kernel == (3 if exp.family == vt.K_SCAN_AX else 2 if exp.family == vt.K_SCAN_KT else int(exp.kt)), r.id
    assert {p[0] for p in plans} == {v.pack() for v in vt.ALL_VARIANTS}


def V(family, mode, width, **kw):
    return vt.Variant(family, mode, kw.pop("paired", False), True, kw.pop("em", False), width, **kw).pack()


# (facts on top of BASE, then the expected (variant, last_kernel, grid, buf_bytes, lds_bytes, lds_launch, table_read))
# staging_bytes(k, n) = (2 (64 n + k) + 63) & ~63: (21, 2) 320, (21, 4) 576, (140, 1) 448, (140, 2) 576.
# k_scan's LDS at G = 5, global: 7 words -> 64 B, + 4 waves x (buf + 32 (buf / 64 + 1)): buf 320 -> 64 + 4 x 512 = 2112,
# buf 576 -> 64 + 4 x 896 = 3648, buf 448 -> 64 + 4 x 704 = 2880; the pass has 2 x 5 + 2 words -> 96 B.
QUIRKS = {
    # no table: 100000 units / 16 per block = 6250 blocks under "grid_blocks", no pad
    "no-table": (dict(units=100000, grid_blocks_kt=100, blocks_per_cu_kt=2),
                 (V(vt.K_SCAN, "global", 2), 0, 6250, 320, 2112, 2112, 0)),
    # a compact table exists but "kt_pipeline" 0 leaves it unread: LF steps, yet the table's cap (100) and pad
    # (160 KiB / 2)
    "compact-unpipelined": (dict(units=100000, grid_blocks_kt=100, blocks_per_cu_kt=2, table=COMPACT, kt_pipeline=0),
                            (V(vt.K_SCAN, "global", 2), 0, 100, 320, 2112, 81920, 0)),
    # the same with "ilp_kt" 4, which also widens the staging buffer (4 windows) though the kernel is NWIN 2
    "compact-ilp_kt4": (dict(units=100000, grid_blocks_kt=100, blocks_per_cu_kt=2, table=COMPACT, ilp_kt=4),
                        (V(vt.K_SCAN, "global", 2), 0, 100, 576, 3648, 81920, 0)),
    # the pass does not read a compact table either: 10^6 windows -> 3907 units of 256 -> 245 blocks, capped at 100
    "compact-pass": (dict(mode=REF, units=1000000, grid_blocks_kt=100, table=COMPACT),
                     (V(vt.K_SCAN, "ref", 2), 0, 100, 320, 96 + 4 * 512, 96 + 4 * 512, 0)),
    # ... and reads a wide one with k_scan (never the pipelined kernel), two windows by "ilp_kt" auto
    "wide-pass": (dict(mode=REF, k=25, units=1000000, table=WIDE),
                  (V(vt.K_SCAN, "ref", 2, kt=True), 1, 245, 320, 96 + 4 * 512, 96 + 4 * 512, 1)),
    # read and pipelined: k_scan_kt; compact takes one window by "ilp_kt" auto, the buffer still two
    "compact-read": (dict(units=100000, table=COMPACT, paired=1),
                     (V(vt.K_SCAN_KT, "global", 1, paired=True, compact=True), 2, 3125, 320, 2112, 2112, 1)),
    # a wide table, not pipelined: k_scan with KT
    "wide-unpipelined": (dict(k=25, table=WIDE, kt_pipeline=0, blocks_per_cu=1),
                         (V(vt.K_SCAN, "global", 2, kt=True), 1, 19, 320, 2112, 2112, 1)),
    # buf_bytes follows the widest of "ilp", "ilp_local", "ilp_kt" (auto: 2), not the chosen width (1) ...
    "buf-read": (dict(k=140, ilp=1, ilp_local=2, ilp_kt=1),
                 (V(vt.K_SCAN, "global", 1), 0, 19, 576, 3648, 3648, 0)),
    # ... the pass leaves "ilp_local" out ...
    "buf-pass": (dict(mode=REF, k=140, units=5000, ilp=1, ilp_local=2, ilp_kt=1),
                 (V(vt.K_SCAN, "ref", 1), 0, 2, 448, 96 + 4 * 704, 96 + 4 * 704, 0)),
    # ... and "ilp_kt" auto counts as 2
    "buf-pass-auto": (dict(mode=REF, k=140, units=5000, ilp=1, ilp_local=2),
                      (V(vt.K_SCAN, "ref", 1), 0, 2, 576, 96 + 4 * 896, 96 + 4 * 896, 0)),
    # the anchor kernel: 2^32 - 1 reads are its last (65535 blocks of 256 reads under "grid_blocks_ax"); its LDS is
    # 5 words -> 48 B + 4 waves x 8000, padded to 160 KiB / 4
    "ax-most-units": (dict(ax_usable=1, sproof_active=1, units=2 ** 32 - 1, blocks_per_cu_ax=4),
                      (V(vt.K_SCAN_AX, "global", 1, sproof=True), 3, 65535, 320, 32048, 40960, 0)),
    # ... 2^32 go to the other kernels (no table here: LF steps, "grid_blocks")
    "ax-too-many-units": (dict(ax_usable=1, sproof_active=1, units=2 ** 32),
                          (V(vt.K_SCAN, "global", 2), 0, 16384, 320, 2112, 2112, 0)),
    # local mode adds the 1008-B quality table, and its histogram has two words per group (80 B)
    "ax-local": (dict(mode=LOCAL, k=70, ax_usable=1, ax_wave_bytes=9700),
                 (V(vt.K_SCAN_AX, "local", 3), 3, 2, 448, 80 + 1008 + 4 * 9700, 80 + 1008 + 4 * 9700, 0)),
}


@pytest.mark.parametrize("name", list(QUIRKS))
def test_quirks_of_the_launch_shape(name, plan_check):
    facts, expected = QUIRKS[name]
    assert set(facts) <= set(FIELDS)
    _, (plan,) = plan_check([dict(BASE, **facts)])
    assert plan == expected, f"{name}: (variant, last_kernel, grid, buf_bytes, lds_bytes, lds_launch, table_read)"
