"""Allele-specific regions (`pileup -H -A -G`), the parts that need no GPU: the numpy restatement of the definition
(asm_regions_ref) on hand-written rows with literal results and against a second formulation, stitch_asm_regions against the
restatement over the whole for every split, the BED text, the row layout and the usage errors of both front ends."""
import itertools
import os
import subprocess
import sys

import numpy as np

from asm_regions_ref import FIRST, LAST, REGION_DTYPE, parts_of, pooled_diff, regions, regions_union_find
from conftest import ROOT
from hifimeth_amd.pileup import ASM_REGION_DTYPE, stitch_asm_regions

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
ASM_DTYPE = np.dtype([("gpos", "<i8"), ("pcov1", "<i4"), ("ncov1", "<i4"), ("pcov2", "<i4"), ("ncov2", "<i4"), ("motif", "<u4"),
                      ("reserved", "<u4"), ("diff", "<f8"), ("pvalue", "<f8")])
MAX_P = 0.01
UP, DOWN, FLAT = (8, 2, 2, 8), (2, 8, 8, 2), (5, 5, 5, 5)     # counts of a row with diff 60, -60, 0


def mk(*specs):
    """rows from (gpos, '+' | '-' | '0', pvalue[, motif[, counts]]): diff is 60 / -60 / 0"""
    rows = np.zeros(len(specs), ASM_DTYPE)
    for r, (gpos, way, p, *more) in zip(rows, specs):
        counts = more[1] if len(more) > 1 else {"+": UP, "-": DOWN, "0": FLAT}[way]
        r["gpos"], r["pvalue"], r["motif"] = gpos, p, more[0] if more else 0
        r["pcov1"], r["ncov1"], r["pcov2"], r["ncov2"] = counts
        r["diff"] = {"+": 60.0, "-": -60.0, "0": 0.0}[way]
    return rows


def brief(regs):
    return [(int(g["start"]), int(g["end"]), int(g["n_loci"]), int(g["sign"]), int(g["flags"])) for g in regs]


HIT, MISS = 1e-4, 0.5


def reg(rows, ctx, max_p, max_gap, min_loci, keep_edges=False):
    """the restatement's answer; the product's stitcher, given the one range, must return the same"""
    want = regions(rows, ctx, max_p, max_gap, min_loci, keep_edges)
    got = stitch_asm_regions([regions(rows, ctx, max_p, max_gap, min_loci, True)], max_gap, min_loci, keep_edges)
    assert got[0].dtype == ASM_REGION_DTYPE and got[0].tobytes() == want[0].tobytes() and got[1] == want[1]
    return want


def test_gap_of_exactly_max_gap_links_and_one_more_does_not():
    rows = mk((10, "+", HIT), (110, "+", HIT), (211, "+", HIT), (311, "+", HIT))
    got, R = reg(rows, 0, MAX_P, 100, 2)
    assert R == 4 and brief(got) == [(10, 111, 2, 1, FIRST), (211, 312, 2, 1, LAST)]
    assert brief(reg(rows, 0, MAX_P, 101, 2)[0]) == [(10, 312, 4, 1, FIRST | LAST)]
    assert brief(reg(rows, 0, MAX_P, 99, 1)[0]) == [(10, 11, 1, 1, FIRST), (110, 111, 1, 1, 0), (211, 212, 1, 1, 0), (311, 312, 1, 1, LAST)]


def test_min_loci_and_keep_edges():
    rows = mk((0, "-", HIT), (1, "-", HIT), (2, "-", HIT), (300, "-", HIT), (301, "-", HIT), (700, "-", HIT), (701, "-", HIT))
    assert brief(reg(rows, 0, MAX_P, 100, 3)[0]) == [(0, 3, 3, -1, FIRST)]                       # n_loci == min_loci stays, min_loci - 1 goes
    assert brief(reg(rows, 0, MAX_P, 100, 4)[0]) == []
    assert brief(reg(rows, 0, MAX_P, 100, 2)[0]) == [(0, 3, 3, -1, FIRST), (300, 302, 2, -1, 0), (700, 702, 2, -1, LAST)]
    # keep_edges: the short chains at either end come too, the short one in the middle does not; flags are the same either way
    assert brief(reg(rows, 0, MAX_P, 100, 3, keep_edges=True)[0]) == [(0, 3, 3, -1, FIRST), (700, 702, 2, -1, LAST)]
    assert brief(reg(rows, 0, MAX_P, 100, 4, keep_edges=True)[0]) == [(0, 3, 3, -1, FIRST), (700, 702, 2, -1, LAST)]


def test_sign_flip_zero_diff_threshold_and_non_hit():
    flip = mk((0, "+", HIT), (1, "+", HIT), (2, "-", HIT), (3, "-", HIT), (4, "+", HIT))
    assert brief(reg(flip, 0, MAX_P, 100, 1)[0]) == [(0, 2, 2, 1, FIRST), (2, 4, 2, -1, 0), (4, 5, 1, 1, LAST)]
    zero = mk((0, "+", HIT), (1, "+", HIT), (2, "0", HIT), (3, "+", HIT), (4, "+", HIT))             # p small, diff == 0: no hit
    assert brief(reg(zero, 0, MAX_P, 100, 1)[0]) == [(0, 2, 2, 1, FIRST), (3, 5, 2, 1, LAST)]
    edge = mk((0, "+", HIT), (1, "+", MAX_P), (2, "+", np.nextafter(MAX_P, 1.0)), (3, "+", HIT))     # p == max_p is a hit
    assert brief(reg(edge, 0, MAX_P, 100, 1)[0]) == [(0, 2, 2, 1, FIRST), (3, 4, 1, 1, LAST)]
    miss = mk((0, "-", HIT), (1, "-", MISS), (2, "-", HIT))                                          # evidence against the region
    assert brief(reg(miss, 0, MAX_P, 100, 1)[0]) == [(0, 1, 1, -1, FIRST), (2, 3, 1, -1, LAST)]
    assert brief(reg(miss, 0, MAX_P, 100, 2)[0]) == []


def test_first_and_last_row_other_contexts_and_the_sums():
    rows = mk((5, "+", MISS), (6, "+", HIT), (7, "+", 1e-9, 0, (30, 0, 1, 29)), (8, "+", MISS), (9, "-", HIT))
    got, R = reg(rows, 0, MAX_P, 100, 1)
    assert R == 5 and brief(got) == [(6, 8, 2, 1, 0), (9, 10, 1, -1, LAST)]                          # row 0 is no hit: no FIRST anywhere
    g = got[0]
    assert (int(g["pcov1"]), int(g["ncov1"]), int(g["pcov2"]), int(g["ncov2"])) == (38, 2, 3, 37)
    assert g["pmin"] == 1e-9 and g["diff"] == 100.0 * 38 / 40 - 100.0 * 3 / 40 and g["motif"] == 0
    # rows of other contexts neither link nor break; key low bits 3 are CHH
    mixed = mk((0, "+", HIT), (1, "-", MISS, 1), (2, "+", HIT), (3, "-", HIT, 2), (4, "+", HIT), (5, "-", HIT, 3), (6, "-", MISS, 1))
    assert brief(reg(mixed, 0, MAX_P, 100, 1)[0]) == [(0, 5, 3, 1, FIRST | LAST)]
    got, R = reg(mixed, 2, MAX_P, 100, 1)
    assert R == 2 and brief(got) == [(3, 6, 2, -1, FIRST | LAST)] and got["motif"][0] == 2
    got, R = reg(mixed, 1, MAX_P, 100, 1, keep_edges=True)
    assert R == 2 and len(got) == 0
    assert reg(mixed[:0], 0, MAX_P, 100, 1)[1] == 0
    # Simpson: every locus leans to haplotype 1, the pooled counts to haplotype 2; sign stays the loci's
    simpson = mk((0, "+", HIT, 0, (9, 1, 80, 20)), (1, "+", HIT, 0, (30, 70, 2, 8)))
    g = reg(simpson, 0, MAX_P, 100, 1)[0][0]
    assert g["sign"] == 1 and g["diff"] == pooled_diff(39, 71, 82, 28) < 0


def _random_rows(rng, n, max_gap):
    rows = np.zeros(n, ASM_DTYPE)
    rows["gpos"] = np.cumsum(rng.choice([1, 2, max_gap - 1, max_gap, max_gap + 1, 3 * max_gap], n, p=[.3, .2, .1, .15, .15, .1]))
    rows["motif"] = rng.choice([0, 0, 0, 1, 2, 3], n)
    tot = rng.integers(5, 40, (2, n))
    k = (rng.random((2, n)) * (tot + 1)).astype(np.int64)
    rows["pcov1"], rows["ncov1"], rows["pcov2"], rows["ncov2"] = k[0], tot[0] - k[0], k[1], tot[1] - k[1]
    rows["diff"] = 100.0 * rows["pcov1"] / tot[0] - 100.0 * rows["pcov2"] / tot[1]
    rows["diff"][rng.random(n) < 0.05] = 0.0
    if rng.random() < 0.5:                                    # long runs of one sign
        rows["diff"] = np.abs(rows["diff"]) * np.repeat(rng.choice([-1.0, 1.0], n // 5 + 1), 5)[:n]
    rows["pvalue"] = rng.choice([1e-30, 1e-4, MAX_P, np.nextafter(MAX_P, 1.0), 0.3, 1.0], n, p=[.2, .35, .15, .1, .1, .1])
    return rows


def test_two_formulations_agree_on_random_rows():
    rng = np.random.default_rng(77)
    seen = 0
    for k in range(3000):
        max_gap, min_loci = int(rng.choice([1, 7, 100])), int(rng.integers(1, 5))
        rows = _random_rows(rng, int(rng.integers(0, 40)), max(max_gap, 2))
        for keep in (False, True):
            a, Ra = reg(rows, k % 3, MAX_P, max_gap, min_loci, keep)
            b, Rb = regions_union_find(rows, k % 3, MAX_P, max_gap, min_loci, keep)
            assert Ra == Rb and a.tobytes() == b.tobytes()
        seen += len(a)
    assert seen > 3000


def _splits(n_rows):
    """every way to cut rows 0 .. n_rows-1 into 2, 3 or 4 adjacent ranges, empty ones included, as row indices"""
    for k in (1, 2, 3):
        yield from itertools.combinations_with_replacement(range(n_rows + 1), k)


def _check_every_split(rows, ctx, max_gap, min_loci):
    end = int(rows["gpos"][-1]) + 1
    whole = {keep: regions(rows, ctx, MAX_P, max_gap, min_loci, keep) for keep in (False, True)}
    n = 0
    for cuts in _splits(len(rows)):
        bounds = [0] + [int(rows["gpos"][c]) if c < len(rows) else end for c in cuts] + [end]
        parts = parts_of(rows, bounds, ctx, MAX_P, max_gap, min_loci)
        for keep in (False, True):
            got, R = stitch_asm_regions(parts, max_gap, min_loci, keep_edges=keep)
            assert got.dtype == ASM_REGION_DTYPE and R == whole[keep][1]
            assert got.tobytes() == whole[keep][0].tobytes(), (cuts, keep)
        n += 1
    return n, parts


def test_stitched_parts_equal_the_whole_for_every_split():
    rng = np.random.default_rng(5)
    sets = [_random_rows(rng, int(rng.integers(1, 10)), 7) for _ in range(40)]
    one = mk(*[(3 * i, "+", HIT) for i in range(8)])          # one chain: every part is a whole chain with both flags
    big = mk(*[(i, "-", HIT, 0, (2 ** 30, 2 ** 31 - 1, 2 ** 31 - 1, 7)) for i in range(6)])          # sums beyond 2^31 (and 2^33)
    two = mk((0, "+", HIT), (1, "+", HIT), (2, "-", HIT, 1), (3, "-", HIT), (4, "-", HIT), (9, "+", MISS), (10, "+", HIT))
    n = 0
    for rows in sets + [one, big, two]:
        for ctx in (0, 2):
            for max_gap, min_loci in ((7, 1), (7, 3), (2, 2)):
                n += _check_every_split(rows, ctx, max_gap, min_loci)[0]
    assert n > 10000
    g = regions(big, 0, MAX_P, 7, 1)[0][0]
    assert g["ncov1"] == 6 * (2 ** 31 - 1) > 2 ** 33 and g["pcov1"] == 6 * 2 ** 30 and g["diff"] == pooled_diff(*(int(g[f]) for f in ("pcov1", "ncov1", "pcov2", "ncov2")))
    # parts that are empty, and parts that are one whole chain, do occur among those splits
    _n, parts = _check_every_split(one, 0, 7, 1)
    assert parts[-1][1] == 0 and parts[0][1] == 8 and int(parts[0][0]["flags"][0]) == FIRST | LAST


def test_regions_bed_text():
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup.__new__(MethylationPileup)       # no engine: names and offsets are all the writer reads
    pu._h = None
    pu.names, pu.offsets = ["chrA", "chrB"], np.array([0, 100, 250])
    rows = np.zeros(3, ASM_REGION_DTYPE)
    rows["start"], rows["end"], rows["n_loci"], rows["sign"], rows["motif"] = [5, 100, 240], [60, 101, 250], [12, 1, 3], [1, -1, -1], [0, 2, 0]
    rows["pcov1"], rows["ncov1"], rows["pcov2"], rows["ncov2"] = [100, 1, 2 ** 33], [20, 6, 1], [10, 6, 5], [110, 1, 2 ** 33]
    rows["diff"], rows["pmin"] = [75.0, -71.4285714, 0.0], [1.5e-12, 0.029137529, 4.1e-5]
    text = pu.asm_regions_bed(rows)
    assert text["CpG"] == ("chrA\t5\t60\t12\t+\t75\t1.5e-12\t100\t20\t10\t110\n"
                           "chrB\t140\t150\t3\t-\t0\t4.1e-05\t8589934592\t1\t5\t8589934592\n")
    assert text["CHH"] == "chrB\t0\t1\t1\t-\t-71.4286\t0.0291375\t1\t6\t6\t1\n" and text["CHG"] == ""


def test_row_layout_matches_the_header(tmp_path):
    from hifimeth_amd.pileup import REGION_FIRST, REGION_LAST
    assert ASM_REGION_DTYPE == REGION_DTYPE and ASM_REGION_DTYPE.itemsize == 80
    names = ("start", "end", "pcov1", "ncov1", "pcov2", "ncov2", "n_loci", "sign", "motif", "flags", "diff", "pmin")
    offsets = (0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64, 72)
    assert ASM_REGION_DTYPE.names == names and tuple(ASM_REGION_DTYPE.fields[n][1] for n in names) == offsets
    src = tmp_path / "t.c"
    fmt = "%zu %u %u %d" + " %zu" * len(names)
    args = ", ".join(["sizeof(hm_asm_region_t)", "HM_REGION_FIRST", "HM_REGION_LAST", "HM_ABI_VERSION"] + [f"offsetof(hm_asm_region_t, {n})" for n in names])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hifimeth_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}", {args}); return 0; }}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert got == [80, REGION_FIRST, REGION_LAST, 5, *offsets] and (REGION_FIRST, REGION_LAST) == (FIRST, LAST)


def test_usage_errors_before_any_device_call(tmp_path):
    """-G without -A, -s / -g / -n without -G or out of range: refused while parsing, by both front ends; nothing is written"""
    bad = {"-G needs -A": (["-G"], ["-H", "-G"]),
           "need -G": (["-H", "-A", "-s", "0.1"], ["-H", "-A", "-g", "10"], ["-H", "-A", "-n", "2"]),
           "-s must be in (0, 1]": (["-H", "-A", "-G", "-s", "0"], ["-H", "-A", "-G", "-s", "1.5"], ["-H", "-A", "-G", "-s", "nan"],
                                    ["-H", "-A", "-G", "-s", "-0.1"]),
           ">= 1": (["-H", "-A", "-G", "-g", "0"], ["-H", "-A", "-G", "-n", "0"], ["-H", "-A", "-G", "-n", "-3"])}
    for why, cases in bad.items():
        for args in cases:
            r = subprocess.run([CLI, "pileup", *args, "ref.fa", "mod.bam", str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
            assert r.returncode != 0 and "USAGE" in r.stderr and why in r.stderr.split("USAGE")[0], args
            r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, "ref.fa", "mod.bam", str(tmp_path / "out")],
                               capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
            assert r.returncode == 2 and why in r.stderr, args
    for args in (["-H", "-A", "-G", "-g", "5x"], ["-H", "-A", "-G", "-s", "0.1z"], ["-H", "-A", "-G", "-n", "2.5"]):   # the whole value must parse
        r = subprocess.run([CLI, "pileup", *args, "ref.fa", "mod.bam", str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "USAGE" in r.stderr, args
    r = subprocess.run([CLI, "pileup", "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(x in r.stderr for x in ("  -G\n", "  -s <p>\n", "  -g <bp>\n", "  -n <int>\n", "asm.regions.<ctx>.bed"))
    assert not os.listdir(tmp_path)
