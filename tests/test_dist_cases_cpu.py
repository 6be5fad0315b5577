"""The data set of tests/dist_cases.py really holds the cases the multi-rank tests of `pileup_dist` are for.  Every condition is
computed from the references -- the CPU oracle's pileup (dist_cases.reference), domains_ref / domains_fit_ref for -D -Y,
the exact Fisher test with asm_regions_ref for -G -- and from locus_ranges, never from the library's kernels: the GPU test cannot
pass on inputs that miss a case."""
import functools
import os
import re

import numpy as np
import pytest

import dist_cases as D
from asm_q_ref import ASM_T
from conftest import ROOT
from hifimeth_amd.pileup import DOMAIN_LEVELS, DOMAIN_MAX_GAP, DOMAIN_PENALTY, locus_ranges

ASM = np.dtype([("gpos", "<i8"), ("pcov1", "<i4"), ("ncov1", "<i4"), ("pcov2", "<i4"), ("ncov2", "<i4"), ("motif", "<u4"),
                ("reserved", "<u4"), ("diff", "<f8"), ("pvalue", "<f8")])
MAX_P = 0.01                       # -s is left at its default
SITE_BIG = 256                     # a locus of this coverage is beyond the -B histogram


def _per_sequence(rows, field="gpos"):
    off = D.offsets()
    return [rows[(rows[field] >= off[s]) & (rows[field] < off[s + 1])] for s in range(len(D.NAMES))]


@functools.lru_cache(maxsize=None)
def domain_segments():
    """-D -Y 5 by the restatements: per context the levels fitted over all sequences, then textbook Viterbi per sequence"""
    from domains_fit_ref import fit_chains, lib_scores
    from domains_ref import domains
    chains = _per_sequence(D.reference()["loci"])
    out = []
    for ctx in range(3):
        lo, hi, _status, _hist = fit_chains(chains, ctx, *DOMAIN_LEVELS[ctx], DOMAIN_PENALTY, DOMAIN_MAX_GAP, 5)
        rule = lib_scores(lo, hi, DOMAIN_PENALTY)
        out += [g for rows in chains for g in domains(rows, ctx, *rule, DOMAIN_MAX_GAP)[0]]
    return out


@functools.lru_cache(maxsize=None)
def asm_rows():
    """the tested loci of -A -a 1: both haplotypes counted, the combined motif, the exact two-sided Fisher p"""
    from test_gpu_pileup_asm import fisher_exact
    ref = D.reference()
    h1, h2 = ({int(x["gpos"]): (int(x["pcov"]), int(x["ncov"])) for x in ref["hap"][k]} for k in (1, 2))
    motif = {int(x["gpos"]): int(x["motif"]) for x in ref["loci"]}
    p_of = functools.lru_cache(maxsize=None)(lambda *t: float(fisher_exact(*t)))
    both = sorted(set(h1) & set(h2))
    rows = np.zeros(len(both), ASM)
    for i, g in enumerate(both):
        t = (*h1[g], *h2[g])
        rows[i] = (g, *t, motif[g], 0, 100.0 * t[0] / (t[0] + t[1]) - 100.0 * t[2] / (t[2] + t[3]), p_of(*t))
    return rows


@functools.lru_cache(maxsize=None)
def asm_regions():
    from asm_regions_ref import regions
    return [g for rows in _per_sequence(asm_rows()) for ctx in range(3) for g in regions(rows, ctx, MAX_P, D.MAX_GAP, D.MIN_LOCI)[0]]


def _whole_chunks(a, b, ranges):
    return [k for k, (lo, hi) in enumerate(ranges) if lo < hi and a <= lo and hi <= b]


def _ranks_with_a_gap(gpos, chunk):
    """the ranks whose chunks hold these loci lie in at least two chunks, with a rank between them that holds none"""
    ranks = sorted({int(g) // chunk for g in gpos})
    return len(ranks) >= 2 and any(b - a > 1 for a, b in zip(ranks, ranks[1:]))


def test_the_genome_and_the_constants():
    header = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    assert int(re.search(r"#define HM_REGION_BLOCK (\d+)", header).group(1)) == D.REGION_BLOCK
    assert int(re.search(r"#define HM_ASM_T (\d+)", header).group(1)) == ASM_T
    assert all(D.N_LOCI % w for w in D.WORLDS) and all(n % 100 for n in D.LENGTHS) and len(D.genome()) == 4
    chunk8 = locus_ranges(D.N_LOCI, 8)[0][1]
    assert chunk8 > 3 * D.REGION_BLOCK
    ctl = (int(D.offsets()[0]), int(D.offsets()[1]))
    assert sum(1 for lo, hi in locus_ranges(D.N_LOCI, 8) if lo < ctl[1] and hi > ctl[0]) >= 2        # the control spans two chunks of eight
    rs = D.reads()
    assert {r.hp for r in rs} == {None, 1, 2} and {r.flag for r in rs} == {0, 16}
    assert {op for r in rs for op, _n in r.cigar} == set("MIDS") and max(len(r.seq) for r in rs) <= 613
    thr = D.reference()["thresholds"]
    for c in range(3):                                                              # ML bytes on both sides of every threshold
        ml = np.concatenate([r.ml for r in rs])
        assert (ml >= thr[c]).any() and (ml < thr[c]).any() and (ml == 255).any() and (ml < 5).any()
    ctl_rows = _per_sequence(D.reference()["loci"])[0]
    assert ctl_rows["pcov"].sum() * 10 < ctl_rows["ncov"].sum() and ctl_rows["pcov"].sum() > 0


def test_the_bed_file_holds_its_intervals():
    off, r8 = D.offsets(), locus_ranges(D.N_LOCI, 8)
    rows = {name: (D.NAMES.index(chrom), int(off[D.NAMES.index(chrom)]) + a, int(off[D.NAMES.index(chrom)]) + b, strand)
            for chrom, a, b, name, strand in D.bed_rows()}
    _s, a, b, _ = rows["whole_chunk"]
    assert [k for k in _whole_chunks(a, b, r8) if 0 < k < 7]
    _s, a, b, _ = rows["whole_block"]
    (k,) = [k for k, (lo, hi) in enumerate(r8) if lo <= a and b <= hi]               # inside one chunk
    first = r8[k][0] + -(-(a - r8[k][0]) // D.REGION_BLOCK) * D.REGION_BLOCK         # the first block edge of that rank's index in it
    assert first + D.REGION_BLOCK <= b
    cuts = [lo for lo, _hi in r8[1:]]
    _s, a, b, strand = rows["flank_up"]
    assert strand == "+" and any(a - 30 < c < a for c in cuts)
    _s, a, b, strand = rows["flank_down"]
    assert strand == "-" and any(b < c < b + 30 for c in cuts)
    for w in D.WORLDS:
        cuts = D.boundaries(w)
        assert rows[f"ends_on_{w}"][2] in cuts and rows[f"starts_on_{w}"][1] in cuts
    sid = rows["on_chrB"][0]
    assert any(hi <= off[sid] or lo >= off[sid + 1] for lo, hi in r8)                # a rank that does not touch that sequence
    assert rows["too_short"][2] - rows["too_short"][1] < 4                            # fewer bases than -J's bins
    cov = D.reference()["loci"]
    for name, (_s, a, b, _) in rows.items():                                          # no interval without counted loci
        assert ((cov["gpos"] >= a) & (cov["gpos"] < b) & (cov["pcov"] + cov["ncov"] >= 2)).any(), name


@pytest.mark.parametrize("world", D.WORLDS)
def test_the_cases_of_a_world(world):
    ranges = locus_ranges(D.N_LOCI, world)
    chunk = ranges[0][1] - ranges[0][0]
    off = [int(x) for x in D.offsets()]
    assert world * chunk > D.N_LOCI and ranges[-1][1] - ranges[-1][0] < chunk        # the padded tail
    assert any(off[s] < lo and hi < off[s + 1] for lo, hi in ranges for s in range(4))     # a chunk strictly inside one sequence
    loci = D.reference()["loci"]
    # -D: an H segment over a whole chunk, and in it a chunk without a CHG row between CHG rows of the same sequence
    high = [(int(g["start"]), int(g["end"])) for g in domain_segments() if g["state"] == 1]
    over = [(a, b, k) for a, b in high for k in _whole_chunks(a, b, ranges)]
    assert over
    chg = loci["gpos"][loci["motif"] == 1]
    empty = []
    for _a, _b, k in over:
        lo, hi = ranges[k]
        (s,) = [s for s in range(4) if off[s] <= lo and hi <= off[s + 1]]
        if not ((chg >= lo) & (chg < hi)).any() and ((chg >= off[s]) & (chg < lo)).any() and ((chg >= hi) & (chg < off[s + 1])).any():
            empty.append(k)
    assert empty
    # -G: a region over a whole chunk
    assert any(_whole_chunks(int(g["start"]), int(g["end"]), ranges) for g in asm_regions())
    # the control sequence misses a chunk
    assert any(hi <= off[0] or lo >= off[1] for lo, hi in ranges)
    # -S 3 -O 2: on both strands a counted cytosine within three bases of a boundary on either side of it
    text = "".join(s for _n, s in D.genome())
    counted = loci["gpos"][loci["pcov"] + loci["ncov"] >= 2]
    for base in "CG":
        mine = {int(g) for g in counted if text[int(g)] == base}
        assert any(mine & set(range(b - 3, b)) and mine & set(range(b, b + 3)) for b in D.boundaries(world)), base
    # the slabs
    n = len(D.reads())
    slab = D.slab(world, n)
    dealt = {(i // slab) % world for i in range(n)}
    if world == 8:
        assert -(-n // slab) == 5 and dealt == {0, 1, 2, 3, 4}                        # the records of slabs 0 .. 4 are all the records
    else:
        assert dealt == set(range(world)) and n // slab > 10 * world                  # many slabs for every rank


def test_the_big_lists_of_world_eight():
    ranges = locus_ranges(D.N_LOCI, 8)
    chunk = ranges[0][1]
    off = [int(x) for x in D.offsets()]
    assert any(any(lo < off[s] and off[s + 1] < hi for s in (1, 2)) for lo, hi in ranges)     # a whole sequence and parts of two others
    loci = D.reference()["loci"]
    big = loci["gpos"][loci["pcov"] + loci["ncov"] >= SITE_BIG]
    assert len(big) and _ranks_with_a_gap(big, chunk)
    rows = asm_rows()
    big_q = rows["gpos"][(rows["pcov1"] + rows["ncov1"] >= ASM_T) | (rows["pcov2"] + rows["ncov2"] >= ASM_T)]
    assert len(big_q) and _ranks_with_a_gap(big_q, chunk)
    stacks = sorted({int(g) // chunk for g in big})
    assert stacks[-1] - stacks[0] >= 3 and all(set(stacks) == {int(g) // chunk for g in x} for x in (big, big_q))


def test_the_error_case():
    g, rs, name = D.ghost()
    on = [i for i, r in enumerate(rs) if g[r.tid][0] == name]
    assert len(on) == 1 and (on[0] // D.SMALL_SLAB) % 3 == 1 and name not in D.NAMES and rs[on[0]].mm
    assert [(r.tid, r.pos) for r in rs] == sorted((r.tid, r.pos) for r in rs)
