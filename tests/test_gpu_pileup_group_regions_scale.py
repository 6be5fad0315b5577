"""`groupdmr` and the group rows at scale on the device: group_regions_scale_cases.build(4096, 1024) -- 4 206 597 rows of context 0
on 8.4 M bases, so that the row selections of hm_dmr_fetch_regions run loci_scan_kernel with two block counts per thread and the
loci selections with three; a chain of 70 001 rows whose sums exceed 2^32; chains of min_loci - 1, min_loci and min_loci + 1 =
4999, 5000, 5001 rows from the last row of a selection block; every linking case at a block edge -- and a reference past 2^32.

hm_pileup_fetch_groups: the integer fields and diff against the samples' sums, the statistic bit-identical within a kind and within
the bar of test_gpu_pileup_groups.py against mpmath.  hm_dmr_fetch_regions: byte for byte against group_regions_ref.regions_fast
on the fetched rows (test_group_regions_scale_cases_cpu.py holds that to the loop restatements).  Nothing here has a tolerance of
its own."""
import numpy as np
import pytest

import bigref
import group_regions_ref as RR
import group_regions_scale_cases as SC
import groups_ref as G
from groups_ref import HM_EINVAL

pytestmark = pytest.mark.gpu

B, T = 4096, 1024
INT_FIELDS = ("gpos", "motif", "m1", "m2", "pcov1", "ncov1", "pcov2", "ncov2")
STAT_FIELDS = ("diff", "D", "phi", "pvalue")


@pytest.fixture(scope="module")
def scale():
    """-> (engine, info, its hm_group_t rows over the whole reference, the rows expected from the samples); read-only"""
    from hifimeth_amd.pileup import MethylationPileup
    samples, info = SC.build(B, T)
    pu = MethylationPileup([("ctg%d" % (k + 1), n) for k, n in enumerate(info["lengths"])], partitions=True, groups=True,
                           group_min_cov=SC.MIN_COV, bases=np.full(info["n"], ord("N"), np.uint8))
    counted = SC.counted(samples)
    for g, s in SC.SAMPLES:
        assert pu.begin_sample(g) == s and pu.load_sample_loci(*samples[(g, s)]) == counted[(g, s)]
    rows = pu.group_tests(min_reps=SC.MIN_REPS)
    rows.setflags(write=False)
    want = SC.expected_rows(samples, info["n"])
    yield pu, info, rows, want
    pu.close()


def _within(rows, lo, hi):
    a, b = np.searchsorted(rows["gpos"], [lo, hi])
    return rows[a:b]


def _ranges(info):
    n, first = info["n"], info["lengths"][0]
    return ((0, n), (0, first), (first, n), (1234567, 7654321))


def _same(pu, rows, ctx, lo, hi, max_p, min_diff, max_gap, min_loci, keep=False):
    got = pu.group_regions(ctx, lo, hi, SC.MIN_REPS, max_p, min_diff, max_gap, min_loci, keep)
    want = RR.regions_fast(_within(rows, lo, hi), ctx, max_p, min_diff, max_gap, min_loci, keep)
    assert got[1:] == want[1:] and len(got[0]) == len(want[0]), (ctx, lo, hi, max_p, min_diff, max_gap, min_loci, keep, got[1:], want[1:], len(got[0]), len(want[0]))
    assert got[0].tobytes() == want[0].tobytes(), (ctx, lo, hi, max_p, min_diff, max_gap, min_loci, keep, np.flatnonzero(got[0] != want[0])[:3])
    return got


# ---- hm_pileup_fetch_groups at 4 Mi rows --------------------------------------------------------------------------------------------
def test_the_rows_are_the_samples_sums(scale):
    _pu, info, rows, want = scale
    assert len(rows) == len(want) == int((info["kind"] != ord("U")).sum()) and int(RR.ctx_mask(rows, 0).sum()) == info["R"] == B * T + 3 * B + 5
    for f in INT_FIELDS + ("diff",):
        assert rows[f].tobytes() == want[f].tobytes(), f


def test_rows_of_one_kind_are_bit_identical(scale):
    """a handful of kinds, millions of rows: group_test_kernel does not depend on the row index, the workgroup or gpos"""
    _pu, info, rows, _want = scale
    kind = info["kind"][info["kind"] != ord("U")]
    seen = {}
    for k, sign in SC.SIGN.items():
        r = rows[kind == ord(k)]
        assert len(r) >= 1000, k
        for f in STAT_FIELDS:
            assert len(np.unique(r[f].view(np.uint64))) == 1, (k, f, np.unique(r[f])[:4])
        seen[k] = tuple(r[0][f] for f in STAT_FIELDS)
        if sign:
            assert seen[k][3] < 0.008 and np.sign(seen[k][0]) == sign, k
    assert seen["N"] == seen["o"] == (0.0, 0.0, 1.0, 1.0) and seen["A"][0] == 10.0 and 0.3 < seen["A"][3] < 1.0
    assert seen["b"] == seen["P"] == seen["O"] and seen["q"][2] > 1.0 and seen["H"][0] == 40.0
    assert int((kind == ord("H")).sum()) >= info["long_n"] and int((kind == ord("N")).sum()) > 3 << 20


def test_one_row_per_kind_against_mpmath(scale):
    from test_gpu_pileup_groups import _check_statistic
    _pu, info, rows, _want = scale
    kind = info["kind"][info["kind"] != ord("U")]
    picked = {k: rows[np.flatnonzero(kind == ord(k))[-1]] for k in SC.SIGN}       # the last of each
    by_gpos = {int(r["gpos"]): SC.kind_sums(k) for k, r in picked.items()}
    worst = _check_statistic(list(picked.values()), lambda r: (by_gpos[int(r["gpos"])], G.stat_mp(*by_gpos[int(r["gpos"])])), G.e_ref())
    print("one row per kind: " + ", ".join("E_gpu(%s) = %.3g" % kv for kv in worst.items()))


@pytest.mark.parametrize("what", ["aligned to nothing", "B T loci", "B T + 1 loci", "B T rows", "B T + 1 rows"])
def test_a_sub_range_fetch_is_the_slice_of_the_whole(scale, what):
    """B T loci are 1024 blocks, one per scan thread and every thread used; one locus more makes two per thread"""
    pu, _info, rows, _want = scale
    lo, hi = {"aligned to nothing": (1234567, 7654321), "B T loci": (5, 5 + B * T), "B T + 1 loci": (4094, 4094 + B * T + 1),
              "B T rows": (0, int(rows["gpos"][B * T])), "B T + 1 rows": (0, int(rows["gpos"][B * T + 1]))}[what]
    got, want = pu.group_tests(lo, hi, SC.MIN_REPS), _within(rows, lo, hi)
    assert len(got) == len(want) > 1 << 20 and got.tobytes() == want.tobytes()
    assert "rows" not in what or len(got) == B * T + ("+ 1" in what)


# ---- hm_dmr_fetch_regions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2, 3])
def test_regions_equal_the_restatement(scale, which):
    """the whole reference, each sequence and a range aligned to nothing; contexts 0 and 1 with both keep_edges, context 2 once"""
    pu, info, rows, _want = scale
    t = info["thresholds"][which]
    n = 0
    for lo, hi in _ranges(info):
        for ctx in (0, 1):
            for keep in (False, True):
                got = _same(pu, rows, ctx, lo, hi, *t, keep)
                n += len(got[0])
                if (lo, hi, ctx) == (0, info["n"], 0):
                    assert got[1] == info["R"]
    n += len(_same(pu, rows, 2, 0, info["n"], *t)[0])
    assert n >= (12 if t[3] == info["min_loci"] else 20000)
    if which == 0:
        lo_, hi_ = info["n_chains_bounds"]
        assert lo_ <= len(pu.group_regions(0, 0, info["n"], SC.MIN_REPS, *t)[0]) == info["n_chains"] <= hi_


def test_the_chains_the_builder_names(scale):
    pu, info, rows, _want = scale
    at = info["row_gpos"]
    got, R, hits = _same(pu, rows, 0, 0, info["n"], 0.01, 0.0, SC.MAX_GAP, 1)
    assert R == info["R"] and hits == int(np.count_nonzero(SC._table(lambda k: SC.SIGN.get(k, 0))[info["row_kind"]]))
    where = {int(s): k for k, s in enumerate(got["start"])}
    for name, (a, b, sign, flags) in info["chains"].items():
        g = got[where[int(at[a])]]
        assert (int(g["end"]), int(g["n_loci"]), int(g["sign"]), int(g["flags"])) == (int(at[b]) + 1, b - a + 1, sign, flags), name
    # the long heavy chain: more rows than a uint16 counts, sums that an int32 -- and a uint32 -- cannot hold
    a, b = info["chains"]["long heavy"][:2]
    long = got[where[int(at[a])]]
    sums = tuple(int(long[f]) for f in ("pcov1", "ncov1", "pcov2", "ncov2"))
    assert long["n_loci"] == 70001 == info["long_n"] and a % B == B - 1 and sums == info["long_sums"] and min(sums) > 1 << 32
    assert long["diff"].tobytes() == RR.pooled_diff(*sums).tobytes() and (long["m1_min"], long["m2_min"], long["phi_max"]) == (2, 2, 1.0)
    # of the chains of 4999, 5000 and 5001 rows the two of >= min_loci, and the long one
    m = info["min_loci"]
    assert m == 5000 and info["thresholds"][1] == (0.01, 0.0, SC.MAX_GAP, m)
    for lo, hi in ((0, info["n"]), (0, info["lengths"][0])):
        kept = _same(pu, rows, 0, lo, hi, *info["thresholds"][1])[0]
        assert kept["n_loci"].tolist() == [m, m + 1, 70001] and kept["start"].tolist() == [int(at[info["chains"][k][0]]) for k in ("min_loci", "min_loci + 1", "long heavy")]
    assert _same(pu, rows, 0, 0, info["n"], 0.01, 0.0, SC.MAX_GAP, m - 1)[0]["n_loci"].tolist() == [m - 1, m, m + 1, 70001]
    # the sequence boundary: one chain over the whole reference, two per sequence
    a, b = info["chains"]["sequence boundary"][:2]
    first = info["lengths"][0]
    one, two = _same(pu, rows, 0, 0, first, 0.01, 0.0, SC.MAX_GAP, 1)[0], _same(pu, rows, 0, first, info["n"], 0.01, 0.0, SC.MAX_GAP, 1)[0]
    assert (int(one[-1]["start"]), int(one[-1]["end"]), int(one[-1]["flags"])) == (int(at[a]), int(at[a + 1]) + 1, RR.LAST)
    assert (int(two[0]["start"]), int(two[0]["end"]), int(two[0]["flags"])) == (int(at[a + 2]), int(at[b]) + 1, RR.FIRST) and int(two[-1]["flags"]) == RR.LAST


def test_the_cap_rule_at_scale(scale):
    from hifimeth_amd.pileup import GROUP_REGION_DTYPE
    from test_gpu_pileup_group_regions import _raw
    pu, info, rows, _want = scale
    t = info["thresholds"][0]
    want, R, hits = RR.regions_fast(rows, 0, *t)
    n = len(want)
    args = (0, info["n"], SC.MIN_REPS, 0, *t, 0)
    out = np.full(n * GROUP_REGION_DTYPE.itemsize, 0x55, np.uint8).view(GROUP_REGION_DTYPE)
    assert _raw(pu, *args, out=out, cap=n - 1) == (n, R, hits) and (out.view(np.uint8) == 0x55).all()      # nothing written
    assert _raw(pu, *args, out=out, cap=n) == (n, R, hits) and out.tobytes() == want.tobytes() and n > 5000


@pytest.mark.parametrize("where", ["inside the long heavy chain", "at row B T", "behind row B T"])
def test_two_stitched_fetches_equal_the_whole(scale, where):
    """the left part has 70 000 odd rows and sums that cross 2^32 when joined; exactly B T rows of context 0 (one block count per
    scan thread, every thread used; the cut lies inside the chain "row B T"); B T + 1 rows"""
    from hifimeth_amd.pileup import stitch_group_regions
    pu, info, rows, _want = scale
    at, n = info["row_gpos"], info["n"]
    cut = int({"inside the long heavy chain": at[info["chains"]["long heavy"][0] + 35000], "at row B T": at[B * T], "behind row B T": at[B * T] + 1}[where])
    for t in info["thresholds"][:2]:
        parts = [pu.group_regions(0, a, b, SC.MIN_REPS, *t, True)[:2] for a, b in ((0, cut), (cut, n))]
        assert where == "inside the long heavy chain" or parts[0][1] == B * T + (where == "behind row B T")
        assert parts[0][0][-1]["flags"] & RR.LAST and parts[1][0][0]["flags"] & RR.FIRST
        for keep in (False, True):
            got, R = stitch_group_regions(parts, t[2], t[3], keep_edges=keep)
            want = RR.regions_fast(rows, 0, *t, keep)
            assert R == want[1] == info["R"] and got.tobytes() == want[0].tobytes(), (where, t, keep)
            assert len(got) < len(parts[0][0]) + len(parts[1][0])                 # one chain was joined


def test_chaining_by_q_at_scale(scale):
    from hifimeth_amd.pileup import group_p_cutoff, group_qvalues
    pu, info, rows, _want = scale
    q, m = group_qvalues(rows)
    want_q, want_m = G.bh(rows["pvalue"], rows["motif"])
    assert q.tobytes() == want_q.tobytes() and m.tolist() == want_m and want_m[0] == info["R"]
    n = []
    for max_q in (0.05, 0.2):
        cut = group_p_cutoff(rows, q, max_q)
        assert cut.tobytes() == RR.p_cutoff(rows["pvalue"], q, rows["motif"], max_q).tobytes() and (cut > 0).all()
        for ctx in (0, 1):
            got = pu.group_regions(ctx, 0, info["n"], SC.MIN_REPS, float(cut[ctx]), 0.0, SC.MAX_GAP, 2)
            want = RR.regions_fast(rows, ctx, 1.0, 0.0, SC.MAX_GAP, 2, q=q, max_q=max_q)
            assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:]
            n.append(len(got[0]))
    assert n[0] < n[2] and min(n) > 0                          # at 0.05 only the rows of kinds 'H', 'p' and 'q' are hits of context 0


def test_other_fetches_in_between_change_nothing_at_scale(scale):
    """d_grows against the shared d_rows / d_blk / d_offs once all of them have grown"""
    pu, info, rows, _want = scale
    args = (0, 0, info["n"], SC.MIN_REPS, *info["thresholds"][0])
    first = pu.group_regions(*args)
    loci = pu.loci()
    part = pu.group_tests(777777, 999999, SC.MIN_REPS)
    again = pu.group_regions(*args)
    assert again[0].tobytes() == first[0].tobytes() and again[1:] == first[1:] and len(first[0]) == info["n_chains"]
    assert len(loci) == len(info["gpos"]) and loci["gpos"].tobytes() == info["gpos"].tobytes() and part.tobytes() == _within(rows, 777777, 999999).tobytes()


# ---- a reference past 2^32 bases ----------------------------------------------------------------------------------------------------------
def test_regions_around_two_to_the_32():
    """2 + 2 samples on a few dozen loci of a reference of [2^31, 2^31, the rest]: chains that end on the last base of a sequence and
    go on with the first of the next, at 2^31 and at 2^32; one wholly above 2^32; in context 1 a pair exactly MAX_GAP apart across
    2^32, in context 2 one MAX_GAP + 1 apart, in both a hit 2^32 less a few bases in front of the pair; the last base"""
    import torch
    from hifimeth_amd.pileup import MethylationPileup, stitch_group_regions
    from test_gpu_pileup_group_regions import _raw
    B31, B32 = bigref.B31, bigref.B32
    total = bigref.HOST_LEN[B32]
    lengths = [B31, B31, total - B32]
    need = total * (1 + 4 * 7 + 18) + total // 8 + (1 << 30)  # as test_groups_around_two_to_the_32
    free, _all = torch.cuda.mem_get_info()
    if free < need + (8 << 30):
        pytest.skip("the card has %.1f GB free, the case needs %.1f GB plus 8 GB" % (free / 1e9, need / 1e9))
    loci = [(5, "P"), (7, "P"), (9, "O"), (11, "C"), (20, "N"),
            (B31 - 4, "P"), (B31 - 2, "q"), (B31 - 1, "P"), (B31, "P"), (B31 + 2, "P"), (B31 + 5, "N"), (B31 + 7, "M"),
            (B32 - 9, "N"), (B32 - 5, "C"), (B32 - 4, "P"), (B32 - 2, "O"), (B32 - 1, "P"), (B32, "P"), (B32 + 1, "C"), (B32 + 2, "q"), (B32 + 3, "O"),
            (B32 + 20, "N"), (B32 + 100, "M"), (B32 + 102, "M"), (B32 + 104, "M"), (B32 + 105, "U"), (B32 + 106, "M"), (B32 + 200, "N"),
            (total - 3, "A"), (total - 1, "P")]
    gpos, kind = np.array([g for g, _k in loci], np.int64), [k for _g, k in loci]
    pu = MethylationPileup([("c%d" % k, n) for k, n in enumerate(lengths)], partitions=True, groups=True, group_min_cov=SC.MIN_COV,
                           bases=np.full(total, ord("N"), np.uint8))
    try:
        assert pu.n_loci == total > B32
        for g, s in ((2, 0), (1, 0), (1, 1), (2, 1)):
            here = [k for k in range(len(loci)) if SC.KINDS[kind[k]][g][s] is not None]
            counts = [SC.KINDS[kind[k]][g][s] for k in here]
            assert pu.begin_sample(g) == s
            assert pu.load_sample_loci(gpos[here][::-1], [c[0] for c in counts][::-1], [c[1] for c in counts][::-1], [SC.KINDS[kind[k]][0] for k in here][::-1]) == len(here)
        rows = pu.group_tests(min_reps=SC.MIN_REPS)
        assert rows["gpos"].tolist() == [g for g, k in loci if k != "U"] and rows["motif"].tolist() == [SC.KINDS[k][0] for _g, k in loci if k != "U"]
        tested = [k for k in kind if k != "U"]
        for r, k in zip(rows, tested):                        # a kind's rows are bit-identical below 2^31 and above 2^32 ('q': phi > 1)
            assert r["diff"] == G.stat_f64(*SC.kind_sums(k))[0] and (r["pvalue"] < 0.008) == bool(SC.SIGN[k]), (k, r)
            assert all(r[f].tobytes() == rows[tested.index(k)][f].tobytes() for f in STAT_FIELDS), (k, r)
        assert rows[tested.index("q")]["gpos"] < B31 and rows[tested.index("q")]["phi"] > 1.0 and tested.count("q") == 2
        offs = [0, B31, B32, total]
        ranges = [(0, total)] + list(zip(offs[:-1], offs[1:]))
        for ctx in (0, 1, 2):
            for keep in (False, True):
                for max_gap, min_loci in ((SC.MAX_GAP, 1), (SC.MAX_GAP, 3), (SC.MAX_GAP + 1, 2)):
                    whole = None
                    for lo, hi in ranges:
                        got = pu.group_regions(ctx, lo, hi, SC.MIN_REPS, 0.01, 0.0, max_gap, min_loci, keep)
                        want = RR.regions_fast(rows[(rows["gpos"] >= lo) & (rows["gpos"] < hi)], ctx, 0.01, 0.0, max_gap, min_loci, keep)
                        assert got[0].tobytes() == want[0].tobytes() and got[1:] == want[1:], (ctx, keep, max_gap, min_loci, lo, hi)
                        whole = whole or got
                    parts = [pu.group_regions(ctx, lo, hi, SC.MIN_REPS, 0.01, 0.0, max_gap, min_loci, True)[:2] for lo, hi in ranges[1:]]
                    stitched, R_ = stitch_group_regions(parts, max_gap, min_loci, keep_edges=keep)
                    assert stitched.tobytes() == whole[0].tobytes() and R_ == whole[1], (ctx, keep, max_gap, min_loci)
        chains = lambda ctx, lo, hi, max_gap=SC.MAX_GAP: [(int(g["start"]), int(g["end"]), int(g["n_loci"]), int(g["sign"]), int(g["flags"]))
                                                          for g in pu.group_regions(ctx, lo, hi, SC.MIN_REPS, 0.01, 0.0, max_gap, 1)[0]]
        assert chains(0, 0, total) == [(5, 8, 2, 1, RR.FIRST), (B31 - 4, B31 + 3, 5, 1, 0), (B31 + 7, B31 + 8, 1, -1, 0), (B32 - 4, B32 + 3, 4, 1, 0),
                                       (B32 + 100, B32 + 107, 4, -1, 0), (total - 1, total, 1, 1, RR.LAST)]
        assert chains(0, 0, B31)[-1] == (B31 - 4, B31, 3, 1, RR.LAST) and chains(0, B31, B32)[0] == (B31, B31 + 3, 2, 1, RR.FIRST)
        assert chains(0, B31, B32)[-1] == (B32 - 4, B32, 2, 1, RR.LAST) and chains(0, B32, total)[0] == (B32, B32 + 3, 2, 1, RR.FIRST)
        # contexts 1 and 2: a first hit 2^32 - 11 and 2^32 - 16 bases in front of the next (no link, whatever 32 bits of that say), then
        assert chains(1, 0, total) == [(9, 10, 1, 1, RR.FIRST), (B32 - 2, B32 + 4, 2, 1, RR.LAST)]  # exactly MAX_GAP apart
        assert chains(2, 0, total) == [(11, 12, 1, -1, RR.FIRST), (B32 - 5, B32 - 4, 1, -1, 0), (B32 + 1, B32 + 2, 1, -1, RR.LAST)]     # MAX_GAP + 1 apart ...
        assert chains(2, 0, total, SC.MAX_GAP + 1) == [(11, 12, 1, -1, RR.FIRST), (B32 - 5, B32 + 2, 2, -1, RR.LAST)]                 # ... and linked at that
        assert _raw(pu, 0, total + 1, SC.MIN_REPS, 0, 0.01, 0.0, SC.MAX_GAP, 1, 0)[0] == HM_EINVAL
    finally:
        pu.close()
        torch.cuda.empty_cache()
