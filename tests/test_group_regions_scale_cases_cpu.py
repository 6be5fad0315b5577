"""The references of tests/test_gpu_pileup_group_regions_scale.py without a GPU: group_regions_ref.regions_fast against the two loop
formulations, byte for byte; group_regions_scale_cases.build at (B, T) = (16, 8) -- its rows restated by groups_ref.GroupLoader
and stat_f64 -- holding every property its info claims; groups_ref.bh against a loop over ranks; stitch_group_regions over the
parts of the small case at every cut."""
import functools

import numpy as np
import pytest

import group_regions_ref as RR
import group_regions_scale_cases as SC
import groups_ref as G

B, T = 16, 8
HEAVY_SCALE = 1000                                            # see test_stitched_parts_of_the_small_case


@functools.lru_cache(maxsize=None)
def small():
    """-> (samples, info, the hm_group_t rows of build(16, 8) made as RR.dataset_rows() makes its own)"""
    samples, info = SC.build(B, T)
    ref = G.GroupLoader(info["n"], SC.MIN_COV)
    counted = SC.counted(samples)
    for g, s in SC.SAMPLES:
        assert ref.begin_sample(g) == s and ref.load(*samples[(g, s)]) == counted[(g, s)]
    tested = ref.tested(SC.MIN_REPS)
    rows = np.zeros(len(tested), RR.ROW_DTYPE)
    for k, (gpos, motif, m1, p1, n1, m2, p2, n2) in enumerate(tested):
        d, D, phi, p = G.stat_f64(*ref.sums(gpos))
        rows[k] = (gpos, p1, n1, p2, n2, motif, m1, m2, d, D, phi, p)
    rows.setflags(write=False)
    return samples, info, rows


def _all_three(rows, ctx, max_p, min_diff, max_gap, min_loci, keep, **by_q):
    fast = RR.regions_fast(rows, ctx, max_p, min_diff, max_gap, min_loci, keep, **by_q)
    for chains_of in (RR.chains_walk, RR.chains_union_find):
        want = RR.regions(rows, ctx, max_p, min_diff, max_gap, min_loci, keep, chains_of=chains_of, **by_q)
        assert fast[0].dtype == RR.REGION_DTYPE and fast[0].tobytes() == want[0].tobytes() and fast[1:] == want[1:], (ctx, max_p, min_diff, max_gap, min_loci, keep)
    return len(fast[0])


def test_the_fast_restatement_equals_the_two_loops():
    n = 0
    for rows, sets in ((RR.crafted_rows(), ((0.01, 10.0, 10, 1), (0.01, 0.0, 10, 3), (1.0, 0.0, 4, 2))), (RR.dataset_rows(), RR.THRESHOLDS),
                       (small()[2], small()[1]["thresholds"])):
        for ctx in (0, 1, 2):
            for t in sets:
                for keep in (False, True):
                    n += _all_three(rows, ctx, *t, keep)
    assert n > 500
    rows = RR.dataset_rows()
    q, _m = G.bh(rows["pvalue"], rows["motif"])
    for max_q in (0.05, 0.3, 1e-12):                          # by q; under the last no row is a hit
        for ctx in (0, 1, 2):
            assert (_all_three(rows, ctx, 1.0, 0.0, 30, 2, False, q=q, max_q=max_q) > 0) == (max_q > 1e-12)
    assert RR.regions_fast(rows[:0], 0, 0.01, 0.0, 5, 1)[1:] == (0, 0) and RR.regions_fast(rows[:1], int(min(rows["motif"][0], 2)), 1.0, 0.0, 5, 1, True)[1] == 1


def test_the_small_case_gives_the_rows_it_was_made_for():
    """the integer fields and diff from the samples alone (what the GPU test compares 4 Mi rows with) equal the restated loader's;
    per kind the statistic is what SIGN says: the hits' p below 0.008, D = 0 and p = 1 for 'N' and 'o', 'A' a hit only at max_p 1"""
    samples, info, rows = small()
    want = SC.expected_rows(samples, info["n"])
    for f in ("gpos", "motif", "m1", "m2", "pcov1", "ncov1", "pcov2", "ncov2", "diff"):
        assert want[f].tobytes() == rows[f].tobytes(), f
    tested = info["kind"] != ord("U")
    assert rows["gpos"].tolist() == info["gpos"][tested].tolist() and (info["kind"] == ord("U")).sum() >= 1
    kind = info["kind"][tested]
    assert {chr(k) for k in kind} == set(SC.KINDS) - {"U"}     # every kind has a row
    for k, sign in SC.SIGN.items():
        r = rows[kind == ord(k)]
        assert len({x.tobytes() for x in r}) == len(r) and (r["motif"] == SC.KINDS[k][0]).all()      # they differ in gpos alone
        d, D, phi, p = G.stat_f64(*SC.kind_sums(k))
        assert (r["diff"] == d).all() and (r["D"] == D).all() and (r["phi"] == phi).all() and (r["pvalue"] == p).all(), k
        if sign:
            assert p < 0.008 and np.sign(d) == sign, k
        else:
            assert (D == 0.0 and p == 1.0 and d == 0.0) if k in "No" else (d == 10.0 and 0.3 < p < 1.0), k
    assert G.stat_f64(*SC.kind_sums("q"))[2] > 1.0 and SC.kind_sums("p")[3] == 3 and SC.kind_sums("b") == SC.kind_sums("P")
    assert min(SC.kind_sums("H")[k] for k in (1, 5)) == 2000000 and 1000000 < G.LIMIT


def test_the_small_case_holds_what_info_claims():
    """the chains listed with their lengths, signs, flags and first rows modulo B; the slices of both selections; the chains at the
    first thresholds within their bounds; the sums of the long heavy chain.  At B = 16 that chain has B + 2 rows, not 70 001: its
    sums are asserted as the rows' own, and that 70 001 such rows exceed 2^32 in each of the four."""
    _samples, info, rows = small()
    R, n = info["R"], info["n"]
    cpg = rows[RR.ctx_mask(rows, 0)]
    assert (R, n) == (B * T + 3 * B + 5, (2 * T + 4) * B - 1) == (len(cpg), sum(info["lengths"])) and cpg["gpos"][0] == 0 and cpg["gpos"][-1] == n - 1
    assert cpg["gpos"].tolist() == info["row_gpos"].tolist()
    blocks = lambda x: -(-x // B)
    assert (blocks(R), blocks(n)) == (T + 4, 2 * T + 4) and -(-blocks(R) // T) == 2 and -(-blocks(n) // T) == 3      # per = 2 and 3
    assert (np.diff(cpg["gpos"]) == 2).sum() > R // 2
    got, R_, hits = RR.regions_fast(rows, 0, 0.01, 0.0, SC.MAX_GAP, 1)
    by_start = {int(g["start"]): g for g in got}
    assert R_ == R and hits > 3 * B
    for name, (a, b, sign, flags) in info["chains"].items():
        g = by_start[int(cpg["gpos"][a])]
        assert (int(g["end"]), int(g["n_loci"]), int(g["sign"]), int(g["flags"])) == (int(cpg["gpos"][b]) + 1, b - a + 1, sign, flags), name
    c = info["chains"]
    m = info["min_loci"]
    assert m == B + 3 and [c[k][1] - c[k][0] + 1 for k in ("min_loci - 1", "min_loci", "min_loci + 1")] == [m - 1, m, m + 1]
    assert all(c[k][0] % B == B - 1 for k in ("min_loci - 1", "min_loci", "min_loci + 1", "long heavy"))
    assert c["min_loci - 1"][0] < B < 2 * B <= c["min_loci - 1"][1] and c["row B T"][0] < B * T <= c["row B T"][1]
    at = lambda r: int(cpg["gpos"][r])
    assert at(3 * B) - at(3 * B - 1) == SC.MAX_GAP and at(7 * B) - at(7 * B - 1) == SC.MAX_GAP + 1
    inside = {int(g): chr(k) for g, k in zip(info["gpos"], info["kind"])}
    assert inside[at(B) - 1] == "U" and inside[at(2 * B) - 1] == "O" and at(B) - at(B - 1) == at(2 * B) - at(2 * B - 1) == 2
    kept = RR.regions_fast(rows, 0, *info["thresholds"][1])[0]
    assert [int(g["n_loci"]) for g in kept] == [m, m + 1] and info["thresholds"][1][3] == m
    # the sequence boundary: one chain over the whole, two per sequence
    first = info["lengths"][0]
    a, b = c["sequence boundary"][:2]
    assert at(a + 1) < first == at(a + 2)
    one, two = RR.regions_fast(rows[rows["gpos"] < first], 0, 0.01, 0.0, SC.MAX_GAP, 1)[0], RR.regions_fast(rows[rows["gpos"] >= first], 0, 0.01, 0.0, SC.MAX_GAP, 1)[0]
    assert (int(one[-1]["start"]), int(one[-1]["end"]), int(one[-1]["flags"])) == (at(a), at(a + 1) + 1, RR.LAST)
    assert (int(two[0]["start"]), int(two[0]["end"]), int(two[0]["flags"])) == (at(a + 2), at(b) + 1, RR.FIRST)
    # the long heavy chain
    a, b = c["long heavy"][:2]
    long = by_start[at(a)]
    assert info["long_n"] == b - a + 1 == B + 2 and tuple(int(long[f]) for f in ("pcov1", "ncov1", "pcov2", "ncov2")) == info["long_sums"]
    assert all(s % info["long_n"] == 0 and s // info["long_n"] * 70001 > 1 << 32 for s in info["long_sums"])
    assert long["diff"] == RR.pooled_diff(*info["long_sums"]) == 40.0
    # chains at the first thresholds, and rows of the other contexts
    lo, hi = info["n_chains_bounds"]
    assert lo <= len(RR.regions_fast(rows, 0, *info["thresholds"][0])[0]) == info["n_chains"] <= hi
    assert len(RR.regions_fast(rows, 1, 0.01, 0.0, SC.MAX_GAP, 1)[0]) >= 2 and RR.regions_fast(rows, 1, 0.01, 0.0, SC.MAX_GAP, 1)[1] > 3
    weak, strict = RR.regions_fast(rows, 0, *info["thresholds"][2])[2], RR.regions_fast(rows, 0, 0.01, 0.0, SC.MAX_GAP, 1)[2]
    assert weak > strict                                      # 'A' rows are hits at max_p 1
    assert len(RR.regions_fast(rows, 0, *info["thresholds"][3])[0]) and at(a) not in {int(g["start"]) for g in RR.regions_fast(rows, 0, *info["thresholds"][3])[0]}


def _bh_loop(p, motif):
    """Benjamini-Hochberg by the book, a loop from the largest p down: q_(k) = min(1, min over j >= k of p_(j) m / j)"""
    q, m = [float("nan")] * len(p), [0, 0, 0]
    for c in range(3):
        idx = sorted((i for i in range(len(p)) if min(int(motif[i]), 2) == c), key=lambda i: p[i])
        m[c] = len(idx)
        run = 1.0
        for rank in range(len(idx), 0, -1):
            run = min(run, float(p[idx[rank - 1]]) * float(m[c]) / float(rank))
            q[idx[rank - 1]] = run
    return np.array(q, np.float64), m


def test_the_vectorised_bh_equals_a_loop_over_ranks():
    """groups_ref.bh is the restatement the GPU test applies to 4 Mi rows; equal p gives equal q, per context"""
    rows = RR.dataset_rows()
    rng = np.random.default_rng(12)
    tied_p = rng.choice(np.concatenate([rng.random(12) ** 4, [1.0, G.DBL_MIN]]), 3000)
    for p, motif in ((rows["pvalue"], rows["motif"]), (tied_p, rng.integers(0, 4, 3000)), (small()[2]["pvalue"], small()[2]["motif"])):
        got, want = G.bh(p, motif), _bh_loop(p, motif)
        assert got[0].tobytes() == want[0].tobytes() and list(got[1]) == want[1]
        for c in range(3):
            sel = np.minimum(motif, 2) == c
            assert all(len(set(got[0][sel][p[sel] == v])) == 1 for v in np.unique(p[sel]))
    assert len(np.unique(tied_p)) <= 14


@pytest.mark.parametrize("keep", [False, True])
def test_stitched_parts_of_the_small_case(keep):
    """stitch_group_regions over the parts on either side of every base equals the fast restatement over the whole.  The four
    counts of the rows of kind 'H' are multiplied by 1000 here (int32 holds them, diff stays 40), so that the B + 2 rows of the long
    heavy chain sum to more than 2^32 and a cut inside it makes the stitch add across that on the host."""
    from hifimeth_amd.pileup import stitch_group_regions
    _samples, info, rows = small()
    rows = rows.copy()
    heavy = np.isin(rows["gpos"], info["gpos"][info["kind"] == ord("H")])
    for f in ("pcov1", "ncov1", "pcov2", "ncov2"):
        rows[f][heavy] *= HEAVY_SCALE
    a, b = (int(info["row_gpos"][r]) for r in info["chains"]["long heavy"][:2])
    n, joined = info["n"], 0
    for max_p, min_diff, max_gap, min_loci in info["thresholds"][:3]:
        whole = RR.regions_fast(rows, 0, max_p, min_diff, max_gap, min_loci, keep)
        long = whole[0][whole[0]["start"] == a]
        if info["long_n"] < min_loci:                         # the chain is not returned: the parts' pieces are still joined, then dropped
            assert len(long) == 0
            long = RR.regions_fast(rows, 0, max_p, min_diff, max_gap, 1)[0]
            long = long[long["start"] == a]
        assert len(long) == 1 and min(int(long[0][f]) for f in ("pcov1", "ncov1", "pcov2", "ncov2")) > 1 << 32
        for cut in range(n + 1):
            parts = RR.parts_of(rows, [0, cut, n], 0, max_p, min_diff, max_gap, min_loci)
            got, R = stitch_group_regions(parts, max_gap, min_loci, keep_edges=keep)
            assert got.tobytes() == whole[0].tobytes() and R == whole[1], (cut, min_loci)
            if a < cut <= b:
                left, right = parts[0][0][-1], parts[1][0][0]
                assert left["flags"] & RR.LAST and right["flags"] & RR.FIRST and int(left["pcov1"]) + int(right["pcov1"]) == int(long[0]["pcov1"])
                joined += 1
    assert joined >= 3 * B
