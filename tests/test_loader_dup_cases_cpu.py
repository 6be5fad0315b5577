"""loader_dup_cases.py held to itself, without a GPU: the two routes to the expected counters agree for every case, loader and row
order; every case puts its rows where it says; the sizes stay within what a quick GPU test may load."""
import numpy as np
import pytest

import loader_dup_cases as D
from loader_dup_cases import GROUP, HM_EDATA, LOADERS, WAVE

CASES = D.cases()


def _last(case, loader="groupdiff"):
    return case.calls(loader)[-1][1]


def test_the_catalogue_holds_what_it_must():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for want in ("pairs-across", "pairs-within", "k-fold, contiguous", "k-fold, stride 257", "neighbours", "across-slabs", "across-calls",
                 "with-other-bad-rows", "identical-duplicates"):
        assert any(n.startswith(want) for n in names), want
    assert D.TOTAL <= 10000 and len(D.LENGTHS) == 3
    for case in CASES:
        for loader in LOADERS:
            calls = case.calls(loader)
            assert sum(len(rows[0]) for _t, rows in calls) <= D.MAX_ROWS, case
            targets = [t for t, _rows in calls]
            assert targets == sorted(targets) and set(targets) <= {1, 2} and targets[0] == 1, case
            for _t, rows in calls:
                assert len({len(x) for x in rows}) == 1 and all(x.dtype == np.int64 for x in rows)


def test_the_message_is_the_engines():
    """the literals test_gpu_pileup_loaders.py pins"""
    assert D.message("diff", 2, 3, 0, 7, 11) == ("hm_pileup_load_loci: 23 bad rows: 2 gpos outside the reference, 3 negative count, 7 motif above 3, "
                                                "11 locus given twice for one part")
    assert D.message("samplecorr", 2, 3, 5, 7, 11) == ("hm_sample_load: 28 bad rows: 2 gpos outside the reference, 3 negative count, "
                                                      "5 count above 2^20 - 1, 7 motif above 3, 11 locus given twice in one sample")
    assert D.message("groupdiff", 0, 0, 4, 0, 0) == "hm_pileup_load_sample_loci: 4 bad rows: 4 count above 2^20 - 1"


@pytest.mark.parametrize("loader", LOADERS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_two_routes_agree_in_every_order(case, loader):
    """sum (k - 1) against the restatement fed the rows in order, as placed and in three permutations: the counters do not depend on
    the order, and neither do the planes of `diff` (a duplicate adds) nor, where duplicates equal their partners, those of the others"""
    first = None
    for order in range(D.N_ORDERS):
        want = D.by_counts(case, loader, order)
        got, ref = D.by_restatement(case, loader, order)
        print(case, loader, order, want["returns"], want["dup"], want["added"], got["added"], want["message"])
        assert got["returns"] == want["returns"] and want["returns"][-1] == HM_EDATA and all(r > 0 for r in want["returns"][:-1])
        assert got["dup"] == want["dup"] > 0 and got["message"] == want["message"]
        assert got["added"] in (None, want["added"]) and (got["added"] is None) == (loader == "diff")
        assert (got["covered"] == want["covered"]).all() and len(want["covered"]) > 0
        planes = {k: v.copy() for k, v in ref.planes.items()}
        if loader == "diff":                                  # every counted row added: the planes hold the sum of their counts
            weight = sum(int((p + n)[_counted(g, p, n, m, False)].sum()) for _t, (g, p, n, m) in case.calls(loader, order))
            assert int(planes["pcov"].sum() + planes["ncov"].sum()) == weight == int(sum(planes[k].sum() for k in ("pcov1", "ncov1", "pcov2", "ncov2")))
        if first is None:
            first = (want, planes)
        assert (want["returns"], want["dup"], want["message"], want["added"]) == tuple(first[0][k] for k in ("returns", "dup", "message", "added"))
        if loader == "diff" or case.name == "identical-duplicates":
            assert all((planes[k] == first[1][k]).all() for k in planes), order


def _counted(g, p, n, m, limited):
    ok = (g >= 0) & (g < D.TOTAL) & (p >= 0) & (n >= 0) & (m <= 3)
    return ok & (p + n > 0) & ((p + n < D.LIMIT) | (not limited))


def test_duplicates_are_sum_k_minus_one_by_hand():
    """the rule on the smallest input, written out: a locus of 4 rows, one of 2, one alone, one row without a count, one bad row"""
    g, p, n, m = (np.array(x, np.int64) for x in ([7, 7, 9, 7, 9, 7, 3, 7, 7], [1, 0, 2, 0, 2, 5, 1, 0, 1], [0, 1, 2, 3, 0, 5, 1, 0, 1], [0, 1, 2, 3, 0, 1, 2, 3, 4]))
    case = D.Case("by hand", [(1, (g, p, n, m))], "none")
    for loader in LOADERS:
        want = D.by_counts(case, loader)
        assert want["dup"] == (4 - 1) + (2 - 1) and want["added"] == (7 if loader == "diff" else 3) and want["covered"].tolist() == [3, 7, 9]
        assert want["message"].endswith(": 5 bad rows: 1 motif above 3, 4 " + D.DUP_TEXT[loader])
        assert D.by_restatement(case, loader)[0]["message"] == want["message"]


# ---- every case meets the placement it claims --------------------------------------------------------------------------------------
def _pair_kind(p, n, a, b):
    """the kind of every pair of rows (a, b), -1 for none of the four"""
    pa, na, pb, nb = p[a] > 0, n[a] > 0, p[b] > 0, n[b] > 0
    out = np.full(len(a), -1)
    for k, (w, x, y, z) in enumerate(((True, True, True, True), (True, False, False, True), (False, True, True, False), (True, False, True, False))):
        out[(pa == w) & (na == x) & (pb == y) & (nb == z)] = k
    return out


PLACED = {
    "different workgroups": lambda a, b, s: (a // GROUP != b // GROUP).all(),
    "adjacent lanes of one wavefront": lambda a, b, s: (b == a + 1).all() and (a // WAVE == b // WAVE).all(),
    "lanes l and 63 - l of one wavefront": lambda a, b, s: (a // WAVE == b // WAVE).all() and (a % WAVE + b % WAVE == 63).all()
    and ((a % WAVE == 0) & (b % WAVE == 63)).any() and ((a % WAVE == 31) & (b % WAVE == 32)).any(),
    "two wavefronts of one workgroup": lambda a, b, s: (a // GROUP == b // GROUP).all() and (a // WAVE != b // WAVE).all(),
    "different launches": lambda a, b, s: (a // s != b // s).all(),
    "one launch, different workgroups": lambda a, b, s: (a // s == b // s).all() and (a % s // GROUP != b % s // GROUP).all(),
    "slabs of 1000": lambda a, b, s: s == 1000 and (a // s != b // s).all() and (a % s // WAVE != b % s // WAVE).any(),
}


@pytest.mark.parametrize("case", [c for c in CASES if c.partners is not None], ids=repr)
def test_pairs_stand_where_the_case_says(case):
    g, p, n, m = _last(case)
    a, b = case.partners[:, 0], case.partners[:, 1]
    slab = case.slab or len(g)
    assert (g[a] == g[b]).all() and len(np.unique(g[a])) == len(a) and (a < b).all()
    assert PLACED[case.claim](a, b, slab), case.claim
    in_runs = np.concatenate(list(case.runs.values())) if case.runs else np.zeros(0, np.int64)
    loci, k = np.unique(g, return_counts=True)
    assert sorted(loci[k == 2].tolist()) == sorted(g[a].tolist()) and int((k > 2).sum()) == (len(case.runs) if case.runs else 0)
    if case.kinds is not None:
        assert (_pair_kind(p, n, a, b) == case.kinds).all()
        assert (np.bincount(case.kinds, minlength=4) >= len(a) // 4).all() and ((m[a] != m[b]).any() and ((p[a] != p[b]) | (n[a] != n[b])).any())
    else:                                                     # identical-duplicates: every row of a locus equals the others
        assert case.name == "identical-duplicates"
        for x in (p, n, m):
            assert (x[a] == x[b]).all()
            assert all(len(set(x[at].tolist())) == 1 for at in case.runs.values())
        assert sorted(len(at) for at in case.runs.values()) == [3, 64, 65] and len(in_runs) == 132


def test_pairs_across_holds_every_kind_256_times():
    case = D.case("pairs-across")
    assert len(case.partners) == 2048 and (np.bincount(case.kinds, minlength=4) >= 256).all()
    g, p, n, m = _last(case)
    assert (np.bincount(_pair_kind(p, n, case.partners[:, 0], case.partners[:, 1]), minlength=4) == 512).all()
    for other in CASES:
        if other.name.startswith("across-slabs"):             # the same rows, cut into launches
            assert all((x == y).all() for x, y in zip(_last(other), _last(case))) and other.slab and len(g) > other.slab or other.slab == len(g)


@pytest.mark.parametrize("name", ["k-fold, contiguous", "k-fold, stride 257"])
def test_folds_stand_where_the_case_says(name):
    case = D.case(name)
    g, p, n, m = _last(case)
    loci, k = np.unique(g, return_counts=True)
    assert sorted(set(k[k > 1].tolist())) == list(D.FOLDS) and sorted(case.runs) == sorted(loci[k > 1].tolist()) and (k == 1).sum() >= 100
    for locus, at in case.runs.items():
        assert (g[at] == locus).all() and len(at) == k[loci == locus][0]
        step = np.diff(at) % len(g)
        if case.claim == "contiguous":
            assert (step == 1).all()
        else:                                                 # the next row of a locus: the next lane of the next workgroup, around the end of the call
            assert case.claim == "stride 257" and (step == D.STRIDE).all() and len(g) % D.STRIDE and len({int(i) // GROUP for i in at}) >= min(len(at), 16)
        kinds = {(bool(x), bool(y)) for x, y in zip(p[at], n[at])}
        assert len(at) < 8 or kinds == {(True, True), (True, False), (False, True)}       # the kinds are mixed


def test_neighbours_share_their_words():
    near = D.neighbour_loci()
    for name in ("neighbours", "identical-duplicates"):
        g = _last(D.case(name))[0]
        loci, k = np.unique(g, return_counts=True)
        twice = set(loci[k >= 2].tolist())
        assert set(near.tolist()) <= twice
        assert {100, 101, 201, 202} <= twice and set(D.ENDS) <= twice
        words = np.unique(np.array(sorted(twice)) // 32, return_counts=True)
        assert (words[1] == 32).sum() >= 2                    # whole bitmap words: eight sample-count words, sixteen level words each
        assert D.OFFSETS[1] // 32 == (D.OFFSETS[1] - 1) // 32 and set(range(4096, 4128)) <= twice      # one word across a contig boundary
        assert D.TOTAL % 32 and set(range(D.TOTAL // 32 * 32, D.TOTAL)) <= twice             # the last, partial word


def test_across_calls_is_what_it_says():
    case = D.case("across-calls")
    for loader in LOADERS:
        (t1, r1), (t2, r2), (t3, r3) = case.calls(loader)
        assert (t1, t2, t3) == (1, 2, 2)
        assert len(np.unique(r1[0])) == len(r1[0]) == 600 and sorted(r1[0].tolist()) == sorted(r2[0].tolist()) and len(np.unique(r3[0])) == len(r3[0])
        again = np.intersect1d(r2[0], r3[0])
        want = D.by_counts(case, loader)
        assert len(again) == want["dup"] == 300 and len(r3[0]) == 400
        assert want["returns"] == [600, 600, HM_EDATA] and want["added"] == 1200 + (400 if loader == "diff" else 100)
        assert want["message"] == "%s: 300 bad rows: 300 %s" % (D.WHO[loader], D.DUP_TEXT[loader])


def test_other_bad_rows_are_all_there():
    case = D.case("with-other-bad-rows")
    for loader in LOADERS:
        g, p, n, m = _last(case, loader)
        want = D.by_counts(case, loader)
        big = 0 if loader == "diff" else 6
        assert want["message"] == D.message(loader, 5, 4, big, 7, 40 + 2 + 64) and want["dup"] == 106       # 40 pairs, a locus of 3 rows, one of 65
        assert ((p == 0) & (n == 0) & (m <= 3)).sum() == 6 and (len(g) == 1500 + 80 + 68 + 16 + 6 + big)
        loci, k = np.unique(g[_counted(g, p, n, m, loader != "diff")], return_counts=True)
        assert sorted(k[k > 1].tolist()) == [2] * 40 + [3, 65]                # the bad rows and the rows without a count on these loci change nothing
