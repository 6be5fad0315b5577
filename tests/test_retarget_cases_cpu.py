"""The inputs of test_gpu_pileup_retarget.py are what retarget_cases.py says they are: the in-bounds rule holds for every case, job A
and job B differ in everything that is compared, and job B's loaded rows meet job A's seen bits.  Needs no GPU."""
import numpy as np
import pytest

import retarget_cases as R


def test_every_case_keeps_the_rule():
    """`changed` and `shorter` only where nothing is resident; every family at every depth onto `same`"""
    assert len(set(R.RECORD_CASES)) == len(R.RECORD_CASES)
    for family, depth, target in R.RECORD_CASES:
        assert family in R.FAMILIES and depth in R.DEPTHS and target in R.TARGETS
        assert R.rule_holds(depth, target), (family, depth, target)
    assert not R.rule_holds("a", "shorter") and not R.rule_holds("b", "changed") and R.rule_holds("b", "same")
    for family in R.FAMILIES:
        if family != "plain, plane functions":
            assert {(d, t) for f, d, t in R.RECORD_CASES if f == family} >= {(d, "same") for d in R.DEPTHS}, family
    for target in ("changed", "shorter"):
        names = {n for f, d, t in R.RECORD_CASES if t == target for n in R.FAMILIES[f][1]}
        assert names >= set(R.PLANE_FNS) | {"patterns", "bedmethyl_0", "linkage", "readpos"}, target
    cat = {n for n, _f in R.S.CATALOGUE}
    assert all(set(names) <= cat for _o, names in R.FAMILIES.values())


def test_the_references_are_what_their_names_say():
    first, same, changed, shorter = (R.reference(n) for n in ("first", "same", "changed", "shorter"))
    length = lambda g: [len(s) for _n, s in g]  # noqa: E731
    assert same == first and same is not None
    assert length(changed) == length(first) and all(a != b for (_n, a), (_m, b) in zip(changed, first))
    assert R.cpg_list(changed) != R.cpg_list(first) and len(set(R.cpg_list(changed)) ^ set(R.cpg_list(first))) > 100
    assert all(a < b for a, b in zip(length(shorter), length(first))) and sum(length(shorter)) < sum(length(first))
    assert 0 < len(R.cpg_list(shorter)) < len(R.cpg_list(first))
    assert 3000 < sum(length(first)) < 10000 and len(first) == 3


def test_the_reads_lie_inside_their_reference_and_carry_haplotypes():
    for name in ("A",) + R.TARGETS:
        g, reads = R.job(name)
        assert len(reads) == R.N_READS and {r.hp for r in reads} == {0, 1, 2} and {r.flag & 16 for r in reads} == {0, 16}
        assert {r.tid for r in reads} == {0, 1, 2} and all(len(s) == R.N_READS // R.N_SLABS for s in R.slabs(reads))
        assert len({r.mapq >= R.FILTER["min_mapq"] for r in reads}) == 2          # the mapq filter drops some reads and keeps some
    assert [r.seq for r in R.job("A")[1]] != [r.seq for r in R.job("same")[1]]


def _differs(a, b):
    return not np.array_equal(a, b) if isinstance(a, np.ndarray) else a != b


@pytest.mark.parametrize("target", R.TARGETS)
def test_job_a_and_job_b_differ_in_every_compared_output(target):
    """histograms, thresholds of the feeding, planes (the loci rows: every function of the planes follows them) and each table"""
    a, b = R.restated("A"), R.restated(target)
    assert set(a) == set(b) >= {"histograms", "loci", "loci_part1", "loci_part2", "bedmethyl_0", "bedmethyl_1", "patterns", "linkage", "readpos"}
    for key in a:
        if key != "thresholds":
            assert (key == "histograms" or len(b[key]) > 20) and _differs(a[key], b[key]), key
    assert a["thresholds"] != b["thresholds"]
    # the histogram's three contexts each differ, so a stale histogram moves every median
    assert all((a["histograms"][c] != b["histograms"][c]).any() and b["histograms"][c].sum() > 1000 for c in range(3))


def test_trim_and_filters_change_job_b():
    """the options that persist over the second call change what job B gives: an engine that lost them would show"""
    plain, cut, kept = R.restated("same"), R.restated("same", trim=True), R.restated("same", filtered=True)
    assert cut["readpos"] != plain["readpos"] and cut["loci"] != plain["loci"] and (cut["histograms"] != plain["histograms"]).any()
    assert kept["loci"] != plain["loci"] and len(kept["loci"]) > 100          # (the histograms take every primary read: no filter)
    from oracle import pileup_oracle as P
    g, reads = R.job("same")
    dicts = [R.C.as_dict(r) for r in reads]
    thr = kept["thresholds"][-1]
    every, by_mapq, by_both = (len(P.pileup(dicts, g, thresholds=thr, **kw)["records"])
                               for kw in ({}, dict(min_mapq=R.FILTER["min_mapq"]), R.FILTER))
    assert every > by_mapq > by_both > 0                                       # each of the two filters drops reads of job B


# ---- the loaded rows --------------------------------------------------------------------------------------------------------------------
def _counted(rows):
    g, p, n, _m = rows
    return set(g[p + n > 0].tolist())


def test_loaded_rows_are_clean_and_job_b_meets_job_a():
    """no row set holds a locus twice or a bad row; per part, job B hits loci that job A hit for that part (stale seen bits would
    make them duplicates) and loci that no row of job A hit"""
    all_a = set().union(*(_counted(R.load_rows("A", k)) for k in range(4)))
    for job in "AB":
        for k in range(4):
            g, p, n, m = R.load_rows(job, k)
            assert len(g) == R.N_ROWS == len(np.unique(g)) and g.min() >= 0 and g.max() < R.TOTAL and (p >= 0).all() and (n >= 0).all() and m.max() <= 3
            assert 0 < (p + n >= R.LOAD_MIN_COV).sum() < (p + n > 0).sum() <= R.N_ROWS
    for k in range(4):
        a, b = _counted(R.load_rows("A", k)), _counted(R.load_rows("B", k))
        assert len(a & b) > 100 and len(b - all_a) > 100, k
        # ... in the same words of the same bitmap: the reference and with it the words per bitmap are the same
        assert {g // 32 for g in a} & {g // 32 for g in b - a}
    assert R.load_genome() == R.load_genome() and sum(len(s) for _n, s in R.load_genome()) == R.TOTAL
    assert (R.TOTAL + 31) // 32 * 32 != R.TOTAL                                  # the last word of a bitmap is a partial one


def test_duplicated_rows_hold_k_minus_one_duplicates():
    rows = R.load_rows("B", 0)
    for k in (2, 3):
        g, p, n, _m = R.duplicated(rows, k)
        loci, times = np.unique(g[p + n > 0], return_counts=True)
        assert len(g) == R.N_ROWS + 5 * (k - 1) and int((times - 1).sum()) == 5 * (k - 1) and times.max() == k


def test_loader_jobs_differ_by_the_restatements():
    da, ra = R.diff_restated("A")
    db, rb = R.diff_restated("B")
    assert min(ra + rb) > 0 and all(_differs(da.planes[k], db.planes[k]) for k in da.planes)
    ga, ia, ra = R.groups_restated("A")
    gb, ib, rb = R.groups_restated("B")
    assert ia == [0, 1, 0, 1] and ib == [0, 0, 1, 1] and min(ra + rb) > 0
    assert all(_differs(ga.planes[k], gb.planes[k]) for k in ga.planes)
    assert all(_differs(ga.moment[g], gb.moment[g]) and _differs(ga.samples[g], gb.samples[g]) for g in (1, 2))
    assert len(gb.tested(1)) > 20 and ga.tested(1) != gb.tested(1)
    sa, ra = R.samples_restated("A")
    sb, rb = R.samples_restated("B")
    assert (sa.opened, sb.opened) == (3, 2) and min(ra + rb) > 0
    assert all(_differs(sa.level[k], sb.level[k]) for k in range(2)) and sa.level[2].any() and not sb.level[2:].any()
    assert len(sb.sums()) == 9 and len(sa.sums()) == 18 and sa.sums()[:3] != sb.sums()[:3]
    import intervals_ref as I
    start, end = R.load_intervals()
    assert I.interval_sums(sb, start, end, 0).shape == (len(start), 2, 2) and I.interval_sums(sb, start, end, 0).any()
