"""The derivation of tests/members_cases.py without a GPU: fed the member sets of the textbook restatements on the batch of the GPU
test, it returns what tests/patterns_ref.py, tests/bedmethyl_ref.py and tests/linkage_ref.py return, with and without the
filters; and the batch holds the conditions it is built for."""
import bedmethyl_ref as BR
import linkage_ref as LR
import members_cases as C
import patterns_ref as PR


def _members(min_mapq=0, min_pi=0.0):
    g = C.genome()
    off = C.offsets(g)
    return [(hp, {int(off[sid]) + soff: int(p) for (sid, soff), p in PR.member_loci(C.as_dict(r), g, min_mapq, min_pi).items()})
            for hp, r in zip(C.HPS, C.reads())]


def test_batch_holds_its_cases():
    g, reads = C.genome(), C.reads()
    cpg, sid = C.reference_cpgs(g)
    nA = len(g[0][1])
    assert [int(x) for x in cpg] == list(C.A_CPGS) + [nA + x for x in C.B_CPGS] and list(sid) == [0] * len(C.A_CPGS) + [1] * len(C.B_CPGS)
    assert [len(s) for _n, s in g] == [3300, 2800] and PR.reference_cpgs(g) == [list(C.A_CPGS), list(C.B_CPGS)]
    cols = [sum(n for op, n in r.cigar if op in "M=X") for r in reads]
    assert cols == [1600, 1250, 900, 800] and sum(cols[:3]) + 345 == 4095 and reads[3].pos + 345 == 1445      # the block edge splits a CpG
    assert reads[0].pos == 0 and reads[0].flag == 0 and reads[1].flag == 16 and [op for op, _n in reads[1].cigar] == list("SMIMDMNMS")
    cls = [BR.classes(C.as_dict(r), g) for r in reads]
    member = lambda c, s, x: isinstance(c.get((s, x)), tuple)
    assert all(member(cls[0], 0, x) for x in (1010, 1018, 1023, 1030, 1040)) and cls[0][(0, 600)] == "nocall"
    assert cls[1][(0, 1899)] == "diff" and cls[1][(0, 2050)] == "delete" and cls[1][(0, 2251)] == "diff" and member(cls[1], 0, 2262)
    assert cls[1][(0, 2961)] == "end" and member(cls[1], 0, 2056) and member(cls[1], 0, 1750)
    assert cls[2][(1, 999)] == "end" and member(cls[2], 1, 150) and member(cls[2], 1, 152)
    assert cls[3][(1, 1150)] == "diff" and cls[3][(1, 1260)] == "diff" and member(cls[3], 1, 1440) and member(cls[3], 1, 1445)
    probs = [p for _hp, m in _members() for p in m.values()]
    assert min(probs) < C.THR - 1 and max(probs) > C.THR and C.THR in probs and C.THR - 1 in probs
    took = [BR.takes_part(C.as_dict(r), g, *C.FILTERS) for r in reads]
    by_q = [BR.takes_part(C.as_dict(r), g, C.FILTERS[0], 0.0) for r in reads]
    by_f = [BR.takes_part(C.as_dict(r), g, 0, C.FILTERS[1]) for r in reads]
    assert took == [True, True, False, False] and by_q == [True, True, False, True] and by_f == [True, True, True, False]
    assert [bool(m) for _hp, m in _members(*C.FILTERS)] == took and all(m for _hp, m in _members())


def _check(min_mapq, min_pi):
    g = C.genome()
    recs = [C.as_dict(r) for r in C.reads()]
    bed, pat, link = C.derive(_members(min_mapq, min_pi), g)
    kw = dict(min_mapq=min_mapq, min_pi=min_pi)
    want = PR.rows(recs, g, C.K, thr=C.THR, min_reads=1, **kw)
    assert pat == {start: list(cnt[:4]) for start, _end, cnt, _n, _k in want} and len(want) >= 8
    for s in (0, 1, 2):
        want = BR.rows(recs, g, thr=C.THR, min_valid=1, part=s, hps=list(C.HPS), **kw)
        assert bed[s] == {row[0]: (row[1], row[2]) for row in want} and (want or (s == 2 and min_mapq))
    want = LR.rows(recs, g, C.MAX_DIST, thr=C.THR, min_pairs=1, **kw)
    assert link == {row[0]: list(row[1:]) for row in want} and len(want) >= 8
    return bed, pat, link


def test_derivation_returns_the_restatements():
    bed, pat, link = _check(0, 0.0)
    assert 2 in link and any(c[1] for c in link.values()) and any(c[2] for c in link.values())      # d = 2 (150 | 152), UM and MU occur
    assert all(any(c[b] for c in pat.values()) for b in range(4)) and 3300 + 1440 in pat            # the window across the block edge
    assert bed[0][1023] == (1, 0) and bed[0][1030] == (0, 1) and 1023 not in bed[1] and bed[2][3300 + 152] == (1, 0)


def test_derivation_under_the_filters():
    bed, pat, link = _check(*C.FILTERS)
    assert not bed[2] and all(g < 3300 for g in bed[0]) and all(g < 3300 for g in pat)
    assert (bed, pat, link) != _check(0, 0.0)
