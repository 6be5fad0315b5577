"""The four consumers of "a CpG member" on the device agree: on the batch of tests/members_cases.py in ONE engine with partitions,
-E 2, -M and -L 64, what numpy derives from the motif-0 records of hm_pileup_fetch_records (grouped by `order`) and the reference
text equals n_mod / n_canon of hm_pileup_fetch_bedmethyl per set, the counts of hm_pileup_fetch_patterns and the rows of
hm_pileup_fetch_linkage; without filters and with a -q / -f that drop one record each; and every fetch is byte for byte the one of
an engine with that option alone.  test_pileup_members_cpu.py checks the derivation against the textbook restatements."""
import numpy as np
import pytest

import members_cases as C
import patterns_ref as PR

pytestmark = pytest.mark.gpu
_RUNS = {}


def _engine(min_mapq, min_pi, **opts):
    from hifimeth_amd.pileup import MethylationPileup
    pu = MethylationPileup(C.genome(), min_mapq=min_mapq, min_pi=min_pi, **opts)
    for hp, r in zip(C.HPS, C.reads()):                          # `order` = the index in reads()
        assert (r.hp or 0) == hp and pu.add(r) == 1
    pu.flush()                                                   # one batch: 4550 columns, five 1024-column tiles, two 4096 blocks
    g, p, m, o = pu.records()
    at = np.lexsort((m, g, o))                                   # the append order is not fixed
    recs = np.rec.fromarrays([o[at], g[at], m[at], p[at]], names="order,gpos,motif,prob")
    pu.count([C.THR, 128, 128])
    out = dict(recs=recs)
    if opts.get("patterns"):
        out["patterns"] = pu.patterns(min_reads=1)
    if opts.get("bedmethyl"):
        out["bedmethyl"] = [pu.bedmethyl(min_valid=1, partition=s) for s in ((0, 1, 2) if opts.get("partitions") else (0,))]
    if opts.get("linkage"):
        out["linkage"] = pu.linkage(min_pairs=1)
    pu.close()
    return out


def _run(filters):
    """the engine with everything on, and the engines with one option each, once per filter setting"""
    if filters not in _RUNS:
        _RUNS[filters] = dict(all=_engine(*filters, partitions=True, patterns=C.K, bedmethyl=True, linkage=C.MAX_DIST),
                              partitions=_engine(*filters, partitions=True), patterns=_engine(*filters, patterns=C.K),
                              bedmethyl=_engine(*filters, bedmethyl=True), linkage=_engine(*filters, linkage=C.MAX_DIST))
    return _RUNS[filters]


def _members(recs):
    cpg = recs[recs["motif"] == 0]
    return [(hp, {int(g): int(p) for g, p in zip(cpg["gpos"][cpg["order"] == i], cpg["prob"][cpg["order"] == i])})
            for i, hp in enumerate(C.HPS)]


@pytest.mark.parametrize("filters", [(0, 0.0), C.FILTERS], ids=["plain", "q_and_f"])
def test_the_four_consumers_agree(filters):
    from hifimeth_amd.pileup import PATTERN_SPAN
    got = _run(filters)["all"]
    members = _members(got["recs"])
    chrs, off = C.genome(), C.offsets(C.genome())
    for (_hp, mem), r in zip(members, C.reads()):                # the records' members are the restatement's
        assert mem == {int(off[sid]) + soff: p for (sid, soff), p in PR.member_loci(C.as_dict(r), chrs, *filters).items()}
    took = [bool(m) for _hp, m in members]
    assert took == ([True, True, False, False] if filters == C.FILTERS else [True] * 4)
    assert set(got["recs"]["order"]) == {i for i, t in enumerate(took) if t}                          # every motif of a dropped record
    bed, pat, link = C.derive(members, chrs, span=PATTERN_SPAN)
    rows = got["patterns"]
    cpg, _sid = C.reference_cpgs(chrs)
    assert {int(w["start"]): [int(x) for x in w["counts"][:4]] for w in rows} == pat and len(rows) == len(pat) >= 5
    assert not rows["counts"][:, 4:].any() and (rows["k"] == C.K).all() and (rows["n"] == rows["counts"].sum(axis=1)).all()
    assert (rows["end"] == cpg[np.searchsorted(cpg, rows["start"]) + 1] + 2).all()
    for s in (0, 1, 2):
        rows = got["bedmethyl"][s]
        assert {int(w["gpos"]): (int(w["n_mod"]), int(w["n_canon"])) for w in rows} == bed[s] and len(rows) == len(bed[s])
    assert bed[1] and (bed[2] or filters == C.FILTERS) and len(bed[0]) >= 15
    rows = got["linkage"]
    assert {int(w["dist"]): [int(w[k]) for k in ("n_uu", "n_um", "n_mu", "n_mm")] for w in rows} == link and len(rows) == len(link) >= 5
    if filters == C.FILTERS:                                     # the dropped records are in none of the four outputs
        plain = _run((0, 0.0))["all"]
        nA = len(chrs[0][1])
        assert (got["recs"]["gpos"] < nA).all() and (plain["recs"]["gpos"] >= nA).any()
        for name, field in (("patterns", "start"), ("linkage", None)):
            assert got[name].tobytes() != plain[name].tobytes()
            assert field is None or ((got[name][field] < nA).all() and (plain[name][field] >= nA).any())
        for s in (0, 1, 2):
            assert (got["bedmethyl"][s]["gpos"] < nA).all() and (plain["bedmethyl"][s]["gpos"] >= nA).any()
        assert len(got["bedmethyl"][2]) == 0


@pytest.mark.parametrize("filters", [(0, 0.0), C.FILTERS], ids=["plain", "q_and_f"])
def test_each_fetch_equals_the_engine_with_that_option_alone(filters):
    runs = _run(filters)
    both = runs["all"]
    assert len(both["recs"]) > 100
    for name in ("partitions", "patterns", "bedmethyl", "linkage"):
        assert runs[name]["recs"].tobytes() == both["recs"].tobytes(), name
    assert both["patterns"].tobytes() == runs["patterns"]["patterns"].tobytes() and len(both["patterns"])
    assert both["bedmethyl"][0].tobytes() == runs["bedmethyl"]["bedmethyl"][0].tobytes() and len(both["bedmethyl"][0])
    assert both["linkage"].tobytes() == runs["linkage"]["linkage"].tobytes() and len(both["linkage"])
