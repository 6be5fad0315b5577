"""The inputs and the catalogue of tests/sequence_cases.py, without a GPU: the catalogue covers every read-only export the header
declares (a fetch added later without an entry fails here), and the inputs are not degenerate -- by the CPU restatements alone."""
import os
import re

import numpy as np
import pytest

import bedmethyl_ref as BR
import groups_ref as G
import linkage_ref as LR
import patterns_ref as PR
import pileup_cases as C
import readpos_ref as RR
import sequence_cases as S
from conftest import ROOT
from oracle import pileup_oracle as P

HEADER = os.path.join(ROOT, "include", "hifimeth_hip.h")


def _declared():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return set(re.findall(r"\b(hm_(?:pileup|group|asm|sites|domain)_\w+)\s*\(", text))


def test_exports_table_is_the_header():
    declared = _declared()
    assert len(declared) > 40 and declared == set(S.EXPORTS), (sorted(declared - set(S.EXPORTS)), sorted(set(S.EXPORTS) - declared))
    assert set(S.EXPORTS.values()) == {"reader", "mutator", "lifecycle", "host"}


def test_every_reader_has_a_catalogue_entry():
    names = [n for n, _f in S.CATALOGUE] + [n for n, _f in S.LOAD_CATALOGUE if n not in dict(S.CATALOGUE)]
    assert len(names) == len(set(names)) and set(names) == set(S.CALLS)
    called = {e for n in names for e in S.CALLS[n]}
    assert called <= set(S.EXPORTS) and all(S.EXPORTS[e] == "reader" for e in called), called
    missing = {e for e, cls in S.EXPORTS.items() if cls == "reader"} - called
    assert not missing, missing
    for what in S.ROW_FETCHES:                                # every row fetch also only counted and with a short cap
        assert {"count_only_" + what, "cap_short_" + what} <= set(dict(S.CATALOGUE))
    assert {"count_only_groups", "cap_short_groups"} <= set(dict(S.LOAD_CATALOGUE))


@pytest.mark.parametrize("which", [0, 1])
def test_record_input_is_not_degenerate(which):
    g, reads = S.record_input(which)
    assert len(g) == 3 and 5000 <= sum(len(s) for _n, s in g) <= 6500 and len(reads) == 60
    assert {r.flag & 16 for r in reads} == {0, 16} and {r.hp for r in reads} == {0, 1, 2}
    assert all({"I", "D"} <= {op for op, _n in r.cigar} for r in reads) and any(r.cigar[0][0] == "S" for r in reads) and any(r.cigar[-1][0] == "S" for r in reads)
    cut = [S.trimmed(r) for r in reads]
    assert all(len(t.ml) < len(r.ml) for t, r in zip(cut, reads))                                   # the trim drops entries of every read
    assert all(len(RR.entries(C.as_dict(t))) == len(RR.trim_entries(RR.entries(C.as_dict(r)), len(r.seq), *S.TRIM)) for t, r in zip(cut, reads))
    dicts = [C.as_dict(t) for t in cut]
    for slab in S.slabs(cut):                                 # every slab projects records and has a histogram to take medians of
        got = P.pileup([C.as_dict(t) for t in slab], g)
        assert len(slab) == 20 and len(got["records"]) > 500 and all(got["bins"][c].sum() > 100 for c in range(3))
        assert all(1 <= t <= 255 for t in S.median_thresholds(got["bins"]))
    whole = P.pileup(dicts, g)
    assert {m for *_x, m in whole["loci"]} == {0, 1, 2}                                             # all three motifs have loci
    thr = S.median_thresholds(whole["bins"])
    parts = [{(sid, soff): (p, n) for sid, soff, p, n, _m in P.pileup([d for d, r in zip(dicts, reads) if r.hp == hp], g, thresholds=thr)["loci"]}
             for hp in (1, 2)]
    assert len(parts[0]) > 500 and len(parts[1]) > 500                                              # both partitions are populated
    tested = [k for k in parts[0] if k in parts[1] and sum(parts[0][k]) >= S.ASM_MIN_COV and sum(parts[1][k]) >= S.ASM_MIN_COV]
    assert len(tested) > 50
    k, span = S.RECORD_OPTIONS["patterns"], 150
    assert len(PR.rows(dicts, g, k, span, thr[0], min_reads=2)) > 20                               # -E windows
    hps = [r.hp for r in reads]
    assert all(len(BR.rows(dicts, g, thr[0], 1, part, hps)) > 20 for part in (0, 1, 2))             # -M rows of every set
    assert len(LR.rows(dicts, g, S.RECORD_OPTIONS["linkage"], thr[0])) > 20                         # -L distances
    ends = {(m, e) for m, e, _d, n_m, n_u, _s in RR.rows(dicts, g, S.RECORD_OPTIONS["profile"], thr) if n_m + n_u}
    assert ends == {(m, e) for m in range(3) for e in range(3)}                                     # -P rows at both ends and inside


def test_the_two_record_inputs_differ():
    (g0, r0), (g1, r1) = S.record_input(0), S.record_input(1)
    assert [len(s) for _n, s in g0] != [len(s) for _n, s in g1] and [r.pos for r in r0] != [r.pos for r in r1]


def test_load_input_is_not_degenerate():
    assert sorted(G.dataset()) == [(g, s) for g in (1, 2) for s in range(3)]
    ref = G.dataset_loader()
    assert len(ref.tested(1)) > len(ref.tested(2)) > len(ref.tested(3)) > 20
    assert [len(s) for _n, s in S.load_genome()] == list(G.LENGTHS)


def test_ladder_rows_triple_per_step():
    planes = S.ladder_planes()
    assert all(len(x) == S.LADDER_N and x.dtype == np.int32 for x in planes)
    for (a, b), (c, d) in zip(S.LADDER[:-1], S.LADDER[1:]):
        assert c <= a and b <= d                                                                    # nested
    for kind in ("loci", "asm", "domains"):
        n = [S.ladder_rows(kind, lo, hi, planes) for lo, hi in S.LADDER]
        assert n[0] == 1 and all(y >= 3 * x for x, y in zip(n[:-1], n[1:])), (kind, n)
    assert S.ladder_rows("loci", *S.LADDER[-1], planes) == S.LADDER_N
    # hits of both signs and both domain states occur: the regions and the segments are more than one
    pc, nc, _key, p1, n1, p2, n2 = planes
    assert {int(x) for x in np.sign(p1 * (p2 + n2) - p2 * (p1 + n1))} == {-1, 1} and len({(int(a), int(b)) for a, b in zip(pc, nc)}) == 2
