"""CPU pins beneath tests/test_gpu_scan_edges.py: the case builders of tests/scan_cases.py hold what they are for (their own
assertions run here, without a GPU), the site lists written out from the construction of boundary_motifs() are the oracle's,
and the reference's own scanner (tests/golden/scan_edges.json, made by tools/make_golden.py from oracle/_ref/ref_scan) lists
the same sites as both."""
import json
import os

import numpy as np
import pytest

import scan_cases as S
from conftest import GOLDEN


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "scan_edges.json")))


def test_every_builder_holds_its_class():
    reads, expected, boundary = S.boundary_motifs()
    assert len(reads) == len(expected) == len(boundary) == 320 and set(boundary) == set(S.BOUNDARIES)
    assert {r.flag for r in reads} == {4, 16} and all(r.l_qseq == 3100 for r in reads)
    tails = S.tail_lengths()
    assert sorted(r.l_qseq for r in tails) == sorted(S.TAIL_LENGTHS) and len(S.TAIL_LENGTHS) == 24
    assert {(a.l_qseq % 4, b.l_qseq % 4) for a, b in zip(tails, tails[1:])} >= {(a, b) for a in range(4) for b in range(4) if a != b}
    wide = S.mixed_widths()
    assert len({tuple(a.dtype.itemsize for a in (r.fi, r.fp, r.ri, r.rp)) for r in wide}) == 16 and len(wide) == 32
    assert [S.scan_partition(n) for n in S.MANY_CHUNKS] == [(1, 1), (1, 0), (2, 511), (2, 0), (3, 341), (4, 255)]
    for n in S.MANY_CHUNKS:
        reads = S.many_chunks(n)
        assert sum(-(-r.l_qseq // S.CHUNK) for r in reads) == n and reads[-1].l_qseq == S.CHUNK
        assert sum(r.l_qseq > S.CHUNK for r in reads) == 1
    lists, order = S.expected_sites(S.many_chunks(3075))
    assert 300_000 < len(order[0]) <= 1_500_000 and sum(len(x[0]) for x in lists) == len(order[0])
    bare = S.site_free_reads(1025)
    assert len(bare) == 1025 and len(S.expected_sites(bare[:50])[1][0]) == 0


def test_literal_boundary_lists_are_the_oracles(oracle):
    reads, expected, _boundary = S.boundary_motifs()
    n = 0
    for rd, want in zip(reads, expected):
        fwd = oracle.decode(rd)
        for c in range(3):
            assert sorted(oracle.scan(fwd, c).tolist()) == [q for k, q, _ in want if k == c], (rd.name, c)
        for _k, q, s in want:
            assert oracle.window(rd, fwd, q)[1] == s, (rd.name, q)     # FWD = 0, REV = 1: the strand the window is built for
        n += len(want)
    assert n == 2 * 9 * len(S.BOUNDARIES)      # eight motifs per boundary, one of them (CCG) two sites; forward and flag 16
    # the order of the calls, built from the literal lists: forward-strand sites by qoff, then the reverse-strand ones
    _lists, (o_r, o_s, o_q, o_c) = S.expected_sites(reads)
    lit = [(i, s, q, k) for i, want in enumerate(expected) for k, q, s in sorted(want, key=lambda t: (t[2], t[1]))]
    assert lit == list(zip(o_r.tolist(), o_s.tolist(), o_q.tolist(), o_c.tolist()))


def test_reference_scanner_lists_the_same_sites(oracle, golden):
    """tests/golden/scan_edges.json holds the records the builders make today, and the reference's lists on them are the
    oracle's and, for the boundary reads, the literal ones"""
    assert [(r["name"], r["flag"], r["seq"]) for r in golden] == S.golden_records()
    reads, literal = S.golden_reads()
    by_name = {rd.name: rd for rd in reads}
    n_lit = 0
    for r in golden:
        fwd = oracle.decode(by_name[r["name"]])
        for c, key in enumerate(("cpg", "chg", "chh")):
            assert r[key] == oracle.scan(fwd, c).tolist(), (r["name"], key)      # emission order included
            if r["name"] in literal:
                assert sorted(r[key]) == [q for k, q, _ in literal[r["name"]] if k == c], (r["name"], key)
        n_lit += r["name"] in literal
    assert n_lit == 32 * len(S.GOLDEN_BOUNDARIES) and len(golden) == n_lit + len(S.TAIL_LENGTHS)
    assert np.sum([len(r["cpg"]) + len(r["chg"]) + len(r["chh"]) for r in golden]) > 5000
