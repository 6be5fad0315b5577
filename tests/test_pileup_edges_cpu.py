"""CPU pins beneath tests/test_gpu_pileup_edges.py: on the hand-built edge alignments of tests/pileup_cases.py the oracle's
projection equals the reference's own BamMapInfo / 5mc_motif_finder.cpp (tests/golden/align_edges.json, made by
tools/make_golden.py from oracle/_ref/ref_align), and on the foreign MM/ML dialects the oracle's parser, the host mirror and
the CLI's parser list the same entries as the reference's parser core (tests/golden/modparse_edges.json)."""
import json
import os
import subprocess

import numpy as np
import pytest

import bamutil
import pileup_cases as C
from conftest import GOLDEN, ROOT

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")


@pytest.fixture(scope="module")
def P():
    from oracle import pileup_oracle
    return pileup_oracle


@pytest.fixture(scope="module")
def edges():
    return json.load(open(os.path.join(GOLDEN, "align_edges.json")))


def test_oracle_matches_reference_on_edge_alignments(P, edges):
    """the assertions of test_alignment_matches_reference, on the records the case builder makes today (so a change of the
    builder without a new fixture fails here, not on the GPU)"""
    genome = [tuple(x) for x in edges["genome"]]
    assert genome == C.genome()
    reads = C.fixture_reads()
    assert [(r.name, r.flag, r.tid, r.pos, r.cigar_string(), r.seq) for r in reads] == \
        [(x["name"], x["flag"], x["tid"], x["pos"], x["cigar"], x["seq"]) for x in edges["reads"]]
    ops, n_samples = set(), 0
    for r in edges["reads"]:
        d = r["ref"]
        assert d is not None
        ops |= {c for c in r["cigar"] if not c.isdigit()}
        a = P.map_info(r["flag"], r["pos"], P.parse_cigar(r["cigar"]), r["seq"], genome[r["tid"]][1])
        for k in ("qas", "sas", "qpos", "spos", "qb", "qe", "sb", "se", "as_size", "qdir"):
            assert a[k] == d[k], (k, r["name"])
        assert a["pi"] == d["pi"], r["name"]                # same double arithmetic: 100.0 * n / as_size
        L = len(r["seq"])
        assert P.chh_mapped_samples(a, L) == [tuple(x) for x in d["chh"]], r["name"]
        assert [s for _, s in P.cpg_records(a, L)] == [x[1] for x in d["cpg"]], r["name"]
        if a["qdir"] == 0:
            assert P.cpg_records(a, L) == [tuple(x) for x in d["cpg"]], r["name"]
            stored = r["seq"]
            assert sorted(P.chg_records(a, L)) == sorted(tuple(x) for x in d["chg"] if stored[x[0]] == "C"), r["name"]
        n_samples += len(d["cpg"]) + len(d["chg"]) + len(d["chh"])
    assert ops == set("MIDNSHP=X") and len(edges["reads"]) >= 100 and n_samples > 300
    names = {r["name"] for r in edges["reads"]}
    assert {"zoo_H_then_S_f", "zoo_all_S_r", "zoo_all_I_f", "zoo_zero_ops_r", "bnd_tail1_2r", "bnd_head1_1f", "bnd_tailclip0_r", "bnd_tail_D2_f"} <= names
    assert not names & set(C.REF_UNDEFINED)


def test_reference_build_reproduces_the_edge_fixture(P, edges, tmp_path):
    if not P.ref_align_available():
        pytest.skip("oracle/_ref/ref_align not built (reference absent)")
    genome = [tuple(x) for x in edges["genome"]]
    fa = str(tmp_path / "g.fa")
    bamutil.write_fasta(fa, genome)
    out = P.ref_align(fa, [(r["flag"], r["tid"], r["pos"], r["cigar"], r["seq"]) for r in edges["reads"]])
    assert len(out) == len(edges["reads"])
    for r, d in zip(edges["reads"], out):
        want = dict(r["ref"])
        for k in ("cpg", "chg", "chh"):
            want[k] = [tuple(x) for x in want[k]]
        assert d == want, r["name"]
    # and, beyond the recorded sample, every read of every class (whole chromosomes included) against the oracle
    reads = [r for r in C.everything() if r.name not in C.REF_UNDEFINED]
    out = P.ref_align(fa, [(r.flag, r.tid, r.pos, r.cigar_string(), r.seq) for r in reads])
    assert len(out) == len(reads) > 600
    for r, d in zip(reads, out):
        a = P.map_info(r.flag, r.pos, r.cigar, r.seq, genome[r.tid][1])
        assert all(a[k] == d[k] for k in ("qas", "sas", "qpos", "spos", "qb", "qe", "sb", "se", "as_size", "qdir", "pi")), r.name
        assert P.chh_mapped_samples(a, len(r.seq)) == d["chh"] and [s for _, s in P.cpg_records(a, len(r.seq))] == [x[1] for x in d["cpg"]], r.name


def _tuples(mods):
    return [(int(m["qoff"]), int(m["strand"]), m["unmod_base"].decode(), m["code"].decode(), int(m["prob"])) for m in mods]


def test_mm_dialect_parsers_agree(P, tmp_path):
    """foreign_tags(): the oracle's parse_mods, the host mirror and the CLI's `modlist` list the same entries in the same
    order; where the reference's parser core accepts the list (all but ChEBI codes and N+m / N+h) they are its entries."""
    from hifimeth_amd.pileup import parse_mods
    from hifimeth_amd.synth import read_from_ascii
    reads = C.foreign_tags()
    gold = {r["name"]: r for r in json.load(open(os.path.join(GOLDEN, "modparse_edges.json")))["records"]}
    assert set(gold) == {r.name for r in C.fixture_tag_reads()}
    refused = sorted(n for n, r in gold.items() if r["mods"] is None)
    assert refused and all(n.endswith(("_chebi", "_N_m", "_N_h")) for n in refused)
    want, n_ref = [], 0
    for r in reads:
        g = gold.get(r.name)
        w = [tuple(m) for m in P.parse_mods(P.fwd_rev(r.seq, r.flag)[0], r.mm, r.ml)]
        if g is not None:
            assert (g["flag"], g["seq"], g["mm"], g["ml"]) == (r.flag, r.seq, r.mm, [int(v) for v in r.ml]), r.name
        if g is not None and g["mods"] is not None:
            assert w == [tuple(m) for m in g["mods"]], r.name
            n_ref += len(w)
        assert _tuples(parse_mods(r.seq, r.flag, r.mm, r.ml)) == w, r.name
        want.append(w)
    assert n_ref > 300 and {c for w in want for _q, _s, _b, c, _p in w} >= {"m", "h", "a", "n"}
    src = str(tmp_path / "mods.bam")
    plain = [read_from_ascii(r.seq.encode(), *([np.zeros(len(r.seq), np.uint8)] * 4), flag=r.flag, name=r.name) for r in reads]
    bamutil.reads_to_bam(src, plain, extra_aux=lambda i, rd: bamutil.aux_Z("MM", reads[i].mm) + bamutil.aux_B("ML", np.asarray(reads[i].ml, np.uint8)))
    out = subprocess.run([CLI, "modlist", src], capture_output=True, text=True, check=True).stdout.split("\n")
    li = 0
    for r, w in zip(reads, want):
        n = int(out[li]); li += 1
        got = []
        for _ in range(n):
            q, st, ub, code, pr = out[li].split(); li += 1
            got.append((int(q), int(st), ub, code, int(pr)))
        assert got == w, r.name
