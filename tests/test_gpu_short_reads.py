"""The CNN kernels on reads shorter than the window (401) and than a trunk tile (112): the read sets of tests/short_cases.py through
every kernel path, values compared.  Runs on the GPU box only:  python -m pytest tests/test_gpu_short_reads.py -m gpu -q -s

Every other value test stages reads of 1000 bases and more; test_gpu_scan_edges.py sends reads down to one base through the engine
but compares site lists, order and windows only.  What a short read changes: most steps of the sliding-window trunk are constant
steps, kept rows pass constant -> computed -> constant within one read and reach the next read within four tiles, a site's left and
right edge chains lie in or next to constant tiles, conv1's padded row holds fewer real rows than taps, a site is a left-edge and a
right-edge case at once, the strip tail's marks are sized by rows (480 per base here) while its sites are sized by bases, and small
groups hold no site of a context.  A wrong constant row, a kept row leaked from the neighbouring read or a list entry one tile off
is a gross error: the bar is test_gpu_logits.py's, unchanged -- per context and stratum
    e = max_k |l_k - l64_k| / (1 + max_k |l64_k|) <= 8 x max(E_oracle, 1e-6)
against fp64 logits of the oracle's windows (tests/cnn64.py), with the stratum "both" (the window hangs over both ends of the read)
next to start / middle / end.  tests/test_short_cases_cpu.py shows on the CPU that this bar rejects a zero row outside the read
(> 60 000 x the bar in every stratum that has such rows).

Measured on an MI355X, worst E_gpu / E_oracle over all configurations (CpG / CHG / CHH): ladder 1.69 / 1.22 / 1.63, crowd
1.18 / 0.76 / 1.23, sandwich 1.89 / 1.56 / 2.15; the bar is 8."""
import os
import subprocess

import numpy as np
import pytest

import bamutil
import short_cases as S
from cnn64 import ALL_STRATA, CNN64, reference_sites, site_errors, strata
from conftest import ROOT, WEIGHTS
from scan_cases import expected_sites
from test_gpu_logits import CONFIGS, NAMES, _check, _engine, _errors, _stage
from test_gpu_parity import DP_TOL, _run

pytestmark = pytest.mark.gpu

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
SHORT = {"min_read_size": 1}

CROWD_CONFIGS = {
    "trunk1": CONFIGS["trunk1"],
    "p0-trunk1": CONFIGS["p0-trunk1"],
    "p1-trunk0": CONFIGS["p1-trunk0"],
    "trunk3-cu1-g8192": {"trunk": 1, "trunk_impl": 3, "num_cu": 1, "group_bases": 8192},
    "trunk3-cu7-g8192": {"trunk": 1, "trunk_impl": 3, "num_cu": 7, "group_bases": 8192},
    "trunk3-cu1024-g8192": {"trunk": 1, "trunk_impl": 3, "num_cu": 1024, "group_bases": 8192},
    "one-read-per-group": {"trunk": 1, "group_bases": 1},
}
VARIANTS = [("trunk_impl", v) for v in (0, 1, 2, 3)] + [("edge_impl", v) for v in (0, 1)] + [("tail_impl", v) for v in (0, 1, 2, 3)]

_REF, _BYTES = {}, {}


def _ref(name, oracle, oracle_models):
    """(reads, sites, strata names) of a short read set: fp64 and fp32-oracle logits of its sites, computed once per module.  The names
    are the strata the set populates in every context (CHH: on both strands): those short_cases.REQUIRED_STRATA asks for at least, and
    together they hold every site."""
    if name not in _REF:
        reads = S.SETS[name]()
        f64 = [CNN64(os.path.join(WEIGHTS, n + ".hmw")) for n in NAMES]
        # the sandwich holds every read twice: the reference of a read is computed once and stands at both places
        first, uniq, distinct = {}, [], []
        for r in reads:
            if id(r) not in first:
                first[id(r)] = len(distinct)
                distinct.append(r)
            uniq.append(first[id(r)])
        once = reference_sites(oracle, distinct, {"o32": oracle_models, "f64": f64}, min_len=1)
        sites = []
        for s in once:
            cut = np.searchsorted(s["rid"], np.arange(len(distinct) + 1))
            idx = np.concatenate([np.arange(cut[u], cut[u + 1]) for u in uniq])
            d = {k: v[idx] for k, v in s.items()}
            d["rid"] = np.concatenate([np.full(cut[u + 1] - cut[u], i, np.int32) for i, u in enumerate(uniq)])
            sites.append(d)
        names =tuple(n for n in ALL_STRATA if all(m.any() for c in range(3) for m in strata(sites[c], c, (n,)).values()))
        assert set(S.REQUIRED_STRATA[name]) <= set(names), (name, names)
        for c, s in enumerate(sites):
            s["e_oracle"] = float(site_errors(s["o32"], s["f64"]).max(initial=0.0))
            assert sum(int(m.sum()) for m in strata(s, c, names).values()) == len(s["qoff"]) > 0, (name, NAMES[c])
        _REF[name] = (reads, sites, names)
    return _REF[name]


def _short_engine(opts, **kw):
    return _engine({**SHORT, **opts, **kw})


def _reference_bytes(name, reads):
    """(calls, logits) of `reads` on the streaming trunk (trunk_impl 1: every position computed), once per module"""
    if name not in _BYTES:
        m = _short_engine({"trunk": 1, "trunk_impl": 1})
        try:
            calls, logits = _run(m, reads)
        finally:
            m.close()
        assert len(calls) > 1000 and len(logits) == 8 * len(calls)
        _BYTES[name] = (calls.tobytes(), logits)
    return _BYTES[name]


# ---- logits against fp64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(CONFIGS))
@pytest.mark.parametrize("set_name", ["ladder", "sandwich"])
def test_short_read_logits_within_the_bar(oracle, oracle_models, set_name, cfg):
    reads, sites, names = _ref(set_name, oracle, oracle_models)
    m = _short_engine(CONFIGS[cfg])
    try:
        _stage(m, reads)
        _check(set_name, cfg, sites, _errors(m, reads, sites, names=names))
    finally:
        m.close()


@pytest.mark.parametrize("cfg", list(CROWD_CONFIGS))
def test_crowd_logits_within_the_bar(oracle, oracle_models, cfg):
    """1500 reads of 1 .. 64 bases: equal-cost runs of dozens of reads that start on any of a tiny read's four tile kinds (one
    workgroup, seven, more workgroups than tiles), ~90 groups of which some hold no CpG / CHG site, and one read per group"""
    reads, sites, names = _ref("crowd", oracle, oracle_models)
    assert names == ("both",)
    m = _short_engine(CROWD_CONFIGS[cfg])
    try:
        _stage(m, reads)
        _check("crowd", cfg, sites, _errors(m, reads, sites, names=names))
    finally:
        m.close()


# ---- byte identity between kernel variants ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt,value", VARIANTS)
def test_kernel_variants_are_byte_identical_on_short_reads(opt, value):
    reads = S.ladder() + S.sandwich()
    want = _reference_bytes("ladder+sandwich", reads)
    m = _short_engine({"trunk": 1, opt: value})
    try:
        calls, logits = _run(m, reads)
    finally:
        m.close()
    assert (calls.tobytes(), logits) == want, (opt, value)


@pytest.mark.parametrize("group_bases", [0, 4096, 1])
@pytest.mark.parametrize("num_cu", [1, 5, 256, 1024])
def test_sliding_window_trunk_is_byte_identical_on_the_crowd_whatever_the_runs(num_cu, group_bases):
    reads = S.crowd()
    want = _reference_bytes("crowd", reads)
    m = _short_engine({"trunk": 1, "trunk_impl": 3, "num_cu": num_cu, "group_bases": group_bases})
    try:
        calls, logits = _run(m, reads)
    finally:
        m.close()
    assert (calls.tobytes(), logits) == want, (num_cu, group_bases)


# ---- batch and engine state --------------------------------------------------------------------------------------------------------
def test_batches_of_short_reads_through_one_engine(oracle, oracle_models):
    """crowd -> sandwich -> ladder -> crowd through one engine (buffers sized by the crowd's rows, then by the sandwich's bases): every
    batch within the bar, and its calls and logits the bytes a fresh engine gives for that set alone"""
    cfg = {"trunk": 1, "trunk_impl": 3, "num_cu": 7, "group_bases": 8192}
    fresh = {}
    for name in ("crowd", "sandwich", "ladder"):
        m = _short_engine(cfg)
        try:
            calls, logits = _run(m, S.SETS[name]())
            fresh[name] = (calls.tobytes(), logits)
        finally:
            m.close()
    m = _short_engine(cfg)
    try:
        for name in ("crowd", "sandwich", "ladder", "crowd"):
            reads, sites, names = _ref(name, oracle, oracle_models)
            _stage(m, reads)
            _check(name, "one engine", sites, _errors(m, reads, sites, names=names))
            got = (m.fetch().tobytes(), b"".join(m.site_logits(c).tobytes() for c in range(3)))
            assert got == fresh[name], name
    finally:
        m.close()


# ---- constant steps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_cu", [1, 5, 256])
@pytest.mark.parametrize("set_name", ["ladder", "crowd"])
def test_constant_steps_are_the_plans(set_name, num_cu):
    """hm_trunk3.hip counts the tiles it stored as constant steps: per read and strand view the first tile and the tiles at u0 >= len,
    short_cases.plan() summed -- most of a short read's tiles -- whatever the runs; the calls stay the streaming trunk's bytes"""
    from hifimeth_amd import MethylationCaller
    reads = S.SETS[set_name]()
    want_bytes = _reference_bytes(set_name, reads)
    want = sum(S.plan(r.l_qseq)[1] for r in reads)
    tiles = sum(S.plan(r.l_qseq)[0] for r in reads)
    with MethylationCaller(device=0, min_read_size=1, timing=True) as m:
        m.set_option("trunk", 1)
        m.set_option("trunk_impl", 3)
        m.set_option("num_cu", num_cu)
        calls, logits = _run(m, reads)
        tm = m.timing()
    assert (calls.tobytes(), logits) == want_bytes
    assert min(tm["trunk_launches"]) > 0 and sum(tm["front_launches"]) == 0
    assert list(tm["trunk_const_steps"]) == [want, want, 2 * want], (tm["trunk_const_steps"], want)
    assert [p // 112 for p in tm["trunk_positions"]] == [tiles, tiles, 2 * tiles]
    if set_name == "crowd":
        assert 2 * want > tiles      # more constant tiles than computed ones


# ---- calls -----------------------------------------------------------------------------------------------------------------------------
def _ladder_calls():
    from hifimeth_amd import MethylationCaller
    if "calls" not in _BYTES:
        with MethylationCaller(device=0, min_read_size=1) as m:      # default options but for the minimum length
            _BYTES["calls"] = m.call(S.ladder()).copy()
    return _BYTES["calls"]


def test_calls_of_the_ladder(oracle, oracle_models):
    """p against the fp32 oracle (|dp| <= 1e-4, ML within 1 as in test_gpu_parity._check_calls), the ML byte of the engine's own p, the
    reference's order"""
    reads = S.ladder()
    calls = _ladder_calls()
    _lists, (o_r, o_s, o_q, o_c) = expected_sites(reads)
    assert len(calls) == len(o_r) > 2000
    for f, want in (("read_id", o_r), ("strand", o_s), ("qoff", o_q), ("ctx", o_c)):
        assert np.array_equal(calls[f], want), f
    assert np.isfinite(calls["p"]).all() and (calls["p"] >= 0).all() and (calls["p"] <= 1).all()
    assert (calls["scaled_prob"] == np.minimum(255, (255 * calls["p"]).astype(np.int64))).all()
    # the fp32 oracle's p and ML of the same sites: softmax of the logits the logit tests share (per context in (read, qoff) order)
    _reads, sites, _names = _ref("ladder", oracle, oracle_models)
    worst = 0.0
    for c in range(3):
        got = calls[calls["ctx"] == c]
        got = got[np.lexsort((got["qoff"], got["read_id"]))]
        s = sites[c]
        assert np.array_equal(got["read_id"], s["rid"]) and np.array_equal(got["qoff"], s["qoff"]) and np.array_equal(got["strand"], s["strand"]), c
        p, ml = oracle.softmax(s["o32"])
        worst = max(worst, float(np.abs(got["p"] - p).max()))
        assert np.abs(got["scaled_prob"].astype(int) - ml.astype(int)).max() <= 1, c
    print(f"ladder: {len(calls)} calls, max|dp|={worst:.2e}")
    assert worst <= DP_TOL, worst


def _parse_mm(fwd: bytes, mm: str, ml):
    """MM:Z / ML:B:C -> [(qoff, strand, ml)]: forward calls by qoff, then reverse calls by qoff"""
    seq = np.frombuffer(fwd, np.uint8)
    out, k = [], 0
    for part in mm.rstrip(";").split(";"):
        head, *deltas = part.split(",")
        strand = {"C+m": 0, "G-m": 1}[head]
        cand = np.flatnonzero(seq == ord("G" if strand else "C"))
        i = -1
        for d in deltas:
            i += int(d) + 1
            out.append((int(cand[i]), strand, int(ml[k])))
            k += 1
    assert k == len(ml)
    return out


def test_cli_calls_the_ladder_with_l_1_and_nothing_with_l_1000(tmp_path, oracle):
    reads = S.ladder()
    calls = _ladder_calls()
    src, dst, none = str(tmp_path / "in.bam"), str(tmp_path / "out.bam"), str(tmp_path / "none.bam")
    bamutil.reads_to_bam(src, reads)
    for args in (["-l", "1", src, dst], ["-l", "1000", src, none]):
        subprocess.run([CLI, "call", "-t", "4", *args], check=True, timeout=120, stderr=subprocess.DEVNULL)
    _, recs = bamutil.read_bam(dst)
    assert len(recs) == len(reads)
    n = 0
    for i, (rd, rec) in enumerate(zip(reads, recs)):
        assert rec["name"] == rd.name
        tags = {t[0]: t for t in bamutil.parse_aux(rec["aux"])}
        mine = calls[calls["read_id"] == i]
        if len(mine) == 0:
            assert "MM" not in tags and "ML" not in tags and "MN" not in tags, rd.name
            continue
        got = _parse_mm(oracle.decode(rd), tags["MM"][2], tags["ML"][2])
        assert got == list(zip(mine["qoff"].tolist(), mine["strand"].tolist(), mine["scaled_prob"].tolist())), rd.name
        assert tags["MN"][2] == rd.l_qseq
        n += len(got)
    assert n == len(calls)
    _, recs = bamutil.read_bam(none)
    assert len(recs) == len(reads)
    for rec in recs:
        assert not {"MM", "ML", "MN"} & {t[0] for t in bamutil.parse_aux(rec["aux"])}, rec["name"]


# ---- a read without bases -----------------------------------------------------------------------------------------------------------
def test_a_zero_length_read_is_passed_through():
    """l_qseq = 0 with four empty kinetics arrays and min_read_size 0: check_read (hm_engine.cpp) passes the read through like a read
    under the minimum length -- it has no site, and staged it would own four constant tiles whose feature-row loads clamp to position
    len - 1 = -1.  Pinned: hm_submit_read returns 0, and wherever the read stands in a batch its neighbours' calls and logits are the
    bytes of the batch without it."""
    from hifimeth_amd import MethylationCaller
    a, b = next(r for r in S.ladder() if r.l_qseq == 249), S.sandwich()[0]
    zero = S.zero_length_read()
    assert zero.l_qseq == 0 and zero.has_kinetics() and a.l_qseq > 0 and b.l_qseq > 1000
    with MethylationCaller(device=0, min_read_size=0) as m:
        m.set_option("trunk", 1)
        m.clear()
        assert m.submit(0, a) is True and m.submit(1, zero) is False and m.submit(2, b) is True
        m.upload()
        m.run()
        got = m.fetch().copy()
        got_lg = b"".join(m.site_logits(c).tobytes() for c in range(3))
        m.clear()
        assert m.submit(0, a) and m.submit(2, b)
        m.upload()
        m.run()
        want = m.fetch().copy()
        want_lg = b"".join(m.site_logits(c).tobytes() for c in range(3))
        m.clear()
        assert len(want) > 500 and set(np.unique(want["read_id"]).tolist()) == {0, 2}
        assert got.tobytes() == want.tobytes() and got_lg == want_lg
        for reads in ([zero, a, b], [a, b, zero]):
            calls = m.call(reads, first_id=0 if reads[0] is a else -1)
            assert np.array_equal(np.where(calls["read_id"] == 1, 2, calls["read_id"]), want["read_id"])
            calls["read_id"] = want["read_id"]
            assert calls.tobytes() == want.tobytes()
        assert len(m.call([zero])) == 0 and len(m.call([zero, zero])) == 0
