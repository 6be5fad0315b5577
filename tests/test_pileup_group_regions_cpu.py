"""`groupdmr` without a GPU: the restatement of tests/group_regions_ref.py in its two formulations against each other and against
literal chains, hm_dmr_p_cutoff and stitch_group_regions (both host only) against it, the command's usage and option errors, the
symbols -- and the condition that the random data set of tests/test_gpu_pileup_group_regions.py holds regions at all."""
import os
import subprocess

import numpy as np
import pytest

import group_regions_ref as RR
import groups_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")


def _random_rows(n, seed):
    """n rows in runs: p from a few values around 0.01, diff of either sign around 10, three contexts, gaps of 1 .. 12"""
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, RR.ROW_DTYPE)
    rows["gpos"] = np.cumsum(rng.integers(1, 13, n))
    rows["motif"] = rng.choice([0, 0, 0, 1, 2, 3], n)
    rows["pvalue"] = rng.choice([1e-6, 0.01, np.nextafter(0.01, 1), 0.2, 1.0], n, p=[0.55, 0.1, 0.05, 0.2, 0.1])
    run = np.repeat(rng.choice([-1.0, 1.0], n // 8 + 1), 8)[:n]
    rows["diff"] = run * rng.choice([0.0, 9.5, 10.0, 30.0], n, p=[0.05, 0.1, 0.15, 0.7])
    rows["phi"] = rng.choice([1.0, 1.5, 4.0], n)
    rows["m1"], rows["m2"] = rng.integers(2, 4, n), rng.integers(2, 4, n)
    for f in ("pcov1", "ncov1", "pcov2", "ncov2"):
        rows[f] = rng.integers(1, 60, n)
    return rows


def test_the_crafted_rows_give_the_chains_written_here():
    rows = RR.crafted_rows()
    got, R, hits = RR.regions(rows, 0, 0.01, 10.0, 10, 1)
    assert R == 22 and hits == 18                             # no hits: 50 (p), 131 (under min_diff), 150 (diff 0), 151 (p just above)
    assert [(int(g["start"]), int(g["end"]), int(g["n_loci"]), int(g["sign"]), int(g["flags"])) for g in got] == [
        (3, 6, 2, 1, RR.FIRST), (20, 21, 1, 1, 0), (40, 46, 2, 1, 0), (52, 53, 1, 1, 0), (70, 71, 1, 1, 0), (72, 75, 2, -1, 0), (90, 101, 2, 1, 0),
        (111, 112, 1, 1, 0), (130, 131, 1, 1, 0), (132, 133, 1, -1, 0), (170, 191, 4, -1, RR.LAST)]
    first, last = got[0], got[-1]
    assert (first["m1_min"], first["m2_min"], first["phi_max"], first["pmin"]) == (2, 3, 2.5, 1e-9)
    assert (last["m1_min"], last["m2_min"], last["phi_max"], last["pmin"]) == (2, 2, 3.0, 1e-300)
    assert first["pcov1"] == (7 + 3) + (7 + 0) and first["diff"] == RR.pooled_diff(17, 3 + 0 + 3 + 2, 2 + 3 + 2 + 5, 9 + 1 + 9 + 1)
    assert [int(g["n_loci"]) for g in RR.regions(rows, 0, 0.01, 10.0, 10, 2)[0]] == [2, 2, 2, 2, 4]
    assert [int(g["start"]) for g in RR.regions(rows, 0, 0.01, 10.0, 10, 3, keep_edges=True)[0]] == [3, 170]
    # without min_diff 130 .. 131 link, and 131 | 132 is a sign flip
    assert (130, 132, 2) in [(int(g["start"]), int(g["end"]), int(g["n_loci"])) for g in RR.regions(rows, 0, 0.01, 0.0, 10, 1)[0]]
    chh, R2, hits2 = RR.regions(rows, 2, 0.01, 0.0, 10, 1)
    assert R2 == 4 and hits2 == 4 and [(int(g["start"]), int(g["end"]), int(g["sign"]), float(g["phi_max"])) for g in chh] == [
        (160, 162, 1, 7.0), (162, 163, -1, 1.0), (175, 176, 1, 1.0)]
    assert RR.regions(rows, 1, 0.01, 0.0, 10, 1)[1:] == (1, 1)


def test_the_two_formulations_agree():
    sets = [RR.crafted_rows(), _random_rows(700, 1), _random_rows(700, 2), RR.dataset_rows()]
    n = 0
    for rows in sets:
        for ctx in (0, 1, 2):
            for max_p, min_diff, max_gap, min_loci in ((0.01, 10.0, 10, 1), (0.01, 0.0, 4, 2), (1.0, 0.0, 30, 3), (0.5, 9.5, 1, 1)) + RR.THRESHOLDS:
                for keep in (False, True):
                    a = RR.regions(rows, ctx, max_p, min_diff, max_gap, min_loci, keep)
                    b = RR.regions(rows, ctx, max_p, min_diff, max_gap, min_loci, keep, chains_of=RR.chains_union_find)
                    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
                    n += len(a[0])
    assert n > 1000


def test_host_p_cutoff_equals_the_restatement():
    from hifimeth_amd.caller import HifimethError
    from hifimeth_amd.pileup import GROUP_DTYPE, group_p_cutoff, group_qvalues
    assert GROUP_DTYPE == RR.ROW_DTYPE
    rng = np.random.default_rng(8)
    rows = np.zeros(500, GROUP_DTYPE)
    rows["motif"] = rng.choice([0, 2, 3], 500)                # no CHG row at all
    rows["pvalue"] = rng.choice(np.concatenate([rng.random(40) ** 3, [1.0, G.DBL_MIN, 1e-300]]), 500)      # ties in p
    q, _m = group_qvalues(rows)
    assert q.tobytes() == G.bh(rows["pvalue"], rows["motif"])[0].tobytes()
    seen = set()
    for max_q in (1e-320, 1e-3, 0.01, 0.05, 0.3, 1.0):        # no row under the first, all rows under the last
        got = group_p_cutoff(rows, q, max_q)
        want = RR.p_cutoff(rows["pvalue"], q, rows["motif"], max_q)
        assert got.tobytes() == want.tobytes() and got[1] == 0.0
        for c in (0, 2):                                      # {q <= F} == {p <= cutoff}
            sel = RR.ctx_mask(rows, c)
            assert ((q[sel] <= max_q) == (rows["pvalue"][sel] <= got[c])).all()
        seen.add((got[0] > 0, got[0] == rows["pvalue"][RR.ctx_mask(rows, 0)].max()))
    assert seen == {(False, False), (True, False), (True, True)}
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(HifimethError):
            group_p_cutoff(rows, q, bad)
    rows["pvalue"][3] = 0.0                                   # what hm_group_qvalues refuses
    with pytest.raises(HifimethError):
        group_p_cutoff(rows, q, 0.05)
    assert group_p_cutoff(rows[:0], q[:0], 0.05).tolist() == [0.0, 0.0, 0.0]


def test_chaining_by_q_is_chaining_by_the_cutoff():
    rows = RR.dataset_rows()
    q, _m = G.bh(rows["pvalue"], rows["motif"])
    for max_q in (0.05, 0.3):
        cut = RR.p_cutoff(rows["pvalue"], q, rows["motif"], max_q)
        for ctx in (0, 1, 2):
            by_q = RR.regions(rows, ctx, 1.0, 0.0, 30, 2, q=q, max_q=max_q)
            assert cut[ctx] > 0 and len(by_q[0]) > 0
            by_p = RR.regions(rows, ctx, cut[ctx], 0.0, 30, 2)
            assert by_q[0].tobytes() == by_p[0].tobytes() and by_q[1:] == by_p[1:]


@pytest.mark.parametrize("keep", [False, True])
def test_stitch_equals_the_whole_at_every_split(keep):
    from hifimeth_amd.pileup import GROUP_REGION_DTYPE, stitch_group_regions
    assert GROUP_REGION_DTYPE == RR.REGION_DTYPE and GROUP_REGION_DTYPE.itemsize == 96
    rows = RR.crafted_rows()
    lo, hi = 0, int(rows["gpos"][-1]) + 2
    merged = 0
    for ctx, max_p, min_diff, max_gap, min_loci in ((0, 0.01, 10.0, 10, 1), (0, 0.01, 0.0, 10, 3), (2, 0.01, 0.0, 10, 2)):
        whole = RR.regions(rows, ctx, max_p, min_diff, max_gap, min_loci, keep)
        for m in range(lo, hi + 1):
            for bounds in ([lo, m, hi], [lo, m, min(m + 3, hi), min(m + 40, hi), hi]):
                parts = RR.parts_of(rows, bounds, ctx, max_p, min_diff, max_gap, min_loci)
                got, R = stitch_group_regions(parts, max_gap, min_loci, keep_edges=keep)
                assert got.dtype == GROUP_REGION_DTYPE and got.tobytes() == whole[0].tobytes() and R == whole[1], (ctx, m, bounds)
                merged += sum(len(p[0]) for p in parts) > len(got)
    assert merged > 50                                        # chains were really joined


def test_stitch_of_the_random_rows():
    from hifimeth_amd.pileup import stitch_group_regions
    rows = _random_rows(700, 4)
    hi = int(rows["gpos"][-1]) + 1
    rng = np.random.default_rng(6)
    for _ in range(12):
        bounds = [0] + sorted(rng.integers(0, hi, 5).tolist()) + [hi]
        for keep in (False, True):
            whole = RR.regions(rows, 0, 0.01, 10.0, 8, 2, keep)
            got, R = stitch_group_regions(RR.parts_of(rows, bounds, 0, 0.01, 10.0, 8, 2), 8, 2, keep_edges=keep)
            assert got.tobytes() == whole[0].tobytes() and R == whole[1] and len(got) > 10


def test_the_data_set_holds_regions():
    """not a measurement: the GPU comparison on the random data set cannot pass on empty output.  At the first thresholds of
    RR.THRESHOLDS the restatement alone finds at least 20 regions of >= 3 loci, of both signs, and at least 3 shorter chains."""
    rows = RR.dataset_rows()
    max_p, min_diff, max_gap, min_loci = RR.THRESHOLDS[0]
    assert min_loci == 3
    kept, R, hits = RR.regions(rows, 0, max_p, min_diff, max_gap, min_loci)
    every = RR.regions(rows, 0, max_p, min_diff, max_gap, 1)[0]
    assert len(kept) >= 20 and (kept["n_loci"] >= 3).all()
    assert (kept["sign"] > 0).sum() >= 5 and (kept["sign"] < 0).sum() >= 5
    assert len(every) - len(kept) >= 3 and R > hits > 3 * len(kept)
    for t in RR.THRESHOLDS:
        for ctx in (0, 1, 2):
            assert len(RR.regions(rows, ctx, t[0], t[1], t[2], min(t[3], 2 if ctx else t[3]))[0]) > 0, (t, ctx)
    assert (rows["phi"] > 1).sum() >= 50 and {int(x) for x in rows["m1"]} >= {2, 3}


def test_the_layout_lies_across_a_workgroup_of_the_row_selection():
    kind = RR.layout()
    assert len(kind) == RR.TOTAL
    cpg = [i for i, k in enumerate(kind) if k not in ".UO"]
    first = cpg.index(3000 + RR.LONG_AT)
    assert first < 4096 < first + RR.LONG_N - 1 and all(kind[i] in "Ppq" for i in cpg[first:first + RR.LONG_N])
    assert kind[cpg[first - 1]] == "N" and kind[cpg[first + RR.LONG_N]] == "N"


def test_symbols_header_and_python_names():
    from hifimeth_amd import pileup as P
    from hifimeth_amd._lib import lib
    L = lib()
    assert L.hm_abi_version() == 5
    for name in ("hm_dmr_fetch_regions", "hm_dmr_p_cutoff"):
        assert hasattr(L, name), name
    for name in ("group_regions", "group_regions_bed"):
        assert hasattr(P.MethylationPileup, name), name
    assert callable(P.group_p_cutoff) and callable(P.stitch_group_regions) and callable(P.groupdmr_summary_tsv)
    header = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    assert "} hm_group_region_t;" in header and "int hm_dmr_p_cutoff(" in header


def _run(args):
    return subprocess.run([CLI, *args], capture_output=True, text=True, timeout=60)


def test_usage_of_the_command():
    r = _run(["groupdmr", "-h"])
    assert r.returncode == 0 and "groupdmr [OPTIONS] reference a1,a2,... b1,b2,... output-prefix" in r.stderr
    assert [x.strip() for x in r.stderr.splitlines() if x.startswith("  -")] == [
        "-a <int>", "-r <int>", "-s <p>", "-F <q>", "-m <pct>", "-g <bp>", "-n <int>", "-L", "-t <CPU threads>", "-d <int>"]
    assert "With -G" not in r.stderr and "no region-level" in r.stderr and "descriptive" in r.stderr and "regiondiff -R" in r.stderr
    tail = ["f", "a,b", "c,d", "o"]
    ranges = "-s and -F must be in (0, 1], -m in [0, 100], -g and -n integers >= 1"
    for args, text in ((["-s", "0.01", "-F", "0.05"], "-s and -F exclude each other"), (["-F", "0.05", "-s", "0.01"], "-s and -F exclude each other"),
                       (["-s", "0"], ranges), (["-s", "1.5"], ranges), (["-F", "0"], ranges), (["-F", "nan"], ranges), (["-m", "-1"], ranges),
                       (["-m", "100.5"], ranges), (["-g", "0"], ranges), (["-n", "0"], ranges), (["-n", "x"], ranges),
                       (["-r", "0"], "-r an integer in [1, 255]"), (["-a", "0"], "-a must be an integer"),
                       (["-Q"], "unrecognised option -Q\n"), (["-G"], "unrecognised option -G\n"), (["-R", "x.bed"], "unrecognised option -R\n")):
        r = _run(["groupdmr", *args, *tail])
        assert r.returncode == 1 and r.stderr.startswith("ERROR: ") and text in r.stderr.splitlines()[0] + "\n", (args, r.stderr[:300])
    r = _run(["groupdmr", "f", "a,b", "c", "o"])
    assert r.returncode == 1 and "group 2 has 1 samples, fewer than -r 2" in r.stderr
    assert _run(["groupdmr", "f", "a,b", "o"]).returncode == 1
    top = _run([]).stderr
    assert "groupdmr [OPTIONS] reference a1,a2,... b1,b2,... output-prefix" in top
    for line in ("pileup [OPTIONS] reference mod-bam output-prefix", "groupdiff [OPTIONS] reference a1,a2,... b1,b2,... output-prefix",
                 "regiondiff -R bed [OPTIONS]", "samplecorr [OPTIONS]", "diff [OPTIONS] reference prefix1 prefix2 output-prefix"):
        assert line in top, line
