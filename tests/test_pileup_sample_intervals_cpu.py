"""`regiondiff` without a device: the restatement (intervals_ref.py) of the interval sums against its own locus-by-locus loops, of
the test on hand-made tables, E_ref -- the worst relative error of the float64 form of the statistic against mpmath at 50 digits --
and the command's usage, its cross-option checks and the header's declarations, which need no GPU.
test_gpu_pileup_sample_intervals.py takes 8 x E_ref as its bar.

Measured here: E_ref = 1.9e-14 for t, 1.2e-15 for df, 7.5e-15 for p (the 138 cases with a finite statistic: 132 tiles of the data set
and 6 hand-made ones)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import intervals_ref as I
import samples_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
BLOCK = 4096


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------
def _small():
    """three samples on 600 bases: contexts interleaved, stored values 0, 0xFFFF, 1 and 32769 among them"""
    rng = np.random.default_rng(5)
    ref = S.SampleLoader(600, 4)
    g = np.flatnonzero(rng.random(600) < 0.7)
    motif = rng.integers(0, 4, len(g))
    for _s in range(3):
        has = rng.random(len(g)) < 0.8
        cov = rng.integers(1, 13, len(g))
        p = np.where(rng.random(len(g)) < 0.15, 0, np.where(rng.random(len(g)) < 0.15, cov, rng.binomial(cov, 0.5)))
        assert ref.open() >= 0 and ref.load(g[has], p[has], (cov - p)[has], motif[has]) == has.sum()
    return ref


def test_running_sums_equal_the_loops():
    ref = _small()
    stored = set(np.unique(ref.level[:3]).tolist())
    assert {0, S.BELOW, 1, 32769} <= stored and not ref.level[3].any()
    start = [0, 0, 5, 17, 300, 599, 600, 250, 250, -9, 590, 700, 40, 41]
    end = [600, 0, 6, 450, 301, 600, 600, 260, 260, 20, 650, 800, 41, 41]
    differ = False
    for ctx in range(3):
        for lo, hi in ((0, 600), (13, 577), (300, 300)):
            for complete in (False, True):
                got = I.interval_sums(ref, start, end, ctx, lo, hi, complete)
                assert got.shape == (len(start), 3, 2) and got.dtype == np.uint64
                assert got.tolist() == [[list(x) for x in row] for row in I.interval_sums_by_loops(ref, start, end, ctx, lo, hi, complete)]
            differ |= I.interval_sums(ref, start, end, ctx).tolist() != I.interval_sums(ref, start, end, ctx, complete=True).tolist()
    assert differ
    whole = I.interval_sums(ref, [0], [600], 0)[0]
    assert whole[:, 0].min() > 20 and (whole[:, 1] > whole[:, 0]).all()
    parts = I.interval_sums(ref, [0], [600], 0, 0, 123) + I.interval_sums(ref, [0], [600], 0, 123, 600)
    assert (parts == whole).all()


# ---- the test ---------------------------------------------------------------------------------------------------------------------------
def test_every_outcome_occurs_and_is_what_the_definition_says():
    r = {k: I.welch(*v) for k, v in I.HAND.items()}
    for k, v in r.items():
        m1, m2, n1, n2, mean1, mean2, t, df, p = v
        if k.startswith("tested"):
            assert m1 >= 2 and m2 >= 2 and math.isfinite(t) and math.isfinite(df) and I.DBL_MIN <= p <= 1.0, k
            assert min(m1, m2) - 1 <= df * (1 + 1e-12) and df <= (m1 + m2 - 2) * (1 + 1e-12), k       # Welch-Satterthwaite's range
        elif k.startswith("untested"):
            assert (m1 < 2 or m2 < 2) and all(x != x for x in (t, df, p)), k
    assert r["tested, far apart"][8] < 1e-3 < 0.2 < r["tested, close"][8]
    assert r["tested, equal means with spread"][6:] == (0.0, 2.0, 1.0)
    assert r["tested, a sample out of it"][:4] == (2, 3, 22, 31) and r["tested, two against five"][:2] == (2, 5)
    assert r["untested, too few loci"][:4] == (1, 3, 10, 31) and r["untested, too few loci"][4] == 100.0 * 163840 / (10 * 32768)
    assert r["untested, nothing"][:6][:4] == (0, 0, 0, 0) and r["untested, nothing"][4] != r["untested, nothing"][4]
    assert r["se2 = 0, equal means"][6:] == (0.0, 4.0, 1.0)
    t, df, p = r["se2 = 0, unequal means"][6:]
    assert t == -math.inf and df != df and p != p
    assert r["se2 = 0, unequal the other way"][6] == -math.inf and r["se2 = 0, unequal the other way"][:2] == (2, 2)
    swapped = I.welch(I.HAND["se2 = 0, unequal means"][0], (2, 2, 2, 1, 1, 1))
    assert swapped[6] == math.inf
    # against scipy's own Welch test on the levels
    from scipy import stats
    pairs, group = I.HAND["tested, close"]
    x = [100.0 * su / (n * 32768.0) for n, su in pairs]
    want = stats.ttest_ind(x[:3], x[3:], equal_var=False)
    got = r["tested, close"]
    assert abs(got[6] - want.statistic) <= 1e-12 * abs(want.statistic) and abs(got[8] - want.pvalue) <= 1e-11 * want.pvalue


def test_the_data_set_is_not_degenerate():
    tests = [I.welch(*c) for c in I.cases()[len(I.HAND):]]
    tested = [t for t in tests if t[6] == t[6]]
    assert len(tests) == 3 * 44 and len(tested) > 100 and len(tests) - len(tested) >= 0
    p = [t[8] for t in tested]
    assert min(p) < 1e-3 and max(p) > 0.5                       # the middle sequence differs, the others do not
    q = I.bh([t[8] for t in tests])
    assert sum(1 for v in q if v <= 0.05) >= 5 and sum(1 for v in q if v > 0.5) >= 5


def test_bh():
    nan = math.nan
    assert I.bh([]) == [] and I.bh([0.5]) == [0.5]
    q = I.bh([0.01, nan, 0.04, 0.03, 0.03, 1.0, nan])
    assert q[1] != q[1] and q[6] != q[6]
    assert q[0] == min(0.01 * 5 / 1, 0.03 * 5 / 3) and q[3] == q[4] == 0.03 * 5 / 3 and q[2] == 0.04 * 5 / 4 and q[5] == 1.0
    assert I.bh([0.9, 0.8]) == [0.9, 0.9] and I.bh([0.2, 0.1, 0.1]) == [0.2 * 3 / 3, 0.1 * 3 / 2, 0.1 * 3 / 2]


def test_texts():
    ivs = [("ctg1", 5, 90, "a", "+"), ("ctg2", 0, 10, ".", "."), ("ctg2", 3, 4, "x", "-")]
    tests = [I.welch(*I.HAND[k]) for k in ("tested, far apart", "untested, nothing", "se2 = 0, unequal means")]
    q = I.bh([t[8] for t in tests])
    lines = I.regiondiff_tsv(ivs, tests, q).splitlines()
    assert lines[0].split("\t") == ["#chrom", "start", "end", "name", "strand", "m1", "m2", "loci1", "loci2", "mean1", "mean2", "diff", "t", "df", "p", "q"]
    assert all(len(x.split("\t")) == 16 for x in lines) and len(lines) == 4
    assert lines[1].split("\t")[:9] == ["ctg1", "5", "90", "a", "+", "3", "3", "31", "31"] and lines[1].split("\t")[14] == lines[1].split("\t")[15]
    assert lines[2].split("\t")[5:] == ["0", "0", "0", "0"] + ["nan"] * 7
    assert lines[3].split("\t")[9:] == ["3.05176", "6.10352", "-3.05176", "-inf", "nan", "nan", "nan"]
    s = I.regiondiff_summary_tsv({0: tests, 2: tests[1:]}, {0: q, 2: [math.nan, math.nan]})
    assert s == "ctx\tintervals\ttested\tq<=0.05\tq<=0.01\nCpG\t3\t2\t1\t1\nCHH\t2\t1\t0\t0\n"


def test_measure_e_ref():
    """prints the figures DESIGN.md section 10 quotes; the float64 form is a reference, so all it has to be is close"""
    e = I.e_ref()
    n = sum(1 for c in I.cases() if I.welch_mp(*c) is not None)
    print("E_ref over %d cases: t %.3g, df %.3g, p %.3g" % (n, e["t"], e["df"], e["p"]))
    assert 0 < e["t"] < 1e-10 and 0 < e["df"] < 1e-10 and 0 < e["p"] < 1e-9


# ---- the command: usage and the checks between options, no device ---------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([CLI, "regiondiff", *args], capture_output=True, text=True, timeout=60)


def test_usage():
    r = _cli("-h")
    assert r.returncode == 0 and "regiondiff -R intervals.bed [OPTIONS] reference a1,a2,... b1,b2,... output-prefix" in r.stderr
    assert all("\n  -%s" % f in r.stderr for f in "Raklr") and "\n  -t" in r.stderr and "\n  -d" in r.stderr
    assert "\n  -Q" not in r.stderr and "\n  -C" not in r.stderr and "\n  -J" not in r.stderr
    assert "Default: 5" in r.stderr and "Default: 3" in r.stderr and "Default: 2" in r.stderr
    top = subprocess.run([CLI], capture_output=True, text=True, timeout=60)
    assert "regiondiff -R bed [OPTIONS] reference a1,a2,... b1,b2,... output-prefix" in top.stderr + top.stdout


def test_cross_option_errors(tmp_path):
    bed = str(tmp_path / "iv.bed")
    for args, text in (((), "regiondiff needs -R"), (("-a", "3"), "regiondiff needs -R"), (("-R", bed, "-a", "0"), "-a must be an integer in [1, 1048575]"),
                       (("-R", bed, "-a", "1048576"), "-a must be"), (("-R", bed, "-l", "0"), "-l an integer >= 1"), (("-R", bed, "-l", "x"), "-l an integer >= 1"),
                       (("-R", bed, "-r", "1"), "-r an integer in [2, 64]"), (("-R", bed, "-r", "65"), "-r an integer in [2, 64]"),
                       (("-R", bed, "-Q", "1"), "unrecognised option -Q"), (("-R", bed, "-C", "2"), "unrecognised option -C")):
        r = _cli(*args, "ref.fa", "a,b", "c,d", str(tmp_path / "out"))
        assert r.returncode == 1 and text in r.stderr and "USAGE:" in r.stderr, args
    assert _cli("-R", bed, "ref.fa", "a,b", "c,d").returncode == 1 and _cli("-R", bed, "ref.fa", "a,b", "c,d", "out", "more").returncode == 1
    r = _cli("-R", bed, "-r", "3", str(tmp_path / "no.fa"), "a,b,c", "d,e", str(tmp_path / "out"))
    assert r.returncode == 1 and "group 2 has 2 samples, fewer than -r 3" in r.stderr
    r = _cli("-R", bed, str(tmp_path / "no.fa"), ",".join("a%d" % k for k in range(40)), ",".join("b%d" % k for k in range(25)), str(tmp_path / "out"))
    assert r.returncode == 1 and "2 to 64 samples in all, the lists name 65" in r.stderr and "USAGE:" in r.stderr
    r = _cli("-R", bed, str(tmp_path / "no.fa"), "a,,b", "c,d", str(tmp_path / "out"))
    assert r.returncode == 1 and "an empty prefix in the list of group 1" in r.stderr
    assert "no.fa" not in r.stderr and not os.listdir(tmp_path)       # before any file is opened


def test_the_header_declares_the_calls():
    text = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    for name in ("hm_sample_fetch_intervals", "hm_sample_interval_test", "hm_sample_qvalues"):
        assert re.search(r"^int(64_t)? %s\(" % name, text, re.M), name
    for name, fields in (("hm_sample_interval_t", "uint64_t n, su;"), ("hm_sample_test_t", "double mean1, mean2, t, df, pvalue;")):
        assert re.search(r"typedef struct \{[^}]*%s[^}]*\} %s;" % (re.escape(fields), name), text), name
    assert "#define HM_ABI_VERSION 5" in text
    from hifimeth_amd import _lib
    L = _lib.lib()
    assert all(hasattr(L, n) for n in ("hm_sample_fetch_intervals", "hm_sample_interval_test", "hm_sample_qvalues"))
