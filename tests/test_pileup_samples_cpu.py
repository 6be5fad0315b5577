"""`samplecorr` without a device: the restatement (samples_ref.py) on hand tables and against numpy.corrcoef, its matrix products
against its own locus-by-locus loops, and the command's usage and list checks, which need no GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import samples_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
ULPS = 4 * 2.0 ** -53     # of an r of magnitude 1 with exact num, va, vb: two square roots, a product and a quotient, half an ulp each at most twice over


def _two(rows_i, rows_j, min_cov=5, total=64):
    """two samples from [(gpos, k, n)] each -> the loader"""
    ref = S.SampleLoader(total, 2, min_cov)
    for rows in (rows_i, rows_j):
        assert ref.open() >= 0
        assert ref.load([g for g, _k, _n in rows], [k for _g, k, _n in rows], [n - k for _g, k, n in rows], 0) == len(rows)
    return ref


def _pair(ref, i, j, ctx=0, **kw):
    return next(e for e in ref.sums(**kw) if e[:3] == (i, j, ctx))


def test_identical_samples_give_one():
    rows = [(g, k, 10) for g, k in enumerate([0, 3, 5, 10, 7, 2])]
    e = _pair(_two(rows, rows), 0, 1)
    assert e[3] == 6 and e[4] == e[5] and e[6] == e[7] == e[8]
    assert abs(S.corr(e)[0] - 1.0) <= ULPS          # sqrt(va) * sqrt(va) need not be va


def test_mirrored_levels_give_minus_one():
    """u_j = 32768 - u_i exactly: n = 8 divides k 2^15, so the floor cuts nothing"""
    a = [(g, k, 8) for g, k in enumerate([0, 1, 3, 8, 6, 2])]
    b = [(g, 8 - k, 8) for g, k, _n in a]
    ref = _two(a, b)
    assert (ref.level[1, :6].astype(int) - 1 == 32768 - (ref.level[0, :6].astype(int) - 1)).all()
    assert abs(S.corr(_pair(ref, 0, 1))[0] + 1.0) <= ULPS


def test_a_constant_sample_and_a_single_locus_give_nan():
    a = [(g, k, 10) for g, k in enumerate([1, 4, 9])]
    ref = _two(a, [(g, 5, 10) for g in range(3)])
    assert math.isnan(S.corr(_pair(ref, 0, 1))[0]) and math.isnan(S.corr(_pair(ref, 1, 1))[0]) and abs(S.corr(_pair(ref, 0, 0))[0] - 1.0) <= ULPS
    ref = _two(a[:1], a[:1])
    e = _pair(ref, 0, 1)
    assert e[3] == 1 and math.isnan(S.corr(e)[0]) and S.corr(e)[1] == 100.0 * S.level(1, 10) / 32768
    e = _pair(ref, 0, 1, ctx=2)                               # no locus at all: no mean either
    assert e[3:] == (0,) * 6 and all(math.isnan(x) for x in S.corr(e))


def test_a_locus_below_the_coverage_counts_for_nobody():
    a = [(0, 1, 10), (1, 5, 10), (2, 2, 4), (3, 9, 10)]       # locus 2 has 4 calls in sample 0
    b = [(0, 2, 10), (1, 6, 10), (2, 7, 10), (3, 8, 10)]
    ref = _two(a, b)
    assert ref.level[0, 2] == S.BELOW and ref.level[1, 2] == S.level(7, 10) + 1
    assert _pair(ref, 0, 1)[3] == 3 and _pair(ref, 0, 0)[3] == 3 and _pair(ref, 1, 1)[3] == 4
    assert ref.planes["pcov"][2] == 7 and ref.planes["ncov"][2] == 3     # the pooled counts are those of the counting sample
    assert _pair(ref, 1, 1, complete=True)[3] == 3            # complete mode drops the locus for everybody
    assert ref.load([2], [5], [5], [0]) == S.HM_EDATA and ref.bad[S.KINDS[4]] == 1      # a row below the coverage was a row


def test_check_order_and_kinds():
    ref = S.SampleLoader(64, 2)
    assert ref.load([1], [5], [5], [0]) == S.HM_ESTATE and ref.open() == 0
    rows = ([-1, 64, 5, 5, 5, 5, 6, 6, 7], [5, 5, -1, 1 << 20, -1, 1 << 20, 5, 5, 0], [5, 5, 1 << 21, 0, 5, 0, 5, 5, 0], [9, 0, 9, 9, 0, 0, 4, 0, 3])
    assert ref.load(*rows) == S.HM_EDATA
    assert ref.bad == {S.KINDS[0]: 2, S.KINDS[1]: 2, S.KINDS[2]: 2, S.KINDS[3]: 1, S.KINDS[4]: 0}     # the row without a count passes the checks and is ignored
    assert ref.load([1], [5], [5], [0]) == S.HM_ESTATE and ref.open() == S.HM_ESTATE
    ref = S.SampleLoader(64, 2)
    assert [ref.open(), ref.open(), ref.open()] == [0, 1, S.HM_ESTATE]


@pytest.mark.parametrize("n,complete", [(2, False), (3, True), (5, False), (5, True)])
def test_matrix_products_equal_the_loops(n, complete):
    ref = S.loaded(n)
    for lo, hi in ((0, S.TOTAL), (255, 2049), (3001, 3002)):
        assert ref.sums(lo, hi, complete) == ref.sums_by_loops(lo, hi, complete)
    full = ref.sums(complete=complete)
    assert len(full) == 3 * n * (n + 1) // 2 and all(min(e[3] for e in full if e[2] == c) >= 20 for c in range(3))


def test_complete_differs_from_pairwise_at_the_locus_one_sample_misses():
    ref = S.loaded(3)
    g = S.ALL_BUT_ONE
    c = min(int(ref.planes["key"][g]) & 3, 2)
    assert _pair(ref, 0, 1, c, lo=g, hi=g + 1)[3] == 1 and _pair(ref, 0, 2, c, lo=g, hi=g + 1)[3] == 0
    assert _pair(ref, 0, 1, c, lo=g, hi=g + 1, complete=True)[3] == 0


def test_r_against_numpy_corrcoef():
    """the same quantised levels through numpy's float64 Pearson: within 1e-12"""
    ref = S.loaded(5)
    worst = 0.0
    for e in ref.sums():
        i, j, c = e[:3]
        L = ref.level[[i, j]].astype(np.int64)
        sel = ((L != 0) & (L != S.BELOW)).all(axis=0) & (np.minimum(ref.planes["key"] & 3, 2) == c)
        assert sel.sum() == e[3] >= 20
        want = 1.0 if i == j else np.corrcoef((L[0, sel] - 1).astype(float), (L[1, sel] - 1).astype(float))[0, 1]
        worst = max(worst, abs(S.corr(e)[0] - want))
        assert S.corr(e)[1] == pytest.approx(100.0 * (L[0, sel] - 1).mean() / 32768, rel=1e-13)
    print("worst |r - corrcoef| = %.3g" % worst)
    assert worst <= 1e-12


def test_texts():
    ref = S.loaded(3)
    names = ["a", "b/c", "d"]
    e = ref.sums()
    t = S.samplecorr_tsv(names, e, 1).splitlines()
    assert t[0].split("\t") == ["sample_i", "sample_j", "n", "mean_i", "mean_j", "r"] and [x.split("\t")[:2] for x in t[1:]] == [["a", "b/c"], ["a", "d"], ["b/c", "d"]]
    m = [x.split("\t") for x in S.samplecorr_matrix_tsv(names, e, 1).splitlines()]
    assert m[0] == ["sample"] + names and [x[0] for x in m[1:]] == names and all(m[1 + k][1 + k] == "1" for k in range(3)) and m[1][2] == m[2][1] == t[1].split("\t")[5]
    s = S.samplecorr_samples_tsv(names, e, (0, 2)).splitlines()
    assert s[0] == "ctx\tsample\tn\tmean" and [x.split("\t")[0] for x in s[1:]] == ["CpG"] * 3 + ["CHH"] * 3
    const = _two([(0, 5, 10), (1, 5, 10)], [(0, 1, 10), (1, 2, 10)])
    assert S.samplecorr_matrix_tsv(["x", "y"], const.sums(), 0) == "sample\tx\ty\nx\tnan\tnan\ny\tnan\t1\n"


# ---- the command: usage and the checks of the list, no device ------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([CLI, "samplecorr", *args], capture_output=True, text=True, timeout=60)


def test_usage():
    r = _cli("-h")
    assert r.returncode == 0 and "samplecorr [OPTIONS] reference s1,s2,...,sN output-prefix" in r.stderr
    assert all("\n  -%s" % f in r.stderr for f in "aktd") and "\n  -r" not in r.stderr and "\n  -Q" not in r.stderr


@pytest.mark.parametrize("n", [1, 65])
def test_the_list_takes_two_to_64_samples(n, tmp_path):
    r = _cli(str(tmp_path / "no.fa"), ",".join("s%d" % k for k in range(n)), str(tmp_path / "out"))
    assert r.returncode == 1 and "2 to 64 samples, the list names %d" % n in r.stderr and "USAGE:" in r.stderr
    assert "no.fa" not in r.stderr and not os.listdir(tmp_path)       # before any file is opened


def test_bad_options(tmp_path):
    for args, text in ((("-a", "0"), "-a must be an integer in [1, 1048575]"), (("-a", "1048576"), "-a must be"), (("-r", "2"), "unrecognised option -r")):
        r = _cli(*args, "ref.fa", "a,b", str(tmp_path / "out"))
        assert r.returncode == 1 and text in r.stderr and "USAGE:" in r.stderr
    assert _cli("ref.fa", "a,b").returncode == 1 and _cli("ref.fa", "a,b", "out", "more").returncode == 1
