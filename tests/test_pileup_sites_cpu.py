"""Host side of `pileup -B / -e` (no GPU): hm_sites_table -- the one implementation of the binomial test and of the
Benjamini-Hochberg q-values -- against exact arithmetic and a sort-based BH, the text of the sites files, and the command lines'
argument errors, which are decided before any device call.

Tolerance of a p-value, derived and not measured: the exponent of a term adds five values of magnitude <= log 4096! ~ 3e4, each
rounded once (ulp 3.6e-12 there), about 2e-11 absolute, which is the relative error of the term and of the sum of such terms;
the bound is 1e-9 relative, x50 over that.  Where a rule fixes the value it must be met exactly: k = 0 -> 1.0, rate 0 -> DBL_MIN,
rate 1 -> 1.0, and a tail below the smallest normal double is reported as DBL_MIN (never 0)."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_pileup_sites import DBL_MIN, bh_by_sort, binomial_tail_exact

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
NAN = float("nan")
RATES = (0.0, 1e-6, 0.013, 0.5, 1.0)
BIG_N = (256, 257, 1000, 4096)


def _big(rows):
    """[(pcov, ncov, motif)] -> LOCUS_DTYPE array with ascending gpos"""
    from hifimeth_amd.pileup import LOCUS_DTYPE
    big = np.zeros(len(rows), LOCUS_DTYPE)
    big["gpos"] = 1000 + 3 * np.arange(len(rows))
    for i, (p, n, m) in enumerate(rows):
        big[i]["pcov"], big[i]["ncov"], big[i]["motif"] = p, n, m
    return big


def _check_p(got, k, n, e):
    if k == 0 or e == 1.0:
        assert got == 1.0, (k, n, e)
        return 0.0
    if e == 0.0:
        assert got == DBL_MIN, (k, n, e)
        return 0.0
    want = binomial_tail_exact(k, n, e)
    if want < Fraction(DBL_MIN):                              # clamped by rule
        assert got == DBL_MIN, (k, n, e)
        return 0.0
    assert DBL_MIN <= got <= 1.0
    err = float(abs(Fraction(float(got)) - want) / want)
    assert err <= 1e-9, (k, n, e, got, float(want), err)
    return err


def test_exact_reference_by_hand():
    assert binomial_tail_exact(0, 7, 0.25) == 1
    assert binomial_tail_exact(2, 2, 0.5) == Fraction(1, 4) and binomial_tail_exact(1, 2, 0.5) == Fraction(3, 4)
    assert binomial_tail_exact(2, 3, 0.25) == Fraction(3 * 3 + 1, 64)               # 3 (1/4)^2 (3/4) + (1/4)^3
    assert binomial_tail_exact(1, 30, 0.5) == 1 - Fraction(1, 2 ** 30)
    assert binomial_tail_exact(5, 5, 1.0) == 1 and binomial_tail_exact(3, 5, 0.0) == 0


def test_exact_reference_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    for k, n, e in ((3, 30, 0.013), (100, 500, 0.25), (1, 4096, 1e-6), (40, 40, 0.5)):
        assert abs(stats.binom.sf(k - 1, n, e) / float(binomial_tail_exact(k, n, e)) - 1) < 1e-10


@pytest.mark.parametrize("rate", RATES)
def test_pvalues_against_exact_arithmetic(rate):
    from hifimeth_amd.pileup import sites_table
    bins = np.zeros((3, 256, 256), np.uint64)
    small = [(k, n) for n in list(range(1, 41)) + [255] for k in (range(n + 1) if n <= 40 else (0, 1, n // 2, n))]
    for k, n in small:
        bins[0, n, k] = 1
    big_kn = [(k, n) for n in BIG_N for k in (0, 1, n // 2, n)]
    t = sites_table([rate, NAN, rate], bins, _big([(k, n - k, 0) for k, n in big_kn]))
    worst = 0.0
    for k, n in small:
        worst = max(worst, _check_p(t.ptab[0, n, k], k, n, rate))
    for (k, n), got in zip(big_kn, t.big_p):
        worst = max(worst, _check_p(got, k, n, rate))
    print(f"rate {rate}: worst relative error of p over {len(small) + len(big_kn)} cases {worst:.3e}")
    # the table is a function of the rate, not of the bins: every k <= n < 256 of a tested context is filled, the rest is NaN
    filled = ~np.isnan(t.ptab)
    assert filled[0].sum() == filled[2].sum() == 256 * 257 // 2 and not filled[1].any()
    assert (t.ptab[0][filled[0]] == t.ptab[2][filled[2]]).all()
    assert all(filled[0, n, k] == (k <= n) for n in (0, 1, 100, 255) for k in (0, 1, 100, 255))
    assert (t.m == [len(small) + len(big_kn), 0, 0]).all()
    assert (~np.isnan(t.qtab)).sum() == len(small) and not np.isnan(t.big_q).any()


def _expand(t, bins, big, c):
    """one (p, q) per locus of context c, as the table gives them"""
    n, k = np.nonzero(bins[c])
    cnt = bins[c][n, k].astype(np.int64)
    sel = big["motif"] == c
    p = np.concatenate([np.repeat(t.ptab[c][n, k], cnt), t.big_p[sel]])
    q = np.concatenate([np.repeat(t.qtab[c][n, k], cnt), t.big_q[sel]])
    return p, q


def test_bh_against_sort_based_reference():
    from hifimeth_amd.pileup import sites_table
    rng = np.random.default_rng(3)
    bins = np.zeros((3, 256, 256), np.uint64)
    for c in (0, 1):                                          # CpG tested, CHG populated but not tested, CHH tested and empty
        n = rng.integers(1, 256, 400)
        k = (rng.random(400) * np.minimum(n + 1, 8)).astype(np.int64)            # small k: p-values all over (0, 1]
        np.add.at(bins[c], (n, k), rng.integers(1, 40, 400))
        bins[c, 1:200, 0] += 3                                # ties: different (0, n), all with p = 1.0 bit for bit
    big = _big([(int(k), int(n - k), int(m)) for k, n, m in zip(rng.integers(0, 12, 60), rng.integers(256, 5000, 60), rng.integers(0, 2, 60))])
    t = sites_table([0.01, NAN, 0.2], bins, big)
    assert (t.m == [bins[0].sum() + (big["motif"] == 0).sum(), bins[1].sum() + (big["motif"] == 1).sum(), 0]).all()
    p, q = _expand(t, bins, big, 0)
    assert len(p) == t.m[0] > 5000 and not np.isnan(p).any() and not np.isnan(q).any()
    want = bh_by_sort(p)
    assert (np.abs(q - want) <= np.spacing(want)).all(), np.abs(q - want).max()
    # big loci whose p falls strictly between two table entries, ties at 1.0, q monotone in p and equal for equal p
    tab = np.unique(t.ptab[0][bins[0] > 0])
    bp = t.big_p[big["motif"] == 0]
    assert ((bp > tab[0]) & (bp < tab[-1]) & ~np.isin(bp, tab)).sum() >= 5
    assert (p == 1.0).sum() >= 3 * 199 and set(q[p == 1.0]) == {1.0}
    order = np.argsort(p, kind="stable")
    assert (np.diff(q[order]) >= 0).all() and (q >= p).all() and (q <= 1).all() and (q < 0.05).any()
    for v in np.unique(p)[:50]:
        assert len(set(q[p == v])) == 1
    # the context without a rate: nothing in its tables, its big loci NaN; the tested context without loci: p filled, no q
    assert np.isnan(t.ptab[1]).all() and np.isnan(t.qtab[1]).all() and np.isnan(t.big_p[big["motif"] == 1]).all()
    assert np.isnan(t.big_q[big["motif"] == 1]).all() and not np.isnan(t.big_q[big["motif"] == 0]).any()
    assert (~np.isnan(t.ptab[2])).sum() == 256 * 257 // 2 and np.isnan(t.qtab[2]).all()
    # the same loci under another rate, now with CHG tested: an independent problem per context
    t2 = sites_table([0.01, 0.03, NAN], bins, big)
    assert (t2.qtab[0][bins[0] > 0] == t.qtab[0][bins[0] > 0]).all()
    p1, q1 = _expand(t2, bins, big, 1)
    want1 = bh_by_sort(p1)
    assert (np.abs(q1 - want1) <= np.spacing(want1)).all()
    # one locus: q = p
    one = np.zeros((3, 256, 256), np.uint64)
    one[2, 30, 3] = 1
    t3 = sites_table([NAN, NAN, 0.013], one)
    assert t3.qtab[2, 30, 3] == t3.ptab[2, 30, 3] and (t3.m == [0, 0, 1]).all() and len(t3.big_p) == 0


def test_sites_table_rejects_what_is_no_histogram():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import HifimethError, sites_table
    ok = np.zeros((3, 256, 256), np.uint64)
    for rates in ([1.5, NAN, NAN], [NAN, -0.1, NAN], [NAN, NAN, float("inf")]):
        with pytest.raises(HifimethError):
            sites_table(rates, ok)
    for n, k in ((3, 4), (0, 0), (200, 255)):                 # k > n, or a locus without reads
        bad = ok.copy()
        bad[1, n, k] = 1
        with pytest.raises(HifimethError):
            sites_table([0.1, 0.1, 0.1], bad)
    for row in ((10, 20, 0), (300, 5, 3), (-1, 400, 1)):      # n < 256, no such context, a negative count
        with pytest.raises(HifimethError):
            sites_table([0.1, 0.1, 0.1], ok, _big([row]))
    with pytest.raises(HifimethError):
        sites_table([0.1, 0.1], ok)
    assert lib().hm_sites_table(None, None, None, 0, None, None, None, None, None) == -1


def test_rates():
    from hifimeth_amd.pileup import parse_rates, rates_from_sums
    assert parse_rates("0.1,0,1") == [0.1, 0.0, 1.0] and parse_rates("1e-3,.5,2.5E-1") == [0.001, 0.5, 0.25]
    r = parse_rates("nan,0.043210000000000001,nan")
    assert np.isnan(r[0]) and np.isnan(r[2]) and r[1] == 0.04321
    for bad in ("", "0.1,0.2", "0.1,0.2,0.3,0.4", "0.1,0.2,1.5", "0.1,-0.2,0.3", "0.1,abc,0.3", "0.1,,0.3", "0.1,NaN,0.3", "inf,0,0",
                "0x1p-3,0,0", "0.1, 0.2,0.3", "1e,0,0", "+0.5,0,0"):
        with pytest.raises(ValueError):
            parse_rates(bad)
    r = rates_from_sums([1, 0, 2 ** 40 + 1, 2, 0, 2 ** 41])
    assert r[0] == 1 / 3 and np.isnan(r[1]) and r[2] == float(2 ** 40 + 1) / float(2 ** 40 + 1 + 2 ** 41)


def test_sites_bed_and_rates_text():
    from hifimeth_amd.pileup import SITE_DTYPE, MethylationPileup, sites_rates_tsv
    assert SITE_DTYPE.itemsize == 40 and SITE_DTYPE.fields["pvalue"][1] == 24 and SITE_DTYPE.fields["qvalue"][1] == 32
    pu = MethylationPileup.__new__(MethylationPileup)                     # formatting needs names and offsets only
    pu.names = ["chrA", "chrB"]
    pu.offsets = np.array([0, 100, 250], np.int64)
    pu._h = None
    rows = np.zeros(5, SITE_DTYPE)
    rows["gpos"] = [3, 99, 100, 249, 7]
    rows["motif"] = [0, 1, 2, 0, 0]
    rows["pcov"] = [2, 0, 3, 5000, 1]
    rows["ncov"] = [28, 7, 27, 65000, 2]
    rows["pvalue"] = [0.0583120589, 1.0, 0.006862305873597698, DBL_MIN, 0.5]
    rows["qvalue"] = [0.0874680883, 1.0, 0.010345601906416684, 3.35518887e-304, 1.0]
    text = pu.sites_bed(rows)
    assert text["CpG"] == ("chrA\t3\t4\t6.66667\t2\t28\t0.0583121\t0.0874681\n"
                           "chrB\t149\t150\t7.14286\t5000\t65000\t2.22507e-308\t3.35519e-304\n"
                           "chrA\t7\t8\t33.3333\t1\t2\t0.5\t1\n")
    assert text["CHG"] == "chrA\t99\t100\t0\t0\t7\t1\t1\n"
    assert text["CHH"] == "chrB\t0\t1\t10\t3\t27\t0.00686231\t0.0103456\n"
    assert pu.sites_bed(rows[:0]) == {"CpG": "", "CHG": "", "CHH": ""}
    # the first six columns are the cov.bed row
    from hifimeth_amd.pileup import LOCUS_DTYPE
    loci = np.zeros(5, LOCUS_DTYPE)
    for f in ("gpos", "pcov", "ncov", "motif"):
        loci[f] = rows[f]
    cov = pu.bed(loci)
    for c in ("CpG", "CHG", "CHH"):
        assert [r.rsplit("\t", 2)[0] for r in text[c].splitlines()] == cov[c].splitlines()
    assert sites_rates_tsv([12, 0, 3, 988, 0, 297], [0.012, NAN, 0.01], [70, 5, 123456789012]) == \
        "CpG\t12\t988\t0.012\t70\nCHG\t0\t0\tnan\t5\nCHH\t3\t297\t0.01\t123456789012\n"
    assert sites_rates_tsv([0] * 6, [1 / 3, 0.0, 1.0], [1, 2, 3]) == "CpG\t0\t0\t0.33333333333333331\t1\nCHG\t0\t0\t0\t2\nCHH\t0\t0\t1\t3\n"


BAD_ARGS = (["-B", "ctl", "-e", "0.1,0.2,0.3"], ["-e", "0.1,0.2"], ["-e", "0.1,abc,0.3"], ["-e", "0.1,0.2,0.3,0.4"], ["-e", "0.1,,0.3"],
            ["-e", "0.1,0.2,1.5"], ["-e", "2,0.2,0.5"], ["-e", "0.1,0.2,inf"])


def test_cli_argument_errors_need_no_device(tmp_path):
    """-B with -e, a malformed -e, a rate outside [0, 1]: usage on stderr, EXIT_FAILURE, nothing created -- before a file or a
    device is opened"""
    for k, args in enumerate(BAD_ARGS):
        r = subprocess.run([CLI, "pileup", *args, str(tmp_path / "no.fa"), str(tmp_path / "no.bam"), str(tmp_path / f"out{k}")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, (args, r.stderr)
        assert "USAGE" in r.stderr and "ERROR" in r.stderr and "no HIP device" not in r.stderr and "no.bam" not in r.stderr
        assert ("-B and -e" if "-B" in args else "-e takes") in r.stderr.split("USAGE")[0]
        assert os.listdir(tmp_path) == []
    # well-formed options get as far as the input file
    for args in (["-e", "0.1,nan,1e-3"], ["-B", "ctl"], ["-H", "-A", "-e", "0,1,.5"]):
        r = subprocess.run([CLI, "pileup", *args, str(tmp_path / "no.fa"), str(tmp_path / "no.bam"), str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "USAGE" not in r.stderr and "no.bam" in r.stderr and "sites:" in r.stderr
    r = subprocess.run([CLI, "pileup", "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-B <sequence name>" in r.stderr and "-e <r_cpg,r_chg,r_chh>" in r.stderr and ".sites." in r.stderr


def test_pileup_dist_argument_errors_need_no_device(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for args in BAD_ARGS:
        r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, "no.fa", "no.bam", str(tmp_path / "o")],
                           capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
        assert r.returncode == 2 and "usage" in r.stderr, (args, r.stderr)
        assert ("-B and -e" if "-B" in args else "-e") in r.stderr.splitlines()[-1]
        assert os.listdir(tmp_path) == []


def test_abi_struct():
    from hifimeth_amd._lib import lib
    L = lib()
    for name in ("hm_pileup_control_sums", "hm_pileup_site_histogram", "hm_sites_table", "hm_pileup_fetch_sites"):
        assert name in L._hm_symbols
    assert L.hm_abi_version() == 5                                        # no existing struct changed
