"""`pileup -L` without a GPU: the textbook restatement (tests/linkage_ref.py) on a hand-made alignment with the four counts written
out by hand, the inputs of the GPU test checked for the conditions they are built for, the min / max / first identity the engine
counts by against direct counting, hm_linkage_stats -- host only -- against the direct formulas, and the command line's refusals."""
import ctypes
import math
import os
import subprocess

import numpy as np

import linkage_cases as C
import linkage_ref as R
import patterns_cases as K
from conftest import ROOT
from patterns_ref import member_loci, reference_cpgs

HM_EINVAL = -1
CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")


def _rec(pos, cigar, seq, ml, flag=0, mapq=60):
    """a forward record with one C+m call per C of `seq`, ML as given"""
    assert seq.count("C") == len(ml)
    return dict(flag=flag, tid=0, pos=pos, mapq=mapq, cigar=cigar, seq=seq, mm="C+m" + ",0" * len(ml) + ";", ml=list(ml))


#        0         1         2
#        0123456789012345678901234567
CHR = "ATCGATTCGAAACGTTTTTTTTTTTCGA"       # CpGs at 2, 7, 12, 25: distances 5, 10, 23, 5, 18, 13
CHRS = [("c", CHR)]


def test_restatement_on_a_hand_made_alignment():
    full = lambda ml, **kw: _rec(0, [("M", 28)], CHR, ml, **kw)
    recs = [full([200, 200, 10, 200]),                                                          # M M U M
            full([128, 127, 128, 0]),                                                           # M U M U at thr 128
            _rec(0, [("M", 9), ("D", 2), ("M", 17)], CHR[:9] + CHR[11:], [200, 10, 200, 10]),    # a deletion between 7 and 12: all four
            _rec(0, [("M", 6), ("D", 4), ("M", 18)], CHR[:6] + CHR[10:], [200, 200, 200]),       # 7 deleted: members 2, 12, 25
            _rec(0, [("M", 13)], CHR[:13], [10, 10, 200]),                                      # ends on the C of 12: members 2, 7
            full([10, 10, 10, 10], mapq=3)]
    # the classes per record at 2, 7, 12, 25 (thr 128): rec0 M M U M, rec1 M U M U, rec2 M U M U, rec3 M - M M, rec4 U U - -, rec5 U U U U
    #           UU UM MU MM
    want = {5: [3, 2, 3, 1],     # (2, 7): MM MU MU UU UU (recs 0 1 2 4 5) and (7, 12): MU UM UM UU (recs 0 1 2 5)
            10: [1, 0, 1, 3],    # (2, 12): MU MM MM MM UU (recs 0 1 2 3 5)
            13: [1, 1, 2, 1],    # (12, 25): UM MU MU MM UU (recs 0 1 2 3 5)
            18: [3, 0, 0, 1],    # (7, 25): MM UU UU UU (recs 0 1 2 5)
            23: [1, 0, 2, 2]}    # (2, 25): MM MU MU MM UU (recs 0 1 2 3 5)
    got = R.pairs(recs, CHRS, 100, thr=128)
    assert got == want
    assert R.pairs(recs, CHRS, 12, thr=128) == {5: want[5], 10: want[10]}                         # 13 is beyond max_dist 12
    assert R.pairs(recs, CHRS, 13, thr=128).keys() == {5, 10, 13}
    assert R.pairs(recs, CHRS, 100, thr=128, min_mapq=5)[5] == [1, 2, 3, 1]                       # the last record leaves: two UU fewer
    n5 = sum(want[5])
    assert R.pairs(recs, CHRS, 100, thr=0)[5] == [0, 0, 0, n5] and R.pairs(recs, CHRS, 100, thr=255)[5] == [n5, 0, 0, 0]
    rows = R.rows(recs, CHRS, 23, thr=128, min_pairs=5)
    assert rows == [(5, 3, 2, 3, 1), (10, 1, 0, 1, 3), (13, 1, 1, 2, 1), (23, 1, 0, 2, 2)]        # 18 has four pairs
    assert len(R.rows(recs, CHRS, 23, thr=128, min_pairs=0)) == 22 and R.rows(recs, CHRS, 23, thr=128, min_pairs=10) == []
    # one row by hand: n 9, concordance 4 / 9, r = (1 * 3 - 3 * 2) / sqrt(4 * 5 * 3 * 6)
    assert R.tsv_text(rows[:1]) == R.HEADER + "5\t9\t3\t2\t3\t1\t%.6g\t%.6g\n" % (4 / 9, -3 / math.sqrt(360))
    assert R.tsv_text([(7, 0, 0, 0, 0)]) == R.HEADER + "7\t0\t0\t0\t0\t0\tnan\tnan\n"


def test_gpu_inputs_hold_their_cases():
    g = C.genome()
    assert g[:3] == K.genome() and tuple(reference_cpgs(g)[C.LK_TID]) == C.LK and tuple(reference_cpgs(g)[C.BIG_TID]) == C.big_cpgs()
    reads = C.reads()
    mem = lambda r, **kw: {s: p for (_t, s), p in member_loci(C.as_dict(r), g, **kw).items()}
    named = lambda n: [r for r in reads if r.name == n]
    assert reads[0].name == "long_f" and len(reads[0].seq) == 1600 and {1018, 1030} <= set(mem(reads[0]))  # a pair across column 1024
    assert len(reads[0].seq) + len(reads[1].seq) < 4096 < len(reads[0].seq) + len(reads[1].seq) + len(reads[2].seq)
    for t in "fr":
        for n in ("reach_", "gapD_", "gapN_", "eq_"):
            assert set(mem(named(n + t)[0])) == set(C.LK), n
        assert [op for op, _n in named("gapD_" + t)[0].cigar] == ["M", "D", "M"] and [op for op, _n in named("gapN_" + t)[0].cigar] == ["M", "N", "M"]
        assert set(mem(named("single_" + t)[0])) == {450}
        assert set(mem(named("adj_a_" + t)[0])) == {50, 52} and set(mem(named("adj_b_" + t)[0])) == {60, 450, 461}
        a, b = named("twin_" + t)
        assert set(mem(a)) == {50, 52} and set(mem(b)) == {60, 450, 461} and b.flag & 2048 and not a.flag & 2048
        assert [mem(named("eq_" + t)[0])[s] for s in C.LK] == [C.THR, C.THR, C.THR - 1, C.THR - 1, 255]
        big = mem(named("big_" + t)[0])
        assert {100, 102, 16484, 16486} <= set(big) and len(big) > 90
    # neighbours in the input: the last member of adj_a_r is 52, the first of adj_b_f 60 -- 8 apart, and no pair
    i = next(k for k, r in enumerate(reads) if r.name == "adj_b_f")
    assert reads[i - 1].name == "adj_a_r" and reads[i - 1].pos + 15 > reads[i].pos
    assert C.LK[1] - C.LK[0] == 2 and C.LK[3] - C.LK[0] == C.MAX_DIST and C.LK[4] - C.LK[2] == C.MAX_DIST + 1
    recs = [C.as_dict(r) for r in reads]
    at = R.pairs(recs, g, C.MAX_DIST, thr=C.THR)
    assert C.MAX_DIST in at and C.MAX_DIST + 1 not in at and C.MAX_DIST + 1 in R.pairs(recs, g, C.MAX_DIST + 1, thr=C.THR)
    # d = 8 comes from lk's 52 | 60 alone: the eight records that hold both, none from adj_a | adj_b or the twins
    assert sum(at[8]) == 8 + sum(len({a + 8 for a in mem(r)} & set(mem(r))) for r in reads if r.tid != C.LK_TID)
    eq = R.pairs([C.as_dict(named("eq_f")[0])], g, C.MAX_DIST, thr=C.THR)
    assert eq[2] == [0, 0, 0, 1] and eq[8] == [0, 0, 1, 0] and eq[390] == [1, 0, 0, 0]            # pa == pb == t; t | t - 1; both t - 1
    far = R.pairs([C.as_dict(named("big_f")[0])], g, 16384, thr=C.THR)
    assert sum(far[16384]) == 2 and 16386 not in far
    assert 16386 in R.pairs([C.as_dict(named("big_f")[0])], g, 16386, thr=C.THR)
    crowd = C.crowd(300)
    assert len(crowd) == 300 and sum(R.pairs([C.as_dict(r) for r in crowd], g, C.MAX_DIST, thr=C.THR)[2]) == 300


def test_min_max_first_identity_for_every_threshold():
    """what the engine keeps per distance -- histograms of min(pa, pb), max(pa, pb) and pa -- gives the four classes of direct
    counting for all 256 thresholds (and 256: nothing methylated)"""
    rng = np.random.default_rng(4204)
    n, D = 4000, 6
    pa, pb, d = rng.integers(0, 256, n), rng.integers(0, 256, n), rng.integers(2, D + 1, n)
    pa[::9] = pb[::9]                                                       # ties
    pa[::50], pb[1::50] = 0, 255
    H = np.zeros((D + 1, 3, 256), np.int64)
    for a, b, k in zip(pa, pb, d):
        H[k, 0, min(a, b)] += 1
        H[k, 1, max(a, b)] += 1
        H[k, 2, a] += 1
    for t in range(257):
        for k in range(2, D + 1):
            m = d == k
            direct = [int((m & ~(pa >= t) & ~(pb >= t)).sum()), int((m & ~(pa >= t) & (pb >= t)).sum()),
                      int((m & (pa >= t) & ~(pb >= t)).sum()), int((m & (pa >= t) & (pb >= t)).sum())]
            tot, mm, uu = int(H[k, 0].sum()), int(H[k, 0, t:].sum()), int(H[k, 1, :t].sum())
            mu = int(H[k, 2, t:].sum()) - mm
            assert [uu, tot - mm - uu - mu, mu, mm] == direct, (t, k)


def _stats(uu, um, mu, mm):
    from hifimeth_amd.pileup import LINKAGE_DTYPE, linkage_stats
    w = np.zeros(1, LINKAGE_DTYPE)
    w["n_uu"], w["n_um"], w["n_mu"], w["n_mm"] = uu, um, mu, mm
    return linkage_stats(w[0])


def test_linkage_stats_exact_values():
    assert _stats(3, 0, 0, 5) == (1.0, 1.0) and _stats(0, 4, 9, 0) == (0.0, -1.0)
    assert _stats(2, 2, 2, 2) == (0.5, 0.0)
    for c in ((7, 0, 0, 0), (0, 0, 0, 7), (3, 4, 0, 0), (0, 0, 4, 3), (3, 0, 4, 0), (0, 4, 0, 3)):   # a margin is 0
        conc, r = _stats(*c)
        assert math.isnan(r) and conc == (c[0] + c[3]) / 7
    from hifimeth_amd.pileup import linkage_tsv, LINKAGE_DTYPE
    rows = np.zeros(3, LINKAGE_DTYPE)
    rows["dist"] = (5, 6, 7)
    rows["n_uu"], rows["n_um"], rows["n_mu"], rows["n_mm"] = (3, 7, 0), (2, 0, 0), (3, 0, 0), (1, 0, 0)
    assert linkage_tsv(rows) == R.tsv_text([(5, 3, 2, 3, 1), (6, 7, 0, 0, 0), (7, 0, 0, 0, 0)])
    assert linkage_tsv(rows).splitlines()[2:] == ["6\t7\t7\t0\t0\t0\t1\tnan", "7\t0\t0\t0\t0\t0\tnan\tnan"]


def test_linkage_stats_against_the_formulas():
    """Against the direct formulas on Python ints.  The concordance is one rounded division of exact integers.  r's numerator is an
    exact integer rounded once on either side; the denominator is four factors below 2^53 multiplied and rooted (three roundings
    and a half), against Python's correctly rounded root of the exact product: a few 2^-53 relative in all, far below 1e-12 --
    also where mm * uu and mu * um agree in their leading digits, which is what the exact numerator is for"""
    rng = np.random.default_rng(4205)
    for trial in range(400):
        hi = int((1, 3, 50, 100000, 2 ** 31, 2 ** 40)[trial % 6])
        c = [int(x) for x in rng.integers(0, hi + 1, 4)]
        if trial % 5 == 0:                                                  # nearly independent: the numerator cancels
            c = [c[0], c[1], c[0] + int(rng.integers(0, 3)), c[1] + int(rng.integers(0, 3))]
        if not sum(c):
            continue
        got, want = _stats(*c), R.stats(*c)
        assert abs(got[0] - want[0]) <= 1e-12 * abs(want[0]), (c, got, want)
        assert (math.isnan(got[1]) and math.isnan(want[1])) or abs(got[1] - want[1]) <= 1e-12 * abs(want[1]), (c, got, want)
        assert 0.0 <= got[0] <= 1.0 and (math.isnan(got[1]) or -1.0 - 1e-12 <= got[1] <= 1.0 + 1e-12)


def test_linkage_stats_refuses_what_is_no_row():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import LINKAGE_DTYPE
    L = lib()
    out = np.zeros(2)
    w = np.zeros(1, LINKAGE_DTYPE)
    assert w.itemsize == 40
    assert L.hm_linkage_stats(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == HM_EINVAL   # n == 0
    assert L.hm_linkage_stats(None, out.ctypes.data_as(ctypes.c_void_p)) == HM_EINVAL
    w["n_um"] = 1
    assert L.hm_linkage_stats(w.ctypes.data_as(ctypes.c_void_p), None) == HM_EINVAL
    assert L.hm_linkage_stats(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == 0 and out[0] == 0.0


def test_cli_refusals(tmp_path):
    """usage errors come before the device is touched: -z without -L, -L outside 2 .. 16 384 or not a number, -z below 0"""
    for args in (["-z", "3"], ["-L", "1"], ["-L", "16385"], ["-L", "0"], ["-L", "x"], ["-L", "12.5"], ["-L", "100", "-z", "-1"],
                 ["-L", "100", "-z", "x"]):
        r = subprocess.run([CLI, "pileup", *args, str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"), str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "ERROR: -" in r.stderr and "-L" in r.stderr.split("\n")[0], (args, r.stderr[:300])
    assert not os.listdir(tmp_path)
    r = subprocess.run([CLI, "pileup"], capture_output=True, text=True, timeout=60)
    assert "-L <bp>" in r.stderr + r.stdout and "-z <int>" in r.stderr + r.stdout
