"""`pileup -E` without a GPU: the textbook restatement (tests/patterns_ref.py) on hand-made alignments with the expected counts
written out by hand, the inputs of the GPU test checked for the conditions they are built for, and hm_pattern_stats -- host only --
against the direct formulas."""
import ctypes

import numpy as np

import patterns_cases as K
import patterns_ref as R

HM_EINVAL = -1


def _rec(pos, cigar, seq, ml, flag=0, mapq=60):
    """a forward record with one C+m call per C of `seq`, ML as given"""
    assert seq.count("C") == len(ml)
    return dict(flag=flag, tid=0, pos=pos, mapq=mapq, cigar=cigar, seq=seq, mm="C+m" + ",0" * len(ml) + ";", ml=list(ml))


#        0         1         2
#        0123456789012345678901234567
CHR = "ATCGATTCGAAACGTTTTTTTTTTTCGA"       # CpGs at 2, 7, 12, 25
CHRS = [("c", CHR)]


def test_restatement_on_hand_made_alignments():
    assert R.reference_cpgs(CHRS) == [[2, 7, 12, 25]]
    full = lambda ml: _rec(0, [("M", 28)], CHR, ml)
    recs = [full([200, 200, 10, 200]),                                                         # patterns 2->7: 11, 7->12: 10
            full([128, 127, 128, 0]),                                                          # 128 is methylated at thr 128
            _rec(0, [("M", 9), ("D", 2), ("M", 17)], CHR[:9] + CHR[11:], [200, 200, 200, 200]),  # deletion between 7 and 12: both kept
            _rec(0, [("M", 6), ("D", 4), ("M", 18)], CHR[:6] + CHR[10:], [200, 200, 200]),       # deletion over 7
            _rec(0, [("M", 7), ("X", 1), ("M", 20)], CHR[:7] + "T" + CHR[8:], [200, 200, 200]),  # mismatch at the C of 7
            _rec(0, [("M", 8), ("I", 1), ("M", 20)], CHR[:8] + "A" + CHR[8:], [200, 200, 200, 200]),  # run break inside CpG 7
            _rec(0, [("M", 13)], CHR[:13], [200, 200, 200]),                                   # ends on the C of 12
            _rec(0, [("M", 28)], CHR, [10, 10, 10, 10], mapq=3)]
    # k = 2, span 5: windows (2, 7) and (7, 12); (12, 25) is 13 wide
    w = R.windows(recs, CHRS, 2, max_span=5, thr=128)
    #                  00 10 01 11   (bit 0 = the left locus)
    assert w == {(0, 2): [1, 1, 0, 3],     # all but the del-over-7, mismatch and run-break records; rec 1 is 128, 127 -> 10; mapq 3 -> 00
                 (0, 7): [1, 1, 1, 1]}     # recs 0 (10), 1 (127, 128 -> 01), 2 (11), 7 (00); the one that ends on C of 12: not at 12
    assert R.windows(recs, CHRS, 2, max_span=4, thr=128) == {}
    w13 = R.windows(recs, CHRS, 2, max_span=13, thr=128)
    assert set(w13) == {(0, 2), (0, 7), (0, 12)} and sum(w13[(0, 12)]) == 7
    # the mapq filter takes the last record out
    assert R.windows(recs, CHRS, 2, max_span=5, thr=128, min_mapq=5)[(0, 7)] == [0, 1, 1, 1]
    # k = 3 at span 10: (2, 7, 12) only
    assert R.windows(recs, CHRS, 3, max_span=10, thr=128) == {(0, 2): [1, 0, 0, 1, 0, 1, 0, 1]}
    # thresholds 0 and 255
    assert R.windows(recs, CHRS, 2, max_span=5, thr=0)[(0, 2)] == [0, 0, 0, 5]
    assert R.windows(recs, CHRS, 2, max_span=5, thr=255)[(0, 2)] == [5, 0, 0, 0]
    rows = R.rows(recs, CHRS, 2, max_span=5, thr=128, min_reads=4)
    assert rows == [(2, 9, (1, 1, 0, 3) + (0,) * 12, 5, 2), (7, 14, (1, 1, 1, 1) + (0,) * 12, 4, 2)]
    assert R.rows(recs, CHRS, 2, max_span=5, thr=128, min_reads=5) == rows[:1]
    assert R.rows(recs, CHRS, 2, max_span=5, thr=128, min_reads=6) == []
    assert R.bed_text(rows[:1], CHRS) == "c\t2\t9\t5\t%.6g\t%.6g\t0.2\t70\t1,1,0,3\n" % (
        -(0.2 * np.log2(0.2) * 2 + 0.6 * np.log2(0.6)) / 2, 1 - 0.04 - 0.04 - 0.36)


def test_gpu_inputs_hold_their_cases():
    g = K.genome()
    assert tuple(map(tuple, R.reference_cpgs(g))) == (K.CHR1, K.CHR2, K.CHR3)
    assert g[0][1][-1] == "C" and g[1][1][0] == "G"
    reads = {r.name: r for r in K.reads()}
    mem = lambda n, **kw: {s for (_t, s) in R.member_loci(K.as_dict(reads[n]), g, **kw)}
    for t in "fr":
        assert mem("A_eq_" + t) == {100, 104, 110, 120}
        assert mem("A_del110_" + t) == {100, 104, 120}
        assert mem("A_mmC104_" + t) == mem("A_mmG105_" + t) == {100, 110, 120}
        assert mem("A_miss110_" + t) == {100, 104, 120}
        assert mem("A_ins_" + t) == {100, 104, 110, 120}
        assert mem("A_brk120_" + t) == {100, 104, 110}
        assert mem("A_end111_" + t) == {100, 104, 110} and mem("A_end110_" + t) == {100, 104}
        assert mem("A_clip_" + t) == mem("A_secondary_" + t) == {100, 104, 110, 120}
        assert mem("A_mapq10_" + t, min_mapq=20) == set() and mem("A_lowid_" + t, min_pi=97.0) == set()
        assert mem("A_lowid_" + t) == {100, 104, 110, 120}
        assert mem("span_" + t) == {300, 450, 601} and mem("c2_" + t) == {150}
        assert mem("c3end_" + t) == {498} and mem("c1end_" + t) == {1400}
    assert mem("long_f") == set(K.CHR1) and mem("unmapped") == set()
    eq = R.member_loci(K.as_dict(reads["A_eq_r"]), g)
    assert [eq[(0, s)] for s in (100, 104, 110, 120)] == [K.THR, K.THR - 1, 255, 0]
    # span exactly 150 and 151
    for k in (2, 3, 4):
        w = R.windows([K.as_dict(r) for r in K.reads()], g, k)
        assert ((0, 300) in w) == (k == 2) and (0, 450) not in w
        assert (0, 0) in w and (1, 150) not in w and ((2, 50) in w) and (2, 498) not in w
        assert (0, 1400) not in w


def _stats(counts, k):
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import PATTERN_DTYPE, pattern_stats
    w = np.zeros(1, PATTERN_DTYPE)
    w["counts"][0, :len(counts)] = counts
    w["n"], w["k"] = sum(counts), k
    return pattern_stats(w[0]), w, lib()


def test_pattern_stats_exact_values():
    import math
    for k in (2, 3, 4):
        for b in range(1 << k):
            c = [0] * (1 << k)
            c[b] = 7
            (ent, epi, pdr, lvl), _w, _L = _stats(c, k)
            assert ent == 0.0 and math.copysign(1.0, ent) == 1.0 and epi == 0.0
            assert (pdr == 0.0) == (b in (0, (1 << k) - 1)) and (pdr in (0.0, 1.0))
            assert lvl == 100.0 * bin(b).count("1") / k
    (ent, epi, pdr, lvl), _w, _L = _stats([3] * 16, 4)
    assert ent == 1.0 and epi == 1.0 - 16 * (1 / 16) ** 2 and pdr == 1.0 - 6 / 48 and lvl == 50.0


def test_pattern_stats_against_the_formulas():
    """Each value lies in [0, 100] and is at most ~50 rounded fp64 operations (2^k <= 16 terms of two or three each): the two
    implementations differ by far less than 50 * 100 * 2^-53 ~ 6e-13 < 1e-12"""
    rng = np.random.default_rng(4105)
    for trial in range(300):
        k = int(rng.integers(2, 5))
        hi = int((1, 3, 50, 100000, 2 ** 31)[trial % 5])
        c = [int(x) for x in rng.integers(0, hi + 1, 1 << k)]
        if trial % 7 == 0:
            c[int(rng.integers(0, 1 << k))] = 0
        if not sum(c) or sum(c) >= 2 ** 32:
            continue
        got, _w, _L = _stats(c, k)
        want = R.stats(c, k)
        assert all(abs(a - b) <= 1e-12 for a, b in zip(got, want)), (c, k, got, want)
        assert 0.0 <= got[0] <= 1.0 + 1e-12 and 0.0 <= got[1] < 1.0 and 0.0 <= got[2] <= 1.0 and 0.0 <= got[3] <= 100.0


def test_pattern_stats_refuses_what_is_no_window():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import PATTERN_DTYPE
    L = lib()
    out = np.zeros(4)
    w = np.zeros(1, PATTERN_DTYPE)
    w["counts"][0, :4] = (1, 2, 3, 4)
    for n, k, rc in ((10, 2, 0), (10, 1, HM_EINVAL), (10, 5, HM_EINVAL), (9, 2, HM_EINVAL), (10, 3, 0)):
        w["n"], w["k"] = n, k
        assert L.hm_pattern_stats(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == rc, (n, k)
    w["counts"][0, :] = 0
    w["n"], w["k"] = 0, 2
    assert L.hm_pattern_stats(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == HM_EINVAL
    assert L.hm_pattern_stats(None, out.ctypes.data_as(ctypes.c_void_p)) == HM_EINVAL
