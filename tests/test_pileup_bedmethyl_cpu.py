"""`pileup -M` without a GPU: the textbook restatement (tests/bedmethyl_ref.py) on hand-made alignments with the expected classes
written out by hand, the inputs of the GPU test checked for the rule each is named for, the new symbol and its binding, and the
command line's refusals, which come before any device is opened."""
import ctypes
import os
import subprocess

import bedmethyl_cases as K
import bedmethyl_ref as R
from conftest import ROOT

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")


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
    cls = lambda rec, **kw: {g: c for (_s, g), c in R.classes(rec, CHRS, **kw).items()}
    assert cls(_rec(0, [("M", 28)], CHR, [200, 10, 128, 127])) == {2: ("member", 200), 7: ("member", 10), 12: ("member", 128), 25: ("member", 127)}
    # the call at 7 dropped: C+m,0,1,0 skips the second C
    nocall = dict(_rec(0, [("M", 28)], CHR, [200, 10, 128, 127]), mm="C+m,0,1,0;", ml=[200, 128, 127])
    assert cls(nocall) == {2: ("member", 200), 7: "nocall", 12: ("member", 128), 25: ("member", 127)}
    # D over 6 .. 9 removes C and G of 7; D over 12 only the C; N over 25, 26
    rec = _rec(0, [("M", 6), ("D", 4), ("M", 2), ("D", 1), ("M", 12), ("N", 2), ("M", 1)], CHR[:6] + CHR[10:12] + CHR[13:25] + CHR[27:], [200])
    assert cls(rec) == {2: ("member", 200), 7: "delete", 12: "delete"}
    # mismatch at the C of 2 and at the G of 8; an insertion between C and G of 12; the alignment ends on the C of 25
    rec = _rec(0, [("M", 2), ("X", 1), ("M", 5), ("X", 1), ("M", 4), ("I", 2), ("M", 13)],
               CHR[:2] + "T" + CHR[3:8] + "T" + CHR[9:13] + "AA" + CHR[13:26], [200, 200, 200])
    assert cls(rec) == {2: "diff", 7: "diff", 12: "diff", 25: "end"}
    # D removes the G of 7 only: diff; the alignment begins on the G of 2: nothing there
    rec = _rec(3, [("M", 5), ("D", 1), ("M", 19)], CHR[3:8] + CHR[9:], [200, 200, 200])
    assert cls(rec) == {7: "diff", 12: ("member", 200), 25: ("member", 200)}
    # the filters
    low = _rec(0, [("M", 28)], CHR, [1, 2, 3, 4], mapq=3)
    assert len(cls(low)) == 4 and cls(low, min_mapq=5) == {}
    assert cls(dict(low, flag=4)) == {} and cls(dict(low, mm=None, ml=None)) == {}
    recs = [_rec(0, [("M", 28)], CHR, [200, 10, 128, 127]), nocall, low]
    assert R.counters(recs, CHRS, thr=128)[0] == {(0, 2): [2, 1, 0, 0, 0], (0, 7): [0, 2, 1, 0, 0], (0, 12): [2, 1, 0, 0, 0], (0, 25): [0, 3, 0, 0, 0]}
    assert R.counters(recs, CHRS, thr=128, hps=[1, 2, 0])[1] == {(0, 2): [1, 0, 0, 0, 0], (0, 7): [0, 1, 0, 0, 0], (0, 12): [1, 0, 0, 0, 0], (0, 25): [0, 1, 0, 0, 0]}
    rows = R.rows(recs, CHRS, thr=128, min_valid=3)
    assert rows == [(2, 2, 1, 0, 0, 0), (12, 2, 1, 0, 0, 0), (25, 0, 3, 0, 0, 0)]
    assert R.bed_text(rows[:1], CHRS) == "c\t2\t3\tm\t3\t.\t2\t3\t255,0,0\t3\t66.67\t2\t1\t0\t0\t0\t0\t0\n"
    assert R.bed_text([(7, 0, 0, 1, 2, 3)], CHRS) == "c\t7\t8\tm\t0\t.\t7\t8\t255,0,0\t0\t0.00\t0\t0\t0\t3\t0\t2\t1\n"


def test_gpu_inputs_hold_their_cases():
    g = K.genome()
    assert tuple(map(tuple, R.reference_cpgs(g))) == (K.CHR1, K.CHR2, K.CHR3)
    assert g[0][1][-1] == "C" and g[1][1][0] == "G" and g[0][1][200:203] == "CGG" and g[2][1][-2:] == "CG"
    reads = {r.name: r for r in K.reads()}
    cls = lambda n, **kw: {s: c for (_t, s), c in R.classes(K.as_dict(reads[n]), g, **kw).items()}
    kind = lambda n, **kw: {s: (c[0] if isinstance(c, tuple) else c) for s, c in cls(n, **kw).items()}
    M = "member"
    for t in "fr":
        assert cls("A_eq_" + t) == {100: (M, K.THR), 104: (M, K.THR - 1), 110: (M, 255), 120: (M, 0)}
        assert kind("A_nocall110_" + t) == {100: M, 104: M, 110: "nocall", 120: M}
        for n in ("A_mmC104_", "A_mmG105_", "A_ins_", "A_delG_", "A_skipG_"):
            assert kind(n + t) == {100: M, 104: "diff", 110: M, 120: M}, n
        assert kind("A_delC_" + t) == kind("A_delCG_" + t) == {100: M, 104: "delete", 110: M, 120: M}
        assert kind("A_del3_" + t) == {100: "delete", 104: "delete", 110: "delete", 120: M}
        assert kind("A_skipCG_" + t) == {100: M, 110: M, 120: M}
        assert kind("A_mix_" + t) == kind("A_clip_" + t) == kind("A_secondary_" + t) == {100: M, 104: M, 110: M, 120: M}
        assert kind("A_endC_" + t) == kind("A_endC_I_" + t) == {100: M, 104: M, 110: "end"}
        assert kind("A_endC_I_more_" + t) == {100: M, 104: M, 110: "diff", 120: M}
        assert kind("A_beginG_" + t) == {110: M, 120: M}
        assert kind("A_noentries_" + t) == {}
        assert kind("A_mapq10_" + t, min_mapq=20) == {} and kind("A_lowid_" + t, min_pi=97.0) == {} and len(kind("A_lowid_" + t)) == 4
        assert kind("cgg_" + t) == {200: M, 300: M}
        assert kind("c1end_" + t) == {1400: M} and kind("c2_" + t) == {150: M} and kind("c3end_" + t) == {498: M}
        assert kind("c2del_" + t) == {250: "delete"}
        assert kind("c3del_" + t) == {50: "delete", 60: "delete", 75: "delete", 90: "delete"}
    assert kind("unmapped") == {} and kind("head") == {0: M}
    assert kind("long_nocall") == {s: ("nocall" if s in (1023, 1030) else M) for s in K.CHR1}
    assert kind("long_mmG448") == {s: ("diff" if s == 447 else M) for s in K.CHR1}
    # the reverse read on the reference CGG leaves a CHG record at 200 next to its CpG record
    from oracle import pileup_oracle as P
    recs = P.read_contribution(K.as_dict(reads["cgg_r"]), g)[1]
    assert sorted(m for _t, s, _p, m in recs if s == 200) == [0, 1]
    # the filters change the result
    rs = [K.as_dict(r) for r in K.reads()]
    assert R.rows(rs, g, K.THR, 0) != R.rows(rs, g, K.THR, 0, min_mapq=20, min_pi=97.0)
    dg, dr = K.dense()
    assert len(R.reference_cpgs(dg)[0]) == 5000
    d = R.classes(K.as_dict(dr[2]), dg)
    assert sum(1 for c in d.values() if c == "delete") == 1500 and d[(0, 3500)] == "diff"
    assert sum(1 for c in R.classes(K.as_dict(dr[3]), dg).values() if c == "nocall") == 500
    assert sum(1 for c in R.classes(K.as_dict(dr[4]), dg).values() if c == "diff") == 80


def test_classes_add_up_per_record():
    """over the reference CpGs whose C is a match column of a record that takes part: members + nocall + diff + the one the
    alignment may end on -- every such CpG has exactly one of them, and a deleted C is never a match column"""
    for genome, reads in ((K.genome(), K.reads()), K.dense()):
        cpgs = R.reference_cpgs(genome)
        for r in reads:
            rec = K.as_dict(r)
            c = R.classes(rec, genome)
            if not R.takes_part(rec, genome):
                assert c == {}
                continue
            match, deleted, _last = R.walk(rec)
            on_match = [g for g in cpgs[r.tid] if g in match]
            n = {k: 0 for k in ("member", "nocall", "diff", "end", "delete")}
            for (_s, g), v in c.items():
                n[v[0] if isinstance(v, tuple) else v] += 1
                assert (g in match) != (v == "delete")
            assert n["member"] + n["nocall"] + n["diff"] + n["end"] == len(on_match), r.name
            assert n["end"] <= 1 and n["delete"] == sum(1 for g in cpgs[r.tid] if g in deleted)


def test_symbol_and_binding():
    from hifimeth_amd import _lib
    from hifimeth_amd.pileup import BEDMETHYL_DTYPE
    L = _lib.lib()
    fn = L.hm_pileup_fetch_bedmethyl
    assert fn.restype is ctypes.c_int64
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64]
    assert BEDMETHYL_DTYPE.itemsize == 32
    assert fn(None, 0, 0, 1, 1, None, 0) == -1        # HM_EINVAL: no engine


def test_cli_refuses_v_without_M_before_any_device(tmp_path):
    for args in (["-v", "3"], ["-M", "-v", "-1"], ["-M", "-v", "2x"], ["-M", "-v", ""]):
        r = subprocess.run([CLI, "pileup", *args, str(tmp_path / "no.fa"), str(tmp_path / "no.bam"), str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "-v" in r.stderr and "USAGE" in r.stderr and "-M" in r.stderr, args
        assert "no.bam" not in r.stderr and not os.listdir(tmp_path)       # neither input was opened, nothing written
