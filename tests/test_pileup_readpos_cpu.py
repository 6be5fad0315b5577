"""`pileup -P` / `pileup -I` without a GPU: a known answer worked out by hand pins tests/readpos_ref.py (the reference of
test_gpu_pileup_readpos.py); the host-only statistics and TSV text; the struct layout; the usage errors of the command line and of
pileup_dist, which come before a device is touched."""
import ctypes
import os
import subprocess
import sys

import numpy as np

import readpos_ref as R
from conftest import ROOT

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_EINVAL = -1

# One chromosome of 35 bases and three records on it, each entry placed by hand (D = 4):
#   offset  0....5....0....5....0....5....0....
#   ref     TCGATCAGTTCATTGATACGATTCATTGGATTACG
# r1  forward, 20M at 0, L = 20: 5mC entries on C1 (200), C5 (100), C10 (50), C18 (255) and on G14 (10)
#       CpG  C1 G2        p = 1   d5 1  d3 18 -> 5' 1
#       CHG  C5 A6 G7     p = 5   d5 5  d3 14 -> interior
#       CHH  C10 A11 T12  p = 10               -> interior
#       CHH  T12 T13 G14  p = 14  d5 14 d3 5  -> interior   (the G of a reverse-strand CHH)
#       CpG  C18 G19      p = 18  d5 18 d3 1  -> 3' 1
# r2  reverse, 7M at 16, L = 7 < 2 D, odd: stored TACGATT, as sequenced AATCGTA, one entry on its middle base C3 (128)
#       CpG at reference 18: stored C2 G3, the called C is base 7 - 1 - 3 = 3: d5 3 = d3 3 -> the tie goes to 5' 3
# r3  reverse, 12M at 23, L = 12: stored CATTGGATTACG, as sequenced CGTAATCCAATG, entries on C0 (30), C6 (60), C7 (90), G11 (250)
#       CHH  stored C0 A1 T2  (reference strand C)  p = 11 - 0 = 11, the G of the read: d3 0 -> 3' 0
#       CHH  stored T2 T3 G4  (recorded at the G)   p = 11 - 4 = 7   d5 7 d3 4 = D -> interior
#       CHH  stored T3 G4 G5                        p = 11 - 5 = 6                 -> interior
#       CpG  stored C10 G11, the G the last stored base: p = 11 - 11 = 0 -> 5' 0
REF = [("chr", "TCGATCAGTTCATTGATACG" "ATT" "CATTGGATTACG")]
READS = [
    dict(flag=0, tid=0, pos=0, mapq=60, cigar=[("M", 20)], seq="TCGATCAGTTCATTGATACG", mm="C+m,0,0,0,0;G-m,2;", ml=[200, 100, 50, 255, 10]),
    dict(flag=16, tid=0, pos=16, mapq=60, cigar=[("M", 7)], seq="TACGATT", mm="C+m,0;", ml=[128]),
    dict(flag=16, tid=0, pos=23, mapq=60, cigar=[("M", 12)], seq="CATTGGATTACG", mm="C+m,0,0,0;G-m,1;", ml=[30, 60, 90, 250]),
]
THR = (128, 100, 60)
#         motif end dist n_m n_u sum_ml
WANT = [(0, 0, 0, 0, 1, 30),            # r3's CpG, 30 < 128
        (0, 0, 1, 1, 0, 200),           # r1 C1
        (0, 0, 3, 1, 0, 128),           # r2's middle base, 128 >= 128
        (0, 1, 1, 1, 0, 255),           # r1 C18
        (1, 2, 0, 1, 0, 100),           # r1 C5, 100 >= 100
        (2, 1, 0, 1, 0, 250),           # r3 G11
        (2, 2, 0, 2, 2, 210)]           # 50, 10 (r1) below 60; 90, 60 (r3) at or above


def test_known_answer():
    assert len(REF[0][1]) == 35 and all(REF[0][1][r["pos"]:r["pos"] + len(r["seq"])] == r["seq"] for r in READS)
    assert R.rows(READS, REF, 4, THR) == WANT
    every = R.rows(READS, REF, 4, THR, min_calls=0)
    assert len(every) == 3 * 9 and [r for r in every if r[3] + r[4]] == WANT
    assert [r[:3] for r in every[:9]] == [(0, 0, d) for d in range(4)] + [(0, 1, d) for d in range(4)] + [(0, 2, 0)]
    assert R.rows(READS, REF, 4, THR, min_calls=2) == WANT[-1:]
    assert sum(r[3] + r[4] for r in WANT) == sum(len(R.projected(r, REF)) for r in READS) == 10
    # another threshold moves calls between n_m and n_u and leaves sum_ml alone
    other = R.rows(READS, REF, 4, (129, 101, 0))
    assert [r[:3] + r[5:] for r in other] == [r[:3] + r[5:] for r in WANT]
    assert other[2][3:5] == (0, 1) and other[4][3:5] == (0, 1) and other[6][3:5] == (4, 0)


def test_known_answer_other_reach():
    """D = 1: only the first and the last base are end rows; D = 8 > L / 2 of every read: r2 (L = 7) has no interior"""
    one = R.rows(READS, REF, 1, THR)
    assert one == [(0, 0, 0, 0, 1, 30), (0, 2, 0, 3, 0, 583), (1, 2, 0, 1, 0, 100), (2, 1, 0, 1, 0, 250), (2, 2, 0, 2, 2, 210)]
    wide = {r[:3]: r[3:] for r in R.rows(READS, REF, 8, THR)}
    assert wide[(0, 0, 3)] == (1, 0, 128) and wide[(1, 0, 5)] == (1, 0, 100) and wide[(2, 1, 5)] == (1, 1, 70)
    assert wide[(2, 1, 4)] == (1, 0, 90) and (2, 0, 6) not in wide          # r3's C6: d5 6 > d3 5, it joins r1's G14 under 3' 5
    assert wide[(2, 2, 0)] == (0, 1, 50)                 # r1's C10 alone: d5 10, d3 9


def test_known_answer_trimmed():
    """-I deletes entries: 1:1 takes r3's first and last base, 2:2 also r1's C1 and C18, 0:2 only the 3' ones, 4:3 all of r2"""
    assert R.rows(READS, REF, 4, THR, trim=(1, 1)) == [WANT[1], WANT[2], WANT[3], WANT[4], WANT[6]]
    assert R.rows(READS, REF, 4, THR, trim=(2, 2)) == [WANT[2], WANT[4], WANT[6]]
    assert R.rows(READS, REF, 4, THR, trim=(0, 2)) == [WANT[0], WANT[1], WANT[2], WANT[4], WANT[6]]
    assert R.rows(READS, REF, 4, THR, trim=(3, 3)) == [WANT[2], WANT[4], WANT[6]]             # r2: p = 3 = n5 stays
    assert R.rows(READS, REF, 4, THR, trim=(4, 3)) == [WANT[4], WANT[6]]                      # r2: n5 + n3 = L
    assert R.rows(READS, REF, 4, THR, trim=(3, 4)) == [WANT[4], WANT[6]]                      # r2: p = 3 > L - 1 - 4
    assert R.rows(READS, REF, 4, THR, trim=(20, 0)) == []
    assert [len(R.surviving_entries(r, 1, 1)) for r in READS] == [5, 1, 2]
    gone = R.surviving_entries(READS[1], 4, 3)
    assert len(gone) == 1 and gone[0]["unmod_base"] == b"A" and gone.dtype.itemsize == 8     # the record stays in the input


def test_filters():
    lowq = [dict(READS[0], mapq=5)] + READS[1:]
    assert R.rows(lowq, REF, 4, THR, min_mapq=10) == [WANT[0], WANT[2], WANT[5], (2, 2, 0, 2, 0, 150)]
    secondary = [dict(READS[0], flag=256)] + READS[1:]
    assert R.rows(secondary, REF, 4, THR) == WANT                                              # a record of its own
    assert R.rows([dict(READS[0], flag=4)] + READS[1:], REF, 4, THR) == R.rows(lowq, REF, 4, THR, min_mapq=10)


def test_tsv_text_and_stats():
    from hifimeth_amd.pileup import READPOS_DTYPE, readpos_stats, readpos_tsv
    assert READPOS_DTYPE.itemsize == 40
    rows = np.zeros(len(WANT) + 1, READPOS_DTYPE)
    for i, w in enumerate(WANT):
        rows[i] = (w[0], w[1], w[2], 0, w[3], w[4], w[5])
    rows[-1] = (2, 2, 0, 0, 0, 0, 0)
    text = readpos_tsv(rows)
    assert text == R.tsv_text(WANT + [(2, 2, 0, 0, 0, 0)])
    assert text.splitlines() == ["#context\tend\tdist\tn\tn_m\tn_u\tpercent\tmean_ml", "CpG\t5p\t0\t1\t0\t1\t0\t30", "CpG\t5p\t1\t1\t1\t0\t100\t200",
                                 "CpG\t5p\t3\t1\t1\t0\t100\t128", "CpG\t3p\t1\t1\t1\t0\t100\t255", "CHG\tinterior\t0\t1\t1\t0\t100\t100",
                                 "CHH\t3p\t0\t1\t1\t0\t100\t250", "CHH\tinterior\t0\t4\t2\t2\t50\t52.5", "CHH\tinterior\t0\t0\t0\t0\tnan\tnan"]
    assert readpos_stats(rows[6]) == (50.0, 52.5)
    rng = np.random.default_rng(4301)
    for trial in range(200):                            # one rounded product and division of exact integers: the same double
        hi = int((1, 50, 10 ** 6, 2 ** 40)[trial % 4])
        n_m, n_u = int(rng.integers(0, hi + 1)), int(rng.integers(1, hi + 1))
        s = int(rng.integers(0, 255 * (n_m + n_u) + 1))
        w = np.zeros(1, READPOS_DTYPE)
        w["n_m"], w["n_u"], w["sum_ml"] = n_m, n_u, s
        got = readpos_stats(w[0])
        assert got == (100.0 * n_m / (n_m + n_u), s / (n_m + n_u)) and "%g" % got[0] == "%g" % (100.0 * n_m / (n_m + n_u))


def test_stats_refuse_what_is_no_row():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import READPOS_DTYPE
    L = lib()
    out = np.zeros(2)
    w = np.zeros(1, READPOS_DTYPE)
    assert L.hm_readpos_stats(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == HM_EINVAL   # n == 0
    assert L.hm_readpos_stats(None, out.ctypes.data_as(ctypes.c_void_p)) == HM_EINVAL
    w["n_u"] = 1
    assert L.hm_readpos_stats(w.ctypes.data_as(ctypes.c_void_p), None) == HM_EINVAL
    assert L.hm_readpos_stats(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == 0 and out[0] == 0.0


def test_header_layout(tmp_path):
    """hm_readpos_t as the header declares it is READPOS_DTYPE; no existing struct changed"""
    from hifimeth_amd.pileup import READPOS_DTYPE
    names = ["motif", "end", "dist", "reserved", "n_m", "n_u", "sum_ml"]
    args = ", ".join(["sizeof(hm_readpos_t)", "HM_ABI_VERSION", "HM_READPOS_5P", "HM_READPOS_3P", "HM_READPOS_INTERIOR"]
                     + [f"offsetof(hm_readpos_t, {n})" for n in names])
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hifimeth_hip.h"\nint main(void) { printf("' + "%zu %d %d %d %d" + " %zu" * len(names)
                   + '\\n", ' + args + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[:5] == [40, 5, 0, 1, 2]
    assert got[5:] == [READPOS_DTYPE.fields[n][1] for n in names]


def test_cli_refusals(tmp_path):
    """usage errors come before the device is touched: -y without -P, -P outside 1 .. 2048 or not a number, -y below 0, a -I that
    is not n5[:n3]"""
    for args in (["-y", "3"], ["-P", "0"], ["-P", "2049"], ["-P", "x"], ["-P", "12.5"], ["-P", "-4"], ["-P", "100", "-y", "-1"],
                 ["-P", "100", "-y", "x"], ["-I", "x"], ["-I", "-1"], ["-I", "3:"], ["-I", ":3"], ["-I", "3:-1"], ["-I", "1:2:3"],
                 ["-I", "2.5"], ["-I", "3:x"], ["-P", "10", "-I", ""]):
        r = subprocess.run([CLI, "pileup", *args, str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"), str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "ERROR: -" in r.stderr and "-P" in r.stderr.split("\n")[0], (args, r.stderr[:300])
    assert not os.listdir(tmp_path)
    r = subprocess.run([CLI, "pileup"], capture_output=True, text=True, timeout=60)
    assert all(t in r.stderr + r.stdout for t in ("-P <bp>", "-y <int>", "-I <n5>[:<n3>]"))


def test_pileup_dist_refusals(tmp_path):
    for args in (["-y", "3"], ["-P", "0"], ["-P", "2049"], ["-P", "8", "-y", "-1"], ["-I", "x"], ["-I", "1:2:3"], ["-I", "-1"], ["-I", "3:"]):
        r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"),
                            str(tmp_path / "out")], capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 2 and ("-P" in r.stderr or "-y" in r.stderr), (args, r.stderr[-300:])
    assert not os.listdir(tmp_path)


def test_bins_cover_every_position():
    """every p of every L lands in exactly one row, 5' and 3' mirror each other, and a tie is 5'"""
    for D in (1, 4, 7):
        for L in range(1, 4 * D + 3):
            got = [R.bin_of(p, L, D) for p in range(L)]
            assert all((e == 2 and d == 0) or (e in (0, 1) and 0 <= d < D) for e, d in got)
            for p, (e, d) in enumerate(got):
                q = L - 1 - p
                if p < q:
                    assert got[q] == ((1, d) if e == 0 else (2, 0)) and e != 1
                elif p == q:
                    assert (e, d) == ((0, p) if p < D else (2, 0))
