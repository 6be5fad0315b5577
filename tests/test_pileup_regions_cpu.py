"""`pileup -R` / `pileup -J` without a GPU: hand-computed answers for the restatement (tests/regions_ref.py), the Python BED parser,
hm_region_stats, the header's layout, and the errors the command line reports before it touches a device."""
import ctypes
import gzip
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import regions_ref as R
from conftest import ROOT

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_EINVAL = -1

# Twelve loci, written out by hand.  locus: (pcov, ncov, context)
#  0 (1, 0, CpG)  ppm 1 000 000        1 (0, 0, -)  uncovered            2 (1, 2, CHG)  (2e6 + 3) / 6 = 333 333 (.8 down)
#  3 (2, 1, CHH)  (4e6 + 3) / 6 = 666 667 (.2: 666 666.67 rounds up)     4 (0, 3, CpG)  0
#  5 (1, 1, CpG)  500 000              6 (0, 0, -)                       7 (1, 3999999, CHG)  1/4e6 = 0.25 ppm -> 0
#  8 (1, 1999999, CHH)  1/2e6 = 0.5 ppm exactly -> rounds half UP to 1   9 (3, 0, CHH)  1 000 000
# 10 (0, 1, CHG)  0                   11 (1, 0, CpG)  1 000 000
PC = [1, 0, 1, 2, 0, 1, 0, 1, 1, 3, 0, 1]
NC = [0, 0, 2, 1, 3, 1, 0, 3999999, 1999999, 0, 1, 0]
KY = [0, 0, 1, 2, 0, 0, 3, 1, 2, 2, 1, 0]


def test_locus_ppm_rounds_half_up():
    assert [R.locus_ppm(p, n) for p, n in ((1, 0), (1, 2), (2, 1), (0, 3), (1, 1), (1, 3999999), (1, 1999999), (3, 1999997))] == \
        [1000000, 333333, 666667, 0, 500000, 0, 1, 2]
    big = 2 ** 31 - 1
    assert R.locus_ppm(big, big) == 500000 and R.locus_ppm(big, 0) == 1000000


def test_known_answer_regions():
    run = R.Running(PC, NC, KY)
    got = R.region_sums(run, [0, 0, 2, 1, 6, 8], [12, 5, 4, 2, 7, 9])
    assert got[0].tolist() == [[4, 3, 4, 2500000], [3, 2, 4000002, 333333], [3, 6, 2000000, 1666668]]   # everything
    assert got[1].tolist() == [[2, 1, 3, 1000000], [1, 1, 2, 333333], [1, 2, 1, 666667]]
    assert got[2].tolist() == [[0, 0, 0, 0], [1, 1, 2, 333333], [1, 2, 1, 666667]]
    assert not got[3].any() and not got[4].any()                                                          # uncovered loci only
    assert got[5].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [1, 1, 1999999, 1]]                            # the .5 ppm locus
    two = R.region_sums(R.Running(PC, NC, KY, min_cov=3), [0], [12])[0]
    assert two.tolist() == [[1, 0, 3, 0], [2, 2, 4000001, 333333], [3, 6, 2000000, 1666668]]              # loci 0, 5, 10, 11 fall out
    # a chunk's planes with a base, and the clamp: the two halves add up to the whole
    left = R.region_sums(R.Running(PC[:5], NC[:5], KY[:5]), [0, 2], [12, 9])
    right = R.region_sums(R.Running(PC[5:], NC[5:], KY[5:], base=5), [0, 2], [12, 9])
    assert (left + right == R.region_sums(run, [0, 2], [12, 9])).all()
    assert (R.region_sums(run, [0], [12], lo=2, hi=4)[0] == got[2]).all()


def test_known_answer_stats_and_text():
    w, m = R.stats(4, 3, 4, 2500000)
    assert w == 100.0 * 3 / 7 and m == 62.5
    assert all(math.isnan(x) for x in R.stats(0, 0, 0, 0))
    sums = R.region_sums(R.Running(PC, NC, KY), [0, 1], [12, 2])
    text = R.regions_text([("chrA", 0, 12, "all", "+"), ("chrA", 1, 2, ".", ".")], sums)
    assert text["CpG"] == ("#chrom\tstart\tend\tname\tstrand\tn_loci\tpcov\tncov\tweighted\tmean\n"
                           "chrA\t0\t12\tall\t+\t4\t3\t4\t42.8571\t62.5\nchrA\t1\t2\t.\t.\t0\t0\t0\tnan\tnan\n")
    assert text["CHH"].split("\n")[1] == "chrA\t0\t12\tall\t+\t3\t6\t2000000\t0.000299999\t55.5556"


def test_known_answer_metaplot():
    """one sequence [0, 12): an interval [4, 8) on +, the same on -, and one of 1 base that 2 bins leave out; flank 4 in 2 bins"""
    run = R.Running(PC, NC, KY)
    assert R.meta_edges(4, 8, 0, 12, 2, 4, 2) == [0, 2, 4, 6, 8, 10, 12]
    assert R.meta_edges(1, 11, 0, 12, 3, 4, 2) == [0, 0, 1, 4, 7, 11, 12, 12]       # floor(j 10 / 3); both flanks cut by the sequence
    assert R.meta_edges(5, 9, 4, 10, 2, 0, 0) == [5, 7, 9]
    tab, used = R.metaplot(run, [4], [8], [0], [12], "+", 2, 4, 2)
    assert used == 1 and tab[:, :, 0].tolist() == [[1] * 6] * 3
    assert tab[0, :, 1].tolist() == [1, 0, 2, 0, 0, 1] and tab[1, :, 1].tolist() == [0, 1, 0, 1, 0, 1] and tab[2, :, 1].tolist() == [0, 1, 0, 0, 2, 0]
    rev, _ = R.metaplot(run, [4], [8], [0], [12], "-", 2, 4, 2)
    assert (rev == tab[:, ::-1]).all()
    both, used = R.metaplot(run, [4, 4, 3], [8, 8, 4], [0, 0, 0], [12, 12, 12], "+-.", 2, 4, 2)
    assert used == 2 and (both == tab + rev).all()
    edge, _ = R.metaplot(run, [0], [4], [0], [12], ".", 2, 4, 2)                     # at the sequence start: no upstream bin has a width
    assert edge[0, :, 0].tolist() == [0, 0, 1, 1, 1, 1] and not edge[:, :2, 1:].any()
    text = R.metaplot_text(both, 2, 1, 2, 2)
    assert text["CpG"].startswith("#regions\t2\t1\n#bin\tpart\tn_regions\tn_loci\tpcov\tncov\tweighted\tmean\n0\tup\t2\t2\t2\t0\t100\t100\n")
    assert [ln.split("\t")[1] for ln in text["CHG"].split("\n")[2:8]] == ["up", "up", "body", "body", "down", "down"]


# ---- the BED parser ------------------------------------------------------------------------------------------------------------------
NAMES, LENGTHS = ["chr1", "chr2"], [100, 50]
GOOD = ("# a comment\ntrack name=x\nbrowser position chr1\n\nchr1\t0\t10\n"
        "chr2\t5\t50\tgeneB\t0\t-\nchr1\t99\t100\t\t0\t*\textra\r\nchr1\t3\t7\tg\t1\t+\n")


def _write(tmp_path, text, name="r.bed", gz=False):
    path = str(tmp_path / name)
    with (gzip.open(path, "wt") if gz else open(path, "w")) as f:
        f.write(text)
    return path


@pytest.mark.parametrize("gz", [False, True])
def test_parser_good(tmp_path, gz):
    from hifimeth_amd.pileup import parse_regions_bed
    r = parse_regions_bed(_write(tmp_path, GOOD, gz=gz), NAMES, LENGTHS)
    assert len(r) == 4 and r.sid.tolist() == [0, 1, 0, 0] and r.start.tolist() == [0, 5, 99, 3] and r.end.tolist() == [10, 50, 100, 7]
    assert r.name == [".", "geneB", ".", "g"] and r.strand == [".", "-", ".", "+"]
    c = r.coords([0, 100, 150])
    assert c["start"].tolist() == [0, 105, 99, 3] and c["end"].tolist() == [10, 150, 100, 7]
    assert c["seq_start"].tolist() == [0, 100, 0, 0] and c["seq_end"].tolist() == [100, 150, 100, 100] and c["strand"] == b".-.+"
    assert len(parse_regions_bed(_write(tmp_path, "#only\n\n", "e.bed"), NAMES, LENGTHS)) == 0


@pytest.mark.parametrize("line,what", [("chrX\t0\t5", "unknown sequence chrX"), ("chr1\t5\t5", "start >= end"), ("chr1\t7\t5", "start >= end"),
                                       ("chr1\t-1\t5", "start < 0"), ("chr2\t0\t51", "past the end"), ("chr1\t0", "fewer than 3"),
                                       ("chr1 0 5", "fewer than 3"), ("chr1\tx\t5", "integers"), ("chr1\t0\t5.0", "integers")])
def test_parser_bad(tmp_path, line, what):
    from hifimeth_amd.pileup import parse_regions_bed
    with pytest.raises(ValueError, match=r"r\.bed:3: .*" + what):
        parse_regions_bed(_write(tmp_path, "#c\nchr1\t0\t1\n" + line + "\n"), NAMES, LENGTHS)


def test_parse_metaplot():
    from hifimeth_amd.pileup import parse_metaplot
    assert parse_metaplot("20") == (20, 0, 0) and parse_metaplot("20:2000:10") == (20, 2000, 10) and parse_metaplot("1000:1000:1000") == (1000, 1000, 1000)
    for bad in ("0", "1001", "x", "20:2000", "20:2000:3", "20:0:2", "20:10:0", "20:2000:10:1", "-5", "2.5", "", "20:2000:1001", "20::"):
        with pytest.raises(ValueError):
            parse_metaplot(bad)


# ---- the C library's host-only parts -------------------------------------------------------------------------------------------------
def test_region_stats_and_geometry():
    from hifimeth_amd._lib import lib
    from hifimeth_amd.pileup import REGION_SUM_DTYPE, region_geometry, region_stats
    assert region_stats(dict(n_loci=4, pcov=3, ncov=4, ppm=2500000)) == (100.0 * 3 / 7, 62.5) == R.stats(4, 3, 4, 2500000)
    assert region_stats(dict(n_loci=3, pcov=6, ncov=2000000, ppm=1666668)) == R.stats(3, 6, 2000000, 1666668)
    big = 3 * (2 ** 31 - 1)
    assert region_stats(dict(n_loci=3, pcov=big, ncov=big, ppm=1500000)) == (50.0, 50.0)
    L, out = lib(), np.zeros(2)
    w = np.zeros(1, REGION_SUM_DTYPE)
    assert L.hm_region_stats(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)) == HM_EINVAL      # n_loci == 0
    assert L.hm_region_stats(None, out.ctypes.data_as(ctypes.c_void_p)) == HM_EINVAL
    w["n_loci"], w["pcov"] = 1, 1
    assert L.hm_region_stats(w.ctypes.data_as(ctypes.c_void_p), None) == HM_EINVAL
    B, part = region_geometry()
    assert B >= 256 and B & (B - 1) == 0 and part >= 2


def test_tsv_writers_equal_the_restatement():
    from hifimeth_amd.pileup import METABIN_DTYPE, REGION_SUM_DTYPE, Regions, metaplot_tsv, regions_tsv
    run = R.Running(PC, NC, KY)
    want = R.region_sums(run, [0, 1], [12, 2])
    sums = np.zeros((2, 3), REGION_SUM_DTYPE)
    for q, k in enumerate(R.QUANTITIES):
        sums[k] = want[:, :, q]
    reg = Regions([0, 0], [0, 1], [12, 2], ["all", "."], ["+", "."])
    assert regions_tsv(reg, ["chrA"], sums) == R.regions_text([("chrA", 0, 12, "all", "+"), ("chrA", 1, 2, ".", ".")], want)
    tab, used = R.metaplot(run, [4, 4, 3], [8, 8, 4], [0, 0, 0], [12, 12, 12], "+-.", 2, 4, 2)
    rows = np.zeros(18, METABIN_DTYPE)
    for c in range(3):
        for b in range(6):
            rows[c * 6 + b] = (c, b, *tab[c, b])
    assert metaplot_tsv(rows, used, 1, 2, 2) == R.metaplot_text(tab, used, 1, 2, 2)


def test_header_layout(tmp_path):
    """the two structs as the header declares them are the numpy mirrors; the ABI version stays"""
    from hifimeth_amd.pileup import METABIN_DTYPE, REGION_SUM_DTYPE, region_geometry
    fields = [("hm_region_sum_t", n) for n in REGION_SUM_DTYPE.names] + [("hm_metabin_t", n) for n in METABIN_DTYPE.names]
    args = ", ".join(["sizeof(hm_region_sum_t)", "sizeof(hm_metabin_t)", "(size_t)HM_ABI_VERSION", "(size_t)HM_REGION_BLOCK", "(size_t)HM_REGION_SCAN_BLOCKS"]
                     + [f"offsetof({t}, {n})" for t, n in fields])
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hifimeth_hip.h"\nint main(void) { printf("' + " %zu" * (5 + len(fields))
                   + '\\n", ' + args + "); return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got[:3] == [32, 48, 5] and tuple(got[3:5]) == region_geometry()
    assert got[5:] == [REGION_SUM_DTYPE.fields[n][1] for n in REGION_SUM_DTYPE.names] + [METABIN_DTYPE.fields[n][1] for n in METABIN_DTYPE.names]


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_cli_usage_errors(tmp_path):
    """-C or -J without -R, a -C below 1, a -J that is not bins[:flank:flank_bins]: before any file is opened"""
    bed = str(tmp_path / "r.bed")
    cases = [["-J", "20"], ["-C", "2"], ["-R", bed, "-C", "0"], ["-R", bed, "-C", "x"], ["-R", bed, "-J", "0"], ["-R", bed, "-J", "1001"],
             ["-R", bed, "-J", "20:2000"], ["-R", bed, "-J", "20:2000:3"], ["-R", bed, "-J", "20:0:4"], ["-R", bed, "-J", "20:100:0"],
             ["-R", bed, "-J", "x"], ["-R", bed, "-J", "20:2000:10:1"], ["-R", bed, "-J", "2.5"]]
    for args in cases:
        r = subprocess.run([CLI, "pileup", *args, str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"), str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "ERROR: -C" in r.stderr.split("\n")[0], (args, r.stderr[:300])
    assert not os.listdir(tmp_path)
    r = subprocess.run([CLI, "pileup"], capture_output=True, text=True, timeout=60)
    assert all(t in r.stderr + r.stdout for t in ("-R <bed>", "-C <int>", "-J <bins>[:<flank_bp>:<flank_bins>]"))


def test_cli_file_errors_need_no_device(tmp_path):
    """the intervals are read and checked once the reference is known and before the engine is made: every error names its line"""
    import pileup_cases as C
    from bamutil import aligned_to_bam, write_fasta
    fa, bam = str(tmp_path / "ref.fa"), str(tmp_path / "in.bam")
    write_fasta(fa, C.genome())
    aligned_to_bam(bam, C.genome(), C.boundaries()[:3])
    n = len(C.genome()[1][1])
    for line, what in (("chrX\t0\t5", "unknown sequence chrX"), (f"chr2\t0\t{n + 1}", "past the end of chr2"), ("chr1\t5\t5", "start >= end"),
                       ("chr1\t-2\t5", "start < 0"), ("chr1\t1", "fewer than 3"), ("chr1\ta\t9", "integers")):
        bed = _write(tmp_path, "#c\nchr1\t0\t1\n" + line + "\n")
        r = subprocess.run([CLI, "pileup", "-R", bed, "-d", "99", fa, bam, str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and f"ERROR: {bed}:3: " in r.stderr and what in r.stderr, (line, r.stderr[-400:])
    r = subprocess.run([CLI, "pileup", "-R", str(tmp_path / "none.bed"), "-d", "99", fa, bam, str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "none.bed" in r.stderr
    assert not [f for f in os.listdir(tmp_path) if f.startswith("out")]


def test_pileup_dist_refusals(tmp_path):
    for args in (["-J", "20"], ["-C", "2"], ["-R", "r.bed", "-C", "0"], ["-R", "r.bed", "-J", "20:2000:3"], ["-R", "r.bed", "-J", "0"]):
        r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, str(tmp_path / "ref.fa"), str(tmp_path / "in.bam"),
                            str(tmp_path / "out")], capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 2 and "-C" in r.stderr, (args, r.stderr[-300:])
    assert not os.listdir(tmp_path)
