"""Host side of `pileup -H -A` (no GPU): the exact Fisher reference that the GPU tests compare against, checked against scipy;
the text of <prefix>.asm.<ctx>.bed; the command lines' argument errors, which are decided before any device call."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_pileup_asm import fisher_exact, fisher_weights

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")


def test_exact_reference_by_hand():
    assert fisher_exact(1, 0, 0, 1) == 1
    assert fisher_exact(3, 0, 0, 3) == Fraction(2, 20)                    # C(6, 3) = 20 tables' weight, the two corners
    assert fisher_exact(3, 1, 1, 3) == Fraction(2 * (1 + 16), 70)         # w = 1, 16, 36, 16, 1
    assert fisher_exact(5, 5, 5, 5) == 1
    assert fisher_exact(2, 3, 0, 0) == 1                                  # an empty row: one table
    assert fisher_weights(3, 1, 1, 3) == (0, [1, 16, 36, 16, 1], 70)
    assert fisher_weights(4, 0, 3, 1)[0] == 3                             # c1 = 7 > r2 = 4: the first cell starts at 3
    assert fisher_exact(2000, 0, 0, 2000) < Fraction(1, 10 ** 1200)
    with pytest.raises(AssertionError):                                   # band_check refuses a weight on the band edge
        import test_gpu_pileup_asm as T
        orig = T.fisher_weights
        T.fisher_weights = lambda *t: (0, [10 ** 7, 10 ** 7 + 1, 10 ** 9], 10 ** 9 + 2 * 10 ** 7 + 1)
        try:
            T.fisher_exact(0, 1, 1, 1, band_check=True)
        finally:
            T.fisher_weights = orig


def test_exact_reference_against_scipy():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(7)
    worst = 0.0
    for t in rng.integers(0, 61, (3000, 4)).tolist() + [[40, 0, 0, 40], [0, 0, 3, 4], [17, 17, 17, 17]]:
        if t[0] + t[1] == 0 and t[2] + t[3] == 0:
            continue
        want = float(fisher_exact(*t))
        got = stats.fisher_exact([[t[0], t[1]], [t[2], t[3]]])[1]
        worst = max(worst, abs(got - want) / want)
    assert worst < 1e-10, worst


def test_asm_bed_text():
    from hifimeth_amd.pileup import ASM_DTYPE, MethylationPileup
    assert ASM_DTYPE.itemsize == 48 and ASM_DTYPE.fields["diff"][1] == 32 and ASM_DTYPE.fields["pvalue"][1] == 40
    pu = MethylationPileup.__new__(MethylationPileup)                     # formatting needs names and offsets only
    pu.names = ["chrA", "chrB"]
    pu.offsets = np.array([0, 100, 250], np.int64)
    pu._h = None
    rows = np.zeros(6, ASM_DTYPE)
    rows["gpos"] = [3, 99, 100, 101, 249, 7]
    rows["motif"] = [0, 1, 2, 0, 0, 0]
    for k, t in enumerate([(5, 5, 5, 5), (1, 7, 6, 2), (9, 0, 0, 9), (2000, 0, 0, 2000), (1, 2, 3, 3), (7, 3, 8, 1)]):
        rows["pcov1"][k], rows["ncov1"][k], rows["pcov2"][k], rows["ncov2"][k] = t
    rows["diff"] = [0.0, -62.5, 100.0, 100.0, 100.0 / 3 - 50.0, 70.0 - 800.0 / 9]
    rows["pvalue"] = [1.0, 0.040559440559440559, 4.113533525298231e-05, 2.2250738585072014e-308, 1.0, 0.58204334365325072]
    text = pu.asm_bed(rows)
    assert text["CpG"] == ("chrA\t3\t4\t0\t1\t5\t5\t5\t5\n"
                           "chrB\t1\t2\t100\t2.22507e-308\t2000\t0\t0\t2000\n"
                           "chrB\t149\t150\t-16.6667\t1\t1\t2\t3\t3\n"
                           "chrA\t7\t8\t-18.8889\t0.582043\t7\t3\t8\t1\n")
    assert text["CHG"] == "chrA\t99\t100\t-62.5\t0.0405594\t1\t7\t6\t2\n"
    assert text["CHH"] == "chrB\t0\t1\t100\t4.11353e-05\t9\t0\t0\t9\n"
    assert pu.asm_bed(rows[:0]) == {"CpG": "", "CHG": "", "CHH": ""}


def test_cli_argument_errors_need_no_device(tmp_path):
    """-A without -H, -a without -A, -a 0: usage on stderr, EXIT_FAILURE, nothing created -- before a file or a device is opened"""
    for k, args in enumerate((["-A"], ["-a", "4"], ["-H", "-a", "4"], ["-H", "-A", "-a", "0"], ["-H", "-A", "-a", "-2"])):
        prefix = str(tmp_path / f"out{k}")
        r = subprocess.run([CLI, "pileup", *args, str(tmp_path / "no.fa"), str(tmp_path / "no.bam"), prefix],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 1, r.stderr
        assert "USAGE" in r.stderr and "ERROR" in r.stderr and "no HIP device" not in r.stderr and "no.bam" not in r.stderr
        assert os.listdir(tmp_path) == []
    r = subprocess.run([CLI, "pileup", "-A", "a", "b", "c"], capture_output=True, text=True, timeout=60)
    assert "-H" in r.stderr.split("USAGE")[0]
    r = subprocess.run([CLI, "pileup", "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "-A\n" in r.stderr and "-a <int>" in r.stderr and ".asm." in r.stderr


def test_pileup_dist_argument_errors_need_no_device(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    for args, word in ((["-A"], "-H"), (["-H", "-a", "3"], "-A"), (["-H", "-A", "-a", "0"], ">= 1")):
        r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, "no.fa", "no.bam", str(tmp_path / "o")],
                           capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
        assert r.returncode == 2 and word in r.stderr and "usage" in r.stderr, r.stderr
        assert os.listdir(tmp_path) == []
