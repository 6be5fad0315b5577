"""Host side of `pileup -H -A -Q` (no GPU): hm_asm_qvalues -- the one implementation of the Benjamini-Hochberg q-values of the
haplotype test -- against numpy BH over the expanded multiset of p-values (asm_q_ref.bh_numpy, the definition in the header
restated), bit for bit; its refusals; the structs' sizes; the summary's text and the command lines' argument errors, which are
decided before any device call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from asm_q_ref import ASM_BINS, ASM_DTYPE, BIN_DTYPE, DBL_MIN, bh_numpy, cases, expected, make_big, make_tab
from conftest import ROOT

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
HM_OK, HM_EINVAL = 0, -1


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def test_bh_numpy_by_hand():
    # m = 4: sorted p 0.01, 0.02, 0.02, 0.5 -> p m / R = 0.04, 0.08 / 3 (R = 3 for the tie), 0.5 * 4 / 4
    q = bh_numpy(np.array([0.02, 0.5, 0.01, 0.02]))
    assert q[2] == min(0.01 * 4.0 / 1.0, 0.02 * 4.0 / 3.0) and q[0] == q[3] == 0.02 * 4.0 / 3.0 and q[1] == 0.5
    assert (bh_numpy(np.array([1.0, 1.0, 1.0])) == 1.0).all()
    assert (bh_numpy(np.array([0.9, 0.8])) == [0.9, 0.9]).all()          # the running minimum from the largest p, capped at 1
    assert bh_numpy(np.array([DBL_MIN]))[0] == DBL_MIN and len(bh_numpy(np.zeros(0))) == 0


def test_structs_and_abi():
    from hifimeth_amd import pileup
    from hifimeth_amd._lib import lib
    assert pileup.ASM_BIN_DTYPE.itemsize == 32 and pileup.ASMQ_DTYPE.itemsize == 56 and pileup.ASM_DTYPE.itemsize == 48
    assert pileup.ASM_BIN_DTYPE == BIN_DTYPE and pileup.ASM_DTYPE == ASM_DTYPE
    assert pileup.ASMQ_DTYPE.names[:-1] == pileup.ASM_DTYPE.names and pileup.ASMQ_DTYPE.fields["qvalue"][1] == 48
    assert pileup.ASM_BINS == ASM_BINS == 12979200
    assert lib().hm_abi_version() == 5
    header = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    assert "#define HM_ABI_VERSION 5\n" in header and "#define HM_ASM_BINS 12979200 " in header


@pytest.mark.parametrize("name", list(cases()))
def test_qvalues_bit_equal_to_numpy_bh(name):
    from hifimeth_amd.pileup import asm_qvalues
    tab, big = cases()[name]
    want_tq, want_bq, want_m = expected(tab, big)
    t = asm_qvalues(tab, big)
    assert (t.m == want_m).all(), (t.m, want_m)
    assert (_bits(t.tab["qvalue"]) == _bits(want_tq)).all()
    assert (_bits(t.big_q) == _bits(want_bq)).all()
    assert not np.isnan(t.tab["qvalue"]).any() and not np.isnan(t.big_q).any()
    assert (t.tab["qvalue"] >= t.tab["pvalue"]).all() and (t.tab["qvalue"] <= 1.0).all()
    for f in ("bin", "count", "pvalue"):                     # nothing but qvalue is written
        assert (t.tab[f] == tab[f]).all()
    assert np.isnan(tab["qvalue"]).all()                     # ... and into a copy


def test_cases_hold_what_they_claim():
    c = cases()
    tab, big = c["mixed"]
    ctx = tab["bin"] // (2080 * 2080)
    assert set(ctx.tolist()) == {0, 2} and set(big["motif"].tolist()) == {0, 2, 3}           # CHG is empty, motif 3 counts as CHH
    assert (tab["count"] > 1).any() and (tab["pvalue"] == DBL_MIN).any() and (tab["pvalue"] == 1.0).any()
    assert (tab["pvalue"][ctx == 0] == 0.03).sum() == 3 and (big["pvalue"] == 0.03).sum() == 1
    _tq, _bq, m = expected(tab, big)
    assert m.tolist() == [1055 + 2, 0, 16 + 4]
    assert (c["all_one"][0]["pvalue"] == 1.0).all() and len(c["one_bin_locus"][0]) == 1 and len(c["one_big_locus"][1]) == 1
    rt, rb = c["random"]
    assert len(rt) > 2000 and len(np.unique(rt["pvalue"])) < 110 and rt["count"].max() == 1000 and len(rb) == 200
    assert (np.diff(rt["bin"].astype(np.int64)) > 0).all()


def _call(tab, big, sentinel=7.0):
    """hm_asm_qvalues on copies with every output pre-set to a sentinel -> (rc, tab, big_q, m)"""
    from hifimeth_amd._lib import lib
    tab = tab.copy()
    tab["qvalue"] = sentinel
    big_q = np.full(len(big), sentinel)
    m = np.full(3, 99, np.uint64)
    rc = lib().hm_asm_qvalues(tab.ctypes.data_as(C.c_void_p), len(tab), big.ctypes.data_as(C.c_void_p), len(big),
                              big_q.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p))
    return rc, tab, big_q, m


def test_refusals_leave_the_outputs_untouched():
    from hifimeth_amd.pileup import asm_qvalues
    from hifimeth_amd.caller import HifimethError
    tab, big = cases()["mixed"]
    rc, t, bq, m = _call(tab, big)
    assert rc == HM_OK and not (t["qvalue"] == 7.0).any() and not (bq == 7.0).any() and m.sum() == 1077

    def edit(a, i, field, v):
        a = a.copy()
        a[field][i] = v
        return a

    swapped = tab.copy()
    swapped[[2, 3]] = swapped[[3, 2]]
    bad = {
        "tab not ascending": (swapped, big),
        "a bin twice": (edit(tab, 4, "bin", tab["bin"][3]), big),
        "bin beyond the table": (edit(tab, len(tab) - 1, "bin", ASM_BINS), big),
        "count 0": (edit(tab, 5, "count", 0), big),
        "p = 0": (edit(tab, 1, "pvalue", 0.0), big),
        "p subnormal": (edit(tab, 1, "pvalue", DBL_MIN / 2), big),
        "p > 1": (edit(tab, 1, "pvalue", np.nextafter(1.0, 2.0)), big),
        "p NaN": (edit(tab, 1, "pvalue", np.nan), big),
        "p negative": (edit(tab, 1, "pvalue", -0.5), big),
        "big p NaN": (tab, edit(big, 0, "pvalue", np.nan)),
        "big p = 0": (tab, edit(big, 5, "pvalue", 0.0)),
        "big motif 4": (tab, edit(big, 2, "motif", 4)),
        "big row that is dense": (tab, edit(big, 0, "pcov1", 58)),
        "big negative counter": (tab, edit(big, 1, "ncov2", -1)),
    }
    for why, (t_in, b_in) in bad.items():
        rc, t, bq, m = _call(t_in, b_in)
        assert rc == HM_EINVAL, why
        assert (t["qvalue"] == 7.0).all() and (bq == 7.0).all() and (m == 99).all(), why
        with pytest.raises(HifimethError):
            asm_qvalues(t_in, b_in)
    # the edge that is still big: one total of exactly 64, the other small
    rc, _t, bq, _m = _call(make_tab([]), make_big([(63, 1, 0, 1, 0, 0.5), (0, 1, 0, 64, 1, 0.25)]))
    assert rc == HM_OK and not (bq == 7.0).any()


def test_summary_text():
    from hifimeth_amd.pileup import asm_qvalues, asm_summary_tsv
    tab, big = cases()["mixed"]
    t = asm_qvalues(tab, big)
    q = np.concatenate([np.repeat(t.tab["qvalue"], tab["count"].astype(np.int64)), t.big_q])
    ctx = np.concatenate([np.repeat(tab["bin"] // (2080 * 2080), tab["count"].astype(np.int64)), np.minimum(big["motif"], 2)])
    lines = asm_summary_tsv(t).splitlines()
    assert [x.split("\t")[0] for x in lines] == ["CpG", "CHG", "CHH"]
    for c, line in enumerate(lines):
        assert [int(x) for x in line.split("\t")[1:]] == [(ctx == c).sum(), ((ctx == c) & (q <= 0.05)).sum(), ((ctx == c) & (q <= 0.01)).sum()]
    assert lines[1] == "CHG\t0\t0\t0" and int(lines[0].split("\t")[2]) >= int(lines[0].split("\t")[3]) > 0


def test_asm_bed_tenth_column():
    """asm_bed is a function of the rows alone: the 56-byte dtype prints qvalue behind the nine columns, the 48-byte one is unchanged"""
    from hifimeth_amd.pileup import ASMQ_DTYPE, MethylationPileup
    pu = MethylationPileup.__new__(MethylationPileup)       # no engine: names and offsets are all asm_bed reads
    pu._h = None
    pu.names, pu.offsets = ["chrA", "chrB"], np.array([0, 100, 250])
    rows = np.zeros(3, ASMQ_DTYPE)
    rows["gpos"], rows["motif"] = [5, 100, 249], [0, 2, 1]
    rows["pcov1"], rows["ncov1"], rows["pcov2"], rows["ncov2"] = [5, 1, 0], [0, 6, 9], [0, 6, 9], [5, 1, 0]
    rows["diff"], rows["pvalue"], rows["qvalue"] = [100.0, -71.4285714, -100.0], [0.0079365079, 0.029137529, 4.1e-5], [0.0238, np.nan, 1.0]
    with_q = pu.asm_bed(rows)
    plain = pu.asm_bed(rows[[n for n in rows.dtype.names if n != "qvalue"]])
    assert with_q["CpG"] == "chrA\t5\t6\t100\t0.00793651\t5\t0\t0\t5\t0.0238\n"
    assert with_q["CHH"] == "chrB\t0\t1\t-71.4286\t0.0291375\t1\t6\t6\t1\tnan\n"
    assert with_q["CHG"] == "chrB\t149\t150\t-100\t4.1e-05\t0\t9\t9\t0\t1\n"
    for c in with_q:
        assert [x.rsplit("\t", 1)[0] for x in with_q[c].splitlines()] == plain[c].splitlines()


def test_usage_errors_before_any_device_call(tmp_path):
    """-Q without -A is refused while parsing, by both front ends; nothing is written"""
    for args in (["-Q"], ["-H", "-Q"]):
        r = subprocess.run([CLI, "pileup", *args, "ref.fa", "mod.bam", str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "USAGE" in r.stderr and "-Q needs -A" in r.stderr.split("USAGE")[0]
    r = subprocess.run([CLI, "pileup", "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  -Q\n" in r.stderr and "asm.summary.tsv" in r.stderr
    for args in (["-Q"], ["-H", "-Q"]):
        r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, "ref.fa", "mod.bam", str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=120, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 2 and "-Q needs -A" in r.stderr
    assert not os.listdir(tmp_path)
