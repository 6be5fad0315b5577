"""The fit of `pileup -D`'s two levels (`-D -Y`) without a GPU: hm_domain_refit against the plain division and clamp, the stop rule
of the package's DomainFit and of the restatement in domains_fit_ref.py on crafted histories, the restatement's fit of a synthetic
two-level track, the text of <prefix>.domains.fit.tsv, the three symbols and the usage errors of the front ends."""
import ctypes
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from domains_fit_ref import (EPS, HM_EDATA, HM_EINVAL, HM_OK, TRACK_LEVELS, fit, fit_chains, fit_tsv, lib_refit, lib_scores, refit_py,
                             synthetic_track)

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
X, Y = (10, 90, 5, 80, 20, 5), (20, 80, 5, 70, 30, 5)          # sums whose levels are 0.1 : 0.8 and 0.2 : 0.7


def test_symbols_and_abi_version():
    from hifimeth_amd._lib import HM_ABI_VERSION, lib
    L = lib()
    assert HM_ABI_VERSION == 5 and L.hm_abi_version() == 5
    assert {"hm_pileup_domain_sums", "hm_pileup_domain_sums_part", "hm_domain_refit"} <= set(L._hm_symbols)
    header = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    assert all(f" {name}(" in header for name in ("hm_pileup_domain_sums", "hm_pileup_domain_sums_part", "hm_domain_refit"))


def test_refit_equals_the_division_and_clamp():
    from hifimeth_amd.pileup import domain_refit
    cases = [X, Y, (1, 2, 1, 2, 1, 1), (7, 13, 3, 29, 2, 9), (123456, 7654321, 99, 7654321, 123456, 77),
             (0, 1, 1, 1, 0, 1),                                                                # both levels clamp
             ((1 << 33) + 1, (1 << 35) + 7, 5, (1 << 36) + 3, (1 << 33) + 5, 5),                # sums beyond 2^32
             ((1 << 45) + 1, (1 << 47) + 3, 1 << 27, (1 << 47) + 11, (1 << 44) + 1, 1 << 27)]
    for sums in cases:
        want = refit_py(sums)
        assert want is not None and lib_refit(sums, 8.0) == (HM_OK, *want) and domain_refit(sums, 8.0) == want, sums
    assert lib_refit(X, 8.0)[1:] == (0.1, 0.8) and lib_refit((1, 2, 1, 2, 1, 1), 0.0)[1:] == (1 / 3, 2 / 3)


def test_refit_clamps_at_one_millionth():
    for sums, want in [((0, 50, 5, 50, 0, 5), (EPS, 1 - EPS)), ((1, 10 ** 7, 5, 10 ** 7, 1, 5), (EPS, 1 - EPS)),
                       ((1, 999998, 5, 1, 1, 2), (1 / 999999, 0.5)), ((1, 10 ** 6, 5, 1, 1, 2), (EPS, 0.5)),
                       ((1, 1, 2, 999999, 1, 5), (0.5, min(999999 / 10 ** 6, 1 - EPS)))]:
        assert refit_py(sums) == want and lib_refit(sums, 8.0) == (HM_OK, *want), sums
    assert 1 / 999999 > EPS > 1 / (10 ** 6 + 1)


def test_refit_ends_the_fit():
    from hifimeth_amd.pileup import HifimethError, domain_refit
    for sums in [(0, 0, 0, 80, 20, 5), (10, 90, 5, 0, 0, 0), (0, 0, 0, 0, 0, 0),            # an empty state
                 (80, 20, 5, 10, 90, 5), (50, 50, 5, 50, 50, 5), (1, 1, 1, 2, 2, 3),          # l' >= h'
                 (0, 9, 1, 0, 7, 1), (9, 0, 1, 7, 0, 1),                                      # both clamp to the same end
                 (10 ** 12, 10 ** 12 + 1, 5, 10 ** 12 + 1, 10 ** 12, 5)]:                     # l' < h', but a weight rounds to 0
        rc, lo, hi = lib_refit(sums, 8.0)
        assert rc == HM_EDATA and lo != lo and hi != hi, sums                               # the levels are untouched
        assert domain_refit(sums, 8.0) is None
    l2, h2 = refit_py((10 ** 12, 10 ** 12 + 1, 5, 10 ** 12 + 1, 10 ** 12, 5))
    assert l2 < h2 and lib_scores(l2, h2, 8.0) is None
    from hifimeth_amd._lib import lib
    d = ctypes.c_double(0.0)
    ok = (ctypes.c_int64 * 6)(*X)
    assert lib().hm_domain_refit(None, 8.0, ctypes.byref(d), ctypes.byref(d)) == HM_EINVAL
    assert lib().hm_domain_refit(ok, 8.0, None, ctypes.byref(d)) == HM_EINVAL and lib().hm_domain_refit(ok, 8.0, ctypes.byref(d), None) == HM_EINVAL
    assert lib().hm_domain_refit(ok, -1.0, ctypes.byref(d), ctypes.byref(d)) == HM_EINVAL
    assert lib().hm_domain_refit(ok, float("nan"), ctypes.byref(d), ctypes.byref(d)) == HM_EINVAL
    assert lib().hm_domain_refit((ctypes.c_int64 * 6)(10, 90, 5, 80, -20, 5), 8.0, ctypes.byref(d), ctypes.byref(d)) == HM_EINVAL
    with pytest.raises(HifimethError):
        domain_refit((10, 90, 5, 80, -20, 5), 8.0)


# ---- the stop rule on crafted histories: sums_of is a table over (A, B) ---------------------------------------------------------------
def _both(sums_of, lo, hi, penalty, max_iter):
    """the restatement and the package's iteration agree -> (lo, hi, status, history)"""
    from hifimeth_amd.pileup import fit_levels
    calls = []

    def logged(A, B, S):
        calls.append((A, B, S))
        return sums_of(A, B, S)
    want = fit(sums_of, lo, hi, penalty, max_iter)
    got = fit_levels(logged, lo, hi, penalty, max_iter)
    assert got == want and [c[:2] for c in calls] == [h[3:5] for h in want[3]] and {c[2] for c in calls} == {lib_scores(lo, hi, penalty)[2]}
    return want


def test_stop_rule_fixed_point():
    r = _both(lambda A, B, S: X, 0.3, 0.6, 8.0, 10)
    AX, BX, _ = lib_scores(0.1, 0.8, 8.0)
    assert r[:3] == (0.1, 0.8, "converged") and [h[:5] for h in r[3]] == [(0, 0.3, 0.6, *lib_scores(0.3, 0.6, 8.0)[:2]), (1, 0.1, 0.8, AX, BX)]
    assert _both(lambda A, B, S: X, 0.1, 0.8, 8.0, 10)[:3] == (0.1, 0.8, "converged")       # started on it: one iteration
    assert len(_both(lambda A, B, S: X, 0.1, 0.8, 8.0, 10)[3]) == 1
    # levels that differ from the start's, with the start's weights: converged, and the result is the start
    lo = 0.1 * (1 + 2 ** -40)
    assert lib_scores(lo, 0.8, 8.0) == (AX, BX, 8 << 16)
    assert _both(lambda A, B, S: X, lo, 0.8, 8.0, 10)[:3] == (lo, 0.8, "converged")


def test_stop_rule_two_cycle_entered_at_either_member():
    sx, sy = lib_scores(0.1, 0.8, 8.0)[:2], lib_scores(0.2, 0.7, 8.0)[:2]
    assert sy < sx                                            # 0.2 : 0.7 has the smaller (A, B)

    def sums_of(A, B, S):                                     # under 0.1 : 0.8 the data say 0.2 : 0.7 and the reverse
        return Y if (A, B) == sx else X
    at_x, at_y, far = (_both(sums_of, *start, 8.0, 10) for start in ((0.1, 0.8), (0.2, 0.7), (0.3, 0.6)))
    assert at_x[:3] == at_y[:3] == far[:3] == (0.2, 0.7, "cycle")
    assert [len(r[3]) for r in (at_x, at_y, far)] == [2, 2, 3]
    # entered next to a member: start levels with the scores of 0.2 : 0.7 that are not 0.2 : 0.7 -- the result is the cycle's
    lo = 0.2 * (1 + 2 ** -40)
    assert lib_scores(lo, 0.7, 8.0)[:2] == sy
    assert _both(sums_of, lo, 0.7, 8.0, 10)[:3] == (0.2, 0.7, "cycle")
    # a 3-cycle: the smallest (A, B) wherever it is entered
    Z = (30, 70, 5, 60, 40, 5)
    sz = lib_scores(0.3, 0.6, 8.0)[:2]
    assert sz < sy

    def three(A, B, S):
        return {sx: Y, sy: Z, sz: X}[A, B]
    for start in ((0.1, 0.8), (0.2, 0.7), (0.3, 0.6)):
        r = _both(three, *start, 8.0, 10)
        assert r[:3] == (0.3, 0.6, "cycle") and len(r[3]) == 3


def test_stop_rule_max_iter_one_state_and_degenerate():
    sx = lib_scores(0.1, 0.8, 8.0)[:2]
    r = _both(lambda A, B, S: X, 0.3, 0.6, 8.0, 1)
    assert r[:3] == (0.1, 0.8, "max_iter") and len(r[3]) == 1
    assert _both(lambda A, B, S: X, 0.1, 0.8, 8.0, 1)[:3] == (0.1, 0.8, "converged")         # convergence is looked at first
    chain = {lib_scores(0.3, 0.6, 8.0)[:2]: X, sx: Y, lib_scores(0.2, 0.7, 8.0)[:2]: (25, 75, 5, 65, 35, 5)}
    r = _both(lambda A, B, S: chain[A, B], 0.3, 0.6, 8.0, 3)
    assert r[:3] == (0.25, 0.65, "max_iter") and [h[1:3] for h in r[3]] == [(0.3, 0.6), (0.1, 0.8), (0.2, 0.7)]
    r = _both(lambda A, B, S: X if (A, B) != sx else (100, 900, 50, 0, 0, 0), 0.3, 0.6, 8.0, 10)
    assert r[:3] == (0.1, 0.8, "one_state") and len(r[3]) == 2
    assert _both(lambda A, B, S: (0, 0, 0, 0, 0, 0), 0.3, 0.6, 8.0, 10)[:3] == (0.3, 0.6, "one_state")
    r = _both(lambda A, B, S: X if (A, B) != sx else (80, 20, 5, 10, 90, 5), 0.3, 0.6, 8.0, 10)
    assert r[:3] == (0.1, 0.8, "degenerate") and len(r[3]) == 2
    from hifimeth_amd.pileup import DomainFit, HifimethError
    with pytest.raises(HifimethError):
        DomainFit(0.6, 0.3, 8.0, 5)                           # the start levels are the caller's error
    with pytest.raises(ValueError):
        DomainFit(0.3, 0.6, 8.0, 0)


# ---- the synthetic track ------------------------------------------------------------------------------------------------------------
def test_reference_fit_recovers_the_two_levels():
    """a property of the restatement (and of hard EM), checked before anything is compared with it: from 0.3 : 0.6 the fit of the
    committed seed converges, and each level ends strictly nearer to the one the track was drawn at than it started"""
    chains, lengths = synthetic_track()
    assert len(chains) == 3 and sum(int((c["motif"] == 0).sum()) for c in chains) >= 20000
    assert all(c["gpos"][0] >= sum(lengths[:k]) and c["gpos"][-1] < sum(lengths[:k + 1]) for k, c in enumerate(chains))
    lo, hi, status, history = fit_chains(chains, 0, 0.3, 0.6, 8.0, 1000, 30)
    print("fit:", lo, hi, status, len(history), "iterations")
    assert status == "converged" and len(history) >= 2
    assert abs(lo - TRACK_LEVELS[0]) < abs(0.3 - TRACK_LEVELS[0]) and abs(hi - TRACK_LEVELS[1]) < abs(0.6 - TRACK_LEVELS[1])
    assert all(h[5][2] + h[5][5] == history[0][5][2] + history[0][5][5] for h in history)       # every iteration sums every row
    assert refit_py(history[-2][5]) == (lo, hi) and lib_scores(lo, hi, 8.0)[:2] == history[-1][3:5]


def test_fit_tsv_text():
    from hifimeth_amd.pileup import domains_fit_tsv
    fits = [(0.1, 0.8, "converged", [(0, 0.3, 0.6, 45426, -36675, X), (1, 0.1, 0.8, 136278, -98571, X)]), None,
            (1 / 3, 0.6, "one_state", [(0, 1 / 3, 0.6, 38521, -33475, (0, 0, 0, 1 << 40, 3, 9))])]
    want = ("CpG\t0\t0.29999999999999999\t0.59999999999999998\t45426\t-36675\t10\t90\t5\t80\t20\t5\n"
            "CpG\t1\t0.10000000000000001\t0.80000000000000004\t136278\t-98571\t10\t90\t5\t80\t20\t5\n"
            "CpG\tconverged\t0.10000000000000001\t0.80000000000000004\n"
            "CHH\t0\t0.33333333333333331\t0.59999999999999998\t38521\t-33475\t0\t0\t0\t1099511627776\t3\t9\n"
            "CHH\tone_state\t0.33333333333333331\t0.59999999999999998\n")
    assert domains_fit_tsv(fits) == want == fit_tsv(fits)
    from hifimeth_amd.pileup import parse_domain_levels
    assert parse_domain_levels("0.10000000000000001:0.80000000000000004,nan,0.33333333333333331:0.59999999999999998") == \
        [(0.1, 0.8), None, (1 / 3, 0.6)]                      # -u takes the file's levels back as they stand


def test_usage_errors(tmp_path):
    for args, why in [(["-Y", "5"], "-Y needs -D"), (["-D", "-Y", "0"], "integer >= 1"), (["-D", "-Y", "-3"], "integer >= 1"),
                      (["-D", "-Y", "2.5"], "integer >= 1"), (["-D", "-Y", "x"], "integer >= 1"), (["-Y", "0"], "-Y needs -D")]:
        r = subprocess.run([CLI, "pileup", *args, "ref.fa", "mod.bam", str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "USAGE" in r.stderr and why in r.stderr.split("USAGE")[0], args
    r = subprocess.run([CLI, "pileup", "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  -Y <n>\n" in r.stderr and "domains.fit.tsv" in r.stderr
    r = subprocess.run([CLI, "pileup", "-D", "-Y", "7", str(tmp_path / "no.fa"), str(tmp_path / "no.bam"), str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "USAGE" not in r.stderr and "7 iterations at most" in r.stderr and not os.listdir(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for args, why in [(["-Y", "5"], "-Y needs -D"), (["-D", "-Y", "0"], "integer >= 1")]:
        r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, "ref.fa", "mod.bam", str(tmp_path / "out")],
                           capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
        assert r.returncode == 2 and why in r.stderr, args
