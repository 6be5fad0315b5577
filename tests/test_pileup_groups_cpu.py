"""`groupdiff` without a GPU: the restatement of tests/groups_ref.py checked against itself and against scipy, the library's symbols,
and E_ref -- the worst relative error of the float64 form of the statistic against mpmath at 50 digits -- measured over the hand-made
loci and the random data set that tests/test_gpu_pileup_groups.py loads.  The GPU tests take 8 x E_ref as their bar.

Measured here: E_ref = 8.2e-11 for D, 2.5e-14 for phi, 5.4e-11 for p (496 loci of the data set and 12 hand-made ones)."""
import os

import numpy as np
import pytest

import groups_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_header_and_python_names():
    from hifimeth_amd import pileup as P
    from hifimeth_amd._lib import lib
    L = lib()
    for name in ("hm_pileup_group_sample", "hm_pileup_load_sample_loci", "hm_pileup_fetch_groups", "hm_pileup_group_planes", "hm_group_qvalues"):
        assert hasattr(L, name), name
    assert P.GROUP_DTYPE.itemsize == 64
    for name in ("begin_sample", "load_sample_loci", "group_tests", "groups_bed"):
        assert hasattr(P.MethylationPileup, name), name
    assert callable(P.group_qvalues) and callable(P.groups_summary_tsv)
    header = open(os.path.join(ROOT, "include", "hifimeth_hip.h")).read()
    assert "more than two samples, replicates" not in header and "} hm_group_t;" in header


def test_host_qvalues_equal_the_restatement():
    """hm_group_qvalues needs no device: ties, three contexts, motif 3 with CHH, an empty context"""
    from hifimeth_amd.pileup import GROUP_DTYPE, group_qvalues
    rng = np.random.default_rng(5)
    rows = np.zeros(400, GROUP_DTYPE)
    rows["motif"] = rng.choice([0, 2, 3], 400)
    rows["pvalue"] = rng.choice(np.concatenate([rng.random(60), [1.0, G.DBL_MIN, 1e-300]]), 400)
    q, m = group_qvalues(rows)
    want, wm = G.bh(rows["pvalue"], rows["motif"])
    assert q.tobytes() == want.tobytes() and m.tolist() == wm and wm[1] == 0
    for c in (0, 2):                                          # equal p, equal q; q is monotone in p
        sel = np.minimum(rows["motif"], 2) == c
        order = np.argsort(rows["pvalue"][sel])
        assert (np.diff(q[sel][order]) >= 0).all()
        assert len({(a, b) for a, b in zip(rows["pvalue"][sel], q[sel])}) == len(set(rows["pvalue"][sel]))
    rows["pvalue"][7] = 0.0
    from hifimeth_amd.caller import HifimethError
    with pytest.raises(HifimethError):
        group_qvalues(rows)


def test_swapping_the_groups_negates_diff_and_keeps_the_rest():
    for name, s in G.cases().items():
        d, D, phi, p = G.stat_f64(*s)
        sd, sD, sphi, sp = G.stat_f64(*(s[4:] + s[:4]))
        assert sd == -d and (sD, sphi, sp) == (D, phi, p), name


def test_planes_do_not_depend_on_the_order():
    data = G.dataset()
    base = G.dataset_loader()
    rng = np.random.default_rng(2)
    keys = sorted(data)
    for _ in range(2):
        ref = G.GroupLoader(G.TOTAL, G.MIN_COV)
        for k in rng.permutation(len(keys)):                  # the samples in any order, each in two calls of shuffled rows
            g, _s = keys[k]
            rows = data[keys[k]]
            order = rng.permutation(len(rows[0]))
            cut = len(order) // 3
            assert ref.begin_sample(g) >= 0
            for part in (order[:cut], order[cut:]):
                assert ref.load(*(x[part] for x in rows)) >= 0
        for name in base.planes:
            assert (ref.planes[name] == base.planes[name]).all(), name
        for g in (1, 2):
            assert (ref.moment[g] == base.moment[g]).all() and (ref.samples[g] == base.samples[g]).all()


def test_loader_rules():
    ref = G.GroupLoader(100, 5)
    assert ref.load([1], [3], [3], [0]) == G.HM_ESTATE and ref.begin_sample(3) == G.HM_EINVAL
    assert ref.begin_sample(1) == 0
    assert ref.load([1, 2, 3, 2], [3, 1, 0, 0], [3, 1, 0, 0], [0, 1, 1, 1]) == 1      # 2 is below the coverage, 3 and the second 2 have no count
    assert ref.begin_sample(1) == 1 and ref.load([1, 2], [6, 9], [0, 0], [2, 0]) == 2  # the same loci in another sample
    assert ref.sums(1)[:4] == (9, 12, ((9 << 20) // 6) + (36 << 20) // 6, 2) and ref.planes["key"][1] == 2 and ref.samples[1][2] == 1
    assert ref.begin_sample(2) == 0
    assert ref.load([100, 5, 6, 7, 2, 2], [1, -1, G.LIMIT, 1, 1, 1], [1, 1, 0, 1, 1, 1], [0, 0, 0, 4, 0, 0]) == G.HM_EDATA
    assert list(ref.bad.values()) == [1, 1, 1, 1, 1]          # 2 is seen although it is below the coverage: its second row is a duplicate
    assert ref.load([9], [5], [5], [0]) == G.HM_ESTATE and ref.begin_sample(1) == G.HM_ESTATE
    full = G.GroupLoader(10, 1)
    assert [full.begin_sample(2) for _ in range(256)] == list(range(255)) + [G.HM_ESTATE]


def test_f_tail_agrees_with_betainc():
    from scipy.special import betainc
    from scipy.stats import f as fdist
    for nu in (1, 2, 3, 4, 7, 50, 254, 508):
        for F in (1e-8, 0.3, 1.0, 4.5, 30.0, 1e3, 1e6):
            a, b = fdist.sf(F, 1, nu), betainc(nu / 2, 0.5, nu / (nu + F))
            assert abs(a - b) <= 1e-12 * b, (nu, F, a, b)


def test_phi_is_one_when_the_samples_of_a_group_agree():
    rng = np.random.default_rng(9)
    for _ in range(200):
        groups = []
        for _g in range(2):
            k0, n0 = int(rng.integers(0, 9)), int(rng.integers(1, 9))
            k0 = min(k0, n0)
            groups.append([(k0 * f, n0 * f) for f in rng.integers(1, 6, int(rng.integers(2, 5))).tolist()])     # one proportion, any coverage
        s = G.sums_of(*groups)
        assert G.stat_f64(*s)[2] == 1.0 and G.stat_mp(*s)[1] == 1


def test_hand_made_loci():
    import mpmath as mp
    refs = G.references()
    for name in ("D = 0", "D = 0 with spread", "both groups at 0"):
        (_d, D, _phi, p), (mD, _mphi, mp_) = refs[name]
        assert D == 0.0 and p == 1.0 and mD == 0 and mp_ == 1, name
    assert refs["D = 0 with spread"][0][2] > 1.0 and refs["D = 0"][0][2] == 1.0
    for name in ("group 1 at 0", "group 1 at 1", "near 2^20, all methylated against none"):
        (d, D, phi, p), (mD, mphi, mp_) = refs[name]
        assert np.isfinite([d, D, phi, p]).all() and D > 0 and 0 < p < 1 and G.rel(D, mD) < 1e-12 and G.rel(p, mp_) < 1e-9, name
    assert abs(refs["group 1 at 0"][0][0]) == 100.0 * 12 / 22 and refs["group 1 at 1"][0][0] == 100.0 - 100.0 * 9 / 30
    assert G.cases()["nu = 1"][3] + G.cases()["nu = 1"][7] - 2 == 1
    (_d, _D, _phi, p), (_mD, _mphi, mp_) = refs["nu = 1"]
    with mp.workdps(50):                                      # nu = 1: the Cauchy tail, p = 1 - (2 / pi) atan(sqrt(F))
        F = refs["nu = 1"][1][0] / refs["nu = 1"][1][1]
        assert abs(mp_ - (1 - 2 / mp.pi * mp.atan(mp.sqrt(F)))) < mp.mpf(10) ** -40
    s = G.cases()["near 2^20 per sample"]
    assert s[1] == 2 * G.BIG and s[2] < 1 << 41 and refs["near 2^20 per sample"][0][2] >= 1.0
    near, below = refs["p near DBL_MIN"], refs["p below DBL_MIN"]
    assert G.DBL_MIN <= near[1][2] < 1e-306 and G.rel(near[0][3], near[1][2]) < 1e-9
    assert below[1][2] < G.DBL_MIN and below[0][3] == G.DBL_MIN
    assert refs["overdispersed, nu = 4"][0][2] > 1.0 and refs["many samples, overdispersed"][0][2] > 1.0


def test_the_data_set_holds_what_the_gpu_tests_need():
    ref = G.dataset_loader()
    refs = G.references()
    tested = {r: ref.tested(r) for r in (1, 2, 3)}
    phi = [refs["locus %d" % row[0]][1][1] for row in tested[2]]
    assert sum(x > 1 for x in phi) >= 50 and sum(x == 1 for x in phi) >= 50
    rows = [np.concatenate([v[i] for v in G.dataset().values()]) for i in range(3)]
    low = (rows[1] + rows[2] > 0) & (rows[1] + rows[2] < G.MIN_COV)
    assert low.sum() >= 50                                    # rows dropped by -a
    assert len(tested[1]) > len(tested[2]) > len(tested[3]) >= 50      # loci dropped by -r
    for r in (1, 2, 3):
        assert set(G.ENDS) <= {row[0] for row in tested[r]}
    assert {row[1] for row in tested[2]} == {0, 1, 2, 3}


def test_measure_e_ref():
    """prints the figures DESIGN.md section 10 quotes; the float64 form is a reference, so all it has to be is close"""
    e = G.e_ref()
    print("E_ref over %d loci: D %.3g, phi %.3g, p %.3g" % (len(G.cases()), e["D"], e["phi"], e["p"]))
    assert 0 < e["D"] < 1e-8 and 0 < e["phi"] < 1e-12 and 0 < e["p"] < 1e-8


def test_usage_of_the_command():
    import subprocess
    cli = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
    r = subprocess.run([cli, "groupdiff", "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "groupdiff [OPTIONS] reference a1,a2,... b1,b2,... output-prefix" in r.stderr
    assert [x.strip() for x in r.stderr.splitlines() if x.startswith("  -")] == ["-a <int>", "-r <int>", "-t <CPU threads>", "-d <int>"]
    for args, text in ((["-r", "0", "f", "a", "b", "o"], "-r an integer in [1, 255]"), (["-a", "0", "f", "a", "b", "o"], "-a must be an integer"),
                       (["-Q", "f", "a", "b", "o"], "unrecognised option -Q\n")):
        r = subprocess.run([cli, "groupdiff", *args], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and text in r.stderr, (args, r.stderr[:200])
    r = subprocess.run([cli, "groupdiff", "f", "a,b", "c", "o"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "group 2 has 1 samples, fewer than -r 2" in r.stderr
    top = subprocess.run([cli], capture_output=True, text=True, timeout=60).stderr
    assert "groupdiff [OPTIONS] reference a1,a2,... b1,b2,... output-prefix" in top
