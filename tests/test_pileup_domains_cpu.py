"""Methylation domains (`pileup -D`) without a GPU: the restatement in domains_ref.py against exhaustive search, the scan form the
device uses against that restatement, hm_domain_scores, the BED text, the row layout and the usage errors of the CLI."""
import ctypes
import itertools
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from domains_ref import AFTER_BREAK, BEFORE_BREAK, DOMAIN_DTYPE, domains, emissions, path_score, switch_costs, viterbi

CLI = os.path.join(ROOT, "hifimeth_amd", "bin", "hifimeth-hip")
LOCUS_DTYPE = np.dtype([("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("motif", "<u4"), ("reserved", "<u4")])


def _loci(gpos, pcov, ncov, motif=0):
    rows = np.zeros(len(gpos), LOCUS_DTYPE)
    rows["gpos"], rows["pcov"], rows["ncov"], rows["motif"] = gpos, pcov, ncov, motif
    return rows


def _random_case(rng, R):
    """small weights and counts: ties of every kind are common"""
    A, B, S = int(rng.integers(1, 4)), -int(rng.integers(1, 4)), int(rng.integers(0, 7))
    max_gap = int(rng.integers(1, 4))
    gpos = np.cumsum(rng.integers(1, 6, R))
    return _loci(gpos, rng.integers(0, 4, R), rng.integers(0, 4, R)), A, B, S, max_gap


def test_reference_path_is_optimal_among_all_paths():
    rng = np.random.default_rng(2024)
    ties = 0
    for _ in range(1500):
        R = int(rng.integers(1, 11))
        loci, A, B, S, max_gap = _random_case(rng, R)
        r = loci[loci["pcov"] + loci["ncov"] > 0]
        e, cost = emissions(r["pcov"], r["ncov"], A, B), switch_costs(r["gpos"], S, max_gap)
        z = viterbi(e, cost)
        scores = [path_score(p, e, cost) for p in itertools.product((0, 1), repeat=len(r))]
        best = max(scores) if scores else 0
        assert path_score(z, e, cost) == best
        ties += scores.count(best) > 1
        segs, n = domains(loci, 0, A, B, S, max_gap)
        assert n == len(r) and int(segs["n_loci"].sum()) == n
        assert int(segs["pcov"].sum()) == int(r["pcov"].sum()) and int(segs["ncov"].sum()) == int(r["ncov"].sum())
    assert ties > 300                                         # the tie rule was exercised


# ---- the form the device computes: two scans over monoids ----------------------------------------------------
INF, CSAT = 1 << 62, 1 << 48
KEEP = 2


def _fwd_op(a, b):
    """x -> clamp(x + c, lo, hi): b after a, the sum saturated as DomFwd::op does"""
    c = a[0] + b[0]
    lo, hi = min(max(a[1] + b[0], b[1]), b[2]), min(max(a[2] + b[0], b[1]), b[2])
    assert abs(a[1] + b[0]) < 1 << 63 and abs(a[2] + b[0]) < 1 << 63 and abs(c) < 1 << 63        # what int64 holds
    if c >= CSAT:
        c, lo = CSAT, hi
    elif c <= -CSAT:
        c, hi = -CSAT, lo
    return (c, lo, hi)


def _bwd_op(a, b):
    return b if b != KEEP else a


def _scan(items, op, identity, cuts):
    """the inclusive scan computed block-wise: blocks reduced, the aggregates scanned, every block scanned again from its carry"""
    edges = [0] + sorted(cuts) + [len(items)]
    carry, out = identity, []
    for a, b in zip(edges, edges[1:]):
        run, agg = carry, identity
        for x in items[a:b]:
            agg = op(agg, x)                                  # the reduce pass never sees the carry
            run = op(run, x)
            out.append(run)
        carry = op(carry, agg)
    return out


def _scan_states(e, cost, cuts_f, cuts_b):
    R = len(e)
    if R == 0:
        return []
    f = _scan([(e[t], e[t] - cost[t], e[t] + cost[t]) for t in range(R)], _fwd_op, (0, -INF, INF), cuts_f)
    d = [min(max(c, lo), hi) for c, lo, hi in f]
    code = [1 if d[t] > cost[t + 1] else 0 if d[t] < -cost[t + 1] else KEEP for t in range(R - 1)] + [1 if d[-1] > 0 else 0]
    return _scan(code[::-1], _bwd_op, KEEP, cuts_b)[::-1]


def test_scan_form_equals_the_reference_under_every_partition():
    rng = np.random.default_rng(7)
    for _ in range(600):
        R = int(rng.integers(1, 40))
        loci, A, B, S, max_gap = _random_case(rng, R)
        r = loci[loci["pcov"] + loci["ncov"] > 0]
        e, cost = emissions(r["pcov"], r["ncov"], A, B), switch_costs(r["gpos"], S, max_gap)
        want = viterbi(e, cost)
        for _k in range(3):
            cuts = [sorted(set(int(x) for x in rng.integers(0, len(e) + 1, int(rng.integers(0, 6))))) for _j in range(2)]
            assert _scan_states(e, cost, *cuts) == want


def test_scan_form_with_saturating_sums():
    """counters at the clamp and weights at their bounds: the sum of e passes +-2^48 within 20 rows, in both directions, and comes back"""
    rng = np.random.default_rng(11)
    big = (1 << 20) + 5
    for trial in range(60):
        R = 120
        pc, nc = np.zeros(R, np.int64), np.zeros(R, np.int64)
        kind = rng.integers(0, 4, R // 20).repeat(20)        # runs of 20: all methylated, all unmethylated, small, small
        pc[kind == 0], nc[kind == 1] = big, big
        small = kind >= 2
        pc[small], nc[small] = rng.integers(0, 3, small.sum()), rng.integers(0, 3, small.sum())
        gpos = np.cumsum(rng.integers(1, 4, R))
        A, B, S = 1 << 24, -(1 << 24), int(rng.choice([0, 1, 1 << 24]))
        loci = _loci(gpos, pc, nc)
        r = loci[loci["pcov"] + loci["ncov"] > 0]
        e, cost = emissions(r["pcov"], r["ncov"], A, B), switch_costs(r["gpos"], S, 2)
        assert max(abs(x) for x in e) <= 1 << 45
        want = viterbi(e, cost)
        for cuts in ([], [len(e) // 2], list(range(0, len(e), 7)), [int(x) for x in rng.integers(0, len(e), 5)]):
            assert _scan_states(e, cost, cuts, cuts[::2]) == want, trial


# ---- segments --------------------------------------------------------------------------------------------------------------------
def test_segments_by_hand():
    A, B, S = 3, -3, 4
    #        high high | gap 6 > 5: break | high, low low low (e = -9 < -S), another context inside, an uncovered and a negative locus
    loci = _loci([10, 12, 18, 20, 21, 22, 23, 24, 25], [5, 5, 5, 0, 9, 0, 0, -1, 0], [0, 0, 0, 3, 9, 0, 3, 9, 3], [0, 0, 0, 0, 1, 0, 0, 0, 3])
    segs, R = domains(loci, 0, A, B, S, 5)
    assert R == 5
    assert [tuple(int(g[f]) for f in ("start", "end", "n_loci", "state", "flags", "pcov", "ncov")) for g in segs] == [
        (10, 13, 2, 1, AFTER_BREAK | BEFORE_BREAK, 10, 0), (18, 19, 1, 1, AFTER_BREAK, 5, 0), (20, 24, 2, 0, BEFORE_BREAK, 0, 6)]
    assert [float(x) for x in segs["level"]] == [100.0, 100.0, 0.0] and [float(x) for x in segs["score"]] == [30 / 65536, 15 / 65536, -18 / 65536]
    chh, R2 = domains(loci, 2, A, B, S, 5)                    # key low bits 3 count as CHH
    assert R2 == 1 and int(chh[0]["start"]) == 25 and int(chh[0]["motif"]) == 2
    assert domains(loci, 1, A, B, S, 5)[1] == 1
    assert len(domains(loci[:0], 0, A, B, S, 5)[0]) == 0
    # under a switch penalty no evidence outweighs, everything linked is one segment, of the state the sum favours
    one, _ = domains(_loci([1, 2, 3, 4], [9, 0, 0, 9], [0, 5, 5, 0]), 0, 1, -1, 1000, 5)
    assert len(one) == 1 and int(one[0]["state"]) == 1 and int(one[0]["flags"]) == AFTER_BREAK | BEFORE_BREAK
    # a tie at the end is low, and a tie at a break keeps the state of the right-hand side
    tie, _ = domains(_loci([1, 2], [1, 1], [1, 1]), 0, 2, -2, 1, 5)
    assert [int(s) for s in tie["state"]] == [0]
    brk, _ = domains(_loci([1, 50], [1, 4], [1, 0]), 0, 2, -2, 1, 5)
    assert [int(s) for s in brk["state"]] == [1, 1] and [int(f) for f in brk["flags"]] == [AFTER_BREAK | BEFORE_BREAK] * 2


# ---- the C library's host-only part ------------------------------------------------------------------------------------------------
def _llround(x):
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def test_domain_scores():
    from hifimeth_amd.pileup import DOMAIN_LEVELS, DOMAIN_MAX_GAP, DOMAIN_PENALTY, HifimethError, domain_scores
    assert DOMAIN_LEVELS == ((0.1, 0.8), (0.05, 0.5), (0.02, 0.2)) and (DOMAIN_PENALTY, DOMAIN_MAX_GAP) == (8.0, 1000)
    for lo, hi in DOMAIN_LEVELS:
        want = (_llround(65536 * math.log(hi / lo)), _llround(65536 * math.log((1 - hi) / (1 - lo))), 8 * 65536)
        assert domain_scores(lo, hi, 8.0) == want and domain_scores(lo, hi) == want
        assert 0 < want[0] <= 1 << 24 and -(1 << 24) <= want[1] < 0
    assert domain_scores(0.1, 0.8, 8.0) == (136278, -98571, 524288)
    assert domain_scores(0.3, 0.6, 0.0)[2] == 0 and domain_scores(0.3, 0.6, 256.0)[2] == 1 << 24
    nan = float("nan")
    bad = [(0.0, 0.5, 1), (-0.1, 0.5, 1), (0.5, 0.5, 1), (0.6, 0.5, 1), (0.5, 1.0, 1), (0.5, 1.5, 1), (nan, 0.5, 1), (0.2, nan, 1),
           (0.2, 0.8, -1e-9), (0.2, 0.8, nan), (0.2, 0.8, float("inf")), (0.2, 0.8, 256.001),
           (1e-120, 0.5, 1),                                  # A beyond 2^24 (B cannot pass -2^24: 1 - hi >= 2^-53)
           (0.5, 0.5 + 1e-12, 1)]                             # A rounds to 0
    for args in bad:
        with pytest.raises(HifimethError):
            domain_scores(*args)
    from hifimeth_amd._lib import lib
    a = ctypes.c_int64(0)
    assert lib().hm_domain_scores(0.1, 0.8, 8.0, None, ctypes.byref(a), ctypes.byref(a)) == -1      # HM_EINVAL


def test_domains_bed_text():
    from hifimeth_amd.pileup import DOMAIN_AFTER_BREAK, DOMAIN_BEFORE_BREAK, DOMAIN_DTYPE as D, domains_bed
    assert D == DOMAIN_DTYPE and D.itemsize == 64 and (DOMAIN_AFTER_BREAK, DOMAIN_BEFORE_BREAK) == (AFTER_BREAK, BEFORE_BREAK)
    rows = np.zeros(3, D)
    rows["start"], rows["end"], rows["n_loci"], rows["state"], rows["motif"] = [5, 100, 130], [61, 101, 140], [20, 1, 4], [1, 0, 1], [0, 0, 2]
    rows["pcov"], rows["ncov"] = [70, 1, 12345678], [30, 2, 1]
    rows["level"] = [70.0, 100 / 3, 100.0 * 12345678 / 12345679]
    rows["score"] = [1.5, -0.123456789, 1234567.891]
    text = domains_bed(rows, ["chrA", "chrB"], [0, 100, 200])
    assert text == {"CpG": "chrA\t5\t61\t20\tH\t70\t70\t30\t1.5\nchrB\t0\t1\t1\tL\t33.3333\t1\t2\t-0.123457\n",
                    "CHG": "", "CHH": "chrB\t30\t40\t4\tH\t100\t12345678\t1\t1.23457e+06\n"}


def test_row_layout_matches_header(tmp_path):
    src = tmp_path / "t.c"
    names = list(DOMAIN_DTYPE.names)
    fmt = " ".join(["%zu"] + ["%u"] * 2 + ["%d"] + ["%zu"] * len(names)) + "\\n"
    args = ", ".join(["sizeof(hm_domain_t)", "HM_DOMAIN_AFTER_BREAK", "HM_DOMAIN_BEFORE_BREAK", "HM_ABI_VERSION"] + [f"offsetof(hm_domain_t, {n})" for n in names])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hifimeth_hip.h"\n'
                   f'int main(void) {{ printf("{fmt}", {args}); return 0; }}\n')
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "t")], text=True).split()]
    assert got == [64, AFTER_BREAK, BEFORE_BREAK, 5] + [DOMAIN_DTYPE.fields[n][1] for n in names]


def test_cli_usage_errors(tmp_path):
    bad = {"need -D": (["-u", "0.1:0.8"], ["-x", "8"], ["-j", "1000"], ["-H", "-j", "5"]),
           "0 < lo < hi < 1": (["-D", "-u", "0.8:0.1"], ["-D", "-u", "0:0.5"], ["-D", "-u", "0.5:1"], ["-D", "-u", "0.5"], ["-D", "-u", "0.1:0.8,0.1:0.8"],
                               ["-D", "-u", "0.1:0.8,0.1:0.8,0.1:0.8,0.1:0.8"], ["-D", "-u", "0.1:0.8x"], ["-D", "-u", "0.1:0.8,nan,0.3:"],
                               ["-D", "-u", "NaN:0.5"], ["-D", "-u", ""]),
           "[0, 256]": (["-D", "-x", "-1"], ["-D", "-x", "257"], ["-D", "-x", "nan"], ["-D", "-x", "8z"]),
           ">= 1": (["-D", "-j", "0"], ["-D", "-j", "-4"], ["-D", "-j", "2.5"], ["-D", "-j", "7b"])}
    for why, cases in bad.items():
        for args in cases:
            r = subprocess.run([CLI, "pileup", *args, "ref.fa", "mod.bam", str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
            assert r.returncode != 0 and "USAGE" in r.stderr and why in r.stderr.split("USAGE")[0], args
    r = subprocess.run([CLI, "pileup", "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and all(x in r.stderr for x in ("  -D\n", "  -u <lo:hi[,lo:hi,lo:hi]>\n", "  -x <nats>\n", "  -j <bp>\n", "domains.<ctx>.bed",
                                                             "Default: 0.1:0.8,0.05:0.5,0.02:0.2", "nobody has tuned them on data"))
    # values that parse get past the options: the run then fails on the missing reference, not on usage
    r = subprocess.run([CLI, "pileup", "-D", "-u", "nan,0.2:0.7,nan", "-x", "0", "-j", "1", str(tmp_path / "no.fa"), str(tmp_path / "no.bam"),
                        str(tmp_path / "out")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "USAGE" not in r.stderr and "domains: levels nan,0.2:0.7,nan, switch penalty 0 nats, loci linked up to 1 bases" in r.stderr
    assert not os.listdir(tmp_path)
