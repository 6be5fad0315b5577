"""The fit of `pileup -D`'s two levels (`-D -Y`) on the device: hm_pileup_domain_sums[_part] over caller-owned crafted planes against
the textbook restatement (domains_fit_ref.py) AND against the sums read off hm_pileup_fetch_domains' segments, the pieces' sums
against the whole's, fit_domain_levels against the restatement's history, and `pileup -D -Y` / `pileup_dist -D -Y` against each other,
against `-D -u <fitted levels>` and against the restatement.  Everything is compared by equality.

Geometry (hm_pileup.hip): the row scans work on 1024 rows per workgroup (SCAN_ROWS); domain_sums_kernel runs 256 threads per
workgroup, one row per thread and trip, and at most 1024 workgroups (DOM_SUMS_WGS): 262 144 rows per trip of its grid-stride loop."""
import ctypes
import subprocess
import sys
from functools import partial

import numpy as np
import pytest

from domains_fit_ref import LOCUS_DTYPE, fit_chains, fit_tsv, state_sums, synthetic_track
from test_gpu_pileup_asm import CTX, ROOT, _dist_env, _run_cli, _write_bam
from test_gpu_pileup_domains import _parse_cov
from test_gpu_pileup_domains_parts import _dist, _mixed, _two_sequences

pytestmark = pytest.mark.gpu

WG = 1024                                                     # rows per row-scan workgroup
TRIP = 256 * 1024                                             # rows per trip of domain_sums_kernel's loop
TIE = (4, -4, 8, 7)                                           # (A, B, S, max_gap); e = 4 (pcov - ncov)
FREE = (4, -4, 0, 7)                                          # S = 0: every row takes the state of its own sign
SCORES = (136278, -98571, 524288, 1000)                       # domain_scores(0.1, 0.8, 8)


@pytest.fixture(scope="module")
def pu():
    from hifimeth_amd.pileup import MethylationPileup
    p = MethylationPileup([("c", "ACGT" * 50)])              # caller-owned planes: the reference plays no part
    yield p
    p.close()


def _dev(host):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x, np.int32)).cuda() for x in host]


def _loci(host, lo, hi, base=0):
    """the planes' loci [lo, hi) as hm_locus_t-like rows (every locus: the restatement selects the rows itself)"""
    p, u, key = (np.asarray(x, np.int64)[lo:hi] for x in host)
    rows = np.zeros(hi - lo, LOCUS_DTYPE)
    rows["gpos"], rows["pcov"], rows["ncov"], rows["motif"] = base + np.arange(lo, hi), p, u, key & 3
    return rows


def _segment_sums(segs):
    out = [0] * 6
    for g in segs:
        z = int(g["state"])
        out[3 * z] += int(g["pcov"])
        out[3 * z + 1] += int(g["ncov"])
        out[3 * z + 2] += int(g["n_loci"])
    return tuple(out)


def _check(pu, host, dev, ctx, rule, lo=0, hi=None, base=0):
    """the device's sums over [lo, hi) equal the restatement's and those of the device's own segments -> the sums"""
    hi = len(host[0]) if hi is None else hi
    got = pu.domain_sums(ctx, lo, hi, *rule, planes=dev, plane_base=base)
    segs, R = pu.domains(ctx, lo, hi, *rule, planes=dev, plane_base=base)
    assert got == _segment_sums(segs) and got[2] + got[5] == R, (ctx, rule, lo, hi)
    assert got == state_sums([_loci(host, lo, hi, base)], ctx, *rule), (ctx, rule, lo, hi)
    return got


def _track(R, seed, dense=False):
    """planes with exactly R CpG rows in stretches of 5 .. 40 rows, high (3 +- noise : 0 .. 1) or low; unless dense a CpG row
    sits on every odd locus between CHG rows and uncovered loci, and a few stretches start behind a gap of 12 loci (a break
    under max_gap 7)"""
    rng = np.random.default_rng(seed)
    run = np.repeat(rng.integers(0, 2, R // 5 + 1), rng.integers(5, 41, R // 5 + 1))[:R]
    p = np.where(run, rng.integers(1, 5, R), rng.integers(0, 2, R))
    u = np.where(run, rng.integers(0, 2, R), rng.integers(1, 5, R))
    zero = p + u == 0
    p[zero & (run == 1)], u[zero & (run == 0)] = 1, 1
    if dense:
        return (p, u, (np.arange(R) % 1013) << 2), R
    step = np.full(R, 2)
    step[(np.diff(run, prepend=run[:1]) != 0) & (rng.random(R) < 0.2)] = 12
    at = np.cumsum(step) - 1
    n = int(at[-1]) + 2 if R else 9
    P, U, key = np.zeros(n, np.int64), np.zeros(n, np.int64), (np.arange(n) % 1013) << 2
    P[0::4], U[0::4], key[0::4] = 1, 2, key[0::4] | 1         # CHG rows on every fourth locus
    if R:
        P[at], U[at], key[at] = p, u, key[at] & ~3
    return (P, U, key), R


@pytest.mark.parametrize("R", [0, 1, 1023, 1024, 1025, 2 * WG + 1, 3 * WG + 1, 5 * WG + 1])
def test_row_counts_at_the_scan_workgroup_edges(pu, R):
    """R rows of the context: none, one, one scan workgroup less one row / exactly / and one row, and a few workgroups and one
    row: 4 to 21 workgroups of domain_sums_kernel"""
    host, _ = _track(R, 100 + R)
    dev = _dev(host)
    for rule in (TIE, SCORES, FREE):
        got = _check(pu, host, dev, 0, rule)
        assert got[2] + got[5] == R and (R < 1000 or (got[2] > 100 and got[5] > 100))
    sums = (ctypes.c_int64 * 6)(*[7] * 6)
    ptrs = [ctypes.c_void_p(t.data_ptr()) for t in dev]
    assert pu._L.hm_pileup_domain_sums(pu._h, *ptrs, 0, 0, len(host[0]), 0, *TIE, sums) == R      # the return value is R
    assert tuple(sums) == _check(pu, host, dev, 0, TIE)
    other = _check(pu, host, dev, 1, TIE)                     # the CHG rows of the same planes
    assert other[2] + other[5] == (len(host[0]) + 3) // 4 and other[5] == 0


def test_grid_stride_loop_takes_a_second_trip(pu):
    """TRIP + 777 rows: the 1024 workgroups of domain_sums_kernel each take 256 rows, and the first four workgroups a second trip"""
    host, R = _track(TRIP + 777, 5, dense=True)
    dev = _dev(host)
    assert R == TRIP + 777 and len(host[0]) == R
    got = _check(pu, host, dev, 0, TIE)
    assert got[2] + got[5] == R and min(got[2], got[5]) > 100000
    # the rows of the second trip matter: without them the sums are others
    assert pu.domain_sums(0, 0, TRIP, *TIE, planes=dev) != got


def test_counters_beyond_the_clamp_and_sums_beyond_32_bits(pu):
    big, huge = (1 << 20) + 5, (1 << 30) - 3
    p = np.array([big, 0, 3, 0, 2 * big, 0, huge, huge, huge, huge, huge, 0, 0, 0, 0, 0, 0, 2, 0], np.int64)
    u = np.array([0, big, 0, 3, 0, 3 * big, 0, 1, 0, 2, 0, huge, huge, huge, huge, huge, huge, 0, 7], np.int64)
    host = (p, u, np.arange(len(p)) << 2)
    dev = _dev(host)
    for rule in (TIE, FREE, SCORES, (1 << 24, -(1 << 24), 1 << 24, 5), (1, -1, 0, 1)):
        got = _check(pu, host, dev, 0, rule)
        assert got[0] + got[3] == int(p.sum()) > 1 << 32 and got[1] + got[4] == int(u.sum()) > 1 << 32
    got = _check(pu, host, dev, 0, FREE)                      # every row on its own: unclamped sums per sign
    assert got == (0, int(u[p < u].sum()), int((p < u).sum()), int(p[p > u].sum()), int(u[p > u].sum()), int((p > u).sum()))
    assert got[3] > 1 << 32 and got[1] > 1 << 32


def test_all_rows_in_one_state(pu):
    R = 2 * WG + 52
    for p, u, state in ((3, 0, 1), (0, 3, 0), (2, 2, 0)):      # high, low, and ties throughout: low
        host = (np.full(R, p), np.full(R, u), np.arange(R) << 2)
        got = _check(pu, host, _dev(host), 0, TIE)
        want = [0] * 6
        want[3 * state:3 * state + 3] = p * R, u * R, R
        assert got == tuple(want)


def test_ties_breaks_and_no_switch_penalty(pu):
    """small counters under e = 4 (pcov - ncov), S = 8 and max_gap 7: ties of every kind, a quarter of the loci uncovered, the three
    contexts interleaved; and the same planes under S = 0"""
    n = 3000
    for seed in (21, 22):
        host = _mixed(n, seed)
        dev = _dev(host)
        for ctx in range(3):
            for rule in (TIE, FREE, (4, -4, 8, 1), (3, -5, 2, 2)):
                got = _check(pu, host, dev, ctx, rule)
                assert got[2] > 50 and got[5] > 50
    p = np.zeros(60, np.int64)
    u = np.zeros(60, np.int64)
    p[10:20], p[40:50], u[5:10], u[50:55] = 3, 3, 3, 3        # low, high | break | high, low
    host = (p, u, np.arange(60) << 2)
    assert _check(pu, host, _dev(host), 0, TIE) == (0, 30, 10, 60, 0, 20)
    p[10:20], p[40:50], u[10:20], u[40:50] = 1, 1, 1, 1       # the high rows tie: across the break each side follows its own end
    assert _check(pu, host, _dev(host), 0, TIE) == (20, 50, 30, 0, 0, 0)


def test_range_off_a_block_edge_with_a_plane_base(pu):
    """the compaction counts per 4096 loci from `lo`: ranges that start and end off those edges, plane_base far beyond 2^32"""
    host, R = _track(6000, 77)
    dev = _dev(host)
    n = len(host[0])
    assert n > 3 * 4096
    for lo, hi, base in ((37, n - 11, 10 ** 10 + 7), (4095, 4097 + 4096, 1 << 32), (4097, n, 3), (5000, 5000, 9), (123, 124, 0)):
        whole = _check(pu, host, dev, 0, TIE, lo, hi, base)
        assert whole == _check(pu, host, dev, 0, TIE, lo, hi, 0)      # the sums do not depend on plane_base
    assert _check(pu, host, dev, 0, TIE, 37, n - 11) != _check(pu, host, dev, 0, TIE)


# ---- pieces ------------------------------------------------------------------------------------------------------------------------
def _piece_sums(pu, dev, edges, ctx, rule, base=0):
    """the chain of pieces cut at edges -> per piece the sums of hm_pileup_domain_sums_part, after passes S and C and the two walks;
    each is also what the piece's own segments (pass G) add up to"""
    from hifimeth_amd.pileup import (DOMAIN_PASS_CODES, DOMAIN_PASS_SEGMENTS, DOMAIN_PASS_SUMMARY, domain_backward_carries,
                                     domain_forward_carries)
    A, B, S, max_gap = rule
    pieces = [partial(pu.domains_part, ctx, a, b, planes=dev, plane_base=base) for a, b in zip(edges, edges[1:])]
    summaries = [p(DOMAIN_PASS_SUMMARY, {}, *rule) for p in pieces]
    fwd = domain_forward_carries(summaries, S, max_gap)
    codes = [p(DOMAIN_PASS_CODES, f, *rule) if s["n_rows"] else {} for p, s, f in zip(pieces, summaries, fwd)]
    bwd = domain_backward_carries(summaries, codes, S, max_gap)
    out = []
    for (a, b), p, s, f, w in zip(zip(edges, edges[1:]), pieces, summaries, fwd, bwd):
        got = pu.domain_sums(ctx, a, b, *rule, planes=dev, plane_base=base, carry={**f, **w})
        assert got[2] + got[5] == s["n_rows"]
        if s["n_rows"]:
            assert got == _segment_sums(p(DOMAIN_PASS_SEGMENTS, {**f, **w}, *rule)["segments"]), (a, b)
        out.append(got)
    return out


def _add(parts):
    return tuple(sum(col) for col in zip(*parts))


def test_piece_sums_add_up_to_the_whole(pu):
    n = 60
    p, u = np.zeros(n, np.int64), np.zeros(n, np.int64)
    p[10:20], p[40:50], u[5:10], u[50:55] = 3, 3, 3, 3        # low rows 5 .. 9, high 10 .. 19, 20 loci without a row, high 40 .. 49, low 50 .. 54
    host = (p, u, np.arange(n) << 2)
    dev = _dev(host)
    whole = _check(pu, host, dev, 0, TIE)
    assert whole == (0, 30, 10, 60, 0, 20)
    cases = {"inside a segment": [15], "on a state change": [10], "next to one": [9, 11], "inside the break": [30], "at its ends": [20, 40],
             "an empty piece": [12, 12], "a piece without rows inside the break": [25, 35], "many": [7, 10, 15, 30, 30, 45, 50, 52]}
    for name, cuts in cases.items():
        parts = _piece_sums(pu, dev, [0, *cuts, n], 0, TIE)
        assert _add(parts) == whole, name
    assert _piece_sums(pu, dev, [0, 12, 12, n], 0, TIE)[1] == (0,) * 6 and _piece_sums(pu, dev, [0, 15, n], 0, TIE)[0] == (0, 15, 5, 15, 0, 5)
    # a piece's rows take the states the chain gives them, not those of the piece alone: a weak high row is low on its own side
    p2, u2 = np.array([3, 3, 3, 1, 1, 0, 0]), np.array([0, 0, 0, 0, 0, 3, 3])
    host2 = (p2, u2, np.arange(7) << 2)
    dev2 = _dev(host2)
    whole2 = _check(pu, host2, dev2, 0, TIE)
    alone = pu.domain_sums(0, 3, 7, *TIE, planes=dev2)
    parts = _piece_sums(pu, dev2, [0, 3, 7], 0, TIE)
    assert _add(parts) == whole2 == (0, 6, 2, 11, 0, 5) and alone == (2, 6, 4, 0, 0, 0) and parts[1] != alone


def test_piece_sums_on_mixed_planes_and_over_scan_workgroups(pu):
    n = 120
    host = _mixed(n, 21)
    dev = _dev(host)
    rng = np.random.default_rng(23)
    for ctx in range(3):
        for rule in (TIE, SCORES):
            whole = _check(pu, host, dev, ctx, rule)
            for cut in range(0, n + 1, 3):
                assert _add(_piece_sums(pu, dev, [0, cut, n], ctx, rule)) == whole, (ctx, rule, cut)
            for _ in range(4):
                cuts = sorted(int(x) for x in rng.integers(0, n + 1, 3))
                assert _add(_piece_sums(pu, dev, [0, *cuts, n], ctx, rule, base=1 << 33)) == whole, (ctx, rule, cuts)
    host, R = _track(3 * WG + 5, 9)
    dev = _dev(host)
    rows = np.flatnonzero((host[2] & 3) == 0)
    rows = rows[(host[0] + host[1])[rows] > 0]
    assert len(rows) == R
    whole = _check(pu, host, dev, 0, TIE)
    cuts = [int(rows[k]) for k in (1023, 1024, 1025, 2048, 3076)]
    parts = _piece_sums(pu, dev, [0, *cuts, len(host[0])], 0, TIE)
    assert _add(parts) == whole and [s[2] + s[5] for s in parts] == [1023, 1, 1, 1023, 1028, 1]


def test_argument_errors_leave_the_engine_usable(pu):
    from hifimeth_amd.caller import HifimethError
    host = _mixed(120, 21)
    dev = _dev(host)
    want = _check(pu, host, dev, 0, TIE)
    ptrs = [ctypes.c_void_p(t.data_ptr()) for t in dev]
    sums = (ctypes.c_int64 * 6)()
    assert pu._L.hm_pileup_domain_sums(pu._h, *ptrs, 0, 0, 120, 0, *TIE, None) == -1
    assert pu._L.hm_pileup_domain_sums_part(pu._h, *ptrs, 0, 0, 120, 0, *TIE, None, sums) == -1
    for bad in ((0, -4, 8, 7), (4, 0, 8, 7), (4, -4, -1, 7), (4, -4, 8, 0), ((1 << 24) + 1, -4, 8, 7)):
        with pytest.raises(HifimethError, match="hm_pileup_domain_sums"):
            pu.domain_sums(0, 0, 120, *bad, planes=dev)
    with pytest.raises(HifimethError):
        pu.domain_sums(3, 0, 120, *TIE, planes=dev)
    with pytest.raises(HifimethError, match="hm_pileup_domain_sums_part"):
        pu.domain_sums(0, 40, 120, *TIE, planes=dev, plane_base=1000, carry={"has_prev": 1, "prev_gpos": 1040, "prev_d": 0})
    with pytest.raises(HifimethError, match="hm_pileup_domain_sums_part"):
        pu.domain_sums(0, 40, 120, *TIE, planes=dev, carry={"has_next": 1, "next_gpos": 130, "last_state": 2})
    assert pu.domain_sums(0, 0, 120, *TIE, planes=dev) == want and pu.domain_sums(0, 50, 50, *TIE, planes=dev) == (0,) * 6


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def track():
    """the synthetic two-level track as planes over a reference of its three sequences"""
    from hifimeth_amd.pileup import MethylationPileup
    chains, lengths = synthetic_track()
    n = sum(lengths)
    host = [np.zeros(n, np.int64) for _ in range(3)]
    for rows in chains:
        g = rows["gpos"]
        host[0][g], host[1][g], host[2][g] = rows["pcov"], rows["ncov"], (g % 1013) << 2 | rows["motif"]
    p = MethylationPileup([(f"s{k}", "A" * length) for k, length in enumerate(lengths)])
    yield p, chains, _dev(host)
    p.close()


@pytest.mark.parametrize("ctx,lo,hi,penalty,max_iter", [(0, 0.3, 0.6, 8.0, 30), (0, 0.4, 0.5, 0.0, 30), (1, 0.5, 0.9, 2.0, 30),
                                                        (0, 0.01, 0.02, 8.0, 30), (2, 0.3, 0.6, 8.0, 1)])
def test_fit_equals_the_reference_history(track, ctx, lo, hi, penalty, max_iter):
    """fit_domain_levels over the three sequences of the synthetic track: the levels, the status and every row of the history --
    (A, B) and the six sums included -- are the restatement's"""
    p, chains, dev = track
    want = fit_chains(chains, ctx, lo, hi, penalty, 1000, max_iter)
    got = p.fit_domain_levels(ctx, lo, hi, penalty, 1000, max_iter, planes=dev)
    print("fit:", got[:3], len(got[3]), "iterations")
    assert got == want
    assert want[2] == {0.01: "one_state", 1: "max_iter"}.get(lo if lo == 0.01 else max_iter, "converged")


@pytest.fixture(scope="module")
def cli_fit(tmp_path_factory):
    """`pileup -D -Y 20` on reads over two sequences with a high CpG domain around the middle of the concatenated reference"""
    from bamutil import write_fasta
    tmp = tmp_path_factory.mktemp("fit")
    genome, reads, _border = _two_sequences("domain")
    bam, fa, prefix = str(tmp / "mod.bam"), str(tmp / "ref.fa"), str(tmp / "cli")
    _write_bam(bam, genome, reads)
    write_fasta(fa, genome)
    args = ["-D", "-u", "0.3:0.6,nan,0.2:0.5", "-x", "1.5", "-j", "150"]
    r = _run_cli([*args, "-Y", "20", fa, bam, prefix])
    assert f"{prefix}.domains.fit.tsv" in r.stderr
    return tmp, genome, fa, bam, prefix, args


def _domain_files(prefix, fit=True):
    return {n: open(f"{prefix}.domains.{n}").read() for n in [f"{c}.bed" for c in CTX] + (["fit.tsv"] if fit else [])}


def test_cli_fit_equals_the_reference_and_the_run_with_its_levels(cli_fit):
    from hifimeth_amd.pileup import domains_fit_tsv
    tmp, genome, fa, bam, prefix, args = cli_fit
    got = _domain_files(prefix)
    cov = _parse_cov(prefix, genome)
    fits = [None if start is None else fit_chains([cov[s, c] for s in range(len(genome))], c, *start, 1.5, 150, 20)
            for c, start in enumerate(((0.3, 0.6), None, (0.2, 0.5)))]
    print(got["fit.tsv"])
    assert got["fit.tsv"] == fit_tsv(fits) == domains_fit_tsv(fits)
    assert fits[0][2] == "converged" and len(fits[0][3]) >= 2 and fits[0][:2] != (0.3, 0.6)
    last = {f[0]: f for f in (line.split("\t") for line in got["fit.tsv"].splitlines()) if len(f) == 4}
    assert set(last) == {"CpG", "CHH"}
    levels = ",".join("nan" if c not in last else f"{last[c][2]}:{last[c][3]}" for c in CTX)
    _run_cli(["-D", "-u", levels, "-x", "1.5", "-j", "150", fa, bam, prefix + "u"])
    again = _domain_files(prefix + "u", fit=False)
    assert again == {k: v for k, v in got.items() if k != "fit.tsv"} and again["CpG.bed"] and not again["CHG.bed"]
    _run_cli([*args, fa, bam, prefix + "0"])                 # the start levels give other segments: the fit did something
    assert _domain_files(prefix + "0", fit=False)["CpG.bed"] != got["CpG.bed"]
    assert not [f for f in tmp.iterdir() if f.name.endswith("fit.tsv") and f.name != "cli.domains.fit.tsv"]
    for c in CTX:                                             # every other file of the run is the run's without -Y
        assert open(f"{prefix}.{c}.cov.bed").read() == open(f"{prefix}0.{c}.cov.bed").read()


def test_pileup_dist_fit_on_two_ranks(cli_fit):
    """python -m hifimeth_amd.pileup_dist -D -Y on two gloo ranks sharing the card, their border inside a high CpG domain, and as a
    world of one: domains.*.bed and domains.fit.tsv are `pileup -D -Y`'s byte for byte"""
    tmp, genome, fa, bam, prefix, args = cli_fit
    want = _domain_files(prefix)
    _dist([*args, "-Y", "20"], fa, bam, str(tmp / "gloo"), 29597)
    assert _domain_files(str(tmp / "gloo")) == want
    r = subprocess.run([sys.executable, "-m", "hifimeth_amd.pileup_dist", *args, "-Y", "20", "--slab", "7", fa, bam, str(tmp / "one")],
                       capture_output=True, text=True, env=_dist_env(), cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _domain_files(str(tmp / "one")) == want
