"""`pileup -D`, `-D -Y` and the row fetches beyond 2^20 rows of one context: the planes of domains_scale_cases.py at u = 1024, the
device's scan unit.  Up to 1 048 576 rows every thread of rowscan_carry_kernel holds ONE aggregate (and up to 4 Mi loci every thread
of loci_scan_kernel one block count); here the break-delimited ranges A, B, C and the whole W give it slices of 2 and 3, short
and empty slices, and the reduce-only passes' extra identity slot a slice of its own -- the path a chromosome takes.

Nothing here has a tolerance: rows compare as raw 64-byte records, floats as bits.  The expectation is ONE pass of
domains_ref.domains over W; that its cut at the breaks is the reference of A, B and C is what test_pileup_domains_scale_cpu.py
shows at a small scan unit, together with what the planes hold."""
import numpy as np
import pytest

from domains_ref import ctx_rows, domains
from domains_scale_cases import TIE, build
from test_gpu_pileup_domains import _host_loci
from test_gpu_pileup_domains_parts import SCORES, _chain, _raw

pytestmark = pytest.mark.gpu

U = 1024                                                      # rows per row-scan workgroup (SCAN_ROWS) and threads of the carry kernel
BASE = (1 << 32) + 3


class _Case:
    pass


@pytest.fixture(scope="module")
def case():
    import torch
    from hifimeth_amd.pileup import MethylationPileup
    c = _Case()
    c.host, c.info = build(U)
    c.n, c.R, c.g, c.ranges = c.info["n"], c.info["R"], c.info["row_locus"], c.info["ranges"]
    assert c.R == 2 * U * U + 3 * U + 5 and -(-c.n // 4096) == 2052 and -(-2052 // 1024) == 3     # loci_scan_kernel: per = 3
    nagg = {k: -(-r[3] // U) for k, r in c.ranges.items()}
    assert nagg == {"A": 1024, "B": 1025, "C": 1028, "W": 2052} and c.ranges["C"][0] % 4096 != 0
    c.loci = _host_loci(c.host, 0, c.n)
    c.segs, R = domains(c.loci, 0, *TIE)                      # the one long step: a few seconds
    c.rows = ctx_rows(c.loci, 0)
    c.z = np.repeat(c.segs["state"], c.segs["n_loci"]).astype(np.int64)
    assert R == c.R == len(c.z) and len(c.segs) > 5000
    c.pu = MethylationPileup([("c", "ACGT" * 50)])           # caller-owned planes: the reference plays no part
    c.dev = [torch.from_numpy(x).cuda() for x in c.host]
    yield c
    c.pu.close()


def _equal(got, want, what):
    """raw rows; a difference is reported by its first row and the fields that differ there"""
    if len(got) == len(want) and np.array_equal(_raw(got), _raw(want)):
        return
    m = min(len(got), len(want))
    bad = np.flatnonzero((_raw(got[:m]) != _raw(want[:m])).any(axis=1))
    if len(bad) == 0:
        raise AssertionError(f"{what}: {len(got)} rows, {len(want)} expected; the first {m} are equal")
    k = int(bad[0])
    fields = {f: (got[k][f], want[k][f]) for f in got.dtype.names if got[k][f].tobytes() != want[k][f].tobytes()}
    raise AssertionError(f"{what}: {len(got)} rows, {len(want)} expected, {len(bad)} of the first {m} differ; row {k} (got, expected): {fields}")


@pytest.mark.parametrize("name,base", [("W", 0), ("W", BASE), ("C", 0), ("C", BASE)])
def test_loci_fetch(case, name, base):
    """hm_pileup_fetch_loci: block counts in every slice of loci_scan_kernel's threads"""
    lo, hi, _first, _rows = case.ranges[name]
    got = case.pu.loci(lo, hi, planes=case.dev, plane_base=base)
    want = case.loci[(case.loci["gpos"] >= lo) & (case.loci["gpos"] < hi)].copy()
    want["gpos"] += base
    assert len(want) > (1 << 21) and got.dtype == want.dtype
    assert len(got) == len(want) and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (name, base)


def _slice(case, name):
    lo, hi, first, rows = case.ranges[name]
    return lo, hi, first, rows, case.segs[(case.segs["start"] >= lo) & (case.segs["end"] <= hi)]


@pytest.mark.parametrize("name", ["A", "B", "C", "W"])
def test_domains_over_one_range(case, name):
    lo, hi, _first, rows, want = _slice(case, name)
    assert int(want["n_loci"].sum()) == rows
    got, n_ctx = case.pu.domains(0, lo, hi, *TIE, planes=case.dev)
    assert n_ctx == rows
    _equal(got, want, f"range {name}")
    if name == "C":                                           # the same loci as a chunk of its own whose element 0 is locus BASE + lo
        chunk = [t[lo:] for t in case.dev]
        moved, n2 = case.pu.domains(0, 0, hi - lo, *TIE, planes=chunk, plane_base=BASE + lo)
        moved["start"] -= BASE
        moved["end"] -= BASE
        assert n2 == rows
        _equal(moved, want, "range C with a plane_base")


def test_domains_under_scores_over_the_whole(case):
    """the default kind of rule: S far above a row's score and max_gap 1000, so neither break of the planes is one"""
    want, R = domains(case.loci, 0, *SCORES)
    got, n_ctx = case.pu.domains(0, 0, case.n, *SCORES, planes=case.dev)
    assert n_ctx == R == case.R and len(want) > 1000 and (want["flags"] != 0).sum() == 2
    _equal(got, want, "W under SCORES")


def test_the_other_context_over_the_whole(case):
    """the CHG rows of the same planes: R + 4 rows, no break"""
    want, R = domains(case.loci, 1, *TIE)
    got, n_ctx = case.pu.domains(1, 0, case.n, *TIE, planes=case.dev)
    assert n_ctx == R == case.R + 4 and len(want) > 5000
    _equal(got, want, "W, context 1")


@pytest.mark.parametrize("name", ["A", "B", "C", "W"])
def test_state_sums(case, name):
    """`-D -Y`: the six sums of hm_pileup_domain_sums against those of the reference's states"""
    lo, hi, first, rows = case.ranges[name]
    r, z = case.rows[first:first + rows], case.z[first:first + rows]
    want = []
    for s in (0, 1):
        want += [int(r["pcov"][z == s].astype(np.int64).sum()), int(r["ncov"][z == s].astype(np.int64).sum()), int((z == s).sum())]
    got = case.pu.domain_sums(0, lo, hi, *TIE, planes=case.dev)
    assert got == tuple(want) and got[2] + got[5] == rows and min(got[2], got[5]) > rows // 4, name


def _stretch(case, k):
    return case.info["stretches"][k][0]


CUTS = {"a left piece of exactly 2^20 rows": lambda c: [int(c.g[U * U])],
        "inside a stretch of C": lambda c: [int(c.g[U * U + 2 * U + 5])],
        "a stretch of A and both breaks": lambda c: [int(c.g[_stretch(c, 0) + 3 * U + 7]),
                                                                                       int(c.g[U * U]) - 5, int(c.g[U * U + 1])]}
PIECE_ROWS = {"a left piece of exactly 2^20 rows": [U * U, U * U + 3 * U + 5],
              "inside a stretch of C": [U * U + 2 * U + 5, U * U + U],
              "a stretch of A and both breaks": None}


@pytest.mark.parametrize("where", list(CUTS))
def test_pieces_against_the_whole(case, where):
    """`pileup_dist -D`: the chained passes over pieces of W, stitched, against ONE hm_pileup_fetch_domains over W.  The summary pass
    and the codes pass are reduce-only: a piece of exactly 2^20 rows gives rowscan_carry_kernel 1025 slots"""
    cuts = CUTS[where](case)
    whole, R = case.pu.domains(0, 0, case.n, *TIE, planes=case.dev)
    assert R == case.R
    got, parts = _chain(case.pu, case.dev, [0, *cuts, case.n], 0, TIE)
    _equal(got, whole, where)
    _equal(got, case.segs, where + ", against the reference")
    rows = [int(p["n_loci"].sum()) for p in parts]
    first = _stretch(case, 0) + 3 * U + 7
    assert rows == (PIECE_ROWS[where] or [first, U * U - first, 1, U * U + 3 * U + 4])
    if PIECE_ROWS[where]:
        assert min(rows) >= 1 << 20
        a, b, _name, _d_in = case.info["stretches"][2]
        assert where.startswith("a left") or a < rows[0] < b
