"""The generic selection kernels behind every row fetch (select_count_kernel / loci_scan_kernel / select_write_kernel): what they
could get wrong whatever the selection is -- the range's offset in the planes, the block edges, the count-only call, the order of
the rows -- checked once for each selection against a numpy selection written from the predicates' definitions in
include/hifimeth_hip.h, never from the engine.

The planes are the caller's, handed in with a non-zero plane_base.  They hold one locus in front of the range and then the
range's 2 x 4096 + 1 loci: the fetch is over [1, 8194), two full compaction blocks plus one locus, and no block starts on a
multiple of 4096 in plane coordinates.  The locus in front of the range would pass every predicate.  Selected loci sit at range
offsets 0, 4095, 4096, 8191 and 8192 and at a handful inside; every plane set also holds loci that a predicate rejects for a
reason of its own: both counters 0, a negative counter, a haplotype total below min_cov, a motif outside the mask or context.

Only gpos and the integer count columns are compared: the statistical columns belong to the per-feature tests.  The rows of the
region and the domain step's first selection (n_ctx_rows) never leave the device, so these two cases are parametrised until every
such row comes back as a chain / segment of its own: adjacent rows lean opposite ways, all others are further apart than max_gap."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BLOCK = 4096
LO, HI = 1, 1 + 2 * BLOCK + 1
PLANE_BASE = 3_000_000_017
EDGES = (0, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK)          # range offsets
INSIDE = (7, 100, 2049, 5000, 6001, 7777)
MIN_COV, CTX, CTX_MASK = 5, 0, 0b101


def _keys(motif, rng):
    return ((rng.integers(0, 1 << 20, len(motif)) << 2) | motif).astype(np.int64)


def _combined():
    """(pcov, ncov, key) as int64, plane coordinates"""
    rng = np.random.default_rng(41)
    n = HI
    pcov, ncov, motif = np.zeros(n, np.int64), np.zeros(n, np.int64), rng.integers(0, 4, n)
    pcov[0], ncov[0], motif[0] = 9, 9, CTX                     # in front of the range: never a row
    hot = np.array(EDGES + INSIDE) + LO
    motif[hot] = CTX
    # adjacent rows lean opposite ways (pcov - ncov changes sign), no row has pcov == ncov
    for off, (p, u) in zip(EDGES + INSIDE, ((20, 0), (30, 2), (0, 20), (0, 15), (18, 1), (3, 1), (0, 1), (12, 30), (300, 10), (1, 0), (5, 9))):
        pcov[off + LO], ncov[off + LO] = p, u
    for off, (p, u, m) in {1: (-3, 5, CTX), 2: (4, -1, CTX), 3: (0, 0, CTX),        # a negative counter; an uncovered locus
                           BLOCK - 3: (6, 6, 1), BLOCK + 2: (2, 8, 2), 2 * BLOCK - 3: (7, 1, 3),   # other contexts; key bits 3 = CHH
                           2 * BLOCK - 5: (-2, -2, 2), 4000: (0, 0, 2)}.items():
        pcov[off + LO], ncov[off + LO], motif[off + LO] = p, u, m
    return pcov, ncov, _keys(motif, rng)


def _haplotypes():
    """(pcov1, ncov1, pcov2, ncov2, key) as int64, plane coordinates"""
    rng = np.random.default_rng(42)
    n = HI
    c = np.zeros((4, n), np.int64)
    motif = rng.integers(0, 4, n)
    c[:, 0], motif[0] = (9, 1, 1, 9), CTX                      # in front of the range: never a row
    hot = np.array(EDGES + INSIDE) + LO
    motif[hot] = CTX
    # adjacent rows lean opposite ways (diff changes sign), no row has diff == 0; one row has a haplotype total >= 64 (a big locus)
    rows = ((10, 0, 0, 10), (10, 1, 2, 10), (0, 10, 10, 0), (1, 9, 9, 1), (9, 1, 1, 9), (5, 0, 1, 4), (70, 5, 3, 40), (2, 3, 3, 2),
            (6, 6, 1, 11), (0, 5, 5, 0), (8, 2, 2, 8))
    for off, r in zip(EDGES + INSIDE, rows):
        c[:, off + LO] = r
    for off, (r, m) in {1: ((-1, 20, 10, 10), CTX), 2: ((10, 10, 10, -1), CTX),      # a negative counter
                        3: ((2, 2, 10, 10), CTX), BLOCK + 1 + 1: ((10, 10, 4, 0), CTX),  # a haplotype total below min_cov
                        BLOCK - 3: ((9, 2, 2, 9), 1), 2 * BLOCK - 3: ((2, 9, 9, 2), 3),  # tested, in another context
                        4000: ((0, 0, 0, 0), CTX)}.items():
        c[:, off + LO], motif[off + LO] = r, m
    return c[0], c[1], c[2], c[3], _keys(motif, rng)


# ---- the predicates, from include/hifimeth_hip.h -----------------------------------------------------------------------------
def is_covered(p, u):                                              # hm_pileup_fetch_loci: a counter of either sign counts
    return (p != 0) | (u != 0)


def is_counted(p, u):                                              # -B and -D: both counters are counts, one is positive
    return (p >= 0) & (u >= 0) & (p + u > 0)


def is_tested(p1, n1, p2, n2):                                     # -A: four counts, each haplotype with at least min_cov reads
    return (p1 >= 0) & (n1 >= 0) & (p2 >= 0) & (n2 >= 0) & (p1 + n1 >= MIN_COV) & (p2 + n2 >= MIN_COV)


def context(key):                                               # the file a row is in: key bits 3 count as CHH
    return np.minimum(key & 3, 2)


def _want(sel, cols):
    """the rows a fetch over [LO, HI) returns for the plane-wide mask sel: gpos, then cols of the selected loci"""
    i = np.nonzero(sel[LO:HI])[0] + LO
    return np.stack([i + PLANE_BASE] + [c[i] for c in cols], axis=1)


@pytest.fixture(scope="module")
def engine():
    import torch
    from hifimeth_amd.pileup import MethylationPileup, asm_qvalues, sites_table
    pu = MethylationPileup([("c", "ACGT")])                    # every fetch below runs on the caller's planes
    comb, hap = _combined(), _haplotypes()
    dev = lambda planes: [torch.from_numpy(x.astype(np.int32)).cuda() for x in planes]
    comb_dev, hap_dev = dev(comb), dev(hap)
    bins, big = pu.asm_histogram(LO, HI, MIN_COV, planes=hap_dev, plane_base=PLANE_BASE)
    asm_table = asm_qvalues(pu.asm_bin_pvalues(bins), big)
    sbins, sbig = pu.site_histogram(LO, HI, planes=comb_dev, plane_base=PLANE_BASE)
    site_table = sites_table([0.01, float("nan"), 0.02], sbins, sbig)
    assert site_table.ctx_mask == CTX_MASK
    yield dict(pu=pu, comb=comb, hap=hap, comb_dev=comb_dev, hap_dev=hap_dev, asm_table=asm_table, asm_big=big, site_table=site_table,
               site_big=sbig)
    pu.close()


def _ptrs(tensors):
    return [C.c_void_p(t.data_ptr()) for t in tensors]


def _np(x):
    return x.ctypes.data_as(C.c_void_p)


def _case(e, kind):
    """-> (fn, args in front of (out, cap), dtype, row columns, wanted rows, n_ctx_rows or None, wanted n_ctx_rows)"""
    from hifimeth_amd import pileup as P
    L = e["pu"]._L
    p, u, key = e["comb"]
    p1, n1, p2, n2, hkey = e["hap"]
    ones = np.ones(HI, np.int64)
    if kind == "loci":
        return (L.hm_pileup_fetch_loci, (*_ptrs(e["comb_dev"]), PLANE_BASE, LO, HI), P.LOCUS_DTYPE, ("gpos", "pcov", "ncov", "motif"),
                _want(is_covered(p, u), (p, u, key & 3)), None, None)
    if kind in ("asm", "asm_q"):
        want = _want(is_tested(p1, n1, p2, n2), (p1, n1, p2, n2, hkey & 3))
        args = (*_ptrs(e["hap_dev"]), PLANE_BASE, LO, HI, MIN_COV)
        cols = ("gpos", "pcov1", "ncov1", "pcov2", "ncov2", "motif")
        if kind == "asm":
            return L.hm_pileup_fetch_asm, args, P.ASM_DTYPE, cols, want, None, None
        t = e["asm_table"]
        return (L.hm_pileup_fetch_asm_q, (*args, _np(t.tab), len(t.tab), _np(t.big), _np(t.big_q), len(t.big)), P.ASMQ_DTYPE, cols, want,
                None, None)
    if kind == "sites":
        t = e["site_table"]
        sel = is_counted(p, u) & (((CTX_MASK >> context(key)) & 1) == 1)
        return (L.hm_pileup_fetch_sites, (*_ptrs(e["comb_dev"]), PLANE_BASE, LO, HI, CTX_MASK, *(_np(x) for x in (t.ptab, t.qtab, t.big, t.big_p, t.big_q)),
                                          len(t.big)), P.SITE_DTYPE, ("gpos", "pcov", "ncov", "motif"), _want(sel, (p, u, context(key))), None, None)
    n_ctx = C.c_int64(-1)
    if kind == "region_rows":                                   # max_p 1, max_gap 1, min_loci 1: every context row is a chain
        want = _want(is_tested(p1, n1, p2, n2) & (context(hkey) == CTX), (p1, n1, p2, n2, ones))
        want = np.insert(want, 1, want[:, 0] + 1, axis=1)
        return (L.hm_pileup_fetch_asm_regions, (*_ptrs(e["hap_dev"]), PLANE_BASE, LO, HI, MIN_COV, CTX, C.c_double(1.0), 1, 1, 0, C.byref(n_ctx)),
                P.ASM_REGION_DTYPE, ("start", "end", "pcov1", "ncov1", "pcov2", "ncov2", "n_loci"), want, n_ctx, len(want))
    assert kind == "domain_rows"                                # S 0, max_gap 1: every context row is a segment
    want = _want(is_counted(p, u) & (context(key) == CTX), (p, u, ones))
    want = np.insert(want, 1, want[:, 0] + 1, axis=1)
    return (L.hm_pileup_fetch_domains, (*_ptrs(e["comb_dev"]), PLANE_BASE, LO, HI, CTX, 65536, -65536, 0, 1, C.byref(n_ctx)), P.DOMAIN_DTYPE,
            ("start", "end", "pcov", "ncov", "n_loci"), want, n_ctx, len(want))


def test_crafted_planes_hold_the_cases():
    p, u, key = _combined()
    p1, n1, p2, n2, hkey = _haplotypes()
    hot = np.array(EDGES + INSIDE) + LO
    r = slice(LO, HI)
    for sel in (is_covered(p, u), is_counted(p, u) & (context(key) == CTX), is_counted(p, u) & (((CTX_MASK >> context(key)) & 1) == 1),
                is_tested(p1, n1, p2, n2), is_tested(p1, n1, p2, n2) & (context(hkey) == CTX)):
        assert sel[hot].all() and sel[0] and not sel[r].all()
    assert (is_covered(p, u) & ~is_counted(p, u))[r].any() and ((p == 0) & (u == 0))[r].any()          # a negative counter; uncovered
    assert (is_counted(p, u) & (context(key) != CTX))[r].any() and (is_counted(p, u) & (context(key) == 1))[r].any() and ((key & 3) == 3)[r].any()
    pos = (p1 >= 0) & (n1 >= 0) & (p2 >= 0) & (n2 >= 0)
    assert (~pos & (p1 + n1 >= MIN_COV) & (p2 + n2 >= MIN_COV))[r].any()                          # rejected for the sign alone
    assert (pos & ((p1 + n1 < MIN_COV) | (p2 + n2 < MIN_COV)) & (p1 + n1 + p2 + n2 > 0))[r].any()   # ... for min_cov alone
    assert (is_tested(p1, n1, p2, n2) & (context(hkey) != CTX))[r].any()                             # ... for the context alone
    # every context row is a chain / a segment of its own: neighbours one base apart lean opposite ways
    for rows, lean in ((np.nonzero((is_counted(p, u) & (context(key) == CTX))[r])[0] + LO, p - u),
                       (np.nonzero((is_tested(p1, n1, p2, n2) & (context(hkey) == CTX))[r])[0] + LO, p1 * (p2 + n2) - p2 * (p1 + n1))):
        assert (lean[rows] != 0).all()
        near = np.diff(rows) <= 1
        assert near.sum() == 2 and (np.sign(lean[rows][:-1][near]) != np.sign(lean[rows][1:][near])).all()


@pytest.mark.parametrize("kind", ["loci", "asm", "asm_q", "sites", "region_rows", "domain_rows"])
def test_selection_over_an_offset_range(engine, kind):
    fn, args, dtype, cols, want, n_ctx, want_ctx = _case(engine, kind)
    pu = engine["pu"]
    counted_only = pu._check(fn(pu._h, *args, None, 0))
    if n_ctx is not None:
        assert n_ctx.value == want_ctx
        n_ctx.value = -1
    rows = np.zeros(counted_only + 1, dtype)                   # one row of room to spare: nothing may be written into it
    filled = pu._check(fn(pu._h, *args, _np(rows), len(rows)))
    assert counted_only == filled == len(want) and len(want) >= len(EDGES + INSIDE)
    assert rows[filled:].tobytes() == bytes(dtype.itemsize)
    if n_ctx is not None:
        assert n_ctx.value == want_ctx
    got = np.stack([rows[c][:filled].astype(np.int64) for c in cols], axis=1)
    assert (got == want).all(), (kind, got[(got != want).any(axis=1)][:4], want[(got != want).any(axis=1)][:4])
    assert (np.diff(got[:, 0]) > 0).all() and got[0, 0] == PLANE_BASE + LO and got[-1, 0] == PLANE_BASE + HI - 1


def test_big_lists_of_the_histograms(engine):
    """the write halves of the two histograms are selections too: the loci beyond the bins, over the same offset range"""
    p, u, key = engine["comb"]
    p1, n1, p2, n2, hkey = engine["hap"]
    big = engine["site_big"]
    want = _want(is_counted(p, u) & (p + u >= 256), (p, u, context(key)))
    assert len(want) >= 1 and (np.stack([big[c].astype(np.int64) for c in ("gpos", "pcov", "ncov", "motif")], axis=1) == want).all()
    big = engine["asm_big"]
    want = _want(is_tested(p1, n1, p2, n2) & ((p1 + n1 >= 64) | (p2 + n2 >= 64)), (p1, n1, p2, n2, hkey & 3))
    assert len(want) >= 1 and len(big) == len(want)
    assert (np.stack([big[c].astype(np.int64) for c in ("gpos", "pcov1", "ncov1", "pcov2", "ncov2", "motif")], axis=1) == want).all()
