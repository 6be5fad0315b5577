"""Allele-specific regions (`pileup -H -A -G`), restated in plain numpy / Python from include/hifimeth_hip.h: what
hm_pileup_fetch_asm_regions must return, given the hm_asm_t rows of the range, and what stitch_asm_regions guarantees.

Per context c and range: ROWS = the hm_asm_t rows with min(motif, 2) == c, ascending.  Row i is a HIT when pvalue_i <= max_p and
diff_i != 0, its sign that of diff_i.  Rows i-1 and i are LINKED when both are hits of one sign and gpos_i - gpos_{i-1} <= max_gap.
A CHAIN is a maximal run of consecutively linked hits (a row that is no hit breaks it; a single hit is a chain of one).  Returned,
ascending: the chains with n_loci >= min_loci and, with keep_edges, every chain that holds the first or the last row."""
import numpy as np

REGION_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("pcov1", "<i8"), ("ncov1", "<i8"), ("pcov2", "<i8"), ("ncov2", "<i8"),
                         ("n_loci", "<i4"), ("sign", "<i4"), ("motif", "<u4"), ("flags", "<u4"), ("diff", "<f8"), ("pmin", "<f8")])
FIRST, LAST = 1, 2


def ctx_rows(rows, ctx):
    return rows[np.minimum(rows["motif"], 2) == ctx]


def pooled_diff(P1, N1, P2, N2):
    """the host's 100 * P1 / (P1 + N1) - 100 * P2 / (P2 + N2): multiply, divide, subtract, each rounded once in fp64"""
    P1, N1, P2, N2 = (np.float64(int(x)) for x in (P1, N1, P2, N2))
    return np.float64(100.0) * P1 / (P1 + N1) - np.float64(100.0) * P2 / (P2 + N2)


def _sign(r, max_p):
    if not r["pvalue"] <= max_p or r["diff"] == 0:
        return 0
    return 1 if r["diff"] > 0 else -1


def _region(r, i, j, sign, ctx, flags):
    """the chain r[i .. j] (inclusive)"""
    g = np.zeros((), REGION_DTYPE)
    g["start"], g["end"] = r["gpos"][i], r["gpos"][j] + 1
    sums = [int(r[f][i:j + 1].astype(np.int64).sum()) for f in ("pcov1", "ncov1", "pcov2", "ncov2")]
    g["pcov1"], g["ncov1"], g["pcov2"], g["ncov2"] = sums
    g["n_loci"], g["sign"], g["motif"], g["flags"] = j - i + 1, sign, ctx, flags
    g["diff"] = pooled_diff(*sums)
    g["pmin"] = r["pvalue"][i:j + 1].min()
    return g


def _select(chains, n_rows, r, ctx, min_loci, keep_edges):
    out = []
    for i, j, s in sorted(chains):
        flags = (FIRST if i == 0 else 0) | (LAST if j == n_rows - 1 else 0)
        if j - i + 1 >= min_loci or (keep_edges and flags):
            out.append(_region(r, i, j, s, ctx, flags))
    return np.array(out, REGION_DTYPE) if out else np.zeros(0, REGION_DTYPE)


def regions(rows, ctx, max_p, max_gap, min_loci, keep_edges=False):
    """-> (regions, R): one walk over the context's rows, a chain kept open while the next row links to its last"""
    r = ctx_rows(rows, ctx)
    chains, start, prev = [], None, 0                         # prev: the sign of row i - 1
    for i in range(len(r)):
        s = _sign(r[i], max_p)
        linked = start is not None and s != 0 and s == prev and r["gpos"][i] - r["gpos"][i - 1] <= max_gap
        if not linked:
            if start is not None:
                chains.append((start, i - 1, prev))
            start = i if s else None
        prev = s
    if start is not None:
        chains.append((start, len(r) - 1, prev))
    return _select(chains, len(r), r, ctx, min_loci, keep_edges), len(r)


def regions_union_find(rows, ctx, max_p, max_gap, min_loci, keep_edges=False):
    """the same from a second formulation: every link (i - 1, i) found on its own, the chains are the connected components of the
    hits under those links"""
    r = ctx_rows(rows, ctx)
    n = len(r)
    sign = np.where(r["pvalue"] <= max_p, np.sign(r["diff"]), 0).astype(np.int64)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    link = (sign[1:] != 0) & (sign[1:] == sign[:-1]) & (np.diff(r["gpos"]) <= max_gap)
    for i in np.nonzero(link)[0]:
        parent[find(int(i) + 1)] = find(int(i))
    members = {}
    for i in np.nonzero(sign)[0]:
        members.setdefault(find(int(i)), []).append(int(i))
    chains = [(m[0], m[-1], int(sign[m[0]])) for m in members.values()]
    assert all(m == list(range(m[0], m[-1] + 1)) for m in members.values())
    return _select(chains, n, r, ctx, min_loci, keep_edges), n


def parts_of(rows, bounds, ctx, max_p, max_gap, min_loci):
    """what a caller fetches for the adjacent ranges [bounds[k], bounds[k + 1]) with keep_edges: [(regions, R)] -- the input of
    stitch_asm_regions, whose result must equal regions() over all rows, byte for byte, for either keep_edges"""
    return [regions(rows[(rows["gpos"] >= a) & (rows["gpos"] < b)], ctx, max_p, max_gap, min_loci, keep_edges=True)
            for a, b in zip(bounds[:-1], bounds[1:])]
