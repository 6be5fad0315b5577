"""Regions between replicate groups (`groupdmr`), restated in plain numpy / Python from include/hifimeth_hip.h: what
hm_dmr_fetch_regions must return given the hm_group_t rows of the range, what hm_dmr_p_cutoff returns, and what
stitch_group_regions guarantees.  Shares no code with hifimeth_amd.pileup.

Per context c and range: ROWS = the hm_group_t rows with min(motif, 2) == c, ascending.  Row i is a HIT when pvalue_i <= max_p,
diff_i != 0 and |diff_i| >= min_diff (with q given: q_i <= max_q instead of the first), its sign that of diff_i.  Rows i-1 and i are
LINKED when both are hits of one sign and gpos_i - gpos_{i-1} <= max_gap.  A CHAIN is a maximal run of consecutively linked hits.
Returned, ascending: the chains with n_loci >= min_loci and, with keep_edges, every chain that holds the first or the last row.

regions() walks the rows in Python (chains_walk, or chains_union_find as a second formulation); regions_fast() is the same in
whole-array numpy, for the millions of rows of tests/test_gpu_pileup_group_regions_scale.py.

crafted_rows() are hand-written rows; layout() is what the GPU test loads so that the engine's own rows show every case;
dataset() is its random 3 + 3 data set and dataset_rows() the rows of that data set from groups_ref.stat_f64."""
import functools

import numpy as np

import groups_ref as G

ROW_DTYPE = np.dtype([("gpos", "<i8"), ("pcov1", "<i4"), ("ncov1", "<i4"), ("pcov2", "<i4"), ("ncov2", "<i4"), ("motif", "<u4"),
                      ("m1", "<u2"), ("m2", "<u2"), ("diff", "<f8"), ("D", "<f8"), ("phi", "<f8"), ("pvalue", "<f8")])
REGION_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("pcov1", "<i8"), ("ncov1", "<i8"), ("pcov2", "<i8"), ("ncov2", "<i8"),
                         ("n_loci", "<i4"), ("sign", "<i4"), ("motif", "<u4"), ("flags", "<u4"), ("m1_min", "<u2"), ("m2_min", "<u2"),
                         ("reserved", "<u4"), ("diff", "<f8"), ("pmin", "<f8"), ("phi_max", "<f8")])
FIRST, LAST = 1, 2


def ctx_mask(rows, ctx):
    return np.minimum(rows["motif"], 2) == ctx


def pooled_diff(P1, N1, P2, N2):
    """100 * P1 / (P1 + N1) - 100 * P2 / (P2 + N2): multiply, divide, subtract, each rounded once in fp64"""
    P1, N1, P2, N2 = (np.float64(int(x)) for x in (P1, N1, P2, N2))
    return np.float64(100.0) * P1 / (P1 + N1) - np.float64(100.0) * P2 / (P2 + N2)


def signs(r, max_p, min_diff, q=None, max_q=None):
    """per row +1 / -1 for a hit of that sign, 0 for none"""
    chosen = (r["pvalue"] <= max_p) if q is None else (q <= max_q)
    hit = chosen & (r["diff"] != 0) & (np.abs(r["diff"]) >= min_diff)
    return np.where(hit, np.sign(r["diff"]), 0).astype(np.int64)


def _region(r, i, j, sign, ctx, flags):
    """the chain r[i .. j] (inclusive)"""
    g = np.zeros((), REGION_DTYPE)
    g["start"], g["end"] = r["gpos"][i], r["gpos"][j] + 1
    sums = [int(r[f][i:j + 1].astype(np.int64).sum()) for f in ("pcov1", "ncov1", "pcov2", "ncov2")]
    g["pcov1"], g["ncov1"], g["pcov2"], g["ncov2"] = sums
    g["n_loci"], g["sign"], g["motif"], g["flags"] = j - i + 1, sign, ctx, flags
    g["m1_min"], g["m2_min"] = r["m1"][i:j + 1].min(), r["m2"][i:j + 1].min()
    g["diff"] = pooled_diff(*sums)
    g["pmin"] = r["pvalue"][i:j + 1].min()
    g["phi_max"] = r["phi"][i:j + 1].max()
    return g


def _select(chains, r, ctx, min_loci, keep_edges):
    out = []
    for i, j, s in sorted(chains):
        flags = (FIRST if i == 0 else 0) | (LAST if j == len(r) - 1 else 0)
        if j - i + 1 >= min_loci or (keep_edges and flags):
            out.append(_region(r, i, j, s, ctx, flags))
    return np.array(out, REGION_DTYPE) if out else np.zeros(0, REGION_DTYPE)


def chains_walk(r, sign, max_gap):
    """[(first row, last row, sign)]: one walk, a chain kept open while the next row links to its last"""
    chains, start = [], None
    gpos = r["gpos"].tolist()
    sign = sign.tolist()
    for i, s in enumerate(sign):
        linked = start is not None and s != 0 and s == sign[i - 1] and gpos[i] - gpos[i - 1] <= max_gap
        if not linked:
            if start is not None:
                chains.append((start, i - 1, sign[i - 1]))
            start = i if s else None
    if start is not None:
        chains.append((start, len(sign) - 1, sign[-1]))
    return chains


def chains_union_find(r, sign, max_gap):
    """the same from a second formulation: every link (i - 1, i) found on its own, the chains are the connected components of the
    hits under those links"""
    n = len(r)
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
    assert all(m == list(range(m[0], m[-1] + 1)) for m in members.values())
    return [(m[0], m[-1], int(sign[m[0]])) for m in members.values()]


def regions(rows, ctx, max_p, min_diff, max_gap, min_loci, keep_edges=False, q=None, max_q=None, chains_of=chains_walk):
    """-> (regions, R, hits)"""
    sel = ctx_mask(rows, ctx)
    r = rows[sel]
    sign = signs(r, max_p, min_diff, None if q is None else np.asarray(q)[sel], max_q)
    return _select(chains_of(r, sign, max_gap), r, ctx, min_loci, keep_edges), len(r), int(np.count_nonzero(sign))


def pooled_diff_of(P1, N1, P2, N2):
    """pooled_diff on int64 arrays: the same three operations, each rounded once per element"""
    P1, N1, P2, N2 = (np.asarray(x, np.int64).astype(np.float64) for x in (P1, N1, P2, N2))
    return np.float64(100.0) * P1 / (P1 + N1) - np.float64(100.0) * P2 / (P2 + N2)


def regions_fast(rows, ctx, max_p, min_diff, max_gap, min_loci, keep_edges=False, q=None, max_q=None):
    """regions() a third time, without a loop over rows or chains, for millions of rows: the links as one mask, a chain's head a hit
    not linked to the row in front of it, its tail a hit to which the next row is not linked, every per-chain quantity a reduceat
    over [head, tail + 1).  -> (regions, R, hits), equal to regions()'s byte for byte"""
    sel = ctx_mask(rows, ctx)
    r = rows[sel]
    sign = signs(r, max_p, min_diff, None if q is None else np.asarray(q)[sel], max_q)
    n, hit = len(r), sign != 0
    hits = int(np.count_nonzero(hit))
    if not hits:
        return np.zeros(0, REGION_DTYPE), n, 0
    link = hit[1:] & (sign[1:] == sign[:-1]) & (np.diff(r["gpos"]) <= max_gap)
    head, tail = hit.copy(), hit.copy()
    head[1:] &= ~link
    tail[:-1] &= ~link
    first, last = np.flatnonzero(head), np.flatnonzero(tail)
    assert len(first) == len(last) and (first <= last).all()
    flags = np.where(first == 0, FIRST, 0) | np.where(last == n - 1, LAST, 0)
    keep = (last - first + 1 >= min_loci) | ((flags != 0) if keep_edges else False)
    first, last, flags = first[keep], last[keep], flags[keep]
    g = np.zeros(len(first), REGION_DTYPE)
    if not len(g):
        return g, n, hits
    # reduceat reduces [idx[k], idx[k + 1]): heads and ends interleaved, the even results are the chains'; one padding element
    # so that the end of a chain with the last row is an index
    idx = np.stack([first, last + 1], axis=1).ravel()
    over = lambda op, x: op.reduceat(np.concatenate([x, x[:1]]), idx)[::2]
    g["start"], g["end"] = r["gpos"][first], r["gpos"][last] + 1
    for f in ("pcov1", "ncov1", "pcov2", "ncov2"):
        g[f] = over(np.add, r[f].astype(np.int64))
    g["n_loci"], g["sign"], g["motif"], g["flags"] = last - first + 1, sign[first], ctx, flags
    g["m1_min"], g["m2_min"] = over(np.minimum, r["m1"]), over(np.minimum, r["m2"])
    g["diff"] = pooled_diff_of(g["pcov1"], g["ncov1"], g["pcov2"], g["ncov2"])
    g["pmin"], g["phi_max"] = over(np.minimum, r["pvalue"]), over(np.maximum, r["phi"])
    return g, n, hits


def p_cutoff(p, q, motif, max_q):
    """per context the largest p among the rows with q <= max_q, 0.0 without one"""
    ctx = np.minimum(np.asarray(motif), 2)
    out = np.zeros(3, np.float64)
    for c in range(3):
        under = np.asarray(p)[(ctx == c) & (np.asarray(q) <= max_q)]
        if len(under):
            out[c] = under.max()
    return out


def parts_of(rows, bounds, ctx, max_p, min_diff, max_gap, min_loci):
    """what a caller fetches for the adjacent ranges [bounds[k], bounds[k + 1]) with keep_edges: [(regions, R)] -- the input of
    stitch_group_regions, whose result must equal regions() over all rows, byte for byte, for either keep_edges"""
    return [regions(rows[(rows["gpos"] >= a) & (rows["gpos"] < b)], ctx, max_p, min_diff, max_gap, min_loci, keep_edges=True)[:2]
            for a, b in zip(bounds[:-1], bounds[1:])]


# ---- hand-written rows: (gpos, motif, diff, pvalue, phi, m1, m2); counts follow from gpos so that sums tell rows apart ---------------
def _rows(spec):
    rows = np.zeros(len(spec), ROW_DTYPE)
    for k, (gpos, motif, diff, p, phi, m1, m2) in enumerate(spec):
        rows[k] = (gpos, 7 + gpos % 5, 3 + gpos % 3, 2 + gpos % 7, 9 + gpos % 2, motif, m1, m2, diff, 1.0, phi, p)
    return rows


@functools.lru_cache(maxsize=None)
def crafted_rows():
    """CpG rows with every case at max_p 0.01, min_diff 10, max_gap 10; rows of CHG and CHH (motif 2 and 3) lie among them"""
    H, W = 1e-4, 0.5                                          # a hit's p, a non-hit's
    return _rows([
        (3, 0, 40.0, H, 1.0, 3, 3), (5, 0, 35.0, 1e-9, 2.5, 2, 3),                      # holds row 0
        (20, 0, 50.0, H, 1.0, 3, 3),                                                    # a single hit
        (40, 0, 30.0, H, 1.0, 3, 3), (41, 1, 60.0, H, 1.0, 3, 3), (45, 0, 31.0, H, 1.5, 3, 2), (50, 0, 5.0, W, 1.0, 3, 3),
        (52, 0, 33.0, H, 1.0, 3, 3),                                                    # ... ended by a tested non-hit; CHG inside
        (70, 0, 20.0, H, 1.0, 3, 3), (72, 0, -20.0, H, 1.0, 3, 3), (74, 0, -25.0, 0.01, 4.0, 3, 3),    # a sign flip; p == max_p
        (90, 0, 15.0, H, 1.0, 3, 3), (100, 0, 15.0, H, 1.0, 3, 3), (111, 0, 15.0, H, 1.0, 3, 3),        # gaps of 10 and 11
        (130, 0, 10.0, H, 1.0, 3, 3), (131, 0, 9.999999, H, 1.0, 3, 3), (132, 0, -10.0, H, 1.0, 3, 3),  # at and under min_diff
        (150, 0, 0.0, H, 1.0, 3, 3), (151, 0, 44.0, np.nextafter(0.01, 1), 1.0, 3, 3),                  # diff 0; p just above
        (160, 2, 22.0, H, 1.0, 3, 3), (161, 3, 23.0, H, 7.0, 2, 2), (162, 2, -23.0, H, 1.0, 3, 3),      # CHH, motif 2 and 3 together
        (170, 0, -45.0, H, 1.0, 3, 3), (175, 3, 45.0, H, 1.0, 3, 3), (180, 0, -46.0, 1e-300, 1.0, 3, 3),
        (185, 0, -47.0, H, 3.0, 2, 2), (190, 0, -48.0, H, 1.0, 3, 3),                   # holds the last CpG row
    ])


# ---- what the GPU test loads for the crafted cases: a reference of two sequences, every base of which has a kind -----------------------
LENGTHS = (3000, 1500)
OFFSETS = np.array([0, 3000, 4500], np.int64)
TOTAL = 4500
MIN_COV, MIN_REPS, MAX_GAP = 5, 2, 5
LONG_AT, LONG_N = 300, 1000                                   # the chain of 1000 rows: sequence 2, from this offset on
# kind -> (motif, samples of group 1, samples of group 2), a sample (pcov, ncov) or None (no row)
KINDS = {
    "P": (0, [(20, 0)] * 3, [(0, 20)] * 3),                   # a hit, group 1 above
    "M": (0, [(0, 20)] * 3, [(20, 0)] * 3),                   # a hit, group 2 above
    "N": (0, [(10, 10)] * 3, [(10, 10)] * 3),                 # tested, no hit: D = 0, p = 1
    "U": (0, [(20, 0)] * 3, [(0, 20), None, None]),           # not tested: one counting sample in group 2
    "O": (1, [(20, 0)] * 3, [(0, 20)] * 3),                   # a hit of another context
    "A": (0, [(12, 8)] * 3, [(10, 10)] * 3),                  # diff = 10 exactly (60 - 50), p about 0.3
    "B": (0, [(12, 8), (12, 8), (11, 9)], [(10, 10)] * 3),    # diff = 8.33
    "p": (0, [(20, 0), (17, 3), None], [(0, 20), (2, 18), (1, 19)]),   # a hit with m1 = 2 and phi > 1
    "q": (0, [(20, 0), (17, 3), (19, 1)], [(0, 20), (2, 18), (1, 19)]),  # a hit with phi > 1
}
SCENES = {0: "PP", 10: "P", 20: "PPPNP", 35: "PPMM", 50: "P", 55: "P", 61: "P", 70: "P", 72: "O", 75: "P", 85: "P", 88: "O", 91: "P",
          100: "P", 102: "U", 104: "P", 110: "ABA"}
# the chains of sequence 1 at max_p 0.01, min_diff 0, max_gap 5, min_loci 1: (start, end, n_loci, sign)
SEQ1_CHAINS = [(0, 2, 2, 1), (10, 11, 1, 1), (20, 23, 3, 1), (24, 25, 1, 1), (35, 37, 2, 1), (37, 39, 2, -1), (50, 56, 2, 1), (61, 62, 1, 1),
               (70, 76, 2, 1), (85, 86, 1, 1), (91, 92, 1, 1), (100, 105, 2, 1), (2997, 3000, 3, 1)]


@functools.lru_cache(maxsize=None)
def layout():
    """-> the kind of every base, a str of TOTAL characters ('.': nothing loaded).  Sequence 1: the scenes, tested non-hits from 120
    on, three hits at its end.  Sequence 2: two hits at its start (one chain with those three over the whole reference, two chains
    per sequence), non-hits, the chain of LONG_N rows -- it lies across row 4096 of the whole reference, where the row selection
    passes from one workgroup to the next --, non-hits, two hits at its end."""
    kind = ["."] * TOTAL
    for at, scene in SCENES.items():
        kind[at:at + len(scene)] = scene
    kind[120:2997] = "N" * (2997 - 120)
    kind[2997:3000] = "PPP"
    seq2 = ["N"] * 1500
    seq2[0:2] = "PP"
    seq2[LONG_AT:LONG_AT + LONG_N] = ["p" if k % 7 == 3 else "q" if k % 5 == 2 else "P" for k in range(LONG_N)]
    seq2[1498:1500] = "PP"
    kind[3000:] = seq2
    return "".join(kind)


def layout_samples():
    """-> {(group, sample index): (gpos, pcov, ncov, motif)} of layout()"""
    out = {}
    kind = layout()
    for g in (1, 2):
        for s in range(3):
            rows = [(i, *KINDS[k][g][s], KINDS[k][0]) for i, k in enumerate(kind) if k != "." and KINDS[k][g][s] is not None]
            out[(g, s)] = tuple(np.array(x, np.int64) for x in zip(*rows))
    return out


# ---- the random data set: rows that come in runs, so that chains of several loci exist ---------------------------------------------------
# the thresholds the GPU test fetches it with, the first the one test_the_data_set_holds_regions is about
THRESHOLDS = ((0.01, 0.0, 30, 3), (0.05, 20.0, 10, 2), (0.02, 0.0, 100, 5), (1.0, 0.0, 4, 1))


@functools.lru_cache(maxsize=None)
def dataset(n_loci=1600, seed=23):
    """-> {(group, sample index): (gpos, pcov, ncov, motif)}: n_loci loci of the two sequences, both ends of each among them.  The
    reference is cut into stretches of 90 bases; in a stretch group 1 lies above group 2, below it, or level with it, and every
    sample draws its calls around its group's level, half of the loci with a level of its own (overdispersion).  Six loci in ten
    are CpG.  A sample misses one locus in ten and is below the minimum coverage at some."""
    rng = np.random.default_rng(seed)
    ends = [0, 2999, 3000, 4499]
    loci = np.sort(np.concatenate([ends, rng.choice(np.setdiff1d(np.arange(TOTAL), ends), n_loci - 4, replace=False)])).astype(np.int64)
    motif = rng.choice([0, 1, 2, 3], n_loci, p=[0.6, 0.15, 0.15, 0.1])
    state = rng.choice([1, -1, 0], TOTAL // 90 + 1, p=[0.3, 0.3, 0.4])[loci // 90]
    level = np.stack([0.5 + 0.3 * state, 0.5 - 0.3 * state], axis=1)
    noisy = rng.random(n_loci) < 0.5
    out = {}
    for g in (1, 2):
        for s in range(3):
            lv = np.where(noisy, np.clip(level[:, g - 1] + rng.normal(0, 0.08, n_loci), 0, 1), level[:, g - 1])
            n = rng.integers(3, 40, n_loci)
            k = rng.binomial(n, lv)
            present = rng.random(n_loci) < 0.9
            present[np.isin(loci, ends)] = True
            order = rng.permutation(np.flatnonzero(present))
            out[(g, s)] = (loci[order], k[order], (n - k)[order], motif[order])
    return out


@functools.lru_cache(maxsize=None)
def dataset_rows(min_reps=MIN_REPS):
    """the hm_group_t rows of dataset() from the restated loader and groups_ref.stat_f64"""
    ref = G.GroupLoader(TOTAL, MIN_COV)
    for (g, s), rows in sorted(dataset().items()):
        assert ref.begin_sample(g) == s and ref.load(*rows) >= 0
    tested = ref.tested(min_reps)
    rows = np.zeros(len(tested), ROW_DTYPE)
    for k, (gpos, motif, m1, p1, n1, m2, p2, n2) in enumerate(tested):
        d, D, phi, p = G.stat_f64(*ref.sums(gpos))
        rows[k] = (gpos, p1, n1, p2, n2, motif, m1, m2, d, D, phi, p)
    return rows
