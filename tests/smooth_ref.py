"""`smooth` restated: the kernel-smoothed rows of include/hifimeth_hip.h (hm_smooth_fetch) from (gpos, pcov, ncov, motif)
rows and the sequence offsets, twice -- window by window as the definition reads, and from running sums -- plus the two numbers
of hm_smooth_stats and the writer of the command's files.  Exact: the window sums are sums of non-negative int64 terms whose total
stays below 2^60 under the bound pcov, ncov < 2^31, so a window's int64 sum is the integer sum; the running sums are Python ints."""
import bisect
import itertools

import numpy as np

SMOOTH_DTYPE = np.dtype([("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("loci", "<i8"), ("wp", "<i8"), ("wn", "<i8")])
LOCUS_DTYPE = np.dtype([("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("motif", "<u4"), ("reserved", "<u4")])
CTX_NAME = ("CpG", "CHG", "CHH")
MAX_H = 16384


def locus_rows(gpos, pcov, ncov, motif):
    rows = np.zeros(len(gpos), LOCUS_DTYPE)
    rows["gpos"], rows["pcov"], rows["ncov"], rows["motif"] = gpos, pcov, ncov, motif
    return rows[np.argsort(rows["gpos"], kind="stable")]


def counting(rows, ctx, min_cov):
    """the counting loci of context ctx, ascending: (gpos, pcov, ncov) as int64 arrays"""
    rows = rows[np.argsort(rows["gpos"], kind="stable")]
    cov = rows["pcov"].astype(np.int64) + rows["ncov"].astype(np.int64)
    keep = (rows["motif"] == ctx) & (cov >= min_cov)
    return rows["gpos"][keep].astype(np.int64), rows["pcov"][keep].astype(np.int64), rows["ncov"][keep].astype(np.int64)


def sequence_of(offsets, g):
    """[S0, S1) of the sequence that holds global position g (empty sequences hold nothing)"""
    s = bisect.bisect_right(offsets, g) - 1
    return int(offsets[s]), int(offsets[s + 1])


def _rows(out):
    return np.array(out, SMOOTH_DTYPE) if out else np.zeros(0, SMOOTH_DTYPE)


def smooth_direct(rows, offsets, ctx, h, min_cov=1, min_loci=1, lo=0, hi=None):
    """the definition, window by window: O(loci x window)"""
    assert 1 <= h <= MAX_H and min_cov >= 1 and min_loci >= 1
    offsets = [int(x) for x in offsets]
    hi = offsets[-1] if hi is None else hi
    pos, pc, nc = counting(rows, ctx, min_cov)
    out = []
    for k in range(int(np.searchsorted(pos, lo)), int(np.searchsorted(pos, hi))):
        g = int(pos[k])
        s0, s1 = sequence_of(offsets, g)
        a, b = np.searchsorted(pos, max(s0, g - h + 1)), np.searchsorted(pos, min(s1 - 1, g + h - 1), side="right")
        w = h - np.abs(pos[a:b] - g)
        assert (w >= 1).all() and (w <= h).all()
        L, P, N = int(b - a), int((w * pc[a:b]).sum()), int((w * nc[a:b]).sum())
        if L >= min_loci:
            out.append((g, int(pc[k]), int(nc[k]), L, P, N))
    return _rows(out)


def smooth_prefix(rows, offsets, ctx, h, min_cov=1, min_loci=1, lo=0, hi=None):
    """the same from running sums over the counting loci, in Python ints: with S(v)[k] the sum of v over the first k loci and
    M(v)[k] that of position x v, the left half [x, g] weighs (h - g) S + M and the right half (g, y] weighs (h + g) S - M"""
    assert 1 <= h <= MAX_H and min_cov >= 1 and min_loci >= 1
    offsets = [int(x) for x in offsets]
    hi = offsets[-1] if hi is None else hi
    pos, pc, nc = (x.tolist() for x in counting(rows, ctx, min_cov))
    run = lambda v: [0] + list(itertools.accumulate(v))
    Sp, Sn = run(pc), run(nc)
    Mp, Mn = run(j * v for j, v in zip(pos, pc)), run(j * v for j, v in zip(pos, nc))
    out = []
    for k in range(bisect.bisect_left(pos, lo), bisect.bisect_left(pos, hi)):
        g = pos[k]
        s0, s1 = sequence_of(offsets, g)
        a, b = bisect.bisect_left(pos, max(s0, g - h + 1)), bisect.bisect_right(pos, min(s1 - 1, g + h - 1))
        m = k + 1                                             # the loci a .. k are the left half, g included; m .. b - 1 the right
        P = (h - g) * (Sp[m] - Sp[a]) + (Mp[m] - Mp[a]) + (h + g) * (Sp[b] - Sp[m]) - (Mp[b] - Mp[m])
        N = (h - g) * (Sn[m] - Sn[a]) + (Mn[m] - Mn[a]) + (h + g) * (Sn[b] - Sn[m]) - (Mn[b] - Mn[m])
        if b - a >= min_loci:
            out.append((g, pc[k], nc[k], b - a, P, N))
    return _rows(out)


def stats(row, h):
    """hm_smooth_stats: (smoothed level in percent, effective coverage)"""
    wp, wn = float(int(row["wp"])), float(int(row["wn"]))
    return 100.0 * wp / (wp + wn), (wp + wn) / h


def bed_text(rows, names, offsets, h):
    """the text of <prefix>.smooth.<ctx>.bed"""
    offsets = [int(x) for x in offsets]
    text = []
    for r in rows:
        s = bisect.bisect_right(offsets, int(r["gpos"])) - 1
        k = int(r["gpos"]) - offsets[s]
        level, eff = stats(r, h)
        text.append("%s\t%d\t%d\t%g\t%d\t%d\t%d\t%.3f\n" % (names[s], k, k + 1, level, r["pcov"], r["ncov"], r["loci"], eff))
    return "".join(text)


def write_outputs(prefix, rows_by_ctx, names, offsets, h, min_cov=1, min_loci=1):
    """<prefix>.smooth.<ctx>.bed for every context of rows_by_ctx ({ctx: LOCUS_DTYPE rows of ALL contexts the sample has}) and
    <prefix>.smooth.summary.tsv: ctx, counting loci, rows written, h -- one line per context that has a file, in context order.
    -> the paths written"""
    paths, summary = [], []
    for ctx in sorted(rows_by_ctx):
        rows = smooth_prefix(rows_by_ctx[ctx], offsets, ctx, h, min_cov, min_loci)
        paths.append("%s.smooth.%s.bed" % (prefix, CTX_NAME[ctx]))
        with open(paths[-1], "w") as f:
            f.write(bed_text(rows, names, offsets, h))
        summary.append("%s\t%d\t%d\t%d\n" % (CTX_NAME[ctx], len(counting(rows_by_ctx[ctx], ctx, min_cov)[0]), len(rows), h))
    paths.append(prefix + ".smooth.summary.tsv")
    with open(paths[-1], "w") as f:
        f.write("".join(summary))
    return paths


# ---- the cases of the two test files ------------------------------------------------------------------------------------------
BOUNDARY_LENGTHS = (1, 2, 5, 3000, 70000)
HALF_WIDTHS = (1, 2, 7, 500, 4096, 16384)


def boundary_rows(seed=11, density=0.3):
    """random loci of all three contexts at about 30 % of the positions of the BOUNDARY_LENGTHS sequences, counts 0 .. 6 on either
    side (loci without a call are dropped: the loader ignores them); the first and the last base of every sequence carry a locus,
    CpG and CHH in turn.  -> (rows, offsets)"""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(BOUNDARY_LENGTHS)]).astype(np.int64)
    total = int(offsets[-1])
    hit = rng.random(total) < density
    pcov, ncov, motif = rng.integers(0, 7, total), rng.integers(0, 7, total), rng.integers(0, 3, total)
    ends = np.concatenate([offsets[:-1], offsets[1:] - 1])
    hit[ends], pcov[ends], ncov[ends], motif[ends] = True, 3, 1, np.tile([0, 2], len(ends) // 2)
    gpos = np.flatnonzero(hit & (pcov + ncov > 0))
    return locus_rows(gpos, pcov[gpos], ncov[gpos], motif[gpos]), offsets


def exact_rows(mirror):
    """one sequence of 40 000 bases, every position a CpG locus with pcov = 2^31 - 1, ncov = 0 (mirror: the other way round)"""
    n, big = 40000, 2 ** 31 - 1
    z = np.zeros(n, np.int64)
    rows = locus_rows(np.arange(n), z if mirror else z + big, z + big if mirror else z, z)
    return rows, np.array([0, n], np.int64)
