"""`regiondiff` restated in numpy, Python integers and mpmath; shares no code with hifimeth_amd.pileup.

interval_sums() is hm_sample_fetch_intervals over the planes of a samples_ref.SampleLoader: per interval (clamped to [lo, hi)) and
opened sample the number of loci of one context at which the sample counts -- in complete mode at which all count -- and the sum
of their levels, from running sums in int64; interval_sums_by_loops() is the same thing locus by locus in Python integers, which
test_pileup_sample_intervals_cpu.py holds the running sums to.  welch() is hm_sample_interval_test in float64 with
scipy.special.betainc, welch_mp() the same statistic in mpmath at 50 digits from the exact integers.  bh() is Benjamini-Hochberg over
the finite p.  regiondiff_tsv() and regiondiff_summary_tsv() are the texts of the command's files.  dataset() / loaded() are the
data the GPU tests load, interval_classes() the intervals they ask for."""
import functools
import math
import sys

import numpy as np

from samples_ref import BELOW, SampleLoader

CTX = ("CpG", "CHG", "CHH")
DBL_MIN = sys.float_info.min
NAN = math.nan


# ---- the sums -------------------------------------------------------------------------------------------------------------------------
def interval_sums(ref, start, end, ctx, lo=0, hi=None, complete=False):
    """-> uint64 (n_iv, M, 2): (n, su) per interval and opened sample"""
    hi = ref.total if hi is None else hi
    M = ref.opened
    c, counts, u = ref._selected(0, ref.total, complete)
    counts = counts & (c == ctx)
    cn = np.zeros((M, ref.total + 1), np.int64)
    cu = np.zeros((M, ref.total + 1), np.int64)
    np.cumsum(counts, axis=1, out=cn[:, 1:])
    np.cumsum(np.where(counts, u, 0), axis=1, out=cu[:, 1:])
    a = np.clip(np.asarray(start, np.int64), lo, hi)
    b = np.clip(np.asarray(end, np.int64), lo, hi)
    out = np.zeros((len(a), M, 2), np.uint64)
    out[:, :, 0] = (cn[:, b] - cn[:, a]).T
    out[:, :, 1] = (cu[:, b] - cu[:, a]).T
    return out


def interval_sums_by_loops(ref, start, end, ctx, lo=0, hi=None, complete=False):
    """interval_sums(), locus by locus from the definition -> [[(n, su)] * M] * n_iv in Python integers"""
    hi = ref.total if hi is None else hi
    M = ref.opened
    out = []
    for s0, e0 in zip(start, end):
        acc = [[0, 0] for _ in range(M)]
        for g in range(min(max(int(s0), lo), hi), min(max(int(e0), lo), hi)):
            if min(int(ref.planes["key"][g]) & 3, 2) != ctx:
                continue
            v = [int(x) for x in ref.level[:M, g]]
            ok = [x != 0 and x != BELOW for x in v]
            if complete and not all(ok):
                continue
            for s in range(M):
                if ok[s]:
                    acc[s][0] += 1
                    acc[s][1] += v[s] - 1
        out.append([tuple(x) for x in acc])
    return out


# ---- the test -------------------------------------------------------------------------------------------------------------------------
def _used(sums, group, min_loci):
    """-> per group the (n, su) of its used samples, ascending in sample index"""
    return [[(int(n), int(su)) for (n, su), g in zip(sums, group) if g == k and int(n) >= min_loci] for k in (1, 2)]


def welch(sums, group, min_loci=3, min_reps=2):
    """one interval: sums = M pairs (n, su) -> (m1, m2, n1, n2, mean1, mean2, t, df, p) in float64"""
    from scipy.special import betainc
    used = _used(sums, group, min_loci)
    m = [len(x) for x in used]
    loci = [sum(n for n, _ in x) for x in used]
    xs = [[100.0 * float(su) / (float(n) * 32768.0) for n, su in x] for x in used]
    mean = [sum(x) / len(x) if x else NAN for x in xs]
    if m[0] < min_reps or m[1] < min_reps:
        return (m[0], m[1], loci[0], loci[1], mean[0], mean[1], NAN, NAN, NAN)
    var = [sum((v - mu) * (v - mu) for v in x) / (len(x) - 1) for x, mu in zip(xs, mean)]
    a1, a2 = var[0] / m[0], var[1] / m[1]
    se2, d = a1 + a2, mean[0] - mean[1]
    if se2 == 0.0:
        if d == 0.0:
            return (m[0], m[1], loci[0], loci[1], mean[0], mean[1], 0.0, float(m[0] + m[1] - 2), 1.0)
        return (m[0], m[1], loci[0], loci[1], mean[0], mean[1], math.copysign(math.inf, d), NAN, NAN)
    t = d / math.sqrt(se2)
    df = se2 * se2 / (a1 * a1 / (m[0] - 1) + a2 * a2 / (m[1] - 1))
    p = float(betainc(0.5 * df, 0.5, df / (df + t * t)))
    return (m[0], m[1], loci[0], loci[1], mean[0], mean[1], t, df, min(1.0, max(p, DBL_MIN)))


def welch_mp(sums, group, min_loci=3, min_reps=2):
    """welch() at 50 digits from the exact integers -> (t, df, p) as mpf, or None where welch() gives no finite t, df, p"""
    import mpmath
    with mpmath.workdps(50):
        used = _used(sums, group, min_loci)
        m = [len(x) for x in used]
        if m[0] < min_reps or m[1] < min_reps:
            return None
        xs = [[mpmath.mpf(100 * su) / (n * 32768) for n, su in x] for x in used]
        mean = [mpmath.fsum(x) / len(x) for x in xs]
        var = [mpmath.fsum((v - mu) ** 2 for v in x) / (len(x) - 1) for x, mu in zip(xs, mean)]
        a1, a2 = var[0] / m[0], var[1] / m[1]
        se2 = a1 + a2
        if se2 == 0:
            return None
        t = (mean[0] - mean[1]) / mpmath.sqrt(se2)
        df = se2 ** 2 / (a1 ** 2 / (m[0] - 1) + a2 ** 2 / (m[1] - 1))
        p = mpmath.betainc(df / 2, mpmath.mpf(1) / 2, 0, df / (df + t * t), regularized=True) if t != 0 else mpmath.mpf(1)
        return t, df, p


def relerr(got, want):
    """|got - want| / |want| of a float against an mpf; 0 where both are 0"""
    import mpmath
    with mpmath.workdps(50):
        if want == 0:
            return 0.0 if got == 0 else math.inf
        return float(abs(mpmath.mpf(got) - want) / abs(want))


def bh(p):
    """Benjamini-Hochberg among the finite entries of p, as R's p.adjust: q = running minimum from the largest p down of
    min(1, p m / R), R = the entries with p <= it; NaN stays NaN"""
    p = [float(x) for x in p]
    fin = sorted((x, i) for i, x in enumerate(p) if x == x)
    m = len(fin)
    q = [NAN] * len(p)
    run = 1.0
    for k in range(m - 1, -1, -1):
        R = k + 1
        while R < m and fin[R][0] == fin[k][0]:
            R += 1
        run = min(run, min(1.0, fin[k][0] * float(m) / float(R)))
        q[fin[k][1]] = run
    return q


# ---- the texts ------------------------------------------------------------------------------------------------------------------------
def _g6(v):
    return "nan" if v != v else "%.6g" % v


def regiondiff_tsv(intervals, tests, q):
    """intervals: (chrom, start, end, name, strand) per interval; tests: welch() tuples; q: bh() of their p"""
    text = "#chrom\tstart\tend\tname\tstrand\tm1\tm2\tloci1\tloci2\tmean1\tmean2\tdiff\tt\tdf\tp\tq\n"
    for iv, (m1, m2, n1, n2, mean1, mean2, t, df, p), qv in zip(intervals, tests, q):
        text += "%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t" % (*iv, m1, m2, n1, n2)
        text += "\t".join(_g6(v) for v in (mean1, mean2, mean1 - mean2, t, df, p, qv)) + "\n"
    return text


def regiondiff_summary_tsv(tests, q):
    """tests, q: {context index: ...} of the contexts written"""
    text = "ctx\tintervals\ttested\tq<=0.05\tq<=0.01\n"
    for c in sorted(tests):
        text += "%s\t%d\t%d\t%d\t%d\n" % (CTX[c], len(tests[c]), sum(1 for r in tests[c] if r[6] == r[6]), sum(1 for v in q[c] if v <= 0.05),
                                          sum(1 for v in q[c] if v <= 0.01))
    return text


# ---- the data set of the GPU tests -----------------------------------------------------------------------------------------------------
def lengths(block):
    """three sequences of 3 x block + 777 bases, none a multiple of anything"""
    return (block + 300, block, block + 477)


@functools.lru_cache(maxsize=None)
def dataset(n_samples, block):
    """-> per sample (gpos, pcov, ncov, motif) in shuffled order.  About half of the positions are loci, the three contexts (motifs
    0 .. 3) interleaved.  A quarter of the loci are `core`: every sample has 5 .. 40 calls there, so complete mode keeps them;
    elsewhere a sample has a row with probability 0.8 and 1 .. 12 calls, on both sides of the minimum coverage 5.  A tenth of the
    rows have no methylated call (stored 1, u = 0), a tenth only methylated calls (stored 32769, u = 32768).  The second half of
    the samples is up to 50 points lower in the middle sequence, so the groups differ there.  The four positions around every block
    edge and both ends of the reference are core loci."""
    total = sum(lengths(block))
    rng = np.random.default_rng(2000 + n_samples)
    locus = rng.random(total) < 0.5
    edges = np.array([0, 1, total - 2, total - 1] + [b * block + d for b in (1, 2, 3) for d in (-2, -1, 0, 1)])
    locus[edges] = True
    g = np.flatnonzero(locus)
    motif = rng.integers(0, 4, len(g))
    core = rng.random(len(g)) < 0.25
    core[np.isin(g, edges)] = True
    base = rng.random(len(g))
    middle = (g >= lengths(block)[0]) & (g < lengths(block)[0] + lengths(block)[1])
    out = []
    for s in range(n_samples):
        has = core | (rng.random(len(g)) < 0.8)
        cov = np.where(core, rng.integers(5, 41, len(g)), rng.integers(1, 13, len(g)))
        shift = np.where(middle & (s >= n_samples // 2), -0.5, 0.0)
        p = rng.binomial(cov, np.clip(base + shift + rng.normal(0, 0.05, len(g)), 0, 1))
        kind = rng.random(len(g))
        p = np.where(kind < 0.1, 0, np.where(kind < 0.2, cov, p))
        order = rng.permutation(np.flatnonzero(has))
        out.append((g[order], p[order], (cov - p)[order], motif[order]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def loaded(n_samples, block, opened=None):
    ref = SampleLoader(sum(lengths(block)), n_samples)
    for rows in dataset(n_samples, block)[:opened]:
        ref.open()
        ref.load(*rows)
    return ref


def interval_classes(ref, ctx, block, lo, hi):
    """-> [(class, start, end)]: every class of interval the query kernel tells apart, for the range [lo, hi) of `ref`"""
    total = ref.total
    ok = (ref.level[:ref.opened] != 0) & (ref.level[:ref.opened] != BELOW)
    hit = np.flatnonzero(ok.all(axis=0) & (np.minimum(ref.planes["key"] & 3, 2) == ctx) & (np.arange(total) >= lo) & (np.arange(total) < hi))
    g = int(hit[len(hit) // 2])                                   # a locus of the context at which every sample counts
    e1, e2, e3 = lo + block, lo + 2 * block, lo + 3 * block       # the block edges of the range
    assert lo + 5 < e1 and e3 + 5 < hi
    out = [("empty", g, g), ("empty at lo", lo, lo), ("one base on a counting locus", g, g + 1),
           ("inside one block", lo + 5, lo + 700), ("starts on a block edge", e1, e1 + 333), ("ends on a block edge", e2 - 333, e2),
           ("one whole block", e1, e2), ("two partial blocks, none between", e1 - 100, e1 + 100), ("two partial blocks, one between", e1 - 7, e2 + 9),
           ("two partial blocks, two between", e1 - 1, e3 + 1), ("edge to edge over two blocks", e1, e3), ("the whole range", lo, hi),
           ("the whole reference", 0, total), ("past lo", lo - 50 if lo >= 50 else -50, lo + 60), ("past hi", hi - 60, hi + 50),
           ("past both", -5, total + 5), ("wholly below", -30, lo), ("wholly above", hi, hi + 30), ("far outside", total + 10, total + 20),
           ("duplicate", lo + 5, lo + 700), ("nested", lo + 100, lo + 200), ("overlapping", lo + 600, e1 + 50),
           ("descending 3", e2 + 10, e2 + 90), ("descending 2", e1 + 10, e1 + 90), ("descending 1", lo + 10, lo + 90)]
    return out


# ---- the cases of the statistic: hand-made ones and the tiles of the data set ------------------------------------------------------------
GROUPS6 = (1, 1, 1, 2, 2, 2)
HAND = {  # name -> (M pairs (n, su), group): every class of outcome
    "tested, far apart": ([(10, 10 * 30000), (12, 12 * 29000), (9, 9 * 31000), (10, 10 * 3000), (11, 11 * 2500), (10, 10 * 4000)], GROUPS6),
    "tested, close": ([(10, 163840), (12, 200000), (9, 140000), (10, 165000), (11, 170000), (10, 150000)], GROUPS6),
    "tested, one group constant": ([(4, 4 * 1000), (8, 8 * 1000), (5, 5 * 1000), (10, 99999), (11, 170000), (10, 150000)], GROUPS6),
    "tested, two against five": ([(30, 500000), (31, 400000), (40, 77), (41, 1000000), (29, 3), (50, 50 * 32768), (3, 0)], (1, 1, 2, 2, 2, 2, 2)),
    "tested, a sample out of it": ([(10, 163840), (12, 200000), (9, 9 * 32768), (10, 165000), (11, 170000), (10, 150000)], (1, 1, 0, 2, 2, 2)),
    "tested, equal means with spread": ([(10, 100000), (10, 200000), (10, 100000), (10, 200000)], (1, 1, 2, 2)),
    "untested, too few loci": ([(10, 163840), (2, 20000), (2, 14000), (10, 165000), (11, 170000), (10, 150000)], GROUPS6),
    "untested, an empty group": ([(10, 163840), (12, 200000), (9, 140000), (0, 0), (0, 0), (1, 5)], GROUPS6),
    "untested, nothing": ([(0, 0)] * 6, GROUPS6),
    "se2 = 0, equal means": ([(4, 4 * 1000), (8, 8 * 1000), (5, 5 * 1000), (3, 3 * 1000), (7, 7 * 1000), (10, 10 * 1000)], GROUPS6),
    "se2 = 0, unequal means": ([(4, 4 * 1000), (8, 8 * 1000), (5, 5 * 1000), (3, 3 * 2000), (7, 7 * 2000), (10, 10 * 2000)], GROUPS6),
    "se2 = 0, unequal the other way": ([(4, 4 * 32768), (8, 8 * 32768), (3, 0), (7, 0)], (2, 2, 1, 1)),
}


@functools.lru_cache(maxsize=None)
def cases(block=4096):
    """-> [(pairs, group)]: HAND, then the tiles of 300 bases of the six-sample data set in every context, pairwise"""
    ref = loaded(6, block)
    starts = np.arange(0, ref.total, 300)
    out = list(HAND.values())
    for c in range(3):
        for row in interval_sums(ref, starts, starts + 300, c).tolist():
            out.append(([tuple(x) for x in row], GROUPS6))
    return out


@functools.lru_cache(maxsize=None)
def e_ref():
    """the float64 form's worst relative error against mpmath over cases() -> {"t", "df", "p"}"""
    worst = {"t": 0.0, "df": 0.0, "p": 0.0}
    for pairs, group in cases():
        want = welch_mp(pairs, group)
        if want is None:
            continue
        got = welch(pairs, group)
        for k, a, b in zip(("t", "df", "p"), got[6:], want):
            worst[k] = max(worst[k], relerr(a, b))
    return worst
