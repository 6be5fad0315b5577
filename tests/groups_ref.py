"""`groupdiff` restated in numpy, scipy and mpmath; shares no code with hifimeth_amd.pileup.

GroupLoader is hm_pileup_group_sample / hm_pileup_load_sample_loci: the combined and partition planes, the moment and sample-count
planes, the seen set of the open sample, the coverage filter, the error kinds in their order, the voiding.  stat_f64 is the
statistic of include/hifimeth_hip.h in float64 from its formulas, with scipy.special.betainc for the last step; stat_mp the same
from exact rationals in mpmath at 50 digits.  bh is the Benjamini-Hochberg rule of hm_group_qvalues.  dataset() is the random
3 + 3 data set the GPU tests load, EDGE the hand-made loci, e_ref() the worst relative error of stat_f64 against stat_mp over both."""
import functools
import sys

import numpy as np

HM_EINVAL, HM_EDATA, HM_ESTATE = -1, -4, -5
DBL_MIN = sys.float_info.min
LIMIT = 1 << 20                                               # a sample's pcov + ncov at a locus stays below this
MAX_SAMPLES = 255
KINDS = ("gpos outside the reference", "negative count", "count above 2^20 - 1", "motif above 3", "locus given twice in one sample")


class GroupLoader:
    def __init__(self, total, min_cov=5):
        self.total, self.min_cov = total, min_cov
        self.planes = {k: np.zeros(total, np.int64) for k in ("pcov", "ncov", "key", "pcov1", "ncov1", "pcov2", "ncov2")}
        self.moment = {g: np.zeros(total, np.uint64) for g in (1, 2)}
        self.samples = {g: np.zeros(total, np.int64) for g in (1, 2)}
        self.n_samples = {1: 0, 2: 0}
        self.open, self.seen, self.failed = 0, set(), False
        self.bad = {k: 0 for k in KINDS}

    def begin_sample(self, part):
        if part not in (1, 2):
            return HM_EINVAL
        if self.failed or self.n_samples[part] >= MAX_SAMPLES:
            return HM_ESTATE
        self.open, self.seen = part, set()
        self.n_samples[part] += 1
        return self.n_samples[part] - 1

    def load(self, gpos, pcov, ncov, motif):
        if self.failed or not self.open:
            return HM_ESTATE
        g_ = self.open
        self.bad = {k: 0 for k in KINDS}
        added = 0
        for g, p, n, m in zip(*(np.asarray(x, np.int64).tolist() for x in (gpos, pcov, ncov, np.broadcast_to(motif, np.shape(gpos))))):
            if g < 0 or g >= self.total:
                self.bad[KINDS[0]] += 1
            elif p < 0 or n < 0:
                self.bad[KINDS[1]] += 1
            elif p + n >= LIMIT:
                self.bad[KINDS[2]] += 1
            elif m > 3:
                self.bad[KINDS[3]] += 1
            elif p + n == 0:
                continue
            elif g in self.seen:
                self.bad[KINDS[4]] += 1
            else:
                self.seen.add(g)
                if p + n < self.min_cov:
                    continue
                for name, v in (("pcov", p), ("ncov", n), ("pcov%d" % g_, p), ("ncov%d" % g_, n)):
                    self.planes[name][g] += v
                self.planes["key"][g] = max(self.planes["key"][g], m)
                self.moment[g_][g] += np.uint64((p * p << 20) // (p + n))
                self.samples[g_][g] += 1
                added += 1
        if sum(self.bad.values()):
            self.failed = True
            return HM_EDATA
        return added

    def loci(self, part=0):
        """covered loci of the combined planes (part 0) or of a group's -> gpos, pcov, ncov, motif"""
        tag = "" if part == 0 else str(part)
        p, n = self.planes["pcov" + tag], self.planes["ncov" + tag]
        g = np.flatnonzero((p | n) != 0)
        return g, p[g], n[g], self.planes["key"][g] & 3

    def tested(self, min_reps, lo=0, hi=None):
        """-> [(gpos, motif, m1, pcov1, ncov1, m2, pcov2, ncov2)] of [lo, hi), ascending"""
        hi = self.total if hi is None else hi
        m1, m2 = self.samples[1], self.samples[2]
        g = np.flatnonzero((m1 >= min_reps) & (m2 >= min_reps) & (m1 + m2 - 2 >= 1))
        g = g[(g >= lo) & (g < hi)]
        P = self.planes
        return [(int(i), int(P["key"][i] & 3), int(m1[i]), int(P["pcov1"][i]), int(P["ncov1"][i]), int(m2[i]), int(P["pcov2"][i]), int(P["ncov2"][i]))
                for i in g]

    def sums(self, gpos):
        """-> (K1, N1, Q1, m1, K2, N2, Q2, m2) of a locus, Python integers: the arguments of stat_f64 and stat_mp"""
        P = self.planes
        out = []
        for g in (1, 2):
            k = int(P["pcov%d" % g][gpos])
            out += [k, k + int(P["ncov%d" % g][gpos]), int(self.moment[g][gpos]), int(self.samples[g][gpos])]
        return tuple(out)


def sums_of(group1, group2, min_cov=1):
    """the sums of a locus from the samples' (k, n) pairs -> (K1, N1, Q1, m1, K2, N2, Q2, m2)"""
    out = []
    for grp in (group1, group2):
        cnt = [(k, n) for k, n in grp if n >= min_cov]
        out += [sum(k for k, _ in cnt), sum(n for _, n in cnt), sum((k * k << 20) // n for k, n in cnt), len(cnt)]
    return tuple(out)


def np_diff(K1, N1, K2, N2):
    return np.float64(100.0) * np.float64(K1) / np.float64(N1) - np.float64(100.0) * np.float64(K2) / np.float64(N2)


def stat_f64(K1, N1, Q1, m1, K2, N2, Q2, m2):
    """-> (diff, D, phi, p) in float64, formula by formula"""
    from scipy.special import betainc
    f = np.float64
    nu = m1 + m2 - 2
    p0, u0 = f(K1 + K2) / f(N1 + N2), f(N1 + N2 - K1 - K2) / f(N1 + N2)
    s, x2 = [], []
    with np.errstate(all="ignore"):
        for K, N, Q in ((K1, N1, Q1), (K2, N2, Q2)):
            ph, uh = f(K) / f(N), f(N - K) / f(N)
            a = f(0.0) if K == 0 else f(K) * np.log(ph / p0)
            b = f(0.0) if N == K else f(N - K) * np.log(uh / u0)
            s.append(a + b)
            t = f(0.0) if K in (0, N) else (f(Q) * f(2.0 ** -20) - f(K) * f(K) / f(N)) / (ph * uh)
            x2.append(max(t, f(0.0)))
    D = max(f(2.0) * (s[0] + s[1]), f(0.0))
    phi = max(f(1.0), (x2[0] + x2[1]) / f(nu))
    if D == 0.0:
        p = f(1.0)
    else:
        F = D / phi
        p = max(f(betainc(f(nu) / 2, 0.5, f(nu) / (f(nu) + F))), f(DBL_MIN))
    return np_diff(K1, N1, K2, N2), D, phi, p


def stat_mp(K1, N1, Q1, m1, K2, N2, Q2, m2):
    """-> (D, phi, p) as mpmath numbers at 50 digits, from exact integers; p is 1 when D is 0 and is NOT floored"""
    import mpmath as mp
    with mp.workdps(50):
        nu = m1 + m2 - 2
        K0, N0 = K1 + K2, N1 + N2
        D, X2 = mp.mpf(0), mp.mpf(0)
        for K, N, Q in ((K1, N1, Q1), (K2, N2, Q2)):
            if K:
                D += K * mp.log(mp.mpf(K * N0) / (N * K0))
            if N - K:
                D += (N - K) * mp.log(mp.mpf((N - K) * N0) / (N * (N0 - K0)))
            if K not in (0, N):
                t = (mp.mpf(Q) / (1 << 20) - mp.mpf(K * K) / N) / (mp.mpf(K) / N * (mp.mpf(N - K) / N))
                X2 += max(t, 0)
        D = max(2 * D, mp.mpf(0))
        phi = max(mp.mpf(1), X2 / nu)
        if K1 * N2 == K2 * N1:                                # equal proportions: D is 0, not the rounding of the logs
            return mp.mpf(0), phi, mp.mpf(1)
        F = D / phi
        return D, phi, mp.betainc(mp.mpf(nu) / 2, mp.mpf(1) / 2, 0, nu / (nu + F), regularized=True)


def rel(got, want):
    """|got - want| / |want| with want an mpmath number; 0 when both are 0"""
    import mpmath as mp
    with mp.workdps(50):
        want = mp.mpf(want)
        if want == 0:
            return 0.0 if got == 0 else float("inf")
        return float(abs(mp.mpf(float(got)) - want) / abs(want))


def bh(p, ctx):
    """q per row: Benjamini-Hochberg among the rows of the row's context, min(motif, 2); m per context"""
    p, ctx = np.asarray(p, np.float64), np.minimum(np.asarray(ctx), 2)
    q, m = np.full(len(p), np.nan), [0, 0, 0]
    for c in range(3):
        idx = np.flatnonzero(ctx == c)
        m[c] = len(idx)
        if not len(idx):
            continue
        pc = p[idx]
        order = np.argsort(pc, kind="stable")
        ps = pc[order]
        R = np.searchsorted(ps, ps, side="right")             # loci with p <= this one
        raw = np.minimum(1.0, ps * float(m[c]) / R.astype(np.float64))
        q[idx[order]] = np.minimum.accumulate(raw[::-1])[::-1]
    return q, m


# ---- the hand-made loci: name -> (samples of group 1, samples of group 2, min_reps at which the locus is tested) ----------------------
BIG = LIMIT - 1
EDGE = {
    "D = 0": ([(5, 10), (10, 20)], [(3, 6), (6, 12)], 2),
    "D = 0 with spread": ([(2, 10), (8, 10)], [(5, 10), (5, 10)], 2),
    "both groups at 0": ([(0, 10), (0, 5)], [(0, 7), (0, 9)], 2),
    "group 1 at 0": ([(0, 10), (0, 12)], [(5, 10), (7, 12)], 2),
    "group 1 at 1": ([(10, 10), (8, 8)], [(3, 10), (2, 9), (4, 11)], 2),
    "nu = 1": ([(3, 10), (6, 10)], [(9, 10)], 1),
    "near 2^20 per sample": ([(700000, BIG), (700100, BIG)], [(699000, BIG), (699500, BIG - 1)], 2),
    "near 2^20, all methylated against none": ([(BIG, BIG), (BIG, BIG)], [(0, BIG), (0, BIG)], 2),
    "overdispersed, nu = 4": ([(1, 30), (15, 30), (29, 30)], [(2, 30), (3, 30), (4, 30)], 3),
    "p near DBL_MIN": ([(870, 870)] * 100, [(0, 870)] * 100, 2),       # 1.7e-307, eight times DBL_MIN
    "p below DBL_MIN": ([(BIG, BIG)] * 128, [(0, BIG)] * 128, 2),
    "many samples, overdispersed": ([(k % 17 + 1, 40) for k in range(60)], [(k % 5 + 30, 40) for k in range(60)], 2),
}


# ---- the random data set of the GPU tests: three contigs, three samples per group -----------------------------------------------------
LENGTHS = (3001, 2500, 1777)
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)])
TOTAL = int(OFFSETS[-1])
ENDS = [int(x) for s in range(3) for x in (OFFSETS[s], OFFSETS[s + 1] - 1)]
MIN_COV = 5


@functools.lru_cache(maxsize=None)
def dataset(n_loci=500, seed=11):
    """-> {(group, sample index): (gpos, pcov, ncov, motif)}: n_loci loci, the contig ends among them with every sample counting.
    A locus has a level per group (equal in half of them); each sample draws its own level around it (so some loci are
    overdispersed) or takes it as it is, a coverage of 0 .. 39 (below MIN_COV in some, 0 = row absent in some) and binomial calls.
    Rows are shuffled; about one in sixteen present rows carries no count."""
    rng = np.random.default_rng(seed)
    loci = np.concatenate([ENDS, rng.choice(np.setdiff1d(np.arange(TOTAL), ENDS), n_loci - len(ENDS), replace=False)]).astype(np.int64)
    motif = rng.integers(0, 4, n_loci)
    level = rng.random((n_loci, 2))
    same = rng.random(n_loci) < 0.5
    level[same, 1] = level[same, 0]
    noisy = rng.random(n_loci) < 0.5
    out = {}
    for g in (1, 2):
        for s in range(3):
            lv = np.where(noisy, np.clip(level[:, g - 1] + rng.normal(0, 0.25, n_loci), 0, 1), level[:, g - 1])
            n = rng.integers(0, 40, n_loci)
            n[: len(ENDS)] = np.maximum(n[: len(ENDS)], MIN_COV + s)
            k = rng.binomial(n, lv)
            present = (n > 0) | (rng.random(n_loci) < 0.0625)
            order = rng.permutation(np.flatnonzero(present))
            out[(g, s)] = (loci[order], k[order], (n - k)[order], motif[order])
    return out


@functools.lru_cache(maxsize=None)
def dataset_loader():
    ref = GroupLoader(TOTAL, MIN_COV)
    for (g, s), rows in sorted(dataset().items()):
        assert ref.begin_sample(g) == s
        assert ref.load(*rows) == int((rows[1] + rows[2] >= MIN_COV).sum())
    return ref


@functools.lru_cache(maxsize=None)
def cases():
    """every locus the statistic is checked on: name -> its sums.  The hand-made ones and the data set's loci tested at min_reps 1"""
    out = {name: sums_of(g1, g2) for name, (g1, g2, _r) in EDGE.items()}
    ref = dataset_loader()
    for row in ref.tested(1):
        out["locus %d" % row[0]] = ref.sums(row[0])
    return out


@functools.lru_cache(maxsize=None)
def references():
    """name -> ((diff, D, phi, p) in float64, (D, phi, p) in mpmath)"""
    return {name: (stat_f64(*s), stat_mp(*s)) for name, s in cases().items()}


@functools.lru_cache(maxsize=None)
def e_ref():
    """-> {"D", "phi", "p"}: the worst relative error of the float64 form against mpmath over cases(); p below DBL_MIN is left out
    (both forms floor it)"""
    worst = {"D": 0.0, "phi": 0.0, "p": 0.0}
    for (_d, D, phi, p), (mD, mphi, mp_) in references().values():
        worst["D"] = max(worst["D"], rel(D, mD))
        worst["phi"] = max(worst["phi"], rel(phi, mphi))
        if mp_ >= DBL_MIN:
            worst["p"] = max(worst["p"], rel(p, mp_))
    return worst
