"""`samplecorr` restated in numpy and Python integers; shares no code with hifimeth_amd.pileup.

SampleLoader is hm_sample_open / hm_sample_load: the combined planes, the uint16 level planes with their stored values
(0 nothing seen, u + 1, 0xFFFF seen below the coverage), the duplicates, the error kinds in their check order, the voiding.  Its
sums() are the six integer sums of every pair i <= j per context over any [lo, hi), pairwise or complete, as matrix products in
int64; sums_by_loops() is the same thing locus by locus in Python integers, which test_pileup_samples_cpu.py holds the products to.
corr() is r and the two means from Python integers (exact num, va, vb, one conversion each).  The three *_tsv functions are the
texts of the command's files.  dataset(n) is the data the GPU tests load."""
import functools
import math

import numpy as np

HM_EINVAL, HM_EDATA, HM_ESTATE = -1, -4, -5
LIMIT = 1 << 20                                               # a sample's pcov + ncov at a locus stays below this
BELOW = 0xFFFF
MAX_SAMPLES = 64
MIN_COV = 5
KINDS = ("gpos outside the reference", "negative count", "count above 2^20 - 1", "motif above 3", "locus given twice in one sample")
CTX = ("CpG", "CHG", "CHH")
LENGTHS = (8191, 4099, 7777)                                  # three sequences, none a multiple of anything
OFFSETS = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
TOTAL = int(OFFSETS[-1])
ENDS = [0, TOTAL - 1] + [int(o) + d for o in OFFSETS[1:-1] for d in (-1, 0)]     # position 0, the last base, both sides of every boundary


def level(k, n):
    return (k << 15) // n


class SampleLoader:
    def __init__(self, total, n_samples, min_cov=MIN_COV):
        self.total, self.n_samples, self.min_cov = total, n_samples, min_cov
        self.planes = {k: np.zeros(total, np.int64) for k in ("pcov", "ncov", "key")}
        self.level = np.zeros((n_samples, total), np.uint16)
        self.opened, self.failed = 0, False
        self.bad = {k: 0 for k in KINDS}

    def open(self):
        if self.failed or self.opened >= self.n_samples:
            return HM_ESTATE
        self.opened += 1
        return self.opened - 1

    def load(self, gpos, pcov, ncov, motif):
        if self.failed or not self.opened:
            return HM_ESTATE
        mine = self.level[self.opened - 1]
        self.bad = {k: 0 for k in KINDS}
        wrote = 0
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
            elif mine[g] != 0:
                self.bad[KINDS[4]] += 1
            else:
                counts = p + n >= self.min_cov
                mine[g] = level(p, p + n) + 1 if counts else BELOW
                self.planes["key"][g] = max(self.planes["key"][g], m)
                if counts:
                    self.planes["pcov"][g] += p
                    self.planes["ncov"][g] += n
                wrote += 1
        if sum(self.bad.values()):
            self.failed = True
            return HM_EDATA
        return wrote

    def loci(self):
        """covered loci of the combined planes -> gpos, pcov, ncov, motif"""
        p, n = self.planes["pcov"], self.planes["ncov"]
        g = np.flatnonzero((p | n) != 0)
        return g, p[g], n[g], self.planes["key"][g] & 3

    def _selected(self, lo, hi, complete):
        """-> (ctx per position of [lo, hi), counts (M, hi - lo) bool, levels (M, hi - lo) int64, 0 where the sample does not count)"""
        M = self.opened
        L = self.level[:M, lo:hi]
        counts = (L != 0) & (L != BELOW)
        if complete:
            counts = counts & counts.all(axis=0)
        u = np.where(counts, L.astype(np.int64) - 1, 0)
        return np.minimum(self.planes["key"][lo:hi] & 3, 2), counts, u

    def sums(self, lo=0, hi=None, complete=False):
        """-> [(i, j, ctx, n, si, sj, sii, sjj, sij)] in the order of hm_sample_fetch_sums, Python integers"""
        hi = self.total if hi is None else hi
        ctx, counts, u = self._selected(lo, hi, complete)
        out = []
        for c in range(3):
            C = counts[:, ctx == c].astype(np.int64)
            U = u[:, ctx == c]
            Q = U * U
            n, si, sj, sii, sjj, sij = C @ C.T, U @ C.T, C @ U.T, Q @ C.T, C @ Q.T, U @ U.T
            out += [(i, j, c, *(int(x[i, j]) for x in (n, si, sj, sii, sjj, sij))) for i in range(self.opened) for j in range(i, self.opened)]
        return out

    def sums_by_loops(self, lo=0, hi=None, complete=False):
        """sums(), locus by locus from the definition"""
        hi = self.total if hi is None else hi
        M = self.opened
        acc = {(c, i, j): [0] * 6 for c in range(3) for i in range(M) for j in range(i, M)}
        for g in range(lo, hi):
            v = [int(x) for x in self.level[:M, g]]
            ok = [x != 0 and x != BELOW for x in v]
            if not any(ok) or (complete and not all(ok)):
                continue
            c = min(int(self.planes["key"][g]) & 3, 2)
            for i in range(M):
                for j in range(i, M):
                    if ok[i] and ok[j]:
                        ui, uj = v[i] - 1, v[j] - 1
                        for k, x in enumerate((1, ui, uj, ui * ui, uj * uj, ui * uj)):
                            acc[(c, i, j)][k] += x
        return [(i, j, c, *acc[(c, i, j)]) for c in range(3) for i in range(M) for j in range(i, M)]


def corr(entry):
    """(i, j, ctx, n, si, sj, sii, sjj, sij) in Python integers -> (r, mean_i, mean_j): num, va, vb exact, each converted to float once"""
    _i, _j, _c, n, si, sj, sii, sjj, sij = (int(x) for x in entry)
    num, va, vb = n * sij - si * sj, n * sii - si * si, n * sjj - sj * sj
    r = math.nan if n < 2 or va == 0 or vb == 0 else float(num) / (math.sqrt(float(va)) * math.sqrt(float(vb)))
    mean = [math.nan if n == 0 else 100.0 * float(s) / (float(n) * 32768.0) for s in (si, sj)]
    return r, mean[0], mean[1]


def _by_pair(entries, ctx):
    return {(e[0], e[1]): e for e in entries if e[2] == ctx}


def samplecorr_tsv(names, entries, ctx):
    pairs = _by_pair(entries, ctx)
    text = "sample_i\tsample_j\tn\tmean_i\tmean_j\tr\n"
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            r, mi, mj = corr(pairs[(i, j)])
            text += "%s\t%s\t%d\t%.6g\t%.6g\t%.6g\n" % (names[i], names[j], pairs[(i, j)][3], mi, mj, r)
    return text


def samplecorr_matrix_tsv(names, entries, ctx):
    pairs = _by_pair(entries, ctx)
    text = "sample\t" + "\t".join(names) + "\n"
    for i in range(len(names)):
        text += names[i] + "".join("\t%.6g" % corr(pairs[(min(i, j), max(i, j))])[0] for j in range(len(names))) + "\n"
    return text


def samplecorr_samples_tsv(names, entries, contexts=(0, 1, 2)):
    """entries: the pairwise sums, whose diagonal is a sample's own counting loci"""
    text = "ctx\tsample\tn\tmean\n"
    for c in contexts:
        pairs = _by_pair(entries, c)
        for i in range(len(names)):
            text += "%s\t%s\t%d\t%.6g\n" % (CTX[c], names[i], pairs[(i, i)][3], corr(pairs[(i, i)])[1])
    return text


# ---- the data set of the GPU tests ------------------------------------------------------------------------------------------------------
ALL_BUT_ONE = 3001                                            # every sample but the last counts here


def pool(tile):
    """the loci of the data set: the contig ends, the last position of a tile and the first of the next (twice), ALL_BUT_ONE, and
    random ones; -> (sorted gpos, motif per locus in 0 .. 3, whether every sample has a row there: the named ones)"""
    rng = np.random.default_rng(11)
    fixed = ENDS + [tile - 1, tile, 7 * tile - 1, 7 * tile, 7 * tile + 1, ALL_BUT_ONE]
    g = np.unique(np.concatenate([fixed, rng.choice(TOTAL, 700, replace=False)])).astype(np.int64)
    return g, rng.integers(0, 4, len(g)), np.isin(g, fixed)


@functools.lru_cache(maxsize=None)
def dataset(n_samples, tile=256):
    """-> per sample (gpos, pcov, ncov, motif) in shuffled order.  A third of the loci are `core`: every sample has 5 .. 40 calls
    there, so complete mode keeps them.  Elsewhere a sample has a row with probability 0.8 and 1 .. 12 calls, on both sides of the
    minimum coverage 5.  The levels follow a locus effect plus a sample effect, so r spreads.  At ALL_BUT_ONE all samples count but
    the last, which has 2 calls."""
    g, motif, always = pool(tile)
    rng = np.random.default_rng(1000 + n_samples)
    core = rng.random(len(g)) < 1 / 3
    core[g == ALL_BUT_ONE] = True
    base = rng.random(len(g))
    out = []
    for s in range(n_samples):
        has = core | always | (rng.random(len(g)) < 0.8)
        cov = np.where(core, rng.integers(5, 41, len(g)), rng.integers(1, 13, len(g)))
        if s == n_samples - 1:
            cov[g == ALL_BUT_ONE] = 2
        p = rng.binomial(cov, np.clip(base + rng.normal(0, 0.05 + 0.3 * s / n_samples, len(g)), 0, 1))
        order = rng.permutation(np.flatnonzero(has))
        out.append((g[order], p[order], (cov - p)[order], motif[order]))
    return tuple(out)


def loaded(n_samples, tile=256, opened=None, min_cov=MIN_COV):
    ref = SampleLoader(TOTAL, n_samples, min_cov)
    for rows in dataset(n_samples, tile)[:opened]:
        ref.open()
        ref.load(*rows)
    return ref
