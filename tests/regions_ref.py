"""Plain numpy restatement of `pileup -R` / `pileup -J` (include/hifimeth_hip.h: methylation of given intervals, metaplots): from loci
rows or three plane arrays to the sums per interval, the metaplot's table and the text of both outputs.  Plain module, imported by
test_pileup_regions_cpu.py and test_gpu_pileup_regions.py.  Nothing here is shared with the library: the definition in the header
is the specification, and the sums are taken as differences of whole-range running sums, with no blocks anywhere.
"""
import numpy as np

CTX = ("CpG", "CHG", "CHH")
QUANTITIES = ("n_loci", "pcov", "ncov", "ppm")


def locus_ppm(p, n):
    """(2 000 000 p + cov) / (2 cov) in integer division, cov = p + n > 0: the fraction in parts per million, rounded half up"""
    p, cov = int(p), int(p) + int(n)
    return (2000000 * p + cov) // (2 * cov)


def planes_from_loci(loci, n_loci):
    """LOCUS_DTYPE-like rows (gpos, pcov, ncov, motif) -> (pcov, ncov, key) planes over [0, n_loci)"""
    pc, nc, ky = (np.zeros(n_loci, np.int64) for _ in range(3))
    g = np.asarray(loci["gpos"], np.int64)
    pc[g], nc[g], ky[g] = loci["pcov"], loci["ncov"], loci["motif"]
    return pc, nc, ky


class Running:
    """running sums of the four quantities per context over planes whose element 0 is locus `base`"""

    def __init__(self, pcov, ncov, key, min_cov=1, base=0):
        pc, nc = np.asarray(pcov).astype(np.int64), np.asarray(ncov).astype(np.int64)
        ctx = np.asarray(key).astype(np.int64) & 3
        cov = pc + nc
        counted = cov >= min_cov
        ppm = np.zeros(len(pc), np.int64)
        ppm[counted] = (2000000 * pc[counted] + cov[counted]) // (2 * cov[counted])
        self.base, self.n = base, len(pc)
        self.run = np.zeros((3, 4, len(pc) + 1), np.int64)
        for c in range(3):
            on = counted & (ctx == c)
            for q, v in enumerate((np.ones(len(pc), np.int64), pc, nc, ppm)):
                self.run[c, q, 1:] = np.cumsum(np.where(on, v, 0))

    def sums(self, a, b, lo=None, hi=None):
        """the [3, 4] sums over the global [a, b), clamped to the global [lo, hi) (default: all the planes)"""
        lo = self.base if lo is None else lo
        hi = self.base + self.n if hi is None else hi
        a, b = (min(max(x, lo), hi) - self.base for x in (a, b))
        return self.run[:, :, b] - self.run[:, :, a] if b > a else np.zeros((3, 4), np.int64)


def region_sums(running, start, end, lo=None, hi=None):
    """-> int64 [n, 3, 4]: interval, context, (n_loci, pcov, ncov, ppm)"""
    return np.array([running.sums(int(a), int(b), lo, hi) for a, b in zip(start, end)], np.int64).reshape(len(start), 3, 4)


def meta_edges(s, e, S0, S1, bins, flank, flank_bins):
    """the n_bins + 1 edges of an interval in reference direction, clamped to its sequence"""
    w = flank // flank_bins if flank_bins else 0
    edges = [s - flank + j * w for j in range(flank_bins)] + [s + (j * (e - s)) // bins for j in range(bins + 1)] \
        + [e + j * w for j in range(1, flank_bins + 1)]
    return [min(max(x, S0), S1) for x in edges]


def metaplot(running, start, end, seq_start, seq_end, strand, bins, flank=0, flank_bins=0, lo=None, hi=None):
    """-> (table int64 [3, n_bins, 5]: n_regions, n_loci, pcov, ncov, ppm; n_used)"""
    nb = bins + 2 * flank_bins
    tab = np.zeros((3, nb, 5), np.int64)
    used = 0
    for s, e, S0, S1, st in zip(start, end, seq_start, seq_end, strand):
        s, e, S0, S1 = int(s), int(e), int(S0), int(S1)
        if e - s < bins:
            continue
        used += 1
        x = meta_edges(s, e, S0, S1, bins, flank, flank_bins)
        for g in range(nb):
            b = nb - 1 - g if st in ("-", ord("-")) else g
            if x[g + 1] > x[g]:
                tab[:, b, 0] += 1
            tab[:, b, 1:] += running.sums(x[g], x[g + 1], lo, hi)
    return tab, used


def stats(n_loci, pcov, ncov, ppm):
    """(weighted, mean) percent; nan without a counted locus"""
    if not n_loci:
        return float("nan"), float("nan")
    return 100.0 * pcov / (pcov + ncov), ppm / n_loci / 1e4


def _columns(v):
    return "%d\t%d\t%d\t%.6g\t%.6g\n" % (v[0], v[1], v[2], *stats(*(int(x) for x in v)))


def regions_text(rows, sums):
    """rows = [(chrom, start, end, name, strand)], sums [n, 3, 4] -> {context: text of <prefix>.regions.<ctx>.tsv}"""
    head = "#chrom\tstart\tend\tname\tstrand\tn_loci\tpcov\tncov\tweighted\tmean\n"
    return {CTX[c]: head + "".join("%s\t%d\t%d\t%s\t%s\t" % tuple(r) + _columns(sums[i, c]) for i, r in enumerate(rows)) for c in range(3)}


def metaplot_text(tab, n_used, n_skipped, bins, flank_bins):
    """-> {context: text of <prefix>.metaplot.<ctx>.tsv}"""
    head = "#regions\t%d\t%d\n#bin\tpart\tn_regions\tn_loci\tpcov\tncov\tweighted\tmean\n" % (n_used, n_skipped)
    part = lambda b: "up" if b < flank_bins else "body" if b < flank_bins + bins else "down"  # noqa: E731
    return {CTX[c]: head + "".join("%d\t%s\t%d\t" % (b, part(b), tab[c, b, 0]) + _columns(tab[c, b, 1:]) for b in range(tab.shape[1]))
            for c in range(3)}
