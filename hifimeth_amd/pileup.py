"""Host-side mirror of `hifimeth pileup` (reference src/app/hifimeth/pileup.cpp:461-606) over the hm_pileup_* C ABI.

    pu = MethylationPileup(genome)            # [(name, SEQUENCE)]   <- HbnDatabase
    for rec in aligned_reads: pu.add(rec)     # one iteration of s_genomic_methy_freq_thread
    pu.flush()
    bins = pu.histograms()                    # 3 x 256
    thr = pu.resolve_thresholds(bins)         # s_resolve_scaled_prob_threshold
    pu.count(thr)
    loci = pu.loci()                          # rows of the three BED files
    text = pu.bed(loci)

Haplotype-resolved (`partitions=True`): records whose `hp` is 1 or 2 (the BAM's HP tag) are also counted into that
partition's planes with the same thresholds; `pu.loci(partition=1)` / `pu.loci(partition=2)` are the rows of
<prefix>.hap1.* / <prefix>.hap2.*, each locus in the context of the combined output.

Allele-specific methylation (`pileup -H -A`): `pu.asm(min_cov=5)` are the loci where each haplotype has at least `min_cov`
counted calls, with the difference of the two methylation percentages and the two-sided Fisher exact p-value of
[[pcov1, ncov1], [pcov2, ncov2]], both computed on the device; `pu.asm_bed(rows)` is the text of <prefix>.asm.<ctx>.bed.

With q-values (`pileup -H -A -Q`): `pu.asm_histogram()` counts the tested loci per (context, pcov1, ncov1, pcov2, ncov2) -- a fixed
table of 3 x 2080 x 2080 bins for haplotype totals below 64, the few loci beyond it listed --, `pu.asm_bin_pvalues(bins)` gives every
tuple that occurs the p the device computes for it, `asm_qvalues(tab, big)` -- host only, the C library's -- solves the
Benjamini-Hochberg q-values per context, and `pu.asm(table=...)` are the rows with a `qvalue` field, the tenth column of `asm_bed`.

Allele-specific regions (`pileup -H -A -G`): `pu.asm_regions(ctx)` chains the context's tested rows on the device -- consecutive
rows with pvalue <= max_p and a difference of the same sign, at most max_gap apart, broken by any tested row that is none -- into
rows with the pooled counts (ASM_REGION_DTYPE); `pu.asm_regions_bed(rows)` is the text of <prefix>.asm.regions.<ctx>.bed, and
`stitch_asm_regions(parts, ...)` -- host only -- joins the chains of adjacent ranges into what one fetch over their union returns.

Two samples instead of two haplotypes (`hifimeth-hip diff`): on an engine made with partitions=True that never saw a read,
`pu.load_loci(1, *read_cov_bed(path1, names, offsets))` and the same for part 2 put two samples' <prefix>.<ctx>.cov.bed rows into
the partition planes; the three paragraphs above then hold for sample 1 against sample 2, unchanged.

Replicates (`hifimeth-hip groupdiff`): on an engine made with partitions=True, groups=True, `pu.begin_sample(part)` opens the next
sample of group 1 or 2 and `pu.load_sample_loci(*read_cov_bed(...))` adds its rows; `pu.group_tests(min_reps=2)` returns the loci
with enough replicates on both sides (GROUP_DTYPE: pooled counts, diff, likelihood ratio D, dispersion phi, pvalue of the F test on
D / phi), `group_qvalues(rows)` their BH q per context, `pu.groups_bed(rows, q)` and `groups_summary_tsv(rows, q, m)` the text of
<prefix>.groups.<ctx>.bed and <prefix>.groups.summary.tsv.  include/hifimeth_hip.h has the definition of the statistic.
Regions between the groups (`hifimeth-hip groupdmr`): `pu.group_regions(ctx, lo, hi, min_reps, max_p, min_diff, max_gap, min_loci,
keep_edges)` chains those loci on the device as asm_regions chains the haplotypes' (GROUP_REGION_DTYPE) and returns (rows,
n_ctx_rows, n_hits); `group_p_cutoff(rows, q, max_q)` turns a q threshold into the max_p of each context, `stitch_group_regions`
joins adjacent ranges, `pu.group_regions_bed(rows)` and `groupdmr_summary_tsv` are the text of <prefix>.groupdmr.*.

N samples (`hifimeth-hip samplecorr`): on an engine made with samples=N, `pu.open_sample()` opens the next sample and
`pu.load_sample(*read_cov_bed(...))` writes its rows into its uint16 level plane; `pu.sample_sums(lo, hi, complete=False)` returns
the integer sums of every pair i <= j per context (SAMPLE_PAIR_DTYPE), `sample_corr(entries)` Pearson's r of the quantised levels
and the two mean levels, `samplecorr_tsv`, `samplecorr_matrix_tsv` and `samplecorr_samples_tsv` the text of
<prefix>.samplecorr.<ctx>.tsv, <prefix>.samplecorr.<ctx>.matrix.tsv and <prefix>.samplecorr.samples.tsv.

Two groups of samples over given intervals (`hifimeth-hip regiondiff`): on the same planes, `pu.sample_intervals(start, end, ctx)`
returns per interval and sample the counting loci and the sum of their levels, `sample_interval_test(sums, group)` Welch's t-test of
the two groups on the samples' interval levels (SAMPLE_TEST_DTYPE), `sample_qvalues(p)` the BH q-values among the tested intervals,
`regiondiff_tsv` and `regiondiff_summary_tsv` the text of <prefix>.regiondiff.<ctx>.tsv and <prefix>.regiondiff.summary.tsv.

Binomial test per locus (`pileup -B control` / `-e r,r,r`): is a locus methylated at all, against the caller's false-positive
rate?  `pu.control_sums(lo, hi)` over an unmethylated control sequence gives the rates (`rates_from_sums`), `pu.site_histogram()`
counts the loci per (motif, pcov, pcov + ncov), `sites_table(rates, bins, big)` -- host only, the C library's -- solves p-values
and Benjamini-Hochberg q-values for every triple, `pu.sites(table)` are the rows and `pu.sites_bed(rows)` the text of
<prefix>.sites.<ctx>.bed; `sites_rates_tsv` is <prefix>.sites.rates.tsv.

Methylation domains (`pileup -D`): `pu.domains(ctx, A=..., B=..., S=...)` segments the context's covered loci into low and high
stretches on the device -- the one optimal path of a two-state model whose weights are integers (`domain_scores(lo, hi, penalty)`,
host only, the C library's) -- one row per segment with the pooled counts (DOMAIN_DTYPE); `pu.domains_bed(rows)` is the text of
<prefix>.domains.<ctx>.bed.

The same segments from pieces (`pileup_dist -D`): `pu.domains_part(ctx, lo, hi, pass_, carry)` is one stateless pass over a piece
(summary, codes, segments), `chain_domain_parts(pieces, A, B, S, max_gap)` chains the passes of consecutive pieces through O(1) carries
(`domain_forward_carries`, `domain_backward_carries`: host only, Python ints) and `stitch_domains(parts, A, B)` joins the segments
that cross a cut -- byte for byte what one `pu.domains` over the whole gives.

The two levels fitted from the data (`pileup -D -Y n`): `pu.domain_sums(ctx, lo, hi, A, B, S)` are pcov, ncov and the number of
loci summed per state on the device, without a segment being built; `domain_refit(sums, penalty)` -- host only, the C library's --
turns them into the next levels; `DomainFit` is the stop rule of the iteration (hard EM), `pu.fit_domain_levels(ctx, lo, hi, ...)`
runs it over the sequences of the reference and `domains_fit_tsv` is the text of <prefix>.domains.fit.tsv.  All of it is integer
sums and one rounded division per level: the fit is the same however the planes are cut into pieces or over ranks.

Read-level CpG patterns (`pileup -E k`, `patterns=k`): every reference CpG heads a window of k adjacent reference CpGs at most
`pattern_span` bases apart; a read that carries a call at all k of them adds one to the window's count of its pattern (bit i = the
i-th call is methylated) -- the one output that keeps the calls of a molecule together.  `pu.patterns(lo, hi, min_reads)` are the
windows with at least min_reads such reads (PATTERN_DTYPE), `pattern_stats(row)` -- host only, the C library's -- their methylation
entropy, epipolymorphism, proportion of discordant reads and level, `pu.patterns_bed(rows)` the text of <prefix>.patterns.CpG.bed.

bedMethyl rows (`pileup -M`, `bedmethyl=True`): per reference CpG how many reads that pass -q / -f gave a methylated or an
unmethylated call (n_mod, n_canon), covered the intact CG without a call (n_nocall), showed another base at the C or the G or
broke off between them (n_diff), or have the C inside a deletion (n_delete) -- what tells "10 of 10 reads methylated" from "10 of
the 40 reads there could be called at all".  `pu.bedmethyl(lo, hi, min_valid, partition)` are the CpGs some read was classed at
with n_mod + n_canon >= min_valid (BEDMETHYL_DTYPE), `pu.bedmethyl_bed(rows)` the text of <prefix>.bedmethyl.CpG.bed in modkit's
18 columns.

Co-methylation by distance (`pileup -L bp`, `linkage=bp`): every two CpG calls of one alignment record that lie d <= bp reference
bases apart count once under their exact distance d as UU, UM, MU or MM (the first letter for the lower coordinate) -- the decay
curve of the coupling along single molecules.  The engine counts the pairs threshold-free as they pass (three 256-bin histograms
per distance) and classes them by the CpG threshold of the last count().  `pu.linkage(min_pairs)` are the distances with at least
min_pairs pairs (LINKAGE_DTYPE), `linkage_stats(row)` -- host only, the C library's -- their concordance and phi coefficient,
`pu.linkage_tsv(rows)` the text of <prefix>.linkage.CpG.tsv.

Methylation by position in the read (`pileup -P bp`, `profile=bp`) and end trimming (`pileup -I n5:n3`, `trim=(n5, n3)`): every
call the CNN makes within 200 bases of a read end saw a zero-padded kinetics window.  With profile=D every counted call also counts
by its offset p in the read as sequenced (L bases): in row (5', p) or (3', L - 1 - p) when the nearer end is fewer than D bases
away (ties to 5'), else in the row `interior` -- threshold-free histograms of the ML byte on the device, classed by the thresholds
of the last count().  `pu.readpos(min_calls)` are the rows with at least min_calls calls (READPOS_DTYPE), `readpos_stats(row)` --
host only, the C library's -- percent methylated and mean ML byte, `readpos_tsv(rows)` the text of <prefix>.readpos.tsv.  With
trim=(n5, n3) the engine drops the entries in the first n5 and the last n3 bases of every read before anything sees them.

Intervals and metaplots (`pileup -R bed [-C min-cov] [-J bins[:flank:flank_bins]]`): `parse_regions_bed(path, names, lengths)`
reads the intervals (`Regions`), `pu.regions(start, end, min_cov)` sums the planes over each of them per context -- n_loci, pcov,
ncov and ppm, the sum of the loci's own fractions in parts per million, exact integers (REGION_SUM_DTYPE, [n, 3]) -- from a
two-level prefix index the call builds on the device, so that an interval costs the same whatever its length.
`pu.metaplot(**regions.coords(pu.offsets), bins=..)` cuts every interval and its flanks into bins and sums the bins over the
intervals (METABIN_DTYPE).  `region_stats(row)` -- host only, the C library's -- are the weighted and the mean percentage,
`regions_tsv` / `metaplot_tsv` the text of <prefix>.regions.<ctx>.tsv / <prefix>.metaplot.<ctx>.tsv.

By sequence context (`pileup -S flank [-O min-cov]`): `pu.context(flank, min_cov)` sums the loci per context and per k-mer around the
called cytosine, k = 3 + 2 flank, read on the cytosine's strand -- int64 [3, 4^k + 1, 4] of (n_loci, pcov, ncov, ppm), the last row
`other` (no C / G at the locus, a window that leaves its sequence, a base outside ACGT).  `context_kmer(code, k)` /
`context_code(kmer)` name the rows, `context_tsv(table, flank)` is the text of <prefix>.context.<ctx>.tsv, with the percentages
of `region_stats`.

Fused with the caller (`pileup -K`): `pu.add_called(read, calls)` takes the records `MethylationCaller` returned for an aligned read
instead of parsed MM / ML -- the same effect as add() of that read carrying the calls as tags, without the tag text.

Multi-GPU (one process per GPU, records dealt to ranks in slabs): `reduce_over_ranks` sums the histograms with an
all-reduce before the thresholds are resolved, and after counting reduce-scatters the per-locus planes (sum for
pcov / ncov, max for the motif key) so that every rank ends up owning one contiguous range of loci.
There is no CPU fallback: construction fails without the HIP library and a gfx950 device.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from ._lib import lib
from .caller import HifimethError

MOD_DTYPE = np.dtype([("qoff", "<i4"), ("strand", "u1"), ("unmod_base", "S1"), ("code", "S1"), ("prob", "u1")])
LOCUS_DTYPE = np.dtype([("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("motif", "<u4"), ("reserved", "<u4")])
ASM_DTYPE = np.dtype([("gpos", "<i8"), ("pcov1", "<i4"), ("ncov1", "<i4"), ("pcov2", "<i4"), ("ncov2", "<i4"), ("motif", "<u4"),
                      ("reserved", "<u4"), ("diff", "<f8"), ("pvalue", "<f8")])     # hm_asm_t, 48 bytes
ASMQ_DTYPE = np.dtype(ASM_DTYPE.descr + [("qvalue", "<f8")])                          # hm_asmq_t, 56 bytes
GROUP_DTYPE = np.dtype([("gpos", "<i8"), ("pcov1", "<i4"), ("ncov1", "<i4"), ("pcov2", "<i4"), ("ncov2", "<i4"), ("motif", "<u4"),
                        ("m1", "<u2"), ("m2", "<u2"), ("diff", "<f8"), ("D", "<f8"), ("phi", "<f8"), ("pvalue", "<f8")])  # hm_group_t, 64 bytes
SAMPLE_PAIR_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("ctx", "<u4"), ("reserved", "<u4"), ("n", "<u8"), ("si", "<u8"), ("sj", "<u8"),
                              ("sii", "<u8"), ("sjj", "<u8"), ("sij", "<u8")])  # hm_sample_pair_t, 64 bytes
SAMPLE_MAX = 64  # HM_SAMPLE_MAX
SAMPLE_TEST_DTYPE = np.dtype([("m1", "<i4"), ("m2", "<i4"), ("n1", "<u8"), ("n2", "<u8"), ("mean1", "<f8"), ("mean2", "<f8"), ("t", "<f8"),
                              ("df", "<f8"), ("pvalue", "<f8")])  # hm_sample_test_t, 64 bytes
ASM_BIN_DTYPE = np.dtype([("bin", "<u4"), ("reserved", "<u4"), ("count", "<u8"), ("pvalue", "<f8"), ("qvalue", "<f8")])  # hm_asm_bin_t, 32 bytes
ASM_REGION_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("pcov1", "<i8"), ("ncov1", "<i8"), ("pcov2", "<i8"), ("ncov2", "<i8"),
                             ("n_loci", "<i4"), ("sign", "<i4"), ("motif", "<u4"), ("flags", "<u4"), ("diff", "<f8"),
                             ("pmin", "<f8")])                                      # hm_asm_region_t, 80 bytes
GROUP_REGION_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("pcov1", "<i8"), ("ncov1", "<i8"), ("pcov2", "<i8"), ("ncov2", "<i8"),
                               ("n_loci", "<i4"), ("sign", "<i4"), ("motif", "<u4"), ("flags", "<u4"), ("m1_min", "<u2"), ("m2_min", "<u2"),
                               ("reserved", "<u4"), ("diff", "<f8"), ("pmin", "<f8"), ("phi_max", "<f8")])  # hm_group_region_t, 96 bytes
REGION_FIRST, REGION_LAST = 1, 2                                                    # HM_REGION_FIRST, HM_REGION_LAST
ASM_T, ASM_PAIRS = 64, 2080                                                           # HM_ASM_T, HM_ASM_PAIRS
ASM_BINS = 3 * ASM_PAIRS * ASM_PAIRS                                                  # HM_ASM_BINS
SITE_DTYPE = np.dtype([("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("motif", "<u4"), ("reserved", "<u4"), ("pvalue", "<f8"),
                       ("qvalue", "<f8")])                                            # hm_site_t, 40 bytes
SITE_BINS = 3 * 256 * 256                                                             # HM_SITE_BINS
DOMAIN_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("pcov", "<i8"), ("ncov", "<i8"), ("n_loci", "<i4"), ("state", "<u4"),
                         ("motif", "<u4"), ("flags", "<u4"), ("level", "<f8"), ("score", "<f8")])  # hm_domain_t, 64 bytes
PATTERN_DTYPE = np.dtype([("start", "<i8"), ("end", "<i8"), ("counts", "<u4", (16,)), ("n", "<u4"), ("k", "<u4")])  # hm_pattern_t, 88 bytes
BEDMETHYL_DTYPE = np.dtype([("gpos", "<i8"), ("n_mod", "<u4"), ("n_canon", "<u4"), ("n_nocall", "<u4"), ("n_diff", "<u4"),
                            ("n_delete", "<u4"), ("reserved", "<u4")])                # hm_bedmethyl_t, 32 bytes
LINKAGE_DTYPE = np.dtype([("dist", "<u4"), ("reserved", "<u4"), ("n_uu", "<u8"), ("n_um", "<u8"), ("n_mu", "<u8"),
                          ("n_mm", "<u8")])                                          # hm_linkage_t, 40 bytes
LINKAGE_MAX_DIST = 16384                                 # the largest `pileup -L`
READPOS_DTYPE = np.dtype([("motif", "<u4"), ("end", "<u4"), ("dist", "<u4"), ("reserved", "<u4"), ("n_m", "<u8"), ("n_u", "<u8"),
                          ("sum_ml", "<u8")])                                        # hm_readpos_t, 40 bytes
READPOS_MAX = 2048                                       # the largest `pileup -P`
REGION_SUM_DTYPE = np.dtype([("n_loci", "<i8"), ("pcov", "<i8"), ("ncov", "<i8"), ("ppm", "<i8")])                       # hm_region_sum_t, 32 bytes
METABIN_DTYPE = np.dtype([("motif", "<i4"), ("bin", "<i4"), ("n_regions", "<i8")] + REGION_SUM_DTYPE.descr)           # hm_metabin_t, 48 bytes
SMOOTH_DTYPE = np.dtype([("gpos", "<i8"), ("pcov", "<i4"), ("ncov", "<i4"), ("loci", "<i8"), ("wp", "<i8"), ("wn", "<i8")])  # hm_smooth_t, 40 bytes
METAPLOT_MAX_BINS = 1000                                 # the largest `pileup -J` bins (and flank_bins)
CONTEXT_MAX_FLANK = 3                                    # the largest `pileup -S`: k = 9
CONTEXT_PATH_AUTO, CONTEXT_PATH_LDS, CONTEXT_PATH_GLOBAL = -1, 0, 1                   # HM_CONTEXT_PATH_*
READPOS_ENDS = ("5p", "3p", "interior")                  # hm_readpos_t.end 0, 1, 2 as <prefix>.readpos.tsv names them
PATTERN_SPAN, PATTERN_MIN_READS = 150, 10                # `pileup -E`'s default -w and -o
DOMAIN_AFTER_BREAK, DOMAIN_BEFORE_BREAK = 1, 2                                        # HM_DOMAIN_AFTER_BREAK, HM_DOMAIN_BEFORE_BREAK
DOMAIN_PASS_SUMMARY, DOMAIN_PASS_CODES, DOMAIN_PASS_SEGMENTS, DOMAIN_KEEP = 0, 1, 2, 2   # HM_DOMAIN_PASS_*, HM_DOMAIN_KEEP
DOMAIN_LEVELS = ((0.1, 0.8), (0.05, 0.5), (0.02, 0.2))  # `pileup -D`'s default low : high level per context: conventions, not tuned on data
DOMAIN_PENALTY, DOMAIN_MAX_GAP = 8.0, 1000               # ... its default switch penalty (nats) and largest linking distance
CTX_NAMES = ("CpG", "CHG", "CHH")
_CHEBI = {27551: "m", 76792: "h", 76794: "f", 76793: "c", 16964: "g", 80961: "e", 17477: "b", 28871: "a",
          44605: "o", 18107: "n"}
_RC = bytes.maketrans(b"ACGTN", b"TGCAN")


def parse_mods(stored_seq: str, flag: int, mm: Optional[str], ml) -> np.ndarray:
    """extract_bam_base_mods (src/corelib/bam_mod_parser.cpp:231-286), vectorised: the k-th entry of an edit
    series sits on the (sum of (delta+1))-th occurrence of the unmodified base in the forward-strand sequence."""
    if mm is None or ml is None or len(ml) == 0:
        return np.zeros(0, MOD_DTYPE)
    if not mm.endswith(";"):
        raise HifimethError("The MM aux tag must end with ';'")
    s = stored_seq.encode()
    fwd = np.frombuffer(s.translate(_RC)[::-1] if flag & 16 else s, np.uint8)
    ml = np.asarray(ml, np.uint8)
    out, pi = [], 0
    for series in mm[:-1].split(";"):
        if len(series) < 3 or series[0] not in "CGTAUN" or series[1] not in "+-":
            raise HifimethError(f"Corrupted edit series {series};")
        head, _, rest = series.partition(",")
        codes = head[2:]
        codes = _CHEBI[int(codes)] if codes[:1].isdigit() else codes.replace(".", "").replace("?", "")
        deltas = np.array([int(x) for x in rest.split(",")] if rest else [], np.int64)
        where = np.nonzero(fwd == ord(series[0]))[0]
        nth = np.cumsum(deltas + 1) - 1
        if len(nth) and nth[-1] >= len(where):
            raise HifimethError(f"edit series runs past the read end: {series};")
        q = where[nth]
        n = len(q) * len(codes)
        if pi + n > len(ml):
            raise HifimethError("ML is shorter than the MM edit lists")
        m = np.zeros(n, MOD_DTYPE)
        m["qoff"] = np.repeat(q, len(codes))
        m["strand"] = 0 if series[1] == "+" else 1
        m["unmod_base"] = series[0].encode()
        m["code"] = np.tile(np.frombuffer(codes.encode(), "S1"), len(q))
        m["prob"] = ml[pi:pi + n]
        pi += n
        out.append(m)
    return np.concatenate(out) if out else np.zeros(0, MOD_DTYPE)


def resolve_threshold(bins) -> Tuple[int, int]:
    """s_resolve_scaled_prob_threshold for one context (pileup.cpp:355-436) -> (threshold, samples in window)"""
    a = np.asarray(bins, np.uint64)
    st, en = 20, 236
    while st < 256 and a[st] < 10:
        st += 1
    while en and a[en - 1] < 10:
        en -= 1
    if en - st < 50:
        return 128, 0
    w = a[st:en]
    total = int(w.sum())
    return (128 if total < 10000 else st + int(np.argmin(w))), total


def parse_rates(text: str) -> List[float]:
    """the argument of -e: three decimals in [0, 1] or `nan` (context not tested), comma-separated; ValueError otherwise"""
    import re
    parts = text.split(",")
    if len(parts) != 3:
        raise ValueError("three comma-separated rates expected (CpG,CHG,CHH)")
    out = []
    for t in parts:
        if t == "nan":
            out.append(float("nan"))
        elif re.fullmatch(r"(\d+\.?\d*|\.\d+)([eE][+-]?\d+)?", t) and 0.0 <= float(t) <= 1.0:
            out.append(float(t))
        else:
            raise ValueError(f"rate {t!r} is neither a decimal in [0, 1] nor nan")
    return out


def rates_from_sums(sums) -> List[float]:
    """sums = (P_cpg, P_chg, P_chh, N_cpg, N_chg, N_chh) of the control sequence -> e_c = P_c / (P_c + N_c), NaN without calls"""
    s = [int(x) for x in sums]
    return [float(s[c]) / float(s[c] + s[3 + c]) if s[c] + s[3 + c] else float("nan") for c in range(3)]


class SitesTable:
    """what hm_sites_table returns: ptab / qtab [3, 256, 256] indexed [motif, n, k], the big loci (n >= 256) with big_p / big_q,
    m[3] = loci per context, and the rates it was solved for"""
    def __init__(self, rates, ptab, qtab, big, big_p, big_q, m):
        self.rates, self.ptab, self.qtab, self.big, self.big_p, self.big_q, self.m = rates, ptab, qtab, big, big_p, big_q, m

    @property
    def ctx_mask(self) -> int:
        return sum(1 << c for c in range(3) if not np.isnan(self.rates[c]))


def sites_table(rates, bins: np.ndarray, big: Optional[np.ndarray] = None) -> SitesTable:
    """p-values and BH q-values of every (motif, pcov, pcov + ncov), by the C library (host only: no GPU is needed).
    bins: uint64 [3, 256, 256] (or flat) from site_histogram, summed over the job; big: its LOCUS_DTYPE list, ascending."""
    L = lib()
    r = np.ascontiguousarray(rates, np.float64)
    b = np.ascontiguousarray(bins, np.uint64).reshape(-1)
    big = np.zeros(0, LOCUS_DTYPE) if big is None else np.ascontiguousarray(big, LOCUS_DTYPE)
    if r.shape != (3,) or b.size != SITE_BINS:
        raise HifimethError("sites_table: three rates and 3 x 256 x 256 bins expected")
    ptab, qtab = np.empty(SITE_BINS, np.float64), np.empty(SITE_BINS, np.float64)
    big_p, big_q = np.empty(len(big), np.float64), np.empty(len(big), np.float64)
    m = np.zeros(3, np.uint64)
    if L.hm_sites_table(*(x.ctypes.data_as(C.c_void_p) for x in (r, b, big)), len(big),
                        *(x.ctypes.data_as(C.c_void_p) for x in (ptab, qtab, big_p, big_q, m))) != 0:
        raise HifimethError("hm_sites_table: a rate outside [0, 1], or bins / big loci that are no counts")
    return SitesTable(r, ptab.reshape(3, 256, 256), qtab.reshape(3, 256, 256), big, big_p, big_q, m)


class AsmTable:
    """what asm_qvalues returns: tab (ASM_BIN_DTYPE: the tuples that occur, ascending in bin, with count, pvalue, qvalue), the big loci
    (ASM_DTYPE, a haplotype total >= 64) with big_q, and m[3] = tested loci per context"""
    def __init__(self, tab, big, big_q, m):
        self.tab, self.big, self.big_q, self.m = tab, big, big_q, m


def asm_qvalues(tab: np.ndarray, big: Optional[np.ndarray] = None) -> AsmTable:
    """Benjamini-Hochberg q-values per context of the haplotype test, by the C library (host only: no GPU is needed).
    tab: what asm_bin_pvalues gave for the job-wide bins; big: the job's big loci (asm_histogram), ascending in gpos."""
    tab = np.array(tab, ASM_BIN_DTYPE)                      # a copy: the q-values are written into it
    big = np.zeros(0, ASM_DTYPE) if big is None else np.ascontiguousarray(big, ASM_DTYPE)
    big_q = np.full(len(big), np.nan)
    m = np.zeros(3, np.uint64)
    if lib().hm_asm_qvalues(tab.ctypes.data_as(C.c_void_p), len(tab), big.ctypes.data_as(C.c_void_p), len(big),
                            big_q.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_asm_qvalues: bins that are not ascending or empty, a p outside [DBL_MIN, 1], or big loci that are none")
    return AsmTable(tab, big, big_q, m)


def asm_summary_tsv(table: AsmTable) -> str:
    """the text of <prefix>.asm.summary.tsv: ctx, tested loci, loci with q <= 0.05, loci with q <= 0.01 -- from the table's weights"""
    ctx = np.concatenate([table.tab["bin"] // (ASM_PAIRS * ASM_PAIRS), np.minimum(table.big["motif"], 2)]).astype(np.int64)
    w = np.concatenate([table.tab["count"], np.ones(len(table.big), np.uint64)])
    q = np.concatenate([table.tab["qvalue"], table.big_q])
    return "".join("%s\t%d\t%d\t%d\n" % (CTX_NAMES[c], int(table.m[c]), int(w[(ctx == c) & (q <= 0.05)].sum()),
                                          int(w[(ctx == c) & (q <= 0.01)].sum())) for c in range(3))


def group_qvalues(rows: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """`groupdiff` (hm_group_qvalues, host only): -> (q, m): q[i] = the Benjamini-Hochberg value of rows[i]["pvalue"] among the rows
    of its context (equal p gives equal q), m[ctx] = tested loci per context.  rows: what group_tests returned for the whole job."""
    rows = np.ascontiguousarray(rows, GROUP_DTYPE)
    q = np.full(len(rows), np.nan)
    m = np.zeros(3, np.uint64)
    if lib().hm_group_qvalues(rows.ctypes.data_as(C.c_void_p), len(rows), q.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_group_qvalues: a motif above 3 or a p outside [DBL_MIN, 1]")
    return q, m


def groups_summary_tsv(rows: np.ndarray, q: np.ndarray, m) -> str:
    """the text of <prefix>.groups.summary.tsv: ctx, tested loci, loci with q <= 0.05, loci with q <= 0.01, loci with phi > 1"""
    ctx = np.minimum(rows["motif"], 2)
    return "".join("%s\t%d\t%d\t%d\t%d\n" % (CTX_NAMES[c], int(m[c]), int(((ctx == c) & (q <= 0.05)).sum()), int(((ctx == c) & (q <= 0.01)).sum()),
                                              int(((ctx == c) & (rows["phi"] > 1.0)).sum())) for c in range(3))


def group_p_cutoff(rows: np.ndarray, q: np.ndarray, max_q: float) -> np.ndarray:
    """`groupdmr -F` (hm_dmr_p_cutoff, host only): -> cutoff[3]: per context the largest pvalue among the rows with q <= max_q, 0
    where there is none.  q is monotone in p, so the rows with q <= max_q are those with pvalue <= cutoff: group_regions with
    max_p = cutoff[ctx] chains them; a context whose cutoff is 0 has no regions.  rows, q: group_tests' and group_qvalues' of the job."""
    rows = np.ascontiguousarray(rows, GROUP_DTYPE)
    q = np.ascontiguousarray(q, np.float64)
    assert q.shape == (len(rows),)
    cutoff = np.zeros(3, np.float64)
    if lib().hm_dmr_p_cutoff(rows.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), len(rows), float(max_q),
                               cutoff.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_dmr_p_cutoff: max_q outside (0, 1], a motif above 3 or a p outside [DBL_MIN, 1]")
    return cutoff


def groupdmr_summary_tsv(tested, hits, cutoff, regions) -> str:
    """the text of <prefix>.groupdmr.summary.tsv: per context ctx, tested loci, hits, the p cutoff used (nan: none), regions, loci
    in regions, regions +, regions -.  tested[c], hits[c]: summed over the fetches of context c; regions[c]: all its rows"""
    return "".join("%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d\n" % (
        CTX_NAMES[c], tested[c], hits[c], _g6(float(cutoff[c])), len(regions[c]), int(regions[c]["n_loci"].sum()),
        int((regions[c]["sign"] > 0).sum()), int((regions[c]["sign"] < 0).sum())) for c in range(3))


def sample_geometry() -> Tuple[int, int]:
    """-> (HM_SAMPLE_TILE, HM_SAMPLE_MAX) of the library: the positions a workgroup of sample_sums takes at a time, the most samples"""
    out = np.zeros(2, np.int64)
    lib().hm_sample_geometry(out.ctypes.data_as(C.c_void_p))
    return int(out[0]), int(out[1])


def sample_corr(entries: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """`samplecorr` (hm_sample_corr, host only): -> (r, mean_i, mean_j) per entry of sample_sums: Pearson's r of the quantised
    levels from the exact 128-bit num, va, vb (NaN when n < 2 or a variance is 0) and the mean levels in percent (NaN when n = 0)"""
    entries = np.ascontiguousarray(entries, SAMPLE_PAIR_DTYPE)
    r, mi, mj = (np.full(len(entries), np.nan) for _ in range(3))
    if lib().hm_sample_corr(entries.ctypes.data_as(C.c_void_p), len(entries), *(a.ctypes.data_as(C.c_void_p) for a in (r, mi, mj))) != 0:
        raise HifimethError("hm_sample_corr: bad argument")
    return r, mi, mj


def _sample_pairs(entries: np.ndarray, ctx: int):
    """the entries of context `ctx` with their r and means -> {(i, j): (entry, r, mean_i, mean_j)}"""
    e = np.ascontiguousarray(entries, SAMPLE_PAIR_DTYPE)
    e = e[e["ctx"] == ctx]
    return {(int(x["i"]), int(x["j"])): (x, *v) for x, *v in zip(e, *sample_corr(e))}


def samplecorr_tsv(names: Sequence[str], entries: np.ndarray, ctx: int) -> str:
    """the text of <prefix>.samplecorr.<ctx>.tsv: a header, then per pair i < j in index order sample_i, sample_j, n, mean_i,
    mean_j, r.  entries: what sample_sums returned for the whole reference; names: the samples' in index order."""
    pairs = _sample_pairs(entries, ctx)
    return "sample_i\tsample_j\tn\tmean_i\tmean_j\tr\n" + "".join(
        "%s\t%s\t%d\t%.6g\t%.6g\t%.6g\n" % (names[i], names[j], int(x["n"]), mi, mj, r) for (i, j), (x, r, mi, mj) in sorted(pairs.items()) if i < j)


def samplecorr_matrix_tsv(names: Sequence[str], entries: np.ndarray, ctx: int) -> str:
    """the text of <prefix>.samplecorr.<ctx>.matrix.tsv: `sample` and the N names, then per sample its name and N values of r; the
    diagonal is the r of the diagonal entry, 1 when the sample has variance and nan otherwise"""
    pairs = _sample_pairs(entries, ctx)
    n = len(names)
    return "sample\t" + "\t".join(names) + "\n" + "".join(
        names[i] + "".join("\t%.6g" % pairs[(min(i, j), max(i, j))][1] for j in range(n)) + "\n" for i in range(n))


def samplecorr_samples_tsv(names: Sequence[str], entries: np.ndarray, contexts: Sequence[int] = (0, 1, 2)) -> str:
    """the text of <prefix>.samplecorr.samples.tsv: a header, then per context of `contexts` and sample ctx, sample, counting loci,
    mean level in percent, from the diagonal entries of sample_sums(complete=False)"""
    text = "ctx\tsample\tn\tmean\n"
    for c in contexts:
        pairs = _sample_pairs(entries, c)
        text += "".join("%s\t%s\t%d\t%.6g\n" % (CTX_NAMES[c], names[i], int(pairs[(i, i)][0]["n"]), pairs[(i, i)][2]) for i in range(len(names)))
    return text


def sample_interval_test(sums: np.ndarray, group: Sequence[int], min_loci: int = 3, min_reps: int = 2) -> np.ndarray:
    """`regiondiff` (hm_sample_interval_test, host only): sums = what sample_intervals returned, (n_iv, M, 2) uint64; group[s] = 1
    or 2, or 0 for a sample that takes no part.  -> SAMPLE_TEST_DTYPE [n_iv]: per interval the used samples of each group (those
    with >= min_loci counting loci), their loci, the groups' mean levels in percent, and Welch's t, df and two-sided p-value; NaN
    where fewer than min_reps samples of a group are used, and p NaN where the samples of both groups do not vary at all but the
    means differ.  include/hifimeth_hip.h has the definition."""
    sums = np.ascontiguousarray(sums, np.uint64)
    assert sums.ndim == 3 and sums.shape[2] == 2
    group = np.ascontiguousarray(group, np.uint8)
    assert group.size == sums.shape[1]
    out = np.zeros(sums.shape[0], SAMPLE_TEST_DTYPE)
    if lib().hm_sample_interval_test(sums.ctypes.data_as(C.c_void_p), sums.shape[0], sums.shape[1], group.ctypes.data_as(C.c_void_p),
                                     min_loci, min_reps, out.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_sample_interval_test: bad argument")
    return out


def sample_qvalues(p: np.ndarray) -> np.ndarray:
    """`regiondiff` (hm_sample_qvalues, host only): the Benjamini-Hochberg q-values of p among its finite entries; NaN stays NaN"""
    p = np.ascontiguousarray(p, np.float64).reshape(-1)
    q = np.full(p.size, np.nan)
    if lib().hm_sample_qvalues(p.ctypes.data_as(C.c_void_p), p.size, q.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_sample_qvalues: a p-value outside [DBL_MIN, 1]")
    return q


def _g6(v: float) -> str:
    return "nan" if v != v else "%.6g" % v


def regiondiff_tsv(regions: "Regions", names: Sequence[str], tests: np.ndarray, q: np.ndarray) -> str:
    """the text of <prefix>.regiondiff.<ctx>.tsv: the header, then per interval in input order chrom, start, end, name, strand, m1,
    m2, loci1, loci2, mean1, mean2, diff, t, df, p, q (nan where not tested); tests = sample_interval_test's rows of the context,
    q = sample_qvalues(tests["pvalue"])"""
    head = "#chrom\tstart\tend\tname\tstrand\tm1\tm2\tloci1\tloci2\tmean1\tmean2\tdiff\tt\tdf\tp\tq\n"
    return head + "".join(
        "%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t" % (names[regions.sid[i]], regions.start[i], regions.end[i], regions.name[i], regions.strand[i],
                                                int(r["m1"]), int(r["m2"]), int(r["n1"]), int(r["n2"]))
        + "\t".join(_g6(float(v)) for v in (r["mean1"], r["mean2"], r["mean1"] - r["mean2"], r["t"], r["df"], r["pvalue"], q[i])) + "\n"
        for i, r in enumerate(tests))


def regiondiff_summary_tsv(tests: dict, q: dict) -> str:
    """the text of <prefix>.regiondiff.summary.tsv: the header, then per context of `tests` (keyed 0, 1, 2, in that order) ctx,
    intervals, tested intervals, those with q <= 0.05 and with q <= 0.01"""
    return "ctx\tintervals\ttested\tq<=0.05\tq<=0.01\n" + "".join(
        "%s\t%d\t%d\t%d\t%d\n" % (CTX_NAMES[c], len(tests[c]), int((~np.isnan(tests[c]["t"])).sum()), int((q[c] <= 0.05).sum()), int((q[c] <= 0.01).sum()))
        for c in sorted(tests))


def stitch_asm_regions(parts, max_gap: int, min_loci: int, keep_edges: bool = False) -> Tuple[np.ndarray, int]:
    """parts = [(rows, n_ctx_rows)]: what asm_regions(..., keep_edges=True) gave for adjacent ranges of one sequence and one
    context, in ascending order, all with the same max_p / max_gap / min_loci.  -> (rows, n_ctx_rows) equal, byte for byte, to
    one fetch over the union of the ranges with this keep_edges.  Host only.
    A part without rows of the context (n_ctx_rows == 0) neither links nor breaks.  The chain that holds a part's last row (LAST)
    and the one that holds the next non-empty part's first row (FIRST) are one chain when they have the same sign and
    right.start - (left.end - 1) <= max_gap: sums and n_loci add, pmin is the minimum, diff is recomputed from the sums; a chain
    may span many parts.  FIRST / LAST survive only on a chain that reaches the first / last row of the whole."""
    return _stitch_regions(parts, max_gap, min_loci, keep_edges, ASM_REGION_DTYPE, lambda whole, more: None)


def _merge_group_region(whole, more) -> None:
    for c in ("m1_min", "m2_min"):
        whole[c] = min(whole[c], more[c])
    whole["phi_max"] = max(whole["phi_max"], more["phi_max"])


def stitch_group_regions(parts, max_gap: int, min_loci: int, keep_edges: bool = False) -> Tuple[np.ndarray, int]:
    """stitch_asm_regions for group_regions: parts = [(rows, n_ctx_rows)] of group_regions(..., keep_edges=True) over adjacent
    ranges of one sequence and one context, ascending, all with the same max_p / min_diff / max_gap / min_loci.  -> (rows,
    n_ctx_rows) equal, byte for byte, to one fetch over the union with this keep_edges.  Where two chains are one, m1_min and
    m2_min also take the minimum and phi_max the maximum.  Host only."""
    return _stitch_regions(parts, max_gap, min_loci, keep_edges, GROUP_REGION_DTYPE, _merge_group_region)


def _stitch_regions(parts, max_gap: int, min_loci: int, keep_edges: bool, dtype, merge) -> Tuple[np.ndarray, int]:
    """the walk both stitches share; merge(whole, more) folds in what the family's chains carry beyond sums, n_loci and pmin"""
    parts = [(np.ascontiguousarray(r, dtype), int(n)) for r, n in parts if int(n)]
    out: List[np.ndarray] = []
    open_ = None                                  # the chain that holds the last row seen so far, if that row is a hit
    for k, (rows, _) in enumerate(parts):
        for g in rows:
            g = g.copy()
            f = int(g["flags"])
            g["flags"] = (f & REGION_FIRST if k == 0 else 0) | (f & REGION_LAST if k == len(parts) - 1 else 0)
            if open_ is not None and f & REGION_FIRST and g["sign"] == open_["sign"] and g["start"] - (open_["end"] - 1) <= max_gap:
                for c in ("pcov1", "ncov1", "pcov2", "ncov2", "n_loci"):
                    open_[c] += g[c]
                open_["end"] = g["end"]
                open_["pmin"] = min(open_["pmin"], g["pmin"])
                open_["flags"] |= g["flags"]
                P1, N1, P2, N2 = (np.float64(open_[c]) for c in ("pcov1", "ncov1", "pcov2", "ncov2"))
                open_["diff"] = np.float64(100.0) * P1 / (P1 + N1) - np.float64(100.0) * P2 / (P2 + N2)
                merge(open_, g)
            else:
                out.append(g)
                open_ = g
            if not f & REGION_LAST:
                open_ = None
        if not len(rows) or not int(rows[-1]["flags"]) & REGION_LAST:
            open_ = None
    keep = [g for g in out if g["n_loci"] >= min_loci or (keep_edges and g["flags"])]
    rows = np.array(keep, dtype) if keep else np.zeros(0, dtype)
    return rows, sum(n for _, n in parts)


def domain_scores(level_lo: float, level_hi: float, penalty: float = DOMAIN_PENALTY) -> Tuple[int, int, int]:
    """-> (A, B, S), the integer weights of domains() in Q16 nats for a low and a high methylation level (fractions) and a switch
    penalty in nats: A = round(65536 log(hi / lo)) per methylated read, B = round(65536 log((1 - hi) / (1 - lo))) per unmethylated
    read, S = round(65536 penalty).  By the C library (host only: no GPU is needed)."""
    A, B, S = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    if lib().hm_domain_scores(level_lo, level_hi, penalty, C.byref(A), C.byref(B), C.byref(S)) != 0:
        raise HifimethError("hm_domain_scores: 0 < level_lo < level_hi < 1 and penalty >= 0 expected, with weights of at most 2^24")
    return int(A.value), int(B.value), int(S.value)


def domain_refit(sums, penalty: float = DOMAIN_PENALTY) -> Optional[Tuple[float, float]]:
    """sums = (P0, N0, R0, P1, N1, R1), the counters and loci per state -> the next levels (P0 / (P0 + N0), P1 / (P1 + N1)), each
    clamped to [1e-6, 1 - 1e-6]; None where the fit ends here: a state without loci, or levels that are no valid pair for
    domain_scores.  By the C library (host only)."""
    lo, hi = C.c_double(0.0), C.c_double(0.0)
    rc = lib().hm_domain_refit((C.c_int64 * 6)(*(int(x) for x in sums)), penalty, C.byref(lo), C.byref(hi))
    if rc not in (0, -4):                                                             # HM_OK, HM_EDATA
        raise HifimethError("hm_domain_refit: six sums >= 0 and penalty >= 0 expected")
    return (float(lo.value), float(hi.value)) if rc == 0 else None


class DomainFit:
    """The iteration that fits the two levels of one context (include/hifimeth_hip.h has the definition).  While `status` is None,
    `rule` = (A, B, S) is what the state sums are wanted under; step(sums) takes them.  Then `status` is one of converged, cycle,
    max_iter, one_state, degenerate, (`lo`, `hi`) the result and `rule` its scores.  `history`: per iteration
    (i, lo, hi, A, B, sums)."""

    def __init__(self, level_lo: float, level_hi: float, penalty: float = DOMAIN_PENALTY, max_iter: int = 20):
        if max_iter < 1:
            raise ValueError("max_iter must be >= 1")
        self.lo, self.hi, self.penalty, self.max_iter = float(level_lo), float(level_hi), penalty, max_iter
        self.rule = domain_scores(self.lo, self.hi, penalty)
        self.status: Optional[str] = None
        self.history: List[tuple] = []

    def _end(self, status: str, lo: float, hi: float) -> None:
        self.status, self.lo, self.hi = status, lo, hi
        self.rule = domain_scores(lo, hi, self.penalty)

    def step(self, sums) -> None:
        assert self.status is None
        sums = tuple(int(x) for x in sums)
        i, (A, B, _) = len(self.history), self.rule
        self.history.append((i, self.lo, self.hi, A, B, sums))
        new = domain_refit(sums, self.penalty)
        if new is None:
            return self._end("one_state" if sums[2] == 0 or sums[5] == 0 else "degenerate", self.lo, self.hi)
        A2, B2, _ = domain_scores(*new, self.penalty)
        seen = [(h[3], h[4]) for h in self.history]
        if (A2, B2) == (A, B):
            return self._end("converged", self.lo, self.hi)
        if (A2, B2) in seen:                                  # iterations j .. i, j with the levels that closed the cycle
            j = seen.index((A2, B2))
            members = [((A2, B2), new)] + [((h[3], h[4]), (h[1], h[2])) for h in self.history[j + 1:]]
            return self._end("cycle", *min(members)[1])
        if i + 1 == self.max_iter:
            return self._end("max_iter", *new)
        self.lo, self.hi = new
        self.rule = (A2, B2, self.rule[2])


def fit_levels(sums_of, level_lo: float, level_hi: float, penalty: float = DOMAIN_PENALTY, max_iter: int = 20):
    """sums_of(A, B, S) -> the six state sums of everything that is fitted -> (lo, hi, status, history) of DomainFit"""
    fit = DomainFit(level_lo, level_hi, penalty, max_iter)
    while fit.status is None:
        fit.step(sums_of(*fit.rule))
    return fit.lo, fit.hi, fit.status, fit.history


def domains_fit_tsv(fits) -> str:
    """the text of <prefix>.domains.fit.tsv.  fits: per context None (not segmented) or (lo, hi, status, history).  One row per
    context and iteration -- ctx, iter, level_lo, level_hi, A, B, P0, N0, R0, P1, N1, R1 -- then ctx, status, level_lo, level_hi:
    the result, which -u takes back as it stands."""
    text = []
    for c, fit in enumerate(fits):
        if fit is None:
            continue
        lo, hi, status, history = fit
        for i, l, h, A, B, sums in history:
            text.append("%s\t%d\t%.17g\t%.17g\t%d\t%d\t" % (CTX_NAMES[c], i, l, h, A, B) + "\t".join("%d" % x for x in sums) + "\n")
        text.append("%s\t%s\t%.17g\t%.17g\n" % (CTX_NAMES[c], status, lo, hi))
    return "".join(text)


class _DomainPart(C.Structure):                                                       # hm_domain_part_t, 104 bytes
    _fields_ = [(n, C.c_int64) for n in ("prev_gpos", "prev_d", "next_gpos")] + \
               [(n, C.c_int32) for n in ("has_prev", "has_next", "last_state", "back")] + \
               [(n, C.c_int64) for n in ("n_rows", "first_gpos", "last_gpos", "e_first", "c", "lo", "hi", "d_last")]


def domain_forward_carries(summaries, S: int, max_gap: int) -> List[dict]:
    """summaries: what pass S gave for the consecutive pieces of one context and sequence -> per piece the carry that passes C and
    G take: has_prev, prev_gpos, prev_d -- whether a row precedes the piece, and the nearest one's locus and d.  A piece without
    rows hands its carry on.  A composite is only ever applied to a d within +-2^46 and two are never composed, so its constant
    form (lo == hi) is exact here."""
    out, has, g, d = [], False, 0, 0
    for s in summaries:
        out.append({"has_prev": has, "prev_gpos": g, "prev_d": d})
        if s["n_rows"]:
            s0 = S if has and s["first_gpos"] - g <= max_gap else 0
            d = min(max(d if has else 0, -s0), s0) + s["e_first"]                  # row 0
            d = min(max(d + s["c"], s["lo"]), s["hi"])                             # rows 1 .. R - 1
            has, g = True, s["last_gpos"]
    return out


def domain_backward_carries(summaries, codes, S: int, max_gap: int) -> List[dict]:
    """... and, with what pass C gave (d_last, back), per piece what pass G takes besides: has_next, next_gpos -- whether a row
    follows the piece, and the nearest one's locus -- and last_state, the state of the piece's last row: the back-pointer across
    the cut (1 if d_last > S_link, 0 if d_last < -S_link, else the state of the row behind it; S_link = S up to max_gap, else
    0), or d_last > 0 where nothing follows."""
    out, has, g, z = [None] * len(summaries), False, 0, 0
    for i in range(len(summaries) - 1, -1, -1):
        s, c = summaries[i], codes[i]
        out[i] = {"has_next": has, "next_gpos": g, "last_state": z}
        if not s["n_rows"]:
            continue
        link = S if has and g - s["last_gpos"] <= max_gap else 0
        last = (1 if c["d_last"] > 0 else 0) if not has else 1 if c["d_last"] > link else 0 if c["d_last"] < -link else z
        out[i]["last_state"] = last
        z = last if c["back"] == DOMAIN_KEEP else c["back"]                        # the state of the piece's first row
        has, g = True, s["first_gpos"]
    return out


def chain_domain_parts(pieces, A: int, B: int, S: int, max_gap: int) -> List[np.ndarray]:
    """pieces: consecutive pieces of one context and sequence, each a callable piece(pass_, carry, A, B, S, max_gap) -> dict like
    functools.partial(pu.domains_part, ctx, lo, hi, planes=..., plane_base=...).  -> the segments of every piece, for
    stitch_domains: pass S on every piece, the carries from left to right, pass C, the carries from right to left, pass G.  Where
    the pieces live in several processes, those run the same three passes with the two carry functions between their exchanges."""
    rule = (A, B, S, max_gap)
    summaries = [p(DOMAIN_PASS_SUMMARY, {}, *rule) for p in pieces]
    fwd = domain_forward_carries(summaries, S, max_gap)
    codes = [p(DOMAIN_PASS_CODES, f, *rule) if s["n_rows"] else {} for p, s, f in zip(pieces, summaries, fwd)]
    bwd = domain_backward_carries(summaries, codes, S, max_gap)
    return [p(DOMAIN_PASS_SEGMENTS, {**f, **b}, *rule)["segments"] if s["n_rows"] else np.zeros(0, DOMAIN_DTYPE)
            for p, s, f, b in zip(pieces, summaries, fwd, bwd)]


def stitch_domains(parts, A: int, B: int) -> np.ndarray:
    """parts: the segments chain_domain_parts gave for consecutive pieces -> the segments of the whole.  A piece's first segment
    always starts at its first row; it continues the last segment before it when the states are equal and no break lies between
    (it lacks DOMAIN_AFTER_BREAK): pcov, ncov and n_loci add, end is the right one's, the flags are the outer ends', level and
    score are recomputed from the sums, each operation rounded once in fp64 as the device does."""
    out: List[np.ndarray] = []
    for rows in parts:
        for k, g in enumerate(np.ascontiguousarray(rows, DOMAIN_DTYPE)):
            g = g.copy()
            if k == 0 and out and out[-1]["state"] == g["state"] and not int(g["flags"]) & DOMAIN_AFTER_BREAK:
                o = out[-1]
                for c in ("pcov", "ncov", "n_loci"):
                    o[c] += g[c]
                o["end"] = g["end"]
                o["flags"] = (int(o["flags"]) & DOMAIN_AFTER_BREAK) | (int(g["flags"]) & DOMAIN_BEFORE_BREAK)
                P, N = np.float64(int(o["pcov"])), np.float64(int(o["ncov"]))
                o["level"] = np.float64(100.0) * P / (P + N)
                o["score"] = (P * np.float64(A) + N * np.float64(B)) / np.float64(65536.0)
            else:
                out.append(g)
    return np.array(out, DOMAIN_DTYPE) if out else np.zeros(0, DOMAIN_DTYPE)


def parse_domain_levels(text: str) -> List[Optional[Tuple[float, float]]]:
    """the value of -u: lo:hi once for all contexts or three times (CpG,CHG,CHH), `nan` instead of a pair: that context is not
    segmented (None); ValueError unless the whole text parses"""
    items = text.split(",")
    if len(items) not in (1, 3):
        raise ValueError("one lo:hi pair or three expected")
    out = []
    for t in items:
        if t == "nan":
            out.append(None)
            continue
        if ":" not in t or set(t) - set("0123456789.eE+-:"):
            raise ValueError("lo:hi or nan expected")
        a, b = t.split(":", 1)
        out.append((float(a), float(b)))
    return out * 3 if len(out) == 1 else out


def domains_bed(rows: np.ndarray, names: Sequence[str], offsets) -> dict:
    """the text of <prefix>.domains.{CpG,CHG,CHH}.bed: chrom, start, end, n_loci, L|H, level, pcov, ncov, score"""
    sid, soff = locate(offsets, rows["start"])
    text = {k: [] for k in CTX_NAMES}
    for s, k, r in zip(sid, soff, rows):
        text[CTX_NAMES[int(r["motif"])]].append("%s\t%d\t%d\t%d\t%s\t%g\t%d\t%d\t%.6g\n" % (
            names[s], k, k + (r["end"] - r["start"]), r["n_loci"], "H" if r["state"] else "L", r["level"], r["pcov"], r["ncov"], r["score"]))
    return {k: "".join(v) for k, v in text.items()}


def pattern_stats(row) -> Tuple[float, float, float, float]:
    """one PATTERN_DTYPE row -> (entropy, epipolymorphism, pdr, level) by the C library (host only: no GPU is needed): with
    f = counts / n over the non-empty patterns, (0 - sum f log2 f) / k, 1 - sum f^2, 1 - (counts[0] + counts[2^k - 1]) / n and
    100 sum popcount(pattern) counts / (k n)"""
    w = np.array(row, PATTERN_DTYPE).reshape(1)
    out = np.zeros(4, np.float64)
    if lib().hm_pattern_stats(w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_pattern_stats: k in 2..4 and n = the sum of the 2^k counts > 0 expected")
    return tuple(float(x) for x in out)


def linkage_stats(row) -> Tuple[float, float]:
    """one LINKAGE_DTYPE row -> (concordance, r) by the C library (host only: no GPU is needed): (n_uu + n_mm) / n and the phi
    coefficient (n_mm n_uu - n_mu n_um) / sqrt of the product of the four margins, nan when a margin is 0"""
    w = np.array(row, LINKAGE_DTYPE).reshape(1)
    out = np.zeros(2, np.float64)
    if lib().hm_linkage_stats(w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_linkage_stats: n = n_uu + n_um + n_mu + n_mm > 0 expected")
    return tuple(float(x) for x in out)


def linkage_tsv(rows: np.ndarray) -> str:
    """the text of <prefix>.linkage.CpG.tsv: the header, then dist, n, n_uu, n_um, n_mu, n_mm, concordance, r per row (a row
    without pairs has no statistics: nan)"""
    text = ["#dist\tn\tn_uu\tn_um\tn_mu\tn_mm\tconcordance\tr\n"]
    for r in rows:
        c = [int(r[k]) for k in ("n_uu", "n_um", "n_mu", "n_mm")]
        st = linkage_stats(r) if sum(c) else (float("nan"), float("nan"))
        text.append("%d\t%d\t%d\t%d\t%d\t%d\t%.6g\t%.6g\n" % (int(r["dist"]), sum(c), *c, *st))
    return "".join(text)


def readpos_stats(row) -> Tuple[float, float]:
    """one READPOS_DTYPE row -> (percent methylated, mean ML byte) by the C library (host only: no GPU is needed)"""
    w = np.array(row, READPOS_DTYPE).reshape(1)
    out = np.zeros(2, np.float64)
    if lib().hm_readpos_stats(w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_readpos_stats: n = n_m + n_u > 0 expected")
    return tuple(float(x) for x in out)


def readpos_tsv(rows: np.ndarray) -> str:
    """the text of <prefix>.readpos.tsv: the header, then context, end, dist, n, n_m, n_u, percent, mean_ml per row (a row without
    calls has no statistics: nan)"""
    text = ["#context\tend\tdist\tn\tn_m\tn_u\tpercent\tmean_ml\n"]
    for r in rows:
        n_m, n_u = int(r["n_m"]), int(r["n_u"])
        st = readpos_stats(r) if n_m + n_u else (float("nan"), float("nan"))
        text.append("%s\t%s\t%d\t%d\t%d\t%d\t%g\t%.6g\n" % (CTX_NAMES[int(r["motif"])], READPOS_ENDS[int(r["end"])], int(r["dist"]), n_m + n_u,
                                                           n_m, n_u, *st))
    return "".join(text)


def region_geometry() -> Tuple[int, int]:
    """(HM_REGION_BLOCK, HM_REGION_SCAN_BLOCKS) of the loaded library: the loci per block of the interval index, and the blocks
    per workgroup of its scan (host only: no GPU is needed)"""
    g = np.zeros(2, np.int64)
    lib().hm_region_geometry(g.ctypes.data_as(C.c_void_p))
    return int(g[0]), int(g[1])


class Regions:
    """the intervals of a BED file in input order: sid (index of the sequence), start, end (positions in it, int64), name, strand
    ('+', '-' or '.')"""

    def __init__(self, sid, start, end, name, strand):
        self.sid, self.start, self.end = (np.asarray(x, np.int64).reshape(-1) for x in (sid, start, end))
        self.name, self.strand = list(name), list(strand)

    def __len__(self):
        return len(self.sid)

    def coords(self, offsets) -> dict:
        """global locus coordinates, as regions() and metaplot() take them: start, end, seq_start, seq_end, strand"""
        off = np.asarray(offsets, np.int64)
        return {"start": off[self.sid] + self.start, "end": off[self.sid] + self.end, "seq_start": off[self.sid],
                "seq_end": off[self.sid + 1], "strand": "".join(self.strand).encode()}


def parse_regions_bed(path: str, names: Sequence[str], lengths) -> Regions:
    """`pileup -R`: a BED file, plain or gzip, of at least 3 tab-separated columns.  Empty lines and lines starting with `#`,
    `track` or `browser` are skipped; the name is column 4 or `.`, the strand column 6 if it is `+` or `-`, else `.`.  ValueError
    naming the line for fewer columns, coordinates that are no integers, an unknown sequence, start < 0, start >= end or
    end > the sequence's length."""
    import gzip
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    sid_of = {n: i for i, n in enumerate(names)}
    sid, start, end, name, strand = [], [], [], [], []
    with (gzip.open(path, "rt") if gz else open(path, "r")) as f:
        for no, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line or line.startswith(("#", "track", "browser")):
                continue
            col = line.split("\t")
            bad = lambda what: ValueError(f"{path}:{no}: {what}")  # noqa: E731
            if len(col) < 3:
                raise bad("fewer than 3 tab-separated columns")
            try:
                a, b = int(col[1]), int(col[2])
            except ValueError:
                raise bad("start and end must be integers") from None
            if col[0] not in sid_of:
                raise bad(f"unknown sequence {col[0]}")
            if a < 0:
                raise bad("start < 0")
            if a >= b:
                raise bad("start >= end")
            if b > int(lengths[sid_of[col[0]]]):
                raise bad(f"end {b} is past the end of {col[0]} ({int(lengths[sid_of[col[0]]])})")
            sid.append(sid_of[col[0]])
            start.append(a)
            end.append(b)
            name.append(col[3] if len(col) > 3 and col[3] else ".")
            strand.append(col[5] if len(col) > 5 and col[5] in ("+", "-") else ".")
    return Regions(sid, start, end, name, strand)


def parse_metaplot(text: str) -> Tuple[int, int, int]:
    """`pileup -J`: bins[:flank_bp:flank_bins] -> (bins, flank, flank_bins); bins in 1 .. 1000, the flank 0:0 or flank_bp >= 1 a
    multiple of flank_bins in 1 .. 1000.  ValueError otherwise."""
    parts = text.split(":")
    if len(parts) not in (1, 3) or not all(t.isascii() and t.isdigit() and len(t) < 18 for t in parts):
        raise ValueError("bins[:flank_bp:flank_bins] expected")
    bins, flank, fb = (int(t) for t in parts + ["0", "0"][:3 - len(parts)])
    if not 1 <= bins <= METAPLOT_MAX_BINS or fb > METAPLOT_MAX_BINS or (flank == 0) != (fb == 0) or (fb and flank % fb):
        raise ValueError("bins in [1, 1000], flank_bp a multiple of flank_bins in [1, 1000] (or both 0) expected")
    return bins, flank, fb


def region_stats(row) -> Tuple[float, float]:
    """one REGION_SUM_DTYPE row (or the four sums of a METABIN_DTYPE row) -> (weighted, mean) percent by the C library (host only:
    no GPU is needed): 100 pcov / (pcov + ncov) and ppm / n_loci / 10^4"""
    w = np.zeros(1, REGION_SUM_DTYPE)
    for k in REGION_SUM_DTYPE.names:
        w[k] = row[k]
    out = np.zeros(2, np.float64)
    if lib().hm_region_stats(w.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_region_stats: n_loci > 0 expected")
    return tuple(float(x) for x in out)


def smooth_stats(row, half_width: int) -> Tuple[float, float]:
    """one SMOOTH_DTYPE row -> (smoothed level in percent, effective coverage) by the C library (host only: no GPU is needed):
    100 wp / (wp + wn) and (wp + wn) / half_width"""
    r = np.zeros(1, SMOOTH_DTYPE)
    for k in SMOOTH_DTYPE.names:
        r[k] = row[k]
    out = np.zeros(2, np.float64)
    if lib().hm_smooth_stats(r.ctypes.data_as(C.c_void_p), half_width, out.ctypes.data_as(C.c_void_p)) != 0:
        raise HifimethError("hm_smooth_stats: half_width >= 1 and wp + wn > 0 expected")
    return tuple(float(x) for x in out)


def _region_columns(r) -> str:
    st = region_stats(r) if int(r["n_loci"]) else (float("nan"), float("nan"))
    return "%d\t%d\t%d\t%.6g\t%.6g\n" % (int(r["n_loci"]), int(r["pcov"]), int(r["ncov"]), *st)


def regions_tsv(regions: Regions, names: Sequence[str], sums: np.ndarray) -> dict:
    """the text of <prefix>.regions.{CpG,CHG,CHH}.tsv: the header, then chrom, start, end, name, strand, n_loci, pcov, ncov,
    weighted, mean per interval in input order (an interval without a counted locus has no percentages: nan); sums = [n, 3]"""
    head = "#chrom\tstart\tend\tname\tstrand\tn_loci\tpcov\tncov\tweighted\tmean\n"
    return {CTX_NAMES[c]: head + "".join(
        "%s\t%d\t%d\t%s\t%s\t" % (names[regions.sid[i]], regions.start[i], regions.end[i], regions.name[i], regions.strand[i])
        + _region_columns(sums[i, c]) for i in range(len(regions))) for c in range(3)}


def metaplot_tsv(rows: np.ndarray, n_used: int, n_skipped: int, bins: int, flank_bins: int) -> dict:
    """the text of <prefix>.metaplot.{CpG,CHG,CHH}.tsv: `#regions used skipped`, the header, then bin, part (up, body, down),
    n_regions, n_loci, pcov, ncov, weighted, mean per bin; rows = the 3 x (bins + 2 flank_bins) METABIN_DTYPE rows"""
    nb = bins + 2 * flank_bins
    head = "#regions\t%d\t%d\n#bin\tpart\tn_regions\tn_loci\tpcov\tncov\tweighted\tmean\n" % (n_used, n_skipped)
    part = lambda b: "up" if b < flank_bins else "body" if b < flank_bins + bins else "down"  # noqa: E731
    return {CTX_NAMES[c]: head + "".join("%d\t%s\t%d\t" % (b, part(b), int(rows[c * nb + b]["n_regions"])) + _region_columns(rows[c * nb + b])
                                         for b in range(nb)) for c in range(3)}


def context_geometry() -> Tuple[int, int, int]:
    """(HM_CONTEXT_SPAN, HM_CONTEXT_LDS_FLANK, HM_CONTEXT_LDS_MAX_FLANK) of the loaded library: the loci a workgroup of the
    k-mer kernel takes side by side, the largest flank that takes the LDS path, and the largest that could (host only)"""
    g = np.zeros(3, np.int64)
    lib().hm_context_geometry(g.ctypes.data_as(C.c_void_p))
    return int(g[0]), int(g[1]), int(g[2])


def context_kmer(code: int, k: int) -> str:
    """row `code` of a `pileup -S` table as its k bases (A = 0, C = 1, G = 2, T = 3, first base most significant); 4^k: `other`"""
    if not 0 <= code <= 4 ** k:
        raise ValueError(f"code {code} outside [0, 4^{k}]")
    return "other" if code == 4 ** k else "".join("ACGT"[(code >> (2 * (k - 1 - j))) & 3] for j in range(k))


def context_code(kmer: str) -> int:
    """the inverse of context_kmer: k bases of ACGT, or `other` (which needs no k: use 4^k)"""
    code = 0
    for ch in kmer:
        code = code * 4 + "ACGT".index(ch)
    return code


def context_tsv(table: np.ndarray, flank: int) -> dict:
    """the text of <prefix>.context.{CpG,CHG,CHH}.tsv from context()'s [3, K + 1, 4] table: the header, then per k-mer with a
    counted locus, in k-mer order, context, n_loci, pcov, ncov, weighted, mean; `other` last if it is not empty"""
    k = 3 + 2 * flank
    table = np.asarray(table, np.int64)
    assert table.shape == (3, 4 ** k + 1, 4)
    head = "#context\tn_loci\tpcov\tncov\tweighted\tmean\n"
    text = {}
    for c in range(3):
        rows = np.zeros(table.shape[1], REGION_SUM_DTYPE)
        for q, name in enumerate(REGION_SUM_DTYPE.names):
            rows[name] = table[c, :, q]
        text[CTX_NAMES[c]] = head + "".join(context_kmer(int(code), k) + "\t" + _region_columns(rows[code])
                                            for code in np.flatnonzero(rows["n_loci"] > 0))
    return text


def sites_rates_tsv(sums, rates, m) -> str:
    """the text of <prefix>.sites.rates.tsv: ctx, P_c, N_c, rate, m_c (the counts are 0 when the rates were given with -e)"""
    return "".join("%s\t%d\t%d\t%s\t%d\n" % (CTX_NAMES[c], int(sums[c]), int(sums[3 + c]),
                                             "nan" if np.isnan(rates[c]) else "%.17g" % rates[c], int(m[c])) for c in range(3))


def locate(offsets, gpos) -> Tuple[np.ndarray, np.ndarray]:
    """loci of the concatenated reference -> (sequence index, offset in that sequence), both int64; offsets = the n + 1 sequence
    starts.  What every BED writer below names its rows by; a locus on a sequence boundary belongs to the sequence that starts
    there, and empty sequences own none."""
    offsets = np.asarray(offsets, np.int64)
    gpos = np.asarray(gpos, np.int64)
    sid = np.searchsorted(offsets, gpos, side="right") - 1
    return sid, gpos - offsets[sid]


def read_cov_bed(path: str, fasta_names: Sequence[str], offsets, motif: Optional[int] = None):
    """`diff`: one <prefix>.<ctx>.cov.bed, plain or gzip -> (gpos, pcov, ncov, motif) as int64, int32, int32, uint32 arrays, the
    arguments of MethylationPileup.load_loci.  offsets = the n + 1 sequence starts of the concatenated reference; motif = the
    file's context index (0 CpG, 1 CHG, 2 CHH), by default read from the file name.  A row is chrom, start, start + 1, a column
    that is not read, pcov, ncov; further columns (cov2bed's motif) are ignored and empty lines skipped.  ValueError naming file and
    line for fewer than 6 tab-separated columns, an unknown sequence, a start that is no integer inside the sequence,
    end != start + 1, or a count that is not a plain decimal integer in 0 .. 2^31 - 1."""
    import gzip
    if motif is None:
        found = [c for c, n in enumerate(CTX_NAMES) if (".%s.cov.bed" % n) in os.path.basename(path)]
        if len(found) != 1:
            raise ValueError(f"{path}: the context is not in the file name, give motif")
        motif = found[0]
    offsets = np.asarray(offsets, np.int64)
    sid_of = {n: i for i, n in enumerate(fasta_names)}
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    gpos, pcov, ncov = [], [], []

    def number(text):                                         # digits only, at most 18 of them: what the CLI takes
        return int(text) if text.isascii() and text.isdigit() and len(text) <= 18 else None

    with (gzip.open(path, "rt", newline="\n") if gz else open(path, "r", newline="\n")) as f:   # a line ends at \n, as in the CLI
        for no, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if line.endswith("\r"):
                line = line[:-1]
            if not line:
                continue
            col = line.split("\t")
            bad = lambda what: ValueError(f"{path}:{no}: {what}")  # noqa: E731
            if len(col) < 6:
                raise bad("fewer than 6 tab-separated columns")
            if col[0] not in sid_of:
                raise bad(f"unknown sequence {col[0]}")
            sid = sid_of[col[0]]
            start, end, p, n = number(col[1]), number(col[2]), number(col[4]), number(col[5])
            if start is None or start >= offsets[sid + 1] - offsets[sid]:
                raise bad(f"start is not an integer inside {col[0]} ({int(offsets[sid + 1] - offsets[sid])} bases)")
            if end != start + 1:
                raise bad("end is not start + 1")
            if p is None or n is None or p > 0x7fffffff or n > 0x7fffffff:
                raise bad("the counts in columns 5 and 6 must be integers in 0 .. 2147483647")
            gpos.append(int(offsets[sid]) + start)
            pcov.append(p)
            ncov.append(n)
    return (np.array(gpos, np.int64), np.array(pcov, np.int32), np.array(ncov, np.int32), np.full(len(gpos), motif, np.uint32))


class MethylationPileup:
    def __init__(self, genome: Sequence[Tuple[str, str]], device: int = 0, min_mapq: int = 0, min_pi: float = 0.0,
                 planes=None, partitions: bool = False, partition_planes=None, bases=None, patterns: int = 0,
                 pattern_span: int = PATTERN_SPAN, bedmethyl: bool = False, linkage: int = 0, profile: int = 0,
                 trim: Tuple[int, int] = (0, 0), groups: bool = False, group_min_cov: int = 5, samples: int = 0,
                 sample_min_cov: int = 5):
        """genome: [(name, SEQUENCE)].  bases: optional, the concatenated upper-case bases of the whole reference as a
        C-contiguous uint8 buffer (ndarray, bytes, memoryview), handed to the engine as it is -- for references of gigabases,
        where joining, upper-casing and encoding strings would copy them three times; the second member of each genome entry
        may then be the sequence's length instead of its text.
        planes: optional (pcov, ncov, key) torch CUDA tensors (int32, int32, int32-as-bits) of total genome length
        that the engine counts into -- used when a collective consumes them afterwards.
        partitions: also count per haplotype (HP 1 / 2); partition_planes: optional ((pcov1, ncov1), (pcov2, ncov2)) int32
        torch CUDA tensors for them, like `planes`.
        patterns: 0, or k in (2, 3, 4): also count the read-level patterns over windows of k adjacent reference CpGs whose first
        and last locus are at most pattern_span (1 .. 65 536) bases apart (+72 B per reference CpG, 8 B per window record).
        bedmethyl: also count the depth classes per reference CpG (+28 B per reference CpG, +68 B with partitions).
        linkage: 0, or max_dist in 2 .. 16 384: also count the pairs of CpG calls of one record by their distance up to max_dist
        (+6 144 B per distance, whatever the depth).
        profile: 0, or D in 1 .. 2 048: also count every projected call by its position in the read, the D bases at either end one
        row each (+3 x (2 D + 1) x 2 048 B: 12.6 MB at 1 024).
        trim: (n5, n3): the entries in the first n5 and the last n3 bases of every read are dropped.
        groups (needs partitions=True): replicate groups -- begin_sample / load_sample_loci / group_tests (+18.125 B per reference
        base); group_min_cov: the coverage a sample needs at a locus to count there.
        samples: 0, or N in 2 .. 64: N samples' level planes -- open_sample / load_sample / sample_sums (+2 N B per reference
        base); sample_min_cov: the coverage a sample needs at a locus to count there."""
        self._L = lib()
        self._h = C.c_void_p()
        if self._L.hm_pileup_create(C.byref(self._h), device) != 0:
            raise HifimethError(self._L.hm_pileup_last_error(None).decode())
        self._planes = planes
        self.partitions = bool(partitions)
        self._check(self._L.hm_pileup_set_option(self._h, b"min_mapq", float(min_mapq)))
        self._check(self._L.hm_pileup_set_option(self._h, b"min_pi", float(min_pi)))
        if self.partitions:
            self._check(self._L.hm_pileup_set_option(self._h, b"partitions", 2.0))
            for part, pair in enumerate(partition_planes or (), 1):
                self._check(self._L.hm_pileup_use_partition_planes(self._h, part, *(C.c_void_p(t.data_ptr()) for t in pair)))
        elif partition_planes is not None:
            raise HifimethError("partition_planes without partitions=True")
        self.pattern_k = int(patterns)
        if patterns:
            self._check(self._L.hm_pileup_set_option(self._h, b"patterns", float(patterns)))
            self._check(self._L.hm_pileup_set_option(self._h, b"pattern_span", float(pattern_span)))
        if bedmethyl:
            self._check(self._L.hm_pileup_set_option(self._h, b"bedmethyl", 1.0))
        self.linkage_max_dist = int(linkage)
        if linkage:
            self._check(self._L.hm_pileup_set_option(self._h, b"linkage", float(linkage)))
        self.profile = int(profile)
        if profile:
            self._check(self._L.hm_pileup_set_option(self._h, b"profile", float(profile)))
        if tuple(trim) != (0, 0):
            self._check(self._L.hm_pileup_set_option(self._h, b"trim5", float(trim[0])))
            self._check(self._L.hm_pileup_set_option(self._h, b"trim3", float(trim[1])))
        if groups:
            self._check(self._L.hm_pileup_set_option(self._h, b"groups", 1.0))
            self._check(self._L.hm_pileup_set_option(self._h, b"group_min_cov", float(group_min_cov)))
        if samples:
            self._check(self._L.hm_pileup_set_option(self._h, b"samples", float(samples)))
            self._check(self._L.hm_pileup_set_option(self._h, b"sample_min_cov", float(sample_min_cov)))
        if planes is not None:
            self._check(self._L.hm_pileup_use_planes(self._h, *(C.c_void_p(t.data_ptr()) for t in planes)))
        self.set_reference(genome, bases)

    def set_reference(self, genome: Sequence[Tuple[str, str]], bases=None):
        """hm_pileup_set_reference: `genome` and `bases` as for the constructor, which ends with this call.  A later call
        re-targets the engine: it keeps its options and the caller's planes (which stay the caller's to zero, and must hold the new
        reference) and is otherwise a new engine on `genome` -- staged and resident records, histograms, every table, the seen
        bits, the opened samples and a void state are dropped.  A call that fails leaves engine and object as they were."""
        lengths = np.array([int(s) if isinstance(s, (int, np.integer)) else len(s) for _, s in genome], np.int64)
        if bases is None:
            if any(isinstance(s, (int, np.integer)) for _, s in genome):
                raise HifimethError("a genome entry that gives a length needs `bases`")
            bases = "".join(s for _, s in genome).upper().encode()
        flat = np.frombuffer(bases, np.uint8) if not isinstance(bases, np.ndarray) else bases
        if flat.dtype != np.uint8 or flat.ndim != 1 or not flat.flags.c_contiguous or flat.size != int(lengths.sum()):
            raise HifimethError("bases: one contiguous uint8 per reference base expected (%d)" % int(lengths.sum()))
        self._check(self._L.hm_pileup_set_reference(self._h, len(genome), lengths.ctypes.data_as(C.c_void_p),
                                                    flat.ctypes.data_as(C.c_void_p)))
        self.names = [n for n, _ in genome]
        self.lengths = lengths
        self.offsets = np.concatenate([[0], np.cumsum(lengths)])
        self._order = 0

    def close(self):
        if self._h:
            self._L.hm_pileup_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise HifimethError(self._L.hm_pileup_last_error(self._h).decode())
        return rc

    def _rows(self, fn, dtype, *args) -> np.ndarray:
        """the rows of one of the engine's row fetches fn(handle, *args, out, cap): asked for their number, then fetched"""
        n = self._check(fn(self._h, *args, None, 0))
        out = np.zeros(n, dtype)
        if n:
            self._check(fn(self._h, *args, out.ctypes.data_as(C.c_void_p), n))
        return out

    @property
    def n_loci(self) -> int:
        return int(self.offsets[-1])

    def add(self, read, order: Optional[int] = None) -> int:
        """read: synth.AlignedRead-like (flag, tid, pos, mapq, cigar_u32(), seq, seq4, mm, ml[, hp]).  -> 1 staged / 0 skipped.
        With partitions, a read whose hp is 1 or 2 is also counted in that partition; any other hp only in the combined output."""
        if order is None:
            order = self._order
        self._order = order + 1
        mods = parse_mods(read.seq, read.flag, read.mm, read.ml)
        if len(mods) == 0 or read.flag & 4:
            return 0
        seq4 = np.ascontiguousarray(read.seq4, np.uint8)
        cig = np.ascontiguousarray(read.cigar_u32(), np.uint32)
        args = (self._h, order, read.flag, read.tid, read.pos, read.mapq, len(read.seq), seq4.ctypes.data_as(C.c_void_p),
                len(cig), cig.ctypes.data_as(C.c_void_p), len(mods), mods.ctypes.data_as(C.c_void_p))
        if not self.partitions:
            return self._check(self._L.hm_pileup_submit_read(*args))
        hp = getattr(read, "hp", None)
        return self._check(self._L.hm_pileup_submit_read_hp(*args, hp if hp in (1, 2) else 0))

    def add_called(self, read, calls: np.ndarray, order: Optional[int] = None, hp: int = 0) -> int:
        """The fused path (hm_pileup_submit_read_calls): `read` as for add() -- its mm / ml are not looked at --, `calls` = the
        caller.CALL_DTYPE records the caller mirror returned for this read (FWD strand by ascending qoff, then REV), handed to the
        engine as they are: no MM/ML text is written or parsed.  Same effect as add() of the read carrying those calls as tags.
        -> 1 staged / 0 skipped (no calls, unmapped)."""
        from .caller import CALL_DTYPE
        if order is None:
            order = self._order
        self._order = order + 1
        if calls.dtype != CALL_DTYPE or not calls.flags.c_contiguous:   # (a slice of the caller's result is a view: no copy)
            calls = np.ascontiguousarray(calls, CALL_DTYPE)
        seq4 = np.ascontiguousarray(read.seq4, np.uint8)
        cig = np.ascontiguousarray(read.cigar_u32(), np.uint32)
        return self._check(self._L.hm_pileup_submit_read_calls(
            self._h, order, read.flag, read.tid, read.pos, read.mapq, len(read.seq), seq4.ctypes.data_as(C.c_void_p), len(cig),
            cig.ctypes.data_as(C.c_void_p), len(calls), calls.ctypes.data_as(C.c_void_p), hp))

    def flush(self):
        self._check(self._L.hm_pileup_run(self._h))

    def num_records(self) -> int:
        return int(self._L.hm_pileup_num_records(self._h))

    def histograms(self) -> np.ndarray:
        b = np.zeros(768, np.uint64)
        self._check(self._L.hm_pileup_histograms(self._h, b.ctypes.data_as(C.c_void_p)))
        return b.reshape(3, 256)

    def records(self):
        """projected calls still resident (unordered): (gpos, prob, motif, order)"""
        n = self.num_records()
        g, p, m, o = np.zeros(n, np.int64), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        self._check(self._L.hm_pileup_fetch_records(self._h, *(x.ctypes.data_as(C.c_void_p) for x in (g, p, m, o)), n))
        return g, p, m, o

    def label_histograms(self, labels: np.ndarray) -> np.ndarray:
        """`hifimeth eval` (eval.cpp:469-560): resident records joined with per-locus truth labels (int8 over the
        concatenated reference: -1 none, 0 unmethylated, 1 methylated) -> counts[motif, label, scaled_prob]"""
        lab = np.ascontiguousarray(labels, np.int8)
        b = np.zeros(1536, np.uint64)
        self._check(self._L.hm_pileup_label_histograms(self._h, lab.ctypes.data_as(C.c_void_p), lab.size,
                                                       b.ctypes.data_as(C.c_void_p)))
        return b.reshape(3, 2, 256)

    @staticmethod
    def resolve_thresholds(bins) -> List[int]:
        return [resolve_threshold(bins[c])[0] for c in range(3)]

    def count(self, thresholds: Sequence[int]):
        t = np.asarray(thresholds, np.uint8)
        self._check(self._L.hm_pileup_count(self._h, t.ctypes.data_as(C.c_void_p)))

    def loci(self, lo: int = 0, hi: Optional[int] = None, planes=None, plane_base: int = 0, partition: int = 0) -> np.ndarray:
        """covered loci of [lo, hi) (plane coordinates) in ascending order; planes = torch tensors or None (own).
        partition 1 / 2 (planes None): that haplotype's counts, motif from the combined key plane."""
        hi = self.n_loci if hi is None else hi
        if planes is not None:
            ptrs = [C.c_void_p(t.data_ptr()) for t in planes]
        elif partition:
            pc, nc = C.c_void_p(), C.c_void_p()
            self._check(self._L.hm_pileup_partition_planes(self._h, partition, C.byref(pc), C.byref(nc)))
            ptrs = [pc, nc, None]                 # key NULL = the engine's combined key plane
        else:
            ptrs = [None, None, None]
        return self._rows(self._L.hm_pileup_fetch_loci, LOCUS_DTYPE, *ptrs, plane_base, lo, hi)

    def _load(self, call, gpos, pcov, ncov, motif, *lead) -> int:
        """the rows of a load as one LOCUS_DTYPE array, given to the engine call `call` behind its leading arguments"""
        gpos = np.ascontiguousarray(gpos, np.int64)
        rows = np.zeros(len(gpos), LOCUS_DTYPE)
        rows["gpos"], rows["pcov"], rows["ncov"], rows["motif"] = gpos, pcov, ncov, motif
        return self._check(call(self._h, *lead, rows.ctypes.data_as(C.c_void_p), len(rows)))

    def load_loci(self, part: int, gpos, pcov, ncov, motif) -> int:
        """`diff` (hm_pileup_load_loci): counts from elsewhere -- the rows of a sample's *.cov.bed, as read_cov_bed returns them
        -- added into partition `part` (1 or 2) and the combined planes; motif an array or one context index for all rows.  Needs
        partitions=True and an engine that never saw a read; afterwards loci(), asm(), asm_histogram(), asm_regions() and the
        other plane fetches work as after count(), part 1 against part 2.  -> the number of rows that added a count.
        HifimethError for a row outside the reference, a negative count, a motif above 3 or a locus given twice for one part:
        the engine's planes are then void and it refuses further loads and fetches."""
        return self._load(self._L.hm_pileup_load_loci, gpos, pcov, ncov, motif, part)

    def begin_sample(self, part: int) -> int:
        """`groupdiff` (hm_pileup_group_sample): opens the next sample of group `part` (1 or 2); load_sample_loci then adds its rows.
        -> the sample's index within its group.  Needs groups=True and an engine that never saw a read or a load_loci."""
        return self._check(self._L.hm_pileup_group_sample(self._h, part))

    def load_sample_loci(self, gpos, pcov, ncov, motif) -> int:
        """`groupdiff` (hm_pileup_load_sample_loci): rows of the open sample, as read_cov_bed returns them; any number of calls.
        A locus with pcov + ncov >= group_min_cov adds its counts to the group's partition planes and the combined ones, its
        moment floor(pcov^2 2^20 / (pcov + ncov)) and one sample.  -> the number of rows that added.  HifimethError for a row
        outside the reference, a negative count, a count of 2^20 or more, a motif above 3 or a locus twice in this sample: the
        engine is then void."""
        return self._load(self._L.hm_pileup_load_sample_loci, gpos, pcov, ncov, motif)

    def group_planes(self, part: int, lo: int = 0, hi: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """-> (moment uint64, samples uint8) of group `part` over [lo, hi): the sum of the counting samples' moments and their number"""
        hi = self.n_loci if hi is None else hi
        moment, samples = np.zeros(max(hi - lo, 0), np.uint64), np.zeros(max(hi - lo, 0), np.uint8)
        self._check(self._L.hm_pileup_group_planes(self._h, part, lo, hi, moment.ctypes.data_as(C.c_void_p), samples.ctypes.data_as(C.c_void_p)))
        return moment, samples

    def group_tests(self, lo: int = 0, hi: Optional[int] = None, min_reps: int = 2) -> np.ndarray:
        """`groupdiff` (hm_pileup_fetch_groups): the loci of [lo, hi) with at least min_reps counting samples in each group and
        m1 + m2 >= 3, ascending (GROUP_DTYPE): the pooled counts, diff, the binomial likelihood ratio D, the dispersion phi
        = max(1, Pearson X2 / nu) and pvalue = P(F(1, nu) >= D / phi), nu = m1 + m2 - 2."""
        hi = self.n_loci if hi is None else hi
        return self._rows(self._L.hm_pileup_fetch_groups, GROUP_DTYPE, lo, hi, min_reps)

    def groups_bed(self, rows: np.ndarray, q: np.ndarray) -> dict:
        """the text of <prefix>.groups.{CpG,CHG,CHH}.bed: chrom, k, k+1, diff, p, q, m1, pcov1, ncov1, m2, pcov2, ncov2, phi"""
        sid, soff = locate(self.offsets, rows["gpos"])
        text = {k: [] for k in CTX_NAMES}
        for s, k, r, qv in zip(sid, soff, rows, q):
            text[CTX_NAMES[min(int(r["motif"]), 2)]].append("%s\t%d\t%d\t%g\t%.6g\t%.6g\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n" % (
                self.names[s], k, k + 1, r["diff"], r["pvalue"], qv, r["m1"], r["pcov1"], r["ncov1"], r["m2"], r["pcov2"], r["ncov2"], r["phi"]))
        return {k: "".join(v) for k, v in text.items()}

    def group_regions(self, ctx: int, lo: int = 0, hi: Optional[int] = None, min_reps: int = 2, max_p: float = 0.01, min_diff: float = 0.0,
                      max_gap: int = 500, min_loci: int = 3, keep_edges: bool = False) -> Tuple[np.ndarray, int, int]:
        """`groupdmr` (hm_dmr_fetch_regions) -> (rows, n_ctx_rows, n_hits): the chains of context ctx among the
        group_tests() rows of [lo, hi), ascending (GROUP_REGION_DTYPE), the number of those rows and of the hits among them.  A row
        is a hit when pvalue <= max_p, diff != 0 and |diff| >= min_diff; linking, chains, min_loci, keep_edges and flags as in
        asm_regions.  Per chain also the largest phi and the fewest counting samples of each group among its rows.  The rows are
        staged and tested on the device; none comes to the host."""
        hi = self.n_loci if hi is None else hi
        n_ctx_rows, n_hits = C.c_int64(0), C.c_int64(0)
        rows = self._rows(self._L.hm_dmr_fetch_regions, GROUP_REGION_DTYPE, lo, hi, min_reps, ctx, max_p, min_diff, max_gap,
                          min_loci, int(bool(keep_edges)), C.byref(n_ctx_rows), C.byref(n_hits))
        return rows, int(n_ctx_rows.value), int(n_hits.value)

    def group_regions_bed(self, rows: np.ndarray) -> dict:
        """the text of <prefix>.groupdmr.{CpG,CHG,CHH}.bed: chrom, start, end, <ctx>_<k> (k from 1 in the order of rows), n_loci, .,
        +|-, diff, pmin, m1_min, pcov1, ncov1, m2_min, pcov2, ncov2, phi_max.  rows: every region of the job, per context in file
        order (sequence by sequence)."""
        sid, soff = locate(self.offsets, rows["start"])
        text = {k: [] for k in CTX_NAMES}
        for s, k, r in zip(sid, soff, rows):
            name = CTX_NAMES[int(r["motif"])]
            text[name].append("%s\t%d\t%d\t%s_%d\t%d\t.\t%s\t%g\t%.6g\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n" % (
                self.names[s], k, k + (r["end"] - r["start"]), name, len(text[name]) + 1, r["n_loci"], "+" if r["sign"] > 0 else "-",
                r["diff"], r["pmin"], r["m1_min"], r["pcov1"], r["ncov1"], r["m2_min"], r["pcov2"], r["ncov2"], r["phi_max"]))
        return {k: "".join(v) for k, v in text.items()}

    def open_sample(self) -> int:
        """`samplecorr` (hm_sample_open): opens the next sample; load_sample then writes its rows.  -> its index.  Needs
        samples=N and an engine that never saw a read, a load_loci or a begin_sample."""
        return self._check(self._L.hm_sample_open(self._h))

    def load_sample(self, gpos, pcov, ncov, motif) -> int:
        """`samplecorr` (hm_sample_load): rows of the open sample, as read_cov_bed returns them; any number of calls.  A
        locus stores floor(pcov 2^15 / (pcov + ncov)) + 1 if pcov + ncov >= sample_min_cov (its counts then also go to the combined
        planes), else 0xFFFF.  -> the number of rows that wrote a value.  HifimethError for a row outside the reference, a negative
        count, a count of 2^20 or more, a motif above 3 or a locus twice in this sample: the engine is then void."""
        return self._load(self._L.hm_sample_load, gpos, pcov, ncov, motif)

    def sample_plane(self, s: int, lo: int = 0, hi: Optional[int] = None) -> np.ndarray:
        """-> the stored uint16 values of sample s over [lo, hi): 0 nothing seen, level + 1, or 0xFFFF seen below sample_min_cov"""
        hi = self.n_loci if hi is None else hi
        out = np.zeros(max(hi - lo, 0), np.uint16)
        self._check(self._L.hm_sample_plane(self._h, s, lo, hi, out.ctypes.data_as(C.c_void_p)))
        return out

    def sample_sums(self, lo: int = 0, hi: Optional[int] = None, complete: bool = False) -> np.ndarray:
        """`samplecorr` (hm_sample_fetch_sums): per context and pair i <= j of the samples opened so far, context-major, the
        exact integer sums n, si, sj, sii, sjj, sij over the loci of [lo, hi) where both count -- complete: where all count
        (SAMPLE_PAIR_DTYPE).  Additive over adjacent ranges."""
        hi = self.n_loci if hi is None else hi
        out = np.zeros(3 * (SAMPLE_MAX * (SAMPLE_MAX + 1) // 2), SAMPLE_PAIR_DTYPE)
        n = self._check(self._L.hm_sample_fetch_sums(self._h, lo, hi, int(complete), out.ctypes.data_as(C.c_void_p)))
        return out[:n].copy()

    def sample_intervals(self, start, end, ctx: int, lo: int = 0, hi: Optional[int] = None, complete: bool = False) -> np.ndarray:
        """`regiondiff` (hm_sample_fetch_intervals): per interval [start[i], end[i]) -- GLOBAL locus coordinates, clamped to
        [lo, hi) -- and sample opened so far, the number of loci of context ctx at which the sample counts (complete: at which
        all count) and the sum of its levels there: uint64 (n_iv, M, 2), exact.  Additive over adjacent ranges."""
        hi = self.n_loci if hi is None else hi
        a, b = (np.ascontiguousarray(x, np.int64).reshape(-1) for x in (start, end))
        assert a.size == b.size
        out = np.zeros((a.size, SAMPLE_MAX, 2), np.uint64)
        n = self._check(self._L.hm_sample_fetch_intervals(self._h, lo, hi, ctx, int(complete), a.ctypes.data_as(C.c_void_p),
                                                          b.ctypes.data_as(C.c_void_p), a.size, out.ctypes.data_as(C.c_void_p)))
        m = n // a.size if a.size else 0
        return out.reshape(-1)[:2 * n].reshape(a.size, m, 2).copy()

    def bed(self, loci: np.ndarray) -> dict:
        """the text of <prefix>.{CpG,CHG,CHH}.cov.bed (pileup.cpp:562-590)"""
        sid, soff = locate(self.offsets, loci["gpos"])
        rows = {k: [] for k in CTX_NAMES}
        for s, k, p, n, m in zip(sid, soff, loci["pcov"], loci["ncov"], loci["motif"]):
            rows[CTX_NAMES[int(m)]].append("%s\t%d\t%d\t%g\t%d\t%d\n" % (self.names[s], k, k + 1, 100.0 * p / (p + n), p, n))
        return {k: "".join(v) for k, v in rows.items()}

    def asm(self, lo: int = 0, hi: Optional[int] = None, min_cov: int = 5, planes=None, plane_base: int = 0,
            table: Optional[AsmTable] = None) -> np.ndarray:
        """tested loci of [lo, hi) (plane coordinates) in ascending order: each haplotype with pcov + ncov >= min_cov.
        planes = (pcov1, ncov1, pcov2, ncov2, key) torch tensors whose element 0 is locus plane_base, or None (own; needs
        partitions=True).  diff = 100 p1 / (p1 + n1) - 100 p2 / (p2 + n2), pvalue = two-sided Fisher exact test (R's rule).
        table (asm_qvalues, solved for the same min_cov): the rows also carry its qvalue (ASMQ_DTYPE), NaN where it has none."""
        hi = self.n_loci if hi is None else hi
        ptrs = [None] * 5 if planes is None else [C.c_void_p(t.data_ptr()) for t in planes]
        if table is None:
            return self._rows(self._L.hm_pileup_fetch_asm, ASM_DTYPE, *ptrs, plane_base, lo, hi, min_cov)
        return self._rows(self._L.hm_pileup_fetch_asm_q, ASMQ_DTYPE, *ptrs, plane_base, lo, hi, min_cov,
                          table.tab.ctypes.data_as(C.c_void_p), len(table.tab), table.big.ctypes.data_as(C.c_void_p),
                          table.big_q.ctypes.data_as(C.c_void_p), len(table.big))

    def asm_histogram(self, lo: int = 0, hi: Optional[int] = None, min_cov: int = 5, planes=None, plane_base: int = 0,
                      bins: Optional[np.ndarray] = None):
        """-> (bins, big): bins (uint64 [ASM_BINS]; added into `bins` when given) = tested loci of [lo, hi) per dense tuple, index
        (motif * 2080 + pair(pcov1, ncov1)) * 2080 + pair(pcov2, ncov2), pair(p, n) = t (t + 1) / 2 + p, t = p + n < 64; big = the
        tested loci with a haplotype total >= 64, ascending, as asm() rows (ASM_DTYPE)"""
        hi = self.n_loci if hi is None else hi
        bins = np.zeros(ASM_BINS, np.uint64) if bins is None else bins
        if not (isinstance(bins, np.ndarray) and bins.dtype == np.uint64 and bins.size == ASM_BINS and bins.flags.c_contiguous
                and bins.flags.writeable):
            raise HifimethError("asm_histogram: bins must be a contiguous uint64 array of 3 x 2080 x 2080")
        ptrs = [None] * 5 if planes is None else [C.c_void_p(t.data_ptr()) for t in planes]
        pb = bins.ctypes.data_as(C.c_void_p)
        big = np.zeros(4096, ASM_DTYPE)           # big loci are rare at HiFi coverage: room for them in the first call
        n = self._check(self._L.hm_pileup_asm_histogram(self._h, *ptrs, plane_base, lo, hi, min_cov, pb, big.ctypes.data_as(C.c_void_p), len(big)))
        if n > len(big):                          # nothing was written or added: again, with room for the list
            big = np.zeros(n, ASM_DTYPE)
            self._check(self._L.hm_pileup_asm_histogram(self._h, *ptrs, plane_base, lo, hi, min_cov, pb, big.ctypes.data_as(C.c_void_p), n))
        return bins, big[:n].copy()

    def asm_bin_pvalues(self, bins: np.ndarray) -> np.ndarray:
        """the non-empty bins of the job-wide `bins`, ascending (ASM_BIN_DTYPE): count, and the pvalue the device computes for a
        row carrying the bin's tuple; qvalue NaN until asm_qvalues"""
        b = np.ascontiguousarray(bins, np.uint64).reshape(-1)
        if b.size != ASM_BINS:
            raise HifimethError("asm_bin_pvalues: 3 x 2080 x 2080 bins expected")
        tab = np.zeros(int(np.count_nonzero(b)), ASM_BIN_DTYPE)   # their number is known here: one upload, one compaction
        n = self._check(self._L.hm_pileup_asm_bin_pvalues(self._h, b.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p), len(tab)))
        if n != len(tab):
            raise HifimethError("asm_bin_pvalues: the engine found %d non-empty bins, the host %d" % (n, len(tab)))
        return tab

    def asm_bed(self, rows: np.ndarray) -> dict:
        """the text of <prefix>.asm.{CpG,CHG,CHH}.bed: chrom, k, k+1, diff, pvalue, pcov1, ncov1, pcov2, ncov2; rows with a qvalue
        (ASMQ_DTYPE) print it as a tenth column"""
        sid, soff = locate(self.offsets, rows["gpos"])
        text = {k: [] for k in CTX_NAMES}
        with_q = "qvalue" in rows.dtype.names
        for s, k, r in zip(sid, soff, rows):
            text[CTX_NAMES[int(r["motif"])]].append("%s\t%d\t%d\t%g\t%.6g\t%d\t%d\t%d\t%d" % (
                self.names[s], k, k + 1, r["diff"], r["pvalue"], r["pcov1"], r["ncov1"], r["pcov2"], r["ncov2"])
                + ("\t%.6g\n" % r["qvalue"] if with_q else "\n"))
        return {k: "".join(v) for k, v in text.items()}

    def asm_regions(self, ctx: int, lo: int = 0, hi: Optional[int] = None, min_cov: int = 5, max_p: float = 0.01, max_gap: int = 500,
                    min_loci: int = 3, planes=None, plane_base: int = 0, keep_edges: bool = False) -> Tuple[np.ndarray, int]:
        """-> (rows, n_ctx_rows): the chains of context ctx (0 CpG, 1 CHG, 2 CHH) among the asm() rows of [lo, hi), ascending
        (ASM_REGION_DTYPE), and the number of those rows.  A row is a hit when pvalue <= max_p and diff != 0; consecutive rows of
        the context are linked when both are hits of one sign at most max_gap apart; a chain is a maximal run of linked hits, so a
        tested row that is no hit breaks it.  Returned: the chains of at least min_loci loci and, with keep_edges, every chain
        that holds the first or the last row (flags REGION_FIRST / REGION_LAST), for stitch_asm_regions.  `sign` is the loci's;
        `diff`, on the pooled counts, can disagree with it.  planes as for asm()."""
        hi = self.n_loci if hi is None else hi
        ptrs = [None] * 5 if planes is None else [C.c_void_p(t.data_ptr()) for t in planes]
        n_ctx_rows = C.c_int64(0)
        rows = self._rows(self._L.hm_pileup_fetch_asm_regions, ASM_REGION_DTYPE, *ptrs, plane_base, lo, hi, min_cov, ctx, max_p,
                          max_gap, min_loci, int(bool(keep_edges)), C.byref(n_ctx_rows))
        return rows, int(n_ctx_rows.value)

    def asm_regions_bed(self, rows: np.ndarray) -> dict:
        """the text of <prefix>.asm.regions.{CpG,CHG,CHH}.bed: chrom, start, end, n_loci, +|-, diff, pmin, pcov1, ncov1, pcov2, ncov2"""
        sid, soff = locate(self.offsets, rows["start"])
        text = {k: [] for k in CTX_NAMES}
        for s, k, r in zip(sid, soff, rows):
            text[CTX_NAMES[int(r["motif"])]].append("%s\t%d\t%d\t%d\t%s\t%g\t%.6g\t%d\t%d\t%d\t%d\n" % (
                self.names[s], k, k + (r["end"] - r["start"]), r["n_loci"], "+" if r["sign"] > 0 else "-", r["diff"], r["pmin"],
                r["pcov1"], r["ncov1"], r["pcov2"], r["ncov2"]))
        return {k: "".join(v) for k, v in text.items()}

    def _plane_ptrs(self, planes):
        return [None, None, None] if planes is None else [C.c_void_p(t.data_ptr()) for t in planes]

    def control_sums(self, lo: int, hi: int, planes=None) -> np.ndarray:
        """(P_cpg, P_chg, P_chh, N_cpg, N_chg, N_chh): pcov and ncov summed per context over the covered loci of [lo, hi) (plane
        coordinates) -- the control sequence's range, or a rank's part of it"""
        s = np.zeros(6, np.uint64)
        self._check(self._L.hm_pileup_control_sums(self._h, *self._plane_ptrs(planes), lo, hi, s.ctypes.data_as(C.c_void_p)))
        return s

    def site_histogram(self, lo: int = 0, hi: Optional[int] = None, planes=None, plane_base: int = 0, bins: Optional[np.ndarray] = None):
        """-> (bins, big): bins[motif, n, k] (uint64 [3, 256, 256]; added into `bins` when given) = covered loci of [lo, hi) with
        pcov = k, pcov + ncov = n < 256; big = the loci with n >= 256, ascending (LOCUS_DTYPE)"""
        hi = self.n_loci if hi is None else hi
        bins = np.zeros((3, 256, 256), np.uint64) if bins is None else bins
        assert bins.dtype == np.uint64 and bins.size == SITE_BINS and bins.flags.c_contiguous
        ptrs, pb = self._plane_ptrs(planes), bins.ctypes.data_as(C.c_void_p)
        big = np.zeros(0, LOCUS_DTYPE)
        n = self._check(self._L.hm_pileup_site_histogram(self._h, *ptrs, plane_base, lo, hi, pb, None, 0))
        if n:                                     # nothing was added: again, with room for the list
            big = np.zeros(n, LOCUS_DTYPE)
            self._check(self._L.hm_pileup_site_histogram(self._h, *ptrs, plane_base, lo, hi, pb, big.ctypes.data_as(C.c_void_p), n))
        return bins, big

    def sites(self, table: SitesTable, lo: int = 0, hi: Optional[int] = None, planes=None, plane_base: int = 0) -> np.ndarray:
        """rows of [lo, hi) (plane coordinates), ascending: the covered loci of the contexts `table` tests, pvalue / qvalue looked
        up in it on the device"""
        hi = self.n_loci if hi is None else hi
        return self._rows(self._L.hm_pileup_fetch_sites, SITE_DTYPE, *self._plane_ptrs(planes), plane_base, lo, hi, table.ctx_mask,
                          *(x.ctypes.data_as(C.c_void_p) for x in (table.ptab, table.qtab, table.big, table.big_p, table.big_q)), len(table.big))

    def sites_bed(self, rows: np.ndarray) -> dict:
        """the text of <prefix>.sites.{CpG,CHG,CHH}.bed: the six columns of the cov.bed row, then pvalue and qvalue"""
        sid, soff = locate(self.offsets, rows["gpos"])
        text = {k: [] for k in CTX_NAMES}
        for s, k, r in zip(sid, soff, rows):
            p, n = int(r["pcov"]), int(r["ncov"])
            text[CTX_NAMES[int(r["motif"])]].append("%s\t%d\t%d\t%g\t%d\t%d\t%.6g\t%.6g\n" % (
                self.names[s], k, k + 1, 100.0 * p / (p + n), p, n, r["pvalue"], r["qvalue"]))
        return {k: "".join(v) for k, v in text.items()}

    def num_pattern_records(self) -> int:
        return int(self._L.hm_pileup_num_pattern_records(self._h))

    def patterns(self, lo: int = 0, hi: Optional[int] = None, min_reads: int = PATTERN_MIN_READS) -> np.ndarray:
        """the windows whose first reference CpG lies in [lo, hi), ascending (PATTERN_DTYPE), with at least min_reads reads that
        carry a call at all k loci: counts[pattern], bit i of the pattern = the read's call at the i-th locus reaches the CpG
        threshold count() was given.  Needs patterns=k, after count()."""
        hi = self.n_loci if hi is None else hi
        return self._rows(self._L.hm_pileup_fetch_patterns, PATTERN_DTYPE, lo, hi, min_reads)

    def patterns_bed(self, rows: np.ndarray) -> str:
        """the text of <prefix>.patterns.CpG.bed: chrom, start, end, n, entropy, epipolymorphism, pdr, level, the 2^k counts joined
        by commas"""
        sid, soff = locate(self.offsets, rows["start"])
        text = []
        for s, k, r in zip(sid, soff, rows):
            text.append("%s\t%d\t%d\t%d\t%.6g\t%.6g\t%.6g\t%.6g\t" % (self.names[s], k, k + (r["end"] - r["start"]), r["n"], *pattern_stats(r))
                        + ",".join("%d" % c for c in r["counts"][:1 << int(r["k"])]) + "\n")
        return "".join(text)

    def linkage(self, min_pairs: int = 1) -> np.ndarray:
        """the distances d in [2, max_dist] with at least min_pairs pairs, ascending (LINKAGE_DTYPE; min_pairs 0: every distance):
        the pairs of CpG calls of one record d bases apart by class, M = the call reaches the CpG threshold the last count() was
        given, the first letter for the lower coordinate.  Needs linkage=max_dist, after count()."""
        return self._rows(self._L.hm_pileup_fetch_linkage, LINKAGE_DTYPE, min_pairs)

    def linkage_tsv(self, rows: np.ndarray) -> str:
        """the text of <prefix>.linkage.CpG.tsv"""
        return linkage_tsv(rows)

    def readpos(self, min_calls: int = 1) -> np.ndarray:
        """the rows of the read-position table with at least min_calls calls (READPOS_DTYPE; min_calls 0: all 3 x (2 D + 1)): by
        context, then 5' by ascending distance, 3' by ascending distance, interior; methylated = the ML byte reaches the context's
        threshold of the last count().  Needs profile=D, after count()."""
        return self._rows(self._L.hm_pileup_fetch_readpos, READPOS_DTYPE, min_calls)

    def readpos_histograms(self) -> np.ndarray:
        """the table itself, uint64 [3, 2 D + 1, 256]: context, bin (5' 0 .. D - 1, 3' 0 .. D - 1, interior), ML byte"""
        h = np.zeros((3, 2 * self.profile + 1, 256), np.uint64)
        self._check(self._L.hm_pileup_readpos_histograms(self._h, h.ctypes.data_as(C.c_void_p), h.size))
        return h

    def add_readpos(self, hist: np.ndarray):
        """add another engine's readpos_histograms() to this one's table (the multi-rank path)"""
        h = np.ascontiguousarray(hist, np.uint64)
        self._check(self._L.hm_pileup_add_readpos(self._h, h.ctypes.data_as(C.c_void_p), h.size))

    def _range_ptrs(self, planes, partition: int):
        """(pcov, ncov, key) of a call over a plane range: the caller's tensors, a partition's counts with the combined key, or own"""
        if planes is not None or not partition:
            return self._plane_ptrs(planes)
        pc, nc = C.c_void_p(), C.c_void_p()
        self._check(self._L.hm_pileup_partition_planes(self._h, partition, C.byref(pc), C.byref(nc)))
        return [pc, nc, None]

    def regions(self, start, end, min_cov: int = 1, lo: int = 0, hi: Optional[int] = None, planes=None, plane_base: int = 0,
                partition: int = 0) -> np.ndarray:
        """the sums of the intervals [start[i], end[i]) -- GLOBAL locus coordinates, Regions.coords(pu.offsets) -- per context over
        the loci with pcov + ncov >= min_cov: REGION_SUM_DTYPE [n, 3].  [lo, hi) (plane coordinates), planes, plane_base and
        partition as for loci(); every interval is clamped to the range, so the results of disjoint ranges add up."""
        hi = self.n_loci if hi is None else hi
        a, b = (np.ascontiguousarray(x, np.int64).reshape(-1) for x in (start, end))
        assert a.size == b.size
        out = np.zeros((a.size, 3), REGION_SUM_DTYPE)
        self._check(self._L.hm_pileup_fetch_regions(self._h, *self._range_ptrs(planes, partition), plane_base, lo, hi, min_cov,
                                                    a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), a.size,
                                                    out.ctypes.data_as(C.c_void_p)))
        return out

    def metaplot(self, start, end, seq_start, seq_end, strand=None, bins: int = 20, flank: int = 0, flank_bins: int = 0,
                 min_cov: int = 1, lo: int = 0, hi: Optional[int] = None, planes=None, plane_base: int = 0, partition: int = 0):
        """-> (rows, n_used): METABIN_DTYPE rows [3 x (bins + 2 flank_bins)], context-major: every interval of at least `bins`
        bases cut into `bins` body bins and, with flank > 0, flank_bins bins of flank / flank_bins bases on either side (clamped
        to the interval's sequence [seq_start, seq_end)), numbered from upstream for strand + or . and mirrored for -, and summed
        over the n_used intervals.  Coordinates, range and planes as for regions(); strand = bytes of +, - or . per interval."""
        hi = self.n_loci if hi is None else hi
        a, b, s0, s1 = (np.ascontiguousarray(x, np.int64).reshape(-1) for x in (start, end, seq_start, seq_end))
        assert a.size == b.size == s0.size == s1.size and (strand is None or len(strand) == a.size)
        out = np.zeros(3 * (bins + 2 * flank_bins) if bins > 0 and flank_bins >= 0 else 0, METABIN_DTYPE)
        n_used = C.c_int64(0)
        self._check(self._L.hm_pileup_fetch_metaplot(
            self._h, *self._range_ptrs(planes, partition), plane_base, lo, hi, min_cov, *(x.ctypes.data_as(C.c_void_p) for x in (a, b, s0, s1)),
            bytes(strand) if strand is not None else None, a.size, bins, flank, flank_bins,
            out.ctypes.data_as(C.c_void_p), C.byref(n_used)))
        return out, int(n_used.value)

    def context(self, flank: int = 0, min_cov: int = 1, lo: int = 0, hi: Optional[int] = None, planes=None, plane_base: int = 0,
                partition: int = 0, path: int = CONTEXT_PATH_AUTO) -> np.ndarray:
        """methylation by the k = 3 + 2 flank bases around each cytosine (`pileup -S`): int64 [3, 4^k + 1, 4] -- context, row
        (the k-mer's code, context_kmer(); the last row `other`), (n_loci, pcov, ncov, ppm) -- over the loci of [lo, hi) with
        pcov + ncov >= min_cov.  Range, planes, plane_base and partition as for loci(); the tables of disjoint ranges add up.
        path: the accumulation path (CONTEXT_PATH_LDS / _GLOBAL), for measurements and tests; both give the same table."""
        hi = self.n_loci if hi is None else hi
        ptrs = self._range_ptrs(planes, partition)
        if ptrs[0] is not None and ptrs[2] is None:         # a partition's counts: the combined key is named, not implied
            key = C.c_void_p()
            self._check(self._L.hm_pileup_planes(self._h, None, None, C.byref(key), None))
            ptrs[2] = key
        args = (self._h, *ptrs, plane_base, lo, hi, min_cov, flank)
        if path == CONTEXT_PATH_AUTO:
            out = self._rows(lambda *a: self._L.hm_pileup_fetch_context(*args, *a[1:]), REGION_SUM_DTYPE)
        else:
            out = self._rows(lambda *a: self._L.hm_pileup_fetch_context_path(*args, path, *a[1:]), REGION_SUM_DTYPE)
        return np.stack([out[k] for k in REGION_SUM_DTYPE.names], axis=-1).reshape(3, -1, 4)

    def fetch_smooth(self, ctx: int, lo: int = 0, hi: Optional[int] = None, half_width: int = 500, min_cov: int = 1, min_loci: int = 1,
                     partition: int = 0) -> np.ndarray:
        """`smooth` (hm_smooth_fetch): the counting loci of context ctx in [lo, hi), ascending (SMOOTH_DTYPE) -- key motif ctx,
        pcov + ncov >= min_cov -- each with the loci of its window and the sums of their pcov and ncov under the triangular kernel of
        half-width half_width in [1, 16384], cut at its sequence; rows with fewer than min_loci loci in the window are left out.
        partition 1 / 2: that partition's counts.  After count() or load_loci()."""
        hi = self.n_loci if hi is None else hi
        return self._rows(self._L.hm_smooth_fetch, SMOOTH_DTYPE, partition, ctx, lo, hi, half_width, min_cov, min_loci)

    def bedmethyl(self, lo: int = 0, hi: Optional[int] = None, min_valid: int = 1, partition: int = 0) -> np.ndarray:
        """the reference CpGs of [lo, hi), ascending (BEDMETHYL_DTYPE), at which a read was classed and n_mod + n_canon >= min_valid
        (0: also those seen only as nocall, diff or delete).  partition 1 / 2: the reads of that haplotype.  Needs bedmethyl=True,
        after count()."""
        hi = self.n_loci if hi is None else hi
        return self._rows(self._L.hm_pileup_fetch_bedmethyl, BEDMETHYL_DTYPE, partition, lo, hi, min_valid)

    def bedmethyl_bed(self, rows: np.ndarray) -> str:
        """the text of <prefix>.bedmethyl.CpG.bed, modkit's 18 columns: chrom, start, end, m, min(1000, Nvalid), ., start, end,
        255,0,0, Nvalid, percent modified, Nmod, Ncanonical, Nother_mod = 0, Ndelete, Nfail = 0, Ndiff, Nnocall"""
        sid, soff = locate(self.offsets, rows["gpos"])
        text = []
        for s, k, r in zip(sid, soff, rows):
            nm, nc = int(r["n_mod"]), int(r["n_canon"])
            nv = nm + nc
            text.append("%s\t%d\t%d\tm\t%d\t.\t%d\t%d\t255,0,0\t%d\t%.2f\t%d\t%d\t0\t%d\t0\t%d\t%d\n" % (
                self.names[s], k, k + 1, min(1000, nv), k, k + 1, nv, 100.0 * nm / nv if nv else 0.0, nm, nc, r["n_delete"], r["n_diff"],
                r["n_nocall"]))
        return "".join(text)

    def domains(self, ctx: int, lo: int = 0, hi: Optional[int] = None, A: Optional[int] = None, B: Optional[int] = None,
                S: Optional[int] = None, max_gap: int = DOMAIN_MAX_GAP, planes=None, plane_base: int = 0) -> Tuple[np.ndarray, int]:
        """-> (rows, n_ctx_rows): the segments of context ctx (0 CpG, 1 CHG, 2 CHH) over [lo, hi), ascending (DOMAIN_DTYPE), and
        the number of loci they partition -- those with pcov, ncov >= 0 and pcov + ncov > 0 in that context.  A locus with k
        methylated and u unmethylated reads (each clamped to 2^20 - 1) scores k * A + u * B in the high state; a change of state
        between loci at most max_gap apart costs S, beyond that nothing (a break); the path of the largest total is found exactly
        (hm_pileup_fetch_domains has the tie rule) and a segment is a maximal run of one state without a break.  A, B, S default to
        domain_scores() of DOMAIN_LEVELS[ctx] and DOMAIN_PENALTY.  planes as for loci()."""
        hi = self.n_loci if hi is None else hi
        if A is None or B is None or S is None:
            A, B, S = domain_scores(*DOMAIN_LEVELS[ctx])
        n_ctx_rows = C.c_int64(0)
        rows = self._rows(self._L.hm_pileup_fetch_domains, DOMAIN_DTYPE, *self._plane_ptrs(planes), plane_base, lo, hi, ctx, A, B, S,
                          max_gap, C.byref(n_ctx_rows))
        return rows, int(n_ctx_rows.value)

    def domains_part(self, ctx: int, lo: int, hi: int, pass_: int, carry: Optional[dict] = None, A: Optional[int] = None,
                     B: Optional[int] = None, S: Optional[int] = None, max_gap: int = DOMAIN_MAX_GAP, planes=None,
                     plane_base: int = 0) -> dict:
        """one pass of hm_pileup_fetch_domains_part over the piece [lo, hi) of context ctx -> its results as Python ints.
        pass_ DOMAIN_PASS_SUMMARY: n_rows, first_gpos, last_gpos, e_first, c, lo, hi.  DOMAIN_PASS_CODES, carry = {has_prev,
        prev_gpos, prev_d}: also d_last and back.  DOMAIN_PASS_SEGMENTS, carry = that and {has_next, next_gpos, last_state}: also
        d_last and "segments" (DOMAIN_DTYPE).  A piece without rows gives n_rows = 0 and nothing else.  The carries are those of
        domain_forward_carries / domain_backward_carries; chain_domain_parts runs all of it."""
        if A is None or B is None or S is None:
            A, B, S = domain_scores(*DOMAIN_LEVELS[ctx])
        part = _DomainPart(**{k: int(v) for k, v in (carry or {}).items()})
        args = (*self._plane_ptrs(planes), plane_base, lo, hi, ctx, A, B, S, max_gap, pass_, C.byref(part))
        rows = np.zeros(64, DOMAIN_DTYPE)                     # most pieces fit; a pass is repeated only for one that does not
        n = self._check(self._L.hm_pileup_fetch_domains_part(self._h, *args, rows.ctypes.data_as(C.c_void_p), len(rows)))
        if pass_ == DOMAIN_PASS_SEGMENTS and n > len(rows):
            rows = np.zeros(n, DOMAIN_DTYPE)
            self._check(self._L.hm_pileup_fetch_domains_part(self._h, *args, rows.ctypes.data_as(C.c_void_p), n))
        out = {"n_rows": int(part.n_rows)}
        if out["n_rows"]:
            names = ("first_gpos", "last_gpos", "e_first") + (("c", "lo", "hi") if pass_ == DOMAIN_PASS_SUMMARY else ("d_last",)) \
                + (("back",) if pass_ == DOMAIN_PASS_CODES else ())
            out.update((k, int(getattr(part, k))) for k in names)
        if pass_ == DOMAIN_PASS_SEGMENTS:
            out["segments"] = rows[:n].copy()
        return out

    def domains_bed(self, rows: np.ndarray) -> dict:
        """domains_bed() with this reference's names"""
        return domains_bed(rows, self.names, self.offsets)

    def domain_sums(self, ctx: int, lo: int = 0, hi: Optional[int] = None, A: Optional[int] = None, B: Optional[int] = None,
                    S: Optional[int] = None, max_gap: int = DOMAIN_MAX_GAP, planes=None, plane_base: int = 0,
                    carry: Optional[dict] = None) -> Tuple[int, ...]:
        """-> (P0, N0, R0, P1, N1, R1): pcov, ncov and the number of loci of context ctx over [lo, hi), by the state domains()
        gives each locus (0 low, 1 high) -- summed on the device without building a segment (hm_pileup_domain_sums).  With
        `carry` [lo, hi) is a PIECE and the states are those the chain gives it: the carry of domains_part's segments pass
        (hm_pileup_domain_sums_part).  Arguments as for domains()."""
        hi = self.n_loci if hi is None else hi
        if A is None or B is None or S is None:
            A, B, S = domain_scores(*DOMAIN_LEVELS[ctx])
        sums = (C.c_int64 * 6)()
        args = (*self._plane_ptrs(planes), plane_base, lo, hi, ctx, A, B, S, max_gap)
        if carry is None:
            self._check(self._L.hm_pileup_domain_sums(self._h, *args, sums))
        else:
            part = _DomainPart(**{k: int(v) for k, v in carry.items()})
            self._check(self._L.hm_pileup_domain_sums_part(self._h, *args, C.byref(part), sums))
        return tuple(int(x) for x in sums)

    def fit_domain_levels(self, ctx: int, lo: float, hi: float, penalty: float = DOMAIN_PENALTY, max_gap: int = DOMAIN_MAX_GAP,
                          max_iter: int = 20, planes=None, plane_base: int = 0):
        """-> (lo, hi, status, history): the two levels of context ctx fitted to the planes from the start (lo, hi), by hard EM
        over the sequences of the reference: domain_sums per sequence under the current levels, the levels refitted from the
        sums (DomainFit has the stop rule).  The planes span the whole reference."""
        def sums_of(A, B, S):
            per_seq = [self.domain_sums(ctx, int(a) - plane_base, int(b) - plane_base, A, B, S, max_gap, planes, plane_base)
                       for a, b in zip(self.offsets[:-1], self.offsets[1:])]
            return [sum(col) for col in zip(*per_seq)] if per_seq else [0] * 6
        return fit_levels(sums_of, lo, hi, penalty, max_iter)


# ---- multi-GPU exchange: histograms all-reduced, per-locus planes reduce-scattered ------------
def locus_ranges(n_loci: int, world: int) -> List[Tuple[int, int]]:
    """contiguous, equal-size (padded) ranges: rank r owns [r*chunk, min(n_loci, (r+1)*chunk))"""
    chunk = (n_loci + world - 1) // world
    return [(min(n_loci, r * chunk), min(n_loci, (r + 1) * chunk)) for r in range(world)]


def allreduce_histograms(dist, bins: np.ndarray, device: str = "cpu") -> np.ndarray:
    import torch
    t = torch.from_numpy(bins.astype(np.int64).reshape(-1)).to(device)
    if dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return t.cpu().numpy().astype(np.uint64).reshape(3, 256)


def reduce_scatter_sum(dist, planes, force: bool = False):
    """the SUM half of reduce_scatter_planes for further count planes (the haplotype partitions' pcov / ncov) -> (slices,
    base); same layout and the same RCCL / gloo split"""
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    if world == 1 and not (force and dist.is_initialized()):
        return list(planes), 0
    import torch
    outs = []
    for t in planes:
        assert t.numel() % world == 0
        chunk = t.numel() // world
        if t.is_cuda:
            o = torch.empty(chunk, dtype=t.dtype, device=t.device)
            dist.reduce_scatter_tensor(o, t, op=dist.ReduceOp.SUM)
        else:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            o = t[rank * chunk:(rank + 1) * chunk].clone()
        outs.append(o)
    return outs, rank * (planes[0].numel() // world)


def reduce_scatter_planes(dist, pcov, ncov, key, force: bool = False):
    """-> (pcov, ncov, key, base): this rank's slice of the job-wide planes, `base` = its first locus.
    pcov / ncov are summed, key (order << 2 | motif; hm_pileup_submit_read keeps order < 2^29, so the key is < 2^31 and
    compares as int32 exactly like the device's uint32 atomicMax) takes the maximum.
    Planes must be padded to world * chunk elements.  RCCL reduce-scatters; gloo (CPU tests) all-reduces and slices."""
    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    n = pcov.numel()
    assert n % world == 0
    chunk = n // world
    if world == 1 and not (force and dist.is_initialized()):
        return pcov, ncov, key, 0
    import torch
    outs = []
    for t, op in ((pcov, dist.ReduceOp.SUM), (ncov, dist.ReduceOp.SUM), (key, dist.ReduceOp.MAX)):
        if t.is_cuda:
            o = torch.empty(chunk, dtype=t.dtype, device=t.device)
            dist.reduce_scatter_tensor(o, t, op=op)
        else:
            dist.all_reduce(t, op=op)
            o = t[rank * chunk:(rank + 1) * chunk].clone()
        outs.append(o)
    return outs[0], outs[1], outs[2], rank * chunk
