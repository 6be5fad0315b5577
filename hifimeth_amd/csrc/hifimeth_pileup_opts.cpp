// hifimeth_pileup_opts.cpp -- the options of `pileup`, `diff`, `groupdiff`, `samplecorr`, `regiondiff`, `groupdmr` and `smooth`: one table that is parser and usage text at once, two strict number
// parsers, and the checks between options as one ordered list.  A new option is one row here, a field of PileupOptions, a rule if
// it depends on another option, and its cases in tools/make_cli_options.py.
#include "hifimeth_pileup_opts.h"

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "hm_bam.h"

bool whole_int(const char* text, long long lo, long long hi, long long& out) {
    char* end = nullptr;
    errno = 0;
    const long long x = strtoll(text, &end, 10);
    if (end == text || *end || errno || x < lo || x > hi) return false;
    out = x;
    return true;
}

bool whole_double(const char* text, double& out) {
    char* end = nullptr;
    errno = 0;
    const double x = strtod(text, &end);
    if (end == text || *end || errno) return false;
    out = x;
    return true;
}

namespace {

// the three shapes most rows' parse actions have: a flag, an atoi field, a strict integer in [LO, HI] (int or long long field)
using O = PileupOptions;
template <bool O::*Field>
bool flag(const char*, O& o) { return o.*Field = true; }
template <int O::*Field>
bool lenient(const char* v, O& o) { o.*Field = atoi(v); return true; }
template <auto Field, long long LO, long long HI>
bool integer(const char* v, O& o) {
    long long x = 0;
    if (!whole_int(v, LO, HI, x)) return false;
    o.*Field = x;
    return true;
}

// the argument of -e: three comma-separated fields, each `nan` or a plain decimal in [0, 1]
bool parse_rates(const char* text, double rates[3]) {
    const char* p = text;
    for (int c = 0; c < 3; ++c) {
        const char* e = strchr(p, c < 2 ? ',' : '\0');
        if (!e || e == p) return false;
        const std::string t(p, e);
        if (t == "nan") rates[c] = std::nan("");
        else {
            if (t.find_first_not_of("0123456789.eE+-") != std::string::npos || !(isdigit((unsigned char)t[0]) || t[0] == '.')) return false;
            char* end = nullptr;
            rates[c] = strtod(t.c_str(), &end);
            if (end != t.c_str() + t.size() || !(rates[c] >= 0.0 && rates[c] <= 1.0)) return false;
        }
        p = e + 1;
    }
    return true;
}

// -J: bins[:flank_bp:flank_bins]; false unless the whole text parses and lies in the ranges hm_pileup_fetch_metaplot takes
bool parse_metaplot(const char* text, int& bins, long long& flank, int& flank_bins) {
    long long v[3] = {0, 0, 0};
    int n = 0;
    for (const char* c = text;; ++n) {
        char* end = nullptr;
        errno = 0;
        if (n == 3 || !isdigit((unsigned char)*c)) return false;
        v[n] = strtoll(c, &end, 10);
        if (errno) return false;
        if (!*end) break;
        if (*end != ':') return false;
        c = end + 1;
    }
    if (n != 0 && n != 2) return false;
    if (v[0] < 1 || v[0] > 1000 || v[2] > 1000 || (v[1] == 0) != (v[2] == 0) || (v[2] && v[1] % v[2])) return false;
    bins = (int)v[0];
    flank = v[1];
    flank_bins = (int)v[2];
    return true;
}

// -I: n5[:n3], integers >= 0, one number for both ends; false unless the whole text parses
bool parse_trim(const char* text, long long& n5, long long& n3) {
    char* end = nullptr;
    errno = 0;
    if (!isdigit((unsigned char)*text)) return false;
    n5 = n3 = strtoll(text, &end, 10);
    if (errno || n5 > INT_MAX) return false;
    if (!*end) return true;
    if (*end != ':' || !isdigit((unsigned char)end[1])) return false;
    const char* second = end + 1;
    n3 = strtoll(second, &end, 10);
    return !errno && !*end && n3 <= INT_MAX;
}

// -u: one lo:hi pair for all contexts or three, each pair possibly nan; false unless the whole text parses
bool parse_levels(const char* text, double lo[3], double hi[3]) {
    std::vector<std::string> items(1);
    for (const char* p = text; *p; ++p) {
        if (*p == ',') items.emplace_back();
        else items.back() += *p;
    }
    if (items.size() != 1 && items.size() != 3) return false;
    for (int c = 0; c < 3; ++c) {
        const std::string& t = items[items.size() == 1 ? 0 : (size_t)c];
        if (t == "nan") { lo[c] = hi[c] = std::nan(""); continue; }
        const size_t colon = t.find(':');
        if (colon == std::string::npos || t.find_first_not_of("0123456789.eE+-:") != std::string::npos) return false;
        const std::string a = t.substr(0, colon), b = t.substr(colon + 1);
        char *ea = nullptr, *eb = nullptr;
        lo[c] = strtod(a.c_str(), &ea);
        hi[c] = strtod(b.c_str(), &eb);
        if (a.empty() || b.empty() || *ea || *eb) return false;
    }
    return true;
}

// One row per flag, in the order `pileup -h` lists them.  `help` is the text under "  -x <metavar>", with $0 for the program; a
// flag without a metavar takes no value.  `diff` carries the flags of DIFF_FLAGS, in that order, under `diff_help` where its
// wording differs.  `parse` writes the option's field and returns false for a value it does not take; that is reported by the
// rules below, or at once with `fatal` where the row has one.
struct Option {
    char letter;
    const char* metavar;
    bool (*parse)(const char* v, PileupOptions& o);
    const char* help;
    const char* diff_help;  // nullptr: as help
    const char* fatal;
};

const Option OPTIONS[] = {
    {'q', "<mapQ>", lenient<&O::min_mapq>, "Minimum mapping quality score\n    Default: 0"},
    {'f', "<Alignment identity>", [](const char* v, O& o) { o.min_pi = atof(v); return true; }, "Default: 0"},
    {'t', "<CPU threads>", [](const char* v, O& o) { o.threads = std::max(1, atoi(v)); return true; }, "Number of CPU threads\n    Default: 8"},
    {'d', "<int>", lenient<&O::device>, "GPU ordinal\n    Default: 0"},
    {'b', "<int>", [](const char* v, O& o) { o.read_batch = std::max(1, atoi(v)); return true; }, "BAM records per GPU batch\n    Default: 512"},
    {'H', nullptr, flag<&O::haplotypes>,
     "Haplotype-resolved output: records tagged HP:i:1 / HP:i:2 are also counted into\n"
     "    <prefix>.hap1.<ctx>.cov.bed / <prefix>.hap2.<ctx>.cov.bed (same thresholds as the combined files)"},
    {'A', nullptr, flag<&O::asm_test>,
     "With -H: test every locus where both haplotypes are covered for a difference between them and write\n"
     "    <prefix>.asm.<ctx>.bed: chrom, start, end, hap1 % - hap2 %, two-sided Fisher exact p-value, pcov1, ncov1, pcov2, ncov2"},
    {'a', "<int>", lenient<&O::asm_min_cov>,
     "With -A: minimum coverage (pcov + ncov) of each haplotype at a tested locus\n    Default: 5",
     "Minimum coverage (pcov + ncov) of each sample at a tested locus\n    Default: 5"},
    {'Q', nullptr, flag<&O::asm_q>,
     "With -A: a tenth column, the Benjamini-Hochberg q-value of the p-value among all tested loci of the context, and\n"
     "    <prefix>.asm.summary.tsv: ctx, tested loci, loci with q <= 0.05, loci with q <= 0.01",
     "A tenth column, the Benjamini-Hochberg q-value of the p-value among all tested loci of the context, and\n"
     "    <output-prefix>.diff.summary.tsv: ctx, tested loci, loci with q <= 0.05, loci with q <= 0.01"},
    {'G', nullptr, flag<&O::asm_regions>,
     "With -A: chain the tested loci of each context into regions and write <prefix>.asm.regions.<ctx>.bed: chrom, start, end,\n"
     "    loci, + or - (the sign of hap1 % - hap2 % at every locus), hap1 % - hap2 % of the pooled counts, smallest p-value,\n"
     "    pcov1, ncov1, pcov2, ncov2 summed over the loci.  A region is a run of consecutive tested loci that all have p <= -s and a\n"
     "    difference of the same sign, each at most -g bases after the one before; a tested locus that does not qualify ends it.\n"
     "    The pooled difference can have the other sign than the loci; there is no region-level p-value (the loci were selected by p)",
     "Chain the tested loci of each context into regions and write <output-prefix>.diff.regions.<ctx>.bed: chrom, start, end,\n"
     "    loci, + or -, sample 1 % - sample 2 % of the pooled counts, smallest p-value, pcov1, ncov1, pcov2, ncov2 summed over the loci"},
    {'s', "<p>", [](const char* v, O& o) { return whole_double(v, o.region_max_p) && o.region_max_p > 0.0 && o.region_max_p <= 1.0; },
     "With -G: largest p-value of a locus in a region, in (0, 1]\n    Default: 0.01"},
    {'g', "<bp>", integer<&O::region_max_gap, 1, LLONG_MAX>, "With -G: largest distance between consecutive loci of a region, >= 1\n    Default: 500"},
    {'n', "<int>", integer<&O::region_min_loci, 1, INT_MAX>, "With -G: smallest number of loci of a region, >= 1\n    Default: 3"},
    {'B', "<sequence name>", [](const char* v, O& o) { o.control = v; return true; },
     "Test every covered locus for methylation above the caller's false-positive rate, measured per context on this\n"
     "    unmethylated control sequence (chloroplast, spiked-in lambda) as sum(pcov) / sum(pcov + ncov): write <prefix>.sites.<ctx>.bed,\n"
     "    the rows of <prefix>.<ctx>.cov.bed followed by the one-sided binomial p-value and its Benjamini-Hochberg q-value within\n"
     "    the context, and <prefix>.sites.rates.tsv: ctx, P, N, rate, loci"},
    {'e', "<r_cpg,r_chg,r_chh>", [](const char* v, O& o) { o.rates_given = true; return parse_rates(v, o.rates); },
     "Instead of -B: the three rates, each a decimal in [0, 1] or nan (context not tested), e.g. those an earlier\n"
     "    run wrote to <prefix>.sites.rates.tsv",
     nullptr,
     "ERROR: -e takes three comma-separated rates, each a decimal in [0, 1] or nan\n"},
    {'D', nullptr, flag<&O::domains>,
     "Cut the covered loci of each context into low (L) and high (H) methylated stretches and write <prefix>.domains.<ctx>.bed:\n"
     "    chrom, start, end, loci, L or H, 100 * pcov / (pcov + ncov) of the pooled counts, pcov, ncov, score (the pooled log-likelihood\n"
     "    ratio high : low in nats).  The stretches are the best path of a two-state model: a read counts log(hi / lo) when methylated\n"
     "    and log((1 - hi) / (1 - lo)) when not, a change of state costs -x, and loci more than -j bases apart are not linked.  The\n"
     "    combined counts are segmented, with or without -H.  The defaults below are conventions; nobody has tuned them on data"},
    {'u', "<lo:hi[,lo:hi,lo:hi]>", [](const char* v, O& o) { return parse_levels(v, o.domain_lo, o.domain_hi); },
     "With -D: the low and the high methylation level, 0 < lo < hi < 1, one pair for all contexts or one per\n"
     "    context (CpG,CHG,CHH); nan instead of a pair: that context is not segmented\n    Default: 0.1:0.8,0.05:0.5,0.02:0.2"},
    {'x', "<nats>", [](const char* v, O& o) { return whole_double(v, o.domain_penalty) && o.domain_penalty >= 0.0 && o.domain_penalty <= 256.0; },
     "With -D: penalty of a change of state, in [0, 256]\n    Default: 8"},
    {'j', "<bp>", integer<&O::domain_max_gap, 1, LLONG_MAX>, "With -D: largest distance between two loci that still links them, >= 1\n    Default: 1000"},
    {'Y', "<n>", integer<&O::domain_fit_iter, 1, LLONG_MAX>,
     "With -D: fit the two levels of every segmented context from the data, starting from -u: segment, take each\n"
     "    state's pooled methylation level as its new level, at most n times (hard EM; it stops when the integer weights repeat).\n"
     "    Also writes <prefix>.domains.fit.tsv: per context and iteration ctx, iter, lo, hi, A, B, P0, N0, R0, P1, N1, R1, then\n"
     "    ctx, status, lo, hi -- the fitted levels, which -u takes back"},
    {'E', "<2|3|4>", integer<&O::patterns, 2, 4>,
     "Read-level CpG patterns: every reference CpG heads a window of k adjacent reference CpGs; a read with a call at all\n"
     "    k of them counts under its pattern (bit i set: the i-th call is methylated; a deletion, mismatch or missing call at any\n"
     "    of the loci and the read does not count).  Writes <prefix>.patterns.CpG.bed: chrom, start, end, reads, methylation entropy\n"
     "    (bits per CpG), epipolymorphism, proportion of discordant reads, methylation level of those reads in %, the 2^k counts by\n"
     "    pattern.  The combined reads are counted, with or without -H"},
    {'w', "<bp>", integer<&O::pattern_span, 1, 65536>, "With -E: largest distance between the first and the last CpG of a window, in [1, 65536]\n    Default: 150"},
    {'o', "<int>", integer<&O::pattern_min_reads, 1, LLONG_MAX>, "With -E: smallest number of reads spanning a window that is written, >= 1\n    Default: 10"},
    {'M', nullptr, flag<&O::bedmethyl>,
     "bedMethyl output: write <prefix>.bedmethyl.CpG.bed (with -H also <prefix>.hap1. and <prefix>.hap2.bedmethyl.CpG.bed), one row\n"
     "    per reference CpG in modkit's 18 columns: chrom, start, end, m, min(1000, Nvalid), ., start, end, 255,0,0, Nvalid, percent\n"
     "    modified, Nmod, Ncanonical, Nother_mod (0), Ndelete, Nfail (0), Ndiff, Nnocall.  Nvalid = Nmod + Ncanonical; of the reads that\n"
     "    pass -q and -f, Nnocall covered the intact CG without a call, Ndiff show another base at the C or the G (or break off between\n"
     "    them), Ndelete have the C inside a deletion"},
    {'v', "<int>", integer<&O::bedmethyl_min_valid, 0, LLONG_MAX>,
     "With -M: smallest Nvalid of a row that is written, >= 0 (0: also CpGs seen only as nocall, diff or delete)\n    Default: 1"},
    {'L', "<bp>", integer<&O::linkage, 2, 16384>,
     "Within-read co-methylation by distance, bp in [2, 16384]: every two CpG calls of one read (one alignment record) that lie\n"
     "    d <= bp reference bases apart count once under d, as UU, UM, MU or MM (U unmethylated, M methylated by the CpG threshold; the\n"
     "    first letter is the call at the lower coordinate).  Writes <prefix>.linkage.CpG.tsv: a header line, then per distance dist, n,\n"
     "    n_uu, n_um, n_mu, n_mm, concordance (n_uu + n_mm) / n and the phi coefficient r (nan when a margin is empty).  The combined\n"
     "    reads are counted, with or without -H"},
    {'z', "<int>", integer<&O::linkage_min_pairs, 0, LLONG_MAX>,
     "With -L: smallest number of pairs of a distance that is written, >= 0 (0: every distance from 2 to bp)\n    Default: 1"},
    {'P', "<bp>", integer<&O::profile, 1, 2048>,
     "Methylation by position in the read, bp in [1, 2048]: every call that is counted also counts by its offset p in the read as\n"
     "    sequenced (L bases): in row 5' d = p or row 3' d = L - 1 - p when the nearer end is d < bp bases away (ties go to 5'), else in\n"
     "    the row `interior`.  Writes <prefix>.readpos.tsv: a header line, then per context and row context, end, dist, n, n_m, n_u,\n"
     "    percent methylated and the mean ML byte.  Calls within 200 bases of a read end saw a zero-padded kinetics window"},
    {'y', "<int>", integer<&O::profile_min_calls, 0, LLONG_MAX>, "With -P: smallest n of a row that is written, >= 0 (0: every row)\n    Default: 1"},
    {'I', "<n5>[:<n3>]", [](const char* v, O& o) { return parse_trim(v, o.trim5, o.trim3); },
     "Leave the calls in the first n5 and the last n3 bases of every read (as sequenced) out of all outputs; one number\n    sets both ends\n"
     "    Default: 0:0"},
    {'R', "<bed>", [](const char* v, O& o) { o.intervals = v; return true; },
     "Methylation of given intervals: a BED file (plain or gzip) of at least 3 tab-separated columns, name in column 4,\n"
     "    strand in column 6; empty lines and lines starting with #, track or browser are skipped.  Writes <prefix>.regions.<ctx>.tsv\n"
     "    (with -H also <prefix>.hap1. and <prefix>.hap2.regions.<ctx>.tsv): a header line, then per interval in input order chrom,\n"
     "    start, end, name, strand, n_loci, pcov, ncov, weighted = 100 pcov / (pcov + ncov) and mean, the mean of the loci's own\n"
     "    percentages (nan without a counted locus).  Intervals may overlap, nest and come in any order"},
    {'C', "<int>", integer<&O::interval_min_cov, 1, LLONG_MAX>, "With -R: smallest coverage (pcov + ncov) of a locus that counts, >= 1\n    Default: 1"},
    {'J', "<bins>[:<flank_bp>:<flank_bins>]", [](const char* v, O& o) { return parse_metaplot(v, o.meta_bins, o.meta_flank, o.meta_flank_bins); },
     "With -R: the metaplot.  Every interval of at least <bins> bases is cut into <bins> in [1, 1000] equal\n"
     "    bins, and each flank of flank_bp bases (a multiple of flank_bins in [1, 1000]) into flank_bins; a flank ends at its sequence's\n"
     "    end.  Bins run from upstream to downstream, mirrored for intervals on the - strand, and are summed over the intervals.  Writes\n"
     "    <prefix>.metaplot.<ctx>.tsv (with -H per haplotype too): `#regions used skipped`, a header line, then per bin bin, part (up,\n"
     "    body, down), n_regions, n_loci, pcov, ncov, weighted, mean\n    Default flank: 0:0"},
    {'S', "<flank>", integer<&O::context_flank, 0, 3>,
     "Methylation by sequence context: flank in [0, 3] bases on either side of the three-base context, k = 3 + 2 flank\n"
     "    (3, 5, 7 or 9), read on the strand of the called cytosine.  Writes <prefix>.context.<ctx>.tsv (with -H also\n"
     "    <prefix>.hap1. and <prefix>.hap2.context.<ctx>.tsv): a header line, then per k-mer with a counted locus, in k-mer order,\n"
     "    context, n_loci, pcov, ncov, weighted = 100 pcov / (pcov + ncov) and mean, the mean of the loci's own percentages; a last\n"
     "    row `other` holds the loci whose window leaves their sequence or holds a base outside ACGT"},
    {'O', "<int>", integer<&O::context_min_cov, 1, LLONG_MAX>, "With -S: smallest coverage (pcov + ncov) of a locus that counts, >= 1\n    Default: 1"},
    {'K', nullptr, flag<&O::kinetics>,
     "The input is an aligned BAM that carries the kinetics tags fi / fp / ri / rp instead of MM / ML: call 5mC on the\n"
     "    fly and pile the calls up directly.  For equal -c -l -p -T -q -f the output files are byte-identical to those of\n"
     "    `$0 call` on that BAM followed by `$0 pileup` on its output; no mod-BAM is written.  (Give -T explicitly\n"
     "    for that comparison: its default is chosen per run from the data and moves p by up to 1e-5.)  -b is not used:\n"
     "    records are batched by bases.  Only with -K, with the meaning and defaults of `call`:"},
    {'m', "<dir>", [](const char* v, O& o) { o.model_dir = v; return true; }, "Model directory holding {CpG,CHG,CHH}.onnx or .hmw\n    Default: <exe_dir>/../weights"},
    {'c', "<list>", [](const char* v, O& o) { return hmbam::parse_ctx(v, o.ctx_mask); },
     "Contexts to call: cpg,chg,chh\n    Default: all",
     nullptr,
     "Illegal argument to option '-c'\n"},
    {'l', "<int>", lenient<&O::min_read_size>, "Minimum read length to call\n    Default: 1000"},
    {'p', "<0|1|2>", lenient<&O::precision>, "Arithmetic of the CNN (see `call`)\n    Default: 1"},
    {'T', "<0|1>", lenient<&O::trunk>, "conv1..conv4 once per site (0) / once per read position (1)\n    Default: per context, from the first batch"},
};
const char DIFF_FLAGS[] = "aQGsgntd";
// `groupdiff` has two rows of its own, which neither `pileup -h` nor `diff -h` prints, and takes -t and -d from the table above
const Option GROUP_OPTIONS[] = {
    {'a', "<int>", integer<&O::group_min_cov, 1, (1 << 20) - 1>,
     "Minimum coverage (pcov + ncov) a sample needs at a locus to count there, in [1, 1048575]\n    Default: 5"},
    {'r', "<int>", integer<&O::group_min_reps, 1, 255>,
     "Minimum number of counting samples in each group at a tested locus, in [1, 255]; a locus also needs three\n"
     "    counting samples in all\n    Default: 2"},
};
const char GROUP_FLAGS[] = "artd";
// and so has `samplecorr`
const Option SAMPLE_OPTIONS[] = {
    {'a', "<int>", integer<&O::sample_min_cov, 1, (1 << 20) - 1>,
     "Minimum coverage (pcov + ncov) a sample needs at a locus to count there, in [1, 1048575]\n    Default: 5"},
    {'k', nullptr, flag<&O::sample_complete>,
     "Complete mode: every pair is taken over the loci where all samples count, not over those where its two samples count"},
};
const char SAMPLE_FLAGS[] = "aktd";
// and `regiondiff` five
const Option REGION_OPTIONS[] = {
    {'R', "<bed>", [](const char* v, O& o) { o.intervals = v; return true; },
     "The intervals to test, fixed before looking at the data: a BED file (plain or gzip) of at least 3 tab-separated columns,\n"
     "    name in column 4, strand in column 6; empty lines and lines starting with #, track or browser are skipped.  Intervals may\n"
     "    overlap, nest and come in any order.  Mandatory"},
    {'a', "<int>", integer<&O::sample_min_cov, 1, (1 << 20) - 1>,
     "Minimum coverage (pcov + ncov) a sample needs at a locus to count there, in [1, 1048575]\n    Default: 5"},
    {'k', nullptr, flag<&O::sample_complete>,
     "Complete mode: a locus is taken only where all samples of both groups count, not wherever the sample itself counts"},
    {'l', "<int>", integer<&O::region_min_sample_loci, 1, LLONG_MAX>,
     "Minimum number of counting loci a sample needs in an interval to be used there, >= 1\n    Default: 3"},
    {'r', "<int>", integer<&O::region_min_reps, 2, 64>,
     "Minimum number of used samples in each group of a tested interval, in [2, 64]\n    Default: 2"},
};
const char REGION_FLAGS[] = "Raklrtd";
// `groupdmr` takes -a and -r from `groupdiff`'s rows and brings six: its -s, -g and -n are not "With -G"
template <double O::*Field>
bool unit_interval(const char* v, O& o) { return whole_double(v, o.*Field) && o.*Field > 0.0 && o.*Field <= 1.0; }
const Option DMR_OPTIONS[] = {
    {'s', "<p>", unit_interval<&O::dmr_max_p>, "Largest p-value of a locus in a region, in (0, 1]\n    Default: 0.01"},
    {'F', "<q>", unit_interval<&O::dmr_max_q>,
     "Instead of -s: largest Benjamini-Hochberg q-value (within the context, over the whole job) of a locus in a region, in (0, 1]"},
    {'m', "<pct>", [](const char* v, O& o) { return whole_double(v, o.dmr_min_diff) && o.dmr_min_diff >= 0.0 && o.dmr_min_diff <= 100.0; },
     "Smallest |group 1 % - group 2 %| of a locus in a region, in [0, 100]\n    Default: 0"},
    {'g', "<bp>", integer<&O::dmr_max_gap, 1, LLONG_MAX>, "Largest distance between consecutive loci of a region, >= 1\n    Default: 500"},
    {'n', "<int>", integer<&O::dmr_min_loci, 1, INT_MAX>, "Smallest number of loci of a region, >= 1\n    Default: 3"},
    {'L', nullptr, flag<&O::dmr_loci>,
     "Also write <output-prefix>.groups.<ctx>.bed and <output-prefix>.groups.summary.tsv, as `groupdiff` with the same -a -r"},
};
const char DMR_FLAGS[] = "arsFmgnLtd";
// `smooth` brings three
const Option SMOOTH_OPTIONS[] = {
    {'W', "<bp>", integer<&O::smooth_half_width, 1, 16384>,
     "Half-width of the triangular kernel in bases, in [1, 16384]: a locus d < bp bases away has the weight bp - d\n    Default: 500"},
    {'a', "<int>", integer<&O::smooth_min_cov, 1, INT_MAX>,
     "Minimum coverage (pcov + ncov) of a locus that counts: as a row and in the windows of the others, >= 1\n    Default: 1"},
    {'i', "<int>", integer<&O::smooth_min_loci, 1, LLONG_MAX>,
     "Smallest number of counting loci in the window of a row that is written, the locus itself included, >= 1\n    Default: 1"},
};
const char SMOOTH_FLAGS[] = "Waitd";

const char PILEUP_HEADER[] =
    "USAGE:\n"
    "  $0 pileup [OPTIONS] reference mod-bam output-prefix\n"
    "\n"
    "DESCRIPTION:\n"
    "  Compute aggregate cytosine methylation states on the genomic reference\n"
    "\n"
    "OPTIONAL ARGUMENTS:\n";
const char DIFF_HEADER[] =
    "USAGE:\n"
    "  $0 diff [OPTIONS] reference prefix1 prefix2 output-prefix\n"
    "\n"
    "DESCRIPTION:\n"
    "  Test two samples for differential methylation, locus by locus, from the files two `pileup` runs wrote:\n"
    "  <prefix1>.<ctx>.cov.bed against <prefix2>.<ctx>.cov.bed for ctx in CpG, CHG, CHH (plain or gzip; a row is chrom, start,\n"
    "  start + 1, a percentage that is not read, methylated calls, unmethylated calls; further columns are ignored).  A context\n"
    "  without both files is skipped.  Writes <output-prefix>.diff.<ctx>.bed: chrom, start, end, sample 1 % - sample 2 %, two-sided\n"
    "  Fisher exact p-value, pcov1, ncov1, pcov2, ncov2 for every locus where each sample has at least -a calls; a locus the two\n"
    "  samples list under different contexts goes to the later one of CpG, CHG, CHH\n"
    "\n"
    "OPTIONAL ARGUMENTS (as the same letters of `pileup -H -A`):\n";

const char GROUP_HEADER[] =
    "USAGE:\n"
    "  $0 groupdiff [OPTIONS] reference a1,a2,... b1,b2,... output-prefix\n"
    "\n"
    "DESCRIPTION:\n"
    "  Test two groups of replicates for differential methylation, locus by locus.  Every element of the two comma-separated lists\n"
    "  is a prefix as `diff` takes it: <prefix>.<ctx>.cov.bed for ctx in CpG, CHG, CHH, plain or gzip.  A context is skipped unless\n"
    "  every sample of both groups has its file.  A sample counts at a locus with at least -a calls; a locus is tested with\n"
    "  at least -r counting samples in each group.  The test is the binomial likelihood ratio D of the pooled group counts, divided\n"
    "  by the dispersion phi = max(1, Pearson X2 of the samples around their group / nu), against F(1, nu), nu = counting samples - 2.\n"
    "  Writes <output-prefix>.groups.<ctx>.bed: chrom, start, end, group 1 % - group 2 %, p-value, Benjamini-Hochberg q-value within\n"
    "  the context, m1, pcov1, ncov1, m2, pcov2, ncov2 (counting samples and their pooled calls), phi; and\n"
    "  <output-prefix>.groups.summary.tsv: ctx, tested loci, loci with q <= 0.05, loci with q <= 0.01, loci with phi > 1\n"
    "\n"
    "OPTIONAL ARGUMENTS:\n";

const char SAMPLE_HEADER[] =
    "USAGE:\n"
    "  $0 samplecorr [OPTIONS] reference s1,s2,...,sN output-prefix\n"
    "\n"
    "DESCRIPTION:\n"
    "  The sample-by-sample correlation matrix of 2 to 64 pileups, per context.  Every element of the comma-separated list is a\n"
    "  prefix as `diff` takes it: <prefix>.<ctx>.cov.bed for ctx in CpG, CHG, CHH, plain or gzip.  A context is skipped unless every\n"
    "  sample has its file.  A sample counts at a locus with at least -a calls; its level there is floor(pcov * 32768 / (pcov + ncov)).\n"
    "  r is Pearson's correlation of the levels of two samples over the loci where both count (with -k: where all samples count),\n"
    "  from exact integer sums; nan with fewer than two such loci or a sample that is constant over them.\n"
    "  Writes <output-prefix>.samplecorr.<ctx>.tsv: sample_i, sample_j, shared loci n, mean level of i and of j over them in\n"
    "  percent, r, for every pair i < j; <output-prefix>.samplecorr.<ctx>.matrix.tsv: the N x N matrix of r under the samples' names;\n"
    "  and <output-prefix>.samplecorr.samples.tsv: ctx, sample, its counting loci, its mean level over them in percent\n"
    "\n"
    "OPTIONAL ARGUMENTS:\n";

const char REGION_HEADER[] =
    "USAGE:\n"
    "  $0 regiondiff -R intervals.bed [OPTIONS] reference a1,a2,... b1,b2,... output-prefix\n"
    "\n"
    "DESCRIPTION:\n"
    "  Test two groups of replicates for differential methylation over given intervals (promoters, gene bodies, tiles).  Every\n"
    "  element of the two comma-separated lists is a prefix as `diff` takes it: <prefix>.<ctx>.cov.bed for ctx in CpG, CHG, CHH,\n"
    "  plain or gzip; the groups hold 2 to 64 samples together and at least -r each.  A context is skipped unless every sample has\n"
    "  its file.  A sample counts at a locus with at least -a calls; its level there is floor(pcov * 32768 / (pcov + ncov)), and its\n"
    "  level in an interval the mean of those over its counting loci, if it has at least -l.  An interval is tested with at least -r\n"
    "  such samples in each group, by Welch's t-test on the samples' interval levels: the spread between replicates is the yardstick.\n"
    "  Writes <output-prefix>.regiondiff.<ctx>.tsv: a header line, then per interval in input order chrom, start, end, name, strand,\n"
    "  m1, m2 (used samples), loci1, loci2 (their counting loci), mean1, mean2 (percent), diff = mean1 - mean2, t, df, p and the\n"
    "  Benjamini-Hochberg q-value among the tested intervals of the context (nan where not tested); and\n"
    "  <output-prefix>.regiondiff.summary.tsv: ctx, intervals, tested, intervals with q <= 0.05, with q <= 0.01\n"
    "\n"
    "ARGUMENTS:\n";

const char DMR_HEADER[] =
    "USAGE:\n"
    "  $0 groupdmr [OPTIONS] reference a1,a2,... b1,b2,... output-prefix\n"
    "\n"
    "DESCRIPTION:\n"
    "  Differentially methylated regions between two groups of replicates.  The samples are given, loaded and tested locus by locus\n"
    "  as by `groupdiff` (-a, -r; `$0 groupdiff -h` has the test).  Per sequence and context the tested loci are then chained: a region\n"
    "  is a run of consecutive tested loci that all have p <= -s (or q <= -F), |group 1 % - group 2 %| >= -m and a difference of the\n"
    "  same sign, each at most -g bases after the one before; a tested locus that does not qualify ends it, a locus that is not\n"
    "  tested or belongs to another context does nothing.  Regions of at least -n loci are written.\n"
    "  Writes <output-prefix>.groupdmr.<ctx>.bed: chrom, start, end, name (<ctx>_<number>), loci, ., + or - (the sign of group 1 % -\n"
    "  group 2 % at every locus), group 1 % - group 2 % of the pooled counts, smallest p-value, then m1, pcov1, ncov1, m2, pcov2, ncov2\n"
    "  (fewest counting samples of the group at a locus; calls summed over the loci) and the largest phi; and\n"
    "  <output-prefix>.groupdmr.summary.tsv: ctx, tested loci, qualifying loci, the p cutoff used (nan: none), regions, loci in\n"
    "  regions, regions +, regions -.  The pooled difference can have the other sign than the loci.  There is no region-level\n"
    "  p-value: the loci were selected by their p, so a test of the pooled counts would not be one.  The BED file is valid input to\n"
    "  `regiondiff -R`, which adds the samples' levels per region; its p on regions found from the same samples is descriptive\n"
    "  only, for the same reason\n"
    "\n"
    "OPTIONAL ARGUMENTS:\n";

const char SMOOTH_HEADER[] =
    "USAGE:\n"
    "  $0 smooth [OPTIONS] reference prefix output-prefix\n"
    "\n"
    "DESCRIPTION:\n"
    "  Kernel-smoothed methylation levels of one sample, from the files a `pileup` run wrote: <prefix>.<ctx>.cov.bed for ctx in CpG,\n"
    "  CHG, CHH, plain or gzip, read as `diff` reads them; a context without its file is skipped.  A locus counts with at least -a\n"
    "  calls.  Every counting locus borrows from the counting loci of its context and sequence less than -W bases away, each\n"
    "  weighted by -W minus its distance (a triangular kernel): P and N are the weighted sums of their methylated and unmethylated\n"
    "  calls, all in integers.  Nothing crosses a sequence end; loci of other contexts or below -a in between are ignored.\n"
    "  Writes <output-prefix>.smooth.<ctx>.bed: chrom, start, end, the smoothed level 100 P / (P + N), the locus' own pcov and ncov,\n"
    "  the counting loci in its window, and the effective coverage (P + N) / -W, for every counting locus with at least -i loci in\n"
    "  its window; and <output-prefix>.smooth.summary.tsv: ctx, counting loci, rows written, -W\n"
    "\n"
    "OPTIONAL ARGUMENTS:\n";

const Option* find_option(Command cmd, char letter) {
    if (cmd == CMD_DIFF && !strchr(DIFF_FLAGS, letter)) return nullptr;
    if (cmd == CMD_GROUPDMR) {
        if (!strchr(DMR_FLAGS, letter)) return nullptr;
        for (const Option& opt : DMR_OPTIONS)
            if (opt.letter == letter) return &opt;
    }
    if (cmd == CMD_GROUPDIFF || cmd == CMD_GROUPDMR) {
        if (!strchr(cmd == CMD_GROUPDMR ? DMR_FLAGS : GROUP_FLAGS, letter)) return nullptr;
        for (const Option& opt : GROUP_OPTIONS)
            if (opt.letter == letter) return &opt;
    }
    if (cmd == CMD_SAMPLECORR) {
        if (!strchr(SAMPLE_FLAGS, letter)) return nullptr;
        for (const Option& opt : SAMPLE_OPTIONS)
            if (opt.letter == letter) return &opt;
    }
    if (cmd == CMD_SMOOTH) {
        if (!strchr(SMOOTH_FLAGS, letter)) return nullptr;
        for (const Option& opt : SMOOTH_OPTIONS)
            if (opt.letter == letter) return &opt;
    }
    if (cmd == CMD_REGIONDIFF) {
        if (!strchr(REGION_FLAGS, letter)) return nullptr;
        for (const Option& opt : REGION_OPTIONS)
            if (opt.letter == letter) return &opt;
    }
    for (const Option& opt : OPTIONS)
        if (opt.letter == letter) return &opt;
    return nullptr;
}

void print_text(const char* text, const char* exe) {  // $0: the program
    for (const char* p = text; *p; ++p) {
        if (p[0] == '$' && p[1] == '0') { fputs(exe, stderr); ++p; }
        else fputc(*p, stderr);
    }
}

void usage(Command cmd, const char* exe) {
    print_text(cmd == CMD_DIFF ? DIFF_HEADER : cmd == CMD_GROUPDIFF ? GROUP_HEADER : cmd == CMD_SAMPLECORR ? SAMPLE_HEADER :
               cmd == CMD_REGIONDIFF ? REGION_HEADER : cmd == CMD_GROUPDMR ? DMR_HEADER : cmd == CMD_SMOOTH ? SMOOTH_HEADER : PILEUP_HEADER, exe);
    const auto row = [&](const Option& opt) {
        fprintf(stderr, "  -%c%s%s\n    ", opt.letter, opt.metavar ? " " : "", opt.metavar ? opt.metavar : "");
        print_text(cmd == CMD_DIFF && opt.diff_help ? opt.diff_help : opt.help, exe);
        fputc('\n', stderr);
    };
    if (cmd == CMD_DIFF) for (const char* f = DIFF_FLAGS; *f; ++f) row(*find_option(cmd, *f));
    else if (cmd == CMD_GROUPDIFF) for (const char* f = GROUP_FLAGS; *f; ++f) row(*find_option(cmd, *f));
    else if (cmd == CMD_SAMPLECORR) for (const char* f = SAMPLE_FLAGS; *f; ++f) row(*find_option(cmd, *f));
    else if (cmd == CMD_REGIONDIFF) for (const char* f = REGION_FLAGS; *f; ++f) row(*find_option(cmd, *f));
    else if (cmd == CMD_GROUPDMR) for (const char* f = DMR_FLAGS; *f; ++f) row(*find_option(cmd, *f));
    else if (cmd == CMD_SMOOTH) for (const char* f = SMOOTH_FLAGS; *f; ++f) row(*find_option(cmd, *f));
    else for (const Option& opt : OPTIONS) row(opt);
}

// what the command line held, by flag letter: given at all; given with a value its row did not take
struct Parsed {
    const PileupOptions& o;
    std::string seen, bad;
    bool levels_bad;  // -D, -u and -x parse, and the levels give no usable weights (levels_ok)
    bool any_seen(const char* letters) const { return seen.find_first_of(letters) != std::string::npos; }
    bool any_bad(const char* letters) const { return bad.find_first_of(letters) != std::string::npos; }
};

// The checks between options.  The first rule that fires is the one reported, whatever the order on the command line, so the order
// of this list is the precedence: the groups asm, call, sites, domains, patterns, bedmethyl, linkage, profile, intervals, context,
// and inside each group the order below.  It is not uniform -- patterns, linkage, profile and context report a bad value before a
// missing parent, asm, domains, bedmethyl and intervals the missing parent first -- and tests/golden/cli_options.json pins it.
// `diff` runs the rules marked CMD_DIFF, `groupdiff` those marked CMD_GROUPDIFF, `samplecorr` those marked CMD_SAMPLECORR,
// `regiondiff` those marked CMD_REGIONDIFF, `groupdmr` those marked CMD_GROUPDMR, `smooth` those marked CMD_SMOOTH.
struct Rule {
    int commands;
    bool (*fires)(const Parsed& p);
    const char* message;
};

const Rule RULES[] = {
    {CMD_PILEUP, [](const Parsed& p) { return p.o.asm_test && !p.o.haplotypes; }, "-A needs -H (the test compares the two haplotypes)"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("a") && !p.o.asm_test; }, "-a needs -A"},
    {CMD_PILEUP, [](const Parsed& p) { return p.o.asm_q && !p.o.asm_test; }, "-Q needs -A (the q-values are those of its p-values)"},
    {CMD_PILEUP | CMD_DIFF, [](const Parsed& p) { return p.o.asm_min_cov < 1; }, "-a must be >= 1"},
    {CMD_PILEUP, [](const Parsed& p) { return p.o.asm_regions && !p.o.asm_test; }, "-G needs -A (the regions are chains of its tested loci)"},
    {CMD_PILEUP | CMD_DIFF, [](const Parsed& p) { return p.any_seen("sgn") && !p.o.asm_regions; }, "-s, -g and -n need -G"},
    {CMD_PILEUP | CMD_DIFF, [](const Parsed& p) { return p.any_bad("sgn"); }, "-s must be in (0, 1], -g and -n integers >= 1"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("mclpT") && !p.o.kinetics; }, "-m, -c, -l, -p and -T need -K (they configure the on-the-fly caller)"},
    {CMD_PILEUP, [](const Parsed& p) { return p.o.min_read_size < 0; }, "-l must be >= 0"},
    {CMD_PILEUP, [](const Parsed& p) { return p.o.precision < 0 || p.o.precision > 2; }, "-p must be 0, 1 or 2"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("mclpT") && (p.o.trunk < -1 || p.o.trunk > 1); }, "-T must be 0 or 1"},
    {CMD_PILEUP, [](const Parsed& p) { return !p.o.control.empty() && p.o.rates_given; }, "-B and -e exclude each other (the rates are measured, or given)"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("uxj") && !p.o.domains; }, "-u, -x and -j need -D"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("Y") && !p.o.domains; }, "-Y needs -D (it fits the levels of -D)"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_bad("Y"); }, "-Y takes the largest number of iterations, an integer >= 1"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_bad("uxj") || p.levels_bad; },
     "-u takes lo:hi with 0 < lo < hi < 1 (levels a 2^24-th of a nat apart at least) or nan, once or per context; "
     "-x must be in [0, 256], -j an integer >= 1"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_bad("Ewo"); }, "-E must be 2, 3 or 4, -w an integer in [1, 65536], -o an integer >= 1"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("wo") && !p.o.patterns; }, "-w and -o need -E"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("v") && !p.o.bedmethyl; }, "-v needs -M"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_bad("v"); }, "-v must be an integer >= 0"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_bad("Lz"); }, "-L must be an integer in [2, 16384], -z an integer >= 0"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("z") && !p.o.linkage; }, "-z needs -L"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_bad("PyI"); }, "-P must be an integer in [1, 2048], -y an integer >= 0, -I n5[:n3] with integers >= 0"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("y") && !p.o.profile; }, "-y needs -P"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("CJ") && p.o.intervals.empty(); }, "-C and -J need -R"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_bad("CJ"); },
     "-C must be an integer >= 1, -J bins[:flank_bp:flank_bins] with bins in [1, 1000] and flank_bp a multiple of flank_bins in [1, 1000]"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_bad("SO"); }, "-S must be an integer in [0, 3], -O an integer >= 1"},
    {CMD_PILEUP, [](const Parsed& p) { return p.any_seen("O") && p.o.context_flank < 0; }, "-O needs -S"},
    {CMD_GROUPDIFF | CMD_GROUPDMR, [](const Parsed& p) { return p.any_bad("ar"); }, "-a must be an integer in [1, 1048575], -r an integer in [1, 255]"},
    {CMD_SAMPLECORR, [](const Parsed& p) { return p.any_bad("a"); }, "-a must be an integer in [1, 1048575]"},
    {CMD_REGIONDIFF, [](const Parsed& p) { return p.o.intervals.empty(); }, "regiondiff needs -R (the intervals to test)"},
    {CMD_REGIONDIFF, [](const Parsed& p) { return p.any_bad("alr"); },
     "-a must be an integer in [1, 1048575], -l an integer >= 1, -r an integer in [2, 64]"},
    {CMD_GROUPDMR, [](const Parsed& p) { return p.any_seen("s") && p.any_seen("F"); }, "-s and -F exclude each other (the loci are chosen by p, or by q)"},
    {CMD_GROUPDMR, [](const Parsed& p) { return p.any_bad("sFmgn"); }, "-s and -F must be in (0, 1], -m in [0, 100], -g and -n integers >= 1"},
    {CMD_SMOOTH, [](const Parsed& p) { return p.any_bad("Wai"); }, "-W must be an integer in [1, 16384], -a an integer in [1, 2147483647], -i an integer >= 1"},
};

}  // namespace

void command_usage(Command cmd, const char* exe) { usage(cmd, exe); }

bool parse_command_line(Command cmd, int argc, char** argv, PileupOptions& o, int& first, int& status, bool (*levels_ok)(PileupOptions&)) {
    const auto leave = [&](int code) { usage(cmd, argv[0]); status = code; return false; };
    Parsed p{o, {}, {}, false};
    int i = 2;
    for (; i < argc; ++i) {
        const char* a = argv[i];
        if (!strcmp(a, "-h")) return leave(0);
        if (a[0] != '-' || !a[1]) break;
        const Option* opt = a[2] ? nullptr : find_option(cmd, a[1]);
        if (opt && !opt->metavar) { opt->parse(nullptr, o); continue; }
        if (i + 1 >= argc) return leave(EXIT_FAILURE);
        if (!opt) {  // pileup's message has never ended its line; the fixture keeps it so until that is changed on purpose
            fprintf(stderr, "ERROR: unrecognised option %s%s", a, cmd == CMD_PILEUP ? "" : "\n");
            return leave(EXIT_FAILURE);
        }
        p.seen += opt->letter;
        if (opt->parse(argv[++i], o)) continue;
        if (opt->fatal) { fputs(opt->fatal, stderr); return leave(EXIT_FAILURE); }
        p.bad += opt->letter;
    }
    if (argc - i != (cmd == CMD_PILEUP || cmd == CMD_SAMPLECORR || cmd == CMD_SMOOTH ? 3 : 4)) return leave(EXIT_FAILURE);
    // ahead of the rules although its rule comes tenth: it only writes the weights, which every earlier way out discards
    p.levels_bad = o.domains && !p.any_bad("uxj") && levels_ok && !levels_ok(o);
    for (const Rule& r : RULES)
        if ((r.commands & cmd) && r.fires(p)) {
            fprintf(stderr, "ERROR: %s\n", r.message);
            return leave(EXIT_FAILURE);
        }
    first = i;
    return true;
}
