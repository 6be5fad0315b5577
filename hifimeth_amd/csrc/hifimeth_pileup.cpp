// hifimeth_pileup.cpp -- `hifimeth-hip pileup [OPTIONS] reference mod-bam output-prefix`
// Same command line, stderr messages and output files as `hifimeth pileup` (src/app/hifimeth/pileup.cpp:22-112,
// 461-606): <prefix>.CpG.cov.bed, <prefix>.CHG.cov.bed, <prefix>.CHH.cov.bed with rows
//   chrom <tab> soff <tab> soff+1 <tab> 100*pcov/(pcov+ncov) <tab> pcov <tab> ncov
// The host parses the BAM and the MM/ML lists (parallel over the reads of a batch); alignment projection,
// histograms and per-locus counting run on the GPU through the hm_pileup_* C ABI.  No temporary file is written:
// the projected calls stay in HBM until the thresholds are known.
// -H (ours): also <prefix>.hap1.<ctx>.cov.bed / <prefix>.hap2.<ctx>.cov.bed from the records' integer HP tag, counted with
// the combined thresholds, each locus in its combined context.
// -A (ours, with -H): also <prefix>.asm.<ctx>.bed, one row per locus where each haplotype has at least -a (default 5) counted
// calls:  chrom <tab> soff <tab> soff+1 <tab> diff <tab> pvalue <tab> pcov1 <tab> ncov1 <tab> pcov2 <tab> ncov2
// (difference of the two methylation percentages, two-sided Fisher exact test; both computed on the GPU).
// -Q (ours, with -A): a tenth column qvalue in those rows, the Benjamini-Hochberg q of the p-value among all tested loci of the context,
// and <prefix>.asm.summary.tsv: ctx, tested loci, loci with q <= 0.05, loci with q <= 0.01.
// -G (ours, with -A): also <prefix>.asm.regions.<ctx>.bed, one row per run of at least -n (default 3) consecutive tested loci of
// the context that all have p <= -s (default 0.01) and a difference of the same sign, each at most -g (default 500) bases from
// the one before:  chrom <tab> start <tab> end <tab> n_loci <tab> +|- <tab> diff <tab> pmin <tab> pcov1 <tab> ncov1 <tab> pcov2 <tab> ncov2
// (the counts pooled over the run's loci; chained on the GPU).
// -B <control sequence> or -e <r_cpg,r_chg,r_chh> (ours): also <prefix>.sites.<ctx>.bed, the rows of <prefix>.<ctx>.cov.bed followed
// by pvalue and qvalue -- the one-sided binomial test of the locus against the context's false-positive rate (measured on the
// unmethylated control sequence, or given) and its Benjamini-Hochberg q-value within the context -- and <prefix>.sites.rates.tsv
// (DESIGN.md section 10).
// -D (ours): also <prefix>.domains.<ctx>.bed, the covered loci of each context cut into low and high methylated stretches by an
// exact two-state Viterbi scan on the GPU (levels -u, switch penalty -x, largest linking distance -j):
//   chrom <tab> start <tab> end <tab> n_loci <tab> L|H <tab> level <tab> pcov <tab> ncov <tab> score      (DESIGN.md section 10).
// -D -Y n (ours): the two levels are fitted from the data first, from -u in at most n iterations of hard EM over the state sums
// the GPU gives (hm_pileup_domain_sums); also <prefix>.domains.fit.tsv, the iterations and the fitted levels.
// -M (ours): also <prefix>.bedmethyl.CpG.bed (under -H also <prefix>.hap1. / <prefix>.hap2.bedmethyl.CpG.bed), modkit's 18 bedMethyl
// columns per reference CpG: besides the methylated and unmethylated calls the reads that covered the CpG without giving one --
// no call, another base, a deletion -- counted on the GPU (hm_pileup_fetch_bedmethyl).
// -L bp (ours): also <prefix>.linkage.CpG.tsv, the within-read co-methylation by distance: per exact distance d <= bp the pairs of
// calls d bases apart on one molecule by class -- both unmethylated, the two discordant orders, both methylated -- with their
// concordance and phi coefficient (hm_pileup_fetch_linkage).
// -P bp (ours): also <prefix>.readpos.tsv, methylation by position in the read: per context the calls 0 .. bp - 1 bases from the read's
// 5' end, from its 3' end, and all others, with the percentage methylated and the mean ML byte (hm_pileup_fetch_readpos, DESIGN.md
// section 10).  -I n5[:n3] (ours): the calls in the first n5 and the last n3 bases of a read are left out of every output.
// -R bed (ours): also <prefix>.regions.<ctx>.tsv, the methylation of each interval of the BED file (loci with coverage >= -C), and with
// -J bins[:flank:flank_bins] <prefix>.metaplot.<ctx>.tsv, the profile across all intervals and their flanks (hm_pileup_fetch_regions,
// hm_pileup_fetch_metaplot).  The file is read and checked before the engine exists.
// -S flank (ours): also <prefix>.context.<ctx>.tsv, the methylation by the k = 3 + 2 flank bases around the called cytosine, read on
// its strand (loci with coverage >= -O; hm_pileup_fetch_context).
// -K (ours): the input is an aligned BAM that still carries the kinetics tags (pbmm2 keeps fi / fp / ri / rp): the reads are called
// on the fly by the call engine and their calls go straight to the pileup engine (hm_pileup_submit_read_calls) -- the files
// `call` followed by `pileup` writes, without the mod-BAM between the two.
#include <strings.h>
#include <zlib.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <climits>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <random>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../../include/hifimeth_hip.h"
#include "hm_bam.h"

using namespace hmbam;

// CIGAR of a record as uint32 ops.  A CIGAR of more than 65535 operations does not fit the 16-bit n_cigar_op field: the
// record then carries the placeholder <l_seq>S<ref_len>N and the real operations in a CG:B,I tag (SAMv1 section 4.2.2);
// htslib's sam_read1 -- what the reference's pileup reads with -- swaps them back in, and so does this.
static void real_cigar(const BamRecord& r, std::vector<uint32_t>& cig) {
    cig.resize((size_t)r.n_cigar());
    if (!cig.empty()) memcpy(cig.data(), r.cigar_bytes(), 4 * cig.size());
    if (cig.size() != 2 || (cig[0] & 15) != 4 || (int32_t)(cig[0] >> 4) != r.l_qseq() || (cig[1] & 15) != 3) return;
    const uint8_t* p = r.data.data() + r.aux_offset();
    const uint8_t* end = r.data.data() + r.data.size();
    AuxField f;
    while (p < end && next_aux(p, end, f))
        if (f.tag[0] == 'C' && f.tag[1] == 'G' && f.type == 'B' && (f.subtype == 'I' || f.subtype == 'i')) {
            cig.resize(f.count);
            memcpy(cig.data(), f.payload, 4 * (size_t)f.count);
            return;
        }
}


namespace {
void report_thresholds(const uint64_t* bins, uint8_t thr[3]);
}  // namespace

namespace {

struct PileupOptions {
    int min_mapq = 0;     // kMinMapQ
    double min_pi = 0.0;  // kMinPi
    int threads = 8;      // kNumThreads
    int device = 0;
    int read_batch = 512;
    bool haplotypes = false;  // -H: also <prefix>.hap1.* / <prefix>.hap2.* from the HP tag
    bool asm_test = false;    // -A: per-locus haplotype difference + Fisher exact test -> <prefix>.asm.*
    int asm_min_cov = 5;      // -a: minimum pcov + ncov of each haplotype for a locus to be tested
    bool asm_min_cov_given = false;
    bool asm_q = false;       // -Q: Benjamini-Hochberg q-value per tested locus, <prefix>.asm.summary.tsv
    bool asm_regions = false; // -G: chains of tested loci that lean the same way -> <prefix>.asm.regions.*
    double region_max_p = 0.01;     // -s: a locus is a hit when its p-value is at most this
    long long region_max_gap = 500; // -g: largest distance between two consecutive loci of a region
    int region_min_loci = 3;        // -n: smallest region written
    bool region_option_given = false, region_option_bad = false;  // any of -s -g -n; one of them with a value out of range
    std::string control;      // -B: name of the unmethylated control sequence -> rates measured there, <prefix>.sites.*
    bool rates_given = false; // -e: the three rates given directly (NaN: context not tested)
    double rates[3] = {0, 0, 0};
    bool domains = false;     // -D: low / high methylated stretches -> <prefix>.domains.*
    double domain_lo[3] = {0.1, 0.05, 0.02}, domain_hi[3] = {0.8, 0.5, 0.2};  // -u: the two levels per context; NaN: not segmented
    double domain_penalty = 8.0;       // -x: cost of a change of state, in nats
    long long domain_max_gap = 1000;   // -j: largest distance that still links two loci
    bool domain_option_given = false, domain_option_bad = false;  // any of -u -x -j; one of them with a value out of range
    long long domain_fit_iter = 0;     // -Y: fit the two levels from the data, at most this many iterations; 0: not asked for
    bool domain_fit_bad = false;
    int patterns = 0;                  // -E: read-level patterns over windows of k adjacent reference CpGs -> <prefix>.patterns.CpG.bed
    long long pattern_span = 150;      // -w: largest distance between the first and the last locus of a window
    long long pattern_min_reads = 10;  // -o: smallest number of reads spanning a window that is written
    bool pattern_option_given = false, pattern_option_bad = false;  // -w or -o; -E, -w or -o with a value out of range
    bool bedmethyl = false;            // -M: bedMethyl rows with the depth classes per reference CpG -> <prefix>.bedmethyl.CpG.bed
    long long bedmethyl_min_valid = 1; // -v: smallest n_mod + n_canon of a row that is written
    bool bedmethyl_option_given = false, bedmethyl_option_bad = false;  // -v; -v with a value out of range
    long long linkage = 0;             // -L: within-read co-methylation by distance up to this many bases -> <prefix>.linkage.CpG.tsv
    long long linkage_min_pairs = 1;   // -z: smallest number of pairs of a distance that is written
    bool linkage_option_given = false, linkage_option_bad = false;  // -z; -L or -z with a value out of range
    long long profile = 0;             // -P: methylation by position in the read, the ends resolved up to this many bases -> <prefix>.readpos.tsv
    long long profile_min_calls = 1;   // -y: smallest number of calls of a row that is written
    long long trim5 = 0, trim3 = 0;    // -I: the calls in the first trim5 / last trim3 bases of a read are dropped
    bool profile_option_given = false, profile_option_bad = false;  // -y; -P, -y or -I with a value out of range
    std::string intervals;             // -R: BED file of intervals -> <prefix>.regions.<ctx>.tsv
    long long interval_min_cov = 1;    // -C: smallest pcov + ncov of a locus that counts under -R / -J
    int meta_bins = 0, meta_flank_bins = 0;  // -J bins[:flank:flank_bins] -> <prefix>.metaplot.<ctx>.tsv
    long long meta_flank = 0;
    bool interval_option_given = false, interval_option_bad = false;  // -C or -J; either with a value out of range
    int context_flank = -1;            // -S: 0 .. 3 -> <prefix>.context.<ctx>.tsv by the 3 + 2 flank bases around the cytosine; -1: off
    long long context_min_cov = 1;     // -O: smallest pcov + ncov of a locus that counts under -S
    bool context_option_given = false, context_option_bad = false;  // -O; -S or -O with a value out of range
    // -K: call on the fly; the options below are `call`'s (hifimeth_call.cpp), same meaning and defaults
    bool kinetics = false;
    bool call_option_given = false;  // any of -m -c -l -p -T: a usage error without -K
    std::string model_dir;           // -m, default <exe_dir>/../weights
    int ctx_mask = 7;                // -c
    int min_read_size = 1000;        // -l
    int precision = 1;               // -p
    int trunk = -1;                  // -T; -1: the call engine decides per context from its first batch
    std::string ref, bam, prefix;
};

void pileup_usage(const char* exe) {
    fprintf(stderr,
            "USAGE:\n  %s pileup [OPTIONS] reference mod-bam output-prefix\n\n"
            "DESCRIPTION:\n  Compute aggregate cytosine methylation states on the genomic reference\n\n"
            "OPTIONAL ARGUMENTS:\n"
            "  -q <mapQ>\n    Minimum mapping quality score\n    Default: 0\n"
            "  -f <Alignment identity>\n    Default: 0\n"
            "  -t <CPU threads>\n    Number of CPU threads\n    Default: 8\n"
            "  -d <int>\n    GPU ordinal\n    Default: 0\n"
            "  -b <int>\n    BAM records per GPU batch\n    Default: 512\n"
            "  -H\n    Haplotype-resolved output: records tagged HP:i:1 / HP:i:2 are also counted into\n"
            "    <prefix>.hap1.<ctx>.cov.bed / <prefix>.hap2.<ctx>.cov.bed (same thresholds as the combined files)\n"
            "  -A\n    With -H: test every locus where both haplotypes are covered for a difference between them and write\n"
            "    <prefix>.asm.<ctx>.bed: chrom, start, end, hap1 %% - hap2 %%, two-sided Fisher exact p-value, pcov1, ncov1, pcov2, ncov2\n"
            "  -a <int>\n    With -A: minimum coverage (pcov + ncov) of each haplotype at a tested locus\n    Default: 5\n"
            "  -Q\n    With -A: a tenth column, the Benjamini-Hochberg q-value of the p-value among all tested loci of the context, and\n"
            "    <prefix>.asm.summary.tsv: ctx, tested loci, loci with q <= 0.05, loci with q <= 0.01\n"
            "  -G\n    With -A: chain the tested loci of each context into regions and write <prefix>.asm.regions.<ctx>.bed: chrom, start, end,\n"
            "    loci, + or - (the sign of hap1 %% - hap2 %% at every locus), hap1 %% - hap2 %% of the pooled counts, smallest p-value,\n"
            "    pcov1, ncov1, pcov2, ncov2 summed over the loci.  A region is a run of consecutive tested loci that all have p <= -s and a\n"
            "    difference of the same sign, each at most -g bases after the one before; a tested locus that does not qualify ends it.\n"
            "    The pooled difference can have the other sign than the loci; there is no region-level p-value (the loci were selected by p)\n"
            "  -s <p>\n    With -G: largest p-value of a locus in a region, in (0, 1]\n    Default: 0.01\n"
            "  -g <bp>\n    With -G: largest distance between consecutive loci of a region, >= 1\n    Default: 500\n"
            "  -n <int>\n    With -G: smallest number of loci of a region, >= 1\n    Default: 3\n"
            "  -B <sequence name>\n    Test every covered locus for methylation above the caller's false-positive rate, measured per context on this\n"
            "    unmethylated control sequence (chloroplast, spiked-in lambda) as sum(pcov) / sum(pcov + ncov): write <prefix>.sites.<ctx>.bed,\n"
            "    the rows of <prefix>.<ctx>.cov.bed followed by the one-sided binomial p-value and its Benjamini-Hochberg q-value within\n"
            "    the context, and <prefix>.sites.rates.tsv: ctx, P, N, rate, loci\n"
            "  -e <r_cpg,r_chg,r_chh>\n    Instead of -B: the three rates, each a decimal in [0, 1] or nan (context not tested), e.g. those an earlier\n"
            "    run wrote to <prefix>.sites.rates.tsv\n"
            "  -D\n    Cut the covered loci of each context into low (L) and high (H) methylated stretches and write <prefix>.domains.<ctx>.bed:\n"
            "    chrom, start, end, loci, L or H, 100 * pcov / (pcov + ncov) of the pooled counts, pcov, ncov, score (the pooled log-likelihood\n"
            "    ratio high : low in nats).  The stretches are the best path of a two-state model: a read counts log(hi / lo) when methylated\n"
            "    and log((1 - hi) / (1 - lo)) when not, a change of state costs -x, and loci more than -j bases apart are not linked.  The\n"
            "    combined counts are segmented, with or without -H.  The defaults below are conventions; nobody has tuned them on data\n"
            "  -u <lo:hi[,lo:hi,lo:hi]>\n    With -D: the low and the high methylation level, 0 < lo < hi < 1, one pair for all contexts or one per\n"
            "    context (CpG,CHG,CHH); nan instead of a pair: that context is not segmented\n    Default: 0.1:0.8,0.05:0.5,0.02:0.2\n"
            "  -x <nats>\n    With -D: penalty of a change of state, in [0, 256]\n    Default: 8\n"
            "  -j <bp>\n    With -D: largest distance between two loci that still links them, >= 1\n    Default: 1000\n"
            "  -Y <n>\n    With -D: fit the two levels of every segmented context from the data, starting from -u: segment, take each\n"
            "    state's pooled methylation level as its new level, at most n times (hard EM; it stops when the integer weights repeat).\n"
            "    Also writes <prefix>.domains.fit.tsv: per context and iteration ctx, iter, lo, hi, A, B, P0, N0, R0, P1, N1, R1, then\n"
            "    ctx, status, lo, hi -- the fitted levels, which -u takes back\n"
            "  -E <2|3|4>\n    Read-level CpG patterns: every reference CpG heads a window of k adjacent reference CpGs; a read with a call at all\n"
            "    k of them counts under its pattern (bit i set: the i-th call is methylated; a deletion, mismatch or missing call at any\n"
            "    of the loci and the read does not count).  Writes <prefix>.patterns.CpG.bed: chrom, start, end, reads, methylation entropy\n"
            "    (bits per CpG), epipolymorphism, proportion of discordant reads, methylation level of those reads in %%, the 2^k counts by\n"
            "    pattern.  The combined reads are counted, with or without -H\n"
            "  -w <bp>\n    With -E: largest distance between the first and the last CpG of a window, in [1, 65536]\n    Default: 150\n"
            "  -o <int>\n    With -E: smallest number of reads spanning a window that is written, >= 1\n    Default: 10\n"
            "  -M\n    bedMethyl output: write <prefix>.bedmethyl.CpG.bed (with -H also <prefix>.hap1. and <prefix>.hap2.bedmethyl.CpG.bed), one row\n"
            "    per reference CpG in modkit's 18 columns: chrom, start, end, m, min(1000, Nvalid), ., start, end, 255,0,0, Nvalid, percent\n"
            "    modified, Nmod, Ncanonical, Nother_mod (0), Ndelete, Nfail (0), Ndiff, Nnocall.  Nvalid = Nmod + Ncanonical; of the reads that\n"
            "    pass -q and -f, Nnocall covered the intact CG without a call, Ndiff show another base at the C or the G (or break off between\n"
            "    them), Ndelete have the C inside a deletion\n"
            "  -v <int>\n    With -M: smallest Nvalid of a row that is written, >= 0 (0: also CpGs seen only as nocall, diff or delete)\n    Default: 1\n"
            "  -L <bp>\n    Within-read co-methylation by distance, bp in [2, 16384]: every two CpG calls of one read (one alignment record) that lie\n"
            "    d <= bp reference bases apart count once under d, as UU, UM, MU or MM (U unmethylated, M methylated by the CpG threshold; the\n"
            "    first letter is the call at the lower coordinate).  Writes <prefix>.linkage.CpG.tsv: a header line, then per distance dist, n,\n"
            "    n_uu, n_um, n_mu, n_mm, concordance (n_uu + n_mm) / n and the phi coefficient r (nan when a margin is empty).  The combined\n"
            "    reads are counted, with or without -H\n"
            "  -z <int>\n    With -L: smallest number of pairs of a distance that is written, >= 0 (0: every distance from 2 to bp)\n    Default: 1\n"
            "  -P <bp>\n    Methylation by position in the read, bp in [1, 2048]: every call that is counted also counts by its offset p in the read as\n"
            "    sequenced (L bases): in row 5' d = p or row 3' d = L - 1 - p when the nearer end is d < bp bases away (ties go to 5'), else in\n"
            "    the row `interior`.  Writes <prefix>.readpos.tsv: a header line, then per context and row context, end, dist, n, n_m, n_u,\n"
            "    percent methylated and the mean ML byte.  Calls within 200 bases of a read end saw a zero-padded kinetics window\n"
            "  -y <int>\n    With -P: smallest n of a row that is written, >= 0 (0: every row)\n    Default: 1\n"
            "  -I <n5>[:<n3>]\n    Leave the calls in the first n5 and the last n3 bases of every read (as sequenced) out of all outputs; one number\n"
            "    sets both ends\n    Default: 0:0\n"
            "  -R <bed>\n    Methylation of given intervals: a BED file (plain or gzip) of at least 3 tab-separated columns, name in column 4,\n"
            "    strand in column 6; empty lines and lines starting with #, track or browser are skipped.  Writes <prefix>.regions.<ctx>.tsv\n"
            "    (with -H also <prefix>.hap1. and <prefix>.hap2.regions.<ctx>.tsv): a header line, then per interval in input order chrom,\n"
            "    start, end, name, strand, n_loci, pcov, ncov, weighted = 100 pcov / (pcov + ncov) and mean, the mean of the loci's own\n"
            "    percentages (nan without a counted locus).  Intervals may overlap, nest and come in any order\n"
            "  -C <int>\n    With -R: smallest coverage (pcov + ncov) of a locus that counts, >= 1\n    Default: 1\n"
            "  -J <bins>[:<flank_bp>:<flank_bins>]\n    With -R: the metaplot.  Every interval of at least <bins> bases is cut into <bins> in [1, 1000] equal\n"
            "    bins, and each flank of flank_bp bases (a multiple of flank_bins in [1, 1000]) into flank_bins; a flank ends at its sequence's\n"
            "    end.  Bins run from upstream to downstream, mirrored for intervals on the - strand, and are summed over the intervals.  Writes\n"
            "    <prefix>.metaplot.<ctx>.tsv (with -H per haplotype too): `#regions used skipped`, a header line, then per bin bin, part (up,\n"
            "    body, down), n_regions, n_loci, pcov, ncov, weighted, mean\n    Default flank: 0:0\n"
            "  -S <flank>\n    Methylation by sequence context: flank in [0, 3] bases on either side of the three-base context, k = 3 + 2 flank\n"
            "    (3, 5, 7 or 9), read on the strand of the called cytosine.  Writes <prefix>.context.<ctx>.tsv (with -H also\n"
            "    <prefix>.hap1. and <prefix>.hap2.context.<ctx>.tsv): a header line, then per k-mer with a counted locus, in k-mer order,\n"
            "    context, n_loci, pcov, ncov, weighted = 100 pcov / (pcov + ncov) and mean, the mean of the loci's own percentages; a last\n"
            "    row `other` holds the loci whose window leaves their sequence or holds a base outside ACGT\n"
            "  -O <int>\n    With -S: smallest coverage (pcov + ncov) of a locus that counts, >= 1\n    Default: 1\n"
            "  -K\n    The input is an aligned BAM that carries the kinetics tags fi / fp / ri / rp instead of MM / ML: call 5mC on the\n"
            "    fly and pile the calls up directly.  For equal -c -l -p -T -q -f the output files are byte-identical to those of\n"
            "    `%s call` on that BAM followed by `%s pileup` on its output; no mod-BAM is written.  (Give -T explicitly\n"
            "    for that comparison: its default is chosen per run from the data and moves p by up to 1e-5.)  -b is not used:\n"
            "    records are batched by bases.  Only with -K, with the meaning and defaults of `call`:\n"
            "  -m <dir>\n    Model directory holding {CpG,CHG,CHH}.onnx or .hmw\n    Default: <exe_dir>/../weights\n"
            "  -c <list>\n    Contexts to call: cpg,chg,chh\n    Default: all\n"
            "  -l <int>\n    Minimum read length to call\n    Default: 1000\n"
            "  -p <0|1|2>\n    Arithmetic of the CNN (see `call`)\n    Default: 1\n"
            "  -T <0|1>\n    conv1..conv4 once per site (0) / once per read position (1)\n    Default: per context, from the first batch\n",
            exe, exe, exe);
}

// s_bam_is_mapped_and_sorted (pileup.cpp:438-459)
bool mapped_and_sorted(const BamHeader& h) {
    bool sorted = false;
    size_t p = 0;
    while (p < h.text.size()) {
        size_t e = h.text.find('\n', p);
        if (e == std::string::npos) e = h.text.size();
        const std::string line = h.text.substr(p, e - p);
        if (line.rfind("@HD", 0) == 0) {
            size_t q = 0;
            while ((q = line.find('\t', q)) != std::string::npos) {
                ++q;
                if (line.compare(q, 3, "SO:") == 0) {
                    size_t t = line.find('\t', q);
                    sorted = line.substr(q + 3, t == std::string::npos ? t : t - q - 3) == "coordinate";
                }
            }
        }
        p = e + 1;
    }
    const bool mapped = !h.refs.empty();
    if (!mapped || !sorted) {
        fprintf(stderr, "ERROR: Methylation frequency could not be computed due to the following errors:\n");
        if (!mapped) fprintf(stderr, "BAM is not mapped\n");
        if (!sorted) fprintf(stderr, "BAM is not sorted\n");
        return false;
    }
    return true;
}

}  // namespace

// corr [-c min_cov] bed1 bed2 : Pearson correlation of the methylation frequencies of the loci two *.cov.bed files
// share (src/app/hifimeth/pileup_correlation.cpp:101-210): rows with pcov + ncov < min_cov (default 5) are dropped,
// loci are keyed by (chromosome id in order of first appearance over both files, start); host only, no GPU.
int cmd_corr(int argc, char** argv) {
    int min_cov = 5;
    int i = 2;
    for (; i < argc; ++i) {
        const std::string a = argv[i];
        if (a.size() < 2 || a[0] != '-') break;
        if (a == "-c" && i + 1 < argc) min_cov = atoi(argv[++i]);
        else { fprintf(stderr, "ERROR: unrecognised option %s", a.c_str()); return 1; }
    }
    if (argc - i != 2) {
        fprintf(stderr, "USAGE:\n  %s corr [-c <min coverage, default 5>] bed1 bed2\n", argv[0]);
        return 1;
    }
    fprintf(stderr, "\n\n====================> Parameters:\nmin-cov: %d\nbed1: %s\nbed2: %s\n\n\n", min_cov, argv[i], argv[i + 1]);
    std::vector<std::string> chr_names;
    auto chr_id = [&](const std::string& nm) {
        for (size_t k = 0; k < chr_names.size(); ++k)
            if (chr_names[k] == nm) return (uint64_t)k;
        chr_names.push_back(nm);
        return (uint64_t)chr_names.size() - 1;
    };
    auto load = [&](const char* path, std::vector<std::pair<uint64_t, double>>& out) {
        gzFile f = gzopen(path, "rb");
        if (!f) { fprintf(stderr, "ERROR: cannot open %s\n", path); return false; }
        static char line[1 << 16];
        std::string last;
        uint64_t sid = 0;
        while (gzgets(f, line, sizeof line)) {
            char* col[6];
            int nc = 0;
            char* p = line;
            col[nc++] = p;
            for (; *p && nc < 6; ++p)
                if (*p == '\t') { *p = 0; col[nc++] = p + 1; }
            if (nc < 6) continue;
            const int pcov = atoi(col[4]), ncov = atoi(col[5]);
            if (pcov + ncov < min_cov) continue;
            if (last != col[0]) { last = col[0]; sid = chr_id(last); }
            out.emplace_back((sid << 32) | (uint64_t)(uint32_t)atoi(col[1]), 1.0 * pcov / (pcov + ncov));
        }
        gzclose(f);
        return true;
    };
    std::vector<std::pair<uint64_t, double>> m1, m2;
    if (!load(argv[i], m1) || !load(argv[i + 1], m2)) return 1;
    auto by_key = [](const std::pair<uint64_t, double>& x, const std::pair<uint64_t, double>& y) { return x.first < y.first; };
    std::sort(m1.begin(), m1.end(), by_key);
    std::sort(m2.begin(), m2.end(), by_key);
    std::vector<double> x, y;
    for (size_t a = 0, b = 0; a < m1.size() && b < m2.size();) {
        if (m1[a].first < m2[b].first) ++a;
        else if (m1[a].first > m2[b].first) ++b;
        else { x.push_back(m1[a++].second); y.push_back(m2[b++].second); }
    }
    const size_t n = x.size();
    if (n < 5) { fprintf(stderr, "Intersect genomic loci is less than 5. Skip computation\n"); return 0; }
    double mx = 0, my = 0;
    for (size_t k = 0; k < n; ++k) { mx += x[k]; my += y[k]; }
    mx /= (double)n;
    my /= (double)n;
    double cov = 0, vx = 0, vy = 0;
    for (size_t k = 0; k < n; ++k) {
        const double dx = x[k] - mx, dy = y[k] - my;
        cov += dx * dy;
        vx += dx * dx;
        vy += dy * dy;
    }
    const double corr = (vx == 0 || vy == 0) ? 0.0 : cov / std::sqrt(vx * vy);
    fprintf(stdout, "Intersect loci: %zu\n", n);
    fprintf(stderr, "correlation: %g\n", corr);
    return 0;
}

// cov2bed REF.fa CONTEXT bismark.cov out.bed : 1-based Bismark coverage rows -> 0-based BED rows with a motif column
// (src/app/hifimeth/cov_to_bed.cpp).  Each input row "chr pos pos freq pcov ncov" is looked up on the reference and
// follows one rule of the table below: rows on a 'C' start a locus, rows on a 'G' either fold into the locus of the
// palindromic partner on the forward strand (CpG: one base left; CAG/CTG: two bases left) or stay where they are
// (CCG's partner CGG, every CHH motif, which is always named by its forward-strand spelling).  A chromosome's loci are
// written when the input moves on to another chromosome, as the reference does.  Neighbours outside the chromosome
// never match (the reference reads into the adjacent sequence there).  Host only, no GPU.
int cmd_cov2bed(int argc, char** argv) {
    if (argc != 6) {
        fprintf(stderr, "USAGE:\n%s %s reference context bismark-call bed\n", argv[0], argv[1]);
        return 1;
    }
    const std::string context = argv[3];
    int ctx = -1;
    if (context.size() == 3) {
        if (strcasecmp(context.c_str(), "CpG") == 0) ctx = 0;
        else if (strcasecmp(context.c_str(), "CHG") == 0) ctx = 1;
        else if (strcasecmp(context.c_str(), "CHH") == 0) ctx = 2;
    }
    if (ctx < 0) {
        fprintf(stderr, "Illegal 5mc context: %s\nPlausible contexts: CpG, CHG, CHH\n", context.c_str());
        return 1;
    }
    Fasta fa;
    std::string err;
    if (!load_fasta(argv[2], fa, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return EXIT_FAILURE; }
    std::vector<int64_t> start(fa.names.size() + 1, 0);
    for (size_t s = 0; s < fa.names.size(); ++s) start[s + 1] = start[s] + fa.length[s];

    // one rule: the row's own base, the 3-mer window it is matched against (offset of the window's first base relative
    // to the row), where the counts go (relative to the row), whether they replace or add, and the motif written
    struct Rule { char base; int win; const char* kmer; int dst; bool add; const char* motif; };
    static const Rule cpg[] = {{'C', 0, "CG", 0, false, "CG"}, {'G', -1, "CG", -1, true, "CG"}};
    static const Rule chg[] = {{'C', 0, "CCG", 0, false, "CCG"}, {'G', -2, "CGG", 0, false, "CCG"},
                               {'C', 0, "CAG", 0, false, "CAG"}, {'G', -2, "CAG", -2, true, "CAG"},
                               {'C', 0, "CTG", 0, false, "CTG"}, {'G', -2, "CTG", -2, true, "CTG"}};
    static const Rule chh[] = {{'C', 0, "CAA", 0, false, "CAA"}, {'C', 0, "CCA", 0, false, "CCA"}, {'C', 0, "CTA", 0, false, "CTA"},
                               {'C', 0, "CAC", 0, false, "CAC"}, {'C', 0, "CCC", 0, false, "CCC"}, {'C', 0, "CTC", 0, false, "CTC"},
                               {'C', 0, "CAT", 0, false, "CAT"}, {'C', 0, "CCT", 0, false, "CCT"}, {'C', 0, "CTT", 0, false, "CTT"},
                               {'G', -2, "TTG", 0, false, "CAA"}, {'G', -2, "TGG", 0, false, "CCA"}, {'G', -2, "TAG", 0, false, "CTA"},
                               {'G', -2, "GTG", 0, false, "CAC"}, {'G', -2, "GGG", 0, false, "CCC"}, {'G', -2, "GAG", 0, false, "CTC"},
                               {'G', -2, "ATG", 0, false, "CAT"}, {'G', -2, "AGG", 0, false, "CCT"}, {'G', -2, "AAG", 0, false, "CTT"}};
    const Rule* rules = ctx == 0 ? cpg : ctx == 1 ? chg : chh;
    const int n_rules = ctx == 0 ? 2 : ctx == 1 ? 6 : 18;

    struct Locus { int pcov, ncov; const char* motif; };
    std::vector<Locus> loci;
    FILE* out = fopen(argv[5], "w");
    if (!out) { fprintf(stderr, "ERROR: cannot open %s for writing\n", argv[5]); return EXIT_FAILURE; }
    gzFile in = gzopen(argv[4], "rb");
    if (!in) { fprintf(stderr, "ERROR: cannot open %s\n", argv[4]); fclose(out); return EXIT_FAILURE; }
    int cur = -1;
    bool bad = false;
    auto dump = [&]() {
        if (cur < 0) return;
        std::string text;
        char row[256];
        for (size_t i = 0; i < loci.size(); ++i) {
            const Locus& l = loci[i];
            if (!l.motif) continue;
            const int cov = l.pcov + l.ncov;
            if (cov <= 0) { fprintf(stderr, "ERROR: locus %s:%zu has no coverage\n", fa.names[cur].c_str(), i); bad = true; return; }
            const int len = snprintf(row, sizeof row, "\t%zu\t%zu\t%g\t%d\t%d\t%s\n", i, i + 1, 100.0 * l.pcov / cov, l.pcov, l.ncov, l.motif);
            text += fa.names[cur];
            text.append(row, (size_t)len);
        }
        fwrite(text.data(), 1, text.size(), out);
    };
    size_t fs = 0, rs = 0;
    static char line[1 << 16];
    std::string last_name;
    while (!bad && gzgets(in, line, sizeof line)) {
        size_t ll = strlen(line);
        while (ll && (line[ll - 1] == '\n' || line[ll - 1] == '\r')) line[--ll] = 0;
        char* col[6];
        int nc = 0;
        char* p = line;
        col[nc++] = p;
        for (; *p && nc < 6; ++p)
            if (*p == '\t') { *p = 0; col[nc++] = p + 1; }
        if (nc < 6) { fprintf(stderr, "ERROR: corrupted bismark record %s\n", line); bad = true; break; }
        if (cur < 0 || last_name != col[0]) {
            const int sid = fa.find(col[0]);
            if (sid < 0) { fprintf(stderr, "ERROR: sequence %s is not in %s\n", col[0], argv[2]); bad = true; break; }
            dump();
            if (bad) break;
            cur = sid;
            last_name = col[0];
            loci.assign((size_t)fa.length[sid], Locus{0, 0, nullptr});
        }
        const int64_t pos1 = atoll(col[1]);
        if (atoll(col[2]) != pos1) { fprintf(stderr, "ERROR: start and end differ: %s:%s-%s\n", col[0], col[1], col[2]); bad = true; break; }
        const int pcov = atoi(col[4]), ncov = atoi(col[5]);
        const int64_t len = fa.length[cur], soff = pos1 - 1;
        if (soff < 0 || soff >= len) { fprintf(stderr, "ERROR: position %s is outside %s\n", col[1], col[0]); bad = true; break; }
        const char* chr = fa.bases.data() + start[cur];
        for (int r = 0; r < n_rules; ++r) {
            const Rule& R = rules[r];
            if (chr[soff] != R.base) continue;
            const int k = (int)strlen(R.kmer);
            const int64_t w = soff + R.win;
            if (w < 0 || w + k > len || strncmp(chr + w, R.kmer, (size_t)k) != 0) continue;
            Locus& l = loci[(size_t)(soff + R.dst)];
            if (R.add) {
                l.pcov += pcov;
                l.ncov += ncov;
                if (!l.motif) l.motif = R.motif;
            } else {
                l = Locus{pcov, ncov, R.motif};
            }
            ++(R.base == 'C' ? fs : rs);
        }
    }
    gzclose(in);
    if (!bad) dump();
    fclose(out);
    if (bad) return EXIT_FAILURE;
    fprintf(stderr, "forward-strand-sites: %zu, reverse-strand-sites: %zu\n", fs, rs);
    return 0;
}

// sample [-s seed] REF.fa in.bam COVERAGE out.bam : random subset of the usable reads of an (unaligned) HiFi BAM adding
// up to COVERAGE x the reference size (src/app/hifimeth/subsample_bam.cpp).  A read is usable when it has >= 5000
// bases and all four kinetics arrays (:18-28); usable reads are shuffled, taken until the base target is reached (the
// read that crosses it included, :97-103) and written in input order (:105-117).  The reference seeds its shuffle from
// std::random_device, so which reads come out is not reproducible there either; `-s` (ours) fixes the seed for tests.
namespace {
std::string human_size(uint64_t bytes) {  // bytes_to_datasize (src/corelib/hbn_aux.cpp:447-490): 1024-based, <= 3 digits
    static const char* unit[] = {"B", "KB", "MB", "GB", "TB", "PB", "EB"};
    if (bytes == 0) return "0B";
    double v = (double)bytes;
    int u = 0;
    while (v >= 1024.0 && u < 6) { v /= 1024.0; ++u; }
    char buf[64];
    if (u == 0 || v >= 100) snprintf(buf, sizeof buf, "%llu", (unsigned long long)std::llround(v));
    else snprintf(buf, sizeof buf, v >= 10 ? "%.1f" : "%.2f", v);
    std::string r = buf;
    if (r.find('.') != std::string::npos) {
        r.erase(r.find_last_not_of('0') + 1);
        if (r.back() == '.') r.pop_back();
    }
    return r + unit[u];
}
}  // namespace

int cmd_sample(int argc, char** argv) {
    int a = 2;
    bool seeded = false;
    uint64_t seed = 0;
    if (argc >= 4 && std::string(argv[2]) == "-s") { seeded = true; seed = strtoull(argv[3], nullptr, 10); a = 4; }
    if (argc - a != 4) {
        fprintf(stderr, "USAGE:\n  %s %s [-s seed] reference input-bam coverage output-bam\n", argv[0], argv[1]);
        return 1;
    }
    const char* ref_path = argv[a];
    const char* in_path = argv[a + 1];
    const int cov = atoi(argv[a + 2]);
    const char* out_path = argv[a + 3];
    Fasta fa;
    std::string err;
    if (!load_fasta(ref_path, fa, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return EXIT_FAILURE; }
    const uint64_t dbsize = fa.bases.size(), target = dbsize * (uint64_t)std::max(cov, 0);

    struct Info { uint32_t id; int32_t length; bool valid, selected; };
    std::vector<Info> list;
    uint64_t total = 0;
    {
        BgzfReader in(in_path, 8);
        BamHeader h;
        if (!in.ok() || !read_header(in, h, err)) { fprintf(stderr, "ERROR: %s: %s\n", in_path, err.empty() ? "cannot open" : err.c_str()); return EXIT_FAILURE; }
        BamRecord r;
        while (read_record(in, r, err)) {
            Info f{(uint32_t)list.size(), r.l_qseq(), false, false};
            if (f.length >= 5000) {
                const KineticsView kv = kinetics_of(r);
                f.valid = kv.arr[0] && kv.arr[1] && kv.arr[2] && kv.arr[3];
            }
            if (f.valid) total += (uint64_t)f.length;
            list.push_back(f);
        }
        if (!err.empty()) { fprintf(stderr, "ERROR: %s: %s\n", in_path, err.c_str()); return EXIT_FAILURE; }
    }
    fprintf(stderr, "DB size: %s\ncoverage: %d, target size: %s\nBAM size: %s\n", human_size(dbsize).c_str(), cov,
            human_size(target).c_str(), human_size(total).c_str());
    std::mt19937 gen(seeded ? (uint32_t)seed : std::random_device{}());
    std::shuffle(list.begin(), list.end(), gen);
    uint64_t picked = 0;
    for (Info& f : list) {
        if (!f.valid) continue;
        picked += (uint64_t)f.length;
        f.selected = true;
        if (picked >= target) break;
    }
    std::sort(list.begin(), list.end(), [](const Info& x, const Info& y) { return x.id < y.id; });

    BgzfReader in(in_path, 8);
    BamHeader h;
    if (!in.ok() || !read_header(in, h, err)) { fprintf(stderr, "ERROR: %s: %s\n", in_path, err.c_str()); return EXIT_FAILURE; }
    BgzfWriter out(out_path, 8, 6);
    if (!out.ok()) { fprintf(stderr, "ERROR: cannot open %s for writing\n", out_path); return EXIT_FAILURE; }
    write_header(out, h);
    BamRecord r;
    size_t id = 0;
    int reads = 0;
    uint64_t bases = 0;
    while (read_record(in, r, err)) {
        if (id >= list.size()) { fprintf(stderr, "ERROR: %s changed between the two passes\n", in_path); return EXIT_FAILURE; }
        const Info& f = list[id++];
        if (!f.valid || !f.selected) continue;
        write_record(out, r);
        ++reads;
        bases += (uint64_t)f.length;
    }
    if (!err.empty() || !out.close()) { fprintf(stderr, "ERROR: %s\n", err.empty() ? "write failed" : err.c_str()); return EXIT_FAILURE; }
    fprintf(stderr, "Target: %s\nExtracted reads: %d (%s)\n", human_size(target).c_str(), reads, human_size(bases).c_str());
    return 0;
}

// eval [-s seed] [-d DUMP.json] [-g device] REF.fa bismark.bed mod.bam PREFIX : read-level benchmark samples
// (src/app/hifimeth/eval.cpp).  Truth labels come from a 0-based Bismark BED (rows with >= 10 reads: all unmethylated -> 0,
// all methylated -> 1, :103-112); every 5mC call of a mapped read that projects onto a labelled locus -- the same
// CpG / CHG / CHH walks as `pileup` (:503-560), here on the GPU through the pileup engine -- becomes one (label,
// probability) sample.  Per context: CHH negatives are thinned to one in ten (:556), small sample sets are replicated
// (:350-440), and five files PREFIX.<ctx>.<i> receive 100 000 positives and 100 000 negatives each, drawn without
// replacement, as "label<TAB>prediction<TAB>probability" (:580-611).  The reference draws with random_device seeds, so
// its files are not reproducible; the counts behind them are: `-d` (ours) writes the thresholds and the
// counts[context][label][scaled_prob] table before thinning, `-s` (ours) fixes the seed of every draw.
int cmd_eval(int argc, char** argv) {
    uint64_t seed = std::random_device{}();
    std::string dump_path;
    int device = 0;
    int a = 2;
    for (; a + 1 < argc && argv[a][0] == '-' && argv[a][1]; a += 2) {
        const std::string k = argv[a];
        if (k == "-s") seed = strtoull(argv[a + 1], nullptr, 10);
        else if (k == "-d") dump_path = argv[a + 1];
        else if (k == "-g") device = atoi(argv[a + 1]);
        else { fprintf(stderr, "ERROR: unrecognised option %s\n", argv[a]); return 1; }
    }
    if (argc - a != 4) {
        fprintf(stderr, "USAGE:\n%s %s [-s seed] [-d counts.json] [-g device] reference bismark mod-bam output-prefix\n", argv[0], argv[1]);
        return 1;
    }
    const char* ref_path = argv[a];
    const char* bed_path = argv[a + 1];
    const char* bam_path = argv[a + 2];
    const std::string prefix = argv[a + 3];
    constexpr uint64_t kTarget = 100000;
    static const char* cn[3] = {"CpG", "CHG", "CHH"};

    Fasta fa;
    std::string err;
    if (!load_fasta(ref_path, fa, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return EXIT_FAILURE; }
    if (fa.names.empty()) { fprintf(stderr, "ERROR: no sequence in %s\n", ref_path); return EXIT_FAILURE; }
    std::vector<int64_t> start(fa.names.size() + 1, 0);
    for (size_t s = 0; s < fa.names.size(); ++s) start[s + 1] = start[s] + fa.length[s];

    // truth labels (s_fill_chr_base_label_with_bismark, eval.cpp:42-114)
    std::vector<int8_t> labels(fa.bases.size(), (int8_t)-1);
    {
        gzFile in = gzopen(bed_path, "rb");
        if (!in) { fprintf(stderr, "ERROR: cannot open %s\n", bed_path); return EXIT_FAILURE; }
        static char line[1 << 16];
        std::string last;
        int sid = -1;
        size_t np = 0, nn = 0;
        while (gzgets(in, line, sizeof line)) {
            size_t ll = strlen(line);
            while (ll && (line[ll - 1] == '\n' || line[ll - 1] == '\r')) line[--ll] = 0;
            if (!ll) continue;
            char* col[6];
            int nc = 0;
            char* p = line;
            col[nc++] = p;
            for (; *p && nc < 6; ++p)
                if (*p == '\t') { *p = 0; col[nc++] = p + 1; }
            if (nc < 6) { fprintf(stderr, "ERROR: corrupted bismark record %s\n", line); gzclose(in); return EXIT_FAILURE; }
            if (sid < 0 || last != col[0]) {
                last = col[0];
                sid = fa.find(last);
                if (sid < 0) { fprintf(stderr, "ERROR: sequence %s is not in %s\n", col[0], ref_path); gzclose(in); return EXIT_FAILURE; }
            }
            const int64_t soff = atoll(col[1]), send = atoll(col[2]);
            if (send - soff != 1 || soff < 0 || soff >= fa.length[(size_t)sid]) {
                fprintf(stderr, "ERROR: bad interval %s:%s-%s\n", col[0], col[1], col[2]);
                gzclose(in);
                return EXIT_FAILURE;
            }
            const int pcov = atoi(col[4]), ncov = atoi(col[5]);
            if (pcov + ncov < 10) continue;
            if (pcov == 0) { labels[(size_t)(start[(size_t)sid] + soff)] = 0; ++nn; }
            else if (ncov == 0) { labels[(size_t)(start[(size_t)sid] + soff)] = 1; ++np; }
        }
        gzclose(in);
        fprintf(stderr, "Load %zu methylated sites and %zu unmethylated sites from %s\n", np, nn, bed_path);
    }

    BgzfReader in(bam_path, 8);
    BamHeader hdr;
    if (!in.ok() || !read_header(in, hdr, err)) { fprintf(stderr, "ERROR: %s%s\n", in.error().c_str(), err.c_str()); return EXIT_FAILURE; }
    std::vector<int> tid2sid(hdr.refs.size(), -2);
    hm_pileup_t* pe = nullptr;
    if (hm_pileup_create(&pe, device) != HM_OK) { fprintf(stderr, "ERROR: %s\n", hm_pileup_last_error(nullptr)); return EXIT_FAILURE; }
    auto die = [&](const std::string& what) {
        fprintf(stderr, "ERROR: %s: %s\n", what.c_str(), hm_pileup_last_error(pe));
        hm_pileup_destroy(pe);
        return EXIT_FAILURE;
    };
    if (hm_pileup_set_reference(pe, (int32_t)fa.names.size(), fa.length.data(), fa.bases.data()) != HM_OK) return die("reference");

    // one pass: the threshold histograms count every primary record with calls, mapped or not (s_prob_bin_thread,
    // eval.cpp:153-211) -- the engine counts the records it is given, the unmapped ones are counted here --; the samples
    // come from the mapped ones, without mapQ / identity filters (:484-489)
    static uint64_t extra[768];
    std::fill(extra, extra + 768, 0);
    constexpr int kBatch = 512;
    std::vector<BamRecord> recs((size_t)kBatch);
    std::vector<std::vector<BaseMod>> mods((size_t)kBatch);
    std::vector<std::string> perr((size_t)kBatch);
    std::vector<uint32_t> cig;
    uint64_t order = 0;
    bool more = true;
    while (more) {
        int n = 0;
        while (n < kBatch && (more = read_record(in, recs[(size_t)n], err))) ++n;
        if (!err.empty()) { fprintf(stderr, "ERROR: Could not read BAM record: %s\n", err.c_str()); hm_pileup_destroy(pe); return EXIT_FAILURE; }
        parallel_run(n, 8, [&](int k) {
            mods[(size_t)k].clear();
            perr[(size_t)k].clear();
            if (!parse_mods(recs[(size_t)k], mods[(size_t)k], perr[(size_t)k])) mods[(size_t)k].clear();
        });
        for (int k = 0; k < n; ++k, ++order) {
            const BamRecord& r = recs[(size_t)k];
            if (!perr[(size_t)k].empty()) {
                fprintf(stderr, "ERROR at parsing read %s\n%s\n", reinterpret_cast<const char*>(r.data.data() + 32), perr[(size_t)k].c_str());
                hm_pileup_destroy(pe);
                return EXIT_FAILURE;
            }
            if (mods[(size_t)k].empty()) continue;
            if (r.flag() & 4) {
                if (!(r.flag() & 0x900))
                    for (const BaseMod& m : mods[(size_t)k]) {
                        const int c = mod_context(r, m.qoff);
                        if (c >= 0) ++extra[c * 256 + m.prob];
                    }
                continue;
            }
            const int tid = r.ref_id();
            if (tid < 0 || tid >= (int)hdr.refs.size()) { fprintf(stderr, "ERROR: mapped record without a reference id\n"); hm_pileup_destroy(pe); return EXIT_FAILURE; }
            if (tid2sid[(size_t)tid] == -2) tid2sid[(size_t)tid] = fa.find(hdr.refs[(size_t)tid].first);
            if (tid2sid[(size_t)tid] < 0) {
                fprintf(stderr, "ERROR: Sequence name %s does not exist\n", hdr.refs[(size_t)tid].first.c_str());
                hm_pileup_destroy(pe);
                return EXIT_FAILURE;
            }
            real_cigar(r, cig);
            if (hm_pileup_submit_read(pe, (uint32_t)order, r.flag(), tid2sid[(size_t)tid], r.pos(), r.mapq(), r.l_qseq(), r.seq4(),
                                      (int32_t)cig.size(), cig.data(), (int64_t)mods[(size_t)k].size(), mods[(size_t)k].data()) < 0)
                return die(std::string("read ") + reinterpret_cast<const char*>(r.data.data() + 32));
        }
        if (hm_pileup_run(pe) != HM_OK) return die("projection");
    }
    static uint64_t bins[768];
    if (hm_pileup_histograms(pe, bins) != HM_OK) return die("histograms");
    for (int i = 0; i < 768; ++i) bins[i] += extra[i];
    uint8_t thr[3];
    report_thresholds(bins, thr);

    static uint64_t cnt[1536];  // [ctx][label][prob]
    if (hm_pileup_label_histograms(pe, labels.data(), (int64_t)labels.size(), cnt) != HM_OK) return die("labels");
    hm_pileup_destroy(pe);
    if (!dump_path.empty()) {
        FILE* f = fopen(dump_path.c_str(), "w");
        if (!f) { fprintf(stderr, "ERROR: cannot open %s for writing\n", dump_path.c_str()); return EXIT_FAILURE; }
        fprintf(f, "{\"thresholds\": [%d, %d, %d], \"counts\": [", thr[0], thr[1], thr[2]);
        for (int i = 0; i < 1536; ++i) fprintf(f, "%s%llu", i ? ", " : "", (unsigned long long)cnt[i]);
        fprintf(f, "]}\n");
        fclose(f);
    }

    std::mt19937_64 gen(seed);
    for (int c = 0; c < 3; ++c) {
        uint64_t* neg = cnt + (c * 2 + 0) * 256;
        uint64_t* pos = cnt + (c * 2 + 1) * 256;
        if (c == 2)  // every unmethylated CHH sample is kept with probability 0.1 (:556)
            for (int i = 0; i < 256; ++i)
                if (neg[i]) neg[i] = std::binomial_distribution<uint64_t>(neg[i], 0.1)(gen);
        uint64_t total[2] = {0, 0};
        for (int i = 0; i < 256; ++i) { total[0] += neg[i]; total[1] += pos[i]; }
        for (int l = 1; l >= 0; --l) {  // over_sampling_eval_samples (:350-440): positives first, as the messages come
            uint64_t* h = l ? pos : neg;
            if (total[l] > 0 && total[l] < kTarget) {
                fprintf(stderr, "Original %s %s samples: %llu\n", cn[c], l ? "positive" : "negative", (unsigned long long)total[l]);
                const uint64_t x = 2 * kTarget / total[l] * 2;
                for (int i = 0; i < 256; ++i) h[i] *= x;
                total[l] *= x;
                fprintf(stderr, "Over-sampled %s %s samples: %llu\n", cn[c], l ? "positive" : "negative", (unsigned long long)total[l]);
            }
        }
        if (total[0] == 0 || total[1] == 0) continue;
        fprintf(stderr, "%s positive samples: %llu, negative samples: %llu\n", cn[c], (unsigned long long)total[1], (unsigned long long)total[0]);
        // kTarget samples without replacement from a multiset given by its histogram: distinct ranks (Floyd), rank -> bin
        auto draw = [&](const uint64_t* h, uint64_t n, std::vector<uint8_t>& out) {
            std::vector<uint64_t> cum(257, 0);
            for (int i = 0; i < 256; ++i) cum[(size_t)i + 1] = cum[(size_t)i] + h[i];
            std::vector<uint64_t> picks;
            picks.reserve(kTarget);
            std::unordered_set<uint64_t> seen;
            seen.reserve(2 * kTarget);
            for (uint64_t j = n - kTarget; j < n; ++j) {
                const uint64_t t = std::uniform_int_distribution<uint64_t>(0, j)(gen);
                const uint64_t v = seen.insert(t).second ? t : j;
                if (v == j && t != j) seen.insert(j);
                picks.push_back(v);
            }
            std::shuffle(picks.begin(), picks.end(), gen);
            out.clear();
            for (uint64_t r : picks) out.push_back((uint8_t)(std::upper_bound(cum.begin(), cum.end(), r) - cum.begin() - 1));
        };
        std::vector<uint8_t> sp, sn;
        for (int i = 0; i < 5; ++i) {  // s_dump_samples (:580-611)
            const std::string path = prefix + "." + cn[c] + "." + std::to_string(i);
            FILE* f = fopen(path.c_str(), "w");
            if (!f) { fprintf(stderr, "ERROR: cannot open %s for writing\n", path.c_str()); return EXIT_FAILURE; }
            draw(pos, total[1], sp);
            draw(neg, total[0], sn);
            for (uint8_t v : sp) fprintf(f, "1\t%d\t%g\n", v >= thr[c] ? 1 : 0, 1.0 * v / 255);
            for (uint8_t v : sn) fprintf(f, "0\t%d\t%g\n", v >= thr[c] ? 1 : 0, 1.0 * v / 255);
            fclose(f);
        }
    }
    return 0;
}

// fastats REF.fa : names, lengths and a checksum of the loaded reference as one JSON object (loader tests; no GPU)
int cmd_fastats(int argc, char** argv) {
    if (argc != 3) return EXIT_FAILURE;
    Fasta fa;
    std::string err;
    if (!load_fasta(argv[2], fa, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return EXIT_FAILURE; }
    printf("{\"seqs\": [");
    size_t off = 0;
    for (size_t i = 0; i < fa.names.size(); ++i) {
        uint64_t h = 1469598103934665603ull;  // FNV-1a over the upper-cased bases
        for (int64_t k = 0; k < fa.length[i]; ++k) h = (h ^ (uint8_t)fa.bases[off + (size_t)k]) * 1099511628211ull;
        off += (size_t)fa.length[i];
        printf("%s{\"name\": \"%s\", \"length\": %lld, \"fnv1a\": \"%016llx\"}", i ? ", " : "", fa.names[i].c_str(),
               (long long)fa.length[i], (unsigned long long)h);
    }
    printf("]}\n");
    return 0;
}

// test seam: the threshold resolver of `pileup` / `eval` on histograms from stdin (n, then n x 3 x 256 counts -> n lines
// "cpg chg chh"); tests/golden/pileup_thresholds.json holds the reference's own answers for the same input format
int cmd_thresholds(int, char**) {
    int n = 0;
    if (scanf("%d", &n) != 1) return EXIT_FAILURE;
    for (int c = 0; c < n; ++c) {
        uint64_t bins[3][256];
        for (auto& b : bins)
            for (auto& v : b) {
                unsigned long long x = 0;
                if (scanf("%llu", &x) != 1) return EXIT_FAILURE;
                v = x;
            }
        uint64_t samples = 0;
        printf("%d %d %d\n", resolve_threshold(bins[0], &samples), resolve_threshold(bins[1], &samples), resolve_threshold(bins[2], &samples));
    }
    return 0;
}

namespace {
// s_resolve_scaled_prob_threshold (pileup.cpp:355-436, eval.cpp:213-305): the three thresholds with the reference's messages
void report_thresholds(const uint64_t* bins, uint8_t thr[3]) {
    static const char* cn[3] = {"CpG", "CHG", "CHH"};
    for (int c = 0; c < 3; ++c) {
        uint64_t samples = 0;
        const int t = resolve_threshold(bins + 256 * c, &samples);
        fprintf(stderr, "%s samples: %llu\n", cn[c], (unsigned long long)samples);
        const uint64_t* a = bins + 256 * c;  // the fallback branch: window narrower than 50 bins or < 10000 samples
        int st = 20, en = 256 - 20;
        while (st < 256 && a[st] < 10) ++st;
        while (en && a[en - 1] < 10) --en;
        const bool fallback = samples < 10000 || en - st < 50;
        if (fallback) fprintf(stderr, "Not enough samples for inferring scaled probability threshold, set it to 128\n");
        else fprintf(stderr, "%s scaled probability threshold: %d\n", cn[c], t);
        thr[c] = (uint8_t)t;
    }
}
}  // namespace

namespace {
// the locus a row is named by
template <class Row>
int64_t row_pos(const Row& r) { return r.gpos; }
inline int64_t row_pos(const hm_domain_t& r) { return r.start; }
inline int64_t row_pos(const hm_pattern_t& r) { return r.start; }
// ... and the context whose file it goes to
template <class Row>
uint32_t row_ctx(const Row& r) { return r.motif < 3 ? r.motif : 2; }
inline uint32_t row_ctx(const hm_pattern_t&) { return 0; }
inline uint32_t row_ctx(const hm_bedmethyl_t&) { return 0; }

// The three files <prefix>.<tag><ctx>.<suffix> of one output, closed when their owner goes.
struct CtxFiles {
    FILE* f[3] = {nullptr, nullptr, nullptr};
    CtxFiles() = default;
    CtxFiles(const CtxFiles&) = delete;
    CtxFiles& operator=(const CtxFiles&) = delete;
    ~CtxFiles() {
        for (FILE* x : f)
            if (x) fclose(x);
    }
    // false (message printed) if one of them cannot be opened
    bool open(const std::string& prefix, const std::string& tag, const char* suffix) {
        static const char* cn[3] = {"CpG", "CHG", "CHH"};
        for (int c = 0; c < 3; ++c) {
            const std::string path = prefix + "." + tag + cn[c] + suffix;
            if ((f[c] = fopen(path.c_str(), "w"))) continue;
            fprintf(stderr, "ERROR: cannot open %s for writing\n", path.c_str());
            return false;
        }
        return true;
    }
};

// The rows of three per-context BED files, sequence by sequence.  fetch(lo, hi, dst, cap) is the engine's row fetch over the
// plane range of one sequence (dst NULL: the number of rows only); format(row, k, buf) prints the columns behind the sequence
// name of a row at offset k and returns their length; the file of a row is its motif.  Rows are formatted by `threads` workers
// over contiguous slices and written slice by slice (pileup.cpp:562-590).  false on an engine error (hm_pileup_last_error).
template <class Row, class Fetch, class Format>
bool write_rows(const Fasta& fa, FILE* const out[3], int threads, Fetch fetch, Format format) {
    std::vector<Row> rows;
    const int fmt_threads = std::max(1, threads);
    std::vector<std::string> text((size_t)fmt_threads * 3);
    int64_t off = 0;
    for (size_t s = 0; s < fa.names.size(); ++s) {
        const int64_t lo = off, hi = off + fa.length[s];
        off = hi;
        int64_t n = fetch(lo, hi, static_cast<Row*>(nullptr), 0);
        if (n > 0) {
            rows.resize((size_t)n);
            n = fetch(lo, hi, rows.data(), n);
        }
        if (n < 0) return false;
        if (n == 0) continue;
        parallel_run(fmt_threads, fmt_threads, [&](int w) {
            for (int c = 0; c < 3; ++c) text[(size_t)w * 3 + c].clear();
            const size_t a = (size_t)n * w / fmt_threads, b = (size_t)n * (w + 1) / fmt_threads;
            char buf[320];
            for (size_t i = a; i < b; ++i) {
                const Row& r = rows[i];
                const int len = format(r, row_pos(r) - lo, buf);
                std::string& t = text[(size_t)w * 3 + row_ctx(r)];
                t += fa.names[s];
                t.append(buf, (size_t)len);
            }
        });
        for (int c = 0; c < 3; ++c)
            for (int w = 0; w < fmt_threads; ++w) {
                const std::string& t = text[(size_t)w * 3 + c];
                if (!t.empty()) fwrite(t.data(), 1, t.size(), out[c]);
            }
    }
    return true;
}

// rows of the three <prefix>.<ctx>.cov.bed files (pileup.cpp:562-590) from planes (pcov, ncov, key): all NULL = the
// engine's own combined planes, else DEVICE planes over the whole concatenated reference.  The context of a row is the
// key's motif.  false on an engine error (hm_pileup_last_error).
bool write_bed(hm_pileup_t* pe, const Fasta& fa, const void* pcov, const void* ncov, const void* key, FILE* out[3], int threads) {
    return write_rows<hm_locus_t>(
        fa, out, threads,
        [&](int64_t lo, int64_t hi, hm_locus_t* dst, int64_t cap) { return hm_pileup_fetch_loci(pe, pcov, ncov, key, 0, lo, hi, dst, cap); },
        [](const hm_locus_t& l, int64_t k, char (&buf)[320]) {
            const double freq = 100.0 * l.pcov / (l.pcov + l.ncov);
            return snprintf(buf, sizeof buf, "\t%lld\t%lld\t%g\t%d\t%d\n", (long long)k, (long long)k + 1, freq, l.pcov, l.ncov);
        });
}

// rows of the three <prefix>.asm.<ctx>.bed files from the engine's own partition and key planes (48 B per tested row on the
// device and here).  false on an engine error.
bool write_asm(hm_pileup_t* pe, const Fasta& fa, int min_cov, FILE* out[3], int threads) {
    return write_rows<hm_asm_t>(
        fa, out, threads,
        [&](int64_t lo, int64_t hi, hm_asm_t* dst, int64_t cap) {
            return hm_pileup_fetch_asm(pe, nullptr, nullptr, nullptr, nullptr, nullptr, 0, lo, hi, min_cov, dst, cap);
        },
        [](const hm_asm_t& r, int64_t k, char (&buf)[320]) {
            return snprintf(buf, sizeof buf, "\t%lld\t%lld\t%g\t%.6g\t%d\t%d\t%d\t%d\n", (long long)k, (long long)k + 1, r.diff, r.pvalue,
                            r.pcov1, r.ncov1, r.pcov2, r.ncov2);
        });
}

// rows of the three <prefix>.asm.regions.<ctx>.bed files, sequence by sequence: a region never crosses a sequence.  false on an
// engine error.
bool write_asm_regions(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, FILE* out[3]) {
    std::vector<hm_asm_region_t> rows;
    int64_t off = 0;
    for (size_t s = 0; s < fa.names.size(); ++s) {
        const int64_t lo = off, hi = off + fa.length[s];
        off = hi;
        for (int c = 0; c < 3; ++c) {
            const auto fetch = [&](hm_asm_region_t* dst, int64_t cap) {
                return hm_pileup_fetch_asm_regions(pe, nullptr, nullptr, nullptr, nullptr, nullptr, 0, lo, hi, o.asm_min_cov, c, o.region_max_p,
                                                   o.region_max_gap, o.region_min_loci, 0, nullptr, dst, cap);
            };
            int64_t n = fetch(nullptr, 0);
            if (n > 0) {
                rows.resize((size_t)n);
                n = fetch(rows.data(), n);
            }
            if (n < 0) return false;
            for (int64_t i = 0; i < n; ++i) {
                const hm_asm_region_t& r = rows[(size_t)i];
                fprintf(out[c], "%s\t%lld\t%lld\t%d\t%c\t%g\t%.6g\t%lld\t%lld\t%lld\t%lld\n", fa.names[s].c_str(), (long long)(r.start - lo),
                        (long long)(r.end - lo), r.n_loci, r.sign > 0 ? '+' : '-', r.diff, r.pmin, (long long)r.pcov1, (long long)r.ncov1,
                        (long long)r.pcov2, (long long)r.ncov2);
            }
        }
    }
    return true;
}

// rows of <prefix>.patterns.CpG.bed (out[0]; a window never crosses a sequence): the statistics are hm_pattern_stats'.  false on an
// engine error.
bool write_patterns(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, FILE* out[3]) {
    return write_rows<hm_pattern_t>(
        fa, out, o.threads,
        [&](int64_t lo, int64_t hi, hm_pattern_t* dst, int64_t cap) { return hm_pileup_fetch_patterns(pe, lo, hi, o.pattern_min_reads, dst, cap); },
        [](const hm_pattern_t& r, int64_t k, char (&buf)[320]) {
            double st[4] = {0, 0, 0, 0};
            hm_pattern_stats(&r, st);
            int len = snprintf(buf, sizeof buf, "\t%lld\t%lld\t%u\t%.6g\t%.6g\t%.6g\t%.6g", (long long)k, (long long)(k + (r.end - r.start)), r.n,
                               st[0], st[1], st[2], st[3]);
            for (uint32_t b = 0; b < (1u << r.k); ++b) len += snprintf(buf + len, sizeof buf - (size_t)len, "%c%u", b ? ',' : '\t', r.counts[b]);
            len += snprintf(buf + len, sizeof buf - (size_t)len, "\n");
            return len;
        });
}

// rows of <prefix>[.hapN].bedmethyl.CpG.bed (out[0]) from set `part` of the depth counters.  false on an engine error.
bool write_bedmethyl(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, int part, FILE* out[3]) {
    return write_rows<hm_bedmethyl_t>(
        fa, out, o.threads,
        [&](int64_t lo, int64_t hi, hm_bedmethyl_t* dst, int64_t cap) { return hm_pileup_fetch_bedmethyl(pe, part, lo, hi, o.bedmethyl_min_valid, dst, cap); },
        [](const hm_bedmethyl_t& r, int64_t k, char (&buf)[320]) {
            const unsigned long long valid = (unsigned long long)r.n_mod + r.n_canon;
            const double percent = valid ? 100.0 * (double)r.n_mod / (double)valid : 0.0;
            return snprintf(buf, sizeof buf, "\t%lld\t%lld\tm\t%llu\t.\t%lld\t%lld\t255,0,0\t%llu\t%.2f\t%u\t%u\t0\t%u\t0\t%u\t%u\n", (long long)k,
                            (long long)k + 1, std::min(1000ull, valid), (long long)k, (long long)k + 1, valid, percent, r.n_mod, r.n_canon,
                            r.n_delete, r.n_diff, r.n_nocall);
        });
}

// <prefix>.linkage.CpG.tsv: the header, then one row per distance with at least -z pairs; the statistics are hm_linkage_stats'
// (a distance without pairs, written under -z 0, has none: nan).  false on an engine error (recorded) or a file error (reported).
bool write_linkage(hm_pileup_t* pe, const PileupOptions& o) {
    std::vector<hm_linkage_t> rows((size_t)o.linkage);
    const int64_t n = hm_pileup_fetch_linkage(pe, o.linkage_min_pairs, rows.data(), (int64_t)rows.size());
    if (n < 0) return false;
    const std::string path = o.prefix + ".linkage.CpG.tsv";
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "ERROR: cannot open %s for writing\n", path.c_str()); return false; }
    fprintf(f, "#dist\tn\tn_uu\tn_um\tn_mu\tn_mm\tconcordance\tr\n");
    for (int64_t i = 0; i < n; ++i) {
        const hm_linkage_t& r = rows[(size_t)i];
        double st[2] = {NAN, NAN};
        hm_linkage_stats(&r, st);
        fprintf(f, "%u\t%llu\t%llu\t%llu\t%llu\t%llu\t%.6g\t%.6g\n", r.dist, (unsigned long long)(r.n_uu + r.n_um + r.n_mu + r.n_mm),
                (unsigned long long)r.n_uu, (unsigned long long)r.n_um, (unsigned long long)r.n_mu, (unsigned long long)r.n_mm, st[0], st[1]);
    }
    return fclose(f) == 0;
}

// <prefix>.readpos.tsv: the header, then one row per context and bin with at least -y calls; percent as cov.bed's fourth column,
// both statistics hm_readpos_stats' (a row without calls, written under -y 0, has none: nan).  false on an engine error (recorded)
// or a file error (reported).
bool write_readpos(hm_pileup_t* pe, const PileupOptions& o) {
    std::vector<hm_readpos_t> rows(3 * (2 * (size_t)o.profile + 1));
    const int64_t n = hm_pileup_fetch_readpos(pe, o.profile_min_calls, rows.data(), (int64_t)rows.size());
    if (n < 0) return false;
    const std::string path = o.prefix + ".readpos.tsv";
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "ERROR: cannot open %s for writing\n", path.c_str()); return false; }
    static const char* const ctx[3] = {"CpG", "CHG", "CHH"};
    static const char* const end[3] = {"5p", "3p", "interior"};
    fprintf(f, "#context\tend\tdist\tn\tn_m\tn_u\tpercent\tmean_ml\n");
    for (int64_t i = 0; i < n; ++i) {
        const hm_readpos_t& r = rows[(size_t)i];
        double st[2] = {NAN, NAN};
        hm_readpos_stats(&r, st);
        fprintf(f, "%s\t%s\t%u\t%llu\t%llu\t%llu\t%g\t%.6g\n", ctx[r.motif % 3], end[r.end % 3], r.dist, (unsigned long long)(r.n_m + r.n_u),
                (unsigned long long)r.n_m, (unsigned long long)r.n_u, st[0], st[1]);
    }
    return fclose(f) == 0;
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

// -R: the intervals of a BED file in input order, in sequence coordinates
struct Intervals {
    std::vector<int> sid;
    std::vector<int64_t> start, end;
    std::vector<std::string> name;
    std::string strand;  // '+', '-' or '.' per interval
};

// Plain or gzip, at least 3 tab-separated columns; empty lines and lines starting with #, track or browser are skipped; the name is
// column 4 or ".", the strand column 6 if it is + or -, else ".".  false (message naming the line printed) for a file that cannot
// be read, too few columns, coordinates that are no integers, an unknown sequence, start < 0, start >= end, end > the sequence.
bool read_intervals(const std::string& path, const Fasta& fa, Intervals& iv) {
    gzFile in = gzopen(path.c_str(), "rb");
    if (!in) { fprintf(stderr, "ERROR: cannot open %s (-R)\n", path.c_str()); return false; }
    std::string line;
    char buf[4096];
    long long no = 0;
    bool ok = true;
    auto bad = [&](const std::string& what) {
        fprintf(stderr, "ERROR: %s:%lld: %s\n", path.c_str(), no, what.c_str());
        return ok = false;
    };
    while (ok) {
        line.clear();
        bool got = false;
        while (gzgets(in, buf, sizeof buf)) {  // a line of any length
            got = true;
            line += buf;
            if (!line.empty() && line.back() == '\n') break;
        }
        if (!got) break;
        ++no;
        while (!line.empty() && (line.back() == '\n' || line.back() == '\r')) line.pop_back();
        if (line.empty() || line[0] == '#' || line.compare(0, 5, "track") == 0 || line.compare(0, 7, "browser") == 0) continue;
        std::vector<std::string> col;
        for (size_t a = 0;;) {
            const size_t b = line.find('\t', a);
            col.push_back(line.substr(a, b == std::string::npos ? b : b - a));
            if (b == std::string::npos) break;
            a = b + 1;
        }
        if (col.size() < 3) { bad("fewer than 3 tab-separated columns"); break; }
        long long x[2];
        bool numbers = true;
        for (int k = 0; k < 2; ++k) {
            char* end = nullptr;
            errno = 0;
            x[k] = strtoll(col[(size_t)k + 1].c_str(), &end, 10);
            if (end == col[(size_t)k + 1].c_str() || *end || errno) numbers = false;
        }
        if (!numbers) { bad("start and end must be integers"); break; }
        const int sid = fa.find(col[0]);
        if (sid < 0) { bad("unknown sequence " + col[0]); break; }
        if (x[0] < 0) { bad("start < 0"); break; }
        if (x[0] >= x[1]) { bad("start >= end"); break; }
        if (x[1] > fa.length[(size_t)sid]) { bad("end " + std::to_string(x[1]) + " is past the end of " + col[0] + " (" + std::to_string(fa.length[(size_t)sid]) + ")"); break; }
        iv.sid.push_back(sid);
        iv.start.push_back(x[0]);
        iv.end.push_back(x[1]);
        iv.name.push_back(col.size() > 3 && !col[3].empty() ? col[3] : ".");
        iv.strand.push_back(col.size() > 5 && (col[5] == "+" || col[5] == "-") ? col[5][0] : '.');
    }
    gzclose(in);
    return ok;
}

// n_loci, pcov, ncov, weighted, mean: the columns both interval outputs end with; the percentages hm_region_stats', nan without a locus
void print_region_columns(FILE* f, const hm_region_sum_t& r) {
    double st[2];
    if (hm_region_stats(&r, st) == HM_OK) fprintf(f, "%lld\t%lld\t%lld\t%.6g\t%.6g\n", (long long)r.n_loci, (long long)r.pcov, (long long)r.ncov, st[0], st[1]);
    else fprintf(f, "%lld\t%lld\t%lld\tnan\tnan\n", (long long)r.n_loci, (long long)r.pcov, (long long)r.ncov);
}

// <prefix>.<tag>regions.<ctx>.tsv and, under -J, <prefix>.<tag>metaplot.<ctx>.tsv from one set of planes (NULL: the engine's own).
// false on an engine error (recorded) or a file error (reported).
bool write_intervals(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, const Intervals& iv, const std::string& tag, const void* const planes[3]) {
    std::vector<int64_t> off(fa.length.size() + 1, 0);
    for (size_t i = 0; i < fa.length.size(); ++i) off[i + 1] = off[i] + fa.length[i];
    const size_t n = iv.sid.size();
    std::vector<int64_t> start(n), end(n), s0(n), s1(n);
    for (size_t i = 0; i < n; ++i) {
        s0[i] = off[(size_t)iv.sid[i]];
        s1[i] = off[(size_t)iv.sid[i] + 1];
        start[i] = s0[i] + iv.start[i];
        end[i] = s0[i] + iv.end[i];
    }
    std::vector<hm_region_sum_t> sums(3 * n);
    if (hm_pileup_fetch_regions(pe, planes[0], planes[1], planes[2], 0, 0, off.back(), o.interval_min_cov, start.data(), end.data(), (int64_t)n,
                                sums.data()) != HM_OK)
        return false;
    {
        CtxFiles out;
        if (!out.open(o.prefix, tag + "regions.", ".tsv")) return false;
        for (int c = 0; c < 3; ++c) {
            fprintf(out.f[c], "#chrom\tstart\tend\tname\tstrand\tn_loci\tpcov\tncov\tweighted\tmean\n");
            for (size_t i = 0; i < n; ++i) {
                fprintf(out.f[c], "%s\t%lld\t%lld\t%s\t%c\t", fa.names[(size_t)iv.sid[i]].c_str(), (long long)iv.start[i], (long long)iv.end[i],
                        iv.name[i].c_str(), iv.strand[i]);
                print_region_columns(out.f[c], sums[3 * i + (size_t)c]);
            }
        }
    }
    if (!o.meta_bins) return true;
    const int nb = o.meta_bins + 2 * o.meta_flank_bins;
    std::vector<hm_metabin_t> rows(3 * (size_t)nb);
    int64_t n_used = 0;
    if (hm_pileup_fetch_metaplot(pe, planes[0], planes[1], planes[2], 0, 0, off.back(), o.interval_min_cov, start.data(), end.data(), s0.data(), s1.data(),
                                 iv.strand.data(), (int64_t)n, o.meta_bins, o.meta_flank, o.meta_flank_bins, rows.data(), &n_used) != HM_OK)
        return false;
    CtxFiles out;
    if (!out.open(o.prefix, tag + "metaplot.", ".tsv")) return false;
    for (int c = 0; c < 3; ++c) {
        fprintf(out.f[c], "#regions\t%lld\t%lld\n#bin\tpart\tn_regions\tn_loci\tpcov\tncov\tweighted\tmean\n", (long long)n_used, (long long)n - (long long)n_used);
        for (int b = 0; b < nb; ++b) {
            const hm_metabin_t& r = rows[(size_t)c * nb + b];
            fprintf(out.f[c], "%d\t%s\t%lld\t", b, b < o.meta_flank_bins ? "up" : b < o.meta_flank_bins + o.meta_bins ? "body" : "down", (long long)r.n_regions);
            print_region_columns(out.f[c], hm_region_sum_t{r.n_loci, r.pcov, r.ncov, r.ppm});
        }
    }
    return true;
}

// <prefix>.<tag>context.<ctx>.tsv from one set of planes (NULL: the engine's own).  false on an engine error (recorded) or a file
// error (reported).
bool write_context(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, const std::string& tag, const void* const planes[3]) {
    int64_t total = 0;
    for (const int64_t len : fa.length) total += len;
    const int k = 3 + 2 * o.context_flank;
    const int64_t rows = (int64_t(1) << (2 * k)) + 1;
    std::vector<hm_region_sum_t> tab(3 * (size_t)rows);
    if (hm_pileup_fetch_context(pe, planes[0], planes[1], planes[2], 0, 0, total, o.context_min_cov, o.context_flank, tab.data(), 3 * rows) != 3 * rows)
        return false;
    CtxFiles out;
    if (!out.open(o.prefix, tag + "context.", ".tsv")) return false;
    std::string kmer((size_t)k, 'A');
    for (int c = 0; c < 3; ++c) {
        fprintf(out.f[c], "#context\tn_loci\tpcov\tncov\tweighted\tmean\n");
        for (int64_t code = 0; code < rows; ++code) {
            const hm_region_sum_t& r = tab[(size_t)c * rows + code];
            if (r.n_loci <= 0) continue;
            for (int j = 0; j < k; ++j) kmer[(size_t)j] = "ACGT"[(code >> (2 * (k - 1 - j))) & 3];
            fprintf(out.f[c], "%s\t", code == rows - 1 ? "other" : kmer.c_str());
            print_region_columns(out.f[c], r);
        }
    }
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

// rows of the three <prefix>.domains.<ctx>.bed files from the engine's combined planes, sequence by sequence: a segment never
// crosses a sequence.  A sequence's rows are the segments of the first segmented context, then the next one's.  false on an engine
// error.
bool write_domains(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, const int64_t A[3], const int64_t B[3], int64_t S, FILE* out[3]) {
    return write_rows<hm_domain_t>(
        fa, out, o.threads,
        [&](int64_t lo, int64_t hi, hm_domain_t* dst, int64_t cap) -> int64_t {
            int64_t total = 0;
            for (int c = 0; c < 3; ++c) {
                if (std::isnan(o.domain_lo[c])) continue;
                const int64_t n = hm_pileup_fetch_domains(pe, nullptr, nullptr, nullptr, 0, lo, hi, c, A[c], B[c], S, o.domain_max_gap, nullptr,
                                                          dst ? dst + total : nullptr, dst ? cap - total : 0);
                if (n < 0) return n;
                total += n;
            }
            return total;
        },
        [](const hm_domain_t& r, int64_t k, char (&buf)[320]) {
            return snprintf(buf, sizeof buf, "\t%lld\t%lld\t%d\t%c\t%g\t%lld\t%lld\t%.6g\n", (long long)k, (long long)(k + (r.end - r.start)),
                            r.n_loci, r.state ? 'H' : 'L', r.level, (long long)r.pcov, (long long)r.ncov, r.score);
        });
}

// `pileup -D -Y` after hm_pileup_count: the two levels of every segmented context fitted by hard EM (include/hifimeth_hip.h has the
// definition), o.domain_lo / domain_hi and A / B replaced by the result, <prefix>.domains.fit.tsv written.  Per iteration the state
// sums of all sequences (hm_pileup_domain_sums: no segment is built), then hm_domain_refit and the stop rule.  1 done, -1 engine
// error (hm_pileup_last_error), 0 another error (message printed).
int fit_domains(hm_pileup_t* pe, const Fasta& fa, PileupOptions& o, int64_t A[3], int64_t B[3], int64_t S) {
    static const char* cn[3] = {"CpG", "CHG", "CHH"};
    const std::string path = o.prefix + ".domains.fit.tsv";
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "ERROR: cannot open %s for writing\n", path.c_str()); return 0; }
    struct Iter { double lo, hi; int64_t A, B; };
    for (int c = 0; c < 3; ++c) {
        if (std::isnan(o.domain_lo[c])) continue;
        std::vector<Iter> seen;
        Iter cur{o.domain_lo[c], o.domain_hi[c], A[c], B[c]}, result = cur;
        const char* status = nullptr;
        while (!status) {
            int64_t sums[6] = {0, 0, 0, 0, 0, 0}, off = 0;
            for (size_t s = 0; s < fa.names.size(); ++s) {
                int64_t one[6];
                const int64_t lo = off, hi = off + fa.length[s];
                off = hi;
                if (hm_pileup_domain_sums(pe, nullptr, nullptr, nullptr, 0, lo, hi, c, cur.A, cur.B, S, o.domain_max_gap, one) < 0) { fclose(f); return -1; }
                for (int k = 0; k < 6; ++k) sums[k] += one[k];
            }
            fprintf(f, "%s\t%zu\t%.17g\t%.17g\t%lld\t%lld", cn[c], seen.size(), cur.lo, cur.hi, (long long)cur.A, (long long)cur.B);
            for (int k = 0; k < 6; ++k) fprintf(f, "\t%lld", (long long)sums[k]);
            fputc('\n', f);
            seen.push_back(cur);
            Iter next = cur;
            int64_t s_unused = 0;
            const int rc = hm_domain_refit(sums, o.domain_penalty, &next.lo, &next.hi);
            if (rc != HM_OK && rc != HM_EDATA) { fclose(f); fprintf(stderr, "ERROR: hm_domain_refit failed\n"); return 0; }
            if (rc == HM_EDATA) { status = sums[2] == 0 || sums[5] == 0 ? "one_state" : "degenerate"; break; }
            if (hm_domain_scores(next.lo, next.hi, o.domain_penalty, &next.A, &next.B, &s_unused) != HM_OK) { status = "degenerate"; break; }
            const auto same = [&](const Iter& x) { return x.A == next.A && x.B == next.B; };
            const auto j = std::find_if(seen.begin(), seen.end(), same);
            if (same(cur)) status = "converged";
            else if (j != seen.end()) {  // iterations j .. i, j with the levels that closed the cycle: the smallest (A, B)
                status = "cycle";
                result = next;
                for (auto m = j + 1; m != seen.end(); ++m)
                    if (std::make_pair(m->A, m->B) < std::make_pair(result.A, result.B)) result = *m;
            } else if ((long long)seen.size() == o.domain_fit_iter) {
                status = "max_iter";
                result = next;
            } else result = cur = next;
        }
        fprintf(f, "%s\t%s\t%.17g\t%.17g\n", cn[c], status, result.lo, result.hi);
        fprintf(stderr, "domains: %s levels fitted in %zu iteration%s (%s): %.17g:%.17g\n", cn[c], seen.size(), seen.size() == 1 ? "" : "s", status,
                result.lo, result.hi);
        o.domain_lo[c] = result.lo;
        o.domain_hi[c] = result.hi;
        int64_t s_again = 0;
        if (hm_domain_scores(result.lo, result.hi, o.domain_penalty, &A[c], &B[c], &s_again) != HM_OK) {
            fclose(f);
            fprintf(stderr, "ERROR: the fitted %s levels are no valid pair\n", cn[c]);
            return 0;
        }
    }
    fclose(f);
    return 1;
}

// `pileup -H -A -Q` after hm_pileup_count: the tested loci of the whole reference counted per tuple, the p of every tuple that
// occurs, the q-values (hm_asm_qvalues), then the rows of write_asm with their q looked up (56 B per row on the device and here),
// and <prefix>.asm.summary.tsv from the table's weights.  1 done, -1 engine error (hm_pileup_last_error), 0 another error (message
// printed).
int write_asm_q(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, const std::string& tag, FILE* out[3], int threads) {
    static const char* cn[3] = {"CpG", "CHG", "CHH"};
    int64_t n_loci = 0;
    for (size_t s = 0; s < fa.names.size(); ++s) n_loci += fa.length[s];
    const int min_cov = o.asm_min_cov;
    std::vector<uint64_t> bins((size_t)HM_ASM_BINS, 0);
    std::vector<hm_asm_t> big(4096);  // big loci are rare at HiFi coverage: room for them in the first call
    int64_t n_big = hm_pileup_asm_histogram(pe, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, n_loci, min_cov, bins.data(), big.data(),
                                            (int64_t)big.size());
    if (n_big > (int64_t)big.size()) {  // nothing was written or added: again, with room for the list
        big.resize((size_t)n_big);
        n_big = hm_pileup_asm_histogram(pe, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, n_loci, min_cov, bins.data(), big.data(), n_big);
    }
    if (n_big < 0) return -1;
    big.resize((size_t)n_big);
    int64_t n_tab = 0;  // the non-empty bins are counted here: one upload and one compaction on the device
    for (const uint64_t b : bins) n_tab += b != 0;
    std::vector<hm_asm_bin_t> tab((size_t)n_tab);
    n_tab = hm_pileup_asm_bin_pvalues(pe, bins.data(), tab.data(), n_tab);
    if (n_tab < 0) return -1;
    std::vector<uint64_t>().swap(bins);
    std::vector<double> big_q(big.size());
    uint64_t m[3];
    if (hm_asm_qvalues(tab.data(), n_tab, big.data(), n_big, big_q.data(), m) != HM_OK) {
        fprintf(stderr, "ERROR: %s: the table of the tested loci is not one the engine wrote\n", tag.c_str());
        return 0;
    }
    const bool ok = write_rows<hm_asmq_t>(
        fa, out, threads,
        [&](int64_t lo, int64_t hi, hm_asmq_t* dst, int64_t cap) {
            return hm_pileup_fetch_asm_q(pe, nullptr, nullptr, nullptr, nullptr, nullptr, 0, lo, hi, min_cov, tab.data(), n_tab, big.data(),
                                         big_q.data(), n_big, dst, cap);
        },
        [](const hm_asmq_t& r, int64_t k, char (&buf)[320]) {
            return snprintf(buf, sizeof buf, "\t%lld\t%lld\t%g\t%.6g\t%d\t%d\t%d\t%d\t%.6g\n", (long long)k, (long long)k + 1, r.diff, r.pvalue,
                            r.pcov1, r.ncov1, r.pcov2, r.ncov2, r.qvalue);
        });
    if (!ok) return -1;
    uint64_t below[3][2] = {{0, 0}, {0, 0}, {0, 0}};  // loci with q <= 0.05, q <= 0.01
    const auto tally = [&](uint32_t c, uint64_t loci, double q) {
        if (q <= 0.05) below[c][0] += loci;
        if (q <= 0.01) below[c][1] += loci;
    };
    for (const hm_asm_bin_t& t : tab) tally(t.bin / (HM_ASM_PAIRS * HM_ASM_PAIRS), t.count, t.qvalue);
    for (size_t i = 0; i < big.size(); ++i) tally(std::min(big[i].motif, 2u), 1, big_q[i]);
    const std::string path = o.prefix + "." + tag + ".summary.tsv";
    FILE* f = fopen(path.c_str(), "w");
    if (!f) { fprintf(stderr, "ERROR: cannot open %s for writing\n", path.c_str()); return 0; }
    for (int c = 0; c < 3; ++c)
        fprintf(f, "%s\t%llu\t%llu\t%llu\n", cn[c], (unsigned long long)m[c], (unsigned long long)below[c][0], (unsigned long long)below[c][1]);
    fclose(f);
    return 1;
}

// Every output of the test between the engine's two partitions, under the file tag `tag` -- "asm" for the two haplotypes of
// `pileup -H -A`, "diff" for the two samples of `diff`: <prefix>.<tag>.<ctx>.bed (write_asm, or under -Q write_asm_q with
// <prefix>.<tag>.summary.tsv) and under -G <prefix>.<tag>.regions.<ctx>.bed (write_asm_regions).  1 done, 0 an error whose message
// is printed, -1 / -2 an engine error (hm_pileup_last_error) in the rows / in the regions.
int write_partition_tests(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, const std::string& tag) {
    {
        CtxFiles out;
        if (!out.open(o.prefix, tag + ".", ".bed")) return 0;
        const int rc = o.asm_q ? write_asm_q(pe, fa, o, tag, out.f, o.threads) : write_asm(pe, fa, o.asm_min_cov, out.f, o.threads) ? 1 : -1;
        if (rc != 1) return rc;
    }
    if (o.asm_regions) {
        CtxFiles out;
        if (!out.open(o.prefix, tag + ".regions.", ".bed")) return 0;
        if (!write_asm_regions(pe, fa, o, out.f)) return -2;
    }
    return 1;
}
}  // namespace

namespace {
// -K: the record loop of the fused path.  Batches of at most kSlabBases bases (the slab of `call`) go through the call engine's
// batch pipeline on two slots: while this thread waits for batch k's calls, hands them to the pileup engine read by read and
// runs the projection, a producer thread inflates batch k+1, stages its kinetics and queues it on the device.  What `call`
// followed by `pileup` does with a record decides what happens here: an accepted read's calls replace whatever MM / ML it
// carried; a read the engine passes through (shorter than -l, a kinetics tag missing or of the wrong length) leaves `call`
// with its MM / ML stripped (apply_calls), so it contributes nothing; unmapped records are not called at all.
// The call engine is created here, after the pileup engine holds its reference and planes: it sizes its read groups from the
// device memory that is still free.  false (message printed) on any error; t = {read, stage + queue, hand-off, wait + GPU} seconds.
bool fused_record_loop(const PileupOptions& o, BgzfReader& in, hm_pileup_t* pe, const std::function<int(const BamRecord&)>& sid_of,
                       uint64_t& n_records, double t[4]) {
    constexpr int64_t kSlabBases = int64_t(6) << 20;
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    if (hm_abi_version() != HM_ABI_VERSION) { fprintf(stderr, "ERROR: libhifimeth_hip.so was built from another include/hifimeth_hip.h\n"); return false; }
    hm_engine_t* eng = nullptr;
    if (hm_create(&eng, o.model_dir.c_str(), o.ctx_mask, o.device) < 0) { fprintf(stderr, "ERROR: call engine: %s\n", hm_last_error(nullptr)); return false; }
    hm_set_option(eng, "min_read_size", o.min_read_size);
    hm_set_option(eng, "precision", o.precision);
    hm_set_option(eng, "slots", 2);
    if (o.trunk >= 0) hm_set_option(eng, "trunk_mask", o.trunk ? o.ctx_mask : 0);  // as `call -T`

    struct Batch {
        std::vector<BamRecord> recs;
        std::vector<hm_read_t> reads;   // the mapped records, read_id = index in recs
        std::vector<uint8_t> accepted;  // per entry of reads
        hm_batch_t* slot = nullptr;     // queued on the device; NULL when the batch has no mapped record
        bool more = true;
        std::string err;
        double t_read = 0, t_stage = 0;
    };
    Batch bb[2];
    auto produce = [&](Batch& b) {
        const auto t0 = clk::now();
        b.recs.clear();
        b.reads.clear();
        b.err.clear();
        b.slot = nullptr;
        for (int64_t bases = 0; bases < kSlabBases;) {
            BamRecord r;
            if (!(b.more = read_record(in, r, b.err))) break;
            bases += r.l_qseq();
            b.recs.push_back(std::move(r));
        }
        const auto t1 = clk::now();
        b.t_read = secs(t0, t1);
        if (!b.err.empty()) { b.err = "Could not read BAM record: " + b.err; return; }
        for (size_t k = 0; k < b.recs.size(); ++k) {
            const BamRecord& r = b.recs[k];
            if (r.flag() & 4) continue;
            const KineticsView kv = kinetics_of(r);
            hm_read_t d{};
            d.read_id = (int32_t)k;
            d.l_qseq = r.l_qseq();
            d.flag = r.flag();
            d.seq4 = r.seq4();
            for (int j = 0; j < 4; ++j) { d.kin[j] = kv.arr[j]; d.width[j] = (uint8_t)kv.width[j]; }
            b.reads.push_back(d);
        }
        if (b.reads.empty()) return;
        b.accepted.assign(b.reads.size(), 0);
        b.slot = hm_batch_begin(eng);
        if (!b.slot || hm_batch_submit_reads(b.slot, b.reads.data(), (int64_t)b.reads.size(), o.threads, b.accepted.data()) < 0 ||
            hm_batch_enqueue(b.slot) < 0)
            b.err = std::string("call engine: ") + hm_last_error(eng);
        b.t_stage = secs(t1, clk::now());
    };
    std::thread producer;
    auto finish = [&](bool ok) {  // every exit: no thread left, no slot held, then the engine
        if (producer.joinable()) producer.join();
        for (Batch& b : bb)
            if (b.slot) hm_batch_release(b.slot);
        hm_destroy(eng);
        return ok;
    };
    std::vector<uint32_t> cig;
    int cur = 0;
    produce(bb[0]);
    while (true) {
        Batch& b = bb[cur];
        t[0] += b.t_read;
        t[1] += b.t_stage;
        if (!b.err.empty()) { fprintf(stderr, "ERROR: %s\n", b.err.c_str()); return finish(false); }
        if (b.more) producer = std::thread(produce, std::ref(bb[cur ^ 1]));
        const auto t2 = clk::now();
        const hm_call_t* calls = nullptr;
        const int64_t got = b.slot ? hm_batch_wait(b.slot, &calls) : 0;
        if (got < 0) { fprintf(stderr, "ERROR: call engine: %s\n", hm_last_error(eng)); return finish(false); }
        const auto t3 = clk::now();
        int64_t ci = 0;
        size_t ri = 0;
        for (size_t k = 0; k < b.recs.size(); ++k) {
            const BamRecord& r = b.recs[k];
            const uint64_t order = n_records++;
            if (r.flag() & 4) continue;
            const bool accepted = b.accepted[ri++] != 0;
            const int64_t c0 = ci;  // calls come grouped by read, in submission order
            while (ci < got && calls[ci].read_id == (int32_t)k) ++ci;
            if (!accepted || ci == c0) continue;
            const int sid = sid_of(r);
            if (sid < 0) return finish(false);
            real_cigar(r, cig);
            const int rc = hm_pileup_submit_read_calls(pe, (uint32_t)order, r.flag(), sid, r.pos(), r.mapq(), r.l_qseq(), r.seq4(),
                                                       (int32_t)cig.size(), cig.data(), ci - c0, calls + c0, o.haplotypes ? haplotype_of(r) : 0);
            if (rc < 0) {
                fprintf(stderr, "ERROR: read %s: %s\n", reinterpret_cast<const char*>(r.data.data() + 32), hm_pileup_last_error(pe));
                return finish(false);
            }
        }
        if (b.slot) hm_batch_release(b.slot);  // the calls are staged in the pileup engine: the slot can take batch k+2
        b.slot = nullptr;
        const auto t4 = clk::now();
        const int rrc = hm_pileup_run(pe);
        t[2] += secs(t3, t4);
        t[3] += secs(t2, t3) + secs(t4, clk::now());
        if (producer.joinable()) producer.join();
        if (rrc != HM_OK) { fprintf(stderr, "ERROR: projection: %s\n", hm_pileup_last_error(pe)); return finish(false); }
        if (!b.more) break;
        cur ^= 1;
    }
    return finish(true);
}
}  // namespace

namespace {
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

// `pileup -B / -e` after hm_pileup_count: rates (measured on the control sequence `control_sid`, unless given), histogram of the
// whole reference, the table, then the rows (40 B per row on the device and here), and
// <prefix>.sites.rates.tsv.  1 done, -1 engine error (hm_pileup_last_error), 0 another error (message printed).
int write_sites(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, int control_sid, int threads) {
    static const char* cn[3] = {"CpG", "CHG", "CHH"};
    std::vector<int64_t> start(fa.names.size() + 1, 0);
    for (size_t s = 0; s < fa.names.size(); ++s) start[s + 1] = start[s] + fa.length[s];
    uint64_t sums[6] = {0, 0, 0, 0, 0, 0};
    double rates[3] = {o.rates[0], o.rates[1], o.rates[2]};
    if (control_sid >= 0) {
        if (hm_pileup_control_sums(pe, nullptr, nullptr, nullptr, start[(size_t)control_sid], start[(size_t)control_sid + 1], sums) != HM_OK) return -1;
        for (int c = 0; c < 3; ++c) rates[c] = sums[c] + sums[3 + c] ? (double)sums[c] / (double)(sums[c] + sums[3 + c]) : std::nan("");
    }
    for (int c = 0; c < 3; ++c) {
        if (std::isnan(rates[c])) fprintf(stderr, "WARNING: %s is not tested: %s\n", cn[c], control_sid >= 0 ? "the control sequence has no calls in this context" : "its rate is nan");
        else fprintf(stderr, "%s false-positive rate: %.17g\n", cn[c], rates[c]);
    }
    std::vector<uint64_t> bins((size_t)HM_SITE_BINS, 0);
    std::vector<hm_locus_t> big;
    int64_t n_big = hm_pileup_site_histogram(pe, nullptr, nullptr, nullptr, 0, 0, start.back(), bins.data(), nullptr, 0);
    if (n_big > 0) {  // nothing was added: again, with room for the loci beyond the histogram
        big.resize((size_t)n_big);
        n_big = hm_pileup_site_histogram(pe, nullptr, nullptr, nullptr, 0, 0, start.back(), bins.data(), big.data(), n_big);
    }
    if (n_big < 0) return -1;
    std::vector<double> ptab((size_t)HM_SITE_BINS), qtab((size_t)HM_SITE_BINS), big_p(big.size()), big_q(big.size());
    uint64_t m[3];
    if (hm_sites_table(rates, bins.data(), big.data(), n_big, ptab.data(), qtab.data(), big_p.data(), big_q.data(), m) != HM_OK) {
        fprintf(stderr, "ERROR: sites: the histogram of the planes is not one of counts\n");
        return 0;
    }
    int ctx_mask = 0;
    for (int c = 0; c < 3; ++c)
        if (!std::isnan(rates[c])) ctx_mask |= 1 << c;  // an untested context keeps its file, without rows
    CtxFiles out;
    if (!out.open(o.prefix, "sites.", ".bed")) return 0;
    const bool ok = !ctx_mask || write_rows<hm_site_t>(
        fa, out.f, threads,
        [&](int64_t lo, int64_t hi, hm_site_t* dst, int64_t cap) {
            return hm_pileup_fetch_sites(pe, nullptr, nullptr, nullptr, 0, lo, hi, ctx_mask, ptab.data(), qtab.data(), big.data(), big_p.data(),
                                         big_q.data(), n_big, dst, cap);
        },
        [](const hm_site_t& r, int64_t k, char (&buf)[320]) {
            const double freq = 100.0 * r.pcov / (r.pcov + r.ncov);
            return snprintf(buf, sizeof buf, "\t%lld\t%lld\t%g\t%d\t%d\t%.6g\t%.6g\n", (long long)k, (long long)k + 1, freq, r.pcov, r.ncov,
                            r.pvalue, r.qvalue);
        });
    if (!ok) return -1;
    const std::string path = o.prefix + ".sites.rates.tsv";
    FILE* f = fopen(path.c_str(), "w");
    if (!f) {
        fprintf(stderr, "ERROR: cannot open %s for writing\n", path.c_str());
        return 0;
    }
    for (int c = 0; c < 3; ++c) {
        char rate[64] = "nan";
        if (!std::isnan(rates[c])) snprintf(rate, sizeof rate, "%.17g", rates[c]);
        fprintf(f, "%s\t%llu\t%llu\t%s\t%llu\n", cn[c], (unsigned long long)sums[c], (unsigned long long)sums[3 + c], rate, (unsigned long long)m[c]);
    }
    fclose(f);
    return 1;
}
}  // namespace

int cmd_pileup(int argc, char** argv) {
    PileupOptions o;
    int i = 2;
    for (; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-h") { pileup_usage(argv[0]); return 0; }
        if (a.size() < 2 || a[0] != '-') break;
        if (a == "-H") { o.haplotypes = true; continue; }  // a flag: takes no value
        if (a == "-A") { o.asm_test = true; continue; }
        if (a == "-Q") { o.asm_q = true; continue; }
        if (a == "-G") { o.asm_regions = true; continue; }
        if (a == "-K") { o.kinetics = true; continue; }
        if (a == "-D") { o.domains = true; continue; }
        if (a == "-M") { o.bedmethyl = true; continue; }
        if (i + 1 >= argc) { pileup_usage(argv[0]); return EXIT_FAILURE; }
        if (a == "-q") o.min_mapq = atoi(argv[++i]);
        else if (a == "-f") o.min_pi = atof(argv[++i]);
        else if (a == "-t") o.threads = std::max(1, atoi(argv[++i]));
        else if (a == "-d") o.device = atoi(argv[++i]);
        else if (a == "-b") o.read_batch = std::max(1, atoi(argv[++i]));
        else if (a == "-a") { o.asm_min_cov = atoi(argv[++i]); o.asm_min_cov_given = true; }
        else if (a == "-s" || a == "-g" || a == "-n") {  // the whole value must parse, and lie in the option's range
            o.region_option_given = true;
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            if (a == "-s") {
                o.region_max_p = strtod(v, &end);
                if (!(o.region_max_p > 0.0 && o.region_max_p <= 1.0)) o.region_option_bad = true;
            } else {
                const long long x = strtoll(v, &end, 10);
                if (x < 1 || (a == "-n" && x > INT_MAX)) o.region_option_bad = true;
                else if (a == "-g") o.region_max_gap = x;
                else o.region_min_loci = (int)x;
            }
            if (end == v || *end || errno) o.region_option_bad = true;
        }
        else if (a == "-u" || a == "-x" || a == "-j") {  // the whole value must parse, and lie in the option's range
            o.domain_option_given = true;
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            if (a == "-u") {
                if (!parse_levels(v, o.domain_lo, o.domain_hi)) o.domain_option_bad = true;
            } else if (a == "-x") {
                o.domain_penalty = strtod(v, &end);
                if (end == v || *end || errno || !(o.domain_penalty >= 0.0 && o.domain_penalty <= 256.0)) o.domain_option_bad = true;
            } else {
                o.domain_max_gap = strtoll(v, &end, 10);
                if (end == v || *end || errno || o.domain_max_gap < 1) o.domain_option_bad = true;
            }
        }
        else if (a == "-E" || a == "-w" || a == "-o") {  // the whole value must parse, and lie in the option's range
            if (a != "-E") o.pattern_option_given = true;
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            const long long x = strtoll(v, &end, 10);
            if (end == v || *end || errno) o.pattern_option_bad = true;
            else if (a == "-E") { if (x < 2 || x > 4) o.pattern_option_bad = true; else o.patterns = (int)x; }
            else if (a == "-w") { if (x < 1 || x > 65536) o.pattern_option_bad = true; else o.pattern_span = x; }
            else { if (x < 1) o.pattern_option_bad = true; else o.pattern_min_reads = x; }
        }
        else if (a == "-L" || a == "-z") {  // the whole value must parse, and lie in the option's range
            if (a == "-z") o.linkage_option_given = true;
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            const long long x = strtoll(v, &end, 10);
            if (end == v || *end || errno) o.linkage_option_bad = true;
            else if (a == "-L") { if (x < 2 || x > 16384) o.linkage_option_bad = true; else o.linkage = x; }
            else { if (x < 0) o.linkage_option_bad = true; else o.linkage_min_pairs = x; }
        }
        else if (a == "-P" || a == "-y") {  // the whole value must parse, and lie in the option's range
            if (a == "-y") o.profile_option_given = true;
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            const long long x = strtoll(v, &end, 10);
            if (end == v || *end || errno) o.profile_option_bad = true;
            else if (a == "-P") { if (x < 1 || x > 2048) o.profile_option_bad = true; else o.profile = x; }
            else { if (x < 0) o.profile_option_bad = true; else o.profile_min_calls = x; }
        }
        else if (a == "-I") { if (!parse_trim(argv[++i], o.trim5, o.trim3)) o.profile_option_bad = true; }
        else if (a == "-R") o.intervals = argv[++i];
        else if (a == "-C") {  // the whole value must parse
            o.interval_option_given = true;
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            o.interval_min_cov = strtoll(v, &end, 10);
            if (end == v || *end || errno || o.interval_min_cov < 1) o.interval_option_bad = true;
        }
        else if (a == "-J") {
            o.interval_option_given = true;
            if (!parse_metaplot(argv[++i], o.meta_bins, o.meta_flank, o.meta_flank_bins)) o.interval_option_bad = true;
        }
        else if (a == "-S" || a == "-O") {  // the whole value must parse
            const bool flank = a == "-S";
            if (!flank) o.context_option_given = true;
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            const long long x = strtoll(v, &end, 10);
            if (end == v || *end || errno || (flank ? x < 0 || x > 3 : x < 1)) o.context_option_bad = true;
            else if (flank) o.context_flank = (int)x;
            else o.context_min_cov = x;
        }
        else if (a == "-v") {  // the whole value must parse
            o.bedmethyl_option_given = true;
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            o.bedmethyl_min_valid = strtoll(v, &end, 10);
            if (end == v || *end || errno || o.bedmethyl_min_valid < 0) o.bedmethyl_option_bad = true;
        }
        else if (a == "-Y") {
            const char* v = argv[++i];
            char* end = nullptr;
            errno = 0;
            o.domain_fit_iter = strtoll(v, &end, 10);
            if (end == v || *end || errno || o.domain_fit_iter < 1) o.domain_fit_bad = true;
        }
        else if (a == "-B") o.control = argv[++i];
        else if (a == "-e") {
            o.rates_given = true;
            if (!parse_rates(argv[++i], o.rates)) {
                fprintf(stderr, "ERROR: -e takes three comma-separated rates, each a decimal in [0, 1] or nan\n");
                pileup_usage(argv[0]);
                return EXIT_FAILURE;
            }
        }
        else if (a == "-m" || a == "-c" || a == "-l" || a == "-p" || a == "-T") {
            o.call_option_given = true;
            const char* v = argv[++i];
            if (a == "-m") o.model_dir = v;
            else if (a == "-l") o.min_read_size = atoi(v);
            else if (a == "-p") o.precision = atoi(v);
            else if (a == "-T") o.trunk = atoi(v);
            else if (!parse_ctx(v, o.ctx_mask)) { fprintf(stderr, "Illegal argument to option '-c'\n"); pileup_usage(argv[0]); return EXIT_FAILURE; }
        }
        else { fprintf(stderr, "ERROR: unrecognised option %s", a.c_str()); pileup_usage(argv[0]); return EXIT_FAILURE; }
    }
    if (argc - i != 3) { pileup_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad_asm = o.asm_test && !o.haplotypes ? "-A needs -H (the test compares the two haplotypes)"
                          : o.asm_min_cov_given && !o.asm_test ? "-a needs -A"
                          : o.asm_q && !o.asm_test ? "-Q needs -A (the q-values are those of its p-values)"
                          : o.asm_min_cov < 1 ? "-a must be >= 1"
                          : o.asm_regions && !o.asm_test ? "-G needs -A (the regions are chains of its tested loci)"
                          : o.region_option_given && !o.asm_regions ? "-s, -g and -n need -G"
                          : o.region_option_bad ? "-s must be in (0, 1], -g and -n integers >= 1" : nullptr;
    if (bad_asm) { fprintf(stderr, "ERROR: %s\n", bad_asm); pileup_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad_call = o.call_option_given && !o.kinetics ? "-m, -c, -l, -p and -T need -K (they configure the on-the-fly caller)"
                           : o.min_read_size < 0 ? "-l must be >= 0"
                           : o.precision < 0 || o.precision > 2 ? "-p must be 0, 1 or 2"
                           : o.call_option_given && (o.trunk < -1 || o.trunk > 1) ? "-T must be 0 or 1" : nullptr;
    if (bad_call) { fprintf(stderr, "ERROR: %s\n", bad_call); pileup_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad_sites = !o.control.empty() && o.rates_given ? "-B and -e exclude each other (the rates are measured, or given)" : nullptr;
    if (bad_sites) { fprintf(stderr, "ERROR: %s\n", bad_sites); pileup_usage(argv[0]); return EXIT_FAILURE; }
    int64_t dom_A[3] = {0, 0, 0}, dom_B[3] = {0, 0, 0}, dom_S = 0;  // the integer weights of the levels (hm_domain_scores)
    for (int c = 0; c < 3 && o.domains && !o.domain_option_bad; ++c)
        if (!std::isnan(o.domain_lo[c]) && hm_domain_scores(o.domain_lo[c], o.domain_hi[c], o.domain_penalty, &dom_A[c], &dom_B[c], &dom_S) != HM_OK)
            o.domain_option_bad = true;
    const char* bad_domains = o.domain_option_given && !o.domains ? "-u, -x and -j need -D"
                              : (o.domain_fit_iter || o.domain_fit_bad) && !o.domains ? "-Y needs -D (it fits the levels of -D)"
                              : o.domain_fit_bad ? "-Y takes the largest number of iterations, an integer >= 1"
                              : o.domain_option_bad ? "-u takes lo:hi with 0 < lo < hi < 1 (levels a 2^24-th of a nat apart at least) or nan, once or per context; "
                                                      "-x must be in [0, 256], -j an integer >= 1" : nullptr;
    if (bad_domains) { fprintf(stderr, "ERROR: %s\n", bad_domains); pileup_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad_patterns = o.pattern_option_bad ? "-E must be 2, 3 or 4, -w an integer in [1, 65536], -o an integer >= 1"
                               : o.pattern_option_given && !o.patterns ? "-w and -o need -E" : nullptr;
    if (bad_patterns) { fprintf(stderr, "ERROR: %s\n", bad_patterns); pileup_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad_bedmethyl = o.bedmethyl_option_given && !o.bedmethyl ? "-v needs -M" : o.bedmethyl_option_bad ? "-v must be an integer >= 0" : nullptr;
    if (bad_bedmethyl) { fprintf(stderr, "ERROR: %s\n", bad_bedmethyl); pileup_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad_linkage = o.linkage_option_bad ? "-L must be an integer in [2, 16384], -z an integer >= 0"
                              : o.linkage_option_given && !o.linkage ? "-z needs -L" : nullptr;
    if (bad_linkage) { fprintf(stderr, "ERROR: %s\n", bad_linkage); pileup_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad_profile = o.profile_option_bad ? "-P must be an integer in [1, 2048], -y an integer >= 0, -I n5[:n3] with integers >= 0"
                              : o.profile_option_given && !o.profile ? "-y needs -P" : nullptr;
    if (bad_profile) { fprintf(stderr, "ERROR: %s\n", bad_profile); pileup_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad_intervals = o.interval_option_given && o.intervals.empty() ? "-C and -J need -R"
                                : o.interval_option_bad ? "-C must be an integer >= 1, -J bins[:flank_bp:flank_bins] with bins in [1, 1000] and flank_bp a "
                                                          "multiple of flank_bins in [1, 1000]" : nullptr;
    if (bad_intervals) { fprintf(stderr, "ERROR: %s\n", bad_intervals); pileup_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad_context = o.context_option_bad ? "-S must be an integer in [0, 3], -O an integer >= 1"
                              : o.context_option_given && o.context_flank < 0 ? "-O needs -S" : nullptr;
    if (bad_context) { fprintf(stderr, "ERROR: %s\n", bad_context); pileup_usage(argv[0]); return EXIT_FAILURE; }
    const bool sites = !o.control.empty() || o.rates_given;
    if (o.kinetics && o.model_dir.empty()) o.model_dir = exe_dir() + "/../weights";
    o.ref = argv[i];
    o.bam = argv[i + 1];
    o.prefix = argv[i + 2];
    fprintf(stderr, "\n\n====================> Parameters:\nmin-mapQ: %d\nmin-identity: %g\nCPU threads: %d\n"
                    "Genomic reference: %s\nmod-bam: %s\noutput prefix: %s\n",
            o.min_mapq, o.min_pi, o.threads, o.ref.c_str(), o.bam.c_str(), o.prefix.c_str());
    if (o.haplotypes) fprintf(stderr, "haplotypes: HP 1 / 2 -> %s.hap1.* / %s.hap2.*\n", o.prefix.c_str(), o.prefix.c_str());
    if (o.asm_test) fprintf(stderr, "asm: min haplotype coverage %d -> %s.asm.*\n", o.asm_min_cov, o.prefix.c_str());
    if (o.asm_q) fprintf(stderr, "asm: Benjamini-Hochberg q-values per context -> tenth column, %s.asm.summary.tsv\n", o.prefix.c_str());
    if (o.asm_regions)
        fprintf(stderr, "asm: regions of >= %d loci with p <= %g and one sign, gaps <= %lld -> %s.asm.regions.*\n", o.region_min_loci, o.region_max_p,
                o.region_max_gap, o.prefix.c_str());
    if (!o.control.empty()) fprintf(stderr, "sites: binomial test against the rates of control sequence %s -> %s.sites.*\n", o.control.c_str(), o.prefix.c_str());
    if (o.rates_given) fprintf(stderr, "sites: binomial test against the rates %g,%g,%g -> %s.sites.*\n", o.rates[0], o.rates[1], o.rates[2], o.prefix.c_str());
    if (o.domains) {
        std::string levels;
        for (int c = 0; c < 3; ++c) {
            char t[64] = "nan";
            if (!std::isnan(o.domain_lo[c])) snprintf(t, sizeof t, "%g:%g", o.domain_lo[c], o.domain_hi[c]);
            levels += (c ? "," : "") + std::string(t);
        }
        fprintf(stderr, "domains: levels %s, switch penalty %g nats, loci linked up to %lld bases -> %s.domains.*\n", levels.c_str(), o.domain_penalty,
                o.domain_max_gap, o.prefix.c_str());
        if (o.domain_fit_iter)
            fprintf(stderr, "domains: the levels are fitted from the data, %lld iterations at most -> %s.domains.fit.tsv\n", o.domain_fit_iter, o.prefix.c_str());
    }
    if (o.patterns)
        fprintf(stderr, "patterns: windows of %d reference CpGs within %lld bases, spanned by >= %lld reads -> %s.patterns.CpG.bed\n", o.patterns,
                o.pattern_span, o.pattern_min_reads, o.prefix.c_str());
    if (o.bedmethyl)
        fprintf(stderr, "bedmethyl: reference CpGs with Nvalid >= %lld, 18 columns -> %s.bedmethyl.CpG.bed%s\n", o.bedmethyl_min_valid, o.prefix.c_str(),
                o.haplotypes ? ", .hap1. and .hap2. as well" : "");
    if (o.linkage)
        fprintf(stderr, "linkage: pairs of CpG calls of one read up to %lld bases apart, distances with >= %lld pairs -> %s.linkage.CpG.tsv\n", o.linkage,
                o.linkage_min_pairs, o.prefix.c_str());
    if (o.profile)
        fprintf(stderr, "readpos: calls by position in the read, %lld bases from either end resolved, rows with >= %lld calls -> %s.readpos.tsv\n", o.profile,
                o.profile_min_calls, o.prefix.c_str());
    if (!o.intervals.empty()) {
        fprintf(stderr, "regions: intervals of %s, loci with coverage >= %lld -> %s.regions.*\n", o.intervals.c_str(), o.interval_min_cov, o.prefix.c_str());
        if (o.meta_bins)
            fprintf(stderr, "metaplot: %d bins per interval, flanks of %lld bases in %d bins -> %s.metaplot.*\n", o.meta_bins, o.meta_flank,
                    o.meta_flank_bins, o.prefix.c_str());
    }
    if (o.context_flank >= 0)
        fprintf(stderr, "context: loci by the %d bases around the cytosine, coverage >= %lld -> %s.context.*\n", 3 + 2 * o.context_flank, o.context_min_cov,
                o.prefix.c_str());
    if (o.trim5 || o.trim3) fprintf(stderr, "trim: calls in the first %lld and the last %lld bases of a read are left out\n", o.trim5, o.trim3);
    if (o.kinetics)
        fprintf(stderr, "kinetics: called on the fly (models %s, contexts%s%s%s, min read length %d, precision %d, trunk %s)\n", o.model_dir.c_str(),
                o.ctx_mask & 1 ? " CpG" : "", o.ctx_mask & 2 ? " CHG" : "", o.ctx_mask & 4 ? " CHH" : "", o.min_read_size, o.precision,
                o.trunk < 0 ? "auto" : o.trunk ? "1" : "0");
    fprintf(stderr, "\n\n");

    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    const auto t_start = clk::now();
    double t_read = 0, t_parse = 0, t_submit = 0, t_gpu = 0;
    BgzfReader in(o.bam, o.threads);
    BamHeader hdr;
    std::string err;
    if (!in.ok() || !read_header(in, hdr, err)) { fprintf(stderr, "ERROR: %s%s\n", in.error().c_str(), err.c_str()); return EXIT_FAILURE; }
    if (!mapped_and_sorted(hdr)) return 1;

    Fasta fa;
    if (!load_fasta(o.ref, fa, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return EXIT_FAILURE; }
    fprintf(stderr, "Load %zu sequences (%zu bases) from %s\n", fa.names.size(), fa.bases.size(), o.ref.c_str());
    std::vector<int> tid2sid(hdr.refs.size(), -2);  // resolved at first use, as HbnDatabase::seq_name2id
    const int control_sid = o.control.empty() ? -1 : fa.find(o.control);
    if (!o.control.empty() && control_sid < 0) { fprintf(stderr, "ERROR: control sequence %s (-B) is not in %s\n", o.control.c_str(), o.ref.c_str()); return EXIT_FAILURE; }

    Intervals intervals;  // read and checked before the engine exists: a bad file needs no device
    if (!o.intervals.empty() && !read_intervals(o.intervals, fa, intervals)) return EXIT_FAILURE;

    hm_pileup_t* pe = nullptr;
    if (hm_pileup_create(&pe, o.device) != HM_OK) { fprintf(stderr, "ERROR: %s\n", hm_pileup_last_error(nullptr)); return EXIT_FAILURE; }
    std::unique_ptr<hm_pileup_t, decltype(&hm_pileup_destroy)> engine(pe, hm_pileup_destroy);  // destroyed on every way out
    auto die = [&](const std::string& what) {
        fprintf(stderr, "ERROR: %s: %s\n", what.c_str(), hm_pileup_last_error(pe));
        return EXIT_FAILURE;
    };
    hm_pileup_set_option(pe, "min_mapq", o.min_mapq);
    hm_pileup_set_option(pe, "min_pi", o.min_pi);
    if (o.haplotypes && hm_pileup_set_option(pe, "partitions", 2) != HM_OK) return die("partitions");
    if (o.patterns && (hm_pileup_set_option(pe, "patterns", o.patterns) != HM_OK || hm_pileup_set_option(pe, "pattern_span", (double)o.pattern_span) != HM_OK))
        return die("patterns");
    if (o.bedmethyl && hm_pileup_set_option(pe, "bedmethyl", 1) != HM_OK) return die("bedmethyl");
    if (o.linkage && hm_pileup_set_option(pe, "linkage", (double)o.linkage) != HM_OK) return die("linkage");
    if (o.profile && hm_pileup_set_option(pe, "profile", (double)o.profile) != HM_OK) return die("profile");
    if ((o.trim5 || o.trim3) && (hm_pileup_set_option(pe, "trim5", (double)o.trim5) != HM_OK || hm_pileup_set_option(pe, "trim3", (double)o.trim3) != HM_OK))
        return die("trim");
    if (fa.names.empty()) { fprintf(stderr, "ERROR: no sequence in %s\n", o.ref.c_str()); return EXIT_FAILURE; }
    if (hm_pileup_set_reference(pe, (int32_t)fa.names.size(), fa.length.data(), fa.bases.data()) != HM_OK) return die("reference");

    // index of a mapped record's reference sequence in the FASTA; -1 (message printed) if the record has none or the name is unknown
    auto sid_of = [&](const BamRecord& r) {
        const int tid = r.ref_id();
        if (tid < 0 || tid >= (int)hdr.refs.size()) { fprintf(stderr, "ERROR: mapped record without a reference id\n"); return -1; }
        if (tid2sid[(size_t)tid] == -2) tid2sid[(size_t)tid] = fa.find(hdr.refs[(size_t)tid].first);
        if (tid2sid[(size_t)tid] < 0) fprintf(stderr, "ERROR: Sequence name %s does not exist\n", hdr.refs[(size_t)tid].first.c_str());
        return std::max(tid2sid[(size_t)tid], -1);
    };
    uint64_t n_records = 0;
    if (o.kinetics) {
        double t[4] = {0, 0, 0, 0};
        const bool ok = fused_record_loop(o, in, pe, sid_of, n_records, t);
        t_read = t[0]; t_parse = t[1]; t_submit = t[2]; t_gpu = t[3];
        if (!ok) return EXIT_FAILURE;
    } else {
        // Two batches in flight: a producer thread inflates + parses batch k+1 (parse_mods over `threads` workers) while
        // this thread stages batch k and runs the GPU.
        struct Batch {
            std::vector<BamRecord> recs;
            std::vector<std::vector<BaseMod>> mods;
            std::vector<std::string> perr;
            int n = 0;
            bool more = true;
            std::string err;
            double t_read = 0, t_parse = 0;
        };
        Batch bb[2];
        for (Batch& b : bb) {
            b.recs.resize((size_t)o.read_batch);
            b.mods.resize((size_t)o.read_batch);
            b.perr.resize((size_t)o.read_batch);
        }
        auto produce = [&](Batch& b) {
            auto t0 = clk::now();
            b.n = 0;
            b.err.clear();
            while (b.n < o.read_batch && (b.more = read_record(in, b.recs[(size_t)b.n], b.err))) ++b.n;
            auto t1 = clk::now();
            parallel_run(b.n, o.threads, [&](int k) {
                b.mods[(size_t)k].clear();
                b.perr[(size_t)k].clear();
                if (!parse_mods(b.recs[(size_t)k], b.mods[(size_t)k], b.perr[(size_t)k])) b.mods[(size_t)k].clear();
            });
            b.t_read = secs(t0, t1);
            b.t_parse = secs(t1, clk::now());
        };
        int cur = 0;
        produce(bb[0]);
        std::vector<uint32_t> cig;
        while (true) {
            Batch& b = bb[cur];
            t_read += b.t_read;
            t_parse += b.t_parse;
            if (!b.err.empty()) { fprintf(stderr, "ERROR: Could not read BAM record: %s\n", b.err.c_str()); return EXIT_FAILURE; }
            std::thread producer;
            if (b.more) producer = std::thread(produce, std::ref(bb[cur ^ 1]));
            auto fail_out = [&]() { if (producer.joinable()) producer.join(); return EXIT_FAILURE; };
            auto t2 = clk::now();
            for (int k = 0; k < b.n; ++k) {
                const BamRecord& r = b.recs[(size_t)k];
                const uint64_t order = n_records++;
                if (!b.perr[(size_t)k].empty()) {
                    fprintf(stderr, "ERROR at parsing read %s\n%s\n", reinterpret_cast<const char*>(r.data.data() + 32), b.perr[(size_t)k].c_str());
                    return fail_out();
                }
                if (b.mods[(size_t)k].empty() || (r.flag() & 4)) continue;
                const int sid = sid_of(r);
                if (sid < 0) return fail_out();
                real_cigar(r, cig);
                const int rc = hm_pileup_submit_read_hp(pe, (uint32_t)order, r.flag(), sid, r.pos(), r.mapq(), r.l_qseq(),
                                                        r.seq4(), (int32_t)cig.size(), cig.data(), (int64_t)b.mods[(size_t)k].size(),
                                                        b.mods[(size_t)k].data(), o.haplotypes ? haplotype_of(r) : 0);
                if (rc < 0) {
                    fprintf(stderr, "ERROR: read %s: %s\n", reinterpret_cast<const char*>(r.data.data() + 32), hm_pileup_last_error(pe));
                    return fail_out();
                }
            }
            auto t3 = clk::now();
            t_submit += secs(t2, t3);
            const int rrc = hm_pileup_run(pe);
            t_gpu += secs(t3, clk::now());
            if (producer.joinable()) producer.join();
            if (rrc != HM_OK) return die("projection");
            if (!b.more) break;
            cur ^= 1;
        }
    }
    const auto t_loop = clk::now();

    static uint64_t bins[768];
    if (hm_pileup_histograms(pe, bins) != HM_OK) return die("histograms");
    uint8_t thr[3];
    report_thresholds(bins, thr);
    if (hm_pileup_count(pe, thr) != HM_OK) return die("count");

    // one set of three files per output: the combined planes, then (-H) each partition's pcov / ncov with the combined key
    std::vector<std::string> tags{""};
    std::vector<const void*> planes{nullptr, nullptr, nullptr};
    if (o.haplotypes) {
        void* key = nullptr;
        if (hm_pileup_planes(pe, nullptr, nullptr, &key, nullptr) != HM_OK) return die("planes");
        for (int part = 1; part <= 2; ++part) {
            void *pc = nullptr, *nc = nullptr;
            if (hm_pileup_partition_planes(pe, part, &pc, &nc) != HM_OK) return die("partition planes");
            tags.push_back("hap" + std::to_string(part) + ".");
            planes.insert(planes.end(), {pc, nc, key});
        }
    }
    for (size_t t = 0; t < tags.size(); ++t) {
        CtxFiles out;
        if (!out.open(o.prefix, tags[t], ".cov.bed")) return EXIT_FAILURE;
        if (!write_bed(pe, fa, planes[3 * t], planes[3 * t + 1], planes[3 * t + 2], out.f, o.threads)) return die("loci");
    }
    if (o.asm_test) {  // -Q and -G need -A
        const int rc = write_partition_tests(pe, fa, o, "asm");
        if (rc < 0) return die(rc == -1 ? "asm" : "asm regions");
        if (rc == 0) return EXIT_FAILURE;
    }
    if (o.domains) {
        if (o.domain_fit_iter) {
            const int rc = fit_domains(pe, fa, o, dom_A, dom_B, dom_S);
            if (rc < 0) return die("domains fit");
            if (rc == 0) return EXIT_FAILURE;
        }
        CtxFiles out;
        if (!out.open(o.prefix, "domains.", ".bed")) return EXIT_FAILURE;
        if (!write_domains(pe, fa, o, dom_A, dom_B, dom_S, out.f)) return die("domains");
    }
    if (o.patterns) {
        FILE* out[3] = {fopen((o.prefix + ".patterns.CpG.bed").c_str(), "w"), nullptr, nullptr};
        if (!out[0]) { fprintf(stderr, "ERROR: cannot open %s.patterns.CpG.bed for writing\n", o.prefix.c_str()); return EXIT_FAILURE; }
        const bool ok = write_patterns(pe, fa, o, out);
        fclose(out[0]);
        if (!ok) return die("patterns");
    }
    for (int part = 0; o.bedmethyl && part <= (o.haplotypes ? 2 : 0); ++part) {
        const std::string path = o.prefix + (part ? ".hap" + std::to_string(part) : std::string()) + ".bedmethyl.CpG.bed";
        FILE* out[3] = {fopen(path.c_str(), "w"), nullptr, nullptr};
        if (!out[0]) { fprintf(stderr, "ERROR: cannot open %s for writing\n", path.c_str()); return EXIT_FAILURE; }
        const bool ok = write_bedmethyl(pe, fa, o, part, out);
        fclose(out[0]);
        if (!ok) return die("bedmethyl");
    }
    if (o.linkage && !write_linkage(pe, o)) return die("linkage");
    if (o.profile && !write_readpos(pe, o)) return die("readpos");
    for (size_t t = 0; !o.intervals.empty() && t < tags.size(); ++t)
        if (!write_intervals(pe, fa, o, intervals, tags[t], &planes[3 * t])) return die("regions");
    for (size_t t = 0; o.context_flank >= 0 && t < tags.size(); ++t)
        if (!write_context(pe, fa, o, tags[t], &planes[3 * t])) return die("context");
    if (sites) {
        const int rc = write_sites(pe, fa, o, control_sid, o.threads);
        if (rc < 0) return die("sites");
        if (rc == 0) return EXIT_FAILURE;
    }
    engine.reset();
    fprintf(stderr, o.kinetics ? "## %llu records in %.2f s: [producer thread: BAM read %.2f s, kinetics staging + queueing %.2f s] overlapped with "
                                 "[call hand-off %.2f s, waiting for calls + GPU projection %.2f s]; thresholds + count + BED %.2f s\n"
                               : "## %llu records in %.2f s: [producer thread: BAM read %.2f s, MM/ML parse %.2f s] overlapped with "
                                 "[staging %.2f s, GPU projection %.2f s]; thresholds + count + BED %.2f s\n",
            (unsigned long long)n_records, secs(t_start, clk::now()), t_read, t_parse, t_submit, t_gpu, secs(t_loop, clk::now()));
    return 0;
}

// ---- diff [OPTIONS] reference prefix1 prefix2 out-prefix (ours) -----------------------------------------------------------------------
// Two-sample differential methylation from two pileups: the rows of <prefix1>.<ctx>.cov.bed go into the engine's partition 1, those
// of <prefix2>.<ctx>.cov.bed into partition 2 (hm_pileup_load_loci), and the per-locus test, its q-values and the regions of
// `pileup -H -A [-Q] [-G]` are written for sample 1 against sample 2 as <out>.diff.* (DESIGN.md section 10).  Files and not two BAMs:
// each sample keeps the thresholds its own pileup inferred, and files from pileup_dist or cov2bed compare as well.
namespace {

void diff_usage(const char* exe) {
    fprintf(stderr,
            "USAGE:\n  %s diff [OPTIONS] reference prefix1 prefix2 output-prefix\n\n"
            "DESCRIPTION:\n  Test two samples for differential methylation, locus by locus, from the files two `pileup` runs wrote:\n"
            "  <prefix1>.<ctx>.cov.bed against <prefix2>.<ctx>.cov.bed for ctx in CpG, CHG, CHH (plain or gzip; a row is chrom, start,\n"
            "  start + 1, a percentage that is not read, methylated calls, unmethylated calls; further columns are ignored).  A context\n"
            "  without both files is skipped.  Writes <output-prefix>.diff.<ctx>.bed: chrom, start, end, sample 1 %% - sample 2 %%, two-sided\n"
            "  Fisher exact p-value, pcov1, ncov1, pcov2, ncov2 for every locus where each sample has at least -a calls; a locus the two\n"
            "  samples list under different contexts goes to the later one of CpG, CHG, CHH\n\n"
            "OPTIONAL ARGUMENTS (as the same letters of `pileup -H -A`):\n"
            "  -a <int>\n    Minimum coverage (pcov + ncov) of each sample at a tested locus\n    Default: 5\n"
            "  -Q\n    A tenth column, the Benjamini-Hochberg q-value of the p-value among all tested loci of the context, and\n"
            "    <output-prefix>.diff.summary.tsv: ctx, tested loci, loci with q <= 0.05, loci with q <= 0.01\n"
            "  -G\n    Chain the tested loci of each context into regions and write <output-prefix>.diff.regions.<ctx>.bed: chrom, start, end,\n"
            "    loci, + or -, sample 1 %% - sample 2 %% of the pooled counts, smallest p-value, pcov1, ncov1, pcov2, ncov2 summed over the loci\n"
            "  -s <p>\n    With -G: largest p-value of a locus in a region, in (0, 1]\n    Default: 0.01\n"
            "  -g <bp>\n    With -G: largest distance between consecutive loci of a region, >= 1\n    Default: 500\n"
            "  -n <int>\n    With -G: smallest number of loci of a region, >= 1\n    Default: 3\n"
            "  -t <CPU threads>\n    Number of CPU threads\n    Default: 8\n"
            "  -d <int>\n    GPU ordinal\n    Default: 0\n",
            exe);
}

// a whole field as a non-negative decimal integer of at most 18 digits -> true; a sign, a blank or anything else: false
bool parse_count(const char* a, const char* b, long long& v) {
    if (a == b || b - a > 18) return false;
    v = 0;
    for (; a < b; ++a) {
        if (*a < '0' || *a > '9') return false;
        v = v * 10 + (*a - '0');
    }
    return true;
}

// One <prefix>.<ctx>.cov.bed, plain or gzip, into partition `part` with motif `motif`: read in blocks of whole lines, each block
// parsed by `threads` workers over contiguous runs of lines and handed to the engine run by run.  Empty lines are skipped.  false
// with a message naming the file and, for a bad line, its number.
bool load_cov_bed(hm_pileup_t* pe, const Fasta& fa, const std::vector<int64_t>& seq_start, const std::string& path, int part, uint32_t motif,
                  int threads, uint64_t& n_rows) {
    constexpr size_t BLOCK = size_t(32) << 20;
    gzFile in = gzopen(path.c_str(), "rb");
    if (!in) { fprintf(stderr, "ERROR: cannot open %s\n", path.c_str()); return false; }
    struct Part {
        std::vector<hm_locus_t> rows;
        long long lines = 0, bad_line = 0;  // lines seen; the 1-based one among them that is bad, 0: none
        std::string what;
    };
    std::vector<Part> parts((size_t)threads);
    std::vector<size_t> cut((size_t)threads + 1);
    std::string buf;
    long long lines_before = 0;
    bool eof = false, ok = true;
    while (ok && !eof) {
        const size_t have = buf.size();
        buf.resize(have + BLOCK);
        const int got = gzread(in, &buf[have], (unsigned)BLOCK);
        if (got < 0) { fprintf(stderr, "ERROR: %s: cannot read (not a gzip or text file?)\n", path.c_str()); ok = false; break; }
        buf.resize(have + (size_t)got);
        eof = (size_t)got < BLOCK;
        size_t end = buf.size();  // the block ends behind its last newline; the rest waits for the next read
        if (!eof) {
            const size_t nl = buf.rfind('\n');
            if (nl == std::string::npos) continue;  // a line longer than a block: read on
            end = nl + 1;
        }
        for (int k = 0; k <= threads; ++k) {  // worker k takes the lines that start in [cut[k], cut[k + 1])
            size_t at = end * (size_t)k / (size_t)threads;
            if (at > 0 && at < end) {
                const void* nl = memchr(buf.data() + at - 1, '\n', end - at + 1);
                at = nl ? (size_t)(static_cast<const char*>(nl) - buf.data()) + 1 : end;
            }
            cut[(size_t)k] = at;
        }
        parallel_run(threads, threads, [&](int k) {
            Part& P = parts[(size_t)k];
            P.rows.clear();
            P.lines = P.bad_line = 0;
            std::string last;
            int sid = -1;
            const char* p = buf.data() + cut[(size_t)k];
            const char* const stop = buf.data() + cut[(size_t)k + 1];
            while (p < stop) {
                const char* nl = static_cast<const char*>(memchr(p, '\n', (size_t)(stop - p)));
                const char* e = nl ? nl : stop;
                const char* next = nl ? nl + 1 : stop;
                if (e > p && e[-1] == '\r') --e;
                ++P.lines;
                if (e == p) { p = next; continue; }
                const auto bad = [&](const std::string& what) { P.bad_line = P.lines; P.what = what; };
                const char* col[7];  // starts of columns 1 .. 6 and the end of column 6
                int nc = 0;
                col[nc++] = p;
                for (const char* q = p; q < e && nc < 7; ++q)
                    if (*q == '\t') col[nc++] = q + 1;
                if (nc < 6) { bad("fewer than 6 tab-separated columns"); return; }
                if (nc == 6) col[6] = e + 1;
                if (sid < 0 || last.size() != (size_t)(col[1] - 1 - col[0]) || memcmp(last.data(), col[0], last.size()) != 0) {
                    last.assign(col[0], col[1] - 1);
                    sid = fa.find(last);
                    if (sid < 0) { bad("unknown sequence " + last); return; }
                }
                long long start = 0, stop1 = 0, pc = 0, nc_ = 0;
                if (!parse_count(col[1], col[2] - 1, start) || start >= fa.length[(size_t)sid]) {
                    bad("start is not an integer inside " + last + " (" + std::to_string(fa.length[(size_t)sid]) + " bases)");
                    return;
                }
                if (!parse_count(col[2], col[3] - 1, stop1) || stop1 != start + 1) { bad("end is not start + 1"); return; }
                if (!parse_count(col[4], col[5] - 1, pc) || !parse_count(col[5], col[6] - 1, nc_) || pc > INT32_MAX || nc_ > INT32_MAX) {
                    bad("the counts in columns 5 and 6 must be integers in 0 .. 2147483647");
                    return;
                }
                P.rows.push_back(hm_locus_t{seq_start[(size_t)sid] + start, (int32_t)pc, (int32_t)nc_, motif, 0});
                p = next;
            }
        });
        for (const Part& P : parts) {
            if (P.bad_line) {
                fprintf(stderr, "ERROR: %s:%lld: %s\n", path.c_str(), lines_before + P.bad_line, P.what.c_str());
                ok = false;
                break;
            }
            lines_before += P.lines;
            const int64_t rc = hm_pileup_load_loci(pe, part, P.rows.data(), (int64_t)P.rows.size());
            if (rc < 0) { fprintf(stderr, "ERROR: %s: %s\n", path.c_str(), hm_pileup_last_error(pe)); ok = false; break; }
            n_rows += (uint64_t)rc;
        }
        buf.erase(0, end);
    }
    gzclose(in);
    return ok;
}

// <prefix>.<ctx>.cov.bed, or that name with .gz behind it, whichever can be opened; empty if neither
std::string find_cov_bed(const std::string& prefix, const char* ctx) {
    for (const char* gz : {"", ".gz"}) {
        const std::string path = prefix + "." + ctx + ".cov.bed" + gz;
        if (FILE* f = fopen(path.c_str(), "rb")) { fclose(f); return path; }
    }
    return std::string();
}

}  // namespace

int cmd_diff(int argc, char** argv) {
    static const char* cn[3] = {"CpG", "CHG", "CHH"};
    PileupOptions o;
    int i = 2;
    for (; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-h") { diff_usage(argv[0]); return 0; }
        if (a.size() < 2 || a[0] != '-') break;
        if (a == "-Q") { o.asm_q = true; continue; }
        if (a == "-G") { o.asm_regions = true; continue; }
        if (i + 1 >= argc) { diff_usage(argv[0]); return EXIT_FAILURE; }
        const char* v = argv[++i];
        char* end = nullptr;
        errno = 0;
        if (a == "-t") o.threads = std::max(1, atoi(v));
        else if (a == "-d") o.device = atoi(v);
        else if (a == "-a") o.asm_min_cov = atoi(v);
        else if (a == "-s") {
            o.region_option_given = true;
            o.region_max_p = strtod(v, &end);
            if (end == v || *end || errno || !(o.region_max_p > 0.0 && o.region_max_p <= 1.0)) o.region_option_bad = true;
        } else if (a == "-g" || a == "-n") {
            o.region_option_given = true;
            const long long x = strtoll(v, &end, 10);
            if (end == v || *end || errno || x < 1 || (a == "-n" && x > INT_MAX)) o.region_option_bad = true;
            else if (a == "-g") o.region_max_gap = x;
            else o.region_min_loci = (int)x;
        } else { fprintf(stderr, "ERROR: unrecognised option %s\n", a.c_str()); diff_usage(argv[0]); return EXIT_FAILURE; }
    }
    if (argc - i != 4) { diff_usage(argv[0]); return EXIT_FAILURE; }
    const char* bad = o.asm_min_cov < 1 ? "-a must be >= 1"
                      : o.region_option_given && !o.asm_regions ? "-s, -g and -n need -G"
                      : o.region_option_bad ? "-s must be in (0, 1], -g and -n integers >= 1" : nullptr;
    if (bad) { fprintf(stderr, "ERROR: %s\n", bad); diff_usage(argv[0]); return EXIT_FAILURE; }
    o.ref = argv[i];
    const std::string sample[2] = {argv[i + 1], argv[i + 2]};
    o.prefix = argv[i + 3];
    fprintf(stderr, "\n\n====================> Parameters:\nCPU threads: %d\nGenomic reference: %s\nsample 1: %s.<ctx>.cov.bed\nsample 2: %s.<ctx>.cov.bed\n"
                    "output prefix: %s\ndiff: min sample coverage %d -> %s.diff.*\n",
            o.threads, o.ref.c_str(), sample[0].c_str(), sample[1].c_str(), o.prefix.c_str(), o.asm_min_cov, o.prefix.c_str());
    if (o.asm_q) fprintf(stderr, "diff: Benjamini-Hochberg q-values per context -> tenth column, %s.diff.summary.tsv\n", o.prefix.c_str());
    if (o.asm_regions)
        fprintf(stderr, "diff: regions of >= %d loci with p <= %g and one sign, gaps <= %lld -> %s.diff.regions.*\n", o.region_min_loci, o.region_max_p,
                o.region_max_gap, o.prefix.c_str());
    fprintf(stderr, "\n\n");

    using clk = std::chrono::steady_clock;
    const auto t_start = clk::now();
    std::string files[3][2];  // found before the reference is read and the engine exists: a job without input needs neither
    int n_ctx = 0;
    for (int c = 0; c < 3; ++c) {
        for (int s = 0; s < 2; ++s) files[c][s] = find_cov_bed(sample[s], cn[c]);
        if (!files[c][0].empty() && !files[c][1].empty()) { ++n_ctx; continue; }
        for (int s = 0; s < 2; ++s)
            if (files[c][s].empty()) fprintf(stderr, "Skip context %s: %s.%s.cov.bed is missing\n", cn[c], sample[s].c_str(), cn[c]);
        files[c][0].clear();
    }
    if (!n_ctx) { fprintf(stderr, "ERROR: no context has a cov.bed file of both samples\n"); return EXIT_FAILURE; }
    Fasta fa;
    std::string err;
    if (!load_fasta(o.ref, fa, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return EXIT_FAILURE; }
    if (fa.names.empty()) { fprintf(stderr, "ERROR: no sequence in %s\n", o.ref.c_str()); return EXIT_FAILURE; }
    fprintf(stderr, "Load %zu sequences (%zu bases) from %s\n", fa.names.size(), fa.bases.size(), o.ref.c_str());
    std::vector<int64_t> seq_start(fa.names.size() + 1, 0);
    for (size_t s = 0; s < fa.names.size(); ++s) seq_start[s + 1] = seq_start[s] + fa.length[s];

    hm_pileup_t* pe = nullptr;
    if (hm_pileup_create(&pe, o.device) != HM_OK) { fprintf(stderr, "ERROR: %s\n", hm_pileup_last_error(nullptr)); return EXIT_FAILURE; }
    std::unique_ptr<hm_pileup_t, decltype(&hm_pileup_destroy)> engine(pe, hm_pileup_destroy);  // destroyed on every way out
    auto die = [&](const std::string& what) {
        fprintf(stderr, "ERROR: %s: %s\n", what.c_str(), hm_pileup_last_error(pe));
        return EXIT_FAILURE;
    };
    if (hm_pileup_set_option(pe, "partitions", 2) != HM_OK) return die("partitions");
    if (hm_pileup_set_reference(pe, (int32_t)fa.names.size(), fa.length.data(), fa.bases.data()) != HM_OK) return die("reference");
    uint64_t n_rows[2] = {0, 0};
    for (int c = 0; c < 3; ++c)
        for (int s = 0; s < 2 && !files[c][0].empty(); ++s)
            if (!load_cov_bed(pe, fa, seq_start, files[c][s], s + 1, (uint32_t)c, o.threads, n_rows[s])) return EXIT_FAILURE;
    const auto t_load = clk::now();
    const int rc = write_partition_tests(pe, fa, o, "diff");
    if (rc < 0) return die(rc == -1 ? "diff" : "diff regions");
    if (rc == 0) return EXIT_FAILURE;
    engine.reset();
    const auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    fprintf(stderr, "## %llu + %llu covered loci of %d contexts in %.2f s: parse + load %.2f s; test + BED %.2f s\n", (unsigned long long)n_rows[0],
            (unsigned long long)n_rows[1], n_ctx, secs(t_start, clk::now()), secs(t_start, t_load), secs(t_load, clk::now()));
    return 0;
}
