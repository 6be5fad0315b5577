// hifimeth_pileup.cpp -- `hifimeth-hip pileup [OPTIONS] reference mod-bam output-prefix` and `hifimeth-hip diff`.
// `pileup` has the command line, stderr messages and <prefix>.<ctx>.cov.bed files of `hifimeth pileup` (src/app/hifimeth/pileup.cpp:
// 22-112, 461-606).  The host parses the BAM and the MM/ML lists (parallel over the reads of a batch); alignment projection,
// histograms and per-locus counting run on the GPU through the hm_pileup_* C ABI.  No temporary file is written: the projected
// calls stay in HBM until the thresholds are known.  Every further output (-H, -A, -B, -D, -E, -M, -L, -P, -R, -S, -K, ...) is ours:
// the option table of hifimeth_pileup_opts.cpp, which `pileup -h` prints, says what each one writes, DESIGN.md section 10 how.
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <climits>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hifimeth_hip.h"
#include "hifimeth_pileup_opts.h"
#include "hm_bam.h"
#include "hm_cli.h"

using namespace hmbam;

static const char* const CTX_NAME[3] = {"CpG", "CHG", "CHH"};  // the contexts, as files and messages name them

// CIGAR of a record as uint32 ops.  A CIGAR of more than 65535 operations does not fit the 16-bit n_cigar_op field: the
// record then carries the placeholder <l_seq>S<ref_len>N and the real operations in a CG:B,I tag (SAMv1 section 4.2.2);
// htslib's sam_read1 -- what the reference's pileup reads with -- swaps them back in, and so does this.
void real_cigar(const BamRecord& r, std::vector<uint32_t>& cig) {
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

// s_resolve_scaled_prob_threshold (pileup.cpp:355-436, eval.cpp:213-305): the three thresholds with the reference's messages
void report_thresholds(const uint64_t* bins, uint8_t thr[3]) {
    for (int c = 0; c < 3; ++c) {
        uint64_t samples = 0;
        const int t = resolve_threshold(bins + 256 * c, &samples);
        fprintf(stderr, "%s samples: %llu\n", CTX_NAME[c], (unsigned long long)samples);
        const uint64_t* a = bins + 256 * c;  // the fallback branch: window narrower than 50 bins or < 10000 samples
        int st = 20, en = 256 - 20;
        while (st < 256 && a[st] < 10) ++st;
        while (en && a[en - 1] < 10) --en;
        const bool fallback = samples < 10000 || en - st < 50;
        if (fallback) fprintf(stderr, "Not enough samples for inferring scaled probability threshold, set it to 128\n");
        else fprintf(stderr, "%s scaled probability threshold: %d\n", CTX_NAME[c], t);
        thr[c] = (uint8_t)t;
    }
}

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
inline uint32_t row_ctx(const hm_smooth_t&) { return 0; }  // one context per file: the caller's

// An output file, closed when its owner goes; empty (message printed) if it cannot be opened.
struct CloseFile { void operator()(FILE* f) const { fclose(f); } };
using OutFile = std::unique_ptr<FILE, CloseFile>;
OutFile open_out(const std::string& path) {
    OutFile f(fopen(path.c_str(), "w"));
    if (!f) fprintf(stderr, "ERROR: cannot open %s for writing\n", path.c_str());
    return f;
}

// The three files <prefix>.<tag><ctx>.<suffix> of one output.
struct CtxFiles {
    OutFile own[3];
    FILE* f[3] = {nullptr, nullptr, nullptr};
    // false (message printed) if one of them cannot be opened
    bool open(const std::string& prefix, const std::string& tag, const char* suffix) {
        for (int c = 0; c < 3; ++c) {
            own[c] = open_out(prefix + "." + tag + CTX_NAME[c] + suffix);
            if (!(f[c] = own[c].get())) return false;
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
    OutFile out = open_out(o.prefix + ".linkage.CpG.tsv");
    if (!out) return false;
    FILE* f = out.get();
    fprintf(f, "#dist\tn\tn_uu\tn_um\tn_mu\tn_mm\tconcordance\tr\n");
    for (int64_t i = 0; i < n; ++i) {
        const hm_linkage_t& r = rows[(size_t)i];
        double st[2] = {NAN, NAN};
        hm_linkage_stats(&r, st);
        fprintf(f, "%u\t%llu\t%llu\t%llu\t%llu\t%llu\t%.6g\t%.6g\n", r.dist, (unsigned long long)(r.n_uu + r.n_um + r.n_mu + r.n_mm),
                (unsigned long long)r.n_uu, (unsigned long long)r.n_um, (unsigned long long)r.n_mu, (unsigned long long)r.n_mm, st[0], st[1]);
    }
    return fclose(out.release()) == 0;
}

// <prefix>.readpos.tsv: the header, then one row per context and bin with at least -y calls; percent as cov.bed's fourth column,
// both statistics hm_readpos_stats' (a row without calls, written under -y 0, has none: nan).  false on an engine error (recorded)
// or a file error (reported).
bool write_readpos(hm_pileup_t* pe, const PileupOptions& o) {
    std::vector<hm_readpos_t> rows(3 * (2 * (size_t)o.profile + 1));
    const int64_t n = hm_pileup_fetch_readpos(pe, o.profile_min_calls, rows.data(), (int64_t)rows.size());
    if (n < 0) return false;
    OutFile out = open_out(o.prefix + ".readpos.tsv");
    if (!out) return false;
    FILE* f = out.get();
    static const char* const end[3] = {"5p", "3p", "interior"};
    fprintf(f, "#context\tend\tdist\tn\tn_m\tn_u\tpercent\tmean_ml\n");
    for (int64_t i = 0; i < n; ++i) {
        const hm_readpos_t& r = rows[(size_t)i];
        double st[2] = {NAN, NAN};
        hm_readpos_stats(&r, st);
        fprintf(f, "%s\t%s\t%u\t%llu\t%llu\t%llu\t%g\t%.6g\n", CTX_NAME[r.motif % 3], end[r.end % 3], r.dist, (unsigned long long)(r.n_m + r.n_u),
                (unsigned long long)r.n_m, (unsigned long long)r.n_u, st[0], st[1]);
    }
    return fclose(out.release()) == 0;
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
    const OutFile out = open_out(o.prefix + ".domains.fit.tsv");
    if (!out) return 0;
    FILE* f = out.get();
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
                if (hm_pileup_domain_sums(pe, nullptr, nullptr, nullptr, 0, lo, hi, c, cur.A, cur.B, S, o.domain_max_gap, one) < 0) return -1;
                for (int k = 0; k < 6; ++k) sums[k] += one[k];
            }
            fprintf(f, "%s\t%zu\t%.17g\t%.17g\t%lld\t%lld", CTX_NAME[c], seen.size(), cur.lo, cur.hi, (long long)cur.A, (long long)cur.B);
            for (int k = 0; k < 6; ++k) fprintf(f, "\t%lld", (long long)sums[k]);
            fputc('\n', f);
            seen.push_back(cur);
            Iter next = cur;
            int64_t s_unused = 0;
            const int rc = hm_domain_refit(sums, o.domain_penalty, &next.lo, &next.hi);
            if (rc != HM_OK && rc != HM_EDATA) { fprintf(stderr, "ERROR: hm_domain_refit failed\n"); return 0; }
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
        fprintf(f, "%s\t%s\t%.17g\t%.17g\n", CTX_NAME[c], status, result.lo, result.hi);
        fprintf(stderr, "domains: %s levels fitted in %zu iteration%s (%s): %.17g:%.17g\n", CTX_NAME[c], seen.size(), seen.size() == 1 ? "" : "s", status,
                result.lo, result.hi);
        o.domain_lo[c] = result.lo;
        o.domain_hi[c] = result.hi;
        int64_t s_again = 0;
        if (hm_domain_scores(result.lo, result.hi, o.domain_penalty, &A[c], &B[c], &s_again) != HM_OK) {
            fprintf(stderr, "ERROR: the fitted %s levels are no valid pair\n", CTX_NAME[c]);
            return 0;
        }
    }
    return 1;
}

// `pileup -H -A -Q` after hm_pileup_count: the tested loci of the whole reference counted per tuple, the p of every tuple that
// occurs, the q-values (hm_asm_qvalues), then the rows of write_asm with their q looked up (56 B per row on the device and here),
// and <prefix>.asm.summary.tsv from the table's weights.  1 done, -1 engine error (hm_pileup_last_error), 0 another error (message
// printed).
int write_asm_q(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, const std::string& tag, FILE* out[3], int threads) {
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
    const OutFile f = open_out(o.prefix + "." + tag + ".summary.tsv");
    if (!f) return 0;
    for (int c = 0; c < 3; ++c)
        fprintf(f.get(), "%s\t%llu\t%llu\t%llu\n", CTX_NAME[c], (unsigned long long)m[c], (unsigned long long)below[c][0], (unsigned long long)below[c][1]);
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

// `pileup -B / -e` after hm_pileup_count: rates (measured on the control sequence `control_sid`, unless given), histogram of the
// whole reference, the table, then the rows (40 B per row on the device and here), and
// <prefix>.sites.rates.tsv.  1 done, -1 engine error (hm_pileup_last_error), 0 another error (message printed).
int write_sites(hm_pileup_t* pe, const Fasta& fa, const PileupOptions& o, int control_sid, int threads) {
    std::vector<int64_t> start(fa.names.size() + 1, 0);
    for (size_t s = 0; s < fa.names.size(); ++s) start[s + 1] = start[s] + fa.length[s];
    uint64_t sums[6] = {0, 0, 0, 0, 0, 0};
    double rates[3] = {o.rates[0], o.rates[1], o.rates[2]};
    if (control_sid >= 0) {
        if (hm_pileup_control_sums(pe, nullptr, nullptr, nullptr, start[(size_t)control_sid], start[(size_t)control_sid + 1], sums) != HM_OK) return -1;
        for (int c = 0; c < 3; ++c) rates[c] = sums[c] + sums[3 + c] ? (double)sums[c] / (double)(sums[c] + sums[3 + c]) : std::nan("");
    }
    for (int c = 0; c < 3; ++c) {
        if (std::isnan(rates[c])) fprintf(stderr, "WARNING: %s is not tested: %s\n", CTX_NAME[c], control_sid >= 0 ? "the control sequence has no calls in this context" : "its rate is nan");
        else fprintf(stderr, "%s false-positive rate: %.17g\n", CTX_NAME[c], rates[c]);
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
    const OutFile f = open_out(o.prefix + ".sites.rates.tsv");
    if (!f) return 0;
    for (int c = 0; c < 3; ++c) {
        char rate[64] = "nan";
        if (!std::isnan(rates[c])) snprintf(rate, sizeof rate, "%.17g", rates[c]);
        fprintf(f.get(), "%s\t%llu\t%llu\t%s\t%llu\n", CTX_NAME[c], (unsigned long long)sums[c], (unsigned long long)sums[3 + c], rate, (unsigned long long)m[c]);
    }
    return 1;
}

// the engine's last error behind what was being done, as the exit status
int engine_error(hm_pileup_t* pe, const std::string& what) {
    fprintf(stderr, "ERROR: %s: %s\n", what.c_str(), hm_pileup_last_error(pe));
    return EXIT_FAILURE;
}

// the engine's options from the command line's: nullptr, or what the engine refused (hm_pileup_last_error)
const char* configure_engine(hm_pileup_t* pe, const PileupOptions& o) {
    hm_pileup_set_option(pe, "min_mapq", o.min_mapq);
    hm_pileup_set_option(pe, "min_pi", o.min_pi);
    if (o.haplotypes && hm_pileup_set_option(pe, "partitions", 2) != HM_OK) return "partitions";
    if (o.patterns && (hm_pileup_set_option(pe, "patterns", o.patterns) != HM_OK || hm_pileup_set_option(pe, "pattern_span", (double)o.pattern_span) != HM_OK))
        return "patterns";
    if (o.bedmethyl && hm_pileup_set_option(pe, "bedmethyl", 1) != HM_OK) return "bedmethyl";
    if (o.linkage && hm_pileup_set_option(pe, "linkage", (double)o.linkage) != HM_OK) return "linkage";
    if (o.profile && hm_pileup_set_option(pe, "profile", (double)o.profile) != HM_OK) return "profile";
    if ((o.trim5 || o.trim3) && (hm_pileup_set_option(pe, "trim5", (double)o.trim5) != HM_OK || hm_pileup_set_option(pe, "trim3", (double)o.trim3) != HM_OK))
        return "trim";
    return nullptr;
}

// Every file of a counted engine, in the order of the options' echo: 0, or the exit status behind a printed message (-Y refits o's weights)
int write_outputs(hm_pileup_t* pe, const Fasta& fa, PileupOptions& o, const Intervals& intervals, int control_sid) {
    // one set of three files per output: the combined planes, then (-H) each partition's pcov / ncov with the combined key
    std::vector<std::string> tags{""};
    std::vector<const void*> planes{nullptr, nullptr, nullptr};
    if (o.haplotypes) {
        void* key = nullptr;
        if (hm_pileup_planes(pe, nullptr, nullptr, &key, nullptr) != HM_OK) return engine_error(pe, "planes");
        for (int part = 1; part <= 2; ++part) {
            void *pc = nullptr, *nc = nullptr;
            if (hm_pileup_partition_planes(pe, part, &pc, &nc) != HM_OK) return engine_error(pe, "partition planes");
            tags.push_back("hap" + std::to_string(part) + ".");
            planes.insert(planes.end(), {pc, nc, key});
        }
    }
    for (size_t t = 0; t < tags.size(); ++t) {
        CtxFiles out;
        if (!out.open(o.prefix, tags[t], ".cov.bed")) return EXIT_FAILURE;
        if (!write_bed(pe, fa, planes[3 * t], planes[3 * t + 1], planes[3 * t + 2], out.f, o.threads)) return engine_error(pe, "loci");
    }
    if (o.asm_test) {  // -Q and -G need -A
        const int rc = write_partition_tests(pe, fa, o, "asm");
        if (rc < 0) return engine_error(pe, rc == -1 ? "asm" : "asm regions");
        if (rc == 0) return EXIT_FAILURE;
    }
    if (o.domains) {
        if (o.domain_fit_iter) {
            const int rc = fit_domains(pe, fa, o, o.dom_A, o.dom_B, o.dom_S);
            if (rc < 0) return engine_error(pe, "domains fit");
            if (rc == 0) return EXIT_FAILURE;
        }
        CtxFiles out;
        if (!out.open(o.prefix, "domains.", ".bed")) return EXIT_FAILURE;
        if (!write_domains(pe, fa, o, o.dom_A, o.dom_B, o.dom_S, out.f)) return engine_error(pe, "domains");
    }
    if (o.patterns) {
        const OutFile f = open_out(o.prefix + ".patterns.CpG.bed");
        if (!f) return EXIT_FAILURE;
        FILE* out[3] = {f.get(), nullptr, nullptr};
        if (!write_patterns(pe, fa, o, out)) return engine_error(pe, "patterns");
    }
    for (int part = 0; o.bedmethyl && part <= (o.haplotypes ? 2 : 0); ++part) {
        const OutFile f = open_out(o.prefix + (part ? ".hap" + std::to_string(part) : std::string()) + ".bedmethyl.CpG.bed");
        if (!f) return EXIT_FAILURE;
        FILE* out[3] = {f.get(), nullptr, nullptr};
        if (!write_bedmethyl(pe, fa, o, part, out)) return engine_error(pe, "bedmethyl");
    }
    if (o.linkage && !write_linkage(pe, o)) return engine_error(pe, "linkage");
    if (o.profile && !write_readpos(pe, o)) return engine_error(pe, "readpos");
    for (size_t t = 0; !o.intervals.empty() && t < tags.size(); ++t)
        if (!write_intervals(pe, fa, o, intervals, tags[t], &planes[3 * t])) return engine_error(pe, "regions");
    for (size_t t = 0; o.context_flank >= 0 && t < tags.size(); ++t)
        if (!write_context(pe, fa, o, tags[t], &planes[3 * t])) return engine_error(pe, "context");
    if (!o.control.empty() || o.rates_given) {
        const int rc = write_sites(pe, fa, o, control_sid, o.threads);
        if (rc < 0) return engine_error(pe, "sites");
        if (rc == 0) return EXIT_FAILURE;
    }
    return 0;
}
// the `Parameters:` block on stderr
void echo_parameters(const PileupOptions& o) {
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
}

// The record loop over a mod-BAM.  0, or EXIT_FAILURE behind a printed message; the seconds of the four stages are added to t_*.
int modbam_record_loop(const PileupOptions& o, BgzfReader& in, hm_pileup_t* pe, const std::function<int(const BamRecord&)>& sid_of,
                       uint64_t& n_records, double& t_read, double& t_parse, double& t_submit, double& t_gpu) {
    using clk = std::chrono::steady_clock;
    auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    auto die = [&](const std::string& what) { return engine_error(pe, what); };
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
    return 0;
}

// -D: the integer weights of the levels (hm_domain_scores) into o; false if a pair of levels gives none
bool domain_weights(PileupOptions& o) {
    for (int c = 0; c < 3; ++c)
        if (!std::isnan(o.domain_lo[c]) && hm_domain_scores(o.domain_lo[c], o.domain_hi[c], o.domain_penalty, &o.dom_A[c], &o.dom_B[c], &o.dom_S) != HM_OK)
            return false;
    return true;
}
}  // namespace

int cmd_pileup(int argc, char** argv) {
    PileupOptions o;
    int first = 0, status = 0;
    if (!parse_command_line(CMD_PILEUP, argc, argv, o, first, status, domain_weights)) return status;
    if (o.kinetics && o.model_dir.empty()) o.model_dir = exe_dir() + "/../weights";
    o.ref = argv[first];
    o.bam = argv[first + 1];
    o.prefix = argv[first + 2];
    echo_parameters(o);

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
    auto die = [&](const std::string& what) { return engine_error(pe, what); };
    if (const char* refused = configure_engine(pe, o)) return die(refused);
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
    } else if (modbam_record_loop(o, in, pe, sid_of, n_records, t_read, t_parse, t_submit, t_gpu)) return EXIT_FAILURE;
    const auto t_loop = clk::now();

    static uint64_t bins[768];
    if (hm_pileup_histograms(pe, bins) != HM_OK) return die("histograms");
    uint8_t thr[3];
    report_thresholds(bins, thr);
    if (hm_pileup_count(pe, thr) != HM_OK) return die("count");

    if (const int rc = write_outputs(pe, fa, o, intervals, control_sid)) return rc;
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

using clk = std::chrono::steady_clock;
double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// What `diff`, `groupdiff` and `samplecorr` do before their first load.  The files are found before the reference is read and the
// engine exists: a job without input needs neither.
struct CovJob {
    std::vector<std::string> files[3];  // per context the file of every sample, in the order of `samples`; empty: context skipped
    int n_ctx = 0, threads = 1;  // -t
    Fasta fa;
    std::vector<int64_t> seq_start;
    std::unique_ptr<hm_pileup_t, decltype(&hm_pileup_destroy)> engine{nullptr, hm_pileup_destroy};  // destroyed on every way out
};

// One <prefix>.<ctx>.cov.bed, plain or gzip, with motif `motif`: read in blocks of whole lines, each block parsed by `threads` workers
// over contiguous runs of lines and handed run by run to `load`, the engine call of the command (hm_pileup_load_loci for a partition,
// hm_pileup_load_sample_loci, hm_sample_load), which answers the rows it took or an error of the job's engine.  Empty lines are skipped.  false
// with a message naming the file and, for a bad line, its number.
using LoadCall = std::function<int64_t(const hm_locus_t*, int64_t)>;
bool load_cov_bed(const CovJob& job, const std::string& path, const LoadCall& load, uint32_t motif, int threads, uint64_t& n_rows) {
    const Fasta& fa = job.fa;
    const std::vector<int64_t>& seq_start = job.seq_start;
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
            const int64_t rc = load(P.rows.data(), (int64_t)P.rows.size());
            if (rc < 0) { fprintf(stderr, "ERROR: %s: %s\n", path.c_str(), hm_pileup_last_error(job.engine.get())); ok = false; break; }
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

// A context counts if every sample has its file ("a cov.bed file of <whose>").  The engine gets `options` -- a refusal is reported
// as `what` -- and then the reference.  -> 0, or the exit status behind a message.
int open_cov_job(const PileupOptions& o, const std::vector<std::string>& samples, const char* whose, const char* what,
                 std::initializer_list<std::pair<const char*, double>> options, CovJob& job) {
    for (int c = 0; c < 3; ++c) {
        bool all = true;
        for (const std::string& s : samples) {
            job.files[c].push_back(find_cov_bed(s, CTX_NAME[c]));
            if (!job.files[c].back().empty()) continue;
            fprintf(stderr, "Skip context %s: %s.%s.cov.bed is missing\n", CTX_NAME[c], s.c_str(), CTX_NAME[c]);
            all = false;
        }
        if (all) ++job.n_ctx;
        else job.files[c].clear();
    }
    if (!job.n_ctx) { fprintf(stderr, "ERROR: no context has a cov.bed file of %s\n", whose); return EXIT_FAILURE; }
    job.threads = o.threads;
    Fasta& fa = job.fa;
    std::string err;
    if (!load_fasta(o.ref, fa, err)) { fprintf(stderr, "ERROR: %s\n", err.c_str()); return EXIT_FAILURE; }
    if (fa.names.empty()) { fprintf(stderr, "ERROR: no sequence in %s\n", o.ref.c_str()); return EXIT_FAILURE; }
    fprintf(stderr, "Load %zu sequences (%zu bases) from %s\n", fa.names.size(), fa.bases.size(), o.ref.c_str());
    job.seq_start.assign(fa.names.size() + 1, 0);
    for (size_t s = 0; s < fa.names.size(); ++s) job.seq_start[s + 1] = job.seq_start[s] + fa.length[s];

    hm_pileup_t* pe = nullptr;
    if (hm_pileup_create(&pe, o.device) != HM_OK) { fprintf(stderr, "ERROR: %s\n", hm_pileup_last_error(nullptr)); return EXIT_FAILURE; }
    job.engine.reset(pe);
    for (const auto& opt : options)
        if (hm_pileup_set_option(pe, opt.first, opt.second) != HM_OK) return engine_error(pe, what);
    if (hm_pileup_set_reference(pe, (int32_t)fa.names.size(), fa.length.data(), fa.bases.data()) != HM_OK) return engine_error(pe, "reference");
    return 0;
}

std::vector<std::string> split_list(const std::string& text) {
    std::vector<std::string> items(1);
    for (const char c : text) {
        if (c == ',') items.emplace_back();
        else items.back() += c;
    }
    return items;
}

// The samples of `samplecorr` (one comma list) or of `groupdiff` and `regiondiff` (one list per group): every element a prefix as
// `diff` takes it.  The checks print their message and answer false; each command runs them where it always has.
struct SampleSet {
    std::vector<std::string> group[2];  // the lists as given; group[1] stays empty for one list
    std::vector<std::string> sample;    // the files of a context: group 1's samples, then group 2's
    std::vector<uint8_t> member;        // the group of every sample, 1 or 2
    const int lists;
    SampleSet(const char* list1, const char* list2 = nullptr) : lists(list2 ? 2 : 1) {
        for (int g = 0; g < lists; ++g) {
            group[g] = split_list(g ? list2 : list1);
            sample.insert(sample.end(), group[g].begin(), group[g].end());
            member.insert(member.end(), group[g].size(), (uint8_t)(g + 1));
        }
    }
    // at least `min` and at most HM_SAMPLE_MAX samples in all, else the message and the command's usage
    bool count_fits(Command cmd, const char* command, size_t min, const char* argv0) const {
        if (sample.size() >= min && sample.size() <= HM_SAMPLE_MAX) return true;
        fprintf(stderr, lists == 2 ? "ERROR: %s takes 2 to %d samples in all, the lists name %zu\n" : "ERROR: %s takes 2 to %d samples, the list names %zu\n",
                command, HM_SAMPLE_MAX, sample.size());
        command_usage(cmd, argv0);
        return false;
    }
    // list by list: no empty prefix, at least min_reps samples (-r), at most max_group (0: any number)
    bool lists_fit(long long min_reps, size_t max_group) const {
        for (int g = 0; g < lists; ++g) {
            for (const std::string& s : group[g]) {
                if (!s.empty()) continue;
                if (lists == 2) fprintf(stderr, "ERROR: an empty prefix in the list of group %d\n", g + 1);
                else fprintf(stderr, "ERROR: an empty prefix in the list of samples\n");
                return false;
            }
            if ((long long)group[g].size() < min_reps) {
                fprintf(stderr, "ERROR: group %d has %zu samples, fewer than -r %lld\n", g + 1, group[g].size(), min_reps);
                return false;
            }
            if (max_group && group[g].size() > max_group) { fprintf(stderr, "ERROR: group %d has more than %zu samples\n", g + 1, max_group); return false; }
        }
        return true;
    }
    void echo() const {
        for (int g = 0; g < lists; ++g)
            for (size_t i = 0; i < group[g].size(); ++i) {
                if (lists == 2) fprintf(stderr, "group %d ", g + 1);
                fprintf(stderr, "sample %zu: %s.<ctx>.cov.bed\n", i + 1, group[g][i].c_str());
            }
    }
};

// Every sample of the set in turn: open_sample(i) announces it to the engine (0, or the exit status behind its message), then the
// files of its contexts go through `load`, their rows counted in n_rows_of(i).  A sample's contexts share its plane or seen
// bitmap: one locus, one context.  -> 0, or the exit status behind a message.
int load_samples(const CovJob& job, const SampleSet& set, const std::function<int(size_t)>& open_sample, const LoadCall& load,
                 const std::function<uint64_t&(size_t)>& n_rows_of) {
    for (size_t i = 0; i < set.sample.size(); ++i) {
        if (const int failed = open_sample(i)) return failed;
        for (int c = 0; c < 3; ++c)
            if (!job.files[c].empty() && !load_cov_bed(job, job.files[c][i], load, (uint32_t)c, job.threads, n_rows_of(i))) return EXIT_FAILURE;
    }
    return 0;
}

}  // namespace

int cmd_diff(int argc, char** argv) {
    PileupOptions o;
    int first = 0, status = 0;
    if (!parse_command_line(CMD_DIFF, argc, argv, o, first, status)) return status;
    o.ref = argv[first];
    const std::vector<std::string> sample = {argv[first + 1], argv[first + 2]};
    o.prefix = argv[first + 3];
    fprintf(stderr, "\n\n====================> Parameters:\nCPU threads: %d\nGenomic reference: %s\nsample 1: %s.<ctx>.cov.bed\nsample 2: %s.<ctx>.cov.bed\n"
                    "output prefix: %s\ndiff: min sample coverage %d -> %s.diff.*\n",
            o.threads, o.ref.c_str(), sample[0].c_str(), sample[1].c_str(), o.prefix.c_str(), o.asm_min_cov, o.prefix.c_str());
    if (o.asm_q) fprintf(stderr, "diff: Benjamini-Hochberg q-values per context -> tenth column, %s.diff.summary.tsv\n", o.prefix.c_str());
    if (o.asm_regions)
        fprintf(stderr, "diff: regions of >= %d loci with p <= %g and one sign, gaps <= %lld -> %s.diff.regions.*\n", o.region_min_loci, o.region_max_p,
                o.region_max_gap, o.prefix.c_str());
    fprintf(stderr, "\n\n");

    const auto t_start = clk::now();
    CovJob job;
    if (const int failed = open_cov_job(o, sample, "both samples", "partitions", {{"partitions", 2}}, job)) return failed;
    hm_pileup_t* pe = job.engine.get();
    uint64_t n_rows[2] = {0, 0};
    for (int c = 0; c < 3; ++c)
        for (int s = 0; s < 2 && !job.files[c].empty(); ++s) {
            const LoadCall load = [&](const hm_locus_t* rows, int64_t n) { return hm_pileup_load_loci(pe, s + 1, rows, n); };
            if (!load_cov_bed(job, job.files[c][(size_t)s], load, (uint32_t)c, o.threads, n_rows[s])) return EXIT_FAILURE;
        }
    const auto t_load = clk::now();
    const int rc = write_partition_tests(pe, job.fa, o, "diff");
    if (rc < 0) return engine_error(pe, rc == -1 ? "diff" : "diff regions");
    if (rc == 0) return EXIT_FAILURE;
    job.engine.reset();
    fprintf(stderr, "## %llu + %llu covered loci of %d contexts in %.2f s: parse + load %.2f s; test + BED %.2f s\n", (unsigned long long)n_rows[0],
            (unsigned long long)n_rows[1], job.n_ctx, secs(t_start, clk::now()), secs(t_start, t_load), secs(t_load, clk::now()));
    return 0;
}

// ---- smooth [OPTIONS] reference prefix out-prefix (ours) ------------------------------------------------------------------------------
// Kernel-smoothed levels of one sample: the rows of <prefix>.<ctx>.cov.bed go into the engine's partition 1 as `diff` loads them,
// and per context with a file the rows of hm_smooth_fetch are written sequence by sequence, the chunks `diff` fetches in
// (DESIGN.md section 10).
int cmd_smooth(int argc, char** argv) {
    PileupOptions o;
    int first = 0, status = 0;
    if (!parse_command_line(CMD_SMOOTH, argc, argv, o, first, status)) return status;
    o.ref = argv[first];
    const std::vector<std::string> sample = {argv[first + 1]};
    o.prefix = argv[first + 2];
    const int32_t h = (int32_t)o.smooth_half_width, min_cov = (int32_t)o.smooth_min_cov;
    fprintf(stderr, "\n\n====================> Parameters:\nCPU threads: %d\nGenomic reference: %s\nsample: %s.<ctx>.cov.bed\noutput prefix: %s\n"
                    "smooth: triangular kernel of half-width %d, min coverage %d, min loci per window %lld -> %s.smooth.*\n\n\n",
            o.threads, o.ref.c_str(), sample[0].c_str(), o.prefix.c_str(), h, min_cov, o.smooth_min_loci, o.prefix.c_str());

    const auto t_start = clk::now();
    CovJob job;
    if (const int failed = open_cov_job(o, sample, "the sample", "partitions", {{"partitions", 2}}, job)) return failed;
    hm_pileup_t* pe = job.engine.get();
    uint64_t n_rows = 0;
    const LoadCall load = [&](const hm_locus_t* rows, int64_t n) { return hm_pileup_load_loci(pe, 1, rows, n); };
    for (int c = 0; c < 3; ++c)
        if (!job.files[c].empty() && !load_cov_bed(job, job.files[c][0], load, (uint32_t)c, o.threads, n_rows)) return EXIT_FAILURE;
    const auto t_load = clk::now();

    uint64_t counting[3] = {0, 0, 0}, written[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c) {
        if (job.files[c].empty()) continue;
        const OutFile f = open_out(o.prefix + ".smooth." + CTX_NAME[c] + ".bed");
        if (!f) return EXIT_FAILURE;
        FILE* const out[3] = {f.get(), f.get(), f.get()};
        std::atomic<bool> ok{true};
        const bool done = write_rows<hm_smooth_t>(
            job.fa, out, o.threads,
            [&](int64_t lo, int64_t hi, hm_smooth_t* dst, int64_t cap) -> int64_t {
                const int64_t n = hm_smooth_fetch(pe, 1, c, lo, hi, h, min_cov, o.smooth_min_loci, dst, cap);
                if (dst || n < 0) return n;
                // the first of the two calls per sequence: the counting loci are the rows under -i 1
                const int64_t all = o.smooth_min_loci > 1 ? hm_smooth_fetch(pe, 1, c, lo, hi, h, min_cov, 1, nullptr, 0) : n;
                if (all < 0) return all;
                counting[c] += (uint64_t)all;
                written[c] += (uint64_t)n;
                return n;
            },
            [&](const hm_smooth_t& r, int64_t k, char (&buf)[320]) {
                double st[2] = {0, 0};
                if (hm_smooth_stats(&r, h, st) != HM_OK) ok = false;
                return snprintf(buf, sizeof buf, "\t%lld\t%lld\t%g\t%d\t%d\t%lld\t%.3f\n", (long long)k, (long long)k + 1, st[0], r.pcov, r.ncov,
                                (long long)r.loci, st[1]);
            });
        if (!done) return engine_error(pe, "smooth");
        if (!ok) { fprintf(stderr, "ERROR: smooth: a row without a call in its window\n"); return EXIT_FAILURE; }
    }
    const OutFile summary = open_out(o.prefix + ".smooth.summary.tsv");
    if (!summary) return EXIT_FAILURE;
    for (int c = 0; c < 3; ++c)
        if (!job.files[c].empty())
            fprintf(summary.get(), "%s\t%llu\t%llu\t%d\n", CTX_NAME[c], (unsigned long long)counting[c], (unsigned long long)written[c], h);
    job.engine.reset();
    fprintf(stderr, "## %llu covered loci of %d contexts in %.2f s: parse + load %.2f s; smooth + BED %.2f s\n", (unsigned long long)n_rows, job.n_ctx,
            secs(t_start, clk::now()), secs(t_start, t_load), secs(t_load, clk::now()));
    return 0;
}

// ---- groupdiff [OPTIONS] reference a1,a2,... b1,b2,... out-prefix (ours) --------------------------------------------------------------
// Differential methylation between two groups of replicates: every list element is a prefix as `diff` takes it, every sample is
// loaded as one sample of its group (hm_pileup_group_sample, hm_pileup_load_sample_loci), and the loci with at least -r counting
// samples on both sides are tested with the spread between the replicates (hm_pileup_fetch_groups).  The rows
// of the whole reference wait on the host (64 B each) for their q-values (hm_group_qvalues) and are then written.
namespace {
struct GroupQRow {  // what write_rows formats: the row and its q, named by gpos and motif as every row
    int64_t gpos;
    uint32_t motif;
    const hm_group_t* g;
    double q;
};

// What `groupdiff` and `groupdmr` share up to the first fetch: the lists checked against -r, the engine with the groups planes, and
// every sample loaded as one sample of its group; n_rows[g] = the counting loci group g + 1 added.  -> 0, or the exit status
// behind a message.
int load_groups(const PileupOptions& o, const SampleSet& set, CovJob& job, uint64_t n_rows[2]) {
    if (!set.lists_fit(o.group_min_reps, 255)) return EXIT_FAILURE;
    if (const int failed = open_cov_job(o, set.sample, "every sample", "groups",
                                        {{"partitions", 2}, {"groups", 1}, {"group_min_cov", (double)o.group_min_cov}}, job))
        return failed;
    hm_pileup_t* pe = job.engine.get();
    return load_samples(
        job, set, [&](size_t i) { return hm_pileup_group_sample(pe, set.member[i]) < 0 ? engine_error(pe, "group sample") : 0; },
        [&](const hm_locus_t* rows, int64_t n) { return hm_pileup_load_sample_loci(pe, rows, n); }, [&](size_t i) -> uint64_t& { return n_rows[set.member[i] - 1]; });
}

// The tested loci of the whole reference, sequence by sequence, appended to `rows` (64 B each).  false on an engine error.
bool fetch_group_rows(const CovJob& job, int32_t min_reps, std::vector<hm_group_t>& rows) {
    hm_pileup_t* pe = job.engine.get();
    const std::vector<int64_t>& seq_start = job.seq_start;
    for (size_t s = 0; s < job.fa.names.size(); ++s) {
        const int64_t n = hm_pileup_fetch_groups(pe, seq_start[s], seq_start[s + 1], min_reps, nullptr, 0);
        if (n < 0) return false;
        if (n == 0) continue;
        rows.resize(rows.size() + (size_t)n);
        if (hm_pileup_fetch_groups(pe, seq_start[s], seq_start[s + 1], min_reps, rows.data() + rows.size() - n, n) != n) return false;
    }
    return true;
}

// <prefix>.groups.<ctx>.bed and <prefix>.groups.summary.tsv from the tested loci of the job, their q-values and m[ctx] =
// the tested loci per context (hm_group_qvalues).  false, behind a message, for a file that cannot be opened.
bool write_group_loci(const PileupOptions& o, const Fasta& fa, const std::vector<hm_group_t>& rows, const std::vector<double>& q, const uint64_t m[3]) {
    {
        CtxFiles out;
        if (!out.open(o.prefix, "groups.", ".bed")) return false;
        write_rows<GroupQRow>(
            fa, out.f, o.threads,
            [&](int64_t lo, int64_t hi, GroupQRow* dst, int64_t cap) {  // the rows are ascending in gpos
                const auto at = [&](int64_t g) {
                    return std::lower_bound(rows.begin(), rows.end(), g, [](const hm_group_t& r, int64_t v) { return r.gpos < v; }) - rows.begin();
                };
                const int64_t a = at(lo), b = at(hi);
                for (int64_t i = a; dst && b - a <= cap && i < b; ++i) dst[i - a] = GroupQRow{rows[(size_t)i].gpos, rows[(size_t)i].motif, &rows[(size_t)i], q[(size_t)i]};
                return b - a;
            },
            [](const GroupQRow& r, int64_t k, char (&buf)[320]) {
                const hm_group_t& g = *r.g;
                return snprintf(buf, sizeof buf, "\t%lld\t%lld\t%g\t%.6g\t%.6g\t%d\t%d\t%d\t%d\t%d\t%d\t%.6g\n", (long long)k, (long long)k + 1, g.diff,
                                g.pvalue, r.q, (int)g.m1, g.pcov1, g.ncov1, (int)g.m2, g.pcov2, g.ncov2, g.phi);
            });
    }
    uint64_t tally[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};  // loci with q <= 0.05, q <= 0.01, phi > 1
    for (size_t i = 0; i < rows.size(); ++i) {
        const uint32_t c = std::min(rows[i].motif, 2u);
        tally[c][0] += q[i] <= 0.05;
        tally[c][1] += q[i] <= 0.01;
        tally[c][2] += rows[i].phi > 1.0;
    }
    const OutFile f = open_out(o.prefix + ".groups.summary.tsv");
    if (!f) return false;
    for (int c = 0; c < 3; ++c)
        fprintf(f.get(), "%s\t%llu\t%llu\t%llu\t%llu\n", CTX_NAME[c], (unsigned long long)m[c], (unsigned long long)tally[c][0], (unsigned long long)tally[c][1],
                (unsigned long long)tally[c][2]);
    return true;
}
}  // namespace

int cmd_groupdiff(int argc, char** argv) {
    PileupOptions o;
    int first = 0, status = 0;
    if (!parse_command_line(CMD_GROUPDIFF, argc, argv, o, first, status)) return status;
    o.ref = argv[first];
    const SampleSet set(argv[first + 1], argv[first + 2]);
    o.prefix = argv[first + 3];
    fprintf(stderr, "\n\n====================> Parameters:\nCPU threads: %d\nGenomic reference: %s\n", o.threads, o.ref.c_str());
    set.echo();
    fprintf(stderr, "output prefix: %s\ngroupdiff: min sample coverage %lld, min replicates per group %lld -> %s.groups.*\n\n\n", o.prefix.c_str(),
            o.group_min_cov, o.group_min_reps, o.prefix.c_str());

    const auto t_start = clk::now();
    CovJob job;
    uint64_t n_rows[2] = {0, 0};
    if (const int failed = load_groups(o, set, job, n_rows)) return failed;
    const auto t_load = clk::now();

    std::vector<hm_group_t> rows;
    if (!fetch_group_rows(job, (int32_t)o.group_min_reps, rows)) return engine_error(job.engine.get(), "groups");
    job.engine.reset();
    std::vector<double> q(rows.size());
    uint64_t m[3];
    if (hm_group_qvalues(rows.data(), (int64_t)rows.size(), q.data(), m) != HM_OK) {
        fprintf(stderr, "ERROR: groupdiff: the tested loci are not rows the engine wrote\n");
        return EXIT_FAILURE;
    }
    if (!write_group_loci(o, job.fa, rows, q, m)) return EXIT_FAILURE;
    fprintf(stderr, "## %zu + %zu samples, %llu + %llu counting loci of %d contexts, %zu tested in %.2f s: parse + load %.2f s; test + BED %.2f s\n",
            set.group[0].size(), set.group[1].size(), (unsigned long long)n_rows[0], (unsigned long long)n_rows[1], job.n_ctx, rows.size(), secs(t_start, clk::now()),
            secs(t_start, t_load), secs(t_load, clk::now()));
    return 0;
}

// ---- groupdmr [OPTIONS] reference a1,a2,... b1,b2,... out-prefix (ours) ---------------------------------------------------------------
// Differentially methylated regions between two groups of replicates: loaded as `groupdiff` loads, then per sequence and context
// the tested loci are chained on the device (hm_dmr_fetch_regions).  Only the regions come to the
// host, unless -F (the q-values need every p of the job: hm_group_qvalues, hm_dmr_p_cutoff) or -L (the loci are an output) ask
// for the rows.
int cmd_groupdmr(int argc, char** argv) {
    PileupOptions o;
    int first = 0, status = 0;
    if (!parse_command_line(CMD_GROUPDMR, argc, argv, o, first, status)) return status;
    o.ref = argv[first];
    const SampleSet set(argv[first + 1], argv[first + 2]);
    o.prefix = argv[first + 3];
    const bool by_q = o.dmr_max_q > 0.0;
    fprintf(stderr, "\n\n====================> Parameters:\nCPU threads: %d\nGenomic reference: %s\n", o.threads, o.ref.c_str());
    set.echo();
    fprintf(stderr, "output prefix: %s\ngroupdmr: min sample coverage %lld, min replicates per group %lld; regions of >= %lld loci with %s <= %g, |diff| >= %g and one sign, "
                    "gaps <= %lld -> %s.groupdmr.*\n", o.prefix.c_str(), o.group_min_cov, o.group_min_reps, o.dmr_min_loci, by_q ? "q" : "p",
            by_q ? o.dmr_max_q : o.dmr_max_p, o.dmr_min_diff, o.dmr_max_gap, o.prefix.c_str());
    if (o.dmr_loci) fprintf(stderr, "groupdmr: the tested loci as `groupdiff` writes them -> %s.groups.*\n", o.prefix.c_str());
    fprintf(stderr, "\n\n");

    const auto t_start = clk::now();
    CovJob job;
    uint64_t n_rows[2] = {0, 0};
    if (const int failed = load_groups(o, set, job, n_rows)) return failed;
    hm_pileup_t* pe = job.engine.get();
    const Fasta& fa = job.fa;
    const auto t_load = clk::now();

    double cutoff[3] = {o.dmr_max_p, o.dmr_max_p, o.dmr_max_p};
    uint64_t tested[3] = {0, 0, 0};
    if (by_q || o.dmr_loci) {
        std::vector<hm_group_t> rows;
        if (!fetch_group_rows(job, (int32_t)o.group_min_reps, rows)) return engine_error(pe, "groups");
        std::vector<double> q(rows.size());
        if (hm_group_qvalues(rows.data(), (int64_t)rows.size(), q.data(), tested) != HM_OK ||
            (by_q && hm_dmr_p_cutoff(rows.data(), q.data(), (int64_t)rows.size(), o.dmr_max_q, cutoff) != HM_OK)) {
            fprintf(stderr, "ERROR: groupdmr: the tested loci are not rows the engine wrote\n");
            return EXIT_FAILURE;
        }
        if (o.dmr_loci && !write_group_loci(o, fa, rows, q, tested)) return EXIT_FAILURE;
    }

    CtxFiles out;
    if (!out.open(o.prefix, "groupdmr.", ".bed")) return EXIT_FAILURE;
    uint64_t hits[3] = {0, 0, 0}, regions[3] = {0, 0, 0}, loci[3] = {0, 0, 0}, plus[3] = {0, 0, 0};
    std::vector<hm_group_region_t> rows;
    for (int c = 0; c < 3; ++c) {
        if (!(cutoff[c] > 0.0)) continue;  // -F and no locus under it: nothing to chain
        uint64_t in_ctx = 0;
        for (size_t s = 0; s < fa.names.size(); ++s) {
            const int64_t lo = job.seq_start[s], hi = job.seq_start[s + 1];
            int64_t R = 0, H = 0;
            const auto fetch = [&](hm_group_region_t* dst, int64_t cap) {
                return hm_dmr_fetch_regions(pe, lo, hi, (int32_t)o.group_min_reps, c, cutoff[c], o.dmr_min_diff, o.dmr_max_gap,
                                            (int32_t)o.dmr_min_loci, 0, &R, &H, dst, cap);
            };
            int64_t n = fetch(nullptr, 0);
            if (n > 0) {
                rows.resize((size_t)n);
                n = fetch(rows.data(), n);
            }
            if (n < 0) return engine_error(pe, "group regions");
            in_ctx += (uint64_t)R;
            hits[c] += (uint64_t)H;
            for (int64_t i = 0; i < n; ++i) {
                const hm_group_region_t& r = rows[(size_t)i];
                fprintf(out.f[c], "%s\t%lld\t%lld\t%s_%llu\t%d\t.\t%c\t%g\t%.6g\t%d\t%lld\t%lld\t%d\t%lld\t%lld\t%.6g\n", fa.names[s].c_str(),
                        (long long)(r.start - lo), (long long)(r.end - lo), CTX_NAME[c], (unsigned long long)++regions[c], r.n_loci, r.sign > 0 ? '+' : '-',
                        r.diff, r.pmin, (int)r.m1_min, (long long)r.pcov1, (long long)r.ncov1, (int)r.m2_min, (long long)r.pcov2, (long long)r.ncov2, r.phi_max);
                loci[c] += (uint64_t)r.n_loci;
                plus[c] += r.sign > 0;
            }
        }
        tested[c] = in_ctx;
    }
    job.engine.reset();
    const OutFile f = open_out(o.prefix + ".groupdmr.summary.tsv");
    if (!f) return EXIT_FAILURE;
    for (int c = 0; c < 3; ++c) {
        char cut[32] = "nan";
        if (cutoff[c] > 0.0) snprintf(cut, sizeof cut, "%.6g", cutoff[c]);
        fprintf(f.get(), "%s\t%llu\t%llu\t%s\t%llu\t%llu\t%llu\t%llu\n", CTX_NAME[c], (unsigned long long)tested[c], (unsigned long long)hits[c], cut,
                (unsigned long long)regions[c], (unsigned long long)loci[c], (unsigned long long)plus[c], (unsigned long long)(regions[c] - plus[c]));
    }
    fprintf(stderr, "## %zu + %zu samples, %llu + %llu counting loci of %d contexts, %llu regions in %.2f s: parse + load %.2f s; regions + BED %.2f s\n",
            set.group[0].size(), set.group[1].size(), (unsigned long long)n_rows[0], (unsigned long long)n_rows[1], job.n_ctx,
            (unsigned long long)(regions[0] + regions[1] + regions[2]), secs(t_start, clk::now()), secs(t_start, t_load), secs(t_load, clk::now()));
    return 0;
}

// ---- samplecorr [OPTIONS] reference s1,s2,...,sN out-prefix (ours) -------------------------------------------------------------------
// The sample-by-sample correlation matrix per context: every list element is a prefix as `diff` takes it, every sample's rows go
// into its own level plane (hm_sample_open, hm_sample_load), and one fetch over the whole reference gives the exact
// integer sums of every pair (hm_sample_fetch_sums), from which hm_sample_corr makes r and the means.
int cmd_samplecorr(int argc, char** argv) {
    PileupOptions o;
    int first = 0, status = 0;
    if (!parse_command_line(CMD_SAMPLECORR, argc, argv, o, first, status)) return status;
    o.ref = argv[first];
    const SampleSet set(argv[first + 1]);
    const std::vector<std::string>& sample = set.sample;
    o.prefix = argv[first + 2];
    const int N = (int)sample.size();
    if (!set.count_fits(CMD_SAMPLECORR, "samplecorr", 2, argv[0]) || !set.lists_fit(0, 0)) return EXIT_FAILURE;  // before any file is opened
    fprintf(stderr, "\n\n====================> Parameters:\nCPU threads: %d\nGenomic reference: %s\n", o.threads, o.ref.c_str());
    set.echo();
    fprintf(stderr, "output prefix: %s\nsamplecorr: min sample coverage %lld, %s -> %s.samplecorr.*\n\n\n", o.prefix.c_str(), o.sample_min_cov,
            o.sample_complete ? "loci where all samples count" : "loci where both samples of a pair count", o.prefix.c_str());

    const auto t_start = clk::now();
    CovJob job;
    if (const int failed = open_cov_job(o, sample, "every sample", "samples", {{"samples", (double)N}, {"sample_min_cov", (double)o.sample_min_cov}}, job))
        return failed;
    hm_pileup_t* pe = job.engine.get();
    auto die = [&](const std::string& what) { return engine_error(pe, what); };
    uint64_t n_rows = 0;
    if (const int failed = load_samples(
            job, set, [&](size_t) { return hm_sample_open(pe) < 0 ? die("sample") : 0; },
            [&](const hm_locus_t* rows, int64_t n) { return hm_sample_load(pe, rows, n); }, [&](size_t) -> uint64_t& { return n_rows; }))
        return failed;
    const auto t_load = clk::now();

    // the samples file always reports a sample's own counting loci: the diagonal of the pairwise sums
    const size_t pairs = (size_t)N * (size_t)(N + 1) / 2;
    std::vector<hm_sample_pair_t> own(3 * pairs), sums;
    if (hm_sample_fetch_sums(pe, 0, job.seq_start.back(), 0, own.data()) != (int64_t)own.size()) return die("sample sums");
    if (o.sample_complete) {
        sums.resize(own.size());
        if (hm_sample_fetch_sums(pe, 0, job.seq_start.back(), 1, sums.data()) != (int64_t)sums.size()) return die("sample sums");
    }
    job.engine.reset();
    const std::vector<hm_sample_pair_t>& e = o.sample_complete ? sums : own;
    std::vector<double> r(e.size()), mi(e.size()), mj(e.size()), own_mean(own.size());
    if (hm_sample_corr(e.data(), (int64_t)e.size(), r.data(), mi.data(), mj.data()) != HM_OK ||
        hm_sample_corr(own.data(), (int64_t)own.size(), nullptr, own_mean.data(), nullptr) != HM_OK) {
        fprintf(stderr, "ERROR: samplecorr: hm_sample_corr refused the sums\n");
        return EXIT_FAILURE;
    }
    // entry of context c and pair i <= j: context-major, then i, then j
    const auto at = [&](int c, int i, int j) { return (size_t)c * pairs + (size_t)i * (size_t)N - (size_t)i * (size_t)(i - 1) / 2 + (size_t)(j - i); };
    const OutFile samples_file = open_out(o.prefix + ".samplecorr.samples.tsv");
    if (!samples_file) return EXIT_FAILURE;
    FILE* fs = samples_file.get();
    fprintf(fs, "ctx\tsample\tn\tmean\n");
    for (int c = 0; c < 3; ++c) {
        if (job.files[c].empty()) continue;
        for (int i = 0; i < N; ++i)
            fprintf(fs, "%s\t%s\t%llu\t%.6g\n", CTX_NAME[c], sample[(size_t)i].c_str(), (unsigned long long)own[at(c, i, i)].n, own_mean[at(c, i, i)]);
        OutFile table = open_out(o.prefix + ".samplecorr." + CTX_NAME[c] + ".tsv");
        if (!table) return EXIT_FAILURE;
        FILE* f = table.get();
        fprintf(f, "sample_i\tsample_j\tn\tmean_i\tmean_j\tr\n");
        for (int i = 0; i < N; ++i)
            for (int j = i + 1; j < N; ++j) {
                const size_t k = at(c, i, j);
                fprintf(f, "%s\t%s\t%llu\t%.6g\t%.6g\t%.6g\n", sample[(size_t)i].c_str(), sample[(size_t)j].c_str(), (unsigned long long)e[k].n, mi[k], mj[k], r[k]);
            }
        table = open_out(o.prefix + ".samplecorr." + CTX_NAME[c] + ".matrix.tsv");
        if (!table) return EXIT_FAILURE;
        f = table.get();
        fprintf(f, "sample");
        for (const std::string& s : sample) fprintf(f, "\t%s", s.c_str());
        fputc('\n', f);
        for (int i = 0; i < N; ++i) {
            fputs(sample[(size_t)i].c_str(), f);
            for (int j = 0; j < N; ++j) fprintf(f, "\t%.6g", r[at(c, std::min(i, j), std::max(i, j))]);
            fputc('\n', f);
        }
    }
    fprintf(stderr, "## %d samples, %llu rows of %d contexts in %.2f s: parse + load %.2f s; sums + tables %.2f s\n", N, (unsigned long long)n_rows, job.n_ctx,
            secs(t_start, clk::now()), secs(t_start, t_load), secs(t_load, clk::now()));
    return 0;
}

// ---- regiondiff -R intervals.bed [OPTIONS] reference a1,a2,... b1,b2,... out-prefix (ours) ------------------------------------------
// Two groups of replicates tested over given intervals: every sample's rows go into its own level plane as `samplecorr` loads
// them, group 1's samples first; per context the intervals are fetched in chunks (hm_sample_fetch_intervals: per interval and
// sample the counting loci and the sum of their levels, exact), tested on the host (hm_sample_interval_test: Welch's t-test on the
// samples' interval levels) and given q-values among the tested intervals of the context (hm_sample_qvalues).
namespace {
// %.6g, with every NaN as `nan` whatever its sign
std::string g6(double v) {
    if (v != v) return "nan";
    char buf[40];
    snprintf(buf, sizeof buf, "%.6g", v);
    return buf;
}
}  // namespace

int cmd_regiondiff(int argc, char** argv) {
    PileupOptions o;
    int first = 0, status = 0;
    if (!parse_command_line(CMD_REGIONDIFF, argc, argv, o, first, status)) return status;
    o.ref = argv[first];
    const SampleSet set(argv[first + 1], argv[first + 2]);
    o.prefix = argv[first + 3];
    const size_t N = set.sample.size();
    if (!set.count_fits(CMD_REGIONDIFF, "regiondiff", 0, argv[0]) || !set.lists_fit(o.region_min_reps, 0)) return EXIT_FAILURE;  // before any file is opened
    fprintf(stderr, "\n\n====================> Parameters:\nCPU threads: %d\nGenomic reference: %s\nintervals: %s\n", o.threads, o.ref.c_str(), o.intervals.c_str());
    set.echo();
    fprintf(stderr, "output prefix: %s\nregiondiff: min sample coverage %lld, min loci per sample %lld, min samples per group %lld, %s -> %s.regiondiff.*\n\n\n",
            o.prefix.c_str(), o.sample_min_cov, o.region_min_sample_loci, o.region_min_reps,
            o.sample_complete ? "loci where all samples count" : "loci where the sample counts", o.prefix.c_str());

    const auto t_start = clk::now();
    CovJob job;
    if (const int failed = open_cov_job(o, set.sample, "every sample", "samples", {{"samples", (double)N}, {"sample_min_cov", (double)o.sample_min_cov}}, job))
        return failed;
    hm_pileup_t* pe = job.engine.get();
    const Fasta& fa = job.fa;
    auto die = [&](const std::string& what) { return engine_error(pe, what); };
    Intervals iv;
    if (!read_intervals(o.intervals, fa, iv)) return EXIT_FAILURE;
    const size_t n = iv.sid.size();
    std::vector<int64_t> start(n), end(n);
    for (size_t i = 0; i < n; ++i) {
        start[i] = job.seq_start[(size_t)iv.sid[i]] + iv.start[i];
        end[i] = job.seq_start[(size_t)iv.sid[i]] + iv.end[i];
    }
    uint64_t n_rows = 0;
    if (const int failed = load_samples(
            job, set, [&](size_t) { return hm_sample_open(pe) < 0 ? die("sample") : 0; },
            [&](const hm_locus_t* rows, int64_t k) { return hm_sample_load(pe, rows, k); }, [&](size_t) -> uint64_t& { return n_rows; }))
        return failed;
    const auto t_load = clk::now();

    // the sums of a chunk of intervals wait on the host, 16 N bytes each: chunks of at most 512 MB whatever the file's length
    const size_t chunk = std::max<size_t>(1, (size_t(1) << 29) / (sizeof(hm_sample_interval_t) * N));
    std::vector<hm_sample_interval_t> sums(std::min(chunk, n) * N);
    std::vector<hm_sample_test_t> tests[3];
    std::vector<double> q[3];
    for (int c = 0; c < 3; ++c) {
        if (job.files[c].empty()) continue;
        tests[c].resize(n);
        for (size_t a = 0; a < n; a += chunk) {
            const size_t m = std::min(chunk, n - a);
            if (hm_sample_fetch_intervals(pe, 0, job.seq_start.back(), c, o.sample_complete ? 1 : 0, start.data() + a, end.data() + a, (int64_t)m,
                                          sums.data()) != (int64_t)(m * N))
                return die("interval sums");
            if (hm_sample_interval_test(sums.data(), (int64_t)m, (int32_t)N, set.member.data(), o.region_min_sample_loci, (int32_t)o.region_min_reps,
                                        tests[c].data() + a) != HM_OK) {
                fprintf(stderr, "ERROR: regiondiff: hm_sample_interval_test refused the sums\n");
                return EXIT_FAILURE;
            }
        }
        std::vector<double> pv(n);
        for (size_t i = 0; i < n; ++i) pv[i] = tests[c][i].pvalue;
        q[c].resize(n);
        if (hm_sample_qvalues(pv.data(), (int64_t)n, q[c].data()) != HM_OK) {
            fprintf(stderr, "ERROR: regiondiff: hm_sample_qvalues refused the p-values\n");
            return EXIT_FAILURE;
        }
    }
    job.engine.reset();
    const OutFile summary = open_out(o.prefix + ".regiondiff.summary.tsv");
    if (!summary) return EXIT_FAILURE;
    FILE* fs = summary.get();
    fprintf(fs, "ctx\tintervals\ttested\tq<=0.05\tq<=0.01\n");
    size_t tested_all = 0;
    for (int c = 0; c < 3; ++c) {
        if (job.files[c].empty()) continue;
        const OutFile table = open_out(o.prefix + ".regiondiff." + CTX_NAME[c] + ".tsv");
        if (!table) return EXIT_FAILURE;
        FILE* f = table.get();
        fprintf(f, "#chrom\tstart\tend\tname\tstrand\tm1\tm2\tloci1\tloci2\tmean1\tmean2\tdiff\tt\tdf\tp\tq\n");
        unsigned long long tested = 0, q05 = 0, q01 = 0;
        for (size_t i = 0; i < n; ++i) {
            const hm_sample_test_t& r = tests[c][i];
            fprintf(f, "%s\t%lld\t%lld\t%s\t%c\t%d\t%d\t%llu\t%llu\t%s\t%s\t%s\t%s\t%s\t%s\t%s\n", fa.names[(size_t)iv.sid[i]].c_str(), (long long)iv.start[i],
                    (long long)iv.end[i], iv.name[i].c_str(), iv.strand[i], r.m1, r.m2, (unsigned long long)r.n1, (unsigned long long)r.n2, g6(r.mean1).c_str(),
                    g6(r.mean2).c_str(), g6(r.mean1 - r.mean2).c_str(), g6(r.t).c_str(), g6(r.df).c_str(), g6(r.pvalue).c_str(), g6(q[c][i]).c_str());
            tested += r.t == r.t;
            q05 += q[c][i] <= 0.05;
            q01 += q[c][i] <= 0.01;
        }
        fprintf(fs, "%s\t%zu\t%llu\t%llu\t%llu\n", CTX_NAME[c], n, tested, q05, q01);
        tested_all += tested;
    }
    fprintf(stderr, "## %zu + %zu samples, %llu rows of %d contexts, %zu intervals, %zu tests in %.2f s: parse + load %.2f s; sums + tests + tables %.2f s\n",
            set.group[0].size(), set.group[1].size(), (unsigned long long)n_rows, job.n_ctx, n, tested_all, secs(t_start, clk::now()), secs(t_start, t_load),
            secs(t_load, clk::now()));
    return 0;
}
