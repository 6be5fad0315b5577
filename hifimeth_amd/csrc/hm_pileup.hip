// hm_pileup.hip -- `hifimeth pileup` on gfx950: alignment projection of the per-read 5mC calls, the 3 x 256
// probability histograms and the per-locus methylated / unmethylated counters, all resident in HBM.
//
// What the reference does on the CPU (src/app/hifimeth/pileup.cpp:208-353, 514-560): per read it expands the CIGAR
// into two gapped strings (bam_info.cpp:262-371), walks them three times with strncmp / a 3-mer hash to find CpG,
// CHG and CHH columns where read and reference agree, looks the read offset up in a per-read table of ML bytes,
// spills {sid, soff, prob, motif} to a temporary file, and after the thresholds are known replays the file one
// chromosome at a time into two int arrays.
//
// Here: the gapped strings are never built.  A motif can only sit on consecutive aligned pairs, so the host turns
// each CIGAR into "match runs" (maximal stretches of M/=/X columns: read offset, reference offset, length) and one
// GPU thread per aligned column tests the 2- and 3-column motifs straight from the 4-bit SEQ and the reference
// bytes.  This is byte / integer work bound by HBM traffic; no LDS tiling or MFMA applies.  Kernels:
//   entries_kernel<PMod>   thread per MM/ML entry : ML byte -> per-base plane (last entry wins, as the reference's
//                   sequential overwrite), context histograms through LDS
//   entries_kernel<PCall>  thread per call : the same for records submitted with their hm_call_t calls instead of parsed
//                   MM/ML lists (hm_pileup_submit_read_calls, the fused `pileup -K` path)
//   identity_kernel thread per column      : matches per read (only when -f > 0)
//   project_kernel  thread per column      : motif tests, plane lookup, wave-aggregated append of 12-byte records
//   count_kernel<CountPlanes>    thread per record : atomic add into pcov / ncov, atomic max into the motif key
//   count_kernel<CountHpPlanes>  the same + one more atomic add into the record's haplotype planes (partitions = 2 only)
//   load_rows_kernel<Sink>  thread per row : (`diff`, `groupdiff`, `samplecorr`) the rows of a *.cov.bed file checked and the bad ones
//                   (outside the reference, negative, too big, a locus twice) counted by kind; the sink says where a good row goes:
//                   LoadPlanes one partition's planes and the combined ones, GroupLoadPlanes also a group's moment and sample-count
//                   planes, SampleLoadPlanes one sample's uint16 level plane
//   The column kernels (identity, project, pattern, depth) and MemberSel see the staged batch as one BatchView; the tiled ones
//   walk it with walk_columns, test a CpG member with cpg_columns / cpg_call and append with stage_record / flush_stage.
//   pattern_kernel  thread per column      : (`pileup -E`) a CpG member that heads a window of k reference CpGs looks the other
//                   k - 1 up in the read's following runs and appends one 8-byte window record; pattern_count_kernel adds
//                   the records into 16 bins per reference CpG; RefCpgSel lists the reference CpGs, PatSel the rows
//   depth_kernel    thread per column      : (`pileup -M`) a column on the C of a reference CG whose read is no member there adds
//                   NOCALL or DIFF to the CpG's depth counters; depth_gap_kernel, thread per D operation, adds DELETE;
//                   depth_count_kernel, thread per resident record, adds MOD or CANON; BmSel the bedMethyl rows
//   linkage_pair_kernel  thread per member : (`pileup -L`) MemberSel lists a batch's CpG members in column order; a member pairs with
//                   the later members of its record within max_dist and adds each pair to three 256-bin histograms per distance;
//                   linkage_reduce_kernel, workgroup per distance, turns them into UU / UM / MU / MM once the threshold is known;
//                   LinkSel the rows
//   project_kernel<true>  (`pileup -P`) the projection that also adds every record it emits to the read-position table, by its
//                   offset in the read: rows within D of a read end by global atomics, the interior rows through LDS;
//                   readpos_reduce_kernel, workgroup per row, sums a row under the thresholds; ReadPosSel the rows
//   select_count / loci_scan / select_write   the rows of a SELECTION over a range in ascending order (count per block, scan,
//                   write); every output below is a selection struct (its planes, pred, take) plus per-row kernels
//   LociSel         covered loci
//   AsmSel          loci where both haplotypes reach a minimum coverage; asm_test_kernel then runs one thread per compact row:
//                   methylation difference + two-sided Fisher exact test
//   asm_hist / BinsSel / asm_q_write   Benjamini-Hochberg q-values of that test (`pileup -H -A -Q`): tested loci counted per
//                   (context, p1, n1, p2, n2), the non-empty bins compacted and given their p by asm_test_kernel, q looked up per row
//   AsmSel<ASM_CTX> / RegionSel   allele-specific regions (`pileup -H -A -G`): the tested rows of one context compacted and tested,
//                   then a selection over ROW indices: a thread that owns a chain head walks to the chain's tail
//   GroupCtxSel / RegionSel<GroupChain>   regions between replicate groups (`groupdmr`): the same walk over the group rows of a context
//   sites_* / SitesSel   binomial test per locus (`pileup -B / -e`): control sums, histogram of (motif, pcov, pcov + ncov) through
//                   LDS, the loci beyond the histogram listed (SitesBigSel), rows written by table lookup
//   DomRowSel / rowscan_* / DomHeadSel   methylation domains (`pileup -D`): the rows of one context compacted, a two-state Viterbi
//                   path as two scans over a monoid (reduce per workgroup, one workgroup scans the aggregates, re-scan), segment
//                   heads compacted, one thread per segment (domain_build_part_kernel); for the fit of the levels (`-D -Y`) the
//                   rows' counters summed by state behind the two scans instead (domain_sums_kernel)
//   block_split / *_block_sums / RegionScan, SampleIvScan / *_query / metaplot   sums over given intervals: the sums per block of
//                   HM_REGION_BLOCK loci (twelve for `pileup -R`, `-J`; a pair per sample of the level planes for `regiondiff`), their
//                   scan by the row-scan skeleton above, then a wavefront per interval (or per bin and stride of intervals) reads the
//                   index and sums the loci of its two partial blocks (region_add over its lanes; sample_wave_add through LDS)
//   smooth_prefix_kernel / SmoothSel   kernel-smoothed levels (`smooth`): per position the running sums and first moments of the
//                   counting loci of one context, restarted every HM_SMOOTH_SPAN positions; a row is a few differences of them
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/hifimeth_hip.h"
#include "hm_host.h"

using namespace hm;

namespace {

thread_local std::string g_pileup_create_error;

// ---- device-side records -----------------------------------------------------------------------------------
struct PRead {
    int64_t seq4_off;   // byte offset of the 4-bit SEQ in the batch slab
    int64_t plane_off;  // offset of base 0 in the per-base mod plane
    int32_t l_qseq;
    uint32_t order;
    int32_t as_size;    // alignment columns incl. gaps (denominator of the identity)
    uint8_t rev, primary, pass, hp;  // hp: haplotype partition 0 (none), 1, 2
};

struct PRun {
    int64_t g0;         // reference offset (concatenated) of the run's first column
    int32_t read;
    int32_t q0;         // offset in SEQ as stored
    int32_t len;
    int32_t pad;
};

// The two entry types unpack themselves into mod_entry's arguments: ml() the ML byte, rank() what orders the entries of one
// position, is_m() a 5mC entry, on_cg() unmodified base C or G.
struct PMod {
    int32_t read;
    int32_t qoff;
    uint32_t bits;      // idx_in_read << 10 | is_m << 9 | unmod_is_CG << 8 | prob
    __device__ uint32_t ml() const { return bits & 255u; }
    __device__ uint32_t rank() const { return (bits >> 10) + 1u; }
    __device__ bool is_m() const { return bits & 0x200u; }
    __device__ bool on_cg() const { return bits & 0x100u; }
};

// Every call is a 5mC entry on a C (FWD) or G (REV), and a read has at most one per position, so the rank is a constant.
// hm_call_t::ctx is not used: at read ends and next to N it is not what the bases of the written-and-parsed MM list give.
struct PCall {          // 12 bytes: hm_call_t without p, read_id replaced by the index of the staged read
    int32_t read;
    int32_t qoff;
    uint8_t strand, ctx, prob, reserved;
    __device__ uint32_t ml() const { return prob; }
    __device__ uint32_t rank() const { return 1u; }
    __device__ bool is_m() const { return true; }
    __device__ bool on_cg() const { return true; }
};
static_assert(sizeof(PCall) == 12 && sizeof(hm_call_t) == 16, "staged calls are the first 12 bytes of hm_call_t");

struct PRec {           // 12 bytes
    uint32_t glo;       // gpos & 0xffffffff
    uint32_t hi;        // gpos >> 32 (8 bits) | prob << 8 | motif << 16 | hp << 18
    uint32_t order;
    __host__ __device__ int64_t gpos() const { return (int64_t)glo | ((int64_t)(hi & 255u) << 32); }
    __host__ __device__ uint32_t prob() const { return (hi >> 8) & 255u; }
    __host__ __device__ uint32_t motif() const { return (hi >> 16) & 3u; }
    __host__ __device__ uint32_t hp() const { return (hi >> 18) & 3u; }
    __host__ __device__ static PRec make(int64_t gpos, uint32_t prob, uint32_t motif, uint32_t hp, uint32_t order) {
        return PRec{(uint32_t)gpos, (uint32_t)((uint64_t)gpos >> 32) | (prob << 8) | (motif << 16) | (hp << 18), order};
    }
};

// The staged batch as every column kernel and MemberSel see it: match runs with the batch column of each run's first column
// (col0[n_runs] = n_cols), the records, their 4-bit SEQ, the reference, the per-base 5mC plane, and what -f needs.
struct BatchView {
    const PRun* runs;
    const int64_t* col0;
    int n_runs;
    int64_t n_cols;
    const PRead* reads;
    const uint8_t* slab;
    const char* ref;
    const uint32_t* plane;
    const int32_t* matches;
    double min_pi;
};

constexpr int TPB = 256;

__device__ __forceinline__ char nib_char(uint32_t c) {  // s_decode_bam_query_base (bam_info.cpp:100-121)
    return c == 1 ? 'A' : c == 2 ? 'C' : c == 4 ? 'G' : c == 8 ? 'T' : 'N';
}
__device__ __forceinline__ char comp_char(char c) {     // completement_residue (bam_info.cpp:146-167)
    return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
}
__device__ __forceinline__ char stored_base(const uint8_t* __restrict__ slab, const PRead& r, int k) {
    const uint32_t b = slab[r.seq4_off + (k >> 1)];
    return nib_char((k & 1) ? (b & 15u) : (b >> 4));
}
// BamQuerySequence::fwd_rqs[k] (bam_info.cpp:169-222)
__device__ __forceinline__ char fwd_base(const uint8_t* __restrict__ slab, const PRead& r, int k) {
    return r.rev ? comp_char(stored_base(slab, r, r.l_qseq - 1 - k)) : stored_base(slab, r, k);
}
__device__ __forceinline__ bool isH(char c) { return c == 'A' || c == 'C' || c == 'T'; }
__device__ __forceinline__ bool isD(char c) { return c == 'A' || c == 'G' || c == 'T'; }

// ---- mods: plane scatter + histograms (pileup.cpp:237-284) ---------------------------------------------------
// One entry of a read (an MM/ML entry, or a call): a 5mC entry writes the per-base plane word project_kernel reads
// (bit 0x100 + ML byte; `rank` above them orders the entries of one position: the largest wins); an entry on C / G of a
// primary record counts in the workgroup's context histogram h[3][256], the context taken from the read's own bases.
// `pileup -I` (Trim): an entry in the first n5 or the last n3 bases of the read as sequenced does neither -- for every kernel
// behind this one the read has no entry there.  0:0 drops nothing.
struct Trim {
    int32_t n5, n3;
};
__device__ __forceinline__ void mod_entry(const PRead& r, int q, uint32_t prob, uint32_t rank, bool is_m, bool cg, Trim trim,
                                          const uint8_t* __restrict__ slab, uint32_t* __restrict__ plane, uint32_t* h) {
    if (q < trim.n5 || q > r.l_qseq - 1 - trim.n3) return;
    if (is_m)  // code 'm': read_mods[qoff] = prob, later entries overwrite earlier ones
        atomicMax(&plane[r.plane_off + q], (rank << 9) | 0x100u | prob);
    if (r.primary && cg) {
        const int L = r.l_qseq;
        const char c0 = fwd_base(slab, r, q);
        int ctx = -1;
        if (c0 == 'C') {
            const char c1 = q + 1 < L ? fwd_base(slab, r, q + 1) : 'N';
            const char c2 = q + 2 < L ? fwd_base(slab, r, q + 2) : 'N';
            if (q + 1 < L && c1 == 'G') ctx = 0;
            else if (q + 2 < L && isH(c1) && c2 == 'G') ctx = 1;
            else if (q + 2 < L && isH(c1) && isH(c2)) ctx = 2;
        } else if (q - 2 >= 0) {  // the G of [AGT][AGT]G
            if (c0 == 'G' && isD(fwd_base(slab, r, q - 1)) && isD(fwd_base(slab, r, q - 2))) ctx = 2;
        }
        if (ctx >= 0) atomicAdd(&h[ctx * 256 + prob], 1u);
    }
}

// A workgroup-private histogram of n bins in LDS: zeroed; and added to the global bins, one atomic per non-empty bin
__device__ __forceinline__ void hist_zero(uint32_t* h, int n) {
    for (int i = threadIdx.x; i < n; i += TPB) h[i] = 0u;
    __syncthreads();
}
__device__ __forceinline__ void hist_flush(const uint32_t* h, int n, unsigned long long* __restrict__ bins) {
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += TPB)
        if (h[i]) atomicAdd(&bins[i], (unsigned long long)h[i]);
}

template <class Entry>  // PMod or PCall
__global__ __launch_bounds__(TPB) void entries_kernel(const Entry* __restrict__ entries, int64_t n, const PRead* __restrict__ reads,
                                                       const uint8_t* __restrict__ slab, uint32_t* __restrict__ plane,
                                                       unsigned long long* __restrict__ bins, Trim trim) {
    __shared__ uint32_t h[3 * 256];
    hist_zero(h, 768);
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const Entry e = entries[i];
        mod_entry(reads[e.read], e.qoff, e.ml(), e.rank(), e.is_m(), e.on_cg(), trim, slab, plane, h);
    }
    hist_flush(h, 768, bins);
}

// run holding global column c: largest r in [lo, hi) with col0[r] <= c
__device__ __forceinline__ int find_run(const int64_t* __restrict__ col0, int n_runs, int64_t c, int lo = 0, int hi = -1) {
    if (hi < 0) hi = n_runs;  // col0[lo] <= c < col0[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (col0[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- identity: s_calc_ident_perc numerator (bam_info.cpp:11-23); gap columns never match ---------------------
__global__ __launch_bounds__(TPB) void identity_kernel(BatchView b, int32_t* __restrict__ matches) {
    const int64_t c = (int64_t)blockIdx.x * TPB + threadIdx.x;
    int rd = -1;
    bool eq = false;
    if (c < b.n_cols) {
        const int ri = find_run(b.col0, b.n_runs, c);
        const PRun run = b.runs[ri];
        const int o = (int)(c - b.col0[ri]);
        rd = run.read;
        eq = stored_base(b.slab, b.reads[rd], run.q0 + o) == b.ref[run.g0 + o];
    }
    const int first = __shfl(rd, 0);
    if (__all(rd == first)) {  // the common case: one read per wavefront -> one atomic
        const unsigned long long bal = __ballot(eq);
        if ((threadIdx.x & 63) == 0 && first >= 0 && bal) atomicAdd(&matches[first], __popcll(bal));
    } else if (eq) {
        atomicAdd(&matches[rd], 1);
    }
}

// ---- what the tiled column kernels share --------------------------------------------------------------------
// A workgroup walks PTILE consecutive columns, stages its records in LDS and appends them to the global list with
// ONE atomic (same-address atomics from every wavefront serialise in L2 and dominated an earlier version).
constexpr int PTILE = 1024;

// The walk: body(ri, run, o, in_range) per column of the workgroup's tile -- run index, run, offset in the run; beyond the
// batch's last column in_range is false and the rest unset.  Every lane of a wavefront enters the body on every trip, so a
// body may hold wavefront collectives (stage_record).  Opens with a barrier: what a kernel set in LDS before it is visible.
template <class Body>
__device__ __forceinline__ void walk_columns(const BatchView& b, Body body) {
    __shared__ int run_range[2];  // runs touched by this tile: the per-column search starts from here
    if (threadIdx.x < 2) {
        const int64_t c = min((int64_t)blockIdx.x * PTILE + (threadIdx.x ? PTILE - 1 : 0), b.n_cols - 1);
        run_range[threadIdx.x] = find_run(b.col0, b.n_runs, c) + (int)threadIdx.x;
    }
    __syncthreads();
    const int run_lo = run_range[0], run_hi = run_range[1];
    for (int it = 0; it < PTILE / TPB; ++it) {
        const int64_t c = (int64_t)blockIdx.x * PTILE + it * TPB + threadIdx.x;
        const bool in_range = c < b.n_cols;
        int ri = 0, o = 0;
        PRun run{};
        if (in_range) {
            ri = find_run(b.col0, b.n_runs, c, run_lo, run_hi);
            run = b.runs[ri];
            o = (int)(c - b.col0[ri]);
        }
        body(ri, run, o, in_range);
    }
}

// append one record per lane with `pred` to the workgroup's LDS stage: one LDS atomic per wavefront
template <class Rec>
__device__ __forceinline__ void stage_record(bool pred, const Rec& rec, Rec* __restrict__ stage, int* __restrict__ n_stage) {
    const unsigned long long b = __ballot(pred);
    if (!b) return;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)b) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(n_stage, __popcll(b));
    base = __shfl(base, leader);
    if (pred) stage[base + __popcll(b & ((1ull << lane) - 1ull))] = rec;
}

// the workgroup's *n_stage staged records appended to `out` behind one atomic on `counter`; they move as a stream of dwords
template <class Rec>
__device__ __forceinline__ void flush_stage(const Rec* stage, const int* n_stage, Rec* __restrict__ out,
                                            unsigned long long* __restrict__ counter) {
    static_assert(sizeof(Rec) % 4 == 0, "staged records move as dwords");
    __shared__ unsigned long long out_base;
    __syncthreads();
    const int n = *n_stage;
    if (threadIdx.x == 0 && n) out_base = atomicAdd(counter, (unsigned long long)n);
    __syncthreads();
    if (n) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(stage);
        uint32_t* dst = reinterpret_cast<uint32_t*>(out + out_base);
        for (int i = threadIdx.x; i < (int)(sizeof(Rec) / 4) * n; i += TPB) dst[i] = src[i];
    }
}

// -q and -f: the one place that compares a record's identity with min_pi
__device__ __forceinline__ bool read_takes_part(const PRead& rd, int read, const int32_t* __restrict__ matches, double min_pi) {
    return rd.pass && !(min_pi > 0.0 && 100.0 * matches[read] / rd.as_size < min_pi);
}

// The CpG member of include/hifimeth_hip.h, in two halves.  cpg_columns: stored bases and reference both show CG on two
// columns of one run -- from characters the caller holds, or loaded at offset `off` of `run` (off + 1 < run.len).
__device__ __forceinline__ bool cpg_columns(char q0, char q1, char s0, char s1) {
    return q0 == 'C' && q1 == 'G' && s0 == 'C' && s1 == 'G';
}
__device__ __forceinline__ bool cpg_columns(const BatchView& b, const PRead& rd, const PRun& run, int off) {
    const int qp = run.q0 + off;
    const int64_t g = run.g0 + off;
    return cpg_columns(stored_base(b.slab, rd, qp), stored_base(b.slab, rd, qp + 1), b.ref[g], b.ref[g + 1]);
}
// cpg_call: the ML byte of the 5mC entry of the CpG whose C is stored base qp, or -1: a reverse record carries it on the G
__device__ __forceinline__ int cpg_call(const BatchView& b, const PRead& rd, int qp) {
    const uint32_t v = b.plane[rd.plane_off + (rd.rev ? rd.l_qseq - 1 - (qp + 1) : qp)];
    return (v & 0x100u) ? (int)(v & 255u) : -1;
}
// both: the member's ML byte at offset `off` of `run`, or -1
__device__ __forceinline__ int cpg_member(const BatchView& b, const PRead& rd, const PRun& run, int off) {
    return cpg_columns(b, rd, run, off) ? cpg_call(b, rd, run.q0 + off) : -1;
}

// ---- methylation by position in the read (`pileup -P`; include/hifimeth_hip.h has the definition) ---------------------------
// hist[(motif * (2 D + 1) + bin) * 256 + ML byte], uint64: bin d5 < D the 5' rows, D + d3 the 3' rows, 2 D the interior row --
// the order in which a fetch returns them.  Threshold-free, as the linkage histograms are; integer atomics only.
constexpr int READPOS_MAX = 2048;
struct ReadPos {
    unsigned long long* hist;
    int D;
    __host__ __device__ int rows() const { return 2 * D + 1; }
};
// One projected record whose 5mC entry sits at plane index p of a read of L bases.  About 1 - 2 D / L of all records are
// interior: those go to the workgroup's h[3][256] in LDS; an end row is one of 2 D x 256 addresses per context, a global atomic.
__device__ __forceinline__ void readpos_add(const ReadPos& rp, uint32_t* h, const PRec& r, int p, int L) {
    const int d5 = p, d3 = L - 1 - p;
    if (min(d5, d3) >= rp.D) atomicAdd(&h[r.motif() * 256u + r.prob()], 1u);
    else atomicAdd(&rp.hist[((size_t)r.motif() * rp.rows() + (d5 <= d3 ? d5 : rp.D + d3)) * 256 + r.prob()], 1ull);
}

// ---- projection (pileup.cpp:286-347, 5mc_motif_finder.cpp:104-144) -----------------------------------------
// PROFILE (`pileup -P`): every record also counts in the read-position table, at the plane index its 5mC entry was found at.
template <bool PROFILE>
__global__ __launch_bounds__(TPB) void project_kernel(BatchView b, PRec* __restrict__ out, unsigned long long* __restrict__ counter,
                                                       ReadPos rp) {
    __shared__ PRec stage[2 * PTILE];  // a column yields at most two records (CpG + the reverse-strand CGG of CHG)
    __shared__ int n_stage;
    __shared__ uint32_t interior[PROFILE ? 3 * 256 : 1];
    if (threadIdx.x == 0) n_stage = 0;
    if constexpr (PROFILE)
        for (int i = threadIdx.x; i < 3 * 256; i += TPB) interior[i] = 0u;
    walk_columns(b, [&](int, const PRun& run, int o, bool in_range) {
        bool e0 = false, e1 = false;
        PRec r0{}, r1{};
        [[maybe_unused]] int p0 = 0, p1 = 0, len = 0;  // PROFILE: the plane indices of r0 and r1, the read's length
        const int rem = run.len - o;
        if (in_range && rem >= 2) {
            const PRead rd = b.reads[run.read];
            if (read_takes_part(rd, run.read, b.matches, b.min_pi)) {
                const int qp = run.q0 + o, L = rd.l_qseq;
                const int64_t g = run.g0 + o;
                const char q0 = stored_base(b.slab, rd, qp), q1 = stored_base(b.slab, rd, qp + 1);
                const char s0 = b.ref[g], s1 = b.ref[g + 1];
                char q2 = '-', s2 = '*';
                if (rem >= 3) { q2 = stored_base(b.slab, rd, qp + 2); s2 = b.ref[g + 2]; }
                const bool eq3 = rem >= 3 && q0 == s0 && q1 == s1 && q2 == s2;
                auto look = [&](int qoff, int64_t soff, uint32_t motif) {
                    const uint32_t v = b.plane[rd.plane_off + qoff];
                    if (v & 0x100u) {
                        e1 = true;
                        r1 = PRec::make(soff, v & 255u, motif, rd.hp, rd.order);
                        if constexpr (PROFILE) p1 = qoff;
                    }
                };
                if constexpr (PROFILE) len = L;
                if (cpg_columns(q0, q1, s0, s1)) {  // CpG, recorded at the reference C
                    const int p = cpg_call(b, rd, qp);
                    if (p >= 0) {
                        e0 = true;
                        r0 = PRec::make(g, (uint32_t)p, 0, rd.hp, rd.order);
                        if constexpr (PROFILE) p0 = rd.rev ? L - 1 - (qp + 1) : qp;  // cpg_call's index
                    }
                }
                if (eq3 && q0 == 'C' && q2 == 'G') {  // CHG: forward reads CCG/CAG/CTG, reverse reads CGG/CAG/CTG
                    const bool mid = rd.rev ? (q1 == 'G' || q1 == 'A' || q1 == 'T') : (q1 == 'C' || q1 == 'A' || q1 == 'T');
                    if (mid) look(rd.rev ? L - 1 - (qp + 2) : qp, g, 1);
                } else if (eq3 && q0 == 'C' && isH(q1) && isH(q2)) {  // CHH on the reference's forward strand
                    look(rd.rev ? L - 1 - qp : qp, g, 2);
                } else if (eq3 && isD(q0) && isD(q1) && q2 == 'G') {  // CHH on the reverse strand, recorded at the G
                    look(rd.rev ? L - 1 - (qp + 2) : qp + 2, g + 2, 2);
                }
            }
        }
        stage_record(e0, r0, stage, &n_stage);
        stage_record(e1, r1, stage, &n_stage);
        if constexpr (PROFILE) {
            if (e0) readpos_add(rp, interior, r0, p0, len);
            if (e1) readpos_add(rp, interior, r1, p1, len);
        }
    });
    flush_stage(stage, &n_stage, out, counter);
    if constexpr (PROFILE)  // behind flush_stage's barriers: one atomic per non-empty bin, as hist_flush
        for (int i = threadIdx.x; i < 3 * 256; i += TPB)
            if (interior[i]) atomicAdd(&rp.hist[((size_t)(i >> 8) * rp.rows() + 2 * rp.D) * 256 + (i & 255)], (unsigned long long)interior[i]);
}

// ---- counting (pileup.cpp:529-557) -------------------------------------------------------------------------
struct CountPlanes {
    int32_t *pcov, *ncov;
    uint32_t* key;
};
struct CountHpPlanes : CountPlanes {  // + the haplotype partitions' pcov / ncov
    int32_t *pcov1, *ncov1, *pcov2, *ncov2;
};

// With CountHpPlanes a record tagged hp 1 / 2 also adds to that partition's pcov / ncov with the same threshold.  No key
// atomics there: a partition's loci take their motif from the combined key plane.
template <class Planes>
__global__ __launch_bounds__(TPB) void count_kernel(const PRec* __restrict__ recs, int64_t n, uint32_t thr_packed, Planes pl) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const PRec r = recs[i];
        const int64_t g = r.gpos();
        const uint32_t motif = r.motif();
        const bool pos = r.prob() >= ((thr_packed >> (8 * motif)) & 255u);
        atomicAdd(pos ? &pl.pcov[g] : &pl.ncov[g], 1);
        atomicMax(&pl.key[g], (r.order << 2) | motif);
        if constexpr (std::is_same_v<Planes, CountHpPlanes>) {
            if (r.hp() == 1u) atomicAdd(pos ? &pl.pcov1[g] : &pl.ncov1[g], 1);
            else if (r.hp() == 2u) atomicAdd(pos ? &pl.pcov2[g] : &pl.ncov2[g], 1);
        }
    }
}

// ---- counts from elsewhere (`diff`, `groupdiff`, `samplecorr`): rows of a *.cov.bed file into the engine's planes ----------------
// load_rows_kernel<Sink>: a thread per row, grid-stride.  A row is checked before anything is written -- gpos inside [0, total),
// both counts >= 0, for a LIMITED sink pcov + ncov < 2^20, motif <= 3, in this order, the first failure names the row -- and a bad
// row adds nothing.  A row without a count is skipped.  Every other row goes to the sink's take(), which says where a row of its
// loader goes and answers ROW_ADDED, ROW_DUP, both or nothing.  c[LOAD_ADDED] counts the rows that added, c[LOAD_BAD_*] the bad ones
// by kind: summed per wavefront, one global atomic per wavefront and non-zero counter.  Every sink writes by integer atomics only:
// the planes do not depend on row order or launch geometry.
enum LoadCounter { LOAD_ADDED = 0, LOAD_BAD_GPOS, LOAD_BAD_COUNT, LOAD_BAD_BIG, LOAD_BAD_MOTIF, LOAD_BAD_DUP, LOAD_COUNTERS };
constexpr uint32_t ROW_ADDED = 1u << LOAD_ADDED, ROW_DUP = 1u << LOAD_BAD_DUP;
constexpr int64_t LOAD_SLAB_ROWS = int64_t(1) << 20, LOAD_SLAB_MAX = int64_t(1) << 24;  // 24 MB of rows on the device by default
constexpr int32_t GROUP_COUNT_LIMIT = 1 << 20;  // a sample's pcov + ncov at a locus stays below this
constexpr int GROUP_MAX_SAMPLES = 255;          // per group: the sample counts are bytes
constexpr int SAMPLE_MAX = HM_SAMPLE_MAX, SAMPLE_TILE = HM_SAMPLE_TILE;
constexpr uint32_t SAMPLE_BELOW = 0xFFFFu;

// THE DUPLICATE RULE, the same for the three sinks.  A row that passes the checks and carries a count is a duplicate exactly when
// an earlier or concurrent row of the same locus was given to the same target: the partition for `diff`, the open sample for the
// other two; the window runs from when the target's planes were last cleared or opened, across slabs and across calls.  Of k such
// rows on one locus exactly k - 1 count in c[LOAD_BAD_DUP], whatever the launch geometry, the row order or the slab size, because
// each sink decides by the old value of ONE atomic operation on ONE word per locus and target: an atomicOr on a seen bitmap
// (`diff`: the partition's, `groupdiff`: the open sample's) or a compare-and-swap on the level word (`samplecorr`).  Exactly one
// of the k rows finds the locus unseen.  What a duplicate adds is the sink's own business: in `diff` it still adds, in the other
// two it adds nothing and which row wins is open.

// `diff` (hm_pileup_load_loci): the combined planes + those of the partition the rows go to.  A row takes its locus' bit in the
// seen bitmap of its target first -- the old bit says whether the locus came before: a duplicate, which still adds -- then adds
// to its partition's planes and to the combined ones and raises the key to its motif (`order` bits stay 0).  Counts that a
// caller's planes held before the first load are not rows: they make nothing a duplicate.
struct LoadPlanes : CountPlanes {
    static constexpr bool LIMITED = false;
    int32_t *part_pcov, *part_ncov;
    uint32_t* seen;  // the target's bitmap, 32 loci per word: the partition's for `diff`, the open sample's for a group

    __device__ bool seen_before(int64_t g) const {
        const uint32_t bit = 1u << (g & 31);
        return atomicOr(&seen[g >> 5], bit) & bit;
    }
    __device__ uint32_t take(const hm_locus_t& r) const {
        const int64_t g = r.gpos;
        const bool dup = seen_before(g);
        if (r.pcov) {
            atomicAdd(&part_pcov[g], r.pcov);
            atomicAdd(&pcov[g], r.pcov);
        }
        if (r.ncov) {
            atomicAdd(&part_ncov[g], r.ncov);
            atomicAdd(&ncov[g], r.ncov);
        }
        atomicMax(&key[g], r.motif);
        return dup ? ROW_ADDED | ROW_DUP : ROW_ADDED;
    }
};

// `groupdiff` (hm_pileup_load_sample_loci): the rows of ONE sample of a group.  LIMITED: a sample's count stays below 2^20, so
// q = floor(k^2 2^20 / n) needs no more than 60 bits.  `seen` is the open SAMPLE's bitmap -- cleared when the sample is opened --
// never the partition's: a group's samples share a partition on purpose.  It takes the locus' bit first: the old bit says
// whether this sample gave the locus before, a duplicate, which adds nothing.  A row below the
// sample minimum coverage keeps its bit and adds nothing.  Every other row adds its counts as LoadPlanes does, q to the group's
// moment plane and 1 to the locus' byte of the group's sample-count plane: an add to the aligned word that holds the byte, which
// never carries since a group has at most 255 samples.
struct GroupLoadPlanes : LoadPlanes {
    static constexpr bool LIMITED = true;
    unsigned long long* moment;  // Q_g
    uint32_t* samples;           // m_g, four loci per word
    int32_t min_cov;

    __device__ uint32_t take(const hm_locus_t& r) const {
        const int64_t g = r.gpos;
        if (seen_before(g)) return ROW_DUP;
        const int32_t cov = r.pcov + r.ncov;
        if (cov < min_cov) return 0u;
        if (r.pcov) {
            atomicAdd(&part_pcov[g], r.pcov);
            atomicAdd(&pcov[g], r.pcov);
            atomicAdd(&moment[g], ((unsigned long long)r.pcov * (unsigned long long)r.pcov << 20) / (unsigned long long)cov);
        }
        if (r.ncov) {
            atomicAdd(&part_ncov[g], r.ncov);
            atomicAdd(&ncov[g], r.ncov);
        }
        atomicMax(&key[g], r.motif);
        atomicAdd(&samples[g >> 2], 1u << (8 * (g & 3)));
        return ROW_ADDED;
    }
};

// `samplecorr` (hm_sample_load): the rows of ONE sample into its uint16 level plane, LIMITED as a group's.  The stored value of a
// locus is 0 (nothing seen), u + 1 with the level u = floor(k 2^15 / n) in [0, 32768] (the sample counts there), or SAMPLE_BELOW
// (seen, below the minimum coverage).  There are no 16-bit atomics: the value goes in by a compare-and-swap on the aligned 32-bit
// word that holds the locus and its neighbour, retried while only the neighbour's half changed.  A half that is not 0 -- before the
// first try or after a lost one -- is a duplicate, which adds nothing: of two rows of one locus exactly one wins, in one slab or in
// two.  The winner raises the key and, if the sample counts, adds its counts to the combined planes.  Which of two duplicate rows
// wins depends on the launch, but a duplicate voids the engine.
struct SampleLoadPlanes : CountPlanes {
    static constexpr bool LIMITED = true;
    uint32_t* level;  // the open sample's plane, two loci per word
    int32_t min_cov;

    __device__ uint32_t take(const hm_locus_t& r) const {
        const int64_t g = r.gpos;
        const int32_t cov = r.pcov + r.ncov;
        const bool counts = cov >= min_cov;
        const uint32_t value = counts ? (uint32_t)(((unsigned long long)r.pcov << 15) / (unsigned long long)cov) + 1u : SAMPLE_BELOW;
        const int shift = 16 * (int)(g & 1);
        uint32_t* word = &level[g >> 1];
        uint32_t old = *word;
        bool wrote = false;
        while (((old >> shift) & 0xFFFFu) == 0u) {
            const uint32_t prev = atomicCAS(word, old, old | (value << shift));
            if (prev == old) { wrote = true; break; }
            old = prev;
        }
        if (!wrote) return ROW_DUP;
        atomicMax(&key[g], r.motif);
        if (counts) {
            if (r.pcov) atomicAdd(&pcov[g], r.pcov);
            if (r.ncov) atomicAdd(&ncov[g], r.ncov);
        }
        return ROW_ADDED;
    }
};

template <class Sink>
__global__ __launch_bounds__(TPB) void load_rows_kernel(const hm_locus_t* __restrict__ rows, int64_t n, int64_t total, Sink sink,
                                                         unsigned long long* __restrict__ c) {
    uint32_t mine[LOAD_COUNTERS] = {0u, 0u, 0u, 0u, 0u, 0u};
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const hm_locus_t r = rows[i];
        if (r.gpos < 0 || r.gpos >= total) { ++mine[LOAD_BAD_GPOS]; continue; }
        if (r.pcov < 0 || r.ncov < 0) { ++mine[LOAD_BAD_COUNT]; continue; }
        if constexpr (Sink::LIMITED)
            if ((int64_t)r.pcov + r.ncov >= GROUP_COUNT_LIMIT) { ++mine[LOAD_BAD_BIG]; continue; }
        if (r.motif > 3u) { ++mine[LOAD_BAD_MOTIF]; continue; }
        if (r.pcov == 0 && r.ncov == 0) continue;
        const uint32_t did = sink.take(r);
        if (did & ROW_ADDED) ++mine[LOAD_ADDED];
        if (did & ROW_DUP) ++mine[LOAD_BAD_DUP];
    }
    for (int k = 0; k < LOAD_COUNTERS; ++k) {
        uint32_t v = mine[k];
        for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&c[k], (unsigned long long)v);
    }
}

// ---- the pair sums of M samples over [lo, hi) (hm_sample_fetch_sums; include/hifimeth_hip.h has the definition) ------------
// Workgroup (x, y, z) walks the tiles x, x + gridDim.x, ... of SAMPLE_TILE positions (tiles start at multiples of SAMPLE_TILE, the
// range cuts the first and the last) for context z; thread t of it owns pair y * TPB + t of the M (M + 1) / 2 pairs i <= j, in
// the order of the output, and keeps its six sums in registers across all its tiles.  Per tile, thread t reads position t: the
// key and the M stored values, plane after plane, so a wavefront reads 128 contiguous bytes of each plane.  A position that can add
// -- of context z, and with a value in any sample, or in `complete` mode a counting value in all M -- puts its values into LDS,
// one row per position, and its row number on a list (the order of the list is open: the sums are integers).  Rows are `pitch`
// 32-bit words apart, pitch odd, so the 64 rows a wavefront writes fall into 64 different banks; in the walk all threads read the
// same row, and the words of the samples i and j of neighbouring pairs are neighbours.  Each thread then walks the list.  u <= 2^15,
// so a product fits 32 bits and each sum advances by one 32 x 32 + 64-bit multiply-add.  One 64-bit atomicAdd per sum at the end, into
// table[(z * pairs + pair) * 6 + {n, si, sj, sii, sjj, sij}]: integer adds only, so the table depends on neither the grid nor the order.
__global__ __launch_bounds__(TPB) void sample_sums_kernel(const uint16_t* __restrict__ planes, int64_t stride, int M, const uint32_t* __restrict__ key,
                                                           int64_t lo, int64_t hi, int complete, unsigned long long* __restrict__ table) {
    static_assert(SAMPLE_TILE == TPB, "thread t reads position t of a tile");
    extern __shared__ uint32_t sample_lds[];
    const int pitch = ((M + 1) / 2) | 1;                     // words per row
    uint16_t* const vals = reinterpret_cast<uint16_t*>(sample_lds);  // [SAMPLE_TILE][2 * pitch]
    int* const list = reinterpret_cast<int*>(sample_lds + SAMPLE_TILE * pitch);  // [SAMPLE_TILE], then the count
    int* const count = list + SAMPLE_TILE;
    const uint32_t ctx = blockIdx.z;
    const int pairs = M * (M + 1) / 2;
    int pair = (int)blockIdx.y * TPB + (int)threadIdx.x, pi = 0, pj = 0;
    const bool owner = pair < pairs;
    if (owner) {
        int left = pair;
        while (left >= M - pi) { left -= M - pi; ++pi; }
        pj = pi + left;
    }
    unsigned long long n = 0, si = 0, sj = 0, sii = 0, sjj = 0, sij = 0;
    const int64_t first = lo / SAMPLE_TILE, last = (hi + SAMPLE_TILE - 1) / SAMPLE_TILE;
    for (int64_t tile = first + blockIdx.x; tile < last; tile += gridDim.x) {
        if (threadIdx.x == 0) *count = 0;
        __syncthreads();
        const int64_t g = tile * SAMPLE_TILE + threadIdx.x;
        if (g >= lo && g < hi && min(key[g] & 3u, 2u) == ctx) {
            uint16_t* const row = vals + (size_t)threadIdx.x * 2 * pitch;
            bool any = false, all = true;
            for (int s = 0; s < M; ++s) {
                const uint16_t v = planes[(int64_t)s * stride + g];
                row[s] = v;
                any |= v != 0;
                all &= v != 0 && v != SAMPLE_BELOW;
            }
            if (complete ? all : any) list[atomicAdd(count, 1)] = (int)threadIdx.x;
        }
        __syncthreads();
        const int m = *count;
        if (owner) {
            for (int k = 0; k < m; ++k) {
                const uint16_t* const row = vals + (size_t)list[k] * 2 * pitch;
                const uint32_t vi = row[pi], vj = row[pj];
                if (vi == 0u || vi == SAMPLE_BELOW || vj == 0u || vj == SAMPLE_BELOW) continue;
                const uint32_t ui = vi - 1u, uj = vj - 1u;
                n += 1;
                si += ui;
                sj += uj;
                sii += (unsigned long long)(ui * ui);
                sjj += (unsigned long long)(uj * uj);
                sij += (unsigned long long)(ui * uj);
            }
        }
        __syncthreads();
    }
    if (!owner || n == 0) return;
    unsigned long long* const t = table + ((size_t)ctx * pairs + pair) * 6;
    atomicAdd(&t[0], n);
    atomicAdd(&t[1], si);
    atomicAdd(&t[2], sj);
    atomicAdd(&t[3], sii);
    atomicAdd(&t[4], sjj);
    atomicAdd(&t[5], sij);
}

// ---- the sums of M samples over given intervals (hm_sample_fetch_intervals; include/hifimeth_hip.h has the definition) ----------
// The interval skeleton (block_split here, the host side with `pileup -R / -J`) over M planes: per block and sample the pair (n, su)
// of the call's context and mode.  The index is SAMPLE-major, idx[s * nblk + b], and scanned as ONE sequence of M * nblk pairs: a
// query only ever subtracts two entries of one sample, so the running sum may run on from one sample into the next, and the
// scan's element stays one pair (a row of 2 M = 128 values per block, as RegionScan keeps its twelve, would not fit the registers).
// The M-sample reduction (sample_wave_add; DESIGN.md section 10 has the reasoning) goes through LDS, in two phases per 64
// positions.  Phase 1, lane = position: the key once and the M values once, each into row t of the wavefront's tile (zeros for
// another context); the ballot of "can add" is one mask in every lane.  Phase 2, lane = (sample s, part q): with P the power of
// two >= M and G = 64 / P, lane s * G + q reads the words q, q + G, ... of row s, two positions each.  Rows are 32 + G words
// apart: no bank conflict.  The phases are ordered by wavefront-scope fences: the tile is the wavefront's own.
struct SampleIvPlanes {
    const uint16_t* planes;
    int64_t stride;
    const uint32_t* key;
    int M, G;  // samples opened; parts per sample = 64 / (the power of two >= max(M, 2))
    uint32_t ctx;
    int complete;
    __host__ __device__ int pitch() const { return 32 + G; }  // words per tile row
};
using SamplePair = hm_sample_interval_t;

// [a, b), lo <= a <= b, cut at the blocks of HM_REGION_BLOCK positions from lo (`pileup -R` and `regiondiff` both): the loci of
// [a, head_end) and of [tail_begin, b) are summed one by one, the whole blocks between them, if row_last > row_first, are
// prefix(row_last) - prefix(row_first) of the scanned index.  Within one block the head is [a, b) and the tail empty; a's
// remainder runs to its block's end, so that nothing is ever subtracted from a partial sum.
struct BlockSplit { int64_t head_end, tail_begin, row_first, row_last; };
__device__ __forceinline__ BlockSplit block_split(int64_t lo, int64_t a, int64_t b) {
    const int64_t ba = (a - lo) / HM_REGION_BLOCK, bb = (b - lo) / HM_REGION_BLOCK;
    if (ba == bb) return BlockSplit{b, b, ba, ba};
    return BlockSplit{lo + (ba + 1) * HM_REGION_BLOCK, lo + bb * HM_REGION_BLOCK, ba, bb - 1};
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wavefront adds the loci of [a, b) -- the same in all its lanes, inside the planes -- to the (n, su) of lane (s, q); `tile`
// is the wavefront's M rows of pitch() words
__device__ __forceinline__ void sample_wave_add(const SampleIvPlanes& v, uint32_t* tile, int64_t a, int64_t b, unsigned long long& n,
                                                unsigned long long& su) {
    const int lane = threadIdx.x & 63, q = lane & (v.G - 1), s = lane / v.G, pitch = v.pitch();
    uint16_t* const half = reinterpret_cast<uint16_t*>(tile);
    for (int64_t g0 = a; g0 < b; g0 += 64) {
        const int64_t g = g0 + lane;
        const bool mine = g < b && min(v.key[g] & 3u, 2u) == v.ctx;
        if (__ballot(mine) == 0ull) continue;
        bool all = mine;
        for (int t = 0; t < v.M; ++t) {
            const uint32_t x = mine ? v.planes[(int64_t)t * v.stride + g] : 0u;
            half[t * 2 * pitch + lane] = (uint16_t)x;
            all = all && x != 0u && x != SAMPLE_BELOW;
        }
        const unsigned long long ok = __ballot(v.complete ? all : mine);
        wave_lds_sync();
        if (ok != 0ull && s < v.M) {
            for (int w = q; w < 32; w += v.G) {
                const uint32_t word = tile[s * pitch + w], bits = (uint32_t)(ok >> (2 * w)) & 3u;
                const uint32_t x0 = word & 0xFFFFu, x1 = word >> 16;
                if ((bits & 1u) && x0 != 0u && x0 != SAMPLE_BELOW) {
                    n += 1;
                    su += x0 - 1u;
                }
                if ((bits & 2u) && x1 != 0u && x1 != SAMPLE_BELOW) {
                    n += 1;
                    su += x1 - 1u;
                }
            }
        }
        wave_lds_sync();
    }
}

// the G parts of every sample added up: lane (s, 0) holds the sample's sums
__device__ __forceinline__ void sample_parts_sum(int G, unsigned long long& n, unsigned long long& su) {
    for (int d = G >> 1; d; d >>= 1) {
        n += __shfl_xor(n, d);
        su += __shfl_xor(su, d);
    }
}

// idx[s * nblk + blockIdx.x] = (n, su) of sample s over block blockIdx.x of [lo, hi): each wavefront takes a quarter of the block
__global__ __launch_bounds__(TPB) void sample_block_sums_kernel(SampleIvPlanes v, int64_t lo, int64_t hi, int64_t nblk, SamplePair* __restrict__ idx) {
    extern __shared__ uint32_t sample_iv_lds[];
    __shared__ unsigned long long part[TPB / 64][2 * SAMPLE_MAX];
    constexpr int64_t QUARTER = HM_REGION_BLOCK / (TPB / 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, s = lane / v.G;
    const int64_t a = lo + (int64_t)blockIdx.x * HM_REGION_BLOCK + w * QUARTER, b = min(hi, a + QUARTER);
    unsigned long long n = 0, su = 0;
    if (a < b) sample_wave_add(v, sample_iv_lds + w * v.M * v.pitch(), a, b, n, su);
    sample_parts_sum(v.G, n, su);
    if ((lane & (v.G - 1)) == 0 && s < v.M) {
        part[w][2 * s] = n;
        part[w][2 * s + 1] = su;
    }
    __syncthreads();
    if ((int)threadIdx.x < v.M) {
        SamplePair t{0, 0};
        for (int k = 0; k < TPB / 64; ++k) {
            t.n += part[k][2 * threadIdx.x];
            t.su += part[k][2 * threadIdx.x + 1];
        }
        idx[(int64_t)threadIdx.x * nblk + blockIdx.x] = t;
    }
}

// the M * nblk pairs of the index -> their inclusive scan, in place
struct SampleIvScan {
    using T = SamplePair;
    SamplePair* idx;
    __host__ __device__ __forceinline__ static T identity() { return T{0, 0}; }
    __device__ __forceinline__ static T shfl_up(const T& v, int d) {
        return T{(uint64_t)__shfl_up((unsigned long long)v.n, d), (uint64_t)__shfl_up((unsigned long long)v.su, d)};
    }
    __device__ __forceinline__ static T op(const T& a, const T& b) { return T{a.n + b.n, a.su + b.su}; }
    __device__ __forceinline__ T load(int64_t j) const { return idx[j]; }
    __device__ __forceinline__ void store(int64_t j, const T& f) const { idx[j] = f; }
};

// out[i * M + s] = (n, su) of sample s over interval i clamped to [lo, hi): a wavefront per interval, over a grid stride
__global__ __launch_bounds__(TPB) void sample_query_kernel(SampleIvPlanes v, int64_t lo, int64_t hi, int64_t nblk, const SamplePair* __restrict__ idx,
                                                            const int64_t* __restrict__ start, const int64_t* __restrict__ end, int64_t n_iv,
                                                            SamplePair* __restrict__ out) {
    extern __shared__ uint32_t sample_iv_lds[];
    const int lane = threadIdx.x & 63, s = lane / v.G;
    const bool owner = (lane & (v.G - 1)) == 0 && s < v.M;
    uint32_t* const tile = sample_iv_lds + (threadIdx.x >> 6) * v.M * v.pitch();
    for (int64_t i = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); i < n_iv; i += (int64_t)gridDim.x * (TPB / 64)) {
        const int64_t a = min(max(start[i], lo), hi), b = min(max(end[i], lo), hi);
        unsigned long long n = 0, su = 0;
        const BlockSplit sp = block_split(lo, a, b);
        sample_wave_add(v, tile, a, sp.head_end, n, su);
        if (sp.tail_begin < b) sample_wave_add(v, tile, sp.tail_begin, b, n, su);
        if (owner && sp.row_last > sp.row_first) {  // the sample's own stretch of the index
            const SamplePair hiw = idx[(int64_t)s * nblk + sp.row_last], low = idx[(int64_t)s * nblk + sp.row_first];
            n += hiw.n - low.n;
            su += hiw.su - low.su;
        }
        sample_parts_sum(v.G, n, su);
        if (owner) out[i * v.M + s] = SamplePair{n, su};
    }
}

// ---- resident records joined with per-locus truth labels (`hifimeth eval`, src/app/hifimeth/eval.cpp:469-560) ----
// labels[g]: -1 no truth, 0 unmethylated, 1 methylated.  bins[(motif * 2 + label) * 256 + prob] counts the records whose
// locus carries a label; workgroup-private histogram in LDS, one global atomic per non-empty bin and workgroup.
__global__ __launch_bounds__(TPB) void label_kernel(const PRec* __restrict__ recs, int64_t n, const int8_t* __restrict__ labels,
                                                     unsigned long long* __restrict__ bins) {
    __shared__ uint32_t h[1536];
    hist_zero(h, 1536);
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const PRec r = recs[i];
        const int lab = labels[r.gpos()];
        if (lab >= 0) atomicAdd(&h[(r.motif() * 2u + (lab ? 1u : 0u)) * 256u + r.prob()], 1u);
    }
    hist_flush(h, 1536, bins);
}

// ---- covered loci of a range, ascending ---------------------------------------------------------------------
constexpr int LOCI_PER_BLOCK = 4096;  // 16 per thread

// One skeleton for every "rows of the selected indices of [lo, hi), ascending" output: select_count_kernel (count_block),
// loci_scan_kernel, select_write_kernel (compact_block), one workgroup per LOCI_PER_BLOCK indices in both, over a SELECTION
// passed by value: a struct of planes and parameters with Row, pred(i) = what the count step counts, and take(i, row) = the
// same selection with the row built.  stage_rows() on the host drives the three.

// the sum of v over the workgroup, in every thread; a barrier is due before the next call
__device__ __forceinline__ int block_sum(int v) {
    __shared__ int wsum[TPB / 64];
    for (int d = 32; d; d >>= 1) v += __shfl_down(v, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    return wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// The count step: block_counts[blockIdx.x] = the number of the workgroup's LOCI_PER_BLOCK loci i for which pred(i) holds.
template <class Pred>
__device__ __forceinline__ void count_block(int64_t lo, int64_t hi, int32_t* __restrict__ block_counts, Pred pred) {
    const int64_t base = lo + (int64_t)blockIdx.x * LOCI_PER_BLOCK;
    int cnt = 0;
    for (int k = 0; k < LOCI_PER_BLOCK / TPB; ++k) {
        const int64_t i = base + k * TPB + threadIdx.x;
        if (i < hi && pred(i)) ++cnt;
    }
    cnt = block_sum(cnt);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = cnt;
}

// The write step: the rows of the workgroup's LOCI_PER_BLOCK loci for which take(i, row) holds, in ascending order from
// out[offs[blockIdx.x]] on.  take must select what the count step's pred selected.
template <class Row, class Take>
__device__ __forceinline__ void compact_block(int64_t lo, int64_t hi, const int64_t* __restrict__ offs, Row* __restrict__ out, Take take) {
    __shared__ int wsum[TPB / 64];
    __shared__ int carry;
    if (threadIdx.x == 0) carry = 0;
    const int64_t base = lo + (int64_t)blockIdx.x * LOCI_PER_BLOCK;
    const int64_t o0 = offs[blockIdx.x];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = 0; k < LOCI_PER_BLOCK / TPB; ++k) {
        __syncthreads();
        const int64_t i = base + k * TPB + threadIdx.x;
        Row r;
        const bool sel = i < hi && take(i, r);
        const unsigned long long b = __ballot(sel);
        if (lane == 0) wsum[w] = __popcll(b);
        __syncthreads();
        int before = carry;
        for (int j = 0; j < w; ++j) before += wsum[j];
        if (sel) out[o0 + before + __popcll(b & ((1ull << lane) - 1ull))] = r;
        __syncthreads();
        if (threadIdx.x == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    }
}

template <class Sel>
__global__ __launch_bounds__(TPB) void select_count_kernel(Sel sel, int64_t lo, int64_t hi, int32_t* __restrict__ block_counts) {
    count_block(lo, hi, block_counts, [&](int64_t i) { return sel.pred(i); });
}

template <class Sel>
__global__ __launch_bounds__(TPB) void select_write_kernel(Sel sel, int64_t lo, int64_t hi, const int64_t* __restrict__ offs,
                                                            typename Sel::Row* __restrict__ out) {
    compact_block(lo, hi, offs, out, [&](int64_t i, typename Sel::Row& r) { return sel.take(i, r); });
}

// single-workgroup exclusive scan; total -> offs[n]
__global__ __launch_bounds__(1024) void loci_scan_kernel(const int32_t* __restrict__ counts, int n,
                                                          int64_t* __restrict__ offs) {
    __shared__ int64_t part[1024];
    const int per = (n + 1023) / 1024;
    const int lo = threadIdx.x * per, hi = min(n, lo + per);
    int64_t s = 0;
    for (int i = lo; i < hi; ++i) s += counts[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int64_t v = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int64_t run = part[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) {
        offs[i] = run;
        run += counts[i];
    }
    if (threadIdx.x == 1023) offs[n] = part[1023];
}

struct RangePlanes {  // of a call over a plane range: (pcov, ncov, key)
    const int32_t *pc, *nc;
    const uint32_t* ky;
};

// covered loci: a counter of either sign counts
struct LociSel {
    using Row = hm_locus_t;
    RangePlanes s;
    int64_t plane_base;
    __device__ bool pred(int64_t i) const { return (s.pc[i] | s.nc[i]) != 0; }
    __device__ bool take(int64_t i, Row& l) const {
        const int32_t p = s.pc[i], n = s.nc[i];
        if ((p | n) == 0) return false;
        l.gpos = plane_base + i;
        l.pcov = p;
        l.ncov = n;
        l.motif = s.ky[i] & 3u;
        l.reserved = 0;
        return true;
    }
};

// ---- read-level CpG patterns (`pileup -E`; include/hifimeth_hip.h has the definition) ----------------------------------------
constexpr int PAT_MAX_SPAN = 65536;

struct PWin {            // 8 bytes: a record that is a member at all k loci of the window headed by reference CpG `rank`
    uint32_t rank;
    uint8_t prob[4];     // by locus, leftmost first; beyond k: 0
};
static_assert(sizeof(PWin) == 8, "window records move as two dwords");

// end of the reference sequence that holds locus g: seq_off[s + 1] for the largest s with seq_off[s] <= g
__device__ __forceinline__ int64_t seq_end_of(const int64_t* __restrict__ seq_off, int n_seqs, int64_t g) {
    int lo = 0, hi = n_seqs;  // seq_off[lo] <= g < seq_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (seq_off[mid] <= g) lo = mid; else hi = mid;
    }
    return seq_off[hi];
}

// first index in a[0, n) with a[i] >= g
__device__ __forceinline__ int64_t lower_rank(const int64_t* __restrict__ a, int64_t n, int64_t g) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] < g) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the reference CpGs over [0, total): C and G of one sequence (the pair that straddles two sequences is none)
struct RefCpgSel {
    using Row = int64_t;
    const char* ref;
    const int64_t* seq_off;
    int n_seqs;
    int64_t total;
    __device__ bool pred(int64_t i) const {
        return i + 1 < total && ref[i] == 'C' && ref[i + 1] == 'G' && i + 1 < seq_end_of(seq_off, n_seqs, i);
    }
    __device__ bool take(int64_t i, Row& g) const {
        g = i;
        return pred(i);
    }
};

// what a window is made of, for the kernels and the selection below
struct PatRule {
    const int64_t* cpg_pos;  // the reference CpGs, ascending
    int64_t n_cpg;
    const int64_t* seq_off;
    int n_seqs;
    int k, max_span;
    // window r exists: k loci of one sequence within max_span
    __device__ bool valid(int64_t r) const {
        if (r + k - 1 >= n_cpg) return false;
        const int64_t first = cpg_pos[r], last = cpg_pos[r + k - 1];
        return last - first <= max_span && last < seq_end_of(seq_off, n_seqs, first);
    }
};

// One thread per aligned column, project_kernel's geometry.  A column that is a CpG member and whose locus heads a valid window
// walks the read's runs forward to the other k - 1 loci and applies the member test there; a read that is a member at all of them
// leaves one PWin.  The walk ends within max_span <= PAT_MAX_SPAN reference bases.
__global__ __launch_bounds__(TPB) void pattern_kernel(BatchView b, PatRule rule, PWin* __restrict__ out,
                                                       unsigned long long* __restrict__ counter) {
    __shared__ PWin stage[PTILE];  // a column heads at most one window
    __shared__ int n_stage;
    if (threadIdx.x == 0) n_stage = 0;
    walk_columns(b, [&](int ri, const PRun& run, int o, bool in_range) {
        bool e = false;
        PWin w{};
        if (in_range && run.len - o >= 2) {
            const PRead rd = b.reads[run.read];
            const int p0 = read_takes_part(rd, run.read, b.matches, b.min_pi) ? cpg_member(b, rd, run, o) : -1;
            if (p0 >= 0) {
                const int64_t g = run.g0 + o;
                const int64_t r = lower_rank(rule.cpg_pos, rule.n_cpg, g);
                if (r < rule.n_cpg && rule.cpg_pos[r] == g && rule.valid(r)) {
                    w.rank = (uint32_t)r;
                    w.prob[0] = (uint8_t)p0;
                    e = true;
                    int rj = ri;
                    PRun cur = run;
                    for (int i = 1; i < rule.k && e; ++i) {
                        const int64_t gi = rule.cpg_pos[r + i];
                        while (cur.g0 + cur.len <= gi) {  // the run that holds g_i, if one of this read's does
                            if (++rj >= b.n_runs) { e = false; break; }
                            cur = b.runs[rj];
                            if (cur.read != run.read) { e = false; break; }
                        }
                        if (!e || cur.g0 > gi || cur.g0 + cur.len - gi < 2) { e = false; break; }
                        const int pi = cpg_member(b, rd, cur, (int)(gi - cur.g0));
                        if (pi < 0) e = false;
                        else w.prob[i] = (uint8_t)pi;
                    }
                }
            }
        }
        stage_record(e, w, stage, &n_stage);
    });
    flush_stage(stage, &n_stage, out, counter);
}

// hist[rank * 16 + pattern] += 1 per window record, bit i of the pattern = prob[i] >= thr: integer atomics, any order
__global__ __launch_bounds__(TPB) void pattern_count_kernel(const PWin* __restrict__ wins, int64_t n, uint32_t thr, int k,
                                                             uint32_t* __restrict__ hist) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const PWin w = wins[i];
        uint32_t pat = 0;
        for (int j = 0; j < k; ++j) pat |= (w.prob[j] >= thr ? 1u : 0u) << j;
        atomicAdd(&hist[(size_t)w.rank * 16 + pat], 1u);
    }
}

// ranks[0], ranks[1] = the first reference CpG at or behind lo, hi: the windows whose first locus lies in [lo, hi)
__global__ void pattern_ranks_kernel(const int64_t* __restrict__ cpg_pos, int64_t n_cpg, int64_t lo, int64_t hi, int64_t* __restrict__ ranks) {
    if (threadIdx.x < 2) ranks[threadIdx.x] = lower_rank(cpg_pos, n_cpg, threadIdx.x ? hi : lo);
}

// the rows over RANKS: a valid window with at least min_reads contributing records
struct PatSel {
    using Row = hm_pattern_t;
    PatRule rule;
    const uint32_t* hist;
    int64_t min_reads;
    __device__ bool pred(int64_t r) const {
        if (!rule.valid(r)) return false;
        int64_t n = 0;
        for (int b = 0; b < 16; ++b) n += hist[r * 16 + b];
        return n >= min_reads;
    }
    __device__ bool take(int64_t r, Row& w) const {
        if (!rule.valid(r)) return false;
        int64_t n = 0;
        for (int b = 0; b < 16; ++b) n += (w.counts[b] = hist[r * 16 + b]);
        if (n < min_reads) return false;
        w.start = rule.cpg_pos[r];
        w.end = rule.cpg_pos[r + rule.k - 1] + 2;
        w.n = (uint32_t)n;
        w.k = (uint32_t)rule.k;
        return true;
    }
};

// ---- bedMethyl depth classes (`pileup -M`; include/hifimeth_hip.h has the definition) ----------------------------------------
// Five uint32 counters per reference CpG and set (0 = every record, 1 / 2 = the haplotype partitions):
// bm[(set * n_cpg + rank) * BM_CLASSES + class].  NOCALL and DIFF come from the aligned columns (depth_kernel), DELETE from the
// D operations (depth_gap_kernel), both behind the projection; MOD and CANON from the resident records once the threshold is
// known (depth_count_kernel).  Integer atomics only: any order gives the same counters.
enum BmClass { BM_MOD = 0, BM_CANON, BM_NOCALL, BM_DIFF, BM_DELETE, BM_CLASSES };

struct PGap {           // 16 bytes: one D operation of non-zero length
    int64_t g0;         // reference offset (concatenated) of the first deleted base
    int32_t len;
    int32_t read;
};

struct BmCounters {
    const int64_t* cpg_pos;  // the reference CpGs, ascending
    int64_t n_cpg;
    uint32_t* bm;
    // rank of the reference CpG whose C is g, or -1 (the C | G that straddles two sequences is none)
    __device__ int64_t rank_of(int64_t g) const {
        const int64_t r = lower_rank(cpg_pos, n_cpg, g);
        return r < n_cpg && cpg_pos[r] == g ? r : -1;
    }
    // hp is 1 or 2 only on an engine with the partitions option, whose counters hold three sets
    __device__ void add(int64_t rank, int cls, uint32_t hp) const {
        atomicAdd(&bm[rank * BM_CLASSES + cls], 1u);
        if (hp) atomicAdd(&bm[((int64_t)hp * n_cpg + rank) * BM_CLASSES + cls], 1u);
    }
};

// One thread per aligned column, project_kernel's geometry.  Only a column on the C of a reference CG goes further: the
// alignment ends on it (nothing), its run ends on it or the stored bases are not C, G (DIFF), the read carries no 5mC entry there
// (NOCALL); a member column adds nothing here, its record does in depth_count_kernel.
__global__ __launch_bounds__(TPB) void depth_kernel(BatchView b, int64_t total, BmCounters cnt) {
    walk_columns(b, [&](int ri, const PRun& run, int o, bool in_range) {
        if (!in_range) return;
        const int64_t g = run.g0 + o;
        if (b.ref[g] != 'C' || g + 1 >= total || b.ref[g + 1] != 'G') return;
        const PRead rd = b.reads[run.read];
        if (!read_takes_part(rd, run.read, b.matches, b.min_pi)) return;
        int cls = BM_DIFF;
        if (o == run.len - 1) {  // the run ends on the C
            if (ri + 1 == b.n_runs || b.runs[ri + 1].read != run.read) return;  // ... and so does the alignment
        } else if (cpg_columns(b, rd, run, o)) {
            if (cpg_call(b, rd, run.q0 + o) >= 0) return;  // a member
            cls = BM_NOCALL;
        }
        const int64_t r = cnt.rank_of(g);
        if (r >= 0) cnt.add(r, cls, rd.hp);
    });
}

// One thread per D operation: DELETE at every reference CpG whose C it removes.  A long deletion is a loop in one thread.
__global__ __launch_bounds__(TPB) void depth_gap_kernel(const PGap* __restrict__ gaps, int64_t n, const PRead* __restrict__ reads,
                                                         const int32_t* __restrict__ matches, double min_pi, BmCounters cnt) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const PGap gap = gaps[i];
        const PRead rd = reads[gap.read];
        if (!read_takes_part(rd, gap.read, matches, min_pi)) continue;
        const int64_t r1 = lower_rank(cnt.cpg_pos, cnt.n_cpg, gap.g0 + gap.len);
        for (int64_t r = lower_rank(cnt.cpg_pos, cnt.n_cpg, gap.g0); r < r1; ++r) cnt.add(r, BM_DELETE, rd.hp);
    }
}

// One thread per resident record: a CpG (motif 0) record is a member at the reference CpG gpos -> MOD or CANON by thr[CpG]
__global__ __launch_bounds__(TPB) void depth_count_kernel(const PRec* __restrict__ recs, int64_t n, uint32_t thr, BmCounters cnt) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const PRec rec = recs[i];
        if (rec.motif()) continue;
        const int64_t r = cnt.rank_of(rec.gpos());
        if (r >= 0) cnt.add(r, rec.prob() >= thr ? BM_MOD : BM_CANON, rec.hp());
    }
}

// the rows over RANKS of one set (bm points at the set's counters): a reference CpG some record was classed at, with
// n_mod + n_canon >= min_valid
struct BmSel {
    using Row = hm_bedmethyl_t;
    const int64_t* cpg_pos;
    const uint32_t* bm;
    int64_t min_valid;
    __device__ bool pred(int64_t r) const {
        const uint32_t* c = bm + r * BM_CLASSES;
        return ((uint64_t)c[0] + c[1] + c[2] + c[3] + c[4]) >= 1 && (int64_t)c[BM_MOD] + c[BM_CANON] >= min_valid;
    }
    __device__ bool take(int64_t r, Row& w) const {
        if (!pred(r)) return false;
        const uint32_t* c = bm + r * BM_CLASSES;
        w.gpos = cpg_pos[r];
        w.n_mod = c[BM_MOD];
        w.n_canon = c[BM_CANON];
        w.n_nocall = c[BM_NOCALL];
        w.n_diff = c[BM_DIFF];
        w.n_delete = c[BM_DELETE];
        w.reserved = 0;
        return true;
    }
};

// ---- within-read CpG co-methylation by distance (`pileup -L`; include/hifimeth_hip.h has the definition) ---------------------
// The thresholds arrive with hm_pileup_count, the pairs of a batch are gone by then, and there are too many to keep.  So the
// pairs are counted threshold-free: per distance d three 256-bin uint64 histograms over the pair's two ML bytes,
// lh[(d * 3 + LH_MIN) * 256 + min(pa, pb)], ... LH_MAX ... max(pa, pb), ... LH_FIRST ... pa (the lower coordinate's), from
// which the four classes follow for any threshold (linkage_reduce_kernel).  Integer atomics only: any order gives the same table.
constexpr int LINK_MAX_DIST = 16384;
enum LinkHist { LH_MIN = 0, LH_MAX, LH_FIRST, LH_HISTS };

struct PMember {        // 16 bytes: a member locus of record `read` of the batch
    int64_t g;
    int32_t read;
    uint32_t prob;
};
static_assert(sizeof(PMember) == 16, "member entries are 16 bytes");

// The batch's member list over its aligned COLUMNS [0, n_cols): column order keeps the members of a record together and ascending
// in g.  The selection skeleton asks per index, not per tile: the run search is the un-hinted one.
struct MemberSel {
    using Row = PMember;
    BatchView b;
    // the ML byte of the member at column c, or -1
    __device__ int member(int64_t c, Row& m) const {
        const int ri = find_run(b.col0, b.n_runs, c);
        const PRun run = b.runs[ri];
        const int o = (int)(c - b.col0[ri]);
        if (run.len - o < 2) return -1;
        const PRead rd = b.reads[run.read];
        if (!read_takes_part(rd, run.read, b.matches, b.min_pi)) return -1;
        const int p = cpg_member(b, rd, run, o);
        if (p < 0) return -1;
        m.g = run.g0 + o;
        m.read = run.read;
        m.prob = (uint32_t)p;
        return p;
    }
    __device__ bool pred(int64_t c) const {
        Row m;
        return member(c, m) >= 0;
    }
    __device__ bool take(int64_t c, Row& m) const { return member(c, m) >= 0; }
};

// One thread per list entry i: the pairs (i, j), j behind i in the same record with 2 <= g_j - g_i <= max_dist, three atomics each.
// The walk ends at the record's last member or max_dist bases on; no workgroup waits for another.
__global__ __launch_bounds__(TPB) void linkage_pair_kernel(const PMember* __restrict__ list, int64_t n, int max_dist,
                                                            unsigned long long* __restrict__ lh) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) {
        const PMember a = list[i];
        for (int64_t j = i + 1; j < n; ++j) {
            const PMember b = list[j];
            if (b.read != a.read) break;
            const int64_t d = b.g - a.g;
            if (d > max_dist) break;
            if (d < 2) continue;  // members are CG dinucleotides: never nearer than 2
            unsigned long long* h = lh + (size_t)d * (LH_HISTS * 256);
            atomicAdd(&h[LH_MIN * 256 + min(a.prob, b.prob)], 1ull);
            atomicAdd(&h[LH_MAX * 256 + max(a.prob, b.prob)], 1ull);
            atomicAdd(&h[LH_FIRST * 256 + a.prob], 1ull);
        }
    }
}

// One workgroup per distance d, thread v holds bin v: with t the CpG threshold, n = sum min, MM = sum_{v >= t} min,
// UU = sum_{v < t} max, MU = sum_{v >= t} first - MM, UM = n - MM - UU - MU -> tab[d * 4 + (UU, UM, MU, MM)]
__global__ __launch_bounds__(256) void linkage_reduce_kernel(const unsigned long long* __restrict__ lh, uint32_t thr,
                                                              unsigned long long* __restrict__ tab) {
    __shared__ unsigned long long part[256 / 64][4];
    const unsigned long long* h = lh + (size_t)blockIdx.x * (LH_HISTS * 256);
    const uint32_t v = threadIdx.x;
    const unsigned long long mn = h[LH_MIN * 256 + v], mx = h[LH_MAX * 256 + v], fi = h[LH_FIRST * 256 + v];
    unsigned long long s[4] = {mn, v >= thr ? mn : 0ull, v < thr ? mx : 0ull, v >= thr ? fi : 0ull};  // n, MM, UU, M at the first
    for (int c = 0; c < 4; ++c) {
        for (int d = 32; d; d >>= 1) s[c] += __shfl_down(s[c], d);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t[4];
        for (int c = 0; c < 4; ++c) t[c] = part[0][c] + part[1][c] + part[2][c] + part[3][c];
        const unsigned long long n = t[0], mm = t[1], uu = t[2], mu = t[3] - mm;
        unsigned long long* o = tab + (size_t)blockIdx.x * 4;
        o[0] = uu;
        o[1] = n - mm - uu - mu;
        o[2] = mu;
        o[3] = mm;
    }
}

// the rows over DISTANCES: n = the four counts' sum >= min_pairs
struct LinkSel {
    using Row = hm_linkage_t;
    const unsigned long long* tab;
    int64_t min_pairs;
    __device__ bool pred(int64_t d) const {
        const unsigned long long* c = tab + d * 4;
        return c[0] + c[1] + c[2] + c[3] >= (unsigned long long)min_pairs;
    }
    __device__ bool take(int64_t d, Row& w) const {
        if (!pred(d)) return false;
        const unsigned long long* c = tab + d * 4;
        w.dist = (uint32_t)d;
        w.reserved = 0;
        w.n_uu = c[0];
        w.n_um = c[1];
        w.n_mu = c[2];
        w.n_mm = c[3];
        return true;
    }
};

// ---- the rows of the read-position table (`pileup -P`) -----------------------------------------------------------------------
// One workgroup per histogram row (motif, bin), thread v holds bin v: with t the motif's threshold, n_m = sum_{v >= t} h[v]
// (count_kernel's >=), n_u = sum_{v < t} h[v], sum_ml = sum v h[v] -> tab[row * 3 + (n_m, n_u, sum_ml)]
__global__ __launch_bounds__(256) void readpos_reduce_kernel(ReadPos rp, uint32_t thr_packed, unsigned long long* __restrict__ tab) {
    __shared__ unsigned long long part[256 / 64][3];
    const uint32_t thr = (thr_packed >> (8 * (blockIdx.x / (unsigned)rp.rows()))) & 255u;
    const uint32_t v = threadIdx.x;
    const unsigned long long h = rp.hist[(size_t)blockIdx.x * 256 + v];
    unsigned long long s[3] = {v >= thr ? h : 0ull, v < thr ? h : 0ull, h * v};
    for (int c = 0; c < 3; ++c) {
        for (int d = 32; d; d >>= 1) s[c] += __shfl_down(s[c], d);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) tab[(size_t)blockIdx.x * 3 + threadIdx.x] = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// the rows over the table's ROW indices, which are in output order: n_m + n_u >= min_calls
struct ReadPosSel {
    using Row = hm_readpos_t;
    const unsigned long long* tab;
    int D;
    int64_t min_calls;
    __device__ bool pred(int64_t i) const { return tab[i * 3] + tab[i * 3 + 1] >= (unsigned long long)min_calls; }
    __device__ bool take(int64_t i, Row& w) const {
        if (!pred(i)) return false;
        const int bin = (int)(i % (2 * D + 1));
        w.motif = (uint32_t)(i / (2 * D + 1));
        w.end = bin < D ? 0u : bin < 2 * D ? 1u : 2u;
        w.dist = bin < D ? (uint32_t)bin : bin < 2 * D ? (uint32_t)(bin - D) : 0u;
        w.reserved = 0;
        w.n_m = tab[i * 3];
        w.n_u = tab[i * 3 + 1];
        w.sum_ml = tab[i * 3 + 2];
        return true;
    }
};

// hm_pileup_add_readpos: counts from elsewhere, counter by counter
__global__ __launch_bounds__(TPB) void readpos_add_kernel(const unsigned long long* __restrict__ add, int64_t n, unsigned long long* __restrict__ hist) {
    for (int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * TPB) hist[i] += add[i];
}

// ---- allele-specific methylation: loci tested between the two haplotype partitions -----------------
// A locus is tested when each haplotype has pcov + ncov >= min_cov.  The planes may be the caller's: counters that are not
// plain counts (negative) never pass, so the table lookups below stay inside [0, total].
constexpr int LFACT_N = 65536;  // log n! for n < LFACT_N from the uploaded table, beyond it from lgamma in the kernel

__device__ __forceinline__ bool asm_tested(int32_t p1, int32_t n1, int32_t p2, int32_t n2, int32_t min_cov) {
    return (p1 | n1 | p2 | n2) >= 0 && (int64_t)p1 + n1 >= min_cov && (int64_t)p2 + n2 >= min_cov;
}

// the row of a tested locus; diff and pvalue are filled by asm_test_kernel
__device__ __forceinline__ void asm_row(hm_asm_t& r, int64_t gpos, int32_t p1, int32_t n1, int32_t p2, int32_t n2, uint32_t key) {
    r.gpos = gpos;
    r.pcov1 = p1;
    r.ncov1 = n1;
    r.pcov2 = p2;
    r.ncov2 = n2;
    r.motif = key & 3u;
    r.reserved = 0;
    r.diff = 0.0;
    r.pvalue = 0.0;
}

__device__ __forceinline__ double lfact(const double* __restrict__ tab, int64_t k) {
    return k < LFACT_N ? tab[k] : lgamma((double)k + 1.0);
}

// One thread per tested row.  With the margins of [[p1, n1], [p2, n2]] fixed the first cell x runs over
// [max(0, c1 - r2), min(r1, c1)] and P(x) is proportional to exp(l(x)), l(x) = -log(x! (r1-x)! (c1-x)! (r2-c1+x)!).
// Two-sided p, R's fisher.test rule: the sum of P(x) over the tables with P(x) <= P(observed) * (1 + 1e-7), taken in logs as
// l(x) - l(observed) <= log1p(1e-7): ties that differ by rounding only fall on the same side.  Numerator and denominator are
// both summed as exp(l(x) - l(near the mode)) in ascending x, so the value is a pure function of the four counts, terms never
// overflow, and a row where every table is included gives num == den bit for bit, i.e. exactly 1.
__global__ __launch_bounds__(TPB) void asm_test_kernel(hm_asm_t* __restrict__ rows, int64_t n_rows, const double* __restrict__ tab) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t a = rows[i].pcov1, b = rows[i].ncov1, c = rows[i].pcov2, d = rows[i].ncov2;
    const int64_t r1 = a + b, r2 = c + d, c1 = a + c;
    // IEEE multiply, divide, subtract, each rounded once: bit-equal to the host's 100.0 * p1 / (p1 + n1) - 100.0 * p2 / (p2 + n2)
    rows[i].diff = __dsub_rn(__ddiv_rn(__dmul_rn(100.0, (double)a), (double)r1), __ddiv_rn(__dmul_rn(100.0, (double)c), (double)r2));
    const int64_t xlo = c1 > r2 ? c1 - r2 : 0, xhi = r1 < c1 ? r1 : c1;
    auto l = [&](int64_t x) { return -(((lfact(tab, x) + lfact(tab, r1 - x)) + lfact(tab, c1 - x)) + lfact(tab, r2 - c1 + x)); };
    int64_t xm = (int64_t)(((double)c1 + 1.0) * ((double)r1 + 1.0) / ((double)(r1 + r2) + 2.0));  // the mode, give or take rounding
    xm = xm < xlo ? xlo : xm > xhi ? xhi : xm;
    const double lref = l(xm), lobs = l(a);
    const double band = 9.9999995000000333e-08;  // log1p(1e-7)
    double num = 0.0, den = 0.0;
    for (int64_t x = xlo; x <= xhi; ++x) {
        const double lx = l(x);
        const double e = exp(lx - lref);
        den += e;
        if (lx - lobs <= band) num += e;
    }
    double p = num / den;
    if (lobs - lref < -600.0) {  // exp(l(observed) - lref) nears the subnormals: sum the included tables relative to the observed one
        double rel = 0.0;
        for (int64_t x = xlo; x <= xhi; ++x) {
            const double t = l(x) - lobs;
            if (t <= band) rel += exp(t);
        }
        p = exp((lobs - lref) + log(rel / den));
    }
    rows[i].pvalue = p > 1.0 ? 1.0 : p >= DBL_MIN ? p : DBL_MIN;  // never 0: a p-value below the smallest normal double is reported as that
}

// ---- per-locus binomial test against a false-positive rate (`pileup -B / -e`) ----------------------
// With the rates fixed, p and q of a locus are functions of (motif, pcov, pcov + ncov) alone, so the device only counts how many
// loci carry each triple (sites_hist_kernel), the host solves the table (hm_sites_table) and a second pass writes the rows by
// lookup (SitesSel).  A locus takes part when both counters are counts and one is positive: the planes may be the
// caller's, and a negative counter never indexes a table.  A key whose low bits are 3 is CHH, as in the BED writers.
constexpr int SITE_N = 256;      // loci with pcov + ncov below this are histogrammed, the others listed ("big" loci)
constexpr int SITE_LDS_N = 64;   // ... and below this in the workgroup's LDS histogram: 3 x 64 x 64 x 4 B = 48 KB

__device__ __forceinline__ bool site_counted(int32_t p, int32_t n) { return (p | n) > 0; }
__device__ __forceinline__ uint32_t site_motif(uint32_t key) { return min(key & 3u, 2u); }

// sums[motif] += pcov, sums[3 + motif] += ncov over the counted loci of [lo, hi): registers, wavefront shuffle, LDS, then at
// most six global atomics per workgroup
__global__ __launch_bounds__(TPB) void sites_sums_kernel(const int32_t* __restrict__ pcov, const int32_t* __restrict__ ncov,
                                                          const uint32_t* __restrict__ key, int64_t lo, int64_t hi,
                                                          unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long part[TPB / 64][6];
    unsigned long long s[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = lo + (int64_t)blockIdx.x * TPB + threadIdx.x; i < hi; i += (int64_t)gridDim.x * TPB) {
        const int32_t p = pcov[i], n = ncov[i];
        if (!site_counted(p, n)) continue;
        const uint32_t m = site_motif(key[i]);
        for (uint32_t c = 0; c < 3; ++c) {  // (no dynamic register indexing)
            s[c] += m == c ? (unsigned long long)p : 0ull;
            s[3 + c] += m == c ? (unsigned long long)n : 0ull;
        }
    }
    for (int c = 0; c < 6; ++c) {
        for (int d = 32; d; d >>= 1) s[c] += __shfl_down(s[c], d);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned long long t = 0;
        for (int w = 0; w < TPB / 64; ++w) t += part[w][threadIdx.x];
        if (t) atomicAdd(&sums[threadIdx.x], t);
    }
}

// bins[(motif * 256 + n) * 256 + k] += 1 for every counted locus with k = pcov, n = pcov + ncov < 256; block_big[b] = number of
// loci with n >= 256 in the b-th LOCI_PER_BLOCK loci of the range (the counts loci_scan_kernel turns into offsets).  At 30x
// nearly every locus falls on a few dozen triples, so the corner n < 64 is counted in LDS and reaches `bins` once per
// workgroup, as in mods_kernel; only the rare loci outside it pay a global atomic each.  A workgroup walks the blocks
// b = blockIdx.x, + gridDim.x, ...: the host keeps that below 2^19 blocks, so an LDS counter (uint32) cannot wrap.
__global__ __launch_bounds__(TPB) void sites_hist_kernel(const int32_t* __restrict__ pcov, const int32_t* __restrict__ ncov,
                                                          const uint32_t* __restrict__ key, int64_t lo, int64_t hi, int64_t nblk,
                                                          unsigned long long* __restrict__ bins, int32_t* __restrict__ block_big) {
    __shared__ uint32_t h[3 * SITE_LDS_N * SITE_LDS_N];
    for (int i = threadIdx.x; i < 3 * SITE_LDS_N * SITE_LDS_N; i += TPB) h[i] = 0u;
    __syncthreads();
    for (int64_t b = blockIdx.x; b < nblk; b += gridDim.x) {  // (uniform over the workgroup: the barriers below are safe)
        const int64_t base = lo + b * LOCI_PER_BLOCK;
        int big = 0;
        for (int k = 0; k < LOCI_PER_BLOCK / TPB; ++k) {
            const int64_t i = base + k * TPB + threadIdx.x;
            if (i >= hi) continue;
            const int32_t p = pcov[i], n = ncov[i];
            if (!site_counted(p, n)) continue;
            const int64_t tot = (int64_t)p + n;
            const uint32_t m = site_motif(key[i]);
            if (tot < SITE_LDS_N) atomicAdd(&h[(m * SITE_LDS_N + (uint32_t)tot) * SITE_LDS_N + (uint32_t)p], 1u);
            else if (tot < SITE_N) atomicAdd(&bins[(m * SITE_N + (uint32_t)tot) * SITE_N + (uint32_t)p], 1ull);
            else ++big;
        }
        big = block_sum(big);
        if (threadIdx.x == 0) block_big[b] = big;
        __syncthreads();
    }
    for (int i = threadIdx.x; i < 3 * SITE_LDS_N * SITE_LDS_N; i += TPB)
        if (h[i]) {
            const uint32_t m = (uint32_t)i / (SITE_LDS_N * SITE_LDS_N), n = ((uint32_t)i / SITE_LDS_N) % SITE_LDS_N, k = (uint32_t)i % SITE_LDS_N;
            atomicAdd(&bins[(m * SITE_N + n) * SITE_N + k], (unsigned long long)h[i]);
        }
}

// the big loci (n >= 256) of the range, where sites_hist_kernel counted them
struct SitesBigSel {
    using Row = hm_locus_t;
    RangePlanes s;
    int64_t plane_base;
    __device__ bool pred(int64_t i) const { return site_counted(s.pc[i], s.nc[i]) && (int64_t)s.pc[i] + s.nc[i] >= SITE_N; }
    __device__ bool take(int64_t i, Row& l) const {
        const int32_t p = s.pc[i], n = s.nc[i];
        if (!site_counted(p, n) || (int64_t)p + n < SITE_N) return false;
        l.gpos = plane_base + i;
        l.pcov = p;
        l.ncov = n;
        l.motif = site_motif(s.ky[i]);
        l.reserved = 0;
        return true;
    }
};

// a row of <prefix>.sites.<ctx>.bed: a counted locus whose context is tested (bit `motif` of ctx_mask)
__device__ __forceinline__ bool site_tested(int32_t p, int32_t n, uint32_t key, uint32_t ctx_mask) {
    return site_counted(p, n) && ((ctx_mask >> site_motif(key)) & 1u);
}

// rows with pvalue / qvalue looked up: n < 256 in tab[(motif * 256 + n) * 256 + k] (ptab, then qtab behind it), a big locus by
// its position in the ascending list `big` (big_p / big_q run parallel to it; NaN if the list does not hold the locus)
struct SitesSel {
    using Row = hm_site_t;
    RangePlanes s;
    int64_t plane_base;
    uint32_t ctx_mask;
    const double* tab;
    const hm_locus_t* big;
    const double* big_pq;
    int64_t n_big;
    __device__ bool pred(int64_t i) const { return site_tested(s.pc[i], s.nc[i], s.ky[i], ctx_mask); }
    __device__ bool take(int64_t i, Row& r) const {
        const int32_t p = s.pc[i], n = s.nc[i];
        const uint32_t ky = s.ky[i];
        if (!site_tested(p, n, ky, ctx_mask)) return false;
        r.gpos = plane_base + i;
        r.pcov = p;
        r.ncov = n;
        r.motif = site_motif(ky);
        r.reserved = 0;
        const int64_t tot = (int64_t)p + n;
        if (tot < SITE_N) {
            const uint32_t t = (r.motif * SITE_N + (uint32_t)tot) * SITE_N + (uint32_t)p;
            r.pvalue = tab[t];
            r.qvalue = tab[3 * SITE_N * SITE_N + t];
        } else {
            int64_t a = 0, b = n_big;  // first entry with gpos >= r.gpos
            while (a < b) {
                const int64_t mid = (a + b) >> 1;
                if (big[mid].gpos < r.gpos) a = mid + 1; else b = mid;
            }
            const bool found = a < n_big && big[a].gpos == r.gpos;
            r.pvalue = found ? big_pq[a] : __longlong_as_double(0x7ff8000000000000ll);
            r.qvalue = found ? big_pq[n_big + a] : __longlong_as_double(0x7ff8000000000000ll);
        }
        return true;
    }
};

// ---- Benjamini-Hochberg q-values of the haplotype test (`pileup -H -A -Q`) --------------------------------
// asm_test_kernel makes pvalue a function of (p1, n1, p2, n2), so BH needs the number of tested loci per tuple and context only.
// Tuples with both haplotype totals below ASM_T are counted in bins[HM_ASM_BINS] (asm_hist_kernel), the others ("big" loci) listed;
// the non-empty bins are compacted (BinsSel), turned into pseudo-rows for asm_test_kernel (asm_bin_rows_kernel) and take its p
// (asm_bin_p_kernel); the host solves the q-values (hm_asm_qvalues) and asm_q_write_kernel puts them next to the rows
// AsmSel + asm_test_kernel produced.  Only counters that pass asm_tested ever form a bin index.
constexpr int ASM_T = HM_ASM_T;
constexpr uint32_t ASM_PAIRS = HM_ASM_PAIRS;
static_assert(ASM_T * (ASM_T + 1) / 2 == HM_ASM_PAIRS && 3ll * HM_ASM_PAIRS * HM_ASM_PAIRS == HM_ASM_BINS, "the dense tuple space");

// of a tested locus: both haplotype totals below ASM_T
__device__ __forceinline__ bool asm_dense(int32_t p1, int32_t n1, int32_t p2, int32_t n2) {
    return (int64_t)p1 + n1 < ASM_T && (int64_t)p2 + n2 < ASM_T;
}
__device__ __forceinline__ uint32_t asm_pair(int32_t p, int32_t n) {  // 0 <= p, n and p + n < ASM_T -> [0, ASM_PAIRS)
    const uint32_t t = (uint32_t)(p + n);
    return t * (t + 1) / 2 + (uint32_t)p;
}
__device__ __forceinline__ void asm_unpair(uint32_t pair, int32_t& p, int32_t& n) {
    uint32_t t = 0;
    while ((t + 1) * (t + 2) / 2 <= pair) ++t;
    p = (int32_t)(pair - t * (t + 1) / 2);
    n = (int32_t)t - p;
}
__device__ __forceinline__ uint32_t asm_bin(uint32_t key, int32_t p1, int32_t n1, int32_t p2, int32_t n2) {  // of a tested dense locus
    return (site_motif(key) * ASM_PAIRS + asm_pair(p1, n1)) * ASM_PAIRS + asm_pair(p2, n2);
}

// bins[asm_bin] += 1 for every tested dense locus of [lo, hi), block_big[b] = number of tested big loci in the b-th LOCI_PER_BLOCK
// loci.  Tested loci are a few percent of the reference and spread over far more bins than LDS holds (104 MB): one 64-bit global
// atomic each.
__global__ __launch_bounds__(TPB) void asm_hist_kernel(const int32_t* __restrict__ pcov1, const int32_t* __restrict__ ncov1,
                                                        const int32_t* __restrict__ pcov2, const int32_t* __restrict__ ncov2,
                                                        const uint32_t* __restrict__ key, int64_t lo, int64_t hi, int32_t min_cov,
                                                        unsigned long long* __restrict__ bins, int32_t* __restrict__ block_big) {
    count_block(lo, hi, block_big, [&](int64_t i) {
        const int32_t p1 = pcov1[i], n1 = ncov1[i], p2 = pcov2[i], n2 = ncov2[i];
        if (!asm_tested(p1, n1, p2, n2, min_cov)) return false;
        if (!asm_dense(p1, n1, p2, n2)) return true;
        atomicAdd(&bins[asm_bin(key[i], p1, n1, p2, n2)], 1ull);
        return false;
    });
}

struct AsmPlanes {  // of a call over the haplotype planes: (pcov, ncov) of HP 1 and HP 2, key
    const int32_t *p1, *n1, *p2, *n2;
    const uint32_t* ky;
};

// The tested loci (ASM_ALL), those of context `ctx` (ASM_CTX: step 1 of `-G`), or the big ones where asm_hist_kernel counted them
// (ASM_BIG), as rows for asm_test_kernel.  Only ASM_CTX reads the key to select.
enum AsmWhich { ASM_ALL, ASM_CTX, ASM_BIG };
template <AsmWhich W>
struct AsmSel {
    using Row = hm_asm_t;
    AsmPlanes s;
    int64_t plane_base;
    int32_t min_cov;
    uint32_t ctx;
    __device__ bool selects(int64_t i, int32_t p1, int32_t n1, int32_t p2, int32_t n2) const {
        return asm_tested(p1, n1, p2, n2, min_cov) && (W != ASM_CTX || site_motif(s.ky[i]) == ctx) && (W != ASM_BIG || !asm_dense(p1, n1, p2, n2));
    }
    __device__ bool pred(int64_t i) const { return selects(i, s.p1[i], s.n1[i], s.p2[i], s.n2[i]); }
    __device__ bool take(int64_t i, Row& r) const {
        const int32_t p1 = s.p1[i], n1 = s.n1[i], p2 = s.p2[i], n2 = s.n2[i];
        if (!selects(i, p1, n1, p2, n2)) return false;
        asm_row(r, plane_base + i, p1, n1, p2, n2, s.ky[i]);
        return true;
    }
};

// ---- replicate groups (`groupdiff`, hm_pileup_fetch_groups; include/hifimeth_hip.h has the definition) ---------------------------
struct GroupPlanes {  // the partition planes hold K_g and N_g - K_g; with them the moment Q_g and the sample count m_g of each group
    AsmPlanes a;
    const unsigned long long *q1, *q2;
    const uint8_t *m1, *m2;
};

// the loci with min_reps counting samples in each group and at least one degree of freedom; D, phi, pvalue by group_test_kernel
struct GroupSel {
    using Row = hm_group_t;
    GroupPlanes s;
    int32_t min_reps;
    __device__ bool selects(int m1, int m2) const { return m1 >= min_reps && m2 >= min_reps && m1 + m2 >= 3; }
    __device__ bool pred(int64_t i) const { return selects(s.m1[i], s.m2[i]); }
    __device__ bool take(int64_t i, Row& r) const {
        const int m1 = s.m1[i], m2 = s.m2[i];
        if (!selects(m1, m2)) return false;
        r.gpos = i;
        r.pcov1 = s.a.p1[i];
        r.ncov1 = s.a.n1[i];
        r.pcov2 = s.a.p2[i];
        r.ncov2 = s.a.n2[i];
        r.motif = s.a.ky[i] & 3u;
        r.m1 = (uint16_t)m1;
        r.m2 = (uint16_t)m2;
        r.diff = r.D = r.phi = r.pvalue = 0.0;
        return true;
    }
};

// ... of context `ctx` only (step 1 of `groupdmr`)
struct GroupCtxSel {
    using Row = hm_group_t;
    GroupSel all;
    uint32_t ctx;
    __device__ bool pred(int64_t i) const { return all.pred(i) && site_motif(all.s.a.ky[i]) == ctx; }
    __device__ bool take(int64_t i, Row& r) const { return site_motif(all.s.a.ky[i]) == ctx && all.take(i, r); }
};

// x log(x / e) + e - x for a count x and its expectation e > 0, given d = x - e to full precision (the caller has it as an exact
// integer over N): Loader's series in v = d / (x + e) where the three terms would cancel, the plain form elsewhere.  >= 0.
__device__ __forceinline__ double deviance_part(double x, double e, double d) {
    if (fabs(d) < 0.1 * (x + e)) {
        const double v = d / (x + e), v2 = v * v;
        double s = d * v, ej = 2.0 * x * v;
        for (int j = 1; j < 1000; ++j) {
            ej *= v2;
            const double s1 = s + ej / (double)(2 * j + 1);
            if (s1 == s) break;
            s = s1;
        }
        return s;
    }
    return x == 0.0 ? e : x * log(x / e) - d;
}

// The continued fraction of the incomplete beta function, modified Lentz: I_x(a, b) = x^a (1 - x)^b / (a B(a, b)) * beta_cf(a, b, x),
// quick for x < (a + 1) / (a + b + 2).  Host and device: hm_sample_interval_test runs it on the host.
__host__ __device__ __forceinline__ double beta_cf(double a, double b, double x) {
    const double tiny = 1e-300, qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 2000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 1.2e-16) break;
    }
    return h;
}

// One thread per tested row.  coef[nu] = Gamma((nu + 1) / 2) / (sqrt(pi) Gamma(nu / 2 + 1)) = 1 / (a B(a, 1/2)), a = nu / 2, from the host.
// D: with E_g = N_g K / N the four "observed - expected" sum to 0, so D = 2 sum deviance_part(observed, expected) over the four
// cells, each >= 0 -- nothing cancels between the cells, and K_g - E_g = (K_g N - N_g K) / N has an exact integer numerator.
// X2: Q_g 2^-20 - K_g^2 / N_g = (Q_g N_g - K_g^2 2^20) / (N_g 2^20), the numerator exact in 128 bits.
__global__ __launch_bounds__(TPB) void group_test_kernel(hm_group_t* __restrict__ rows, int64_t n_rows, GroupPlanes s,
                                                          const double* __restrict__ coef) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_rows) return;
    const hm_group_t r = rows[i];
    const int64_t Kg[2] = {r.pcov1, r.pcov2}, Ng[2] = {(int64_t)r.pcov1 + r.ncov1, (int64_t)r.pcov2 + r.ncov2};
    const unsigned long long Qg[2] = {s.q1[r.gpos], s.q2[r.gpos]};
    const int64_t K = Kg[0] + Kg[1], N = Ng[0] + Ng[1];
    const int nu = (int)r.m1 + (int)r.m2 - 2;
    rows[i].diff = __dsub_rn(__ddiv_rn(__dmul_rn(100.0, (double)Kg[0]), (double)Ng[0]), __ddiv_rn(__dmul_rn(100.0, (double)Kg[1]), (double)Ng[1]));
    double D = 0.0, X2 = 0.0;
    const int64_t num = Kg[0] * Ng[1] - Ng[0] * Kg[1];  // (K_1 - E_1) N = -(K_2 - E_2) N
    if (num != 0) {
        for (int g = 0; g < 2; ++g) {
            const double d = (double)(g ? -num : num) / (double)N;
            const double e = (double)Ng[g] * (double)K / (double)N, f = (double)Ng[g] * (double)(N - K) / (double)N;
            D += deviance_part((double)Kg[g], e, d) + deviance_part((double)(Ng[g] - Kg[g]), f, -d);
        }
        D *= 2.0;
    }
    for (int g = 0; g < 2; ++g) {
        if (Kg[g] == 0 || Kg[g] == Ng[g]) continue;
        const __int128 a = (__int128)Qg[g] * (__int128)Ng[g] - ((__int128)(Kg[g] * Kg[g]) << 20);
        if (a <= 0) continue;
        const double ad = (double)(uint64_t)(a >> 64) * 18446744073709551616.0 + (double)(uint64_t)a;
        X2 += ad * (double)Ng[g] / (1048576.0 * (double)(Kg[g] * (Ng[g] - Kg[g])));
    }
    const double phi = fmax(1.0, X2 / (double)nu);
    rows[i].D = D;
    rows[i].phi = phi;
    if (D == 0.0) {
        rows[i].pvalue = 1.0;
        return;
    }
    const double F = D / phi, a = 0.5 * (double)nu;
    const double x = (double)nu / ((double)nu + F), y = F / ((double)nu + F);
    const double xa = y < 0.5 ? exp(a * log1p(-y)) : pow(x, a);
    const double front = coef[nu] * xa * sqrt(y);
    const double p = x < (a + 1.0) / (a + 2.5) ? front * beta_cf(a, 0.5, x) : 1.0 - 2.0 * a * front * beta_cf(0.5, a, y);
    rows[i].pvalue = p > 1.0 ? 1.0 : p >= DBL_MIN ? p : DBL_MIN;  // never 0, as asm_test_kernel's
}

// the non-empty bins of bins[0, n) in ascending index: the skeleton over the bin array instead of a plane range
struct BinsSel {
    using Row = hm_asm_bin_t;
    const unsigned long long* bins;
    __device__ bool pred(int64_t i) const { return bins[i] != 0ull; }
    __device__ bool take(int64_t i, Row& r) const {
        const unsigned long long c = bins[i];
        if (!c) return false;
        r.bin = (uint32_t)i;
        r.reserved = 0;
        r.count = c;
        r.pvalue = 0.0;
        r.qvalue = __longlong_as_double(0x7ff8000000000000ll);
        return true;
    }
};

// One thread per compact bin: the hm_asm_t row of a locus carrying the bin's tuple (gpos = the bin index, motif = its context).
__global__ __launch_bounds__(TPB) void asm_bin_rows_kernel(const hm_asm_bin_t* __restrict__ tab, int64_t n, hm_asm_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t b = tab[i].bin;
    hm_asm_t r;
    r.gpos = b;
    asm_unpair((b / ASM_PAIRS) % ASM_PAIRS, r.pcov1, r.ncov1);
    asm_unpair(b % ASM_PAIRS, r.pcov2, r.ncov2);
    r.motif = b / (ASM_PAIRS * ASM_PAIRS);
    r.reserved = 0;
    r.diff = 0.0;
    r.pvalue = 0.0;
    rows[i] = r;
}

// ... and what asm_test_kernel computed for it, back into the bin's entry
__global__ __launch_bounds__(TPB) void asm_bin_p_kernel(const hm_asm_t* __restrict__ rows, int64_t n, hm_asm_bin_t* __restrict__ tab) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < n) tab[i].pvalue = rows[i].pvalue;
}

// One thread per tested row (AsmSel's, after asm_test_kernel): the row with its qvalue -- a dense row's from the entry of
// its bin in tab[0, n_tab) (ascending in bin), a big row's from big_q at its place in big[0, n_big) (ascending in gpos); NaN when
// the entry is not there (a table made with another min_cov, a list that misses the locus).
__global__ __launch_bounds__(TPB) void asm_q_write_kernel(const hm_asm_t* __restrict__ rows, int64_t n_rows,
                                                           const hm_asm_bin_t* __restrict__ tab, int64_t n_tab,
                                                           const hm_asm_t* __restrict__ big, const double* __restrict__ big_q,
                                                           int64_t n_big, hm_asmq_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_rows) return;
    const hm_asm_t r = rows[i];
    double q = __longlong_as_double(0x7ff8000000000000ll);
    if (asm_dense(r.pcov1, r.ncov1, r.pcov2, r.ncov2)) {
        const uint32_t bin = asm_bin(r.motif, r.pcov1, r.ncov1, r.pcov2, r.ncov2);
        int64_t a = 0, b = n_tab;  // first entry with bin >= the row's
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (tab[mid].bin < bin) a = mid + 1; else b = mid;
        }
        if (a < n_tab && tab[a].bin == bin) q = tab[a].qvalue;
    } else {
        int64_t a = 0, b = n_big;  // first entry with gpos >= the row's
        while (a < b) {
            const int64_t mid = (a + b) >> 1;
            if (big[mid].gpos < r.gpos) a = mid + 1; else b = mid;
        }
        if (a < n_big && big[a].gpos == r.gpos) q = big_q[a];
    }
    hm_asmq_t o;
    o.gpos = r.gpos;
    o.pcov1 = r.pcov1;
    o.ncov1 = r.ncov1;
    o.pcov2 = r.pcov2;
    o.ncov2 = r.ncov2;
    o.motif = r.motif;
    o.reserved = r.reserved;
    o.diff = r.diff;
    o.pvalue = r.pvalue;
    o.qvalue = q;
    out[i] = o;
}

// ---- `pileup -H -A -G`: chains of tested rows that lean the same way (include/hifimeth_hip.h has the definition) ----------------
// Step 1 is the skeleton over the loci with the context added to the selection (AsmSel<ASM_CTX>); asm_test_kernel then fills diff
// and pvalue.
// Step 2 runs over the row indices [0, n_rows) the way the selections above run over loci: the selected index is the head of a
// returned chain, and the thread that owns it walks the rows forward to the chain's tail.  Only comparisons and integer sums: the
// result does not depend on how the rows fall on threads and workgroups, and a chain may cross any number of them.
struct RegionRule {
    double max_p;
    int64_t max_gap;
    int32_t min_loci, keep_edges;
};
struct GroupRegionRule : RegionRule {  // `groupdmr`: a hit also needs |diff| >= min_diff
    double min_diff;
};

// +1 / -1: rows[i] is a hit of that sign; 0: it is none
__device__ __forceinline__ int region_sign(const hm_asm_t* __restrict__ rows, int64_t i, const RegionRule& rule) {
    const double d = rows[i].diff;
    return rows[i].pvalue <= rule.max_p ? (d > 0.0) - (d < 0.0) : 0;
}
__device__ __forceinline__ int region_sign(const hm_group_t* __restrict__ rows, int64_t i, const GroupRegionRule& rule) {
    const double d = rows[i].diff;
    return rows[i].pvalue <= rule.max_p && fabs(d) >= rule.min_diff ? (d > 0.0) - (d < 0.0) : 0;
}
// rows i - 1 and i, i >= 1, are within max_gap: linked when both are also hits of one sign
template <class Unit>
__device__ __forceinline__ bool region_near(const Unit* __restrict__ rows, int64_t i, const RegionRule& rule) {
    return rows[i].gpos - rows[i - 1].gpos <= rule.max_gap;
}
// rows[i] starts a chain (of sign s)
template <class Unit, class Rule>
__device__ __forceinline__ bool region_head(const Unit* __restrict__ rows, int64_t i, const Rule& rule, int& s) {
    s = region_sign(rows, i, rule);
    return s != 0 && !(i > 0 && region_sign(rows, i - 1, rule) == s && region_near(rows, i, rule));
}
// rows[j] continues the chain of sign s that holds rows[j - 1]
template <class Unit, class Rule>
__device__ __forceinline__ bool region_next(const Unit* __restrict__ rows, int64_t j, int64_t n_rows, int s, const Rule& rule) {
    return j < n_rows && region_sign(rows, j, rule) == s && region_near(rows, j, rule);
}
__device__ __forceinline__ bool region_returned(int64_t n_loci, uint32_t flags, const RegionRule& rule) {
    return n_loci >= rule.min_loci || (rule.keep_edges && flags);
}

// What a family of rows adds to the walk: the rows it chains (Unit), the chain it returns (Row), its rule, and what a chain carries
// beyond the four sums and pmin -- started at the chain's head, fed every further row, stored once the chain is returned.
struct AsmChain {  // `pileup -H -A -G`, `diff -G`: nothing more
    using Unit = hm_asm_t;
    using Row = hm_asm_region_t;
    using Rule = RegionRule;
    __device__ void start(const Unit&) {}
    __device__ void add(const Unit&) {}
    __device__ void store(Row&) const {}
};
struct GroupChain {  // `groupdmr`: the largest dispersion and the fewest counting samples of each group among the chain's rows
    using Unit = hm_group_t;
    using Row = hm_group_region_t;
    using Rule = GroupRegionRule;
    double phi_max;
    uint16_t m1_min, m2_min;
    __device__ void start(const Unit& r) {
        phi_max = r.phi;
        m1_min = r.m1;
        m2_min = r.m2;
    }
    __device__ void add(const Unit& r) {
        phi_max = r.phi > phi_max ? r.phi : phi_max;
        m1_min = r.m1 < m1_min ? r.m1 : m1_min;
        m2_min = r.m2 < m2_min ? r.m2 : m2_min;
    }
    __device__ void store(Row& g) const {
        g.m1_min = m1_min;
        g.m2_min = m2_min;
        g.reserved = 0;
        g.phi_max = phi_max;
    }
};

// the hits among the group rows, by row index: what hm_dmr_fetch_regions counts for n_hits
struct GroupHitSel {
    using Row = int64_t;
    const hm_group_t* rows;
    GroupRegionRule rule;
    __device__ bool pred(int64_t i) const { return region_sign(rows, i, rule) != 0; }
    __device__ bool take(int64_t i, Row& r) const {
        r = i;
        return pred(i);
    }
};

template <class Chain>
struct RegionSel {
    using Row = typename Chain::Row;
    const typename Chain::Unit* rows;
    int64_t n_rows;
    typename Chain::Rule rule;
    uint32_t ctx;
    // The walk stops after min_loci rows: a chain that long is returned whatever its flags, a shorter one has been walked to its tail.
    __device__ bool pred(int64_t i) const {
        int s;
        if (!region_head(rows, i, rule, s)) return false;
        int64_t j = i + 1;
        while (j - i < rule.min_loci && region_next(rows, j, n_rows, s, rule)) ++j;
        return region_returned(j - i, (i == 0 ? HM_REGION_FIRST : 0u) | (j == n_rows ? HM_REGION_LAST : 0u), rule);
    }
    __device__ bool take(int64_t i, Row& g) const {
        int s;
        if (!region_head(rows, i, rule, s)) return false;
        int64_t P1 = 0, N1 = 0, P2 = 0, N2 = 0;
        double pmin = rows[i].pvalue;
        Chain more;
        more.start(rows[i]);
        int64_t j = i;
        do {
            P1 += rows[j].pcov1;
            N1 += rows[j].ncov1;
            P2 += rows[j].pcov2;
            N2 += rows[j].ncov2;
            const double pv = rows[j].pvalue;
            pmin = pv < pmin ? pv : pmin;
            more.add(rows[j]);
            ++j;
        } while (region_next(rows, j, n_rows, s, rule));
        g.flags = (i == 0 ? HM_REGION_FIRST : 0u) | (j == n_rows ? HM_REGION_LAST : 0u);
        if (!region_returned(j - i, g.flags, rule)) return false;
        g.start = rows[i].gpos;
        g.end = rows[j - 1].gpos + 1;
        g.pcov1 = P1;
        g.ncov1 = N1;
        g.pcov2 = P2;
        g.ncov2 = N2;
        g.n_loci = (int32_t)(j - i);
        g.sign = s;
        g.motif = ctx;
        // as the rows' own diff, on the pooled sums: each total is >= 1 (min_cov >= 1; a counting sample has group_min_cov >= 1 calls)
        g.diff = __dsub_rn(__ddiv_rn(__dmul_rn(100.0, (double)P1), (double)(P1 + N1)), __ddiv_rn(__dmul_rn(100.0, (double)P2), (double)(P2 + N2)));
        g.pmin = pmin;
        more.store(g);
        return true;
    }
};

// ---- `pileup -D`: methylation domains by a two-state Viterbi scan (include/hifimeth_hip.h has the definition) -------------------
// Step 1 is the skeleton over the loci with the context in the selection; the rows stay on the device.
struct DomRow {
    int64_t gpos;
    int32_t pcov, ncov;
};
struct DomSum {  // pcov and ncov summed over rows 0 .. t
    int64_t P, N;
};
struct DomRule {
    int64_t A, B, S, max_gap;
};
constexpr int64_t DOM_W = int64_t(1) << 24;        // |A|, |B|, S <= this
constexpr int32_t DOM_COV = (int32_t(1) << 20) - 1;  // a counter enters e_t clamped to this

struct DomRowSel {
    using Row = DomRow;
    RangePlanes s;
    int64_t plane_base;
    uint32_t ctx;
    __device__ static bool selects(int32_t p, int32_t n, uint32_t key, uint32_t ctx) { return site_counted(p, n) && site_motif(key) == ctx; }
    __device__ bool pred(int64_t i) const { return selects(s.pc[i], s.nc[i], s.ky[i], ctx); }
    __device__ bool take(int64_t i, Row& r) const {
        const int32_t p = s.pc[i], n = s.nc[i];
        if (!selects(p, n, s.ky[i], ctx)) return false;
        r.gpos = plane_base + i;
        r.pcov = p;
        r.ncov = n;
        return true;
    }
};

// Step 2, the row-scan skeleton: the inclusive scan of n elements under an associative operation, in three launches -- every
// workgroup reduces its SCAN_ROWS elements to one aggregate (rowscan_reduce_kernel), ONE workgroup turns the aggregates into
// their exclusive scan (rowscan_carry_kernel), every workgroup scans its elements again from its carry (rowscan_apply_kernel).
// No workgroup waits for another inside a launch.  A scan Sc brings: T, identity(), shfl_up(v, d) (v of the lane d below),
// op(a, b) with a the earlier operand, load(j) = element j, store(j, v) = what to keep of the inclusive scan at j.
constexpr int SCAN_ITEMS = 4;                 // consecutive elements per thread
constexpr int SCAN_ROWS = TPB * SCAN_ITEMS;   // elements per workgroup

// v = one value per thread of a workgroup of NT threads -> the combination of the values of all lower threads (identity for thread
// 0), and `total` = that of all NT, in every thread.  Wave64 shuffle scan, then the wavefront totals through LDS.
template <int NT, class Sc>
__device__ __forceinline__ typename Sc::T block_scan(const Sc& sc, typename Sc::T v, typename Sc::T& total) {
    using T = typename Sc::T;
    __shared__ T wtot[NT / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        const T o = Sc::shfl_up(v, d);
        if (lane >= d) v = sc.op(o, v);
    }
    if (lane == 63) wtot[w] = v;
    __syncthreads();
    T ex = Sc::shfl_up(v, 1);
    if (lane == 0) ex = Sc::identity();
    T pre = Sc::identity();
    total = Sc::identity();
    for (int j = 0; j < NT / 64; ++j) {
        if (j == w) pre = total;
        total = sc.op(total, wtot[j]);
    }
    return sc.op(pre, ex);
}

template <class Sc>
__global__ __launch_bounds__(TPB) void rowscan_reduce_kernel(Sc sc, int64_t n, typename Sc::T* __restrict__ agg) {
    using T = typename Sc::T;
    const int64_t j0 = (int64_t)blockIdx.x * SCAN_ROWS + (int64_t)threadIdx.x * SCAN_ITEMS;
    T v = Sc::identity();
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (j0 + k < n) v = sc.op(v, sc.load(j0 + k));
    T total;
    block_scan<TPB>(sc, v, total);
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// agg[0, nagg) -> their exclusive scan, in place: a thread owns a contiguous slice
template <class Sc>
__global__ __launch_bounds__(1024) void rowscan_carry_kernel(Sc sc, typename Sc::T* __restrict__ agg, int64_t nagg) {
    using T = typename Sc::T;
    const int64_t per = (nagg + 1023) / 1024;
    const int64_t lo = (int64_t)threadIdx.x * per, hi = min(nagg, lo + per);
    T v = Sc::identity();
    for (int64_t i = lo; i < hi; ++i) v = sc.op(v, agg[i]);
    T total;
    T run = block_scan<1024>(sc, v, total);
    for (int64_t i = lo; i < hi; ++i) {
        const T a = agg[i];
        agg[i] = run;
        run = sc.op(run, a);
    }
}

template <class Sc>
__global__ __launch_bounds__(TPB) void rowscan_apply_kernel(Sc sc, int64_t n, const typename Sc::T* __restrict__ carry) {
    using T = typename Sc::T;
    const int64_t j0 = (int64_t)blockIdx.x * SCAN_ROWS + (int64_t)threadIdx.x * SCAN_ITEMS;
    T item[SCAN_ITEMS];
    T v = Sc::identity();
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        item[k] = j0 + k < n ? sc.load(j0 + k) : Sc::identity();
        v = sc.op(v, item[k]);
    }
    T total;
    const T before = block_scan<TPB>(sc, v, total);
    T run = sc.op(carry[blockIdx.x], before);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        run = sc.op(run, item[k]);
        if (j0 + k < n) sc.store(j0 + k, run);
    }
}

// The forward scan.  With d_t = delta_t(1) - delta_t(0) the Viterbi recurrence is d_t = clamp(d_{t-1}, -S_t, S_t) + e_t, d_{-1} = 0
// (DESIGN.md section 10 has the derivation).  Row t is the function x -> clamp(x + c, lo, hi) with c = e_t, lo = e_t - S_t,
// hi = e_t + S_t; such functions are closed under composition, so d_t = (f_t o ... o f_0)(0) is an inclusive scan.  Every d lies
// within +-2^46 and so do lo and hi of anything that holds a row; the sum c is kept within +-DOM_CSAT = 2^48: beyond that the
// function is constant on [-2^46, 2^46], which is recorded as lo == hi, and from then on c no longer matters.  P and N ride along.
// The rows may be a PIECE of a range's (hm_pileup_fetch_domains_part): the rows before the piece enter through the nearest one's
// gpos and d.  Row 0 is loaded as the constant function d_0 = clamp(d_prev, -S_0, S_0) + e_0, S_0 = S only if that row exists within
// max_gap, d_prev = 0 without it -- composing a constant (lo == hi) is exact, c no longer matters -- so every d, sum and code
// equals the whole scan's; with no row before it that is d_0 = e_0, the whole range's start.  The last row's code is what the
// caller says (`last_code`), or its end state; its d goes to *d_last.  mask_first (pass S, reduce only): row 0 is the identity
// instead, the composite of rows 1 .. n - 1 needs no carry.
constexpr int64_t DOM_INF = int64_t(1) << 62, DOM_CSAT = int64_t(1) << 48;

struct DomFwd {
    struct T {
        int64_t c, lo, hi, P, N;
    };
    const DomRow* rows;
    int64_t n;
    DomRule rule;
    DomSum* sums;   // out: inclusive sums per row
    uint8_t* code;  // out: the back-pointer function from row t + 1 to row t, or at the last row the end state
    bool mask_first, has_prev;
    int64_t prev_gpos, prev_d;
    int last_code;     // TO0, TO1, KEEP, or -1: d > 0 decides
    int64_t* d_last;   // out
    enum : uint8_t { TO0 = 0, TO1 = 1, KEEP = 2 };

    __host__ __device__ __forceinline__ static T identity() { return T{0, -DOM_INF, DOM_INF, 0, 0}; }
    __device__ __forceinline__ static T shfl_up(const T& v, int d) {
        return T{__shfl_up(v.c, d), __shfl_up(v.lo, d), __shfl_up(v.hi, d), __shfl_up(v.P, d), __shfl_up(v.N, d)};
    }
    // S_t, t >= 1
    __device__ __forceinline__ int64_t switch_cost(int64_t t) const {
        return rows[t].gpos - rows[t - 1].gpos <= rule.max_gap ? rule.S : 0;
    }
    __device__ __forceinline__ T load(int64_t t) const {
        if (t == 0 && mask_first) return identity();
        const DomRow r = rows[t];
        const int64_t e = (int64_t)min(r.pcov, DOM_COV) * rule.A + (int64_t)min(r.ncov, DOM_COV) * rule.B;
        if (t > 0) {
            const int64_t s = switch_cost(t);
            return T{e, e - s, e + s, r.pcov, r.ncov};
        }
        const int64_t s = has_prev && r.gpos - prev_gpos <= rule.max_gap ? rule.S : 0;
        const int64_t d = min(max(has_prev ? prev_d : 0, -s), s) + e;
        return T{d, d, d, r.pcov, r.ncov};
    }
    __device__ __forceinline__ static T op(const T& a, const T& b) {  // b after a
        T r;
        r.c = a.c + b.c;
        r.lo = min(max(a.lo + b.c, b.lo), b.hi);
        r.hi = min(max(a.hi + b.c, b.lo), b.hi);
        if (r.c >= DOM_CSAT) {
            r.c = DOM_CSAT;
            r.lo = r.hi;
        } else if (r.c <= -DOM_CSAT) {
            r.c = -DOM_CSAT;
            r.hi = r.lo;
        }
        r.P = a.P + b.P;
        r.N = a.N + b.N;
        return r;
    }
    __device__ __forceinline__ void store(int64_t t, const T& f) const {
        const int64_t d = min(max(f.c, f.lo), f.hi);  // f(0)
        sums[t] = DomSum{f.P, f.N};
        if (t + 1 == n) {
            code[t] = last_code >= 0 ? (uint8_t)last_code : d > 0 ? TO1 : TO0;
            *d_last = d;
        } else {
            const int64_t s = switch_cost(t + 1);
            code[t] = d > s ? TO1 : d < -s ? TO0 : KEEP;
        }
    }
};

// The backward scan.  The back-pointer from row t + 1 is constant 1, constant 0 or the identity, never a swap, so the state of row
// t is the nearest code at or right of t that is no identity (the last row's code is its end state): element j of this scan is
// row n - 1 - j, and the later operand wins unless it is the identity.
struct DomBwd {
    using T = int;
    const uint8_t* code;
    int64_t n;
    uint8_t* state;  // out: z_t

    __host__ __device__ __forceinline__ static T identity() { return DomFwd::KEEP; }
    __device__ __forceinline__ static T shfl_up(T v, int d) { return __shfl_up(v, d); }
    __device__ __forceinline__ T load(int64_t j) const { return code[n - 1 - j]; }
    __device__ __forceinline__ static T op(T a, T b) { return b != DomFwd::KEEP ? b : a; }
    __device__ __forceinline__ void store(int64_t j, T z) const { state[n - 1 - j] = (uint8_t)z; }
};

// Steps 3 and 4 run over the row indices [0, n): a head is row 0, a row that follows a break, or one whose state differs from its
// predecessor's; the heads are compacted, and one thread per segment reads its tail off the next head.  No thread walks a segment.
__device__ __forceinline__ bool domain_break(const DomRow* __restrict__ rows, int64_t i, int64_t max_gap) {  // between rows i - 1 and i, i >= 1
    return rows[i].gpos - rows[i - 1].gpos > max_gap;
}
__device__ __forceinline__ bool domain_head(const DomRow* __restrict__ rows, const uint8_t* __restrict__ state, int64_t i, int64_t max_gap) {
    return i == 0 || state[i] != state[i - 1] || domain_break(rows, i, max_gap);
}

struct DomHeadSel {
    using Row = int64_t;  // the head's row index
    const DomRow* rows;
    const uint8_t* state;
    int64_t max_gap;
    __device__ bool pred(int64_t i) const { return domain_head(rows, state, i, max_gap); }
    __device__ bool take(int64_t i, Row& h) const {
        h = i;
        return pred(i);
    }
};

// the segment s of n_seg; first_break / last_break: whether a break lies before row 0 / behind row n - 1
__device__ __forceinline__ hm_domain_t domain_segment(const DomRow* __restrict__ rows, const DomSum* __restrict__ sums,
                                                      const uint8_t* __restrict__ state, const int64_t* __restrict__ heads, int64_t s,
                                                      int64_t n_seg, int64_t n, const DomRule& rule, uint32_t ctx, bool first_break,
                                                      bool last_break) {
    const int64_t h = heads[s], next = s + 1 < n_seg ? heads[s + 1] : n;
    const int64_t P = sums[next - 1].P - (h ? sums[h - 1].P : 0), N = sums[next - 1].N - (h ? sums[h - 1].N : 0);
    hm_domain_t g;
    g.start = rows[h].gpos;
    g.end = rows[next - 1].gpos + 1;
    g.pcov = P;
    g.ncov = N;
    g.n_loci = (int32_t)(next - h);
    g.state = state[h];
    g.motif = ctx;
    g.flags = ((h == 0 ? first_break : domain_break(rows, h, rule.max_gap)) ? HM_DOMAIN_AFTER_BREAK : 0u) |
              ((next == n ? last_break : domain_break(rows, next, rule.max_gap)) ? HM_DOMAIN_BEFORE_BREAK : 0u);
    // each operation rounded once: bit-equal to the host's 100.0 * P / (P + N) and (P * A + N * B) / 65536.0; P + N > 0 in every row
    g.level = __ddiv_rn(__dmul_rn(100.0, (double)P), (double)(P + N));
    g.score = __ddiv_rn(__dadd_rn(__dmul_rn((double)P, (double)rule.A), __dmul_rn((double)N, (double)rule.B)), 65536.0);
    return g;
}

// one thread per segment; the edges of a piece break only where the caller says so, those of a whole range always
__global__ __launch_bounds__(TPB) void domain_build_part_kernel(const DomRow* __restrict__ rows, const DomSum* __restrict__ sums,
                                                                 const uint8_t* __restrict__ state, const int64_t* __restrict__ heads,
                                                                 int64_t n_seg, int64_t n, DomRule rule, uint32_t ctx, bool first_break,
                                                                 bool last_break, hm_domain_t* __restrict__ out) {
    const int64_t s = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (s >= n_seg) return;
    out[s] = domain_segment(rows, sums, state, heads, s, n_seg, n, rule, ctx, first_break, last_break);
}

// `pileup -D -Y`: sums[0..5] += P0, N0, R0, P1, N1, R1 -- the unclamped pcov and ncov and the number of the n compact rows by
// their state.  Registers over a grid stride, wavefront shuffle, LDS, then at most six integer atomics per workgroup, as
// sites_sums_kernel; the host keeps the grid at DOM_SUMS_WGS workgroups at most.
constexpr int DOM_SUMS_WGS = 1024;

__global__ __launch_bounds__(TPB) void domain_sums_kernel(const DomRow* __restrict__ rows, const uint8_t* __restrict__ state, int64_t n,
                                                           unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long part[TPB / 64][6];
    unsigned long long s[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t t = (int64_t)blockIdx.x * TPB + threadIdx.x; t < n; t += (int64_t)gridDim.x * TPB) {
        const DomRow r = rows[t];
        const bool high = state[t] != 0;
        s[0] += high ? 0ull : (unsigned long long)r.pcov;
        s[1] += high ? 0ull : (unsigned long long)r.ncov;
        s[2] += high ? 0ull : 1ull;
        s[3] += high ? (unsigned long long)r.pcov : 0ull;
        s[4] += high ? (unsigned long long)r.ncov : 0ull;
        s[5] += high ? 1ull : 0ull;
    }
    for (int c = 0; c < 6; ++c) {
        for (int d = 32; d; d >>= 1) s[c] += __shfl_down(s[c], d);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][c] = s[c];
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned long long t = 0;
        for (int w = 0; w < TPB / 64; ++w) t += part[w][threadIdx.x];
        if (t) atomicAdd(&sums[threadIdx.x], t);
    }
}

// ---- sums over given intervals, metaplots (`pileup -R`, `pileup -J`; include/hifimeth_hip.h has the definition) ----------------
// Twelve int64 quantities, k = 4 * context + {n_loci, pcov, ncov, ppm}: hm_region_sum_t[3] as one array.  The index of a range
// [lo, hi) is idx[b * 12 + k] = the sum over the blocks 0 .. b of HM_REGION_BLOCK loci (region_block_sums_kernel, then the row scan
// above in place with RegionScan: no workgroup waits for another).  ONE wavefront answers a query: block_split, its loci over the lanes.
constexpr int REGION_LANES = 12;
static_assert(HM_REGION_BLOCK >= TPB && (HM_REGION_BLOCK & (HM_REGION_BLOCK - 1)) == 0, "a block is a power of two of whole workgroup passes");
static_assert(HM_REGION_SCAN_BLOCKS == SCAN_ROWS, "the header names the row scan's partition");
static_assert(sizeof(hm_region_sum_t) * 3 == sizeof(int64_t) * REGION_LANES, "a row of the index is three hm_region_sum_t");

struct RegionAcc {
    int64_t v[REGION_LANES];
};

// (2 000 000 p + cov) / (2 cov) for 0 <= p <= cov < 2^32, cov > 0, exactly: the numerator is below 2^53, so the fp64 quotient is
// within one of the integer one, and the remainder says which way
__device__ __forceinline__ int64_t region_ppm(int64_t p, int64_t cov) {
    const int64_t num = 2000000 * p + cov, den = 2 * cov;
    const int64_t q = (int64_t)((double)num / (double)den);
    const int64_t r = num - q * den;
    return r < 0 ? q - 1 : r >= den ? q + 1 : q;
}

// locus i of the planes, if it counts, into its context's four sums
__device__ __forceinline__ void region_add(const RangePlanes& s, int64_t min_cov, int64_t i, RegionAcc& a) {
    const int64_t p = s.pc[i], n = s.nc[i], cov = p + n;
    if (cov < min_cov) return;
    const uint32_t c = s.ky[i] & 3u;
    const int64_t ppm = region_ppm(p, cov);
#pragma unroll
    for (uint32_t m = 0; m < 3; ++m) {
        const bool on = c == m;
        a.v[4 * m] += on ? 1 : 0;
        a.v[4 * m + 1] += on ? p : 0;
        a.v[4 * m + 2] += on ? n : 0;
        a.v[4 * m + 3] += on ? ppm : 0;
    }
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {  // in every lane
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// the lanes' partial sums -> lane k < REGION_LANES returns quantity k's total plus its `whole`
__device__ __forceinline__ int64_t wave_lane_totals(const RegionAcc& a, int64_t whole) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < REGION_LANES; ++k) {
        const int64_t t = wave_sum(a.v[k]);
        if (lane == k) whole += t;
    }
    return whole;
}

// ... and of the workgroup: thread k < REGION_LANES returns quantity k's total over all its wavefronts (the others 0)
__device__ __forceinline__ int64_t block_lane_totals(const RegionAcc& a, int64_t whole) {
    __shared__ int64_t part[TPB / 64][REGION_LANES];
    const int64_t v = wave_lane_totals(a, whole);
    if ((threadIdx.x & 63) < REGION_LANES) part[threadIdx.x >> 6][threadIdx.x & 63] = v;
    __syncthreads();
    int64_t t = 0;
    for (int w = 0; threadIdx.x < REGION_LANES && w < TPB / 64; ++w) t += part[w][threadIdx.x];
    return t;
}

// idx[blockIdx.x * 12 + k] = quantity k summed over block blockIdx.x of [lo, hi)
__global__ __launch_bounds__(TPB) void region_block_sums_kernel(RangePlanes s, int64_t lo, int64_t hi, int64_t min_cov,
                                                                 int64_t* __restrict__ idx) {
    const int64_t base = lo + (int64_t)blockIdx.x * HM_REGION_BLOCK;
    RegionAcc a{};
#pragma unroll 4
    for (int k = 0; k < HM_REGION_BLOCK / TPB; ++k) {
        const int64_t i = base + k * TPB + threadIdx.x;
        if (i < hi) region_add(s, min_cov, i, a);
    }
    const int64_t t = block_lane_totals(a, 0);
    if (threadIdx.x < REGION_LANES) idx[(int64_t)blockIdx.x * REGION_LANES + threadIdx.x] = t;
}

// the block sums -> their inclusive scan, in place: an element is loaded and stored by the one thread that owns it
struct RegionScan {
    using T = RegionAcc;
    int64_t* idx;
    __host__ __device__ __forceinline__ static T identity() { return T{}; }
    __device__ __forceinline__ static T shfl_up(const T& v, int d) {
        T r;
#pragma unroll
        for (int k = 0; k < REGION_LANES; ++k) r.v[k] = __shfl_up(v.v[k], d);
        return r;
    }
    __device__ __forceinline__ static T op(const T& a, const T& b) {
        T r;
#pragma unroll
        for (int k = 0; k < REGION_LANES; ++k) r.v[k] = a.v[k] + b.v[k];
        return r;
    }
    __device__ __forceinline__ T load(int64_t j) const {
        T r;
#pragma unroll
        for (int k = 0; k < REGION_LANES; ++k) r.v[k] = idx[j * REGION_LANES + k];
        return r;
    }
    __device__ __forceinline__ void store(int64_t j, const T& f) const {
#pragma unroll
        for (int k = 0; k < REGION_LANES; ++k) idx[j * REGION_LANES + k] = f.v[k];
    }
};

struct RegionIndex {  // of the planes' range [lo, hi) under min_cov
    RangePlanes s;
    int64_t lo, hi, min_cov;
    const int64_t* idx;
};

// One wavefront adds the sums over [a, b), lo <= a <= b <= hi, both the same in all its lanes: the loci of block_split's head and
// tail into the lanes' partial sums, its whole blocks from the index into `whole` of lane k < 12
__device__ __forceinline__ void wave_range_add(const RegionIndex& ix, int64_t a, int64_t b, RegionAcc& acc, int64_t& whole) {
    const int lane = threadIdx.x & 63;
    const BlockSplit sp = block_split(ix.lo, a, b);
    for (int64_t i = a + lane; i < sp.head_end; i += 64) region_add(ix.s, ix.min_cov, i, acc);
    for (int64_t i = sp.tail_begin + lane; i < b; i += 64) region_add(ix.s, ix.min_cov, i, acc);
    if (lane < REGION_LANES && sp.row_last > sp.row_first) whole += ix.idx[sp.row_last * REGION_LANES + lane] - ix.idx[sp.row_first * REGION_LANES + lane];
}

__device__ __forceinline__ int64_t clamp_to(int64_t x, int64_t lo, int64_t hi) { return min(max(x, lo), hi); }

// out[i * 12 + k] = quantity k of interval i, clamped to the range: a wavefront per interval, over a grid stride
__global__ __launch_bounds__(TPB) void region_query_kernel(RegionIndex ix, int64_t plane_base, const int64_t* __restrict__ start,
                                                            const int64_t* __restrict__ end, int64_t n, int64_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * (TPB / 64)) {
        RegionAcc acc{};
        int64_t whole = 0;
        wave_range_add(ix, clamp_to(start[i] - plane_base, ix.lo, ix.hi), clamp_to(end[i] - plane_base, ix.lo, ix.hi), acc, whole);
        const int64_t v = wave_lane_totals(acc, whole);
        if (lane < REGION_LANES) out[i * REGION_LANES + lane] = v;
    }
}

struct MetaGeom {
    int32_t bins, flank_bins;
    int64_t flank;
    __host__ __device__ int n_bins() const { return bins + 2 * flank_bins; }
};
struct MetaIv {  // a used interval [s, e) on its sequence [S0, S1), global coordinates; 40 bytes
    int64_t s, e, S0, S1, neg;
};

// bin `out_bin` of an interval as the output numbers it (mirrored for the reverse strand) -> [a, b), clamped to the sequence
__host__ __device__ inline void metabin_range(const MetaGeom& m, const MetaIv& r, int out_bin, int64_t& a, int64_t& b) {
    const int g = r.neg ? m.n_bins() - 1 - out_bin : out_bin;  // in reference direction
    const int64_t w = m.flank_bins ? m.flank / m.flank_bins : 0;
    if (g < m.flank_bins) {
        a = r.s - m.flank + g * w;
        b = a + w;
    } else if (g < m.flank_bins + m.bins) {
        const int64_t j = g - m.flank_bins, len = r.e - r.s;
        a = r.s + j * len / m.bins;
        b = r.s + (j + 1) * len / m.bins;
    } else {
        a = r.e + (g - m.flank_bins - m.bins) * w;
        b = a + w;
    }
    a = a < r.S0 ? r.S0 : a > r.S1 ? r.S1 : a;
    b = b < r.S0 ? r.S0 : b > r.S1 ? r.S1 : b;
}

// tab[bin * 12 + k] += quantity k of bin blockIdx.x over the intervals: a wavefront keeps its partial sums over a stride of the
// intervals (blockIdx.y), then one reduction and at most twelve 64-bit atomics per workgroup.  Integers: exact in any order.
__global__ __launch_bounds__(TPB) void metaplot_kernel(RegionIndex ix, int64_t plane_base, MetaGeom m, const MetaIv* __restrict__ iv,
                                                        int64_t n, unsigned long long* __restrict__ tab) {
    RegionAcc acc{};
    int64_t whole = 0;
    for (int64_t i = (int64_t)blockIdx.y * (TPB / 64) + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.y * (TPB / 64)) {
        int64_t a, b;
        metabin_range(m, iv[i], (int)blockIdx.x, a, b);
        wave_range_add(ix, clamp_to(a - plane_base, ix.lo, ix.hi), clamp_to(b - plane_base, ix.lo, ix.hi), acc, whole);
    }
    const int64_t t = block_lane_totals(acc, whole);
    if (t) atomicAdd(&tab[(int64_t)blockIdx.x * REGION_LANES + threadIdx.x], (unsigned long long)t);
}

// ---- kernel-smoothed levels (`smooth`; include/hifimeth_hip.h has the definition) ------------------------------------------------
// The triangular kernel is a box convolved with a box, so the weighted sums of a window are differences of two running sums over
// the counting loci: the plain sum of v and its first moment, the sum of (j - origin) v, for v = pcov and ncov (and the plain count).
// The running sums RESTART every HM_SMOOTH_SPAN = 2 * 16384 positions of the span [a, b) the fetch reads, and a block's moments are
// measured from the block's first position: with counts below 2^31 a plain sum stays below 2^46 and a moment below 2^61, whatever the
// range, and one half of a window (at most 16384 positions) lies in at most two blocks.  One record of five sums per POSITION of the
// span (40 B), written by smooth_prefix_kernel, one workgroup per block; a row is then SmoothSel's handful of lookups, whatever h.
constexpr int SMOOTH_TPB = 256, SMOOTH_ITEMS = 4;  // threads of a workgroup (1024 spill: 128 registers do not hold a pass); consecutive positions per thread and pass
static_assert(HM_SMOOTH_SPAN >= 2 * HM_SMOOTH_MAX_HALF_WIDTH && HM_SMOOTH_SPAN % (SMOOTH_TPB * SMOOTH_ITEMS) == 0, "a half window lies in two blocks; a block is whole passes");

struct SmoothPre {  // over the counting loci from the block's first position to this one: their number, sum pcov, sum ncov, the two moments
    int64_t n, vp, vn, mp, mn;
};
__device__ __forceinline__ SmoothPre smooth_sum(const SmoothPre& x, const SmoothPre& y) {
    return SmoothPre{x.n + y.n, x.vp + y.vp, x.vn + y.vn, x.mp + y.mp, x.mn + y.mn};
}
__device__ __forceinline__ SmoothPre smooth_diff(const SmoothPre& x, const SmoothPre& y) {
    return SmoothPre{x.n - y.n, x.vp - y.vp, x.vn - y.vn, x.mp - y.mp, x.mn - y.mn};
}

// pre[i - a] for the positions i of block blockIdx.x of [a, b): per pass a thread sums its SMOOTH_ITEMS positions, the wavefronts scan
// those sums by shuffles, their totals meet in LDS (two buffers: one barrier per pass), and the block's running sum is carried on
__global__ __launch_bounds__(SMOOTH_TPB) void smooth_prefix_kernel(RangePlanes s, int64_t a, int64_t b, uint32_t ctx, int64_t min_cov,
                                                                    SmoothPre* __restrict__ pre) {
    __shared__ SmoothPre wtot[2][SMOOTH_TPB / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t base = a + (int64_t)blockIdx.x * HM_SMOOTH_SPAN;
    SmoothPre carry{0, 0, 0, 0, 0};
    for (int pass = 0; pass < HM_SMOOTH_SPAN / (SMOOTH_TPB * SMOOTH_ITEMS); ++pass) {
        const int64_t d0 = (int64_t)pass * (SMOOTH_TPB * SMOOTH_ITEMS) + (int64_t)threadIdx.x * SMOOTH_ITEMS;
        SmoothPre v[SMOOTH_ITEMS], run{0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < SMOOTH_ITEMS; ++k) {
            const int64_t d = d0 + k, i = base + d;
            if (i < b) {
                const int64_t p = s.pc[i], n = s.nc[i];
                if (p + n >= min_cov && (s.ky[i] & 3u) == ctx) run = smooth_sum(run, SmoothPre{1, p, n, d * p, d * n});
            }
            v[k] = run;
        }
        SmoothPre inc = run;  // the inclusive scan of `run` over the wavefront
        for (int d = 1; d < 64; d <<= 1) {
            const SmoothPre t{__shfl_up(inc.n, d), __shfl_up(inc.vp, d), __shfl_up(inc.vn, d), __shfl_up(inc.mp, d), __shfl_up(inc.mn, d)};
            if (lane >= d) inc = smooth_sum(inc, t);
        }
        if (lane == 63) wtot[pass & 1][w] = inc;
        __syncthreads();
        SmoothPre before = smooth_sum(carry, smooth_diff(inc, run));  // everything of the block in front of this thread's positions
        for (int j = 0; j < SMOOTH_TPB / 64; ++j) {
            const SmoothPre t = wtot[pass & 1][j];
            if (j < w) before = smooth_sum(before, t);
            carry = smooth_sum(carry, t);
        }
#pragma unroll
        for (int k = 0; k < SMOOTH_ITEMS; ++k) {
            const int64_t i = base + d0 + k;
            if (i < b) pre[i - a] = smooth_sum(before, v[k]);
        }
    }
}

// The rows of `smooth`: the counting loci of context ctx with at least min_loci counting loci in their window.  g is the plane index
// and the global position at once (the engine's own planes).  [a, b) is the span `pre` covers: every window of [lo, hi) lies in it.
struct SmoothSel {
    using Row = hm_smooth_t;
    RangePlanes s;
    const SmoothPre* pre;
    int64_t a;
    const int64_t* seq_off;  // n_seqs + 1
    int n_seqs;
    uint32_t ctx;
    int64_t h, min_cov, min_loci;
    // the counting loci j of [x, y], a <= x <= y < x + HM_SMOOTH_MAX_HALF_WIDTH, each with the weight c0 + sg j (sg = +-1), added to
    // (L, P, N).  In a block that starts at B the weight is (c0 + sg B) + sg (j - B): |c0 + sg B| < 2^16 for both halves of a window,
    // so the products stay below 2^62
    __device__ void add_part(int64_t x, int64_t y, int64_t c0, int64_t sg, int64_t& L, int64_t& P, int64_t& N) const {
        for (int64_t blk = (x - a) / HM_SMOOTH_SPAN; blk <= (y - a) / HM_SMOOTH_SPAN; ++blk) {  // one or two
            const int64_t B = a + blk * HM_SMOOTH_SPAN, first = max(x, B), last = min(y, B + HM_SMOOTH_SPAN - 1);
            SmoothPre t = pre[last - a];
            if (first > B) t = smooth_diff(t, pre[first - 1 - a]);
            const int64_t k = c0 + sg * B;
            L += t.n;
            P += k * t.vp + sg * t.mp;
            N += k * t.vn + sg * t.mn;
        }
    }
    __device__ bool counts(int64_t g, int32_t& p, int32_t& n) const {
        p = s.pc[g];
        n = s.nc[g];
        return (int64_t)p + n >= min_cov && (s.ky[g] & 3u) == ctx;
    }
    // the window of the counting locus g, cut at its sequence: [x, g] with the weights h - g + j, (g, y] with h + g - j
    __device__ void window(int64_t g, int64_t& L, int64_t& P, int64_t& N) const {
        int slo = 0, shi = n_seqs;  // seq_off[slo] <= g < seq_off[shi]
        while (shi - slo > 1) {
            const int mid = (slo + shi) >> 1;
            if (seq_off[mid] <= g) slo = mid; else shi = mid;
        }
        const int64_t x = max(seq_off[slo], g - h + 1), y = min(seq_off[shi] - 1, g + h - 1);
        L = P = N = 0;
        add_part(x, g, h - g, 1, L, P, N);
        if (y > g) add_part(g + 1, y, h + g, -1, L, P, N);
    }
    __device__ bool pred(int64_t g) const {
        int32_t p, n;
        if (!counts(g, p, n)) return false;
        if (min_loci <= 1) return true;
        int64_t L, P, N;
        window(g, L, P, N);
        return L >= min_loci;
    }
    __device__ bool take(int64_t g, Row& r) const {
        int32_t p, n;
        if (!counts(g, p, n)) return false;
        int64_t L, P, N;
        window(g, L, P, N);
        if (L < min_loci) return false;
        r = Row{g, p, n, L, P, N};
        return true;
    }
};

// ---- methylation by the k-mer around the cytosine (`pileup -S`; include/hifimeth_hip.h has the definition) ----------------------
// tab[((c * (K + 1) + row) * 4 + q]: context c, row = the k-mer's code or K for `other`, q = n_loci, pcov, ncov, ppm -- three
// tables of K + 1 hm_region_sum_t as one array of 64-bit counters.  The kernel streams pcov / ncov; only a locus with a count looks
// further: region_add decides whether it counts and what it adds, the reference decides the row.
constexpr int CX_THREADS = 1024;  // of a workgroup: the loci it takes side by side (HM_CONTEXT_SPAN)
constexpr int CX_UNROLL = 8;      // loci per thread whose counters are loaded before any of them is looked at
static_assert(CX_THREADS == HM_CONTEXT_SPAN, "the header names the workgroup's span");
__host__ __device__ constexpr int context_k(int f) { return 3 + 2 * f; }
__host__ __device__ constexpr int64_t context_rows(int f) { return (int64_t(1) << (2 * context_k(f))) + 1; }  // K + 1
__host__ __device__ constexpr int64_t context_counters(int f) { return 3 * context_rows(f) * 4; }
static_assert(context_counters(HM_CONTEXT_LDS_FLANK) * 8 <= 160 * 1024, "the workgroup-private table must fit the CU's LDS");

struct ContextRef {
    const char* ref;         // the concatenated reference
    const int64_t* seq_off;  // n_seqs + 1
    int n_seqs;
};

// the row of locus g: the code of the k bases around the called cytosine, read on the cytosine's strand, or K
template <int F>
__device__ __forceinline__ uint32_t context_row(const ContextRef& r, int64_t g) {
    constexpr int k = context_k(F);
    constexpr uint32_t other = 1u << (2 * k);
    const char c = r.ref[g];
    if (c != 'C' && c != 'G') return other;
    const bool fwd = c == 'C';
    const int64_t a = fwd ? g - F : g - 2 - F, b = a + k;
    // a lies in the sequence that ends at seq_end_of(a); the window is inside one sequence iff it ends there or before, and then
    // that sequence is g's
    if (a < 0 || b > seq_end_of(r.seq_off, r.n_seqs, a)) return other;
    uint32_t code = 0;
#pragma unroll
    for (int j = 0; j < k; ++j) {
        const char x = r.ref[fwd ? a + j : b - 1 - j];
        const uint32_t v = x == 'A' ? 0u : x == 'C' ? 1u : x == 'G' ? 2u : x == 'T' ? 3u : 4u;
        if (v > 3u) return other;
        code = (code << 2) | (fwd ? v : 3u - v);
    }
    return code;
}

// plane element i (locus plane_base + i), which has a count, into the table t (LDS or global)
template <int F>
__device__ __forceinline__ void context_locus(const RangePlanes& s, const ContextRef& r, int64_t plane_base, int64_t min_cov, int64_t i,
                                              unsigned long long* t) {
    RegionAcc a{};
    region_add(s, min_cov, i, a);
    if (!(a.v[0] | a.v[4] | a.v[8])) return;  // below min_cov, or a key of no context
    const uint32_t row = context_row<F>(r, plane_base + i);
#pragma unroll
    for (int m = 0; m < 3; ++m)
        if (a.v[4 * m]) {
            unsigned long long* q = t + ((int64_t)m * context_rows(F) + row) * 4;
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(q + k, (unsigned long long)a.v[4 * m + k]);
        }
}

// tab += the table of [lo, hi): a grid stride of CX_THREADS loci per workgroup, CX_UNROLL strides in flight.  LDS: the workgroup
// adds into a table of its own and ends with one global atomic per non-zero counter, as hist_flush; else every add is a global
// 64-bit atomic.  Integers: exact in any order.
template <int F, bool LDS>
__global__ __launch_bounds__(CX_THREADS) void context_kernel(RangePlanes s, ContextRef r, int64_t plane_base, int64_t lo, int64_t hi,
                                                              int64_t min_cov, unsigned long long* __restrict__ tab) {
    constexpr int N = LDS ? (int)context_counters(F) : 1;
    __shared__ unsigned long long h[N];
    unsigned long long* t = LDS ? h : tab;
    if constexpr (LDS) {
        for (int j = threadIdx.x; j < N; j += CX_THREADS) h[j] = 0ull;
        __syncthreads();
    }
    const int64_t stride = (int64_t)gridDim.x * CX_THREADS;
    for (int64_t i0 = lo + (int64_t)blockIdx.x * CX_THREADS + threadIdx.x; i0 < hi; i0 += stride * CX_UNROLL) {
        int32_t any[CX_UNROLL];
#pragma unroll
        for (int u = 0; u < CX_UNROLL; ++u) {
            const int64_t i = i0 + u * stride;
            any[u] = i < hi ? (s.pc[i] | s.nc[i]) : 0;
        }
#pragma unroll
        for (int u = 0; u < CX_UNROLL; ++u)
            if (any[u]) context_locus<F>(s, r, plane_base, min_cov, i0 + u * stride, t);
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int j = threadIdx.x; j < N; j += CX_THREADS)
            if (h[j]) atomicAdd(&tab[j], h[j]);
    }
}

}  // namespace

// ================================================ host ==========================================================
struct hm_pileup {
    static constexpr DevBuf::Room EXACT = DevBuf::EXACT, HALF = DevBuf::HALF;  // genome-sized, allocated once / grows with the batches
    int device = 0;
    Stream stream;  // declared before every buffer: destroyed after them
    std::string err;
    int min_mapq = 0;
    double min_pi = 0.0;

    // reference
    std::vector<int64_t> seq_off;  // n_seqs + 1
    DevBuf d_ref{EXACT};
    bool own_planes = true;
    DevBuf d_pcov{EXACT}, d_ncov{EXACT}, d_key{EXACT};
    int32_t* pcov = nullptr;
    int32_t* ncov = nullptr;
    uint32_t* key = nullptr;
    // haplotype partitions ("partitions" = 2): pcov / ncov planes of HP 1 and HP 2, +16 B per reference base
    int partitions = 0;
    DevBuf d_hp_pcov[2]{DevBuf(EXACT), DevBuf(EXACT)}, d_hp_ncov[2]{DevBuf(EXACT), DevBuf(EXACT)};
    int32_t* hp_pcov[2] = {nullptr, nullptr};
    int32_t* hp_ncov[2] = {nullptr, nullptr};

    // staged batch (host)
    std::vector<uint8_t> slab;
    std::vector<PRead> reads;
    std::vector<PRun> runs;
    std::vector<int64_t> col0;
    std::vector<PMod> mods;
    std::vector<PCall> calls;  // of the records submitted with calls; n_m_mods counts them too
    std::vector<PGap> gaps;    // `pileup -M`: the D operations of the staged records
    int64_t plane_len = 0, n_m_mods = 0;

    // device
    DevBuf d_slab{HALF}, d_reads{HALF}, d_runs{HALF}, d_col0{HALF}, d_mods{HALF}, d_calls{HALF}, d_plane{HALF}, d_matches{HALF}, d_bins{HALF}, d_counter{HALF}, d_recs{HALF};
    DevBuf d_blk{HALF}, d_offs{HALF}, d_rows{HALF}, d_labels{HALF}, d_lbins{HALF};  // d_rows: the rows of whichever fetch ran last
    DevBuf d_lfact{EXACT};  // log n! table, uploaded by the first hm_pileup_fetch_asm
    // `pileup -B / -e`, allocated by the first call that needs them: control sums, 3 x 256 x 256 bins, ptab + qtab, the big loci
    // (the histogram's list, or the caller's with p and q behind it: they stay while hm_pileup_fetch_sites writes d_rows)
    DevBuf d_ssums{EXACT}, d_sbins{EXACT}, d_stab{EXACT}, d_sbig{HALF}, d_sbigpq{HALF};
    // `pileup -H -A -Q`, allocated by the first call that needs them: HM_ASM_BINS bins (104 MB), hm_asm_t rows (the big loci, the
    // bins' pseudo-rows, the rows hm_pileup_fetch_asm_q adds q to), and the caller's table, big list and its q for that lookup
    DevBuf d_abins{EXACT}, d_arows{HALF}, d_atab{HALF}, d_abig{HALF}, d_abigq{HALF};
    // `pileup -D`, allocated by the first hm_pileup_fetch_domains: per row of the context DomRow, DomSum, code and state (34 B), the
    // workgroup aggregates of the scan that runs, and the segment heads
    DevBuf d_drows{HALF}, d_dsums{HALF}, d_dcode{HALF}, d_dstate{HALF}, d_dagg{HALF}, d_dheads{HALF};
    DevBuf d_dlast{EXACT};  // hm_pileup_fetch_domains_part: the d of a piece's last row, 8 B
    DevBuf d_dstate_sums{EXACT};  // hm_pileup_domain_sums, allocated by its first call: the six state sums, 48 B
    // `pileup -E` ("patterns" = k), all of it only with the option on: the sequence starts and the reference CpGs (8 B each) with
    // their 16 bins (64 B each), resident from hm_pileup_set_reference on; the window records, which grow with the batches as
    // d_recs does, and their counter; the two ranks that bound a fetch
    int patterns = 0, pattern_span = 150;
    DevBuf d_seqoff{EXACT}, d_cpg{EXACT}, d_phist{EXACT}, d_pcounter{EXACT}, d_pranks{EXACT}, d_precs{HALF};
    int64_t n_cpg = 0, n_precs = 0;
    // `pileup -M` ("bedmethyl" = 1), all of it only with the option on: d_seqoff, d_cpg and d_pranks above, shared with -E; five
    // uint32 depth counters per reference CpG and set (20 B, 60 B with partitions), resident from hm_pileup_set_reference on; the
    // staged D operations of a batch
    int bedmethyl = 0;
    DevBuf d_bm{EXACT}, d_gaps{HALF};
    // `pileup -L` ("linkage" = max_dist), all of it only with the option on: three 256-bin uint64 histograms per distance
    // (6 144 B each), resident from hm_pileup_set_reference on; the member list of the batch that runs; the four counts per
    // distance of a fetch
    int linkage = 0;
    DevBuf d_lhist{EXACT}, d_ltab{EXACT}, d_members{HALF};
    uint32_t linkage_thr = 0;  // thr[CpG] of the last hm_pileup_count
    // `pileup -P` ("profile" = D), all of it only with the option on: 3 x (2 D + 1) histogram rows of 256 uint64 (12.6 MB at
    // D = 1024, 25.2 MB at the cap), resident from hm_pileup_set_reference on; the three sums per row of a fetch; what
    // hm_pileup_add_readpos uploads.  `pileup -I` ("trim5", "trim3") travels with entries_kernel's arguments.
    int profile = 0;
    Trim trim{0, 0};
    DevBuf d_rphist{EXACT}, d_rptab{EXACT}, d_rpadd{EXACT};
    // the interval fetch in hand (`pileup -R / -J`, `regiondiff`), whichever ran last, allocated by the first: the index of its range
    // (per HM_REGION_BLOCK loci 96 B, or 16 M B for M samples), the caller's intervals, the sums per interval or the metaplot's table
    DevBuf d_ividx{EXACT}, d_iviv{HALF}, d_ivout{HALF};
    // `pileup -S`, allocated by the first hm_pileup_fetch_context: the table of the flank in hand (6 KB at flank 0, 25 MB at 3),
    // the sequence starts, and the device's CU count (0: not asked yet)
    DevBuf d_cxtab{EXACT}, d_cxoff{EXACT};
    // `smooth`, allocated by the first hm_smooth_fetch: the running sums of the span in hand, 40 B per position (the sequence
    // starts go through d_cxoff)
    DevBuf d_smooth{HALF};
    int n_cus = 0;
    // the loads of `diff`, `groupdiff` and `samplecorr` (load_rows), allocated by the first load: one slab of load_slab rows, whatever
    // a call brings, and the kernel's LOAD_COUNTERS counters.  The three flags are the engine's side of the rule "counts come from records or from
    // loads, never both": a record was ever staged; a load has gone through; a load met a bad row (the planes mean nothing now)
    DevBuf d_load{EXACT}, d_loadcnt{EXACT};
    bool staged_any = false, loaded = false, load_failed = false;
    int64_t load_slab = LOAD_SLAB_ROWS;  // option "load_slab": rows per slab of the next load
    // `groupdiff` ("groups" = 1), all of it only with the option on: per group the moment plane (8 B per base) and the sample-count
    // plane (1 B), and the open sample's seen bitmap (1 bit), resident from hm_pileup_set_reference on (d_gseen is the seen
    // bitmap of whichever loader the engine has: the first hm_pileup_load_loci makes it the two partitions' bitmaps, part k's at
    // word k * seen_words(p), 0.25 B per base, and no sample can be opened after that); the samples opened per
    // group, the group of the open one (0: none yet) and the table of 1 / (a B(a, 1/2)) by degrees of freedom for the fetch
    int groups = 0;
    int32_t group_min_cov = 5;
    DevBuf d_gmoment[2]{DevBuf(EXACT), DevBuf(EXACT)}, d_gsamples[2]{DevBuf(EXACT), DevBuf(EXACT)}, d_gseen{EXACT}, d_gcoef{EXACT};
    int group_samples[2] = {0, 0}, group_open = 0;
    DevBuf d_grows{HALF};  // hm_dmr_fetch_regions: the tested rows of one context (64 B each), allocated by its first call
    // `samplecorr` ("samples" = N), all of it only with the option on: N uint16 level planes of sample_stride values each (2 N B
    // per base), resident from hm_pileup_set_reference on; the samples opened so far (the last one is the open one); the table of
    // a fetch, 3 x N (N + 1) / 2 x 6 uint64
    int samples = 0, samples_open = 0;
    int32_t sample_min_cov = 5;
    int64_t sample_stride = 0;
    DevBuf d_slevel{EXACT}, d_stable{EXACT};
    uint32_t thr_packed = 0;   // the three thresholds of the last hm_pileup_count
    bool counted = false;    // hm_pileup_count has run since hm_pileup_set_reference: what the -E, -M and -L fetches wait for
    int64_t n_recs = 0;
    bool bins_ready = false;

    ~hm_pileup() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {

int pfail(hm_pileup* p, int code, const std::string& msg) {
    if (p) p->err = msg;
    else g_pileup_create_error = msg;
    return code;
}
int pfail_hip(hm_pileup* p, const HipErr& h) {
    return pfail(p, HM_EDEVICE, hip_error_text(h));
}

// every ABI entry point's device work: the engine's device current, a HipErr recorded as the engine's error -> HM_EDEVICE
template <class Body>
auto guarded(hm_pileup* p, Body&& body) -> decltype(body()) {
    return hip_guard(p->device, [p](const HipErr& h) { return pfail_hip(p, h); }, body);
}

// log n! for n < LFACT_N from the host's libm, filled once: what hm_pileup_fetch_asm uploads and hm_sites_table sums with
const std::vector<double>& host_lfact() {
    static const std::vector<double> tab = [] {
        std::vector<double> t((size_t)LFACT_N);
        for (int k = 0; k < LFACT_N; ++k) t[(size_t)k] = std::lgamma((double)k + 1.0);
        return t;
    }();
    return tab;
}

// words of one seen bitmap, 32 loci each: whole words, the load kernel ORs into the word that holds a locus' bit
inline size_t seen_words(const hm_pileup* p) { return ((size_t)std::max<int64_t>(p->seq_off.back(), 1) + 31) / 32; }

inline int grid_for(int64_t n, int cap = 1 << 20) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + TPB - 1) / TPB, cap)); }

// what every call over the engine's own planes answers once hm_pileup_load_loci has met a bad row
const char* const LOAD_FAILED_TEXT = "a load of this engine met bad rows (hm_pileup_load_loci): its planes mean nothing";

// the (pcov, ncov, key) arguments of a call over a plane range: each the caller's plane or, where NULL, the engine's own (with
// pcov NULL plane_base is 0); false (error recorded) if there are none
bool range_planes(hm_pileup* p, const void* pcov, const void* ncov, const void* key, int64_t& plane_base, RangePlanes& s) {
    s.pc = pcov ? static_cast<const int32_t*>(pcov) : p->pcov;
    s.nc = ncov ? static_cast<const int32_t*>(ncov) : p->ncov;
    s.ky = key ? static_cast<const uint32_t*>(key) : p->key;
    if (!pcov) plane_base = 0;
    if ((!pcov || !ncov || !key) && p->load_failed) {
        pfail(p, HM_ESTATE, LOAD_FAILED_TEXT);
        return false;
    }
    if (s.pc && s.nc && s.ky) return true;
    pfail(p, HM_ESTATE, "no planes");
    return false;
}

// ---- the host side of the selection skeleton ---------------------------------------------------------------------------------
inline dim3 row_grid(int64_t n) { return dim3((unsigned)((n + TPB - 1) / TPB)); }  // one thread per row
const auto no_hook = [](auto&&...) {};

// The rows of a selection over the non-empty [lo, hi), ascending, into `buf` on the device -> their number, or an error code;
// under the caller's guard.  launch_count(nblk, block_counts) counts them per LOCI_PER_BLOCK indices.  Once their number is known
// and not 0, want(total) says whether they are written at all and uploads what the write needs; after_write(rows, total) launches
// the per-row kernels that follow the write.  Nothing waits for the write.  `what` is done per sequence when the range is too large.
template <class Sel, class Count, class Want, class After>
int64_t stage_counted_rows(hm_pileup* p, const char* what, const Sel& sel, int64_t lo, int64_t hi, DevBuf& buf, Count launch_count,
                           Want want, After after_write) {
    using Row = typename Sel::Row;
    const int64_t nblk = (hi - lo + LOCI_PER_BLOCK - 1) / LOCI_PER_BLOCK;
    if (nblk >= (int64_t(1) << 31)) return pfail(p, HM_EINVAL, std::string("range too large: ") + what + " per sequence");
    p->d_blk.reserve(4 * (size_t)nblk);
    p->d_offs.reserve(8 * ((size_t)nblk + 1));
    int64_t* offs = p->d_offs.as<int64_t>();
    launch_count(nblk, p->d_blk.as<int32_t>());
    hipLaunchKernelGGL(loci_scan_kernel, dim3(1), dim3(1024), 0, p->stream, p->d_blk.as<int32_t>(), (int)nblk, offs);
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, offs + nblk, 8, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    if (!total || !want(total)) return total;
    buf.reserve(sizeof(Row) * (size_t)total);
    hipLaunchKernelGGL(select_write_kernel<Sel>, dim3((unsigned)nblk), dim3(TPB), 0, p->stream, sel, lo, hi, offs, buf.as<Row>());
    after_write(buf.as<Row>(), total);
    HIP_TRY(hipGetLastError());
    return total;
}

// ... counted by the selection itself
template <class Sel, class Want, class After>
int64_t stage_rows(hm_pileup* p, const Sel& sel, int64_t lo, int64_t hi, DevBuf& buf, Want want, After after_write) {
    return stage_counted_rows(
        p, "fetch", sel, lo, hi, buf,
        [&](int64_t nblk, int32_t* counts) {
            hipLaunchKernelGGL(select_count_kernel<Sel>, dim3((unsigned)nblk), dim3(TPB), 0, p->stream, sel, lo, hi, counts);
        },
        want, after_write);
}

// the cap rule of every fetch: more rows than cap, or no `out`: only counted
inline bool fits(int64_t total, const void* out, int64_t cap) { return total > 0 && total <= cap && out; }

// total staged rows of buf are in `out` when this returns; -> total
template <class Row>
int64_t rows_to_host(hm_pileup* p, const DevBuf& buf, Row* out, int64_t total) {
    HIP_TRY(hipMemcpyAsync(out, buf.p, sizeof(Row) * (size_t)total, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return total;
}

// The rows of a selection over the non-empty [lo, hi) -> their number, or an error code: staged in d_rows, then copied.
// room(total) names the host memory for the rows once their number is known, or NULL: only counted, nothing is written;
// before_write() uploads what the write needs; after_write as above.
template <class Sel, class Room, class Before, class After>
int64_t compact_rows_to(hm_pileup* p, const Sel& sel, int64_t lo, int64_t hi, Room room, Before before_write, After after_write) {
    return guarded(p, [&]() -> int64_t {
        typename Sel::Row* out = nullptr;
        const int64_t total = stage_rows(
            p, sel, lo, hi, p->d_rows,
            [&](int64_t n) {
                if (!(out = room(n))) return false;
                before_write();
                return true;
            },
            after_write);
        return total > 0 && out ? rows_to_host(p, p->d_rows, out, total) : total;
    });
}

// ... into the caller's out[cap]
template <class Sel, class Before, class After>
int64_t compact_rows(hm_pileup* p, const Sel& sel, int64_t lo, int64_t hi, typename Sel::Row* out, int64_t cap, Before before_write,
                     After after_write) {
    return compact_rows_to(p, sel, lo, hi, [&](int64_t total) { return total > cap ? nullptr : out; }, before_write, after_write);
}

// log n!, n < LFACT_N, for asm_test_kernel: uploaded once per engine
void ensure_lfact(hm_pileup* p) {
    if (p->d_lfact.p) return;
    const std::vector<double>& t = host_lfact();
    p->d_lfact.reserve(sizeof(double) * t.size());
    HIP_TRY(hipMemcpyAsync(p->d_lfact.p, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
}

// diff and pvalue of n compact rows
void test_rows(hm_pileup* p, hm_asm_t* rows, int64_t n) {
    hipLaunchKernelGGL(asm_test_kernel, row_grid(n), dim3(TPB), 0, p->stream, rows, n, p->d_lfact.as<double>());
}

// The arguments every call over the haplotype planes shares, by hm_pileup_fetch_asm's rules: the caller's five planes or, where all
// are NULL, the engine's own partition and key planes (plane_base is then 0).  HM_OK, or the error recorded in the name of `who`.
int asm_planes(hm_pileup* p, const char* who, const void* pcov1, const void* ncov1, const void* pcov2, const void* ncov2,
               const void* key, int64_t& plane_base, int64_t lo, int64_t hi, int32_t min_cov, AsmPlanes& s) {
    const std::string w = who;
    if (min_cov < 1) return pfail(p, HM_EINVAL, w + ": min_cov must be >= 1");
    if (lo < 0 || hi < lo) return pfail(p, HM_EINVAL, w + ": bad range");
    const int given = (pcov1 != nullptr) + (ncov1 != nullptr) + (pcov2 != nullptr) + (ncov2 != nullptr) + (key != nullptr);
    if (given != 0 && given != 5) return pfail(p, HM_EINVAL, w + ": give all five planes or none");
    s = AsmPlanes{static_cast<const int32_t*>(pcov1), static_cast<const int32_t*>(ncov1), static_cast<const int32_t*>(pcov2),
                  static_cast<const int32_t*>(ncov2), static_cast<const uint32_t*>(key)};
    if (given) return HM_OK;
    if (p->partitions != 2 || !p->hp_pcov[0] || !p->hp_pcov[1] || !p->key)
        return pfail(p, HM_ESTATE, w + " without partition planes (option partitions = 2, then hm_pileup_set_reference)");
    if (p->load_failed) return pfail(p, HM_ESTATE, w + ": " + LOAD_FAILED_TEXT);
    if (!p->seq_off.empty() && hi > p->seq_off.back()) return pfail(p, HM_EINVAL, w + ": range past the reference");
    s = AsmPlanes{p->hp_pcov[0], p->hp_ncov[0], p->hp_pcov[1], p->hp_ncov[1], p->key};
    plane_base = 0;
    return HM_OK;
}

// The non-empty bins of d_abins in ascending index, in one count and one write pass -> their number, or an error code
// (compact_rows_to's rule for room).  with_p: each entry's pvalue is what asm_test_kernel gives a row carrying the bin's tuple;
// else it is 0.
template <class Room>
int64_t nonempty_bins(hm_pileup* p, Room room, bool with_p) {
    return compact_rows_to(
        p, BinsSel{p->d_abins.as<unsigned long long>()}, 0, HM_ASM_BINS, room, [&] { if (with_p) ensure_lfact(p); },
        [&](hm_asm_bin_t* tab, int64_t total) {
            if (!with_p) return;
            p->d_arows.reserve(sizeof(hm_asm_t) * (size_t)total);
            hm_asm_t* rows = p->d_arows.as<hm_asm_t>();
            hipLaunchKernelGGL(asm_bin_rows_kernel, row_grid(total), dim3(TPB), 0, p->stream, tab, total, rows);
            test_rows(p, rows, total);
            hipLaunchKernelGGL(asm_bin_p_kernel, row_grid(total), dim3(TPB), 0, p->stream, rows, total, tab);
        });
}

// Benjamini-Hochberg over entries that each stand for `loci` loci sharing one p (R's p.adjust(method = "BH") among m loci): over
// the distinct p in ascending order R = the loci with p <= it, then from the largest p down q = the running minimum of
// min(1, p * (double)m / (double)R); store(where, q) takes the q of every entry.
struct BhEntry {
    double p;
    uint64_t loci;
    int64_t where;
};
template <class Store>
void bh_qvalues(std::vector<BhEntry>& ent, uint64_t m, Store store) {
    std::sort(ent.begin(), ent.end(), [](const BhEntry& a, const BhEntry& b) { return a.p < b.p; });
    std::vector<uint64_t> R(ent.size());
    uint64_t seen = 0;
    for (size_t a = 0; a < ent.size();) {
        size_t b = a;
        while (b < ent.size() && ent[b].p == ent[a].p) seen += ent[b++].loci;
        for (; a < b; ++a) R[a] = seen;
    }
    double q = 1.0;
    for (size_t a = ent.size(); a-- > 0;) {
        q = std::min(q, std::min(1.0, ent[a].p * (double)m / (double)R[a]));
        store(ent[a].where, q);
    }
}

void ensure_bins(hm_pileup* p) {
    if (p->bins_ready) return;
    p->d_bins.reserve(768 * sizeof(unsigned long long));
    p->d_counter.reserve(sizeof(unsigned long long));
    HIP_TRY(hipMemsetAsync(p->d_bins.p, 0, 768 * sizeof(unsigned long long), p->stream));
    HIP_TRY(hipMemsetAsync(p->d_counter.p, 0, sizeof(unsigned long long), p->stream));
    p->bins_ready = true;
}

// the uploaded batch of n_runs runs over `cols` columns
BatchView batch_view(const hm_pileup* p, int n_runs, int64_t cols) {
    return BatchView{p->d_runs.as<PRun>(), p->d_col0.as<int64_t>(), n_runs, cols, p->d_reads.as<PRead>(), p->d_slab.as<uint8_t>(),
                     p->d_ref.as<char>(), p->d_plane.as<uint32_t>(), p->d_matches.as<int32_t>(), p->min_pi};
}

PatRule pattern_rule(const hm_pileup* p) {
    return PatRule{p->d_cpg.as<int64_t>(), p->n_cpg, p->d_seqoff.as<int64_t>(), (int)p->seq_off.size() - 1, p->patterns, p->pattern_span};
}

// ranks[0], ranks[1] = the first reference CpG at or behind lo, hi: the reference CpGs of [lo, hi) are the ranks [ranks[0], ranks[1])
int cpg_rank_range(hm_pileup* p, int64_t lo, int64_t hi, int64_t ranks[2]) {
    return guarded(p, [&] {
        hipLaunchKernelGGL(pattern_ranks_kernel, dim3(1), dim3(64), 0, p->stream, p->d_cpg.as<int64_t>(), p->n_cpg, lo, hi, p->d_pranks.as<int64_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(ranks, p->d_pranks.p, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
}

BmCounters depth_counters(const hm_pileup* p, int set = 0) {
    return BmCounters{p->d_cpg.as<int64_t>(), p->n_cpg, p->d_bm.as<uint32_t>() + (size_t)set * (size_t)p->n_cpg * BM_CLASSES};
}

// `pileup -E` and `pileup -M`, under hm_pileup_set_reference's guard once the bases are on their way: the sequence starts, the
// reference CpGs of the whole reference through the selection skeleton (they stay on the device); then what each option keeps per
// reference CpG, zeroed: -E's bins and record counter, -M's depth counters
int list_reference_cpgs(hm_pileup* p) {
    const int n_seqs = (int)p->seq_off.size() - 1;
    const int64_t total = p->seq_off.back();
    p->d_seqoff.reserve(8 * p->seq_off.size());
    HIP_TRY(hipMemcpyAsync(p->d_seqoff.p, p->seq_off.data(), 8 * p->seq_off.size(), hipMemcpyHostToDevice, p->stream));
    p->d_pranks.reserve(16);
    if (p->patterns) {
        p->d_pcounter.reserve(sizeof(unsigned long long));
        HIP_TRY(hipMemsetAsync(p->d_pcounter.p, 0, sizeof(unsigned long long), p->stream));
    }
    p->n_cpg = p->n_precs = 0;
    if (total >= 2) {
        const int64_t n = stage_rows(p, RefCpgSel{p->d_ref.as<char>(), p->d_seqoff.as<int64_t>(), n_seqs, total}, 0, total, p->d_cpg,
                                     [](int64_t) { return true; }, no_hook);
        if (n < 0) return (int)n;
        if (n >= (int64_t(1) << 32)) return pfail(p, HM_EINVAL, std::string(p->patterns ? "patterns" : "bedmethyl") + ": 2^32 reference CpGs or more");
        p->n_cpg = n;
    }
    if (p->patterns) {
        p->d_phist.reserve(64 * (size_t)std::max<int64_t>(p->n_cpg, 1));
        HIP_TRY(hipMemsetAsync(p->d_phist.p, 0, 64 * (size_t)std::max<int64_t>(p->n_cpg, 1), p->stream));
    }
    if (p->bedmethyl) {
        const size_t bytes = sizeof(uint32_t) * BM_CLASSES * (p->partitions == 2 ? 3 : 1) * (size_t)std::max<int64_t>(p->n_cpg, 1);
        p->d_bm.reserve(bytes);
        HIP_TRY(hipMemsetAsync(p->d_bm.p, 0, bytes, p->stream));
    }
    return HM_OK;
}

// `pileup -L`, under hm_pileup_run's guard behind the projection: the batch's member list through the selection skeleton (it
// lives until the next batch), then every pair of it into the histograms.  <= 1024 workgroups: an entry is a loop over its pairs.
int count_linkage_pairs(hm_pileup* p, const BatchView& batch) {
    const int64_t n = stage_rows(p, MemberSel{batch}, 0, batch.n_cols, p->d_members, [](int64_t) { return true; }, no_hook);
    if (n < 0) return (int)n;
    if (n > 1)
        hipLaunchKernelGGL(linkage_pair_kernel, dim3(grid_for(n, 1024)), dim3(TPB), 0, p->stream, p->d_members.as<PMember>(), n, p->linkage,
                           p->d_lhist.as<unsigned long long>());
    return HM_OK;
}

// the read-position table as the kernels see it, and its number of uint64 counters
ReadPos readpos_table(const hm_pileup* p) { return ReadPos{p->d_rphist.as<unsigned long long>(), p->profile}; }
size_t readpos_counters(const hm_pileup* p) { return (size_t)3 * (2 * (size_t)p->profile + 1) * 256; }

void clear_batch(hm_pileup* p) {
    p->slab.clear();
    p->reads.clear();
    p->runs.clear();
    p->col0.clear();
    p->mods.clear();
    p->calls.clear();
    p->gaps.clear();
    p->plane_len = 0;
    p->n_m_mods = 0;
}

// The record-level part of a submission, shared by the MM/ML and the calls form: every argument check, the CIGAR turned into
// match runs (appended to p->runs from `mark` on; with `pileup -M` its D operations to p->gaps as well) and the PRead `r`, which
// the caller pushes once the record's `n_entries` entries (mods or calls, at `entries`) are staged as well.  Returns 1 to go on,
// else the submission's return value.
struct BatchMark {  // where a record's runs and gap records begin: what an error rolls back to
    size_t runs, gaps;
};
void roll_back(hm_pileup* p, const BatchMark& m) {
    p->runs.resize(m.runs);
    p->gaps.resize(m.gaps);
}

int stage_alignment(hm_pileup* p, uint32_t order, int32_t flag, int32_t sid, int64_t pos, int32_t mapq, int32_t l_qseq,
                    const uint8_t* seq4, int32_t n_cigar, const uint32_t* cigar, int64_t n_entries, const void* entries, int32_t hp,
                    PRead& r, BatchMark& mark) {
    if (!p) return HM_EINVAL;
    if (p->loaded || p->load_failed || p->group_open || p->samples_open)
        return pfail(p, HM_ESTATE, "hm_pileup_submit_read on an engine whose counts were loaded (hm_pileup_load_loci, hm_pileup_group_sample, hm_sample_open)");
    if (hp < 0 || hp > 2) return pfail(p, HM_EINVAL, "haplotype partition must be 0, 1 or 2");
    if (hp && p->partitions != 2) return pfail(p, HM_ESTATE, "haplotype partition given but the partitions option is off");
    if (p->seq_off.empty()) return pfail(p, HM_ESTATE, "hm_pileup_submit_read before hm_pileup_set_reference");
    if (n_entries <= 0 || (flag & 4)) return 0;  // pileup.cpp:233-235
    if (n_entries >= (int64_t(1) << 22)) return pfail(p, HM_EINVAL, "more than 2^22 modification entries in one read");
    if (l_qseq < 0 || !seq4 || n_cigar < 0 || (n_cigar && !cigar) || !entries) return pfail(p, HM_EINVAL, "hm_pileup_submit_read: bad argument");
    // key = order << 2 | motif must stay below 2^31: the multi-GPU path max-reduces the key plane as int32
    // (hifimeth_amd/pileup.py: reduce_scatter_planes), where a set top bit would lose against an empty locus
    if (order >= (1u << 29)) return pfail(p, HM_EINVAL, "record order must be < 2^29");
    if (l_qseq >= (1 << 22)) return pfail(p, HM_EINVAL, "reads of 2^22 bases or more are not supported");
    const int n_seqs = (int)p->seq_off.size() - 1;
    if (sid < 0 || sid >= n_seqs) return pfail(p, HM_EINVAL, "sequence index out of range");
    const int64_t ssize = p->seq_off[sid + 1] - p->seq_off[sid];
    if (pos < 0 || pos > ssize) return pfail(p, HM_EDATA, "alignment position outside the reference sequence");
    {   // s_decode_bam_query_base accepts the nibbles 1, 2, 4, 8, 15 only (bam_info.cpp:100-121); two per byte
        static const auto ok = [] {
            std::array<uint8_t, 256> t{};
            auto good = [](int c) { return c == 1 || c == 2 || c == 4 || c == 8 || c == 15; };
            for (int b = 0; b < 256; ++b) t[(size_t)b] = good(b >> 4) && good(b & 15);
            return t;
        }();
        const int full = l_qseq >> 1;
        int bad = -1;
        for (int i = 0; i < full; ++i)
            if (!ok[seq4[i]]) { bad = i; break; }
        if (bad < 0 && (l_qseq & 1) && !ok[(seq4[full] & 0xf0) | 1]) bad = full;
        if (bad >= 0) {
            const int hi = seq4[bad] >> 4, lo = seq4[bad] & 15;
            const bool hi_bad = !(hi == 1 || hi == 2 || hi == 4 || hi == 8 || hi == 15);
            return pfail(p, HM_EDATA, "Illegal BAM base encoded value " + std::to_string(hi_bad ? hi : lo));
        }
    }
    // cigar_to_alignment (bam_info.cpp:262-371) without the strings: match runs + column count
    mark = BatchMark{p->runs.size(), p->gaps.size()};
    int opi = 0;
    int64_t qi = -1, si = -1;
    if (n_cigar > 0) {
        const int op0 = cigar[0] & 15;
        if (op0 == 4) { qi = (int64_t)(cigar[0] >> 4) - 1; opi = 1; }
        else if (op0 == 5) opi = 1;
    }
    int64_t as_size = 0;
    bool open = false;  // the previous column-producing op was a match-type op
    for (; opi < n_cigar; ++opi) {
        const int op = cigar[opi] & 15;
        const int64_t num = cigar[opi] >> 4;
        if (op == 0 || op == 7 || op == 8) {  // M = X
            if (num == 0) continue;
            if (open) p->runs.back().len += (int32_t)num;
            else p->runs.push_back(PRun{p->seq_off[sid] + pos + si + 1, (int32_t)p->reads.size(), (int32_t)(qi + 1), (int32_t)num, 0});
            open = true;
            qi += num; si += num; as_size += num;
        } else if (op == 1) {  // I
            qi += num; as_size += num;
            if (num) open = false;
        } else if (op == 2 || op == 3) {  // D N
            if (p->bedmethyl && op == 2 && num) p->gaps.push_back(PGap{p->seq_off[sid] + pos + si + 1, (int32_t)num, (int32_t)p->reads.size()});
            si += num; as_size += num;
            if (num) open = false;
        } else if (op == 4 || op == 5 || op == 6) {  // S H P: no columns
        } else {
            roll_back(p, mark);
            return pfail(p, HM_EDATA, "Unrecognised CIGAR operation");
        }
        if (qi >= l_qseq || pos + si >= ssize) {
            roll_back(p, mark);
            return pfail(p, HM_EDATA, qi >= l_qseq ? "CIGAR consumes more bases than SEQ holds"
                                                    : "alignment runs past the end of the reference sequence");
        }
    }
    if (as_size >= (int64_t(1) << 31)) { roll_back(p, mark); return pfail(p, HM_EINVAL, "alignment too long"); }
    r = PRead{};
    r.seq4_off = (int64_t)p->slab.size();
    r.plane_off = p->plane_len;
    r.l_qseq = l_qseq;
    r.order = order;
    r.as_size = (int32_t)as_size;
    r.rev = (flag & 16) ? 1 : 0;
    r.primary = (flag & 0x900) ? 0 : 1;
    r.pass = mapq >= p->min_mapq ? 1 : 0;
    r.hp = (uint8_t)hp;
    return 1;
}

// the record joins the staged batch (after its entries)
void commit_read(hm_pileup* p, const PRead& r, const uint8_t* seq4) {
    p->slab.insert(p->slab.end(), seq4, seq4 + (r.l_qseq + 1) / 2);
    p->plane_len += r.l_qseq;
    p->reads.push_back(r);
    p->staged_any = true;
}

// ---- `diff`, `groupdiff`, `samplecorr`: what their calls share ----------------------------------------------------------------------
// The rows of one load through load_rows_kernel<Sink>, slab by slab: the copy of a slab follows the kernel over the one before it
// in the stream.  -> the number of rows that added, or HM_EDATA with the bad rows by kind behind `who` (a duplicate in the words
// of dup_text) on an engine that is void from then on.
template <class Sink>
int64_t load_rows(hm_pileup* p, const char* who, const hm_locus_t* rows, int64_t n, const Sink& sink, const char* dup_text) {
    if (n == 0) return 0;
    const int64_t slab = p->load_slab;
    unsigned long long c[LOAD_COUNTERS] = {0, 0, 0, 0, 0, 0};
    const int rc = guarded(p, [&] {
        p->d_load.reserve(sizeof(hm_locus_t) * (size_t)slab);
        p->d_loadcnt.reserve(sizeof c);
        HIP_TRY(hipMemsetAsync(p->d_loadcnt.p, 0, sizeof c, p->stream));
        for (int64_t at = 0; at < n; at += slab) {
            const int64_t m = std::min(slab, n - at);
            HIP_TRY(hipMemcpyAsync(p->d_load.p, rows + at, sizeof(hm_locus_t) * (size_t)m, hipMemcpyHostToDevice, p->stream));
            hipLaunchKernelGGL(load_rows_kernel<Sink>, dim3(grid_for(m, 4096)), dim3(TPB), 0, p->stream, p->d_load.as<hm_locus_t>(), m,
                               p->seq_off.back(), sink, p->d_loadcnt.as<unsigned long long>());
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(c, p->d_loadcnt.p, sizeof c, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
    if (rc < 0) return rc;
    unsigned long long bad = 0;
    for (int k = LOAD_BAD_GPOS; k < LOAD_COUNTERS; ++k) bad += c[k];
    if (!bad) return (int64_t)c[LOAD_ADDED];
    p->load_failed = true;
    const char* const kind[LOAD_COUNTERS] = {"", "gpos outside the reference", "negative count", "count above 2^20 - 1", "motif above 3", dup_text};
    std::string msg = std::string(who) + ": " + std::to_string(bad) + " bad rows";
    const char* sep = ": ";
    for (int k = LOAD_BAD_GPOS; k < LOAD_COUNTERS; ++k) {
        if (!c[k]) continue;
        msg += sep + std::to_string(c[k]) + " " + kind[k];
        sep = ", ";
    }
    return pfail(p, HM_EDATA, msg);
}

// What the group and the sample calls share: the option on with the reference set (which allocates what the option keeps
// resident), an engine that is not void, the planes the rows go to; each with the words that follow the caller's name.
struct OptionNeeds {
    bool resident, planes;
    const char *needs, *without;
};
OptionNeeds group_needs(const hm_pileup* p) {
    return {p->groups && p->d_gseen.p, p->pcov && p->hp_pcov[0] && p->hp_pcov[1], " needs option groups = 1 and hm_pileup_set_reference",
            " without partition planes"};
}
OptionNeeds sample_needs(const hm_pileup* p) {
    return {p->samples && p->d_slevel.p, p->pcov && p->ncov && p->key, " needs option samples = N and hm_pileup_set_reference", " without planes"};
}
int option_ready(hm_pileup* p, const char* who, const OptionNeeds& o) {
    const std::string w = who;
    if (!o.resident || p->seq_off.empty()) return pfail(p, HM_ESTATE, w + o.needs);
    if (p->load_failed) return pfail(p, HM_ESTATE, w + ": " + LOAD_FAILED_TEXT);
    if (!o.planes) return pfail(p, HM_ESTATE, w + o.without);
    return HM_OK;
}
int option_range(hm_pileup* p, const char* who, const OptionNeeds& o, int64_t lo, int64_t hi) {
    const int rc = option_ready(p, who, o);
    if (rc != HM_OK) return rc;
    if (lo < 0 || hi < lo || hi > p->seq_off.back()) return pfail(p, HM_EINVAL, std::string(who) + ": bad range");
    return HM_OK;
}

// What a job leaves on an engine beside its options and the caller's planes, dropped when hm_pileup_set_reference has accepted its
// arguments: the staged batch; the resident records and pattern windows (their device counters are zeroed with the histograms and
// in list_reference_cpgs); the 768 bins, which the next ensure_bins zeroes; the thresholds of the last count; the three flags of
// "counts come from one source", and with `loaded` the seen bits, since the first load of an engine that has not loaded clears
// both bitmaps; the opened samples; the error text.  The tables that hm_pileup_set_reference sizes are zeroed there.
void drop_job(hm_pileup* p) {
    clear_batch(p);
    p->n_recs = p->n_precs = 0;
    p->bins_ready = false;
    p->counted = false;
    p->thr_packed = p->linkage_thr = 0;
    p->staged_any = p->loaded = p->load_failed = false;
    p->group_samples[0] = p->group_samples[1] = p->group_open = 0;
    p->samples_open = 0;
    p->err.clear();
}

}  // namespace

extern "C" {

int hm_pileup_create(hm_pileup_t** out, int device) {
    if (!out) return pfail(nullptr, HM_EINVAL, "hm_pileup_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return pfail(nullptr, HM_EDEVICE, "no HIP device: the pileup kernels need a gfx950 GPU (there is no CPU fallback)");
    if (device < 0 || device >= n) return pfail(nullptr, HM_EINVAL, "device ordinal out of range");
    std::unique_ptr<hm_pileup> p(new hm_pileup);
    p->device = device;
    const int rc = hip_guard(device, [](const HipErr& h) { return pfail_hip(nullptr, h); }, [&] {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        if (!strstr(prop.gcnArchName, "gfx950"))
            return pfail(nullptr, HM_EDEVICE, "device is " + std::string(prop.gcnArchName) + ", this library holds gfx950 code only");
        HIP_TRY(hipStreamCreateWithFlags(&p->stream.h, hipStreamNonBlocking));
        return HM_OK;
    });
    if (rc < 0) return rc;
    *out = p.release();
    return HM_OK;
}

void hm_pileup_destroy(hm_pileup_t* p) { delete p; }  // ~hm_pileup: device current, stream drained, then the members

const char* hm_pileup_last_error(const hm_pileup_t* p) { return p ? p->err.c_str() : g_pileup_create_error.c_str(); }

int hm_pileup_set_option(hm_pileup_t* p, const char* key, double value) {
    if (!p || !key) return HM_EINVAL;
    const std::string k = key;
    // what is sized or listed when the reference arrives (the partition planes, the reference CpGs and their counters, the
    // linkage histograms) is decided before that; the planes also before the caller hands in planes of their own
    const bool partitions = k == "partitions";
    if (partitions || k == "groups" || k == "samples" || k == "patterns" || k == "pattern_span" || k == "bedmethyl" || k == "linkage" || k == "profile" || k == "trim5" || k == "trim3") {
        if (!p->seq_off.empty() || (partitions && !p->own_planes))
            return pfail(p, HM_ESTATE, k + " must be set before hm_pileup_set_reference" + (partitions ? " / hm_pileup_use_planes" : ""));
    }
    if (k == "min_mapq") p->min_mapq = (int)value;
    else if (k == "min_pi") p->min_pi = value;
    else if (partitions) {
        if (value != 0.0 && value != 2.0) return pfail(p, HM_EINVAL, "partitions must be 0 or 2");
        if (value == 0.0 && p->groups) return pfail(p, HM_ESTATE, "partitions cannot be switched off under option groups");
        p->partitions = (int)value;
    } else if (k == "patterns") {
        if (value != 0.0 && value != 2.0 && value != 3.0 && value != 4.0) return pfail(p, HM_EINVAL, "patterns must be 0, 2, 3 or 4");
        p->patterns = (int)value;
    } else if (k == "pattern_span") {
        if (!(value >= 1.0 && value <= (double)PAT_MAX_SPAN) || value != std::floor(value))
            return pfail(p, HM_EINVAL, "pattern_span must be an integer in 1 .. 65536");
        p->pattern_span = (int)value;
    } else if (k == "bedmethyl") {
        if (value != 0.0 && value != 1.0) return pfail(p, HM_EINVAL, "bedmethyl must be 0 or 1");
        p->bedmethyl = (int)value;
    } else if (k == "linkage") {
        if (value != 0.0 && (!(value >= 2.0 && value <= (double)LINK_MAX_DIST) || value != std::floor(value)))
            return pfail(p, HM_EINVAL, "linkage must be 0 or an integer in 2 .. 16384");
        p->linkage = (int)value;
    } else if (k == "profile") {  // the read-position table is sized when the reference arrives
        if (value != 0.0 && (!(value >= 1.0 && value <= (double)READPOS_MAX) || value != std::floor(value)))
            return pfail(p, HM_EINVAL, "profile must be 0 or an integer in 1 .. 2048");
        p->profile = (int)value;
    } else if (k == "trim5" || k == "trim3") {  // reads are shorter than 2^22 bases: a larger value drops no more
        if (!(value >= 0.0 && value <= (double)INT32_MAX) || value != std::floor(value))
            return pfail(p, HM_EINVAL, k + " must be an integer >= 0");
        (k == "trim5" ? p->trim.n5 : p->trim.n3) = (int32_t)std::min(value, (double)(1 << 22));
    } else if (k == "groups") {  // the moment and sample-count planes are sized when the reference arrives
        if (value != 0.0 && value != 1.0) return pfail(p, HM_EINVAL, "groups must be 0 or 1");
        if (value == 1.0 && p->partitions != 2) return pfail(p, HM_ESTATE, "groups needs option partitions = 2 set before it");
        p->groups = (int)value;
    } else if (k == "group_min_cov") {
        if (!(value >= 1.0 && value < (double)GROUP_COUNT_LIMIT) || value != std::floor(value))
            return pfail(p, HM_EINVAL, "group_min_cov must be an integer in 1 .. 2^20 - 1");
        if (p->group_open) return pfail(p, HM_ESTATE, "group_min_cov must be set before the first hm_pileup_group_sample");
        p->group_min_cov = (int32_t)value;
    } else if (k == "samples") {  // the level planes are sized when the reference arrives
        if (value != 0.0 && (!(value >= 2.0 && value <= (double)SAMPLE_MAX) || value != std::floor(value)))
            return pfail(p, HM_EINVAL, "samples must be 0 or an integer in 2 .. 64");
        p->samples = (int)value;
    } else if (k == "sample_min_cov") {
        if (!(value >= 1.0 && value < (double)GROUP_COUNT_LIMIT) || value != std::floor(value))
            return pfail(p, HM_EINVAL, "sample_min_cov must be an integer in 1 .. 2^20 - 1");
        if (p->samples_open) return pfail(p, HM_ESTATE, "sample_min_cov must be set before the first hm_sample_open");
        p->sample_min_cov = (int32_t)value;
    } else if (k == "load_slab") {  // the device holds one slab of rows whatever a load brings; at any time
        if (!(value >= 1.0 && value <= (double)LOAD_SLAB_MAX) || value != std::floor(value))
            return pfail(p, HM_EINVAL, "load_slab must be an integer in 1 .. 2^24");
        p->load_slab = (int64_t)value;
    } else return pfail(p, HM_EINVAL, "unknown option " + k);
    return HM_OK;
}

int hm_pileup_use_planes(hm_pileup_t* p, void* pcov, void* ncov, void* key) {
    if (!p || !pcov || !ncov || !key) return HM_EINVAL;
    p->own_planes = false;
    p->pcov = static_cast<int32_t*>(pcov);
    p->ncov = static_cast<int32_t*>(ncov);
    p->key = static_cast<uint32_t*>(key);
    return HM_OK;
}

int hm_pileup_use_partition_planes(hm_pileup_t* p, int32_t part, void* pcov, void* ncov) {
    if (!p || !pcov || !ncov || (part != 1 && part != 2)) return pfail(p, HM_EINVAL, "hm_pileup_use_partition_planes: bad argument");
    if (p->partitions != 2) return pfail(p, HM_ESTATE, "hm_pileup_use_partition_planes without the partitions option");
    p->hp_pcov[part - 1] = static_cast<int32_t*>(pcov);
    p->hp_ncov[part - 1] = static_cast<int32_t*>(ncov);
    if (!p->loaded || p->d_gseen.cap < 2 * 4 * seen_words(p)) return HM_OK;  // no seen bitmaps yet: the next load clears both
    return guarded(p, [&] {        // other planes: no row has been given to them
        HIP_TRY(hipMemsetAsync(p->d_gseen.as<uint32_t>() + (size_t)(part - 1) * seen_words(p), 0, 4 * seen_words(p), p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
}

int hm_pileup_partition_planes(hm_pileup_t* p, int32_t part, void** pcov, void** ncov) {
    if (!p || (part != 1 && part != 2)) return pfail(p, HM_EINVAL, "hm_pileup_partition_planes: part must be 1 or 2");
    if (p->partitions != 2 || !p->hp_pcov[part - 1])
        return pfail(p, HM_ESTATE, "no partition planes (partitions option off, or before hm_pileup_set_reference)");
    if (pcov) *pcov = p->hp_pcov[part - 1];
    if (ncov) *ncov = p->hp_ncov[part - 1];
    return HM_OK;
}

int hm_pileup_set_reference(hm_pileup_t* p, int32_t n_seqs, const int64_t* seq_len, const char* bases) {
    if (!p || n_seqs <= 0 || !seq_len || !bases) return pfail(p, HM_EINVAL, "hm_pileup_set_reference: bad argument");
    std::vector<int64_t> seq_off(1, 0);  // the engine keeps its own until every argument has passed
    for (int i = 0; i < n_seqs; ++i) {
        if (seq_len[i] < 0) return pfail(p, HM_EINVAL, "negative sequence length");
        seq_off.push_back(seq_off.back() + seq_len[i]);
        if (seq_off.back() >= (int64_t(1) << 40)) return pfail(p, HM_EINVAL, "reference longer than 2^40 bases");
    }
    const int64_t total = seq_off.back();
    return guarded(p, [&] {
        drop_job(p);
        p->seq_off = std::move(seq_off);
        p->d_ref.reserve((size_t)total + 4);
        HIP_TRY(hipMemcpyAsync(p->d_ref.p, bases, (size_t)total, hipMemcpyHostToDevice, p->stream));
        if (p->own_planes) {
            const size_t bytes = (size_t)std::max<int64_t>(total, 1) * 4;
            p->d_pcov.reserve(bytes);
            p->d_ncov.reserve(bytes);
            p->d_key.reserve(bytes);
            p->pcov = p->d_pcov.as<int32_t>();
            p->ncov = p->d_ncov.as<int32_t>();
            p->key = p->d_key.as<uint32_t>();
            HIP_TRY(hipMemsetAsync(p->pcov, 0, bytes, p->stream));
            HIP_TRY(hipMemsetAsync(p->ncov, 0, bytes, p->stream));
            HIP_TRY(hipMemsetAsync(p->key, 0, bytes, p->stream));
        }
        if (p->partitions == 2) {
            const size_t bytes = (size_t)std::max<int64_t>(total, 1) * 4;
            for (int k = 0; k < 2; ++k) {
                if (p->hp_pcov[k] && p->hp_pcov[k] != p->d_hp_pcov[k].as<int32_t>()) continue;  // caller-owned (hm_pileup_use_partition_planes)
                p->d_hp_pcov[k].reserve(bytes);
                p->d_hp_ncov[k].reserve(bytes);
                p->hp_pcov[k] = p->d_hp_pcov[k].as<int32_t>();
                p->hp_ncov[k] = p->d_hp_ncov[k].as<int32_t>();
                HIP_TRY(hipMemsetAsync(p->hp_pcov[k], 0, bytes, p->stream));
                HIP_TRY(hipMemsetAsync(p->hp_ncov[k], 0, bytes, p->stream));
            }
        }
        if (p->groups) {  // sized in whole words: the kernel adds to the word that holds a locus' byte or bit
            const size_t n = (size_t)std::max<int64_t>(total, 1);
            for (int k = 0; k < 2; ++k) {
                p->d_gmoment[k].reserve(8 * n);
                p->d_gsamples[k].reserve(4 * ((n + 3) / 4));
                HIP_TRY(hipMemsetAsync(p->d_gmoment[k].p, 0, 8 * n, p->stream));
                HIP_TRY(hipMemsetAsync(p->d_gsamples[k].p, 0, 4 * ((n + 3) / 4), p->stream));
            }
            p->d_gseen.reserve(4 * ((n + 31) / 32));
            HIP_TRY(hipMemsetAsync(p->d_gseen.p, 0, 4 * ((n + 31) / 32), p->stream));
        }
        if (p->samples) {  // a plane is a whole number of words: the kernel swaps the word that holds a locus
            p->sample_stride = (std::max<int64_t>(total, 1) + 1) & ~int64_t(1);
            const size_t bytes = 2 * (size_t)p->sample_stride * (size_t)p->samples;
            p->d_slevel.reserve(bytes);
            HIP_TRY(hipMemsetAsync(p->d_slevel.p, 0, bytes, p->stream));
        }
        if (p->patterns || p->bedmethyl) {
            const int rc = list_reference_cpgs(p);
            if (rc != HM_OK) return rc;
        }
        if (p->linkage) {
            const size_t bytes = sizeof(unsigned long long) * LH_HISTS * 256 * ((size_t)p->linkage + 1);
            p->d_lhist.reserve(bytes);
            HIP_TRY(hipMemsetAsync(p->d_lhist.p, 0, bytes, p->stream));
        }
        if (p->profile) {
            const size_t bytes = sizeof(unsigned long long) * readpos_counters(p);
            p->d_rphist.reserve(bytes);
            HIP_TRY(hipMemsetAsync(p->d_rphist.p, 0, bytes, p->stream));
        }
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
}

int hm_pileup_planes(hm_pileup_t* p, void** pcov, void** ncov, void** key, int64_t* n_loci) {
    if (!p || p->seq_off.empty()) return pfail(p, HM_ESTATE, "hm_pileup_planes before hm_pileup_set_reference");
    if (pcov) *pcov = p->pcov;
    if (ncov) *ncov = p->ncov;
    if (key) *key = p->key;
    if (n_loci) *n_loci = p->seq_off.back();
    return HM_OK;
}

int hm_pileup_submit_read(hm_pileup_t* p, uint32_t order, int32_t flag, int32_t sid, int64_t pos, int32_t mapq,
                          int32_t l_qseq, const uint8_t* seq4, int32_t n_cigar, const uint32_t* cigar, int64_t n_mods,
                          const hm_mod_t* mods) {
    return hm_pileup_submit_read_hp(p, order, flag, sid, pos, mapq, l_qseq, seq4, n_cigar, cigar, n_mods, mods, 0);
}

int hm_pileup_submit_read_hp(hm_pileup_t* p, uint32_t order, int32_t flag, int32_t sid, int64_t pos, int32_t mapq,
                             int32_t l_qseq, const uint8_t* seq4, int32_t n_cigar, const uint32_t* cigar, int64_t n_mods,
                             const hm_mod_t* mods, int32_t hp) {
    PRead r;
    BatchMark mark;
    const int rc = stage_alignment(p, order, flag, sid, pos, mapq, l_qseq, seq4, n_cigar, cigar, n_mods, mods, hp, r, mark);
    if (rc != 1) return rc;
    const int32_t ri = (int32_t)p->reads.size();
    const size_t mods_before = p->mods.size();
    const int64_t m_before = p->n_m_mods;
    for (int64_t i = 0; i < n_mods; ++i) {
        const hm_mod_t& m = mods[i];
        if (m.qoff < 0 || m.qoff >= l_qseq) {  // leave the staged batch as it was
            roll_back(p, mark);
            p->mods.resize(mods_before);
            p->n_m_mods = m_before;
            return pfail(p, HM_EDATA, "modification offset outside the read");
        }
        const bool is_m = m.code == 'm';
        const bool cg = m.unmod_base == 'C' || m.unmod_base == 'G';
        if (!is_m && !cg) continue;
        p->mods.push_back(PMod{ri, m.qoff, ((uint32_t)i << 10) | (is_m ? 0x200u : 0u) | (cg ? 0x100u : 0u) | m.prob});
        if (is_m) ++p->n_m_mods;
    }
    commit_read(p, r, seq4);
    return 1;
}

int hm_pileup_submit_read_calls(hm_pileup_t* p, uint32_t order, int32_t flag, int32_t sid, int64_t pos, int32_t mapq,
                                int32_t l_qseq, const uint8_t* seq4, int32_t n_cigar, const uint32_t* cigar,
                                int64_t n_calls, const hm_call_t* calls, int32_t hp) {
    PRead r;
    BatchMark mark;
    const int rc = stage_alignment(p, order, flag, sid, pos, mapq, l_qseq, seq4, n_cigar, cigar, n_calls, calls, hp, r, mark);
    if (rc != 1) return rc;
    // what apply_calls refuses (hm_bam.cpp): an offset outside the read; calls not strictly increasing per strand, FWD first
    const int32_t ri = (int32_t)p->reads.size();
    const size_t calls_before = p->calls.size();
    p->calls.resize(calls_before + (size_t)n_calls);
    PCall* dst = p->calls.data() + calls_before;
    int strand = 0;
    int32_t last = -1;
    for (int64_t i = 0; i < n_calls; ++i) {
        const hm_call_t& c = calls[i];
        const bool outside = c.qoff < 0 || c.qoff >= l_qseq;
        if (c.strand != strand && c.strand == 1) { strand = 1; last = -1; }
        if (outside || c.strand != strand || c.qoff <= last) {  // leave the staged batch as it was
            roll_back(p, mark);
            p->calls.resize(calls_before);
            return outside ? pfail(p, HM_EDATA, "call offset outside the read")
                           : pfail(p, HM_EINVAL, "calls are not strictly increasing per strand, FWD strand first");
        }
        last = c.qoff;
        dst[i] = PCall{ri, c.qoff, c.strand, c.ctx, c.scaled_prob, 0};
    }
    p->n_m_mods += n_calls;
    commit_read(p, r, seq4);
    return 1;
}

int hm_pileup_run(hm_pileup_t* p) {
    if (!p) return HM_EINVAL;
    if (p->reads.empty()) return HM_OK;
    return guarded(p, [&] {
        ensure_bins(p);
        hipStream_t st = p->stream;
        const int n_reads = (int)p->reads.size(), n_runs = (int)p->runs.size();
        p->col0.resize((size_t)n_runs + 1);
        int64_t cols = 0;
        for (int i = 0; i < n_runs; ++i) { p->col0[i] = cols; cols += p->runs[i].len; }
        p->col0[n_runs] = cols;
        const int64_t n_mods = (int64_t)p->mods.size(), n_calls = (int64_t)p->calls.size();
        const int64_t n_gaps = p->bedmethyl && p->n_cpg ? (int64_t)p->gaps.size() : 0;

        p->d_slab.reserve(p->slab.size() + 4);
        p->d_reads.reserve(sizeof(PRead) * (size_t)n_reads);
        p->d_runs.reserve(sizeof(PRun) * (size_t)std::max(n_runs, 1));
        p->d_col0.reserve(sizeof(int64_t) * ((size_t)n_runs + 1));
        p->d_mods.reserve(sizeof(PMod) * (size_t)std::max<int64_t>(n_mods, 1));
        if (n_calls) p->d_calls.reserve(sizeof(PCall) * (size_t)n_calls);
        p->d_plane.reserve(4 * (size_t)std::max<int64_t>(p->plane_len, 1));
        p->d_matches.reserve(4 * (size_t)n_reads);
        p->d_recs.reserve(sizeof(PRec) * (size_t)(p->n_recs + p->n_m_mods + 1), sizeof(PRec) * (size_t)p->n_recs, st);
        if (p->patterns)  // a window record has a member at its head, a member a 5mC entry of its own
            p->d_precs.reserve(sizeof(PWin) * (size_t)(p->n_precs + p->n_m_mods + 1), sizeof(PWin) * (size_t)p->n_precs, st);

        HIP_TRY(hipMemcpyAsync(p->d_slab.p, p->slab.data(), p->slab.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(p->d_reads.p, p->reads.data(), sizeof(PRead) * (size_t)n_reads, hipMemcpyHostToDevice, st));
        if (n_runs) HIP_TRY(hipMemcpyAsync(p->d_runs.p, p->runs.data(), sizeof(PRun) * (size_t)n_runs, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(p->d_col0.p, p->col0.data(), sizeof(int64_t) * ((size_t)n_runs + 1), hipMemcpyHostToDevice, st));
        if (n_mods) HIP_TRY(hipMemcpyAsync(p->d_mods.p, p->mods.data(), sizeof(PMod) * (size_t)n_mods, hipMemcpyHostToDevice, st));
        if (n_calls) HIP_TRY(hipMemcpyAsync(p->d_calls.p, p->calls.data(), sizeof(PCall) * (size_t)n_calls, hipMemcpyHostToDevice, st));
        if (n_gaps) {
            p->d_gaps.reserve(sizeof(PGap) * (size_t)n_gaps);
            HIP_TRY(hipMemcpyAsync(p->d_gaps.p, p->gaps.data(), sizeof(PGap) * (size_t)n_gaps, hipMemcpyHostToDevice, st));
        }
        HIP_TRY(hipMemsetAsync(p->d_plane.p, 0, 4 * (size_t)std::max<int64_t>(p->plane_len, 1), st));
        HIP_TRY(hipMemsetAsync(p->d_matches.p, 0, 4 * (size_t)n_reads, st));

        if (n_mods)  // <= 1024 workgroups: each flushes up to 768 histogram bins with same-address global atomics (~10 ns each)
            hipLaunchKernelGGL(entries_kernel<PMod>, dim3(grid_for(n_mods, 1024)), dim3(TPB), 0, st, p->d_mods.as<PMod>(), n_mods,
                               p->d_reads.as<PRead>(), p->d_slab.as<uint8_t>(), p->d_plane.as<uint32_t>(),
                               p->d_bins.as<unsigned long long>(), p->trim);
        if (n_calls)  // the records submitted with calls: their plane words and histogram counts, same grid rule
            hipLaunchKernelGGL(entries_kernel<PCall>, dim3(grid_for(n_calls, 1024)), dim3(TPB), 0, st, p->d_calls.as<PCall>(), n_calls,
                               p->d_reads.as<PRead>(), p->d_slab.as<uint8_t>(), p->d_plane.as<uint32_t>(),
                               p->d_bins.as<unsigned long long>(), p->trim);
        const BatchView batch = batch_view(p, n_runs, cols);
        if (cols > 0) {
            const int64_t blocks = (cols + TPB - 1) / TPB, pblocks = (cols + PTILE - 1) / PTILE;
            if (blocks >= (int64_t(1) << 31)) return pfail(p, HM_EINVAL, "batch too large: submit fewer records per hm_pileup_run");
            if (p->min_pi > 0.0)
                hipLaunchKernelGGL(identity_kernel, dim3((unsigned)blocks), dim3(TPB), 0, st, batch, p->d_matches.as<int32_t>());
            if (p->profile)
                hipLaunchKernelGGL(project_kernel<true>, dim3((unsigned)pblocks), dim3(TPB), 0, st, batch, p->d_recs.as<PRec>(),
                                   p->d_counter.as<unsigned long long>(), readpos_table(p));
            else
                hipLaunchKernelGGL(project_kernel<false>, dim3((unsigned)pblocks), dim3(TPB), 0, st, batch, p->d_recs.as<PRec>(),
                                   p->d_counter.as<unsigned long long>(), ReadPos{nullptr, 0});
            if (p->patterns && p->n_cpg)
                hipLaunchKernelGGL(pattern_kernel, dim3((unsigned)pblocks), dim3(TPB), 0, st, batch, pattern_rule(p), p->d_precs.as<PWin>(),
                                   p->d_pcounter.as<unsigned long long>());
            if (p->bedmethyl && p->n_cpg)
                hipLaunchKernelGGL(depth_kernel, dim3((unsigned)pblocks), dim3(TPB), 0, st, batch, p->seq_off.back(), depth_counters(p));
        }
        if (n_gaps)  // deletions are rare next to columns: one thread each
            hipLaunchKernelGGL(depth_gap_kernel, dim3(grid_for(n_gaps, 1024)), dim3(TPB), 0, st, p->d_gaps.as<PGap>(), n_gaps,
                               p->d_reads.as<PRead>(), p->d_matches.as<int32_t>(), p->min_pi, depth_counters(p));
        if (p->linkage && cols > 0) {
            const int rc = count_linkage_pairs(p, batch);
            if (rc != HM_OK) return rc;
        }
        HIP_TRY(hipGetLastError());
        unsigned long long n = 0, n_win = 0;
        HIP_TRY(hipMemcpyAsync(&n, p->d_counter.p, sizeof n, hipMemcpyDeviceToHost, st));
        if (p->patterns) HIP_TRY(hipMemcpyAsync(&n_win, p->d_pcounter.p, sizeof n_win, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        p->n_recs = (int64_t)n;
        p->n_precs = (int64_t)n_win;
        clear_batch(p);
        return HM_OK;
    });
}

int64_t hm_pileup_num_records(hm_pileup_t* p) { return p ? p->n_recs : HM_EINVAL; }

int hm_pileup_histograms(hm_pileup_t* p, uint64_t* bins768) {
    if (!p || !bins768) return HM_EINVAL;
    return guarded(p, [&] {
        ensure_bins(p);
        HIP_TRY(hipMemcpyAsync(bins768, p->d_bins.p, 768 * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
}

int64_t hm_pileup_fetch_records(hm_pileup_t* p, int64_t* gpos, uint8_t* prob, uint8_t* motif, uint32_t* order, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (cap < p->n_recs) return p->n_recs;
    std::vector<PRec> h((size_t)p->n_recs);
    const int rc = guarded(p, [&] {
        if (p->n_recs) HIP_TRY(hipMemcpyAsync(h.data(), p->d_recs.p, sizeof(PRec) * h.size(), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
    if (rc < 0) return rc;
    for (size_t i = 0; i < h.size(); ++i) {
        if (gpos) gpos[i] = h[i].gpos();
        if (prob) prob[i] = (uint8_t)h[i].prob();
        if (motif) motif[i] = (uint8_t)h[i].motif();
        if (order) order[i] = h[i].order;
    }
    return p->n_recs;
}

int hm_pileup_label_histograms(hm_pileup_t* p, const int8_t* labels, int64_t n_labels, uint64_t* bins1536) {
    if (!p || !labels || !bins1536) return HM_EINVAL;
    if (p->seq_off.empty()) return pfail(p, HM_ESTATE, "hm_pileup_label_histograms before hm_pileup_set_reference");
    if (n_labels != p->seq_off.back()) return pfail(p, HM_EINVAL, "hm_pileup_label_histograms: one label per reference base expected");
    return guarded(p, [&] {
        p->d_labels.reserve((size_t)n_labels + 1);
        p->d_lbins.reserve(1536 * sizeof(unsigned long long));
        HIP_TRY(hipMemcpyAsync(p->d_labels.p, labels, (size_t)n_labels, hipMemcpyHostToDevice, p->stream));
        HIP_TRY(hipMemsetAsync(p->d_lbins.p, 0, 1536 * sizeof(unsigned long long), p->stream));
        if (p->n_recs) {
            hipLaunchKernelGGL(label_kernel, dim3(grid_for(p->n_recs, 1024)), dim3(TPB), 0, p->stream, p->d_recs.as<PRec>(), p->n_recs,
                               p->d_labels.as<int8_t>(), p->d_lbins.as<unsigned long long>());
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(bins1536, p->d_lbins.p, 1536 * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
}

int hm_pileup_count(hm_pileup_t* p, const uint8_t thr[3]) {
    if (!p || !thr) return HM_EINVAL;
    if (!p->pcov) return pfail(p, HM_ESTATE, "hm_pileup_count before hm_pileup_set_reference / hm_pileup_use_planes");
    if (p->partitions == 2 && (!p->hp_pcov[0] || !p->hp_pcov[1]))
        return pfail(p, HM_ESTATE, "hm_pileup_count without partition planes (hm_pileup_set_reference / hm_pileup_use_partition_planes)");
    return guarded(p, [&] {
        ensure_bins(p);
        const uint32_t packed = thr[0] | ((uint32_t)thr[1] << 8) | ((uint32_t)thr[2] << 16);
        if (p->n_recs) {
            const CountPlanes own{p->pcov, p->ncov, p->key};
            if (p->partitions == 2)
                hipLaunchKernelGGL(count_kernel<CountHpPlanes>, dim3(grid_for(p->n_recs, 1 << 16)), dim3(TPB), 0, p->stream,
                                   p->d_recs.as<PRec>(), p->n_recs, packed,
                                   CountHpPlanes{own, p->hp_pcov[0], p->hp_ncov[0], p->hp_pcov[1], p->hp_ncov[1]});
            else
                hipLaunchKernelGGL(count_kernel<CountPlanes>, dim3(grid_for(p->n_recs, 1 << 16)), dim3(TPB), 0, p->stream,
                                   p->d_recs.as<PRec>(), p->n_recs, packed, own);
            HIP_TRY(hipGetLastError());
        }
        if (p->patterns && p->n_precs) {  // <= 1024 workgroups: every record is one fire-and-forget atomic
            hipLaunchKernelGGL(pattern_count_kernel, dim3(grid_for(p->n_precs, 1024)), dim3(TPB), 0, p->stream, p->d_precs.as<PWin>(),
                               p->n_precs, (uint32_t)thr[0], p->patterns, p->d_phist.as<uint32_t>());
            HIP_TRY(hipGetLastError());
        }
        if (p->bedmethyl && p->n_cpg && p->n_recs) {  // the records are still resident: the CpG ones are the members
            hipLaunchKernelGGL(depth_count_kernel, dim3(grid_for(p->n_recs, 1 << 16)), dim3(TPB), 0, p->stream, p->d_recs.as<PRec>(), p->n_recs,
                               (uint32_t)thr[0], depth_counters(p));
            HIP_TRY(hipGetLastError());
        }
        if (p->patterns) HIP_TRY(hipMemsetAsync(p->d_pcounter.p, 0, sizeof(unsigned long long), p->stream));
        HIP_TRY(hipMemsetAsync(p->d_counter.p, 0, sizeof(unsigned long long), p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        p->n_recs = 0;
        p->n_precs = 0;
        p->counted = true;
        p->linkage_thr = thr[0];
        p->thr_packed = packed;
        return HM_OK;
    });
}

int64_t hm_pileup_fetch_loci(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base,
                             int64_t lo, int64_t hi, hm_locus_t* out, int64_t cap) {
    if (!p || lo < 0 || hi < lo) return pfail(p, HM_EINVAL, "hm_pileup_fetch_loci: bad range");
    RangePlanes s;
    if (!range_planes(p, pcov, ncov, key, plane_base, s)) return HM_ESTATE;
    if (hi == lo) return 0;
    return compact_rows(p, LociSel{s, plane_base}, lo, hi, out, cap, no_hook, no_hook);
}

// ---- `diff` -----------------------------------------------------------------------------------------------------------------------
int64_t hm_pileup_load_loci(hm_pileup_t* p, int32_t part, const hm_locus_t* rows, int64_t n) {
    if (!p) return HM_EINVAL;
    if ((part != 1 && part != 2) || n < 0 || (n && !rows)) return pfail(p, HM_EINVAL, "hm_pileup_load_loci: part must be 1 or 2, n >= 0, rows not NULL");
    if (p->load_failed) return pfail(p, HM_ESTATE, std::string("hm_pileup_load_loci: ") + LOAD_FAILED_TEXT);
    if (p->partitions != 2 || p->seq_off.empty() || !p->pcov || !p->hp_pcov[0] || !p->hp_pcov[1])
        return pfail(p, HM_ESTATE, "hm_pileup_load_loci needs option partitions = 2 and hm_pileup_set_reference");
    if (p->staged_any) return pfail(p, HM_ESTATE, "hm_pileup_load_loci on an engine that has staged records: counts come from records or from loads, not both");
    if (p->group_open || p->samples_open)
        return pfail(p, HM_ESTATE, "hm_pileup_load_loci on an engine that opened a sample (hm_pileup_group_sample, hm_sample_open)");
    // the first rows of this engine (or of a longer reference): d_gseen becomes the two partitions' seen bitmaps, cleared
    if (n && (!p->loaded || p->d_gseen.cap < 2 * 4 * seen_words(p))) {
        const int made = guarded(p, [&] {
            p->d_gseen.reserve(2 * 4 * seen_words(p));
            HIP_TRY(hipMemsetAsync(p->d_gseen.p, 0, 2 * 4 * seen_words(p), p->stream));
            return HM_OK;
        });
        if (made != HM_OK) return made;
    }
    const LoadPlanes sink{{p->pcov, p->ncov, p->key}, p->hp_pcov[part - 1], p->hp_ncov[part - 1],
                          p->d_gseen.as<uint32_t>() + (size_t)(part - 1) * seen_words(p)};
    const int64_t added = load_rows(p, "hm_pileup_load_loci", rows, n, sink, "locus given twice for one part");
    if (n && added >= 0) p->loaded = true;
    return added;
}

// ---- `groupdiff` ------------------------------------------------------------------------------------------------------------------
namespace {
// 1 / (a B(a, 1/2)) = Gamma((nu + 1) / 2) / (sqrt(pi) Gamma(nu / 2 + 1)) for nu = 0 .. 2 GROUP_MAX_SAMPLES - 2, by the recurrence
// c(nu + 2) = c(nu) (nu + 1) / (nu + 2) from c(1) = 2 / pi, c(2) = 1 / 2 in long double, rounded once: uploaded once per engine
void ensure_group_coef(hm_pileup* p) {
    if (p->d_gcoef.p) return;
    static const std::vector<double> tab = [] {
        std::vector<long double> c((size_t)2 * GROUP_MAX_SAMPLES - 1);
        c[0] = 1.0L;
        c[1] = 2.0L / 3.14159265358979323846264338327950288L;
        for (size_t nu = 2; nu < c.size(); ++nu) c[nu] = c[nu - 2] * (long double)(nu - 1) / (long double)nu;
        return std::vector<double>(c.begin(), c.end());
    }();
    p->d_gcoef.reserve(sizeof(double) * tab.size());
    HIP_TRY(hipMemcpyAsync(p->d_gcoef.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
}
}  // namespace

int hm_pileup_group_sample(hm_pileup_t* p, int32_t part) {
    if (!p) return HM_EINVAL;
    if (part != 1 && part != 2) return pfail(p, HM_EINVAL, "hm_pileup_group_sample: part must be 1 or 2");
    const int rc = option_ready(p, "hm_pileup_group_sample", group_needs(p));
    if (rc != HM_OK) return rc;
    if (p->staged_any || p->loaded || p->samples_open)
        return pfail(p, HM_ESTATE, "hm_pileup_group_sample on an engine that staged records or used hm_pileup_load_loci / hm_sample_open: counts come from one source");
    if (p->group_samples[part - 1] >= GROUP_MAX_SAMPLES) return pfail(p, HM_ESTATE, "hm_pileup_group_sample: a group holds at most 255 samples");
    const int cleared = guarded(p, [&] {
        HIP_TRY(hipMemsetAsync(p->d_gseen.p, 0, 4 * (((size_t)std::max<int64_t>(p->seq_off.back(), 1) + 31) / 32), p->stream));
        return HM_OK;
    });
    if (cleared != HM_OK) return cleared;
    p->group_open = part;
    return p->group_samples[part - 1]++;
}

int64_t hm_pileup_load_sample_loci(hm_pileup_t* p, const hm_locus_t* rows, int64_t n) {
    if (!p) return HM_EINVAL;
    if (n < 0 || (n && !rows)) return pfail(p, HM_EINVAL, "hm_pileup_load_sample_loci: n >= 0, rows not NULL");
    const int ready = option_ready(p, "hm_pileup_load_sample_loci", group_needs(p));
    if (ready != HM_OK) return ready;
    if (!p->group_open) return pfail(p, HM_ESTATE, "hm_pileup_load_sample_loci before hm_pileup_group_sample");
    const int g = p->group_open - 1;
    const GroupLoadPlanes sink{{{p->pcov, p->ncov, p->key}, p->hp_pcov[g], p->hp_ncov[g], p->d_gseen.as<uint32_t>()},
                               p->d_gmoment[g].as<unsigned long long>(), p->d_gsamples[g].as<uint32_t>(), p->group_min_cov};
    return load_rows(p, "hm_pileup_load_sample_loci", rows, n, sink, "locus given twice in one sample");
}

namespace {
GroupPlanes group_planes(hm_pileup* p) {
    return GroupPlanes{AsmPlanes{p->hp_pcov[0], p->hp_ncov[0], p->hp_pcov[1], p->hp_ncov[1], p->key}, p->d_gmoment[0].as<unsigned long long>(),
                       p->d_gmoment[1].as<unsigned long long>(), p->d_gsamples[0].as<uint8_t>(), p->d_gsamples[1].as<uint8_t>()};
}
}  // namespace

int64_t hm_pileup_fetch_groups(hm_pileup_t* p, int64_t lo, int64_t hi, int32_t min_reps, hm_group_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (min_reps < 1 || min_reps > GROUP_MAX_SAMPLES) return pfail(p, HM_EINVAL, "hm_pileup_fetch_groups: min_reps must be in 1 .. 255");
    const int rc = option_range(p, "hm_pileup_fetch_groups", group_needs(p), lo, hi);
    if (rc != HM_OK) return rc;
    if (hi == lo) return 0;
    const GroupPlanes s = group_planes(p);
    return compact_rows_to(
        p, GroupSel{s, min_reps}, lo, hi, [&](int64_t total) { return fits(total, out, cap) ? out : nullptr; }, [&] { ensure_group_coef(p); },
        [&](hm_group_t* rows, int64_t total) {
            hipLaunchKernelGGL(group_test_kernel, row_grid(total), dim3(TPB), 0, p->stream, rows, total, s, p->d_gcoef.as<double>());
        });
}

int hm_pileup_group_planes(hm_pileup_t* p, int32_t part, int64_t lo, int64_t hi, uint64_t* moment, uint8_t* samples) {
    if (!p) return HM_EINVAL;
    if (part != 1 && part != 2) return pfail(p, HM_EINVAL, "hm_pileup_group_planes: part must be 1 or 2");
    const int rc = option_range(p, "hm_pileup_group_planes", group_needs(p), lo, hi);
    if (rc != HM_OK || hi == lo) return rc;
    return guarded(p, [&] {
        const size_t n = (size_t)(hi - lo);
        if (moment) HIP_TRY(hipMemcpyAsync(moment, p->d_gmoment[part - 1].as<unsigned long long>() + lo, 8 * n, hipMemcpyDeviceToHost, p->stream));
        if (samples) HIP_TRY(hipMemcpyAsync(samples, p->d_gsamples[part - 1].as<uint8_t>() + lo, n, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
}

int hm_group_qvalues(const hm_group_t* rows, int64_t n, double* q, uint64_t m[3]) {
    if (n < 0 || (n && (!rows || !q)) || !m) return HM_EINVAL;
    for (int64_t i = 0; i < n; ++i)
        if (rows[i].motif > 3u || !(rows[i].pvalue >= DBL_MIN && rows[i].pvalue <= 1.0)) return HM_EINVAL;
    std::vector<BhEntry> ent;
    for (uint32_t c = 0; c < 3; ++c) {
        ent.clear();
        for (int64_t i = 0; i < n; ++i)
            if (std::min(rows[i].motif, 2u) == c) ent.push_back(BhEntry{rows[i].pvalue, 1, i});
        m[c] = ent.size();
        bh_qvalues(ent, m[c], [&](int64_t where, double v) { q[where] = v; });
    }
    return HM_OK;
}

// ---- `groupdmr` -------------------------------------------------------------------------------------------------------------------
int64_t hm_dmr_fetch_regions(hm_pileup_t* p, int64_t lo, int64_t hi, int32_t min_reps, int32_t ctx, double max_p, double min_diff,
                             int64_t max_gap, int32_t min_loci, int32_t keep_edges, int64_t* n_ctx_rows, int64_t* n_hits,
                             hm_group_region_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (min_reps < 1 || min_reps > GROUP_MAX_SAMPLES) return pfail(p, HM_EINVAL, "hm_dmr_fetch_regions: min_reps must be in 1 .. 255");
    if (ctx < 0 || ctx > 2) return pfail(p, HM_EINVAL, "hm_dmr_fetch_regions: ctx must be 0, 1 or 2");
    if (!(max_p > 0.0 && max_p <= 1.0)) return pfail(p, HM_EINVAL, "hm_dmr_fetch_regions: max_p must be in (0, 1]");
    if (!(min_diff >= 0.0 && min_diff <= 100.0)) return pfail(p, HM_EINVAL, "hm_dmr_fetch_regions: min_diff must be in [0, 100]");
    if (max_gap < 1 || min_loci < 1) return pfail(p, HM_EINVAL, "hm_dmr_fetch_regions: max_gap and min_loci must be >= 1");
    const int rc = option_range(p, "hm_dmr_fetch_regions", group_needs(p), lo, hi);
    if (rc != HM_OK) return rc;
    if (n_ctx_rows) *n_ctx_rows = 0;
    if (n_hits) *n_hits = 0;
    if (hi == lo) return 0;
    const GroupPlanes s = group_planes(p);
    return guarded(p, [&]() -> int64_t {
        const int64_t R = stage_rows(  // the context's rows, tested, stay in d_grows
            p, GroupCtxSel{GroupSel{s, min_reps}, (uint32_t)ctx}, lo, hi, p->d_grows,
            [&](int64_t) {
                ensure_group_coef(p);
                return true;
            },
            [&](hm_group_t* rows, int64_t n) {
                hipLaunchKernelGGL(group_test_kernel, row_grid(n), dim3(TPB), 0, p->stream, rows, n, s, p->d_gcoef.as<double>());
            });
        if (R <= 0) return R;
        if (n_ctx_rows) *n_ctx_rows = R;
        const hm_group_t* rows = p->d_grows.as<hm_group_t>();
        const GroupRegionRule rule{{max_p, max_gap, min_loci, keep_edges != 0}, min_diff};
        if (n_hits) {  // counted, never written
            const int64_t hits = stage_rows(p, GroupHitSel{rows, rule}, 0, R, p->d_rows, [](int64_t) { return false; }, no_hook);
            if (hits < 0) return hits;
            *n_hits = hits;
        }
        return compact_rows(p, RegionSel<GroupChain>{rows, R, rule, (uint32_t)ctx}, 0, R, out, cap, no_hook, no_hook);
    });
}

int hm_dmr_p_cutoff(const hm_group_t* rows, const double* q, int64_t n, double max_q, double cutoff[3]) {
    if (n < 0 || (n && (!rows || !q)) || !cutoff || !(max_q > 0.0 && max_q <= 1.0)) return HM_EINVAL;
    for (int64_t i = 0; i < n; ++i)
        if (rows[i].motif > 3u || !(rows[i].pvalue >= DBL_MIN && rows[i].pvalue <= 1.0)) return HM_EINVAL;
    cutoff[0] = cutoff[1] = cutoff[2] = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        double& c = cutoff[std::min(rows[i].motif, 2u)];
        if (q[i] <= max_q && rows[i].pvalue > c) c = rows[i].pvalue;
    }
    return HM_OK;
}

// ---- `samplecorr` -----------------------------------------------------------------------------------------------------------------
int hm_sample_geometry(int64_t out[2]) {
    if (!out) return HM_EINVAL;
    out[0] = HM_SAMPLE_TILE;
    out[1] = HM_SAMPLE_MAX;
    return HM_OK;
}

int hm_sample_open(hm_pileup_t* p) {
    if (!p) return HM_EINVAL;
    const int rc = option_ready(p, "hm_sample_open", sample_needs(p));
    if (rc != HM_OK) return rc;
    if (p->staged_any || p->loaded || p->group_open)
        return pfail(p, HM_ESTATE, "hm_sample_open on an engine that staged records or used hm_pileup_load_loci / hm_pileup_group_sample: counts come from one source");
    if (p->samples_open >= p->samples) return pfail(p, HM_ESTATE, "hm_sample_open: all " + std::to_string(p->samples) + " samples of option samples are open");
    return p->samples_open++;
}

int64_t hm_sample_load(hm_pileup_t* p, const hm_locus_t* rows, int64_t n) {
    if (!p) return HM_EINVAL;
    if (n < 0 || (n && !rows)) return pfail(p, HM_EINVAL, "hm_sample_load: n >= 0, rows not NULL");
    const int ready = option_ready(p, "hm_sample_load", sample_needs(p));
    if (ready != HM_OK) return ready;
    if (!p->samples_open) return pfail(p, HM_ESTATE, "hm_sample_load before hm_sample_open");
    const SampleLoadPlanes sink{{p->pcov, p->ncov, p->key}, p->d_slevel.as<uint32_t>() + (p->samples_open - 1) * (p->sample_stride / 2),
                                p->sample_min_cov};
    return load_rows(p, "hm_sample_load", rows, n, sink, "locus given twice in one sample");
}

int64_t hm_sample_fetch_sums(hm_pileup_t* p, int64_t lo, int64_t hi, int32_t complete, hm_sample_pair_t* out) {
    if (!p) return HM_EINVAL;
    if (complete != 0 && complete != 1) return pfail(p, HM_EINVAL, "hm_sample_fetch_sums: complete must be 0 or 1");
    const int rc = option_range(p, "hm_sample_fetch_sums", sample_needs(p), lo, hi);
    if (rc != HM_OK) return rc;
    const int M = p->samples_open, pairs = M * (M + 1) / 2;
    if (!pairs) return 0;
    if (!out) return pfail(p, HM_EINVAL, "hm_sample_fetch_sums: out is NULL");
    std::vector<unsigned long long> table((size_t)3 * pairs * 6, 0);
    if (hi > lo) {
        const int done = guarded(p, [&] {
            const size_t bytes = sizeof(unsigned long long) * table.size();
            p->d_stable.reserve(sizeof(unsigned long long) * 3 * 6 * (size_t)(SAMPLE_MAX * (SAMPLE_MAX + 1) / 2));
            HIP_TRY(hipMemsetAsync(p->d_stable.p, 0, bytes, p->stream));
            const int64_t tiles = (hi + SAMPLE_TILE - 1) / SAMPLE_TILE - lo / SAMPLE_TILE;
            const int pitch = ((M + 1) / 2) | 1;
            const size_t lds = sizeof(uint32_t) * ((size_t)SAMPLE_TILE * pitch + SAMPLE_TILE + 1);
            const dim3 grid((unsigned)std::min<int64_t>(tiles, 1024), (unsigned)((pairs + TPB - 1) / TPB), 3);
            hipLaunchKernelGGL(sample_sums_kernel, grid, dim3(TPB), lds, p->stream, p->d_slevel.as<uint16_t>(), p->sample_stride, M, p->key, lo, hi,
                               (int)complete, p->d_stable.as<unsigned long long>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(table.data(), p->d_stable.p, bytes, hipMemcpyDeviceToHost, p->stream));
            HIP_TRY(hipStreamSynchronize(p->stream));
            return HM_OK;
        });
        if (done != HM_OK) return done;
    }
    hm_sample_pair_t* e = out;
    const unsigned long long* t = table.data();
    for (uint32_t c = 0; c < 3; ++c)
        for (int i = 0; i < M; ++i)
            for (int j = i; j < M; ++j, ++e, t += 6) *e = hm_sample_pair_t{i, j, c, 0, t[0], t[1], t[2], t[3], t[4], t[5]};
    return (int64_t)3 * pairs;
}

int hm_sample_plane(hm_pileup_t* p, int32_t s, int64_t lo, int64_t hi, uint16_t* out) {
    if (!p) return HM_EINVAL;
    const int rc = option_range(p, "hm_sample_plane", sample_needs(p), lo, hi);
    if (rc != HM_OK) return rc;
    if (s < 0 || s >= p->samples) return pfail(p, HM_EINVAL, "hm_sample_plane: no such sample");
    if (hi == lo) return HM_OK;
    if (!out) return pfail(p, HM_EINVAL, "hm_sample_plane: out is NULL");
    return guarded(p, [&] {
        HIP_TRY(hipMemcpyAsync(out, p->d_slevel.as<uint16_t>() + (int64_t)s * p->sample_stride + lo, 2 * (size_t)(hi - lo), hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
}

int hm_sample_corr(const hm_sample_pair_t* e, int64_t n, double* r, double* mean_i, double* mean_j) {
    if (n < 0 || (n && !e)) return HM_EINVAL;
    const double nan = std::nan("");
    for (int64_t k = 0; k < n; ++k) {
        using u128 = unsigned __int128;  // wraps instead of overflowing on sums no engine wrote; exact below 2^127, as every engine's are
        const u128 cnt = e[k].n, si = e[k].si, sj = e[k].sj;
        const __int128 num = (__int128)(cnt * e[k].sij - si * sj);
        const __int128 va = (__int128)(cnt * e[k].sii - si * si);
        const __int128 vb = (__int128)(cnt * e[k].sjj - sj * sj);
        if (r) r[k] = e[k].n < 2 || va <= 0 || vb <= 0 ? nan : (double)num / (std::sqrt((double)va) * std::sqrt((double)vb));
        const double denom = (double)e[k].n * 32768.0;
        if (mean_i) mean_i[k] = e[k].n ? 100.0 * (double)e[k].si / denom : nan;
        if (mean_j) mean_j[k] = e[k].n ? 100.0 * (double)e[k].sj / denom : nan;
    }
    return HM_OK;
}

// ---- `pileup -E` ------------------------------------------------------------------------------------------------------------------
int64_t hm_pileup_num_pattern_records(hm_pileup_t* p) { return p ? p->n_precs : HM_EINVAL; }

int64_t hm_pileup_fetch_patterns(hm_pileup_t* p, int64_t lo, int64_t hi, int64_t min_reads, hm_pattern_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (!p->patterns || p->seq_off.empty()) return pfail(p, HM_ESTATE, "hm_pileup_fetch_patterns without option patterns (then hm_pileup_set_reference)");
    if (!p->counted) return pfail(p, HM_ESTATE, "hm_pileup_fetch_patterns before hm_pileup_count");
    if (lo < 0 || hi < lo) return pfail(p, HM_EINVAL, "hm_pileup_fetch_patterns: bad range");
    if (min_reads < 1) return pfail(p, HM_EINVAL, "hm_pileup_fetch_patterns: min_reads must be >= 1");
    if (hi == lo || !p->n_cpg) return 0;
    int64_t ranks[2] = {0, 0};  // the windows of [lo, hi) are those headed by its reference CpGs
    const int rc = cpg_rank_range(p, lo, hi, ranks);
    if (rc != HM_OK) return rc;
    if (ranks[1] <= ranks[0]) return 0;
    return compact_rows(p, PatSel{pattern_rule(p), p->d_phist.as<uint32_t>(), min_reads}, ranks[0], ranks[1], out, cap, no_hook, no_hook);
}

// ---- `pileup -M` ------------------------------------------------------------------------------------------------------------------
int64_t hm_pileup_fetch_bedmethyl(hm_pileup_t* p, int32_t part, int64_t lo, int64_t hi, int64_t min_valid, hm_bedmethyl_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (!p->bedmethyl || p->seq_off.empty()) return pfail(p, HM_ESTATE, "hm_pileup_fetch_bedmethyl without option bedmethyl (then hm_pileup_set_reference)");
    if (!p->counted) return pfail(p, HM_ESTATE, "hm_pileup_fetch_bedmethyl before hm_pileup_count");
    if (part < 0 || part > 2) return pfail(p, HM_EINVAL, "hm_pileup_fetch_bedmethyl: part must be 0, 1 or 2");
    if (part && p->partitions != 2) return pfail(p, HM_ESTATE, "hm_pileup_fetch_bedmethyl: part 1 / 2 without the partitions option");
    if (lo < 0 || hi < lo) return pfail(p, HM_EINVAL, "hm_pileup_fetch_bedmethyl: bad range");
    if (min_valid < 0) return pfail(p, HM_EINVAL, "hm_pileup_fetch_bedmethyl: min_valid must be >= 0");
    if (hi == lo || !p->n_cpg) return 0;
    int64_t ranks[2] = {0, 0};
    const int rc = cpg_rank_range(p, lo, hi, ranks);
    if (rc != HM_OK) return rc;
    if (ranks[1] <= ranks[0]) return 0;
    return compact_rows(p, BmSel{p->d_cpg.as<int64_t>(), depth_counters(p, part).bm, min_valid}, ranks[0], ranks[1], out, cap, no_hook, no_hook);
}

// ---- `pileup -L` ------------------------------------------------------------------------------------------------------------------
int64_t hm_pileup_fetch_linkage(hm_pileup_t* p, int64_t min_pairs, hm_linkage_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (!p->linkage || p->seq_off.empty()) return pfail(p, HM_ESTATE, "hm_pileup_fetch_linkage without option linkage (then hm_pileup_set_reference)");
    if (!p->counted) return pfail(p, HM_ESTATE, "hm_pileup_fetch_linkage before hm_pileup_count");
    if (min_pairs < 0) return pfail(p, HM_EINVAL, "hm_pileup_fetch_linkage: min_pairs must be >= 0");
    const int rc = guarded(p, [&] {
        p->d_ltab.reserve(sizeof(unsigned long long) * 4 * ((size_t)p->linkage + 1));
        hipLaunchKernelGGL(linkage_reduce_kernel, dim3((unsigned)p->linkage + 1), dim3(256), 0, p->stream, p->d_lhist.as<unsigned long long>(),
                           p->linkage_thr, p->d_ltab.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        return HM_OK;
    });
    if (rc != HM_OK) return rc;
    return compact_rows(p, LinkSel{p->d_ltab.as<unsigned long long>(), min_pairs}, 2, (int64_t)p->linkage + 1, out, cap, no_hook, no_hook);
}

// ---- `pileup -P` ------------------------------------------------------------------------------------------------------------------
int64_t hm_pileup_fetch_readpos(hm_pileup_t* p, int64_t min_calls, hm_readpos_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (!p->profile || p->seq_off.empty()) return pfail(p, HM_ESTATE, "hm_pileup_fetch_readpos without option profile (then hm_pileup_set_reference)");
    if (!p->counted) return pfail(p, HM_ESTATE, "hm_pileup_fetch_readpos before hm_pileup_count");
    if (min_calls < 0) return pfail(p, HM_EINVAL, "hm_pileup_fetch_readpos: min_calls must be >= 0");
    const int64_t n_rows = 3 * (2 * (int64_t)p->profile + 1);
    const int rc = guarded(p, [&] {
        p->d_rptab.reserve(sizeof(unsigned long long) * 3 * (size_t)n_rows);
        hipLaunchKernelGGL(readpos_reduce_kernel, dim3((unsigned)n_rows), dim3(256), 0, p->stream, readpos_table(p), p->thr_packed,
                           p->d_rptab.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        return HM_OK;
    });
    if (rc != HM_OK) return rc;
    return compact_rows(p, ReadPosSel{p->d_rptab.as<unsigned long long>(), p->profile, min_calls}, 0, n_rows, out, cap, no_hook, no_hook);
}

int64_t hm_pileup_readpos_histograms(hm_pileup_t* p, uint64_t* hist, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (!p->profile || p->seq_off.empty()) return pfail(p, HM_ESTATE, "hm_pileup_readpos_histograms without option profile (then hm_pileup_set_reference)");
    const int64_t n = (int64_t)readpos_counters(p);
    if (!hist || cap < n) return n;
    const int rc = guarded(p, [&] {
        HIP_TRY(hipMemcpyAsync(hist, p->d_rphist.p, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
    return rc != HM_OK ? rc : n;
}

int hm_pileup_add_readpos(hm_pileup_t* p, const uint64_t* hist, int64_t n) {
    if (!p || !hist) return HM_EINVAL;
    if (!p->profile || p->seq_off.empty()) return pfail(p, HM_ESTATE, "hm_pileup_add_readpos without option profile (then hm_pileup_set_reference)");
    if (n != (int64_t)readpos_counters(p)) return pfail(p, HM_EINVAL, "hm_pileup_add_readpos: 3 x (2 x profile + 1) x 256 counters expected");
    return guarded(p, [&] {
        p->d_rpadd.reserve(sizeof(uint64_t) * (size_t)n);
        HIP_TRY(hipMemcpyAsync(p->d_rpadd.p, hist, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, p->stream));
        hipLaunchKernelGGL(readpos_add_kernel, dim3(grid_for(n, 1024)), dim3(TPB), 0, p->stream, p->d_rpadd.as<unsigned long long>(), n,
                           p->d_rphist.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
}

int hm_readpos_stats(const hm_readpos_t* w, double out[2]) {
    if (!w || !out) return HM_EINVAL;
    const uint64_t n = w->n_m + w->n_u;
    if (!n) return HM_EINVAL;
    out[0] = 100.0 * (double)w->n_m / (double)n;  // cov.bed's fourth column
    out[1] = (double)w->sum_ml / (double)n;
    return HM_OK;
}

int hm_linkage_stats(const hm_linkage_t* w, double out[2]) {
    if (!w || !out) return HM_EINVAL;
    const uint64_t n = w->n_uu + w->n_um + w->n_mu + w->n_mm;
    if (!n) return HM_EINVAL;
    out[0] = (double)(w->n_uu + w->n_mm) / (double)n;
    const uint64_t m1 = w->n_mm + w->n_mu, u1 = w->n_um + w->n_uu, m2 = w->n_mm + w->n_um, u2 = w->n_mu + w->n_uu;  // the margins
    // the numerator as an exact integer (counts below 2^63): the two products may agree in all the digits a double holds
    const __int128 num = (__int128)w->n_mm * (__int128)w->n_uu - (__int128)w->n_mu * (__int128)w->n_um;
    out[1] = (!m1 || !u1 || !m2 || !u2) ? std::nan("") : (double)num / std::sqrt((double)m1 * (double)u1 * (double)m2 * (double)u2);
    return HM_OK;
}

int hm_pattern_stats(const hm_pattern_t* w, double out[4]) {
    if (!w || !out || w->k < 2 || w->k > 4 || !w->n) return HM_EINVAL;
    const uint32_t bins = 1u << w->k;
    uint64_t n = 0;
    for (uint32_t b = 0; b < bins; ++b) n += w->counts[b];
    if (n != w->n) return HM_EINVAL;
    const double dn = (double)n;
    double h = 0.0, sq = 0.0;
    uint64_t meth = 0;
    for (uint32_t b = 0; b < bins; ++b) {
        const uint32_t c = w->counts[b];
        if (!c) continue;
        const double f = (double)c / dn;
        h += f * std::log2(f);
        sq += f * f;
        meth += (uint64_t)__builtin_popcount(b) * c;
    }
    out[0] = (0.0 - h) / (double)w->k;  // 0 - h: one pattern gives +0.0
    out[1] = 1.0 - sq;
    out[2] = 1.0 - (double)((uint64_t)w->counts[0] + w->counts[bins - 1]) / dn;
    out[3] = 100.0 * (double)meth / ((double)w->k * dn);
    return HM_OK;
}

int64_t hm_pileup_fetch_asm(hm_pileup_t* p, const void* pcov1, const void* ncov1, const void* pcov2, const void* ncov2,
                            const void* key, int64_t plane_base, int64_t lo, int64_t hi, int32_t min_cov, hm_asm_t* out,
                            int64_t cap) {
    if (!p) return HM_EINVAL;
    AsmPlanes s;
    const int rc = asm_planes(p, "hm_pileup_fetch_asm", pcov1, ncov1, pcov2, ncov2, key, plane_base, lo, hi, min_cov, s);
    if (rc != HM_OK) return rc;
    if (hi == lo) return 0;
    return compact_rows(
        p, AsmSel<ASM_ALL>{s, plane_base, min_cov, 0u}, lo, hi, out, cap, [&] { ensure_lfact(p); },
        [&](hm_asm_t* rows, int64_t total) { test_rows(p, rows, total); });
}

// ---- `pileup -H -A -Q` ------------------------------------------------------------------------------------------------------------
int64_t hm_pileup_asm_histogram(hm_pileup_t* p, const void* pcov1, const void* ncov1, const void* pcov2, const void* ncov2,
                                const void* key, int64_t plane_base, int64_t lo, int64_t hi, int32_t min_cov, uint64_t* bins,
                                hm_asm_t* big, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (!bins) return pfail(p, HM_EINVAL, "hm_pileup_asm_histogram: no bins");
    AsmPlanes s;
    const int rc = asm_planes(p, "hm_pileup_asm_histogram", pcov1, ncov1, pcov2, ncov2, key, plane_base, lo, hi, min_cov, s);
    if (rc != HM_OK) return rc;
    if (hi == lo) return 0;
    const int64_t n_big = guarded(p, [&]() -> int64_t {
        const int64_t n = stage_counted_rows(
            p, "histogram", AsmSel<ASM_BIG>{s, plane_base, min_cov, 0u}, lo, hi, p->d_arows,
            [&](int64_t nblk, int32_t* block_big) {
                p->d_abins.reserve(HM_ASM_BINS * sizeof(unsigned long long));
                HIP_TRY(hipMemsetAsync(p->d_abins.p, 0, HM_ASM_BINS * sizeof(unsigned long long), p->stream));
                hipLaunchKernelGGL(asm_hist_kernel, dim3((unsigned)nblk), dim3(TPB), 0, p->stream, s.p1, s.n1, s.p2, s.n2, s.ky, lo, hi,
                                   min_cov, p->d_abins.as<unsigned long long>(), block_big);
            },
            [&](int64_t n) {
                if (!fits(n, big, cap)) return false;
                ensure_lfact(p);
                return true;
            },
            [&](hm_asm_t* rows, int64_t n) { test_rows(p, rows, n); });
        return fits(n, big, cap) ? rows_to_host(p, p->d_arows, big, n) : n;
    });
    if (n_big < 0 || n_big > cap || (n_big && !big)) return n_big;
    // the range's non-empty bins (few next to HM_ASM_BINS) come to the host compacted and are added there
    std::vector<hm_asm_bin_t> tab;
    const int64_t n_tab = nonempty_bins(p, [&](int64_t n) { tab.resize((size_t)n); return tab.data(); }, false);
    if (n_tab < 0) return n_tab;
    for (const hm_asm_bin_t& t : tab) bins[t.bin] += t.count;
    return n_big;
}

int64_t hm_pileup_asm_bin_pvalues(hm_pileup_t* p, const uint64_t* bins, hm_asm_bin_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (!bins) return pfail(p, HM_EINVAL, "hm_pileup_asm_bin_pvalues: no bins");
    // a tested locus has no haplotype total of 0: pair 0 on either side is no tuple the histogram counts
    for (size_t c = 0; c < 3; ++c)
        for (size_t u = 0; u < ASM_PAIRS; ++u)
            if (bins[(c * ASM_PAIRS + u) * ASM_PAIRS] || bins[c * ASM_PAIRS * ASM_PAIRS + u])
                return pfail(p, HM_EINVAL, "hm_pileup_asm_bin_pvalues: a non-empty bin of a haplotype without calls");
    const int rc = guarded(p, [&] {
        p->d_abins.reserve(HM_ASM_BINS * sizeof(unsigned long long));
        HIP_TRY(hipMemcpyAsync(p->d_abins.p, bins, HM_ASM_BINS * sizeof(uint64_t), hipMemcpyHostToDevice, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        return HM_OK;
    });
    return rc != HM_OK ? rc : nonempty_bins(p, [&](int64_t n) { return n > cap ? nullptr : out; }, true);
}

int hm_asm_qvalues(hm_asm_bin_t* tab, int64_t n_tab, const hm_asm_t* big, int64_t n_big, double* big_q, uint64_t m[3]) {
    if (n_tab < 0 || n_big < 0 || (n_tab && !tab) || (n_big && (!big || !big_q)) || !m) return HM_EINVAL;
    const auto is_p = [](double v) { return v >= DBL_MIN && v <= 1.0; };  // false for NaN
    for (int64_t i = 0; i < n_tab; ++i)
        if (tab[i].bin >= (uint32_t)HM_ASM_BINS || (i && tab[i].bin <= tab[i - 1].bin) || tab[i].count == 0 || !is_p(tab[i].pvalue))
            return HM_EINVAL;
    for (int64_t i = 0; i < n_big; ++i) {
        const hm_asm_t& b = big[i];
        if (b.motif > 3u || (b.pcov1 | b.ncov1 | b.pcov2 | b.ncov2) < 0 || !is_p(b.pvalue) ||
            ((int64_t)b.pcov1 + b.ncov1 < ASM_T && (int64_t)b.pcov2 + b.ncov2 < ASM_T))
            return HM_EINVAL;
    }
    std::vector<BhEntry> ent;
    int64_t i = 0;
    for (uint32_t c = 0; c < 3; ++c) {
        ent.clear();
        m[c] = 0;
        for (; i < n_tab && tab[i].bin / (ASM_PAIRS * ASM_PAIRS) == c; ++i) {  // (ascending in bin: the contexts follow each other)
            ent.push_back(BhEntry{tab[i].pvalue, tab[i].count, i});
            m[c] += tab[i].count;
        }
        for (int64_t j = 0; j < n_big; ++j)
            if (std::min(big[j].motif, 2u) == c) {
                ent.push_back(BhEntry{big[j].pvalue, 1, ~j});
                ++m[c];
            }
        bh_qvalues(ent, m[c], [&](int64_t where, double q) {
            if (where >= 0) tab[where].qvalue = q;
            else big_q[~where] = q;
        });
    }
    return HM_OK;
}

int64_t hm_pileup_fetch_asm_q(hm_pileup_t* p, const void* pcov1, const void* ncov1, const void* pcov2, const void* ncov2,
                              const void* key, int64_t plane_base, int64_t lo, int64_t hi, int32_t min_cov, const hm_asm_bin_t* tab,
                              int64_t n_tab, const hm_asm_t* big, const double* big_q, int64_t n_big, hm_asmq_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (n_tab < 0 || n_big < 0 || (n_tab && !tab) || (n_big && (!big || !big_q))) return pfail(p, HM_EINVAL, "hm_pileup_fetch_asm_q: bad table");
    AsmPlanes s;
    const int rc = asm_planes(p, "hm_pileup_fetch_asm_q", pcov1, ncov1, pcov2, ncov2, key, plane_base, lo, hi, min_cov, s);
    if (rc != HM_OK) return rc;
    if (hi == lo) return 0;
    hipStream_t st = p->stream;
    return guarded(p, [&]() -> int64_t {  // hm_pileup_fetch_asm's rows in d_arows, then q next to each in d_rows
        const int64_t total = stage_rows(
            p, AsmSel<ASM_ALL>{s, plane_base, min_cov, 0u}, lo, hi, p->d_arows,
            [&](int64_t n) {
                if (!fits(n, out, cap)) return false;
                ensure_lfact(p);
                if (n_tab) {
                    p->d_atab.reserve(sizeof(hm_asm_bin_t) * (size_t)n_tab);
                    HIP_TRY(hipMemcpyAsync(p->d_atab.p, tab, sizeof(hm_asm_bin_t) * (size_t)n_tab, hipMemcpyHostToDevice, st));
                }
                if (n_big) {
                    p->d_abig.reserve(sizeof(hm_asm_t) * (size_t)n_big);
                    p->d_abigq.reserve(sizeof(double) * (size_t)n_big);
                    HIP_TRY(hipMemcpyAsync(p->d_abig.p, big, sizeof(hm_asm_t) * (size_t)n_big, hipMemcpyHostToDevice, st));
                    HIP_TRY(hipMemcpyAsync(p->d_abigq.p, big_q, sizeof(double) * (size_t)n_big, hipMemcpyHostToDevice, st));
                }
                return true;
            },
            [&](hm_asm_t* rows, int64_t n) {
                test_rows(p, rows, n);
                p->d_rows.reserve(sizeof(hm_asmq_t) * (size_t)n);
                hipLaunchKernelGGL(asm_q_write_kernel, row_grid(n), dim3(TPB), 0, st, rows, n, p->d_atab.as<hm_asm_bin_t>(), n_tab,
                                   p->d_abig.as<hm_asm_t>(), p->d_abigq.as<double>(), n_big, p->d_rows.as<hm_asmq_t>());
            });
        return fits(total, out, cap) ? rows_to_host(p, p->d_rows, out, total) : total;
    });
}

// ---- `pileup -H -A -G` ------------------------------------------------------------------------------------------------------------
int64_t hm_pileup_fetch_asm_regions(hm_pileup_t* p, const void* pcov1, const void* ncov1, const void* pcov2, const void* ncov2,
                                    const void* key, int64_t plane_base, int64_t lo, int64_t hi, int32_t min_cov, int32_t ctx,
                                    double max_p, int64_t max_gap, int32_t min_loci, int32_t keep_edges, int64_t* n_ctx_rows,
                                    hm_asm_region_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (ctx < 0 || ctx > 2) return pfail(p, HM_EINVAL, "hm_pileup_fetch_asm_regions: ctx must be 0, 1 or 2");
    if (!(max_p > 0.0 && max_p <= 1.0)) return pfail(p, HM_EINVAL, "hm_pileup_fetch_asm_regions: max_p must be in (0, 1]");
    if (max_gap < 1 || min_loci < 1) return pfail(p, HM_EINVAL, "hm_pileup_fetch_asm_regions: max_gap and min_loci must be >= 1");
    AsmPlanes s;
    const int rc = asm_planes(p, "hm_pileup_fetch_asm_regions", pcov1, ncov1, pcov2, ncov2, key, plane_base, lo, hi, min_cov, s);
    if (rc != HM_OK) return rc;
    if (n_ctx_rows) *n_ctx_rows = 0;
    if (hi == lo) return 0;
    return guarded(p, [&]() -> int64_t {
        const int64_t R = stage_rows(  // the context's rows, tested, stay in d_arows
            p, AsmSel<ASM_CTX>{s, plane_base, min_cov, (uint32_t)ctx}, lo, hi, p->d_arows,
            [&](int64_t) {
                ensure_lfact(p);
                return true;
            },
            [&](hm_asm_t* rows, int64_t n) { test_rows(p, rows, n); });
        if (R <= 0) return R;
        if (n_ctx_rows) *n_ctx_rows = R;
        const RegionSel<AsmChain> chains{p->d_arows.as<hm_asm_t>(), R, RegionRule{max_p, max_gap, min_loci, keep_edges != 0}, (uint32_t)ctx};
        return compact_rows(p, chains, 0, R, out, cap, no_hook, no_hook);
    });
}

// ---- `pileup -D` ----------------------------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// the three launches of the row-scan skeleton over n >= 1 elements; d_dagg holds the aggregates
template <class Sc>
void row_scan(hm_pileup* p, const Sc& sc, int64_t n) {
    using T = typename Sc::T;
    const int64_t nagg = (n + SCAN_ROWS - 1) / SCAN_ROWS;
    p->d_dagg.reserve(sizeof(T) * (size_t)nagg);
    T* agg = p->d_dagg.as<T>();
    hipLaunchKernelGGL(rowscan_reduce_kernel<Sc>, dim3((unsigned)nagg), dim3(TPB), 0, p->stream, sc, n, agg);
    hipLaunchKernelGGL(rowscan_carry_kernel<Sc>, dim3(1), dim3(1024), 0, p->stream, sc, agg, nagg);
    hipLaunchKernelGGL(rowscan_apply_kernel<Sc>, dim3((unsigned)nagg), dim3(TPB), 0, p->stream, sc, n, agg);
    HIP_TRY(hipGetLastError());
}

// the combination of all n >= 1 elements, without the re-scan: the reduce, then the carry kernel over the aggregates and one
// identity behind them, whose exclusive scan is the total
template <class Sc>
typename Sc::T row_reduce(hm_pileup* p, const Sc& sc, int64_t n) {
    using T = typename Sc::T;
    const int64_t nagg = (n + SCAN_ROWS - 1) / SCAN_ROWS;
    p->d_dagg.reserve(sizeof(T) * (size_t)(nagg + 1));
    T* agg = p->d_dagg.as<T>();
    T total = Sc::identity();
    HIP_TRY(hipMemcpyAsync(agg + nagg, &total, sizeof(T), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    hipLaunchKernelGGL(rowscan_reduce_kernel<Sc>, dim3((unsigned)nagg), dim3(TPB), 0, p->stream, sc, n, agg);
    hipLaunchKernelGGL(rowscan_carry_kernel<Sc>, dim3(1), dim3(1024), 0, p->stream, sc, agg, nagg + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&total, agg + nagg, sizeof(T), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return total;
}

// Both `-D` entry points, in the name of `who`: pass `pass` over the piece that `part` describes, or with no `part` the whole
// range, which is the one-piece segments pass with no row before or behind it: nothing of a piece is then copied to the host.
// *n_rows takes the number of the context's rows.  With `state_sums` (`pileup -D -Y`, the segments pass only) the rows' states are
// summed instead of cut into segments: no heads, no segment, nothing of the piece but the six sums comes back; -> R.
int64_t fetch_domains(hm_pileup* p, const std::string& who, const void* pcov, const void* ncov, const void* key, int64_t plane_base,
                      int64_t lo, int64_t hi, int32_t ctx, int64_t A, int64_t B, int64_t S, int64_t max_gap, int32_t pass,
                      hm_domain_part_t* part, int64_t* n_rows, hm_domain_t* out, int64_t cap, int64_t* state_sums = nullptr) {
    if (lo < 0 || hi < lo) return pfail(p, HM_EINVAL, who + ": bad range");
    if (ctx < 0 || ctx > 2) return pfail(p, HM_EINVAL, who + ": ctx must be 0, 1 or 2");
    if (A < 1 || A > DOM_W || B > -1 || B < -DOM_W || S < 0 || S > DOM_W)
        return pfail(p, HM_EINVAL, who + ": A must be in (0, 2^24], B in [-2^24, 0), S in [0, 2^24]");
    if (max_gap < 1) return pfail(p, HM_EINVAL, who + ": max_gap must be >= 1");
    RangePlanes s;
    if (!range_planes(p, pcov, ncov, key, plane_base, s)) return HM_ESTATE;
    if ((!pcov || !ncov || !key) && !p->seq_off.empty() && hi > p->seq_off.back())  // an own plane ends with the reference
        return pfail(p, HM_EINVAL, who + ": range past the reference");
    const bool carried = pass != HM_DOMAIN_PASS_SUMMARY;
    const bool has_prev = part && carried && part->has_prev, has_next = part && pass == HM_DOMAIN_PASS_SEGMENTS && part->has_next;
    constexpr int64_t DOM_D = int64_t(1) << 46;  // every d lies within +-2^46
    if (has_prev && (part->prev_d < -DOM_D || part->prev_d > DOM_D)) return pfail(p, HM_EINVAL, who + ": prev_d outside [-2^46, 2^46]");
    if (has_prev && (part->prev_gpos < 0 || part->prev_gpos >= plane_base + lo))
        return pfail(p, HM_EINVAL, who + ": prev_gpos must lie below the piece's first locus");
    if (has_next && part->next_gpos < plane_base + hi) return pfail(p, HM_EINVAL, who + ": next_gpos must lie behind the piece's last locus");
    if (has_next && part->last_state != 0 && part->last_state != 1) return pfail(p, HM_EINVAL, who + ": last_state must be 0 or 1");
    if (n_rows) *n_rows = 0;
    if (state_sums) std::fill(state_sums, state_sums + 6, int64_t(0));
    if (hi == lo) return 0;
    hipStream_t st = p->stream;
    const DomRule rule{A, B, S, max_gap};
    const bool piece_out = part && !state_sums;  // a piece's ends, d_last and summary go back to the caller
    return guarded(p, [&]() -> int64_t {
        // the context's rows with their sums and states stay on the device
        const int64_t R = stage_rows(p, DomRowSel{s, plane_base, (uint32_t)ctx}, lo, hi, p->d_drows, [](int64_t) { return true; }, no_hook);
        if (R <= 0) return R;
        if ((R + SCAN_ROWS - 1) / SCAN_ROWS >= (int64_t(1) << 31) - 1) return pfail(p, HM_EINVAL, "range too large: fetch per sequence");
        p->d_dsums.reserve(sizeof(DomSum) * (size_t)R);
        p->d_dcode.reserve((size_t)R);
        p->d_dstate.reserve((size_t)R);
        p->d_dlast.reserve(8);
        const DomRow* rows = p->d_drows.as<DomRow>();
        const uint8_t* state = p->d_dstate.as<uint8_t>();
        DomRow ends[2];  // a piece's first and last row
        if (piece_out) {
            HIP_TRY(hipMemcpyAsync(&ends[0], rows, sizeof(DomRow), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(&ends[1], rows + (R - 1), sizeof(DomRow), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        DomFwd fwd{rows, R, rule, p->d_dsums.as<DomSum>(), p->d_dcode.as<uint8_t>(), !carried, has_prev, has_prev ? part->prev_gpos : 0,
                   has_prev ? part->prev_d : 0, DomFwd::KEEP, p->d_dlast.as<int64_t>()};
        if (pass == HM_DOMAIN_PASS_SUMMARY) {  // rows 1 .. R - 1 composed; nothing is stored
            const DomFwd::T f = row_reduce(p, fwd, R);
            part->c = f.c;
            part->lo = f.lo;
            part->hi = f.hi;
        } else {
            if (pass == HM_DOMAIN_PASS_SEGMENTS) fwd.last_code = has_next ? part->last_state : -1;
            row_scan(p, fwd, R);
            if (piece_out) {
                HIP_TRY(hipMemcpyAsync(&part->d_last, p->d_dlast.p, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
            }
            const DomBwd bwd{p->d_dcode.as<uint8_t>(), R, p->d_dstate.as<uint8_t>()};
            if (pass == HM_DOMAIN_PASS_CODES) part->back = row_reduce(p, bwd, R);  // the last row's code is KEEP: the transitions inside
            else row_scan(p, bwd, R);
        }
        if (n_rows) *n_rows = R;
        if (state_sums) {
            static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the sums are added as unsigned long long");
            p->d_dstate_sums.reserve(6 * sizeof(int64_t));
            HIP_TRY(hipMemsetAsync(p->d_dstate_sums.p, 0, 6 * sizeof(int64_t), st));
            hipLaunchKernelGGL(domain_sums_kernel, dim3(grid_for(R, DOM_SUMS_WGS)), dim3(TPB), 0, st, rows, state, R,
                               p->d_dstate_sums.as<unsigned long long>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(state_sums, p->d_dstate_sums.p, 6 * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return R;
        }
        if (part) {
            part->first_gpos = ends[0].gpos;
            part->last_gpos = ends[1].gpos;
            part->e_first = (int64_t)std::min(ends[0].pcov, DOM_COV) * A + (int64_t)std::min(ends[0].ncov, DOM_COV) * B;
        }
        if (pass != HM_DOMAIN_PASS_SEGMENTS) return R;
        const bool first_break = !has_prev || ends[0].gpos - part->prev_gpos > max_gap, last_break = !has_next || part->next_gpos - ends[1].gpos > max_gap;
        const int64_t n_seg = stage_rows(
            p, DomHeadSel{rows, state, max_gap}, 0, R, p->d_dheads, [&](int64_t n) { return fits(n, out, cap); },
            [&](int64_t* heads, int64_t n) {
                p->d_rows.reserve(sizeof(hm_domain_t) * (size_t)n);
                hipLaunchKernelGGL(domain_build_part_kernel, row_grid(n), dim3(TPB), 0, st, rows, p->d_dsums.as<DomSum>(), state, heads, n, R,
                                   rule, (uint32_t)ctx, first_break, last_break, p->d_rows.as<hm_domain_t>());
            });
        return fits(n_seg, out, cap) ? rows_to_host(p, p->d_rows, out, n_seg) : n_seg;
    });
}

}  // namespace

extern "C" {

int64_t hm_pileup_fetch_domains(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                                int64_t hi, int32_t ctx, int64_t A, int64_t B, int64_t S, int64_t max_gap, int64_t* n_ctx_rows,
                                hm_domain_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    return fetch_domains(p, "hm_pileup_fetch_domains", pcov, ncov, key, plane_base, lo, hi, ctx, A, B, S, max_gap, HM_DOMAIN_PASS_SEGMENTS,
                         nullptr, n_ctx_rows, out, cap);
}

int64_t hm_pileup_fetch_domains_part(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                                     int64_t hi, int32_t ctx, int64_t A, int64_t B, int64_t S, int64_t max_gap, int32_t pass,
                                     hm_domain_part_t* part, hm_domain_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    const std::string who = "hm_pileup_fetch_domains_part";
    if (!part) return pfail(p, HM_EINVAL, who + ": no part");
    if (pass < HM_DOMAIN_PASS_SUMMARY || pass > HM_DOMAIN_PASS_SEGMENTS) return pfail(p, HM_EINVAL, who + ": pass must be 0, 1 or 2");
    return fetch_domains(p, who, pcov, ncov, key, plane_base, lo, hi, ctx, A, B, S, max_gap, pass, part, &part->n_rows, out, cap);
}

int64_t hm_pileup_domain_sums(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                              int64_t hi, int32_t ctx, int64_t A, int64_t B, int64_t S, int64_t max_gap, int64_t sums[6]) {
    if (!p) return HM_EINVAL;
    if (!sums) return pfail(p, HM_EINVAL, "hm_pileup_domain_sums: no sums");
    return fetch_domains(p, "hm_pileup_domain_sums", pcov, ncov, key, plane_base, lo, hi, ctx, A, B, S, max_gap, HM_DOMAIN_PASS_SEGMENTS,
                         nullptr, nullptr, nullptr, 0, sums);
}

int64_t hm_pileup_domain_sums_part(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                                   int64_t hi, int32_t ctx, int64_t A, int64_t B, int64_t S, int64_t max_gap,
                                   const hm_domain_part_t* part, int64_t sums[6]) {
    if (!p) return HM_EINVAL;
    const std::string who = "hm_pileup_domain_sums_part";
    if (!part) return pfail(p, HM_EINVAL, who + ": no part");
    if (!sums) return pfail(p, HM_EINVAL, who + ": no sums");
    hm_domain_part_t carry = *part;  // only read: the pass's outputs stay here
    return fetch_domains(p, who, pcov, ncov, key, plane_base, lo, hi, ctx, A, B, S, max_gap, HM_DOMAIN_PASS_SEGMENTS, &carry, nullptr,
                         nullptr, 0, sums);
}

int hm_domain_scores(double level_lo, double level_hi, double penalty, int64_t* A, int64_t* B, int64_t* S) {
    if (!A || !B || !S) return HM_EINVAL;
    if (!(level_lo > 0.0 && level_lo < level_hi && level_hi < 1.0) || !(penalty >= 0.0)) return HM_EINVAL;
    const double a = 65536.0 * std::log(level_hi / level_lo), b = 65536.0 * std::log((1.0 - level_hi) / (1.0 - level_lo)),
                 s = 65536.0 * penalty;
    if (!(a <= (double)DOM_W && b >= -(double)DOM_W && s <= (double)DOM_W)) return HM_EINVAL;  // also what llround could not hold
    const int64_t ia = std::llround(a), ib = std::llround(b);
    if (ia < 1 || ib > -1) return HM_EINVAL;  // levels so close that a weight rounds to 0
    *A = ia;
    *B = ib;
    *S = std::llround(s);
    return HM_OK;
}

int hm_domain_refit(const int64_t sums[6], double penalty, double* level_lo, double* level_hi) {
    if (!sums || !level_lo || !level_hi || !(penalty >= 0.0)) return HM_EINVAL;
    for (int k = 0; k < 6; ++k)
        if (sums[k] < 0) return HM_EINVAL;
    const int64_t P0 = sums[0], N0 = sums[1], R0 = sums[2], P1 = sums[3], N1 = sums[4], R1 = sums[5];
    if (R0 == 0 || R1 == 0 || P0 + N0 <= 0 || P1 + N1 <= 0) return HM_EDATA;  // one state; (a row has pcov + ncov > 0)
    constexpr double EPS = 1e-6;
    const double lo = std::min(std::max((double)P0 / (double)(P0 + N0), EPS), 1.0 - EPS);
    const double hi = std::min(std::max((double)P1 / (double)(P1 + N1), EPS), 1.0 - EPS);
    int64_t A, B, S;
    if (!(lo < hi) || hm_domain_scores(lo, hi, penalty, &A, &B, &S) != HM_OK) return HM_EDATA;
    *level_lo = lo;
    *level_hi = hi;
    return HM_OK;
}

// ---- `pileup -B / -e` ---------------------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

// P(X >= k), X ~ Binomial(n, e), 0 < e < 1, 0 < k <= n: the sum the header spells out
double binomial_tail(int64_t k, int64_t n, double log_e, double log1m_e) {
    const std::vector<double>& tab = host_lfact();
    auto lf = [&](int64_t j) { return j < LFACT_N ? tab[(size_t)j] : std::lgamma((double)j + 1.0); };
    const double lfn = lf(n);
    double p = 0.0;
    for (int64_t x = k; x <= n; ++x) p += std::exp(((lfn - lf(x)) - lf(n - x)) + ((double)x * log_e + (double)(n - x) * log1m_e));
    return p > 1.0 ? 1.0 : p >= DBL_MIN ? p : DBL_MIN;
}

}  // namespace

extern "C" {

int hm_pileup_control_sums(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t lo, int64_t hi,
                           uint64_t sums[6]) {
    if (!p) return HM_EINVAL;
    if (lo < 0 || hi < lo || !sums) return pfail(p, HM_EINVAL, "hm_pileup_control_sums: bad argument");
    RangePlanes s;
    int64_t base = 0;
    if (!range_planes(p, pcov, ncov, key, base, s)) return HM_ESTATE;
    std::fill(sums, sums + 6, uint64_t(0));
    if (hi == lo) return HM_OK;
    return guarded(p, [&] {
        hipStream_t st = p->stream;
        p->d_ssums.reserve(6 * sizeof(unsigned long long));
        HIP_TRY(hipMemsetAsync(p->d_ssums.p, 0, 6 * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(sites_sums_kernel, dim3(grid_for(hi - lo, 1024)), dim3(TPB), 0, st, s.pc, s.nc, s.ky, lo, hi,
                           p->d_ssums.as<unsigned long long>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(sums, p->d_ssums.p, 6 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return HM_OK;
    });
}

int64_t hm_pileup_site_histogram(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base,
                                 int64_t lo, int64_t hi, uint64_t* bins, hm_locus_t* big, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (lo < 0 || hi < lo || !bins) return pfail(p, HM_EINVAL, "hm_pileup_site_histogram: bad argument");
    RangePlanes s;
    if (!range_planes(p, pcov, ncov, key, plane_base, s)) return HM_ESTATE;
    if (hi == lo) return 0;
    return guarded(p, [&]() -> int64_t {
        hipStream_t st = p->stream;
        std::vector<uint64_t> h((size_t)HM_SITE_BINS);
        const auto bins_to_host = [&] { HIP_TRY(hipMemcpyAsync(h.data(), p->d_sbins.p, HM_SITE_BINS * sizeof(uint64_t), hipMemcpyDeviceToHost, st)); };
        const int64_t n_big = stage_counted_rows(
            p, "histogram", SitesBigSel{s, plane_base}, lo, hi, p->d_sbig,
            [&](int64_t nblk, int32_t* block_big) {
                p->d_sbins.reserve(HM_SITE_BINS * sizeof(unsigned long long));
                HIP_TRY(hipMemsetAsync(p->d_sbins.p, 0, HM_SITE_BINS * sizeof(unsigned long long), st));
                // <= 512 workgroups of 48 KB LDS (two per CU), more only to keep a workgroup below 2^19 blocks = 2^31 loci (its LDS counters)
                const int64_t grid = std::max(std::min<int64_t>(nblk, 512), (nblk + (int64_t(1) << 19) - 1) >> 19);
                hipLaunchKernelGGL(sites_hist_kernel, dim3((unsigned)grid), dim3(TPB), 0, st, s.pc, s.nc, s.ky, lo, hi, nblk,
                                   p->d_sbins.as<unsigned long long>(), block_big);
            },
            [&](int64_t n) {  // the bins' copy is queued before the list's write
                if (!fits(n, big, cap)) return false;
                bins_to_host();
                return true;
            },
            no_hook);
        if (n_big < 0 || n_big > cap || (n_big && !big)) return n_big;
        if (n_big) rows_to_host(p, p->d_sbig, big, n_big);  // the list, and with it the bins, are on the host when this returns
        else {
            bins_to_host();
            HIP_TRY(hipStreamSynchronize(st));
        }
        for (size_t i = 0; i < h.size(); ++i) bins[i] += h[i];
        return n_big;
    });
}

int hm_sites_table(const double rates[3], const uint64_t* bins, const hm_locus_t* big, int64_t n_big, double* ptab, double* qtab,
                   double* big_p, double* big_q, uint64_t m[3]) {
    if (!rates || !bins || !ptab || !qtab || !m || n_big < 0 || (n_big && (!big || !big_p || !big_q))) return HM_EINVAL;
    for (int c = 0; c < 3; ++c)
        if (!std::isnan(rates[c]) && !(rates[c] >= 0.0 && rates[c] <= 1.0)) return HM_EINVAL;
    for (int t = 0; t < HM_SITE_BINS; ++t)
        if (bins[t] && ((t & 255) > ((t >> 8) & 255) || ((t >> 8) & 255) == 0)) return HM_EINVAL;
    for (int64_t i = 0; i < n_big; ++i)
        if (big[i].motif > 2u || big[i].pcov < 0 || big[i].ncov < 0 || (int64_t)big[i].pcov + big[i].ncov < SITE_N) return HM_EINVAL;
    const double nan = std::nan("");
    std::fill(ptab, ptab + HM_SITE_BINS, nan);
    std::fill(qtab, qtab + HM_SITE_BINS, nan);
    std::fill(big_p, big_p + n_big, nan);
    std::fill(big_q, big_q + n_big, nan);
    std::vector<BhEntry> ent;  // the loci that share one p: a bin (where >= 0: its index) or one big locus (where < 0: ~index)
    for (int c = 0; c < 3; ++c) {
        m[c] = std::accumulate(bins + c * SITE_N * SITE_N, bins + (c + 1) * SITE_N * SITE_N, uint64_t(0));
        for (int64_t i = 0; i < n_big; ++i) m[c] += big[i].motif == (uint32_t)c;
        const double e = rates[c];
        if (std::isnan(e)) continue;
        const double log_e = std::log(e), log1m_e = std::log1p(-e);
        auto pvalue = [&](int64_t k, int64_t n) { return k == 0 || e == 1.0 ? 1.0 : e == 0.0 ? DBL_MIN : binomial_tail(k, n, log_e, log1m_e); };
        ent.clear();
        for (int n = 0; n < SITE_N; ++n)
            for (int k = 0; k <= n; ++k) {
                const int t = (c * SITE_N + n) * SITE_N + k;
                ptab[t] = pvalue(k, n);
                if (bins[t]) ent.push_back(BhEntry{ptab[t], bins[t], t});
            }
        for (int64_t i = 0; i < n_big; ++i) {
            if (big[i].motif != (uint32_t)c) continue;
            // an organelle's loci repeat their counts: the previous locus of the context with the same (k, n) has the value
            const int64_t j = ent.empty() || ent.back().where >= 0 ? -1 : ~ent.back().where;
            big_p[i] = j >= 0 && big[j].pcov == big[i].pcov && big[j].ncov == big[i].ncov
                           ? big_p[j] : pvalue(big[i].pcov, (int64_t)big[i].pcov + big[i].ncov);
            ent.push_back(BhEntry{big_p[i], 1, ~i});
        }
        bh_qvalues(ent, m[c], [&](int64_t where, double q) {
            if (where >= 0) qtab[where] = q;
            else big_q[~where] = q;
        });
    }
    return HM_OK;
}

int64_t hm_pileup_fetch_sites(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                              int64_t hi, int32_t ctx_mask, const double* ptab, const double* qtab, const hm_locus_t* big,
                              const double* big_p, const double* big_q, int64_t n_big, hm_site_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    if (lo < 0 || hi < lo || !ptab || !qtab || n_big < 0 || (n_big && (!big || !big_p || !big_q)) || (ctx_mask & ~7))
        return pfail(p, HM_EINVAL, "hm_pileup_fetch_sites: bad argument");
    RangePlanes s;
    if (!range_planes(p, pcov, ncov, key, plane_base, s)) return HM_ESTATE;
    if (hi == lo) return 0;
    hipStream_t st = p->stream;
    const size_t tab_bytes = HM_SITE_BINS * sizeof(double);
    return guarded(p, [&]() -> int64_t {
        p->d_stab.reserve(2 * tab_bytes);  // before the selection takes their addresses
        p->d_sbig.reserve(sizeof(hm_locus_t) * (size_t)n_big);
        p->d_sbigpq.reserve(2 * sizeof(double) * (size_t)n_big);
        const SitesSel rows{s, plane_base, (uint32_t)ctx_mask, p->d_stab.as<double>(), p->d_sbig.as<hm_locus_t>(), p->d_sbigpq.as<double>(), n_big};
        return compact_rows(
            p, rows, lo, hi, out, cap,
            [&] {
                HIP_TRY(hipMemcpyAsync(p->d_stab.p, ptab, tab_bytes, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(p->d_stab.as<char>() + tab_bytes, qtab, tab_bytes, hipMemcpyHostToDevice, st));
                if (!n_big) return;
                HIP_TRY(hipMemcpyAsync(p->d_sbig.p, big, sizeof(hm_locus_t) * (size_t)n_big, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(p->d_sbigpq.p, big_p, sizeof(double) * (size_t)n_big, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpyAsync(p->d_sbigpq.as<double>() + n_big, big_q, sizeof(double) * (size_t)n_big, hipMemcpyHostToDevice, st));
            },
            no_hook);
    });
}

}  // extern "C"

// ---- the interval fetches: `pileup -R / -J` and, further down, `regiondiff` ---------------------------------------------------------
// One skeleton: check the intervals, stage them, build the index (the block sums, then their scan), one query kernel, the sums
// back.  A fetch plugs in its scan (RegionScan, SampleIvScan), its two kernels and its own argument checks.
namespace {

// the caller's n intervals: n >= 0, the arrays and the output there (else `bad`, the call's words for it), start <= end in each
int check_intervals(hm_pileup* p, const char* who, const char* bad, const int64_t* start, const int64_t* end, int64_t n, bool has_out) {
    if (n < 0 || (n && (!start || !end)) || !has_out) return pfail(p, HM_EINVAL, std::string(who) + ": " + bad);
    for (int64_t i = 0; i < n; ++i)
        if (start[i] > end[i]) return pfail(p, HM_EINVAL, std::string(who) + ": interval " + std::to_string(i) + " has start > end");
    return HM_OK;
}

// start and end as the two halves of d_iviv -> where each is on the device, and room for the sums; under the caller's guard
std::pair<const int64_t*, const int64_t*> stage_intervals(hm_pileup* p, const int64_t* start, const int64_t* end, int64_t n, size_t out_bytes) {
    const size_t bytes = sizeof(int64_t) * (size_t)n;
    p->d_ivout.reserve(out_bytes);
    p->d_iviv.reserve(2 * bytes);
    int64_t* iv = p->d_iviv.as<int64_t>();
    HIP_TRY(hipMemcpyAsync(iv, start, bytes, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemcpyAsync(iv + n, end, bytes, hipMemcpyHostToDevice, p->stream));
    return {iv, iv + n};
}

// the query kernel's launch checked, then its sums from d_ivout to the caller; under the caller's guard
int sums_back(hm_pileup* p, void* out, size_t bytes) {
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, p->d_ivout.p, bytes, hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(hipStreamSynchronize(p->stream));
    return HM_OK;
}

// the index in d_ividx, n elements of the scan Sc: launch(idx) starts the block-sums kernel, then their scan in place; under the caller's guard
template <class Sc, class Launch>
Sc build_index(hm_pileup* p, int64_t n, Launch launch) {
    p->d_ividx.reserve(sizeof(typename Sc::T) * (size_t)n);
    const Sc sc{p->d_ividx.as<std::remove_pointer_t<decltype(Sc::idx)>>()};
    launch(sc.idx);
    HIP_TRY(hipGetLastError());
    row_scan(p, sc, n);
    return sc;
}

// ... of the non-empty [lo, hi) of the planes `s` under min_cov
RegionIndex build_region_index(hm_pileup* p, const RangePlanes& s, int64_t lo, int64_t hi, int64_t min_cov) {
    const int64_t nblk = (hi - lo + HM_REGION_BLOCK - 1) / HM_REGION_BLOCK;
    return RegionIndex{s, lo, hi, min_cov, build_index<RegionScan>(p, nblk, [&](int64_t* idx) {
        hipLaunchKernelGGL(region_block_sums_kernel, dim3((unsigned)nblk), dim3(TPB), 0, p->stream, s, lo, hi, min_cov, idx);
    }).idx};
}

// what both fetches of `pileup -R / -J` check first; the planes into `s`
int region_call(hm_pileup* p, const char* who, const void* pcov, const void* ncov, const void* key, int64_t& plane_base, int64_t lo,
                int64_t hi, int64_t min_cov, const int64_t* start, const int64_t* end, int64_t n, bool has_out, RangePlanes& s) {
    if (lo < 0 || hi < lo || n < 0 || (n && (!start || !end)) || !has_out) return pfail(p, HM_EINVAL, std::string(who) + ": bad argument");
    if (hi - lo >= (int64_t(1) << 31) * HM_REGION_BLOCK) return pfail(p, HM_EINVAL, std::string(who) + ": range too large");
    if (min_cov < 1) return pfail(p, HM_EINVAL, std::string(who) + ": min_cov must be >= 1");
    if (const int rc = check_intervals(p, who, "bad argument", start, end, n, has_out)) return rc;  // only start > end is left to find
    return range_planes(p, pcov, ncov, key, plane_base, s) ? HM_OK : HM_ESTATE;
}

}  // namespace

extern "C" {

int hm_region_geometry(int64_t out[2]) {
    if (!out) return HM_EINVAL;
    out[0] = HM_REGION_BLOCK;
    out[1] = HM_REGION_SCAN_BLOCKS;
    return HM_OK;
}

int hm_pileup_fetch_regions(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                            int64_t hi, int64_t min_cov, const int64_t* start, const int64_t* end, int64_t n, hm_region_sum_t* out) {
    if (!p) return HM_EINVAL;
    RangePlanes s;
    const int rc = region_call(p, "hm_pileup_fetch_regions", pcov, ncov, key, plane_base, lo, hi, min_cov, start, end, n, !n || out, s);
    if (rc != HM_OK || !n) return rc;
    std::fill(out, out + 3 * n, hm_region_sum_t{0, 0, 0, 0});
    if (hi == lo) return HM_OK;
    return guarded(p, [&] {
        hipStream_t st = p->stream;
        const size_t out_bytes = sizeof(hm_region_sum_t) * 3 * (size_t)n;
        const auto [d_start, d_end] = stage_intervals(p, start, end, n, out_bytes);
        const RegionIndex ix = build_region_index(p, s, lo, hi, min_cov);
        hipLaunchKernelGGL(region_query_kernel, dim3(grid_for(n * 64)), dim3(TPB), 0, st, ix, plane_base, d_start, d_end, n, p->d_ivout.as<int64_t>());
        return sums_back(p, out, out_bytes);
    });
}

int hm_pileup_fetch_metaplot(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                             int64_t hi, int64_t min_cov, const int64_t* start, const int64_t* end, const int64_t* seq_start,
                             const int64_t* seq_end, const char* strand, int64_t n, int32_t bins, int64_t flank, int32_t flank_bins,
                             hm_metabin_t* out, int64_t* n_used) {
    if (!p) return HM_EINVAL;
    const char* who = "hm_pileup_fetch_metaplot";
    if (!n_used || (n && (!seq_start || !seq_end))) return pfail(p, HM_EINVAL, std::string(who) + ": bad argument");
    if (bins < 1 || bins > 1000 || flank < 0 || flank_bins < 0 || flank_bins > 1000 || (flank == 0) != (flank_bins == 0) ||
        (flank_bins && flank % flank_bins))
        return pfail(p, HM_EINVAL, std::string(who) + ": bins in [1, 1000], flank >= 0 a multiple of flank_bins in [0, 1000], both 0 or neither, expected");
    RangePlanes s;
    const int rc = region_call(p, who, pcov, ncov, key, plane_base, lo, hi, min_cov, start, end, n, out != nullptr, s);
    if (rc != HM_OK) return rc;
    const MetaGeom m{bins, flank_bins, flank};
    const int nb = m.n_bins();
    std::vector<MetaIv> used;
    for (int64_t i = 0; i < n; ++i) {
        if (seq_start[i] > start[i] || end[i] > seq_end[i])
            return pfail(p, HM_EINVAL, std::string(who) + ": interval " + std::to_string(i) + " is not within its sequence");
        if (end[i] - start[i] >= bins) used.push_back(MetaIv{start[i], end[i], seq_start[i], seq_end[i], strand && strand[i] == '-'});
    }
    *n_used = (int64_t)used.size();
    for (int c = 0; c < 3; ++c)
        for (int b = 0; b < nb; ++b) out[c * nb + b] = hm_metabin_t{c, b, 0, 0, 0, 0, 0};
    for (const MetaIv& r : used)  // the widths after the sequence clamp: the same whatever the planes and the chunk
        for (int b = 0; b < nb; ++b) {
            int64_t x0, x1;
            metabin_range(m, r, b, x0, x1);
            if (x1 > x0)
                for (int c = 0; c < 3; ++c) ++out[c * nb + b].n_regions;
        }
    if (used.empty() || hi == lo) return HM_OK;
    std::vector<int64_t> tab((size_t)nb * REGION_LANES);
    const int gr = guarded(p, [&] {
        hipStream_t st = p->stream;
        const size_t iv_bytes = sizeof(MetaIv) * used.size(), tab_bytes = sizeof(int64_t) * tab.size();
        p->d_iviv.reserve(iv_bytes);
        p->d_ivout.reserve(tab_bytes);
        HIP_TRY(hipMemcpyAsync(p->d_iviv.p, used.data(), iv_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(p->d_ivout.p, 0, tab_bytes, st));
        const RegionIndex ix = build_region_index(p, s, lo, hi, min_cov);
        // about 4 096 workgroups in all: enough to fill the device, few enough that a bin sees few atomics
        const int64_t waves = ((int64_t)used.size() + TPB / 64 - 1) / (TPB / 64);
        const unsigned gy = (unsigned)std::max<int64_t>(1, std::min<int64_t>(waves, (4096 + nb - 1) / nb));
        hipLaunchKernelGGL(metaplot_kernel, dim3((unsigned)nb, gy), dim3(TPB), 0, st, ix, plane_base, m, p->d_iviv.as<MetaIv>(),
                           (int64_t)used.size(), p->d_ivout.as<unsigned long long>());
        return sums_back(p, tab.data(), tab_bytes);
    });
    if (gr != HM_OK) return gr;
    for (int c = 0; c < 3; ++c)
        for (int b = 0; b < nb; ++b) {
            const int64_t* t = &tab[(size_t)b * REGION_LANES + 4 * (size_t)c];
            hm_metabin_t& o = out[c * nb + b];
            o.n_loci = t[0];
            o.pcov = t[1];
            o.ncov = t[2];
            o.ppm = t[3];
        }
    return HM_OK;
}

int hm_region_stats(const hm_region_sum_t* w, double out[2]) {
    if (!w || !out || w->n_loci <= 0 || w->pcov < 0 || w->ncov < 0 || w->pcov + w->ncov <= 0 || w->ppm < 0) return HM_EINVAL;
    out[0] = 100.0 * (double)w->pcov / (double)(w->pcov + w->ncov);
    out[1] = (double)w->ppm / (double)w->n_loci / 1e4;
    return HM_OK;
}

// ---- `smooth` -----------------------------------------------------------------------------------------------------------------------
int64_t hm_smooth_fetch(hm_pileup_t* p, int32_t part, int32_t ctx, int64_t lo, int64_t hi, int32_t half_width, int32_t min_cov,
                        int64_t min_loci, hm_smooth_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    const std::string who = "hm_smooth_fetch";
    if (part < 0 || part > 2) return pfail(p, HM_EINVAL, who + ": part must be 0, 1 or 2");
    if (ctx < 0 || ctx > 2) return pfail(p, HM_EINVAL, who + ": ctx must be 0, 1 or 2");
    if (half_width < 1 || half_width > HM_SMOOTH_MAX_HALF_WIDTH) return pfail(p, HM_EINVAL, who + ": half_width must be in [1, 16384]");
    if (min_cov < 1 || min_loci < 1) return pfail(p, HM_EINVAL, who + ": min_cov and min_loci must be >= 1");
    if (lo < 0 || hi < lo) return pfail(p, HM_EINVAL, who + ": bad range");
    int64_t plane_base = 0;
    RangePlanes s;
    if (!range_planes(p, nullptr, nullptr, nullptr, plane_base, s)) return HM_ESTATE;
    if (p->seq_off.empty()) return pfail(p, HM_ESTATE, who + " before hm_pileup_set_reference");
    if (part) {
        if (p->partitions != 2 || !p->hp_pcov[part - 1] || !p->hp_ncov[part - 1])
            return pfail(p, HM_ESTATE, who + " without partition planes (option partitions = 2, then hm_pileup_set_reference)");
        s.pc = p->hp_pcov[part - 1];
        s.nc = p->hp_ncov[part - 1];
    }
    const int64_t total = p->seq_off.back(), h = half_width;
    if (hi > total) return pfail(p, HM_EINVAL, who + ": range past the reference");
    if (hi == lo) return 0;
    // the planes are read over every window of [lo, hi): the span [a, b), and the running sums cover exactly that
    const int64_t a = std::max<int64_t>(0, lo - h + 1), b = std::min(total, hi + h - 1);
    const int built = guarded(p, [&] {
        p->d_smooth.reserve(sizeof(SmoothPre) * (size_t)(b - a));
        p->d_cxoff.reserve(8 * p->seq_off.size());
        HIP_TRY(hipMemcpyAsync(p->d_cxoff.p, p->seq_off.data(), 8 * p->seq_off.size(), hipMemcpyHostToDevice, p->stream));
        const int64_t nblk = (b - a + HM_SMOOTH_SPAN - 1) / HM_SMOOTH_SPAN;
        hipLaunchKernelGGL(smooth_prefix_kernel, dim3((unsigned)nblk), dim3(SMOOTH_TPB), 0, p->stream, s, a, b, (uint32_t)ctx, (int64_t)min_cov,
                           p->d_smooth.as<SmoothPre>());
        HIP_TRY(hipGetLastError());
        return HM_OK;
    });
    if (built != HM_OK) return built;
    const SmoothSel sel{s, p->d_smooth.as<SmoothPre>(), a, p->d_cxoff.as<int64_t>(), (int)p->seq_off.size() - 1, (uint32_t)ctx, h, min_cov, min_loci};
    return compact_rows(p, sel, lo, hi, out, cap, no_hook, no_hook);
}

int hm_smooth_stats(const hm_smooth_t* r, int32_t half_width, double out[2]) {
    if (!r || !out || half_width < 1 || r->wp < 0 || r->wn < 0 || (r->wp == 0 && r->wn == 0)) return HM_EINVAL;
    const double wp = (double)r->wp, wn = (double)r->wn;
    out[0] = 100.0 * wp / (wp + wn);
    out[1] = (wp + wn) / half_width;
    return HM_OK;
}

}  // extern "C"

// ---- `pileup -S` ------------------------------------------------------------------------------------------------------------------
namespace {

template <int F>
void launch_context(hm_pileup* p, bool lds, unsigned grid, const RangePlanes& s, const ContextRef& r, int64_t plane_base, int64_t lo,
                    int64_t hi, int64_t min_cov, unsigned long long* tab) {
    if constexpr (F <= HM_CONTEXT_LDS_MAX_FLANK) {
        if (lds) {
            hipLaunchKernelGGL((context_kernel<F, true>), dim3(grid), dim3(CX_THREADS), 0, p->stream, s, r, plane_base, lo, hi, min_cov, tab);
            return;
        }
    }
    hipLaunchKernelGGL((context_kernel<F, false>), dim3(grid), dim3(CX_THREADS), 0, p->stream, s, r, plane_base, lo, hi, min_cov, tab);
}

// both entry points; path: HM_CONTEXT_PATH_AUTO, _LDS or _GLOBAL
int64_t fetch_context(hm_pileup* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo, int64_t hi,
                      int64_t min_cov, int32_t flank, int32_t path, hm_region_sum_t* out, int64_t cap) {
    if (!p) return HM_EINVAL;
    const std::string who = "hm_pileup_fetch_context";
    if (p->seq_off.empty()) return pfail(p, HM_ESTATE, who + " before hm_pileup_set_reference");
    if (flank < 0 || flank > 3) return pfail(p, HM_EINVAL, who + ": flank must be 0, 1, 2 or 3");
    if (min_cov < 1) return pfail(p, HM_EINVAL, who + ": min_cov must be >= 1");
    if (lo < 0 || hi < lo) return pfail(p, HM_EINVAL, who + ": bad range");
    if ((!pcov || !ncov || !key) && (pcov || ncov || key)) return pfail(p, HM_EINVAL, who + ": pcov, ncov and key must be all NULL or none");
    if (path != HM_CONTEXT_PATH_AUTO && path != HM_CONTEXT_PATH_GLOBAL && !(path == HM_CONTEXT_PATH_LDS && flank <= HM_CONTEXT_LDS_MAX_FLANK))
        return pfail(p, HM_EINVAL, who + ": no such accumulation path for this flank");
    RangePlanes s;
    if (!range_planes(p, pcov, ncov, key, plane_base, s)) return HM_ESTATE;
    if (plane_base < 0 || plane_base > p->seq_off.back() || hi > p->seq_off.back() - plane_base)
        return pfail(p, HM_EINVAL, who + ": range past the reference");
    const int64_t n = 3 * context_rows(flank);
    if (!out || cap < n) return n;
    std::fill(out, out + n, hm_region_sum_t{0, 0, 0, 0});
    if (hi == lo) return n;
    const bool lds = path == HM_CONTEXT_PATH_AUTO ? flank <= HM_CONTEXT_LDS_FLANK : path == HM_CONTEXT_PATH_LDS;
    return guarded(p, [&]() -> int64_t {
        hipStream_t st = p->stream;
        const size_t bytes = sizeof(hm_region_sum_t) * (size_t)n;
        p->d_cxtab.reserve(bytes);
        p->d_cxoff.reserve(8 * p->seq_off.size());
        HIP_TRY(hipMemcpyAsync(p->d_cxoff.p, p->seq_off.data(), 8 * p->seq_off.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(p->d_cxtab.p, 0, bytes, st));
        if (!p->n_cus) {
            int cus = 0;
            HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->device));
            p->n_cus = cus > 0 ? cus : 256;
        }
        // one workgroup per CU: the LDS table at flank 1 leaves room for no second one, and the loads in flight do not need one
        const unsigned grid = (unsigned)std::min<int64_t>((hi - lo + CX_THREADS - 1) / CX_THREADS, p->n_cus);
        const ContextRef r{p->d_ref.as<char>(), p->d_cxoff.as<int64_t>(), (int)p->seq_off.size() - 1};
        unsigned long long* tab = p->d_cxtab.as<unsigned long long>();
        switch (flank) {
            case 0: launch_context<0>(p, lds, grid, s, r, plane_base, lo, hi, min_cov, tab); break;
            case 1: launch_context<1>(p, lds, grid, s, r, plane_base, lo, hi, min_cov, tab); break;
            case 2: launch_context<2>(p, lds, grid, s, r, plane_base, lo, hi, min_cov, tab); break;
            default: launch_context<3>(p, lds, grid, s, r, plane_base, lo, hi, min_cov, tab); break;
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, p->d_cxtab.p, bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return n;
    });
}

}  // namespace

extern "C" {

int hm_context_geometry(int64_t out[3]) {
    if (!out) return HM_EINVAL;
    out[0] = HM_CONTEXT_SPAN;
    out[1] = HM_CONTEXT_LDS_FLANK;
    out[2] = HM_CONTEXT_LDS_MAX_FLANK;
    return HM_OK;
}

int64_t hm_pileup_fetch_context(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                                int64_t hi, int64_t min_cov, int32_t flank, hm_region_sum_t* out, int64_t cap) {
    return fetch_context(p, pcov, ncov, key, plane_base, lo, hi, min_cov, flank, HM_CONTEXT_PATH_AUTO, out, cap);
}

int64_t hm_pileup_fetch_context_path(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                                     int64_t hi, int64_t min_cov, int32_t flank, int32_t path, hm_region_sum_t* out, int64_t cap) {
    return fetch_context(p, pcov, ncov, key, plane_base, lo, hi, min_cov, flank, path, out, cap);
}

// ---- `regiondiff`: the interval fetch over the M level planes (the skeleton is with `pileup -R / -J` above) ---------------------------
int64_t hm_sample_fetch_intervals(hm_pileup_t* p, int64_t lo, int64_t hi, int32_t ctx, int32_t complete, const int64_t* start,
                                  const int64_t* end, int64_t n_iv, hm_sample_interval_t* out) {
    if (!p) return HM_EINVAL;
    const char* who = "hm_sample_fetch_intervals";
    if (complete != 0 && complete != 1) return pfail(p, HM_EINVAL, std::string(who) + ": complete must be 0 or 1");
    if (ctx < 0 || ctx > 2) return pfail(p, HM_EINVAL, std::string(who) + ": ctx must be 0, 1 or 2");
    const int rc = option_range(p, who, sample_needs(p), lo, hi);
    if (rc != HM_OK) return rc;
    if (const int bad = check_intervals(p, who, "n_iv >= 0, start, end and out not NULL", start, end, n_iv, !n_iv || out)) return bad;
    const int M = p->samples_open;
    if (!M || !n_iv) return 0;
    std::fill(out, out + n_iv * M, hm_sample_interval_t{0, 0});
    if (hi == lo) return n_iv * M;
    const int done = guarded(p, [&] {
        hipStream_t st = p->stream;
        int P = 2;
        while (P < M) P <<= 1;
        const SampleIvPlanes v{p->d_slevel.as<uint16_t>(), p->sample_stride, p->key, M, 64 / P, (uint32_t)ctx, (int)complete};
        const int64_t nblk = (hi - lo + HM_REGION_BLOCK - 1) / HM_REGION_BLOCK;
        const size_t out_bytes = sizeof(SamplePair) * (size_t)n_iv * (size_t)M;
        const size_t lds = sizeof(uint32_t) * (TPB / 64) * (size_t)M * (size_t)v.pitch();
        const auto [d_start, d_end] = stage_intervals(p, start, end, n_iv, out_bytes);
        const SamplePair* idx = build_index<SampleIvScan>(p, (int64_t)M * nblk, [&](SamplePair* sums) {
            hipLaunchKernelGGL(sample_block_sums_kernel, dim3((unsigned)nblk), dim3(TPB), lds, st, v, lo, hi, nblk, sums);
        }).idx;
        // at most 2^14 workgroups: 65 536 wavefronts share the intervals beyond that
        hipLaunchKernelGGL(sample_query_kernel, dim3(grid_for(n_iv * 64, 1 << 14)), dim3(TPB), lds, st, v, lo, hi, nblk, idx, d_start, d_end, n_iv,
                           p->d_ivout.as<SamplePair>());
        return sums_back(p, out, out_bytes);
    });
    return done != HM_OK ? done : n_iv * M;
}

int hm_sample_interval_test(const hm_sample_interval_t* sums, int64_t n_iv, int32_t M, const uint8_t* group, int64_t min_loci,
                            int32_t min_reps, hm_sample_test_t* out) {
    if (n_iv < 0 || M < 1 || M > SAMPLE_MAX || !group || (n_iv && (!sums || !out)) || min_loci < 1 || min_reps < 2 || min_reps > SAMPLE_MAX)
        return HM_EINVAL;
    for (int s = 0; s < M; ++s)
        if (group[s] > 2) return HM_EINVAL;
    const double nan = std::nan("");
    for (int64_t i = 0; i < n_iv; ++i) {
        const hm_sample_interval_t* e = sums + i * M;
        double x[SAMPLE_MAX], mean[2], var[2];
        int m[2] = {0, 0};
        uint64_t loci[2] = {0, 0};
        for (int g = 0; g < 2; ++g) {
            double sum = 0.0;
            for (int s = 0; s < M; ++s) {
                x[s] = nan;
                if (group[s] != g + 1 || e[s].n < (uint64_t)min_loci) continue;
                x[s] = 100.0 * (double)e[s].su / ((double)e[s].n * 32768.0);
                sum += x[s];
                loci[g] += e[s].n;
                ++m[g];
            }
            mean[g] = m[g] ? sum / (double)m[g] : nan;
            double ss = 0.0;
            for (int s = 0; s < M; ++s)
                if (x[s] == x[s]) ss += (x[s] - mean[g]) * (x[s] - mean[g]);
            var[g] = m[g] > 1 ? ss / (double)(m[g] - 1) : nan;
        }
        hm_sample_test_t& r = out[i];
        r = hm_sample_test_t{m[0], m[1], loci[0], loci[1], mean[0], mean[1], nan, nan, nan};
        if (m[0] < min_reps || m[1] < min_reps) continue;
        const double a1 = var[0] / (double)m[0], a2 = var[1] / (double)m[1], se2 = a1 + a2, d = mean[0] - mean[1];
        if (se2 == 0.0) {
            if (d == 0.0) {
                r.t = 0.0;
                r.df = (double)(m[0] + m[1] - 2);
                r.pvalue = 1.0;
            } else {
                r.t = d > 0.0 ? INFINITY : -INFINITY;
            }
            continue;
        }
        r.t = d / std::sqrt(se2);
        r.df = se2 * se2 / (a1 * a1 / (double)(m[0] - 1) + a2 * a2 / (double)(m[1] - 1));
        if (r.t == 0.0) {
            r.pvalue = 1.0;
            continue;
        }
        // the tail of group_test_kernel with F = t^2 and a real nu: 1 / (a B(a, 1/2)) = Gamma(a + 1/2) / (sqrt(pi) Gamma(a + 1)), a <= 63
        const double F = r.t * r.t, a = 0.5 * r.df;
        const double xx = r.df / (r.df + F), y = F / (r.df + F);
        const double xa = y < 0.5 ? std::exp(a * std::log1p(-y)) : std::pow(xx, a);
        const double front = std::tgamma(a + 0.5) / (1.7724538509055160273 * std::tgamma(a + 1.0)) * xa * std::sqrt(y);
        const double pv = xx < (a + 1.0) / (a + 2.5) ? front * beta_cf(a, 0.5, xx) : 1.0 - 2.0 * a * front * beta_cf(0.5, a, y);
        r.pvalue = pv > 1.0 ? 1.0 : pv >= DBL_MIN ? pv : DBL_MIN;
    }
    return HM_OK;
}

int hm_sample_qvalues(const double* pv, int64_t n, double* q) {
    if (n < 0 || (n && (!pv || !q))) return HM_EINVAL;
    std::vector<BhEntry> ent;
    for (int64_t i = 0; i < n; ++i) {
        q[i] = std::nan("");
        if (pv[i] != pv[i]) continue;
        if (!(pv[i] >= DBL_MIN && pv[i] <= 1.0)) return HM_EINVAL;
        ent.push_back(BhEntry{pv[i], 1, i});
    }
    bh_qvalues(ent, ent.size(), [&](int64_t where, double v) { q[where] = v; });
    return HM_OK;
}

}  // extern "C"
