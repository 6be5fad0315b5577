/*
 * hifimeth_hip.h -- C ABI of libhifimeth_hip.so, the MI355X (gfx950) engine for the
 * `hifimeth call` hot path: per-read CpG/CHG/CHH site scan -> 401x8 kinetics window -> CNN ->
 * per-site 5mC probability.
 *
 * The reference has no plugin/FFI layer; this library sits where three C++ classes of the
 * reference sit inside its worker thread (src/app/hifimeth/mod_main.cpp:145-262):
 *
 *   ns_mods::ModModels                  (mod_main.cpp:18-99)         -> hm_create / hm_destroy
 *   ns_mods::EvalKmerFeaturesGenerator  (eval_kmer_features.hpp:13-49)
 *       init(bam1_t*)                                                -> hm_submit_read
 *       extract_{cpg,chg,chh}_samples()                              -> hm_run, hm_scan_sites
 *       get_next_sample_features()                                   -> hm_windows
 *   ns_mods::ModBatch                   (mod_batch.hpp:12-43)
 *       call_mods_for_one_read / call_current_batch                  -> hm_run, hm_cnn_logits
 *       results appended to std::vector<MolMethyCall>                -> hm_fetch / hm_drain
 *
 * Plain pointers and sizes only; every call returns >= 0 on success and a negative HM_E* code
 * on failure (the reference abort()s instead: src/corelib/hbn_aux.hpp:100-104), with the message
 * available from hm_last_error().
 *
 * Two ways to drive an engine:
 *  - the synchronous calls (hm_submit_read ... hm_fetch): ONE implicit batch, one host thread; what the parity tests use;
 *  - the batch pipeline (hm_batch_*): N slots per engine, each with pinned staging memory and its own copy stream.
 *    Staging of different batches may run on different host threads (the reference's workers pull reads from a shared
 *    queue: src/corelib/sam_batch.hpp:38-54); hm_batch_enqueue queues H2D -> scanner -> CNN -> results and returns
 *    without any host/device synchronisation, so batch k+1 is staged and uploaded while batch k computes (the pinned
 *    non-blocking staging of the reference's GPU variant, src/app-gpu/hifimeth-gpu/5mc_call_gpu.cpp:309-334,367).
 */
#ifndef HIFIMETH_HIP_H
#define HIFIMETH_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HM_CTX_CPG 0
#define HM_CTX_CHG 1
#define HM_CTX_CHH 2
#define HM_CTX_ALL 3 /* only as the `ctx` argument of hm_num_sites */

#define HM_OK 0
#define HM_EINVAL (-1)  /* bad argument                                             */
#define HM_EMODEL (-2)  /* model file missing / ill-formed (mod_main.cpp:40-52), or a weight that is not finite (as fp32, or as the fp16 half the kernels keep) */
#define HM_EDEVICE (-3) /* HIP runtime error or no gfx950 device                    */
#define HM_EDATA (-4)   /* illegal base nibble in a read (bam_info.cpp:100-121)     */
#define HM_ESTATE (-5)  /* call out of order (e.g. hm_fetch before hm_run)          */
#define HM_ENOMEM (-6)

typedef struct hm_engine hm_engine_t;

/* One call = the reference's MolMethyCall (src/corelib/5mc_motif_finder.hpp:8-14) plus the
 * context and the float probability the reference never exposes (needed for the |dp| check). */
typedef struct {
    int32_t read_id;     /* qid: the id given to hm_submit_read                           */
    int32_t qoff;        /* forward-strand offset of the cytosine (of the G for strand 1) */
    uint8_t strand;      /* 0 = FWD, 1 = REV (src/corelib/hbn_aux.hpp:60-63)              */
    uint8_t ctx;         /* HM_CTX_*                                                      */
    uint8_t scaled_prob; /* min(255, (int)(255 * p))  (mod_batch.cpp:46-64)               */
    uint8_t reserved;
    float p;             /* softmax(logits)[1]                                            */
} hm_call_t;

/* Accumulated device time per kernel class since the last hm_reset_timing (HIP events on the
 * engine's stream; only collected when option "timing" is 1). */
typedef struct {
    double prep_ms, scan_ms, emit_ms, window_ms;
    double front_ms[3], tail_ms[3];
    int64_t prep_launches, scan_launches, emit_launches, window_launches;
    int64_t front_launches[3], tail_launches[3];
    int64_t front_sites[3]; /* sites processed by the timed front launches */
    int64_t window_sites;
    double pack_ms, empty_ms; /* result packing; CNN launches whose window of the site list turned out empty */
    int64_t pack_launches, empty_launches;
    double trunk_ms[3], edge_ms[3]; /* dense trunk (conv1..conv4 over whole reads) and window-edge kernels */
    int64_t trunk_launches[3], edge_launches[3];
    int64_t trunk_positions[3]; /* (read, strand view) positions evaluated by the timed trunk launches */
    int64_t trunk_list_steps[3]; /* tiles whose conv4 ran over the listed (needed) rows only: 4 m-tiles instead of 7 (sliding-window trunk) */
    int64_t trunk_const_steps[3]; /* tiles stored as constant rows instead of computed: a read's first tile and those behind its end, where no receptive field reaches the read */
    int64_t group_bases;        /* bases per trunk read group in force (option "group_bases", or what the engine sized from free memory) */
    int64_t group_bytes;        /* device bytes the engine holds for a read group's maps, edge rows and hand-off buffers */
    int64_t tail_strip_passes;  /* passes (16 site slots each) of the strip tail kernel (tail_impl 3, CHH): MFMAs issued = passes x a pass's count */
} hm_timing_t;

/* Version of this header's structs (hm_timing_t grows round by round: 4 = round 4, 5 = + tail_strip_passes).  hm_abi_version() returns what the
 * LIBRARY was built with and hm_timing_size() its sizeof(hm_timing_t): a consumer compares both with its own before calling hm_get_timing. */
#define HM_ABI_VERSION 5
int hm_abi_version(void);
size_t hm_timing_size(void);

/* ---- lifetime ---------------------------------------------------------------------------- */
/* model_dir holds {CpG,CHG,CHH}.hmw (flat fp32 container written from the reference's
 * models/{CpG,CHG,CHH}.onnx) or the .onnx files themselves; ctx_mask bit c enables context c
 * (the reference's -c cpg,chg,chh: mod_options.cpp:61-134); device = HIP device ordinal.   */
int hm_create(hm_engine_t** out, const char* model_dir, int ctx_mask, int device);
void hm_destroy(hm_engine_t* e);
const char* hm_last_error(const hm_engine_t* e); /* e may be NULL: error of a failed hm_create */
/* options: "slots" (batches in flight of the hm_batch_* pipeline, default 3), "min_read_size" (-l, default 1000), "timing" (0/1), "sub_batch_sites" (front/tail
 * launch granularity, default 65536), "front_waves" (4 or 8 waves per front workgroup), "precision" (0 = fp32 MFMA, exact;
 * 1 = split-half fp16x3 MFMA with fp32 accumulate (default, |dp| <= 1e-4); 2 = as 1 with plain fp16 WEIGHTS in conv8 and fc1 (their
 * w_lo x_hi product and lo-plane fetches dropped): the part of BASELINE.json configs[4] that holds its bar |dp| <= 1e-3 with margin;
 * as written -- fp16 weights in every layer -- that configuration reaches 2.5e-3 (profiles/r02_term_error_table.txt) and stays closed: 3 is an error), "trunk" (2 = per context by the site density of the FIRST batch the engine is given -- counted
 * on the host when that batch is queued and then fixed for the engine's lifetime, so the calls never depend on host timing --
 * default; 1 = conv1..conv4 once per read position; 0 = once per site; every precision has both forms), "trunk_mask" (0..7: that
 * choice made by the caller, see hm_trunk_mask_for_reads), "trunk_impl" (3 = the streaming trunk as a sliding window over
 * consecutive tiles, default; 1 = streaming 4-wave trunk kernel; 2 = the same on 8 waves; 0 = the 8-wave ConvH form; byte-identical results), "edge_impl" (2 = edge2_kernel computing the E1 rows its chains read, default: with
 * trunk_impl 3 no E1 map is stored or allocated; 1 = edge2_kernel gathering them from the E1 map; 0 = round 2's
 * edge_kernel; byte-identical), "tail_impl" (3 = the strip tail for CHH (16 sites of one E4-row residue class per pass share one strip of rows in LDS; hm_tail_p.hip) and 1 for the sparse contexts, default; 1 = tail with register-resident weights; 2 = the split tail: conv5 + conv6, then conv7 .. softmax over 16 sites per pass ("tail_slice": sites per launch pair); 0 = the streaming tail; byte-identical),
 * "group_bases" (reads per trunk group; default 0 = sized when the first read is staged so that a group's buffers, 5.8 KB per base, take at most a quarter of the device's free memory, and at most 16 Mi bases), "num_cu" (workgroups of the persistent kernels), "conv3_w16" (diagnostic: conv3 of the dense trunk with plain fp16 weights -- measured ABOVE the 1e-3 bar,
 * part of no mode), "stamps" (diagnostic) */
int hm_set_option(hm_engine_t* e, const char* key, int64_t value);

/* ---- staging: the EvalKmerFeaturesGenerator::init seam ----------------------------------- */
/* Copies one read into the pinned staging slab exactly as the BAM record stores it: 4-bit
 * packed SEQ, and the fi/fp/ri/rp B-arrays with element width 1 (B:C codev1) or 2 (B:S frames).
 * A NULL array means the tag is missing.  Returns 1 if the read was accepted, 0 if it is passed
 * through uncalled (l_qseq < min_read_size, l_qseq == 0 or a missing tag: mod_main.cpp:189-196), < 0 on error.
 * The caller keeps ownership of all pointers.                                                */
int hm_submit_read(hm_engine_t* e, int32_t read_id, int32_t l_qseq, int32_t flag, const uint8_t* seq4,
                   const void* fi, int fi_width, const void* fp, int fp_width, const void* ri, int ri_width,
                   const void* rp, int rp_width);
int hm_clear(hm_engine_t* e); /* forget the staged / resident batch */

/* ---- execution --------------------------------------------------------------------------- */
int hm_upload(hm_engine_t* e); /* staged slab -> HBM (async on the engine stream)              */
int hm_run(hm_engine_t* e);    /* scanner + window builder + CNN over the resident batch        */
int hm_sync(hm_engine_t* e);   /* wait for everything queued; reports device-side data errors   */
int64_t hm_num_sites(hm_engine_t* e, int ctx); /* after hm_run: the reference's processed_*_samples */
/* D2H of the results of the last hm_run, ordered by (read submission order, strand, qoff) -- the
 * order build_one_mod_bam needs (mod_main.cpp:217-251).  Returns the number of calls written. */
int64_t hm_fetch(hm_engine_t* e, hm_call_t* out, int64_t cap);
/* convenience: hm_flush = hm_upload + hm_run ; hm_drain = hm_sync + hm_fetch + hm_clear */
int hm_flush(hm_engine_t* e);
int64_t hm_drain(hm_engine_t* e, hm_call_t* out, int64_t cap);

/* ---- the asynchronous batch pipeline -------------------------------------------------------- */
typedef struct hm_batch hm_batch_t;
/* A free slot in STAGING state; blocks while all "slots" are staged or in flight.  NULL on error. */
hm_batch_t* hm_batch_begin(hm_engine_t* e);
/* hm_submit_read into this batch's pinned slab; batches may be staged concurrently from different threads */
int hm_batch_submit_read(hm_batch_t* b, int32_t read_id, int32_t l_qseq, int32_t flag, const uint8_t* seq4,
                         const void* fi, int fi_width, const void* fp, int fp_width, const void* ri, int ri_width,
                         const void* rp, int rp_width);
/* Bulk form: n reads in one call, copied into the slab by `threads` host threads (the per-read layout is fixed by a
 * serial pass first, so the result is identical to n hm_batch_submit_read calls in order).  A read that would be passed
 * through uncalled is skipped exactly as there; accepted[i] (may be NULL) tells which.  Returns the number accepted.
 * All n reads are validated before the first is placed: on an error (HM_EINVAL, HM_ENOMEM = the batch would pass 2^31
 * bases) the batch is exactly as it was before the call. */
typedef struct {
    int32_t read_id, l_qseq, flag;
    uint8_t width[4];     /* element width of fi, fp, ri, rp: 1 (B:C) or 2 (B:S) */
    const uint8_t* seq4;
    const void* kin[4];   /* fi, fp, ri, rp; NULL = tag missing */
} hm_read_t;
int64_t hm_batch_submit_reads(hm_batch_t* b, const hm_read_t* reads, int64_t n, int threads, uint8_t* accepted);
/* The per-context choice the engine makes under "trunk" = 2, as a function of a sample of reads (host only, no device work,
 * only seq4 / l_qseq are read): bit c set = context c takes the dense trunk.  A front end that shards one input over several
 * engines or ranks passes the SAME sample (the head of the file) everywhere and sets the result with the "trunk_mask" option,
 * so that every shard computes with the same kernels and the merged output equals the single-process output byte for byte
 * (the reference's output is deterministic: mod_main.cpp:330-362). */
int hm_trunk_mask_for_reads(const hm_read_t* reads, int64_t n, int ctx_mask);
int64_t hm_batch_staged_bases(const hm_batch_t* b);
/* Queues the batch: async H2D on the slot's stream, scanner + CNN + result packing on the engine's compute stream (site
 * counts are consumed on the device), async D2H of the totals.  Returns at once; batches compute in queueing order. */
int hm_batch_enqueue(hm_batch_t* b);
int hm_batch_done(hm_batch_t* b); /* 1 finished, 0 still in flight, < 0 error; never blocks */
/* Waits for THIS batch only.  Returns its number of calls; with calls != NULL also brings them to the host with one
 * packed D2H and points *calls at them (pinned memory owned by the slot, valid until hm_batch_release), ordered by
 * (read submission order, strand, qoff) like hm_fetch.  HM_EDATA if a staged read held an illegal base. */
int64_t hm_batch_wait(hm_batch_t* b, const hm_call_t** calls);
int64_t hm_batch_num_sites(hm_batch_t* b, int ctx); /* waits like hm_batch_wait(b, NULL) */
int hm_batch_release(hm_batch_t* b); /* the slot may be handed out again */

/* ---- seams used by the parity tests and the feature-extraction roofline ------------------- */
/* extract_*_samples: site list of one context after hm_run, in (read, qoff) order */
int64_t hm_scan_sites(hm_engine_t* e, int ctx, int32_t* read_id, int32_t* qoff, uint8_t* strand, int64_t cap);
/* logits [n][2] (l0, l1) the CNN computed for the sites of one context after hm_run, in hm_scan_sites order, whichever kernels
 * ran (per site, dense trunk, any tail); returns n, HM_EINVAL when n > cap */
int64_t hm_site_logits(hm_engine_t* e, int ctx, float* logits, int64_t cap);
/* the edge kernel's rows -- conv4 rows 0 and 24 per site, [site][side][hi 96 | lo 96] fp16 bit patterns (precision 1, 2) -- of the LAST
 * read group and context the dense trunk path ran (the buffer is reused by every group and context: run one context in one group to
 * see all its sites, in hm_scan_sites order); copies `sites` x 384 halves, HM_EINVAL if the buffer holds fewer (debug / tests) */
int hm_debug_edge_rows(hm_engine_t* e, int64_t sites, uint16_t* rows);
/* get_next_sample_features: raw 401x8 fp32 windows of sites [first, first+n) of context ctx;
 * out_host may be NULL (device-only run for timing) */
int hm_windows(hm_engine_t* e, int ctx, int64_t first, int64_t n, float* out_host);
/* ModBatch::call_current_batch on caller-supplied windows [n][401][8] (host memory) */
int hm_cnn_logits(hm_engine_t* e, int ctx, const float* windows, int64_t n, float* logits, float* p, uint8_t* ml);
/* post-ReLU channels-last activations of conv `layer` (1..8) for one window (debug / tests) */
int64_t hm_debug_layer(hm_engine_t* e, int ctx, const float* window, int layer, float* out, int64_t cap);

/* Model-file utility (no GPU needed): read <src> (.onnx in either shipped dialect, or .hmw) and write
 * the flat fp32 .hmw container.  The same reader serves hm_create, so a model_dir holding the
 * reference's own CpG.onnx / CHG.onnx / CHH.onnx (mod_main.cpp:76,85,94) works unchanged. */
int hm_convert_model(const char* src_path, const char* dst_hmw_path);

/* diagnostic (option "stamps" = 1): shader-clock cycles per phase of the front kernel, summed over
 * all waves of the launches since the option was set; returns the number of slots written */
int hm_get_stamps(hm_engine_t* e, uint64_t* out, int cap);

int hm_get_timing(hm_engine_t* e, hm_timing_t* t);
int hm_reset_timing(hm_engine_t* e);

/* ==== `hifimeth pileup`: per-locus methylation frequencies ========================
 * Replaces the body of s_genomic_methy_freq_thread + the counting loop of s_compute_methy_freq
 * (src/app/hifimeth/pileup.cpp:208-353, 514-560) and the classes they drive:
 *   BamMapInfo::init / cigar_to_alignment   (src/corelib/bam_info.cpp:262-439)     -> hm_pileup_submit_read
 *   (ours) the calls of hm_batch_wait straight into the pileup, no mod-BAM between  -> hm_pileup_submit_read_calls
 *   extract_chh_mapped_samples              (src/corelib/5mc_motif_finder.cpp:104-144)
 *   CpG / CHG loops                         (pileup.cpp:292-335)                     -> hm_pileup_run
 *   3 x 256 probability histograms          (pileup.cpp:237-272)                     -> hm_pileup_histograms
 *   per-locus pcov / ncov / motif           (pileup.cpp:519-560)                     -> hm_pileup_count
 *   rows of <prefix>.<ctx>.cov.bed          (pileup.cpp:562-590)                     -> hm_pileup_fetch_loci
 *   (ours) haplotype difference per locus, rows of <prefix>.asm.<ctx>.bed         -> hm_pileup_fetch_asm
 *   (ours) two samples' *.cov.bed rows into the haplotype planes (`diff`)         -> hm_pileup_load_loci
 *   (ours) two groups of replicates, tested with their spread (`groupdiff`)       -> hm_pileup_group_sample, hm_pileup_fetch_groups
 *   (ours) N samples' correlation matrix per context (`samplecorr`)               -> hm_sample_open, hm_sample_fetch_sums
 *   (ours) two groups of samples tested over given intervals (`regiondiff`)       -> hm_sample_fetch_intervals, hm_sample_interval_test
 *   (ours) kernel-smoothed level per locus of one sample (`smooth`)               -> hm_smooth_fetch
 * The whole genome's counters stay resident in HBM (12 B per reference base, 28 B with the haplotype partitions) and the
 * projected calls wait in HBM (12 B each) until the thresholds are known -- the reference spills them to a temporary file.
 * MM/ML parsing and BED text formatting stay on the host (hm_bam.h).                                           */
typedef struct hm_pileup hm_pileup_t;

/* BaseModInfo (src/corelib/bam_mod_parser.hpp): one (position, code) of the MM lists with its ML byte */
typedef struct {
    int32_t qoff;       /* forward-strand (original read orientation) offset */
    uint8_t strand;     /* 0 '+', 1 '-'                                      */
    char unmod_base;
    char code;          /* 'm' = 5mC; other codes only enter the histograms  */
    uint8_t prob;
} hm_mod_t;

/* one covered locus = one BED row: chrom, soff, soff+1, 100*pcov/(pcov+ncov), pcov, ncov */
typedef struct {
    int64_t gpos;       /* offset into the concatenated reference (sequence offset + soff) */
    int32_t pcov, ncov;
    uint32_t motif;     /* 0 CpG, 1 CHG, 2 CHH: class of the locus' last record in BAM order */
    uint32_t reserved;
} hm_locus_t;

int hm_pileup_create(hm_pileup_t** out, int device);
void hm_pileup_destroy(hm_pileup_t* p);
const char* hm_pileup_last_error(const hm_pileup_t* p); /* p may be NULL: error of a failed create */
/* options: "min_mapq" (-q, default 0), "min_pi" (-f, default 0.0), "partitions" (0 default, or 2: haplotype-resolved
 * counting, see hm_pileup_submit_read_hp; must be set before hm_pileup_set_reference / hm_pileup_use_planes, else HM_ESTATE),
 * "patterns" and "pattern_span" (read-level CpG patterns), "bedmethyl" (per-CpG depth classes), "linkage" (co-methylation by
 * distance), "profile" (methylation by position in the read) and "trim5" / "trim3" (end trimming), all near the end of this header;
 * "load_slab" (hm_pileup_load_loci); "groups" and "group_min_cov" (hm_pileup_group_sample); "samples" and "sample_min_cov"
 * (hm_sample_open) */
int hm_pileup_set_option(hm_pileup_t* p, const char* key, double value);
/* HbnDatabase: n_seqs upper-cased sequences back to back in `bases` (seq_len[i] bytes each).  Allocates and
 * zeroes the per-locus planes unless hm_pileup_use_planes was called before.
 * A LATER CALL re-targets the engine.  After it returns HM_OK the engine cannot be told from a newly created one on which the
 * same options, the same hm_pileup_use_planes and the same hm_pileup_use_partition_planes were applied, followed by this one call:
 *  - options persist, and an option that must be set before hm_pileup_set_reference still answers HM_ESTATE;
 *  - caller-owned planes stay registered; the call does not touch them: they are the caller's to zero, and must hold the new
 *    reference;
 *  - dropped: records submitted and not yet run; resident records and pattern windows (hm_pileup_num_records is 0); the 768
 *    histogram bins; the engine's own planes and every table this call allocates (partition, group and sample planes, the
 *    pattern, bedmethyl, linkage and read-position tables), zeroed and sized for the new reference; the thresholds of the last
 *    hm_pileup_count; "a record was staged", "rows were loaded" and "a load met a bad row" (counts come from one source per
 *    reference, not per engine); all seen bits of the loaders; the samples opened (hm_pileup_group_sample and hm_sample_open
 *    start at 0 again); the error text.
 * Device memory is kept and reused; it grows only where the new reference needs more.  A call that fails on its arguments
 * (HM_EINVAL: n_seqs <= 0, a NULL pointer, a negative length, 2^40 bases or more) leaves the engine as it was. */
int hm_pileup_set_reference(hm_pileup_t* p, int32_t n_seqs, const int64_t* seq_len, const char* bases);
/* Count into caller-owned DEVICE planes of total-reference-length elements (int32 pcov, int32 ncov, uint32 key),
 * e.g. torch tensors that a RCCL reduce-scatter will consume.  The caller zeroes them. */
int hm_pileup_use_planes(hm_pileup_t* p, void* pcov, void* ncov, void* key);
int hm_pileup_planes(hm_pileup_t* p, void** pcov, void** ncov, void** key, int64_t* n_loci);
/* Haplotype partitions (option "partitions" = 2): two more int32 pcov / ncov plane pairs (+16 B per reference base), counted
 * with the combined thresholds; a partition has no key plane of its own -- its loci take the combined motif.  `part` is 1 or 2.
 * hm_pileup_set_reference allocates and zeroes the pairs that were not registered here before (caller-owned DEVICE planes
 * of total-reference-length elements, zeroed by the caller).  A partition's covered loci come from hm_pileup_fetch_loci
 * with that partition's pcov / ncov and the combined key plane. */
int hm_pileup_use_partition_planes(hm_pileup_t* p, int32_t part, void* pcov, void* ncov);
int hm_pileup_partition_planes(hm_pileup_t* p, int32_t part, void** pcov, void** ncov);
/* One mapped record: `order` = its index in the BAM, < 2^29 (decides the motif of a locus hit by two classes), `sid` =
 * index into the reference sequences, SEQ 4-bit packed and CIGAR as the BAM record stores them, `mods` = its
 * parsed MM/ML lists.  Returns 1 if staged, 0 if the record contributes nothing (unmapped, no mods), < 0 on
 * error (illegal base nibble, alignment running past the read or the reference sequence). */
int hm_pileup_submit_read(hm_pileup_t* p, uint32_t order, int32_t flag, int32_t sid, int64_t pos, int32_t mapq,
                          int32_t l_qseq, const uint8_t* seq4, int32_t n_cigar, const uint32_t* cigar,
                          int64_t n_mods, const hm_mod_t* mods);
/* the same with the record's haplotype partition `hp`: 0 (combined output only; = hm_pileup_submit_read), 1 or 2 (also
 * counted in that partition).  HM_EINVAL for hp outside {0, 1, 2}, HM_ESTATE for hp != 0 without the partitions option. */
int hm_pileup_submit_read_hp(hm_pileup_t* p, uint32_t order, int32_t flag, int32_t sid, int64_t pos, int32_t mapq,
                             int32_t l_qseq, const uint8_t* seq4, int32_t n_cigar, const uint32_t* cigar,
                             int64_t n_mods, const hm_mod_t* mods, int32_t hp);
/* The fused path (`pileup -K`): the same record with its 5mC CALLS instead of parsed MM/ML lists --
 * `calls` exactly as hm_batch_wait / hm_fetch deliver them for this read (FWD strand by ascending qoff, then REV strand by
 * ascending qoff; read_id is ignored).  The effect on the engine -- histograms, projected records, planes after
 * hm_pileup_count, return value -- is that of writing the calls into the record as MM/ML (hmbam::apply_calls), parsing them
 * back (hmbam::parse_mods) and passing the result to hm_pileup_submit_read_hp; no tag text is built.  n_calls == 0 returns 0
 * like a record without MM.  Every check of hm_pileup_submit_read_hp holds; in addition HM_EDATA for a qoff outside
 * [0, l_qseq) and HM_EINVAL for calls that are not strictly increasing per strand, FWD before REV.  On an error the staged
 * batch is as it was.  One batch (hm_pileup_run) may mix records submitted with mods and records submitted with calls. */
int hm_pileup_submit_read_calls(hm_pileup_t* p, uint32_t order, int32_t flag, int32_t sid, int64_t pos, int32_t mapq,
                                int32_t l_qseq, const uint8_t* seq4, int32_t n_cigar, const uint32_t* cigar,
                                int64_t n_calls, const hm_call_t* calls, int32_t hp);
/* histograms + projection of the staged records; the projected calls are appended to the HBM-resident list */
int hm_pileup_run(hm_pileup_t* p);
int64_t hm_pileup_num_records(hm_pileup_t* p);
/* bins[ctx*256 + scaled_prob], accumulated over all runs; hm_pileup_add_histograms adds counts from elsewhere */
int hm_pileup_histograms(hm_pileup_t* p, uint64_t* bins768);
/* debug / tests: D2H of the projected calls (unordered): gpos, prob, motif, order */
int64_t hm_pileup_fetch_records(hm_pileup_t* p, int64_t* gpos, uint8_t* prob, uint8_t* motif, uint32_t* order,
                                int64_t cap);
/* `hifimeth eval` (src/app/hifimeth/eval.cpp:469-560): joins the resident records with per-locus truth labels --
 * labels[g] over the concatenated reference: -1 none, 0 unmethylated, 1 methylated (s_fill_chr_base_label_with_bismark,
 * eval.cpp:42-114) -- into bins[(motif * 2 + label) * 256 + scaled_prob].  The records stay resident. */
int hm_pileup_label_histograms(hm_pileup_t* p, const int8_t* labels, int64_t n_labels, uint64_t* bins1536);
/* zero-free accumulate of all resident records into the planes with the given per-context thresholds
 * (prob >= thr -> pcov else ncov; key = max(order << 2 | motif)), with partitions also into the record's partition
 * planes; then drops the records */
int hm_pileup_count(hm_pileup_t* p, const uint8_t thr[3]);
/* covered loci (pcov + ncov > 0) of planes[lo, hi) in ascending order; planes NULL = the engine's own, else
 * DEVICE pointers whose element 0 is locus `plane_base`.  Returns the number of loci (may exceed cap: then
 * nothing is written). */
int64_t hm_pileup_fetch_loci(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key,
                             int64_t plane_base, int64_t lo, int64_t hi, hm_locus_t* out, int64_t cap);

/* ---- allele-specific methylation (`pileup -H -A`): where do the two haplotypes differ -------------
 * A locus is tested when EACH haplotype partition has pcov + ncov >= min_cov.  diff = 100 * p1 / (p1 + n1) - 100 * p2 / (p2 + n2)
 * in fp64 (bit-equal to the host's), pvalue = two-sided Fisher exact test of [[p1, n1], [p2, n2]] with R's rule (margins fixed,
 * sum of the hypergeometric probabilities of all tables with probability <= P(observed) * (1 + 1e-7)), <= 1.0 and never 0
 * (a value below DBL_MIN is reported as DBL_MIN).  Computed on the device from a log n! table (65 536 entries, uploaded by the
 * first call; larger totals use lgamma in the kernel); a pure function of the four counts. */
typedef struct {            /* one tested locus = one row of <prefix>.asm.<ctx>.bed; 48 bytes */
    int64_t gpos;
    int32_t pcov1, ncov1, pcov2, ncov2;
    uint32_t motif, reserved;
    double diff, pvalue;
} hm_asm_t;
/* tested loci of planes[lo, hi) in ascending order.  All five plane pointers NULL = the engine's own partition and key planes;
 * else DEVICE pointers whose element 0 is locus plane_base (what a reduce-scatter leaves on a rank).  Returns the number of
 * rows (may exceed cap: then nothing is written).  HM_ESTATE without option "partitions" = 2 when the planes are NULL,
 * HM_EINVAL for min_cov < 1, lo > hi, or a mix of NULL and non-NULL planes. */
int64_t hm_pileup_fetch_asm(hm_pileup_t* p, const void* pcov1, const void* ncov1, const void* pcov2, const void* ncov2,
                            const void* key, int64_t plane_base, int64_t lo, int64_t hi, int32_t min_cov,
                            hm_asm_t* out, int64_t cap);

/* ---- Benjamini-Hochberg q-values of the test above (`pileup -H -A -Q`) -------------------------------------
 * pvalue is a function of (pcov1, ncov1, pcov2, ncov2) alone, so the q of a locus -- R's p.adjust(method = "BH") among all tested
 * loci of its context, min(key & 3, 2) -- needs only the number of tested loci per tuple: the device counts them
 * (hm_pileup_asm_histogram), computes the p of every tuple that occurs with the kernel that computes a row's
 * (hm_pileup_asm_bin_pvalues), the host solves the q-values once (hm_asm_qvalues) and the device writes the rows by lookup
 * (hm_pileup_fetch_asm_q); no p-value is sorted on the device or exchanged between ranks, and the q next to a p is the q of that
 * exact double.  Tuples with both haplotype totals < HM_ASM_T are dense: with pair(p, n) = t (t + 1) / 2 + p, t = p + n, they fall
 * in bin (c * HM_ASM_PAIRS + pair(pcov1, ncov1)) * HM_ASM_PAIRS + pair(pcov2, ncov2); a tested locus with either total >=
 * HM_ASM_T is "big" and listed instead.  The device bins (104 MB) are allocated by the first of these calls.
 * In the three device calls the planes follow hm_pileup_fetch_asm: all five NULL = the engine's own, else DEVICE pointers whose
 * element 0 is locus plane_base; a mix is HM_EINVAL, NULL without partitions HM_ESTATE; min_cov >= 1 and lo <= hi as there. */
#define HM_ASM_T 64
#define HM_ASM_PAIRS 2080      /* HM_ASM_T (HM_ASM_T + 1) / 2 */
#define HM_ASM_BINS 12979200   /* 3 x 2080 x 2080 */
typedef struct {            /* the tested loci that share one dense tuple; 32 bytes */
    uint32_t bin, reserved;
    uint64_t count;
    double pvalue, qvalue;
} hm_asm_bin_t;
typedef struct {            /* hm_asm_t + qvalue: one row of <prefix>.asm.<ctx>.bed under -Q; 56 bytes */
    int64_t gpos;
    int32_t pcov1, ncov1, pcov2, ncov2;
    uint32_t motif, reserved;
    double diff, pvalue, qvalue;
} hm_asmq_t;
/* ADDS the tested loci of planes[lo, hi) whose haplotype totals are both < HM_ASM_T into the caller's bins[HM_ASM_BINS] and writes
 * the big ones to big[] in ascending order, as hm_pileup_fetch_asm would (diff and pvalue computed).  Returns the number of big
 * loci; when that exceeds cap, or big is NULL while there are some, nothing is written and nothing is added.  hi == lo returns 0. */
int64_t hm_pileup_asm_histogram(hm_pileup_t* p, const void* pcov1, const void* ncov1, const void* pcov2, const void* ncov2,
                                const void* key, int64_t plane_base, int64_t lo, int64_t hi, int32_t min_cov, uint64_t* bins,
                                hm_asm_t* big, int64_t cap);
/* The non-empty bins of bins[HM_ASM_BINS] (the job-wide sum) in ascending bin index, each with the pvalue the device computes for a
 * row carrying its tuple; qvalue = NaN.  Returns their number (may exceed cap: then nothing is written).  HM_EINVAL for a
 * non-empty bin of a tuple no tested locus has (a haplotype total of 0).  Needs neither reference nor planes. */
int64_t hm_pileup_asm_bin_pvalues(hm_pileup_t* p, const uint64_t* bins, hm_asm_bin_t* out, int64_t cap);
/* The q-values, host only (no device is touched): the one implementation behind every front end.  tab[0, n_tab): what
 * hm_pileup_asm_bin_pvalues gave; big[0, n_big): the big loci of the job.  A bin weighs `count` loci of context bin / HM_ASM_PAIRS^2,
 * a big locus one of context min(motif, 2); m[c] = tested loci of context c.  Per context, over the distinct p (bit-equal values
 * grouped) in ascending order: R = number of loci with p <= this one, q = min over this and all larger p of
 * min(1.0, p * (double)m / (double)R), left to right in fp64 -> tab[i].qvalue, big_q[i].  HM_EINVAL, with nothing written, for tab
 * not strictly ascending in bin (or a bin >= HM_ASM_BINS), count == 0, a p outside [DBL_MIN, 1] or NaN, a big locus with
 * motif > 3, negative counts or both totals < HM_ASM_T. */
int hm_asm_qvalues(hm_asm_bin_t* tab, int64_t n_tab, const hm_asm_t* big, int64_t n_big, double* big_q, uint64_t m[3]);
/* The rows of hm_pileup_fetch_asm for the same arguments, field for field, plus qvalue: a dense row's from the entry of its bin
 * in tab, a big row's from big_q at its gpos' place in big (both found by binary search; tab ascending in bin, big in gpos); NaN if
 * the entry is not there.  Returns the number of rows (may exceed cap: then nothing is written). */
int64_t hm_pileup_fetch_asm_q(hm_pileup_t* p, const void* pcov1, const void* ncov1, const void* pcov2, const void* ncov2,
                              const void* key, int64_t plane_base, int64_t lo, int64_t hi, int32_t min_cov,
                              const hm_asm_bin_t* tab, int64_t n_tab, const hm_asm_t* big, const double* big_q, int64_t n_big,
                              hm_asmq_t* out, int64_t cap);

/* ---- allele-specific methylated regions (`pileup -H -A -G`): runs of loci that lean the same way ----------
 * Per context c (0 CpG, 1 CHG, 2 CHH) and plane range [lo, hi).  ROWS r_0 .. r_{R-1}: the rows hm_pileup_fetch_asm returns for
 * [lo, hi) and min_cov whose min(motif, 2) == c, ascending in gpos (the rows of <prefix>.asm.<ctx>.bed for the range); a locus of
 * another context, or one that is not tested, is no row and neither links nor breaks anything.  Row i is a HIT when
 * pvalue_i <= max_p and diff_i != 0; its sign is +1 for diff_i > 0, -1 for diff_i < 0.  Rows i-1 and i are LINKED when both are
 * hits, of the same sign, and gpos_i - gpos_{i-1} <= max_gap.  A CHAIN is a maximal set of consecutively linked hits: a tested
 * row of the context that is no hit breaks it on purpose (it is evidence against the region); a single hit is a chain of one.
 * One hm_asm_region_t per chain: start = gpos of its first locus, end = gpos of its last + 1; pcov1 .. ncov2 the exact int64 sums
 * over its rows; diff = 100 * P1 / (P1 + N1) - 100 * P2 / (P2 + N2) on those pooled sums, the three correctly rounded fp64
 * operations of hm_asm_t::diff in the same order (bit-equal to the host's); pmin = the smallest pvalue among its rows, that row's
 * bits.  `sign` is the property of the LOCI: the pooled diff can have the other sign (Simpson's paradox) or be 0.  flags are
 * always set, whatever keep_edges is.  There is no region-level p-value: the loci were selected by their p, so a test of the
 * pooled counts would not be one.  The rows are a pure function of the hm_asm_t rows and (max_p, max_gap, min_loci, keep_edges):
 * integer sums only, nothing depends on launch geometry. */
#define HM_REGION_FIRST 1u  /* the chain contains r_0 */
#define HM_REGION_LAST 2u   /* the chain contains r_{R-1} */
typedef struct {            /* one chain = one row of <prefix>.asm.regions.<ctx>.bed; 80 bytes */
    int64_t start, end;
    int64_t pcov1, ncov1, pcov2, ncov2;
    int32_t n_loci, sign;
    uint32_t motif, flags;  /* motif = c */
    double diff, pmin;
} hm_asm_region_t;
/* The chains of context ctx in planes[lo, hi), ascending in start: those with n_loci >= min_loci and, when keep_edges != 0, also
 * every chain with flags != 0 whatever its length (what a caller needs to stitch adjacent ranges).  Planes as in
 * hm_pileup_fetch_asm.  Returns the number of regions (may exceed cap: then nothing is written); *n_ctx_rows, if not NULL,
 * receives R.  hi == lo returns 0.  HM_EINVAL for ctx outside 0..2, max_p NaN or outside (0, 1], max_gap < 1, min_loci < 1 and
 * what hm_pileup_fetch_asm refuses. */
int64_t hm_pileup_fetch_asm_regions(hm_pileup_t* p, const void* pcov1, const void* ncov1, const void* pcov2, const void* ncov2,
                                    const void* key, int64_t plane_base, int64_t lo, int64_t hi, int32_t min_cov, int32_t ctx,
                                    double max_p, int64_t max_gap, int32_t min_loci, int32_t keep_edges, int64_t* n_ctx_rows,
                                    hm_asm_region_t* out, int64_t cap);

/* ---- two samples instead of two haplotypes (`diff`): counts loaded into the partition planes -------------------
 * The three families above are functions of two pairs of count planes and a key plane; they know nothing about haplotypes.  This
 * call fills those planes from rows -- the rows of two samples' <prefix>.<ctx>.cov.bed files -- instead of from records, and the
 * engine then answers every fetch that works after hm_pileup_count (hm_pileup_fetch_loci, the asm family, regions, context,
 * domains, sites) as if part 1 and part 2 were HP 1 and HP 2.
 * rows[0, n): HOST memory, any order.  Each row is checked in this order, and the first failure names it: gpos in [0, total
 * reference length); pcov >= 0 and ncov >= 0; motif <= 3.  A row that passes and has pcov + ncov == 0 is ignored.  Every other
 * row ADDS pcov / ncov to the planes of `part` (1 or 2) and to the combined planes -- which so hold the pooled sample -- and
 * raises the key plane at gpos to max(key, motif): where the two samples disagree about a locus' context the LARGER code wins;
 * the `order` bits of the key stay 0.
 * THE DUPLICATE RULE, for this call and for hm_pileup_load_sample_loci and hm_sample_load below.  A row that passes the checks and
 * carries a count is a duplicate exactly when an earlier or concurrent row of the same locus was given to the same TARGET: here
 * the part, there the open sample.  The window runs from when the target's planes were last cleared or opened (here: the
 * first call with rows, or hm_pileup_use_partition_planes for that part after it), across slabs and across calls.  Of k such
 * rows on one locus exactly k - 1 are counted as duplicates, whatever the launch geometry, the order of the rows or
 * "load_slab": the engine decides by one atomic operation on one word per locus and target (here a bit of the part's seen
 * bitmap: 1 bit per base and part, +0.25 B per reference base from the first call with rows on).  What a duplicate adds is
 * each call's own: here it still adds; in the other two it adds nothing and which row wins is open.  Counts that planes
 * registered with hm_pileup_use_partition_planes held beforehand are not rows and make nothing a duplicate.  The pooled counts
 * of a locus must stay below 2^31 (not checked).
 * Returns the number of rows that added a count.  If any row was bad (out of range, negative, motif, duplicate): HM_EDATA,
 * hm_pileup_last_error gives their number and the number of each kind, and the planes mean nothing any more (the good rows and
 * the duplicates were added): every further load, and every fetch over the engine's own planes, returns HM_ESTATE.
 * HM_ESTATE also without option "partitions" = 2, before hm_pileup_set_reference (planes registered with hm_pileup_use_planes /
 * _use_partition_planes are loaded into, but the reference gives the length), and on an engine that ever staged a record:
 * counts come from records or from loads, never both, and after a successful load hm_pileup_submit_read* return HM_ESTATE.
 * HM_EINVAL for part outside {1, 2}, n < 0, or rows NULL with n > 0.  May be called any number of times, for either part, in any
 * interleaving.  The rows go through one device slab of "load_slab" rows (option, 1 .. 2^24, default 2^20 = 24 MB; may be set at
 * any time), slab by slab on the engine's stream: no device memory grows with n.  All adds are integer atomics: the planes depend
 * on neither row order, slab size nor launch geometry.  Not here: pileup_dist (one card holds both samples of a human genome at
 * 28.25 B per base), more than two samples (replicates in two groups: hm_pileup_group_sample below). */
int64_t hm_pileup_load_loci(hm_pileup_t* p, int32_t part, const hm_locus_t* rows, int64_t n);

/* ---- replicate groups (`groupdiff`): several samples per part, tested with their spread ---------------------
 * Sample i of group g in {1, 2} has, at a locus, k_i methylated and n_i total calls.  The sample COUNTS at the locus when
 * n_i >= c, the per-sample minimum coverage (option "group_min_cov").  Over the counting samples of a group:
 *   m_g = their number,  K_g = sum k_i,  N_g = sum n_i,  Q_g = sum q_i,  q_i = floor(k_i^2 * 2^20 / n_i)
 * q_i is an integer (n_i < 2^20, so k_i^2 * 2^20 < 2^60), which makes Q_g -- the one moment the statistic needs beyond the pooled
 * counts -- additive over samples in integer atomics, exactly as the planes are.  A locus is TESTED when m_1 >= r, m_2 >= r and
 * nu = m_1 + m_2 - 2 >= 1 (r = min_reps).  With ph_g = K_g / N_g, ph_0 = (K_1 + K_2) / (N_1 + N_2) and 0 * log(.) = 0:
 *   diff = 100 K_1 / N_1 - 100 K_2 / N_2                       (rounded as hm_asm_t's diff)
 *   D    = 2 sum_g [ K_g log(ph_g / ph_0) + (N_g - K_g) log((1 - ph_g) / (1 - ph_0)) ]       the binomial likelihood ratio, 1 df, >= 0
 *   X2   = sum_g (Q_g 2^-20 - K_g^2 / N_g) / (ph_g (1 - ph_g))    Pearson's statistic of the two-proportion fit; a group with ph_g
 *                                                              in {0, 1} contributes 0, a negative term (the floor in q_i) counts 0
 *   phi  = max(1, X2 / nu),   F = D / phi,   pvalue = P(F(1, nu) >= F) = I_{nu / (nu + F)}(nu / 2, 1 / 2)
 * pvalue is exactly 1 when D == 0 and never 0 (below DBL_MIN it is reported as DBL_MIN).  With phi floored at 1 a locus is never
 * more significant than under the plain binomial model.  This is this library's own definition, not another tool's.
 *
 * Option "groups" (0 default, 1): needs "partitions" = 2 and must be set before hm_pileup_set_reference (else HM_ESTATE), which then
 * also allocates and zeroes, per group, a uint64 moment plane (Q_g) and a uint8 sample-count plane (m_g), and one `seen` bitmap of
 * 1 bit per base (the open sample's: a group's samples share a part on purpose, so nothing is decided per part here):
 * 18.125 B per reference base more.  Without the option nothing is allocated.  Option "group_min_cov" (c: integer >= 1,
 * default 5): HM_ESTATE once a sample has been opened. */
typedef struct {            /* one tested locus = one row of <prefix>.groups.<ctx>.bed; 64 bytes */
    int64_t gpos;
    int32_t pcov1, ncov1, pcov2, ncov2;   /* K_1, N_1 - K_1, K_2, N_2 - K_2 */
    uint32_t motif;
    uint16_t m1, m2;
    double diff, D, phi, pvalue;
} hm_group_t;
/* Opens the next sample of group `part` (1 or 2) and clears the seen bitmap: the rows of hm_pileup_load_sample_loci belong to it
 * until the next call.  Returns the sample's index within its group (0, 1, ...).  HM_EINVAL for a bad part; HM_ESTATE without option
 * "groups" or before hm_pileup_set_reference, on an engine voided by a bad row, on one that staged records or used
 * hm_pileup_load_loci, and for the 256th sample of a group (the sample counts are bytes). */
int hm_pileup_group_sample(hm_pileup_t* p, int32_t part);
/* rows[0, n) of the open sample: HOST memory, any order, any number of calls; they pass through the slab of hm_pileup_load_loci
 * (option "load_slab").  Each row is checked in this order, the first failure names it: gpos in [0, total reference length);
 * pcov >= 0 and ncov >= 0; pcov + ncov < 2^20; motif <= 3.  A row that passes and has no count is ignored.  A row whose seen bit
 * was already set -- the locus came before in THIS sample -- is a duplicate and adds nothing; the same locus in another sample
 * is the point of the exercise.  A row with pcov + ncov < c sets its bit and adds nothing.  Every other row adds pcov / ncov to
 * the group's partition planes and to the combined planes, raises the key to its motif (as hm_pileup_load_loci), adds q_i to the
 * group's moment plane and 1 to its sample count.  Integer atomics only: the planes depend on neither row order, slab size nor
 * launch geometry.  Returns the number of rows that added.  Any bad row: HM_EDATA, hm_pileup_last_error gives the number of each
 * kind, and the engine is void as after hm_pileup_load_loci.  HM_ESTATE before hm_pileup_group_sample; once a sample has been
 * opened hm_pileup_load_loci and hm_pileup_submit_read* return HM_ESTATE, and the other way round.  HM_EINVAL for n < 0 or rows NULL with
 * n > 0.  The other fetches over the engine's planes see the pooled group counts: hm_pileup_fetch_asm is the pooled Fisher test. */
int64_t hm_pileup_load_sample_loci(hm_pileup_t* p, const hm_locus_t* rows, int64_t n);
/* The tested loci of the engine's planes [lo, hi) in ascending order, with diff, D, phi and pvalue computed on the device (fp64;
 * the incomplete beta function by its continued fraction).  Returns their number (may exceed cap, or out NULL: then nothing is
 * written).  hi == lo returns 0.  HM_ESTATE without option "groups", before hm_pileup_set_reference or on a voided engine;
 * HM_EINVAL for min_reps outside 1 .. 255, lo < 0, lo > hi or hi past the reference. */
int64_t hm_pileup_fetch_groups(hm_pileup_t* p, int64_t lo, int64_t hi, int32_t min_reps, hm_group_t* out, int64_t cap);
/* The moment and sample-count planes of group `part` over [lo, hi), copied to HOST memory: moment[hi - lo] and samples[hi - lo],
 * either may be NULL.  For tests and for callers that keep their own statistics.  Errors as hm_pileup_fetch_groups. */
int hm_pileup_group_planes(hm_pileup_t* p, int32_t part, int64_t lo, int64_t hi, uint64_t* moment, uint8_t* samples);
/* Host only.  q[i] = the Benjamini-Hochberg value of rows[i].pvalue among the rows of its context, min(motif, 2) (R's
 * p.adjust(method = "BH")): equal p gives equal q.  m[ctx] receives the number of rows per context.  HM_EINVAL for a motif above 3
 * or a pvalue outside [DBL_MIN, 1]. */
int hm_group_qvalues(const hm_group_t* rows, int64_t n, double* q, uint64_t m[3]);
/* Differentially methylated regions between the groups (`groupdmr`): the chains of hm_asm_region_t above, over group rows.  Per
 * context c and plane range [lo, hi).  ROWS r_0 .. r_{R-1}: the rows hm_pileup_fetch_groups returns for [lo, hi) and min_reps whose
 * min(motif, 2) == c, ascending in gpos, each with the diff and pvalue of that call, bit for bit (the same kernel, a pure function
 * of the planes at the locus); a locus of another context, or one that is not tested, is no row and neither links nor breaks
 * anything.  Row i is a HIT when pvalue_i <= max_p, diff_i != 0 and |diff_i| >= min_diff; its sign is that of diff_i.  LINKED,
 * CHAIN, start, end, the four sums, diff, pmin, sign, flags and what is returned for (min_loci, keep_edges): word for word as for
 * hm_asm_region_t -- a tested row of the context that is no hit breaks a chain.  Also per chain: phi_max = the largest phi among
 * its rows, that row's bits; m1_min / m2_min = the smallest m1 / m2 among its rows.  Comparisons and integer sums only: nothing
 * depends on launch geometry.  There is no region-level p-value, for the reason given there; a test of the samples' levels over
 * these regions (hm_sample_interval_test) is descriptive only when it uses the samples the regions were found from. */
typedef struct {            /* one chain = one row of <prefix>.groupdmr.<ctx>.bed; 96 bytes */
    int64_t start, end;
    int64_t pcov1, ncov1, pcov2, ncov2;   /* exact sums of the rows' pooled group counts */
    int32_t n_loci, sign;
    uint32_t motif, flags;                /* motif = c; HM_REGION_FIRST / HM_REGION_LAST */
    uint16_t m1_min, m2_min;              /* fewest counting samples of a group at any locus of the chain */
    uint32_t reserved;                    /* 0 */
    double diff, pmin, phi_max;
} hm_group_region_t;
/* The chains of context ctx in the engine's planes [lo, hi), ascending in start: those with n_loci >= min_loci and, when
 * keep_edges != 0, also every chain with flags != 0 whatever its length.  The rows are staged and tested on the device and never
 * visit the host (64 B per row of the context in a buffer the first call allocates).  Returns the number of regions (may exceed
 * cap, or out NULL: then nothing is written); *n_ctx_rows receives R and *n_hits the number of hits, either may be NULL.  hi == lo
 * returns 0.  Errors as hm_pileup_fetch_groups; HM_EINVAL also for ctx outside 0..2, max_p NaN or outside (0, 1], min_diff NaN or
 * outside [0, 100], max_gap < 1 and min_loci < 1. */
int64_t hm_dmr_fetch_regions(hm_pileup_t* p, int64_t lo, int64_t hi, int32_t min_reps, int32_t ctx, double max_p, double min_diff,
                             int64_t max_gap, int32_t min_loci, int32_t keep_edges, int64_t* n_ctx_rows, int64_t* n_hits,
                             hm_group_region_t* out, int64_t cap);
/* Host only.  cutoff[c] = the largest pvalue among the rows of context c whose q is <= max_q, or 0 when there is none; q = what
 * hm_group_qvalues gave for the same rows.  BH q is monotone in p, so {q <= max_q} == {pvalue <= cutoff[c]}: chaining "by q" is
 * hm_dmr_fetch_regions with max_p = cutoff[c], and a context whose cutoff is 0 has no regions.  HM_EINVAL for max_q NaN
 * or outside (0, 1] and for what hm_group_qvalues refuses. */
int hm_dmr_p_cutoff(const hm_group_t* rows, const double* q, int64_t n, double max_q, double cutoff[3]);

/* ---- N samples (`samplecorr`): the sample-by-sample correlation matrix per context ---------------------------
 * There are N samples, 2 <= N <= 64 (HM_SAMPLE_MAX).  Sample s has, at a locus, k methylated and n total calls.  It COUNTS there
 * when n >= c, the per-sample minimum coverage (option "sample_min_cov", default 5, range 1 .. 2^20 - 1), and its LEVEL there is
 * the integer u = floor(k * 2^15 / n) in [0, 32768].  The context of a locus is min(key & 3, 2), as everywhere else.
 * For a context, a pair i <= j and a set of loci, take the loci where both i and j count -- in COMPLETE mode the loci where all
 * the samples opened so far count -- and over those loci
 *   n = their number,  si = sum u_i,  sj = sum u_j,  sii = sum u_i^2,  sjj = sum u_j^2,  sij = sum u_i u_j
 * All six are uint64 and exact: with u^2 <= 2^30 none overflows below 2^33 loci.  The diagonal i = j carries a sample's own locus
 * count and moments.  With num = n sij - si sj, va = n sii - si^2 and vb = n sjj - sj^2 computed exactly in 128-bit integers and
 * each converted to double once,
 *   r = num / (sqrt(va) * sqrt(vb)),  NaN when n < 2, va = 0 or vb = 0;   mean level in percent = 100 si / (n 2^15), NaN when n = 0
 * This is Pearson's r of the QUANTISED levels u, not of the ratios k / n: this library's own definition, not another tool's.  The
 * sums are integers, so they depend on no order; floating point appears in hm_sample_corr only, on the host.
 *
 * Option "samples" (0 default, or N in 2 .. 64): must be set before hm_pileup_set_reference (else HM_ESTATE), which then also
 * allocates and zeroes N uint16 level planes, 2 N bytes per reference base; a reference that does not fit fails as for the other
 * planes.  Without the option nothing is allocated.  It needs neither "partitions" nor "groups".  Option "sample_min_cov" (c):
 * HM_ESTATE once a sample has been opened.  A plane stores per locus 0 (nothing seen), u + 1 (the sample counts), or 0xFFFF (seen,
 * below c).  The calls of this family are named hm_sample_*; those that take the engine take the hm_pileup_t they belong to. */
#define HM_SAMPLE_MAX 64   /* samples of one engine */
#define HM_SAMPLE_TILE 256 /* consecutive positions a workgroup of hm_sample_fetch_sums takes at a time; tiles start at multiples of it */
int hm_sample_geometry(int64_t out[2]); /* out[0] = HM_SAMPLE_TILE, out[1] = HM_SAMPLE_MAX as the library was built */
typedef struct {            /* the sums of one context and one pair i <= j; 64 bytes */
    int32_t i, j;
    uint32_t ctx, reserved;
    uint64_t n, si, sj, sii, sjj, sij;
} hm_sample_pair_t;
/* Opens the next sample: the rows of hm_sample_load belong to it until the next call.  Returns its index 0 .. N - 1.
 * HM_ESTATE without option "samples" or before hm_pileup_set_reference, on an engine voided by a bad row, on one that staged a
 * record or used hm_pileup_load_loci / hm_pileup_group_sample, and for sample N + 1.  Once a sample is open, hm_pileup_load_loci,
 * hm_pileup_group_sample and hm_pileup_submit_read* return HM_ESTATE. */
int hm_sample_open(hm_pileup_t* p);
/* rows[0, n) of the open sample: HOST memory, any order, any number of calls; they pass through the slab of hm_pileup_load_loci
 * (option "load_slab").  Each row is checked as hm_pileup_load_sample_loci checks it, in this order, the first failure names it:
 * gpos in [0, total reference length); pcov >= 0 and ncov >= 0; pcov + ncov < 2^20; motif <= 3.  A row that passes and has no
 * count is ignored.  A row whose locus already holds a non-zero value of THIS sample is a duplicate and adds nothing -- counting
 * or not, and of two rows of one locus in one call exactly one is the duplicate.  Every other row writes the sample's value at
 * its locus and raises the key to its motif; if the sample counts there it also adds pcov / ncov to the engine's combined planes,
 * so hm_pileup_fetch_loci sees the pooled counting samples.  The planes depend on neither row order, slab size nor launch
 * geometry.  Returns the number of rows that wrote a value.  Any bad row (duplicates are one kind): HM_EDATA,
 * hm_pileup_last_error gives the number of each kind, and the engine is void as after hm_pileup_load_loci.  HM_ESTATE before
 * hm_sample_open; HM_EINVAL for n < 0 or rows NULL with n > 0. */
int64_t hm_sample_load(hm_pileup_t* p, const hm_locus_t* rows, int64_t n);
/* The sums over the loci of [lo, hi) for the M samples opened so far: 3 M (M + 1) / 2 entries into out (HOST memory), context-major,
 * then i, then j >= i; returns their number.  complete: 0 pairwise, 1 complete mode.  hi == lo gives all-zero sums.  The sums over
 * [lo, m) plus those over [m, hi) equal those over [lo, hi), entry for entry.  HM_EINVAL for lo < 0, lo > hi, hi past the
 * reference, complete outside {0, 1} or out NULL; HM_ESTATE without option "samples", before hm_pileup_set_reference or on a
 * voided engine. */
int64_t hm_sample_fetch_sums(hm_pileup_t* p, int64_t lo, int64_t hi, int32_t complete, hm_sample_pair_t* out);
/* The stored values of sample s (0 .. N - 1; an unopened one is all 0) over [lo, hi), copied to HOST memory: out[hi - lo].  For
 * tests, as hm_pileup_group_planes.  Errors as hm_sample_fetch_sums; HM_EINVAL for a bad s. */
int hm_sample_plane(hm_pileup_t* p, int32_t s, int64_t lo, int64_t hi, uint16_t* out);
/* Host only.  r[k], mean_i[k], mean_j[k] of e[k] by the formula above, k in [0, n); each of the three may be NULL.  HM_EINVAL for
 * n < 0 or e NULL with n > 0. */
int hm_sample_corr(const hm_sample_pair_t* e, int64_t n, double* r, double* mean_i, double* mean_j);

/* ---- N samples over given intervals (`regiondiff`): a two-group test of each interval ------------------------
 * The planes are those of the family above.  M is the number of samples opened so far.  For interval i = [start, end), in global
 * plane coordinates and clamped to [lo, hi), a context ctx and a sample s < M, take the loci g of the interval with
 * min(key[g] & 3, 2) == ctx at which s counts (its plane value is neither 0 nor 0xFFFF) -- in COMPLETE mode only the loci at which
 * all M samples count -- and over those loci
 *   n = their number,  su = the sum of the levels u = value - 1
 * Both are uint64 and exact; they are sums of integers, so they depend on neither the launch geometry nor the order of the
 * intervals, and the sums over [lo, m) plus those over [m, hi) equal those over [lo, hi) for every interval and sample.
 * The index the call builds (per sample a running sum over blocks of HM_REGION_BLOCK positions, 16 M bytes per block) lives in a
 * buffer of the engine that grows on demand and is rebuilt by every call; an engine that never calls this allocates none. */
typedef struct {            /* one (interval, sample); 16 bytes */
    uint64_t n, su;
} hm_sample_interval_t;
/* The sums of n_iv intervals (start[i], end[i]: HOST memory; any order; they may overlap, repeat, be empty or lie outside
 * [lo, hi)) into out[i * M + s] (HOST memory); returns n_iv * M (0 with no sample open).  hi == lo gives zeros.  HM_EINVAL for
 * lo < 0, lo > hi, hi past the reference, ctx outside 0 .. 2, complete outside {0, 1}, n_iv < 0, start, end or out NULL with
 * n_iv > 0, or an interval with start > end; HM_ESTATE without option "samples", before hm_pileup_set_reference or on a voided
 * engine, as hm_sample_fetch_sums. */
int64_t hm_sample_fetch_intervals(hm_pileup_t* p, int64_t lo, int64_t hi, int32_t ctx, int32_t complete, const int64_t* start,
                                  const int64_t* end, int64_t n_iv, hm_sample_interval_t* out);
/* Host only: Welch's t-test of two groups of samples on their interval levels.  This is this library's own statistic -- a t-test
 * on per-sample interval means, as tile-based tools do it -- not another tool's.  sums[i * M + s] as above; group[s] is 1 or 2,
 * or 0 for a sample that takes no part.  Sample s is USED in interval i when n_s >= min_loci (>= 1); its level there is
 * x_s = 100 su_s / (n_s 2^15) percent.  Per group g: m_g = its used samples, n_g = the sum of their n_s, mean_g = the mean of
 * their x_s (NaN when m_g = 0), V_g = their sample variance (two passes, samples in ascending index).  An interval is TESTED
 * when m_1 >= min_reps and m_2 >= min_reps, min_reps in 2 .. 64.  With se2 = V_1 / m_1 + V_2 / m_2:
 *   t = (mean_1 - mean_2) / sqrt(se2),  df = se2^2 / ((V_1 / m_1)^2 / (m_1 - 1) + (V_2 / m_2)^2 / (m_2 - 1))  (Welch-Satterthwaite),
 *   pvalue = I_{df / (df + t^2)}(df / 2, 1 / 2), two-sided, never below DBL_MIN.
 * se2 = 0 with equal means: t = 0, df = m_1 + m_2 - 2, pvalue = 1; with unequal means: t = +-inf, df = NaN, pvalue = NaN (the
 * data give no yardstick; the interval takes no part in hm_sample_qvalues).  An untested interval has t = df = pvalue = NaN.
 * HM_EINVAL for n_iv < 0, M outside 1 .. 64, a NULL pointer with n_iv > 0, group NULL or a group value above 2, min_loci < 1 or
 * min_reps outside 2 .. 64. */
typedef struct {            /* one interval; 64 bytes */
    int32_t m1, m2;
    uint64_t n1, n2;
    double mean1, mean2, t, df, pvalue;
} hm_sample_test_t;
int hm_sample_interval_test(const hm_sample_interval_t* sums, int64_t n_iv, int32_t M, const uint8_t* group, int64_t min_loci,
                            int32_t min_reps, hm_sample_test_t* out);
/* Host only: Benjamini-Hochberg q-values of p[0, n) among its finite entries, as hm_group_qvalues; q[i] = NaN where p[i] is NaN,
 * equal p give equal q.  HM_EINVAL for n < 0, a NULL pointer with n > 0, or a p that is neither NaN nor in [DBL_MIN, 1]. */
int hm_sample_qvalues(const double* p, int64_t n, double* q);

/* ---- per-locus binomial test (`pileup -B / -e`): is a locus methylated at all ------------------------
 * Against a false-positive rate e per context -- given, or measured on an unmethylated control sequence as sum(pcov) /
 * sum(pcov + ncov) -- a covered locus with k = pcov, n = pcov + ncov gets p = P(X >= k), X ~ Binomial(n, e), and the
 * Benjamini-Hochberg q of that p among all covered loci of its context.  p and q are functions of (motif, k, n) alone, so the
 * device counts loci per triple (hm_pileup_site_histogram), the host solves the table once (hm_sites_table) and the device
 * writes the rows by lookup (hm_pileup_fetch_sites); no p-value is sorted or exchanged.
 * In the three device calls the planes follow hm_pileup_fetch_loci: all of pcov / ncov / key NULL = the engine's own combined
 * planes (plane_base is then 0), else DEVICE pointers whose element 0 is locus plane_base; [lo, hi) in plane coordinates.  A
 * locus takes part when pcov >= 0, ncov >= 0 and pcov + ncov > 0 (a negative value in caller-owned planes is no count: such a
 * locus is skipped); its context is min(key & 3, 2), the file the BED writers put it in. */
typedef struct {            /* one row of <prefix>.sites.<ctx>.bed; 40 bytes */
    int64_t gpos;
    int32_t pcov, ncov;
    uint32_t motif, reserved;
    double pvalue, qvalue;
} hm_site_t;
#define HM_SITE_BINS 196608 /* 3 x 256 x 256: index (motif * 256 + n) * 256 + k, for n < 256 */
/* sums[c] = sum of pcov, sums[3 + c] = sum of ncov over the loci of context c in planes[lo, hi) (the control sequence, or a
 * rank's part of it); exact.  There is no plane_base: nothing positional is returned. */
int hm_pileup_control_sums(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t lo, int64_t hi,
                           uint64_t sums[6]);
/* ADDS the loci of planes[lo, hi) with n < 256 into the caller's bins[HM_SITE_BINS] and writes those with n >= 256 (an organelle
 * at thousands-fold coverage) to big[] in ascending order.  Returns the number of big loci; when that exceeds cap, or big is
 * NULL while there are some, nothing is written and nothing is added.  hi == lo returns 0. */
int64_t hm_pileup_site_histogram(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base,
                                 int64_t lo, int64_t hi, uint64_t* bins, hm_locus_t* big, int64_t cap);
/* The test and the q-values, host only (no device is touched): the one implementation behind every front end.
 * rates[c] in [0, 1], or NaN = context c is not tested.  bins / big: what hm_pileup_site_histogram gave, summed / concatenated
 * over the job.  For every (c, n, k) with k <= n < 256 of a tested context ptab[(c * 256 + n) * 256 + k] is
 *   1.0 if k == 0 or e == 1;  DBL_MIN if e == 0 (and k > 0);  else the sum over x = k .. n, ascending, in fp64, of
 *   exp(((lf(n) - lf(x)) - lf(n - x)) + (x * log(e) + (n - x) * log1p(-e))),  lf(j) = lgamma(j + 1) of the host's libm,
 * clamped to [DBL_MIN, 1] (never 0, as hm_asm_t::pvalue); every other entry of ptab is NaN.  big_p[i] is the same for big[i].
 * m[c] = number of loci of context c (bins + big).  q (R's p.adjust(method = "BH") within the context): over the distinct p in
 * ascending order, R = number of loci with p <= this one, q = min over this and all larger p of min(1, p * (double)m / (double)R);
 * qtab is filled where the bin is not empty (NaN elsewhere), big_q[i] for every big locus of a tested context (NaN otherwise).
 * HM_EINVAL for a rate outside [0, 1], a non-empty bin with k > n or n == 0, a big locus with motif > 2, negative counts or
 * n < 256. */
int hm_sites_table(const double rates[3], const uint64_t* bins, const hm_locus_t* big, int64_t n_big, double* ptab,
                   double* qtab, double* big_p, double* big_q, uint64_t m[3]);
/* rows of planes[lo, hi) in ascending order: the loci above whose context has bit `motif` set in ctx_mask (the tested contexts),
 * pvalue / qvalue from ptab / qtab[HM_SITE_BINS] for n < 256, else from big_p / big_q at the locus' place in big[0, n_big) --
 * the job-wide list, ascending in gpos; NaN if it is not there.  Returns the number of rows (may exceed cap: then nothing is
 * written). */
int64_t hm_pileup_fetch_sites(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base,
                              int64_t lo, int64_t hi, int32_t ctx_mask, const double* ptab, const double* qtab,
                              const hm_locus_t* big, const double* big_p, const double* big_q, int64_t n_big,
                              hm_site_t* out, int64_t cap);

/* ---- methylation domains (`pileup -D`): low and high stretches by a two-state Viterbi scan ---------------
 * Per context c (0 CpG, 1 CHG, 2 CHH) and plane range [lo, hi).  ROWS r_0 .. r_{R-1}: the loci of the range with pcov >= 0,
 * ncov >= 0, pcov + ncov > 0 (the loci of the binomial test above) and min(key & 3, 2) == c, ascending in gpos; any other locus
 * is no row and neither links nor breaks anything.
 * Two states, 0 = low and 1 = high, and integer parameters in Q16 fixed-point nats: A in (0, 2^24] the weight of a methylated
 * read, B in [-2^24, 0) that of an unmethylated one, S in [0, 2^24] the switch penalty; max_gap >= 1.  Row t with
 * k = min(pcov, 2^20 - 1), u = min(ncov, 2^20 - 1) scores e_t = k * A + u * B in state 1 and 0 in state 0.  A change of state
 * between rows t-1 and t costs S_t = S when gpos_t - gpos_{t-1} <= max_gap, and S_t = 0 (a BREAK) otherwise and for t = 0.  The
 * path z maximises sum e_t z_t - sum over t >= 1 with z_t != z_{t-1} of S_t.  Among the optimal paths it is the one of plain
 * sequential Viterbi from delta_{-1} = (0, 0) whose back-pointers move only on a strict gain: into state 0 from 1 only if
 * delta(1) - S_t > delta(0), into state 1 from 0 only if delta(0) - S_t > delta(1), and the end state is 1 only if
 * delta_{R-1}(1) > delta_{R-1}(0).
 * A SEGMENT is a maximal run of consecutive rows with equal state and no break inside; the segments partition the rows.  One
 * hm_domain_t per segment: start = gpos of its first row, end = gpos of its last + 1; pcov / ncov the exact sums of the unclamped
 * counters; level = 100 * P / (P + N), rounded like hm_asm_t::diff; score = ((double)P * (double)A + (double)N * (double)B) /
 * 65536.0, four correctly rounded fp64 operations in this order without contraction (bit-equal to the host's): the pooled
 * log-likelihood ratio high : low in nats, for ranking.  Everything is an exact integer function of the planes and
 * (A, B, S, max_gap): nothing depends on launch geometry. */
#define HM_DOMAIN_AFTER_BREAK 1u  /* the first row follows a break or is r_0 */
#define HM_DOMAIN_BEFORE_BREAK 2u /* the last row precedes a break or is r_{R-1} */
typedef struct {                  /* one segment = one row of <prefix>.domains.<ctx>.bed; 64 bytes */
    int64_t start, end;
    int64_t pcov, ncov;
    int32_t n_loci;
    uint32_t state, motif, flags; /* state 0 low / 1 high; motif = c */
    double level, score;
} hm_domain_t;
/* The segments of context ctx in planes[lo, hi), ascending in start.  Planes as in hm_pileup_fetch_loci.  Returns the number of
 * segments (may exceed cap: then nothing is written); *n_ctx_rows, if not NULL, receives R.  hi == lo returns 0.  HM_EINVAL for
 * A, B, S or max_gap outside the ranges above, ctx outside 0..2, lo > hi, and a range over the engine's own planes that ends
 * past the reference. */
int64_t hm_pileup_fetch_domains(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base,
                                int64_t lo, int64_t hi, int32_t ctx, int64_t A, int64_t B, int64_t S, int64_t max_gap,
                                int64_t* n_ctx_rows, hm_domain_t* out, int64_t cap);
/* The same segments from PIECES (`pileup_dist -D`).  Cut [lo, hi) into consecutive pieces in any way -- empty
 * ones, pieces without a row of the context, pieces of separate planes with their own plane_base: the segments of the pieces,
 * chained as below and joined where a segment crosses a cut, are those of one hm_pileup_fetch_domains over [lo, hi), byte for byte.
 * Every pass is stateless (it compacts the piece's rows and scans them again) and takes and gives O(1) bytes in hm_domain_part_t:
 *   pass S (HM_DOMAIN_PASS_SUMMARY), no input: n_rows = R, first_gpos, last_gpos, e_first = e of row 0, and (c, lo, hi), the
 *     function x -> clamp(x + c, lo, hi) that takes d of row 0 to d of row R - 1 (the identity c = 0, lo = -2^62, hi = 2^62 for
 *     R = 1).  Once |c| >= 2^48 the function is constant on [-2^46, 2^46] and given as lo == hi; apply it to values within
 *     +-2^46 only, as min(max(x + c, lo), hi), and never compose two of them.
 *   pass C (HM_DOMAIN_PASS_CODES), input has_prev, prev_gpos, prev_d -- whether a row of the context precedes the piece, and the
 *     nearest one's locus and d: d_last = d of row R - 1, and back = the state of row 0 as a function of the state of row R - 1:
 *     0, 1 or HM_DOMAIN_KEEP (the same state).  d of row 0 is clamp(prev_d, -S_0, S_0) + e_first with S_0 = S if has_prev and
 *     first_gpos - prev_gpos <= max_gap, else clamp(0, 0, 0) + e_first.
 *   pass G (HM_DOMAIN_PASS_SEGMENTS), input as pass C and has_next, next_gpos, last_state -- whether a row follows the piece, the
 *     nearest one's locus, and the state of row R - 1 (0 or 1; without has_next it is d_last > 0): the segments in out[cap] as
 *     hm_pileup_fetch_domains writes them, except that row 0 starts a segment of its own whatever precedes it (joining is the
 *     caller's), and HM_DOMAIN_AFTER_BREAK / HM_DOMAIN_BEFORE_BREAK at the piece's edges say whether prev / next is missing or
 *     more than max_gap away.  Also d_last.
 * The caller chains: d from left to right through e_first and (c, lo, hi); then from right to left the state of a piece's last
 * row -- 1 if d_last > S_link, 0 if d_last < -S_link, else the next piece's first state, S_link = S or 0 by the gap between the
 * two rows -- and of its first row (back applied to it).  Passes S and C return R, pass G the number of segments (may exceed cap:
 * then none is written); all three fill n_rows, first_gpos, last_gpos, e_first when R > 0 and only n_rows = 0 otherwise.
 * Errors as hm_pileup_fetch_domains, and HM_EINVAL for a pass outside 0..2, part NULL, has_prev with prev_d outside
 * [-2^46, 2^46] or prev_gpos negative or not below plane_base + lo, has_next with next_gpos below plane_base + hi or last_state
 * not 0 or 1. */
#define HM_DOMAIN_PASS_SUMMARY 0
#define HM_DOMAIN_PASS_CODES 1
#define HM_DOMAIN_PASS_SEGMENTS 2
#define HM_DOMAIN_KEEP 2
typedef struct {                             /* 104 bytes */
    int64_t prev_gpos, prev_d, next_gpos;    /* in */
    int32_t has_prev, has_next, last_state;  /* in */
    int32_t back;                            /* out, pass C */
    int64_t n_rows, first_gpos, last_gpos, e_first; /* out */
    int64_t c, lo, hi;                       /* out, pass S */
    int64_t d_last;                          /* out, passes C and G */
} hm_domain_part_t;
int64_t hm_pileup_fetch_domains_part(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base,
                                     int64_t lo, int64_t hi, int32_t ctx, int64_t A, int64_t B, int64_t S, int64_t max_gap,
                                     int32_t pass, hm_domain_part_t* part, hm_domain_t* out, int64_t cap);
/* Host only.  The weights for two methylation levels 0 < level_lo < level_hi < 1 (fractions) and a switch penalty in nats:
 * A = llround(65536 * log(level_hi / level_lo)), B = llround(65536 * log((1 - level_hi) / (1 - level_lo))),
 * S = llround(65536 * penalty) -- a read's log-likelihood ratio high : low.  HM_EINVAL unless 0 < level_lo < level_hi < 1,
 * penalty >= 0 and the results lie in hm_pileup_fetch_domains' ranges. */
int hm_domain_scores(double level_lo, double level_hi, double penalty, int64_t* A, int64_t* B, int64_t* S);

/* ---- the two levels fitted from the data (`pileup -D -Y`): hard EM (Viterbi training) ---------------------
 * Fix a context c, penalty, max_gap, starting levels (l_0, h_0) and max_iter >= 1.  A CHAIN is one sequence of the reference: one
 * [lo, hi) of hm_pileup_fetch_domains.  Iteration i = 0, 1, ...:
 *   1. (A_i, B_i, S) = hm_domain_scores(l_i, h_i, penalty).  An error ends the fit with status `degenerate` and iteration i - 1's
 *      levels; for i = 0 it is the caller's error.
 *   2. STATE SUMS (P0, N0, R0, P1, N1, R1): over all rows of context c in all chains the exact int64 sums of the unclamped pcov
 *      and ncov and the number of rows, by the row's state z_t.  Rows and z_t are those of hm_pileup_fetch_domains under
 *      (A_i, B_i, S, max_gap); every chain starts from delta = (0, 0) and decides its own end state.
 *   3. REFIT (hm_domain_refit).  R0 == 0 or R1 == 0: status `one_state`, result (l_i, h_i).  Otherwise
 *      l' = clamp((double)P0 / (double)(P0 + N0)), h' = clamp((double)P1 / (double)(P1 + N1)): one correctly rounded division
 *      each, then the clamp to [1e-6, 1 - 1e-6].  If !(l' < h') or hm_domain_scores(l', h', penalty) fails: status `degenerate`,
 *      result (l_i, h_i).
 *   4. STOP RULE, with (A', B') the scores of (l', h').  (A', B') == (A_i, B_i): status `converged`, result (l_i, h_i) -- the
 *      segmentation that produced the levels is the one that is written.  (A', B') == (A_j, B_j) for a j < i: status `cycle`; the
 *      members of the cycle are the iterations j .. i, j taken with the levels (l', h') that closed it (they have its scores), and
 *      the result is the member with the smallest (A, B) in lexicographic order: it depends on the cycle alone, not on where it
 *      was entered.  i + 1 == max_iter: status `max_iter`, result (l', h').  Otherwise (l_{i+1}, h_{i+1}) = (l', h').
 * The result goes through hm_domain_scores once more and the segments are written with it.  The sums are an integer function of
 * the planes and (A_i, B_i, S, max_gap), and the levels a function of the sums: the fit depends neither on launch geometry nor
 * on how the planes are cut into pieces.
 *
 * sums[6] = P0, N0, R0, P1, N1, R1 of context ctx in planes[lo, hi); returns R = R0 + R1, or < 0.  Arguments and errors as
 * hm_pileup_fetch_domains; HM_EINVAL for sums NULL.  No segment is built and only the sums come back from the device. */
int64_t hm_pileup_domain_sums(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                              int64_t hi, int32_t ctx, int64_t A, int64_t B, int64_t S, int64_t max_gap, int64_t sums[6]);
/* The same for a PIECE: `part` filled as for HM_DOMAIN_PASS_SEGMENTS (has_prev, prev_gpos, prev_d, has_next, next_gpos,
 * last_state) and only read.  The sums of the pieces of a chain add up to the chain's.  Errors as hm_pileup_fetch_domains_part. */
int64_t hm_pileup_domain_sums_part(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base,
                                   int64_t lo, int64_t hi, int32_t ctx, int64_t A, int64_t B, int64_t S, int64_t max_gap,
                                   const hm_domain_part_t* part, int64_t sums[6]);
/* Host only.  Step 3 above: HM_OK and the new levels; HM_EDATA, the levels untouched, where the step ends the fit (`one_state`
 * if R0 == 0 or R1 == 0, else `degenerate`); HM_EINVAL for a NULL, a negative sum or a penalty that is not >= 0. */
int hm_domain_refit(const int64_t sums[6], double penalty, double* level_lo, double* level_hi);

/* ---- read-level CpG patterns (`pileup -E`): which molecules carry which combination of calls -----------------
 * Everything above is a function of the per-locus counters; this is the one output that keeps the calls of a read together.
 * REFERENCE CpGs: per reference sequence the loci g with ref[g] == 'C' && ref[g + 1] == 'G', both bases inside the sequence (the
 * byte comparison of the projection: lower case never matches), c_0 < c_1 < ...; a locus's RANK is its place in the job-wide
 * ascending list.  A record is a MEMBER at reference CpG g exactly when it contributes a CpG (motif 0) record at g to the counters:
 * it passes -q / -f, g and g + 1 lie in one match run, the read's bases as stored are C, G, and the read carries a 5mC call there
 * (the strand rule of the projection); its probability is that call's ML byte.
 * WINDOW j, for k in {2, 3, 4}: the loci c_j .. c_{j+k-1} of one sequence; valid when c_{j+k-1} - c_j <= max_span.  A record
 * CONTRIBUTES to window j iff it is a member at all k loci -- a deletion, mismatch, missing call or run break at any of them and it
 * contributes nothing to that window; an insertion between two loci does not matter.  Its PATTERN has bit i (bit 0 = the leftmost
 * locus) set iff prob_i >= thr[CpG], the >= of hm_pileup_count.  counts[pattern] = the number of contributing records; a window is
 * a ROW when it is valid and n = the sum of its counts >= min_reads.  All integers: nothing depends on launch geometry.
 * Options "patterns" (k: 0 off = default, 2, 3 or 4) and "pattern_span" (max_span, 1 .. 65 536, default 150), both before
 * hm_pileup_set_reference (else HM_ESTATE; HM_EINVAL out of range).  With patterns on, hm_pileup_set_reference lists the reference
 * CpGs (8 B each) and allocates 16 uint32 bins per CpG (64 B), hm_pileup_run also appends one 8-byte window record per member head
 * whose window the read spans, and hm_pileup_count adds them into the bins with thr[0] and drops them.  Not here: CHG / CHH
 * windows, the haplotype partitions, windows with tolerated gaps, any statistical test. */
typedef struct {            /* one window = one row of <prefix>.patterns.CpG.bed; 88 bytes */
    int64_t start, end;     /* c_j, c_{j+k-1} + 2 */
    uint32_t counts[16];    /* by pattern; bins >= 2^k are 0 */
    uint32_t n, k;
} hm_pattern_t;
/* window records resident since the last hm_pileup_count */
int64_t hm_pileup_num_pattern_records(hm_pileup_t* p);
/* The rows whose first locus lies in [lo, hi), ascending.  Returns their number (may exceed cap, or out NULL: then nothing is
 * written).  hi == lo returns 0.  HM_ESTATE without option "patterns" or before hm_pileup_count, HM_EINVAL for lo < 0, lo > hi or
 * min_reads < 1. */
int64_t hm_pileup_fetch_patterns(hm_pileup_t* p, int64_t lo, int64_t hi, int64_t min_reads, hm_pattern_t* out, int64_t cap);
/* Host only: the one implementation behind every front end.  With f_b = counts[b] / n over the non-empty bins b in ascending
 * order, in fp64:  out[0] entropy = (0 - sum f_b log2 f_b) / k, in [0, 1];  out[1] epipolymorphism = 1 - sum f_b^2;
 * out[2] pdr = 1 - (double)(counts[0] + counts[2^k - 1]) / n, the proportion of discordant reads;
 * out[3] level = 100 * sum popcount(b) counts[b] / (k n).  HM_EINVAL for k outside 2..4, n == 0 or n != the sum of the 2^k bins. */
int hm_pattern_stats(const hm_pattern_t* w, double out[4]);

/* ---- bedMethyl rows with per-CpG depth classes (`pileup -M`): how many molecules covered a CpG, called or not --
 * Every output above is built from the reads that carry a usable call at a locus; this one also says how many covered it without
 * giving one.  REFERENCE CpGs and RANKS are those of the patterns above (ref[g] == 'C' && ref[g + 1] == 'G', both bases in one
 * sequence, upper-case bytes only); the list is built when either option is on.
 * A record TAKES PART when hm_pileup_submit_read / _hp / _calls returned 1 for it and it passes -q and -f (the identity test of the
 * projection); secondary and supplementary records do, as in the counters; a record without entries, or an unmapped one, does not.
 * A MATCH RUN is a maximal stretch of M / = / X columns with no I, D or N of non-zero length inside; P, S and H neither make
 * columns nor close a run.  For a record that takes part and a reference CpG g (the C at g, the G at g + 1) at most one CLASS applies:
 *   1. Column g lies in one of the record's match runs.
 *      MOD / CANON  the record is a member at g in the patterns' sense: g and g + 1 in one run, the bases as stored C, G, and a 5mC
 *                   entry at the offset the projection looks up.  MOD when that entry's ML byte is >= thr[CpG] (the >= of
 *                   hm_pileup_count), else CANON.
 *      NOCALL       g and g + 1 in one run, the stored bases C, G, and no 5mC entry at that offset.
 *      nothing      g is the last column of the record's last match run: the alignment ends on the C, the dinucleotide is not covered.
 *      DIFF         every other case: the stored base at g is not C, the stored base at g + 1 is not G, or the run ends at g with
 *                   more of the alignment behind it (an insertion between C and G, g + 1 deleted or skipped by N).
 *   2. DELETE       g lies inside a D operation: a D of length n whose first deleted reference base is s covers s .. s + n - 1.
 *   3. nothing      g lies inside an N operation, outside the alignment, or only g + 1 is covered.
 * COUNTERS: five uint32 per reference CpG -- n_mod, n_canon, n_nocall, n_diff, n_delete.  With option "partitions" = 2 there are
 * three sets: set 0 counts every record that takes part, sets 1 and 2 those submitted with hp 1 or 2.  All of it is an integer
 * function of the records and thr[0]: nothing depends on launch geometry or on how the records are cut into batches.
 * A reference CpG is a ROW of a set when its five counters sum to at least 1 and n_mod + n_canon >= min_valid, min_valid >= 0: with
 * min_valid 0 the CpGs seen only as nocall, diff or delete are listed too.
 * Option "bedmethyl" (0 off = default, 1), before hm_pileup_set_reference (else HM_ESTATE; HM_EINVAL for another value).  With it
 * on, hm_pileup_set_reference lists the reference CpGs (8 B each, shared with the patterns; fewer than 2^32) and allocates the
 * counters (20 B per CpG and set), hm_pileup_run adds NOCALL, DIFF and DELETE behind the projection, and hm_pileup_count adds MOD
 * and CANON from the resident records before it drops them; the counters accumulate over run / count cycles as the planes do.
 * Without it nothing is allocated, uploaded or launched.  Not here: CHG / CHH rows; per-strand rows (a read gives one call per CpG
 * dyad, on its own C, so there is no second strand to report); a no-call band around the threshold (bedMethyl's Nfail is always
 * 0); codes other than m (Nother_mod is always 0: they never reach the counters); pileup_dist. */
typedef struct {            /* one reference CpG = one row of <prefix>.bedmethyl.CpG.bed; 32 bytes */
    int64_t gpos;
    uint32_t n_mod, n_canon, n_nocall, n_diff, n_delete, reserved;
} hm_bedmethyl_t;
/* The rows of set `part` (0 combined, 1 / 2 the haplotype partitions) whose gpos lies in [lo, hi), ascending.  Returns their number
 * (may exceed cap, or out NULL: then nothing is written).  hi == lo returns 0.  HM_ESTATE without option "bedmethyl", before the
 * first hm_pileup_count, or for part 1 / 2 without partitions; HM_EINVAL for part outside 0..2, lo < 0, lo > hi or min_valid < 0. */
int64_t hm_pileup_fetch_bedmethyl(hm_pileup_t* p, int32_t part, int64_t lo, int64_t hi, int64_t min_valid, hm_bedmethyl_t* out,
                                  int64_t cap);

/* ---- within-read CpG co-methylation by distance (`pileup -L`): how the calls of one molecule are coupled --------
 * The co-methylation decay curve: per distance d, how often two CpGs d bases apart on the SAME molecule are both methylated, both
 * unmethylated, or discordant.  A record TAKES PART as under the patterns and bedMethyl above: its submission returned 1 and it
 * passes -q / -f; secondary and supplementary records take part as records of their own.  Its MEMBER LOCI are the reference CpGs at
 * which it is a member in the patterns' sense (g and g + 1 in one match run, the bases as stored C, G, reference C, G, a 5mC entry at
 * the offset the projection looks up: the loci where it leaves a motif-0 record), each with that entry's ML byte `prob`.
 * The counted objects are the unordered pairs of member loci (a, b) of ONE record with a < b and d = b - a in [2, max_dist]; each
 * counts once.  Pairs never join two records, two alignments of one read name included.  With pa, pb the ML bytes at the lower and
 * the higher coordinate and t = thr[CpG] of the last hm_pileup_count, a locus is M iff prob >= t (hm_pileup_count's >=), and the pair
 * falls into one of UU, UM, MU, MM, the first letter for the lower coordinate.
 * The thresholds are known only after the last read and the pairs are too many to keep, so per d three 256-bin uint64 histograms are
 * filled at hm_pileup_run time: H_min[d][min(pa, pb)], H_max[d][max(pa, pb)], H_first[d][pa].  For any t: n = sum H_min[d],
 * MM = sum_{v >= t} H_min[d][v], UU = sum_{v < t} H_max[d][v], MU = sum_{v >= t} H_first[d][v] - MM, UM = n - MM - UU - MU.  Exact
 * integers; (max_dist + 1) * 6 144 bytes whatever the depth; the histograms accumulate over run / count cycles as the planes do, and
 * a fetch applies the LAST count's threshold to all of them.
 * Option "linkage" (max_dist: 0 off = default, else 2 .. 16 384), before hm_pileup_set_reference (else HM_ESTATE; HM_EINVAL out of
 * range).  With it on, hm_pileup_set_reference allocates and zeroes the table, and hm_pileup_run lists the batch's members (16 B
 * each, for the batch's lifetime) and adds their pairs behind the projection.  Without it nothing is allocated, uploaded or
 * launched.  Not here: CHG / CHH pairs, per-haplotype tables, distance bins (rows are exact distances), read-coordinate distances,
 * any statistical test. */
typedef struct {            /* one distance = one row of <prefix>.linkage.CpG.tsv; 40 bytes */
    uint32_t dist, reserved;
    uint64_t n_uu, n_um, n_mu, n_mm;
} hm_linkage_t;
/* The rows of the distances d in [2, max_dist] with n = n_uu + n_um + n_mu + n_mm >= min_pairs, ascending; min_pairs 0 returns every
 * d, the empty ones included.  Returns their number (may exceed cap, or out NULL: then nothing is written).  HM_ESTATE without
 * option "linkage" or before the first hm_pileup_count, HM_EINVAL for min_pairs < 0. */
int64_t hm_pileup_fetch_linkage(hm_pileup_t* p, int64_t min_pairs, hm_linkage_t* out, int64_t cap);
/* Host only, fp64: the one implementation behind every front end.  out[0] concordance = (n_uu + n_mm) / n;  out[1] the phi
 * coefficient r = (n_mm n_uu - n_mu n_um) / sqrt((n_mm + n_mu)(n_um + n_uu)(n_mm + n_um)(n_mu + n_uu)), the numerator an exact
 * integer, NaN when a margin is 0.  HM_EINVAL for n == 0. */
int hm_linkage_stats(const hm_linkage_t* w, double out[2]);

/* ---- methylation by position in the read, end trimming (`pileup -P`, `pileup -I`) ---------------------------
 * The M-bias table of bisulfite pipelines, for this caller: every call is centred in a 401-base kinetics window that is zero-padded
 * within 200 bases of either read end, and this table shows whether the calls made there behave like the others.
 * PROJECTED RECORD: each record the projection emits (what hm_pileup_num_records counts) has a read position p, the index into the
 * read's per-base plane at which the projection found the 5mC entry -- the offset in the read's original orientation, as MM counts
 * it: for a reverse record's CpG the called C of the original strand, for a CHH call on the read's reverse strand the G.
 * BIN: with L = l_qseq as submitted, d5 = p, d3 = L - 1 - p and the option value D: min(d5, d3) >= D is the INTERIOR bin; else
 * d5 <= d3 is bin (5', d5) -- ties go to 5' --; else bin (3', d3).
 * The records that count are exactly those hm_pileup_count will count (a record takes part as everywhere: its submission returned
 * 1 and it passes -q / -f); secondary and supplementary records count as records of their own, as under the linkage above.
 * THE TABLE: the thresholds are known only after the last read, so, like the linkage table, this one is threshold-free:
 * H[motif][bin][ML byte] in uint64, 3 x (2 D + 1) x 256 counters in HBM (12.6 MB at D = 1024, 25.2 MB at D = 2048), filled at
 * hm_pileup_run time.  It accumulates over run / count cycles as the planes do; a fetch applies the LAST hm_pileup_count's thresholds
 * with its >=.  One histogram row gives n_m = sum_{v >= thr[motif]} H[v], n_u = sum_{v < thr[motif]} H[v] and sum_ml = sum v H[v],
 * the sum of the ML bytes, which does not depend on the threshold.  Exact integers.
 * TRIMMING: with "trim5" = n5 and "trim3" = n3 an entry (MM / ML entry or call) of a read at p < n5 or p > L - 1 - n3 is dropped
 * where it would enter the per-base plane and the threshold histograms: it writes no plane word and adds no histogram count, so every
 * output sees "no call" there -- the cov.bed counts, the haplotype, allele-specific, domain, pattern, linkage and fused paths, and
 * the bedMethyl rows, where the call becomes an Nnocall.  n5 + n3 >= L drops every entry of the read.  0:0, the default, changes
 * nothing.
 * Options, before hm_pileup_set_reference (else HM_ESTATE; HM_EINVAL out of range): "profile" (D: 0 off = default, else
 * 1 .. 2048), "trim5" and "trim3" (integers >= 0, default 0).  With "profile" on, hm_pileup_set_reference allocates and zeroes the
 * table and hm_pileup_run's projection adds to it; without it nothing is allocated, uploaded or launched.  Not here: per-haplotype
 * tables, bins wider than a base, np / rq strata, any statistical test, an automatic choice of trim values. */
typedef struct {            /* one (motif, bin) = one row of <prefix>.readpos.tsv; 40 bytes */
    uint32_t motif, end, dist, reserved;    /* end: 0 = 5', 1 = 3', 2 = interior (dist 0) */
    uint64_t n_m, n_u, sum_ml;
} hm_readpos_t;
#define HM_READPOS_5P 0
#define HM_READPOS_3P 1
#define HM_READPOS_INTERIOR 2
/* The rows with n_m + n_u >= min_calls: by motif, then 5' by ascending dist, 3' by ascending dist, interior; min_calls 0 returns all
 * 3 x (2 D + 1) rows.  Returns their number (may exceed cap, or out NULL: then nothing is written).  HM_ESTATE without option
 * "profile" or before the first hm_pileup_count, HM_EINVAL for min_calls < 0. */
int64_t hm_pileup_fetch_readpos(hm_pileup_t* p, int64_t min_calls, hm_readpos_t* out, int64_t cap);
/* The table itself, hist[(motif * (2 D + 1) + bin) * 256 + ML byte] with bin = d5, D + d3 or 2 D (interior): its
 * 3 x (2 D + 1) x 256 counters into hist[cap] -> their number (may exceed cap, or hist NULL: then nothing is written).
 * hm_pileup_add_readpos adds n such counters from elsewhere (another engine's table: the multi-rank path), n exactly that number
 * else HM_EINVAL.  Both HM_ESTATE without option "profile". */
int64_t hm_pileup_readpos_histograms(hm_pileup_t* p, uint64_t* hist, int64_t cap);
int hm_pileup_add_readpos(hm_pileup_t* p, const uint64_t* hist, int64_t n);
/* Host only, fp64: the one implementation behind every front end.  out[0] percent methylated = 100 n_m / (n_m + n_u), out[1] the
 * mean ML byte = sum_ml / (n_m + n_u).  HM_EINVAL for n_m + n_u == 0. */
int hm_readpos_stats(const hm_readpos_t* w, double out[2]);

/* ---- methylation of given intervals, metaplots (`pileup -R`, `pileup -J`) --------------------------------------
 * Sums of the planes over intervals the caller names: promoters, CpG islands, windows of a tiling, genes with their flanks.
 * A LOCUS g with cov = pcov + ncov (64 bits) COUNTS when cov >= min_cov (>= 1).  A counted locus of context c = key & 3 adds to its
 * context: n_loci += 1, pcov += pcov, ncov += ncov, ppm += (2 000 000 pcov + cov) / (2 cov) in integer division: the locus' fraction
 * in parts per million, rounded half up.  An interval's sum is that of the loci in [start, end).  All of it exact integers, so the
 * sums over disjoint plane chunks add up to the whole's and no order of summation matters.
 * HOW: a call builds a two-level index of its range [lo, hi): the twelve sums of every block of HM_REGION_BLOCK loci (block b =
 * loci lo + b HM_REGION_BLOCK ...), then their inclusive scan over the blocks, a scan of as many workgroups as there are
 * HM_REGION_SCAN_BLOCKS blocks (12 x 8 B per block in HBM, allocated by the first call, freed with the engine).  An interval's sum is
 * the scan's difference over the blocks inside it plus the loci of its two partial blocks, summed by one wavefront: its cost does
 * not depend on its length, and overlapping, nested or unsorted intervals cost what disjoint ones do.
 * Without a call nothing is allocated or launched.  Not here: tests between intervals or haplotypes, bigWig output, a tiling made
 * by the tool. */
#ifndef HM_REGION_BLOCK
#define HM_REGION_BLOCK 4096      /* a power of two >= 256: chosen by measurement, DESIGN.md section 10 */
#endif
#define HM_REGION_SCAN_BLOCKS 1024 /* blocks per workgroup of the scan: a range of more loci than the product takes several */
typedef struct {            /* one (interval, context); 32 bytes */
    int64_t n_loci, pcov, ncov, ppm;
} hm_region_sum_t;
/* the two constants the library was built with: out[0] = HM_REGION_BLOCK, out[1] = HM_REGION_SCAN_BLOCKS */
int hm_region_geometry(int64_t out[2]);
/* out[i * 3 + c] = the sum of interval i = [start[i], end[i]) in context c.  start / end are GLOBAL locus coordinates (sequence
 * offset + position, as gpos of the row outputs); planes NULL = the engine's own, else DEVICE pointers whose element 0 is locus
 * `plane_base`, of which [lo, hi) is looked at, as in hm_pileup_fetch_loci.  Every interval is clamped to [plane_base + lo,
 * plane_base + hi): the results of disjoint chunks add up to the whole's.  n == 0 is allowed.  HM_ESTATE without planes (as
 * hm_pileup_fetch_loci), HM_EINVAL for a bad range, min_cov < 1 or start[i] > end[i]. */
int hm_pileup_fetch_regions(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                            int64_t hi, int64_t min_cov, const int64_t* start, const int64_t* end, int64_t n, hm_region_sum_t* out);
/* THE METAPLOT: every interval cut into the same number of bins, the bins of all intervals summed.  For an interval [s, e) on a
 * sequence [S0, S1) (global coordinates): body edges s + floor(j (e - s) / bins), j = 0 .. bins; with w = flank / flank_bins,
 * upstream edges s - flank + j w and downstream edges e + j w, j = 0 .. flank_bins; every edge clamped to [S0, S1], so a flank never
 * reads the neighbouring sequence of the concatenated planes.  Bins are numbered upstream, body, downstream for strand '+' (or
 * anything but '-'; strand NULL: all '+') and mirrored for '-'.  Intervals with e - s < bins are left out; *n_used counts the rest.
 * out[c * n_bins + b], n_bins = bins + 2 flank_bins: the sums of bin b in context c over the used intervals, each bin clamped to
 * [plane_base + lo, plane_base + hi) like an interval above; n_regions = the used intervals whose bin b has a non-zero width after
 * the SEQUENCE clamp: it depends on neither planes nor chunk, so disjoint chunks add up in every field but n_regions, which they
 * share.  HM_EINVAL: bins outside [1, 1000], flank < 0, flank_bins outside [0, 1000], flank_bins == 0 with flank != 0 or the
 * reverse, flank % flank_bins != 0, s > e, S0 > S1, or an interval outside its sequence; the rest as hm_pileup_fetch_regions. */
typedef struct {            /* one (context, bin) = one row of <prefix>.metaplot.<ctx>.tsv; 48 bytes */
    int32_t motif, bin;
    int64_t n_regions, n_loci, pcov, ncov, ppm;
} hm_metabin_t;
int hm_pileup_fetch_metaplot(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                             int64_t hi, int64_t min_cov, const int64_t* start, const int64_t* end, const int64_t* seq_start,
                             const int64_t* seq_end, const char* strand, int64_t n, int32_t bins, int64_t flank, int32_t flank_bins,
                             hm_metabin_t* out, int64_t* n_used);
/* Host only, fp64: the one implementation behind every front end.  out[0] weighted = 100 pcov / (pcov + ncov), out[1] mean =
 * ppm / n_loci / 10^4, the mean of the loci's own percentages.  HM_EINVAL for n_loci == 0 (or a negative member). */
int hm_region_stats(const hm_region_sum_t* w, double out[2]);

/* ---- methylation by the k-mer around each cytosine (`pileup -S`) ------------------------------------------------
 * The three contexts split further by the sequence the cytosine sits in: CCG against CAG / CTG, CAA / CTA against the other CHH, or a
 * caller's error rate that follows a flanking base.  flank = f in {0, 1, 2, 3}, k = 3 + 2 f (3, 5, 7, 9), K = 4^k.
 * A LOCUS g (global coordinate into the concatenated reference) COUNTS exactly as under hm_pileup_fetch_regions: cov = pcov + ncov
 * (64 bits) >= min_cov (>= 1); its context c = key & 3; it adds n_loci += 1, pcov, ncov and ppm += (2 000 000 pcov + cov) / (2 cov).
 * THE ROW it adds to is decided by the reference alone (forward cytosines are recorded at their C, reverse-strand CHH at the G of
 * DDG).  With [S0, S1) the locus' own sequence:
 *   ref[g] == 'C': the window is ref[g - f, g + 3 + f), read left to right;
 *   ref[g] == 'G': the window is ref[g - 2 - f, g + 1 + f), reverse-complemented; the called cytosine is again at offset f;
 *   row `other` (index K): ref[g] is neither C nor G, or the window is not wholly inside [S0, S1) (a window never reads the
 *   neighbouring sequence of the concatenation), or it holds a base outside ACGT.
 * Code: A = 0, C = 1, G = 2, T = 3, first base most significant.  The table is out[c * (K + 1) + code], c = 0 .. 2, code = 0 .. K:
 * 3 (K + 1) entries.  Per context the n_loci of all rows, `other` included, add up to the loci of [lo, hi) with cov >= min_cov in
 * that context.  No row is restricted to the k-mers its context can have: planes handed in may carry any key at any base, and a CpG
 * locus and a reverse-read CGG locus can share g.  All of it exact integers: the tables of disjoint chunks add up to the whole's.
 * HOW: one grid-stride kernel over [lo, hi) with one workgroup of HM_CONTEXT_SPAN threads per CU.  It streams pcov / ncov; only a
 * locus with a count reads key, finds its sequence's end and reads its k reference bytes.  Up to flank HM_CONTEXT_LDS_FLANK the
 * workgroup adds into a table of its own in LDS (6 KB at flank 0, 98 KB at flank 1) and ends with one global atomic per non-zero
 * counter; above it every add is a 64-bit global atomic into the device table (25 MB at flank 3).  The device table is allocated
 * by the first call and freed with the engine; without a call nothing is allocated or launched.
 * Not here: strand-split counts (CpG strands are merged at projection), tests between contexts, IUPAC motif queries, sequence
 * logos, k above 9. */
#define HM_CONTEXT_SPAN 1024        /* loci a workgroup takes side by side */
#define HM_CONTEXT_LDS_MAX_FLANK 1  /* the largest flank whose table fits in LDS at all */
#ifndef HM_CONTEXT_LDS_FLANK
#define HM_CONTEXT_LDS_FLANK 1      /* the largest flank that takes the LDS path: chosen by measurement, DESIGN.md section 10 */
#endif
#define HM_CONTEXT_PATH_AUTO (-1)
#define HM_CONTEXT_PATH_LDS 0
#define HM_CONTEXT_PATH_GLOBAL 1
/* the constants the library was built with: out[0] = HM_CONTEXT_SPAN, out[1] = HM_CONTEXT_LDS_FLANK, out[2] =
 * HM_CONTEXT_LDS_MAX_FLANK (host only) */
int hm_context_geometry(int64_t out[3]);
/* Returns 3 (K + 1); when that exceeds cap, or out is NULL, nothing is written.  Planes NULL = the engine's own, else DEVICE
 * pointers whose element 0 is locus `plane_base`, of which [lo, hi) is looked at, as in hm_pileup_fetch_regions; the reference
 * position of element i is plane_base + i in the engine's reference.  Per haplotype: the same call with a partition's pcov / ncov
 * and the combined key.  HM_ESTATE before hm_pileup_set_reference and without planes (as hm_pileup_fetch_loci); HM_EINVAL for
 * flank outside [0, 3], min_cov < 1, a bad range, a mix of NULL and non-NULL planes, or plane_base + hi beyond the reference. */
int64_t hm_pileup_fetch_context(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                                int64_t hi, int64_t min_cov, int32_t flank, hm_region_sum_t* out, int64_t cap);
/* The same with the accumulation path named: HM_CONTEXT_PATH_AUTO (what hm_pileup_fetch_context takes), _LDS (HM_EINVAL for a flank
 * above HM_CONTEXT_LDS_MAX_FLANK) or _GLOBAL.  Both paths give the same table; this is what measures them against each other
 * (tools/pileup_bench.py --context) and lets a test reach the one the default does not take. */
int64_t hm_pileup_fetch_context_path(hm_pileup_t* p, const void* pcov, const void* ncov, const void* key, int64_t plane_base, int64_t lo,
                                     int64_t hi, int64_t min_cov, int32_t flank, int32_t path, hm_region_sum_t* out, int64_t cap);

/* ---- kernel-smoothed levels per locus (`smooth`) ------------------------------------------------------------------
 * A locus at 5-10x coverage says little on its own; its neighbours of the same context say more.  Everything here is integer-exact:
 * a reference with arbitrary-precision integers reproduces every row bit for bit, whatever the range of the fetch.
 * A LOCUS COUNTS when key & 3 == ctx and pcov + ncov >= min_cov (>= 1).  For a counting locus at global position g of the sequence
 * [S0, S1) and a half-width h in [1, HM_SMOOTH_MAX_HALF_WIDTH], the WINDOW is the counting loci j of the same context with
 * max(S0, g - h + 1) <= j <= min(S1 - 1, g + h - 1); locus j has the weight w_j = h - |j - g|, the triangular kernel in integers 1 .. h
 * (a locus exactly h away has weight 0 and is outside).  The row of g: loci = the number of loci of the window, g included;
 * wp = sum w_j pcov_j; wn = sum w_j ncov_j.  wp / (wp + wn) is the local-constant binomial likelihood fit under that kernel.  Nothing
 * crosses a sequence boundary; loci of other contexts and loci below min_cov between the counting ones are ignored; with h = 1 the
 * row is the locus itself (loci 1, wp = pcov, wn = ncov).  With counts below 2^31 (the bound of hm_pileup_load_loci) wp and wn stay
 * below 2^60.
 * HOW: the triangular kernel is a box convolved with a box, so a row is a few differences of running sums over the counting loci:
 * their number, sum pcov, sum ncov and the two first moments sum (j - origin) pcov, sum (j - origin) ncov.  The call writes these five
 * per POSITION of the span it reads, 40 B each, into a buffer the first call allocates (it grows with the largest span, freed with
 * the engine).  The sums restart every HM_SMOOTH_SPAN positions of the span and a block's moments are measured from the block's
 * start, so every intermediate stays below 2^62 for any legal input and any range; a half window lies in at most two blocks, and
 * the cost of a row does not depend on h.  The rows then go through the selection skeleton of every row fetch.
 * A fetch over [lo, hi) READS the planes over [lo - h + 1, hi + h - 1) clamped to the reference: its rows are the slice of the
 * whole-reference fetch, whatever the chunk.  Not here: smoothing while `pileup` runs, pileup_dist, smoothed levels as the input of
 * groupdiff or samplecorr, other kernels than the triangle. */
#define HM_SMOOTH_MAX_HALF_WIDTH 16384
#define HM_SMOOTH_SPAN 32768 /* positions after which the running sums restart: 2 * HM_SMOOTH_MAX_HALF_WIDTH */
typedef struct {            /* one counting locus = one row of <prefix>.smooth.<ctx>.bed; 40 bytes */
    int64_t gpos;
    int32_t pcov, ncov;     /* the locus' own counts */
    int64_t loci, wp, wn;   /* the window: its loci, and the weighted sums of their pcov and ncov */
} hm_smooth_t;
/* The counting loci of context ctx (0 CpG, 1 CHG, 2 CHH) in [lo, hi) whose window holds at least min_loci loci, ascending in gpos.
 * part 0: the engine's combined planes; 1 or 2: that partition's pcov / ncov with the combined key plane.  Works after
 * hm_pileup_count and after a successful hm_pileup_load_loci.  Returns the number of rows; when that exceeds cap, or out is NULL,
 * nothing is written (as hm_pileup_fetch_loci).  It changes nothing another fetch reads.  HM_EINVAL for ctx outside [0, 2], part
 * outside [0, 2], half_width outside [1, HM_SMOOTH_MAX_HALF_WIDTH], min_cov < 1, min_loci < 1, lo < 0, hi < lo or hi beyond the
 * reference; HM_ESTATE where hm_pileup_fetch_loci over the engine's own planes gives it (no planes; after a load that met a bad
 * row), before hm_pileup_set_reference, and for part 1 / 2 without partition planes. */
int64_t hm_smooth_fetch(hm_pileup_t* p, int32_t part, int32_t ctx, int64_t lo, int64_t hi, int32_t half_width, int32_t min_cov,
                        int64_t min_loci, hm_smooth_t* out, int64_t cap);
/* Host only, fp64: the one implementation behind every front end.  out[0] = the smoothed level in percent, 100 wp / (wp + wn), each
 * integer converted to double first; out[1] = (wp + wn) / half_width, the effective number of calls at full weight.  HM_EINVAL for
 * half_width < 1, a negative sum or wp + wn == 0. */
int hm_smooth_stats(const hm_smooth_t* r, int32_t half_width, double out[2]);

#ifdef __cplusplus
}
#endif
#endif
