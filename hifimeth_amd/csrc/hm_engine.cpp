// hm_engine.cpp -- host side of libhifimeth_hip.so: model loading, read staging, the asynchronous batch pipeline
// and the C ABI of include/hifimeth_hip.h.  Mirrors what ModModels, ModBatch and the worker loop do around the hot
// path in the reference (src/app/hifimeth/mod_main.cpp:18-262); the pinned double-buffered staging follows the shape
// of the reference's GPU variant (src/app-gpu/hifimeth-gpu/5mc_call_gpu.cpp:309-334,367) without its per-site windows.
//
// One engine = one device, one compute stream, N batch slots.  A slot owns pinned staging memory, the device buffers of
// one batch and an I/O stream: queueing a batch enqueues   H2D (slot stream) -> scanner + CNN + pack (compute stream)
// -> D2H of the totals (slot stream)   and returns -- no host/device synchronisation anywhere on the way.  The site
// counts never come back to the host to size the CNN launches: the persistent CNN kernels read them from the scan
// kernel's totals on the device (SiteRange), the host only bounds the launch windows by the number of staged bases.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hifimeth_hip.h"
#include "hm_device.h"
#include "hm_host.h"
#include "hm_kernels.h"
#include "hm_weights.h"

using namespace hm;

namespace {

thread_local std::string g_create_error;

enum Kind { K_PREP, K_SCAN, K_EMIT, K_PACK, K_WINDOW, K_FRONT, K_TAIL, K_TRUNK, K_EDGE, K_TAILG };

struct TimedSpan {
    int kind, ctx;
    int64_t off, cap;  // CNN spans: launch window into the context's site list; K_WINDOW: cap = sites
    Event a, b;
};

struct DeviceModel {
    bool loaded = false;
    int k1 = 0;
    DevBuf params;  // all fragment-packed weights, biases, fc2, bn tables in one allocation
    CtxWeights w{};
};

}  // namespace

// One batch slot: staged reads (pinned), their device buffers, results.
struct hm_batch {
    hm_engine* e = nullptr;
    int id = 0;
    enum State { FREE, STAGING, QUEUED } state = FREE;
    bool uploaded = false, ran = false, have_totals = false, have_calls = false;
    Stream s_io;  // this slot's copies in and out.  Declared before every buffer: destroyed after them
    Event ev_in, ev_comp, ev_out;

    // staged batch (host, pinned)
    PinnedArr<uint8_t> slab;
    PinnedArr<ReadDesc> reads;
    PinnedArr<Chunk> chunks;
    PinnedArr<RInfo> rinfo;      // dense trunk: per read
    PinnedArr<TrunkTile> tiles;  // dense trunk: 112-position tiles of every read, in read order
    PinnedArr<int32_t> tcost;    // per group: running cost of its tiles (n_tiles + 1 entries from 0): what the sliding-window trunk cuts its runs by
    struct Group {               // consecutive reads whose maps share one set of buffers
        int chunk_lo, chunk_hi, tile_lo, tile_hi;
        int64_t bases, rows;
        int cost_lo;             // where the group's running costs start in tcost
    };
    std::vector<Group> groups;
    int64_t total_bases = 0;  // padded to a multiple of 4 per read

    // device
    DevBuf d_raw, d_reads, d_chunks, d_rinfo, d_tiles, d_tcost, d_bases, d_kin, d_sctx, d_counts, d_offs, d_totals, d_err;
    DevBuf d_usites, d_utag, d_csites, d_opos, d_logits, d_p, d_ml, d_calls;
    Pinned<int32_t> h_totals;  // [TOT_COUNT]: the scan kernel's 8 totals + what the trunk and the strip tail count (TotalsSlot)
    Pinned<int32_t> h_err;
    PinnedArr<hm_call_t> h_calls;
    int32_t totals[TOT_COUNT] = {};

    std::vector<TimedSpan> spans;

    ~hm_batch() {  // (the engine's destructor has made the device current)
        if (s_io) (void)hipStreamSynchronize(s_io);
    }
};

namespace {

// Scratch of one read group: what hm_get_timing reports as group_bytes and GROUP_BYTES_PER_BASE budgets for
struct GroupBufs {
    DevBuf d_map[3], d_e4, d_edge4, d_e4row, d_rowlist;  // dense trunk: maps of one read group, edge rows of its sites
    DevBuf d_x6;                // split tail: conv6's rows of one launch (hm_tail_s.hip)
    DevBuf d_mark, d_ccnt, d_order, d_okey;  // strip tail (hm_tail_p.hip): per-map-row marks, class counters, the class-sorted site order and its keys
    DevBuf d_odst;              // strip tail: list position -> the site's slot in the batch's result arrays (tail_fc_kernel's stores)
    DevBuf d_x8;                // the rows of a launch's sites on their way from the strip tail kernel to its second kernel (TAIL_STRIP_HANDOVER_BYTES per site)
    DevBuf d_dump;              // sliding-window trunk: where a warm-up step's conv4 rows go (hm_trunk3.hip)
    int64_t bytes() const {
        const DevBuf* all[] = {&d_map[0], &d_map[1], &d_map[2], &d_e4, &d_edge4, &d_e4row, &d_rowlist, &d_x6, &d_mark, &d_ccnt, &d_order, &d_okey, &d_odst, &d_x8, &d_dump};
        static_assert(sizeof(GroupBufs) == sizeof all / sizeof *all * sizeof(DevBuf), "a member of GroupBufs is missing from bytes()");
        int64_t sum = 0;
        for (const DevBuf* d : all) sum += (int64_t)d->cap;
        return sum;
    }
};

}  // namespace

struct hm_engine {
    int device = 0;
    int num_cu = 256;
    int ctx_mask = 7;
    int min_read_size = 1000;  // mod_options.cpp:10
    int64_t sub_batch = 65536;
    int front_waves = 8;
    // 0 = fp32 MFMA; 1 = split-half f16x3 MFMA with fp32 accumulate (default); 2 = as 1, with plain fp16 WEIGHTS (the w_lo x_hi product
    // and the lo plane's fetches dropped) in conv8 and fc1, |dp| <= 1e-3.  The wider fp16-weight modes of rounds 1 and 2
    // are closed: README "configs[4]", DESIGN.md.
    int precision = 1;
    int conv3_w16 = 0;   // diagnostic: conv3 of the dense trunk with plain fp16 weights (measured above the 1e-3 bar; not part of any mode)
    int max_slots = 3;  // batch slots of the asynchronous API (the legacy calls use one more, slot 0)
    // conv1..conv4: 1 = once per read position (dense trunk, hm_trunk.hip), 0 = once per site (front kernels), 2 = per
    // context whichever is cheaper at the site density of the run's first batch: the trunk costs ~0.9 ns per base and strand
    // view whatever the number of sites, the per-site kernels ~55 ns per site more than the trunk path's per-site share,
    // so the trunk wins above ~1.7 % sites per base (CHH, two views: 3.3 %) -- everything but CpG-only runs on
    // CpG-poor genomes.  Both paths give the same calls to within fp32 re-association.
    int trunk = 2;
    // 3: the streaming trunk as a sliding window (hm_trunk3.hip: 112 rows per layer and tile, 14 % fewer MFMAs), 1: streaming 4-wave trunk
    // kernel (hm_convs.h), 2: the same on 8 waves, 0: the 8-wave ConvH form; byte-identical maps
    int trunk_impl = 3;
    // dense-trunk path, precision 1: 2 = edge2_kernel computing the E1 rows its chains read itself (hm_edge2.hip, E1C): with trunk_impl 3 the
    // trunk then stores no E1 row and the E1 map is not allocated (trunk_stores_e1); 1 = edge2_kernel gathering them from the E1 map,
    // 0 = edge_kernel (hm_trunk.hip); bit-identical
    int edge_impl = 2;
    // dense-trunk path, precision 1: 2 = the split tail (hm_tail_s.hip: conv5 + conv6, then conv7 .. softmax batched over 16 sites),
    // 1 = one kernel with resident weights (hm_tail_r.hip), 0 = tail_kernel_h (streams them per pass); bit-identical
    // 3 (default) = the strip tail (hm_tail_p.hip) for CHH -- 16 sites of one residue class per pass sharing a strip of E4 rows in LDS --
    // and tail_kernel_r for the sparse contexts (their sites are too far apart to share rows)
    int tail_impl = 3;
    int64_t tail_slice = int64_t(1) << 21;  // sites per launch pair of the split tail (option, not the default): its hand-off buffer holds 3.7 KB per site (2 planes x 9 rows x 208 B:
                                            // 7.9 GB at this slice, allocated on first use and NOT part of GROUP_BYTES_PER_BASE's quarter-of-free-memory budget)
    // trunk = 2 is decided ONCE per engine, from the reads of the first non-empty batch that is queued (counted on the
    // host, estimate_density): the choice must not depend on which batches happen to have finished when the next one is
    // queued -- the two paths differ by fp32 re-association (~1e-5 in p), and the reference's output is deterministic.
    int trunk_mask_auto = -1;  // contexts that take the dense trunk under trunk = 2 (-1: not decided yet); guarded by mu
    // reads per trunk group: their maps take ~3.9 KB per base (16 Mi bases: 64 GB of the 288).  Larger groups = fewer launches of the
    // resident-weight kernels, which load their weights once per launch: streamed bench 56.5 M sites/s at 2 Mi, 57.7 M at 16 Mi, 56.4 M at 32 Mi
    // 0 (default) = sized from the device's FREE memory when the first read is staged: the group buffers (maps, edge rows, row lists)
    // take at most a quarter of it, and at most 16 Mi bases (effective_group_bases).  Two engines on one device, or ranks sharing a
    // GPU, then fit by construction; hm_get_timing reports what was chosen and what is allocated.
    int64_t group_bases = 0;
    std::atomic<int64_t> group_bases_eff{0};  // staging threads of several batches may ask at once: all compute the same figure
    bool stamps_on = false;
    std::vector<unsigned long long> stamp_sum;
    bool timing = false;
    std::string err;

    std::mutex mu;  // slot states, error string, event pool, timing
    std::mutex order_mu;  // the kernels of two batches must not interleave on the compute stream
    std::condition_variable cv;
    hm_timing_t acc{};
    int64_t x6_sites = 0;  // the site count grp.d_x6's plane stride was laid out for

    // What the engine holds on the device, in the order it is given back -- members are destroyed last to first: the slots,
    // the models, the scratch all batches share, the event pool, the compute stream.
    Stream stream;  // compute.  Declared before everything that runs on it: destroyed last
    std::vector<Event> pool;
    // scratch shared by all batches: only touched by kernels on the compute stream, which runs batches in order
    DevBuf d_act4, d_win, d_dbg, d_stamps, d_zeros;
    GroupBufs grp;
    DeviceModel model[3];
    std::vector<std::unique_ptr<hm_batch>> slots;  // [0] = the batch of the legacy (synchronous) calls

    ~hm_engine() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
    }
};

namespace {

// Device bytes per base of a read group: E1..E3 maps (2 views x 512 B each), E4 (2 x 384 B), the sites' edge rows (768 B) and map-row
// numbers, row lists -- times the 25 % head-room DevBuf::reserve adds.  The budget is that of the option set with the largest footprint:
// the default kernels (edge_impl 2 with trunk_impl 3) allocate no E1 map and stay 1 280 B per base under it, but options may be switched
// on a live engine after the group size has been fixed, and an engine must then still fit "a quarter of free memory".
constexpr int64_t GROUP_BYTES_PER_BASE = (3 * 2 * 512 + 2 * 384 + 768 + 4 + 8 + 2 * 4 + 8 + 4 + TAIL_STRIP_HANDOVER_BYTES) * 5 / 4;  // (+ the strip tail's marks per map row, its sorted order and
                                                                                                            //  the rows handed to its second kernel, sized per base: a base is at most one site)

int64_t effective_group_bases(hm_engine* e) {
    if (e->group_bases > 0) return e->group_bases;
    if (const int64_t have = e->group_bases_eff.load(std::memory_order_relaxed)) return have;
    size_t free_b = 0, total_b = 0;
    int64_t gb = int64_t(2) << 20;
    int prev = -1;
    (void)hipGetDevice(&prev);   // a getter (hm_get_timing) may come through here: the caller's current device is put back
    if (hipSetDevice(e->device) == hipSuccess && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
        gb = (int64_t)(free_b / 4) / GROUP_BYTES_PER_BASE;
        gb = std::min<int64_t>(gb, int64_t(16) << 20);
        gb = std::max<int64_t>(gb >> 20 << 20, int64_t(1) << 20);  // whole Mi, at least one
    }
    if (prev >= 0 && prev != e->device) (void)hipSetDevice(prev);
    // several staging threads may measure at once and see different amounts of free memory: the FIRST figure stored is the engine's
    int64_t none = 0;
    if (!e->group_bases_eff.compare_exchange_strong(none, gb, std::memory_order_relaxed)) gb = none;
    return gb;
}

// dense trunk bookkeeping of one staged read: its group (a new one when the current holds group_bases), map region, tiles, and the tiles'
// running cost -- a tile where no receptive field reaches the read (the first, u = -200, with the read's warm-up step; those at
// u >= len) is a constant step of trunk3_kernel, an eighth or so of a computed one: the kernel cuts its runs at equal cost
constexpr int TILE_COST = 8, TILE_COST_CONST = 1;
void add_read_tiles(hm_engine* e, hm_batch* b, int ridx, int l_qseq) {
    // a group is closed on its map ROWS -- what every group buffer scales with: ceil((len + 400) / 112) * 112 + 32 per read, 1.03 x the bases for
    // 15 kb reads but 3.5 x for 200-base ones (option -l) -- so that "at most a quarter of free memory" holds for any read length
    if (b->groups.empty() || b->groups.back().rows >= effective_group_bases(e)) {
        b->groups.push_back(hm_batch::Group{(int)b->chunks.n, (int)b->chunks.n, (int)b->tiles.n, (int)b->tiles.n, 0, 0, (int)b->tcost.n});
        b->tcost.push_back(0);
    }
    hm_batch::Group& g = b->groups.back();
    const int ntile = (l_qseq + 2 * TR_PAD + TR_OWN - 1) / TR_OWN;
    b->rinfo.push_back(RInfo{b->total_bases, l_qseq, (int32_t)g.rows});
    for (int t = 0; t < ntile; ++t) {
        const int u0 = -TR_PAD + t * TR_OWN;
        b->tiles.push_back(TrunkTile{ridx, u0});
        b->tcost.push_back(b->tcost.p[b->tcost.n - 1] + (t == 0 ? 2 * TILE_COST_CONST : u0 >= l_qseq ? TILE_COST_CONST : TILE_COST));
    }
    for (int st = 0; st < l_qseq; st += CHUNK) b->chunks.push_back(Chunk{ridx, st});
    g.rows += (int64_t)ntile * TR_OWN + TR_SLACK;
    // the edge kernel addresses a group's map rows (both views) in 27 bits: guaranteed by the 48 Mi cap on group_bases plus one read (< 2^25 rows)
    if (2 * g.rows >= (int64_t(1) << 27)) throw HipErr{hipErrorInvalidValue, "a read group's maps exceed 2^27 rows (group_bases too large)"};
    g.bases += l_qseq;
    g.chunk_hi = (int)b->chunks.n;
    g.tile_hi = (int)b->tiles.n;
}

int fail(hm_engine* e, int code, const std::string& msg) {
    if (e) {
        std::lock_guard<std::mutex> lk(e->mu);
        e->err = msg;
    } else {
        g_create_error = msg;
    }
    return code;
}

int fail_hip(hm_engine* e, const HipErr& h) {
    return fail(e, HM_EDEVICE, hip_error_text(h));
}

// every ABI entry point's device work: the engine's device current, a HipErr recorded as the engine's error -> HM_EDEVICE
template <class Body>
auto guarded(hm_engine* e, Body&& body) -> decltype(body()) {
    return hip_guard(e->device, [e](const HipErr& h) { return fail_hip(e, h); }, body);
}

Event get_event(hm_engine* e) {
    Event ev;
    {
        std::lock_guard<std::mutex> lk(e->mu);
        if (!e->pool.empty()) {
            ev = std::move(e->pool.back());
            e->pool.pop_back();
            return ev;
        }
    }
    HIP_TRY(hipEventCreate(&ev.h));
    return ev;
}

struct Span {
    hm_engine* e;
    std::vector<TimedSpan>* sink;
    TimedSpan ts{};
    bool on;
    Span(hm_engine* eng, std::vector<TimedSpan>* out, int kind, int ctx = 0, int64_t off = 0, int64_t cap = 0)
        : e(eng), sink(out), on(eng->timing && out) {
        if (!on) return;
        ts.kind = kind;
        ts.ctx = ctx;
        ts.off = off;
        ts.cap = cap;
        ts.a = get_event(e);
        ts.b = get_event(e);
        HIP_TRY(hipEventRecord(ts.a, e->stream));
    }
    void end() {
        if (!on) return;
        HIP_TRY(hipEventRecord(ts.b, e->stream));
        sink->push_back(std::move(ts));
        on = false;
    }
};

// spans of finished work -> accumulated timing; `totals` gives the site counts the CNN launch windows resolved to
void collect_timing(hm_engine* e, std::vector<TimedSpan>& spans, const int32_t* totals) {
    if (!spans.empty() && totals) {  // once per timed run of a batch
        std::lock_guard<std::mutex> lk(e->mu);
        for (int c = 0; c < 3; ++c) e->acc.trunk_list_steps[c] += totals[TOT_LIST_STEPS + c];
        for (int c = 0; c < 3; ++c) e->acc.trunk_const_steps[c] += totals[TOT_CONST_STEPS + c];
        e->acc.tail_strip_passes += totals[TOT_STRIP_PASSES];
    }
    for (auto& s : spans) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.a, s.b));
        std::lock_guard<std::mutex> lk(e->mu);
        hm_timing_t& t = e->acc;
        const int64_t n = totals ? std::clamp<int64_t>((int64_t)totals[s.ctx] - s.off, 0, s.cap) : s.cap;
        switch (s.kind) {
        case K_PREP: t.prep_ms += ms; ++t.prep_launches; break;
        case K_SCAN: t.scan_ms += ms; ++t.scan_launches; break;
        case K_EMIT: t.emit_ms += ms; ++t.emit_launches; break;
        case K_PACK: t.pack_ms += ms; ++t.pack_launches; break;
        case K_WINDOW: t.window_ms += ms; ++t.window_launches; t.window_sites += s.cap; break;
        case K_TRUNK: t.trunk_ms[s.ctx] += ms; ++t.trunk_launches[s.ctx]; t.trunk_positions[s.ctx] += s.cap; break;
        case K_EDGE: t.edge_ms[s.ctx] += ms; ++t.edge_launches[s.ctx]; break;
        case K_TAILG: t.tail_ms[s.ctx] += ms; ++t.tail_launches[s.ctx]; break;
        case K_FRONT:
            if (n > 0) { t.front_ms[s.ctx] += ms; ++t.front_launches[s.ctx]; t.front_sites[s.ctx] += n; }
            else { t.empty_ms += ms; ++t.empty_launches; }
            break;
        default:
            if (n > 0) { t.tail_ms[s.ctx] += ms; ++t.tail_launches[s.ctx]; }
            else { t.empty_ms += ms; ++t.empty_launches; }
            break;
        }
        e->pool.push_back(std::move(s.a));
        e->pool.push_back(std::move(s.b));
    }
    spans.clear();
}

// ---- model -> device ----------------------------------------------------------------------
void upload_model(hm_engine* e, int ctx, const HostModel& hmw) {
    DeviceModel& dm = e->model[ctx];
    PackedModel pk = pack_model(hmw);
    dm.params.reserve(pk.blob.size() * sizeof(float));
    HIP_TRY(hipMemcpy(dm.params.p, pk.blob.data(), pk.blob.size() * sizeof(float), hipMemcpyHostToDevice));
    const float* base = dm.params.as<float>();
    for (int i = 0; i < 9; ++i) {
        dm.w.wfrag[i] = base + pk.wfrag_off[i];
        dm.w.bias[i] = base + pk.bias_off[i];
    }
    dm.w.fc2_w = base + pk.fc2_w_off;
    dm.w.fc2_b = base + pk.fc2_b_off;
    dm.w.bn = reinterpret_cast<const BnTables*>(base + pk.bn_off);
    for (int i = 0; i < 9; ++i) dm.w.wfrag_h[i] = reinterpret_cast<const uint16_t*>(base + pk.wfrag_h_off[i]);
    dm.w.bn_h = reinterpret_cast<const BnTablesH*>(base + pk.bn_h_off);
    dm.w.c1f = reinterpret_cast<const uint16_t*>(base + pk.c1f_off);
    dm.w.c1f_bias = base + pk.c1f_bias_off;
    dm.w.c1f_corr = base + pk.c1f_corr_off;
    dm.w.k1 = hmw.k1;
    dm.k1 = hmw.k1;
    dm.loaded = true;
}

size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

// diagnostic: sum the per-wave phase stamps of the front launch that was just queued
void accumulate_stamps(hm_engine* e) {
    const int ns = front_stamp_slots();
    const size_t n = (size_t)e->num_cu * 8 * ns;
    std::vector<unsigned long long> h(n);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(h.data(), e->d_stamps.p, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(e->d_stamps.p, 0, n * sizeof(unsigned long long)));
    e->stamp_sum.resize((size_t)ns * 8, 0);
    for (size_t i = 0; i < n; ++i) e->stamp_sum[i % ((size_t)ns * 8)] += h[i];  // [wave in workgroup][slot]
}

// One front + tail pair over the sites named by `sr`, results to logits / p / ml (indexed by uidx for staged reads,
// by position for caller-supplied windows).
void launch_cnn_pair(hm_engine* e, std::vector<TimedSpan>* spans, int ctx, const SiteRange& sr, const hm_batch* b,
                     const float* windows, float* logits, float* p, uint8_t* ml, float* dbg, int dbg_layer) {
    const DeviceModel& dm = e->model[ctx];
    const ReadDesc* reads = b ? b->d_reads.as<ReadDesc>() : nullptr;
    const uint8_t* bases = b ? b->d_bases.as<uint8_t>() : nullptr;
    const uint32_t* kin = b ? b->d_kin.as<uint32_t>() : nullptr;
    {
        Span sp(e, spans, K_FRONT, ctx, sr.off, sr.cap);
        if (e->precision >= 1)
            launch_front_h(e->stream, dm.k1, sr, reads, bases, kin, windows, dm.w, e->d_act4.as<float>(), e->num_cu, dbg,
                           dbg_layer, e->stamps_on ? e->d_stamps.as<unsigned long long>() : nullptr);
        else
            launch_front(e->stream, dm.k1, sr, reads, bases, kin, windows, dm.w, e->d_act4.as<float>(), e->num_cu, dbg,
                         dbg_layer, e->front_waves, e->stamps_on ? e->d_stamps.as<unsigned long long>() : nullptr);
        if (e->stamps_on) accumulate_stamps(e);
        sp.end();
    }
    {
        Span sp(e, spans, K_TAIL, ctx, sr.off, sr.cap);
        if (e->precision >= 1)
            launch_tail_h(e->stream, e->d_act4.as<float>(), sr, dm.w, logits, p, ml, e->num_cu, dbg, dbg_layer);
        else
            launch_tail(e->stream, e->d_act4.as<float>(), sr, dm.w, logits, p, ml, e->num_cu, dbg, dbg_layer);
        sp.end();
    }
}

// CNN over the caller-supplied windows (the hm_cnn_logits / hm_debug_layer seam): exact counts, host-sized launches
void run_cnn_windows(hm_engine* e, int ctx, const float* windows, int64_t n, float* logits, float* p, uint8_t* ml,
                     float* dbg, int dbg_layer) {
    const int64_t sb = e->sub_batch;
    e->d_act4.reserve((size_t)std::min<int64_t>(std::max<int64_t>(n, 1), sb) * ACT4_FLOATS * sizeof(float));
    std::vector<TimedSpan> spans;
    for (int64_t off = 0; off < n; off += sb) {
        const int m = (int)std::min<int64_t>(sb, n - off);
        const SiteRange sr{nullptr, nullptr, ctx, 0, m};
        launch_cnn_pair(e, e->timing ? &spans : nullptr, ctx, sr, nullptr, windows + (size_t)off * KMER * FEATS,
                        logits + 2 * off, p + off, ml + off, dbg, dbg_layer);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(e->stream));
    collect_timing(e, spans, nullptr);
}

// ---- batch slots ------------------------------------------------------------------------------------------------
hm_batch* new_slot(hm_engine* e, int id) {
    std::unique_ptr<hm_batch> b(new hm_batch());
    b->e = e;
    b->id = id;
    HIP_TRY(hipStreamCreateWithFlags(&b->s_io.h, hipStreamNonBlocking));
    for (Event* ev : {&b->ev_in, &b->ev_comp, &b->ev_out}) HIP_TRY(hipEventCreateWithFlags(&ev->h, hipEventDisableTiming));
    b->h_totals.alloc(TOT_COUNT);
    b->h_err.alloc();
    b->d_totals.reserve(TOT_COUNT * sizeof(int32_t));
    b->d_err.reserve(sizeof(int32_t));
    HIP_TRY(hipMemset(b->d_err.p, 0, sizeof(int32_t)));
    HIP_TRY(hipMemset(b->d_totals.p, 0, TOT_COUNT * sizeof(int32_t)));
    hm_batch* raw = b.get();
    e->slots.push_back(std::move(b));
    return raw;
}

void reset_staging(hm_batch* b) {
    b->slab.n = 0;
    b->reads.n = 0;
    b->chunks.n = 0;
    b->rinfo.n = 0;
    b->tiles.n = 0;
    b->tcost.n = 0;
    b->groups.clear();
    b->total_bases = 0;
    b->uploaded = b->ran = b->have_totals = b->have_calls = false;
    memset(b->totals, 0, sizeof b->totals);
}

// ---- staging: EvalKmerFeaturesGenerator::init, a read into the slot's pinned slab exactly as the BAM record stores it ----
// hm_submit_read / hm_batch_submit_read (stage_read) and hm_batch_submit_reads share check_read and place_read; they differ
// in how they grow the slab and in when the bytes are copied.

// Is the read staged?  1 = yes; 0 = passed through uncalled; < 0 = error, recorded for `who` (`full` = what to do about a full
// batch).  tb = the batch's bases including the accepted reads in front of this one.
int check_read(hm_engine* e, const hm_read_t& r, int64_t tb, const char* who, const char* full) {
    if (r.l_qseq < 0) return fail(e, HM_EINVAL, std::string(who) + ": negative read length");
    if (r.l_qseq < e->min_read_size) return 0;                   // mod_main.cpp:189-192
    // a read without bases (min_read_size 0) has no site: staged, it would own four constant tiles whose feature-row loads clamp their
    // position to len - 1 = -1 -- the element in front of the batch's base and kinetics arrays when the read is the batch's first
    if (r.l_qseq == 0) return 0;
    if (!r.kin[0] || !r.kin[1] || !r.kin[2] || !r.kin[3]) return 0;  // BamKinetics::init false (bam_info.cpp:572-603)
    if (!r.seq4) return fail(e, HM_EINVAL, std::string(who) + ": seq4 is NULL");
    for (int k = 0; k < 4; ++k)
        if (r.width[k] != 1 && r.width[k] != 2) return fail(e, HM_EINVAL, "kinetics element width must be 1 (B:C) or 2 (B:S)");
    // site ranks and per-base offsets inside one batch are 32-bit on the device: keep a batch under 2^31 bases
    if (tb + (int64_t)r.l_qseq + 4 >= (int64_t(1) << 31)) return fail(e, HM_ENOMEM, std::string(who) + ": batch would exceed 2^31 bases; " + full);
    return 1;
}

int64_t padded_bases(int32_t l_qseq) { return ((int64_t)l_qseq + 3) & ~int64_t(3); }

struct SlabCopy {
    const void* src;
    size_t off, bytes;
};

// An accepted read takes its place in the batch: descriptor, chunk / tile lists, total_bases, and room in the slab (which the
// caller has reserved) for its five arrays -- the bytes themselves are the caller's to copy: copies[0..4]
void place_read(hm_batch* b, const hm_read_t& r, SlabCopy* copies) {
    const size_t L = (size_t)r.l_qseq;
    auto place = [&](const void* src, size_t bytes) {
        const int64_t off = (int64_t)b->slab.n;
        *copies++ = SlabCopy{src, (size_t)off, bytes};
        b->slab.n += align16(bytes);
        return off;
    };
    ReadDesc rd{};
    rd.off_seq = place(r.seq4, (L + 1) / 2);
    rd.off_fi = place(r.kin[0], L * r.width[0]);
    rd.off_fp = place(r.kin[1], L * r.width[1]);
    rd.off_ri = place(r.kin[2], L * r.width[2]);
    rd.off_rp = place(r.kin[3], L * r.width[3]);
    rd.base_off = b->total_bases;
    rd.len = r.l_qseq;
    rd.flag = r.flag;
    rd.read_id = r.read_id;
    for (int k = 0; k < 4; ++k) rd.w[k] = r.width[k];
    const int ridx = (int)b->reads.n;
    // dense trunk: the read's maps cover view positions [-200, L + 200) in tiles of TR_OWN; a new group starts when
    // the current one holds group_bases
    b->reads.push_back(rd);
    add_read_tiles(b->e, b, ridx, r.l_qseq);
    b->total_bases += padded_bases(r.l_qseq);
}

int stage_read(hm_batch* b, int32_t read_id, int32_t l_qseq, int32_t flag, const uint8_t* seq4, const void* fi, int fi_w,
               const void* fp, int fp_w, const void* ri, int ri_w, const void* rp, int rp_w) {
    auto width = [](int w) { return (uint8_t)std::clamp(w, 0, 255); };  // (anything but 1 and 2 stays something else)
    const hm_read_t r{read_id, l_qseq, flag, {width(fi_w), width(fp_w), width(ri_w), width(rp_w)}, seq4, {fi, fp, ri, rp}};
    const int rc = check_read(b->e, r, b->total_bases, "hm_submit_read", "flush / queue it first");
    if (rc <= 0) return rc;
    return guarded(b->e, [&] {  // (the pinned allocations belong to this engine's device)
        const size_t L = (size_t)l_qseq;
        const size_t need = align16((L + 1) / 2) + align16(L * fi_w) + align16(L * fp_w) + align16(L * ri_w) + align16(L * rp_w);
        if (b->slab.n + need > b->slab.cap) b->slab.reserve(std::max<size_t>((b->slab.n + need) * 2, size_t(64) << 20));
        SlabCopy copies[5];
        place_read(b, r, copies);
        for (const SlabCopy& c : copies) memcpy(b->slab.p + c.off, c.src, c.bytes);
        return 1;
    });
}

// staged slab + descriptors -> HBM, asynchronously on the slot's stream (everything it reads is pinned)
void enqueue_upload(hm_batch* b) {
    const size_t nr = b->reads.n, nc = b->chunks.n;
    b->d_raw.reserve(std::max<size_t>(b->slab.n, 16));
    b->d_reads.reserve(std::max<size_t>(nr, 1) * sizeof(ReadDesc));
    b->d_chunks.reserve(std::max<size_t>(nc, 1) * sizeof(Chunk));
    const size_t tb = (size_t)std::max<int64_t>(b->total_bases, 4);
    b->d_bases.reserve(tb);
    b->d_sctx.reserve(tb);
    b->d_kin.reserve(tb * sizeof(uint32_t));
    b->d_counts.reserve((nc + 1) * NCNT * sizeof(int32_t));
    b->d_offs.reserve((nc + 1) * NCNT * sizeof(int32_t));
    // every forward position carries at most one site over all contexts
    b->d_usites.reserve(tb * sizeof(USite));
    b->d_utag.reserve(tb);
    b->d_csites.reserve(tb * sizeof(Site));
    b->d_opos.reserve(tb * sizeof(int32_t));
    b->d_logits.reserve(tb * 2 * sizeof(float));
    b->d_p.reserve(tb * sizeof(float));
    b->d_ml.reserve(tb);
    b->d_calls.reserve(tb * sizeof(hm_call_t));
    if (b->slab.n) HIP_TRY(hipMemcpyAsync(b->d_raw.p, b->slab.p, b->slab.n, hipMemcpyHostToDevice, b->s_io));
    if (nr) HIP_TRY(hipMemcpyAsync(b->d_reads.p, b->reads.p, nr * sizeof(ReadDesc), hipMemcpyHostToDevice, b->s_io));
    if (nc) HIP_TRY(hipMemcpyAsync(b->d_chunks.p, b->chunks.p, nc * sizeof(Chunk), hipMemcpyHostToDevice, b->s_io));
    b->d_rinfo.reserve(std::max<size_t>(nr, 1) * sizeof(RInfo));
    b->d_tiles.reserve(std::max<size_t>(b->tiles.n, 1) * sizeof(TrunkTile));
    if (nr) HIP_TRY(hipMemcpyAsync(b->d_rinfo.p, b->rinfo.p, nr * sizeof(RInfo), hipMemcpyHostToDevice, b->s_io));
    if (b->tiles.n) HIP_TRY(hipMemcpyAsync(b->d_tiles.p, b->tiles.p, b->tiles.n * sizeof(TrunkTile), hipMemcpyHostToDevice, b->s_io));
    b->d_tcost.reserve(std::max<size_t>(b->tcost.n, 1) * sizeof(int32_t));
    if (b->tcost.n) HIP_TRY(hipMemcpyAsync(b->d_tcost.p, b->tcost.p, b->tcost.n * sizeof(int32_t), hipMemcpyHostToDevice, b->s_io));
    HIP_TRY(hipEventRecord(b->ev_in, b->s_io));
    b->uploaded = true;
    b->ran = b->have_totals = b->have_calls = false;
}

// Does any selected kernel touch the E1 map?  Not when the sliding-window trunk feeds the edge kernel that computes its own E1 rows; strict
// fp32, the older trunks (which always store their rows), the gathering edge kernels and the conv3_w16 diagnostic keep it.
bool trunk_stores_e1(const hm_engine* e) { return e->precision == 0 || e->trunk_impl != 3 || e->edge_impl != 2 || e->conv3_w16 != 0; }

// Dense trunk path: per read group and context  trunk (conv1..conv4 once per view position) -> edge (the two conv4 rows
// per site that are not samples of the maps) -> tail (gathers its conv4 rows).  Every launch is sized by host-known
// quantities (tiles) or reads its site range from the scanned chunk counters on the device.
void run_trunk_path(hm_batch* b, std::vector<TimedSpan>* spans, int ctx_mask) {
    hm_engine* e = b->e;
    int64_t max_rows = 1, max_bases = 1;
    for (const auto& g : b->groups) {
        max_rows = std::max(max_rows, g.rows);
        max_bases = std::max(max_bases, g.bases);
    }
    const bool store_e1 = trunk_stores_e1(e);
    for (int i = store_e1 ? 0 : 1; i < 3; ++i) e->grp.d_map[i].reserve((size_t)max_rows * 2 * 256 * sizeof(uint16_t));
    e->grp.d_e4.reserve((size_t)max_rows * 2 * C4_CH * sizeof(float));
    e->grp.d_rowlist.reserve(std::max((size_t)(max_rows / TR_OWN + 1) * 2 * 3 * TR_OWN, trunk3_rowlist_bytes((max_rows / TR_OWN + 1) * 2)));
    e->grp.d_dump.reserve(trunk3_dump_bytes(e->num_cu));
    e->grp.d_edge4.reserve((size_t)max_bases * 2 * C4_CH * sizeof(float));
    e->grp.d_e4row.reserve((size_t)max_bases * sizeof(int32_t));
    if (e->tail_impl == 3 && e->precision >= 1 && (ctx_mask >> CHH & 1)) {   // strip tail: sized for the largest group, before anything is queued
        e->grp.d_mark.reserve(tail_strip_mark_bytes(2 * max_rows));
        e->grp.d_ccnt.reserve(tail_strip_count_bytes(2 * max_rows));
        e->grp.d_order.reserve((size_t)max_bases * sizeof(int32_t));
        e->grp.d_okey.reserve((size_t)max_bases * sizeof(int32_t));
        e->grp.d_odst.reserve((size_t)max_bases * sizeof(int32_t));
        e->grp.d_x8.reserve(tail_strip_handover_bytes(max_bases));
    }
    if (!e->d_zeros.p) {
        e->d_zeros.reserve(1024);
        HIP_TRY(hipMemsetAsync(e->d_zeros.p, 0, 1024, e->stream));
    }
    const int32_t* offs = b->d_offs.as<int32_t>();
    for (const auto& g : b->groups) {
        const TrunkMaps maps{{store_e1 ? e->grp.d_map[0].as<uint16_t>() : nullptr, e->grp.d_map[1].as<uint16_t>(), e->grp.d_map[2].as<uint16_t>()},
                             e->grp.d_e4.as<uint16_t>(), g.rows, e->d_zeros.as<uint16_t>(), e->grp.d_rowlist.as<uint8_t>()};
        const int n_tiles = g.tile_hi - g.tile_lo;
        for (int c = 0; c < 3; ++c) {
            if (!(ctx_mask >> c & 1)) continue;
            const DeviceModel& dm = e->model[c];
            const int n_views = c == CHH ? 2 : 1;  // CpG / CHG are called on the forward strand only (eval_kmer_features.cpp:89-126)
            const SiteRange sr{b->d_csites.as<Site>(), b->d_totals.as<int32_t>(), c, 0, (int32_t)std::min<int64_t>(g.bases, INT32_MAX),
                               offs + (size_t)NCNT * g.chunk_lo + c, offs + (size_t)NCNT * g.chunk_hi + c};
            if (e->precision == 0) {  // strict fp32: the same three steps on fp32 maps (hm_trunk_f32.hip)
                {
                    Span sp(e, spans, K_TRUNK, c, 0, (int64_t)n_tiles * TR_OWN * n_views);
                    launch_trunk_f32(e->stream, dm.k1, b->d_tiles.as<TrunkTile>() + g.tile_lo, n_tiles, n_views, c, b->d_rinfo.as<RInfo>(),
                                     b->d_bases.as<uint8_t>(), b->d_kin.as<uint32_t>(), b->d_sctx.as<uint8_t>(), dm.w, maps, e->num_cu);
                    sp.end();
                }
                {
                    Span sp(e, spans, K_EDGE, c);
                    launch_edge_f32(e->stream, dm.k1, sr, b->d_rinfo.as<RInfo>(), b->d_bases.as<uint8_t>(), b->d_kin.as<uint32_t>(), dm.w,
                                    maps, e->grp.d_edge4.as<float>(), e->grp.d_e4row.as<int32_t>(), e->num_cu);
                    sp.end();
                }
                Span sp(e, spans, K_TAILG, c);
                launch_tail_gather_f32(e->stream, sr, dm.w, maps, e->grp.d_edge4.as<float>(), e->grp.d_e4row.as<int32_t>(),
                                       b->d_logits.as<float>(), b->d_p.as<float>(), b->d_ml.as<uint8_t>(), e->num_cu);
                sp.end();
                continue;
            }
            {
                Span sp(e, spans, K_TRUNK, c, 0, (int64_t)n_tiles * TR_OWN * n_views);
                if (e->trunk_impl == 3)
                    launch_trunk3(e->stream, dm.k1, b->d_tiles.as<TrunkTile>() + g.tile_lo, n_tiles, n_views, c, b->d_rinfo.as<RInfo>(),
                                  b->d_bases.as<uint8_t>(), b->d_kin.as<uint32_t>(), b->d_sctx.as<uint8_t>(), b->total_bases, dm.w, maps, e->grp.d_dump.as<uint16_t>(),
                                  b->d_totals.as<int32_t>() + TOT_LIST_STEPS, b->d_tcost.as<int32_t>() + g.cost_lo, e->num_cu, e->conv3_w16 != 0, store_e1);
                else if (e->trunk_impl)
                    launch_trunk2(e->stream, dm.k1, b->d_tiles.as<TrunkTile>() + g.tile_lo, n_tiles, n_views, c, b->d_rinfo.as<RInfo>(),
                                  b->d_bases.as<uint8_t>(), b->d_kin.as<uint32_t>(), b->d_sctx.as<uint8_t>(), dm.w, maps, e->num_cu,
                                  e->trunk_impl == 2);
                else
                    launch_trunk(e->stream, dm.k1, b->d_tiles.as<TrunkTile>() + g.tile_lo, n_tiles, n_views, c, b->d_rinfo.as<RInfo>(),
                                 b->d_bases.as<uint8_t>(), b->d_kin.as<uint32_t>(), b->d_sctx.as<uint8_t>(), dm.w, maps, e->num_cu);
                sp.end();
            }
            {
                Span sp(e, spans, K_EDGE, c);
                if (e->edge_impl >= 1)
                    launch_edge2(e->stream, dm.k1, sr, b->d_rinfo.as<RInfo>(), b->d_bases.as<uint8_t>(), b->d_kin.as<uint32_t>(), dm.w,
                                 maps, e->grp.d_edge4.as<uint16_t>(), e->grp.d_e4row.as<int32_t>(), e->num_cu, e->edge_impl == 2);
                else
                    launch_edge(e->stream, dm.k1, sr, b->d_rinfo.as<RInfo>(), b->d_bases.as<uint8_t>(), b->d_kin.as<uint32_t>(), dm.w,
                                maps, e->grp.d_edge4.as<uint16_t>(), e->grp.d_e4row.as<int32_t>(), e->num_cu);
                sp.end();
            }
            {
                Span sp(e, spans, K_TAILG, c);
                if (e->tail_impl == 2 && e->precision >= 1) {
                    // launches of at most tail_slice sites: the hand-off buffer is laid out (and zeroed: its padding rows are never
                    // written) once, for the largest launch seen
                    const int64_t slice = std::min<int64_t>(e->tail_slice, std::max<int64_t>(max_bases, 1));
                    if (slice > e->x6_sites) {
                        e->grp.d_x6.reserve(tail_split_x6_bytes(slice));
                        HIP_TRY(hipMemsetAsync(e->grp.d_x6.p, 0, tail_split_x6_bytes(slice), e->stream));
                        e->x6_sites = slice;
                    }
                    const size_t ph = tail_split_x6_plane_halves(e->x6_sites);
                    for (int64_t off = 0; off < g.bases; off += e->x6_sites) {
                        SiteRange s2 = sr;
                        s2.off = (int32_t)off;
                        s2.cap = (int32_t)std::min<int64_t>(e->x6_sites, g.bases - off);
                        launch_tail_split(e->stream, s2, dm.w, maps, e->grp.d_edge4.as<uint16_t>() + (size_t)off * (4 * C4_CH),
                                          e->grp.d_e4row.as<int32_t>() + off, e->grp.d_x6.as<uint16_t>(), ph, b->d_logits.as<float>(),
                                          b->d_p.as<float>(), b->d_ml.as<uint8_t>(), e->num_cu);
                    }
                } else if (e->tail_impl == 3 && e->precision >= 1 && c == CHH) {
                    launch_tail_strip(e->stream, sr, dm.w, maps, n_views, e->grp.d_edge4.as<uint16_t>(), e->grp.d_e4row.as<int32_t>(), e->grp.d_mark.as<int32_t>(),
                                      e->grp.d_ccnt.as<int32_t>(), e->grp.d_order.as<int32_t>(), e->grp.d_okey.as<int32_t>(), e->grp.d_odst.as<int32_t>(), e->grp.d_x8.as<uint16_t>(),
                                      b->d_logits.as<float>(), b->d_p.as<float>(), b->d_ml.as<uint8_t>(), b->d_totals.as<int32_t>() + TOT_STRIP_PASSES, e->num_cu, e->precision == 2);
                } else if ((e->tail_impl == 1 || e->tail_impl == 3) && e->precision >= 1)
                    launch_tail_gather_r(e->stream, sr, dm.w, maps, e->grp.d_edge4.as<uint16_t>(), e->grp.d_e4row.as<int32_t>(),
                                         b->d_logits.as<float>(), b->d_p.as<float>(), b->d_ml.as<uint8_t>(), e->num_cu, e->precision == 2);
                else
                    launch_tail_gather(e->stream, sr, dm.w, maps, e->grp.d_edge4.as<uint16_t>(), e->grp.d_e4row.as<int32_t>(),
                                       b->d_logits.as<float>(), b->d_p.as<float>(), b->d_ml.as<uint8_t>(), e->num_cu);
                sp.end();
            }
        }
    }
}

// Which contexts take the dense trunk, from a sample of reads: sites per base per context, counted on the host from the
// 4-bit SEQ as stored (at most the first 4 Mi bases; the BAM flag is ignored: a reverse-complemented read has the same CpG
// count and nearly the same CHG / CHH counts), same motifs as the scanners (eval_kmer_features.cpp:67-126).  The trunk costs
// the same per base whatever the number of sites, the per-site kernels cost per site: the trunk wins above ~1.7 % sites per
// base and strand view (CHH, two views: 3.3 %).
struct SeqView {
    const uint8_t* sq;
    int len;
};
template <class Get>
int trunk_mask_from_sample(size_t n, Get get, int ctx_mask) {
    static const int8_t code[16] = {4, 0, 1, 4, 2, 4, 4, 4, 3, 4, 4, 4, 4, 4, 4, 4};  // =ACMGRSVTWYHKDBN -> A0 C1 G2 T3, else 4
    int64_t cnt[3] = {0, 0, 0}, bases = 0;
    for (size_t r = 0; r < n && bases < (int64_t(4) << 20); ++r) {
        const SeqView v = get(r);
        if (!v.sq || v.len <= 0) continue;
        const uint8_t* sq = v.sq;
        const int L = v.len;
        auto at = [&](int i) { return (int)code[(sq[i >> 1] >> ((~i & 1) << 2)) & 15]; };
        int c0 = at(0), c1 = L > 1 ? at(1) : -1;
        for (int i = 0; i + 1 < L; ++i) {
            const int c2 = i + 2 < L ? at(i + 2) : -1;
            if (c0 == 1 && c1 == 2) ++cnt[CPG];
            if (c2 >= 0) {
                const bool h1 = c1 == 0 || c1 == 1 || c1 == 3, h2 = c2 == 0 || c2 == 1 || c2 == 3;
                if (c0 == 1 && h1 && c2 == 2) ++cnt[CHG];
                if (c0 == 1 && h1 && h2) ++cnt[CHH];
                else if ((c0 == 0 || c0 == 2 || c0 == 3) && (c1 == 0 || c1 == 2 || c1 == 3) && c2 == 2) ++cnt[CHH];
            }
            c0 = c1;
            c1 = c2;
        }
        bases += L;
    }
    int m = 0;
    for (int c = 0; c < 3; ++c)
        if ((ctx_mask >> c & 1) && bases > 0 && (double)cnt[c] >= (c == CHH ? 0.033 : 0.017) * (double)bases) m |= 1 << c;
    return m;
}

// contexts whose conv1..conv4 run as the dense trunk for this engine
int trunk_mask_of(hm_batch* b) {
    hm_engine* e = b->e;
    if (e->trunk == 0) return 0;
    if (e->trunk == 1) return e->ctx_mask;
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->trunk_mask_auto < 0) {
        if (b->reads.n == 0) return e->ctx_mask;  // nothing to count (and nothing to run): decide with the first real batch
        e->trunk_mask_auto = trunk_mask_from_sample(
            b->reads.n, [&](size_t r) { return SeqView{b->slab.p + b->reads.p[r].off_seq, b->reads.p[r].len}; }, e->ctx_mask);
    }
    return e->trunk_mask_auto;
}

// scanner + CNN + pack on the compute stream, then the totals' D2H on the slot stream; returns without waiting
void enqueue_run(hm_batch* b) {
    hm_engine* e = b->e;
    std::vector<TimedSpan>* spans = e->timing ? &b->spans : nullptr;
    const int nc = (int)b->chunks.n;
    HIP_TRY(hipStreamWaitEvent(e->stream, b->ev_in, 0));
    {
        Span sp(e, spans, K_PREP);
        launch_prep(e->stream, b->d_raw.as<uint8_t>(), b->d_reads.as<ReadDesc>(), b->d_chunks.as<Chunk>(), nc, e->ctx_mask,
                    b->d_bases.as<uint8_t>(), b->d_kin.as<uint32_t>(), b->d_sctx.as<uint8_t>(), b->d_counts.as<int32_t>(),
                    b->d_err.as<int32_t>());
        sp.end();
    }
    {
        Span sp(e, spans, K_SCAN);
        launch_scan(e->stream, b->d_counts.as<int32_t>(), nc, b->d_offs.as<int32_t>(), b->d_totals.as<int32_t>());
        sp.end();
    }
    {
        Span sp(e, spans, K_EMIT);
        launch_emit(e->stream, b->d_reads.as<ReadDesc>(), b->d_chunks.as<Chunk>(), nc, e->ctx_mask, b->d_bases.as<uint8_t>(),
                    b->d_offs.as<int32_t>(), b->d_totals.as<int32_t>(), b->d_usites.as<USite>(), b->d_utag.as<uint8_t>(),
                    b->d_csites.as<Site>(), b->d_opos.as<int32_t>());
        sp.end();
    }
    const int trunk_mask = trunk_mask_of(b);  // contexts whose conv1..conv4 run as the dense trunk
    if (trunk_mask) run_trunk_path(b, spans, trunk_mask);
    if ((e->ctx_mask & ~trunk_mask) != 0) {
    // The CNN launches cover [0, bound) of every context's list in windows of `sb` sites; how many sites a window
    // really holds is resolved on the device.  bound = staged bases (a position carries at most one site); the
    // window grows with the batch so that a batch never needs more than ~48 launch pairs per context.
    const int64_t bound = nc ? b->total_bases : 0;
    int64_t sb = std::max<int64_t>(e->sub_batch, (bound / 48 + TAIL_SITES) / TAIL_SITES * TAIL_SITES);
    sb = std::min<int64_t>(sb, int64_t(1) << 20);
    e->d_act4.reserve((size_t)std::min<int64_t>(std::max<int64_t>(bound, 1), sb) * ACT4_FLOATS * sizeof(float));
    for (int c = 0; c < 3; ++c) {
        if (!(e->ctx_mask >> c & 1) || (trunk_mask >> c & 1)) continue;
        for (int64_t off = 0; off < bound; off += sb) {
            const SiteRange sr{b->d_csites.as<Site>(), b->d_totals.as<int32_t>(), c, (int32_t)off,
                               (int32_t)std::min<int64_t>(sb, bound - off)};
            launch_cnn_pair(e, spans, c, sr, b, nullptr, b->d_logits.as<float>(), b->d_p.as<float>(), b->d_ml.as<uint8_t>(),
                            nullptr, 0);
        }
    }
    }
    {
        Span sp(e, spans, K_PACK);
        const int64_t bound = nc ? b->total_bases : 0;
        const int grid = (int)std::clamp<int64_t>((bound / 3 + 255) / 256, 1, (int64_t)e->num_cu * 8);
        launch_pack(e->stream, b->d_usites.as<USite>(), b->d_utag.as<uint8_t>(), b->d_opos.as<int32_t>(), b->d_p.as<float>(),
                    b->d_ml.as<uint8_t>(), b->d_reads.as<ReadDesc>(), b->d_totals.as<int32_t>(), b->d_calls.p, grid);
        sp.end();
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev_comp, e->stream));
    HIP_TRY(hipStreamWaitEvent(b->s_io, b->ev_comp, 0));
    HIP_TRY(hipMemcpyAsync(b->h_totals, b->d_totals.p, TOT_COUNT * sizeof(int32_t), hipMemcpyDeviceToHost, b->s_io));
    HIP_TRY(hipMemcpyAsync(b->h_err, b->d_err.p, sizeof(int32_t), hipMemcpyDeviceToHost, b->s_io));
    HIP_TRY(hipEventRecord(b->ev_out, b->s_io));
    b->ran = true;
    b->have_totals = b->have_calls = false;
}

// wait for THIS batch only: its totals are on the host afterwards; reports device-side data errors
int wait_totals(hm_batch* b) {
    hm_engine* e = b->e;
    if (!b->ran) return HM_OK;
    if (!b->have_totals) {
        HIP_TRY(hipEventSynchronize(b->ev_out));
        memcpy(b->totals, b->h_totals, sizeof b->totals);
        b->have_totals = true;
        collect_timing(e, b->spans, b->totals);
    }
    if (*b->h_err) {
        *b->h_err = 0;
        HIP_TRY(hipMemsetAsync(b->d_err.p, 0, sizeof(int32_t), b->s_io));
        HIP_TRY(hipStreamSynchronize(b->s_io));
        return fail(e, HM_EDATA, "illegal BAM base encoded value in a staged read");
    }
    return HM_OK;
}

// the batch's calls in pinned host memory: one packed D2H of exactly n records
int fetch_calls(hm_batch* b) {
    int rc = wait_totals(b);
    if (rc < 0) return rc;
    if (b->have_calls) return HM_OK;
    const size_t n = (size_t)b->totals[TOT_ALL];
    b->h_calls.reserve(std::max<size_t>(n, 1));
    if (n) {
        HIP_TRY(hipMemcpyAsync(b->h_calls.p, b->d_calls.p, n * sizeof(hm_call_t), hipMemcpyDeviceToHost, b->s_io));
        HIP_TRY(hipStreamSynchronize(b->s_io));
    }
    b->h_calls.n = n;
    b->have_calls = true;
    return HM_OK;
}

hm_batch* legacy(hm_engine* e) { return e->slots[0].get(); }

}  // namespace

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int hm_create(hm_engine_t** out, const char* model_dir, int ctx_mask, int device) {
    if (!out || !model_dir || !(ctx_mask & 7)) return fail(nullptr, HM_EINVAL, "hm_create: bad argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(nullptr, HM_EDEVICE, "hm_create: no usable HIP device (this library has no CPU fallback)");
    std::unique_ptr<hm_engine> e(new hm_engine());  // (a failure below gives back what was made so far: ~hm_engine)
    e->device = device;
    const int rc = hip_guard(device, [](const HipErr& h) { return fail_hip(nullptr, h); }, [&] {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        e->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        e->ctx_mask = ctx_mask & 7;
        HIP_TRY(hipStreamCreateWithFlags(&e->stream.h, hipStreamNonBlocking));
        static const char* names[3] = {"CpG", "CHG", "CHH"};  // mod_main.cpp:76,85,94
        for (int c = 0; c < 3; ++c) {
            if (!(e->ctx_mask >> c & 1)) continue;
            HostModel hmw;
            std::string msg;
            if (!load_model_dir(model_dir, names[c], hmw, msg) || !check_model(hmw, names[c], msg)) return fail(nullptr, HM_EMODEL, msg);
            upload_model(e.get(), c, hmw);
        }
        new_slot(e.get(), 0)->state = hm_batch::STAGING;
        return HM_OK;
    });
    if (rc < 0) return rc;
    *out = e.release();
    return HM_OK;
}

void hm_destroy(hm_engine_t* e) { delete e; }  // ~hm_engine: device current, compute stream drained, then the members

const char* hm_last_error(const hm_engine_t* e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int hm_set_option(hm_engine_t* e, const char* key, int64_t value) {
    if (!e || !key) return HM_EINVAL;
    const std::string k(key);
    if (k == "min_read_size") e->min_read_size = (int)value;
    else if (k == "timing") e->timing = value != 0;
    else if (k == "precision") {
        if (value < 0 || value > 2)
            return fail(e, HM_EINVAL, "precision must be 0 (fp32 MFMA), 1 (split-half f16x3 MFMA, fp32 accumulate) or 2 (as 1 with plain fp16 weights in "
                                      "conv8 and fc1: |dp| <= 1e-3)");
        if (value == 2 && (e->tail_impl == 0 || e->tail_impl == 2))
            return fail(e, HM_EINVAL, "precision 2 needs tail_impl 1 or 3 (the resident / strip tail kernels carry the fp16-weight variants)");
        e->precision = (int)value;
    } else if (k == "conv3_w16") {
        e->conv3_w16 = value != 0;
    } else if (k == "stamps") {
        e->stamps_on = value != 0;
        if (e->stamps_on)
            return guarded(e, [&] {
                const size_t bytes = (size_t)e->num_cu * 8 * front_stamp_slots() * sizeof(unsigned long long);
                e->d_stamps.reserve(bytes);
                HIP_TRY(hipMemset(e->d_stamps.p, 0, bytes));
                e->stamp_sum.assign((size_t)front_stamp_slots() * 8, 0);
                return HM_OK;
            });
    } else if (k == "front_waves") {
        if (value != 4 && value != 8) return fail(e, HM_EINVAL, "front_waves must be 4 or 8");
        e->front_waves = (int)value;
    } else if (k == "sub_batch_sites") {
        if (value < TAIL_SITES) return fail(e, HM_EINVAL, "sub_batch_sites too small");
        e->sub_batch = value / TAIL_SITES * TAIL_SITES;
    } else if (k == "trunk") {
        if (value < 0 || value > 2) return fail(e, HM_EINVAL, "trunk must be 0 (per site), 1 (dense trunk) or 2 (by the site density of the first batch)");
        std::lock_guard<std::mutex> lk(e->mu);
        e->trunk = (int)value;
        e->trunk_mask_auto = -1;
    } else if (k == "trunk_mask") {  // the choice of "trunk" = 2 made by the caller (hm_trunk_mask_for_reads): bit c = context c takes the trunk
        if (value < 0 || value > 7) return fail(e, HM_EINVAL, "trunk_mask must be 0..7");
        std::lock_guard<std::mutex> lk(e->mu);
        e->trunk = 2;
        e->trunk_mask_auto = (int)value & e->ctx_mask;
    } else if (k == "trunk_impl") {
        if (value < 0 || value > 3) return HM_EINVAL;
        e->trunk_impl = (int)value;
    } else if (k == "num_cu") {  // workgroups per persistent launch (default: the device's CU count); experiments with engines side by side
        if (value < 1 || value > 1024) return fail(e, HM_EINVAL, "num_cu must be 1..1024");
        e->num_cu = (int)value;
    } else if (k == "edge_impl") {
        if (value < 0 || value > 2) return fail(e, HM_EINVAL, "edge_impl must be 0, 1 or 2");
        e->edge_impl = (int)value;
    } else if (k == "tail_impl") {
        if (value < 0 || value > 3) return fail(e, HM_EINVAL, "tail_impl must be 0, 1, 2 or 3");
        if (e->precision == 2 && (value == 0 || value == 2))   // those tails have no fp16-weight variant: they would run precision 1
            return fail(e, HM_EINVAL, "tail_impl 0 and 2 do not carry precision 2 (fp16 weights in conv8 and fc1): use tail_impl 1 or 3");
        e->tail_impl = (int)value;
    } else if (k == "tail_slice") {
        if (value < 16) return fail(e, HM_EINVAL, "tail_slice must be at least 16");
        e->tail_slice = value;
    } else if (k == "group_bases") {
        if (value < 0 || value > (int64_t(48) << 20))  // (48 Mi bases = 190 GB of maps; the edge kernel counts map rows in 27 bits)
            return fail(e, HM_EINVAL, "group_bases must be 1 .. 48 Mi (0: sized from free device memory)");
        e->group_bases = value;
    } else if (k == "slots") {
        if (value < 1 || value > 16) return fail(e, HM_EINVAL, "slots must be 1..16");
        e->max_slots = (int)value;
    } else return fail(e, HM_EINVAL, "unknown option " + k);
    return HM_OK;
}

// ---- the synchronous calls: one implicit batch (slot 0) ------------------------------------------------------------
int hm_submit_read(hm_engine_t* e, int32_t read_id, int32_t l_qseq, int32_t flag, const uint8_t* seq4,
                   const void* fi, int fi_w, const void* fp, int fp_w, const void* ri, int ri_w, const void* rp,
                   int rp_w) {
    if (!e) return HM_EINVAL;
    hm_batch* b = legacy(e);
    if (b->uploaded) return fail(e, HM_ESTATE, "hm_submit_read: batch already uploaded; hm_clear first");
    return stage_read(b, read_id, l_qseq, flag, seq4, fi, fi_w, fp, fp_w, ri, ri_w, rp, rp_w);
}

int hm_clear(hm_engine_t* e) {
    if (!e) return HM_EINVAL;
    hm_batch* b = legacy(e);
    (void)hipSetDevice(e->device);
    if (b->ran && !b->have_totals) (void)hipEventSynchronize(b->ev_out);
    if (b->s_io) (void)hipStreamSynchronize(b->s_io);
    try {
        collect_timing(e, b->spans, b->ran ? b->h_totals : nullptr);
    } catch (const HipErr&) {
    }
    reset_staging(b);
    return HM_OK;
}

int hm_upload(hm_engine_t* e) {
    if (!e) return HM_EINVAL;
    return guarded(e, [&] {
        enqueue_upload(legacy(e));
        return HM_OK;
    });
}

int hm_run(hm_engine_t* e) {
    if (!e) return HM_EINVAL;
    hm_batch* b = legacy(e);
    if (!b->uploaded) return fail(e, HM_ESTATE, "hm_run: nothing uploaded");
    return guarded(e, [&] {
        if (b->ran && !b->have_totals) {  // a re-run: fold the previous run's spans first
            int rc = wait_totals(b);
            if (rc < 0) return rc;
        }
        enqueue_run(b);
        return HM_OK;
    });
}

int hm_sync(hm_engine_t* e) {
    if (!e) return HM_EINVAL;
    hm_batch* b = legacy(e);
    return guarded(e, [&] {
        if (!b->ran) {
            if (b->uploaded) HIP_TRY(hipEventSynchronize(b->ev_in));
            return HM_OK;
        }
        return wait_totals(b);
    });
}

int64_t hm_num_sites(hm_engine_t* e, int ctx) {
    if (!e || ctx < 0 || ctx > 3) return HM_EINVAL;
    hm_batch* b = legacy(e);
    if (!b->ran) return fail(e, HM_ESTATE, "hm_num_sites: hm_run first");
    const int rc = guarded(e, [&] { return wait_totals(b); });
    return rc < 0 ? rc : b->totals[ctx];
}

int64_t hm_fetch(hm_engine_t* e, hm_call_t* out, int64_t cap) {
    if (!e || (!out && cap > 0)) return HM_EINVAL;
    hm_batch* b = legacy(e);
    if (!b->ran) return fail(e, HM_ESTATE, "hm_fetch: hm_run first");
    const int rc = guarded(e, [&] { return fetch_calls(b); });
    if (rc < 0) return rc;
    const int64_t n = b->totals[TOT_ALL];
    if (n > cap) return fail(e, HM_EINVAL, "hm_fetch: output capacity too small");
    if (n) memcpy(out, b->h_calls.p, (size_t)n * sizeof(hm_call_t));
    return n;
}

int hm_flush(hm_engine_t* e) {
    int rc = hm_upload(e);
    return rc < 0 ? rc : hm_run(e);
}

int64_t hm_drain(hm_engine_t* e, hm_call_t* out, int64_t cap) {
    const int64_t n = hm_fetch(e, out, cap);
    if (n >= 0) hm_clear(e);
    return n;
}

// ---- the asynchronous batch pipeline ---------------------------------------------------------------------------------
hm_batch_t* hm_batch_begin(hm_engine_t* e) {
    if (!e) return nullptr;
    std::unique_lock<std::mutex> lk(e->mu);
    for (;;) {
        for (size_t i = 1; i < e->slots.size(); ++i)
            if (e->slots[i]->state == hm_batch::FREE) {
                hm_batch* b = e->slots[i].get();
                b->state = hm_batch::STAGING;
                reset_staging(b);
                return b;
            }
        if ((int)e->slots.size() - 1 < e->max_slots) {
            auto failed = [e](const HipErr& h) {  // e->mu is held: not through fail()
                e->err = hip_error_text(h);
                return nullptr;
            };
            return hip_guard(e->device, failed, [e] {
                hm_batch* b = new_slot(e, (int)e->slots.size());
                b->state = hm_batch::STAGING;
                return b;
            });
        }
        e->cv.wait(lk);  // every slot is staged or in flight: wait for an hm_batch_release
    }
}

int hm_batch_submit_read(hm_batch_t* b, int32_t read_id, int32_t l_qseq, int32_t flag, const uint8_t* seq4, const void* fi,
                         int fi_w, const void* fp, int fp_w, const void* ri, int ri_w, const void* rp, int rp_w) {
    if (!b) return HM_EINVAL;
    if (b->state != hm_batch::STAGING) return fail(b->e, HM_ESTATE, "hm_batch_submit_read: batch is not being staged");
    return stage_read(b, read_id, l_qseq, flag, seq4, fi, fi_w, fp, fp_w, ri, ri_w, rp, rp_w);
}

int64_t hm_batch_submit_reads(hm_batch_t* b, const hm_read_t* reads, int64_t n, int threads, uint8_t* accepted) {
    if (!b || (!reads && n > 0) || n < 0) return HM_EINVAL;
    hm_engine* e = b->e;
    if (b->state != hm_batch::STAGING) return fail(e, HM_ESTATE, "hm_batch_submit_reads: batch is not being staged");
    // pass 1 (serial): every read's place in the batch and in the slab
    std::vector<SlabCopy> copies;
    copies.reserve((size_t)n * 5);
    const int64_t taken = guarded(e, [&]() -> int64_t {
        // every read is checked before the first one is placed: an error leaves the batch exactly as it was
        std::vector<uint8_t> take((size_t)n);
        size_t need_total = 0;
        int64_t tb = b->total_bases;
        for (int64_t i = 0; i < n; ++i) {
            const int rc = check_read(e, reads[i], tb, "hm_batch_submit_reads", "nothing was staged -- submit fewer reads per batch");
            if (rc < 0) return rc;
            take[(size_t)i] = (uint8_t)rc;
            const size_t L = (size_t)reads[i].l_qseq;
            need_total += align16((L + 1) / 2) + 4 * align16(L * 2);  // (room for every read of the block, as B:S)
            if (rc) tb += padded_bases(reads[i].l_qseq);
        }
        if (b->slab.n + need_total > b->slab.cap) b->slab.reserve(std::max<size_t>(b->slab.n + need_total, size_t(64) << 20));
        int64_t placed = 0;
        for (int64_t i = 0; i < n; ++i) {
            if (accepted) accepted[i] = take[(size_t)i];
            if (!take[(size_t)i]) continue;
            copies.resize(copies.size() + 5);
            place_read(b, reads[i], &copies[copies.size() - 5]);
            ++placed;
        }
        return placed;
    });
    if (taken < 0) return taken;
    // pass 2: the copies, dealt to the host threads
    const int nt = (int)std::clamp<int64_t>(threads, 1, 64);
    uint8_t* base = b->slab.p;
    auto run = [&](int t) {
        for (size_t i = (size_t)t; i < copies.size(); i += (size_t)nt) memcpy(base + copies[i].off, copies[i].src, copies[i].bytes);
    };
    if (nt == 1 || copies.size() < 64) {
        for (int t = 0; t < nt; ++t) run(t);
    } else {
        std::vector<std::thread> pool;
        for (int t = 1; t < nt; ++t) pool.emplace_back(run, t);
        run(0);
        for (auto& th : pool) th.join();
    }
    return taken;
}

int hm_trunk_mask_for_reads(const hm_read_t* reads, int64_t n, int ctx_mask) {
    if ((!reads && n > 0) || n < 0) return HM_EINVAL;
    return trunk_mask_from_sample((size_t)n, [&](size_t r) { return SeqView{reads[r].seq4, reads[r].l_qseq}; }, ctx_mask & 7);
}

int64_t hm_batch_staged_bases(const hm_batch_t* b) { return b ? b->total_bases : HM_EINVAL; }

int hm_batch_enqueue(hm_batch_t* b) {
    if (!b) return HM_EINVAL;
    hm_engine* e = b->e;
    if (b->state != hm_batch::STAGING) return fail(e, HM_ESTATE, "hm_batch_enqueue: batch is not being staged");
    return guarded(e, [&] {
        enqueue_upload(b);  // slot stream: independent of every other batch
        {
            std::lock_guard<std::mutex> lk(e->mu);
            b->state = hm_batch::QUEUED;
        }
        std::lock_guard<std::mutex> lk(e->order_mu);  // the compute stream takes batches in the order they are queued
        enqueue_run(b);
        return HM_OK;
    });
}

int hm_batch_done(hm_batch_t* b) {
    if (!b) return HM_EINVAL;
    if (b->state != hm_batch::QUEUED) return fail(b->e, HM_ESTATE, "hm_batch_done: batch was not queued");
    if (b->have_totals) return 1;
    const hipError_t q = hipEventQuery(b->ev_out);
    if (q == hipSuccess) return 1;
    if (q == hipErrorNotReady) return 0;
    return fail(b->e, HM_EDEVICE, std::string("HIP error: ") + hipGetErrorString(q));
}

int64_t hm_batch_wait(hm_batch_t* b, const hm_call_t** calls) {
    if (!b) return HM_EINVAL;
    hm_engine* e = b->e;
    if (b->state != hm_batch::QUEUED) return fail(e, HM_ESTATE, "hm_batch_wait: batch was not queued");
    const int rc = guarded(e, [&] { return calls ? fetch_calls(b) : wait_totals(b); });
    if (rc < 0) return rc;
    if (calls) *calls = b->h_calls.p;
    return b->totals[TOT_ALL];
}

int64_t hm_batch_num_sites(hm_batch_t* b, int ctx) {
    if (!b || ctx < 0 || ctx > 3) return HM_EINVAL;
    const int64_t rc = hm_batch_wait(b, nullptr);
    return rc < 0 ? rc : b->totals[ctx];
}

int hm_batch_release(hm_batch_t* b) {
    if (!b) return HM_EINVAL;
    hm_engine* e = b->e;
    if (b->state == hm_batch::QUEUED) {  // never hand a slot back while the device still works on it
        (void)hipSetDevice(e->device);
        (void)hipEventSynchronize(b->ev_out);
        (void)hipStreamSynchronize(b->s_io);
        try {
            collect_timing(e, b->spans, b->h_totals);
        } catch (const HipErr&) {
        }
    }
    {
        std::lock_guard<std::mutex> lk(e->mu);
        b->state = hm_batch::FREE;
    }
    e->cv.notify_all();
    return HM_OK;
}

// ---- seams of the parity tests (operate on the synchronous batch) ---------------------------------------------------------
int64_t hm_scan_sites(hm_engine_t* e, int ctx, int32_t* read_id, int32_t* qoff, uint8_t* strand, int64_t cap) {
    if (!e || ctx < 0 || ctx > 2) return HM_EINVAL;
    hm_batch* b = legacy(e);
    if (!b->ran) return fail(e, HM_ESTATE, "hm_scan_sites: hm_run first");
    int rc = hm_sync(e);
    if (rc < 0) return rc;
    const int64_t n = b->totals[ctx];
    if (n > cap) return fail(e, HM_EINVAL, "hm_scan_sites: output capacity too small");
    if (n == 0) return 0;
    return guarded(e, [&] {
        std::vector<Site> s((size_t)n);
        std::vector<uint8_t> tag((size_t)b->totals[TOT_ALL]);
        HIP_TRY(hipMemcpy(s.data(), b->d_csites.as<Site>() + b->totals[TOT_CTX_BASE + ctx], (size_t)n * sizeof(Site), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(tag.data(), b->d_utag.p, tag.size(), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) {
            if (read_id) read_id[i] = b->reads.p[(size_t)s[(size_t)i].read_idx].read_id;
            if (qoff) qoff[i] = s[(size_t)i].qoff;
            if (strand) strand[i] = tag[(size_t)s[(size_t)i].uidx] >> 2;
        }
        return n;
    });
}

int64_t hm_site_logits(hm_engine_t* e, int ctx, float* logits, int64_t cap) {
    if (!e || ctx < 0 || ctx > 2) return HM_EINVAL;
    hm_batch* b = legacy(e);
    if (!b->ran) return fail(e, HM_ESTATE, "hm_site_logits: hm_run first");
    int rc = hm_sync(e);
    if (rc < 0) return rc;
    const int64_t n = b->totals[ctx];
    if (n > cap) return fail(e, HM_EINVAL, "hm_site_logits: output capacity too small");
    if (n == 0) return 0;
    if (!logits) return HM_EINVAL;
    return guarded(e, [&]() -> int64_t {
        // every tail kernel writes logits[2 * uidx]: gather them in the order of the context's list
        std::vector<Site> s((size_t)n);
        std::vector<float> lg((size_t)b->totals[TOT_ALL] * 2);
        HIP_TRY(hipMemcpy(s.data(), b->d_csites.as<Site>() + b->totals[TOT_CTX_BASE + ctx], (size_t)n * sizeof(Site), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(lg.data(), b->d_logits.p, lg.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; ++i) {
            const size_t u = (size_t)s[(size_t)i].uidx;
            if (u >= (size_t)b->totals[TOT_ALL]) return fail(e, HM_EDEVICE, "hm_site_logits: site index out of range");
            logits[2 * i] = lg[2 * u];
            logits[2 * i + 1] = lg[2 * u + 1];
        }
        return n;
    });
}

int hm_debug_edge_rows(hm_engine_t* e, int64_t sites, uint16_t* rows) {
    if (!e || sites < 0 || (sites > 0 && !rows)) return HM_EINVAL;
    hm_batch* b = legacy(e);
    if (!b->ran) return fail(e, HM_ESTATE, "hm_debug_edge_rows: hm_run first");
    int rc = hm_sync(e);
    if (rc < 0) return rc;
    const size_t bytes = (size_t)sites * 4 * C4_CH * sizeof(uint16_t);
    if (bytes > e->grp.d_edge4.cap) return fail(e, HM_EINVAL, "hm_debug_edge_rows: the edge-row buffer holds fewer sites");
    if (sites == 0) return HM_OK;
    return guarded(e, [&] {
        HIP_TRY(hipMemcpy(rows, e->grp.d_edge4.p, bytes, hipMemcpyDeviceToHost));
        return (int)HM_OK;
    });
}

int hm_windows(hm_engine_t* e, int ctx, int64_t first, int64_t n, float* out_host) {
    if (!e || ctx < 0 || ctx > 2 || first < 0 || n < 0) return HM_EINVAL;
    hm_batch* b = legacy(e);
    if (!b->ran) return fail(e, HM_ESTATE, "hm_windows: hm_run first");
    int rc = hm_sync(e);
    if (rc < 0) return rc;
    if (first + n > b->totals[ctx]) return fail(e, HM_EINVAL, "hm_windows: site range out of bounds");
    if (n == 0) return HM_OK;
    return guarded(e, [&] {
        const size_t bytes = (size_t)n * KMER * FEATS * sizeof(float);
        e->d_win.reserve(bytes);
        std::vector<TimedSpan> spans;
        Span sp(e, &spans, K_WINDOW, 0, 0, n);
        launch_windows(e->stream, b->d_csites.as<Site>() + b->totals[TOT_CTX_BASE + ctx] + first, (int)n, b->d_reads.as<ReadDesc>(),
                       b->d_bases.as<uint8_t>(), b->d_kin.as<uint32_t>(), e->model[ctx].w.bn, e->d_win.as<float>(),
                       e->num_cu * 8);
        sp.end();
        HIP_TRY(hipGetLastError());
        if (out_host) HIP_TRY(hipMemcpyAsync(out_host, e->d_win.p, bytes, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        collect_timing(e, spans, nullptr);
        return HM_OK;
    });
}

int hm_cnn_logits(hm_engine_t* e, int ctx, const float* windows, int64_t n, float* logits, float* p, uint8_t* ml) {
    if (!e || ctx < 0 || ctx > 2 || n < 0 || (!windows && n)) return HM_EINVAL;
    if (!e->model[ctx].loaded) return fail(e, HM_EINVAL, "hm_cnn_logits: context not enabled");
    if (n == 0) return HM_OK;
    return guarded(e, [&] {
        const size_t bytes = (size_t)n * KMER * FEATS * sizeof(float);
        e->d_win.reserve(bytes);
        DevBuf d_lg, d_p, d_ml;  // results of this call only: the staged batch's buffers stay untouched
        d_lg.reserve((size_t)n * 2 * sizeof(float));
        d_p.reserve((size_t)n * sizeof(float));
        d_ml.reserve((size_t)n);
        HIP_TRY(hipMemcpyAsync(e->d_win.p, windows, bytes, hipMemcpyHostToDevice, e->stream));
        run_cnn_windows(e, ctx, e->d_win.as<float>(), n, d_lg.as<float>(), d_p.as<float>(), d_ml.as<uint8_t>(), nullptr, 0);
        if (logits) HIP_TRY(hipMemcpy(logits, d_lg.p, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost));
        if (p) HIP_TRY(hipMemcpy(p, d_p.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
        if (ml) HIP_TRY(hipMemcpy(ml, d_ml.p, (size_t)n, hipMemcpyDeviceToHost));
        return HM_OK;
    });
}

int64_t hm_debug_layer(hm_engine_t* e, int ctx, const float* window, int layer, float* out, int64_t cap) {
    if (!e || ctx < 0 || ctx > 2 || !window || !out || layer < 1 || layer > 8) return HM_EINVAL;
    if (!e->model[ctx].loaded) return fail(e, HM_EINVAL, "hm_debug_layer: context not enabled");
    static const int chans[9] = {8, 128, 128, 128, 96, 96, 96, 64, 64};
    int len = KMER;
    const int k1 = e->model[ctx].k1;
    for (int i = 1; i <= layer; ++i) len = (len + 2 - (i == 1 ? k1 : 3)) / 2 + 1;
    const int64_t nf = (int64_t)len * chans[layer];
    if (nf > cap) return fail(e, HM_EINVAL, "hm_debug_layer: output capacity too small");
    return guarded(e, [&] {
        const size_t bytes = (size_t)KMER * FEATS * sizeof(float);
        e->d_win.reserve(bytes);
        e->d_dbg.reserve((size_t)nf * sizeof(float));
        DevBuf res;  // logits / p / ml of the one window
        res.reserve(64);
        HIP_TRY(hipMemcpyAsync(e->d_win.p, window, bytes, hipMemcpyHostToDevice, e->stream));
        run_cnn_windows(e, ctx, e->d_win.as<float>(), 1, res.as<float>(), res.as<float>() + 2,
                        reinterpret_cast<uint8_t*>(res.as<float>() + 3), e->d_dbg.as<float>(), layer);
        // conv4 is the front->tail hand-off and already sits in HBM
        const void* src = layer == 4 ? e->d_act4.p : e->d_dbg.p;
        HIP_TRY(hipMemcpy(out, src, (size_t)nf * sizeof(float), hipMemcpyDeviceToHost));
        return nf;
    });
}

int hm_convert_model(const char* src_path, const char* dst_hmw_path) {
    if (!src_path || !dst_hmw_path) return fail(nullptr, HM_EINVAL, "hm_convert_model: bad argument");
    const std::string src(src_path);
    HostModel m;
    std::string msg;
    const bool is_hmw = src.size() > 4 && src.compare(src.size() - 4, 4, ".hmw") == 0;
    if (!(is_hmw ? load_hmw(src, m, msg) : load_onnx(src, m, msg))) return fail(nullptr, HM_EMODEL, msg);
    if (!save_hmw(m, dst_hmw_path, msg)) return fail(nullptr, HM_EMODEL, msg);
    return HM_OK;
}

int hm_get_stamps(hm_engine_t* e, uint64_t* out, int cap) {
    if (!e || !out) return HM_EINVAL;
    const int n = (int)std::min<size_t>(e->stamp_sum.size(), (size_t)std::max(cap, 0));
    for (int i = 0; i < n; ++i) out[i] = e->stamp_sum[(size_t)i];
    return n;
}

int hm_get_timing(hm_engine_t* e, hm_timing_t* t) {
    if (!e || !t) return HM_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    *t = e->acc;
    t->group_bases = effective_group_bases(e);  // (sized from free device memory now if no read has been staged yet)
    t->group_bytes = e->grp.bytes();
    return HM_OK;
}

/* ABI of include/hifimeth_hip.h: bumped whenever a struct of the header grows (hm_timing_t: round 4 +64 bytes, round 5 +8); a consumer built
 * against another header sees the mismatch instead of having hm_get_timing write past its struct */
int hm_abi_version(void) { return HM_ABI_VERSION; }
size_t hm_timing_size(void) { return sizeof(hm_timing_t); }

int hm_reset_timing(hm_engine_t* e) {
    if (!e) return HM_EINVAL;
    std::lock_guard<std::mutex> lk(e->mu);
    memset(&e->acc, 0, sizeof e->acc);
    return HM_OK;
}

}  // extern "C"
