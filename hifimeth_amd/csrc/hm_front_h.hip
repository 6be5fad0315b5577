// hm_front_h.hip -- split-half ("f16x3") variant of the front kernel (window + bn0 + conv1..conv4).
//
// Every fp32 value x is carried as two halves  x = hi + lo  (hi = fp16(x), lo = fp16(x - hi), ~22 significant
// bits) and every product as three fp16 MFMAs with fp32 accumulation:
//     w*x ~= w_hi*x_hi + w_hi*x_lo + w_lo*x_hi          (v_mfma_f32_16x16x32_f16, 16x the fp32 MFMA rate)
// The dropped w_lo*x_lo term is ~2^-22 relative.  Accumulators, biases and the ReLU stay fp32; the outputs of a
// layer are split again when they are written to LDS.  Same algorithm and layouts as hm_kernels.hip otherwise:
// one site per workgroup pass, activations channels-last in LDS (now as an fp16 hi plane and an fp16 lo plane,
// 4 bytes per element as before), weights as the MFMA A operand so that a lane owns 4 consecutive channels.
// conv1 on the staged-read path is the exception: bn0 is folded into its weights (hm_weights.cpp), which makes its
// operand -- the one-hot base and the decoded frame counts / 32 -- EXACT in fp16: no lo plane, and the weights' hi and
// lo halves ride along K as extra "taps", so one MFMA product per k-block does the whole job (ConvH<..., KSTACK>).
// Scheduling notes that were each worth 1-3 % in same-box A/Bs: a k-block's LDS reads are interleaved with its first
// MFMAs (ILV), the last k-block of conv2 / conv3 is issued tile by tile so the epilogue starts under it (LASTT), and no
// inline asm may read an MFMA result (the compiler only inserts the required wait states for instructions it can see).
// Reference for what is computed: training/model_cnn.py:8-85 / models/*.onnx (mod_main.cpp:32-98).
#include "hm_convh.h"
#include "hm_stamp.h"
#ifdef HM_TRUNK_STAMP
namespace hm { __device__ unsigned long long g_tail_stamp[8][16]; }
extern "C" int hm_debug_tail_stamps(unsigned long long* out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(hm::g_tail_stamp), sizeof(hm::g_tail_stamp)) != hipSuccess) return -1;
    if (reset) {
        static unsigned long long z[8][16];
        if (hipMemcpyToSymbol(HIP_SYMBOL(hm::g_tail_stamp), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

namespace hm {

template <int I, int N, class F>
__device__ __forceinline__ void static_for_h(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for_h<I + 1, N>(f);
    }
}

// ReLU + split; 4 consecutive channels of position m -> the hi and lo planes (physical row m+1)
template <int ORS>
struct EpiPlanes {
    half_t* hi;
    half_t* lo;
    const float* __restrict__ bias;
    __device__ __forceinline__ void operator()(int m, int col, const f32x4& acc) const {
        half4 h, l;
        split4(acc, h, l);
        *reinterpret_cast<half4*>(hi + (m + 1) * ORS + col) = h;
        *reinterpret_cast<half4*>(lo + (m + 1) * ORS + col) = l;
    }
};

template <int COUT>
struct EpiGlobalF {
    float* __restrict__ out;
    const float* __restrict__ bias;
    __device__ __forceinline__ void operator()(int m, int col, const f32x4& acc) const {
        *reinterpret_cast<float4*>(out + (size_t)m * COUT + col) =
            make_float4(fmaxf(acc[0], 0.f), fmaxf(acc[1], 0.f), fmaxf(acc[2], 0.f), fmaxf(acc[3], 0.f));
    }
};

// EpiPlanes for the folded conv1: the first and last output rows reach the conv's zero padding, where the folded
// constant must not count (see hm_weights.cpp)
template <int ORS, int LOUT>
struct EpiPlanesC1 {
    half_t* hi;
    half_t* lo;
    const float* __restrict__ bias;
    float4 c0, c1;  // this lane's four channels of the pad-row corrections [2][128] (see ConvH, EDGE)
    __device__ __forceinline__ void operator()(int m, int col, const f32x4& acc) const {
        half4 h, l;
        split4(acc, h, l);
        *reinterpret_cast<half4*>(hi + (m + 1) * ORS + col) = h;
        *reinterpret_cast<half4*>(lo + (m + 1) * ORS + col) = l;
    }
};

template <int K1>
struct GeoH {
    static constexpr int L1 = (KMER + 2 - K1) / 2 + 1;
    static constexpr int L2 = (L1 - 1) / 2 + 1;
    static constexpr int L3 = (L2 - 1) / 2 + 1;
    static constexpr int L4 = (L3 - 1) / 2 + 1;
    static constexpr int KT1 = (K1 * FEATS + 31) / 32 * 4;  // taps incl. zero-weight K padding: 12 / 16
    static constexpr int WRS = 8;                            // window row = 8 halves = 16 bytes, no padding needed
    static constexpr int WROWS = 2 * (L1 - 1) + KT1;
    static constexpr int RS = 136;                           // 128 channels + 8 halves: 272-byte rows
    // sizes in halves of ONE plane
    static constexpr int A1 = (L1 + 2) * RS, A2 = (L2 + 2) * RS, A3 = (L3 + 2) * RS, WIN = WROWS * WRS;
    static constexpr int PA = A1 > A3 ? A1 : A3;  // plane size in buffer A
    static constexpr int PB = WIN > A2 ? WIN : A2;
    static constexpr int LDS_HALVES = 2 * PA + 2 * PB;
    static_assert(LDS_HALVES * 2 <= 163840, "LDS plan");
};

template <int C>
__device__ __forceinline__ void zero_rows_h(half_t* hi, half_t* lo, int row0, int row1, int rs) {
    for (int i = threadIdx.x; i < 2 * C; i += blockDim.x) {
        const int which = i / C, c = i - which * C;
        const int o = (which ? row1 : row0) * rs + c;
        hi[o] = (half_t)0.f;
        lo[o] = (half_t)0.f;
    }
}

template <int L, int C, int RS>
__device__ __forceinline__ void dump_planes(const half_t* hi, const half_t* lo, float* __restrict__ dbg) {
    for (int i = threadIdx.x; i < L * C; i += blockDim.x) {
        const int o = (i / C + 1) * RS + (i % C);
        dbg[i] = (float)hi[o] + (float)lo[o];
    }
}

template <int K1, bool RAW, bool STAMP = false>
__global__ __launch_bounds__(512) void front_kernel_h(SiteRange sr,
                                                       const ReadDesc* __restrict__ reads,
                                                       const uint8_t* __restrict__ bases,
                                                       const uint32_t* __restrict__ kin,
                                                       const float* __restrict__ windows, CtxWeights W,
                                                       float* __restrict__ act4, float* __restrict__ dbg, int dbg_layer,
                                                       unsigned long long* __restrict__ stamps) {
    using G = GeoH<K1>;
    const Site* sites;
    const int n_sites = resolve_sites(sr, sites);
    unsigned long long tacc[N_STAMP];
    unsigned long long tprev = 0;
    if (STAMP) {
#pragma unroll
        for (int i = 0; i < N_STAMP; ++i) tacc[i] = 0;
    }
    auto mk = [&](int ph) __attribute__((always_inline)) {
        if (STAMP) {
            const unsigned long long t_ = hm_stamp();
            tacc[ph] += t_ - tprev;
            tprev = t_;
        }
    };
    constexpr int NW = 8;
    __shared__ __attribute__((aligned(16))) half_t smem[G::LDS_HALVES];
    half_t* a_hi = smem;
    half_t* a_lo = smem + G::PA;
    half_t* b_hi = smem + 2 * G::PA;
    half_t* b_lo = smem + 2 * G::PA + G::PB;
    const BnTables* __restrict__ bn = W.bn;

    // window rows of site s -> planes B.  One thread per physical row: 8 halves (16 bytes) per plane.
    // Descriptor of the site whose window is built next: fetched one layer ahead (see the site loop), so that the window
    // build itself only waits for ONE level of global loads (the base / kinetics words), not for a chain of four.
    struct SiteCtx {
        int L, qoff, rev;
        int64_t bo;
    };
    auto fetch_ctx = [&](const int s) __attribute__((always_inline)) {
        SiteCtx c{0, 0, 0, 0};
        if (RAW) {
            const Site st = sites[s];
            c.L = reads[st.read_idx].len;
            c.bo = reads[st.read_idx].base_off;
            c.qoff = st.qoff;
            c.rev = bases[c.bo + c.qoff] == 2;
        }
        return c;
    };
    // caller-supplied float windows (the hm_cnn_logits / hm_debug_layer seam): bn0 in fp32, then split into planes B
    auto build_window = [&](const int s, const int t, const int nt) __attribute__((always_inline)) {
        const float* src = windows + (size_t)s * (KMER * FEATS);
        for (int pr = t; pr < G::WROWS; pr += nt) {
            const int w = pr - 1;
            uint32_t v[8];  // (hi | lo << 16) per channel
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = 0u;
            if (w >= 0 && w < KMER) {
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float x = (src[w * 8 + c] - bn->mean[c]) / bn->sd[c] * bn->gamma[c] + bn->beta[c];
                    const half_t h = (half_t)x;
                    const half_t l = (half_t)(x - (float)h);
                    v[c] = (uint32_t)__builtin_bit_cast(uint16_t, h) | ((uint32_t)__builtin_bit_cast(uint16_t, l) << 16);
                }
            }
            uint4 ph, pl;
            ph.x = (v[0] & 0xffffu) | (v[1] << 16);
            ph.y = (v[2] & 0xffffu) | (v[3] << 16);
            ph.z = (v[4] & 0xffffu) | (v[5] << 16);
            ph.w = (v[6] & 0xffffu) | (v[7] << 16);
            pl.x = (v[0] >> 16) | (v[1] & 0xffff0000u);
            pl.y = (v[2] >> 16) | (v[3] & 0xffff0000u);
            pl.z = (v[4] >> 16) | (v[5] & 0xffff0000u);
            pl.w = (v[6] >> 16) | (v[7] & 0xffff0000u);
            *reinterpret_cast<uint4*>(b_hi + pr * G::WRS) = ph;
            *reinterpret_cast<uint4*>(b_lo + pr * G::WRS) = pl;
        }
    };

    // folded layout (FOLD, every staged-read launch): bn0 lives in conv1's weights, so a window row is 8 EXACT halves --
    // the one-hot base (0 / 1) and the four decoded frame counts / 32 (integers <= 952 scaled by a power of two) -- in one
    // plane; rows outside the read and the conv padding are all zeros
    constexpr bool FOLD = RAW;
    constexpr int HB4V = 2;
    constexpr bool HEADS = RAW;  // the float-window seam (tests) keeps the plain prologues
    auto build_window_f = [&](const SiteCtx& cx, const int t, const int nt) __attribute__((always_inline)) {
        const int L = cx.L, qoff = cx.qoff, rev = cx.rev;
        const int64_t bo = cx.bo;
        // up to 4 rows per thread (two waves beside conv4, whose weight stream keeps the vector-memory pipe busy): the
        // base / kinetics words of all rows are requested first, so the rows share one load latency
        constexpr int NRW = 4;
        int bb[NRW];
        uint32_t kk[NRW];
#pragma unroll
        for (int r = 0; r < NRW; ++r) {
            const int pr = t + r * nt, w = pr - 1;
            const int j = rev ? qoff + HK - w : qoff - HK + w;
            bb[r] = -1;  // zeros: conv padding, beyond the window, or outside the read
            kk[r] = 0;
            if (pr < G::WROWS && w >= 0 && w < KMER && j >= 0 && j < L) {
                bb[r] = bases[bo + j];
                kk[r] = kin[bo + j];
            }
        }
#pragma unroll
        for (int r = 0; r < NRW; ++r) {
            const int pr = t + r * nt;
            if (pr < G::WROWS) {
                uint4 row = make_uint4(0u, 0u, 0u, 0u);
                if (bb[r] >= 0) {
                    int b = bb[r];
                    uint32_t k = kk[r];
                    if (rev) {
                        if (b < 4) b = 3 - b;
                        k = (k >> 16) | (k << 16);
                    }
                    // fp16 1.0 = 0x3c00 in the channel of the base
                    row.x = b == 0 ? 0x3c00u : b == 1 ? 0x3c000000u : 0u;
                    row.y = b == 2 ? 0x3c00u : b == 3 ? 0x3c000000u : 0u;
                    // codev1 byte t -> frames = (((t & 63) + 64) << (t >> 6)) - 64 (bam_info.cpp:562-570); frames / 32 is exact in fp16
                    half_t f[4];
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const uint32_t tt = (k >> (8 * c)) & 255u;
                        f[c] = (half_t)((float)((int)(((tt & 63u) + 64u) << (tt >> 6)) - 64) * 0.03125f);
                    }
                    row.z = (uint32_t)__builtin_bit_cast(uint16_t, f[0]) | ((uint32_t)__builtin_bit_cast(uint16_t, f[1]) << 16);
                    row.w = (uint32_t)__builtin_bit_cast(uint16_t, f[2]) | ((uint32_t)__builtin_bit_cast(uint16_t, f[3]) << 16);
                }
                *reinterpret_cast<uint4*>(b_hi + pr * G::WRS) = row;
            }
        }
    };
    auto build_any = [&](const int s, const SiteCtx& cx, const int t, const int nt) __attribute__((always_inline)) {
        if constexpr (FOLD) build_window_f(cx, t, nt);
        else build_window(s, t, nt);
    };
    using C2 = ConvH<NW, 128, 3, 128, G::L2, G::RS, 1, 8, 3, 1, 0, 0, true, false, 0, true, 1>;
    using C3 = ConvH<NW, 128, 3, 128, G::L3, G::RS, 1, 8, 3, 1, 0, 0, true, false, 0, true, 1>;
    using C4 = ConvH<NW, 128, 3, C4_CH, G::L4, G::RS, 1, 6, 3, 1, 0, 0, true, false, 0, true, 1>;
    using C1 = ConvH<NW, 8, (2 * K1 + 3) / 4 * 4, 128, G::L1, G::WRS, 1, 8, 4, 1, 0, 0, false, true, K1, true>;
    constexpr int HB1 = HEADS ? 3 : 0, HB2 = HEADS ? 2 : 0, HB3 = HEADS ? 2 : 0, HB4 = HEADS ? HB4V : 0;
    typename C1::template Head<HB1> h1;
    if constexpr (FOLD) C1::load_head(reinterpret_cast<const half_t*>(W.c1f), W.c1f_bias, h1);
    typename C2::template Head<HB2> h2;
    typename C3::template Head<HB3> h3;
    typename C4::template Head<HB4> h4;
    C2::load_head(reinterpret_cast<const half_t*>(W.wfrag_h[1]), W.bias[1], h2);
    C3::load_head(reinterpret_cast<const half_t*>(W.wfrag_h[2]), W.bias[2], h3);
    C4::load_head(reinterpret_cast<const half_t*>(W.wfrag_h[3]), W.bias[3], h4);
    if ((int)blockIdx.x < n_sites) build_any(blockIdx.x, fetch_ctx(blockIdx.x), threadIdx.x, NW * 64);
    SiteCtx ncx{0, 0, 0, 0};
    for (int s = blockIdx.x; s < n_sites; s += gridDim.x) {
        if (STAMP) tprev = hm_stamp();
        mk(0);
        float4 cr0 = make_float4(0.f, 0.f, 0.f, 0.f), cr1 = cr0;
        if constexpr (FOLD) {  // conv1's pad-row corrections for this lane's channels: requested before the barrier, used at its accumulator init
            const int ccol = (threadIdx.x >> 6) * 16 + 4 * ((threadIdx.x & 63) >> 4);
            cr0 = *reinterpret_cast<const float4*>(W.c1f_corr + ccol);
            cr1 = *reinterpret_cast<const float4*>(W.c1f_corr + 128 + ccol);
        }
        __syncthreads();  // window of site s complete; previous conv4 done with planes A
        mk(1);

        // conv1: window (planes B) -> planes A
        if constexpr (FOLD)
            C1::run(b_hi, b_hi, reinterpret_cast<const half_t*>(W.c1f), EpiPlanesC1<G::RS, G::L1>{a_hi, a_lo, W.c1f_bias, cr0, cr1},
                    [&](int k) __attribute__((always_inline)) { mk(2 + k); }, &h1);
        else
        ConvH<NW, 8, G::KT1, 128, G::L1, G::WRS, 2, 4, 3>::run(b_hi, b_lo, reinterpret_cast<const half_t*>(W.wfrag_h[0]),
                                                             EpiPlanes<G::RS>{a_hi, a_lo, W.bias[0]}, [&](int k) __attribute__((always_inline)) { mk(2 + k); });
        mk(4);
        {   // next site's descriptor: requested here, three layers before the window build needs it
            const int sn1 = s + gridDim.x;
            if (sn1 < n_sites) {
                ncx = fetch_ctx(sn1);
                asm volatile("" : "+v"(ncx.rev));  // keeps the loads here instead of sinking them to the use after conv4
            }
        }
        zero_rows_h<128>(a_hi, a_lo, 0, G::L1 + 1, G::RS);
        __syncthreads();
        mk(5);
        if constexpr (!RAW) {  // the layer dump only exists on the float-window seam (hm_debug_layer)
            if (dbg && dbg_layer == 1 && s == 0) dump_planes<G::L1, 128, G::RS>(a_hi, a_lo, dbg);
        }

        // conv2: planes A -> planes B
        C2::run(a_hi, a_lo, reinterpret_cast<const half_t*>(W.wfrag_h[1]), EpiPlanes<G::RS>{b_hi, b_lo, W.bias[1]},
                [&](int k) __attribute__((always_inline)) { mk(6 + k); }, &h2);
        mk(8);
        zero_rows_h<128>(b_hi, b_lo, 0, G::L2 + 1, G::RS);
        __syncthreads();
        mk(9);
        if constexpr (!RAW) {  // the layer dump only exists on the float-window seam (hm_debug_layer)
            if (dbg && dbg_layer == 2 && s == 0) dump_planes<G::L2, 128, G::RS>(b_hi, b_lo, dbg);
        }

        // conv3: planes B -> planes A
        C3::run(b_hi, b_lo, reinterpret_cast<const half_t*>(W.wfrag_h[2]), EpiPlanes<G::RS>{a_hi, a_lo, W.bias[2]},
                [&](int k) __attribute__((always_inline)) { mk(10 + k); }, &h3);
        mk(12);
        zero_rows_h<128>(a_hi, a_lo, 0, G::L3 + 1, G::RS);
        __syncthreads();
        mk(13);
        if constexpr (!RAW) {  // the layer dump only exists on the float-window seam (hm_debug_layer)
            if (dbg && dbg_layer == 3 && s == 0) dump_planes<G::L3, 128, G::RS>(a_hi, a_lo, dbg);
        }

        // conv4: planes A -> act4[s] (fp32, hand-off to the tail kernel) on 6 waves (one 16-channel tile column
        // each, its first two weight k-blocks resident, the rest two blocks ahead); the other 2 build the next site's window in planes B meanwhile
        C4::run(a_hi, a_lo, reinterpret_cast<const half_t*>(W.wfrag_h[3]), EpiGlobalF<C4_CH>{act4 + (size_t)s * ACT4_FLOATS, W.bias[3]},
                [&](int k) __attribute__((always_inline)) { mk(14 + k); }, &h4);
        mk(16);
        const int sn = s + gridDim.x;
        if (sn < n_sites && (int)threadIdx.x >= 384) build_any(sn, ncx, threadIdx.x - 384, 128);
        mk(17);
    }
    if (STAMP && (threadIdx.x & 63) == 0) {
        unsigned long long* o = stamps + ((size_t)blockIdx.x * NW + (threadIdx.x >> 6)) * N_STAMP;
#pragma unroll
        for (int i = 0; i < N_STAMP; ++i) o[i] = tacc[i];
    }
}

// ------------------------------------------------------------------------------------------------
// split-half tail: conv5 .. conv8, fc1 on fp16x3 MFMA; fc2 + softmax on the VALU in fp32
// ------------------------------------------------------------------------------------------------
template <int LOUT, int ORS, int OSS>
struct EpiPlanesS {
    half_t* hi;
    half_t* lo;
    const float* __restrict__ bias;
    __device__ __forceinline__ void operator()(int m, int col, const f32x4& acc) const {
        const int site = m / LOUT, p = m - site * LOUT;
        half4 h, l;
        split4(acc, h, l);
        *reinterpret_cast<half4*>(hi + site * OSS + (p + 1) * ORS + col) = h;
        *reinterpret_cast<half4*>(lo + site * OSS + (p + 1) * ORS + col) = l;
    }
};

// conv8's output for the batched fc1: rows 0..LOUT-1 of a site back to back (no padding rows), [site][LOUT][ORS]
template <int LOUT, int ORS>
struct EpiRing {
    half_t* hi;
    half_t* lo;
    const float* __restrict__ bias;
    __device__ __forceinline__ void operator()(int m, int col, const f32x4& acc) const {
        half4 h, l;
        split4(acc, h, l);
        *reinterpret_cast<half4*>(hi + m * ORS + col) = h;
        *reinterpret_cast<half4*>(lo + m * ORS + col) = l;
    }
};

template <int HRS>
struct EpiFc1 {  // ReLU, fp32 h[site][256] for the VALU fc2
    float* out;
    const float* __restrict__ bias;
    __device__ __forceinline__ void operator()(int m, int col, const f32x4& acc) const {
        *reinterpret_cast<float4*>(out + m * HRS + col) =
            make_float4(fmaxf(acc[0], 0.f), fmaxf(acc[1], 0.f), fmaxf(acc[2], 0.f), fmaxf(acc[3], 0.f));
    }
};

struct TailGeoH {
    static constexpr int S = TAIL_SITES;
    static constexpr int L4 = 25, L5 = 13, L6 = 7, L7 = 4, L8 = 2;
    static constexpr int RS96 = 104, RS64 = 72, HRS = 260;  // halves, halves, floats
    static constexpr int IN_SS = (L4 + 2) * RS96, C5_SS = (L5 + 2) * RS96, C6_SS = (L6 + 2) * RS96;
    static constexpr int C7_SS = (L7 + 2) * RS64, C8_SS = (L8 + 2) * RS64;
    static constexpr int P0 = S * IN_SS;  // plane size of buffer 0 (also conv6 / conv8 outputs)
    static constexpr int P1 = S * C5_SS;  // plane size of buffer 1 (also conv7 output; fc1 output as floats)
    // fc1 + fc2 run once per FCB groups: conv8's outputs wait in a ring (one plane = FCB * S sites x 2 rows), so the
    // 131 KB of fc1 weights -- the largest fetch of the tail for its smallest matrix job -- stream once per FCB * S sites
    static constexpr int FCB = 4, RING_SS = L8 * RS64, RING = FCB * S * RING_SS;
    static_assert(S * C6_SS <= P0 && S * C7_SS <= P1 && FCB * S * HRS * 2 <= 2 * P1, "tail LDS plan");
    static constexpr int LDS_HALVES = 2 * P0 + 2 * P1 + 2 * RING;
};

template <int S, int LOUT, int C>
__device__ __forceinline__ void zero_pad_rows_h(half_t* hi, half_t* lo, int rs, int ss) {
    for (int i = threadIdx.x; i < S * 2 * C; i += blockDim.x) {
        const int site = i / (2 * C), rem = i - site * 2 * C;
        const int which = rem / C, c = rem - which * C;
        const int o = site * ss + (which ? (LOUT + 1) : 0) * rs + c;
        hi[o] = (half_t)0.f;
        lo[o] = (half_t)0.f;
    }
}

// GATHER (dense trunk path, hm_trunk.hip): a site's conv4 rows are not read from an act4 hand-off buffer but gathered
// where they were computed: rows 1..23 are rows e4row[site] + 16 s of the dense E4 map, rows 0 and 24 the site's two
// window-edge rows from the edge kernel.  Both producers write their rows already split ([hi 96 | lo 96] fp16 halves,
// the same 384 bytes as fp32), so the gather is a pure copy into the input planes: the spare waves of conv6 / conv7 /
// conv8 issue it as LDS-DMA (global_load_lds_dwordx4: no VGPRs, no VALU split, no ds_write), one 1 KB piece of a plane per
// wave instruction with a per-lane source address (a zero page for padding rows, row pads and sites past the end).
template <bool GATHER = false>
__global__ __launch_bounds__(512) void tail_kernel_h(const float* __restrict__ act4, SiteRange sr, CtxWeights W,
                                                      float* __restrict__ logits,
                                                      float* __restrict__ prob, uint8_t* __restrict__ ml,
                                                      float* __restrict__ dbg, int dbg_layer,
                                                      const half_t* __restrict__ e4 = nullptr,
                                                      const half_t* __restrict__ edge4 = nullptr,
                                                      const int32_t* __restrict__ e4row = nullptr,
                                                      const half_t* __restrict__ zeros = nullptr) {
    using T = TailGeoH;
    constexpr int S = T::S, NW = 8;
    const Site* sites;
    const int n_sites = resolve_sites(sr, sites);
    // A workgroup takes a CONTIGUOUS range of 8-site groups: neighbouring sites read the same E4 rows (a row serves the ~3
    // sites whose windows sample it), so they come from this CU's L1 / its XCD's L2 instead of HBM again.
    const int n_groups = (n_sites + S - 1) / S, base_n = n_groups / (int)gridDim.x, rem_n = n_groups - base_n * (int)gridDim.x;
    const int g_begin = (int)blockIdx.x * base_n + min((int)blockIdx.x, rem_n), g_end = g_begin + base_n + ((int)blockIdx.x < rem_n);
    __shared__ __attribute__((aligned(16))) half_t smem[T::LDS_HALVES];
    half_t* h0 = smem;
    half_t* l0 = smem + T::P0;
    half_t* h1 = smem + 2 * T::P0;
    half_t* l1 = smem + 2 * T::P0 + T::P1;
    float* hfc = reinterpret_cast<float*>(h1);  // fc1 activations (fp32) reuse buffer 1
    half_t* r_hi = smem + 2 * T::P0 + 2 * T::P1;
    half_t* r_lo = r_hi + T::RING;
    constexpr int FCB = T::FCB;
    __shared__ float fc2w[2 * 256 + 2];          // fc2 weights + bias stay in LDS for the whole kernel
    for (int i = threadIdx.x; i < 2 * 256 + 2; i += NW * 64) fc2w[i] = i < 512 ? W.fc2_w[i] : W.fc2_b[i - 512];
    auto wf = [&](int i) { return reinterpret_cast<const half_t*>(W.wfrag_h[i]); };

    // Input staging.  The conv4 rows of a group of S sites (S * 600 float4: the act4 hand-off, or gathered from the E4 map
    // and the edge rows) are brought in by the waves that have NO tile in conv6 / conv7 / conv8, one phase ahead of their
    // use: a wave's vector-memory results return in order, so a prefetch issued by a compute wave stands in front of that
    // wave's next weight fragment and its full HBM latency is exposed at the head of conv5 (measured: 26 of 77 ms).
    //   conv6 phase: waves 6,7 REQUEST sites 3..7 of the next group       (conv6 runs on waves 0..5)
    //   conv7 phase: waves 6,7 split + store them (that part of buffer 0 is dead since conv5); waves 4,5 request sites 0..2
    //   conv8 phase: waves 4,5 split + store sites 0..2 (conv6's output, which lived there, is dead after conv7);
    //                wave 7 requests the map rows of the group after next (GATHER)
    auto wave_id = [&]() __attribute__((always_inline)) { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); };
    constexpr int Q4 = ACT4_FLOATS / 4;
    constexpr int SPLIT_SITE = 3;  // S * C6_SS (conv6's output in buffer 0) ends inside site 2's input rows
    static_assert(S * T::C6_SS <= SPLIT_SITE * T::IN_SS, "conv6's output must not reach the sites staged during conv7");
    constexpr int NHI = ((S - SPLIT_SITE) * Q4 + 127) / 128, NLO = (SPLIT_SITE * Q4 + 127) / 128;
    auto load_row = [&](int grp, int t) __attribute__((always_inline)) {
        int32_t r = 0;
        if (GATHER && t < S && grp * S + t < n_sites) r = e4row[grp * S + t];
        return r;
    };
    // element i (float4 index inside the group) of group `grp`
    auto elem_src = [&](int grp, int i, int) __attribute__((always_inline)) -> const float* {
        const int first = grp * S, site = i / Q4;
        if (first + site >= n_sites) return nullptr;
        return act4 + (size_t)first * ACT4_FLOATS + (size_t)i * 4;
    };
    // ---- GATHER: LDS-DMA staging ----------------------------------------------------------------------------------
    // A plane of the input (hi or lo) is S * 27 rows of 13 sixteen-byte units (12 data + 1 pad) = 2808 units; piece p
    // = units [64 p, 64 p + 64) = one wave instruction (the LDS side of an LDS-DMA is wave-uniform base + 16 * lane).
    constexpr int UNITS = S * (T::L4 + 2) * 13, PIECES = (UNITS + 63) / 64;
    static_assert(T::RS96 * 2 == 13 * 16 && T::IN_SS == (T::L4 + 2) * T::RS96, "input plane = rows of 13 units");
    // pieces below LOW_PIECES overlap conv6's output in buffer 0 and may only be written once conv7 has read it
    constexpr int LOW_PIECES = (S * T::C6_SS * 2 + 1023) / 1024;
    const int lane = threadIdx.x & 63;
    // Pieces [P_LO, P_HI) of plane PL, dealt round-robin to the NWV waves starting at wave W0.  The loop over a wave's
    // pieces is unrolled, so a lane's unit 64 p + lane = U0 (compile time) + t with t = 64 (wave - W0) + lane fixed for the
    // whole kernel: row, channel chunk, site and window position follow from t / 13 and t % 13 (computed once) with two
    // carries instead of two integer divisions per piece, the site's map row comes out of `rows` (lane l holds the row of
    // site l & 7) by readlane, and the source is selected without branches -- the spare waves' address arithmetic, not the
    // DMA, set the length of the conv6 / conv8 phases (measured: 680 cycles per piece).
    auto stage_set = [&](auto pl_, auto plo_, auto phi_, auto w0_, auto nwv_, const int grp, const int32_t rows) __attribute__((always_inline)) {
        constexpr int PL = decltype(pl_)::value, P_LO = decltype(plo_)::value, P_HI = decltype(phi_)::value;
        constexpr int W0 = decltype(w0_)::value, NWV = decltype(nwv_)::value;
        constexpr int K = (P_HI - P_LO + NWV - 1) / NWV;
        const int wo = wave_id() - W0;
        const int t = 64 * wo + lane, tq = t / 13, t13 = t - 13 * tq;
        const uint32_t plane0 = __builtin_amdgcn_readfirstlane(
            (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) half_t*)(PL ? l0 : h0));
        const half_t* e4p = e4 + PL * C4_CH;
        const half_t* edp = edge4 + PL * C4_CH;
        static_for_h<0, K>([&](auto k_) __attribute__((always_inline)) {
            constexpr int k = decltype(k_)::value;
            constexpr int U0 = 64 * (P_LO + k * NWV), AQ = U0 / 13, AR = U0 % 13, BQ = AQ / (T::L4 + 2), BR_ = AQ % (T::L4 + 2);
            if ((P_LO + (k + 1) * NWV <= P_HI) || P_LO + k * NWV + wo < P_HI) {
                const int s1 = AR + t13, c1 = s1 >= 13, ch = s1 - 13 * c1;
                const int s2 = BR_ + tq + c1, c2 = (s2 >= T::L4 + 2) + (s2 >= 2 * (T::L4 + 2)), prow = s2 - (T::L4 + 2) * c2;
                static_assert((T::L4 + 1) + (64 * NWV - 1) / 13 + 1 < 3 * (T::L4 + 2), "at most two row-to-site carries");
                const int site = BQ + c2, pos = prow - 1, gs = grp * S + site;
                const int32_t ra = __builtin_amdgcn_readlane(rows, BQ < S ? BQ : S - 1), rb = __builtin_amdgcn_readlane(rows, BQ + 1 < S ? BQ + 1 : S - 1);
                const int32_t rc = __builtin_amdgcn_readlane(rows, BQ + 2 < S ? BQ + 2 : S - 1);
                const int64_t mrow = (int64_t)(c2 == 0 ? ra : c2 == 1 ? rb : rc) + 16 * pos;
                const bool data = pos >= 0 && pos < C4_LEN && ch < 12 && gs < n_sites && site < S;
                const bool edge = pos == 0 || pos == C4_LEN - 1;
                const half_t* sm = e4p + mrow * (2 * C4_CH) + ch * 8;
                const half_t* se = edp + (int64_t)gs * (4 * C4_CH) + (pos ? 2 * C4_CH : 0) + ch * 8;
                const half_t* src = data ? (edge ? se : sm) : zeros;
                const uint32_t dst = plane0 + 1024u * (uint32_t)(P_LO + k * NWV + wo);
                uint32_t keep;
                if (U0 + 64 * NWV <= UNITS || U0 + t < UNITS)
                    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
            }
        });
    };
    // The same pieces with the lane's (site, window position, channel chunk) of every piece PRECOMPUTED: which unit of the
    // input plane a lane writes depends on the piece and the thread only, not on the group, so a staging thread packs it once
    // per kernel -- offset inside the site's rows (20 bits) | site carry (2) | kind 0 pad / 1 map row / 2 edge row (2) | unit
    // inside the plane (1) -- and a piece then costs ~20 instead of ~60 instructions (the conv8 phase lasted as long as its
    // staging waves' address arithmetic).
    auto stage_desc = [&](auto plo_, auto phi_, auto w0_, auto nwv_, auto k_) __attribute__((always_inline)) -> uint32_t {
        constexpr int P_LO = decltype(plo_)::value, W0 = decltype(w0_)::value, NWV = decltype(nwv_)::value, k = decltype(k_)::value;
        const int wo = max(wave_id() - W0, 0);
        const int t = 64 * wo + lane, tq = t / 13, t13 = t - 13 * tq;
        constexpr int U0 = 64 * (P_LO + k * NWV), AQ = U0 / 13, AR = U0 % 13, BQ = AQ / (T::L4 + 2), BR_ = AQ % (T::L4 + 2);
        const int s1 = AR + t13, c1 = s1 >= 13, ch = s1 - 13 * c1;
        const int s2 = BR_ + tq + c1, c2 = (s2 >= T::L4 + 2) + (s2 >= 2 * (T::L4 + 2)), prow = s2 - (T::L4 + 2) * c2;
        const int site = BQ + c2, pos = prow - 1;
        const bool data = pos >= 0 && pos < C4_LEN && ch < 12 && site < S;
        const bool edge = pos == 0 || pos == C4_LEN - 1;
        const int rel = edge ? (pos ? 2 * C4_CH : 0) + ch * 8 : 16 * pos * (2 * C4_CH) + ch * 8;
        return (data ? (uint32_t)rel : 0u) | ((uint32_t)c2 << 20) | ((data ? (edge ? 2u : 1u) : 0u) << 22) | ((U0 + t < UNITS ? 1u : 0u) << 24);
    };
    auto stage_fast = [&](auto pl_, auto plo_, auto phi_, auto w0_, auto nwv_, const int grp, const int32_t rows, const auto& desc) __attribute__((always_inline)) {
        constexpr int PL = decltype(pl_)::value, P_LO = decltype(plo_)::value, P_HI = decltype(phi_)::value;
        constexpr int W0 = decltype(w0_)::value, NWV = decltype(nwv_)::value;
        constexpr int K = (P_HI - P_LO + NWV - 1) / NWV;
        const int wo = wave_id() - W0;
        const uint32_t plane0 = __builtin_amdgcn_readfirstlane(
            (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) half_t*)(PL ? l0 : h0));
        const half_t* e4p = e4 + PL * C4_CH;
        const half_t* edp = edge4 + PL * C4_CH;
        static_for_h<0, K>([&](auto k_) __attribute__((always_inline)) {
            constexpr int k = decltype(k_)::value;
            constexpr int U0 = 64 * (P_LO + k * NWV), BQ = U0 / 13 / (T::L4 + 2);
            if ((P_LO + (k + 1) * NWV <= P_HI) || P_LO + k * NWV + wo < P_HI) {
                const uint32_t d = desc[k];
                const int rel = d & 0xfffff, c2 = (d >> 20) & 3, kind = (d >> 22) & 3;
                const int gs = grp * S + BQ + c2;
                const int32_t ra = __builtin_amdgcn_readlane(rows, BQ < S ? BQ : S - 1), rb = __builtin_amdgcn_readlane(rows, BQ + 1 < S ? BQ + 1 : S - 1);
                const int32_t rc = __builtin_amdgcn_readlane(rows, BQ + 2 < S ? BQ + 2 : S - 1);
                const int32_t rowv = c2 == 0 ? ra : c2 == 1 ? rb : rc;
                const half_t* sm = e4p + ((int64_t)rowv * (2 * C4_CH) + rel);
                const half_t* se = edp + ((int64_t)gs * (4 * C4_CH) + rel);
                const half_t* src = kind != 0 && gs < n_sites ? (kind == 2 ? se : sm) : zeros;
                const uint32_t dst = plane0 + 1024u * (uint32_t)(P_LO + k * NWV + wo);
                uint32_t keep;
                if (U0 + 64 * NWV <= UNITS || (d >> 24))
                    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                                 : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
            }
        });
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I4 = std::integral_constant<int, 4>;
    using I6 = std::integral_constant<int, 6>;
    using I8 = std::integral_constant<int, 8>;
    using ILOW = std::integral_constant<int, LOW_PIECES>;
    using IPCS = std::integral_constant<int, PIECES>;
    auto put_elem = [&](int i, const float4& v) __attribute__((always_inline)) {  // fp32 -> split planes 0, rows 1..25
        const int site = i / Q4, rem = (i - site * Q4) * 4;
        const int pos = rem / C4_CH, c = rem - pos * C4_CH;
        half4 h, l;
        split4(f32x4{v.x, v.y, v.z, v.w}, h, l);  // conv4 rows are post-ReLU already: the max() is a no-op
        const int o = site * T::IN_SS + (pos + 1) * T::RS96 + c;
        *reinterpret_cast<half4*>(h0 + o) = h;
        *reinterpret_cast<half4*>(l0 + o) = l;
    };
    // zero the two padding rows of input sites [s_lo, s_hi) by threads [0, nt)
    auto zero_in_pads = [&](int s_lo, int s_hi, int t, int nt) __attribute__((always_inline)) {
        for (int i = t; i < (s_hi - s_lo) * 2 * 96; i += nt) {
            const int site = s_lo + i / 192, rem = i % 192;
            const int o = site * T::IN_SS + (rem >= 96 ? (T::L4 + 1) : 0) * T::RS96 + (rem % 96);
            h0[o] = (half_t)0.f;
            l0[o] = (half_t)0.f;
        }
    };
    // "defines" v without an instruction.  The staged rows are written by some waves only and read a phase later behind
    // the same (wave-uniform) condition; the compiler cannot correlate the two branches, so without a definition on the
    // other paths the registers would count as live around the whole loop -- across conv5 -- and spill.
    auto fake_def = [](float4& v) __attribute__((always_inline)) { asm volatile("" : "=v"(v.x), "=v"(v.y), "=v"(v.z), "=v"(v.w)); };
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int32_t pend = 0, rows = 0;  // GATHER: lane l of a staging wave holds the E4 map row (position off - 215) of site l & 7 of the
                                 // group it stages next (rows) / of the group after that (pend, requested a pass ahead)
    int it = 0;
    float4 phi[NHI], plo[NLO];
    // staging descriptors of this thread: conv7 phase (waves 4..7: the lo plane's pieces behind conv6's output), conv8 phase
    // (waves 4..7: the pieces that held conv6's output, both planes)
    constexpr int KB_ = (PIECES - LOW_PIECES + 3) / 4, KC = (LOW_PIECES + 3) / 4;
    uint32_t dB[KB_], dC[KC];
    if constexpr (GATHER) {
        static_for_h<0, KB_>([&](auto k_) __attribute__((always_inline)) { dB[decltype(k_)::value] = stage_desc(ILOW{}, IPCS{}, I4{}, I4{}, k_); });
        static_for_h<0, KC>([&](auto k_) __attribute__((always_inline)) { dC[decltype(k_)::value] = stage_desc(I0{}, ILOW{}, I4{}, I4{}, k_); });
    }

    // first group of this workgroup: staged by everybody
    if constexpr (GATHER) {
        rows = load_row(g_begin, lane & (S - 1));
        if (wave >= 4) pend = load_row(g_begin + 1, lane & (S - 1));
    }
    if (g_begin < g_end) {
        if constexpr (GATHER) {
            stage_set(I0{}, I0{}, IPCS{}, I0{}, I8{}, g_begin, rows);
            stage_set(I1{}, I0{}, IPCS{}, I0{}, I8{}, g_begin, rows);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the DMA is invisible to the compiler's own wait counting
        } else {
            for (int i = threadIdx.x; i < S * Q4; i += NW * 64) {
                const float* src = elem_src(g_begin, i, 0);
                put_elem(i, src ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f));
            }
            zero_in_pads(0, S, threadIdx.x, NW * 64);
        }
    }
    int slot = 0, g_first = g_begin;  // groups g_first, g_first + 1, ... wait in ring slots 0 .. slot-1
#ifdef HM_TRUNK_STAMP
    unsigned long long tts[14], tacc[12] = {};
    unsigned long long tn = 0;
    const bool tst = blockIdx.x == 0 && GATHER;
#define TTS(i) do { if (tst) tts[i] = hm_stamp(); } while (0)
#else
#define TTS(i)
#endif
    for (int g = g_begin; g < g_end; ++g) {
        const bool more = g + 1 < g_end;
        if constexpr (GATHER) {  // map rows of group g + grid (requested one iteration ago) -> LDS
            ++it;
            rows = pend;
        }
        __syncthreads();  // input of group g staged (by the previous iteration's spare waves)
        TTS(0);

        // (wave grids 2x3, 1x6, 4x1 and weight prefetch depths 4, 5 measured the same or worse in same-session A/Bs)
#ifdef HM_TRUNK_STAMP
        ConvH<NW, 96, 3, 96, T::L5, T::RS96, 4, 2, 3, S, T::IN_SS, 0>::run(
            h0, l0, wf(4), EpiPlanesS<T::L5, T::RS96, T::C5_SS>{h1, l1, W.bias[4]},
            [&](int i) __attribute__((always_inline)) { if (tst) tts[10 + i] = hm_stamp(); });
        if (tst) { tacc[10] += tts[10] - tts[0]; tacc[11] += tts[11] - tts[10]; }
#else
        ConvH<NW, 96, 3, 96, T::L5, T::RS96, 4, 2, 3, S, T::IN_SS, 0>::run(
            h0, l0, wf(4), EpiPlanesS<T::L5, T::RS96, T::C5_SS>{h1, l1, W.bias[4]});
#endif
        zero_pad_rows_h<S, T::L5, 96>(h1, l1, T::RS96, T::C5_SS);
        TTS(1);
        __syncthreads();
        TTS(2);
        if (dbg && dbg_layer == 5 && g == 0) dump_planes<T::L5, 96, T::RS96>(h1, l1, dbg);

        // conv6 / conv7 as 1xN grids (a wave owns one 16-channel tile and every position): with 4x2 / 2x4 grids four
        // waves fetched the same weight fragments and the vector-memory pipe, not the MFMA, set the pace
        // (explicit if / else on the wave id, not a call that returns early: the staged rows must not be live across
        //  the other waves' conv code or they spill)
        if (GATHER && wave >= 6) {  // spare in conv6: the hi plane's pieces behind conv6's output, by LDS-DMA
            if (more) stage_set(I0{}, ILOW{}, IPCS{}, I6{}, I2{}, g + 1, rows);  // (this phase lasts as long as conv6: no descriptors spent on it)
        } else if (wave >= 6) {  // spare in conv6: request sites 3..7 of the next group
            if (more) {
                int tl = threadIdx.x;
                asm volatile("" : "+v"(tl));  // keep the element index arithmetic inside the loop (hoisted, it spills)
#pragma unroll
                for (int k = 0; k < NHI; ++k) {
                    const int i = SPLIT_SITE * Q4 + tl - 384 + k * 128;
                    const float* src = i < S * Q4 ? elem_src(g + 1, i, it & 1) : nullptr;
                    phi[k] = src ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            else {
#pragma unroll
                for (int k = 0; k < NHI; ++k) fake_def(phi[k]);
            }
        } else {
            ConvH<NW, 96, 3, 96, T::L6, T::RS96, 1, 6, 3, S, T::C5_SS, 0>::run(
                h1, l1, wf(5), EpiPlanesS<T::L6, T::RS96, T::C6_SS>{h0, l0, W.bias[5]});
#pragma unroll
            for (int k = 0; k < NHI; ++k) fake_def(phi[k]);
        }
        zero_pad_rows_h<S, T::L6, 96>(h0, l0, T::RS96, T::C6_SS);
        TTS(3);
        __syncthreads();
        TTS(4);
        if (dbg && dbg_layer == 6 && g == 0) dump_planes<T::L6, 96, T::RS96>(h0, l0, dbg);

        if (GATHER && wave >= 4) {  // spare in conv7: the same pieces of the lo plane
            if (more) stage_fast(I1{}, ILOW{}, IPCS{}, I4{}, I4{}, g + 1, rows, dB);
        } else if (wave >= 6) {  // spare in conv7: the requested rows -> buffer 0 (behind conv6's output)
            if (more) {
                int tl = threadIdx.x;
                asm volatile("" : "+v"(tl));
#pragma unroll
                for (int k = 0; k < NHI; ++k) {
                    const int i = SPLIT_SITE * Q4 + tl - 384 + k * 128;
                    if (i < S * Q4) put_elem(i, phi[k]);
                }
                zero_in_pads(SPLIT_SITE, S, tl - 384, 128);
            }
#pragma unroll
            for (int k = 0; k < NLO; ++k) fake_def(plo[k]);
        } else if (wave >= 4) {  // request sites 0..2
            if (more) {
                int tl = threadIdx.x;
                asm volatile("" : "+v"(tl));
#pragma unroll
                for (int k = 0; k < NLO; ++k) {
                    const int i = tl - 256 + k * 128;
                    const float* src = i < SPLIT_SITE * Q4 ? elem_src(g + 1, i, it & 1) : nullptr;
                    plo[k] = src ? *reinterpret_cast<const float4*>(src) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else {
#pragma unroll
                for (int k = 0; k < NLO; ++k) fake_def(plo[k]);
            }
        } else {
            ConvH<NW, 96, 3, 64, T::L7, T::RS96, 1, 4, 3, S, T::C6_SS, 0>::run(
                h0, l0, wf(6), EpiPlanesS<T::L7, T::RS64, T::C7_SS>{h1, l1, W.bias[6]});
#pragma unroll
            for (int k = 0; k < NLO; ++k) fake_def(plo[k]);
        }
        zero_pad_rows_h<S, T::L7, 64>(h1, l1, T::RS64, T::C7_SS);
        TTS(5);
        __syncthreads();
        TTS(6);
        if (dbg && dbg_layer == 7 && g == 0) dump_planes<T::L7, 64, T::RS64>(h1, l1, dbg);

        if (GATHER && wave >= 4) {  // spare in conv8: the pieces that held conv6's output (dead since the last barrier)
            if (more) {
                stage_fast(I0{}, I0{}, ILOW{}, I4{}, I4{}, g + 1, rows, dC);
                stage_fast(I1{}, I0{}, ILOW{}, I4{}, I4{}, g + 1, rows, dC);
            }
            pend = load_row(g + 2, lane & (S - 1));
            // everything this wave staged for the next group is in LDS before it reaches the barrier in front of conv5
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else if (wave >= 4) {
            if (more && wave < 6) {  // spare in conv8: sites 0..2 (conv6's output there is dead since the last barrier)
                int tl = threadIdx.x;
                asm volatile("" : "+v"(tl));
#pragma unroll
                for (int k = 0; k < NLO; ++k) {
                    const int i = tl - 256 + k * 128;
                    if (i < SPLIT_SITE * Q4) put_elem(i, plo[k]);
                }
                zero_in_pads(0, SPLIT_SITE, tl - 256, 128);
            }
        } else {
            ConvH<NW, 64, 3, 64, T::L8, T::RS64, 1, 4, 3, S, T::C7_SS, 0>::run(
                h1, l1, wf(7), EpiRing<T::L8, T::RS64>{r_hi + slot * S * T::RING_SS, r_lo + slot * S * T::RING_SS, W.bias[7]});
        }
        TTS(7);
#ifdef HM_TRUNK_STAMP
        if (tst) { for (int i = 0; i < 7; ++i) tacc[i] += tts[i + 1] - tts[i]; ++tn; }
#endif
        if (slot == 0) g_first = g;
        ++slot;
        if (dbg && dbg_layer == 8 && g == 0) {
            __syncthreads();
            for (int i = threadIdx.x; i < T::L8 * 64; i += NW * 64) {
                const int o = (i / 64) * T::RS64 + (i % 64);
                dbg[i] = (float)r_hi[o] + (float)r_lo[o];
            }
        }
        if (slot < FCB && more) continue;  // the loop-top barrier orders this conv8 before the next conv5
        __syncthreads();
        TTS(8);

        // fc1 as a 2-tap "conv" over conv8's two positions (k order l*64 + c; see hm_weights.cpp), FCB * S sites at once;
        // slots this batch did not fill hold stale rows whose results are never written out
        ConvH<NW, 64, 2, 256, 1, T::RS64, 1, 8, 2, FCB * S, T::RING_SS, 0>::run(r_hi, r_lo, wf(8), EpiFc1<T::HRS>{hfc, W.bias[8]});
        __syncthreads();

        // fc2 + softmax (mod_batch.cpp:46-64) in fp32: 16 lanes per site = 2 outputs x 8 partial sums
        {
            static_assert(FCB * S * 16 == NW * 64, "one 16-lane team per site");
            const int bsite = threadIdx.x >> 4, o = (threadIdx.x >> 3) & 1, part = threadIdx.x & 7;
            const float* h = hfc + bsite * T::HRS + part * 32;
            const float* w2 = fc2w + o * 256 + part * 32;
            float sum = 0.f;
#pragma unroll 8
            for (int k = 0; k < 32; ++k) sum = fmaf(h[k], w2[k], sum);
            sum += __shfl_xor(sum, 4, 64);
            sum += __shfl_xor(sum, 2, 64);
            sum += __shfl_xor(sum, 1, 64);
            sum += fc2w[512 + o];
            const float other = __shfl_xor(sum, 8, 64);
            const int sl = bsite / S, site = bsite - sl * S;
            const int gs0 = (g_first + sl) * S;
            if ((threadIdx.x & 15) == 0 && sl < slot && gs0 + site < n_sites) {
                const float v0 = sum, v1 = other;
                const float mx = fmaxf(v0, v1);
                const float e0 = expf(v0 - mx), e1 = expf(v1 - mx);
                const float p1 = e1 / (e0 + e1);
                int q = (int)(255 * p1);
                q = q > 255 ? 255 : q;
                const int dst = sites ? sites[gs0 + site].uidx : gs0 + site;
                logits[2 * (size_t)dst] = v0;
                logits[2 * (size_t)dst + 1] = v1;
                prob[dst] = p1;
                ml[dst] = (uint8_t)q;
            }
        }
        slot = 0;  // hfc (buffer 1) and the ring are next written behind the loop-top barrier / the conv7 barrier
        TTS(9);
#ifdef HM_TRUNK_STAMP
        if (tst) { tacc[8] += tts[9] - tts[8]; tacc[9] += 1; }
#endif
    }
#ifdef HM_TRUNK_STAMP
    if (tst && (threadIdx.x & 63) == 0) {
        for (int i = 0; i < 10; ++i) atomicAdd(&g_tail_stamp[threadIdx.x >> 6][i], tacc[i]);
        atomicAdd(&g_tail_stamp[threadIdx.x >> 6][10], tn);
        atomicAdd(&g_tail_stamp[threadIdx.x >> 6][11], tacc[10]);
        atomicAdd(&g_tail_stamp[threadIdx.x >> 6][12], tacc[11]);
    }
#endif
#undef TTS
}

static int cnn_grid_h(const SiteRange& sr, int per_group, int grid) {
    if (sr.totals) return grid;
    return max(1, min((sr.cap + per_group - 1) / per_group, grid));
}

void launch_tail_h(hipStream_t st, const float* act4, const SiteRange& sr, const CtxWeights& w, float* logits,
                   float* p, uint8_t* ml, int grid, float* dbg, int dbg_layer) {
    if (sr.cap <= 0) return;
    const dim3 g(cnn_grid_h(sr, TAIL_SITES, grid));
    hipLaunchKernelGGL((tail_kernel_h<false>), g, dim3(512), 0, st, act4, sr, w, logits, p, ml, dbg, dbg_layer,
                       nullptr, nullptr, nullptr, nullptr);
}

void launch_tail_gather(hipStream_t st, const SiteRange& sr, const CtxWeights& w, const TrunkMaps& maps, const uint16_t* edge4,
                        const int32_t* e4row, float* logits, float* p, uint8_t* ml, int grid) {
    if (sr.cap <= 0) return;
    const dim3 g(cnn_grid_h(sr, TAIL_SITES, grid));
    hipLaunchKernelGGL((tail_kernel_h<true>), g, dim3(512), 0, st, nullptr, sr, w, logits, p, ml, nullptr, 0,
                       reinterpret_cast<const half_t*>(maps.e4), reinterpret_cast<const half_t*>(edge4), e4row,
                       reinterpret_cast<const half_t*>(maps.zeros));
}

void launch_front_h(hipStream_t st, int k1, const SiteRange& sr, const ReadDesc* reads, const uint8_t* bases,
                    const uint32_t* kin, const float* windows, const CtxWeights& w, float* act4, int grid, float* dbg,
                    int dbg_layer, unsigned long long* stamps) {
    if (sr.cap <= 0) return;
    const dim3 g(cnn_grid_h(sr, 1, grid)), b(512);
    const bool raw = windows == nullptr;
#define HM_FRONT_H(K1, RAW, ST)                                                                                  \
    hipLaunchKernelGGL((front_kernel_h<K1, RAW, ST>), g, b, 0, st, sr, reads, bases, kin, windows, w, act4, dbg, \
                       dbg_layer, stamps)
    if (stamps && raw) {
        if (k1 == 11) HM_FRONT_H(11, true, true); else HM_FRONT_H(13, true, true);
    } else if (k1 == 11) { if (raw) HM_FRONT_H(11, true, false); else HM_FRONT_H(11, false, false); }
    else { if (raw) HM_FRONT_H(13, true, false); else HM_FRONT_H(13, false, false); }
#undef HM_FRONT_H
}

}  // namespace hm
