// Wide models: interaction, and gather + interaction, for 33 <= F <= 128 features on the matrix cores (fp32, "dot").
//   evs_interact_dot_wide           dense form: F feature pointers with row strides
//   evs_emb_interact_wide_stacked   gather form: x + T fp32 tables behind one stacked (T, B) index tensor, one index per bag
//
// The headline kernel (evs_fused.hip) keeps a sample's T T^T as a fixed 2 x 2 grid of 16 x 16 tiles; past 32 features the triangle
// has up to 36 tiles and does not fit a fixed set of accumulators.  Here the ROWS stay and the tiles pass through:
//   * a block of 256 threads owns 16 consecutive samples, each of its four waves takes four of them, one at a time
//   * gather form: the block first brings its index tile into LDS -- one 128-byte run of 16 int64 per table, T x 128 bytes --
//     behind one barrier; a wave then reads its sample's indices from LDS (a column of the tile), not with 8-byte loads from T lines.
//     In LDS a table's run is 17 entries apart, so the 16 lanes of a column read 16 different bank pairs
//   * for v_mfma_f32_16x16x4_f32 the A and the B operand of T T^T have the same lane layout (evs_interact.hip's header): lane
//     (r = lane % 16, q = lane / 16) holds KS = d / 4 elements of row 16 t + r of row-tile t -- the CQ = d / 16 whole 16-byte pieces
//     at q CQ, and for d = 36 element q of the last piece, which the four q share.  A wave loads the NT row-tiles of its sample
//     ONCE, NT KS registers (128 at F = 128, d = 64), and every tile (ti, tj <= ti) is a chain of KS MFMAs between two register
//     sets.  No LDS for operands.  Rows past F read the zero page; row-tiles past F are skipped (wave-uniform).
//   * where two generations of rows fit (NT KS <= 64) the next sample's rows are requested under this sample's MFMAs
//   * output by bands: in R's packed order the pairs of rows 16 ti .. 16 ti + 15 are one contiguous run (band 0: x, then the
//     pairs).  The wave drops the accumulators of band ti into its own LDS band buffer -- the diagonal tile masked to j < i, or
//     j <= i with itself -- at the run's own 16-byte phase, and streams the run out with full-wave 16-byte stores; the first
//     and the last piece of a run go element by element where the run starts or ends inside them.
//   * tables or feature pointers and their row counts or strides travel in the kernel arguments (2 x 128 x 8 bytes): no
//     device-side descriptor, no allocation or synchronisation per call.  Both forms run the same instantiation -- they differ
//     in how a lane forms its row address (a block-uniform branch).
// Templates: d in {16, 32, 36, 64} x NT in {3, 4, 6, 8} (F <= 48 / 64 / 96 / 128): register arrays statically indexed.
#include "evs_fused_wide.h"
#include <string.h>
#include <atomic>

namespace evs {

template <int D, int NT>
__global__ void __launch_bounds__(256) interact_wide_kernel(const WideArgs args) {
    constexpr int KS = D / 4, CQ = D / 16;
    constexpr bool REM = (D % 16) != 0;          // d = 36: a last 16-byte piece shared by the four k-slots
    static_assert(D % 4 == 0 && (D % 16 == 0 || D % 16 == 4), "KS = 4 CQ (+ 1)");
    constexpr int ROWS = 16 * NT;
    constexpr bool AHEAD = NT * KS <= 64;        // two generations of rows in registers
    // the largest band: rows 16 (NT - 1) .. 16 NT - 1 with itself, shifted by up to 3 floats, whole 16-byte pieces
    constexpr int BAND = (256 * (NT - 1) + 136 + 3 + 3) / 4 * 4;
    static_assert(D + 136 + 6 <= BAND, "band 0 carries x");
    constexpr int IDXROW = 17;   // a table's 16 indices and one of padding: the 16 lanes of a column read 16 different bank pairs
    __shared__ int64_t s_idx[(ROWS - 1) * IDXROW];
    __shared__ const char *s_base[ROWS];
    __shared__ int64_t s_aux[ROWS];
    __shared__ __attribute__((aligned(16))) float s_band[4][BAND];

    const WideArgs *ka = (const WideArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    const int F = args.F, B = args.B, out_row = args.out_row;
    const bool gather = args.idx != nullptr;
    const int64_t blk_first = (int64_t)blockIdx.x * 16;

    if (tid < ROWS) {
        s_base[tid] = tid < F ? ka->base[tid] : nullptr;
        s_aux[tid] = tid < F ? ka->aux[tid] : 0;
    }
    if (gather) {   // the index tile: 16 lanes take the 16 samples of one table, 16 tables per pass
        const int s = tid & 15;
        const int64_t b = blk_first + s;
        for (int t = tid >> 4; t < F - 1; t += 16) s_idx[t * IDXROW + s] = b < B ? args.idx[t * args.idx_stride + b] : 0;
    }
    __syncthreads();

    float *band = s_band[wave];
    bool bad = false;

    // the NT KS operand registers of sample `sib` of the block
    auto request = [&](int sib, float (&a)[NT][KS]) {
        const int64_t b = blk_first + sib;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (16 * t < F) {   // wave-uniform
                const int f = 16 * t + r16;
                const char *p = args.zeros;
                if (f < F) {
                    const char *bs = s_base[f];
                    const int64_t ax = s_aux[f];
                    if (!gather || f == 0) {
                        p = bs + b * ax;
                    } else {
                        const int64_t i = s_idx[(f - 1) * IDXROW + sib];
                        if ((uint64_t)i < (uint64_t)ax) p = bs + i * (int64_t)(D * 4);
                        else bad = true;   // a zero row, and the sticky flag
                    }
                }
                // p comes out of LDS, so the compiler cannot see its address space: say that it is global memory, or the rows are
                // flat loads, which count with the LDS reads, and every wait for the band buffer waits for the rows requested ahead
                const global_f32x4 *p4 = (const global_f32x4 *)(p + q * (CQ * 16));
#pragma unroll
                for (int c = 0; c < CQ; c++) {
                    const f32x4 v = p4[c];
                    a[t][4 * c] = v.x; a[t][4 * c + 1] = v.y; a[t][4 * c + 2] = v.z; a[t][4 * c + 3] = v.w;
                }
                if constexpr (REM) {
                    const f32x4 v = *(const global_f32x4 *)(p + 4 * CQ * 16);
                    a[t][4 * CQ] = q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w;
                }
            } else {
#pragma unroll
                for (int s = 0; s < KS; s++) a[t][s] = 0.f;
            }
        }
    };

    // T T^T of one sample from its registers, band by band, into R
    auto consume = [&](int sib, const float (&a)[NT][KS]) {
        float *Rb = args.R + (blk_first + sib) * (int64_t)out_row;
#pragma unroll
        for (int ti = 0; ti < NT; ti++) {
            // A band's offsets, lane masks and buffer positions depend on F, itself and the lane alone, so the compiler would work
            // all NT bands' out in front of the sample loop and keep them: more scalar registers than there are (up to 83 spilled
            // to VGPR lanes) and 4 NT and more VGPRs.  Behind this empty statement it takes the three for unknown, works a band's
            // values out in the band, a few instructions beside its MFMAs, and nothing of a band outlives it.
            int F = args.F, itself = args.itself, lane = tid & 63;
            asm volatile("" : "+s"(F), "+s"(itself), "+v"(lane));
            const int r16 = lane & 15, q = lane >> 4;
            if (16 * ti < F) {   // wave-uniform
                const int i0 = 16 * ti, iend = i0 + 16 < F ? i0 + 16 : F;
                const int tri0 = wide_tri(i0, itself);
                const int head = ti == 0 ? D : 0;                       // band 0 starts with x
                const int len = head + wide_tri(iend, itself) - tri0;
                float *dst = Rb + (ti == 0 ? 0 : D + tri0);
                const int sh = (int)((reinterpret_cast<uintptr_t>(dst) >> 2) & 3);   // the run's phase inside a 16-byte piece
                int ro[4];   // where row 16 ti + 4 q + v starts in the band buffer (this lane's column added), -1: no such row
#pragma unroll
                for (int v = 0; v < 4; v++) {
                    const int i = i0 + 4 * q + v;
                    ro[v] = i < F ? sh + head + wide_tri(i, itself) - tri0 + r16 : -1;
                }
                if (ti == 0 && r16 == 0) {   // x, bit for bit: row 0 is in the lanes (0, q)
#pragma unroll
                    for (int s = 0; s < 4 * CQ; s++) band[sh + q * (4 * CQ) + s] = a[0][s];
                    if constexpr (REM) band[sh + 16 * CQ + q] = a[0][4 * CQ];
                }
#pragma unroll
                for (int tj = 0; tj <= ti; tj++) {
                    f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < KS; s++) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[ti][s], a[tj][s], c, 0, 0, 0);
#pragma unroll
                    for (int v = 0; v < 4; v++)   // c[v] = Z[16 ti + 4 q + v][16 tj + r16]
                        if (ro[v] >= 0 && (tj < ti || r16 < 4 * q + v + itself)) band[ro[v] + 16 * tj] = c[v];
                }
                // the band is complete in LDS (this wave's own writes, in order): stream the run out
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int end = sh + len;
                float *g = dst - sh;   // 16-byte aligned
                for (int p = lane; 4 * p < end; p += 64) {
                    const int L = 4 * p;
                    const f32x4 v = reinterpret_cast<const f32x4 *>(band)[p];
                    if (L >= sh && L + 4 <= end) {
                        __builtin_nontemporal_store(v, reinterpret_cast<f32x4 *>(g + L));   // R is written once and streams out
                    } else {   // the run starts or ends inside this piece
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            if (L + e >= sh && L + e < end) g[L + e] = v[e];
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();   // the next band's writes stay behind these reads
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
    };

    const int first = 4 * wave;
    if (blk_first + first < B) {   // (wave-uniform; a tail block may leave whole waves without a sample)
        float a[NT][KS];
        request(first, a);
#pragma unroll 1
        for (int k = 0; k < 4; k++) {
            const bool more = k + 1 < 4 && blk_first + first + k + 1 < B;
            if constexpr (AHEAD) {
                float n[NT][KS];
                if (more) request(first + k + 1, n);
                consume(first + k, a);
                if (!more) break;
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int s = 0; s < KS; s++) a[t][s] = n[t][s];
            } else {
                consume(first + k, a);
                if (!more) break;
                request(first + k + 1, a);
            }
        }
    }
    if (bad) atomicOr(args.err, 1);
}

// the dispatch record (evs_wide_kernels_seen): id = form (dense, gather) * 16 + d (16, 32, 36, 64) * 4 + nt (3, 4, 6, 8)
constexpr int kWideCount = 32;
static std::atomic<long long> g_wide_seen[kWideCount];

template <int D>
static void launch_wide_d(const WideArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)(((int64_t)a.B + 15) / 16)), block(256);
    switch (wide_nt_id(a.F)) {
    case 0: hipLaunchKernelGGL((interact_wide_kernel<D, 3>), grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL((interact_wide_kernel<D, 4>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((interact_wide_kernel<D, 6>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((interact_wide_kernel<D, 8>), grid, block, 0, st, a); break;
    }
}

static int launch_wide(WideArgs &a, int d, hipStream_t st) {
    a.zeros = reinterpret_cast<const char *>(zero_page());
    a.err = index_error_flag();
    if (!a.zeros || !a.err) return EVS_EHIP;
    for (int f = a.F; f < EVS_MAX_WIDE_FEATURES; f++) { a.base[f] = nullptr; a.aux[f] = 0; }
    a.out_row = d + (a.itself ? a.F * (a.F + 1) / 2 : a.F * (a.F - 1) / 2);
    switch (d) {
    case 16: launch_wide_d<16>(a, st); break;
    case 32: launch_wide_d<32>(a, st); break;
    case 36: launch_wide_d<36>(a, st); break;
    default: launch_wide_d<64>(a, st); break;
    }
    EVS_HIP_CHECK(hipGetLastError());
    g_wide_seen[(a.idx ? 16 : 0) + wide_d_id(d) * 4 + wide_nt_id(a.F)].fetch_add(1, std::memory_order_relaxed);
    return EVS_OK;
}

}  // namespace evs

extern "C" int evs_wide_kernels_seen(char *buf, int n) {
    int len = 0;
    if (buf && n > 0) buf[0] = 0;
    for (int id = 0; id < evs::kWideCount; id++) {
        char line[64];
        const int k = snprintf(line, sizeof line, "wide_%s_d%d_nt%d=%lld\n", id < 16 ? "dense" : "gather", evs::kWideD[(id % 16) / 4],
                               evs::kWideNt[id % 4], evs::g_wide_seen[id].load(std::memory_order_relaxed));
        if (buf && len + k < n) memcpy(buf + len, line, (size_t)k + 1);
        len += k;
    }
    return len;
}

extern "C" int evs_interact_dot_wide(int64_t B, int F, int d, const float *const *feats, const int64_t *feat_strides, int itself,
                                     float *R, void *stream) {
    using namespace evs;
    const char *who = "evs_interact_dot_wide";
    if (int rc = wide_shape_ok(who, B, F, d)) return rc;
    if (B == 0) return EVS_OK;
    EVS_REQUIRE(feats && feat_strides && R, "%s: NULL argument", who);
    EVS_REQUIRE(B < (1ll << 31), "%s: B %lld (below 2^31)", who, (long long)B);
    EVS_REQUIRE(aligned16(R), "%s: R is not 16-byte aligned", who);
    WideArgs a;
    for (int f = 0; f < F; f++) {
        EVS_REQUIRE(feats[f], "%s: feats[%d] is NULL", who, f);
        EVS_REQUIRE(aligned16(feats[f]), "%s: feats[%d] is not 16-byte aligned", who, f);
        EVS_REQUIRE(feat_strides[f] % 4 == 0, "%s: feat_strides[%d] = %lld is not a multiple of 4", who, f, (long long)feat_strides[f]);
        a.base[f] = reinterpret_cast<const char *>(feats[f]);
        a.aux[f] = feat_strides[f] * 4;
    }
    a.idx = nullptr; a.idx_stride = 0;
    a.R = R; a.B = (int)B; a.F = F; a.itself = itself ? 1 : 0;
    return launch_wide(a, d, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int evs_emb_interact_wide_stacked(int64_t B, int T, int d, const void *const *tables, const int64_t *n_rows, const float *x,
                                             int64_t x_stride, const int64_t *indices, int64_t idx_stride, int itself, float *R,
                                             void *stream) {
    using namespace evs;
    const char *who = "evs_emb_interact_wide_stacked";
    EVS_REQUIRE(T >= 0 && T < (1 << 30), "%s: bad shape T=%d", who, T);
    const int F = T + 1;
    if (int rc = wide_shape_ok(who, B, F, d)) return rc;
    if (B == 0) return EVS_OK;
    EVS_REQUIRE(tables && n_rows && x && indices && R, "%s: NULL argument", who);
    EVS_REQUIRE(B < (1ll << 31), "%s: B %lld (below 2^31)", who, (long long)B);
    EVS_REQUIRE(aligned16(R), "%s: R is not 16-byte aligned", who);
    EVS_REQUIRE(aligned16(x) && x_stride % 4 == 0, "%s: x is not 16-byte aligned or its stride %lld is not a multiple of 4", who,
                (long long)x_stride);
    EVS_REQUIRE(reinterpret_cast<uintptr_t>(indices) % 8 == 0 && idx_stride >= 0, "%s: indices are not 8-byte aligned, or a negative stride",
                who);
    WideArgs a;
    a.base[0] = reinterpret_cast<const char *>(x);
    a.aux[0] = x_stride * 4;
    for (int k = 0; k < T; k++) {
        EVS_REQUIRE(n_rows[k] >= 0 && n_rows[k] < (1ll << 31), "%s: table %d: n_rows %lld (below 2^31)", who, k, (long long)n_rows[k]);
        EVS_REQUIRE(tables[k] || n_rows[k] == 0, "%s: table %d is NULL", who, k);
        EVS_REQUIRE(aligned16(tables[k]), "%s: table %d is not 16-byte aligned", who, k);
        a.base[k + 1] = reinterpret_cast<const char *>(tables[k]);
        a.aux[k + 1] = n_rows[k];
    }
    a.idx = indices; a.idx_stride = idx_stride;
    a.R = R; a.B = (int)B; a.F = F; a.itself = itself ? 1 : 0;
    return launch_wide(a, d, reinterpret_cast<hipStream_t>(stream));
}
