// Long-bag sum pooling over ENCODED tables (u16 / u8 / u4) for gfx950: evs_embedding_bag_sum_long.
//
// The fp32 long-bag kernel (evs_gather.hip, bag_sum_long_kernel) keeps K rows of a bag in flight as 16-byte pieces, four VGPRs
// per row.  An encoded piece is 8 / 4 / 2 bytes: the rows wait in registers as RAW code words -- two VGPRs per row for u16, one
// for u8 and u4 -- so a chunk is two to four times as deep on the same register budget, and the decode (LDS table reads, the
// u16 arithmetic) is off the load path: it runs once the words have arrived, while the next chunk's indices are on the wire.
//   * a wave item is (table, 64 / LPR consecutive bags), LPR = d / 4; the LPR lanes that will hold a pooled row own its bag;
//     four items per 256-thread block; the table id is wave-uniform (its descriptors are scalar loads)
//   * the bag's next K indices arrive as coalesced loads of the group (lane l takes index l, l + LPR, ...), each is handed to
//     the group (ds_bpermute), the K pieces are requested back to back in sub-blocks of 8; a sub-block that lies behind the
//     LONGEST bag of the wave is skipped by a wave-uniform branch (ragged batches of short bags request nothing for it), a
//     slot behind this lane's own bag inside a live sub-block reads the zero code page
//   * decoded rows are added in index order, unfused fp32 adds from +0.0f: the bits of the oracle's loop.  The zero code
//     decodes to exactly 0.0f and x + 0.0f is x for every x the accumulator can hold.
#include "evs_common.h"
#include <string.h>
#include <atomic>

namespace evs {

struct LongQArgs {
    const void *table[EVS_MAX_TABLES_PER_LAUNCH];
    const int64_t *indices[EVS_MAX_TABLES_PER_LAUNCH];
    const int64_t *offsets[EVS_MAX_TABLES_PER_LAUNCH];
    int n_rows[EVS_MAX_TABLES_PER_LAUNCH];   // (the entry refuses 2^31 and above)
    int nnz[EVS_MAX_TABLES_PER_LAUNCH];
    float *out;
    int64_t out_tstride, out_bstride;
    int B;
    int T;
    int *err;
    const void *zeros;   // zero_code_page(CODEC)
};

constexpr int kLqCodec[3] = {16, 8, 4};
constexpr int kLqLpr[5] = {4, 8, 9, 16, 32};
constexpr int kLqSub = 8;   // rows per guarded sub-block of a chunk
// K, the rows of a bag in flight per lane.  The raw words of a chunk take at most 64 VGPRs (what the fp32 kernel spends on its
// 16 rows); narrow rows (LPR <= 9: 7 to 16 bags per wave) stop at half of that, the wave has its rows in flight through its
// many bags.  A wave counts at most 63 outstanding vector-memory loads: K plus the next chunk's index loads stays below that
// (56 + 4, not 64 + 4).  u16 at d = 64 spilled two registers at K = 32 under the four-waves bound of the kernel: it runs at 24.
constexpr int lq_chunk(int codec, int lpr) {
    const bool wide = lpr >= 16;
    return codec == 16 ? (lpr == 16 ? 24 : wide ? 32 : 16) : (wide ? 56 : 32);
}
constexpr int lq_codec_id(int codec) { return codec == 16 ? 0 : codec == 8 ? 1 : codec == 4 ? 2 : -1; }
constexpr int lq_lpr_id(int lpr) { return lpr == 4 ? 0 : lpr == 8 ? 1 : lpr == 9 ? 2 : lpr == 16 ? 3 : lpr == 32 ? 4 : -1; }

typedef unsigned lq_u32x2 __attribute__((ext_vector_type(2)));
// the raw words of one piece: 8 / 4 / 2 bytes from global memory
template <int CODEC>
__device__ __forceinline__ void lq_request(const char *p, unsigned &w0, unsigned &w1) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if constexpr (CODEC == 16) {
        const lq_u32x2 v = *reinterpret_cast<const __attribute__((address_space(1))) lq_u32x2 *>(a);
        w0 = v.x; w1 = v.y;
    } else if constexpr (CODEC == 8) {
        w0 = *reinterpret_cast<const __attribute__((address_space(1))) unsigned *>(a);
    } else {
        w0 = *reinterpret_cast<const __attribute__((address_space(1))) unsigned short *>(a);   // byte0 | byte1 << 8
    }
}

// (at least four waves per SIMD: the reference's benchmark shape is 4 096 wave items, four per SIMD of the part -- one round)
template <int CODEC, int LPR, int K>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) bag_sum_long_q_kernel(const LongQArgs args) {
    static_assert(K % kLqSub == 0 && K == lq_chunk(CODEC, LPR), "K is lq_chunk's");
    constexpr int G = 64 / LPR;                      // bags per wave
    constexpr int PB = RowPiece<CODEC>::kBytes;      // bytes per piece: 8 / 4 / 2
    constexpr int row_bytes = LPR * PB;
    constexpr int NIL = (K + LPR - 1) / LPR;         // index loads per lane and chunk
    __shared__ float s_lut[CodecLut<CODEC>::kEntries];
    codec_lut_init<CODEC>(s_lut);
    __syncthreads();                                 // (every wave of the block is here before any of them leaves)
    const int lane = threadIdx.x & 63;
    const int g = lane / LPR, piece = lane - g * LPR;
    const bool lane_on = g < G;
    const int B = args.B;
    const int64_t cpt = (B + G - 1) / G;             // wave items per table
    const int64_t item = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= cpt * args.T) return;                // wave-uniform
    const int t = __builtin_amdgcn_readfirstlane((int)(item / cpt));
    const int64_t b = (item - (int64_t)t * cpt) * G + g;
    const char *__restrict__ W = reinterpret_cast<const char *>(args.table[t]);
    const int64_t *__restrict__ idx = args.indices[t];
    const int64_t *__restrict__ off = args.offsets[t];
    const int n_rows = args.n_rows[t], nnz = args.nnz[t];
    const char *zeros = reinterpret_cast<const char *>(args.zeros) + piece * PB;
    bool bad = false;
    int64_t st = 0;
    int len = 0;
    if (lane_on && b < B) {
        const int64_t s0 = off[b], e0 = (b + 1 < B) ? off[b + 1] : (int64_t)nnz;
        if (s0 >= 0 && e0 >= s0 && e0 <= nnz && e0 - s0 < (1ll << 30)) { st = s0; len = (int)(e0 - s0); }   // (pos + K stays an int)
        else bad = true;
    }
    int maxlen = len;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(maxlen, m, 64); maxlen = o > maxlen ? o : maxlen; }
    maxlen = __builtin_amdgcn_readfirstlane(maxlen);
    // Index e of this lane's bag: the load alone stands under the branch (no load for a position behind the bag's end), the value is
    // looked at a chunk later -- the wait for it stands in front of row_id, not behind the load.
    auto want = [&](int e, int slot) -> bool { return slot < K && e < len; };
    auto request_index = [&](int e, bool w) -> int64_t {
        int64_t v = 0;
        if (w) v = *reinterpret_cast<const __attribute__((address_space(1))) int64_t *>(reinterpret_cast<uintptr_t>(idx + (st + e)));
        return v;
    };
    // the row id of a loaded index (-1: nothing to add)
    auto row_id = [&](int64_t v, bool w) -> int {
        const bool ok = v >= 0 && v < n_rows;
        bad = bad || (w && !ok);
        return (w && ok) ? (int)v : -1;
    };
    int cur[NIL];
    int64_t nxt[NIL];
#pragma unroll
    for (int i = 0; i < NIL; i++) nxt[i] = request_index(piece + LPR * i, want(piece + LPR * i, piece + LPR * i));
#pragma unroll
    for (int i = 0; i < NIL; i++) cur[i] = row_id(nxt[i], want(piece + LPR * i, piece + LPR * i));
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int gbase = g * LPR;
    const char *Wp = W + piece * PB;
    for (int pos = 0; pos < maxlen; pos += K) {
#pragma unroll
        for (int i = 0; i < NIL; i++)   // the next chunk's indices: on the wire under this chunk's rows
            nxt[i] = request_index(pos + K + piece + LPR * i, want(pos + K + piece + LPR * i, piece + LPR * i));
        const int live = maxlen - pos;               // wave-uniform: the slots of this chunk that some bag of the wave still has
        unsigned w0[K], w1[K];
#pragma unroll
        for (int s = 0; s < K; s += kLqSub) {
            if (s < live) {
                int r[kLqSub];
#pragma unroll
                for (int j = 0; j < kLqSub; j++) r[j] = __shfl(cur[(s + j) / LPR], gbase + ((s + j) % LPR), 64);
                __builtin_amdgcn_sched_barrier(0);   // the eight hand-overs back to back, one wait, then the eight requests
#pragma unroll
                for (int j = 0; j < kLqSub; j++) {
                    const bool there = lane_on && r[j] >= 0;   // (d = 36: lane 63 has no group and no bag)
                    w1[s + j] = 0u;
                    lq_request<CODEC>(there ? Wp + (int64_t)r[j] * row_bytes : zeros, w0[s + j], w1[s + j]);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);           // every request of the chunk is out before the first decode
#pragma unroll
        for (int s = 0; s < K; s += kLqSub) {
            if (s < live) {
#pragma unroll
                for (int j = s; j < s + kLqSub; j++) {   // index order, unfused fp32 adds
                    const float4 x = dec_chunk<CODEC>(w0[j], w1[j], s_lut);
                    acc.x = __fadd_rn(acc.x, x.x); acc.y = __fadd_rn(acc.y, x.y);
                    acc.z = __fadd_rn(acc.z, x.z); acc.w = __fadd_rn(acc.w, x.w);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NIL; i++) cur[i] = row_id(nxt[i], want(pos + K + piece + LPR * i, piece + LPR * i));
    }
    if (lane_on && b < B)
        *reinterpret_cast<float4 *>(args.out + (int64_t)t * args.out_tstride + b * args.out_bstride + piece * 4) = acc;
    if (bad) atomicOr(args.err, 1);
}

// the dispatch record (evs_long_q_kernels_seen): id = codec (16, 8, 4) * 5 + lpr (4, 8, 9, 16, 32)
constexpr int kLongQCount = 15;
static std::atomic<long long> g_longq_seen[kLongQCount];

template <int CODEC, int LPR>
static void launch_long_q(const LongQArgs &a, hipStream_t st) {
    constexpr int G = 64 / LPR;
    const int64_t items = (int64_t)a.T * (((int64_t)a.B + G - 1) / G);   // (the entry has checked that the grid holds them)
    hipLaunchKernelGGL((bag_sum_long_q_kernel<CODEC, LPR, lq_chunk(CODEC, LPR)>), dim3((unsigned)((items + 3) / 4)), dim3(256), 0, st, a);
    g_longq_seen[lq_codec_id(CODEC) * 5 + lq_lpr_id(LPR)].fetch_add(1, std::memory_order_relaxed);
}

template <int CODEC>
static void launch_long_q_codec(const LongQArgs &a, int lpr, hipStream_t st) {
    switch (lpr) {
    case 4: launch_long_q<CODEC, 4>(a, st); break;
    case 8: launch_long_q<CODEC, 8>(a, st); break;
    case 9: launch_long_q<CODEC, 9>(a, st); break;
    case 16: launch_long_q<CODEC, 16>(a, st); break;
    default: launch_long_q<CODEC, 32>(a, st); break;
    }
}

}  // namespace evs

extern "C" int evs_long_q_chunk(int codec, int d) {
    if (evs::lq_codec_id(codec) < 0 || d <= 0 || d % 4 != 0 || evs::lq_lpr_id(d / 4) < 0) return 0;
    return evs::lq_chunk(codec, d / 4);
}

extern "C" int evs_long_q_kernels_seen(char *buf, int n) {
    int len = 0;
    if (buf && n > 0) buf[0] = 0;
    for (int id = 0; id < evs::kLongQCount; id++) {
        char line[64];
        const int k = snprintf(line, sizeof line, "longq_c%d_lpr%d=%lld\n", evs::kLqCodec[id / 5], evs::kLqLpr[id % 5],
                               evs::g_longq_seen[id].load(std::memory_order_relaxed));
        if (buf && len + k < n) memcpy(buf + len, line, (size_t)k + 1);
        len += k;
    }
    return len;
}

extern "C" int evs_embedding_bag_sum_long(int T, int64_t B, int d, int codec, const void *const *tables, const int64_t *n_rows,
                                          const int64_t *const *indices, const int64_t *const *offsets, const int64_t *nnz,
                                          float *out, int64_t out_table_stride, int64_t out_bag_stride, void *stream) {
    using namespace evs;
    const char *who = "evs_embedding_bag_sum_long";
    EVS_REQUIRE(T >= 0 && B >= 0, "%s: bad shape T=%d B=%lld", who, T, (long long)B);
    EVS_REQUIRE(lq_codec_id(codec) >= 0, "%s: codec %d (encoded tables only: 16, 8, 4)", who, codec);
    EVS_REQUIRE(d == 16 || d == 32 || d == 36 || d == 64 || d == 128, "%s: no kernel for d=%d (16, 32, 36, 64, 128)", who, d);
    if (T == 0 || B == 0) return EVS_OK;
    EVS_REQUIRE(tables && n_rows && indices && offsets && nnz && out, "%s: NULL argument", who);
    EVS_REQUIRE(B < (1ll << 31), "%s: B %lld (below 2^31)", who, (long long)B);
    EVS_REQUIRE(reinterpret_cast<uintptr_t>(out) % 16 == 0, "%s: out is not 16-byte aligned", who);
    EVS_REQUIRE(out_table_stride % 4 == 0 && out_bag_stride % 4 == 0, "%s: strides %lld / %lld are not multiples of 4", who,
                (long long)out_table_stride, (long long)out_bag_stride);
    for (int k = 0; k < T; k++) {
        EVS_REQUIRE(offsets[k], "%s: offsets[%d] is NULL", who, k);
        EVS_REQUIRE(n_rows[k] >= 0 && nnz[k] >= 0, "%s: table %d has negative size", who, k);
        EVS_REQUIRE(n_rows[k] < (1ll << 31) && nnz[k] < (1ll << 31), "%s: table %d: n_rows %lld, nnz %lld (below 2^31)", who, k,
                    (long long)n_rows[k], (long long)nnz[k]);
        EVS_REQUIRE(tables[k] || n_rows[k] == 0, "%s: table %d is NULL", who, k);
        EVS_REQUIRE(reinterpret_cast<uintptr_t>(tables[k]) % 16 == 0, "%s: table %d is not 16-byte aligned", who, k);
        EVS_REQUIRE(indices[k] || nnz[k] == 0, "%s: indices[%d] is NULL", who, k);
    }
    const int G = 64 / (d / 4);
    const int64_t per_launch = (int64_t)(T < EVS_MAX_TABLES_PER_LAUNCH ? T : EVS_MAX_TABLES_PER_LAUNCH) * ((B + G - 1) / G);
    EVS_REQUIRE((per_launch + 3) / 4 < (1ll << 31), "%s: T=%d x B=%lld bags are more wave items than one grid holds", who, T, (long long)B);
    int *err = index_error_flag();
    const void *zp = zero_code_page(codec);
    if (!err || !zp) return EVS_EHIP;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (int k0 = 0; k0 < T; k0 += EVS_MAX_TABLES_PER_LAUNCH) {
        const int n = (T - k0 < EVS_MAX_TABLES_PER_LAUNCH) ? T - k0 : EVS_MAX_TABLES_PER_LAUNCH;
        LongQArgs a;
        for (int k = 0; k < EVS_MAX_TABLES_PER_LAUNCH; k++) {
            const bool on = k < n;
            a.table[k] = on ? tables[k0 + k] : nullptr;
            a.indices[k] = on ? indices[k0 + k] : nullptr;
            a.offsets[k] = on ? offsets[k0 + k] : nullptr;
            a.n_rows[k] = on ? (int)n_rows[k0 + k] : 0;
            a.nnz[k] = on ? (int)nnz[k0 + k] : 0;
        }
        a.out = out + (int64_t)k0 * out_table_stride;
        a.out_tstride = out_table_stride;
        a.out_bstride = out_bag_stride;
        a.B = (int)B;
        a.T = n;
        a.err = err;
        a.zeros = zp;
        switch (codec) {
        case 16: launch_long_q_codec<16>(a, d / 4, st); break;
        case 8: launch_long_q_codec<8>(a, d / 4, st); break;
        default: launch_long_q_codec<4>(a, d / 4, st); break;
        }
        EVS_HIP_CHECK(hipGetLastError());
    }
    return EVS_OK;
}
