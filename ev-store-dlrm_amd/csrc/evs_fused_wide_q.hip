// Wide models over encoded tables: gather + interaction for 33 <= F <= 128 features, u16 / u8 / u4 rows, in one launch.
//   evs_emb_interact_wide_q_stacked   x (fp32) + T encoded tables behind one stacked (T, B) index tensor, one index per bag
//
// What it keeps of the fp32 unit (evs_fused_wide.hip, whose header explains them): a block of 256 threads owns 16 samples, a wave
// takes four of them one at a time; the index tile goes through LDS, 17 entries per table; tables and row counts travel in the
// kernel arguments; lane (r16, q) holds KS = d / 4 elements of row 16 t + r16; every tile (ti, tj <= ti) is a chain of KS
// v_mfma_f32_16x16x4_f32 between two fp32 register sets; R leaves by bands through the wave's LDS band buffer.
// What is its own:
//   * a row is requested as RAW CODES and decoded after it has arrived.  A lane's piece of an encoded row is the CQ = d / 16 chunks
//     at chunk q CQ -- CQ x 8 / 4 / 2 contiguous bytes -- and, for d = 36, its own element q of the last chunk as one 2-byte or
//     1-byte load: NT (MW + 1) registers per sample in flight (MW = the piece in dwords, at least one) instead of the NT KS of fp32
//     rows.  So EVERY instantiation requests the next sample's codes under this sample's MFMAs, d = 64 at NT = 8 included, and u8 /
//     u4 request two samples ahead where the registers allow it (kDepth, a compile-time constant chosen from the register reports)
//   * a sample is decoded ONCE into a[NT][KS] with evs_common.h's decoders (bit-exact with the reference's): the table of
//     codec_lut_init sits in LDS, filled behind the barrier that the index tile needs anyway; u16 takes the packed main-range
//     form (dec_u16_main2) for a whole row-tile when no lane of the wave holds a tail code in it (one ballot per row-tile)
//   * unaligned rows: encoded rows of d = 36 are 72 / 36 / 18 bytes, so a piece starts on an 8- / 4- / 2-byte boundary.  The
//     pieces are loaded with exactly their own bytes, typed with the alignment they have (global loads; gfx950 takes unaligned
//     dword addresses in the global address space), never an aligned window around them: nothing outside a row is read, so the
//     last row of a table needs no path of its own
//   * x stays fp32: it is row 0 of tile 0, its lanes (0, q) load floats beside the codes and put them over the decoded zero row
//   * an out-of-range index or a row past F reads zero_code_page(CODEC), which decodes to exactly 0.0f
// Static LDS at NT = 8: bands 30.2 KB + index tile 16.9 KB + addresses 2 KB + table up to 2.1 KB = 51.2 KB.
// Templates: codec {16, 8, 4} x d {16, 32, 36, 64} x NT {3, 4, 6, 8}.  fp32 chains only (the integer pipe of evs_fused_rfq.hip's
// u8 path has an error term of its own and is not used here).
#include "evs_fused_wide.h"
#include <string.h>
#include <atomic>

namespace evs {

typedef unsigned wq_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned wq_u32x4 __attribute__((ext_vector_type(4)));

// BYTES raw bytes at p, which is ALIGN-aligned, from the global address space (not flat: evs_fused_wide.hip's request says why)
template <class V, int A>
struct GlobalAs { typedef __attribute__((address_space(1), aligned(A))) V type; };
template <int BYTES, int ALIGN>
__device__ __forceinline__ void load_codes(const char *p, unsigned (&w)[BYTES >= 4 ? BYTES / 4 : 1]) {
    typedef typename GlobalAs<wq_u32x4, (ALIGN < 16 ? ALIGN : 16)>::type g4;
    typedef typename GlobalAs<wq_u32x2, (ALIGN < 8 ? ALIGN : 8)>::type g2;
    typedef typename GlobalAs<unsigned, (ALIGN < 4 ? ALIGN : 4)>::type g1;
    typedef __attribute__((address_space(1))) unsigned short gh;
    if constexpr (BYTES == 32) {
        const wq_u32x4 u = ((const g4 *)p)[0], v = ((const g4 *)p)[1];
        w[0] = u[0]; w[1] = u[1]; w[2] = u[2]; w[3] = u[3]; w[4] = v[0]; w[5] = v[1]; w[6] = v[2]; w[7] = v[3];
    } else if constexpr (BYTES == 16) {
        const wq_u32x4 v = *(const g4 *)p;
        w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
    } else if constexpr (BYTES == 8) {
        const wq_u32x2 v = *(const g2 *)p;
        w[0] = v[0]; w[1] = v[1];
    } else if constexpr (BYTES == 4) {
        w[0] = *(const g1 *)p;
    } else {
        static_assert(BYTES == 2, "pieces of 32, 16, 8, 4 or 2 bytes");
        w[0] = *(const gh *)p;
    }
}

template <int CODEC, int D, int NT>
__global__ void __launch_bounds__(256) interact_wide_q_kernel(const WideArgs args) {
    constexpr int KS = D / 4, CQ = D / 16;
    constexpr bool REM = (D % 16) != 0;          // d = 36: a last chunk shared by the four k-slots, element q each
    static_assert(D % 4 == 0 && (D % 16 == 0 || D % 16 == 4), "KS = 4 CQ (+ 1)");
    static_assert(CODEC == 16 || CODEC == 8 || CODEC == 4, "encoded rows");
    constexpr int CB = CODEC / 2;                // bytes of a chunk of 4 elements
    constexpr int MB = CQ * CB;                  // a lane's piece
    constexpr int MW = MB >= 4 ? MB / 4 : 1;
    constexpr int RW = MW + (REM ? 1 : 0);       // registers of a row-tile in flight
    constexpr int ROWB = D * CODEC / 8;
    constexpr int ALIGN = REM ? CB : (MB < 16 ? MB : 16);   // rows of 72 / 36 / 18 bytes start on chunk boundaries only
    // samples requested ahead of the one in the MFMAs.  From the register reports: u16 at d = 64, NT = 8 takes 251 VGPRs with one
    // ahead (a second set of codes is 80 more), and u8 at d = 64, NT = 8 took 271 with two (one block per CU instead of two);
    // every other u8 / u4 form has the room
    constexpr int kDepth = (CODEC == 16 || (CODEC == 8 && NT * KS == 128)) ? 1 : 2;
    constexpr int ROWS = 16 * NT;
    constexpr int BAND = (256 * (NT - 1) + 136 + 3 + 3) / 4 * 4;   // as evs_fused_wide.hip
    static_assert(D + 136 + 6 <= BAND, "band 0 carries x");
    constexpr int IDXROW = 17;
    __shared__ int64_t s_idx[(ROWS - 1) * IDXROW];
    __shared__ const char *s_base[ROWS];
    __shared__ int64_t s_aux[ROWS];
    __shared__ __attribute__((aligned(16))) float s_band[4][BAND];
    __shared__ float s_lut[CodecLut<CODEC>::kEntries];

    const WideArgs *ka = (const WideArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    const int F = args.F, B = args.B, out_row = args.out_row;
    const int64_t blk_first = (int64_t)blockIdx.x * 16;

    if (tid < ROWS) {
        s_base[tid] = tid < F ? ka->base[tid] : nullptr;
        s_aux[tid] = tid < F ? ka->aux[tid] : 0;
    }
    {   // the index tile: 16 lanes take the 16 samples of one table, 16 tables per pass
        const int s = tid & 15;
        const int64_t b = blk_first + s;
        for (int t = tid >> 4; t < F - 1; t += 16) s_idx[t * IDXROW + s] = b < B ? args.idx[t * args.idx_stride + b] : 0;
    }
    codec_lut_init<CODEC>(s_lut);
    __syncthreads();

    float *band = s_band[wave];
    const float *lut = s_lut;
    bool bad = false;

    // the codes of sample `sib` of the block: RW registers per live row-tile, and x's floats in the lanes (0, q)
    auto request = [&](int sib, unsigned (&w)[NT][RW], float (&xv)[KS]) {
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (16 * t < F) {   // wave-uniform
                const int f = 16 * t + r16;
                const char *p = args.zeros;   // x's own lanes, rows past F, bad indices: the code of 0.0f
                if (f > 0 && f < F) {
                    const int64_t i = s_idx[(f - 1) * IDXROW + sib];
                    if ((uint64_t)i < (uint64_t)s_aux[f]) p = s_base[f] + i * (int64_t)ROWB;
                    else bad = true;   // a zero row, and the sticky flag
                }
                unsigned m[MW];
                load_codes<MB, ALIGN>(p + q * MB, m);
#pragma unroll
                for (int c = 0; c < MW; c++) w[t][c] = m[c];
                if constexpr (REM) {
                    const char *e = p + 4 * MB + ((q * CODEC) >> 3);
                    if constexpr (CODEC == 16) w[t][MW] = *(const __attribute__((address_space(1))) unsigned short *)e;
                    else w[t][MW] = *(const __attribute__((address_space(1))) unsigned char *)e;
                }
            }
        }
        if (r16 == 0) {
            const char *p = s_base[0] + (blk_first + sib) * s_aux[0];
#pragma unroll
            for (int c = 0; c < CQ; c++) {
                const f32x4 v = ((const global_f32x4 *)(p + q * (CQ * 16)))[c];
                xv[4 * c] = v.x; xv[4 * c + 1] = v.y; xv[4 * c + 2] = v.z; xv[4 * c + 3] = v.w;
            }
            if constexpr (REM) xv[4 * CQ] = *(const __attribute__((address_space(1))) float *)(p + 4 * CQ * 16 + 4 * q);
        }
    };

    // codes -> the fp32 operands, once per sample
    auto decode = [&](const unsigned (&w)[NT][RW], const float (&xv)[KS], float (&a)[NT][KS]) {
#pragma unroll
        for (int t = 0; t < NT; t++) {
            if (16 * t < F) {   // wave-uniform
                if constexpr (CODEC == 16) {
                    bool tail = false;
#pragma unroll
                    for (int c = 0; c < MW; c++) tail = tail || (w[t][c] & 0xffffu) > 65000u || (w[t][c] >> 16) > 65000u;
                    if constexpr (REM) tail = tail || w[t][MW] > 65000u;
                    if (__builtin_amdgcn_ballot_w64(tail) == 0ull) {   // no tail code in this row-tile, in any lane
#pragma unroll
                        for (int c = 0; c < MW; c++) {
                            const f32x2 v = dec_u16_main2(w[t][c]);
                            a[t][2 * c] = v[0]; a[t][2 * c + 1] = v[1];
                        }
                        if constexpr (REM) a[t][4 * CQ] = dec_u16_main(w[t][MW]);
                    } else {
#pragma unroll
                        for (int c = 0; c < MW; c++) {
                            a[t][2 * c] = dec_code<16>(w[t][c] & 0xffffu, lut);
                            a[t][2 * c + 1] = dec_code<16>(w[t][c] >> 16, lut);
                        }
                        if constexpr (REM) a[t][4 * CQ] = dec_code<16>(w[t][MW], lut);
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < CQ; c++) {
                        // u8: a chunk is one dword; u4: half of one (dec_chunk reads the low 16 bits)
                        const unsigned cw = CODEC == 8 ? w[t][c] : w[t][c / 2] >> (16 * (c & 1));
                        const float4 v = dec_chunk<CODEC>(cw, 0u, lut);
                        a[t][4 * c] = v.x; a[t][4 * c + 1] = v.y; a[t][4 * c + 2] = v.z; a[t][4 * c + 3] = v.w;
                    }
                    if constexpr (REM) {
                        if constexpr (CODEC == 8) a[t][4 * CQ] = lut[w[t][MW]];
                        else a[t][4 * CQ] = lut[(w[t][MW] >> ((q & 1) ? 0 : 4)) & 15u];   // element 2 j is the HIGH nibble of byte j
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < KS; s++) a[t][s] = 0.f;
            }
        }
        if (r16 == 0) {   // x over the decoded zeros of its lanes
#pragma unroll
            for (int s = 0; s < KS; s++) a[0][s] = xv[s];
        }
    };

    // T T^T of one sample from its registers, band by band, into R: evs_fused_wide.hip's consume, statement for statement
    auto consume = [&](int sib, const float (&a)[NT][KS]) {
        float *Rb = args.R + (blk_first + sib) * (int64_t)out_row;
#pragma unroll
        for (int ti = 0; ti < NT; ti++) {
            // (the empty statement keeps a band's offsets and masks inside the band: see the fp32 unit)
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
    const int64_t left = (int64_t)B - (blk_first + first);
    if (left > 0) {   // (wave-uniform; a tail block may leave whole waves without a sample)
        const int n = left < 4 ? (int)left : 4;
        unsigned w0[NT][RW], w1[kDepth == 2 ? NT : 1][RW];
        float x0[KS], x1[KS], a[NT][KS];
        request(first, w0, x0);
        if constexpr (kDepth == 2)
            if (n > 1) request(first + 1, w1, x1);
#pragma unroll 1
        for (int k = 0; k < n; k += kDepth) {
            decode(w0, x0, a);
            if (k + kDepth < n) request(first + k + kDepth, w0, x0);
            consume(first + k, a);
            if constexpr (kDepth == 2) {
                if (k + 1 >= n) break;
                decode(w1, x1, a);
                if (k + 3 < n) request(first + k + 3, w1, x1);
                consume(first + k + 1, a);
            }
        }
    }
    if (bad) atomicOr(args.err, 1);
}

// the dispatch record (evs_wide_q_kernels_seen): id = codec (16, 8, 4) * 16 + d (16, 32, 36, 64) * 4 + nt (3, 4, 6, 8)
constexpr int kWideQCount = 48;
constexpr int kWideQCodec[3] = {16, 8, 4};
static std::atomic<long long> g_wide_q_seen[kWideQCount];
constexpr int wide_q_codec_id(int codec) { return codec == 16 ? 0 : codec == 8 ? 1 : codec == 4 ? 2 : -1; }

template <int CODEC, int D>
static void launch_wide_q_d(const WideArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)(((int64_t)a.B + 15) / 16)), block(256);
    switch (wide_nt_id(a.F)) {
    case 0: hipLaunchKernelGGL((interact_wide_q_kernel<CODEC, D, 3>), grid, block, 0, st, a); break;
    case 1: hipLaunchKernelGGL((interact_wide_q_kernel<CODEC, D, 4>), grid, block, 0, st, a); break;
    case 2: hipLaunchKernelGGL((interact_wide_q_kernel<CODEC, D, 6>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((interact_wide_q_kernel<CODEC, D, 8>), grid, block, 0, st, a); break;
    }
}

template <int CODEC>
static void launch_wide_q_c(const WideArgs &a, int d, hipStream_t st) {
    switch (d) {
    case 16: launch_wide_q_d<CODEC, 16>(a, st); break;
    case 32: launch_wide_q_d<CODEC, 32>(a, st); break;
    case 36: launch_wide_q_d<CODEC, 36>(a, st); break;
    default: launch_wide_q_d<CODEC, 64>(a, st); break;
    }
}

}  // namespace evs

extern "C" int evs_wide_q_kernels_seen(char *buf, int n) {
    int len = 0;
    if (buf && n > 0) buf[0] = 0;
    for (int id = 0; id < evs::kWideQCount; id++) {
        char line[64];
        const int k = snprintf(line, sizeof line, "wideq_c%d_d%d_nt%d=%lld\n", evs::kWideQCodec[id / 16], evs::kWideD[(id % 16) / 4],
                               evs::kWideNt[id % 4], evs::g_wide_q_seen[id].load(std::memory_order_relaxed));
        if (buf && len + k < n) memcpy(buf + len, line, (size_t)k + 1);
        len += k;
    }
    return len;
}

extern "C" int evs_emb_interact_wide_q_stacked(int64_t B, int T, int d, int codec, const void *const *tables, const int64_t *n_rows,
                                               const float *x, int64_t x_stride, const int64_t *indices, int64_t idx_stride, int itself,
                                               float *R, void *stream) {
    using namespace evs;
    const char *who = "evs_emb_interact_wide_q_stacked";
    EVS_REQUIRE(T >= 0 && T < (1 << 30), "%s: bad shape T=%d", who, T);
    const int F = T + 1;
    if (int rc = wide_shape_ok(who, B, F, d)) return rc;
    EVS_REQUIRE(codec != 32, "%s: codec 32: fp32 tables go to evs_emb_interact_wide_stacked", who);
    EVS_REQUIRE(wide_q_codec_id(codec) >= 0, "%s: bad codec %d (16, 8, 4)", who, codec);
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
    for (int f = F; f < EVS_MAX_WIDE_FEATURES; f++) { a.base[f] = nullptr; a.aux[f] = 0; }
    a.idx = indices; a.idx_stride = idx_stride;
    a.R = R; a.B = (int)B; a.F = F; a.itself = itself ? 1 : 0;
    a.out_row = d + (a.itself ? F * (F + 1) / 2 : F * (F - 1) / 2);
    a.zeros = reinterpret_cast<const char *>(zero_code_page(codec));
    a.err = index_error_flag();
    if (!a.zeros || !a.err) return EVS_EHIP;
    const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (codec) {
    case 16: launch_wide_q_c<16>(a, d, st); break;
    case 8: launch_wide_q_c<8>(a, d, st); break;
    default: launch_wide_q_c<4>(a, d, st); break;
    }
    EVS_HIP_CHECK(hipGetLastError());
    g_wide_q_seen[wide_q_codec_id(codec) * 16 + wide_d_id(d) * 4 + wide_nt_id(F)].fetch_add(1, std::memory_order_relaxed);
    return EVS_OK;
}
