// Online row updates (gfx950): a delta of (table, row) -> new fp32 vector is encoded in the table's codec and stored at its
// row -- and, through a cache's look-up, into the arena row that holds a copy of it.  Shared by evs_update.hip (tables only:
// NoLookup) and evs_cache.hip (the cache tiers: CacheLookup, next to struct evs_cache).
//
// Kernel shape.  One group of 16 lanes per key (four keys per wave, sixteen per block), one row piece per lane: the pieces
// are the PIECES / U / TAIL row shapes the cache's insert kernels copy rows with (evs_cache.hip: sa_insert_one,
// sampled_insert_one) -- d = 36: fp32 nine 16-byte pieces, u16 4 x 16 + 8, u8 2 x 16 + 4, u4 16 + 2 (a u4 row is only 2-byte
// aligned: the same unaligned vector accesses those kernels make).  EVERY lane of a group performs the look-up: the sixteen
// lanes ask for the same words, one line request, and there is no cross-lane hand-off; the group then stores the table row
// and the arena row from the same registers.  Plain vector stores (non-temporal stores ran at half the rate for scattered
// rows: tools/store_pattern_probe.hip).  Residents are counted with a ballot per wave and one atomic per block.
// The look-up only reads: no way word, hash word, priority, list link, stamp or counter of the policy changes.
#pragma once
#include "evs_common.h"
#include "evs_encode.h"
#include "evs_hash.h"

namespace evs {

constexpr int kUpdGroup = 16;                   // lanes per key
constexpr int kUpdKeysPerBlock = 256 / kUpdGroup;

struct NoLookup {                               // a table without a cache in front of it
    static constexpr bool kHas = false;
    unsigned char *arena = nullptr;
    __device__ __forceinline__ unsigned row_base(int) const { return 0u; }
    __device__ __forceinline__ long long find(int, unsigned, const unsigned *) const { return -1; }
};

template <typename LK>
struct RowUpdateArgs {
    const int *keys;                 // (n, 2): table 0-based, row
    const float *values;             // row i at values + i * values_stride (update only)
    long long values_stride, n;
    int n_tables, row_bytes, d, values_aligned;   // values_aligned: base 16-byte aligned and stride % 4 == 0
    unsigned char *tables[kMaxTables];
    long long n_rows[kMaxTables];
    unsigned long long *n_resident;  // may be NULL
    int *err;                        // the sticky index-error flag
    LK lk;
};

// the row shape of a row size: PIECES pieces of UB bytes and a tail of TB bytes (0: none); PIECES = 0: no compiled shape,
// the lanes walk the row's code units
template <int RB> struct RowShape { static constexpr int P = 0, UB = 16, TB = 0; };
template <> struct RowShape<144> { static constexpr int P = 9, UB = 16, TB = 0; };    // d = 36 fp32
template <> struct RowShape<256> { static constexpr int P = 16, UB = 16, TB = 0; };   // d = 64 fp32
template <> struct RowShape<128> { static constexpr int P = 8, UB = 16, TB = 0; };
template <> struct RowShape<64> { static constexpr int P = 4, UB = 16, TB = 0; };
template <> struct RowShape<32> { static constexpr int P = 2, UB = 16, TB = 0; };
template <> struct RowShape<16> { static constexpr int P = 1, UB = 16, TB = 0; };
template <> struct RowShape<72> { static constexpr int P = 4, UB = 16, TB = 8; };     // d = 36 u16: 4 x 16 + 8
template <> struct RowShape<36> { static constexpr int P = 2, UB = 16, TB = 4; };     // d = 36 u8: 2 x 16 + 4
template <> struct RowShape<18> { static constexpr int P = 1, UB = 16, TB = 2; };     // d = 36 u4: 16 + 2
template <> struct RowShape<8> { static constexpr int P = 1, UB = 8, TB = 0; };

typedef unsigned upd_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned upd_u32x2 __attribute__((ext_vector_type(2)));
typedef float upd_f32x4 __attribute__((ext_vector_type(4)));

template <int NB>
__device__ __forceinline__ void upd_store(unsigned char *p, const unsigned (&w)[4]) {
    if constexpr (NB == 16) { upd_u32x4 v; v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3]; *reinterpret_cast<upd_u32x4 *>(p) = v; }
    else if constexpr (NB == 8) { upd_u32x2 v; v.x = w[0]; v.y = w[1]; *reinterpret_cast<upd_u32x2 *>(p) = v; }
    else if constexpr (NB == 4) *reinterpret_cast<unsigned *>(p) = w[0];
    else *reinterpret_cast<unsigned short *>(p) = (unsigned short)w[0];
}
template <int NB>
__device__ __forceinline__ void upd_load(const unsigned char *p, unsigned (&w)[4]) {
    if constexpr (NB == 16) { const upd_u32x4 v = *reinterpret_cast<const upd_u32x4 *>(p); w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
    else if constexpr (NB == 8) { const upd_u32x2 v = *reinterpret_cast<const upd_u32x2 *>(p); w[0] = v.x; w[1] = v.y; }
    else if constexpr (NB == 4) w[0] = *reinterpret_cast<const unsigned *>(p);
    else w[0] = *reinterpret_cast<const unsigned short *>(p);
}

// one code of CODEC bits from one fp32 value: the bits themselves (fp32), or evs_encode.h's encoders on the widened value
template <int CODEC>
__device__ __forceinline__ unsigned upd_code(float f) {
    if constexpr (CODEC == 32) return __float_as_uint(f);
    else if constexpr (CODEC == 16) return (unsigned)(unsigned short)enc_u16((double)f);
    else if constexpr (CODEC == 8) return (unsigned)(unsigned char)enc_u8((double)f);
    else return (unsigned)enc_u4((double)f) & 15u;
}
// NB bytes of an encoded row from the NB * 8 / CODEC values at v (u4: element 2j in the HIGH nibble of byte j)
template <int CODEC, int NB>
__device__ __forceinline__ void upd_encode(const float *v, bool aligned, unsigned (&w)[4]) {
    constexpr int NE = NB * 8 / CODEC;
    w[0] = w[1] = w[2] = w[3] = 0u;
    if constexpr (NE > 0) {
        float f[NE];
        if (NE % 4 == 0 && aligned) {
#pragma unroll
            for (int k = 0; k < NE / 4; k++) {
                const upd_f32x4 q = reinterpret_cast<const upd_f32x4 *>(v)[k];
                f[4 * k] = q.x; f[(4 * k + 1) % NE] = q.y; f[(4 * k + 2) % NE] = q.z; f[(4 * k + 3) % NE] = q.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NE; k++) f[k] = v[k];
        }
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const unsigned c = upd_code<CODEC>(f[e]);
            if constexpr (CODEC == 32) w[e] = c;
            else if constexpr (CODEC == 16) w[e >> 1] |= c << ((e & 1) * 16);
            else if constexpr (CODEC == 8) w[e >> 2] |= c << ((e & 3) * 8);
            else w[e >> 3] |= c << (((e >> 1) & 3) * 8 + ((e & 1) ? 0 : 4));
        }
    }
}

// the key of group `g` of this block -> table / row, range-checked (a key out of range is skipped and flagged)
template <typename LK>
__device__ __forceinline__ bool upd_key(const RowUpdateArgs<LK> &args, long long i, int lane, const long long *s_rows, int &t, unsigned &row) {
    if (i >= args.n) return false;
    const upd_u32x2 k = reinterpret_cast<const upd_u32x2 *>(args.keys)[i];
    t = (int)k.x;
    const int r = (int)k.y;
    if ((unsigned)t >= (unsigned)args.n_tables || r < 0 || (long long)r >= s_rows[t]) {
        if (lane == 0) atomicOr(args.err, 1);
        return false;
    }
    row = (unsigned)r;
    return true;
}
// per block: the table bases, row counts and the look-up's key universe into LDS (a per-lane index into the kernel arguments
// would be a vector-memory round trip in front of every access)
template <typename LK>
__device__ __forceinline__ void upd_stage(const RowUpdateArgs<LK> &args, unsigned char **s_tab, long long *s_rows, unsigned *s_base) {
    for (int i = threadIdx.x; i < kMaxTables; i += blockDim.x) { s_tab[i] = args.tables[i]; s_rows[i] = args.n_rows[i]; }
    if (threadIdx.x < 32) s_base[threadIdx.x] = args.lk.row_base((int)threadIdx.x);
    __syncthreads();
}
__device__ __forceinline__ void upd_count(bool resident_leader, unsigned long long *n_resident, int *s_cnt) {
    const unsigned long long m = __ballot(resident_leader);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0 && n_resident) {
        const int tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (tot) atomicAdd(n_resident, (unsigned long long)tot);
    }
}

// encode + table row (+ arena row when the key is resident)
template <int CODEC, int PIECES, int UB, int TB, typename LK>
__global__ void __launch_bounds__(256) row_update_kernel(const RowUpdateArgs<LK> args) {
    __shared__ unsigned char *s_tab[kMaxTables];
    __shared__ long long s_rows[kMaxTables];
    __shared__ unsigned s_base[32];
    __shared__ int s_cnt[4];
    upd_stage(args, s_tab, s_rows, s_base);
    const int lane = threadIdx.x & (kUpdGroup - 1);
    const long long i = (long long)blockIdx.x * kUpdKeysPerBlock + (threadIdx.x / kUpdGroup);
    int t = 0;
    unsigned row = 0;
    bool resident = false;
    if (upd_key(args, i, lane, s_rows, t, row)) {
        const long long e = args.lk.find(t, row, s_base);
        resident = e >= 0;
        unsigned char *trow = s_tab[t] + (long long)row * args.row_bytes;
        unsigned char *arow = LK::kHas && resident ? args.lk.arena + e * args.row_bytes : nullptr;
        const float *v = args.values + i * args.values_stride;
        const bool al = args.values_aligned != 0;
        unsigned w[4];
        if constexpr (PIECES > 0) {
            constexpr int NE = UB * 8 / CODEC;   // values per piece
            if (lane < PIECES) {
                upd_encode<CODEC, UB>(v + lane * NE, al, w);
                upd_store<UB>(trow + lane * UB, w);
                if (LK::kHas && arow) upd_store<UB>(arow + lane * UB, w);
            } else if (TB > 0 && lane == PIECES) {
                upd_encode<CODEC, (TB > 0 ? TB : 2)>(v + PIECES * NE, al, w);
                upd_store<(TB > 0 ? TB : 2)>(trow + PIECES * UB, w);
                if (LK::kHas && arow) upd_store<(TB > 0 ? TB : 2)>(arow + PIECES * UB, w);
            }
        } else {
            // no compiled shape for this row size: the lanes walk the row's code units (fp32: a word, u16: a code, u8 / u4: a byte)
            constexpr int NB = CODEC == 32 ? 4 : CODEC == 16 ? 2 : 1;
            constexpr int NE = CODEC == 4 ? 2 : 1;
            const int n_units = args.row_bytes / NB;
            for (int u = lane; u < n_units; u += kUpdGroup) {
                unsigned c;
                if constexpr (CODEC == 4) c = (upd_code<4>(v[2 * u]) << 4) | upd_code<4>(v[2 * u + 1]);
                else c = upd_code<CODEC>(v[u * NE]);
                if constexpr (NB == 4) { *reinterpret_cast<unsigned *>(trow + 4 * u) = c; if (LK::kHas && arow) *reinterpret_cast<unsigned *>(arow + 4 * u) = c; }
                else if constexpr (NB == 2) { *reinterpret_cast<unsigned short *>(trow + 2 * u) = (unsigned short)c; if (LK::kHas && arow) *reinterpret_cast<unsigned short *>(arow + 2 * u) = (unsigned short)c; }
                else { trow[u] = (unsigned char)c; if (LK::kHas && arow) arow[u] = (unsigned char)c; }
            }
        }
    }
    upd_count(resident && lane == 0, args.n_resident, s_cnt);
}

// the arena row of every resident key re-copied from its backing row (the caller wrote the table itself)
template <int PIECES, int UB, int TB, typename LK>
__global__ void __launch_bounds__(256) row_refresh_kernel(const RowUpdateArgs<LK> args) {
    __shared__ unsigned char *s_tab[kMaxTables];
    __shared__ long long s_rows[kMaxTables];
    __shared__ unsigned s_base[32];
    __shared__ int s_cnt[4];
    upd_stage(args, s_tab, s_rows, s_base);
    const int lane = threadIdx.x & (kUpdGroup - 1);
    const long long i = (long long)blockIdx.x * kUpdKeysPerBlock + (threadIdx.x / kUpdGroup);
    int t = 0;
    unsigned row = 0;
    bool resident = false;
    if (upd_key(args, i, lane, s_rows, t, row)) {
        const long long e = args.lk.find(t, row, s_base);
        resident = e >= 0;
        if (resident) {
            const unsigned char *trow = s_tab[t] + (long long)row * args.row_bytes;
            unsigned char *arow = args.lk.arena + e * args.row_bytes;
            unsigned w[4];
            if constexpr (PIECES > 0) {
                if (lane < PIECES) { upd_load<UB>(trow + lane * UB, w); upd_store<UB>(arow + lane * UB, w); }
                else if (TB > 0 && lane == PIECES) { upd_load<(TB > 0 ? TB : 2)>(trow + PIECES * UB, w); upd_store<(TB > 0 ? TB : 2)>(arow + PIECES * UB, w); }
            } else {
                for (int u = lane; u < args.row_bytes; u += kUpdGroup) arow[u] = trow[u];
            }
        }
    }
    upd_count(resident && lane == 0, args.n_resident, s_cnt);
}

inline dim3 upd_grid(long long n) { return dim3((unsigned)((n + kUpdKeysPerBlock - 1) / kUpdKeysPerBlock)); }

// compiled shapes: the rows of d = 16 / 32 / 36 / 64 in the codec; every other row size takes the unit walk
template <int CODEC, int D, typename LK>
static void launch_row_update_d(const RowUpdateArgs<LK> &a, hipStream_t st) {
    using S = RowShape<D * CODEC / 8>;
    hipLaunchKernelGGL((row_update_kernel<CODEC, S::P, S::UB, S::TB, LK>), upd_grid(a.n), dim3(256), 0, st, a);
}
template <int CODEC, typename LK>
static void launch_row_update_c(const RowUpdateArgs<LK> &a, hipStream_t st) {
    switch (a.d) {
    case 36: launch_row_update_d<CODEC, 36, LK>(a, st); break;
    case 16: launch_row_update_d<CODEC, 16, LK>(a, st); break;
    case 32: launch_row_update_d<CODEC, 32, LK>(a, st); break;
    case 64: launch_row_update_d<CODEC, 64, LK>(a, st); break;
    default: hipLaunchKernelGGL((row_update_kernel<CODEC, 0, 16, 0, LK>), upd_grid(a.n), dim3(256), 0, st, a); break;
    }
}
template <typename LK>
static void launch_row_update(int codec, const RowUpdateArgs<LK> &a, hipStream_t st) {
    if (codec == 32) launch_row_update_c<32, LK>(a, st);
    else if (codec == 16) launch_row_update_c<16, LK>(a, st);
    else if (codec == 8) launch_row_update_c<8, LK>(a, st);
    else launch_row_update_c<4, LK>(a, st);
}
template <int RB, typename LK>
static void launch_row_refresh_rb(const RowUpdateArgs<LK> &a, hipStream_t st) {
    using S = RowShape<RB>;
    hipLaunchKernelGGL((row_refresh_kernel<S::P, S::UB, S::TB, LK>), upd_grid(a.n), dim3(256), 0, st, a);
}
template <typename LK>
static void launch_row_refresh(const RowUpdateArgs<LK> &a, hipStream_t st) {
    switch (a.row_bytes) {
    case 144: launch_row_refresh_rb<144, LK>(a, st); break;
    case 256: launch_row_refresh_rb<256, LK>(a, st); break;
    case 128: launch_row_refresh_rb<128, LK>(a, st); break;
    case 64: launch_row_refresh_rb<64, LK>(a, st); break;
    case 32: launch_row_refresh_rb<32, LK>(a, st); break;
    case 16: launch_row_refresh_rb<16, LK>(a, st); break;
    case 72: launch_row_refresh_rb<72, LK>(a, st); break;
    case 36: launch_row_refresh_rb<36, LK>(a, st); break;
    case 18: launch_row_refresh_rb<18, LK>(a, st); break;
    case 8: launch_row_refresh_rb<8, LK>(a, st); break;
    default: launch_row_refresh_rb<1, LK>(a, st); break;
    }
}

// argument checks the four entry points share (before the device is touched); 1: nothing to do
inline int upd_check_common(const char *who, int64_t n, const void *keys) {
    EVS_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
    if (n == 0) return 1;
    EVS_REQUIRE(n < (1ll << 31), "%s: at most 2^31 - 1 keys per call", who);
    EVS_REQUIRE(keys, "%s: NULL keys", who);
    return 0;
}

}  // namespace evs
