// Warm start of the batched set-associative tier (gfx950): the kernel that carries out a load plan (evs_cache_warm.h:
// warm_plan).  The host has decided every placement -- the entries arrive sorted by slot, every slot at most once, into a tier
// nothing else touches -- so the kernel makes no choice and needs no compare-and-swap and no atomic: per entry it copies the
// backing row into the arena row the slot owns (copy 0 of a two-copy arena) and stores the way word, all with plain stores
// (non-temporal ones ran at half rate on scattered patterns: README, round 4).
//
// A group of 16 lanes per entry, a 16-byte piece per lane (rows up to 256 bytes in one pass, longer ones in several) plus the
// tail type the insert kernels use for d = 36 (u16 rows 72 B: 8, u8 36 B: 4, u4 18 B: 2).  The table reads are random lines --
// latency, not bytes, is what there is to hide -- so every group keeps kWarmInFlight entries' loads in flight before it stores
// the first; the 16 groups of a block take 16 consecutive entries at a time, so the arena stores run forward through memory.
//
// The pair form (a C1 + C2 pair that shares its set records) is the same walk twice in one launch: the list holds C1's records
// and then C2's, the blocks are split between the tiers in proportion to their counts, each half is compiled for its tier's
// tail type, and a way word goes where the tier's geometry -- ways, word offset, sub-sets: by value -- puts its slot in the
// shared 128-byte record.
#include <type_traits>

#include "evs_cache_warm.h"

namespace evs {
namespace {

constexpr int kWarmLanes = 16;                   // lanes per entry
constexpr int kWarmGroups = 256 / kWarmLanes;    // entries a block takes side by side
constexpr int kWarmInFlight = 4;                 // entries per group whose loads go out together

struct NoTail {};
struct ByteTail {};   // any remainder: copied byte by byte
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <typename T> struct Native { using type = T; };
template <> struct Native<uint2> { typedef unsigned type __attribute__((ext_vector_type(2))); };
template <> struct Native<NoTail> { using type = int; };
template <> struct Native<ByteTail> { using type = unsigned char; };

template <typename TAIL>
__global__ void __launch_bounds__(256) cache_warm_load_kernel(const WarmArgs args) {
    using NT = typename Native<TAIL>::type;
    typedef const __attribute__((address_space(1))) f32x4 *gsrc_t;
    constexpr bool kHasTail = !std::is_same<TAIL, NoTail>::value && !std::is_same<TAIL, ByteTail>::value;
    const int lane = (int)threadIdx.x & (kWarmLanes - 1), group = (int)threadIdx.x / kWarmLanes;
    const int n16 = args.row_bytes >> 4;
    const long long chunk = (long long)kWarmGroups * kWarmInFlight;
    for (long long c0 = (long long)blockIdx.x * chunk; c0 < args.n; c0 += (long long)gridDim.x * chunk) {
        const unsigned char *src[kWarmInFlight];
        unsigned char *dst[kWarmInFlight];
        unsigned slot[kWarmInFlight], word[kWarmInFlight];
        bool ok[kWarmInFlight];
#pragma unroll
        for (int e = 0; e < kWarmInFlight; e++) {
            const long long i = c0 + (long long)e * kWarmGroups + group;
            ok[e] = i < args.n;
            const uint4 r = *reinterpret_cast<const uint4 *>(args.recs + (ok[e] ? i : 0));
            src[e] = reinterpret_cast<const unsigned char *>(((unsigned long long)r.y << 32) | r.x);
            slot[e] = r.z; word[e] = r.w;
            dst[e] = args.arena + ((unsigned long long)slot[e] << args.dual) * (unsigned long long)args.row_bytes;
        }
        NT t[kWarmInFlight] = {};
        if constexpr (kHasTail) {
            if (lane == (n16 & (kWarmLanes - 1))) {
#pragma unroll
                for (int e = 0; e < kWarmInFlight; e++) {
                    typedef const __attribute__((address_space(1))) NT *gtail_t;
                    if (ok[e]) t[e] = *reinterpret_cast<gtail_t>(reinterpret_cast<uintptr_t>(src[e] + n16 * 16));
                }
            }
        }
        for (int p = lane; p < n16; p += kWarmLanes) {
            f32x4 v[kWarmInFlight] = {};
#pragma unroll
            for (int e = 0; e < kWarmInFlight; e++)
                if (ok[e]) v[e] = reinterpret_cast<gsrc_t>(reinterpret_cast<uintptr_t>(src[e]))[p];
#pragma unroll
            for (int e = 0; e < kWarmInFlight; e++)
                if (ok[e]) reinterpret_cast<f32x4 *>(dst[e])[p] = v[e];
        }
        if constexpr (kHasTail) {
            if (lane == (n16 & (kWarmLanes - 1))) {
#pragma unroll
                for (int e = 0; e < kWarmInFlight; e++)
                    if (ok[e]) *reinterpret_cast<NT *>(dst[e] + n16 * 16) = t[e];
            }
        }
        if constexpr (std::is_same<TAIL, ByteTail>::value) {
#pragma unroll
            for (int e = 0; e < kWarmInFlight; e++)
                for (int b = n16 * 16 + lane; ok[e] && b < args.row_bytes; b += kWarmLanes) dst[e][b] = src[e][b];
        }
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < kWarmInFlight; e++)
                if (ok[e]) args.tags[slot[e]] = word[e];
        }
    }
}

template <typename TAIL>
void warm_launch_t(const WarmArgs &a, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((cache_warm_load_kernel<TAIL>), dim3(grid), dim3(256), 0, st, a);
}

// ---- the pair form: both tiers of a C1 + C2 pair that shares its set records, one launch --------------------------------------
// One tier's share of the launch: the `nb` blocks [b0, b0 + nb) walk the tier's n records exactly as the single form does -- 16
// lanes per entry, kWarmInFlight entries' loads out before the first store, 16 consecutive entries per block side by side --
// with the tier's tail type, and store each way word where the tier's geometry puts (effective set, way) in the shared record.
template <typename TAIL>
__device__ __forceinline__ void warm_pair_tier(const WarmRec *recs, const long long n, unsigned *tags, const WarmTier t,
                                               const unsigned block, const unsigned nb) {
    using NT = typename Native<TAIL>::type;
    typedef const __attribute__((address_space(1))) f32x4 *gsrc_t;
    constexpr bool kHasTail = !std::is_same<TAIL, NoTail>::value && !std::is_same<TAIL, ByteTail>::value;
    const int lane = (int)threadIdx.x & (kWarmLanes - 1), group = (int)threadIdx.x / kWarmLanes;
    const int n16 = t.row_bytes >> 4;
    const long long chunk = (long long)kWarmGroups * kWarmInFlight;
    for (long long c0 = (long long)block * chunk; c0 < n; c0 += (long long)nb * chunk) {
        const unsigned char *src[kWarmInFlight];
        unsigned char *dst[kWarmInFlight];
        unsigned slot[kWarmInFlight], word[kWarmInFlight];
        bool ok[kWarmInFlight];
#pragma unroll
        for (int e = 0; e < kWarmInFlight; e++) {
            const long long i = c0 + (long long)e * kWarmGroups + group;
            ok[e] = i < n;
            const uint4 r = *reinterpret_cast<const uint4 *>(recs + (ok[e] ? i : 0));
            src[e] = reinterpret_cast<const unsigned char *>(((unsigned long long)r.y << 32) | r.x);
            slot[e] = r.z; word[e] = r.w;
            ok[e] = ok[e] && (long long)slot[e] < t.n_slots;   // (the host planned every slot inside the tier; a list that is not the plan's stores nothing)
            dst[e] = t.arena + (unsigned long long)slot[e] * (unsigned long long)t.row_bytes;
        }
        NT tl[kWarmInFlight] = {};
        if constexpr (kHasTail) {
            if (lane == (n16 & (kWarmLanes - 1))) {
#pragma unroll
                for (int e = 0; e < kWarmInFlight; e++) {
                    typedef const __attribute__((address_space(1))) NT *gtail_t;
                    if (ok[e]) tl[e] = *reinterpret_cast<gtail_t>(reinterpret_cast<uintptr_t>(src[e] + n16 * 16));
                }
            }
        }
        for (int p = lane; p < n16; p += kWarmLanes) {
            f32x4 v[kWarmInFlight] = {};
#pragma unroll
            for (int e = 0; e < kWarmInFlight; e++)
                if (ok[e]) v[e] = reinterpret_cast<gsrc_t>(reinterpret_cast<uintptr_t>(src[e]))[p];
#pragma unroll
            for (int e = 0; e < kWarmInFlight; e++)
                if (ok[e]) reinterpret_cast<f32x4 *>(dst[e])[p] = v[e];
        }
        if constexpr (kHasTail) {
            if (lane == (n16 & (kWarmLanes - 1))) {
#pragma unroll
                for (int e = 0; e < kWarmInFlight; e++)
                    if (ok[e]) *reinterpret_cast<NT *>(dst[e] + n16 * 16) = tl[e];
            }
        }
        if constexpr (std::is_same<TAIL, ByteTail>::value) {
#pragma unroll
            for (int e = 0; e < kWarmInFlight; e++)
                for (int b = n16 * 16 + lane; ok[e] && b < t.row_bytes; b += kWarmLanes) dst[e][b] = src[e][b];
        }
        if (lane == 0) {
#pragma unroll
            for (int e = 0; e < kWarmInFlight; e++) {
                if (!ok[e]) continue;
                const unsigned es = slot[e] / t.ways, way = slot[e] - es * t.ways;
                const unsigned long long at = (unsigned long long)(es >> t.sub_shift) * t.line_words + t.w_off +
                                              (es & ((1u << t.sub_shift) - 1u)) * t.ways + way;
                tags[at] = word[e];
            }
        }
    }
}

template <typename TAIL1, typename TAIL2>
__global__ void __launch_bounds__(256) cache_warm_load_pair_kernel(const WarmPairArgs args) {
    if (blockIdx.x < args.blocks1) warm_pair_tier<TAIL1>(args.recs, args.n1, args.tags, args.t1, blockIdx.x, args.blocks1);
    else warm_pair_tier<TAIL2>(args.recs + args.n1, args.n2, args.tags, args.t2, blockIdx.x - args.blocks1, gridDim.x - args.blocks1);
}

template <typename TAIL1, typename TAIL2>
void warm_pair_launch_t(const WarmPairArgs &a, unsigned grid, hipStream_t st) {
    hipLaunchKernelGGL((cache_warm_load_pair_kernel<TAIL1, TAIL2>), dim3(grid), dim3(256), 0, st, a);
}
template <typename TAIL1>
void warm_pair_launch_2(const WarmPairArgs &a, unsigned grid, hipStream_t st) {
    switch (a.t2.row_bytes & 15) {
    case 0: warm_pair_launch_t<TAIL1, NoTail>(a, grid, st); break;
    case 8: warm_pair_launch_t<TAIL1, uint2>(a, grid, st); break;
    case 4: warm_pair_launch_t<TAIL1, unsigned>(a, grid, st); break;
    case 2: warm_pair_launch_t<TAIL1, unsigned short>(a, grid, st); break;           // d = 36 u4: 16 + 2
    default: warm_pair_launch_t<TAIL1, ByteTail>(a, grid, st); break;
    }
}

}  // namespace

void warm_load_launch(const WarmArgs &a, hipStream_t st) {
    if (a.n <= 0) return;
    const long long chunk = (long long)kWarmGroups * kWarmInFlight;
    long long grid = (a.n + chunk - 1) / chunk;
    if (grid > (long long)kNumCu * 8) grid = (long long)kNumCu * 8;
    switch (a.row_bytes & 15) {
    case 0: warm_launch_t<NoTail>(a, (unsigned)grid, st); break;
    case 8: warm_launch_t<uint2>(a, (unsigned)grid, st); break;            // d = 36 u16: 4 x 16 + 8
    case 4: warm_launch_t<unsigned>(a, (unsigned)grid, st); break;         // d = 36 u8: 2 x 16 + 4
    case 2: warm_launch_t<unsigned short>(a, (unsigned)grid, st); break;   // d = 36 u4: 16 + 2
    default: warm_launch_t<ByteTail>(a, (unsigned)grid, st); break;
    }
}

void warm_load_pair_launch(WarmPairArgs a, hipStream_t st) {
    if (a.n1 < 0 || a.n2 < 0 || a.n1 + a.n2 <= 0) return;
    const long long chunk = (long long)kWarmGroups * kWarmInFlight;
    const long long want1 = (a.n1 + chunk - 1) / chunk, want2 = (a.n2 + chunk - 1) / chunk;
    long long grid = want1 + want2, b1 = want1;
    if (grid > (long long)kNumCu * 8) {   // blocks in proportion to the tiers' counts, at least one for a tier that has entries
        grid = (long long)kNumCu * 8;
        b1 = (long long)((double)grid * (double)a.n1 / (double)(a.n1 + a.n2) + 0.5);
        if (a.n1 > 0 && b1 < 1) b1 = 1;
        if (a.n2 > 0 && b1 > grid - 1) b1 = grid - 1;
    }
    a.blocks1 = (unsigned)b1;
    switch (a.t1.row_bytes & 15) {
    case 0: warm_pair_launch_2<NoTail>(a, (unsigned)grid, st); break;               // fp32 d = 36: 9 x 16
    case 8: warm_pair_launch_2<uint2>(a, (unsigned)grid, st); break;
    case 4: warm_pair_launch_2<unsigned>(a, (unsigned)grid, st); break;             // d = 36 u8: 2 x 16 + 4
    case 2: warm_pair_launch_2<unsigned short>(a, (unsigned)grid, st); break;
    default: warm_pair_launch_2<ByteTail>(a, (unsigned)grid, st); break;
    }
}

}  // namespace evs
