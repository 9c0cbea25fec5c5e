// Batched LRU and LFU on the set-associative tier (gfx950): the probe + touch kernel and the insert kernel of the
// separate-launch chain  probe -> consumer -> insert  (evs_cache.hip: cache_batch_impl).  The rule: include/evstore_hip.h,
// evs_cache_set_batch_policy, "the batched rule"; the word layout: evs_cache_policy.h.
//
// What keeps the two kernels simple is that they never run at the same time (one stream, one launch each):
//   * the probe launch only TOUCHES ways (tag and copy-select bit stay): a prober's plain read of a set line sees every tag
//     as it stood when the batch arrived, so hit flags are snapshot flags whatever the other blocks have touched so far --
//     and a touch is a pure function of the word of before the batch, which makes it a plain store (see there);
//   * the insert launch only REPLACES ways, each at most once (old word -> a word stamped n, which nobody takes again): a
//     lost compare-and-swap means exactly "that way now belongs to this batch", so ranking again with the returned word
//     ends after at most 8 rounds.
// Ragged bags (evs_cache_lookup_bags; the rule: include/evstore_hip.h there) run the same chain with a probe over the flat
// list of index positions and a pooling kernel as the consumer:  bags_probe -> bags_pool (-> dense interaction) -> insert.
// EvLFU under the "served bags" rule runs  bags_probe (no touch) -> bags_pool (+ the samples' counts) (-> dense interaction) ->
// bags_raise_list -> cache_batch_sa_list_kernel (evs_cache.hip): a sample's count exists only after the pooling has seen all
// its bags, so the raises and the miss lists come from a launch of their own behind it.  "Count first" (evs_cache_set_bag_count)
// takes the counts out of the pooling:  bags_probe -> bags_count (a pass over the flag bytes) -> bags_pool (pooling alone) -> ... ,
// and in fetch-first order  bags_probe -> bags_count -> bags_raise_list -> update -> sa_repoint -> bags_pool (pooling alone).
// The C1 + C2 pair over bags (evs_cache_lookup_bags_c1c2) runs  bags_probe2 -> bags_count2 -> bags_route2 -> bags_pool2 (-> dense
// interaction) -> cache_batch_sa_list2_kernel (evs_cache.hip): the table a missed position is served from depends on its sample's
// count, so the counts come from a pass over the code bytes IN FRONT of the pooling, and the pooling decodes per position.
// Both tiers at order 1 and "count first":  bags_probe2 -> bags_count2 -> bags_route2 -> cache_batch_sa_list2_kernel ->
// bags_repoint2 -> bags_pool2 (-> dense interaction), every missing row read once, by the update.
// Fed backing (evs_cache_fed_begin[_bags]) cuts the fetch-first chains in two where the rows are fetched; its kernels, (B, T) and
// flat, are described in evs_cache_policy.h at FedSrc and at bags_fed_probe_launch.
#include <type_traits>

#include "evs_cache_policy.h"

namespace evs {
namespace {

// One key against its set, shared by the two probe kernels: the set line (one 32-byte request), the way that holds the key
// and the touch.  gid: the key's dense row number (anything in range when !ok: the lane then reads set 0 and hits nothing).
// TOUCH = false (EvLFU bags): the way words are left alone and L / cur are not read.
struct PolKey { unsigned set, tag1, w; int way; };
template <bool TOUCH = true>
__device__ __forceinline__ bool policy_probe_key(const SaGeom &g, const SaUniverse &u, const PolLayout &L, unsigned cur, bool ok, unsigned gid,
                                                 PolKey &k) {
    k.set = 0u; k.tag1 = 0u; k.w = 0u;
    sa_split(g, sa_perm(u, gid), k.set, k.tag1);
    if (!ok) k.set = 0u;
    SaLine line;
    sa_load<8>(g, k.set, line);
    k.way = sa_find<8>(g, line, k.tag1, k.w);
    const bool is_hit = ok && k.way >= 0;
    if (TOUCH && is_hit && pol_last(L, k.w) != cur) {
        // touch: last = n, LFU counter + 1 (saturating), ONCE per way and batch.  A plain store, no compare-and-swap:
        // nothing but touches writes a way word during this launch, every lane that still reads the way's word of
        // before the batch (stamp != n) derives the SAME new word from it, and a lane that reads the new word stores
        // nothing -- so any number of writers, in any order and over stale copies, leave exactly that word.  (As a
        // compare-and-swap the touch made the chain 34 us per batch instead of 21 at B = 2 048: the tables of 3 .. 30
        // rows put every request of a batch on a handful of addresses, and same-address atomics take their turns.)
        const unsigned c = pol_cnt(k.w);
        sa_ways_ptr(g, k.set)[k.way] = pol_word(L, k.w & L.tag_mask, cur, c < kPolCntMax ? c + 1u : kPolCntMax, pol_sel(L, k.w));
    }
    return is_hit;
}

// K1: one 32-lane half-wave per request (T <= 32), one lane per key -- the set line (one 32-byte request), the hit ballot,
// the touch (one 4-byte store where the way does not carry stamp n yet), the row id / address for the consumer, the miss
// record.
__global__ void __launch_bounds__(256) policy_probe_kernel(const PolicyArgs args) {
    __shared__ int s_sum[2];   // hits / all-hit requests of this block
    __shared__ int s_list_n;
    // per-table values out of LDS: a per-lane index into the kernel arguments is a memory round trip in front of the set loads
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32];
    __shared__ const unsigned char *s_table[32];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_list_n = 0;
    const int T = args.T;
    if (threadIdx.x < 32) {
        s_base[threadIdx.x] = args.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = (int)threadIdx.x < T ? args.backing_rows[threadIdx.x] : 0;
        s_table[threadIdx.x] = args.backing[threadIdx.x];
    }
    __syncthreads();
    const SaGeom &g = args.sa;
    const PolLayout &L = args.lay;
    const unsigned cur = args.cur;
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    const long long req_stride = (long long)gridDim.x * 8;
    for (long long req = (long long)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half; req - half - (threadIdx.x >> 6) * 2 < args.B;
         req += req_stride) {
        const bool req_on = req < args.B;
        const bool key_on = req_on && hl < T;
        const int row = key_on ? args.requests[req * T + hl] : -1;
        const bool ok = key_on && row >= 0 && row < s_rows[hl];
        PolKey key;
        const bool is_hit = policy_probe_key(g, args.sau, L, cur, ok, s_base[hl] + (ok ? (unsigned)row : 0u), key);
        const unsigned set = key.set, tag1 = key.tag1, w = key.w;
        const int way = key.way;
        const unsigned long long hm = __ballot(is_hit);
        const int agg = __popc((unsigned)(half ? (hm >> 32) : hm));
        if (key_on) {
            const long long at = req * T + hl;
            args.hit[at] = is_hit ? 1 : 0;
            const unsigned e = is_hit ? sa_entry(g, set, (unsigned)way, w) : 0u;
            if (args.row_ids) args.row_ids[at] = is_hit ? (int)(0x40000000u | e) : (ok ? row : -1);
            else {
                const unsigned char *src = nullptr;
                if (is_hit) src = args.arena + (long long)e * args.row_bytes;
                else if (ok) src = s_table[hl] + (long long)row * args.row_bytes;
                args.row_ptrs[at] = (long long)src;
            }
        }
        {   // the half-wave's misses, packed, behind the block's earlier ones
            const bool is_miss = ok && way < 0;
            const unsigned long long mm = __ballot(is_miss);
            const unsigned mh = (unsigned)(half ? (mm >> 32) : mm);
            int base = 0;
            if (hl == 0 && mh) base = atomicAdd(&s_list_n, __popc(mh));
            base = __shfl(base, half * 32, 64);
            if (is_miss) {
                const int at = base + __popc(mh & ((1u << hl) - 1u));
                if (at < args.list_cap)
                    args.miss_rec[(long long)blockIdx.x * args.list_cap + at] = make_uint4((unsigned)row, (unsigned)hl, set, tag1);
            }
        }
        if (req_on && hl == 0) { atomicAdd(&s_sum[0], agg); if (agg == T) atomicAdd(&s_sum[1], 1); }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_sum[threadIdx.x])
        atomicAdd(&args.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + 38 + threadIdx.x], s_sum[threadIdx.x]);
    if (threadIdx.x == 0) args.list_cnt[blockIdx.x] = s_list_n < args.list_cap ? s_list_n : args.list_cap;
}

// The probe of a fed call's begin (evs_cache_fed_begin; evs_cache_policy.h at FedSrc), all three policies: K1's walk, flags,
// addresses, miss lists and hit totals, and NO write to a way word -- the call may still be dropped (evs_cache_fed_abort), and a
// dropped call must leave the tier as it found it.  What the probe of a one-call lookup does to the ways it hits (the LRU / LFU
// touch, EvLFU's raise to the request's agg_hit) waits for the finish: fed_hits_kernel.  EVLFU: a miss record carries the request's
// agg_hit (row, table | agg << 8, set, tag + 1), as cache_batch_probe_gather_kernel writes it.
template <bool EVLFU>
__global__ void __launch_bounds__(256) fed_probe_kernel(const PolicyArgs args) {
    __shared__ int s_sum[2];   // hits / all-hit requests of this block
    __shared__ int s_list_n;
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32];
    __shared__ const unsigned char *s_table[32];
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_list_n = 0;
    const int T = args.T;
    if (threadIdx.x < 32) {
        s_base[threadIdx.x] = args.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = (int)threadIdx.x < T ? args.backing_rows[threadIdx.x] : 0;
        s_table[threadIdx.x] = args.backing[threadIdx.x];
    }
    __syncthreads();
    const SaGeom &g = args.sa;
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    const long long req_stride = (long long)gridDim.x * 8;
    for (long long req = (long long)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half; req - half - (threadIdx.x >> 6) * 2 < args.B;
         req += req_stride) {
        const bool req_on = req < args.B;
        const bool key_on = req_on && hl < T;
        const int row = key_on ? args.requests[req * T + hl] : -1;
        const bool ok = key_on && row >= 0 && row < s_rows[hl];
        PolKey key;
        const bool is_hit = policy_probe_key<false>(g, args.sau, args.lay, args.cur, ok, s_base[hl] + (ok ? (unsigned)row : 0u), key);
        const unsigned long long hm = __ballot(is_hit);
        const int agg = __popc((unsigned)(half ? (hm >> 32) : hm));
        if (key_on) {
            const long long at = req * T + hl;
            args.hit[at] = is_hit ? 1 : 0;
            const unsigned char *src = nullptr;
            if (is_hit) src = args.arena + (long long)sa_entry(g, key.set, (unsigned)key.way, key.w) * args.row_bytes;
            else if (ok) src = s_table[hl] + (long long)row * args.row_bytes;   // (a fed table: NULL-based, rewritten by sa_repoint_fed_kernel)
            args.row_ptrs[at] = (long long)src;
        }
        {   // the half-wave's misses, packed, behind the block's earlier ones
            const bool is_miss = ok && key.way < 0;
            const unsigned long long mm = __ballot(is_miss);
            const unsigned mh = (unsigned)(half ? (mm >> 32) : mm);
            int base = 0;
            if (hl == 0 && mh) base = atomicAdd(&s_list_n, __popc(mh));
            base = __shfl(base, half * 32, 64);
            if (is_miss) {
                const int at = base + __popc(mh & ((1u << hl) - 1u));
                if (at < args.list_cap)
                    args.miss_rec[(long long)blockIdx.x * args.list_cap + at] =
                        make_uint4((unsigned)row, (unsigned)hl | (EVLFU ? (unsigned)agg << 8 : 0u), key.set, key.tag1);
            }
        }
        if (req_on && hl == 0) { atomicAdd(&s_sum[0], agg); if (agg == T) atomicAdd(&s_sum[1], 1); }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_sum[threadIdx.x])
        atomicAdd(&args.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + 38 + threadIdx.x], s_sum[threadIdx.x]);
    if (threadIdx.x == 0) args.list_cnt[blockIdx.x] = s_list_n < args.list_cap ? s_list_n : args.list_cap;
}

// The hold form of that probe (a call that begins while another is open; evs_cache_policy.h at FedHold): the same kernel, line for
// line -- kept as a kernel of its own so that fed_probe_kernel compiles to what it was --, and every way a position is flagged 1 for
// gets its bit in the call's hold map: the word is read first, the atomicOr goes out only where the bit is still clear, and the lane
// whose atomicOr found it clear counts it.
template <bool EVLFU>
__global__ void __launch_bounds__(256) fed_probe_hold_kernel(const PolicyArgs args, const FedHold fh) {
    __shared__ int s_sum[2];   // hits / all-hit requests of this block
    __shared__ int s_list_n;
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32];
    __shared__ const unsigned char *s_table[32];
    __shared__ int s_held;
    if (threadIdx.x < 2) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_list_n = 0;
    if (threadIdx.x == 0) s_held = 0;
    const int T = args.T;
    if (threadIdx.x < 32) {
        s_base[threadIdx.x] = args.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = (int)threadIdx.x < T ? args.backing_rows[threadIdx.x] : 0;
        s_table[threadIdx.x] = args.backing[threadIdx.x];
    }
    __syncthreads();
    const SaGeom &g = args.sa;
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    const long long req_stride = (long long)gridDim.x * 8;
    for (long long req = (long long)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half; req - half - (threadIdx.x >> 6) * 2 < args.B;
         req += req_stride) {
        const bool req_on = req < args.B;
        const bool key_on = req_on && hl < T;
        const int row = key_on ? args.requests[req * T + hl] : -1;
        const bool ok = key_on && row >= 0 && row < s_rows[hl];
        PolKey key;
        const bool is_hit = policy_probe_key<false>(g, args.sau, args.lay, args.cur, ok, s_base[hl] + (ok ? (unsigned)row : 0u), key);
        const unsigned long long hm = __ballot(is_hit);
        const int agg = __popc((unsigned)(half ? (hm >> 32) : hm));
        if (key_on) {
            const long long at = req * T + hl;
            args.hit[at] = is_hit ? 1 : 0;
            const unsigned char *src = nullptr;
            if (is_hit) src = args.arena + (long long)sa_entry(g, key.set, (unsigned)key.way, key.w) * args.row_bytes;
            else if (ok) src = s_table[hl] + (long long)row * args.row_bytes;   // (a fed table: NULL-based, rewritten by sa_repoint_fed_kernel)
            args.row_ptrs[at] = (long long)src;
        }
        if (is_hit) {   // the hold
            unsigned *word = reinterpret_cast<unsigned *>(fh.mine) + (key.set >> 2);
            const unsigned bit = 1u << ((key.set & 3u) * 8u + (unsigned)key.way);
            if (!(__atomic_load_n(word, __ATOMIC_RELAXED) & bit) && !(atomicOr(word, bit) & bit)) atomicAdd(&s_held, 1);
        }
        {   // the half-wave's misses, packed, behind the block's earlier ones
            const bool is_miss = ok && key.way < 0;
            const unsigned long long mm = __ballot(is_miss);
            const unsigned mh = (unsigned)(half ? (mm >> 32) : mm);
            int base = 0;
            if (hl == 0 && mh) base = atomicAdd(&s_list_n, __popc(mh));
            base = __shfl(base, half * 32, 64);
            if (is_miss) {
                const int at = base + __popc(mh & ((1u << hl) - 1u));
                if (at < args.list_cap)
                    args.miss_rec[(long long)blockIdx.x * args.list_cap + at] =
                        make_uint4((unsigned)row, (unsigned)hl | (EVLFU ? (unsigned)agg << 8 : 0u), key.set, key.tag1);
            }
        }
        if (req_on && hl == 0) { atomicAdd(&s_sum[0], agg); if (agg == T) atomicAdd(&s_sum[1], 1); }
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_sum[threadIdx.x])
        atomicAdd(&args.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + 38 + threadIdx.x], s_sum[threadIdx.x]);
    if (threadIdx.x == 0) args.list_cnt[blockIdx.x] = s_list_n < args.list_cap ? s_list_n : args.list_cap;
    if (threadIdx.x == 0 && s_held) atomicAdd(&fh.counters[0], (unsigned long long)s_held);
}

// ... and, first launch of the finish, what that probe left undone: every position the begin flagged 1 finds its way again (the tier
// has not moved: everything else is refused while the call is open) and is touched (LRU / LFU: policy_probe_key's plain store) or
// raised to its request's agg_hit = the number of its flags that are 1 (EvLFU: sa_raise, the histogram moves into part1 columns
// 0 .. T).  Nothing else writes a way word during this launch; the update runs behind it and reads what it would have read behind
// a probe that touched and raised by itself.
template <bool EVLFU>
__global__ void __launch_bounds__(256) fed_hits_kernel(const PolicyArgs args) {
    __shared__ int s_delta[64];   // priority histogram moves (0 .. T, T <= 32; sized by the word's 6-bit field)
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32];
    const int T = args.T;
    if (threadIdx.x < 64) s_delta[threadIdx.x] = 0;
    if (threadIdx.x < 32) {
        s_base[threadIdx.x] = args.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = (int)threadIdx.x < T ? args.backing_rows[threadIdx.x] : 0;
    }
    __syncthreads();
    const SaGeom &g = args.sa;
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    const long long req_stride = (long long)gridDim.x * 8;
    for (long long req = (long long)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half; req - half - (threadIdx.x >> 6) * 2 < args.B;
         req += req_stride) {
        const bool key_on = req < args.B && hl < T;
        const int row = key_on ? args.requests[req * T + hl] : -1;
        const bool ok = key_on && row >= 0 && row < s_rows[hl] && args.hit[req * T + hl] == 1;   // the begin's hits alone
        PolKey key;
        const bool is_hit = policy_probe_key<!EVLFU>(g, args.sau, args.lay, args.cur, ok, s_base[hl] + (ok ? (unsigned)row : 0u), key);
        (void)is_hit;
        if constexpr (EVLFU) {
            const unsigned long long hm = __ballot(ok);
            const int agg = __popc((unsigned)(half ? (hm >> 32) : hm));
            if (is_hit && sa_prio(key.w) < agg) {
                const int old = sa_raise(g, sa_ways_ptr(g, key.set) + key.way, key.w, agg);
                if (old >= 0) { atomicSub(&s_delta[old], 1); atomicAdd(&s_delta[agg], 1); }
            }
        }
    }
    if constexpr (EVLFU) {
        __syncthreads();
        if ((int)threadIdx.x <= T && s_delta[threadIdx.x])
            atomicAdd(&args.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + threadIdx.x], s_delta[threadIdx.x]);
    }
}

// K1 over ragged bags: one lane per POSITION of the flat, table-major lookup list (evs_cache_lookup_bags).  The lane's table
// comes from the prefix sums of nnz (five steps over an LDS table); per position the int64 index, its range check, the set
// line, the touch (policy_probe_key), then the hit flag, the 8-byte row address for the pooling kernel and -- for a miss --
// the record policy_insert_kernel reads.  An index out of range is no key: flag 0, address 0, no record, the sticky flag.
// EVLFU: no touch and no list -- a provisional record per position for bags_raise_list_kernel (the hit way, or the set and the
// tag of a miss: nothing is searched twice) and pos_sample preset to "no bag covers it".
template <bool EVLFU>
__global__ void __launch_bounds__(256) bags_probe_kernel(const BagArgs args) {
    __shared__ int s_hits, s_list_n;
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32], s_pos0[32];
    __shared__ const long long *s_idx[32];
    __shared__ const unsigned char *s_table[32];
    const PolicyArgs &pa = args.p;
    const int T = pa.T;
    if (threadIdx.x == 0) { s_hits = 0; s_list_n = 0; }
    if (threadIdx.x < 32) {
        const bool tab = (int)threadIdx.x < T;
        s_base[threadIdx.x] = pa.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = tab ? pa.backing_rows[threadIdx.x] : 0;
        s_table[threadIdx.x] = pa.backing[threadIdx.x];
        s_idx[threadIdx.x] = args.indices[threadIdx.x];
        s_pos0[threadIdx.x] = tab ? args.pos0[threadIdx.x] : args.n_pos;   // (past the last table: no position is that far)
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    bool bad = false;
    for (int i = 0; i < args.iters; i++) {   // block-uniform trip count (the ballots below)
        const long long p = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
        const bool on = p < args.n_pos;
        // the table of position p: the largest k with pos0[k] <= p (pos0 never falls, so "pos0[j] <= p" holds for a prefix of j;
        // a table without indices shares its start with the next one and is passed over)
        int k = 0;
#pragma unroll
        for (int step = 16; step >= 1; step >>= 1) k += (on && s_pos0[k + step] <= p) ? step : 0;
        const long long row = on ? s_idx[k][p - s_pos0[k]] : -1;
        const bool ok = on && row >= 0 && row < s_rows[k];
        bad = bad || (on && !ok);
        PolKey key;
        const bool is_hit = policy_probe_key<!EVLFU>(pa.sa, pa.sau, pa.lay, pa.cur, ok, s_base[k] + (ok ? (unsigned)row : 0u), key);
        if (on) {
            pa.hit[p] = is_hit ? 1 : 0;
            const unsigned char *src = nullptr;
            if (is_hit) src = pa.arena + (long long)sa_entry(pa.sa, key.set, (unsigned)key.way, key.w) * pa.row_bytes;
            else if (ok) src = s_table[k] + row * pa.row_bytes;
            pa.row_ptrs[p] = (long long)src;
            if constexpr (EVLFU) {
                args.prov[p] = make_uint4((unsigned)row, (unsigned)k, key.set, is_hit ? (0x80000000u | (unsigned)key.way) : (ok ? key.tag1 : 0u));
                args.pos_sample[p] = -1;
            }
        }
        const unsigned long long hm = __ballot(is_hit);
        if (lane == 0 && hm) atomicAdd(&s_hits, __popcll(hm));
        if constexpr (!EVLFU) {   // the wave's misses, packed, behind the block's earlier ones
            const bool is_miss = ok && key.way < 0;
            const unsigned long long mm = __ballot(is_miss);
            int base = 0;
            if (lane == 0 && mm) base = atomicAdd(&s_list_n, __popcll(mm));
            base = __shfl(base, 0, 64);
            if (is_miss) {
                const int at = base + __popcll(mm & ((1ull << lane) - 1ull));
                if (at < pa.list_cap)
                    pa.miss_rec[(long long)blockIdx.x * pa.list_cap + at] = make_uint4((unsigned)row, (unsigned)k, key.set, key.tag1);
            }
        }
    }
    if (bad) atomicOr(args.err, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_hits) atomicAdd(&pa.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + 38], s_hits);
        if constexpr (!EVLFU) pa.list_cnt[blockIdx.x] = s_list_n < pa.list_cap ? s_list_n : pa.list_cap;
    }
}

// Pooling through the probe's pointer table (embedding_bag_sum_kernel's shape, evs_gather.hip): a lane group of d / 4 lanes
// owns a bag, UNROLL bags in flight per group, the table id wave-uniform (per-table values from scalar loads), index order,
// unfused fp32 adds from +0 -- and the row address read from the table instead of computed from an index: the probe has done
// the range check (address 0: no row).  The bag bounds check and its error flag stay.  A group also tells its sample's word
// (sample_cnt) what the bag was -- empty or not, all hits or not; whoever brings a sample's T-th bag judges the sample,
// counts it into column 39 (all-hit requests) and leaves the word zero for the next launch.
// EVLFU ("served bags"): the judge also writes agg[b] = T - the sample's bags with a miss, and the piece-0 lane of a group tells
// every position its bag covers which sample it belongs to (pos_sample; the probe preset -1).  The map comes from this walk
// and not from a search over the offsets: a bag the bounds check calls empty covers nothing, exactly as it pools nothing.
// COUNT = false (EvLFU "count first": bags_count_kernel has judged the samples in front of this launch): the pooling alone -- no
// flag is read, no sample word, agg, pos_sample or column 39 written; the bounds check and its sticky flag stay.
template <int CODEC, int UNROLL, bool EVLFU, bool COUNT = true>
__global__ void __launch_bounds__(256) bags_pool_kernel(const BagArgs args) {
    __shared__ float s_lut[CodecLut<CODEC>::kEntries];
    __shared__ int s_perfect;
    if constexpr (CODEC != 32) codec_lut_init<CODEC>(s_lut);
    if (COUNT && threadIdx.x == 0) s_perfect = 0;
    __syncthreads();
    const int T = args.p.T;
    const int LPR = args.d / 4;
    const int RPW = kWave / LPR;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int slot = lane / LPR;
    const int piece = lane - slot * LPR;
    const bool lane_on = slot < RPW;
    const long long B = args.p.B;
    const int bags_per_item = RPW * UNROLL;
    const unsigned char *arena = args.p.arena, *arena_end = args.arena_end;
    const int64_t n_items = (int64_t)T * args.chunks_per_table;
    const XcdRange xr = xcd_range(n_items, 4, wave);
    bool bad = false;
    int n_perfect = 0;

    for (int64_t item = xr.first; item < xr.end; item += xr.stride) {
        const int t = __builtin_amdgcn_readfirstlane((int)(item / args.chunks_per_table));
        const long long chunk = item - (long long)t * args.chunks_per_table;
        const long long b0 = chunk * bags_per_item;
        const long long *__restrict__ off = args.offsets[t];
        const long long nnz = args.pos0[t + 1] - args.pos0[t];
        const long long *__restrict__ ptrs = args.p.row_ptrs + args.pos0[t];
        const unsigned char *__restrict__ flags = args.pool_flags ? args.pool_flags + args.pos0[t] : nullptr;

        long long s[UNROLL], len[UNROLL];
        long long maxlen = 0;
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const long long b = b0 + (long long)u * RPW + slot;
            s[u] = 0;
            len[u] = 0;
            if (lane_on && b < B) {
                const long long st = off[b];
                const long long en = (b + 1 < B) ? off[b + 1] : nnz;
                if (st >= 0 && en >= st && en <= nnz) {
                    s[u] = st;
                    len[u] = en - st;
                } else {
                    bad = true;
                }
            }
            maxlen = len[u] > maxlen ? len[u] : maxlen;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {   // wave-wide max bag length (all lanes run the same trip count)
            const long long o = __shfl_xor(maxlen, m, kWave);
            maxlen = o > maxlen ? o : maxlen;
        }

        float4 acc[UNROLL];
        bool miss[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) { acc[u] = make_float4(0.f, 0.f, 0.f, 0.f); miss[u] = false; }

        for (long long j = 0; j < maxlen; j++) {
            const unsigned char *r[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                r[u] = nullptr;
                if (j < len[u]) {
                    r[u] = reinterpret_cast<const unsigned char *>(ptrs[s[u] + j]);
                    // (fetch-first order: an installed miss points into the arena by now -- the probe's flag says what it was)
                    if constexpr (COUNT) miss[u] = miss[u] || (flags ? flags[s[u] + j] == 0 : !(r[u] >= arena && r[u] < arena_end));
                    if constexpr (EVLFU && COUNT) {
                        if (piece == 0) args.pos_sample[args.pos0[t] + s[u] + j] = (int)(b0 + (long long)u * RPW + slot);
                    }
                }
            }
            float4 v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r[u]) v[u] = RowPiece<CODEC>::load(r[u], piece, s_lut);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                if (r[u]) {
                    acc[u].x = __fadd_rn(acc[u].x, v[u].x);
                    acc[u].y = __fadd_rn(acc[u].y, v[u].y);
                    acc[u].z = __fadd_rn(acc[u].z, v[u].z);
                    acc[u].w = __fadd_rn(acc[u].w, v[u].w);
                }
            }
        }

        float *__restrict__ out = args.out + (long long)t * args.out_tstride + (long long)piece * 4;
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const long long b = b0 + (long long)u * RPW + slot;
            if (lane_on && b < B) {
                *reinterpret_cast<float4 *>(out + b * args.out_bstride) = acc[u];
                if (COUNT && piece == 0) {
                    const int mine = 1 | (len[u] > 0 ? 1 << 8 : 0) | (miss[u] ? 1 << 16 : 0);
                    const int all = atomicAdd(&args.sample_cnt[b], mine) + mine;
                    if ((all & 0xff) == T) {   // the sample's last bag: nobody else writes the word any more
                        args.sample_cnt[b] = 0;
                        if (((all >> 8) & 0xff) != 0 && (all >> 16) == 0) n_perfect++;
                        if constexpr (EVLFU) args.agg[b] = T - (all >> 16);
                    }
                }
            }
        }
    }
    if (bad) atomicOr(args.err, 1);
    if constexpr (COUNT) {
        if (n_perfect) atomicAdd(&s_perfect, n_perfect);
        __syncthreads();
        if (threadIdx.x == 0 && s_perfect)
            atomicAdd(&args.p.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + 39], s_perfect);
    }
}

// The count pass of the single tier (EvLFU "count first", evs_cache_set_bag_count(c, 1)): agg_hit(b) is a function of the probe's
// flags and the offsets alone, so it needs no row -- bags_count2_kernel's walk and hand-over over the flag bytes the probe wrote
// (args.p.hit: the caller's array when one was given).  A group of G lanes owns a bag: lane g of the group reads flags
// st + g, st + g + G, ... and tells those positions their sample (pos_sample; the probe preset -1), the group's verdict is one
// ballot, and lane 0 hands it to the sample's word: whoever brings a sample's T-th bag writes agg[b] = T - (bags with a miss),
// counts the all-served sample with a lookup into column 39 and leaves the word zero.  A bag whose offsets are backwards or past
// nnz is empty (served) and raises the sticky flag; an index out of range has flag 0 and makes its bag unserved.
// G = 1 is the pair's lane per bag: neighbouring lanes walk neighbouring bags, whose flags are one contiguous run, so short bags
// coalesce by themselves.  At 100 indices per bag a lane per bag reads bytes 100 apart and stores pos_sample words 400 bytes
// apart -- one line per lane and step; G = 16 makes every step of a group one 16-byte read and one 64-byte store.  The bag of a
// group is wave-uniform in trip count only per group, so the ballot stands behind the walk, where the wave has reconverged.
template <int G>
__global__ void __launch_bounds__(256) bags_count_kernel(const BagArgs args) {
    __shared__ int s_perfect;
    __shared__ long long s_pos0[33];
    __shared__ const long long *s_off[32];
    if (threadIdx.x == 0) s_perfect = 0;
    if (threadIdx.x < 33) s_pos0[threadIdx.x] = args.pos0[threadIdx.x];
    if (threadIdx.x < 32) s_off[threadIdx.x] = args.offsets[threadIdx.x];
    __syncthreads();
    const int T = args.p.T;
    const long long B = args.p.B, n_bags = (long long)T * B;
    constexpr int kBagsPerBlock = 256 / G;
    const int g = threadIdx.x & (G - 1);
    const int lane = threadIdx.x & 63;
    bool bad = false;
    int n_perfect = 0;
    // (block-uniform trip count: every lane of a wave reaches the ballot)
    for (long long i0 = (long long)blockIdx.x * kBagsPerBlock; i0 < n_bags; i0 += (long long)gridDim.x * kBagsPerBlock) {
        const long long i = i0 + threadIdx.x / G;
        const bool on = i < n_bags;
        const int t = on ? (int)(i / B) : 0;
        const long long b = on ? i - (long long)t * B : 0;
        const long long nnz = s_pos0[t + 1] - s_pos0[t];
        long long st = 0, en = 0;
        if (on) {
            const long long *__restrict__ off = s_off[t];
            st = off[b];
            en = (b + 1 < B) ? off[b + 1] : nnz;
            if (!(st >= 0 && en >= st && en <= nnz)) { bad = true; st = 0; en = 0; }
        }
        const unsigned char *__restrict__ flags = args.p.hit + s_pos0[t];
        int *__restrict__ ps = args.pos_sample + s_pos0[t];
        bool miss = false;
        for (long long j = st + g; j < en; j += G) {
            miss = miss || flags[j] == 0;
            ps[j] = (int)b;
        }
        if constexpr (G > 1) {
            const unsigned long long mm = __ballot(miss);
            miss = ((mm >> (lane & ~(G - 1))) & ((1ull << G) - 1ull)) != 0ull;
        }
        if (on && g == 0) {
            const int mine = 1 | (en > st ? 1 << 8 : 0) | (miss ? 1 << 16 : 0);
            const int all = atomicAdd(&args.sample_cnt[b], mine) + mine;
            if ((all & 0xff) == T) {   // the sample's last bag: nobody else writes the word any more
                args.sample_cnt[b] = 0;
                args.agg[b] = T - (all >> 16);
                if (((all >> 8) & 0xff) != 0 && (all >> 16) == 0) n_perfect++;
            }
        }
    }
    if (bad) atomicOr(args.err, 1);
    if (n_perfect) atomicAdd(&s_perfect, n_perfect);
    __syncthreads();
    if (threadIdx.x == 0 && s_perfect)
        atomicAdd(&args.p.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + 39], s_perfect);
}

// EvLFU "served bags", behind the pooling: one lane per position, the probe's grid and walk.  a = agg of the position's sample
// (0 when no valid bag covers it).  A hit way goes to max(old, a): a plain read of the word first, the compare-and-swap
// (sa_raise) only while the priority is below a -- the tables of a few rows put thousands of positions on one word, and every
// one of them after the first finds nothing left to do.  A miss goes into the block's list with its count, in the record
// cache_batch_sa_list_kernel reads; copies of a key fold their counts there.  Nothing but raises writes a way word during
// this launch, so a way the probe found still holds its key.
__global__ void __launch_bounds__(256) bags_raise_list_kernel(const BagArgs args) {
    __shared__ int s_delta[64];   // priority histogram moves (0 .. T, T <= 32; sized by the word's 6-bit field)
    __shared__ int s_list_n;
    const PolicyArgs &pa = args.p;
    const SaGeom &g = pa.sa;
    const int T = pa.T;
    if (threadIdx.x < 64) s_delta[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_list_n = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int i = 0; i < args.iters; i++) {   // block-uniform trip count (the ballot below)
        const long long p = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        int a = 0;
        if (p < args.n_pos) {
            r = args.prov[p];
            const int b = args.pos_sample[p];
            if (b >= 0) a = args.agg[b];
        }
        const bool is_hit = (r.w & 0x80000000u) != 0u;
        const bool is_miss = !is_hit && r.w != 0u;
        if (is_hit && a > 0) {
            unsigned *wp = sa_ways_ptr(g, r.z) + (r.w & 7u);
            const unsigned w = *wp;
            if (sa_prio(w) < a) {
                const int old = sa_raise(g, wp, w, a);
                if (old >= 0) { atomicSub(&s_delta[old], 1); atomicAdd(&s_delta[a], 1); }
            }
        }
        const unsigned long long mm = __ballot(is_miss);
        int base = 0;
        if (lane == 0 && mm) base = atomicAdd(&s_list_n, __popcll(mm));
        base = __shfl(base, 0, 64);
        if (is_miss) {
            const int at = base + __popcll(mm & ((1ull << lane) - 1ull));
            if (at < pa.list_cap)
                pa.miss_rec[(long long)blockIdx.x * pa.list_cap + at] = make_uint4(r.x, r.y | ((unsigned)a << 8), r.z, r.w);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x <= T && s_delta[threadIdx.x])
        atomicAdd(&pa.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + threadIdx.x], s_delta[threadIdx.x]);
    if (threadIdx.x == 0) pa.list_cnt[blockIdx.x] = s_list_n < pa.list_cap ? s_list_n : pa.list_cap;
}

// ---- ragged bags through the C1 + C2 pair (evs_cache_lookup_bags_c1c2; the records: evs_cache_policy.h, BagPairArgs) ----------
// K1 of the pair over bags: bags_probe_kernel's walk, cache_batch_probe2_kernel's look at the shared record -- both tiers' ways of
// the key's set in one line request, "C1 has room" = the key's own C1 set has a free way -- and no write to a way word: the
// raises wait for the samples' counts (bags_route2_kernel).  An index out of range of either tier's table is no key.
constexpr unsigned kProvWayShift = 8, kProvCodeShift = 12, kProvRoom = 1u << 14, kProvKey = 1u << 15;
__global__ void __launch_bounds__(256) bags_probe2_kernel(const BagPairArgs args) {
    __shared__ int s_hits[2];
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32], s_pos0[32];
    __shared__ const long long *s_idx[32];
    const int T = args.T;
    if (threadIdx.x < 2) s_hits[threadIdx.x] = 0;
    if (threadIdx.x < 32) {
        const bool tab = (int)threadIdx.x < T;
        s_base[threadIdx.x] = args.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = tab ? args.rows[threadIdx.x] : 0;
        s_idx[threadIdx.x] = args.indices[threadIdx.x];
        s_pos0[threadIdx.x] = tab ? args.pos0[threadIdx.x] : args.n_pos;
    }
    __syncthreads();
    const SaGeom &g1 = args.sa1, &g2 = args.sa2;
    const bool w88 = g1.ways == 8u && g2.ways == 8u;   // (the reference's 1 : 2 pair: way counts known to the compiler)
    const int lane = threadIdx.x & 63;
    bool bad = false;
    for (int i = 0; i < args.iters; i++) {   // block-uniform trip count (the ballots below)
        const long long p = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
        const bool on = p < args.n_pos;
        int k = 0;
#pragma unroll
        for (int step = 16; step >= 1; step >>= 1) k += (on && s_pos0[k + step] <= p) ? step : 0;
        const long long row = on ? s_idx[k][p - s_pos0[k]] : -1;
        const bool ok = on && row >= 0 && row < s_rows[k];
        bad = bad || (on && !ok);
        unsigned set = 0u, q = 0u;
        sa_divmod(g1, sa_perm(args.sau, s_base[k] + (ok ? (unsigned)row : 0u)), set, q);   // (the tiers share nset: one division)
        if (!ok) { set = 0u; q = 0u; }
        unsigned es1, tg1, es2, tg2, w1 = 0u, w2 = 0u;
        sa_place(g1, set, q, es1, tg1);
        sa_place(g2, set, q, es2, tg2);
        SaLine l1, l2;
        int y1, y2;
        bool room;
        if (w88) {
            sa_load<8>(g1, es1, l1);
            sa_load<8>(g2, es2, l2);
            y1 = sa_find<8>(g1, l1, tg1, w1); y2 = sa_find<8>(g2, l2, tg2, w2);
            room = sa_has_free<8>(g1, l1);
        } else {
            sa_load<0>(g1, es1, l1);
            sa_load<0>(g2, es2, l2);
            y1 = sa_find<0>(g1, l1, tg1, w1); y2 = sa_find<0>(g2, l2, tg2, w2);
            room = sa_has_free<0>(g1, l1);
        }
        const unsigned code = (ok && y1 >= 0) ? 1u : ((ok && y2 >= 0) ? 2u : 0u);
        if (on) {
            const unsigned char *src = nullptr;
            if (code == 1u) src = args.arena1 + (long long)sa_entry(g1, es1, (unsigned)y1, w1) * args.row_bytes1;
            else if (code == 2u) src = args.arena2 + (long long)sa_entry(g2, es2, (unsigned)y2, w2) * args.row_bytes2;
            args.code[p] = (unsigned char)code;
            args.serve[p] = (unsigned char)code;
            args.row_ptrs[p] = (long long)src;
            const unsigned way = code == 1u ? (unsigned)y1 : (code == 2u ? (unsigned)y2 : 0u);
            args.prov[p] = make_uint4((unsigned)row, (unsigned)k | (way << kProvWayShift) | (code << kProvCodeShift) | (room ? kProvRoom : 0u) | (ok ? kProvKey : 0u),
                                      set, q);
            args.pos_sample[p] = -1;
        }
        const unsigned long long h1 = __ballot(code == 1u), h2 = __ballot(code == 2u);
        if (lane == 0) {
            if (h1) atomicAdd(&s_hits[0], __popcll(h1));
            if (h2) atomicAdd(&s_hits[1], __popcll(h2));
        }
    }
    if (bad) atomicOr(args.err, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_hits[0]) atomicAdd(&args.part1_1[(blockIdx.x % kPolReplicas) * kPolPartCols + 38], s_hits[0]);
        if (s_hits[1]) atomicAdd(&args.part1_2[(blockIdx.x % kPolReplicas) * kPolPartCols + 38], s_hits[1]);
    }
}

// The count pass: a lane per bag walks the bag's code bytes -- no row is touched -- tells every position it covers which sample
// it belongs to, and hands its verdict to the sample's word (bags_pool_kernel's sample_cnt hand-over): whoever brings a sample's
// T-th bag writes agg[b] = the sample's served bags, counts an all-served sample with a lookup into column 39 and leaves the
// word zero.  It runs before the pooling because the table a miss is served from depends on agg.  A bag whose offsets are
// backwards or past nnz is empty (served) and raises the sticky flag.
__global__ void __launch_bounds__(256) bags_count2_kernel(const BagPairArgs args) {
    __shared__ int s_perfect;
    __shared__ long long s_pos0[33];
    __shared__ const long long *s_off[32];
    if (threadIdx.x == 0) s_perfect = 0;
    if (threadIdx.x < 33) s_pos0[threadIdx.x] = args.pos0[threadIdx.x];
    if (threadIdx.x < 32) s_off[threadIdx.x] = args.offsets[threadIdx.x];
    __syncthreads();
    const int T = args.T;
    const long long B = args.B, n_bags = (long long)T * B;
    bool bad = false;
    int n_perfect = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_bags; i += (long long)gridDim.x * 256) {
        const int t = (int)(i / B);
        const long long b = i - (long long)t * B;
        const long long nnz = s_pos0[t + 1] - s_pos0[t];
        const long long *__restrict__ off = s_off[t];
        long long st = off[b];
        long long en = (b + 1 < B) ? off[b + 1] : nnz;
        if (!(st >= 0 && en >= st && en <= nnz)) { bad = true; st = 0; en = 0; }
        const unsigned char *__restrict__ code = args.code + s_pos0[t];
        int *__restrict__ ps = args.pos_sample + s_pos0[t];
        bool miss = false;
        for (long long j = st; j < en; j++) {
            miss = miss || code[j] == 0;
            ps[j] = (int)b;
        }
        const int mine = 1 | (en > st ? 1 << 8 : 0) | (miss ? 1 << 16 : 0);
        const int all = atomicAdd(&args.sample_cnt[b], mine) + mine;
        if ((all & 0xff) == T) {   // the sample's last bag: nobody else writes the word any more
            args.sample_cnt[b] = 0;
            args.agg[b] = T - (all >> 16);
            if (((all >> 8) & 0xff) != 0 && (all >> 16) == 0) n_perfect++;
        }
    }
    if (bad) atomicOr(args.err, 1);
    if (n_perfect) atomicAdd(&s_perfect, n_perfect);
    __syncthreads();
    if (threadIdx.x == 0 && s_perfect)
        atomicAdd(&args.part1_1[(blockIdx.x % kPolReplicas) * kPolPartCols + 39], s_perfect);
}

// Route + raise + list: one lane per position, the probe's grid and walk.  a = agg of the position's sample (0 when no valid bag
// covers it).  A hit way goes to max(old, a) in the tier that holds it (a plain read first, as bags_raise_list_kernel).  A miss is
// routed on the snapshot (evlfu_8.cpp:570-601 as cache_batch_probe2_kernel evaluates it: the key's own C1 set has room -> C1;
// else a < threshold -> C1 for an odd table index, C2 for an even one; else C2), gets the destination's table row and serve
// byte, stamps the route filter (odd tables routed to C1) and goes into the block's list of its tier in the record
// cache_batch_sa_list2_kernel reads.  Nothing but raises writes a way word during this launch.
__global__ void __launch_bounds__(256) bags_route2_kernel(const BagPairArgs args) {
    __shared__ int s_delta[2][64];
    __shared__ int s_list_n[2];
    __shared__ const unsigned char *s_tab[2][32];
    const int T = args.T;
    if (threadIdx.x < 128) s_delta[threadIdx.x >> 6][threadIdx.x & 63] = 0;
    if (threadIdx.x < 2) s_list_n[threadIdx.x] = 0;
    if (threadIdx.x < 32) { s_tab[0][threadIdx.x] = args.backing1[threadIdx.x]; s_tab[1][threadIdx.x] = args.backing2[threadIdx.x]; }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int i = 0; i < args.iters; i++) {   // block-uniform trip count (the ballots below)
        const long long p = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
        const bool on = p < args.n_pos;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        int a = 0;
        if (on) {
            r = args.prov[p];
            const int b = args.pos_sample[p];
            if (b >= 0) a = args.agg[b];
        }
        const int k = (int)(r.y & 31u);
        const unsigned code = (r.y >> kProvCodeShift) & 3u;
        const bool is_miss = (r.y & kProvKey) != 0u && code == 0u;
        int dest = 0;
        if (code != 0u) dest = (int)code;
        else if (is_miss) dest = (r.y & kProvRoom) ? 1 : (a < args.threshold ? ((k & 1) ? 1 : 2) : 2);
        const SaGeom &g = dest == 2 ? args.sa2 : args.sa1;
        unsigned es = 0u, tag1 = 0u;
        sa_place(g, r.z, r.w, es, tag1);
        if (code != 0u && a > 0) {
            unsigned *wp = sa_ways_ptr(g, es) + ((r.y >> kProvWayShift) & 15u);
            const unsigned w = *wp;
            if (sa_prio(w) < a) {
                const int old = sa_raise(g, wp, w, a);
                if (old >= 0) { atomicSub(&s_delta[dest - 1][old], 1); atomicAdd(&s_delta[dest - 1][a], 1); }
            }
        }
        if (is_miss) {
            args.serve[p] = (unsigned char)dest;
            args.row_ptrs[p] = (long long)(s_tab[dest - 1][k] + (long long)r.x * (dest == 1 ? args.row_bytes1 : args.row_bytes2));
            if (args.route_filter && dest == 1 && (k & 1))
                args.route_filter[mix64(((unsigned long long)(k + 1) << 32) | r.x) & args.route_mask] = args.route_stamp;
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {   // the wave's misses of each tier, packed, behind the block's earlier ones
            const bool mine = is_miss && dest == t + 1;
            const unsigned long long mm = __ballot(mine);
            int base = 0;
            if (lane == 0 && mm) base = atomicAdd(&s_list_n[t], __popcll(mm));
            base = __shfl(base, 0, 64);
            if (mine) {
                const int at = base + __popcll(mm & ((1ull << lane) - 1ull));
                if (at < args.list_cap)
                    (t ? args.miss_rec2 : args.miss_rec1)[(long long)blockIdx.x * args.list_cap + at] = make_uint4(r.x, (unsigned)k | ((unsigned)a << 8), es, tag1);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x <= T) {
        const int v1 = s_delta[0][threadIdx.x], v2 = s_delta[1][threadIdx.x];
        if (v1) atomicAdd(&args.part1_1[(blockIdx.x % kPolReplicas) * kPolPartCols + threadIdx.x], v1);
        if (v2) atomicAdd(&args.part1_2[(blockIdx.x % kPolReplicas) * kPolPartCols + threadIdx.x], v2);
    }
    if (threadIdx.x == 0) {
        args.list_cnt1[blockIdx.x] = s_list_n[0] < args.list_cap ? s_list_n[0] : args.list_cap;
        args.list_cnt2[blockIdx.x] = s_list_n[1] < args.list_cap ? s_list_n[1] : args.list_cap;
    }
}

// The pair's pooling: bags_pool_kernel's shape (d / 4 lanes per bag, UNROLL bags in flight per group, the table id wave-uniform,
// index order, unfused fp32 adds from +0), both codecs' tables in LDS, and per position the decoder its serve byte names -- the
// rows of a bag may come from two tiers, 16 / 8 / 4 / 2 bytes per piece.  The samples' counts are the count pass's; a bag whose
// offsets are out of order pools nothing, as it counted nothing there.
template <int CODEC1, int CODEC2, int UNROLL>
__global__ void __launch_bounds__(256) bags_pool2_kernel(const BagPairArgs args) {
    __shared__ float s_lut1[CodecLut<CODEC1>::kEntries], s_lut2[CodecLut<CODEC2>::kEntries];
    if constexpr (CODEC1 != 32) codec_lut_init<CODEC1>(s_lut1);
    codec_lut_init<CODEC2>(s_lut2);
    __syncthreads();
    const int T = args.T;
    const int LPR = args.d / 4;
    const int RPW = kWave / LPR;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const int slot = lane / LPR;
    const int piece = lane - slot * LPR;
    const bool lane_on = slot < RPW;
    const long long B = args.B;
    const int bags_per_item = RPW * UNROLL;
    const int64_t n_items = (int64_t)T * args.chunks_per_table;
    const XcdRange xr = xcd_range(n_items, 4, wave);

    for (int64_t item = xr.first; item < xr.end; item += xr.stride) {
        const int t = __builtin_amdgcn_readfirstlane((int)(item / args.chunks_per_table));
        const long long chunk = item - (long long)t * args.chunks_per_table;
        const long long b0 = chunk * bags_per_item;
        const long long *__restrict__ off = args.offsets[t];
        const long long nnz = args.pos0[t + 1] - args.pos0[t];
        const long long *__restrict__ ptrs = args.row_ptrs + args.pos0[t];
        const unsigned char *__restrict__ serve = args.serve + args.pos0[t];

        long long s[UNROLL], len[UNROLL];
        long long maxlen = 0;
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const long long b = b0 + (long long)u * RPW + slot;
            s[u] = 0;
            len[u] = 0;
            if (lane_on && b < B) {
                const long long st = off[b];
                const long long en = (b + 1 < B) ? off[b + 1] : nnz;
                if (st >= 0 && en >= st && en <= nnz) {
                    s[u] = st;
                    len[u] = en - st;
                }
            }
            maxlen = len[u] > maxlen ? len[u] : maxlen;
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {   // wave-wide max bag length (all lanes run the same trip count)
            const long long o = __shfl_xor(maxlen, m, kWave);
            maxlen = o > maxlen ? o : maxlen;
        }

        float4 acc[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);

        for (long long j = 0; j < maxlen; j++) {
            const unsigned char *r[UNROLL];
            int sv[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                r[u] = nullptr;
                sv[u] = 0;
                if (j < len[u]) {
                    r[u] = reinterpret_cast<const unsigned char *>(ptrs[s[u] + j]);
                    sv[u] = serve[s[u] + j];
                }
            }
            float4 v[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (r[u] && sv[u] == 1) v[u] = RowPiece<CODEC1>::load(r[u], piece, s_lut1);
                else if (r[u] && sv[u] == 2) v[u] = RowPiece<CODEC2>::load(r[u], piece, s_lut2);
            }
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                if (r[u] && sv[u] != 0) {
                    acc[u].x = __fadd_rn(acc[u].x, v[u].x);
                    acc[u].y = __fadd_rn(acc[u].y, v[u].y);
                    acc[u].z = __fadd_rn(acc[u].z, v[u].z);
                    acc[u].w = __fadd_rn(acc[u].w, v[u].w);
                }
            }
        }

        float *__restrict__ out = args.out + (long long)t * args.out_tstride + (long long)piece * 4;
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const long long b = b0 + (long long)u * RPW + slot;
            if (lane_on && b < B) *reinterpret_cast<float4 *>(out + b * args.out_bstride) = acc[u];
        }
    }
}

// Fetch-first order, behind the update launch: one lane per position.  A position the probe flagged 0 whose index is in range
// is searched again in its set (the same (set, tag + 1) the probe computed; the line sits in L2 / Infinity Cache, the update
// has just touched it) and re-pointed at the arena row of the way that holds its key now.  Re-probing instead of having the
// insert write its way into the miss record: of the copies of a key only the compare-and-swap's winner knows the way, and
// every copy has to be re-pointed.  Nothing writes a way word during this launch, so the plain line read is the tier as the
// update left it.  FLAT: the bag probe's walk over the flat position list, else the (B, T) probe's half-wave per request.
template <bool FLAT>
__global__ void __launch_bounds__(256) sa_repoint_kernel(const RepointArgs args) {
    __shared__ int s_cnt[2];   // positions re-pointed / left on their table
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32], s_pos0[32];
    __shared__ const long long *s_idx[32];
    const int T = args.T;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 32) {
        const bool tab = (int)threadIdx.x < T;
        s_base[threadIdx.x] = args.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = tab ? args.backing_rows[threadIdx.x] : 0;
        if constexpr (FLAT) {
            s_idx[threadIdx.x] = args.indices[threadIdx.x];
            s_pos0[threadIdx.x] = tab ? args.pos0[threadIdx.x] : args.n_pos;
        }
    }
    __syncthreads();
    const SaGeom &g = args.sa;
    const int lane = threadIdx.x & 63;
    int n_in = 0, n_out = 0;   // this wave's totals, kept on lane 0
    auto one = [&](bool on, long long p, int k, long long row) {
        // (on: the position exists; a hit, a bad index and a lane without a position all read set 0 and store nothing)
        const bool want = on && args.hit[p] == 0 && row >= 0 && row < s_rows[k];
        unsigned set = 0u, tag1 = 0u, w = 0u;
        sa_split(g, sa_perm(args.sau, s_base[k] + (want ? (unsigned)row : 0u)), set, tag1);
        if (!want) set = 0u;
        SaLine line;
        sa_load<8>(g, set, line);
        const int way = sa_find<8>(g, line, tag1, w);
        const bool found = want && way >= 0;
        if (found) args.row_ptrs[p] = (long long)(args.arena + (long long)sa_entry(g, set, (unsigned)way, w) * args.row_bytes);
        const unsigned long long fm = __ballot(found), wm = __ballot(want);
        n_in += __popcll(fm); n_out += __popcll(wm & ~fm);
    };
    if constexpr (FLAT) {
        for (int i = 0; i < args.iters; i++) {   // block-uniform trip count (the ballots)
            const long long p = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
            const bool on = p < args.n_pos;
            int k = 0;
#pragma unroll
            for (int step = 16; step >= 1; step >>= 1) k += (on && s_pos0[k + step] <= p) ? step : 0;
            const long long row = on ? s_idx[k][p - s_pos0[k]] : -1;
            one(on, p, k, row);
        }
    } else {
        const int half = lane >> 5, hl = lane & 31;
        const long long req_stride = (long long)gridDim.x * 8;
        for (long long req = (long long)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half; req - half - (threadIdx.x >> 6) * 2 < args.B;
             req += req_stride) {
            const bool on = req < args.B && hl < T;
            const long long p = req * T + hl;
            const long long row = on ? (long long)args.requests[p] : -1;
            one(on, p, hl, row);
        }
    }
    if (lane == 0) {
        if (n_in) atomicAdd(&s_cnt[0], n_in);
        if (n_out) atomicAdd(&s_cnt[1], n_out);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&args.counters[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// ... of a cache with fed tables (evs_cache_policy.h at FedSrc), (B, T) form: the kernel above, and a missed position of a fed
// table that found no way finds its key's slot of the scratch table again (the walk fed_list's compare-and-swap took, read-only
// now) and is pointed at its fed row -- every missed position of a fed table leaves this launch with an address somebody owns.
__global__ void __launch_bounds__(256) sa_repoint_fed_kernel(const RepointArgs args, const FedSrc fs) {
    __shared__ int s_cnt[4];   // positions re-pointed / left in place / missed positions of fed tables / of those served from the fed block
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32];
    const int T = args.T;
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 32) {
        s_base[threadIdx.x] = args.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = (int)threadIdx.x < T ? args.backing_rows[threadIdx.x] : 0;
    }
    __syncthreads();
    const SaGeom &g = args.sa;
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    int n_in = 0, n_out = 0, n_fed = 0, n_blk = 0;   // this wave's totals, kept on lane 0
    bool bad = false;                                // an index out of range: no key, and the sticky flag says so
    const long long req_stride = (long long)gridDim.x * 8;
    for (long long req = (long long)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half; req - half - (threadIdx.x >> 6) * 2 < args.B;
         req += req_stride) {
        const bool on = req < args.B && hl < T;
        const long long p = req * T + hl;
        const long long row = on ? (long long)args.requests[p] : -1;
        const bool in_range = row >= 0 && row < s_rows[hl];
        const bool want = on && args.hit[p] == 0 && in_range;
        bad = bad || (on && !in_range);
        unsigned set = 0u, tag1 = 0u, w = 0u;
        sa_split(g, sa_perm(args.sau, s_base[hl] + (want ? (unsigned)row : 0u)), set, tag1);
        if (!want) set = 0u;
        SaLine line;
        sa_load<8>(g, set, line);
        const int way = sa_find<8>(g, line, tag1, w);
        const bool found = want && way >= 0;
        const bool block = want && !found && ((fs.fed_mask >> hl) & 1u);
        if (found) args.row_ptrs[p] = (long long)(args.arena + (long long)sa_entry(g, set, (unsigned)way, w) * args.row_bytes);
        if (block) {
            const unsigned long long key = ((unsigned long long)(hl + 1) << 32) | (unsigned)row;
            // (fed_list has seen every record the probe wrote, so the key is there; were it not, the position is served the codec's
            //  zero row and the sticky flag says so -- never an address nobody owns)
            const unsigned char *src = fs.zero_row;
            bool lost = true;
            unsigned h = (unsigned)mix64(key) & fs.slot_mask;
            for (unsigned n = 0; n <= fs.slot_mask; n++, h = (h + 1u) & fs.slot_mask) {
                const unsigned long long kk = fs.slot_key[h];
                if (kk == key) { src = fs.fed + (long long)fs.slot_index[h] * fs.stride; lost = false; break; }
                if (kk == 0ull) break;
            }
            bad = bad || lost;
            args.row_ptrs[p] = (long long)src;
        }
        const unsigned long long fm = __ballot(found), wm = __ballot(want);
        n_in += __popcll(fm); n_out += __popcll(wm & ~fm);
        n_fed += __popcll(__ballot(want && ((fs.fed_mask >> hl) & 1u))); n_blk += __popcll(__ballot(block));
    }
    if (bad) atomicOr(fs.err, 1);
    if (lane == 0) {
        if (n_in) atomicAdd(&s_cnt[0], n_in);
        if (n_out) atomicAdd(&s_cnt[1], n_out);
        if (n_fed) atomicAdd(&s_cnt[2], n_fed);
        if (n_blk) atomicAdd(&s_cnt[3], n_blk);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&args.counters[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    if (threadIdx.x >= 2 && threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&fs.counters[threadIdx.x - 2], (unsigned long long)s_cnt[threadIdx.x]);
}

// The fed list (evs_cache_policy.h at FedSrc): block j walks miss list j, a record per lane.  The trip count is block-uniform (the
// ballot); the claim is one compare-and-swap per slot visited -- 0 -> key wins the slot, the key itself means another copy (of this
// or of another block) won it, anything else is another key's slot: next one.  The table has at least twice as many slots as the
// call has positions, so the walk ends.  The wave's claimants take consecutive list indices from ONE add of their number.
__global__ void __launch_bounds__(64) fed_list_kernel(const FedListArgs args) {
    const uint4 *rec = args.miss_rec + (long long)blockIdx.x * args.list_cap;
    int *rec_slot = args.rec_slot + (long long)blockIdx.x * args.list_cap;
    const int n = args.list_cnt[blockIdx.x];
    const int lane = threadIdx.x;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool on = i < n;
        const uint4 r = rec[on ? i : 0];
        const unsigned t = r.y & 0xffu;
        const bool fed = on && ((args.fed_mask >> (t & 31u)) & 1u);
        const unsigned long long key = ((unsigned long long)(t + 1u) << 32) | r.x;
        unsigned h = (unsigned)mix64(key) & args.slot_mask;
        bool claimed = false;
        if (fed) {
            for (;;) {
                const unsigned long long prev = atomicCAS(&args.slot_key[h], 0ull, key);
                if (prev == 0ull) { claimed = true; break; }
                if (prev == key) break;
                h = (h + 1u) & args.slot_mask;
            }
        }
        const unsigned long long cm = __ballot(claimed);
        int base = 0;
        if (lane == 0 && cm) base = atomicAdd(args.n_keys, __popcll(cm));
        base = __shfl(base, 0, 64);
        if (claimed) {
            const int at = base + __popcll(cm & ((1ull << lane) - 1ull));
            args.keys[at] = key;
            args.slot_index[h] = at;
        }
        if (on) rec_slot[i] = fed ? (int)h : -1;
    }
}

// ---- ragged bags over fed backing (evs_cache_fed_begin_bags; evs_cache_policy.h at bags_fed_probe_launch) --------------------
// The probe of a bag begin, all three policies: bags_probe_kernel's walk, flags, addresses and hit totals, a provisional record per
// position whatever the policy (the finish touches / raises and re-points from it: nothing is searched twice, no index is loaded
// again), and NO write to a way word.  LRU / LFU: the per-block miss lists as bags_probe_kernel writes them.  EVLFU: the lists
// wait for the counts (bags_fed_list_kernel); pos_sample is preset to "no bag covers it".
template <bool EVLFU>
__global__ void __launch_bounds__(256) bags_fed_probe_kernel(const BagArgs args) {
    __shared__ int s_hits, s_list_n;
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32], s_pos0[32];
    __shared__ const long long *s_idx[32];
    __shared__ const unsigned char *s_table[32];
    const PolicyArgs &pa = args.p;
    const int T = pa.T;
    if (threadIdx.x == 0) { s_hits = 0; s_list_n = 0; }
    if (threadIdx.x < 32) {
        const bool tab = (int)threadIdx.x < T;
        s_base[threadIdx.x] = pa.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = tab ? pa.backing_rows[threadIdx.x] : 0;
        s_table[threadIdx.x] = pa.backing[threadIdx.x];
        s_idx[threadIdx.x] = args.indices[threadIdx.x];
        s_pos0[threadIdx.x] = tab ? args.pos0[threadIdx.x] : args.n_pos;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    bool bad = false;
    for (int i = 0; i < args.iters; i++) {   // block-uniform trip count (the ballots below)
        const long long p = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
        const bool on = p < args.n_pos;
        int k = 0;
#pragma unroll
        for (int step = 16; step >= 1; step >>= 1) k += (on && s_pos0[k + step] <= p) ? step : 0;
        const long long row = on ? s_idx[k][p - s_pos0[k]] : -1;
        const bool ok = on && row >= 0 && row < s_rows[k];
        bad = bad || (on && !ok);
        PolKey key;
        const bool is_hit = policy_probe_key<false>(pa.sa, pa.sau, pa.lay, pa.cur, ok, s_base[k] + (ok ? (unsigned)row : 0u), key);
        if (on) {
            pa.hit[p] = is_hit ? 1 : 0;
            const unsigned char *src = nullptr;
            if (is_hit) src = pa.arena + (long long)sa_entry(pa.sa, key.set, (unsigned)key.way, key.w) * pa.row_bytes;
            else if (ok) src = s_table[k] + row * pa.row_bytes;   // (a fed table: NULL-based, rewritten by bags_repoint_fed_kernel)
            pa.row_ptrs[p] = (long long)src;
            args.prov[p] = make_uint4((unsigned)row, (unsigned)k, key.set, is_hit ? (0x80000000u | (unsigned)key.way) : (ok ? key.tag1 : 0u));
            if constexpr (EVLFU) args.pos_sample[p] = -1;
        }
        const unsigned long long hm = __ballot(is_hit);
        if (lane == 0 && hm) atomicAdd(&s_hits, __popcll(hm));
        if constexpr (!EVLFU) {   // the wave's misses, packed, behind the block's earlier ones
            const bool is_miss = ok && key.way < 0;
            const unsigned long long mm = __ballot(is_miss);
            int base = 0;
            if (lane == 0 && mm) base = atomicAdd(&s_list_n, __popcll(mm));
            base = __shfl(base, 0, 64);
            if (is_miss) {
                const int at = base + __popcll(mm & ((1ull << lane) - 1ull));
                if (at < pa.list_cap)
                    pa.miss_rec[(long long)blockIdx.x * pa.list_cap + at] = make_uint4((unsigned)row, (unsigned)k, key.set, key.tag1);
            }
        }
    }
    if (bad) atomicOr(args.err, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_hits) atomicAdd(&pa.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + 38], s_hits);
        if constexpr (!EVLFU) pa.list_cnt[blockIdx.x] = s_list_n < pa.list_cap ? s_list_n : pa.list_cap;
    }
}

// EvLFU, behind bags_count_kernel: bags_raise_list_kernel's listing without its raise -- every missed position into the block's
// list with its sample's count (0 when no valid bag covers it), the record cache_batch_sa_list_fed_kernel reads.  The probe's
// grid and walk, so record i of list j is the one fed_list_kernel gives rec_slot[j * list_cap + i].  Writes no way word.
__global__ void __launch_bounds__(256) bags_fed_list_kernel(const BagArgs args) {
    __shared__ int s_list_n;
    const PolicyArgs &pa = args.p;
    if (threadIdx.x == 0) s_list_n = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int i = 0; i < args.iters; i++) {   // block-uniform trip count (the ballot below)
        const long long p = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
        uint4 r = make_uint4(0u, 0u, 0u, 0u);
        int a = 0;
        if (p < args.n_pos) {
            r = args.prov[p];
            const int b = args.pos_sample[p];
            if (b >= 0) a = args.agg[b];
        }
        const bool is_miss = (r.w & 0x80000000u) == 0u && r.w != 0u;
        const unsigned long long mm = __ballot(is_miss);
        int base = 0;
        if (lane == 0 && mm) base = atomicAdd(&s_list_n, __popcll(mm));
        base = __shfl(base, 0, 64);
        if (is_miss) {
            const int at = base + __popcll(mm & ((1ull << lane) - 1ull));
            if (at < pa.list_cap)
                pa.miss_rec[(long long)blockIdx.x * pa.list_cap + at] = make_uint4(r.x, r.y | ((unsigned)a << 8), r.z, r.w);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) pa.list_cnt[blockIdx.x] = s_list_n < pa.list_cap ? s_list_n : pa.list_cap;
}

// First launch of a bag finish: what bags_fed_probe_kernel left undone to the ways it hit.  The tier has not moved since the begin
// (everything else is refused while the call is open), so the way a record names still holds its key.  LRU / LFU: policy_probe_key's
// touch -- a pure function of the word of before the batch, a plain store, once per way and batch.  EVLFU: bags_raise_list_kernel's
// raise to the count of the position's sample, the histogram moves into part1 columns 0 .. T.
template <bool EVLFU>
__global__ void __launch_bounds__(256) bags_fed_hits_kernel(const BagArgs args) {
    __shared__ int s_delta[64];   // priority histogram moves (0 .. T, T <= 32; sized by the word's 6-bit field)
    const PolicyArgs &pa = args.p;
    const SaGeom &g = pa.sa;
    const int T = pa.T;
    if (threadIdx.x < 64) s_delta[threadIdx.x] = 0;
    __syncthreads();
    for (int i = 0; i < args.iters; i++) {
        const long long p = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
        if (p >= args.n_pos) continue;
        const uint4 r = args.prov[p];
        if ((r.w & 0x80000000u) == 0u) continue;
        unsigned *wp = sa_ways_ptr(g, r.z) + (r.w & 7u);
        const unsigned w = *wp;
        if constexpr (EVLFU) {
            const int b = args.pos_sample[p];
            const int a = b >= 0 ? args.agg[b] : 0;
            if (a > 0 && sa_prio(w) < a) {
                const int old = sa_raise(g, wp, w, a);
                if (old >= 0) { atomicSub(&s_delta[old], 1); atomicAdd(&s_delta[a], 1); }
            }
        } else {
            const PolLayout &L = pa.lay;
            if (pol_last(L, w) != pa.cur) {
                const unsigned c = pol_cnt(w);
                *wp = pol_word(L, w & L.tag_mask, pa.cur, c < kPolCntMax ? c + 1u : kPolCntMax, pol_sel(L, w));
            }
        }
    }
    if constexpr (EVLFU) {
        __syncthreads();
        if ((int)threadIdx.x <= T && s_delta[threadIdx.x])
            atomicAdd(&pa.part1[(blockIdx.x % kPolReplicas) * kPolPartCols + threadIdx.x], s_delta[threadIdx.x]);
    }
}

// The flat form of sa_repoint_fed_kernel, behind the fed insert: one lane per position, read from the begin's records as
// bags_repoint2_kernel reads the pair's.  A miss is searched in its set (the (set, tag + 1) the probe computed): found, it is
// pointed at its arena row; a miss of a fed table that found no way finds its key's slot of the scratch table (read-only) and is
// pointed at its fed row, so the NULL-based address the probe computed for it never reaches the pooling; a miss of an addressed
// table that found no way keeps its table address.  Writes no way word, reads no table and no index.
__global__ void __launch_bounds__(256) bags_repoint_fed_kernel(const BagRepointFedArgs args, const FedSrc fs) {
    __shared__ int s_cnt[4];   // positions re-pointed / left in place / missed positions of fed tables / of those served from the fed block
    if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const SaGeom &g = args.sa;
    const int lane = threadIdx.x & 63;
    int n_in = 0, n_out = 0, n_fed = 0, n_blk = 0;   // this wave's totals, kept on lane 0
    bool bad = false;
    for (int i = 0; i < args.iters; i++) {   // block-uniform trip count (the ballots)
        const long long at = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
        const bool on = at < args.n_pos;
        const long long p = on ? at : 0;
        const uint4 r = args.prov[p];
        const bool hit = (r.w & 0x80000000u) != 0u;
        const bool want = on && !hit && r.w != 0u;
        bad = bad || (on && r.w == 0u);   // an index out of range: no key, and the sticky flag says so
        const int k = (int)(r.y & 31u);
        // (a hit, a bad index and a lane without a position all read set 0 and store nothing)
        const unsigned set = want ? r.z : 0u, tag1 = want ? r.w : 0u;
        unsigned w = 0u;
        SaLine line;
        sa_load<8>(g, set, line);
        const int way = sa_find<8>(g, line, tag1, w);
        const bool found = want && way >= 0;
        const bool of_fed = want && ((fs.fed_mask >> k) & 1u);
        const bool block = of_fed && !found;
        if (found) args.row_ptrs[p] = (long long)(args.arena + (long long)sa_entry(g, set, (unsigned)way, w) * args.row_bytes);
        if (block) {
            const unsigned long long key = ((unsigned long long)(k + 1) << 32) | r.x;
            // (fed_list has seen every record of the lists, so the key is there; were it not, the position is served the codec's zero
            //  row and the sticky flag says so -- never an address nobody owns)
            const unsigned char *src = fs.zero_row;
            bool lost = true;
            unsigned h = (unsigned)mix64(key) & fs.slot_mask;
            for (unsigned n = 0; n <= fs.slot_mask; n++, h = (h + 1u) & fs.slot_mask) {
                const unsigned long long kk = fs.slot_key[h];
                if (kk == key) { src = fs.fed + (long long)fs.slot_index[h] * fs.stride; lost = false; break; }
                if (kk == 0ull) break;
            }
            bad = bad || lost;
            args.row_ptrs[p] = (long long)src;
        }
        const unsigned long long fm = __ballot(found), wm = __ballot(want);
        n_in += __popcll(fm); n_out += __popcll(wm & ~fm);
        n_fed += __popcll(__ballot(of_fed)); n_blk += __popcll(__ballot(block));
    }
    if (bad) atomicOr(fs.err, 1);
    if (lane == 0) {
        if (n_in) atomicAdd(&s_cnt[0], n_in);
        if (n_out) atomicAdd(&s_cnt[1], n_out);
        if (n_fed) atomicAdd(&s_cnt[2], n_fed);
        if (n_blk) atomicAdd(&s_cnt[3], n_blk);
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&args.counters[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    if (threadIdx.x >= 2 && threadIdx.x < 4 && s_cnt[threadIdx.x]) atomicAdd(&fs.counters[threadIdx.x - 2], (unsigned long long)s_cnt[threadIdx.x]);
}

// ... of the C1 + C2 pair that shares its set records (the rule: evs_cache_policy.h at Repoint2Args).  The pair keeps one arena
// row per way, so a way this batch hit can have been this batch's victim: a hit position is searched again too, and one whose
// key is gone is pointed at the table row of its tier -- the same bytes.  A position looks at the ways of the tier its serve byte
// names and at no other: the tier's view of the record is picked per lane (the fields the tiers share stay wave-uniform), then
// sa_split / sa_load / sa_find as everywhere.  W: both tiers' way count when the launcher knows it (8: the reference's 1 : 2
// pair), 0: any shared-record geometry.
__device__ __forceinline__ SaGeom sa_geom_of(const SaGeom &g1, const SaGeom &g2, bool second) {
    // (values, not references, on both sides of every choice: a conditional over two lvalues is an lvalue, and reading it is a
    //  per-lane load through the chosen address -- seven vector loads and a round trip in front of the set line)
    auto pick = [second](unsigned a, unsigned b) { return second ? b : a; };
    SaGeom g = g1;   // (tags, nset, the divider and line_words are the pair's)
    g.tag_mask = pick(g1.tag_mask, g2.tag_mask); g.tag_bits = pick(g1.tag_bits, g2.tag_bits);
    g.w_off = pick(g1.w_off, g2.w_off); g.ways = pick(g1.ways, g2.ways);
    g.sub_shift = pick(g1.sub_shift, g2.sub_shift); g.dual = pick(g1.dual, g2.dual);
    g.stamp_mask = pick(g1.stamp_mask, g2.stamp_mask);
    return g;
}
template <int W>
__global__ void __launch_bounds__(256) sa_repoint2_kernel(const Repoint2Args args) {
    __shared__ int s_cnt[3];   // misses re-pointed / misses left on their table / hits whose way the update took
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32];
    __shared__ const unsigned char *s_tab1[32], *s_tab2[32];
    const int T = args.T;
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 32) {
        s_base[threadIdx.x] = args.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = (int)threadIdx.x < T ? args.rows[threadIdx.x] : 0;
        s_tab1[threadIdx.x] = args.backing1[threadIdx.x];
        s_tab2[threadIdx.x] = args.backing2[threadIdx.x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    int n_in = 0, n_out = 0, n_took = 0;   // this wave's totals, kept on lane 0
    const long long req_stride = (long long)gridDim.x * 8;
    for (long long req = (long long)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half; req - half - (threadIdx.x >> 6) * 2 < args.B;
         req += req_stride) {   // block-uniform trip count (the ballots)
        const bool on = req < args.B && hl < T;
        const long long p = on ? req * T + hl : 0;
        // (the three loads go out together, position 0 for a lane without one: no branch and no wait between them)
        const int row_ld = args.requests[p];
        const int d_ld = args.serve[p], code_ld = args.code[p];
        const long long row = on ? (long long)row_ld : -1;
        const int d = on ? d_ld : 0, code = on ? code_ld : 0;
        // (a bad index, serve byte 0 and a lane without a position all read set 0 of C1's ways and store nothing)
        const bool want = (d == 1 || d == 2) && code <= 2 && row >= 0 && row < s_rows[hl];
        if (on && !(row >= 0 && row < s_rows[hl])) atomicOr(args.err, 1);   // (rare: the one atomic of the launch besides the totals)
        const bool second = want && d == 2;
        const SaGeom g = sa_geom_of(args.sa1, args.sa2, second);
        unsigned es = 0u, tag1 = 0u, w = 0u;
        sa_split(g, sa_perm(args.sau, s_base[hl] + (want ? (unsigned)row : 0u)), es, tag1);
        if (!want) es = 0u;
        SaLine line;
        sa_load<W>(g, es, line);
        const int way = sa_find<W>(g, line, tag1, w);
        const bool hit = code != 0;
        const bool in = want && !hit && way >= 0, out = want && !hit && way < 0, took = want && hit && way < 0;
        const int rb1 = args.row_bytes1, rb2 = args.row_bytes2;
        unsigned char *const ar1 = args.arena1, *const ar2 = args.arena2;
        const long long rb = second ? rb2 : rb1;
        if (in) args.row_ptrs[p] = (long long)((second ? ar2 : ar1) + (long long)sa_entry(g, es, (unsigned)way, w) * rb);
        if (took) args.row_ptrs[p] = (long long)((second ? s_tab2[hl] : s_tab1[hl]) + row * rb);
        n_in += __popcll(__ballot(in)); n_out += __popcll(__ballot(out)); n_took += __popcll(__ballot(took));
    }
    if (lane == 0) {
        if (n_in) atomicAdd(&s_cnt[0], n_in);
        if (n_out) atomicAdd(&s_cnt[1], n_out);
        if (n_took) atomicAdd(&s_cnt[2], n_took);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x])
        atomicAdd(&args.counters[(blockIdx.x % kFetchReplicas) * kFetchRowWords + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// ---- fed backing of the fetch-first pair (evs_cache_pair_fed_begin; the chain and the rule: evs_cache_policy.h at PairFedArgs) ----
// First launch of the finish: what cache_batch_probe2_kernel writes and the begin's probe withheld.  A position whose code is 1 / 2
// finds its way again in that tier's ways (the pair has not moved: everything else is refused while the call is open) and raises
// it to the sample's agg_hit -- the number of the sample's codes that are not 0, which is what the probe's ballot counted --, the
// histogram moves into the tier's replica rows; a miss (code 0, a serve byte) routed to C1 on an odd table stamps the route filter.
template <int W>
__global__ void __launch_bounds__(256) pair_fed_hits_kernel(const PairFedArgs args) {
    __shared__ int s_d1[64], s_d2[64];   // priority histogram moves per tier (0 .. T, T <= 32; sized by the word's 6-bit field)
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32];
    const Repoint2Args &a = args.r;
    const int T = a.T;
    if (threadIdx.x < 64) { s_d1[threadIdx.x] = 0; s_d2[threadIdx.x] = 0; }
    if (threadIdx.x < 32) {
        s_base[threadIdx.x] = a.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = (int)threadIdx.x < T ? a.rows[threadIdx.x] : 0;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    const long long req_stride = (long long)gridDim.x * 8;
    for (long long req = (long long)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half; req - half - (threadIdx.x >> 6) * 2 < a.B;
         req += req_stride) {   // block-uniform trip count (the ballot)
        const bool on = req < a.B && hl < T;
        const long long p = on ? req * T + hl : 0;
        const int row_ld = a.requests[p];
        const int d_ld = a.serve[p], code_ld = a.code[p];
        const long long row = on ? (long long)row_ld : -1;
        const bool ok = row >= 0 && row < s_rows[hl];
        const int code = ok ? code_ld : 0, d = ok ? d_ld : 0;
        const bool hit = code == 1 || code == 2;
        const unsigned long long hm = __ballot(hit);
        const int agg = __popc((unsigned)(half ? (hm >> 32) : hm));
        const bool second = hit && code == 2;
        const SaGeom g = sa_geom_of(a.sa1, a.sa2, second);
        unsigned es = 0u, tag1 = 0u, w = 0u;
        sa_split(g, sa_perm(a.sau, s_base[hl] + (hit ? (unsigned)row : 0u)), es, tag1);
        if (!hit) es = 0u;
        SaLine line;
        sa_load<W>(g, es, line);
        const int way = sa_find<W>(g, line, tag1, w);
        if (hit && way >= 0 && sa_prio(w) < agg) {
            const int old = sa_raise(g, sa_ways_ptr(g, es) + way, w, agg);
            if (old >= 0) { int *sd = second ? s_d2 : s_d1; atomicSub(&sd[old & 63], 1); atomicAdd(&sd[agg & 63], 1); }
        }
        if (args.route_filter && ok && code == 0 && d == 1 && (hl & 1)) {
            const unsigned long long key = ((unsigned long long)(hl + 1) << 32) | (unsigned)row;
            args.route_filter[mix64(key) & args.route_mask] = args.route_stamp;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x <= T) {
        const int i = threadIdx.x;
        if (s_d1[i]) atomicAdd(&args.part1_1[(blockIdx.x % kPolReplicas) * kPolPartCols + i], s_d1[i]);
        if (s_d2[i]) atomicAdd(&args.part1_2[(blockIdx.x % kPolReplicas) * kPolPartCols + i], s_d2[i]);
    }
}

// sa_repoint2_kernel for a pair with fed tables: the rule per position is written at PairFedArgs.  A missed position of a fed table
// that found no way -- turned away, or kept by the other tier -- walks its tier's scratch table read-only, as sa_repoint_fed_kernel
// does; a hit position of a fed table whose way this call's update took is pointed at the spill slot the taker wrote for that arena
// entry.  Every index that reaches an address is checked against what the call allocated: a bug serves the zero row (which the
// begin's probe wrote for every missed position of a fed table) and raises the sticky flag; it never stores an address nobody owns.
template <int W>
__global__ void __launch_bounds__(256) sa_repoint2_fed_kernel(const PairFedArgs pargs) {
    __shared__ int s_cnt[6];   // misses re-pointed / left in place / hits whose way the update took / fed misses / from a fed block / from the spill
    __shared__ unsigned s_base[32];
    __shared__ long long s_rows[32];
    __shared__ const unsigned char *s_tab1[32], *s_tab2[32];
    const Repoint2Args &args = pargs.r;
    const int T = args.T;
    if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 32) {
        s_base[threadIdx.x] = args.sau.row_base[threadIdx.x];
        s_rows[threadIdx.x] = (int)threadIdx.x < T ? args.rows[threadIdx.x] : 0;
        s_tab1[threadIdx.x] = args.backing1[threadIdx.x];
        s_tab2[threadIdx.x] = args.backing2[threadIdx.x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, half = lane >> 5, hl = lane & 31;
    int n_in = 0, n_out = 0, n_took = 0, n_fed = 0, n_blk = 0, n_spill = 0;   // this wave's totals, kept on lane 0
    bool bad = false;
    const long long req_stride = (long long)gridDim.x * 8;
    for (long long req = (long long)blockIdx.x * 8 + (threadIdx.x >> 6) * 2 + half; req - half - (threadIdx.x >> 6) * 2 < args.B;
         req += req_stride) {   // block-uniform trip count (the ballots)
        const bool on = req < args.B && hl < T;
        const long long p = on ? req * T + hl : 0;
        const int row_ld = args.requests[p];
        const int d_ld = args.serve[p], code_ld = args.code[p];
        const long long row = on ? (long long)row_ld : -1;
        const int d = on ? d_ld : 0, code = on ? code_ld : 0;
        const bool in_range = row >= 0 && row < s_rows[hl];
        const bool want = (d == 1 || d == 2) && code <= 2 && in_range;
        bad = bad || (on && !in_range);
        const bool second = want && d == 2;
        const SaGeom g = sa_geom_of(args.sa1, args.sa2, second);
        unsigned es = 0u, tag1 = 0u, w = 0u;
        sa_split(g, sa_perm(args.sau, s_base[hl] + (want ? (unsigned)row : 0u)), es, tag1);
        if (!want) es = 0u;
        SaLine line;
        sa_load<W>(g, es, line);
        const int way = sa_find<W>(g, line, tag1, w);
        const bool hit = code != 0;
        const bool fedt = ((pargs.fed_mask >> hl) & 1u) != 0u;
        const bool in = want && !hit && way >= 0, out = want && !hit && way < 0, took = want && hit && way < 0;
        const long long rb = second ? args.row_bytes2 : args.row_bytes1;
        unsigned char *const ar = second ? args.arena2 : args.arena1;
        const unsigned char *const zero = second ? pargs.f2.zero_row : pargs.f1.zero_row;
        if (in) args.row_ptrs[p] = (long long)(ar + (long long)sa_entry(g, es, (unsigned)way, w) * rb);
        bool blk = false, spl = false;
        if (out && fedt) {   // the key's row of tier d's fed block, through tier d's scratch table
            const unsigned char *const fed = second ? pargs.f2.fed : pargs.f1.fed;
            const long long stride = second ? pargs.f2.stride : pargs.f1.stride;
            const unsigned long long *const slot_key = second ? pargs.f2.slot_key : pargs.f1.slot_key;
            const int *const slot_index = second ? pargs.f2.slot_index : pargs.f1.slot_index;
            const unsigned slot_mask = second ? pargs.f2.slot_mask : pargs.f1.slot_mask;
            const unsigned long long key = ((unsigned long long)(hl + 1) << 32) | (unsigned)row;
            const unsigned char *src = zero;
            unsigned h = (unsigned)mix64(key) & slot_mask;
            for (unsigned n = 0; n <= slot_mask; n++, h = (h + 1u) & slot_mask) {
                const unsigned long long kk = slot_key[h];
                if (kk == key) { if (fed) { src = fed + (long long)slot_index[h] * stride; blk = true; } break; }
                if (kk == 0ull) break;
            }
            bad = bad || !blk;
            args.row_ptrs[p] = (long long)src;
        }
        if (took && fedt) {   // the row the way held when the begin hit it: the taker's spill slot
            const unsigned char *const spill = second ? pargs.f2.spill : pargs.f1.spill;
            const int *const spill_of = second ? pargs.f2.spill_of : pargs.f1.spill_of;
            const long long spill_rows = second ? pargs.f2.spill_rows : pargs.f1.spill_rows;
            const long long entries = second ? pargs.f2.entries : pargs.f1.entries;
            const long long off = args.row_ptrs[p] - (long long)ar;
            const long long entry = off >= 0 ? off / rb : -1;
            const unsigned char *src = zero;
            if (entry >= 0 && entry < entries) {
                const long long s = spill_of[entry];
                if (s >= 0 && s < spill_rows) { src = spill + s * rb; spl = true; }
            }
            bad = bad || !spl;
            args.row_ptrs[p] = (long long)src;
        }
        if (took && !fedt) args.row_ptrs[p] = (long long)((second ? s_tab2[hl] : s_tab1[hl]) + row * rb);
        n_in += __popcll(__ballot(in)); n_out += __popcll(__ballot(out)); n_took += __popcll(__ballot(took));
        n_fed += __popcll(__ballot(want && !hit && fedt)); n_blk += __popcll(__ballot(blk)); n_spill += __popcll(__ballot(spl));
    }
    if (bad) atomicOr(args.err, 1);
    if (lane == 0) {
        if (n_in) atomicAdd(&s_cnt[0], n_in);
        if (n_out) atomicAdd(&s_cnt[1], n_out);
        if (n_took) atomicAdd(&s_cnt[2], n_took);
        if (n_fed) atomicAdd(&s_cnt[3], n_fed);
        if (n_blk) atomicAdd(&s_cnt[4], n_blk);
        if (n_spill) atomicAdd(&s_cnt[5], n_spill);
    }
    __syncthreads();
    const int r = (blockIdx.x % kFetchReplicas) * kFetchRowWords;
    if (threadIdx.x < 3 && s_cnt[threadIdx.x]) atomicAdd(&args.counters[r + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
    if (threadIdx.x == 3 && s_cnt[3]) atomicAdd(&pargs.pair_cnt[r + 0], (unsigned long long)s_cnt[3]);
    if (threadIdx.x == 4 && s_cnt[4]) atomicAdd(&pargs.pair_cnt[r + 1], (unsigned long long)s_cnt[4]);
    if (threadIdx.x == 5 && s_cnt[5]) atomicAdd(&pargs.pair_cnt[r + 3], (unsigned long long)s_cnt[5]);
}

// ... and of the pair's bag form (the rule: evs_cache_policy.h at BagRepoint2Args): sa_repoint2_kernel over the flat position
// list, the bag probe's grid and walk.  The probe left (row, table, code, key bit, set, quotient) in prov[p] and the route launch
// the serving tier in serve[p], so a position costs two loads, sa_place in its tier's view of the record and one line request.
template <int W>
__global__ void __launch_bounds__(256) bags_repoint2_kernel(const BagRepoint2Args args) {
    __shared__ int s_cnt[3];   // misses re-pointed / misses left on their table / hits whose way the update took
    __shared__ const unsigned char *s_tab1[32], *s_tab2[32];
    if (threadIdx.x < 3) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 32) {
        s_tab1[threadIdx.x] = args.backing1[threadIdx.x];
        s_tab2[threadIdx.x] = args.backing2[threadIdx.x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    int n_in = 0, n_out = 0, n_took = 0;   // this wave's totals, kept on lane 0
    for (int i = 0; i < args.iters; i++) {   // block-uniform trip count (the ballots)
        const long long at = ((long long)blockIdx.x + (long long)i * gridDim.x) * 256 + threadIdx.x;
        const bool on = at < args.n_pos;
        const long long p = on ? at : 0;
        // (the two loads go out together, position 0 for a lane without one: no branch and no wait between them)
        const uint4 r = args.prov[p];
        const int d_ld = args.serve[p];
        const int d = on ? d_ld : 0;
        const int k = (int)(r.y & 31u);
        const bool hit = ((r.y >> kProvCodeShift) & 3u) != 0u;
        // (a bad index, serve byte 0 and a lane without a position all read set 0 of C1's ways and store nothing)
        const bool want = (d == 1 || d == 2) && (r.y & kProvKey) != 0u;
        const bool second = want && d == 2;
        const SaGeom g = sa_geom_of(args.sa1, args.sa2, second);
        unsigned es = 0u, tag1 = 0u, w = 0u;
        sa_place(g, want ? r.z : 0u, want ? r.w : 0u, es, tag1);
        SaLine line;
        sa_load<W>(g, es, line);
        const int way = sa_find<W>(g, line, tag1, w);
        const bool in = want && !hit && way >= 0, out = want && !hit && way < 0, took = want && hit && way < 0;
        const int rb1 = args.row_bytes1, rb2 = args.row_bytes2;
        unsigned char *const ar1 = args.arena1, *const ar2 = args.arena2;
        const long long rb = second ? rb2 : rb1;
        if (in) args.row_ptrs[p] = (long long)((second ? ar2 : ar1) + (long long)sa_entry(g, es, (unsigned)way, w) * rb);
        if (took) args.row_ptrs[p] = (long long)((second ? s_tab2[k] : s_tab1[k]) + (long long)r.x * rb);
        n_in += __popcll(__ballot(in)); n_out += __popcll(__ballot(out)); n_took += __popcll(__ballot(took));
    }
    if (lane == 0) {
        if (n_in) atomicAdd(&s_cnt[0], n_in);
        if (n_out) atomicAdd(&s_cnt[1], n_out);
        if (n_took) atomicAdd(&s_cnt[2], n_took);
    }
    __syncthreads();
    if (threadIdx.x < 3 && s_cnt[threadIdx.x])
        atomicAdd(&args.counters[(blockIdx.x % kFetchReplicas) * kFetchRowWords + threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

struct NoTail {};
// the piece types of a row as compiler vector types (loads through an address-space-1 pointer want non-class types)
template <typename U> struct Native { using type = U; };
template <> struct Native<float4> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct Native<uint2> { typedef unsigned type __attribute__((ext_vector_type(2))); };
template <> struct Native<NoTail> { using type = int; };

// One missed key into its set.  Issue order: the set line, then the source row (global loads return in order: the ranking
// and the compare-and-swap go out when the line is there, the row -- a random line of a large table -- still on its way),
// then the CAS, then the row stores nobody waits for.  PIECES x U (+ TAIL) = row_bytes; PIECES = 0: any row size, copied
// after the claim.
// FED: fsrc, when not NULL, is the key's row in the caller's fed block and is read instead of the table row.
// HOLD (evs_cache_policy.h at FedHold): the ways the other open calls hold are no candidates, and a copy of the key that another
// call installed (its stamp is not this batch's) is counted.
template <int PIECES, typename U, typename TAIL, bool FED = false, bool HOLD = false>
__device__ __forceinline__ void policy_insert_one(const PolicyArgs &args, const unsigned char *table, unsigned row, unsigned set, unsigned tag1,
                                                  int *s_stat, const unsigned char *fsrc = nullptr, const FedHold *fh = nullptr) {
    const SaGeom &g = args.sa;
    const PolLayout &L = args.lay;
    const unsigned cur = args.cur;
    unsigned *tags = sa_ways_ptr(g, set);
    SaLine line;
    sa_load<8>(g, set, line);
    unsigned held = 0u;
    if constexpr (HOLD) {
        for (int k = 0; k < fh->n_others; k++) held |= fh->others[k][set];
    }
    __builtin_amdgcn_sched_barrier(0);
    const unsigned char *srow = (FED && fsrc) ? fsrc : table + (long long)row * args.row_bytes;
    using NU = typename Native<U>::type;
    using NT = typename Native<TAIL>::type;
    constexpr int NP = PIECES > 0 ? PIECES : 1;
    NU r[NP];
    NT rt{};
    if constexpr (PIECES > 0) {
        typedef const __attribute__((address_space(1))) NU *gsrc_t;
        const gsrc_t gs = reinterpret_cast<gsrc_t>(reinterpret_cast<uintptr_t>(srow));
#pragma unroll
        for (int k = 0; k < PIECES; k++) r[k] = gs[k];
        if constexpr (!std::is_same<TAIL, NoTail>::value) {
            typedef const __attribute__((address_space(1))) NT *gtail_t;
            rt = *reinterpret_cast<gtail_t>(reinterpret_cast<uintptr_t>(srow + PIECES * sizeof(U)));
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    unsigned w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = sa_way_word(line, j);
    const unsigned sbits = pol_stamp_bits(L), smask = pol_stamp_mask(L);
    int way = -1;
    unsigned old_word = 0u;
#pragma unroll 1
    for (int attempt = 0; attempt <= 8; attempt++) {
        // rank: a free way beats everything (lowest index first); else, among the ways batch n has not touched or filled,
        // LRU the largest circular age, LFU the lowest counter and then the largest age; equal keys: the lowest index
        int best = -1;
        bool dup = false;
        unsigned bk = 0u, bw = 0u, dw = 0u;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const bool is_dup = (w[j] & L.tag_mask) == tag1;
            dup = dup || is_dup;
            if constexpr (HOLD) dw = is_dup ? w[j] : dw;
            const unsigned age = (cur - pol_last(L, w[j])) & smask;
            const unsigned score = L.lfu ? (((kPolCntMax - pol_cnt(w[j])) << sbits) | age) : age;   // (< 2^31: 6 + S <= 31 bits under LFU)
            const bool on = age != 0u && !(HOLD && ((held >> j) & 1u));                             // (a free way is never held)
            const unsigned k = w[j] == 0u ? 0xffffffffu : (on ? score : 0u);                        // 0: not eligible (eligible ways have age >= 1)
            const bool cand = k > bk;
            best = cand ? j : best; bk = cand ? k : bk; bw = cand ? w[j] : bw;
        }
        if constexpr (HOLD) {
            if (dup && pol_last(L, dw) != cur) atomicAdd(&fh->counters[1], 1ull);
        }
        if (dup || best < 0) return;   // another copy of the key got there first / every way belongs to this batch (or is held): turned away
        const unsigned prev = atomicCAS(&tags[best], bw, pol_word(L, tag1, cur, 1u, pol_sel(L, bw) ^ 1u));
        if (prev == bw) { way = best; old_word = bw; break; }
#pragma unroll
        for (int j = 0; j < 8; j++) w[j] = j == best ? prev : w[j];
    }
    if (way < 0) return;
    atomicAdd(&s_stat[old_word == 0u ? 0 : 1], 1);
    // (two-copy arena: the new row goes to the copy the victim's word does NOT name, as the word just installed says)
    unsigned char *drow = args.arena + (long long)sa_entry(g, set, (unsigned)way, (pol_sel(L, old_word) ^ 1u) << kSaSelShift) * args.row_bytes;
    if constexpr (PIECES > 0) {
#pragma unroll
        for (int k = 0; k < PIECES; k++) reinterpret_cast<NU *>(drow)[k] = r[k];
        if constexpr (!std::is_same<TAIL, NoTail>::value) *reinterpret_cast<NT *>(drow + PIECES * sizeof(U)) = rt;
    } else {
        for (int c = 0; c < args.row_bytes; c++) drow[c] = srow[c];
    }
}

// K2: block j takes the misses probe block j listed, a record per lane, dealt round-robin over the block's waves
template <int PIECES, typename U, typename TAIL = NoTail>
__global__ void __launch_bounds__(256) policy_insert_kernel(const PolicyArgs args) {
    __shared__ int s_stat[2];   // [0] free ways taken, [1] evictions
    __shared__ const unsigned char *s_table[32];
    if (threadIdx.x < 2) s_stat[threadIdx.x] = 0;
    if (threadIdx.x < 32) s_table[threadIdx.x] = args.backing[threadIdx.x];
    const uint4 *rec = args.miss_rec + (long long)blockIdx.x * args.list_cap;
    const int nw = (int)blockDim.x >> 6;
    const int i0 = ((int)threadIdx.x & 63) * nw + ((int)threadIdx.x >> 6);
    const int n = args.list_cnt[blockIdx.x];
    __syncthreads();
    for (int i = i0; i < n; i += 64 * nw) {
        const uint4 r = rec[i];
        policy_insert_one<PIECES, U, TAIL>(args, s_table[r.y & 31u], r.x, r.z, r.w, s_stat);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int *p = args.part2 + (blockIdx.x % kPolReplicas) * kPolPartCols;
        if (s_stat[0]) { atomicAdd(&p[0], s_stat[0]); atomicAdd(&p[33], s_stat[0]); }   // (column 0: the one histogram bucket = size)
        if (s_stat[1]) atomicAdd(&p[34], s_stat[1]);
    }
}

// ... over lists whose records of fed tables carry a slot (evs_cache_policy.h at FedSrc): their row comes from the fed block
template <int PIECES, typename U, typename TAIL = NoTail>
__global__ void __launch_bounds__(256) policy_insert_fed_kernel(const PolicyArgs args, const FedSrc fs) {
    __shared__ int s_stat[2];
    __shared__ const unsigned char *s_table[32];
    if (threadIdx.x < 2) s_stat[threadIdx.x] = 0;
    if (threadIdx.x < 32) s_table[threadIdx.x] = args.backing[threadIdx.x];
    const uint4 *rec = args.miss_rec + (long long)blockIdx.x * args.list_cap;
    const int *rec_slot = fs.rec_slot + (long long)blockIdx.x * args.list_cap;
    const int nw = (int)blockDim.x >> 6;
    const int i0 = ((int)threadIdx.x & 63) * nw + ((int)threadIdx.x >> 6);
    const int n = args.list_cnt[blockIdx.x];
    __syncthreads();
    for (int i = i0; i < n; i += 64 * nw) {
        const uint4 r = rec[i];
        const int slot = rec_slot[i];
        const unsigned char *fsrc = slot >= 0 ? fs.fed + (long long)fs.slot_index[slot] * fs.stride : nullptr;
        policy_insert_one<PIECES, U, TAIL, true>(args, s_table[r.y & 31u], r.x, r.z, r.w, s_stat, fsrc);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int *p = args.part2 + (blockIdx.x % kPolReplicas) * kPolPartCols;
        if (s_stat[0]) { atomicAdd(&p[0], s_stat[0]); atomicAdd(&p[33], s_stat[0]); }
        if (s_stat[1]) atomicAdd(&p[34], s_stat[1]);
    }
}

// ... while other calls are open on the cache: their held ways are left alone (evs_cache_policy.h at FedHold).  policy_insert_fed_kernel
// line for line but for the HOLD flag and fh -- a change to either is a change to both.  (One body under both kernels was tried: it
// moves the device code of every policy_insert_fed_kernel instantiation, and of fed_probe_kernel likewise, which this unit does
// not allow a new form to do.)
template <int PIECES, typename U, typename TAIL = NoTail>
__global__ void __launch_bounds__(256) policy_insert_fed_hold_kernel(const PolicyArgs args, const FedSrc fs, const FedHold fh) {
    __shared__ int s_stat[2];
    __shared__ const unsigned char *s_table[32];
    if (threadIdx.x < 2) s_stat[threadIdx.x] = 0;
    if (threadIdx.x < 32) s_table[threadIdx.x] = args.backing[threadIdx.x];
    const uint4 *rec = args.miss_rec + (long long)blockIdx.x * args.list_cap;
    const int *rec_slot = fs.rec_slot + (long long)blockIdx.x * args.list_cap;
    const int nw = (int)blockDim.x >> 6;
    const int i0 = ((int)threadIdx.x & 63) * nw + ((int)threadIdx.x >> 6);
    const int n = args.list_cnt[blockIdx.x];
    __syncthreads();
    for (int i = i0; i < n; i += 64 * nw) {
        const uint4 r = rec[i];
        const int slot = rec_slot[i];
        const unsigned char *fsrc = slot >= 0 ? fs.fed + (long long)fs.slot_index[slot] * fs.stride : nullptr;
        policy_insert_one<PIECES, U, TAIL, true, true>(args, s_table[r.y & 31u], r.x, r.z, r.w, s_stat, fsrc, &fh);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int *p = args.part2 + (blockIdx.x % kPolReplicas) * kPolPartCols;
        if (s_stat[0]) { atomicAdd(&p[0], s_stat[0]); atomicAdd(&p[33], s_stat[0]); }
        if (s_stat[1]) atomicAdd(&p[34], s_stat[1]);
    }
}

template <int PIECES, typename U, typename TAIL = NoTail>
void insert_launch_t(const PolicyArgs &a, const FedSrc *f, const FedHold *h, int grid, unsigned threads, hipStream_t st) {
    if (f && h) hipLaunchKernelGGL((policy_insert_fed_hold_kernel<PIECES, U, TAIL>), dim3((unsigned)grid), dim3(threads), 0, st, a, *f, *h);
    else if (f) hipLaunchKernelGGL((policy_insert_fed_kernel<PIECES, U, TAIL>), dim3((unsigned)grid), dim3(threads), 0, st, a, *f);
    else hipLaunchKernelGGL((policy_insert_kernel<PIECES, U, TAIL>), dim3((unsigned)grid), dim3(threads), 0, st, a);
}

}  // namespace

void policy_probe_launch(const PolicyArgs &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(policy_probe_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void bags_probe_launch(const BagArgs &a, int grid, hipStream_t st) {
    if (a.evlfu) hipLaunchKernelGGL(bags_probe_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(bags_probe_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void bags_raise_list_launch(const BagArgs &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(bags_raise_list_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void sa_repoint_launch(const RepointArgs &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(sa_repoint_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void sa_repoint_flat_launch(const RepointArgs &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(sa_repoint_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void sa_repoint2_launch(const Repoint2Args &a, int grid, hipStream_t st) {
    if (a.sa1.ways == 8u && a.sa2.ways == 8u) hipLaunchKernelGGL(sa_repoint2_kernel<8>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(sa_repoint2_kernel<0>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void bags_repoint2_launch(const BagRepoint2Args &a, int grid, hipStream_t st) {
    if (a.sa1.ways == 8u && a.sa2.ways == 8u) hipLaunchKernelGGL(bags_repoint2_kernel<8>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(bags_repoint2_kernel<0>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void pair_fed_hits_launch(const PairFedArgs &a, int grid, hipStream_t st) {
    if (a.r.sa1.ways == 8u && a.r.sa2.ways == 8u) hipLaunchKernelGGL(pair_fed_hits_kernel<8>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(pair_fed_hits_kernel<0>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void sa_repoint2_fed_launch(const PairFedArgs &a, int grid, hipStream_t st) {
    if (a.r.sa1.ways == 8u && a.r.sa2.ways == 8u) hipLaunchKernelGGL(sa_repoint2_fed_kernel<8>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(sa_repoint2_fed_kernel<0>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

template <int CODEC, int UNROLL>
static void bags_pool_launch_t(const BagArgs &args, unsigned blocks, hipStream_t st) {
    if (args.pool_only) hipLaunchKernelGGL((bags_pool_kernel<CODEC, UNROLL, false, false>), dim3(blocks), dim3(256), 0, st, args);
    else if (args.evlfu) hipLaunchKernelGGL((bags_pool_kernel<CODEC, UNROLL, true>), dim3(blocks), dim3(256), 0, st, args);
    else hipLaunchKernelGGL((bags_pool_kernel<CODEC, UNROLL, false>), dim3(blocks), dim3(256), 0, st, args);
}

void bags_pool_launch(const BagArgs &a, int codec, hipStream_t st) {
    constexpr int kUnroll = 4;   // bags in flight per lane group, as the uncached pooling keeps them
    BagArgs args = a;
    const int bags_per_item = (kWave / (a.d / 4)) * kUnroll;
    args.chunks_per_table = (a.p.B + bags_per_item - 1) / bags_per_item;
    const long long n_items = (long long)a.p.T * args.chunks_per_table;
    long long blocks = (n_items + 3) / 4;
    if (blocks > (long long)kNumCu * 8) blocks = (long long)kNumCu * 8;
    blocks = round_up((int)blocks, kNumXcd);
    switch (codec) {
    case 32: bags_pool_launch_t<32, kUnroll>(args, (unsigned)blocks, st); break;
    case 16: bags_pool_launch_t<16, kUnroll>(args, (unsigned)blocks, st); break;
    case 8: bags_pool_launch_t<8, kUnroll>(args, (unsigned)blocks, st); break;
    default: bags_pool_launch_t<4, kUnroll>(args, (unsigned)blocks, st); break;
    }
}

// the lanes per bag follow the call's mean bag length: up to 4 indices a lane per bag (the pair's walk), up to 16 a group of 4,
// beyond that a group of 16
void bags_count_launch(const BagArgs &a, hipStream_t st) {
    const long long n_bags = (long long)a.p.T * a.p.B;
    const int G = a.n_pos <= 4 * n_bags ? 1 : (a.n_pos <= 16 * n_bags ? 4 : 16);
    long long blocks = (n_bags * G + 255) / 256;
    if (blocks > (long long)kNumCu * 8) blocks = (long long)kNumCu * 8;
    if (blocks < 1) blocks = 1;
    switch (G) {
    case 1: hipLaunchKernelGGL(bags_count_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL(bags_count_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, a); break;
    default: hipLaunchKernelGGL(bags_count_kernel<16>, dim3((unsigned)blocks), dim3(256), 0, st, a); break;
    }
}

void bags_probe2_launch(const BagPairArgs &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(bags_probe2_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void bags_count2_launch(const BagPairArgs &a, hipStream_t st) {
    long long blocks = ((long long)a.T * a.B + 255) / 256;
    if (blocks > (long long)kNumCu * 8) blocks = (long long)kNumCu * 8;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(bags_count2_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
}

void bags_route2_launch(const BagPairArgs &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(bags_route2_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
}

// the six pairs of precisions the reference builds (MGR_VARIANTS)
bool bags_pool2_launch(const BagPairArgs &a, int codec1, int codec2, hipStream_t st) {
    constexpr int kUnroll = 4;
    BagPairArgs args = a;
    const int bags_per_item = (kWave / (a.d / 4)) * kUnroll;
    args.chunks_per_table = (a.B + bags_per_item - 1) / bags_per_item;
    const long long n_items = (long long)a.T * args.chunks_per_table;
    long long blocks = (n_items + 3) / 4;
    if (blocks > (long long)kNumCu * 8) blocks = (long long)kNumCu * 8;
    blocks = round_up((int)blocks, kNumXcd);
    const dim3 grid((unsigned)blocks), block(256);
    const int pair = codec1 * 100 + codec2;
    switch (pair) {
    case 3216: hipLaunchKernelGGL((bags_pool2_kernel<32, 16, kUnroll>), grid, block, 0, st, args); break;
    case 3208: hipLaunchKernelGGL((bags_pool2_kernel<32, 8, kUnroll>), grid, block, 0, st, args); break;
    case 3204: hipLaunchKernelGGL((bags_pool2_kernel<32, 4, kUnroll>), grid, block, 0, st, args); break;
    case 1608: hipLaunchKernelGGL((bags_pool2_kernel<16, 8, kUnroll>), grid, block, 0, st, args); break;
    case 1604: hipLaunchKernelGGL((bags_pool2_kernel<16, 4, kUnroll>), grid, block, 0, st, args); break;
    case 804: hipLaunchKernelGGL((bags_pool2_kernel<8, 4, kUnroll>), grid, block, 0, st, args); break;
    default: return false;
    }
    return true;
}

// compiled per row size like the EvLFU update (row_bytes = PIECES pieces of 16 / 8 bytes + a tail); f: the fed form
static void policy_insert_dispatch(const PolicyArgs &a, const FedSrc *f, const FedHold *h, int grid, unsigned threads, hipStream_t st) {
    switch (a.row_bytes) {
    case 144: insert_launch_t<9, float4>(a, f, h, grid, threads, st); break;     // d = 36 fp32
    case 256: insert_launch_t<16, float4>(a, f, h, grid, threads, st); break;    // d = 64 fp32
    case 128: insert_launch_t<8, float4>(a, f, h, grid, threads, st); break;     // d = 32 fp32, d = 64 u16
    case 64: insert_launch_t<4, float4>(a, f, h, grid, threads, st); break;      // d = 16 fp32, d = 32 u16, d = 64 u8
    case 32: insert_launch_t<2, float4>(a, f, h, grid, threads, st); break;
    case 16: insert_launch_t<1, float4>(a, f, h, grid, threads, st); break;
    case 72: insert_launch_t<4, float4, uint2>(a, f, h, grid, threads, st); break;            // d = 36 u16: 4 x 16 + 8
    case 36: insert_launch_t<2, float4, unsigned>(a, f, h, grid, threads, st); break;         // d = 36 u8: 2 x 16 + 4
    case 18: insert_launch_t<1, float4, unsigned short>(a, f, h, grid, threads, st); break;   // d = 36 u4: 16 + 2
    case 8: insert_launch_t<1, uint2>(a, f, h, grid, threads, st); break;
    default: insert_launch_t<0, float4>(a, f, h, grid, threads, st); break;
    }
}
void policy_insert_launch(const PolicyArgs &a, int grid, unsigned threads, hipStream_t st) { policy_insert_dispatch(a, nullptr, nullptr, grid, threads, st); }
void policy_insert_fed_launch(const PolicyArgs &a, const FedSrc &f, int grid, unsigned threads, hipStream_t st) { policy_insert_dispatch(a, &f, nullptr, grid, threads, st); }
void policy_insert_fed_hold_launch(const PolicyArgs &a, const FedSrc &f, const FedHold &h, int grid, unsigned threads, hipStream_t st) {
    policy_insert_dispatch(a, &f, &h, grid, threads, st);
}

void fed_probe_launch(const PolicyArgs &a, bool evlfu, int grid, hipStream_t st) {
    if (evlfu) hipLaunchKernelGGL(fed_probe_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(fed_probe_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void fed_probe_hold_launch(const PolicyArgs &a, const FedHold &h, bool evlfu, int grid, hipStream_t st) {
    if (evlfu) hipLaunchKernelGGL(fed_probe_hold_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, a, h);
    else hipLaunchKernelGGL(fed_probe_hold_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, a, h);
}

void fed_hits_launch(const PolicyArgs &a, bool evlfu, int grid, hipStream_t st) {
    if (evlfu) hipLaunchKernelGGL(fed_hits_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(fed_hits_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void fed_list_launch(const FedListArgs &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(fed_list_kernel, dim3((unsigned)grid), dim3(64), 0, st, a);
}

void sa_repoint_fed_launch(const RepointArgs &a, const FedSrc &f, int grid, hipStream_t st) {
    hipLaunchKernelGGL(sa_repoint_fed_kernel, dim3((unsigned)grid), dim3(256), 0, st, a, f);
}

void bags_fed_probe_launch(const BagArgs &a, int grid, hipStream_t st) {
    if (a.evlfu) hipLaunchKernelGGL(bags_fed_probe_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(bags_fed_probe_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void bags_fed_list_launch(const BagArgs &a, int grid, hipStream_t st) {
    hipLaunchKernelGGL(bags_fed_list_kernel, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void bags_fed_hits_launch(const BagArgs &a, int grid, hipStream_t st) {
    if (a.evlfu) hipLaunchKernelGGL(bags_fed_hits_kernel<true>, dim3((unsigned)grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(bags_fed_hits_kernel<false>, dim3((unsigned)grid), dim3(256), 0, st, a);
}

void bags_repoint_fed_launch(const BagRepointFedArgs &a, const FedSrc &f, int grid, hipStream_t st) {
    hipLaunchKernelGGL(bags_repoint_fed_kernel, dim3((unsigned)grid), dim3(256), 0, st, a, f);
}

}  // namespace evs
