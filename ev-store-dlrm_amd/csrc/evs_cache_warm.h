// Warm start of the batched set-associative tier (a tier alone, 8 ways, tables in HBM): the placement plan of a bulk load --
// pure host code, every decision of the load is made here -- and the arguments and launcher of the one kernel that carries a
// plan out (evs_cache_warm.hip).  The contract: include/evstore_hip.h at evs_cache_batch_export / evs_cache_batch_load /
// evs_cache_load_plan; the entry points live beside evs_cache_batch_dump in evs_cache.hip, where the cache object is.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "evs_cache_policy.h"

namespace evs {

constexpr int kWarmVersion = 1;
constexpr int kWarmWays = 8;
// state16 (evs_cache_batch_export): the positions of its fields
enum { kWsVersion = 0, kWsPolicy, kWsCap, kWsTables, kWsDim, kWsCodec, kWsBatch, kWsFlush, kWsEvict, kWsRequests, kWsPerfect, kWsHits,
       kWsStampBits, kWsBagRule, kWsInline, kWsSpare };

// host restatement of sa_perm + sa_split (evs_hash.h) for a tier alone (no sub-sets): key -> (set, tag + 1)
inline void warm_place(const SaUniverse &u, const SaGeom &g, int table0, unsigned row, unsigned &set, unsigned &tag1) {
    unsigned x = u.row_base[table0] + row;
    x = (x * kSaMul1) & u.mask; x ^= x >> u.half;
    x = (x * kSaMul2) & u.mask; x ^= x >> u.half;
    const unsigned q = x / g.nset;
    set = x - q * g.nset;
    tag1 = q + 1u;
}
// the stamp an EvLFU batch writes (evs_cache.hip: a.stamp = n % 0x7ffffffe + 1, reduced by sa_cur_stamp) -- LRU / LFU: n itself
inline unsigned warm_cur(int evlfu, unsigned smask, long long n) {
    return evlfu ? (unsigned)((n % 0x7ffffffe) + 1) & smask : (unsigned)((unsigned long long)n & smask);
}
// S: the width of the batch stamp a way word carries under `policy` (0 EvLFU, 1 LRU, 2 LFU)
inline unsigned warm_stamp_bits(const SaGeom &g, int policy) {
    if (policy == 0) return 26u - g.dual - g.tag_bits;
    return pol_stamp_bits(pol_layout(g, policy == 2));
}
// a way's (score, age) as the export reports them
inline void warm_word_fields(const SaGeom &g, int policy, long long n, unsigned w, long long &score, long long &age) {
    const unsigned smask = (1u << warm_stamp_bits(g, policy)) - 1u;
    if (policy == 0) {
        score = (long long)(w >> kSaPrioShift);
        age = (long long)((warm_cur(1, smask, n) - ((w >> g.tag_bits) & g.stamp_mask)) & smask);
    } else {
        const PolLayout l = pol_layout(g, policy == 2);
        score = policy == 2 ? (long long)pol_cnt(w) : 0;
        age = (long long)((warm_cur(0, smask, n) - pol_last(l, w)) & smask);
    }
}
inline unsigned warm_word(const SaGeom &g, int policy, long long n, unsigned tag1, long long score, long long age) {
    const unsigned smask = (1u << warm_stamp_bits(g, policy)) - 1u;
    const unsigned stamp = (warm_cur(policy == 0, smask, n) - (unsigned)((unsigned long long)age & smask)) & smask;
    if (policy == 0) return tag1 | ((stamp & g.stamp_mask) << g.tag_bits) | ((unsigned)score << kSaPrioShift);
    return pol_word(pol_layout(g, policy == 2), tag1, stamp, (unsigned)score, 0u);
}

// The plan of a load into a tier of geometry (u, g) over tables of n_rows[] rows: the way each entry takes (dest[i] = its
// slot 8 * set + way, -1 = turned away), the word of that way (words[i]) and out4 = [placed, turned away, S, the batch number
// after the load].  -> nullptr, or what is wrong with the input (nothing is to be loaded then; out4 untouched).
inline const char *warm_plan(const SaUniverse &u, const SaGeom &g, int policy, long long cap, int n_tables, const int64_t *n_rows,
                             int64_t n, const int64_t *entries, const int64_t *state16, int strict,
                             int64_t *dest, uint32_t *words, int64_t *out4) {
    const unsigned S = warm_stamp_bits(g, policy);
    const long long n_slots = (long long)g.nset * kWarmWays;
    if (n < 0 || (n > 0 && (!entries || !dest || !words))) return "a negative count or a NULL array";
    if (strict && !state16) return "a strict load needs the exported state";
    if (state16) {
        if (state16[kWsVersion] != kWarmVersion) return "unknown format version";
        if (state16[kWsPolicy] != policy) return "the state was exported from a cache of another policy";
        if (state16[kWsBatch] < 0) return "a negative batch number";
        if (strict && (state16[kWsCap] != cap || state16[kWsTables] != n_tables || state16[kWsStampBits] != (int64_t)S))
            return "a strict load needs the capacity, the table count and the key universe (stamp width) of the exporting cache";
    }
    const long long score_lo = policy == 2 ? 1 : 0, score_hi = policy == 0 ? n_tables : policy == 2 ? (long long)kPolCntMax : 0;
    const long long age_cap = (1ll << S) - 2;
    struct Cand { unsigned set, tag1; long long score, age; unsigned long long key; int64_t i; };
    std::vector<Cand> cs((size_t)n);
    long long n_batch = state16 ? (long long)state16[kWsBatch] : 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t *e = entries + 5 * i;
        if (e[0] < 1 || e[0] > n_tables) return "a table outside 1 .. n_tables";
        if (e[1] < 0 || e[1] >= n_rows[e[0] - 1]) return "a row outside its table";
        if (e[2] < score_lo || e[2] > score_hi) return "a score outside the policy's range";
        if (e[3] < 0) return "a negative age";
        Cand &c = cs[(size_t)i];
        warm_place(u, g, (int)(e[0] - 1), (unsigned)e[1], c.set, c.tag1);
        c.score = e[2]; c.age = strict ? e[3] : std::min<long long>(e[3], age_cap);
        c.key = ((unsigned long long)e[0] << 32) | (unsigned long long)e[1];
        c.i = i;
        if (!state16) n_batch = std::max(n_batch, c.age);
    }
    // (everything below is linear in n and in the slot count: a full-size tier is millions of entries)
    long long placed = 0;
    auto dup_in = [](unsigned *tags, int m) {   // the same tag twice among a set's m candidates = the same key twice
        if (m > 16) { std::sort(tags, tags + m); return std::adjacent_find(tags, tags + m) != tags + m; }
        for (int a = 1; a < m; a++)
            for (int b = 0; b < a; b++)
                if (tags[a] == tags[b]) return true;
        return false;
    };
    if (strict) {
        std::vector<unsigned> tag_at((size_t)n_slots, 0u);   // slot -> tag + 1 of the entry that takes it
        for (int64_t i = 0; i < n; i++) {
            const int64_t slot = entries[5 * i + 4];
            if (slot < 0 || slot >= n_slots || (unsigned)(slot / kWarmWays) != cs[(size_t)i].set) return "a slot outside its key's set";
            if (tag_at[(size_t)slot]) return "two entries in one slot";
            tag_at[(size_t)slot] = cs[(size_t)i].tag1;
            dest[i] = slot;
        }
        for (long long s = 0; s < (long long)g.nset; s++) {
            unsigned t8[kWarmWays]; int m = 0;
            for (int w = 0; w < kWarmWays; w++) if (tag_at[(size_t)(s * kWarmWays + w)]) t8[m++] = tag_at[(size_t)(s * kWarmWays + w)];
            if (dup_in(t8, m)) return "a duplicate key";
        }
        placed = n;
    } else {
        // re-placement: the candidates grouped by set (a counting sort), per set the 8 best of (score descending, age
        // ascending, table, row), ways 0 .. 7 in that order
        std::vector<int64_t> first((size_t)g.nset + 1, 0);
        for (const Cand &c : cs) first[(size_t)c.set + 1]++;
        for (size_t s = 0; s < (size_t)g.nset; s++) first[s + 1] += first[s];
        std::vector<int64_t> order((size_t)n), at(first.begin(), first.end() - 1);
        for (int64_t i = 0; i < n; i++) order[(size_t)at[cs[(size_t)i].set]++] = i;
        std::vector<unsigned> tags;
        for (size_t s = 0; s < (size_t)g.nset; s++) {
            int64_t *lo = order.data() + first[s], *hi = order.data() + first[s + 1];
            tags.clear();
            for (int64_t *p = lo; p < hi; p++) tags.push_back(cs[(size_t)*p].tag1);
            if (dup_in(tags.data(), (int)tags.size())) return "a duplicate key";
            std::sort(lo, hi, [&cs](int64_t a, int64_t b) {
                const Cand &x = cs[(size_t)a], &y = cs[(size_t)b];
                if (x.score != y.score) return x.score > y.score;
                if (x.age != y.age) return x.age < y.age;
                return x.key < y.key;
            });
            for (int64_t *p = lo; p < hi; p++) {
                const int rank = (int)(p - lo);
                dest[*p] = rank < kWarmWays ? (int64_t)s * kWarmWays + rank : -1;
                placed += rank < kWarmWays;
            }
        }
    }
    for (const Cand &c : cs) words[c.i] = dest[c.i] >= 0 ? warm_word(g, policy, n_batch, c.tag1, c.score, c.age) : 0u;
    if (out4) { out4[0] = placed; out4[1] = n - placed; out4[2] = (int64_t)S; out4[3] = n_batch; }
    return nullptr;
}

// One entry of a load as the kernel reads it: the backing row's address (the host folds table pointer and row into it), the
// slot and the way word.  Sorted by slot, every slot at most once.
struct WarmRec { unsigned long long src; unsigned slot, word; };
static_assert(sizeof(WarmRec) == 16, "one 16-byte load per entry");
struct WarmArgs {
    const WarmRec *recs; long long n;
    unsigned *tags;           // the way words of a tier alone: word of slot s at tags[s]
    unsigned char *arena;     // slot s owns row s << dual (copy 0 of a two-copy arena)
    unsigned dual;
    int row_bytes;
};
// one launch: every entry's row table -> arena, then its way word (plain stores; nothing else may touch the tier meanwhile)
void warm_load_launch(const WarmArgs &a, hipStream_t st);

}  // namespace evs
