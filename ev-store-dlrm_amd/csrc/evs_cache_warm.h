// Warm start of the batched set-associative tier (a tier alone, 8 ways, tables in HBM) and of the C1 + C2 pair that shares its
// set records (4 .. 16 ways per tier, C2 possibly two sub-sets): the placement plan of a bulk load -- pure host code, every
// decision of the load is made here -- and the arguments and launchers of the kernels that carry a plan out
// (evs_cache_warm.hip).  The contract: include/evstore_hip.h at evs_cache_batch_export / evs_cache_batch_load /
// evs_cache_load_plan and at evs_cache_pair_export / evs_cache_pair_load / evs_cache_pair_load_plan; the entry points live
// beside evs_cache_batch_dump in evs_cache.hip, where the cache object is.
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

// host restatement of sa_perm + sa_split (evs_hash.h): key -> (effective set, tag + 1); a tier alone has no sub-sets (the
// effective set is the set index, the tag the whole quotient)
inline void warm_place(const SaUniverse &u, const SaGeom &g, int table0, unsigned row, unsigned &es, unsigned &tag1) {
    unsigned x = u.row_base[table0] + row;
    x = (x * kSaMul1) & u.mask; x ^= x >> u.half;
    x = (x * kSaMul2) & u.mask; x ^= x >> u.half;
    const unsigned q = x / g.nset;
    es = ((x - q * g.nset) << g.sub_shift) | (q & ((1u << g.sub_shift) - 1u));
    tag1 = (q >> g.sub_shift) + 1u;
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

// One entry of a plan: its (effective) set and tag in the tier it goes to, what it carries, and i = its row in the caller's list
struct WarmCand { unsigned set, tag1; long long score, age; unsigned long long key; int64_t i, slot; };

// The placement of one tier's candidates into n_sets (effective) sets of `ways` ways: dest[c.i] = effective set * ways + way
// (-1: turned away) and words[c.i] for every candidate, `placed` their count.  strict: every candidate to c.slot, which must
// lie in its set and hold one entry; else per set the `ways` best of (score descending, age ascending, table, row) take ways
// 0 .. ways - 1 in that order.  -> nullptr, or what is wrong.  (Linear in the candidates and the slots: a full-size tier is
// millions of entries.)
inline const char *warm_place_cands(const SaGeom &g, int policy, int ways, long long n_sets, int strict, long long n_batch,
                                    const std::vector<WarmCand> &cs, int64_t *dest, uint32_t *words, long long &placed) {
    const long long n_slots = n_sets * ways;
    const int64_t n = (int64_t)cs.size();
    placed = 0;
    auto dup_in = [](unsigned *tags, int m) {   // the same tag twice among a set's m candidates = the same key twice
        if (m > 16) { std::sort(tags, tags + m); return std::adjacent_find(tags, tags + m) != tags + m; }
        for (int a = 1; a < m; a++)
            for (int b = 0; b < a; b++)
                if (tags[a] == tags[b]) return true;
        return false;
    };
    if (strict) {
        std::vector<unsigned> tag_at((size_t)n_slots, 0u);   // slot -> tag + 1 of the entry that takes it
        for (const WarmCand &c : cs) {
            if (c.slot < 0 || c.slot >= n_slots || (unsigned)(c.slot / ways) != c.set) return "a slot outside its key's set";
            if (tag_at[(size_t)c.slot]) return "two entries in one slot";
            tag_at[(size_t)c.slot] = c.tag1;
            dest[c.i] = c.slot;
        }
        for (long long s = 0; s < n_sets; s++) {
            unsigned tw[kSaMaxWays]; int m = 0;
            for (int w = 0; w < ways; w++) if (tag_at[(size_t)(s * ways + w)]) tw[m++] = tag_at[(size_t)(s * ways + w)];
            if (dup_in(tw, m)) return "a duplicate key";
        }
        placed = n;
    } else {
        // re-placement: the candidates grouped by set (a counting sort), per set the best of (score descending, age
        // ascending, table, row), ways 0 .. ways - 1 in that order
        std::vector<int64_t> first((size_t)n_sets + 1, 0);
        for (const WarmCand &c : cs) first[(size_t)c.set + 1]++;
        for (size_t s = 0; s < (size_t)n_sets; s++) first[s + 1] += first[s];
        std::vector<int64_t> order((size_t)n), at(first.begin(), first.end() - 1);
        for (int64_t k = 0; k < n; k++) order[(size_t)at[cs[(size_t)k].set]++] = k;
        std::vector<unsigned> tags;
        for (size_t s = 0; s < (size_t)n_sets; s++) {
            int64_t *lo = order.data() + first[s], *hi = order.data() + first[s + 1];
            tags.clear();
            for (int64_t *p = lo; p < hi; p++) tags.push_back(cs[(size_t)*p].tag1);
            if (dup_in(tags.data(), (int)tags.size())) return "a duplicate key";
            std::sort(lo, hi, [&cs](int64_t a, int64_t b) {
                const WarmCand &x = cs[(size_t)a], &y = cs[(size_t)b];
                if (x.score != y.score) return x.score > y.score;
                if (x.age != y.age) return x.age < y.age;
                return x.key < y.key;
            });
            for (int64_t *p = lo; p < hi; p++) {
                const int rank = (int)(p - lo);
                dest[cs[(size_t)*p].i] = rank < ways ? (int64_t)s * ways + rank : -1;
                placed += rank < ways;
            }
        }
    }
    for (const WarmCand &c : cs) words[c.i] = dest[c.i] >= 0 ? warm_word(g, policy, n_batch, c.tag1, c.score, c.age) : 0u;
    return nullptr;
}

// The plan of a load into a tier ALONE of geometry (u, g) over tables of n_rows[] rows: the way each entry takes (dest[i] = its
// slot 8 * set + way, -1 = turned away), the word of that way (words[i]) and out4 = [placed, turned away, S, the batch number
// after the load].  -> nullptr, or what is wrong with the input (nothing is to be loaded then; out4 untouched).
inline const char *warm_plan(const SaUniverse &u, const SaGeom &g, int policy, long long cap, int n_tables, const int64_t *n_rows,
                             int64_t n, const int64_t *entries, const int64_t *state16, int strict,
                             int64_t *dest, uint32_t *words, int64_t *out4) {
    const unsigned S = warm_stamp_bits(g, policy);
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
    std::vector<WarmCand> cs((size_t)n);
    long long n_batch = state16 ? (long long)state16[kWsBatch] : 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t *e = entries + 5 * i;
        if (e[0] < 1 || e[0] > n_tables) return "a table outside 1 .. n_tables";
        if (e[1] < 0 || e[1] >= n_rows[e[0] - 1]) return "a row outside its table";
        if (e[2] < score_lo || e[2] > score_hi) return "a score outside the policy's range";
        if (e[3] < 0) return "a negative age";
        WarmCand &c = cs[(size_t)i];
        warm_place(u, g, (int)(e[0] - 1), (unsigned)e[1], c.set, c.tag1);
        c.score = e[2]; c.age = strict ? e[3] : std::min<long long>(e[3], age_cap);
        c.key = ((unsigned long long)e[0] << 32) | (unsigned long long)e[1];
        c.i = i; c.slot = e[4];
        if (!state16) n_batch = std::max(n_batch, c.age);
    }
    long long placed = 0;
    if (const char *why = warm_place_cands(g, policy, kWarmWays, (long long)g.nset, strict, n_batch, cs, dest, words, placed)) return why;
    if (out4) { out4[0] = placed; out4[1] = n - placed; out4[2] = (int64_t)S; out4[3] = n_batch; }
    return nullptr;
}

// ---- the C1 + C2 pair that shares its set records (EvLFU; evs_cache.hip: sa_pair_geometry) ----
constexpr int kWarmPairVersion = 3;   // (1: the single tier's state16, 2: the exact engines' state20)
// state32 (evs_cache_pair_export): [version, n_tables, dim, nset], then one block of kWpBlock words per tier at kWpTier0
enum { kWpVersion = 0, kWpTables, kWpDim, kWpNset, kWpTier0 = 4, kWpBlock = 12 };
enum { kWpCap = 0, kWpCodec, kWpWays, kWpSubs, kWpStampBits, kWpBatch, kWpFlush, kWpEvict, kWpRequests, kWpPerfect, kWpHits, kWpSpare };

// The plan of a load into a pair of geometry (u, g1, g2): entries are rows of 6 -- (tier 1 | 2, table_1based, row, score, age,
// slot) --, a key stays in the tier its row names and each tier is placed by warm_place_cands with its own ways and sub-sets.
// dest[i] = the slot in the entry's tier (effective set * ways + way, -1 = turned away), words[i] its way word, out8 = [placed
// in C1, turned away from C1, S1, placed in C2, turned away from C2, S2, the batch number after the load, 0]; n_batch[2] (may be
// NULL) the batch number per tier.  -> nullptr, or what is wrong with the input (out8 untouched; dest / words may be part
// written: the caller plans into arrays of its own).
inline const char *warm_plan_pair(const SaUniverse &u, const SaGeom &g1, const SaGeom &g2, long long cap1, long long cap2, int n_tables,
                                  const int64_t *n_rows1, const int64_t *n_rows2, int64_t n, const int64_t *entries,
                                  const int64_t *state32, int strict, int64_t *dest, uint32_t *words, int64_t *out8, long long *n_batch_out) {
    const SaGeom *g[2] = {&g1, &g2};
    const long long cap[2] = {cap1, cap2};
    const int64_t *n_rows[2] = {n_rows1, n_rows2};
    unsigned S[2];
    long long n_batch[2] = {0, 0};
    if (n < 0 || (n > 0 && (!entries || !dest || !words))) return "a negative count or a NULL array";
    if (strict && !state32) return "a strict load needs the exported state";
    for (int k = 0; k < 2; k++) S[k] = warm_stamp_bits(*g[k], 0);
    if (state32) {
        if (state32[kWpVersion] != kWarmPairVersion) return "unknown format version (the pair's state is version 3)";
        for (int k = 0; k < 2; k++) {
            const int64_t *b = state32 + kWpTier0 + k * kWpBlock;
            if (b[kWpBatch] < 0) return "a negative batch number";
            n_batch[k] = (long long)b[kWpBatch];
            if (strict && (state32[kWpTables] != n_tables || state32[kWpNset] != (int64_t)g[k]->nset || b[kWpCap] != cap[k] ||
                           b[kWpWays] != (int64_t)g[k]->ways || b[kWpSubs] != (int64_t)(1u << g[k]->sub_shift) || b[kWpStampBits] != (int64_t)S[k]))
                return "a strict load needs the capacities, the table count and the geometry (sets, ways, sub-sets, stamp width) of the exporting pair";
        }
    }
    std::vector<WarmCand> cs[2];
    std::vector<unsigned> gid[2];
    for (int k = 0; k < 2; k++) { cs[k].reserve((size_t)n); gid[k].reserve((size_t)n); }
    long long age_max = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t *e = entries + 6 * i;
        if (e[0] < 1 || e[0] > 2) return "a tier outside {1, 2}";
        const int k = (int)e[0] - 1;
        if (e[1] < 1 || e[1] > n_tables) return "a table outside 1 .. n_tables";
        if (e[2] < 0 || e[2] >= n_rows[k][e[1] - 1]) return "a row outside its tier's table";
        if (e[3] < 0 || e[3] > n_tables) return "a score outside 0 .. n_tables";
        if (e[4] < 0) return "a negative age";
        WarmCand c;
        warm_place(u, *g[k], (int)(e[1] - 1), (unsigned)e[2], c.set, c.tag1);
        c.score = e[3]; c.age = strict ? e[4] : std::min<long long>(e[4], (1ll << S[k]) - 2);
        c.key = ((unsigned long long)e[1] << 32) | (unsigned long long)e[2];
        c.i = i; c.slot = e[5];
        age_max = std::max(age_max, c.age);
        cs[k].push_back(c);
        gid[k].push_back(u.row_base[e[1] - 1] + (unsigned)e[2]);
    }
    if (!state32) n_batch[0] = n_batch[1] = age_max;   // the same n for both tiers
    long long placed[2] = {0, 0};
    for (int k = 0; k < 2; k++)
        if (const char *why = warm_place_cands(*g[k], 0, (int)g[k]->ways, (long long)g[k]->nset << g[k]->sub_shift, strict, n_batch[k], cs[k],
                                               dest, words, placed[k]))
            return why;
    // no key lives in both tiers: one bit per dense row number where the universe allows it (the Kaggle tables: 4 MB), else C1's
    // numbers sorted and C2's looked up
    const unsigned long long n_gid = (unsigned long long)u.row_base[n_tables - 1] + (unsigned long long)std::max(n_rows1[n_tables - 1], n_rows2[n_tables - 1]);
    if (n_gid <= (1ull << 30)) {
        std::vector<unsigned long long> bits((size_t)((n_gid + 63) / 64), 0ull);
        for (unsigned x : gid[0]) bits[x >> 6] |= 1ull << (x & 63u);
        for (unsigned x : gid[1])
            if (bits[x >> 6] >> (x & 63u) & 1ull) return "a key in both tiers";
    } else {
        std::sort(gid[0].begin(), gid[0].end());
        for (unsigned x : gid[1])
            if (std::binary_search(gid[0].begin(), gid[0].end(), x)) return "a key in both tiers";
    }
    if (out8) {
        out8[0] = placed[0]; out8[1] = (int64_t)cs[0].size() - placed[0]; out8[2] = (int64_t)S[0];
        out8[3] = placed[1]; out8[4] = (int64_t)cs[1].size() - placed[1]; out8[5] = (int64_t)S[1];
        out8[6] = n_batch[0]; out8[7] = 0;
    }
    if (n_batch_out) { n_batch_out[0] = n_batch[0]; n_batch_out[1] = n_batch[1]; }
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

// The pair form: ONE list, C1's n1 records (sorted by slot) and then C2's n2, ONE launch whose blocks are split between the
// tiers in proportion to their counts.  A tier's view by value: slot s = effective set * ways + way owns arena row s (a pair
// keeps one row per way) and the word record * line_words + w_off + sub * ways + way of the shared records.
struct WarmTier {
    unsigned char *arena;
    int row_bytes;
    unsigned ways, w_off, line_words, sub_shift;
    long long n_slots;        // the tier's slot count (the launcher refuses a list it cannot check against)
};
struct WarmPairArgs {
    const WarmRec *recs; long long n1, n2;
    unsigned *tags;           // the shared set records
    WarmTier t1, t2;
    unsigned blocks1;         // blocks [0, blocks1) place C1's records, the rest C2's (set by the launcher)
};
void warm_load_pair_launch(WarmPairArgs a, hipStream_t st);

}  // namespace evs
