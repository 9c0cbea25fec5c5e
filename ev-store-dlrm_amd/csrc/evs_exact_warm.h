// Warm start of the EXACT batch-1 engines (the device engine of evs_cache.hip and the host engine of evs_hostcache.hip): the
// state format both share and the one function that checks a state before either engine takes it -- pure host code, no GPU
// call.  The contract: include/evstore_hip.h at evs_cache_exact_export / evs_cache_exact_load / evs_hostcache_export /
// evs_hostcache_load / evs_exact_load_check.
#pragma once
#include <cstdint>
#include <vector>

namespace evs {

constexpr int kExactWarmVersion = 2;   // (1 is the batched tier's state16: evs_cache_warm.h)
// state20: the positions of its fields
enum { kXsVersion = 0, kXsPolicy, kXsCap, kXsTables, kXsDim, kXsCodec, kXsMinC1, kXsNPerfect, kXsLeastFreq, kXsFlush, kXsEvict,
       kXsRequests, kXsPerfectHits, kXsHits, kXsMaxPerfect, kXsFlushN, kXsPerfectMode, kXsSpare0, kXsSpare1, kXsSpare2, kXsCount };

// the scalars a loaded cache starts from: state20's when it is given, else derived from the entries
struct ExactScalars {
    int64_t min_c1 = 0, n_perfect = 0, least_freq = 1;
    int64_t n_flush = 0, n_evict = 0, n_requests = 0, n_perfect_hits = 0, n_hits = 0;
};

// What is wrong with a state for a cache of (policy, capacity, n_tables) over tables of n_rows[] rows, or nullptr.  max_freq:
// the device engine's lfu_max_freq (an LFU frequency indexes its list arrays), 0 = unbounded (the host engine).
inline const char *exact_load_check(int policy, int64_t capacity, int n_tables, const int64_t *n_rows, int64_t n, const int64_t *entries,
                                    const int64_t *state20, int strict, int64_t max_freq) {
    if (policy < 0 || policy > 2 || capacity < 1 || n_tables < 1 || n_tables > 64 || !n_rows) return "a policy, capacity or table count out of range";
    if (n < 0 || (n > 0 && !entries)) return "a negative count or a NULL array";
    if (strict && !state20) return "a strict load needs the exported state";
    if (state20) {
        if (state20[kXsVersion] != kExactWarmVersion) return "unknown format version (the exact engines take version 2)";
        if (state20[kXsPolicy] != policy) return "the state was exported from a cache of another policy";
        if (strict && (state20[kXsCap] != capacity || state20[kXsTables] != n_tables))
            return "a strict load needs the capacity and the table count of the exporting cache";
        // min_C1, n_perfect and least_freq are held to the ranges in which they are safe as array indices and TRUSTED beyond that:
        // they are not functions of the entries.  The reference lets min_C1 and least_freq rest on an empty list (the scan moves
        // on at the next eviction, EvLFU_C1.py:47-52; LFU.py:25-28 steps by one whatever lies above) and recounts n_perfect only at
        // a perfect request or a flush, so an honest export can carry values a cross-check against the runs would refuse.  A
        // made-up value costs what it costs the reference: a wrong flush / eviction moment, or the policy's sticky error.
        if (state20[kXsMinC1] < 0 || state20[kXsMinC1] > n_tables) return "min_C1 outside 0 .. n_tables";
        if (state20[kXsNPerfect] < -(1ll << 31) || state20[kXsNPerfect] >= (1ll << 31)) return "n_perfect out of range";
        if (state20[kXsLeastFreq] < 1 || (policy == 2 && max_freq > 0 && state20[kXsLeastFreq] > max_freq - 1)) return "least_freq out of range";
        for (int k = kXsFlush; k <= kXsHits; k++)
            if (state20[k] < 0) return "a negative counter";
    }
    if (n > capacity) return "more entries than the cache's capacity (a load does not shrink)";
    const int64_t lo = policy == 2 ? 1 : 0;
    const int64_t hi = policy == 0 ? n_tables : policy == 1 ? 0 : (max_freq > 0 ? max_freq - 2 : INT64_MAX);
    // duplicates: an open-address set of the keys, load <= 0.5 (linear in n: a full-size tier is millions of entries)
    uint64_t set_mask = 15;
    while ((int64_t)set_mask + 1 < 2 * n) set_mask = set_mask * 2 + 1;
    std::vector<uint64_t> seen((size_t)set_mask + 1, 0);   // (0 = empty: table ids are 1-based, no key is 0)
    for (int64_t i = 0; i < n; i++) {
        const int64_t *e = entries + 3 * i;
        if (e[1] < 1 || e[1] > n_tables) return "a table outside 1 .. n_tables";
        if (e[2] < 0 || e[2] >= n_rows[e[1] - 1] || e[2] > 0xffffffffll) return "a row outside its table";
        if (e[0] < lo || e[0] > hi) return "a score outside the policy's range";
        if (i > 0 && e[0] < e[-3]) return "scores that go down along the array (every list must be one contiguous run)";
        const uint64_t key = ((uint64_t)e[1] << 32) | (uint64_t)e[2];
        uint64_t x = key * 0x9e3779b97f4a7c15ull;
        x ^= x >> 29;
        for (uint64_t at = x & set_mask;; at = (at + 1) & set_mask) {
            if (!seen[at]) { seen[at] = key; break; }
            if (seen[at] == key) return "a duplicate key";
        }
    }
    return nullptr;
}

// the EvLFU constants of a strict load must be the cache's own
inline const char *exact_constants_check(const int64_t *state20, int64_t max_perfect, int64_t flush_n, int perfect_mode) {
    if (state20[kXsMaxPerfect] != max_perfect || state20[kXsFlushN] != flush_n || state20[kXsPerfectMode] != perfect_mode)
        return "a strict load needs the EvLFU constants (max_perfect, flush_n, perfect_mode) of the exporting cache";
    return nullptr;
}

// entries already checked
inline ExactScalars exact_scalars(int policy, int n_tables, int64_t n, const int64_t *entries, const int64_t *state20) {
    ExactScalars s;
    if (state20) {
        s.min_c1 = state20[kXsMinC1]; s.n_perfect = state20[kXsNPerfect]; s.least_freq = state20[kXsLeastFreq];
        s.n_flush = state20[kXsFlush]; s.n_evict = state20[kXsEvict]; s.n_requests = state20[kXsRequests];
        s.n_perfect_hits = state20[kXsPerfectHits]; s.n_hits = state20[kXsHits];
        return s;
    }
    if (n > 0 && policy == 0) {
        s.min_c1 = entries[0];   // (sorted: the first entry sits in the lowest non-empty bucket)
        for (int64_t i = n - 1; i >= 0 && entries[3 * i] == n_tables; i--) s.n_perfect++;
    }
    if (n > 0 && policy == 2) s.least_freq = entries[0];
    return s;
}

inline void exact_state_fill(int64_t *state20, int policy, int64_t cap, int n_tables, int dim, int codec, const ExactScalars &s,
                             int64_t max_perfect, int64_t flush_n, int perfect_mode) {
    for (int k = 0; k < kXsCount; k++) state20[k] = 0;
    state20[kXsVersion] = kExactWarmVersion; state20[kXsPolicy] = policy; state20[kXsCap] = cap; state20[kXsTables] = n_tables;
    state20[kXsDim] = dim; state20[kXsCodec] = codec; state20[kXsMinC1] = s.min_c1; state20[kXsNPerfect] = s.n_perfect;
    state20[kXsLeastFreq] = s.least_freq; state20[kXsFlush] = s.n_flush; state20[kXsEvict] = s.n_evict; state20[kXsRequests] = s.n_requests;
    state20[kXsPerfectHits] = s.n_perfect_hits; state20[kXsHits] = s.n_hits; state20[kXsMaxPerfect] = max_perfect;
    state20[kXsFlushN] = flush_n; state20[kXsPerfectMode] = perfect_mode;
}

}  // namespace evs
