// The small host-side cache of model descriptors behind the lean fused launch (evs_fused_rf_lean.hip): which models have a
// descriptor in device memory, and which slot the next one takes.  Plain C++ -- no HIP -- so that the key, the equality and the
// eviction order can be tested on a machine without a GPU (tests/test_fused_lean_host.py); device memory and the lock are the
// caller's business.
#pragma once
#include <stdint.h>
#include <string.h>

namespace evs {

constexpr int kDescCacheSlots = 8;
constexpr int kDescMaxTables = 32;

// What makes two calls "the same model": the device, the row width, the codec, and the T table addresses with their row counts.
// Row updates (evs_update.hip) write INTO the tables -- addresses and counts stay, so they need no invalidation here.  A model
// that is dropped and another allocated at the same addresses is the same key only if every row count matches as well, and
// then the descriptor's contents are what the new model needs anyway.
struct DescKey {
    int dev = 0, d = 0, codec = 0, T = 0;
    const void *table[kDescMaxTables] = {};
    int64_t n_rows[kDescMaxTables] = {};
    bool operator==(const DescKey &o) const {
        if (dev != o.dev || d != o.d || codec != o.codec || T != o.T) return false;
        for (int k = 0; k < T; k++)
            if (table[k] != o.table[k] || n_rows[k] != o.n_rows[k]) return false;
        return true;
    }
};

// kDescCacheSlots entries, least recently used out.  An entry that a stream capture has used is PINNED: the captured graph
// holds the descriptor's address, so its slot is never handed to another model.
class DescLru {
public:
    // the slot that holds `key` (now the most recently used), or -1
    int find(const DescKey &key) {
        for (int i = 0; i < kDescCacheSlots; i++)
            if (e_[i].used && e_[i].key == key) { e_[i].stamp = ++clock_; return i; }
        return -1;
    }
    // the slot a new key takes: a free one, else the least recently used one that is not pinned; -1: every slot is pinned.
    // *evicts is set when the slot held another model (the caller must wait for launches that may still read it).
    int victim(bool *evicts) const {
        int best = -1;
        for (int i = 0; i < kDescCacheSlots; i++) {
            if (!e_[i].used) { *evicts = false; return i; }
            if (e_[i].pinned) continue;
            if (best < 0 || e_[i].stamp < e_[best].stamp) best = i;
        }
        *evicts = best >= 0;
        return best;
    }
    void put(int slot, const DescKey &key) { e_[slot].used = true; e_[slot].pinned = false; e_[slot].key = key; e_[slot].stamp = ++clock_; }
    void drop(int slot) { e_[slot].used = false; e_[slot].pinned = false; }
    void pin(int slot) { e_[slot].pinned = true; }
    bool pinned(int slot) const { return e_[slot].pinned; }
    bool used(int slot) const { return e_[slot].used; }

private:
    struct Entry { bool used = false, pinned = false; uint64_t stamp = 0; DescKey key; };
    Entry e_[kDescCacheSlots];
    uint64_t clock_ = 0;
};

}  // namespace evs
