// Batched LRU and LFU on the set-associative tier (batch policy 2 of an LRU / LFU cache): the way-word layout above the tag,
// the arguments of the two kernels (evs_cache_policy.hip) and their launchers.  The rule the kernels implement is written
// down in include/evstore_hip.h (evs_cache_set_batch_policy, "the batched rule"); the set geometry, the key permutation, the
// tag field and the copy-select bit are evs_hash.h's, so sa_lookup, the dump and the row updates read such a tier unchanged.
#pragma once
#include "evs_hash.h"

namespace evs {

// The bits of a way word above the tag.  evs_hash.h splits them into a low field [25 - dual : tag_bits] (EvLFU: the stamp of
// the batch that filled the way) and a high field [31 : 26] (EvLFU: the priority); bit 25 of a two-copy arena is `sel`.
//   LFU: high field = the saturating counter (6 bits, 1..63), low field = `last`, the batch that touched the way last:
//        S = 26 - dual - tag_bits stamp bits;
//   LRU: no counter -- the high field holds the HIGH bits of `last`, the low field its low bits: S = 32 - dual - tag_bits.
// `last` is the batch number modulo 2^S; ages are circular: age = (n - last) mod 2^S, 0 = touched or filled by batch n.
struct PolLayout {
    unsigned tag_bits, tag_mask;
    unsigned low_bits, low_mask;   // the low field
    unsigned dual;                 // 1: bit 25 is the copy-select bit
    unsigned lfu;                  // 1: LFU (counter in the high field), 0: LRU
};
constexpr unsigned kPolCntMax = 63u;
__host__ __device__ inline PolLayout pol_layout(const SaGeom &g, int lfu) {
    PolLayout l;
    l.tag_bits = g.tag_bits; l.tag_mask = g.tag_mask;
    l.low_bits = 26u - g.dual - g.tag_bits; l.low_mask = g.stamp_mask;
    l.dual = g.dual; l.lfu = lfu ? 1u : 0u;
    return l;
}
__host__ __device__ inline unsigned pol_stamp_bits(const PolLayout &l) { return l.low_bits + (l.lfu ? 0u : 6u); }
__host__ __device__ inline unsigned pol_stamp_mask(const PolLayout &l) { return (1u << pol_stamp_bits(l)) - 1u; }   // (S <= 31: tag_bits >= 1)
__host__ __device__ inline unsigned pol_last(const PolLayout &l, unsigned w) {
    const unsigned lo = (w >> l.tag_bits) & l.low_mask;
    return l.lfu ? lo : (lo | ((w >> kSaPrioShift) << l.low_bits));
}
__host__ __device__ inline unsigned pol_cnt(unsigned w) { return w >> kSaPrioShift; }   // LFU only
__host__ __device__ inline unsigned pol_sel(const PolLayout &l, unsigned w) { return (w >> kSaSelShift) & l.dual; }
// last: already reduced modulo 2^S
__host__ __device__ inline unsigned pol_word(const PolLayout &l, unsigned tag1, unsigned last, unsigned cnt, unsigned sel) {
    const unsigned hi = l.lfu ? cnt : (last >> l.low_bits);
    return tag1 | ((last & l.low_mask) << l.tag_bits) | ((sel & l.dual) << kSaSelShift) | (hi << kSaPrioShift);
}
__host__ __device__ inline unsigned pol_age(const PolLayout &l, unsigned cur, unsigned w) { return (cur - pol_last(l, w)) & pol_stamp_mask(l); }

// the replica rows the batch kernels add their totals into (evs_cache.hip owns the buffers and folds them: sampled_close_block)
constexpr int kPolPartCols = 40;   // 0 resident-entry delta, 33 free ways taken, 34 evictions, 38 hits, 39 all-hit requests
constexpr int kPolReplicas = 32;

struct PolicyArgs {
    SaGeom sa; SaUniverse sau;
    PolLayout lay;
    unsigned cur;                          // this batch's number modulo 2^S
    const int *requests;                   // (B,T) int32 row ids
    unsigned char *hit;                    // (B,T) out
    long long *row_ptrs;                   // (B,T) out: address of each key's row (arena / table / 0) ...
    int *row_ids;                          // ... or, when not NULL: bit 30 | arena entry, else the table row, -1 = none
    uint4 *miss_rec; int *list_cnt; int list_cap;   // per probe block: its misses as (row, table, set, tag + 1), their number
    int *part1, *part2;
    const unsigned char *backing[32];
    long long backing_rows[32];
    unsigned char *arena;
    long long B;
    int T, row_bytes;
};

// probe + touch: grid blocks of 256 threads, block j walks requests 8 j, 8 (j + grid), ...; writes miss list j
void policy_probe_launch(const PolicyArgs &a, int grid, hipStream_t st);
// insert: block j (`threads` = 64 or 128) takes miss list j
void policy_insert_launch(const PolicyArgs &a, int grid, unsigned threads, hipStream_t st);

// Ragged bags through the same tier (evs_cache_lookup_bags): a lookup is one POSITION of one table's index array, the
// positions of all tables numbered table-major (table k's start at pos0[k]).  `p` is used as above except for requests / B / T
// semantics: p.hit and p.row_ptrs are flat arrays of n_pos entries, p.row_ids is NULL, p.B the number of samples.
struct BagArgs {
    PolicyArgs p;
    const long long *indices[32];          // per table: nnz[k] int64 row ids
    const long long *offsets[32];          // per table: B bag starts (the last bag runs to nnz[k])
    long long pos0[33];                    // prefix sums of nnz; pos0[T] = n_pos
    long long n_pos;
    int iters;                             // probe: block j walks positions 256 (j + i grid) + thread, i < iters
    int *err;                              // the sticky index-error flag
    // pooling
    float *out; long long out_tstride, out_bstride;
    const unsigned char *arena_end;        // a row address in [p.arena, arena_end) is a hit
    int *sample_cnt;                       // B words, zero between launches: bags seen | bags with a lookup << 8 | bags with a miss << 16
    long long chunks_per_table;
    int d;
    // EvLFU under the "served bags" rule (evlfu != 0; include/evstore_hip.h at evs_cache_lookup_bags): p.sa / p.sau are used as
    // above, p.lay and p.cur are not (the way words are evs_hash.h's: priority | filling batch | tag).  A sample's count is known
    // only when all its bags have been judged, so the probe leaves a provisional record per position, the pooling writes the
    // counts and the position -> sample map, and a third launch raises the hit ways and lists the misses:
    int evlfu;
    uint4 *prov;                           // n_pos records: (row, table, set, bit 31 | hit way -- or tag + 1 of a miss -- or 0: no key)
    int *pos_sample;                       // n_pos words: the sample whose bag covers the position (-1: no valid bag does)
    int *agg;                              // B words: the sample's served bags (0 .. T)
    // fetch-first order (evs_cache_set_miss_order): the update has re-pointed the installed misses at the arena before the
    // pooling runs, so "this position was a hit" comes from the probe's flags (not NULL) instead of the address range
    const unsigned char *pool_flags;
    // EvLFU "count first" (evs_cache_set_bag_count(c, 1)): bags_count_launch has judged every sample in front of the pooling,
    // which then only pools -- no sample_cnt hand-over, no agg / pos_sample write, no column-39 add, no look at a flag
    int pool_only;
};
// probe over the flat position list: grid blocks of 256 threads, one lane per position.  LRU / LFU: probe + touch, writes miss
// list j (records as above).  EvLFU: no way word is written; writes prov and presets pos_sample to -1
void bags_probe_launch(const BagArgs &a, int grid, hipStream_t st);
// pooled[k][b] = sum over the bag's positions of the rows the probe's pointer table names (d % 4 == 0, d <= 256); counts the
// all-hit samples into column 39.  EvLFU: also agg and pos_sample.  pool_only: the pooled rows and the sticky flag, nothing else
void bags_pool_launch(const BagArgs &a, int codec, hipStream_t st);
// EvLFU "count first", between the probe and whatever needs a sample's count: a group of 1 / 4 / 16 lanes per bag (by the call's
// mean bag length) walks the bag's flag bytes (p.hit, as the probe wrote them) -- no row is touched -- and writes pos_sample,
// agg[b] = the sample's served bags and the all-served samples with a lookup into column 39; sample_cnt is zero again behind it
void bags_count_launch(const BagArgs &a, hipStream_t st);
// EvLFU, behind the pooling: one lane per position (the probe's grid) -- every hit way to max(old, agg of the position's
// sample) with the histogram moves into part1 columns 0 .. T, every miss into list j as (row, table | agg << 8, set, tag + 1),
// the record cache_batch_sa_list_kernel (evs_cache.hip) reads
void bags_raise_list_launch(const BagArgs &a, int grid, hipStream_t st);

// Ragged bags through the C1 + C2 pair that shares its set records (evs_cache_lookup_bags_c1c2; the rule: include/evstore_hip.h
// there).  Positions are numbered as above.  Where a missed position is served from depends on its sample's agg_hit, and one bag
// can mix rows of two precisions, so the chain is  probe2 -> count -> route + raise + list -> pool2 (-> dense interaction) -> the
// pair's update:
//   prov[p]   the probe's record of position p: x = row, y = table | hit way << 8 | tier code << 12 | "the key's C1 set has a free
//             way" << 14 | "a key" << 15, z = the set index, w = the quotient -- (set, quotient) place the key in either tier
//             (sa_place), so nothing is searched or divided twice
//   code[p]   1 = resident in C1, 2 = in C2, 0 = neither (or no key)
//   serve[p]  the tier whose codec decodes the row row_ptrs[p] names: the code of a hit, the destination of a miss, 0 = no row
struct BagPairArgs {
    SaGeom sa1, sa2; SaUniverse sau;
    const long long *indices[32];
    const long long *offsets[32];
    long long pos0[33];
    long long rows[32];                    // per table: min of the two tiers' row counts (an index past either is no key)
    const unsigned char *backing1[32], *backing2[32];
    unsigned char *arena1, *arena2;
    int row_bytes1, row_bytes2;
    long long n_pos, B;
    int iters, T, d, threshold;
    int *err;
    unsigned char *code, *serve;
    long long *row_ptrs;
    uint4 *prov;
    int *pos_sample, *agg, *sample_cnt;    // as BagArgs has them
    uint4 *miss_rec1, *miss_rec2; int *list_cnt1, *list_cnt2; int list_cap;   // per route block and tier: (row, table | agg << 8, effective set, tag + 1)
    int *part1_1, *part1_2;                // replica rows: columns 0 .. T histogram moves, 38 hits (per tier), 39 all-served samples (C1's)
    unsigned *route_filter; unsigned route_mask, route_stamp;
    float *out; long long out_tstride, out_bstride;
    long long chunks_per_table;
};
// one lane per position (grid blocks of 256 threads, block j walks positions 256 (j + i grid) + thread, i < iters): one read of the
// shared record finds both tiers' ways; writes code, serve and row_ptrs of the hits, prov, pos_sample = -1.  Writes no way word
void bags_probe2_launch(const BagPairArgs &a, int grid, hipStream_t st);
// one lane per bag over the code bytes alone: pos_sample, agg[b] = the sample's served bags, the all-served samples into column 39
void bags_count2_launch(const BagPairArgs &a, hipStream_t st);
// one lane per position (the probe's grid): a miss gets its destination tier, its table address and its serve byte, is stamped
// into the route filter (odd tables routed to C1) and listed for its tier in list j; a hit way goes to max(old, agg)
void bags_route2_launch(const BagPairArgs &a, int grid, hipStream_t st);
// pooled[k][b]: bags_pool_launch's shape, every position decoded by the codec its serve byte names.  false: no kernel for the pair
bool bags_pool2_launch(const BagPairArgs &a, int codec1, int codec2, hipStream_t st);

// Fetch-first order (evs_cache_set_miss_order(c, 1); the chain: evs_cache.hip, cache_batch_impl): behind the policy update, every
// position the probe flagged 0 is searched again in its set -- the line the update touched a moment ago -- and, where the key
// got a way, its slot of the pointer table is re-pointed from the table row at the arena row.  A key that was turned away
// (its set took 8 new keys in this batch) keeps the table address the probe wrote.  An index out of range is no key.  Writes
// no way word, reads no table.  counters: [0] positions re-pointed, [1] positions left on their table (one add per block each).
struct RepointArgs {
    SaGeom sa; SaUniverse sau;
    const int *requests;                   // (B, T) form: int32 row ids ...
    const long long *indices[32];          // ... flat form: per table its int64 row ids, the positions table-major from pos0[]
    long long pos0[33];
    long long backing_rows[32];
    const unsigned char *hit;              // the probe's flags, one per position
    long long *row_ptrs;                   // the pointer table, one slot per position
    unsigned char *arena;
    unsigned long long *counters;
    long long B, n_pos;
    int T, row_bytes, iters;
};
// (B, T) form: the probe's grid and walk (block j: requests 8 j, 8 (j + grid), ...; a half-wave per request, a lane per key)
void sa_repoint_launch(const RepointArgs &a, int grid, hipStream_t st);
// flat form: the bag probe's grid and walk (block j: positions 256 (j + i grid) + thread, i < iters)
void sa_repoint_flat_launch(const RepointArgs &a, int grid, hipStream_t st);

// Fed backing (evs_cache_set_fed_backing; the contract: include/evstore_hip.h at evs_cache_fed_begin): a table in fed_mask has no
// address the GPU reads -- the rows of its missing keys come from the caller, between the probe and the update.  The chain is the
// fetch-first chain cut in two:  (flush ->) probe -> fed_list | the caller fetches | update (fed form) -> sa_repoint (fed form) ->
// consumers -> close.  The begin writes no way word: a call that is dropped (evs_cache_fed_abort) leaves the tier as it found it.
//   fed_probe  K1 of either producer (flags, addresses, miss lists, hit totals) without the LRU / LFU touch and without EvLFU's
//              raise; fed_hits, first launch of the finish, touches / raises the ways of the positions the begin flagged 1.
//   fed_list   walks the probe's per-block miss lists.  A record of a fed table is looked up in a scratch open-address table of
//              64-bit keys (table_1based << 32 | row; a power of two >= 2 x positions, zero at the start of the launch): ONE
//              compare-and-swap claims a slot, the claimant takes the next list index (the appends of a wave are one add of its
//              claimant count), writes the key at keys[index] and stores the index at slot_index[slot]; every record -- claimant or
//              not -- stores its slot at rec_slot[record].  A record of an addressed table gets -1.  Nobody READS slot_index in this
//              launch: the update and the re-point run in later launches, so a key's index is visible to all its copies by then.
//   update     a record with a slot copies its row from fed + slot_index[slot] * stride instead of from the table.
//   re-point   a missed position of a fed table that found no way (its set took 8 new keys) finds its key's slot again and is
//              pointed at its fed row; every missed position of a fed table is rewritten, so the NULL-based address the probe
//              computed for it never reaches a consumer.
struct FedSrc {
    const unsigned char *fed; long long stride;   // row i of the fed block, in the cache's codec
    const int *rec_slot;                          // per miss record (list j from j * list_cap): its slot, -1 = an addressed table
    const int *slot_index;                        // per slot: the list index of the key that claimed it
    const unsigned long long *slot_key;           // the scratch table
    unsigned slot_mask, fed_mask;                 // slots - 1; bit t: table t is fed
    unsigned long long *counters;                 // re-point: [0] missed positions of fed tables, [1] of those served from the fed block
    int *err;                                     // re-point: the sticky index-error flag, raised for an index out of range
    const unsigned char *zero_row;                // re-point: what a position is served whose key the scratch table does not hold (never: see there)
    // a tier of the fed C1 + C2 pair (PairFedArgs below), NULL / 0 for a tier alone: the spill block (a row slot per miss record),
    // spill_of (an int32 per arena entry: the slot its last victim's row went to) and the replica rows of the pair's totals
    unsigned char *spill; int *spill_of;
    unsigned long long *pair_cnt;
    long long spill_rows, entries;                // slots of the spill block, arena entries of the tier (the re-point's bounds)
};
struct FedListArgs {
    const uint4 *miss_rec; const int *list_cnt; int list_cap;   // the probe's lists (either producer: row, table | .. << 8, set, tag + 1)
    unsigned long long *slot_key; int *slot_index; int *rec_slot;
    unsigned slot_mask, fed_mask;
    unsigned long long *keys;                     // out: the fed list
    int *n_keys;                                  // its length (zero at the start of the launch)
};
// the begin's probe (policy_probe_launch's grid and walk) and the finish's touch / raise of the begin's hits; `a` as
// policy_probe_launch takes it (EvLFU: lay and cur unused; fed_hits adds the histogram moves into a.part1)
void fed_probe_launch(const PolicyArgs &a, bool evlfu, int grid, hipStream_t st);
void fed_hits_launch(const PolicyArgs &a, bool evlfu, int grid, hipStream_t st);
// block j (64 threads) takes miss list j
void fed_list_launch(const FedListArgs &a, int grid, hipStream_t st);
// the LRU / LFU insert over lists whose fed records read the fed block (policy_insert_launch's grid and threads)
void policy_insert_fed_launch(const PolicyArgs &a, const FedSrc &f, int grid, unsigned threads, hipStream_t st);
// sa_repoint_launch's (B, T) form for a cache with fed tables
void sa_repoint_fed_launch(const RepointArgs &a, const FedSrc &f, int grid, hipStream_t st);

// Several (B, T) calls of a fed cache open at once (evs_cache_set_fed_depth; the contract: include/evstore_hip.h there).  A call
// that begins while another is open probes a tier the older calls' updates will still move, so every way it flags 1 is HELD until
// it ends: one byte per set in a map of the call's own (bit j = way j; zeroed in front of the probe), set by the probe's hold
// form, read by the hold form of every update that runs while the call is open.  A held way is no candidate there; a set without
// a candidate turns the key away ("left in place": the position is served from the fed block).  No way word is written for a
// hold, so dropping the call is still free: the host stops passing its map.
//   probe, hold form   fed_probe plus, per position flagged 1, the bit: a plain load of the aligned 32-bit word that contains the
//                      set's byte first, an atomicOr only where the bit is still clear (hot keys would queue on one word)
//   update, hold form  the set's hold bytes of the other open calls (up to kFedMaxDepth - 1) are loaded next to the set's line;
//                      the duplicate branch ("another copy got there first") counts a copy whose stamp is not this call's: the
//                      key was missed by this call's probe and installed by a call that finished in between
// counters: [0] hold bits set (one add per probe block), [1] miss records found installed by an earlier call.
constexpr int kFedMaxDepth = 4;
struct FedHold {
    unsigned char *mine;                            // probe: this call's map
    const unsigned char *others[kFedMaxDepth - 1];  // update: the maps of the other open calls ...
    int n_others;                                   // ... and their number
    unsigned long long *counters;
};
void fed_probe_hold_launch(const PolicyArgs &a, const FedHold &h, bool evlfu, int grid, hipStream_t st);
void policy_insert_fed_hold_launch(const PolicyArgs &a, const FedSrc &f, const FedHold &h, int grid, unsigned threads, hipStream_t st);

// Ragged bags over fed backing (evs_cache_fed_begin_bags; the contract: include/evstore_hip.h there): the count-first fetch-first
// bag chain cut in two where the fed chain above is cut:
//   begin    (flush ->) bags_fed_probe -> (EvLFU: bags_count, its column 39 into the call's own replica rows -> bags_fed_list) ->
//            fed_list, as it is, over the bag slab's lists
//   finish   fold -> bags_fed_hits -> the fed insert of the policy, as it is -> bags_repoint_fed -> bags_pool (-> dense interaction)
// All four new kernels walk the flat position list as bags_probe_launch does (block j: positions 256 (j + i grid) + thread,
// i < iters), so list j and rec_slot line up with what the update walks.  `a` is the BagArgs of bags_probe_launch; prov is written
// for all three policies (row, table, set, bit 31 | hit way -- or tag + 1 of a miss -- or 0: no key).
//   bags_fed_probe  flags, addresses (NULL-based for a miss of a fed table), hit totals into a.p.part1, prov; LRU / LFU: the miss
//                   lists too (their records need no count); EvLFU: pos_sample preset to -1.  Writes NO way word.
//   bags_fed_list   EvLFU, behind bags_count: bags_raise_list's listing (row, table | agg << 8, set, tag + 1) without its raise.
//   bags_fed_hits   first launch of the finish: every position prov calls a hit -- LRU / LFU the plain-store touch of the probe,
//                   once per way and batch; EvLFU the raise to agg[pos_sample[p]] with the histogram moves into a.p.part1 (read
//                   first, compare-and-swap only while the priority is below).  Nothing else writes a way word in that launch.
void bags_fed_probe_launch(const BagArgs &a, int grid, hipStream_t st);
void bags_fed_list_launch(const BagArgs &a, int grid, hipStream_t st);
void bags_fed_hits_launch(const BagArgs &a, int grid, hipStream_t st);
// The flat form of sa_repoint_fed_launch, read from prov (no index is loaded, nothing is permuted again): a miss that got a way is
// pointed at its arena row; a miss of a fed table that got none at its fed row through the scratch table (read-only; a key not found
// there: the zero row and the sticky flag); a miss of an addressed table that got none keeps its table address.  A position that
// is no key raises the sticky flag.  counters: the (B, T) form's four ([0] / [1] of `counters`, [0] / [1] of f.counters).
struct BagRepointFedArgs {
    SaGeom sa;
    const uint4 *prov;                     // n_pos records as bags_fed_probe wrote them
    long long *row_ptrs;                   // n_pos slots of the pointer table
    unsigned char *arena;
    unsigned long long *counters;
    long long n_pos;
    int iters, row_bytes;
};
void bags_repoint_fed_launch(const BagRepointFedArgs &a, const FedSrc &f, int grid, hipStream_t st);

// Fetch-first order of the C1 + C2 pair that shares its set records (both tiers at evs_cache_set_miss_order(c, 1); the chain:
// evs_cache.hip, batch_c1c2_impl; the rule: include/evstore_hip.h at evs_cache_lookup_batch_c1c2).  The pair has no two-copy
// arena, so behind the pair's update a way the batch HIT may hold another key.  Every position is searched again in the ways of
// the tier its serve byte d names, and only there -- the two tiers' ways are one 128-byte record, one line request per position:
//   code 0, index in range   found: the slot is re-pointed at tier d's arena row; not found (the key was turned away, or the
//                            route filter gave it to C1 while this position was routed to C2): it keeps tier d's table row
//   code 1 / 2               found: nothing is stored; not found (this call's update took the way): the slot is pointed at
//                            tier d's table row, whose bytes are those the arena held
//   bad index / serve byte 0 untouched
// Writes no way word, does no atomic on a record, reads no table.  counters (one add per block each): [0] miss positions
// re-pointed at an arena, [1] miss positions left in place, [2] hit positions whose way the call's own update took.
// (Same-address device atomics serialise at about 10 ns each: 2 048 blocks adding two or three totals into ONE counter block were 22
//  of this launch's 30 us at B = 16 384.  The pair's totals therefore go into replica rows, a 128-byte line each, which
//  evs_cache_fetch_stats sums; a tier alone keeps adding into row 0.)
constexpr int kFetchReplicas = 32, kFetchRowWords = 16;
struct Repoint2Args {
    SaGeom sa1, sa2; SaUniverse sau;
    const int *requests;                   // (B, T) int32 row ids
    long long rows[32];                    // per table: min of the two tiers' row counts (an index past either is no key)
    const unsigned char *backing1[32], *backing2[32];
    const unsigned char *code;             // (B, T) the probe's tier codes (1 / 2 a hit there, 0 a miss)
    const unsigned char *serve;            // (B, T) the probe's serve bytes (row_tier)
    long long *row_ptrs;                   // (B, T) the pointer table
    unsigned char *arena1, *arena2;
    unsigned long long *counters;          // kFetchReplicas rows of kFetchRowWords words, block j adds into row j % kFetchReplicas, words 0 .. 2
    int *err;                              // the sticky index-error flag: raised for an index out of range (counted nowhere)
    long long B;
    int T, row_bytes1, row_bytes2;
};
// the (B, T) probe's grid and walk (block j: requests 8 j, 8 (j + grid), ...; a half-wave per request, a lane per key); the 8 + 8
// pair has its way counts compiled in, every other shared-record geometry takes the general form
void sa_repoint2_launch(const Repoint2Args &a, int grid, hipStream_t st);

// ... and of the pair's bag form (evs_cache_lookup_bags_c1c2 with both tiers at order 1 and "count first"; the chain: evs_cache.hip,
// cache_bags_c1c2_impl): behind the pair's update and in front of bags_pool2.  The rule per position is Repoint2Args' above, read
// from what the bag probe and the route launch left -- prov[p] holds row, table, tier code, the key bit and (set, quotient), serve[p]
// the serving tier -- so no index is loaded and nothing is divided or permuted again.  Every position with a key is searched,
// whether or not a bag covers it; serve byte 0 (a bad index: the probe has raised the sticky flag) is untouched and counted
// nowhere.  Writes no way word, does no atomic on a record, reads no table.  counters: the (B, T) form's replica rows and words
// (the two forms may alternate on one pair).
struct BagRepoint2Args {
    SaGeom sa1, sa2;
    const unsigned char *backing1[32], *backing2[32];
    const uint4 *prov;                     // n_pos records as bags_probe2 wrote them (BagPairArgs)
    const unsigned char *serve;            // n_pos serve bytes: the code of a hit, the destination bags_route2 gave a miss
    long long *row_ptrs;                   // n_pos slots of the pointer table
    unsigned char *arena1, *arena2;
    unsigned long long *counters;          // kFetchReplicas rows of kFetchRowWords words, block j adds into row j % kFetchReplicas, words 0 .. 2
    long long n_pos;
    int iters, row_bytes1, row_bytes2;
};
// the bag probe's grid and walk (block j: positions 256 (j + i grid) + thread, i < iters); the 8 + 8 pair has its way counts
// compiled in, every other shared-record geometry takes the general form
void bags_repoint2_launch(const BagRepoint2Args &a, int grid, hipStream_t st);

// Fed backing of the fetch-first pair (evs_cache_pair_fed_begin; the contract: include/evstore_hip.h there): the pair's chain cut
// in two where the fed chain of a tier alone is cut:
//   begin    (flush of either tier ->) the pair's probe in fed form (evs_cache.hip: cache_batch_probe2_kernel<true> -- codes, serve
//            bytes, addresses, both tiers' miss lists, hit totals into the call's own rows; NO way word, NO route-filter word; a
//            missed position of a fed table gets its tier's zero row) -> fed_list once per tier, each over its own scratch table
//   finish   fold x 2 -> pair_fed_hits -> the pair's update in fed form, a launch per tier (evs_cache.hip: sa_list_block<FED, SPILL>)
//            -> sa_repoint2_fed -> consumers -> close bookkeeping
//   pair_fed_hits     everything the ordinary probe writes that the begin withheld: a way the begin hit (its code names the tier)
//                     is raised to the sample's agg_hit = the number of its codes that are not 0, the histogram moves into
//                     part1_1 / part1_2 columns 0 .. T; a miss routed to C1 (serve byte 1) on an odd table is stamped into the
//                     route filter.  Nothing else writes a way word in that launch.
//   the spill         The pair keeps ONE arena row per way, so a way the call hit can be the call's victim, and a fed table has no
//                     table row to serve such a position from.  The update's thread that replaces an OCCUPIED way whose old key
//                     belongs to a fed table copies the way's arena row into slot `record index` (list * list_cap + i) of the
//                     tier's spill block -- behind its compare-and-swap, which made the way its own, and in front of the new
//                     row's stores -- and writes that index at spill_of[entry].  A victim of an addressed table is not spilled:
//                     its hit positions are served from the table row, as sa_repoint2 serves them.  A way filled from free has
//                     nothing to spill.
//   sa_repoint2_fed   per position, in the ways of the tier its serve byte d names:
//                       code 0, found                       tier d's arena row
//                       code 0, not found, fed table        fed_d's row through tier d's scratch table (read-only walk; a key the
//                                                           table does not hold: the zero row stays, the sticky flag is raised)
//                       code 0, not found, addressed table  the table row the probe wrote stays
//                       code d, found                       nothing stored
//                       code d, not found, fed table        spill_d + spill_of_d[entry] * row_bytes_d, entry = (the arena address
//                                                           the probe wrote - arena_d) / row_bytes_d
//                       code d, not found, addressed table  tier d's table row
//                     No stamp and no clearing of spill_of: "code d, not found" means this call's update replaced that way, a way
//                     changes at most once per update launch (old -> stamped), so exactly ONE thread won the way's
//                     compare-and-swap and wrote spill_of[entry] -- in this call, in a launch that ended before this one began.
// counters: r.counters as Repoint2Args has them ([2] counts every "code d, not found" position, spill or table); pair_cnt: replica
// rows of kFetchRowWords words -- [0] missed positions of fed tables, [1] of those served from a fed block, [2] rows spilled (the
// update adds it), [3] hit positions served from the spill.
struct PairFedArgs {
    Repoint2Args r;
    FedSrc f1, f2;                         // per tier: the fed block, the scratch table, the zero row, the spill
    unsigned fed_mask;
    unsigned long long *pair_cnt;
    int *part1_1, *part1_2;                // pair_fed_hits: the tiers' replica rows
    unsigned *route_filter; unsigned route_mask, route_stamp;
};
// both: the (B, T) probe's grid and walk, the 8 + 8 pair with its way counts compiled in
void pair_fed_hits_launch(const PairFedArgs &a, int grid, hipStream_t st);
void sa_repoint2_fed_launch(const PairFedArgs &a, int grid, hipStream_t st);

}  // namespace evs
