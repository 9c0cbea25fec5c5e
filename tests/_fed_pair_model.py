"""The fed form of the fetch-first C1 + C2 pair (include/evstore_hip.h at evs_cache_pair_fed_begin; the chain and the spill:
csrc/evs_cache_policy.h at PairFedArgs) restated in Python over tests/_bag_pair_model.py's State / judge / apply and
tests/_pair_fetch_model.py's judge_bt (test infrastructure).

The snapshot side of a begin is the addressed pair's: tier codes, serve bytes, agg_hit, the per-tier miss lists.  On top of it:

  lists     keys_d = every distinct valid key of a FED table that a missed position with serve byte d names, once, as
            table_1based << 32 | row -- the tier's miss list BEFORE the route filter restricted to the fed tables: a key routed both
            ways is in both lists
  source    where the bytes of a position come from behind the finish's update, in the tier d its serve byte names:
              serve byte 0                          NOTHING
              code 0, resident in tier d after      ARENA
              code 0, not resident, fed table       FED_BLOCK   (turned away, or kept by the other tier)
              code 0, not resident, addressed       TABLE
              code d, still resident                ARENA
              code d, gone, fed table               SPILL       (this call's update took the way; the taker spilled the old row)
              code d, gone, addressed               TABLE
  stats     the eight words of evs_cache_pair_fed_stats as one call moves them
  spilled   the occupied ways of keys of fed tables the update replaces (a conflict-free call: _bag_pair_model.apply's choice)"""
import numpy as np

import _bag_pair_model as BP

NOTHING, ARENA, FED_BLOCK, SPILL, TABLE = 0, 1, 2, 3, 4


def is_fed(fed_mask, table0):
    return bool((fed_mask >> table0) & 1)


def fed_lists(j, fed_mask):
    """j: the Judged of the call (_pair_fetch_model.judge_bt) -> (keys1, keys2) as sorted lists of table_1based << 32 | row"""
    return tuple(sorted((t1 << 32) | row for (t1, row) in j.listed[d] if is_fed(fed_mask, t1 - 1)) for d in (0, 1))


def sources(code, serve, rq, after, fed_mask):
    """code / serve (B, T) of the judged call, rq (B, T), after: the State behind the call's update -> (source (B, T), the re-point
    totals {'repointed', 'in_place', 'victim_hits'} as evs_cache_fetch_stats counts them, {'missed', 'from_block', 'from_spill'})"""
    rq = np.asarray(rq, np.int64)
    B, T = rq.shape
    resident = (after.keys(1), after.keys(2))
    src = np.zeros((B, T), np.uint8)
    fetch = {"repointed": 0, "in_place": 0, "victim_hits": 0}
    fed = {"missed": 0, "from_block": 0, "from_spill": 0}
    for b in range(B):
        for k in range(T):
            d = int(serve[b, k])
            if d == 0:
                continue
            assert code[b, k] in (0, d), "a hit is served by the tier that holds it"
            there = (k + 1, int(rq[b, k])) in resident[d - 1]
            f = is_fed(fed_mask, k)
            if code[b, k] == 0:
                src[b, k] = ARENA if there else (FED_BLOCK if f else TABLE)
                fetch["repointed" if there else "in_place"] += 1
                fed["missed"] += int(f)
                fed["from_block"] += int(f and not there)
            else:
                src[b, k] = ARENA if there else (SPILL if f else TABLE)
                fetch["victim_hits"] += int(not there)
                fed["from_spill"] += int(f and not there)
    return src, fetch, fed


def apply_counting(state, j, fed_mask):
    """_bag_pair_model.apply on a conflict-free call, counting the rows the fed update spills: every insert over an occupied way whose
    old key belongs to a fed table -> (state, spilled)"""
    before = [dict(state.slots[k]) for k in (0, 1)]
    BP.apply(state, j)
    spilled = 0
    for k in (0, 1):
        for slot, old in before[k].items():
            new = state.slots[k].get(slot)
            if new is not None and (new[0], new[1]) != (old[0], old[1]) and is_fed(fed_mask, old[0] - 1):
                spilled += 1
    return state, spilled


def stats_step(stats, j, fed_mask, fed, spilled):
    """the eight words after one finished call"""
    k1, k2 = fed_lists(j, fed_mask)
    s = list(stats)
    s[0] += 1
    s[1] += len(k1)
    s[2] += len(k2)
    s[3] += fed["missed"]
    s[4] += fed["from_block"]
    s[5] += spilled
    s[6] += fed["from_spill"]
    return s
