"""The re-point rule of the fetch-first bag form of the C1 + C2 pair (include/evstore_hip.h at evs_cache_lookup_bags_c1c2; the
kernel: csrc/evs_cache_policy.hip, bags_repoint2_kernel) restated in Python over tests/_bag_pair_model.py's State / judge / apply
(test infrastructure).

The snapshot side of a call -- tier codes, serve bytes, agg_hit, the per-tier miss lists, the route filter, pooled -- is
_bag_pair_model's, unchanged: the fetch-first chain moves launches, not the rule.  Behind the pair's update EVERY position of
the flat index arrays, covered by a bag or not, is looked up again in the ways of the tier d its serve byte names, and only there:

  serve byte 0 (a bad index)      served from nothing, counted nowhere
  code 0, serve byte d            key resident in tier d after the call: tier d's ARENA row (total `repointed`); not resident
                                  there (turned away, or routed both ways and C1 took it while this position was routed to
                                  C2): tier d's TABLE row, in place (total `in_place`)
  code d (a hit in tier d)        still resident in tier d: its ARENA row, untouched; gone (this call's update took the way):
                                  tier d's TABLE row (total `victim_hits`)

It is _pair_fetch_model.repoint over flat positions.  It needs only the resident sets after the call, so it is exact on
contended calls too, with the sets taken from the dumps."""
import numpy as np

import _bag_pair_model as BP
from _pair_fetch_model import ARENA, NOTHING, TABLE  # noqa: F401  (re-exported: the per-position sources)

TOTALS = ("repointed", "in_place", "victim_hits")


def resident_sets(after):
    """after: a _bag_pair_model.State, or a pair of key collections {(table_1based, row)} (as read from the two dumps)"""
    if isinstance(after, BP.State):
        return set(after.keys(1)), set(after.keys(2))
    return set(after[0]), set(after[1])


def repoint_flat(j, indices, after):
    """j: the judged call (_bag_pair_model.judge), indices: its T index arrays, after: the pair behind the call's update
    (resident_sets) -> (source: T uint8 arrays of NOTHING | ARENA | TABLE, one per position -- the tier is the serve byte --,
    {'repointed', 'in_place', 'victim_hits'})"""
    resident = resident_sets(after)
    totals = dict.fromkeys(TOTALS, 0)
    source = []
    for k, idx in enumerate(indices):
        idx = np.asarray(idx, np.int64)
        src = np.zeros(len(idx), np.uint8)
        for p in range(len(idx)):
            d = int(j.serve[k][p])
            if d == 0:
                continue
            code = int(j.code[k][p])
            assert code in (0, d), "a hit is served by the tier that holds it"
            there = (k + 1, int(idx[p])) in resident[d - 1]
            src[p] = ARENA if there else TABLE
            if code == 0:
                totals["repointed" if there else "in_place"] += 1
            elif not there:
                totals["victim_hits"] += 1
        source.append(src)
    return source, totals


def add_totals(running, totals, calls=1):
    """the cumulative fetch_stats() of C1 after one more call"""
    running["calls"] = running.get("calls", 0) + calls
    for name in TOTALS:
        running[name] = running.get(name, 0) + totals[name]
    return running
