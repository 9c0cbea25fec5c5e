"""The re-point rule of the fetch-first C1 + C2 pair (include/evstore_hip.h at evs_cache_lookup_batch_c1c2; the kernel:
csrc/evs_cache_policy.hip, sa_repoint2_kernel) restated in Python over tests/_pair_warm_model.py's Geometry and
tests/_bag_pair_model.py's State / judge / apply (test infrastructure).

A (B, T) call is the bag form's call with one index per bag, so the snapshot side -- tier codes, serve bytes, agg_hit, the
per-tier miss lists, the route filter -- is _bag_pair_model.judge's.  Behind the pair's update every position is looked up
again in the ways of the tier d its serve byte names, and only there:

  serve byte 0 (a bad index)      served from nothing, counted nowhere
  code 0, serve byte d            key resident in tier d after the call: tier d's ARENA row (total `repointed`); not resident
                                  there (turned away, or routed both ways and C1 took it while this position was routed to
                                  C2): tier d's TABLE row, in place (total `in_place`)
  code d (a hit in tier d)        still resident in tier d: its ARENA row, untouched; gone (this call's update took the way):
                                  tier d's TABLE row (total `victim_hits`)

Either way the served bytes are tier d's table row in tier d's codec."""
import numpy as np

import _bag_pair_model as BP

NOTHING, ARENA, TABLE = 0, 1, 2


def judge_bt(state, rq, thr):
    """rq (B, T) int row ids against the state as a snapshot -> (_bag_pair_model.Judged, code (B, T), serve (B, T))"""
    rq = np.asarray(rq, np.int64)
    B, T = rq.shape
    offsets = [np.arange(B, dtype=np.int64)] * T
    j = BP.judge(state, B, offsets, [rq[:, k] for k in range(T)], thr)
    return j, np.stack(j.code, 1), np.stack(j.serve, 1)


def repoint(code, serve, rq, after):
    """code / serve (B, T) of the judged call, rq (B, T), after: the State behind the call's update
    -> (source (B, T) of NOTHING | ARENA | TABLE -- the tier is the serve byte --, {'repointed', 'in_place', 'victim_hits'})"""
    rq = np.asarray(rq, np.int64)
    B, T = rq.shape
    resident = (after.keys(1), after.keys(2))
    source = np.zeros((B, T), np.uint8)
    totals = {"repointed": 0, "in_place": 0, "victim_hits": 0}
    for b in range(B):
        for k in range(T):
            d = int(serve[b, k])
            if d == 0:
                continue
            assert code[b, k] in (0, d), "a hit is served by the tier that holds it"
            there = (k + 1, int(rq[b, k])) in resident[d - 1]
            source[b, k] = ARENA if there else TABLE
            if code[b, k] == 0:
                totals["repointed" if there else "in_place"] += 1
            elif not there:
                totals["victim_hits"] += 1
    return source, totals


def expected_rows(serve, rq, dec1, dec2):
    """the fp32 rows the call serves: dec1 / dec2 per table the (n_rows, d) rows each tier's codec decodes; serve byte 0: zeros"""
    rq = np.asarray(rq, np.int64)
    B, T = rq.shape
    out = np.zeros((B, T, dec1[0].shape[1]), np.float32)
    for k in range(T):
        for d, dec in ((1, dec1), (2, dec2)):
            m = serve[:, k] == d
            out[m, k] = dec[k][rq[m, k]]
    return out
