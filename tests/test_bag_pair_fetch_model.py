"""CPU: the re-point rule of the fetch-first bag form of the C1 + C2 pair as tests/_bag_pair_fetch_model.py restates it, on
hand-written states -- a hit whose way the call's own update takes, a key routed both ways, a key turned away, one key at several
positions, an uncovered position, an index out of range -- and its agreement with tests/_pair_fetch_model.py's (B, T) rule when
every bag has one index."""
import numpy as np

import _bag_pair_fetch_model as BF
import _bag_pair_model as BP
import _pair_fetch_model as F
import _pair_warm_model as P

N_ROWS = [200, 1000, 4000]
GEOM = P.Geometry(64, 128, N_ROWS)
T = 3


def _rows_of_set(tier, es, table0, count, skip=()):
    out = [r for r in range(N_ROWS[table0]) if GEOM.place(tier, table0, r)[0] == es and (table0 + 1, r) not in skip]
    assert len(out) >= count
    return out[:count]


def _full_c1_set(es, scores):
    rows = _rows_of_set(1, es, 1, 8)
    return [[1, 2, r, s, 0, es * 8 + j] for j, (r, s) in enumerate(zip(rows, scores))], [(2, r) for r in rows]


def _fresh_rows(used_records, table0, count):
    out = []
    for r in range(N_ROWS[table0]):
        rec = GEOM.record(table0, r)
        if rec not in used_records:
            used_records.add(rec)
            out.append(r)
            if len(out) == count:
                return out
    raise AssertionError("too few records")


def _flat(bags):
    off = [np.cumsum([0] + [len(b) for b in bags[t][:-1]]).astype(np.int64) for t in range(T)]
    idx = [np.array([r for b in bags[t] for r in b], np.int64) for t in range(T)]
    return off, idx


def test_a_hit_whose_way_the_update_takes_in_a_ragged_call():
    """C1 set 0 full, way 0 the lowest; sample 0 hits it twice in one bag (agg_hit 1 leaves it the lowest), sample 1 brings a ninth
    key of the set (odd table, agg_hit 0 < 2: to C1), which takes the way: both hit positions are served from the table"""
    entries, keys = _full_c1_set(0, [0, 2, 2, 2, 2, 2, 2, 2])
    st = BP.State(GEOM, entries)
    newcomer = _rows_of_set(1, 0, 1, 1, skip=set(keys))[0]
    used = {0}
    a, b = _fresh_rows(used, 0, 2), _fresh_rows(used, 2, 2)
    bags = [[[a[0]], [a[1]]], [[keys[0][1], keys[0][1]], [newcomer]], [[b[0]], [b[1]]]]
    off, idx = _flat(bags)
    j = BP.judge(st, 2, off, idx, 2)
    assert j.code[1].tolist() == [1, 1, 0] and j.agg.tolist() == [1, 0] and BP.is_conflict_free(st, j)
    BP.apply(st, j)
    assert (2, newcomer) in st.keys(1) and keys[0] not in st.keys(1)
    source, totals = BF.repoint_flat(j, idx, st)
    assert source[1].tolist() == [BF.TABLE, BF.TABLE, BF.ARENA] and source[0].tolist() == [BF.ARENA] * 2
    assert totals == {"repointed": 5, "in_place": 0, "victim_hits": 2}


def test_a_key_routed_both_ways_by_two_bags():
    """an odd-table key x of a full C1 set in the bags of a sample without a served bag elsewhere (agg_hit 0 < 1: C1) and of a sample
    with one (1 >= 1: C2): the filter keeps it out of C2 and the C2-routed position stays on C2's table"""
    entries, keys = _full_c1_set(3, [2] * 8)
    x = _rows_of_set(1, 3, 1, 1, skip=set(keys))[0]
    st = BP.State(GEOM, entries + [[2, 1, 0, 1, 0, GEOM.place(2, 0, 0)[0] * 8]])
    used = {3, GEOM.record(0, 0)}
    a, b = _fresh_rows(used, 0, 1), _fresh_rows(used, 2, 2)
    bags = [[[a[0]], [0, 0]], [[x], [x]], [[b[0]], [b[1]]]]
    off, idx = _flat(bags)
    j = BP.judge(st, 2, off, idx, 1)
    assert j.agg.tolist() == [0, 1] and j.serve[1].tolist() == [1, 2] and j.filtered == {(2, x)}
    BP.apply(st, j)
    source, totals = BF.repoint_flat(j, idx, st)
    assert source[1].tolist() == [BF.ARENA, BF.TABLE] and source[0].tolist() == [BF.ARENA] * 3
    assert totals == {"repointed": 4, "in_place": 1, "victim_hits": 0}
    # ... and with the resident sets given as the two dumps' keys
    assert BF.repoint_flat(j, idx, (st.keys(1).keys(), st.keys(2).keys()))[1] == totals


def test_turned_away_uncovered_repeated_and_out_of_range():
    """nine new keys of the empty C1 set 5 in one bag of each table: one is turned away.  A position no bag covers (a leading one) is
    searched and counted all the same; a key at several positions counts once per position; an index out of range counts nowhere"""
    rows = [_rows_of_set(1, 5, t, 3) for t in range(T)]
    bags = [[list(rows[0]), []], [list(rows[1]), [rows[1][0]]], [list(rows[2]), [N_ROWS[2]]]]
    off, idx = _flat(bags)
    lead = _fresh_rows({5}, 0, 1)[0]
    idx[0] = np.concatenate([[lead], idx[0]]).astype(np.int64)
    off[0] = off[0] + 1
    j = BP.judge(BP.State(GEOM), 2, off, idx, 2)
    assert j.bad and j.pos_sample[0][0] == -1 and j.serve[0][0] == 1 and j.serve[2].tolist() == [1, 1, 1, 0]
    kept = [(t + 1, rows[t][i]) for i in range(3) for t in range(T)][:8]
    after = BP.State(GEOM, [[1, t1, r, 0, 0, 5 * 8 + w] for w, (t1, r) in enumerate(kept)] + [[1, 1, lead, 0, 0, GEOM.place(1, 0, lead)[0] * 8]])
    source, totals = BF.repoint_flat(j, idx, after)
    assert source[0][0] == BF.ARENA and source[2].tolist() == [BF.ARENA, BF.ARENA, BF.TABLE, BF.NOTHING]
    assert source[1].tolist() == [BF.ARENA] * 4                   # (the repeated key: both its positions)
    assert totals == {"repointed": 10, "in_place": 1, "victim_hits": 0}
    running = BF.add_totals(BF.add_totals({}, totals), totals)
    assert running == {"calls": 2, "repointed": 20, "in_place": 2, "victim_hits": 0}


def test_one_index_per_bag_is_the_bt_rule():
    """random states and calls with one index per bag: source and totals equal _pair_fetch_model.repoint's, whatever `after` is"""
    rs = np.random.RandomState(3)
    for trial in range(20):
        B = int(rs.randint(1, 12))
        entries, seen = [], set()
        for tier in (1, 2):
            for _ in range(40):
                t = int(rs.randint(T))
                r = int(rs.randint(60))
                es = GEOM.place(tier, t, r)[0]
                ways = [s for s in range(es * 8, es * 8 + 8) if (tier, s) not in seen]
                if (t + 1, r) in {(e[1], e[2]) for e in entries} or not ways:
                    continue
                seen.add((tier, ways[0]))
                entries.append([tier, t + 1, r, int(rs.randint(4)), 0, ways[0]])
        st = BP.State(GEOM, entries)
        rq = np.stack([rs.randint(-1, 61, B) for _t in range(T)], 1).astype(np.int32)
        j, code, serve = F.judge_bt(st, rq, 2)
        # any `after` will do: a random subset of the resident and the named keys
        named = [(t + 1, int(rq[b, t])) for b in range(B) for t in range(T)] + list(st.keys(1)) + list(st.keys(2))
        after = ({k for k in named if rs.rand() < 0.5}, {k for k in named if rs.rand() < 0.5})
        src_flat, tot_flat = BF.repoint_flat(j, [rq[:, t] for t in range(T)], after)

        class _After:
            def keys(self, tier):
                return after[tier - 1]
        src_bt, tot_bt = F.repoint(code, serve, rq, _After())
        assert tot_flat == tot_bt, trial
        assert np.array_equal(np.stack(src_flat, 1), src_bt), trial
