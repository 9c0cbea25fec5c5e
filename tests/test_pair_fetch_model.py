"""CPU: the re-point rule of the fetch-first C1 + C2 pair as tests/_pair_fetch_model.py restates it, on hand-made states -- a hit
whose way the call's own update takes, a key routed both ways, a key turned away, an index out of range."""
import numpy as np

import _bag_pair_model as BP
import _pair_fetch_model as F
import _pair_warm_model as P

N_ROWS = [200, 1000, 4000]
GEOM = P.Geometry(64, 128, N_ROWS)


def _rows_of_set(tier, es, table0, count, skip=()):
    out = [r for r in range(N_ROWS[table0]) if GEOM.place(tier, table0, r)[0] == es and (table0 + 1, r) not in skip]
    assert len(out) >= count
    return out[:count]


def _full_c1_set(es, scores):
    """eight keys of table 2 (index 1) filling C1 set es, way j with scores[j] -> entries, the keys"""
    rows = _rows_of_set(1, es, 1, 8)
    return [[1, 2, r, s, 0, es * 8 + j] for j, (r, s) in enumerate(zip(rows, scores))], [(2, r) for r in rows]


def _fresh_rows(used_records, table0, count):
    """rows of `table0` in `count` records nobody uses yet (their C1 sets are empty: such a miss goes to C1)"""
    out = []
    for r in range(N_ROWS[table0]):
        rec = GEOM.record(table0, r)
        if rec not in used_records:
            used_records.add(rec)
            out.append(r)
            if len(out) == count:
                return out
    raise AssertionError("too few records")


def test_geometry_is_the_reference_split():
    t1, t2 = GEOM.tiers
    assert (GEOM.nset, t1.ways, t2.ways, t2.sub_shift, t2.w_off) == (8, 8, 8, 1, 8)


def test_a_hit_whose_way_the_update_takes():
    """C1 set 0 is full and the hit key has its lowest priority; the sample that hits it has agg_hit 1, which leaves it the lowest;
    another sample's missed key of the same set (odd table, agg_hit 0 < threshold) is routed to C1 and takes that way"""
    entries, keys = _full_c1_set(0, [0, 2, 2, 2, 2, 2, 2, 2])
    st = BP.State(GEOM, entries)
    newcomer = _rows_of_set(1, 0, 1, 1, skip=set(keys))[0]
    used = {0}
    a, b = _fresh_rows(used, 0, 2), _fresh_rows(used, 2, 2)
    rq = np.array([[a[0], keys[0][1], b[0]], [a[1], newcomer, b[1]]], np.int32)
    j, code, serve = F.judge_bt(st, rq, thr=2)
    assert code.tolist() == [[0, 1, 0], [0, 0, 0]] and j.agg.tolist() == [1, 0]
    assert serve.tolist() == [[1, 1, 1], [1, 1, 1]] and BP.is_conflict_free(st, j)
    BP.apply(st, j)
    assert (2, newcomer) in st.keys(1) and keys[0] not in st.keys(1) and st.keys(1)[(2, newcomer)] == 0
    source, totals = F.repoint(code, serve, rq, st)
    assert source.tolist() == [[F.ARENA, F.TABLE, F.ARENA], [F.ARENA, F.ARENA, F.ARENA]]
    assert totals == {"repointed": 5, "in_place": 0, "victim_hits": 1}


def test_a_key_routed_both_ways():
    """an odd-table key of a full C1 set: a sample without a hit (agg_hit 0 < 1) sends it to C1, a sample with one (1 >= 1) to C2;
    the route filter keeps it out of C2, so the C2-routed position is served C2's table row in place"""
    entries, keys = _full_c1_set(3, [2] * 8)
    x = _rows_of_set(1, 3, 1, 1, skip=set(keys))[0]
    # the second sample's hit: key (table 1, row 0), resident in C2
    st = BP.State(GEOM, entries + [[2, 1, 0, 1, 0, GEOM.place(2, 0, 0)[0] * 8]])
    used = {3, GEOM.record(0, 0)}
    a, b = _fresh_rows(used, 0, 1), _fresh_rows(used, 2, 2)
    rq = np.array([[a[0], x, b[0]], [0, x, b[1]]], np.int32)
    j, code, serve = F.judge_bt(st, rq, thr=1)
    assert code.tolist() == [[0, 0, 0], [2, 0, 0]] and j.agg.tolist() == [0, 1]
    assert serve[0, 1] == 1 and serve[1, 1] == 2 and not BP.is_conflict_free(st, j)
    assert j.filtered == {(2, x)}
    BP.apply(st, j)
    assert (2, x) in st.keys(1) and (2, x) not in st.keys(2)
    source, totals = F.repoint(code, serve, rq, st)
    assert source[0, 1] == F.ARENA and source[1, 1] == F.TABLE and source[1, 0] == F.ARENA
    assert totals["in_place"] == 1 and totals["victim_hits"] == 0 and totals["repointed"] == 4


def test_a_key_turned_away():
    """nine new keys of one empty C1 set in one call: eight get a way, the ninth is served in place"""
    rows = [_rows_of_set(1, 5, t, 3) for t in range(3)]
    rq = np.array([[rows[0][i], rows[1][i], rows[2][i]] for i in range(3)], np.int32)
    j, code, serve = F.judge_bt(BP.State(GEOM), rq, thr=2)
    assert not code.any() and (serve == 1).all() and len(j.insert[0]) == 9
    kept = [(t + 1, rows[t][i]) for i in range(3) for t in range(3)][:8]
    after = BP.State(GEOM, [[1, t1, r, 0, 0, 5 * 8 + w] for w, (t1, r) in enumerate(kept)])
    source, totals = F.repoint(code, serve, rq, after)
    assert source.tolist() == [[F.ARENA] * 3, [F.ARENA] * 3, [F.ARENA, F.ARENA, F.TABLE]]
    assert totals == {"repointed": 8, "in_place": 1, "victim_hits": 0}


def test_an_index_out_of_range():
    """serve byte 0: served from nothing and in none of the totals; the sample's agg_hit does not count it"""
    entries, keys = _full_c1_set(0, [1] * 8)
    st = BP.State(GEOM, entries)
    rq = np.array([[-1, keys[2][1], N_ROWS[2]], [7, keys[3][1], 9]], np.int32)
    j, code, serve = F.judge_bt(st, rq, thr=2)
    assert j.bad and code.tolist() == [[0, 1, 0], [0, 1, 0]] and serve[0].tolist() == [0, 1, 0] and j.agg.tolist() == [1, 1]
    source, totals = F.repoint(code, serve, rq, st)                # (nothing applied: both hits still resident)
    assert source[0].tolist() == [F.NOTHING, F.ARENA, F.NOTHING]
    assert totals == {"repointed": 0, "in_place": 2, "victim_hits": 0}
    dec = [np.full((n, 4), k + 1, np.float32) for k, n in enumerate(N_ROWS)]
    out = F.expected_rows(serve, rq, dec, [2 * t for t in dec])
    assert not out[0, 0].any() and not out[0, 2].any() and (out[1, 1] == 2).all()
