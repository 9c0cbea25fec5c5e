"""CPU: tests/_fed_pair_model.py -- the fed lists, the source of every position and the eight stats words of the fed C1 + C2 pair --
held to tests/_pair_fetch_model.py's re-point rule on random conflict-free calls, and worked through by hand on the three directed
cases of tests/test_gpu_fed_pair.py: a hit whose way the update takes, a key routed both ways, nine new keys of one empty set."""
import numpy as np
import pytest

import _bag_pair_model as BP
import _fed_pair_common as K
import _fed_pair_model as M
import _pair_fetch_model as F
import _pair_warm_model as P


@pytest.mark.parametrize("shape,caps,mask", [("T3", (64, 128), 0b111), ("T5", (64, 128), 0b11111), ("T3", (36, 96), 0b010), ("T5", (64, 128), 0b01101)])
def test_sources_against_the_repoint_rule(shape, caps, mask):
    n_rows = K.SHAPES[shape]
    T = len(n_rows)
    geom = P.Geometry(caps[0], caps[1], n_rows)
    rs = np.random.RandomState(caps[0] + T + mask)
    st, used = BP.State(geom), set()
    stats = [0] * 8
    seen_spill = 0
    for B, n_new, cover in K.B_CYCLE + K.B_CYCLE:
        rq = K._quiet_call(rs, geom, set(st.keys(1)) | set(st.keys(2)), used, B, n_new, bool(cover))
        j, code, serve = F.judge_bt(st, rq, T)
        assert BP.is_conflict_free(st, j)
        k1, k2 = M.fed_lists(j, mask)
        for d, keys in ((1, k1), (2, k2)):
            assert len(set(keys)) == len(keys)
            named = {((t + 1) << 32) | int(rq[b, t]) for b in range(B) for t in range(T) if code[b, t] == 0 and serve[b, t] == d and M.is_fed(mask, t)}
            assert set(keys) == named
        st, spilled = M.apply_counting(st, j, mask)
        src, fetch, fed = M.sources(code, serve, rq, st, mask)
        src0, totals0 = F.repoint(code, serve, rq, st)
        assert fetch == totals0
        assert np.array_equal(src == M.ARENA, src0 == F.ARENA) and np.array_equal(src == M.NOTHING, src0 == F.NOTHING)
        assert np.array_equal(np.isin(src, (M.FED_BLOCK, M.SPILL, M.TABLE)), src0 == F.TABLE)
        hits = code > 0
        assert int((np.isin(src, (M.SPILL, M.TABLE)) & hits).sum()) == totals0["victim_hits"]
        assert int((np.isin(src, (M.FED_BLOCK, M.TABLE)) & ~hits).sum()) == totals0["in_place"]
        fedcol = np.array([M.is_fed(mask, t) for t in range(T)])
        assert not (np.isin(src, (M.FED_BLOCK, M.SPILL)) & ~fedcol[None, :]).any() and not ((src == M.TABLE) & fedcol[None, :]).any()
        # (several positions may name one victim: the distinct keys served from the spill are rows that were spilled)
        assert len({(t, int(rq[b, t])) for b in range(B) for t in range(T) if src[b, t] == M.SPILL}) <= spilled
        src_none, fetch_none, fed_none = M.sources(code, serve, rq, st, 0)
        assert np.array_equal(src_none == M.TABLE, src0 == F.TABLE) and fed_none == {"missed": 0, "from_block": 0, "from_spill": 0}
        stats = M.stats_step(stats, j, mask, fed, spilled)
        seen_spill += spilled
    assert stats[0] == 2 * len(K.B_CYCLE) and stats[7] == 0 and stats[1] + stats[2] > 0 and stats[3] >= stats[1] + stats[2] > stats[4]
    assert seen_spill > 0, "the stream never replaced a key of a fed table"


def test_a_hit_whose_way_the_update_takes():
    geom = P.Geometry(64, 128, K.SHAPES["T3"])
    rows, newcomer, _ab, rq = K._victim_case(geom)
    es = geom.place(1, 1, rows[0])[0]
    st = BP.State(geom, [[1, 2, r, 0 if i == 0 else 2, 0, es * 8 + i] for i, r in enumerate(rows)])
    j, code, serve = F.judge_bt(st, rq, 2)
    assert code.tolist() == [[0, 1, 0], [0, 0, 0]] and (serve == 1).all()
    k1, k2 = M.fed_lists(j, 0b111)
    assert len(k1) == 5 and k2 == [] and ((2 << 32) | newcomer) in k1 and ((2 << 32) | rows[0]) not in k1
    st, spilled = M.apply_counting(st, j, 0b111)
    assert spilled == 1 and (2, newcomer) in st.keys(1) and (2, rows[0]) not in st.keys(1)
    src, fetch, fed = M.sources(code, serve, rq, st, 0b111)
    assert src.tolist() == [[M.ARENA, M.SPILL, M.ARENA], [M.ARENA] * 3]
    assert fetch == {"repointed": 5, "in_place": 0, "victim_hits": 1} and fed == {"missed": 5, "from_block": 0, "from_spill": 1}
    assert M.stats_step([0] * 8, j, 0b111, fed, spilled) == [1, 5, 0, 5, 0, 1, 1, 0]
    # table 2 addressed: the victim's row is its table row, nothing is spilled
    st2 = BP.State(geom, [[1, 2, r, 0 if i == 0 else 2, 0, es * 8 + i] for i, r in enumerate(rows)])
    st2, spilled2 = M.apply_counting(st2, j, 0b101)
    src2, fetch2, fed2 = M.sources(code, serve, rq, st2, 0b101)
    assert spilled2 == 0 and src2[0, 1] == M.TABLE and fetch2 == fetch and fed2 == {"missed": 4, "from_block": 0, "from_spill": 0}


def test_routed_both_ways_and_turned_away():
    geom = P.Geometry(64, 128, K.SHAPES["T3"])
    full = K._rows_of_set(geom, 1, 3, 1, 9)
    x = full[8]
    used = {3, 5, geom.record(0, 0)}
    a, b = K._fresh_rows(geom, used, 0, 1), K._fresh_rows(geom, used, 2, 2)
    es0 = geom.place(2, 0, 0)[0]
    st = BP.State(geom, [[1, 2, r, 2, 0, 3 * 8 + i] for i, r in enumerate(full[:8])] + [[2, 1, 0, 1, 0, es0 * geom.tiers[1].ways]])
    rq1 = np.array([[a[0], x, b[0]], [0, x, b[1]]], np.int32)
    j, code, serve = F.judge_bt(st, rq1, 1)
    assert serve[0, 1] == 1 and serve[1, 1] == 2 and j.filtered == {(2, x)}
    k1, k2 = M.fed_lists(j, 0b111)
    assert ((2 << 32) | x) in k1 and ((2 << 32) | x) in k2
    BP.apply(st, j)
    src, fetch, fed = M.sources(code, serve, rq1, st, 0b111)
    assert src[0, 1] == M.ARENA and src[1, 1] == M.FED_BLOCK and src[1, 0] == M.ARENA
    assert fetch == {"repointed": 4, "in_place": 1, "victim_hits": 0} and fed == {"missed": 5, "from_block": 1, "from_spill": 0}
    # nine new keys of the empty C1 set 5: eight get a way, whichever they are; the ninth is served from the fed block
    nine = [K._rows_of_set(geom, 1, 5, t, 3) for t in range(3)]
    rq2 = np.array([[nine[0][i], nine[1][i], nine[2][i]] for i in range(3)], np.int32)
    j, code, serve = F.judge_bt(BP.State(geom), rq2, 2)
    assert not code.any() and (serve == 1).all() and len(M.fed_lists(j, 0b111)[0]) == 9
    kept = [(t + 1, int(rq2[i, t])) for i in range(3) for t in range(3)][:8]
    after = BP.State(geom, [[1, t1, r, 0, 0, 5 * 8 + w] for w, (t1, r) in enumerate(kept)])
    src, fetch, fed = M.sources(code, serve, rq2, after, 0b111)
    assert int((src == M.ARENA).sum()) == 8 and int((src == M.FED_BLOCK).sum()) == 1
    assert fetch == {"repointed": 8, "in_place": 1, "victim_hits": 0} and fed == {"missed": 9, "from_block": 1, "from_spill": 0}
