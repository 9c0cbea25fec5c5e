"""CPU: the Python restatement of the pair's bag rule (tests/_bag_pair_model.py) against the (B, T) expectations the warm-start
tests pin the pair to (tests/test_gpu_pair_warm_start.py::_expected) at one index per bag, on hand-made cases of what bags
add -- served bags, uncovered positions, bad offsets and indices, a key routed both ways --, and its conflict-free generator
against its own promise."""
import numpy as np
import pytest

import _bag_pair_model as BP
import _pair_warm_model as P
import test_gpu_pair_warm_start as W

N_ROWS, T = W.N_ROWS, W.T
CAPS = [(64, 128), (64, 96), (32, 128)]


def _export(geom, rs, fill=0.8):
    """a hand-made export: distinct keys placed by the warm start's own plan (non-strict), slot column filled in"""
    n1, n2 = int(geom.tiers[0].cap * fill), int(geom.tiers[1].cap * fill)
    e = P.random_entries(rs, geom, n1, n2, 5)
    dest, _w, _o = P.plan(geom, e)
    e = e[dest >= 0].copy()
    e[:, 5] = dest[dest >= 0]
    return {"entries": e}


@pytest.mark.parametrize("caps", CAPS)
@pytest.mark.parametrize("thr", [1, 2, 3])
def test_one_index_per_bag_is_the_bt_expectation(caps, thr):
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    rs = np.random.RandomState(caps[0] + caps[1] + thr)
    ex = _export(geom, rs)
    e = ex["entries"]
    B = 48
    rq = np.stack([rs.randint(0, n, B) for n in N_ROWS], 1).astype(np.int32)
    for b in range(B):                                  # two columns of three name a resident key
        for t in rs.permutation(T)[:2]:
            rows = e[e[:, 1] == t + 1][:, 2]
            if len(rows):
                rq[b, t] = rows[rs.randint(len(rows))]
    code, serve = W._expected(geom, ex, rq, thr)
    assert (code == 1).any() and (code == 2).any() and (code == 0).any()
    st = BP.State(geom, e)
    j = BP.judge(st, B, [np.arange(B)] * T, [rq[:, t] for t in range(T)], thr)
    for t in range(T):
        assert np.array_equal(j.code[t], code[:, t]) and np.array_equal(j.serve[t], serve[:, t])
    assert np.array_equal(j.agg, (code != 0).sum(1)) and not j.bad
    assert j.hits == (int((code == 1).sum()), int((code == 2).sum())) and j.perfect == int(((code != 0).sum(1) == T).sum())
    # every missed key is listed for the tier that serves it, at its request's count (the maximum over its requests)
    for t in range(T):
        for b in range(B):
            if code[b, t] == 0:
                assert j.listed[serve[b, t] - 1][(t + 1, int(rq[b, t]))] >= j.agg[b]


def test_what_bags_add():
    geom = P.Geometry(64, 128, N_ROWS)
    full = P.keys_of_set(geom, 1, 0, 9)                 # nine keys of C1 set 0: eight fill it, the ninth finds no room
    st = BP.State(geom, [[1, t1, r, 1, 0, i] for i, (t1, r) in enumerate(full[:8])])
    new = full[8]
    k = new[0] - 1
    B, thr = 3, 2
    # table k: the bags start at position 1 -- position 0 is covered by nobody --, samples 0 and 1 name `new`, sample 2's bag is
    # empty.  The other tables' bags are empty, hence served.
    idx = [np.zeros(0, np.int64) for _ in range(T)]
    off = [np.zeros(B, np.int64) for _ in range(T)]
    idx[k] = np.array([new[1], new[1], new[1]], np.int64)
    off[k] = np.array([1, 2, 3], np.int64)
    j = BP.judge(st, B, off, idx, thr)
    assert not j.bad and j.pos_sample[k].tolist() == [-1, 0, 1] and j.bags[k][2] == (3, 3)
    assert j.agg.tolist() == [T - 1, T - 1, T] and j.perfect == 0      # (sample 2 has no lookup: not a perfect request)
    assert j.code[k].tolist() == [0, 0, 0] and j.hits == (0, 0)
    by_parity = 1 if k % 2 == 1 else 2
    # T - 1 = 2 reaches the threshold: C2; the uncovered position counts 0: by the table's parity
    assert j.serve[k].tolist() == [by_parity, 2, 2] and j.listed[1][new] == T - 1
    assert j.listed[by_parity - 1][new] >= 0 and not st.c1_room(k, new[1])
    # offsets past nnz: bags 1 and 2 are empty (served), the sticky flag, trailing positions uncovered
    jb = BP.judge(st, B, [np.array([0, 1, 5], np.int64) if t == k else off[t] for t in range(T)], idx, thr)
    assert jb.bad and jb.pos_sample[k].tolist() == [0, -1, -1] and jb.agg.tolist() == [T - 1, T, T] and jb.bags[k][1:] == [(0, 0), (0, 0)]
    # an index out of range is no key: code 0, no row, never listed, and its bag is not served
    idx[k] = np.array([new[1], N_ROWS[k], -1], np.int64)
    j2 = BP.judge(st, B, [np.array([0, 1, 2], np.int64) if t == k else off[t] for t in range(T)], idx, thr)
    assert j2.bad and j2.code[k].tolist() == [0, 0, 0] and j2.serve[k].tolist() == [2, 0, 0] and j2.agg.tolist() == [T - 1] * 3
    assert set(j2.listed[0]) | set(j2.listed[1]) == {new}
    # a set with room takes the key into C1 whatever the count
    st.slots[0].pop(3)
    j3 = BP.judge(st, B, [np.array([0, 1, 2], np.int64) if t == k else off[t] for t in range(T)], idx, thr)
    assert j3.serve[k].tolist() == [1, 0, 0] and j3.insert[0] == {new: T - 1}
    assert BP.apply(st, j3).slots[0][3] == [new[0], new[1], T - 1]


def test_a_key_routed_both_ways_goes_to_c1():
    geom = P.Geometry(64, 128, N_ROWS)
    # nine keys of table 1 (odd) in one C1 set: eight fill it; the ninth is named by a sample below the threshold (-> C1) and
    # by one at it (-> C2)
    for es in range(geom.nset):
        ks = [key for key in P.keys_of_set(geom, 1, es, 60) if key[0] == 2]
        if len(ks) >= 9:
            break
    st = BP.State(geom, [[1, t1, r, 1, 0, es * 8 + i] for i, (t1, r) in enumerate(ks[:8])])
    new, res = ks[8], ks[0]
    B, thr = 2, T - 1
    # sample 0 misses `new` and a key of table 0 (agg = T - 2 < thr); sample 1 misses `new` alone (agg = T - 1) and hits `res`
    absent0 = next(r for r in range(N_ROWS[0]) if geom.place(1, 0, r)[0] != es)
    idx = [np.array([absent0], np.int64), np.array([new[1], new[1], res[1]], np.int64), np.zeros(0, np.int64)]
    off = [np.array([0, 1], np.int64), np.array([0, 1], np.int64), np.array([0, 0], np.int64)]
    j = BP.judge(st, B, off, idx, thr)
    assert j.agg.tolist() == [T - 2, T - 1]
    assert j.serve[1].tolist() == [1, 2, 1] and j.code[1].tolist() == [0, 0, 1]
    assert new in j.listed[0] and new in j.listed[1] and new in j.filtered and new not in j.insert[1]
    assert j.insert[0][new] == T - 2 and not BP.is_conflict_free(st, j)
    assert j.raise_to[0] == {es * 8: T - 1}


@pytest.mark.parametrize("caps", CAPS)
def test_the_generator_is_conflict_free(caps):
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    rs = np.random.RandomState(caps[1])
    ex = _export(geom, rs, 0.9)
    st = BP.State(geom, ex["entries"])
    used = {(int(t1), int(r)) for t1, r in ex["entries"][:, 1:3]}
    B, n_new_seen, sizes = 12, 0, []
    for call in range(30):
        off, idx = BP.conflict_free_call(rs, st, used, B)
        before = (set(st.keys(1)), set(st.keys(2)))
        j = BP.judge(st, B, off, idx, 2)
        assert BP.is_conflict_free(st, j) and not j.bad and not j.filtered
        named = [(t + 1, int(r)) for t in range(T) for r in idx[t]]
        new = [key for key in named if key not in before[0] and key not in before[1]]
        assert len(new) == len(set(new)), "a new key is named twice"
        recs = [geom.record(t1 - 1, r) for t1, r in new]
        assert len(recs) == len(set(recs)), "two new keys in one set record"
        assert any(len(idx[t]) for t in range(T))
        assert all(en - st_ <= 4 for t in range(T) for st_, en in j.bags[t])
        n_new_seen += len(new)
        BP.apply(st, j)
        k1, k2 = set(st.keys(1)), set(st.keys(2))
        assert not (k1 & k2) and len(k1) <= caps[0] and len(k2) <= caps[1]
        assert all(key in k1 or key in k2 for key in new), "a new key of a conflict-free call is always kept"
        assert all(0 <= e[2] <= T for k in (0, 1) for e in st.slots[k].values())
        sizes.append((len(k1), len(k2)))
    assert n_new_seen >= 30
