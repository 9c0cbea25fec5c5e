"""CPU: the Python restatement of the batched EvLFU rule over ragged bags (tests/_bag_evlfu_model.py; the rule:
include/evstore_hip.h at evs_cache_lookup_bags, "served bags") on hand-worked calls, against a straightforward (B, T)
restatement with one index per bag, and the property the GPU tests rely on: the pinned streams never come near a flush."""
import numpy as np
import pytest

import _bag_evlfu_model as EM
import _batched_policy_model as M

N3 = [50, 50, 50]            # three tables, capacity 16: two sets of eight ways


def _i64(*a):
    return np.array(a, np.int64)


def _call(m, bags):
    """bags[k][b] = the indices of sample b's bag of table k -> the model's flags per table"""
    off = [np.concatenate([[0], np.cumsum([len(x) for x in tb[:-1]])]).astype(np.int64) for tb in bags]
    idx = [np.concatenate([_i64(*x) for x in tb]).astype(np.int64) for tb in bags]
    return m.batch_bags(off, idx)


def _rows_in_set(m, table0, s, n):
    rows = np.arange(m.n_rows[table0])
    return [int(r) for r in rows[M.set_of(table0, rows, m.nset, m.n_rows, m.bits) == s][:n]]


def test_an_empty_bag_counts_as_served():
    m = EM.BagEvLFUModel(16, N3)
    bags = [[[5]], [[]], [[7]]]
    flags = _call(m, bags)
    assert not any(f.any() for f in flags)
    assert m.resident() == {(1, 5): 1, (3, 7): 1}              # two bags with a miss, the empty one served: agg_hit = 1
    assert (m.n_requests, m.n_hits, m.n_perfect) == (1, 0, 0)
    flags = _call(m, bags)
    assert all(f.all() for f in flags)
    assert m.resident() == {(1, 5): 3, (3, 7): 3}              # all three served
    assert (m.n_requests, m.n_hits, m.n_perfect) == (2, 2, 1)
    assert m.hist() == [0, 0, 0, 2]
    # a sample without a single lookup has agg_hit = T and is no perfect hit
    _call(m, [[[]], [[]], [[]]])
    assert (m.n_requests, m.n_perfect) == (3, 1)


def test_one_miss_unserves_its_bag_only():
    m = EM.BagEvLFUModel(16, N3)
    _call(m, [[[1, 2]], [[1]], [[1]]])
    assert set(m.resident().values()) == {0} and m.size() == 4  # every bag had a miss
    flags = _call(m, [[[1, 2, 9]], [[1]], [[1]]])
    assert flags[0].tolist() == [True, True, False]
    assert m.resident() == {(1, 1): 2, (1, 2): 2, (2, 1): 2, (3, 1): 2, (1, 9): 2}
    # an out-of-range index unserves its bag like a miss and is never inserted
    flags = _call(m, [[[1, 50]], [[1]], [[-1]]])
    assert flags[0].tolist() == [True, False] and flags[2].tolist() == [False]
    assert m.resident()[(2, 1)] == 2 and m.size() == 5 and m.n_perfect == 0


def test_the_maximum_over_samples():
    m = EM.BagEvLFUModel(16, N3)
    _call(m, [[[1]], [[1]], [[1]]])
    # sample 0 finds everything (3); sample 1 names (1, 1) too and misses twice (1)
    _call(m, [[[1], [1]], [[1], [30]], [[1], [31]]])
    r = m.resident()
    assert (r[(1, 1)], r[(2, 1)], r[(3, 1)], r[(2, 30)], r[(3, 31)]) == (3, 3, 3, 1, 1)
    assert m.n_perfect == 1
    # a new key named by a sample that counts 2 and by one that counts 1 comes in at 2
    _call(m, [[[40], [40]], [[1], [41]], [[1], [1]]])
    r = m.resident()
    assert (r[(1, 40)], r[(2, 41)]) == (2, 1)
    # ... and a resident way is never lowered: (2, 1) stays at 3 under counts of 2 and 1
    assert r[(2, 1)] == 3 and r[(3, 1)] == 3


def test_an_uncovered_position_counts_zero():
    # table 0: positions 0 and 1 in front of the first bag.  (1, 1) hit there and nowhere else: not raised, not lowered;
    # (1, 40) missed there: inserted at 0 although its call's samples count 3 and 2
    off = [_i64(2, 3), _i64(0, 1), _i64(0, 1)]
    idx = [_i64(1, 40, 1, 41), _i64(1, 1), _i64(1, 1)]
    m2 = EM.BagEvLFUModel(16, N3)
    m2.batch_bags([_i64(0), _i64(0), _i64(0)], [_i64(1), _i64(1), _i64(1)])     # (1, 1), (2, 1), (3, 1) at 0
    flags = m2.batch_bags(off, idx)
    assert flags[0].tolist() == [True, False, True, False]
    r = m2.resident()
    assert r[(1, 40)] == 0 and r[(1, 41)] == 2                  # sample 1: bag 0 has the miss, 2 served
    assert r[(1, 1)] == 3                                       # raised through position 2 (sample 0: 3 served), not through 0
    assert (m2.n_hits, m2.n_perfect) == (6, 1)                  # two hit positions per table
    # uncovered alone: the hit way keeps its priority
    m3 = EM.BagEvLFUModel(16, N3)
    m3.batch_bags([_i64(0), _i64(0), _i64(0)], [_i64(1), _i64(1), _i64(1)])
    m3.batch_bags([_i64(1), _i64(0), _i64(0)], [_i64(1), _i64(1), _i64(1)])     # table 0: bag 0 = [1, 1) empty, position 0 uncovered
    assert m3.resident() == {(1, 1): 0, (2, 1): 3, (3, 1): 3} and m3.n_perfect == 1


def test_backwards_offsets_make_empty_served_bags():
    m = EM.BagEvLFUModel(16, N3)
    # table 0, B = 3: bag 0 = [0, 9) runs past nnz = 4 and bag 1 = [9, 2) is backwards: both empty, both served;
    # bag 2 = [2, 4); positions 0 and 1 are covered by nothing
    off = [_i64(0, 9, 2), _i64(0, 1, 2), _i64(0, 1, 2)]
    idx = [_i64(3, 4, 5, 6), _i64(1, 1, 1), _i64(2, 2, 2)]
    m.batch_bags(off, idx)
    assert m.resident() == {(1, 3): 0, (1, 4): 0, (1, 5): 0, (1, 6): 0, (2, 1): 1, (3, 2): 1}   # samples 0 and 1 count the empty bag
    m.batch_bags(off, idx)
    assert m.resident() == {(1, 3): 0, (1, 4): 0, (1, 5): 3, (1, 6): 3, (2, 1): 3, (3, 2): 3}
    assert m.n_perfect == 3
    # offsets that go back and make two samples' valid bags overlap: the rule leaves the position's count open, the model refuses
    with pytest.raises(AssertionError):
        m.batch_bags([_i64(0, 3, 2), _i64(0, 1, 2), _i64(0, 1, 2)], idx)


def test_no_victim_among_the_ways_the_running_batch_filled():
    m = EM.BagEvLFUModel(16, N3)
    s0 = _rows_in_set(m, 0, 0, 10)
    assert len(s0) == 10
    # nine new keys for set 0 in one call: eight take the free ways, the ninth finds every way stamped by this batch
    _call(m, [[s0[:9]], [[]], [[]]])
    assert m.size() == 8 and m.n_turned == 1 and (1, s0[8]) not in m.where and m.n_evict == 0
    assert set(m.resident().values()) == {2}                    # (the bag with the misses unserved, the two empty ones served)
    # the next call may take them: lowest priority, lowest way index among equals -- way 0, the first key
    _call(m, [[[s0[8]]], [[]], [[]]])
    assert (1, s0[0]) not in m.where and m.where[(1, s0[8])] == (0, 0) and m.n_evict == 1
    # a way hit by the running batch CAN be the victim when it is still the lowest: every way at 2; ways 0 .. 6 go to 3 first,
    # then a call that hits way 7 and brings one new key evicts way 7
    _call(m, [[[s0[8]] + s0[1:7]], [[]], [[]]])
    assert sorted(m.resident().values()) == [2] + [3] * 7
    _call(m, [[[s0[7], s0[9]]], [[]], [[]]])                     # (1, s0[7]) hit, its bag unserved: count 2, no raise; the lowest
    assert (1, s0[7]) not in m.where and m.where[(1, s0[9])] == (0, 7) and m.resident()[(1, s0[9])] == 2
    # modulo 2^S a way filled 2^S batches ago looks filled by the running batch
    w = EM.BagEvLFUModel(16, N3, stamp_bits=2)
    _call(w, [[s0[:8]], [[]], [[]]])
    for _ in range(3):
        _call(w, [[[]], [[]], [[]]])
    _call(w, [[[s0[8]]], [[]], [[]]])                            # batch 5 = 1 mod 4
    assert w.n_turned == 1 and w.size() == 8


class _PlainBT:
    """The (B, T) batched EvLFU rule on a set-associative tier, written without bags: agg_hit = the request's resident keys."""

    def __init__(self, cap, n_rows):
        self.n_rows = n_rows
        self.nset, self.bits = M.geometry(cap, n_rows)
        self.ways = [[None] * 8 for _ in range(self.nset)]
        self.n = 0
        self.n_perfect = 0

    def keys(self):
        return {w[0]: w for ways in self.ways for w in ways if w}

    def batch(self, reqs):
        self.n += 1
        B, T = reqs.shape
        res = self.keys()
        hit = np.array([[(t + 1, int(reqs[b, t])) in res for t in range(T)] for b in range(B)])
        agg = hit.sum(1)
        self.n_perfect += int((agg == T).sum())
        new = {}
        for t in range(T):                                     # (table-major: the bag form's position order, which decides who
            for b in range(B):                                 #  comes first when two new keys meet in one set)
                key = (t + 1, int(reqs[b, t]))
                if hit[b, t]:
                    res[key][1] = max(res[key][1], int(agg[b]))
                else:
                    new[key] = max(new.get(key, 0), int(agg[b]))
        for key, a in new.items():
            ways = self.ways[int(M.set_of(key[0] - 1, key[1], self.nset, self.n_rows, self.bits))]
            free = [j for j, w in enumerate(ways) if w is None]
            old = sorted((w[1], j) for j, w in enumerate(ways) if w is not None and w[2] != self.n)
            j = free[0] if free else (old[0][1] if old else None)
            if j is not None:
                ways[j] = [key, a, self.n]
        return hit


def test_one_index_per_bag_is_the_bt_rule():
    n_rows = [300, 7, 120, 40, 900]
    m, plain = EM.BagEvLFUModel(64, n_rows), _PlainBT(64, n_rows)
    rs = np.random.RandomState(5)
    for i in range(150):
        reqs = np.stack([np.minimum(rs.zipf(1.2, 6) - 1, n - 1) for n in n_rows], 1).astype(np.int32)
        flags = m.batch_bags(*EM.one_per_bag(reqs))
        assert np.array_equal(np.stack(flags, 1), plain.batch(reqs)), "batch %d" % i
        assert m.resident() == {k: w[1] for k, w in plain.keys().items()}, "batch %d" % i
        assert m.n_perfect == plain.n_perfect
    assert m.n_evict > 64 and m.n_perfect > 0 and sum(m.hist()) == m.size() == 64


N_ROWS = [2000] * 26
SHAPES = {"small": (1024, 4, 3, 300), "large": (2048, 8, 4, 200)}      # tests/test_gpu_cache_bags.py: SHAPES
SEED = 3


@pytest.mark.parametrize("shape", ["small", "large"])
def test_the_pinned_streams_never_come_near_a_flush(shape):
    """The GPU tests pin every priority on these streams; a flush, whose victims depend on timing, must not fire: the top
    bucket stays below int(0.95 * capacity) after every call -- while the tier is full and evicting."""
    cap, B, L, n_batches = SHAPES[shape]
    calls, model, top = EM.conflict_free_bag_stream(cap, N_ROWS, B, L, n_batches, SEED)
    assert top < int(0.95 * cap), "top bucket %d of %d: take another seed" % (top, int(0.95 * cap))
    assert top == 0
    assert model.size() == cap and model.n_evict > 2 * cap and model.n_turned == 0
    prios = sorted(model.resident().values())
    assert prios[0] >= 1 and prios[-1] < 26 and prios[len(prios) // 2] >= 10
    assert model.n_hits > 0 and 0 < sum(int(f.sum()) for _, _, fl in calls for f in fl) == model.n_hits


def test_the_one_per_bag_stream_is_conflict_free_and_evicts():
    rows, flags, model = EM.conflict_free_rows_stream(512, N_ROWS, 4, 400, SEED)
    assert model.size() == 512 and model.n_evict > 5 * 512 and model.top_bucket() < int(0.95 * 512)
    assert flags.any() and not flags.all()
