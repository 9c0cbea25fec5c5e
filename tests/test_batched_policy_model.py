"""The Python restatement of the batched LRU / LFU rule (tests/_batched_policy_model.py) held to the sequential oracle
where the two must agree, and the conflict-free streams the GPU tests replay checked for what they promise.  No GPU."""
import numpy as np
import pytest

import _batched_policy_model as M

N_ROWS = [2000] * 26
SHAPES = [(512, 4, 400), (1024, 8, 300)]      # (capacity, batch, batches)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    oracle.build()
    return oracle


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_model_is_the_sequential_policy_one_key_at_a_time(orc, policy, seed):
    """One set (capacity 8), one table, one key per batch: nothing is batched, so the rule IS sequential LRU / LFU and the
    model's hit trace equals the oracle's (oracle.LRU / oracle.LFU take a single table as they are).  The LFU leg runs the
    counter unsaturated, as the oracle's frequencies are."""
    n_keys, n_req = 40, 400
    rs = np.random.RandomState(seed)
    perm = rs.permutation(n_keys)
    rows = M.zipf_rows(rs, n_keys, n_req, 1.3, perm).astype(np.int32)
    tables = [np.zeros((n_keys, 36), np.float32)]
    o = (orc.LRU if policy == "lru" else orc.LFU)(8, tables)
    m = M.BatchedPolicyModel(policy, 8, [n_keys], cnt_max=None)
    assert m.nset == 1
    want = np.array([bool(o.request(np.array([r], np.int32))[0][0]) for r in rows])
    got = np.array([bool(m.batch(np.array([[r]], np.int32))[0, 0]) for r in rows])
    assert np.array_equal(got, want), "first difference at request %d" % int(np.nonzero(got != want)[0][0])
    assert 0.2 < want.mean() < 0.95 and m.n_evict > 20      # (the trace exercises hits, misses and evictions)


@pytest.mark.parametrize("cap,batch,n_batches", SHAPES)
def test_streams_are_conflict_free_and_separate_the_policies(cap, batch, n_batches):
    """The generator's streams bring no two new keys of a batch to one set (checked against a fresh model replaying them),
    evict often, and tell LRU from LFU: the LRU stream through the LFU model changes at least 5 % of the flags."""
    for policy in ("lru", "lfu"):
        reqs, hits, model = M.conflict_free_stream(policy, cap, N_ROWS, batch, n_batches, 3)
        replay = M.BatchedPolicyModel(policy, cap, N_ROWS)
        for i in range(n_batches):
            assert not M.new_key_conflicts(replay, reqs[i]), "batch %d" % i
            assert np.array_equal(replay.batch(reqs[i]), hits[i])
        assert replay.resident() == model.resident()
        assert model.size() == cap and model.n_evict > 10 * cap
        assert 0.6 <= hits.mean() <= 0.85, hits.mean()
        if policy == "lru":
            other = M.BatchedPolicyModel("lfu", cap, N_ROWS)
            flags = np.stack([other.batch(r) for r in reqs])
            print("cap %d batch %d: hit rate %.3f, %.1f %% of %d flags differ under lfu" %
                  (cap, batch, hits.mean(), 100 * (flags != hits).mean(), hits.size))
            assert (flags != hits).mean() >= 0.05


def test_rule_details():
    """the tie-breaks and the 'never a victim in its own batch' clause on hand-made sets (one set of 8 ways, one table)"""
    for policy in ("lru", "lfu"):
        m = M.BatchedPolicyModel(policy, 8, [100])
        for r in range(8):                                   # batches 1..8 fill ways 0..7 in order
            assert not m.batch(np.array([[r]], np.int32)).any()
        assert [w[0][1] for w in m.sets[0]] == list(range(8))
        # batch 9 hits key 0 twice and brings key 50: LRU evicts key 1 (the oldest untouched); LFU too (all counters 1 but
        # key 0's, which counts ONE for the batch)
        h = m.batch(np.array([[0], [0], [50]], np.int32))
        assert h.ravel().tolist() == [True, True, False]
        assert m.sets[0][0][:2] == [(1, 0), 2] and m.sets[0][1][0] == (1, 50)
        # batch 10 touches every resident key but way 7's and brings two new keys: the first takes way 7, the second is
        # turned away (every way carries stamp 10)
        keys = [0, 50, 2, 3, 4, 5, 6, 60, 61]
        h = m.batch(np.array([[k] for k in keys], np.int32))
        assert h.ravel().tolist() == [True] * 7 + [False, False]
        assert m.sets[0][7][0] == (1, 60) and (1, 61) not in m.where and m.size() == 8
    m = M.BatchedPolicyModel("lfu", 8, [100], cnt_max=3)
    for _ in range(6):
        m.batch(np.array([[7]], np.int32))
    assert m.resident() == {(1, 7): 3}                       # saturating
