"""The Python restatement of the batched LRU / LFU rule over ragged bags (tests/_bag_policy_model.py) held to the (B, T)
model where the two must agree, and the conflict-free ragged streams the GPU tests replay checked for what they promise.
No GPU."""
import functools

import numpy as np
import pytest

import _bag_policy_model as BM
import _batched_policy_model as M

N_ROWS = [2000] * 26
SHAPES = [(1024, 4, 3, 300), (2048, 8, 4, 200)]      # (capacity, samples, largest bag, batches)


@functools.lru_cache(maxsize=None)
def _stream(policy, shape):
    return BM.conflict_free_bag_stream(policy, shape[0], N_ROWS, shape[1], shape[2], shape[3], 3)


@functools.lru_cache(maxsize=None)
def _rect_stream():
    return M.conflict_free_stream("lfu", 512, N_ROWS, 4, 100, 3)


def test_one_index_per_bag_is_the_rectangular_rule():
    """every bag of size 1: batch_keys gives the flags, the resident set and n_evict of BatchedPolicyModel.batch"""
    reqs, hits, want = _rect_stream()
    m = BM.BagPolicyModel("lfu", 512, N_ROWS)
    ref = M.BatchedPolicyModel("lfu", 512, N_ROWS)
    for i in range(len(reqs)):
        B, T = reqs[i].shape
        keys = [(t + 1, int(reqs[i][b, t])) for t in range(T) for b in range(B)]       # table-major positions
        flags = m.batch_keys(keys).reshape(T, B).T
        assert np.array_equal(flags, ref.batch(reqs[i])) and np.array_equal(flags, hits[i]), "batch %d" % i
        assert m.resident() == ref.resident() and m.n_evict == ref.n_evict
    assert m.resident() == want.resident() and m.n_evict == want.n_evict > 0
    # ... and through batch_bags with arange offsets the counters are the (B, T) form's
    m = BM.BagPolicyModel("lfu", 512, N_ROWS)
    for i in range(len(reqs)):
        B, T = reqs[i].shape
        flags = m.batch_bags([np.arange(B)] * T, [reqs[i][:, t].astype(np.int64) for t in range(T)])
        assert np.array_equal(np.stack(flags, 1), hits[i])
    assert m.n_requests == hits.shape[0] * hits.shape[1] and m.n_hits == int(hits.sum())
    assert m.n_perfect == int(hits.all(2).sum())


@pytest.mark.parametrize("stamp_bits", [None, 3])
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_the_two_forms_alternate_on_one_model(policy, stamp_bits):
    """batch and batch_keys keep one model's ways in one layout: alternating them call by call (one index per bag) gives
    the flags, the resident set, the scores and the event counts of batch alone -- with plain batch numbers and with a
    3-bit stamp that wraps every 8 calls"""
    reqs = _rect_stream()[0]         # (LFU's conflict-free stream; LRU replays the same requests)
    m = BM.BagPolicyModel(policy, 512, N_ROWS, stamp_bits=stamp_bits)
    ref = M.BatchedPolicyModel(policy, 512, N_ROWS, stamp_bits=stamp_bits)
    for i in range(len(reqs)):
        B, T = reqs[i].shape
        want = ref.batch(reqs[i])
        if i % 3 == 1:
            flags = m.batch(reqs[i])
        else:
            # (positions in batch's own order: under LRU or the wrapping stamp the stream need not stay conflict-free)
            flags = m.batch_keys([(t + 1, int(reqs[i][b, t])) for b in range(B) for t in range(T)]).reshape(B, T)
        assert np.array_equal(flags, want), "call %d" % i
        assert m.resident() == ref.resident() and m.sets == ref.sets and m.events == ref.events, "call %d" % i
    assert ref.n_evict > 0 and m.n_evict == ref.n_evict


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_ragged_streams_are_conflict_free_and_evict(policy, shape):
    """no call of a stream brings two new keys to one set (checked against a fresh model replaying it), the replay
    reproduces the recorded flags, bags of every size 0 .. L occur, and the stream evicts more than 5 x capacity"""
    cap, B, L, n_batches = shape
    calls, model, redrawn = _stream(policy, shape)
    replay = BM.BagPolicyModel(policy, cap, N_ROWS)
    sizes = set()
    for i, (off, idx, flags) in enumerate(calls):
        assert not BM.new_key_conflicts(replay, BM.keys_of(idx)), "call %d" % i
        got = replay.batch_bags(off, idx)
        assert all(np.array_equal(g, f) for g, f in zip(got, flags)), "call %d" % i
        for k in range(26):
            assert len(off[k]) == B and off[k][0] == 0
            sizes |= set(np.diff(np.append(off[k], len(idx[k]))).tolist())
    assert sizes == set(range(L + 1))
    assert replay.resident() == model.resident() and replay.n_evict == model.n_evict
    assert (replay.n_requests, replay.n_hits, replay.n_perfect) == (model.n_requests, model.n_hits, model.n_perfect)
    print("%s cap %d B %d L %d: %.1f x capacity evicted, %.1f %% of the positions redrawn, hit rate %.3f, %d all-hit samples" %
          (policy, cap, B, L, model.n_evict / cap, 100 * redrawn, model.n_hits / sum(len(i) for c in calls for i in c[1]),
           model.n_perfect))
    assert model.n_evict > 5 * cap
    assert model.n_requests == B * n_batches


def test_rule_details_over_positions():
    """one set, one table: the same key at several positions is one touch and one insert; an index out of range is no key"""
    for policy in ("lru", "lfu"):
        m = BM.BagPolicyModel(policy, 8, [100])
        f = m.batch_bags([np.array([0, 3])], [np.array([5, 5, 5, 7, -1, 100])])     # sample 0: 5 5 5; sample 1: 7, -1, 100
        assert not f[0].any() and m.size() == 2 and (1, -1) not in m.where and (1, 100) not in m.where
        f = m.batch_bags([np.array([0, 3])], [np.array([5, 5, 5, 7, 5])])
        assert f[0].all() and m.n_perfect == 2 and m.n_hits == 5 and m.n_requests == 4
        assert m.resident() == ({(1, 5): 0, (1, 7): 0} if policy == "lru" else {(1, 5): 2, (1, 7): 2})
        f = m.batch_bags([np.array([2, 1])], [np.array([5, 5])])        # backwards offsets: bag 0 is empty, bag 1 = {5}
        assert f[0].all() and m.n_perfect == 3
