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


# ------------------------------------------------------------------------------------------------- stamps modulo 2^S
@pytest.mark.parametrize("geom", sorted(M.WRAP_GEOMETRIES))
def test_stamp_bits_of_the_wrap_geometries(geom):
    """sa_make_geom restated: tag bits, the two-copy arena and S of the three geometries the wrap tests use, the refusal
    past 22 tag bits and the no-wrap geometry of the pinned streams."""
    cap, n_rows, S = M.WRAP_GEOMETRIES[geom]
    tb, dual = {"tiny": (22, 0), "tiny-dual": (19, 1), "inline": (17, 1)}[geom]
    for policy in ("evlfu", "lfu", "lru"):
        assert M.stamp_bits_of(policy, cap, n_rows) == (tb, dual, S[policy])
        assert S[policy] == 26 - dual - tb + (6 if policy == "lru" else 0)
    if geom == "tiny":
        with pytest.raises(ValueError):
            M.stamp_bits_of("lfu", 8, n_rows)             # one set: 23 tag bits
    assert M.stamp_bits_of("lfu", 512, N_ROWS) == (11, 1, 14) and M.stamp_bits_of("lru", 512, N_ROWS) == (11, 1, 20)


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_modular_model_is_the_plain_one_before_a_wrap(policy):
    """On the `small` stream no way is left alone for 2^S - 1 batches (S = 14 / 20, 400 batches): holding `last` modulo 2^S
    changes nothing -- flags, ways, counters and dump scores equal the plain model's after every batch, no event counted."""
    cap, batch, n_batches = SHAPES[0]
    S = M.stamp_bits_of(policy, cap, N_ROWS)[2]
    reqs, hits, _ = M.conflict_free_stream(policy, cap, N_ROWS, batch, n_batches, 3)
    plain, mod = M.BatchedPolicyModel(policy, cap, N_ROWS), M.BatchedPolicyModel(policy, cap, N_ROWS, stamp_bits=S)
    for i in range(n_batches):
        assert np.array_equal(plain.batch(reqs[i]), hits[i]) and np.array_equal(mod.batch(reqs[i]), hits[i]), "batch %d" % i
        for wp, wm in zip(plain.sets, mod.sets):
            assert [w and (w[0], w[1], w[2] % (1 << S), w[3]) for w in wp] == [w and tuple(w) for w in wm], "batch %d" % i
        assert plain.resident() == mod.resident()
    assert mod.n_evict == plain.n_evict > 10 * cap and not any(mod.events.values())


def test_modular_rule_details():
    """The three places the modular rule parts from the plain one, on one hand-made set (S = 3: a wrap every 8 batches)."""
    for policy in ("lru", "lfu"):
        m = M.BatchedPolicyModel(policy, 8, [100], stamp_bits=3)
        for r in range(8):                                   # batches 1..8 fill ways 0..7
            m.batch(np.array([[r]], np.int32))
        # batch 9 = 1 + 2^3: key 0 (filled by batch 1) looks touched by the running batch.  A hit leaves its word alone ...
        assert m.batch(np.array([[0]], np.int32)).all()
        assert m.sets[0][0][:3] == [(1, 0), 1, 1] and m.events["count_skipped"] == (policy == "lfu")
        assert m.resident()[(1, 0)] == (0 if policy == "lru" else 1)
        # ... batch 10: key 1 (batch 2) is the lapped one and the plain victim; a new key passes it over and takes way 2
        assert not m.batch(np.array([[50]], np.int32)).any()
        assert m.sets[0][1][0] == (1, 1) and m.sets[0][2][0] == (1, 50) and m.events["victim"] == m.events["passed_over"] == 1
        # batch 12: way 3 (batch 4) is lapped, every other way is hit: the new key is turned away
        m.batch(np.array([[0]], np.int32))
        keys = [0, 1, 50, 4, 5, 6, 7, 60]
        h = m.batch(np.array([[k] for k in keys], np.int32))
        assert h.ravel().tolist() == [True] * 7 + [False] and (1, 60) not in m.where and (1, 3) in m.where
        assert m.events["turned_away"] == 1 and m.events["passed_over"] == 2


@pytest.mark.parametrize("policy,geom", sorted(M.WRAP_CASES))
def test_wrap_streams_cover_what_the_gpu_tests_rely_on(policy, geom):
    """The streams tests/test_gpu_batched_lru_lfu.py replays: conflict-free from batch 2 on (checked against a fresh model),
    reproducible, at least three wraps, every kind of event the policy can show at least five times and a run that parts
    from the plain-integer model -- or, for LRU on `tiny-dual` (S = 12: no wrap in 640 batches), none of that, ten carries
    of `last` from its 6-bit low field into the high one and evictions in between."""
    cap, n_rows, S = M.WRAP_GEOMETRIES[geom]
    S = S[policy]
    assert M.stamp_bits_of(policy, cap, n_rows)[2] == S
    batches, hits, model, parted = M.wrap_case(policy, geom)
    print(policy, geom, "S = %d:" % S, parted)
    replay = M.BatchedPolicyModel(policy, cap, n_rows, stamp_bits=S)
    for i, rq in enumerate(batches):
        assert 2 <= len(rq) <= 4 and rq.shape[1] == len(n_rows) and (rq >= 0).all() and (rq < n_rows[0]).all()
        if i:
            assert not M.new_key_conflicts(replay, rq), "batch %d" % (i + 1)
        assert np.array_equal(replay.batch(rq), hits[i])
    assert replay.resident() == model.resident() and replay.events == model.events
    if (policy, geom) == ("lru", "tiny-dual"):
        low = 26 - 1 - 19                                     # the low field of `last`: 26 - dual - tag bits
        assert len(batches) >> low >= 9 and parted["evictions"] >= 4 * (len(batches) >> low)
        assert not any(parted[k] for k in M.EVENTS) and parted["first"] is None
        return
    assert parted["wraps"] >= 3
    kinds = [k for k in M.EVENTS if policy == "lfu" or k != "count_skipped"]
    assert all(parted[k] >= 5 for k in kinds), parted
    assert parted["flags"] >= 5 and parted["dumps"] >= 5 and parted["first"] > (1 << S)
    assert parted["evictions"] >= 5
