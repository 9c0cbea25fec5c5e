"""tests/_fed_ahead_model.py -- several fed calls open at once, restated in Python -- against the models it wraps, and the argument
refusals of the three entry points that need no GPU (include/evstore_hip.h at evs_cache_set_fed_depth).  Driven begin, finish,
begin, finish the model must BE the wrapped model; on generated streams at depth 2 and 4 no key is resident twice, every way held
at a finish is still there after it, and a key two open calls both missed is installed once."""
import ctypes as C

import numpy as np
import pytest

import _bag_evlfu_model as EM
import _batched_policy_model as M
import _fed_ahead_model as A
import _fed_backing_common as H


@pytest.mark.parametrize("geom", ["G1", "G2"])
@pytest.mark.parametrize("policy", H.POLICIES)
def test_driven_serially_it_is_the_wrapped_model(policy, geom):
    g = H.GEOMS[geom]
    rows, flags = H._bt_stream(policy, geom)
    a = A.FedAheadModel(policy, g["cap"], list(g["n_rows"]))
    w = EM.BagEvLFUModel(g["cap"], list(g["n_rows"])) if policy == "evlfu" else M.BatchedPolicyModel(policy, g["cap"], list(g["n_rows"]))
    for i in range(H.N_BATCHES):
        f, call = a.begin(rows[i])
        a.finish(call)
        if policy == "evlfu":
            w.batch_bags(*EM.one_per_bag(rows[i]))
        else:
            w.batch(rows[i])
        assert np.array_equal(f, flags[i]), "call %d: flags" % (i + 1)
        assert a.resident() == w.resident() and a.m.sets == w.sets, "call %d: the tier" % (i + 1)
    assert a.found_installed == 0 and a.passed_over == 0 and a.ahead_begins == 0 and a.m.n_evict == w.n_evict > 0
    if policy == "evlfu":
        assert (a.n_requests, a.n_hits, a.n_perfect) == (w.n_requests, w.n_hits, w.n_perfect)


@pytest.mark.parametrize("geom,depth", [("G1", 2), ("G2", 2), ("G2", 4)])
@pytest.mark.parametrize("policy", H.POLICIES)
def test_generated_streams_hold_what_they_hit(policy, geom, depth):
    """ahead_stream asserts after every finish that no key is resident twice and that every way the other open calls hold still
    carries its key; here: the stream met the cases at all, and every key two open calls both missed is resident at most once."""
    g = H.GEOMS[geom]
    reqs, flags, model, info = A.searched_stream(policy, g["cap"], g["n_rows"], g["B"], H.N_BATCHES, depth)
    assert info["ahead_begins"] == H.N_BATCHES - 1 and info["held_checked"] > 0
    assert info["both_missed"] > 0 and info["found_installed"] > 0 and info["passed_over"] > 0
    keys = [w[0] for ways in model.m.sets for w in ways if w is not None]
    assert len(keys) == len(set(keys)) == len(model.m.where) <= g["cap"]
    # the replay gives the same flags: the stream is a function of its seed
    again = A.FedAheadModel(policy, g["cap"], list(g["n_rows"]))
    calls = {}
    for op, i in A.schedule(H.N_BATCHES, depth):
        if op == "begin":
            f, calls[i] = again.begin(reqs[i])
            assert np.array_equal(f, flags[i])
            assert len(again.open) <= depth
        else:
            again.finish(calls[i])
    assert again.resident() == model.resident() and again.found_installed == info["found_installed"]


def test_an_abort_gives_the_batch_number_back():
    g = H.GEOMS["G2"]
    rows, _ = H._bt_stream("lru", "G2")
    a = A.FedAheadModel("lru", g["cap"], list(g["n_rows"]))
    for i in range(3):
        a.finish(a.begin(rows[i])[1])
    before = (a.resident(), a.m.n)
    _, p = a.begin(rows[3])
    f1, _q = a.begin(rows[4])
    a.abort()
    f2, q = a.begin(rows[4])
    assert np.array_equal(f1, f2) and q["n"] == p["n"] + 1
    a.abort()
    a.abort()
    assert (a.resident(), a.m.n) == before and not a.open


def test_the_schedule():
    assert A.schedule(3, 1) == [("begin", 0), ("finish", 0), ("begin", 1), ("finish", 1), ("begin", 2), ("finish", 2)]
    assert A.schedule(4, 2) == [("begin", 0), ("begin", 1), ("finish", 0), ("begin", 2), ("finish", 1), ("begin", 3), ("finish", 2), ("finish", 3)]


def test_argument_refusals_without_a_gpu():
    import evstore_dlrm_amd as E
    L = E._lib
    lib = L.lib()
    assert lib.evs_cache_set_fed_depth(None, 2) == L.EVS_EINVAL and b"NULL" in lib.evs_last_error()
    assert lib.evs_cache_fed_open_calls(None) == -1
    out4 = (C.c_int64 * 4)()
    assert lib.evs_cache_fed_ahead_stats(None, out4, None) == L.EVS_EINVAL and b"NULL" in lib.evs_last_error()
    assert lib.evs_cache_fed_ahead_stats(None, None, None) == L.EVS_EINVAL
