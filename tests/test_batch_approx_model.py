"""CPU: the approximate-embedding mode of the batched EvLFU rule as tests/_batch_approx_model.py restates it, on hand-made states,
and the cover of the streams tests/test_gpu_batch_approx.py runs -- so that what those streams exercise is checked without a GPU."""
import numpy as np
import pytest

import _bag_evlfu_model as EM
import _batch_approx_model as A
import _batched_policy_model as M

N_ROWS = [50, 60, 70, 80]       # T = 4
CAP = 64


def _model(keys, prio=1):
    m = A.BatchApproxModel(CAP, N_ROWS)
    m.n = 9
    for k in keys:
        m.place(k, prio)
    return m


def test_hits_at_tables_1_and_3_thres_2():
    """table 0 has no hit below it: the zero row; table 2 is served what table 1 is served"""
    m = _model([(2, 11), (4, 13)])
    flags, served = m.batch(np.array([[5, 11, 12, 13]], np.int32), 2)
    assert flags.tolist() == [[2, 1, 2, 1]]
    assert served == [[None, (2, 11), (2, 11), (4, 13)]]
    assert m.resident() == {(2, 11): 2, (4, 13): 2}, "raised to agg_hit = 2; nothing inserted for the approximated positions"
    assert m.approx_counters() == {"calls": 1, "samples": 1, "substituted": 1, "zero_rows": 1}
    assert (m.n_hits, m.n_perfect, m.n_requests, m.n_fetched) == (2, 0, 1, 0)
    tabs = [np.arange(n * 3, dtype=np.float32).reshape(n, 3) + 1000 * t for t, n in enumerate(N_ROWS)]
    rows = A.served_rows(served, tabs, 3)
    assert not rows[0, 0].any() and np.array_equal(rows[0, 2], tabs[1][11]) and np.array_equal(rows[0, 3], tabs[3][13])


def test_a_sample_below_the_threshold_is_unaffected():
    m = _model([(2, 11), (4, 13)])
    flags, served = m.batch(np.array([[5, 11, 12, 14]], np.int32), 2)        # one hit
    assert flags.tolist() == [[0, 1, 0, 0]]
    assert served == [[(1, 5), (2, 11), (3, 12), (4, 14)]]
    assert m.resident() == {(2, 11): 1, (4, 13): 1, (1, 5): 1, (3, 12): 1, (4, 14): 1}
    assert m.approx_counters() == {"calls": 1, "samples": 0, "substituted": 0, "zero_rows": 0}
    assert m.n_fetched == 3


def test_a_key_approximated_by_one_sample_and_missed_by_another_is_inserted_once_at_the_others_count():
    m = _model([(2, 11), (4, 13), (1, 7), (2, 21)])
    rq = np.array([[5, 11, 12, 13],      # agg 2: (1, 5) and (3, 12) approximated
                   [5, 22, 12, 14],      # agg 0: (1, 5), (2, 22), (3, 12), (4, 14) missed at count 0
                   [7, 23, 12, 15],      # agg 1: (3, 12) missed at count 1
                   [7, 21, 12, 13]], np.int32)   # agg 3: (3, 12) approximated
    flags, served = m.batch(rq, 2)
    assert flags.tolist() == [[2, 1, 2, 1], [0, 0, 0, 0], [1, 0, 0, 0], [1, 1, 2, 1]]
    assert served[0] == [None, (2, 11), (2, 11), (4, 13)] and served[3] == [(1, 7), (2, 21), (2, 21), (4, 13)]
    res = m.resident()
    assert res[(3, 12)] == 1 and res[(1, 5)] == 0, "the maximum over the positions that were not approximated"
    assert res[(4, 13)] == 3 and res[(2, 11)] == 2 and res[(1, 7)] == 3 and res[(2, 21)] == 3
    assert len(res) == 4 + 6 and m.size() == 10
    assert m.approx_counters() == {"calls": 1, "samples": 2, "substituted": 2, "zero_rows": 1}


def test_an_index_out_of_range_is_no_key_and_never_approximated():
    m = _model([(2, 11), (4, 13), (3, 1)])
    flags, served = m.batch(np.array([[-1, 11, 70, 13], [50, 11, 1, 13]], np.int32), 2)
    assert flags.tolist() == [[0, 1, 0, 1], [0, 1, 1, 1]]
    assert served[0] == [None, (2, 11), None, (4, 13)]
    assert set(m.resident()) == {(2, 11), (4, 13), (3, 1)}
    assert m.approx_counters() == {"calls": 1, "samples": 0, "substituted": 0, "zero_rows": 0}
    assert m.n_perfect == 0


@pytest.mark.parametrize("name", sorted(A.STREAMS))
def test_thres_T_equals_the_mode_off_and_the_plain_model(name):
    """a sample at thres = T has no miss: the same flags and state as thres = 0, and as BagEvLFUModel with one index per bag"""
    g = A.STREAMS[name]
    rows = A.stream(name)[0]
    on, off = A.BatchApproxModel(g["cap"], list(g["n_rows"])), A.BatchApproxModel(g["cap"], list(g["n_rows"]))
    plain = EM.BagEvLFUModel(g["cap"], list(g["n_rows"]))
    for rq in rows[:4]:
        f1, s1 = on.batch(rq, g["T"])
        f0, s0 = off.batch(rq, 0)
        fp = np.stack(plain.batch_bags(*EM.one_per_bag(rq)), 1)
        assert np.array_equal(f1, f0) and s1 == s0 and not (f1 == 2).any()
        assert np.array_equal(f0.astype(bool), fp)
        assert on.resident() == off.resident() == plain.resident() and on.base_counters() == off.base_counters()
        assert (off.n_hits, off.n_perfect, off.n_evict) == (plain.n_hits, plain.n_perfect, plain.n_evict)
    assert on.approx_counters() == {"calls": 4, "samples": 0, "substituted": 0, "zero_rows": 0}
    assert off.approx_counters() == {"calls": 0, "samples": 0, "substituted": 0, "zero_rows": 0}


@pytest.mark.parametrize("name", sorted(A.STREAMS))
def test_the_gpu_streams_cover_what_they_are_for(name):
    g = A.STREAMS[name]
    rows, flags, served, model, top = A.stream(name)
    nb, B, T = rows.shape
    assert (nb, B, T) == (g["n_batches"], g["B"], g["T"]) and 6 <= nb <= 10
    two = flags == 2
    approximated = two.any(2)
    assert approximated.mean() >= 0.10, "at least 10 % of the samples are approximated"
    assert (~approximated).mean() >= 0.10, "and at least 10 % are not"
    n_zero = sum(1 for i in range(nb) for b in range(B) for t in range(T) if two[i, b, t] and served[i][b][t] is None)
    assert n_zero >= 1 and int(two.sum()) - n_zero >= 1, "a zero-row and a substituted position"
    assert model.approx_counters() == {"calls": nb, "samples": int(approximated.sum()), "substituted": int(two.sum()) - n_zero, "zero_rows": n_zero}
    assert top < int(0.95 * g["cap"]), "the top bucket stays below the flush"
    assert model.n_turned == 0 and model.n_evict > 0 and model.n_fetched > 0
    # conflict-free under THIS model: replaying the stream, no call brings two inserted keys to one set
    replay = A.BatchApproxModel(g["cap"], list(g["n_rows"]))
    for i in range(nb):
        assert not A.insert_conflicts(replay, rows[i], g["thres"])
        f, s = replay.batch(rows[i], g["thres"])
        assert np.array_equal(f, flags[i]) and s == served[i]
    assert replay.resident() == model.resident()
    # ... and the non-approximating model's state diverges from it
    plain = EM.BagEvLFUModel(g["cap"], list(g["n_rows"]))
    for i in range(nb):
        plain.batch_bags(*EM.one_per_bag(rows[i]))
    assert plain.resident() != model.resident()


def test_the_toggled_stream_approximates_where_the_threshold_is_on():
    """the stream of test_setting_toggled_and_alternated_with_a_bag_call: every call conflict-free under its own threshold, the
    approximating calls approximate, the others and the bag calls do not"""
    g = A.STREAMS["G26"]
    rows, final = A.toggle_stream()
    m = A.BatchApproxModel(g["cap"], list(g["n_rows"]))
    n_on = 0
    for i, what in enumerate(A.TOGGLE_PLAN):
        thres = 0 if what == "bags" else what
        assert not A.insert_conflicts(m, rows[i], thres)
        before = m.approx_counters()
        if what == "bags":
            m.batch_bags(*EM.one_per_bag(rows[i]))
        else:
            flags, _ = m.batch(rows[i], what)
            assert bool((flags == 2).any()) == (what > 0 and i > 0), "call %d" % (i + 1)
        n_on += thres > 0
        assert (m.approx_counters() != before) == (thres > 0)
    assert m.resident() == final.resident() and m.approx_counters() == final.approx_counters()
    assert m.a_calls == n_on == 4 and m.a_sub > 0 and m.a_zero > 0 and m.top_bucket() < int(0.95 * g["cap"])


def test_entries_of_a_hand_made_state_lie_in_their_sets():
    m = _model([(2, 11), (4, 13), (1, 7)], prio=2)
    e = m.entries()
    assert e.shape == (3, 5) and (e[:, 2] == 2).all() and (e[:, 3] == 1).all()
    for t1, row, _sc, _age, slot in e.tolist():
        assert slot // M.WAYS == int(M.set_of(t1 - 1, row, m.nset, N_ROWS, m.bits))
