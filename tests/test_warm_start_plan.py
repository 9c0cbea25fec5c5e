"""CPU: the placement plan of a warm start (evs_cache_load_plan -- pure host code, the function evs_cache_batch_load runs)
held to its Python restatement (tests/_warm_start_model.py) on hand-worked cases, on every refusal the header lists and on
random entry lists across capacities and policies.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _batched_policy_model as M
import _warm_start_model as W

N_ROWS = [40, 1000, 5000]
POLICIES = ["evlfu", "lru", "lfu"]


def _lib():
    import evstore_dlrm_amd as E
    return E._lib, E._lib.lib()


def c_plan(policy, cap, n_rows, entries, state=None, strict=False):
    """-> (rc, dest, words, out4, message)"""
    L, lib = _lib()
    entries = np.ascontiguousarray(np.asarray(entries, np.int64).reshape(-1, 5))
    n = entries.shape[0]
    rows = np.asarray(n_rows, np.int64)
    dest, words, out4 = np.full(max(n, 1), -7, np.int64), np.zeros(max(n, 1), np.uint32), np.full(4, -7, np.int64)
    st = None if state is None else np.ascontiguousarray(state, np.int64)
    rc = lib.evs_cache_load_plan(W.POLICY_ID[policy], cap, len(n_rows), rows.ctypes.data, n, entries.ctypes.data if n else None,
                                 None if st is None else st.ctypes.data, int(strict), dest.ctypes.data, words.ctypes.data, out4.ctypes.data)
    return rc, dest[:n], words[:n], out4, lib.evs_last_error().decode()


def state_of(policy, cap, n_rows, n=0, version=1):
    S = M.stamp_bits_of(policy, cap, n_rows)[2]
    return np.array([version, W.POLICY_ID[policy], cap, len(n_rows), 36, 32, n, 1, 2, 3, 4, 5, S, 0, -1, 0], np.int64)


def keys_of_set(cap, n_rows, s, count):
    """the first `count` keys, in (table, row) order, whose set is s"""
    nset, bits = M.geometry(cap, n_rows)
    out = []
    for t in range(len(n_rows)):
        for row in range(n_rows[t]):
            if W.place(t, row, nset, n_rows, bits)[0] == s:
                out.append((t + 1, row))
                if len(out) == count:
                    return out
    raise AssertionError("too few keys in set %d" % s)


def check_against_model(policy, cap, n_rows, entries, state=None, strict=False):
    rc, dest, words, out4, msg = c_plan(policy, cap, n_rows, entries, state, strict)
    assert rc == 0, msg
    mdest, mwords, mout4 = W.plan(policy, cap, n_rows, entries, state, strict)
    assert np.array_equal(dest, mdest)
    assert np.array_equal(words, mwords)
    assert list(out4) == mout4
    return dest, words, out4


def test_eleven_candidates_of_one_set_keep_the_eight_the_order_says():
    """(score, age) per key, keys k0 < k1 < ... in (table, row) order.  Sorted by score descending, age ascending, key:
    k4 (3, 2), k1 (3, 9) | k6 (2, 1), k2 (2, 4), k3 (2, 4), k10 (2, 7) | k7 (1, 0), k0 (1, 5), k5 (1, 5), k9 (1, 5) | k8 (0, 0):
    the first eight take ways 0 .. 7 in that order, k5, k9 and k8 are turned away."""
    cap, s = 64, 3
    keys = keys_of_set(cap, N_ROWS, s, 11)
    sa = [(1, 5), (3, 9), (2, 4), (2, 4), (3, 2), (1, 5), (2, 1), (1, 0), (0, 0), (1, 5), (2, 7)]
    entries = np.array([[k[0], k[1], sc, age, 0] for k, (sc, age) in zip(keys, sa)], np.int64)
    order = [4, 1, 6, 2, 3, 10, 7, 0]
    want = np.full(11, -1, np.int64)
    for way, k in enumerate(order):
        want[k] = s * 8 + way
    for perm in (np.arange(11), np.arange(11)[::-1], np.random.RandomState(0).permutation(11)):     # the input order decides nothing
        rc, dest, words, out4, msg = c_plan("evlfu", cap, N_ROWS, entries[perm])
        assert rc == 0, msg
        assert np.array_equal(dest, want[perm])
        assert list(out4[:2]) == [8, 3] and np.all(words[dest < 0] == 0) and np.all(words[dest >= 0] != 0)
        check_against_model("evlfu", cap, N_ROWS, entries[perm])
    # the word of way 0: k4's tag, priority 3, stamp = (stamp of batch n) - 2 with n = the largest age = 9
    tb, _dual, S = M.stamp_bits_of("evlfu", cap, N_ROWS)
    nset, bits = M.geometry(cap, N_ROWS)
    w = int(words[list(perm).index(4)])
    assert w & ((1 << tb) - 1) == W.place(keys[4][0] - 1, keys[4][1], nset, N_ROWS, bits)[1]
    assert w >> 26 == 3 and (w >> tb) & ((1 << S) - 1) == (9 + 1 - 2) and (w >> 25) & 1 == 0
    assert out4[3] == 9 and out4[2] == S


@pytest.mark.parametrize("policy", POLICIES)
def test_ages_are_clamped_below_the_next_batchs_stamp(policy):
    cap, n_rows, S_all = M.WRAP_GEOMETRIES["tiny"]
    S = S_all[policy]
    score = {"evlfu": 2, "lru": 0, "lfu": 7}[policy]
    entries = np.array([[1, 10, score, 10 ** 6, 0], [2, 11, score, (1 << S) - 1, 0], [3, 12, score, (1 << S) - 2, 0], [4, 13, score, 1, 0]], np.int64)
    dest, words, out4 = check_against_model(policy, cap, n_rows, entries)
    assert out4[2] == S and out4[3] == (1 << S) - 2          # without a state the batch number is the largest clamped age
    tb = M.stamp_bits_of(policy, cap, n_rows)[0]
    nxt = W.cur_stamp(policy, S, int(out4[3]) + 1)
    low_bits = S - (6 if policy == "lru" else 0)
    for i, w in enumerate(words):
        stamp = (int(w) >> tb) & ((1 << low_bits) - 1)
        if policy == "lru":
            stamp |= (int(w) >> 26) << low_bits
        assert stamp != nxt, "entry %d carries the next batch's stamp" % i
    assert len({int(w) >> tb for w in words[:3]}) == 1               # the three old entries share the clamped stamp
    # with a state the batch number is the state's, the ages still clamped
    st = state_of(policy, cap, n_rows, n=12345)
    _d, _w, out4 = check_against_model(policy, cap, n_rows, entries, st)
    assert out4[3] == 12345
    # a strict load keeps the ages as they are (modulo 2^S)
    st = state_of(policy, cap, n_rows, n=77)
    d0, _w, _o = check_against_model(policy, cap, n_rows, entries)
    strict_entries = entries.copy()
    strict_entries[:, 4] = d0
    check_against_model(policy, cap, n_rows, strict_entries, st, strict=True)


@pytest.mark.parametrize("policy", POLICIES)
def test_strict_places_every_entry_in_its_own_slot_and_refuses_a_foreign_one(policy):
    L, _ = _lib()
    cap = 128
    rs = np.random.RandomState(3)
    entries = W.random_entries(rs, policy, N_ROWS, 60, 500)
    dest, _w, _o = check_against_model(policy, cap, N_ROWS, entries)
    placed = entries[dest >= 0].copy()
    placed[:, 4] = dest[dest >= 0]
    # any free way of the key's own set will do, not only the one re-placement chose
    placed[0, 4] = placed[0, 4] // 8 * 8 + 7 if (placed[0, 4] // 8 * 8 + 7) not in set(placed[1:, 4]) else placed[0, 4]
    st = state_of(policy, cap, N_ROWS, n=900)
    d, w, out4 = check_against_model(policy, cap, N_ROWS, placed, st, strict=True)
    assert np.array_equal(d, placed[:, 4]) and list(out4[:2]) == [len(placed), 0] and out4[3] == 900
    bad = placed.copy()
    bad[5, 4] = (bad[5, 4] + 8) % (cap // 8 * 8)                      # the same way of the NEXT set
    rc, _d, _w, _o, msg = c_plan(policy, cap, N_ROWS, bad, st, True)
    assert rc == L.EVS_EINVAL and "slot" in msg
    with pytest.raises(W.Refused):
        W.plan(policy, cap, N_ROWS, bad, st, True)
    for slot in (-1, cap // 8 * 8):
        bad = placed.copy()
        bad[5, 4] = slot
        assert c_plan(policy, cap, N_ROWS, bad, st, True)[0] == L.EVS_EINVAL
    two = placed.copy()                                                # two keys of one set in one slot
    sets = two[:, 4] // 8
    i, j = next((i, j) for i in range(len(two)) for j in range(i + 1, len(two)) if sets[i] == sets[j])
    two[j, 4] = two[i, 4]
    rc, _d, _w, _o, msg = c_plan(policy, cap, N_ROWS, two, st, True)
    assert rc == L.EVS_EINVAL and "slot" in msg
    with pytest.raises(W.Refused):
        W.plan(policy, cap, N_ROWS, two, st, True)


@pytest.mark.parametrize("policy", POLICIES)
def test_every_refusal_names_its_reason_and_plans_nothing(policy):
    L, _ = _lib()
    cap = 64
    T = len(N_ROWS)
    ok_score = {"evlfu": 1, "lru": 0, "lfu": 5}[policy]
    good = np.array([[1, 3, ok_score, 2, 0], [2, 999, ok_score, 0, 0], [3, 4999, ok_score, 7, 0]], np.int64)
    assert c_plan(policy, cap, N_ROWS, good)[0] == 0

    def refused(entries, state=None, strict=False, word=None):
        rc, dest, _w, out4, msg = c_plan(policy, cap, N_ROWS, entries, state, strict)
        assert rc == L.EVS_EINVAL, msg
        assert "evs_cache_load_plan" in msg and (word is None or word in msg), msg
        assert np.all(out4 == -7)                                      # nothing was reported
        with pytest.raises(W.Refused):
            W.plan(policy, cap, N_ROWS, entries, state, strict)

    def with_(i, col, v):
        e = good.copy()
        e[i, col] = v
        return e

    refused(with_(0, 0, 0), word="table")
    refused(with_(0, 0, T + 1), word="table")
    refused(with_(1, 1, -1), word="row")
    refused(with_(1, 1, 1000), word="row")
    refused(with_(0, 1, 40), word="row")                               # (in range for the other tables)
    refused(np.concatenate([good, good[1:2]]), word="duplicate")
    refused(with_(2, 3, -1), word="age")
    bad_scores = {"evlfu": (-1, T + 1), "lru": (-1, 1), "lfu": (0, 64)}[policy]
    for sc in bad_scores:
        refused(with_(0, 2, sc), word="score")
    refused(good, state_of(policy, cap, N_ROWS, version=2), word="version")
    refused(good, state_of(policy, cap, N_ROWS, version=0), word="version")
    other = [p for p in POLICIES if p != policy][0]
    st = state_of(policy, cap, N_ROWS)
    st[1] = W.POLICY_ID[other]
    refused(good, st, word="policy")
    refused(good, None, True, word="strict")                           # strict without a state
    for pos, v in ((2, 128), (3, T + 1), (12, 3)):                     # capacity, n_tables, S of the exporter
        st = state_of(policy, cap, N_ROWS)
        st[pos] = v
        refused(good, st, True)
        assert c_plan(policy, cap, N_ROWS, good, st, False)[0] == 0    # ... which only a strict load holds the cache to


def test_bad_plan_arguments():
    L, lib = _lib()
    rows = np.asarray(N_ROWS, np.int64)
    e = np.array([[1, 3, 0, 0, 0]], np.int64)
    d, w, o = np.zeros(1, np.int64), np.zeros(1, np.uint32), np.zeros(4, np.int64)
    args = (e.ctypes.data, None, 0, d.ctypes.data, w.ctypes.data, o.ctypes.data)
    assert lib.evs_cache_load_plan(3, 64, 3, rows.ctypes.data, 1, *args) == L.EVS_EINVAL and b"policy" in lib.evs_last_error()
    assert lib.evs_cache_load_plan(0, 64, 0, rows.ctypes.data, 1, *args) == L.EVS_EINVAL
    assert lib.evs_cache_load_plan(0, 64, 3, None, 1, *args) == L.EVS_EINVAL
    assert lib.evs_cache_load_plan(0, 7, 3, rows.ctypes.data, 1, *args) == L.EVS_EINVAL and b"capacity" in lib.evs_last_error()
    assert lib.evs_cache_load_plan(0, 64, 3, rows.ctypes.data, -1, *args) == L.EVS_EINVAL
    assert lib.evs_cache_load_plan(0, 64, 3, rows.ctypes.data, 1, None, None, 0, d.ctypes.data, w.ctypes.data, o.ctypes.data) == L.EVS_EINVAL
    # n = 0 plans nothing and says so
    assert lib.evs_cache_load_plan(0, 64, 3, rows.ctypes.data, 0, None, None, 0, None, None, o.ctypes.data) == 0
    assert list(o) == [0, 0, M.stamp_bits_of("evlfu", 64, N_ROWS)[2], 0]
    # a geometry the set-associative form cannot take: tags of more than 22 bits
    huge = np.asarray([1 << 30] * 3, np.int64)
    assert lib.evs_cache_load_plan(0, 64, 3, huge.ctypes.data, 0, None, None, 0, None, None, o.ctypes.data) == L.EVS_EINVAL


@pytest.mark.parametrize("policy", POLICIES)
def test_two_hundred_random_lists_agree_with_the_model_entry_for_entry(policy):
    rs = np.random.RandomState({"evlfu": 11, "lru": 12, "lfu": 13}[policy])
    geoms = [(64, N_ROWS), (128, N_ROWS), (256, N_ROWS), (72, N_ROWS), M.WRAP_GEOMETRIES["tiny"][:2], M.WRAP_GEOMETRIES["tiny-dual"][:2]]
    turned = 0
    for case in range(200):
        cap, n_rows = geoms[case % len(geoms)]
        S = M.stamp_bits_of(policy, cap, n_rows)[2]
        n = int(rs.randint(0, 3 * cap))
        entries = W.random_entries(rs, policy, [min(r, 3000) for r in n_rows], n, int(rs.choice([4, 1 << S, 1 << (S + 2)])))
        state = state_of(policy, cap, n_rows, n=int(rs.randint(0, 1 << 20))) if case % 2 else None
        dest, words, out4 = check_against_model(policy, cap, n_rows, entries, state)
        turned += int(out4[1])
        placed = dest[dest >= 0]
        assert len(set(placed.tolist())) == len(placed) and out4[0] + out4[1] == n and out4[0] <= cap // 8 * 8
        if case % 4 == 1:       # what was placed goes back strictly, word for word
            back = entries[dest >= 0].copy()
            back[:, 4] = placed
            back[:, 3] = np.minimum(back[:, 3], (1 << S) - 2)
            d2, w2, _o = check_against_model(policy, cap, n_rows, back, state, strict=True)
            assert np.array_equal(d2, placed) and np.array_equal(w2, words[dest >= 0])
    assert turned > 0           # (the lists do overfill sets)
