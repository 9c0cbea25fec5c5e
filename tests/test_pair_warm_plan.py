"""CPU: the placement plan of the pair's warm start (evs_cache_pair_load_plan -- pure host code, the function
evs_cache_pair_load runs) held to its Python restatement (tests/_pair_warm_model.py): on the five record shapes the geometry
formula gives (8 + 2 x 8, 8 + 12, 8 + 6, 4 + 2 x 8, 8 + 4 ways), strict and non-strict, over-full sets, ages past the stamp
width, and every refusal the header lists.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _pair_warm_model as P

N_ROWS = [40, 1000, 5000]
T = len(N_ROWS)
# (cap1, cap2) -> (nset, C1 ways, C2 ways, C2 sub-sets)
SHAPES = {(64, 128): (8, 8, 8, 2), (64, 96): (8, 8, 12, 1), (48, 40): (6, 8, 6, 1), (32, 128): (8, 4, 8, 2), (128, 64): (16, 8, 4, 1)}
CAPS = list(SHAPES)


def _lib():
    import evstore_dlrm_amd as E
    return E._lib, E._lib.lib()


def c_plan(caps, entries, state=None, strict=False, n_rows1=N_ROWS, n_rows2=N_ROWS):
    """-> (rc, dest, words, out8, message); the outputs are pre-filled so that a refusal can be seen to leave them alone"""
    L, lib = _lib()
    entries = np.ascontiguousarray(np.asarray(entries, np.int64).reshape(-1, 6))
    n = entries.shape[0]
    r1, r2 = np.asarray(n_rows1, np.int64), np.asarray(n_rows2, np.int64)
    dest, words, out8 = np.full(max(n, 1), -7, np.int64), np.full(max(n, 1), 0xABCD, np.uint32), np.full(8, -7, np.int64)
    st = None if state is None else np.ascontiguousarray(state, np.int64)
    rc = lib.evs_cache_pair_load_plan(caps[0], caps[1], len(n_rows1), r1.ctypes.data, r2.ctypes.data, n, entries.ctypes.data if n else None,
                                      None if st is None else st.ctypes.data, int(strict), dest.ctypes.data, words.ctypes.data, out8.ctypes.data)
    return rc, dest[:n], words[:n], out8, lib.evs_last_error().decode()


def check_against_model(caps, entries, state=None, strict=False):
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    rc, dest, words, out8, msg = c_plan(caps, entries, state, strict)
    assert rc == 0, msg
    mdest, mwords, mout8 = P.plan(geom, entries, state, strict)
    assert np.array_equal(dest, mdest)
    assert np.array_equal(words, mwords)
    assert list(out8) == mout8
    return dest, words, out8


@pytest.mark.parametrize("caps", CAPS)
def test_the_model_has_the_shapes_the_formula_gives(caps):
    g = P.Geometry(caps[0], caps[1], N_ROWS)
    assert (g.nset, g.tiers[0].ways, g.tiers[1].ways, 1 << g.tiers[1].sub_shift) == SHAPES[caps]
    assert g.tiers[0].sub_shift == 0 and g.tiers[1].w_off == (g.tiers[0].ways + 3) // 4 * 4
    # every slot of both tiers has a word of its own inside the 32-word record
    at = [g.word_index(k, s) for k in (1, 2) for s in range(g.n_slots(k))]
    assert len(set(at)) == len(at) and max(at) < g.nset * 32 and g.n_slots(1) <= caps[0] and g.n_slots(2) <= caps[1]
    # the plan reports the model's stamp widths
    rc, _d, _w, out8, msg = c_plan(caps, np.zeros((0, 6), np.int64))
    assert rc == 0 and list(out8) == [0, 0, g.tiers[0].S, 0, 0, g.tiers[1].S, 0, 0], msg


@pytest.mark.parametrize("caps", [(16, 128), (256, 64)])
def test_capacities_without_a_shared_record_are_refused(caps):
    L, _ = _lib()
    with pytest.raises(P.Refused):
        P.Geometry(caps[0], caps[1], N_ROWS)
    rc, _d, _w, out8, msg = c_plan(caps, np.array([[1, 1, 3, 0, 0, 0]], np.int64))
    assert rc == L.EVS_EINVAL and "4 ways" in msg and np.all(out8 == -7)


@pytest.mark.parametrize("caps", CAPS)
def test_an_overfull_set_keeps_the_best_ways_of_each_tier(caps):
    """effective set 3 of C1 and effective set 5 of C2 each get ways + 3 candidates with hand-made (score, age): the `ways` best
    of (score descending, age ascending, table, row) take ways 0 .. ways - 1, three are turned away per tier, and the input
    order decides nothing"""
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    rows, want = [], {}
    taken = set()
    for tier, es in ((1, 3), (2, 5)):
        ways = geom.tiers[tier - 1].ways
        keys = P.keys_of_set(geom, tier, es, ways + 3, skip=taken)
        taken |= set(keys)
        sa = [((7 * j) % 4 % (T + 1), (5 * j) % 6) for j in range(ways + 3)]
        order = sorted(range(ways + 3), key=lambda j: (-sa[j][0], sa[j][1], keys[j]))
        for rank, j in enumerate(order):
            want[(tier,) + keys[j]] = es * ways + rank if rank < ways else -1
        rows += [[tier, k[0], k[1], s, a, 0] for k, (s, a) in zip(keys, sa)]
    entries = np.array(rows, np.int64)
    for perm in (np.arange(len(rows)), np.arange(len(rows))[::-1], np.random.RandomState(1).permutation(len(rows))):
        dest, words, out8 = check_against_model(caps, entries[perm])
        assert [want[tuple(e[:3])] for e in entries[perm].tolist()] == dest.tolist()
        assert list(out8[[0, 1, 3, 4]]) == [geom.tiers[0].ways, 3, geom.tiers[1].ways, 3]
        assert np.all(words[dest < 0] == 0) and np.all(words[dest >= 0] != 0)
        assert out8[6] == 5                                            # without a state: the largest age, for both tiers


@pytest.mark.parametrize("caps", CAPS)
def test_ages_are_clamped_per_tier_and_strict_keeps_them(caps):
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    S1, S2 = geom.tiers[0].S, geom.tiers[1].S
    entries = np.array([[1, 1, 10, 2, 10 ** 7, 0], [1, 2, 11, 2, (1 << S1) - 1, 0], [1, 3, 12, 2, 1, 0],
                        [2, 2, 13, 1, 10 ** 7, 0], [2, 3, 14, 1, (1 << S2) - 2, 0], [2, 1, 15, 0, 0, 0]], np.int64)
    dest, words, out8 = check_against_model(caps, entries)
    assert out8[6] == max((1 << S1) - 2, (1 << S2) - 2) and np.all(dest >= 0)
    for i, e in enumerate(entries):                                    # no loaded way carries the next batch's stamp
        t = geom.tiers[e[0] - 1]
        assert (int(words[i]) >> t.tag_bits) & ((1 << t.S) - 1) != P.cur_stamp(t.S, int(out8[6]) + 1), i
    st = P.state_of(geom, n=12345)
    _d, _w, out8 = check_against_model(caps, entries, st)
    assert out8[6] == 12345
    back = entries.copy()
    back[:, 5] = dest
    d2, w2, out8 = check_against_model(caps, back, P.state_of(geom, n=77), strict=True)     # ages as they are, modulo 2^S
    assert np.array_equal(d2, dest) and out8[6] == 77


@pytest.mark.parametrize("caps", CAPS)
def test_random_lists_agree_with_the_model_entry_for_entry(caps):
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    rs = np.random.RandomState(sum(caps))
    turned = [0, 0]
    for case in range(40):
        n1, n2 = int(rs.randint(0, 3 * caps[0])), int(rs.randint(0, 3 * caps[1]))
        S = min(geom.tiers[0].S, geom.tiers[1].S)
        entries = P.random_entries(rs, geom, n1, n2, int(rs.choice([4, 1 << S, 1 << (S + 3)])))
        state = P.state_of(geom, n=int(rs.randint(0, 1 << 20)), counters=(1, 2, 3, 4, 5)) if case % 2 else None
        dest, words, out8 = check_against_model(caps, entries, state)
        turned[0] += int(out8[1])
        turned[1] += int(out8[4])
        for k in (1, 2):
            placed = dest[(entries[:, 0] == k) & (dest >= 0)]
            assert len(set(placed.tolist())) == len(placed) == out8[3 * k - 3] and (len(placed) == 0 or placed.max() < geom.n_slots(k))
        assert out8[0] + out8[1] == n1 and out8[3] + out8[4] == n2
        if case % 4 == 1:           # what was placed goes back strictly, word for word
            back = entries[dest >= 0].copy()
            back[:, 5] = dest[dest >= 0]
            for k in (1, 2):
                m = back[:, 0] == k
                back[m, 4] = np.minimum(back[m, 4], (1 << geom.tiers[k - 1].S) - 2)
            d2, w2, _o = check_against_model(caps, back, state, strict=True)
            assert np.array_equal(d2, dest[dest >= 0]) and np.array_equal(w2, words[dest >= 0])
    assert turned[0] > 0 and turned[1] > 0           # (the lists do overfill sets of both tiers)


@pytest.mark.parametrize("caps", [(64, 128), (64, 96)])
def test_every_refusal_names_its_reason_and_plans_nothing(caps):
    L, _ = _lib()
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    good = np.array([[1, 1, 3, 1, 2, 0], [1, 2, 999, 0, 0, 0], [2, 3, 4999, 3, 7, 0], [2, 2, 17, 2, 1, 0]], np.int64)
    dest, _w, _o = check_against_model(caps, good)
    strict_good = good.copy()
    strict_good[:, 5] = dest
    st = P.state_of(geom, n=9)
    check_against_model(caps, strict_good, st, strict=True)

    def refused(entries, state=None, strict=False, word=None):
        rc, d, w, out8, msg = c_plan(caps, entries, state, strict)
        assert rc == L.EVS_EINVAL, msg
        assert "evs_cache_pair_load_plan" in msg and (word is None or word in msg), msg
        assert np.all(out8 == -7) and np.all(d == -7) and np.all(w == 0xABCD)      # the outputs are untouched
        with pytest.raises(P.Refused):
            P.plan(geom, entries, state, strict)

    def with_(i, col, v, base=good):
        e = base.copy()
        e[i, col] = v
        return e

    def st_(pos, v):
        s = st.copy()
        s[pos] = v
        return s

    refused(with_(0, 0, 0), word="tier")
    refused(with_(0, 0, 3), word="tier")
    refused(with_(0, 1, 0), word="table")
    refused(with_(0, 1, T + 1), word="table")
    refused(with_(1, 2, -1), word="row")
    refused(with_(1, 2, 1000), word="row")
    refused(with_(0, 2, 40), word="row")                               # (in range for the other tables)
    refused(with_(2, 3, -1), word="score")
    refused(with_(2, 3, T + 1), word="score")
    refused(with_(3, 4, -1), word="age")
    refused(np.concatenate([good, good[1:2]]), word="duplicate")       # a key twice in C1
    refused(np.concatenate([good, good[3:4]]), word="duplicate")       # ... in C2
    both = good[1:2].copy()
    both[0, 0] = 2
    refused(np.concatenate([good, both]), word="both tiers")           # a key in both tiers
    for version in (1, 2, 0):
        refused(good, st_(0, version), word="version")
    v1 = np.array([1, 0, caps[0], T, 36, 8, 9, 0, 0, 0, 0, 0, geom.tiers[0].S, 0, -1, 0] + [0] * 16, np.int64)   # a single tier's state16
    refused(good, v1, word="version")
    refused(strict_good, None, True, word="strict")
    # strict: the exporter's geometry, per tier
    for pos in (1, 3, P.TIER0 + P.B_CAP, P.TIER0 + P.B_WAYS, P.TIER0 + P.B_SUBS, P.TIER0 + P.B_S,
                P.TIER0 + P.BLOCK + P.B_CAP, P.TIER0 + P.BLOCK + P.B_WAYS, P.TIER0 + P.BLOCK + P.B_SUBS, P.TIER0 + P.BLOCK + P.B_S):
        refused(strict_good, st_(pos, st[pos] + 1), True, word="geometry")
        assert c_plan(caps, good, st_(pos, st[pos] + 1), False)[0] == 0          # ... which only a strict load holds the pair to
    # strict: a slot outside its key's effective set (the same way of the next set), outside the tier, taken twice
    for i in (0, 2):
        ways = geom.tiers[good[i, 0] - 1].ways
        refused(with_(i, 5, (strict_good[i, 5] + ways) % geom.n_slots(int(good[i, 0])), strict_good), st, True, word="slot")
        refused(with_(i, 5, -1, strict_good), st, True, word="slot")
        refused(with_(i, 5, geom.n_slots(int(good[i, 0])), strict_good), st, True, word="slot")
    es = geom.place(1, 0, 3)[0]
    twin = P.keys_of_set(geom, 1, es, 1, skip={(1, 3)})[0]
    two = np.concatenate([strict_good, [[1, twin[0], twin[1], 0, 0, strict_good[0, 5]]]])
    refused(two, st, True, word="slot")


def test_tiers_over_tables_of_different_lengths_share_the_larger_universe():
    """C2's tables are shorter: a row past C2's table is refused for tier 2 and fine for tier 1, and the universe (the row bases)
    comes from the larger count per table"""
    L, _ = _lib()
    rows2 = [40, 600, 5000]
    e1 = np.array([[1, 2, 700, 1, 0, 0]], np.int64)
    e2 = np.array([[2, 2, 700, 1, 0, 0]], np.int64)
    geom = P.Geometry(64, 128, N_ROWS, rows2)
    rc, dest, words, out8, msg = c_plan((64, 128), e1, n_rows2=rows2)
    md, mw, mo = P.plan(geom, e1)
    assert rc == 0 and np.array_equal(dest, md) and np.array_equal(words, mw) and list(out8) == mo, msg
    rc, _d, _w, _o, msg = c_plan((64, 128), e2, n_rows2=rows2)
    assert rc == L.EVS_EINVAL and "row" in msg


def test_bad_plan_arguments():
    L, lib = _lib()
    rows = np.asarray(N_ROWS, np.int64)
    e = np.array([[1, 1, 3, 0, 0, 0]], np.int64)
    d, w, o = np.zeros(1, np.int64), np.zeros(1, np.uint32), np.zeros(8, np.int64)
    tail = (e.ctypes.data, None, 0, d.ctypes.data, w.ctypes.data, o.ctypes.data)
    assert lib.evs_cache_pair_load_plan(64, 128, 0, rows.ctypes.data, rows.ctypes.data, 1, *tail) == L.EVS_EINVAL
    assert lib.evs_cache_pair_load_plan(64, 128, 3, None, rows.ctypes.data, 1, *tail) == L.EVS_EINVAL
    assert lib.evs_cache_pair_load_plan(0, 128, 3, rows.ctypes.data, rows.ctypes.data, 1, *tail) == L.EVS_EINVAL and b"capacities" in lib.evs_last_error()
    assert lib.evs_cache_pair_load_plan(64, 128, 3, rows.ctypes.data, rows.ctypes.data, -1, *tail) == L.EVS_EINVAL
    assert lib.evs_cache_pair_load_plan(64, 128, 3, rows.ctypes.data, rows.ctypes.data, 1, None, None, 0, d.ctypes.data, w.ctypes.data, o.ctypes.data) == L.EVS_EINVAL
    assert lib.evs_cache_pair_load_plan(64, 128, 3, rows.ctypes.data, rows.ctypes.data, 0, None, None, 0, None, None, o.ctypes.data) == 0
    # the C ABI refuses bad handles before it touches a device
    buf = (C.c_int64 * 32)()
    assert lib.evs_cache_pair_export(None, None, None, 0, None, None) == L.EVS_EINVAL and b"evs_cache_pair_export" in lib.evs_last_error()
    assert lib.evs_cache_pair_load(None, None, 0, None, None, 0, None, None) == L.EVS_EINVAL and b"NULL cache" in lib.evs_last_error()
    assert lib.evs_cache_pair_load(None, None, -1, buf, None, 0, None, None) == L.EVS_EINVAL and b"negative" in lib.evs_last_error()
    assert lib.evs_cache_pair_load(None, None, 1, buf, buf, 2, None, None) == L.EVS_EINVAL and b"strict" in lib.evs_last_error()
