"""Several calls open at once on a fed cache (evs_cache_set_fed_depth; include/evstore_hip.h there): a begin probes the tier as it
stands, holds every way it hits until the call ends, finishes come oldest first, an abort drops the newest.  Driven serially a
depth-4 cache must be its depth-1 twin call by call; pipelined it must be tests/_fed_ahead_model.py, flag for flag and way for
way, on streams whose outcome does not depend on timing; directed cases pin a held way that survives, a set whose eight ways are
all held, a key two open calls both missed, the abort, the protocol and the lookup_stream driver.

Geometries, tables and helpers are tests/_fed_backing_common.py's; the row source is test_gpu_fed_backing.py's, restated."""
import numpy as np
import pytest
import torch

import _batched_policy_model as M
import _fed_ahead_model as A
import _fed_backing_common as H

pytestmark = pytest.mark.gpu

GEOMS, POLICIES, N_BATCHES = H.GEOMS, H.POLICIES, H.N_BATCHES
_dev, _dump, _bits, _rows_exact, _refused = H._dev, H._dump, H._bits, H._rows_exact, H._refused


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _row_bytes(geom, codec):
    return GEOMS[geom]["d"] * codec // 8


class _Source:
    """a row source over encoded host tables: a numpy gather; remembers the keys of every call"""

    def __init__(self, raws, rb, alter=None):
        self.flat = [np.ascontiguousarray(r).view(np.uint8).reshape(-1, rb) for r in raws]
        self.rb, self.alter, self.seen = rb, alter, []

    def __call__(self, keys):
        assert keys.dtype == np.uint64 and keys.ndim == 1
        self.seen.append(keys.copy())
        t = (keys >> np.uint64(32)).astype(np.int64) - 1
        r = (keys & np.uint64(0xffffffff)).astype(np.int64)
        out = np.empty((len(keys), self.rb), np.uint8)
        for k in np.unique(t):
            out[t == k] = self.flat[k][r[t == k]]
        return out if self.alter is None else self.alter(out)


def _cache_d(E, policy, geom, codec, depth=None, alter=None):
    """-> (a fed cache, every table fed, with its source set and its depth given; the source)"""
    g = GEOMS[geom]
    raws, _ = H._tables(geom, codec)
    c = E.GpuCache(policy, g["cap"], g["T"], g["d"], codec).set_miss_order("fetch-first")
    c.set_fed_backing([None] * g["T"], g["n_rows"])
    src = _Source(raws, _row_bytes(geom, codec), alter)
    c.set_row_source(src)
    if depth is not None:
        assert c.set_fed_depth(depth) is c
    return c, src


def _cache_b(E, policy, geom, codec):
    raws, _ = H._tables(geom, codec)
    return H._cache(E, policy, geom, codec, [_dev(r) for r in raws], order="fetch-first")


def _want_keys(rq, flags, n_rows):
    want = set()
    for t in range(rq.shape[1]):
        col = rq[:, t].astype(np.int64)
        ok = (col >= 0) & (col < n_rows[t]) & ~flags[:, t]
        want |= {((t + 1) << 32) | int(r) for r in col[ok]}
    return want


def _check_list(keys, rq, flags, n_rows):
    got = [int(k) for k in keys]
    assert len(set(got)) == len(got), "a key is listed twice"
    assert set(got) == _want_keys(rq, flags, n_rows)


def _fed_of(src, keys):
    """the source's rows for a begin's keys in a device block of the call's own (None for an empty list)"""
    if keys.numel() == 0:
        return None
    return torch.from_numpy(src(keys.cpu().numpy().view(np.uint64))).cuda()


def _state(c):
    return _dump(c), c.batch_stats(), c.fetch_stats(), c.fed_stats()


def _x(gen, B, d):
    return torch.empty(B, d, device="cuda").uniform_(-1, 1, generator=gen)


# ------------------------------------------------------------------------------------------------ 1. serial equals today
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("geom,codec", [("G1", 32), ("G2", 8)])
def test_driven_serially_a_deep_cache_is_its_depth_1_twin(E, policy, geom, codec):
    """begin, finish, begin, finish at depth 4 against a depth-1 twin over the conflict-free stream, lookup_finish and
    lookup_finish_interact alternating: flags, output bits, dump, batch_stats, fetch_stats and fed_stats equal call by call, and
    fed_ahead_stats all zero: no call was ever begun behind another."""
    g = GEOMS[geom]
    reqs, want_flags = H._bt_stream(policy, geom)
    _, tabs = H._tables(geom, codec)
    c4, s4 = _cache_d(E, policy, geom, codec, depth=4)
    c1, s1 = _cache_d(E, policy, geom, codec)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)
    for i in range(N_BATCHES):
        r = _dev(reqs[i])
        x = _x(gen, g["B"], g["d"]) if i % 2 else None
        res = []
        for c, s in ((c4, s4), (c1, s1)):
            hit, keys = c.lookup_begin(r)
            assert c.fed_open_calls() == 1
            fed = _fed_of(s, keys)
            out = c.lookup_finish(fed) if x is None else c.lookup_finish_interact(fed, x)
            assert c.fed_open_calls() == 0
            res.append((hit.cpu().numpy().astype(bool), out.cpu().numpy(), sorted(int(k) for k in keys)))
        assert np.array_equal(res[0][0], want_flags[i]) and np.array_equal(res[1][0], want_flags[i]), "call %d: flags" % (i + 1)
        assert np.array_equal(_bits(res[0][1]), _bits(res[1][1])), "call %d: output bits" % (i + 1)
        assert res[0][2] == res[1][2], "call %d: the lists" % (i + 1)
        if x is None:
            _rows_exact(res[0][1], tabs, reqs[i])
        assert _state(c4) == _state(c1), "call %d: dump and statistics" % (i + 1)
    assert c4.fed_ahead_stats() == {"ahead_begins": 0, "hold_bits": 0, "found_installed": 0}
    assert c4.batch_stats()["n_evict"] > 0


# ------------------------------------------------------------------------------------------- 2. pipelined against the model
def _pipelined(E, policy, geom, codec, depth, drive):
    """the searched stream of (policy, geom, depth) through `drive`, which yields per call (index, flags, out, x or None, keys or
    None) in the order of the finishes; everything the model pins is compared"""
    g = GEOMS[geom]
    n_rows = list(g["n_rows"])
    reqs, want_flags, model, info = A.searched_stream(policy, g["cap"], g["n_rows"], g["B"], N_BATCHES, depth)
    assert info["passed_over"] >= 1 and info["found_installed"] >= 1, "the stream does not exercise the feature"
    _, tabs = H._tables(geom, codec)
    c, src = _cache_d(E, policy, geom, codec, depth=depth)
    b = _cache_b(E, policy, geom, codec)
    done = 0
    for i, flags, out, x, keys in drive(c, src, reqs):
        assert i == done, "finishes come oldest first"
        done += 1
        assert np.array_equal(flags, want_flags[i]), "call %d: flags" % (i + 1)
        if keys is not None:
            _check_list(keys, reqs[i], flags, n_rows)
        if x is None:
            _rows_exact(out, tabs, reqs[i])
        else:                                                      # the same bytes through the same kernel
            _, Rb = b.lookup_interact(_dev(reqs[i]), x)
            assert np.array_equal(_bits(out), _bits(Rb.cpu().numpy())), "call %d: R" % (i + 1)
    assert done == N_BATCHES and c.fed_open_calls() == 0
    assert _dump(c) == model.resident(), "the resident set after the drain"
    s = c.batch_stats()
    assert s["n_flush"] == 0 and s["size"] == len(model.m.where) and s["n_evict"] == model.m.n_evict
    assert (s["n_requests"], s["n_hits"], s["n_perfect_hits"]) == (model.n_requests, model.n_hits, model.n_perfect)
    if policy == "evlfu":
        assert s["hist"] == model.m.hist()
    a = c.fed_ahead_stats()
    assert a["found_installed"] == model.found_installed and a["ahead_begins"] == model.ahead_begins == N_BATCHES - 1
    assert a["hold_bits"] > 0
    assert c.fed_stats()["calls"] == N_BATCHES


def _manual(depth):
    def drive(c, src, reqs):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(17)
        d, B = c.dim, reqs.shape[1]
        open_calls = {}
        for op, i in A.schedule(len(reqs), depth):
            if op == "begin":
                r = _dev(reqs[i])
                hit, keys = c.lookup_begin(r)
                open_calls[i] = (r, hit, keys, _fed_of(src, keys), _x(gen, B, d) if i % 2 else None)
                assert c.fed_open_calls() == len(open_calls) <= depth
            else:
                r, hit, keys, fed, x = open_calls.pop(i)
                out = c.lookup_finish(fed) if x is None else c.lookup_finish_interact(fed, x)
                yield i, hit.cpu().numpy().astype(bool), out.cpu().numpy(), x, keys.cpu().numpy()
    return drive


@pytest.mark.parametrize("policy,geom,depth,codec", [(p, "G1", 2, 32) for p in POLICIES] + [(p, "G2", 4, 32) for p in POLICIES] + [("evlfu", "G2", 4, 4)])
def test_pipelined_calls_are_the_model(E, policy, geom, depth, codec):
    """Steady state begin k + D - 1, finish k.  Per call: the model's flags, the list as a set equal to the distinct missed keys of
    those flags and without a duplicate, exact rows (plain finishes) or R bit-equal to lookup_interact of a fetch-first cache over
    the same tables in HBM.  After the drain: the model's resident set and scores, the counters it keeps, and fed_ahead_stats'
    third word = the model's records found installed.  The stream is searched so that an update passed over a held way and a
    record was found installed at least once."""
    _pipelined(E, policy, geom, codec, depth, _manual(depth))


# ------------------------------------------------------------------------------------------------- 3. / 4. directed: holds
def _set_keys(geom, table0, s, n, skip=()):
    """n rows of table `table0` whose keys fall into set s"""
    g = GEOMS[geom]
    nset, bits = M.geometry(g["cap"], g["n_rows"])
    rows = np.arange(g["n_rows"][table0])
    rows = rows[M.set_of(table0, rows, nset, list(g["n_rows"]), bits) == s]
    rows = [int(r) for r in rows if int(r) not in skip]
    assert len(rows) >= n
    return rows[:n]


def _filled_set(E, policy, depth=2):
    """G2: a cache and its model with set s holding eight keys of table 1, one brought per serial call (columns 0 and 2 stay on
    one resident key each, in other sets) -> (cache, source, model, s, the eight rows, a ninth row of set s)"""
    g = GEOMS["G2"]
    nset, bits = M.geometry(g["cap"], g["n_rows"])
    others = {int(M.set_of(t, 0, nset, list(g["n_rows"]), bits)) for t in (0, 2)}
    s = next(k for k in range(nset) if k not in others)
    rows9 = _set_keys("G2", 1, s, 9)
    c, src = _cache_d(E, policy, "G2", 32, depth=depth)
    model = A.FedAheadModel(policy, g["cap"], list(g["n_rows"]))
    for r1 in rows9[:8]:
        rq = np.array([[0, r1, 0], [0, r1, 0]], np.int32)
        c.lookup_batch(_dev(rq))
        model.finish(model.begin(rq)[1])
    assert _dump(c) == model.resident() and sum(w is not None for w in model.m.sets[s]) == 8
    return c, src, model, s, rows9[:8], rows9[8]


@pytest.mark.parametrize("policy", POLICIES)
def test_a_held_way_survives(E, policy):
    """Serially the older call's one new key of a full set takes way j.  The newer call, begun behind it, hit the key in way j:
    the new key takes the next-ranked way, the newer call's position is flagged 1 and served its exact row, both keys are
    resident, and the tier is the model's."""
    _, tabs = H._tables("G2", 32)
    c, src, model, s, rows8, new = _filled_set(E, policy)
    model.m.n += 1                                                 # (the way the next batch's new key takes, no way held)
    j = model._rank(model.m.sets[s], s, set(), model.m.n)
    model.m.n -= 1
    kept = model.m.sets[s][j][0]
    p_rq = np.array([[0, new, 0]] * 3, np.int32)
    q_rq = np.array([[0, kept[1], 0]] * 2, np.int32)
    hp, kp = c.lookup_begin(_dev(p_rq))
    hq, kq = c.lookup_begin(_dev(q_rq))
    fp, mp = model.begin(p_rq)
    fq, mq = model.begin(q_rq)
    assert np.array_equal(hp.cpu().numpy().astype(bool), fp) and np.array_equal(hq.cpu().numpy().astype(bool), fq)
    assert fq.all() and [int(k) for k in kp] == [(2 << 32) | new] and kq.numel() == 0
    out_p = c.lookup_finish(_fed_of(src, kp))
    model.finish(mp)
    assert model.passed_over == 1 and model.m.where[(2, new)][1] != j and model.m.where[kept] == (s, j)
    out_q = c.lookup_finish(None)
    model.finish(mq)
    _rows_exact(out_p.cpu().numpy(), tabs, p_rq)
    _rows_exact(out_q.cpu().numpy(), tabs, q_rq)
    d = _dump(c)
    assert kept in d and (2, new) in d and d == model.resident()
    assert c.fed_ahead_stats() == {"ahead_begins": 1, "hold_bits": 3, "found_installed": 0}


@pytest.mark.parametrize("policy", POLICIES)
def test_every_way_held_turns_the_key_away(E, policy):
    """The newer call hits all eight ways of a set, the older call brings one new key to it: the key is turned away and served from
    the fed block -- from_block goes up by its positions, its bytes are exact -- and the set is unchanged."""
    _, tabs = H._tables("G2", 32)
    c, src, model, s, rows8, new = _filled_set(E, policy)
    before = {k for k in _dump(c)}
    fs0 = c.fed_stats()
    p_rq = np.array([[0, new, 0]] * 5, np.int32)
    q_rq = np.array([[0, r1, 0] for r1 in rows8], np.int32)
    hp, kp = c.lookup_begin(_dev(p_rq))
    hq, kq = c.lookup_begin(_dev(q_rq))
    assert hq.all() and kq.numel() == 0 and [int(k) for k in kp] == [(2 << 32) | new]
    out_p = c.lookup_finish(_fed_of(src, kp))
    out_q = c.lookup_finish(None)
    _rows_exact(out_p.cpu().numpy(), tabs, p_rq)
    _rows_exact(out_q.cpu().numpy(), tabs, q_rq)
    fs = c.fed_stats()
    assert fs["from_block"] == fs0["from_block"] + 5 and fs["missed"] == fs0["missed"] + 5
    assert set(_dump(c)) == before and (2, new) not in before
    _, mp = model.begin(p_rq)
    _, mq = model.begin(q_rq)
    model.finish(mp)
    model.finish(mq)
    assert _dump(c) == model.resident()
    assert c.fed_ahead_stats()["hold_bits"] == 8 + 2               # (the eight ways of set s and the two resident keys of columns 0 and 2)


# ----------------------------------------------------------------------------------------------------- 5. both missed
@pytest.mark.parametrize("policy", POLICIES)
def test_a_key_both_calls_missed_is_installed_once(E, policy):
    """Key K is missed by two open calls; the source answers the second time with other bytes.  K is in both lists, resident once
    after both finishes, the newer call's position carries the OLDER call's bytes (the row in the arena was not replaced), and one
    record was found installed."""
    g = GEOMS["G2"]
    _, tabs = H._tables("G2", 32)
    answers = []

    def alter(a):
        answers.append(1)
        return a if len(answers) < 3 else (-a.view(np.float32)).view(np.uint8)

    c, src = _cache_d(E, policy, "G2", 32, depth=2, alter=alter)
    warm = np.array([[0, 5, 0]], np.int32)
    c.lookup_batch(_dev(warm))                                     # answer 1
    K = 77
    rq = np.array([[0, K, 0]], np.int32)
    hp, kp = c.lookup_begin(_dev(rq))
    hq, kq = c.lookup_begin(_dev(rq))
    assert [int(k) for k in kp] == [int(k) for k in kq] == [(2 << 32) | K]
    assert np.array_equal(hp.cpu().numpy(), hq.cpu().numpy()) and hp.cpu().numpy().tolist() == [[1, 0, 1]]
    fed_p, fed_q = _fed_of(src, kp), _fed_of(src, kq)              # answers 2 and 3: the third is altered
    assert not torch.equal(fed_p, fed_q)
    out_p = c.lookup_finish(fed_p).cpu().numpy()
    out_q = c.lookup_finish(fed_q).cpu().numpy()
    _rows_exact(out_p, tabs, rq)
    _rows_exact(out_q, tabs, rq)                                   # the older call's bytes, not the altered ones
    d = _dump(c)
    assert set(d) == {(1, 0), (2, 5), (3, 0), (2, K)}
    assert c.fed_ahead_stats() == {"ahead_begins": 1, "hold_bits": 2, "found_installed": 1}
    assert c.fed_stats()["keys"] == 3 + 1 + 1


# ----------------------------------------------------------------------------------------------------------- 6. abort
@pytest.mark.parametrize("policy", POLICIES)
def test_an_abort_leaves_no_trace_at_depth_2(E, policy):
    """Begin P, begin Q, abort Q, (Q again: the same flags and keys; abort), finish P: dump with scores, batch_stats, fetch_stats and
    fed_stats are those of a depth-1 twin that never saw Q, there and after every further batch of the stream.  Then P open, Q
    open, abort, abort: the cache is as before P."""
    reqs, want_flags = H._bt_stream(policy, "G2")
    _, tabs = H._tables("G2", 32)
    c1, s1 = _cache_d(E, policy, "G2", 32, depth=2)
    c2, _ = _cache_d(E, policy, "G2", 32)
    for i in range(3):
        for c in (c1, c2):
            c.lookup_batch(_dev(reqs[i]))
    rp, rq = _dev(reqs[3]), _dev(reqs[5])
    hp, kp = c1.lookup_begin(rp)
    hq, kq = c1.lookup_begin(rq)
    hq0, kq0 = hq.cpu().numpy().copy(), sorted(int(k) for k in kq)
    assert hq0.any() and kq0 and c1.fed_open_calls() == 2
    c1.lookup_abort()
    assert c1.fed_open_calls() == 1
    hq, kq = c1.lookup_begin(rq)
    assert np.array_equal(hq.cpu().numpy(), hq0) and sorted(int(k) for k in kq) == kq0
    c1.lookup_abort()
    out = c1.lookup_finish(_fed_of(s1, kp))
    assert np.array_equal(hp.cpu().numpy().astype(bool), want_flags[3])
    _rows_exact(out.cpu().numpy(), tabs, reqs[3])
    c2.lookup_batch(rp)
    assert _state(c1) == _state(c2)
    for i in range(4, 8):
        r = _dev(reqs[i])
        (h1, o1), (h2, o2) = c1.lookup_batch(r), c2.lookup_batch(r)
        assert np.array_equal(h1.cpu().numpy().astype(bool), want_flags[i]) and torch.equal(h1, h2), "call %d: flags" % (i + 1)
        assert _state(c1) == _state(c2), "call %d" % (i + 1)
    before = _state(c1)
    c1.lookup_begin(_dev(reqs[8]))
    c1.lookup_begin(_dev(reqs[9]))
    c1.lookup_abort()
    c1.lookup_abort()
    assert c1.fed_open_calls() == 0 and _state(c1) == before == _state(c2)
    for i in range(8, N_BATCHES):
        r = _dev(reqs[i])
        (h1, o1), (h2, o2) = c1.lookup_batch(r), c2.lookup_batch(r)
        assert np.array_equal(h1.cpu().numpy().astype(bool), want_flags[i]) and torch.equal(h1, h2), "call %d: flags" % (i + 1)
    assert _state(c1) == _state(c2)


# -------------------------------------------------------------------------------------------------------- 7. protocol
@pytest.mark.parametrize("policy", POLICIES)
def test_the_protocol_at_depth(E, policy):
    g = GEOMS["G2"]
    L = E._lib
    T, d, B = g["T"], g["d"], g["B"]
    _, tabs = H._tables("G2", 32)
    reqs, _ = H._bt_stream(policy, "G2")
    c, src = _cache_d(E, policy, "G2", 32)
    r = [_dev(reqs[i]) for i in range(4)]
    if policy == "evlfu":
        c.set_bag_rule("served-bags")
        c.set_bag_count("count-first")
    # the default depth refuses a second begin, in the words of ever
    c.lookup_begin(r[0])
    msg = _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_begin(r[1]))
    assert "a fed call is open" in msg and c.fed_open_calls() == 1
    _refused(E, L.EVS_ESTATE, policy, lambda: c.set_fed_depth(2))
    c.lookup_abort()
    for bad in (0, 5, -1):
        _refused(E, L.EVS_EINVAL, None, lambda: c.set_fed_depth(bad))
    c.set_fed_depth(2)
    h0, k0 = c.lookup_begin(r[0])
    h1, k1 = c.lookup_begin(r[1])
    assert c.fed_open_calls() == 2
    msg = _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_begin(r[2]))
    assert "evs_cache_set_fed_depth" in msg and "2 fed calls" in msg
    # refused with both calls left open
    off, idx = [_dev(np.arange(4, dtype=np.int64))] * T, [_dev(np.zeros(4, np.int64))] * T
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags_begin(off, idx))
    from evstore_dlrm_amd import gpu_cache as GC
    other, _ = _cache_d(E, policy, "G2", 32)
    if policy == "evlfu":
        _refused(E, L.EVS_ESTATE, policy, lambda: GC.lookup_begin_c1c2(c, other, r[2], threshold=2))
        _refused(E, L.EVS_ESTATE, policy, lambda: GC.lookup_begin_c1c2(other, c, r[2], threshold=2))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.set_fed_depth(4))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.batch_stats())
    with pytest.raises(L.EvsError) as ei:
        c.batch_dump()
    assert ei.value.code == L.EVS_ESTATE
    _refused(E, L.EVS_ESTATE, policy, lambda: c.update_rows(np.array([[0, 1]], np.int64), torch.zeros(1, d, device="cuda")))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.set_fed_backing([None] * T, g["n_rows"]))
    assert c.fed_open_calls() == 2
    # finishes come out oldest first: each is fed the rows of its own list and serves its own batch
    out0 = c.lookup_finish(_fed_of(src, k0))
    assert c.fed_open_calls() == 1
    out1 = c.lookup_finish(_fed_of(src, k1))
    assert c.fed_open_calls() == 0
    _rows_exact(out0.cpu().numpy(), tabs, reqs[0])
    _rows_exact(out1.cpu().numpy(), tabs, reqs[1])
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_abort())
    c.set_fed_depth(1)
    c.lookup_begin(r[2])
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_begin(r[3]))
    c.lookup_abort()
    # destroying a cache with two calls open is fine
    c.set_fed_depth(2)
    c.lookup_begin(r[2])
    c.lookup_begin(r[3])
    del c


# ---------------------------------------------------------------------------------------------------- 8. lookup_stream
def _streamed(depth):
    def drive(c, src, reqs):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(17)
        d, B = c.dim, reqs.shape[1]
        xs = [_x(gen, B, d) if i % 2 else None for i in range(len(reqs))]
        items = [_dev(reqs[i]) if xs[i] is None else (_dev(reqs[i]), xs[i]) for i in range(len(reqs))]
        for i, (hit, out) in enumerate(c.lookup_stream(items, depth=depth)):
            yield i, hit.cpu().numpy().astype(bool), out.cpu().numpy(), xs[i], None
    return drive


@pytest.mark.parametrize("policy", POLICIES)
def test_lookup_stream_is_the_manual_loop(E, policy):
    """At depth 2 over the twelve batches lookup_stream yields what the manual loop of test 2 yields: the same stream, the same
    model, the same comparisons."""
    _pipelined(E, policy, "G1", 32, 2, _streamed(2))


def test_lookup_stream_drops_every_open_call_when_the_source_raises(E):
    g = GEOMS["G2"]
    reqs, _ = H._bt_stream("lru", "G2")
    _, tabs = H._tables("G2", 32)
    c, src = _cache_d(E, "lru", "G2", 32, depth=2)
    n = []

    def failing(keys):
        n.append(1)
        if len(n) == 3:
            raise RuntimeError("the store is away")
        return src(keys)

    c.set_row_source(failing)
    got = []
    with pytest.raises(RuntimeError, match="the store is away"):
        for hit, out in c.lookup_stream([_dev(reqs[i]) for i in range(6)]):
            got.append(out)
    assert len(got) >= 1 and c.fed_open_calls() == 0
    c.set_row_source(src)
    hit, out = c.lookup_batch(_dev(reqs[2]))
    _rows_exact(out.cpu().numpy(), tabs, reqs[2])
    assert c.fed_open_calls() == 0
