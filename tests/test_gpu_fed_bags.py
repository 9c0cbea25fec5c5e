"""Ragged bags over fed backing (evs_cache_fed_begin_bags / _fed_finish_bags / _fed_finish_bags_interact; include/evstore_hip.h):
the count-first fetch-first bag chain cut in two.  The begin probes the flat position list without writing a way word (EvLFU: and
counts the samples' served bags) and hands back every distinct missing key of a fed table once; the caller supplies the rows; the
finish touches / raises, inserts from the fed block, re-points and pools.

The twin throughout is a second cache over the same tables in HBM at order 1 (EvLFU: bag rule + count-first), driven through
lookup_bags[_interact]: flags, pooled bits / R, dump, batch_stats with hist and fetch_stats must be equal on every call whose
outcome does not depend on timing.  Geometries, tables, streams and numpy pooling: tests/_fed_bags_common.py, computed once."""
import numpy as np
import pytest
import torch

import _bag_evlfu_model as EM
import _batched_policy_model as M
import _fed_backing_common as F
import _fed_bags_common as H

pytestmark = pytest.mark.gpu

GEOMS, POLICIES, N_BATCHES = H.GEOMS, H.POLICIES, H.N_BATCHES
_dev, _dump, _bits, _refused = F._dev, F._dump, F._bits, F._refused


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

    def __init__(self, raws, rb):
        self.flat, self.rb, self.seen = [np.ascontiguousarray(r).view(np.uint8).reshape(-1, rb) for r in raws], rb, []

    def __call__(self, keys):
        assert keys.dtype == np.uint64 and keys.ndim == 1
        self.seen.append(keys.copy())
        t = (keys >> np.uint64(32)).astype(np.int64) - 1
        r = (keys & np.uint64(0xffffffff)).astype(np.int64)
        out = np.empty((len(keys), self.rb), np.uint8)
        for k in np.unique(t):
            out[t == k] = self.flat[k][r[t == k]]
        return out

    def rows(self, keys):
        """the device block of a key tensor (None for an empty list); not remembered"""
        if keys.numel() == 0:
            return None
        seen = len(self.seen)
        out = torch.from_numpy(self(keys.cpu().numpy().view(np.uint64))).cuda()
        del self.seen[seen:]
        return out


def _bag_settings(c, policy):
    if policy == "evlfu":
        c.set_bag_rule("served-bags")
        c.set_bag_count("count-first")
    return c


def _cache_twin(E, policy, geom, codec, raws=None):
    g = GEOMS[geom]
    raws = H.tables(geom, codec)[0] if raws is None else raws
    c = E.GpuCache(policy, g["cap"], g["T"], g["d"], codec).set_miss_order("fetch-first")
    c.set_backing([_dev(r) for r in raws])
    return _bag_settings(c, policy)


def _cache_fed(E, policy, geom, codec, fed=None, raws=None, source=False, order="fetch-first", settings=True):
    """-> (the fed cache, its source -- set on the cache when `source`); fed: the fed tables (default: all of them)"""
    g = GEOMS[geom]
    raws = H.tables(geom, codec)[0] if raws is None else raws
    fed = set(range(g["T"])) if fed is None else set(fed)
    c = E.GpuCache(policy, g["cap"], g["T"], g["d"], codec)
    if order is not None:
        c.set_miss_order(order)
    assert c.set_fed_backing([None if t in fed else _dev(raws[t]) for t in range(g["T"])], g["n_rows"]) is c
    src = _Source(raws, _row_bytes(geom, codec))
    if source:
        assert c.set_row_source(src, bags=True) is c
    return (_bag_settings(c, policy) if settings else c), src


def _up(off, idx):
    return [_dev(o) for o in off], [_dev(i) for i in idx]


def _np_pooled(ly):
    return torch.stack([t for t in ly]).cpu().numpy()


def _np_flags(hits):
    return [h.cpu().numpy().astype(bool) for h in hits]


def _check_list(keys, idx, flags, n_rows, fed):
    got = [int(k) for k in keys.cpu().numpy()]
    assert len(set(got)) == len(got), "a key is listed twice"
    assert set(got) == H.want_keys(idx, flags, n_rows, fed)
    return len(got)


def _fed_call(c, src, off, idx, x=None):
    """begin -> the source -> finish on a fed cache -> (flags, pooled (T, B, d) or R, the key tensor)"""
    lS_o, lS_i = _up(off, idx)
    hits, keys = c.lookup_bags_begin(lS_o, lS_i)
    keys = keys.clone()
    fed = src.rows(keys)
    out = _np_pooled(c.lookup_bags_finish(fed)) if x is None else c.lookup_bags_finish_interact(fed, x).cpu().numpy()
    return _np_flags(hits), out, keys


def _twin_call(c, off, idx, x=None):
    lS_o, lS_i = _up(off, idx)
    if x is None:
        hits, ly = c.lookup_bags(lS_o, lS_i)
        return _np_flags(hits), _np_pooled(ly)
    hits, R = c.lookup_bags_interact(lS_o, lS_i, x)
    return _np_flags(hits), R.cpu().numpy()


def _same_state(a, b, what=""):
    assert _dump(a) == _dump(b), what + ": resident sets and scores"
    assert a.batch_stats() == b.batch_stats(), what + ": statistics"
    assert a.fetch_stats() == b.fetch_stats(), what + ": fetch statistics"


def _index_error_once(E):
    L = E._lib
    assert L.lib().evs_check_index_errors(None) == L.EVS_EINDEX
    assert L.lib().evs_check_index_errors(None) == 0


# ------------------------------------------------------------------------------------------- 1. twins on conflict-free streams
def _twins(E, policy, geom, codec, form, fed=None):
    g = GEOMS[geom]
    T, d, B = g["T"], g["d"], g["B"]
    n_rows = list(g["n_rows"])
    fed = list(range(T)) if fed is None else fed
    calls = H.stream(policy, geom)
    _, tabs = H.tables(geom, codec)
    b = _cache_twin(E, policy, geom, codec)
    c, src = _cache_fed(E, policy, geom, codec, fed)
    model = H.new_model(policy, geom)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)
    n_keys = n_missed = 0
    for i, (off, idx, want_flags) in enumerate(calls):
        model.batch_bags(off, idx)
        x = torch.empty(B, d, device="cuda").uniform_(-1, 1, generator=gen) if form == "interact" else None
        fb, ob = _twin_call(b, off, idx, x)
        fc, oc, keys = _fed_call(c, src, off, idx, x)
        for t in range(T):
            assert np.array_equal(fc[t], fb[t]) and np.array_equal(fc[t], want_flags[t]), "call %d, table %d: flags" % (i + 1, t)
        assert np.array_equal(_bits(oc), _bits(ob)), "call %d: the fed cache's output differs from the twin's" % (i + 1)
        if form == "bags":
            assert np.array_equal(_bits(oc), _bits(H.np_pool(tabs, off, idx, B))), "call %d: pooled rows" % (i + 1)
        n_keys += _check_list(keys, idx, fc, n_rows, fed)
        assert all((int(k) >> 32) - 1 in fed for k in keys.cpu().numpy())
        n_missed += sum(int(((np.asarray(idx[t]) >= 0) & (np.asarray(idx[t]) < n_rows[t]) & ~fc[t]).sum()) for t in fed)
        assert _dump(c) == _dump(b) == model.resident(), "call %d: resident sets" % (i + 1)
    _same_state(c, b, "after the stream")
    s = c.batch_stats()
    assert s["n_evict"] > 0 and s["n_hits"] > 0 and s["n_flush"] == 0
    assert (s["n_requests"], s["n_hits"], s["n_perfect_hits"]) == (model.n_requests, model.n_hits, model.n_perfect)
    fs = c.fed_stats()
    assert fs["calls"] == N_BATCHES and fs["keys"] == n_keys and fs["missed"] == n_missed
    if len(fed) == T:
        f = c.fetch_stats()
        assert fs["from_block"] == f["in_place"] and fs["missed"] == f["in_place"] + f["repointed"]


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("geom,codec,form", [("G1", 32, "bags"), ("G1", 32, "interact"), ("G1", 8, "bags"), ("G2", 4, "bags"), ("G2", 16, "bags")])
def test_twins_on_conflict_free_bag_streams(E, policy, geom, codec, form):
    """Every table fed, twelve calls.  Per call: flags equal the twin's and the model's; pooled / R bits equal the twin's, pooled
    equal numpy pooling over the table rows; the key list, as a set and without a duplicate, is the distinct valid missed keys of
    the fed tables computed from flags and indices.  After the stream dump, batch_stats with hist and fetch_stats are equal and
    fed_stats adds up.  (The streams themselves are held to an eviction, no flush and a listed key named by two samples:
    _fed_bags_common.stream.)"""
    _twins(E, policy, geom, codec, form)


# ---------------------------------------------------------------------------------------------------------------- 2. mixed
@pytest.mark.parametrize("policy", POLICIES)
def test_mixed_addressed_and_fed_tables(E, policy):
    """G2 with table 1 addressed in HBM and tables 0 and 2 fed: the list names tables 0 and 2 only, everything else as above."""
    _twins(E, policy, "G2", 32, "bags", fed=[0, 2])


# ------------------------------------------------------------------------------------------------ 3. one key, listed once
@pytest.mark.parametrize("policy", POLICIES)
def test_one_key_in_most_positions_is_listed_once(E, policy):
    """A call of 2 400 positions over all three tables' bags (ten blocks of the walk): 1 500 of them name row 77 of the
    3000-row table, missing, spread over every sample's bag; the rest are a handful of other keys.  n_keys is exact and every
    position is served its row."""
    g = GEOMS["G2"]
    T, B, n_rows = g["T"], g["B"], list(g["n_rows"])
    _, tabs = H.tables("G2", 32)
    c, src = _cache_fed(E, policy, "G2", 32)
    rs = np.random.RandomState(5)
    few = [np.array([1, 3]), np.array([77, 500, 900, 1200]), np.array([4, 9, 33])]
    sets = [H.set_of("G2", (t + 1, int(r))) for t in range(T) for r in few[t]]
    assert max(np.bincount(sets)) <= 8                             # (every key finds a way: nothing depends on timing)
    sizes = {0: 300, 1: 1800, 2: 300}
    idx, off = [], []
    for t in range(T):
        col = few[t][rs.randint(0, len(few[t]), sizes[t])].astype(np.int64)
        if t == 1:
            col[rs.permutation(sizes[t])[:1500]] = 77
        cuts = np.sort(rs.randint(0, sizes[t] + 1, B - 1))
        idx.append(col)
        off.append(np.concatenate([[0], cuts]).astype(np.int64))
    assert sum(len(i) for i in idx) >= 2000 and int((idx[1] == 77).sum()) * 2 > sum(len(i) for i in idx)
    flags, out, keys = _fed_call(c, src, off, idx)
    assert not any(f.any() for f in flags)
    assert _check_list(keys, idx, flags, n_rows, range(T)) == sum(len(np.unique(i)) for i in idx)
    assert np.array_equal(_bits(out), _bits(H.np_pool(tabs, off, idx, B)))
    assert c.fed_stats() == {"calls": 1, "keys": int(keys.numel()), "missed": sum(len(i) for i in idx), "from_block": 0}
    flags, out, keys = _fed_call(c, src, off, idx)
    assert all(f.all() for f in flags) and keys.numel() == 0
    assert np.array_equal(_bits(out), _bits(H.np_pool(tabs, off, idx, B)))


# -------------------------------------------------------------------------------------------------------------- 4. crowded
@pytest.mark.parametrize("policy", POLICIES)
def test_crowded_sets_pool_from_the_fed_block(E, policy):
    """G1C (8 sets), a fresh cache, one call with 13 new keys of set 0, each named by one position (and a few keys of other
    sets): 8 take the set's ways, 5 are turned away and pooled straight from the fed block.  from_block equals the twin's
    in-place count, pooled bits are the table rows -- whichever five lost."""
    g = GEOMS["G1C"]
    T, B, n_rows = g["T"], g["B"], list(g["n_rows"])
    _, tabs = H.tables("G1C", 32)
    nset, bits = M.geometry(g["cap"], g["n_rows"])
    bags, n0 = {}, 0
    for t in range(T):
        rows = np.arange(n_rows[t])
        in0 = rows[M.set_of(t, rows, nset, n_rows, bits) == 0]
        out0 = rows[M.set_of(t, rows, nset, n_rows, bits) == 1 + t % 7]   # (at most four new keys for each of the other sets)
        take = in0[:1] if n0 < 13 and len(in0) else in0[:0]
        n0 += len(take)
        bags[(t % B, t)] = list(take) + list(out0[:1])
        bags[((t + 7) % B, t)] = list(out0[:1])
    assert n0 == 13
    off, idx = H.call_of(B, T, bags)
    b = _cache_twin(E, policy, "G1C", 32)
    c, src = _cache_fed(E, policy, "G1C", 32)
    fb, ob = _twin_call(b, off, idx)
    fc, oc, keys = _fed_call(c, src, off, idx)
    assert not any(f.any() for f in fc) and all(np.array_equal(a, bb) for a, bb in zip(fc, fb))
    _check_list(keys, idx, fc, n_rows, range(T))
    want = H.np_pool(tabs, off, idx, B)
    assert np.array_equal(_bits(oc), _bits(want)) and np.array_equal(_bits(ob), _bits(want))
    f, fs = b.fetch_stats(), c.fed_stats()
    assert f["in_place"] == 5 and fs["from_block"] == f["in_place"] == c.fetch_stats()["in_place"]
    assert fs["missed"] == sum(len(i) for i in idx) == f["in_place"] + f["repointed"]
    assert c.batch_stats() == b.batch_stats() and len(_dump(c)) == len(_dump(b))
    before = _dump(c)
    fc, oc, keys = _fed_call(c, src, off, idx)                     # the five come back as misses, the set is full of this batch's peers' ways
    assert all(np.array_equal(fc[t], np.array([(t + 1, int(r)) in before for r in idx[t]], bool)) for t in range(T))
    assert np.array_equal(_bits(oc), _bits(want))


# ---------------------------------------------------------------------------------------------------------- 5. whose bytes
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("codec", [32, 8])
def test_served_rows_are_the_fed_bytes(E, policy, codec):
    """The source feeds rows that differ from the tables the geometry usually has (fp32: the sign flipped; u8: every byte
    complemented): pooled equals numpy pooling, in index order, over what was fed -- in this call and, after the fed block has
    been overwritten, in later calls that hit (fed = None is accepted for an empty list)."""
    from oracle import oracle as orc
    g = GEOMS["G2"]
    T, B, d, n_rows = g["T"], g["B"], g["d"], list(g["n_rows"])
    raws, tabs = H.tables("G2", codec)
    if codec == 32:
        fed_raws = [-t for t in tabs]
        fed_tabs = fed_raws
    else:
        fed_raws = [255 - np.ascontiguousarray(r).view(np.uint8) for r in raws]
        fed_tabs = [orc.decode(r, 8, d) for r in fed_raws]
    c, src = _cache_fed(E, policy, "G2", codec, raws=fed_raws)
    off, idx, _ = H.stream(policy, "G2")[0]
    lS_o, lS_i = _up(off, idx)
    hits, keys = c.lookup_bags_begin(lS_o, lS_i)
    assert not any(h.any() for h in hits) and keys.numel() > 0
    rb = _row_bytes("G2", codec)
    wide = torch.full((int(keys.numel()), rb + 48), 0xa5, dtype=torch.uint8, device="cuda")   # rows 48 bytes apart from each other
    fed = wide[:, :rb]
    fed.copy_(src.rows(keys))
    want = H.np_pool(fed_tabs, off, idx, B)
    assert not np.array_equal(_bits(want), _bits(H.np_pool(tabs, off, idx, B)))
    assert np.array_equal(_bits(_np_pooled(c.lookup_bags_finish(fed))), _bits(want))
    torch.cuda.synchronize()
    wide.fill_(0x5a)                                               # the finish has run: the block is the caller's again
    hits, keys = c.lookup_bags_begin(lS_o, lS_i)
    assert all(h.all() for h in hits) and keys.numel() == 0
    assert np.array_equal(_bits(_np_pooled(c.lookup_bags_finish(None))), _bits(want))


# ------------------------------------------------------------------------------------------------ 6. EvLFU hit-and-victim
def test_evlfu_hit_way_is_the_same_calls_victim(E):
    """The directed (B, T) case of tests/_fed_backing_common.py, one index per bag: the last call hits a key and evicts it.  The
    update runs in front of the pooling; the evicted key's pooled row is still its own (the old copy of the two-copy arena), the
    replacing key's row is the row just fed."""
    g = GEOMS["G2"]
    B = g["B"]
    rows, flags, at, old, new, resident = F._victim_hit_case()
    _, tabs = H.tables("G2", 32)
    b = _cache_twin(E, "evlfu", "G2", 32)
    c, src = _cache_fed(E, "evlfu", "G2", 32)
    for i in range(at + 1):
        off, idx = EM.one_per_bag(rows[i])
        fb, ob = _twin_call(b, off, idx)
        fc, oc, keys = _fed_call(c, src, off, idx)
        assert np.array_equal(np.stack(fc, 1), flags[i]) and np.array_equal(np.stack(fb, 1), flags[i]), "call %d: flags" % (i + 1)
        assert np.array_equal(_bits(oc), _bits(H.np_pool(tabs, off, idx, B))) and np.array_equal(_bits(oc), _bits(ob)), "call %d" % (i + 1)
    listed = {int(k) for k in keys.cpu().numpy()}
    assert (new[0] << 32 | new[1]) in listed and (old[0] << 32 | old[1]) not in listed
    assert (rows[at][:, old[0] - 1] == old[1]).any() and (rows[at][:, new[0] - 1] == new[1]).any()
    assert _dump(c) == _dump(b) == resident and c.batch_stats() == b.batch_stats() and c.batch_stats()["n_flush"] == 0


# -------------------------------------------------------------------------------------- 7. what is no key, what is uncovered
@pytest.mark.parametrize("policy", POLICIES)
def test_what_is_no_key_and_what_is_uncovered(E, policy):
    """An index out of range inside a bag: flag 0, pools nothing, not listed, the sticky flag raised once the finish has returned.
    Offsets that start past position 0: the positions in front are uncovered -- a missed key there is listed and resident
    afterwards (EvLFU: at priority 0).  An empty table.  A call with no missing key: no key listed, fed = None."""
    g = GEOMS["G2"]
    L = E._lib
    T, B, n_rows = g["T"], g["B"], list(g["n_rows"])
    _, tabs = H.tables("G2", 32)
    b = _cache_twin(E, policy, "G2", 32)
    c, src = _cache_fed(E, policy, "G2", 32)
    # table 0: positions 0, 1 uncovered (every bag starts at 2 or later); table 1: an index past the table and a negative one;
    # table 2: no index at all
    idx = [np.array([4, 2, 0, 1, 0, 1], np.int64), np.array([10, n_rows[1], 11, -1, 12, 10], np.int64), np.zeros(0, np.int64)]
    off = [np.minimum(2 + np.arange(B), 6).astype(np.int64), np.minimum(np.arange(B) * 2, 6).astype(np.int64), np.zeros(B, np.int64)]
    L.lib().evs_check_index_errors(None)                           # (whatever an earlier test left)
    assert L.lib().evs_check_index_errors(None) == 0
    fb, ob = _twin_call(b, off, idx)
    torch.cuda.synchronize()
    _index_error_once(E)
    fc, oc, keys = _fed_call(c, src, off, idx)
    torch.cuda.synchronize()
    _index_error_once(E)
    assert not any(f.any() for f in fc)
    _check_list(keys, idx, fc, n_rows, range(T))
    assert {int(k) for k in keys.cpu().numpy()} == {(1 << 32) | r for r in (0, 1, 2, 4)} | {(2 << 32) | r for r in (10, 11, 12)}
    want = H.np_pool(tabs, off, idx, B)
    assert np.array_equal(_bits(oc), _bits(want)) and np.array_equal(_bits(ob), _bits(want))
    assert not oc[2].any() and np.array_equal(_bits(oc[1][1]), _bits(tabs[1][11]))   # (bag 1 of table 1: row 11 and a bad index)
    dump = _dump(c)
    assert set(dump) == {(1, 0), (1, 1), (1, 2), (1, 4), (2, 10), (2, 11), (2, 12)}
    if policy == "evlfu":
        assert dump[(1, 4)] == 0 and dump[(1, 2)] == 0             # the uncovered keys
        assert dump[(1, 0)] > 0
    _same_state(c, b, "after the call")
    # no missing key: the same call again but for its bad indices
    idx2 = [idx[0], np.array([10, 11, 12, 10], np.int64), idx[2]]
    off2 = [off[0], np.minimum(np.arange(B) * 2, 4).astype(np.int64), off[2]]
    fb, ob = _twin_call(b, off2, idx2)
    lS_o, lS_i = _up(off2, idx2)
    hits, keys = c.lookup_bags_begin(lS_o, lS_i)
    assert keys.numel() == 0 and all(h.all() for h in hits)
    oc = _np_pooled(c.lookup_bags_finish(None))
    assert np.array_equal(_bits(oc), _bits(H.np_pool(tabs, off2, idx2, B))) and np.array_equal(_bits(oc), _bits(ob))
    torch.cuda.synchronize()
    assert L.lib().evs_check_index_errors(None) == 0
    _same_state(c, b, "after the all-hit call")


# -------------------------------------------------------------------------------------------------------------- 8. long bags
@pytest.mark.parametrize("max_bag", [12, 40])
def test_long_bags(E, max_bag):
    """G3, bags of up to 12 and up to 40 indices: the count pass's 4- and 16-lane groups (a mean above 4 / above 16 per bag)."""
    g = GEOMS["G3"]
    T, B, n_rows = g["T"], g["B"], list(g["n_rows"])
    _, tabs = H.tables("G3", 32)
    model = H.new_model("evlfu", "G3")
    rs = np.random.RandomState(100 + max_bag)

    def draw():
        """the plain draw: the cache holds every key, so the outcome does not depend on timing; bag 19 of table 1 runs past nnz
        and bag 20 goes back -- both empty, their run uncovered"""
        sizes = rs.randint(0, max_bag + 1, size=(B, T))
        idx = [rs.randint(0, n_rows[t], int(sizes[:, t].sum())).astype(np.int64) for t in range(T)]
        off = [np.concatenate([[0], np.cumsum(sizes[:-1, t])]).astype(np.int64) for t in range(T)]
        off[1][20] = 10 ** 6
        return off, idx
    first = draw()
    E._lib.lib().evs_check_index_errors(None)
    b = _cache_twin(E, "evlfu", "G3", 32)
    c, src = _cache_fed(E, "evlfu", "G3", 32)
    for i, (off, idx) in enumerate([first, first, draw()]):
        mean = sum(len(ix) for ix in idx) / float(T * B)
        assert (4 < mean <= 16) if max_bag == 12 else mean > 16
        want_flags = model.batch_bags(off, idx)
        fb, ob = _twin_call(b, off, idx)
        fc, oc, keys = _fed_call(c, src, off, idx)
        torch.cuda.synchronize()
        _index_error_once(E)                                       # (the bad bags)
        assert all(np.array_equal(fc[t], want_flags[t]) and np.array_equal(fb[t], want_flags[t]) for t in range(T)), "call %d: flags" % (i + 1)
        assert np.array_equal(_bits(oc), _bits(ob)) and np.array_equal(_bits(oc), _bits(H.np_pool(tabs, off, idx, B))), "call %d" % (i + 1)
        _check_list(keys, idx, fc, n_rows, range(T))
    assert _dump(c) == _dump(b) == model.resident()
    _same_state(c, b, "after the stream")
    assert c.batch_stats()["n_perfect_hits"] == model.n_perfect


# ------------------------------------------------------------------------------------------------------- 9. the walk loops
@pytest.mark.parametrize("policy", ["evlfu", "lru"])
def test_the_walk_loops(E, policy):
    """One call of 8192 x 256 + 1 000 positions over G3's tables: the blocks of all four flat kernels take a second pass.  The
    capacity holds every key (no set gets more than 8), so the outcome does not depend on timing: flags, pooled bits and the dump
    equal the twin's."""
    g = GEOMS["G3"]
    T, B, n_rows = g["T"], g["B"], list(g["n_rows"])
    nset, bits = M.geometry(g["cap"], g["n_rows"])
    per_set = np.bincount(np.concatenate([M.set_of(t, np.arange(n_rows[t]), nset, n_rows, bits) for t in range(T)]), minlength=nset)
    assert per_set.max() <= 8
    n_pos = 8192 * 256 + 1000
    rs = np.random.RandomState(11)
    sizes = [n_pos // 3, n_pos // 3, n_pos - 2 * (n_pos // 3)]
    idx = [rs.randint(0, n_rows[t], sizes[t]).astype(np.int64) for t in range(T)]
    off = [np.concatenate([[0], np.sort(rs.randint(0, sizes[t] + 1, B - 1))]).astype(np.int64) for t in range(T)]
    b = _cache_twin(E, policy, "G3", 32)
    c, src = _cache_fed(E, policy, "G3", 32)
    warm = H.call_of(B, T, {(0, t): list(range(0, n_rows[t], 2)) for t in range(T)})   # every other row resident: hits and misses
    _twin_call(b, *warm)
    _fed_call(c, src, *warm)
    lS_o, lS_i = _up(off, idx)
    hb, lb = b.lookup_bags(lS_o, lS_i)
    hc, keys = c.lookup_bags_begin(lS_o, lS_i)
    assert int(keys.numel()) == sum(n // 2 for n in n_rows) == sum(len(np.unique(i[i % 2 == 1])) for i in idx)   # every odd row, once
    lc = c.lookup_bags_finish(src.rows(keys.clone()))
    for t in range(T):
        assert torch.equal(hc[t], hb[t]) and torch.equal(hc[t].cpu(), torch.from_numpy((idx[t] % 2 == 0).astype(np.uint8))), "table %d: flags" % t
        assert torch.equal(lc[t].view(torch.int32), lb[t].view(torch.int32)), "table %d: pooled bits" % t
    assert _dump(c) == _dump(b) and len(_dump(c)) == sum(n_rows)
    assert c.batch_stats() == b.batch_stats() and c.fetch_stats() == b.fetch_stats()


# --------------------------------------------------------------------------------------- 10. the protocol and the envelope
def _serves(c, src, tabs, geom, seed):
    """a cold-then-warm pair of bag calls: pooled rows exact; the second call's flags are residency in the dump taken before it"""
    g = GEOMS[geom]
    rs = np.random.RandomState(seed)
    off, idx = H.call_of(g["B"], g["T"], {(b, t): list(rs.randint(0, g["n_rows"][t], 2)) for b in range(3) for t in range(g["T"])})
    want = H.np_pool(tabs, off, idx, g["B"])
    _, out, _ = _fed_call(c, src, off, idx)
    assert np.array_equal(_bits(out), _bits(want))
    before = _dump(c)
    flags, out, _ = _fed_call(c, src, off, idx)
    assert np.array_equal(_bits(out), _bits(want))
    res = [np.array([(t + 1, int(r)) in before for r in idx[t]], bool) for t in range(g["T"])]
    assert all(np.array_equal(a, b) for a, b in zip(flags, res)) and any(r.any() for r in res)


@pytest.mark.parametrize("policy", POLICIES)
def test_the_envelope(E, policy):
    """Every refusal carries its code and names the policy, and the cache serves afterwards: order 0; EvLFU without the bag rule /
    without count-first (naming the setter); the one-call bag forms without a row source; B = 0; a NULL index array with nnz > 0."""
    L = E._lib
    g = GEOMS["G2"]
    T, B, d = g["T"], g["B"], g["d"]
    _, tabs = H.tables("G2", 32)
    off, idx = _up(*H.stream(policy, "G2")[0][:2])
    seed = iter(range(100, 200))
    c, src = _cache_fed(E, policy, "G2", 32, order=None, settings=False)
    msg = _refused(E, L.EVS_EINVAL, policy, lambda: c.lookup_bags_begin(off, idx))
    assert "fetch-first" in msg and "evs_cache_set_miss_order" in msg
    c.set_miss_order("fetch-first")
    if policy == "evlfu":
        assert "evs_cache_set_bag_rule" in _refused(E, L.EVS_EINVAL, policy, lambda: c.lookup_bags_begin(off, idx))
        c.set_bag_rule("served-bags")
        assert "evs_cache_set_bag_count" in _refused(E, L.EVS_EINVAL, policy, lambda: c.lookup_bags_begin(off, idx))
        c.set_bag_count("count-first")
    _serves(c, src, tabs, "G2", next(seed))
    # the one-call forms, no source set: the library's refusal comes through and names the new calls
    x = torch.zeros(B, d, device="cuda")
    assert "evs_cache_fed_begin_bags" in _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags(off, idx))
    assert "evs_cache_fed_begin_bags" in _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags_interact(off, idx, x))
    c.set_row_source(src)                                          # ... and with a source that was not given for bags
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags(off, idx))
    assert not src.seen
    c.set_row_source(src, bags=True)
    hits, ly = c.lookup_bags(off, idx)
    assert np.array_equal(_bits(_np_pooled(ly)), _bits(H.np_pool(tabs, *H.stream(policy, "G2")[0][:2], B)))
    c.set_row_source(None)
    # argument checks of the bag form, before anything is allocated
    empty = [torch.zeros(0, dtype=torch.int64, device="cuda")] * T
    _refused(E, L.EVS_EINVAL, None, lambda: c.lookup_bags_begin(empty, empty))                  # B = 0
    st = torch.cuda.current_stream().cuda_stream
    import ctypes as C
    arr = (C.c_void_p * T)(*[o.data_ptr() for o in off])
    nul = (C.c_void_p * T)(*([None] * T))
    nnz = (C.c_int64 * T)(*[int(i.numel()) for i in idx])
    n = C.c_int64()
    kb = torch.empty(4096, dtype=torch.int64, device="cuda")
    assert L.lib().evs_cache_fed_begin_bags(c._h, B, nul, arr, nnz, None, kb.data_ptr(), C.byref(n), st) == L.EVS_EINVAL
    assert b"indices[0] is NULL" in L.lib().evs_last_error()
    assert L.lib().evs_cache_fed_begin_bags(c._h, B, arr, arr, nnz, None, kb.data_ptr() + 4, C.byref(n), st) == L.EVS_EINVAL
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_abort())    # (none of them opened a call)
    _serves(c, src, tabs, "G2", next(seed))
    # a cache without a fed table
    plain = _cache_twin(E, policy, "G2", 32)
    _refused(E, L.EVS_ESTATE, policy, lambda: plain.lookup_bags_begin(off, idx))
    plain.lookup_bags(off, idx)


@pytest.mark.parametrize("policy", POLICIES)
def test_the_protocol(E, policy):
    """A finish of the other form is EVS_ESTATE, names the right call and leaves the call open; a second begin of either form and
    every other call are refused while a bag call is open; argument errors of the finish are EVS_EINVAL and leave it open."""
    L = E._lib
    g = GEOMS["G2"]
    T, B, d, n_rows = g["T"], g["B"], g["d"], g["n_rows"]
    rb = d * 4
    _, tabs = H.tables("G2", 32)
    st = torch.cuda.current_stream().cuda_stream
    calls = H.stream(policy, "G2")
    c, src = _cache_fed(E, policy, "G2", 32)
    out = torch.empty(T, B, d, device="cuda")
    assert L.lib().evs_cache_fed_finish_bags(c._h, None, 0, out.data_ptr(), B * d, d, st) == L.EVS_ESTATE
    assert policy.encode() in L.lib().evs_last_error()
    for i in range(3):
        _fed_call(c, src, *calls[i][:2])
    off, idx = calls[3][:2]
    lS_o, lS_i = _up(off, idx)
    rows = _dev(np.zeros((B, T), np.int32))
    x = torch.zeros(B, d, device="cuda")
    # a (B, T) call is open: the bag finishes name the (B, T) ones and leave it open
    hit, keys = c.lookup_begin(rows)
    fed = src.rows(keys.clone())
    assert "evs_cache_fed_finish " in _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags_finish(fed)).replace("/", " ")
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags_finish_interact(fed, x))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags_begin(lS_o, lS_i))
    c.lookup_finish(fed)
    # a bag call is open
    hits, keys = c.lookup_bags_begin(lS_o, lS_i)
    keys = keys.clone()
    assert any(h.any() for h in hits) and keys.numel() > 0
    fed = src.rows(keys)
    assert "evs_cache_fed_finish_bags" in _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_finish(fed))
    assert "evs_cache_fed_finish_bags" in _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_finish_interact(fed, x))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags_begin(lS_o, lS_i))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_begin(rows))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.batch_stats())
    with pytest.raises(E._lib.EvsError) as ei:
        c.batch_dump()
    assert ei.value.code == L.EVS_ESTATE
    _refused(E, L.EVS_ESTATE, policy, lambda: c.refresh_rows(np.array([[0, 1]], np.int64)))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.set_fed_backing([None] * T, n_rows))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.set_backing([_dev(t) for t in tabs]))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.export_state())
    c.set_row_source(src, bags=True)
    n_seen = len(src.seen)
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags(lS_o, lS_i))       # (through the row source: its begin is the second one)
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags_interact(lS_o, lS_i, x))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_batch(rows))
    assert len(src.seen) == n_seen
    c.set_row_source(None)
    # argument errors of the finish leave it open
    lib = L.lib()
    assert lib.evs_cache_fed_finish_bags(c._h, None, rb, out.data_ptr(), B * d, d, st) == L.EVS_EINVAL and b"NULL fed" in lib.evs_last_error()
    assert lib.evs_cache_fed_finish_bags(c._h, fed.data_ptr() + 4, rb, out.data_ptr(), B * d, d, st) == L.EVS_EINVAL
    assert lib.evs_cache_fed_finish_bags(c._h, fed.data_ptr(), rb + 4, out.data_ptr(), B * d, d, st) == L.EVS_EINVAL
    assert lib.evs_cache_fed_finish_bags(c._h, fed.data_ptr(), rb - 16, out.data_ptr(), B * d, d, st) == L.EVS_EINVAL and b"below" in lib.evs_last_error()
    assert lib.evs_cache_fed_finish_bags(c._h, fed.data_ptr(), rb, out.data_ptr() + 4, B * d, d, st) == L.EVS_EINVAL
    assert lib.evs_cache_fed_finish_bags(c._h, fed.data_ptr(), rb, out.data_ptr(), B * d + 2, d, st) == L.EVS_EINVAL
    R = torch.empty(B, d + (T + 1) * T // 2, device="cuda")
    assert lib.evs_cache_fed_finish_bags_interact(c._h, fed.data_ptr(), rb, x.data_ptr() + 4, d, 0, R.data_ptr(), st) == L.EVS_EINVAL
    got = _np_pooled(c.lookup_bags_finish(fed))
    assert np.array_equal(_bits(got), _bits(H.np_pool(tabs, off, idx, B)))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_abort())
    _serves(c, src, tabs, "G2", 7)
    # hit = NULL: the cache's own flag bytes serve the call
    import ctypes as C
    off, idx = calls[4][:2]
    lS_o, lS_i = _up(off, idx)
    before = _dump(c)
    idx_c = (C.c_void_p * T)(*[t.data_ptr() if t.numel() else None for t in lS_i])
    off_c = (C.c_void_p * T)(*[t.data_ptr() for t in lS_o])
    nnz_c = (C.c_int64 * T)(*[int(t.numel()) for t in lS_i])
    kb = torch.empty(sum(len(i) for i in idx), dtype=torch.int64, device="cuda")
    n = C.c_int64()
    assert lib.evs_cache_fed_begin_bags(c._h, B, idx_c, off_c, nnz_c, None, kb.data_ptr(), C.byref(n), st) == 0
    keys = kb[:n.value].clone()
    assert n.value > 0 and sorted(keys.tolist()) == sorted({((t + 1) << 32) | int(r) for t in range(T) for r in idx[t] if (t + 1, int(r)) not in before})
    fed = src.rows(keys)
    assert lib.evs_cache_fed_finish_bags(c._h, fed.data_ptr(), rb, out.data_ptr(), B * d, d, st) == 0
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(H.np_pool(tabs, off, idx, B)))
    # destroy with an open bag call is fine
    c.lookup_bags_begin(lS_o, lS_i)
    del c


# ---------------------------------------------------------------------------------------------- 11. an abort leaves no trace
@pytest.mark.parametrize("policy", POLICIES)
def test_an_abort_leaves_no_trace(E, policy):
    """Two fed caches on the conflict-free stream; after three calls one of them begins a DIFFERENT call (the stream's fifth: hits
    among its positions) and drops it -- twice: the same begin gives the same key set.  The begin wrote no way word: dump (scores
    included) and batch_stats with hist are what they were, and equal the other cache's there and after every further call of the
    stream -- no touch, raise or stamp of the dropped probe is left to steer a victim choice."""
    g = GEOMS["G2"]
    T, B = g["T"], g["B"]
    _, tabs = H.tables("G2", 32)
    calls = H.stream(policy, "G2")
    c1, src = _cache_fed(E, policy, "G2", 32)
    c2, _ = _cache_fed(E, policy, "G2", 32)
    for i in range(3):
        for c in (c1, c2):
            _fed_call(c, src, *calls[i][:2])
    s0, d0, f0, fs0 = c1.batch_stats(), _dump(c1), c1.fetch_stats(), c1.fed_stats()
    lS_o, lS_i = _up(*calls[4][:2])
    listed = []
    for _ in range(2):
        hits, keys = c1.lookup_bags_begin(lS_o, lS_i)
        assert any(h.any() for h in hits) and keys.numel() > 0
        listed.append((sorted(int(k) for k in keys.cpu().numpy()), [h.cpu().numpy().copy() for h in hits]))
        c1.lookup_abort()
        assert c1.batch_stats() == s0 == c2.batch_stats() and _dump(c1) == d0 == _dump(c2)
        assert c1.fetch_stats() == f0 and c1.fed_stats() == fs0
    assert listed[0][0] == listed[1][0] and all(np.array_equal(a, b) for a, b in zip(listed[0][1], listed[1][1]))
    for i in range(3, N_BATCHES):
        off, idx, want_flags = calls[i]
        f1, o1, _ = _fed_call(c1, src, off, idx)
        f2, o2, _ = _fed_call(c2, src, off, idx)
        assert all(np.array_equal(f1[t], want_flags[t]) and np.array_equal(f2[t], want_flags[t]) for t in range(T)), "call %d: flags" % (i + 1)
        assert np.array_equal(_bits(o1), _bits(H.np_pool(tabs, off, idx, B))) and np.array_equal(_bits(o1), _bits(o2))
        _same_state(c1, c2, "call %d" % (i + 1))
    assert c1.fed_stats() == c2.fed_stats()


# ------------------------------------------------------------------------------- 12. bag calls alternate with (B, T) calls
@pytest.mark.parametrize("policy", POLICIES)
def test_bag_calls_alternate_with_bt_calls(E, policy):
    """One fed cache takes bag calls and (B, T) calls in turn (through the row source), its twin lookup_bags / lookup_batch: they
    share stamp, ordinal, counters and the pending flush, so flags, outputs, dump and statistics agree call by call."""
    g = GEOMS["G2"]
    T, B = g["T"], g["B"]
    _, tabs = H.tables("G2", 32)
    b = _cache_twin(E, policy, "G2", 32)
    c, src = _cache_fed(E, policy, "G2", 32, source=True)
    n_calls = 0
    for i, call in enumerate(H.mixed_stream(policy, "G2")):
        if call[0] == "bags":
            _, off, idx, want_flags = call
            lS_o, lS_i = _up(off, idx)
            (hb, lb), (hc, lc) = b.lookup_bags(lS_o, lS_i), c.lookup_bags(lS_o, lS_i)
            assert all(np.array_equal(a, w) and np.array_equal(a2, w) for a, a2, w in zip(_np_flags(hc), _np_flags(hb), want_flags)), "call %d: flags" % (i + 1)
            assert np.array_equal(_bits(_np_pooled(lc)), _bits(H.np_pool(tabs, off, idx, B))), "call %d: pooled rows" % (i + 1)
            assert np.array_equal(_bits(_np_pooled(lc)), _bits(_np_pooled(lb)))
        else:
            _, rows, want_flags = call
            r = _dev(rows)
            (hb, ob), (hc, oc) = b.lookup_batch(r), c.lookup_batch(r)
            assert np.array_equal(hc.cpu().numpy().astype(bool), want_flags) and torch.equal(hb, hc), "call %d: flags" % (i + 1)
            F._rows_exact(oc.cpu().numpy(), tabs, rows)
            assert torch.equal(ob.view(torch.int32), oc.view(torch.int32))
        n_calls += 1
        _same_state(c, b, "call %d" % (i + 1))
    s = c.batch_stats()
    assert s["n_flush"] == 0 and s["n_evict"] > 0
    assert c.fed_stats()["calls"] == n_calls == c.fetch_stats()["calls"]


# --------------------------------------------------------------------------------------------------------------- 13. files
@pytest.mark.parametrize("policy", POLICIES)
def test_file_tier_as_the_row_source(E, policy, tmp_path):
    """.bin tables behind FileTier(paths, row_bytes, 0) -- nothing registered, every table staged -- and
    set_row_source(tier.fetch, bags=True), the fetch function unchanged: lookup_bags and lookup_bags_interact give the twin's
    results on the G2 stream."""
    g = GEOMS["G2"]
    T, d, B = g["T"], g["d"], g["B"]
    _, tabs = H.tables("G2", 32)
    paths = []
    for k, t in enumerate(tabs):
        p = tmp_path / ("ev-table-%d.bin" % (k + 1))
        t.tofile(p)
        paths.append(str(p))
    tier = E.FileTier(paths, d * 4, 0)
    assert not any(tier.registered)
    c = E.GpuCache(policy, g["cap"], T, d, 32).set_miss_order("fetch-first")
    _bag_settings(c.set_fed_backing([None] * T, tier.n_rows).set_row_source(tier.fetch, bags=True), policy)
    b = _cache_twin(E, policy, "G2", 32)
    x = torch.empty(B, d, device="cuda").uniform_(-1, 1)
    for i, (off, idx, want_flags) in enumerate(H.stream(policy, "G2")):
        lS_o, lS_i = _up(off, idx)
        if i % 2 == 0:
            (hb, ob), (hc, oc) = b.lookup_bags(lS_o, lS_i), c.lookup_bags(lS_o, lS_i)
            ob, oc = _np_pooled(ob), _np_pooled(oc)
            assert np.array_equal(_bits(oc), _bits(H.np_pool(tabs, off, idx, B))), "call %d: pooled rows" % (i + 1)
        else:
            (hb, ob), (hc, oc) = b.lookup_bags_interact(lS_o, lS_i, x), c.lookup_bags_interact(lS_o, lS_i, x)
            ob, oc = ob.cpu().numpy(), oc.cpu().numpy()
        assert all(np.array_equal(a, w) for a, w in zip(_np_flags(hc), want_flags)), "call %d: flags" % (i + 1)
        assert np.array_equal(_bits(oc), _bits(ob)), "call %d" % (i + 1)
    _same_state(c, b, "after the stream")
    tier.close()
