"""The set-associative cache tier over caller-fed rows (evs_cache_set_fed_backing; evs_cache_fed_begin / _fed_finish;
include/evstore_hip.h).  A fed table has no address the GPU reads: the begin probes and hands back the distinct missing keys,
the caller supplies their rows, the finish runs update -> re-point -> consumers.  On conflict-free streams a fed cache D must
agree with cache B -- the same tables in HBM, fetch-first -- flag for flag, bit for bit, way for way and counter for counter,
and with the Python models; directed cases pin the list, a crowded set (rows served straight from the fed block), whose bytes
are served, the EvLFU way that is hit and replaced by one batch, an index out of range, the protocol and the envelope, and the
composition with FileTier.fetch.

Geometries, streams, tables and helpers (G1, G1C, G2; twelve conflict-free batches per stream) are tests/_fed_backing_common.py's,
where every reference is computed once."""
import ctypes as C

import numpy as np
import pytest
import torch

import _batched_policy_model as M
import _bag_evlfu_model as EM
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


def _flat(raws, rb):
    return [np.ascontiguousarray(r).view(np.uint8).reshape(-1, rb) for r in raws]


class _Source:
    """a row source over encoded host tables: a numpy gather; remembers the keys of every call"""

    def __init__(self, raws, rb, alter=None):
        self.flat, self.rb, self.alter, self.seen = _flat(raws, rb), rb, alter, []

    def __call__(self, keys):
        assert keys.dtype == np.uint64 and keys.ndim == 1
        self.seen.append(keys.copy())
        t = (keys >> np.uint64(32)).astype(np.int64) - 1
        r = (keys & np.uint64(0xffffffff)).astype(np.int64)
        out = np.empty((len(keys), self.rb), np.uint8)
        for k in np.unique(t):
            out[t == k] = self.flat[k][r[t == k]]
        return out if self.alter is None else self.alter(out)


def _cache_b(E, policy, geom, codec):
    raws, tabs = H._tables(geom, codec)
    return H._cache(E, policy, geom, codec, [_dev(r) for r in raws], order="fetch-first"), tabs


def _cache_d(E, policy, geom, codec, fed=None, alter=None, order="fetch-first"):
    """-> (the fed cache with its source set, the source); fed: the fed tables (default: all of them)"""
    g = GEOMS[geom]
    raws, _ = H._tables(geom, codec)
    fed = set(range(g["T"])) if fed is None else set(fed)
    c = E.GpuCache(policy, g["cap"], g["T"], g["d"], codec)
    if order is not None:
        c.set_miss_order(order)
    assert c.set_fed_backing([None if t in fed else _dev(raws[t]) for t in range(g["T"])], g["n_rows"]) is c
    src = _Source(raws, _row_bytes(geom, codec), alter)
    assert c.set_row_source(src) is c
    return c, src


def _want_keys(rq, flags, n_rows, fed):
    """the distinct (table_1based << 32 | row) with flag 0 and a valid index in fed tables"""
    want = set()
    for t in fed:
        col = rq[:, t].astype(np.int64)
        ok = (col >= 0) & (col < n_rows[t]) & ~flags[:, t]
        want |= {((t + 1) << 32) | int(r) for r in col[ok]}
    return want


def _check_list(keys, rq, flags, n_rows, fed):
    got = [int(k) for k in keys]
    assert len(set(got)) == len(got), "a key is listed twice"
    assert set(got) == _want_keys(rq, flags, n_rows, fed)


def _twins(E, policy, geom, codec, fed=None):
    """B and D through the conflict-free stream, lookup_batch and lookup_interact alternating"""
    g = GEOMS[geom]
    T, d, B = g["T"], g["d"], g["B"]
    n_rows = list(g["n_rows"])
    fed = list(range(T)) if fed is None else fed
    reqs, want_flags = H._bt_stream(policy, geom)
    b, tabs = _cache_b(E, policy, geom, codec)
    dd, src = _cache_d(E, policy, geom, codec, fed)
    model = EM.BagEvLFUModel(g["cap"], n_rows) if policy == "evlfu" else M.BatchedPolicyModel(policy, g["cap"], n_rows)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(13)
    n_keys = n_missed = 0
    for i in range(N_BATCHES):
        rq = reqs[i]
        r = _dev(rq)
        if policy == "evlfu":
            model.batch_bags(*EM.one_per_bag(rq))
        else:
            model.batch(rq)
        n_src = len(src.seen)
        if i % 2 == 0:
            res = [c.lookup_batch(r) for c in (b, dd)]
        else:
            x = torch.empty(B, d, device="cuda").uniform_(-1, 1, generator=gen)
            res = [c.lookup_interact(r, x) for c in (b, dd)]
        flags = [h.cpu().numpy().astype(bool) for h, _ in res]
        outs = [o.cpu().numpy() for _, o in res]
        assert np.array_equal(flags[0], want_flags[i]) and np.array_equal(flags[1], want_flags[i]), "call %d: flags" % (i + 1)
        assert np.array_equal(_bits(outs[1]), _bits(outs[0])), "call %d: D's output differs from B's" % (i + 1)
        if i % 2 == 0:
            _rows_exact(outs[1], tabs, rq)
        want = _want_keys(rq, flags[1], n_rows, fed)
        if want:
            assert len(src.seen) == n_src + 1
            _check_list(src.seen[-1], rq, flags[1], n_rows, fed)
            assert all((int(k) >> 32) - 1 in fed for k in src.seen[-1])
        else:
            assert len(src.seen) == n_src                         # (an empty list: the source is not asked)
        n_keys += len(want)
        n_missed += int(sum((~flags[1][:, t]).sum() for t in fed))
        assert _dump(dd) == _dump(b) == model.resident(), "call %d: resident sets" % (i + 1)
        assert dd.batch_stats() == b.batch_stats(), "call %d: statistics" % (i + 1)
        assert dd.fetch_stats() == b.fetch_stats(), "call %d: fetch statistics" % (i + 1)
    s = dd.batch_stats()
    assert s["n_evict"] > 0 and s["n_hits"] > 0 and s["n_flush"] == 0
    fs = dd.fed_stats()
    assert fs["calls"] == N_BATCHES and fs["keys"] == n_keys and fs["missed"] == n_missed
    if len(fed) == T:
        assert fs["from_block"] == dd.fetch_stats()["in_place"]


# ------------------------------------------------------------------------------------------------- 1. parity, 2. the list
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("geom,codec", [("G1", 32), ("G1", 8), ("G2", 32), ("G2", 8), ("G2", 16), ("G2", 4)])
def test_parity_with_hbm_tables(E, policy, geom, codec):
    """Every table fed, the source a numpy gather from the encoded tables.  After every call: flags equal B's and the model's,
    out / R bit-equal to B's (out also to the decoded table rows), dump, batch_stats (with hist) and fetch_stats equal; the keys
    the source was asked for are, as a set and without a duplicate, the distinct valid missed keys computed from the flags."""
    _twins(E, policy, geom, codec)


# ---------------------------------------------------------------------------------------------------------------- 3. mixed
@pytest.mark.parametrize("policy", POLICIES)
def test_mixed_addressed_and_fed_tables(E, policy):
    """G2 with table 1 addressed in HBM and tables 0 and 2 fed: the list names tables 0 and 2 only, everything else as above."""
    _twins(E, policy, "G2", 32, fed=[0, 2])


@pytest.mark.parametrize("policy", POLICIES)
def test_one_missing_row_in_most_positions_is_listed_once(E, policy):
    """Row 3 of the 5-row table, missing, in every position of its column but two: one key, one fed row, every copy served."""
    g = GEOMS["G2"]
    B = g["B"]
    c, src = _cache_d(E, policy, "G2", 32)
    _, tabs = H._tables("G2", 32)
    rq = np.tile(np.array([[0, 100, 7]], np.int32), (B, 1))
    c.lookup_batch(_dev(rq))
    rq[:, 0] = 3
    rq[5, 0] = rq[20, 0] = 0
    hit, keys = c.lookup_begin(_dev(rq))
    assert [int(k) for k in keys] == [(1 << 32) | 3]
    hit = hit.cpu().numpy().astype(bool)
    assert int((~hit).sum()) == B - 2
    out = c.lookup_finish(torch.from_numpy(src(keys.cpu().numpy().view(np.uint64))).cuda())
    _rows_exact(out.cpu().numpy(), tabs, rq)
    assert set(_dump(c)) == {(1, 0), (2, 100), (3, 7), (1, 3)}
    assert c.fed_stats() == {"calls": 2, "keys": 4, "missed": 3 * B + B - 2, "from_block": 0}


# -------------------------------------------------------------------------------------------------------------- 4. crowded
@pytest.mark.parametrize("policy", POLICIES)
def test_crowded_sets_serve_from_the_fed_block(E, policy):
    """Uniform rows over 8 sets (G1C): most calls bring more than 8 new keys to some set, and the keys turned away are served
    straight from the fed block.  Every served row is bit-exact, flags are residency at arrival, no key is resident twice,
    size <= capacity, in_place > 0 and fed_stats agrees with it, and the next call serves."""
    g = GEOMS["G1C"]
    B, T, cap = g["B"], g["T"], g["cap"]
    _, tabs = H._tables("G1C", 32)
    c, _src = _cache_d(E, policy, "G1C", 32)
    rs = np.random.RandomState(9)
    for i in range(N_BATCHES):
        rq = np.stack([rs.randint(0, n, B) for n in g["n_rows"]], 1).astype(np.int32)
        before = _dump(c) if i else {}
        hit, out = c.lookup_batch(_dev(rq))
        hit = hit.cpu().numpy().astype(bool)
        _rows_exact(out.cpu().numpy(), tabs, rq)
        want = np.array([[(t + 1, int(rq[b, t])) in before for t in range(T)] for b in range(B)])
        assert np.array_equal(hit, want), "call %d: flags are not residency at arrival" % (i + 1)
        assert len(_dump(c)) == c.batch_stats()["size"] <= cap
        f, fs = c.fetch_stats(), c.fed_stats()
        assert fs["from_block"] == f["in_place"] and fs["missed"] == f["in_place"] + f["repointed"]
    assert f["in_place"] > 0, "no set was ever crowded"
    assert fs["calls"] == N_BATCHES


# ---------------------------------------------------------------------------------------------------------- 5. whose bytes
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("codec", [32, 8])
def test_served_rows_are_the_fed_bytes(E, policy, codec):
    """The source feeds rows that differ from the tables (fp32: the sign flipped; u8: every byte complemented): every position
    returns the fed bytes.  After the finish has run the fed block is overwritten and the same keys looked up again: all hit,
    the list is empty, fed = None is accepted and the rows are still the bytes first fed -- they live in the arena."""
    from oracle import oracle as orc
    g = GEOMS["G2"]
    d = g["d"]
    raws, tabs = H._tables("G2", codec)
    if codec == 32:
        alter = lambda a: (-a.view(np.float32)).view(np.uint8)
        fed_tabs = [-t for t in tabs]
    else:
        alter = lambda a: 255 - a
        fed_tabs = [orc.decode(255 - np.ascontiguousarray(r).view(np.uint8), 8, d) for r in raws]
    c, src = _cache_d(E, policy, "G2", codec, alter=alter)
    rs = np.random.RandomState(8)
    rq = np.stack([rs.randint(0, n, 5) for n in g["n_rows"]], 1).astype(np.int32)
    r = _dev(rq)
    hit, keys = c.lookup_begin(r)
    assert not hit.any() and len(keys) == len({(t, int(v)) for t in range(g["T"]) for v in rq[:, t]})
    rb = _row_bytes("G2", codec)
    wide = torch.full((len(keys), rb + 48), 0xa5, dtype=torch.uint8, device="cuda")    # rows 48 bytes apart from each other
    fed = wide[:, :rb]
    fed.copy_(torch.from_numpy(src(keys.cpu().numpy().view(np.uint64))))
    assert fed.stride(0) == rb + 48
    out = c.lookup_finish(fed)
    _rows_exact(out.cpu().numpy(), fed_tabs, rq)
    torch.cuda.synchronize()
    wide.fill_(0x5a)                                                # the finish has run: the block is the caller's again
    hit, keys = c.lookup_begin(r)
    assert hit.all() and keys.numel() == 0
    out = c.lookup_finish(None)
    _rows_exact(out.cpu().numpy(), fed_tabs, rq)
    hit, out = c.lookup_batch(r)                                   # ... and through the source, which is not asked
    assert hit.all() and len(src.seen) == 1
    _rows_exact(out.cpu().numpy(), fed_tabs, rq)


# ------------------------------------------------------------------------------------------------ 6. EvLFU hit-and-victim
def test_evlfu_hit_way_is_the_same_batchs_victim(E):
    """The directed case of tests/test_gpu_host_setassoc.py with every row fed: the last call hits a key and evicts it.  The
    evicted key's row is still its own (the old copy of the two-copy arena), the replacing key's row is the row just fed."""
    g = GEOMS["G2"]
    rows, flags, at, old, new, resident = H._victim_hit_case()
    b_old = [(b, t) for b in range(g["B"]) for t in range(g["T"]) if (t + 1, int(rows[at][b, t])) == old]
    b_new = [(b, t) for b in range(g["B"]) for t in range(g["T"]) if (t + 1, int(rows[at][b, t])) == new]
    assert b_old and b_new
    c, src = _cache_d(E, "evlfu", "G2", 32)
    _, tabs = H._tables("G2", 32)
    for i in range(at + 1):
        hit, out = c.lookup_batch(_dev(rows[i]))
        assert np.array_equal(hit.cpu().numpy().astype(bool), flags[i]), "call %d: flags" % (i + 1)
        out = out.cpu().numpy()
        _rows_exact(out, tabs, rows[i])
    assert (new[0] << 32 | new[1]) in {int(k) for k in src.seen[-1]} and (old[0] << 32 | old[1]) not in {int(k) for k in src.seen[-1]}
    for b, t in b_old:
        assert np.array_equal(_bits(out[b, t]), _bits(tabs[t][old[1]]))
    for b, t in b_new:
        assert np.array_equal(_bits(out[b, t]), _bits(tabs[t][new[1]]))
    assert _dump(c) == resident and c.batch_stats()["n_flush"] == 0


# ------------------------------------------------------------------------------------------------- 7. an index out of range
@pytest.mark.parametrize("policy", POLICIES)
def test_an_index_out_of_range(E, policy):
    """An index past its table and a negative one in a batch of the conflict-free stream (taking keys away keeps it conflict-
    free): not listed, flag 0, the output cache B gives (a zero row), the tier as B's, and the sticky flag of
    evs_check_index_errors is raised by the finish."""
    g = GEOMS["G2"]
    L = E._lib
    B = g["B"]
    b, tabs = _cache_b(E, policy, "G2", 32)
    c, src = _cache_d(E, policy, "G2", 32)
    reqs, _ = H._bt_stream(policy, "G2")
    for i in range(3):
        for cache in (b, c):
            cache.lookup_batch(_dev(reqs[i]))
    rq2 = reqs[3].copy()
    rq2[17, 1] = g["n_rows"][1]
    rq2[18, 2] = -1
    L.lib().evs_check_index_errors(None)                           # (whatever an earlier test left)
    assert L.lib().evs_check_index_errors(None) == 0
    hb, ob = b.lookup_batch(_dev(rq2))
    torch.cuda.synchronize()
    assert L.lib().evs_check_index_errors(None) == 0               # (the one-call (B, T) form raises none: what follows is D's)
    hit, keys = c.lookup_begin(_dev(rq2))
    assert L.lib().evs_check_index_errors(None) == 0               # (... and the finish's, not the begin's)
    hit_np = hit.cpu().numpy().astype(bool)
    assert not hit_np[17, 1] and not hit_np[18, 2]
    _check_list(keys.cpu().numpy(), rq2, hit_np, list(g["n_rows"]), range(g["T"]))
    assert all(0 <= (int(k) & 0xffffffff) < g["n_rows"][(int(k) >> 32) - 1] for k in keys.cpu().numpy())
    out = c.lookup_finish(torch.from_numpy(src(keys.cpu().numpy().view(np.uint64))).cuda())
    assert L.lib().evs_check_index_errors(None) == L.EVS_EINDEX
    assert L.lib().evs_check_index_errors(None) == 0
    assert np.array_equal(hit_np, hb.cpu().numpy().astype(bool))
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(ob.cpu().numpy()))
    assert not out[17, 1].any() and not out[18, 2].any()
    assert all(0 <= r < g["n_rows"][t - 1] for t, r in _dump(c))
    assert _dump(c) == _dump(b) and c.batch_stats() == b.batch_stats() and c.fetch_stats() == b.fetch_stats()


# --------------------------------------------------------------------------------------------- 8. protocol and envelope
def _serves(c, tabs, n_rows, seed):
    """a cold-then-hit pair of calls: rows exact; the second call's flags are residency in the dump taken before it (which
    runs the EvLFU flush a close may have asked for: the pairs of one test add up on one cache), and it hits"""
    rs = np.random.RandomState(seed)
    rq = np.stack([rs.randint(0, n, 5) for n in n_rows], 1).astype(np.int32)
    hit, out = c.lookup_batch(_dev(rq))
    _rows_exact(out.cpu().numpy(), tabs, rq)
    before = _dump(c)
    hit, out = c.lookup_batch(_dev(rq))
    _rows_exact(out.cpu().numpy(), tabs, rq)
    want = np.array([[(t + 1, int(rq[b, t])) in before for t in range(rq.shape[1])] for b in range(rq.shape[0])])
    assert np.array_equal(hit.cpu().numpy().astype(bool), want) and want.any()


@pytest.mark.parametrize("policy", POLICIES)
def test_the_envelope(E, policy):
    """Every refusal carries its code and names the policy, and the cache serves afterwards."""
    g = GEOMS["G2"]
    L = E._lib
    T, d, n_rows = g["T"], g["d"], g["n_rows"]
    raws, tabs = H._tables("G2", 32)
    st = torch.cuda.current_stream().cuda_stream
    rq = _dev(np.zeros((4, T), np.int32))
    x = torch.zeros(4, d, device="cuda")
    seed = iter(range(100, 200))
    # a fed cache at order 0: the begin says fetch-first; then the order may still be given
    c, src = _cache_d(E, policy, "G2", 32, order=None)
    msg = _refused(E, L.EVS_EINVAL, policy, lambda: c.lookup_begin(rq))
    assert "fetch-first" in msg and "evs_cache_set_miss_order" in msg
    c.set_miss_order("fetch-first")
    _serves(c, tabs, n_rows, next(seed))
    # the one-call lookups without a source name the begin / finish calls
    c.set_row_source(None)
    assert "evs_cache_fed_begin" in _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_batch(rq))
    assert "evs_cache_fed_begin" in _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_interact(rq, x))
    c.set_row_source(src)
    _serves(c, tabs, n_rows, next(seed))
    # both bag entry points
    off, idx = [_dev(np.arange(4, dtype=np.int64))] * T, [_dev(np.zeros(4, np.int64))] * T
    if policy == "evlfu":
        c.set_bag_rule("served-bags")
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags(off, idx))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags_interact(off, idx, x))
    _serves(c, tabs, n_rows, next(seed))
    # a threshold of the approximate mode in force (EvLFU: the other policies refuse the setter)
    if policy == "evlfu":
        c.set_batch_approx(2)
        assert "evs_cache_set_batch_approx" in _refused(E, L.EVS_EINVAL, policy, lambda: c.lookup_begin(rq))
        c.set_batch_approx(0)
        _serves(c, tabs, n_rows, next(seed))
    else:                                                          # (no threshold can be in force: the setter refuses it)
        _refused(E, L.EVS_EINVAL, policy, lambda: c.set_batch_approx(2))
    # a tier of a pair / triple call
    other, _ = _cache_b(E, policy, "G2", 32)
    out = torch.empty(4, T, d, device="cuda")
    tier = torch.empty(4, T, dtype=torch.uint8, device="cuda")
    for a, b in ((c, other), (other, c)):
        assert L.lib().evs_cache_lookup_batch_c1c2(a._h, b._h, 4, rq.data_ptr(), out.data_ptr(), tier.data_ptr(), 2, st) == L.EVS_EINVAL
        assert policy.encode() in L.lib().evs_last_error()
        assert L.lib().evs_cache_request_c1c2(a._h, b._h, 4, rq.data_ptr(), out.data_ptr(), tier.data_ptr(), 2, st) == L.EVS_EINVAL
        assert policy != "evlfu" or b"evlfu" in L.lib().evs_last_error()   # (an lru / lfu pair is refused as ever, its wording names no policy)
    # ... of the pair's bag calls, of the tier server
    from evstore_dlrm_amd import gpu_cache as GC
    if policy == "evlfu":
        other.set_bag_rule("served-bags")
    _refused(E, L.EVS_EINVAL, policy, lambda: GC.lookup_bags_c1c2(c, other, off, idx, threshold=2))
    _refused(E, L.EVS_EINVAL, policy, lambda: GC.lookup_bags_interact_c1c2(c, other, off, idx, x, threshold=2))
    ring = torch.empty(4, T, d, device="cuda")
    srv = C.c_void_p()
    for a, b in ((c, other), (other, c)):
        assert L.lib().evs_tiers_serve_start(C.byref(srv), a._h, b._h, None, 2, ring.data_ptr(), 4, 200) == L.EVS_EINVAL
        assert policy != "evlfu" or b"evlfu" in L.lib().evs_last_error()
    _serves(c, tabs, n_rows, next(seed))
    # the warm start
    _serves(other, tabs, n_rows, 99)
    state = other.export_state()
    _refused(E, L.EVS_EINVAL, policy, lambda: c.export_state())
    fresh, _ = _cache_d(E, policy, "G2", 32)
    _refused(E, L.EVS_EINVAL, policy, lambda: fresh.load_state(state))
    partner, _ = _cache_b(E, policy, "G2", 32)                     # (fresh: the pair's load wants two unused caches)
    o8 = (C.c_int64 * 8)()
    for a, b in ((fresh, partner), (partner, fresh)):
        assert L.lib().evs_cache_pair_load(a._h, b._h, 0, None, None, 0, o8, st) == L.EVS_EINVAL
        assert policy.encode() in L.lib().evs_last_error()
    _serves(fresh, tabs, n_rows, next(seed))
    _serves(c, tabs, n_rows, next(seed))
    # the exact path and its server
    fresh2, _ = _cache_d(E, policy, "G2", 32)
    _refused(E, L.EVS_ESTATE, policy, lambda: fresh2.request(rq))
    _refused(E, L.EVS_ESTATE, policy, lambda: fresh2.serve_start())
    assert L.lib().evs_cache_exact_load(fresh2._h, 0, None, None, 0, st) == L.EVS_ESTATE and policy.encode() in L.lib().evs_last_error()
    _serves(fresh2, tabs, n_rows, next(seed))
    # row updates: no table to write or to read again
    keys = np.array([[0, 1], [1, 5]], np.int64)
    _refused(E, L.EVS_ESTATE, policy, lambda: c.update_rows(keys, torch.zeros(2, d, device="cuda")))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.refresh_rows(keys))
    _serves(c, tabs, n_rows, next(seed))


@pytest.mark.parametrize("policy", POLICIES)
def test_the_protocol(E, policy):
    """finish / abort without an open call, a second begin, anything else while a call is open: EVS_ESTATE.  Argument errors
    of the finish are EVS_EINVAL and leave the call open.  After an abort the batch is not counted: batch_stats (hist
    included), the dump with its scores, fetch_stats and fed_stats are what they were, and the same begin lists the same keys."""
    g = GEOMS["G2"]
    L = E._lib
    T, d, n_rows, B = g["T"], g["d"], g["n_rows"], g["B"]
    rb = d * 4
    _, tabs = H._tables("G2", 32)
    st = torch.cuda.current_stream().cuda_stream
    c, src = _cache_d(E, policy, "G2", 32)
    reqs, _ = H._bt_stream(policy, "G2")
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_abort())
    assert L.lib().evs_cache_fed_finish(c._h, None, 0, torch.empty(4, T, d, device="cuda").data_ptr(), st) == L.EVS_ESTATE
    assert policy.encode() in L.lib().evs_last_error()
    for i in range(3):                                             # warm: the next batch of the stream has hits and misses
        c.lookup_batch(_dev(reqs[i]))
    r = _dev(reqs[3])
    s0, d0, f0, fs0 = c.batch_stats(), _dump(c), c.fetch_stats(), c.fed_stats()
    hit, keys = c.lookup_begin(r)
    hit0, keys0 = hit.cpu().numpy().copy(), sorted(int(k) for k in keys)
    assert hit0.any() and not hit0.all() and keys0
    # everything else is refused while the call is open
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_begin(r))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.batch_stats())
    with pytest.raises(E._lib.EvsError) as ei:
        c.batch_dump()
    assert ei.value.code == L.EVS_ESTATE
    _refused(E, L.EVS_ESTATE, policy, lambda: c.refresh_rows(np.array([[0, 1]], np.int64)))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.set_fed_backing([None] * T, n_rows))
    raws = H._tables("G2", 32)[0]
    _refused(E, L.EVS_ESTATE, policy, lambda: c.set_backing([_dev(t) for t in raws]))
    assert c._fed                                                  # (the refused set_backing left the object a fed cache)
    n_seen = len(src.seen)
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_batch(r))   # (through the row source: its begin is the second one)
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_interact(r, torch.zeros(B, d, device="cuda")))
    assert len(src.seen) == n_seen
    _refused(E, L.EVS_ESTATE, policy, lambda: c.export_state())
    donor, _ = _cache_b(E, policy, "G2", 32)
    donor.lookup_batch(_dev(reqs[0]))
    state = donor.export_state()
    _refused(E, L.EVS_ESTATE, policy, lambda: c.load_state(state))
    # argument errors leave it open
    out = torch.empty(B, T, d, device="cuda")
    assert L.lib().evs_cache_fed_finish(c._h, None, rb, out.data_ptr(), st) == L.EVS_EINVAL and b"NULL fed" in L.lib().evs_last_error()
    fed = torch.zeros(len(keys0) * rb + 16, dtype=torch.uint8, device="cuda")
    assert L.lib().evs_cache_fed_finish(c._h, fed.data_ptr() + 4, rb, out.data_ptr(), st) == L.EVS_EINVAL
    assert L.lib().evs_cache_fed_finish(c._h, fed.data_ptr(), rb + 4, out.data_ptr(), st) == L.EVS_EINVAL
    assert L.lib().evs_cache_fed_finish(c._h, fed.data_ptr(), rb - 16, out.data_ptr(), st) == L.EVS_EINVAL and b"below" in L.lib().evs_last_error()
    # abort: not counted, nothing inserted
    c.lookup_abort()
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_abort())
    assert c.batch_stats() == s0 and _dump(c) == d0 and c.fetch_stats() == f0 and c.fed_stats() == fs0
    hit, keys = c.lookup_begin(r)
    assert np.array_equal(hit.cpu().numpy(), hit0) and sorted(int(k) for k in keys) == keys0
    out = c.lookup_finish(torch.from_numpy(src(keys.cpu().numpy().view(np.uint64))).cuda())
    _rows_exact(out.cpu().numpy(), tabs, reqs[3])
    s2 = c.batch_stats()
    assert s2["n_requests"] == s0["n_requests"] + B and s2["n_hits"] == s0["n_hits"] + int(hit0.sum())
    assert c.fed_stats()["calls"] == fs0["calls"] + 1 and c.fetch_stats()["calls"] == f0["calls"] + 1
    _serves(c, tabs, n_rows, 7)
    # destroy with an open call is fine
    c.lookup_begin(r)
    del c


@pytest.mark.parametrize("policy", POLICIES)
def test_an_abort_leaves_no_trace(E, policy):
    """Two fed caches on the conflict-free stream; after three batches one of them begins a DIFFERENT batch (the stream's fifth:
    hits among its positions) and drops it.  Its batch_stats, dump (scores included) and counters equal the other's there and
    after every further batch of the stream: no raise, no touch and no stamp of the dropped probe is left to steer a victim
    choice.  The begin wrote no way word: the dump is what it was while the call is still to be dropped."""
    g = GEOMS["G2"]
    reqs, want_flags = H._bt_stream(policy, "G2")
    _, tabs = H._tables("G2", 32)
    c1, _ = _cache_d(E, policy, "G2", 32)
    c2, _ = _cache_d(E, policy, "G2", 32)
    for i in range(3):
        for c in (c1, c2):
            c.lookup_batch(_dev(reqs[i]))
    s0, d0 = c1.batch_stats(), _dump(c1)
    r4 = _dev(reqs[4])
    hit, keys = c1.lookup_begin(r4)
    assert hit.any() and keys.numel() > 0
    c1.lookup_abort()
    assert c1.batch_stats() == s0 == c2.batch_stats() and _dump(c1) == d0 == _dump(c2)
    for i in range(3, N_BATCHES):
        r = _dev(reqs[i])
        (h1, o1), (h2, o2) = c1.lookup_batch(r), c2.lookup_batch(r)
        assert np.array_equal(h1.cpu().numpy().astype(bool), want_flags[i]) and torch.equal(h1, h2), "call %d: flags" % (i + 1)
        _rows_exact(o1.cpu().numpy(), tabs, reqs[i])
        assert _dump(c1) == _dump(c2), "call %d: resident sets and scores" % (i + 1)
        assert c1.batch_stats() == c2.batch_stats() and c1.fetch_stats() == c2.fetch_stats(), "call %d: statistics" % (i + 1)
    assert c1.fed_stats() == c2.fed_stats()


# ---------------------------------------------------------------------------------------------------------------- 9. files
@pytest.mark.parametrize("policy", POLICIES)
def test_file_tier_as_the_row_source(E, policy, tmp_path):
    """.bin tables behind FileTier(paths, row_bytes, 0) -- nothing registered, every table staged -- and
    set_row_source(tier.fetch): the results of cache B on the G2 stream."""
    g = GEOMS["G2"]
    T, d = g["T"], g["d"]
    raws, tabs = H._tables("G2", 32)
    paths = []
    for k, t in enumerate(tabs):
        p = tmp_path / ("ev-table-%d.bin" % (k + 1))
        t.tofile(p)
        paths.append(str(p))
    tier = E.FileTier(paths, d * 4, 0)
    assert not any(tier.registered)
    c = E.GpuCache(policy, g["cap"], T, d, 32).set_miss_order("fetch-first")
    c.set_fed_backing([None] * T, tier.n_rows).set_row_source(tier.fetch)
    b, _ = _cache_b(E, policy, "G2", 32)
    reqs, want_flags = H._bt_stream(policy, "G2")
    for i in range(N_BATCHES):
        r = _dev(reqs[i])
        (hb, ob), (hc, oc) = b.lookup_batch(r), c.lookup_batch(r)
        assert np.array_equal(hc.cpu().numpy().astype(bool), want_flags[i]) and torch.equal(hb, hc)
        assert np.array_equal(_bits(oc.cpu().numpy()), _bits(ob.cpu().numpy()))
        _rows_exact(oc.cpu().numpy(), tabs, reqs[i])
    assert _dump(c) == _dump(b) and c.batch_stats() == b.batch_stats() and c.fetch_stats() == b.fetch_stats()
    tier.close()
