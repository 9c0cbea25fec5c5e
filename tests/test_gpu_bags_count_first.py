"""The count-first EvLFU bag chain (GpuCache.set_bag_count("count-first"), evs_cache_set_bag_count(c, 1); csrc/evs_cache_policy.hip:
bags_count_kernel, bags_pool_kernel<.., COUNT = false>): every sample's served-bag count from a launch of its own behind the probe,
which lets a fetch-first cache (set_miss_order) run  probe -> count -> raise + list -> update -> sa_repoint -> pooling  over tables
in HBM or in pinned host memory.  The rule has not changed, so the yardsticks are the default chain and the Python restatement of
the rule (tests/_bag_evlfu_model.py).  Four caches see the same calls -- A: HBM tables, order 0, the default count (the yardstick);
A': HBM, order 0, count-first; B: HBM, order 1, count-first; C: pinned tables, order 1, count-first.

The geometries are tests/test_gpu_host_setassoc.py's: G1 -- 26 tables of 300 rows, d = 36, capacity 512 (64 sets; 64 = 8 sets for
the crowded cases), B = 40 / 64 -- and G2 -- 3 tables of 5 / 3000 / 70 rows, d = 16, capacity 64, B = 37: a 5-row table that puts
hundreds of positions on one way word, a B that fills neither a wave nor a block.

The warm start reads HBM tables only (C's export keeps its EVS_ESTATE, tests/test_gpu_host_setassoc.py), so the exported state is
compared over A, A' and B."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _bag_evlfu_model as EM
import _bag_policy_model as BP
import _batched_policy_model as M

pytestmark = pytest.mark.gpu

G1 = dict(T=26, n_rows=tuple([300] * 26), d=36, cap=512, B=40)
G1C = dict(T=26, n_rows=tuple([300] * 26), d=36, cap=64, B=64)      # the crowded form: 8 sets
G2 = dict(T=3, n_rows=(5, 3000, 70), d=16, cap=64, B=37)
G3 = dict(T=3, n_rows=(400, 413, 426), d=16, cap=8192, B=37)            # long bags: a cache in which nothing is evicted
GEOMS = {"G1": G1, "G1C": G1C, "G2": G2, "G3": G3}
N_BATCHES = 12
SEED = 3
# (stream arguments, what the model says of the stream: the largest top bucket, evictions, all-served samples, positions)
STREAMS = {"G1": (dict(max_bag=5, alpha=2.0), (262, 182, 65, 31320)),
           "G2": (dict(max_bag=4, alpha=1.3), (43, 30, 268, 2739))}


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _pin(a):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).pin_memory()


@functools.lru_cache(maxsize=None)
def _tables(geom, codec, seed=21):
    """-> (what set_backing takes (host arrays), the fp32 rows a lookup must return)"""
    from oracle import oracle as orc
    g = GEOMS[geom]
    tabs = orc.kaggle_tables(list(g["n_rows"]), seed, g["d"])
    if codec == 32:
        return tabs, tabs
    raws = [orc.encode_table(np.clip(t * np.sqrt(len(t)), -1, 1), codec) for t in tabs]
    return raws, [orc.decode(a, codec, g["d"]) for a in raws]


def _cache(E, geom, codec, backing, order=None, count=None, policy="evlfu", rule="served-bags", inline=None):
    g = GEOMS[geom]
    c = E.GpuCache(policy, g["cap"], g["T"], g["d"], codec)
    if order is not None:
        assert c.set_miss_order(order) is c
    if inline is not None:
        c.set_inline_update(inline)
    c.set_backing(backing)
    if rule:
        c.set_bag_rule(rule)
    if count is not None:
        assert c.set_bag_count(count) is c
    return c


def _four(E, geom, codec):
    """-> ((A, A', B, C), the HBM tensors)"""
    raws, _ = _tables(geom, codec)
    dev = [_dev(r) for r in raws]
    a = _cache(E, geom, codec, dev, inline=False)
    a2 = _cache(E, geom, codec, dev, count="count-first", inline=False)
    b = _cache(E, geom, codec, dev, order="fetch-first", count="count-first")
    c = _cache(E, geom, codec, [_pin(r) for r in raws], order="fetch-first", count="count-first")
    return (a, a2, b, c), dev


def _cache_c(E, geom, codec=32):
    """-> (C, its pinned tensors, the same tables in HBM, the fp32 rows)"""
    raws, tabs = _tables(geom, codec)
    pinned = [_pin(r) for r in raws]
    return _cache(E, geom, codec, pinned, order="fetch-first", count="count-first"), pinned, [_dev(r) for r in raws], tabs


def _dump(c):
    d = c.batch_dump()
    keys = [(int(t), int(r)) for _, t, r in d]
    assert len(set(keys)) == len(keys), "a key is resident twice"
    return {k: int(s) for k, (s, _, _) in zip(keys, d)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _np_pooled(ly):
    return torch.stack([t for t in ly]).cpu().numpy()


def _np_flags(hits):
    return [h.cpu().numpy().astype(bool) for h in hits]


def _apply_emb(E, ev, lS_o, lS_i):
    return _np_pooled(E.apply_emb(lS_o, lS_i, ev, lazy=False))


def _index_error_once(E):
    L = E._lib
    assert L.lib().evs_check_index_errors(None) == L.EVS_EINDEX
    assert L.lib().evs_check_index_errors(None) == 0


def _refused(E, code, word, fn):
    with pytest.raises(E._lib.EvsError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    assert word is None or word in str(ei.value), str(ei.value)
    return str(ei.value)


class _Account:
    """fetch_stats / batch_stats of one order-1 cache, call by call"""

    def __init__(self, c):
        self.c, self.f = c, c.fetch_stats()
        self.s = c.batch_stats() if self.f["calls"] else {"size": 0, "n_evict": 0}
        self.calls = self.f["calls"]

    def step(self):
        """-> (re-pointed, in place, size + evictions) of the last call"""
        f, s = self.c.fetch_stats(), self.c.batch_stats()
        self.calls += 1
        assert f["calls"] == self.calls
        out = (f["repointed"] - self.f["repointed"], f["in_place"] - self.f["in_place"],
               s["size"] - self.s["size"] + s["n_evict"] - self.s["n_evict"])
        self.f, self.s = f, s
        return out


def _set_rows(geom, t, s, want_in=True):
    """rows of table t whose set is (want_in) / is not s"""
    g = GEOMS[geom]
    nset, bits = M.geometry(g["cap"], g["n_rows"])
    rows = np.arange(g["n_rows"][t])
    return rows[(M.set_of(t, rows, nset, list(g["n_rows"]), bits) == s) == want_in]


def _set_of(geom, key):
    g = GEOMS[geom]
    nset, bits = M.geometry(g["cap"], g["n_rows"])
    return int(M.set_of(key[0] - 1, key[1], nset, list(g["n_rows"]), bits))


def _call_of(B, T, bags):
    """{(sample, table): [rows]} -> (offsets, indices) with every other bag empty"""
    off, idx = [], []
    for t in range(T):
        per = [np.asarray(bags.get((b, t), []), np.int64) for b in range(B)]
        off.append(np.concatenate([[0], np.cumsum([len(p) for p in per[:-1]])]).astype(np.int64))
        idx.append(np.concatenate(per + [np.zeros(0, np.int64)]).astype(np.int64))
    return off, idx


def _up(off, idx):
    return [_dev(o) for o in off], [_dev(i) for i in idx]


# ------------------------------------------------------------------------------------------- 1. twins on conflict-free streams
@functools.lru_cache(maxsize=None)
def _stream(geom):
    """-> the calls of the geometry's conflict-free stream, after holding the stream to what the model said of it when the test
    was written (a changed generator must not hollow the test out)"""
    g = GEOMS[geom]
    kw, (top, n_evict, n_perfect, n_positions) = STREAMS[geom]
    calls, model, got_top = EM.conflict_free_bag_stream(g["cap"], list(g["n_rows"]), g["B"], kw["max_bag"], N_BATCHES, SEED, alpha=kw["alpha"])
    assert got_top == top < int(0.95 * g["cap"]), "the stream would flush"
    assert (model.n_evict, model.n_perfect, model.n_turned) == (n_evict, n_perfect, 0)
    assert sum(len(ix) for _, idx, _ in calls for ix in idx) == n_positions
    assert any((np.diff(np.append(o, len(ix))) == 0).any() for off, idx, _ in calls for o, ix in zip(off, idx)), "no empty bag"
    return calls


@pytest.mark.parametrize("geom,codec,form", [("G1", 32, "bags"), ("G1", 32, "bags_interact"), ("G1", 8, "bags"), ("G1", 4, "bags"),
                                             ("G2", 32, "bags"), ("G2", 32, "bags_interact")])
def test_twins_on_conflict_free_streams(E, geom, codec, form):
    """No call brings two new keys to one set and no flush fires, so the rule is deterministic.  After every call: the flags of
    all four equal the model's; A's pooled rows bit-equal to apply_emb over the HBM tables; all four outputs bit-equal; the four
    dumps equal the model's resident set and priorities; batch_stats equal across the four (hist included) and the model's;
    A's and A''s exported state equal in every word, B's equal but for the inline setting; and for B and C every missed position
    re-pointed and one installed way per distinct missed key (nothing is turned away on these streams)."""
    g = GEOMS[geom]
    T, d, B = g["T"], g["d"], g["B"]
    calls = _stream(geom)
    caches, dev = _four(E, geom, codec)
    ev = E.EVTables(dev, d, codec)
    acct = [_Account(c) for c in caches[2:]]
    model = EM.BagEvLFUModel(g["cap"], list(g["n_rows"]))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(12)
    for i, (off, idx, want_flags) in enumerate(calls):
        model.batch_bags(off, idx)
        resident = model.resident()
        lS_o, lS_i = _up(off, idx)
        if form == "bags":
            res = [c.lookup_bags(lS_o, lS_i) for c in caches]
            outs = [_np_pooled(ly) for _, ly in res]
            assert np.array_equal(_bits(outs[0]), _bits(_apply_emb(E, ev, lS_o, lS_i))), "call %d: pooled rows" % (i + 1)
        else:
            x = torch.empty(B, d, device="cuda").uniform_(-1, 1, generator=gen)
            res = [c.lookup_bags_interact(lS_o, lS_i, x) for c in caches]
            outs = [o.cpu().numpy() for _, o in res]
        for k in range(4):
            got = _np_flags(res[k][0])
            assert all(np.array_equal(a, b) for a, b in zip(got, want_flags)), "call %d, cache %d: flags" % (i + 1, k)
            assert np.array_equal(_bits(outs[k]), _bits(outs[0])), "call %d: cache %d's output differs from A's" % (i + 1, k)
        dumps = [_dump(c) for c in caches]
        stats = [c.batch_stats() for c in caches]
        assert dumps[0] == dumps[1] == dumps[2] == dumps[3] == resident, "call %d: resident sets" % (i + 1)
        assert stats[0] == stats[1] == stats[2] == stats[3], "call %d: statistics\n%s" % (i + 1, stats)
        st = stats[0]
        assert (st["size"], st["n_hits"], st["n_requests"], st["n_evict"], st["n_perfect_hits"], st["hist"], st["n_flush"]) == \
            (model.size(), model.n_hits, model.n_requests, model.n_evict, model.n_perfect, model.hist(), 0), "call %d: counters" % (i + 1)
        sa, sa2, sb = (c.export_state() for c in caches[:3])
        assert np.array_equal(sa["entries"], sa2["entries"]) and np.array_equal(sa["state"], sa2["state"]), "call %d: A' state" % (i + 1)
        keep = np.arange(len(sa["state"])) != 14               # (state[14]: the inline-update setting)
        assert np.array_equal(sa["entries"], sb["entries"]) and np.array_equal(sa["state"][keep], sb["state"][keep]), "call %d: B state" % (i + 1)
        missed = [(k + 1, int(r)) for k in range(T) for r, f in zip(idx[k], want_flags[k]) if not f]
        assert all(k in resident for k in missed)              # (nothing turned away)
        for a in acct:
            assert a.step() == (len(missed), 0, len(set(missed))), "call %d" % (i + 1)
    assert stats[0]["n_evict"] > 0 and stats[0]["n_perfect_hits"] > 0
    assert caches[0].fetch_stats() == caches[1].fetch_stats() == {"calls": 0, "repointed": 0, "in_place": 0}


# -------------------------------------------------------------------------------- 2. a hit way that is the same call's victim
def test_a_hit_way_is_the_same_calls_victim(E):
    """The case the two-copy arena exists for, over bags.  Set s of G2 is filled one key a call: `old` at priority 0 (its sample's
    other two bags miss), seven more at priority 2 (their samples' other bags are empty).  Then one call: sample 0 hits `old`
    while its other two bags miss -- count 1, the way is raised to 1 and stays the set's lowest --, sample 1 brings `new`, a fresh
    key of set s, with two empty bags -- count 2.  The model says `new` takes `old`'s way.  The update runs in front of the
    pooling, so when the pooling reads, the way names `new`: `old`'s pooled row must still be ITS table row (the copy the update
    left alone), and the next call hits `new` and misses `old`."""
    g = G2
    T, B, n_rows = g["T"], 3, list(g["n_rows"])
    s = 3
    in_s = [int(r) for r in _set_rows("G2", 1, s)[:9]]
    old, others, new = in_s[0], in_s[1:8], in_s[8]
    # fresh keys of tables 0 and 2 in sets other than s, pairwise different sets per call
    side0 = [int(r) for r in _set_rows("G2", 0, s, False)]
    side2 = [int(r) for r in _set_rows("G2", 2, s, False)]
    pick = [(a, b) for a in side0 for b in side2 if _set_of("G2", (1, a)) != _set_of("G2", (3, b))]
    (a0, b0), (a1, b1) = pick[0], [p for p in pick if p[0] != pick[0][0] and p[1] != pick[0][1]][0]
    calls = [_call_of(B, T, {(0, 0): [a0], (0, 1): [old], (0, 2): [b0]})]
    calls += [_call_of(B, T, {(0, 1): [r]}) for r in others]
    calls.append(_call_of(B, T, {(0, 0): [a1], (0, 1): [old], (0, 2): [b1], (1, 1): [new]}))
    calls.append(_call_of(B, T, {(0, 1): [new], (1, 1): [old]}))
    model = EM.BagEvLFUModel(g["cap"], n_rows)
    c, _pinned, dev, tabs = _cache_c(E, "G2")
    ev = E.EVTables(dev, g["d"], 32)
    for i, (off, idx) in enumerate(calls):
        assert not BP.new_key_conflicts(model, BP.keys_of(idx)), "call %d is not conflict-free" % i
        before = dict(model.where)
        want = model.batch_bags(off, idx)
        if i == len(calls) - 2:                                 # the model says so: hit, raised to 1, and replaced by `new`
            assert want[1].tolist() == [True, False]
            assert (2, old) not in model.where and model.where[(2, new)] == before[(2, old)] and model.resident()[(2, new)] == 2
        lS_o, lS_i = _up(off, idx)
        hits, ly = c.lookup_bags(lS_o, lS_i)
        got = _np_flags(hits)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "call %d: flags" % i
        pooled = _np_pooled(ly)
        assert np.array_equal(_bits(pooled), _bits(_apply_emb(E, ev, lS_o, lS_i))), "call %d: pooled rows" % i
        if i == len(calls) - 2:
            assert np.array_equal(_bits(pooled[1, 0]), _bits(tabs[1][old])), "the hit position was not read from the old copy"
            assert np.array_equal(_bits(pooled[1, 1]), _bits(tabs[1][new]))
        assert _dump(c) == model.resident(), "call %d: resident set / priorities" % i
    assert want[1].tolist() == [True, False]                    # the last call: `new` hits, `old` is gone
    assert model.n_evict == 2 and model.n_turned == 0 and c.batch_stats()["n_flush"] == 0


# ------------------------------------------------------------------------------------------------------------ 3. a crowded set
def test_a_crowded_set(E):
    """Ten fresh keys of one set in one call, each in a bag of its own (capacity 64: 8 sets): 8 are installed, the other two are
    turned away and pooled in place from the pinned table -- fetch_stats says so --, every pooled row is bit-equal and no key is
    resident twice."""
    g = G1C
    T, B = g["T"], 10
    s = 5
    c, _pinned, dev, tabs = _cache_c(E, "G1C")
    ev = E.EVTables(dev, g["d"], 32)
    away = [int(_set_rows("G1C", t, s, False)[0]) for t in range(T)]    # one resident key per table, none in set s
    warm = _up(*_call_of(B, T, {(0, t): [away[t]] for t in range(T)}))
    c.lookup_bags(*warm)
    hits, _ = c.lookup_bags(*warm)
    assert torch.cat(hits).all() and set(_dump(c)) == {(t + 1, away[t]) for t in range(T)}
    fresh = [int(r) for r in _set_rows("G1C", 0, s)[:10]]
    assert len(fresh) == 10
    bags = {(b, 0): [fresh[b]] for b in range(B)}
    bags.update({(0, t): [away[t]] for t in range(1, T)})
    lS_o, lS_i = _up(*_call_of(B, T, bags))
    acct = _Account(c)
    hits, ly = c.lookup_bags(lS_o, lS_i)
    got = _np_flags(hits)
    assert not got[0].any() and all(f.all() for f in got[1:])
    pooled = _np_pooled(ly)
    assert np.array_equal(_bits(pooled), _bits(_apply_emb(E, ev, lS_o, lS_i)))
    assert np.array_equal(_bits(pooled[0]), _bits(tabs[0][fresh]))
    after = _dump(c)
    kept = [r for r in fresh if (1, r) in after]
    assert len(kept) == 8
    assert acct.step() == (8, 2, 8)
    hits, ly = c.lookup_bags(lS_o, lS_i)                        # the next call: flags = residency, rows exact again
    assert np.array_equal(_np_flags(hits)[0], np.array([(1, r) in after for r in fresh]))
    assert np.array_equal(_bits(_np_pooled(ly)), _bits(pooled))


# ---------------------------------------------------------------------------------------------------- 4. the arena serves hits
def test_the_arena_serves_hits(E):
    """Three calls on one key set (no set receives more than 8 of its keys) warm C; then the pinned tables are overwritten in
    place from the CPU.  The same call again returns the OLD rows bit for bit and re-points nothing -- hits never touch the
    table.  A call with one more key, in a bag of its own, returns the NEW table's row for it: the update read it once, now."""
    g = G2
    T, B, n_rows = g["T"], 6, g["n_rows"]
    c, pinned, dev, tabs = _cache_c(E, "G2")
    ev_old = E.EVTables(dev, g["d"], 32)
    rs = np.random.RandomState(6)
    bags = {(b, t): rs.randint(0, n_rows[t], rs.randint(0, 4)).tolist() for b in range(B - 1) for t in range(T)}
    keys = {(t + 1, r) for (b, t), rows in bags.items() for r in rows}
    assert 8 <= len(keys) and max(np.bincount([_set_of("G2", k) for k in keys])) <= 8
    off, idx = _call_of(B, T, bags)
    lS_o, lS_i = _up(off, idx)
    for _ in range(3):
        hits, ly = c.lookup_bags(lS_o, lS_i)
    assert torch.cat(hits).all()
    want_old = _apply_emb(E, ev_old, lS_o, lS_i)
    assert np.array_equal(_bits(_np_pooled(ly)), _bits(want_old))
    torch.cuda.synchronize()
    new_tabs = [(-2.0 * t - 1.0).astype(np.float32) for t in tabs]
    for p, n in zip(pinned, new_tabs):
        assert p.dtype == torch.float32 and tuple(p.shape) == n.shape
        p.copy_(torch.from_numpy(n))                           # in place: the cache holds the tensor's address
    acct = _Account(c)
    hits, ly = c.lookup_bags(lS_o, lS_i)
    assert torch.cat(hits).all()
    assert np.array_equal(_bits(_np_pooled(ly)), _bits(want_old)), "a hit was not served from the arena"
    assert acct.step() == (0, 0, 0)
    fresh = next(int(r) for r in range(n_rows[1]) if (2, int(r)) not in keys and
                 sum(_set_of("G2", k) == _set_of("G2", (2, int(r))) for k in keys) < 8)
    bags[(B - 1, 1)] = [fresh]
    off2, idx2 = _call_of(B, T, bags)
    lS_o2, lS_i2 = _up(off2, idx2)
    hits, ly = c.lookup_bags(lS_o2, lS_i2)
    got, pooled = _np_flags(hits), _np_pooled(ly)
    assert not got[1][-1] and got[1][:-1].all() and got[0].all() and got[2].all()
    assert np.array_equal(_bits(pooled[1, B - 1]), _bits(new_tabs[1][fresh])), "the new key's row is not the table's of now"
    assert np.array_equal(_bits(pooled[:, :B - 1]), _bits(want_old[:, :B - 1]))
    assert acct.step() == (1, 0, 1)


# ------------------------------------------------------------------------------------------------------------ 5. what is no key
@pytest.mark.parametrize("which", ["C", "A'"])
def test_what_is_no_key(E, which):
    """One call, run three times, that holds indices out of range (-1 and n_rows in table 0, 3000 in table 1), a bag whose
    offsets go back and one that runs past nnz (table 1: both empty, hence served; the run between them is covered by no bag) and
    empty bags; no position is covered twice.  The kernels' own range checks handle all of it.  Flags, the dump's priorities (the
    counts), and the counters equal the model's; the out-of-range indices are never inserted; evs_check_index_errors reports
    once per call; pooled rows bit-equal to apply_emb."""
    g = G2
    T, B, n_rows = g["T"], 6, list(g["n_rows"])
    off = [np.arange(B, dtype=np.int64),
           np.array([0, 2, 10 ** 6, 5, 7, 8], np.int64),       # bag 1 = [2, 10^6) runs past nnz, bag 2 = [10^6, 5) goes back; 2 .. 4 uncovered
           np.array([0, 0, 3, 3, 4, 6], np.int64)]
    idx = [np.array([0, 1, -1, 2, 5, 3], np.int64),
           np.array([11, 12, 13, 14, 15, 16, 3000, 18, 19, 11], np.int64),
           np.array([1, 2, 3, 4, 5, 6, 7], np.int64)]
    raws, tabs = _tables("G2", 32)
    dev = [_dev(r) for r in raws]
    ev = E.EVTables(dev, g["d"], 32)
    if which == "C":
        c = _cache(E, "G2", 32, [_pin(r) for r in raws], order="fetch-first", count="count-first")
    else:
        c = _cache(E, "G2", 32, dev, count="count-first")
    model = EM.BagEvLFUModel(g["cap"], n_rows)
    lS_o, lS_i = _up(off, idx)
    want_pooled = _apply_emb(E, ev, lS_o, lS_i)
    _index_error_once(E)
    for call in range(3):
        want = model.batch_bags(off, idx)
        hits, ly = c.lookup_bags(lS_o, lS_i)
        _index_error_once(E)
        got = _np_flags(hits)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), "call %d: flags" % call
        assert not got[0][2] and not got[0][4] and not got[1][6]
        assert np.array_equal(_bits(_np_pooled(ly)), _bits(want_pooled)), "call %d: pooled rows" % call
        after = _dump(c)
        assert after == model.resident(), "call %d: resident set / priorities" % call
        assert all(0 <= r < n_rows[t - 1] for t, r in after)
        st = c.batch_stats()
        assert (st["size"], st["n_hits"], st["n_requests"], st["n_evict"], st["n_perfect_hits"], st["hist"], st["n_flush"]) == \
            (model.size(), model.n_hits, model.n_requests, 0, model.n_perfect, model.hist(), 0), "call %d: counters" % call
    assert model.n_turned == 0 and model.n_hits > 0
    res = model.resident()
    assert res[(2, 13)] == 0 and res[(2, 11)] > 0               # an uncovered hit is never raised; a covered copy of a key is
    assert model.n_perfect > 0                                  # (sample 1: three served bags, one lookup)


@pytest.mark.parametrize("max_bag,lanes", [(12, 4), (40, 16)])
def test_long_bags_take_the_lane_groups(E, max_bag, lanes):
    """The count kernel gives a bag 1, 4 or 16 lanes by the call's mean bag length (above 4 / above 16 indices); the streams above
    stay at one.  Bags of 0 .. 12 and 0 .. 40 indices -- lengths that are no multiple of the group, empty bags, a bag of exactly
    one group, an index out of range, a bag past nnz and one that goes back with an uncovered run between them -- on A, A' and C
    over a cache large enough that nothing is evicted or turned away (the dump is then the model's whatever the timing): three
    calls, the second the first again."""
    g = G3
    T, d, B, cap, n_rows = g["T"], g["d"], g["B"], g["cap"], g["n_rows"]
    raws, _ = _tables("G3", 32)
    dev = [_dev(r) for r in raws]
    ev = E.EVTables(dev, d, 32)
    caches = [_cache(E, "G3", 32, dev), _cache(E, "G3", 32, dev, count="count-first"),
              _cache(E, "G3", 32, [_pin(r) for r in raws], order="fetch-first", count="count-first")]
    model = EM.BagEvLFUModel(cap, list(n_rows))
    rs = np.random.RandomState(100 + max_bag)

    def draw():
        sizes = rs.randint(0, max_bag + 1, size=(B, T))
        sizes[3, 0], sizes[4, 0], sizes[5, 1] = lanes, 0, lanes + 1
        idx = [rs.randint(0, n_rows[t], int(sizes[:, t].sum())).astype(np.int64) for t in range(T)]
        off = [np.concatenate([[0], np.cumsum(sizes[:-1, t])]).astype(np.int64) for t in range(T)]
        idx[0][len(idx[0]) // 2] = n_rows[0]
        idx[2][1] = -1
        off[1][20] = 10 ** 6                                   # bag 19 runs past nnz, bag 20 goes back: both empty, their run uncovered
        return off, idx
    first = draw()
    for call, (off, idx) in enumerate([first, first, draw()]):
        n_pos = sum(len(i) for i in idx)
        assert (4 if lanes == 4 else 16) * T * B < n_pos and (lanes == 16 or n_pos <= 16 * T * B)
        want = model.batch_bags(off, idx)
        lS_o, lS_i = _up(off, idx)
        want_pooled = _apply_emb(E, ev, lS_o, lS_i)
        _index_error_once(E)
        for k, c in enumerate(caches):
            hits, ly = c.lookup_bags(lS_o, lS_i)
            _index_error_once(E)
            got = _np_flags(hits)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), "call %d, cache %d: flags" % (call, k)
            assert np.array_equal(_bits(_np_pooled(ly)), _bits(want_pooled)), "call %d, cache %d: pooled rows" % (call, k)
            assert _dump(c) == model.resident(), "call %d, cache %d: resident set / priorities" % (call, k)
            st = c.batch_stats()
            assert (st["size"], st["n_hits"], st["n_requests"], st["n_evict"], st["n_perfect_hits"], st["hist"], st["n_flush"]) == \
                (model.size(), model.n_hits, model.n_requests, 0, model.n_perfect, model.hist(), 0), "call %d, cache %d: counters" % (call, k)
    assert model.n_evict == 0 and model.n_turned == 0 and model.n_hits > 0 and len(set(model.resident().values())) > 2


# ------------------------------------------------------------------------------------------------------- 6. mixing and toggling
def _mixed_stream(geom, n_calls, seed):
    """conflict-free calls against ONE model, bag calls (even) alternating with (B, T) calls (odd) -> [(kind, offsets, indices,
    flags, the model's resident set after the call)]"""
    g = GEOMS[geom]
    n_rows, T, B = list(g["n_rows"]), g["T"], g["B"]
    rs = np.random.RandomState(seed)
    perms = [rs.permutation(n) for n in n_rows]
    model = EM.BagEvLFUModel(g["cap"], n_rows)
    out = []
    for i in range(n_calls):
        if i % 2 == 0:
            off, idx, flags, _ = BP.conflict_free_bags(model, rs, perms, B, 4)
        else:
            reqs = np.stack([M.zipf_rows(rs, n_rows[t], B, 1.3, perms[t]) for t in range(T)], 1).astype(np.int32)
            owner = {}
            for b in range(B):
                for t in range(T):
                    for _ in range(1000):
                        key = (t + 1, int(reqs[b, t]))
                        if key in model.where or owner.setdefault(_set_of(geom, key), key) == key:
                            break
                        reqs[b, t] = M.zipf_rows(rs, n_rows[t], 1, 1.3, perms[t])[0]
                    else:
                        raise AssertionError("no conflict-free row")
            off, idx = EM.one_per_bag(reqs)
            flags = model.batch_bags(off, idx)
        assert model.top_bucket() < int(0.95 * g["cap"]), "the stream would flush"
        out.append(("bags" if i % 2 == 0 else "bt", off, idx, flags, model.resident()))
    assert model.n_evict > 0
    return out


def test_bag_calls_alternate_with_the_bt_forms(E):
    """On C, lookup_bags / lookup_bags_interact alternate with lookup_batch / lookup_interact (one index per table); A -- HBM, order
    0, the default count, the chain of launches -- is driven the same way: flags (the model's), outputs bit for bit, dumps (the
    model's) and statistics are equal call by call."""
    g = G2
    T, d, B = g["T"], g["d"], g["B"]
    raws, _ = _tables("G2", 32)
    dev = [_dev(r) for r in raws]
    a = _cache(E, "G2", 32, dev, inline=False)
    c = _cache(E, "G2", 32, [_pin(r) for r in raws], order="fetch-first", count="count-first")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    for i, (kind, off, idx, want, resident) in enumerate(_mixed_stream("G2", 10, 7)):
        x = torch.empty(B, d, device="cuda").uniform_(-1, 1, generator=gen)
        if kind == "bags":
            lS_o, lS_i = _up(off, idx)
            if i % 4 == 0:
                res = [k.lookup_bags(lS_o, lS_i) for k in (a, c)]
                outs = [_np_pooled(o) for _, o in res]
            else:
                res = [k.lookup_bags_interact(lS_o, lS_i, x) for k in (a, c)]
                outs = [o.cpu().numpy() for _, o in res]
            flags = [np.concatenate(_np_flags(h)) for h, _ in res]
            want = np.concatenate(want)
        else:
            rq = _dev(np.stack(idx, 1).astype(np.int32))
            res = [k.lookup_batch(rq) if i % 4 == 1 else k.lookup_interact(rq, x) for k in (a, c)]
            outs = [o.cpu().numpy() for _, o in res]
            flags = [h.cpu().numpy().astype(bool) for h, _ in res]
            want = np.stack(want, 1)
        assert np.array_equal(flags[0], want) and np.array_equal(flags[1], want), "call %d: flags" % i
        assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "call %d: outputs" % i
        assert _dump(a) == _dump(c) == resident, "call %d: resident sets" % i
        assert a.batch_stats() == c.batch_stats(), "call %d: statistics" % i
    assert c.fetch_stats()["calls"] == 10 and c.batch_stats()["n_flush"] == 0


def test_the_setting_flips_between_calls(E):
    """An order-0 cache whose count setting is flipped before every call equals, call by call, a cache that was never told: flags,
    pooled bits, dump, statistics, exported state.  An order-1 cache flipped back to "pooling-walk" refuses its next bag call
    with today's message; told "count-first" again it serves the following one."""
    g = G2
    calls = _stream("G2")
    raws, _ = _tables("G2", 32)
    dev = [_dev(r) for r in raws]
    a = _cache(E, "G2", 32, dev)
    f = _cache(E, "G2", 32, dev)
    o1 = _cache(E, "G2", 32, [_pin(r) for r in raws], order="fetch-first", count="count-first")
    for i, (off, idx, want) in enumerate(calls):
        lS_o, lS_i = _up(off, idx)
        f.set_bag_count("count-first" if i % 2 == 0 else "pooling-walk")
        (ha, la), (hf, lf) = a.lookup_bags(lS_o, lS_i), f.lookup_bags(lS_o, lS_i)
        assert all(np.array_equal(x, y) for x, y in zip(_np_flags(hf), want)) and torch.equal(torch.cat(ha), torch.cat(hf))
        assert np.array_equal(_bits(_np_pooled(la)), _bits(_np_pooled(lf))), "call %d: pooled rows" % i
        assert _dump(a) == _dump(f) and a.batch_stats() == f.batch_stats(), "call %d" % i
        sa, sf = a.export_state(), f.export_state()
        assert np.array_equal(sa["entries"], sf["entries"]) and np.array_equal(sa["state"], sf["state"]), "call %d: exported state" % i
        if i % 3 == 1:
            o1.set_bag_count("pooling-walk")
            n = o1.fetch_stats()["calls"]
            msg = _refused(E, E._lib.EVS_EINVAL, "evlfu", lambda: o1.lookup_bags(lS_o, lS_i))
            assert "pooling" in msg and "fetch-first bag form" in msg and o1.fetch_stats()["calls"] == n
            o1.set_bag_count("count-first")
        ho, lo = o1.lookup_bags(lS_o, lS_i)
        assert torch.equal(torch.cat(ho), torch.cat(ha)) and np.array_equal(_bits(_np_pooled(lo)), _bits(_np_pooled(la))), "call %d: order 1" % i
        assert _dump(o1) == _dump(a) and o1.batch_stats() == a.batch_stats(), "call %d: order 1" % i
    assert a.batch_stats()["n_evict"] > 0


# ------------------------------------------------------------------------------------------ 7. contended streams and the flush
def _plain_calls(g, n_calls, seed, max_bag=2, alpha=2.0):
    """the generators' plain draw, no conflict avoidance: bag sizes uniform in 0 .. max_bag, Zipf rows"""
    T, B, n_rows = g["T"], g["B"], g["n_rows"]
    rs = np.random.RandomState(seed)
    perms = [rs.permutation(n) for n in n_rows]
    calls = []
    for _ in range(n_calls):
        sizes = rs.randint(0, max_bag + 1, size=(B, T))
        idx = [np.concatenate([M.zipf_rows(rs, n_rows[t], int(sizes[b, t]), alpha, perms[t]) for b in range(B)]).astype(np.int64) for t in range(T)]
        off = [np.concatenate([[0], np.cumsum(sizes[:-1, t])]).astype(np.int64) for t in range(T)]
        calls.append((off, idx))
    return calls


def test_contended_streams_and_the_flush(E):
    """G1's crowded form (8 sets, B = 64) on C: most calls bring many new keys to a set, so which of them wins a way is a matter
    of timing; the invariants are not -- flags = residency at arrival (the dump taken before the call, which runs a flush the
    last close asked for), pooled rows bit-equal to apply_emb, no key twice, size <= capacity, hist sums to size, n_hits grows by
    the flagged positions, and every missed key position is either re-pointed or served in place.
    At 26 tables the plain stream never has an all-served sample (the model: the top bucket stays empty), so no flush would ever
    fire; three directed calls in the middle -- 64 keys, eight to every set, one in a bag of its own per sample and table:
    installed (a key the stream had left resident can lose its way to the others there; the second call then brings it back and
    the third finds all), then all hit -- put the whole capacity into the top bucket.  The stream goes on across the flush."""
    g = G1C
    T, B, cap, d = g["T"], g["B"], g["cap"], g["d"]
    c, _pinned, dev, _tabs = _cache_c(E, "G1C")
    ev = E.EVTables(dev, d, 32)
    full = _call_of(B, T, {(s, t): [int(_set_rows("G1C", t, s)[0])] for s in range(8) for t in range(8)})
    assert np.bincount([_set_of("G1C", k) for k in BP.keys_of(full[1])], minlength=8).tolist() == [8] * 8
    plain = _plain_calls(g, 16, 9)
    calls = plain[:8] + [full, full, full] + plain[8:]
    before, n_hits, flushes, perfect, all_served_at, f0, n_in_place = {}, 0, [], [], [], c.fetch_stats(), 0
    for i, (off, idx) in enumerate(calls):
        lS_o, lS_i = _up(off, idx)
        if i:
            before = _dump(c)
        hits, ly = c.lookup_bags(lS_o, lS_i)
        got = np.concatenate(_np_flags(hits))
        keys = BP.keys_of(idx)
        assert np.array_equal(got, np.array([k in before for k in keys], bool)), "call %d: flags are not residency at arrival" % i
        assert np.array_equal(_bits(_np_pooled(ly)), _bits(_apply_emb(E, ev, lS_o, lS_i))), "call %d: pooled rows" % i
        n_hits += int(got.sum())
        f1 = c.fetch_stats()
        assert f1["repointed"] - f0["repointed"] + f1["in_place"] - f0["in_place"] == int((~got).sum()), "call %d" % i
        n_in_place += f1["in_place"] - f0["in_place"]
        f0 = f1
        st = c.batch_stats()
        after = _dump(c)
        assert len(after) == st["size"] <= cap and sum(st["hist"]) == st["size"] and max(after.values()) <= T, "call %d" % i
        assert (st["n_hits"], st["n_requests"]) == (n_hits, B * (i + 1)), "call %d: counters" % i
        flushes.append(st["n_flush"])
        perfect.append(st["n_perfect_hits"])
        if i in (9, 10) and got.all():                          # a directed call that finds every key: its 8 samples with a lookup all served
            assert perfect[i] - perfect[i - 1] == 8
            all_served_at.append(i)
    assert all_served_at and flushes[all_served_at[0] - 1] == 0 and flushes[-1] >= 1, (all_served_at, flushes)
    assert n_in_place > 0, "no set was ever crowded"


# ---------------------------------------------------------------------------------------------------------------- 8. refusals
def _small_call(geom, B=4):
    T = GEOMS[geom]["T"]
    return [_dev(np.arange(B, dtype=np.int64))] * T, [_dev(np.zeros(B, np.int64))] * T


def _serves_bags(c, tabs, geom):
    """the same small call twice: rows exact, then all hits"""
    lo, li = _small_call(geom)
    for _ in range(2):
        hits, ly = c.lookup_bags(lo, li)
        for t in range(GEOMS[geom]["T"]):
            assert np.array_equal(_bits(ly[t].cpu().numpy()), _bits(tabs[t][[0] * 4]))
    assert torch.cat(hits).all()


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_refusal_of_the_setter_on_lru_lfu(E, policy):
    L = E._lib
    raws, tabs = _tables("G2", 32)
    c = _cache(E, "G2", 32, [_dev(r) for r in raws], policy=policy, rule=None)
    _refused(E, L.EVS_EINVAL, policy, lambda: c.set_bag_count("count-first"))
    assert L.lib().evs_cache_set_bag_count(c._h, 2) == L.EVS_EINVAL and policy.encode() in L.lib().evs_last_error()
    assert L.lib().evs_cache_set_bag_count(c._h, -1) == L.EVS_EINVAL
    with pytest.raises(ValueError):
        c.set_bag_count("sideways")
    assert c.set_bag_count("pooling-walk") is c
    _serves_bags(c, tabs, "G2")


def test_refusals_of_an_order_1_count_first_call(E, tmp_path):
    """Each refusal comes before anything is allocated and leaves the cache serving a following valid call."""
    g = G2
    L = E._lib
    raws, tabs = _tables("G2", 32)
    lo, li = _small_call("G2")
    x = torch.zeros(4, g["d"], device="cuda")
    # without a bag rule
    c = _cache(E, "G2", 32, [_pin(r) for r in raws], order="fetch-first", count="count-first", rule=None)
    _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_bags(lo, li))
    _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_bags_interact(lo, li, x))
    assert c.fetch_stats()["calls"] == 0
    c.set_bag_rule("served-bags")
    _serves_bags(c, tabs, "G2")
    assert c.fetch_stats()["calls"] == 2
    # the plan / sampled policy
    for name in ("sampled", "plan"):
        c = _cache(E, "G2", 32, [_pin(r) for r in raws], order="fetch-first", count="count-first")
        c.set_batch_policy(name)
        assert name in _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_bags(lo, li))
        assert c.fetch_stats()["calls"] == 0
        c.set_batch_policy("setassoc")                         # (nothing was allocated: the policy may still be given)
        _serves_bags(c, tabs, "G2")
        assert c.fetch_stats()["calls"] == 2
    # file-backed tables
    paths = []
    for k, t in enumerate(tabs):
        p = tmp_path / ("ev-table-%d.bin" % (k + 1))
        t.tofile(p)
        paths.append(str(p))
    ft = E.FileTier(paths, g["d"] * 4, 1 << 30)
    c = E.GpuCache("evlfu", g["cap"], g["T"], g["d"], 32).set_miss_order("fetch-first")
    c.set_file_backing(ft)
    c.set_bag_rule("served-bags").set_bag_count("count-first")
    _refused(E, L.EVS_ESTATE, "evlfu", lambda: c.lookup_bags(lo, li))
    assert c.fetch_stats()["calls"] == 0
    # order 0 + count-first over pinned tables: consume-first still reads HBM only
    c = _cache(E, "G2", 32, [_pin(r) for r in raws], count="count-first")
    _refused(E, L.EVS_ESTATE, "evlfu", lambda: c.lookup_bags(lo, li))
    _refused(E, L.EVS_ESTATE, "evlfu", lambda: c.lookup_bags_interact(lo, li, x))
    c.set_backing([_dev(r) for r in raws])
    _serves_bags(c, tabs, "G2")
    assert c.fetch_stats()["calls"] == 0


@pytest.mark.parametrize("switch,value", [("EVS_SA_DUAL", "0"), ("EVS_SA_WAYS", "16")])
def test_refusals_behind_a_process_wide_switch(switch, value):
    """EVS_SA_DUAL=0 / EVS_SA_WAYS=16 are read once per process: an order-1 count-first call is refused with the switch named; with
    the one-copy arena an order-0 count-first cache serves and equals the default chain (tests/_bags_count_first_env_child.py,
    started fresh)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("EVS_SA_DUAL", "EVS_SA_WAYS", "EVS_CACHE_POLICY")}
    env[switch] = value
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_bags_count_first_env_child.py"), switch], env=env, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
