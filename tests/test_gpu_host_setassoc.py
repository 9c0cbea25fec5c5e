"""The set-associative cache tier in fetch-first order (evs_cache_set_miss_order(c, 1): probe -> update -> sa_repoint ->
consumers; include/evstore_hip.h) over tables in HBM and in pinned host memory.  On conflict-free streams three caches see the
same calls -- A: HBM tables, order 0, the two-launch chain (the yardstick); B: HBM tables, order 1; C: pinned tables, order 1 --
and must agree flag for flag, bit for bit and way for way, with each other and with the Python models of the rule
(tests/_batched_policy_model.py, _bag_policy_model.py, _bag_evlfu_model.py).  Directed cases pin what the re-point kernel does
with copies of a key, a crowded set, an index out of range and an EvLFU way that is hit and replaced by one batch; crowded
streams hold the invariants; an overwritten pinned table shows that hits are served from the arena; the refusals leave the
cache serving.

Two geometries: G1 -- 26 tables of 300 rows, d = 36, capacity 512 (64 sets; 64 = 8 sets for the crowded cases), B = 40 / 64 --
and G2 -- 3 tables of 5 / 3000 / 70 rows, d = 16, capacity 64, B = 37: few tables, a tiny table that puts many positions on one
way, a B that fills neither a wave nor a block."""
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
GEOMS = {"G1": G1, "G1C": G1C, "G2": G2}
POLICIES = ("evlfu", "lru", "lfu")
N_BATCHES = 12
SEED = 3
# The bag stream of G1: a call has ~2600 positions over 64 sets, and a conflict-free call brings at most one new key per set.  At
# the generators' default Zipf exponent (1.3) no such draw exists (conflict_free_bags gives up after 1000 redraws); at 2.0 the
# redraws land on keys the call already brought.
BAG_ALPHA = 2.0


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
    raws = [orc.encode_table(np.clip(t * np.sqrt(len(t)), -1, 1), codec) for t in tabs]   # (spread over the codec's range: rows differ)
    return raws, [orc.decode(a, codec, g["d"]) for a in raws]


def _cache(E, policy, geom, codec, backing, order=None, inline=None):
    g = GEOMS[geom]
    c = E.GpuCache(policy, g["cap"], g["T"], g["d"], codec)
    if order is not None:
        assert c.set_miss_order(order) is c
    if inline is not None:
        c.set_inline_update(inline)
    c.set_backing(backing)
    return c


def _three(E, policy, geom, codec):
    """-> (A, B, C), the fp32 rows, the HBM tensors"""
    raws, tabs = _tables(geom, codec)
    dev = [_dev(r) for r in raws]
    a = _cache(E, policy, geom, codec, dev, inline=False)
    b = _cache(E, policy, geom, codec, dev, order="fetch-first")
    c = _cache(E, policy, geom, codec, [_pin(r) for r in raws], order="fetch-first")
    return (a, b, c), tabs, dev


def _dump(c):
    d = c.batch_dump()
    keys = [(int(t), int(r)) for _, t, r in d]
    assert len(set(keys)) == len(keys), "a key is resident twice"
    return {k: int(s) for k, (s, _, _) in zip(keys, d)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows_exact(out, tabs, rq):
    for t in range(rq.shape[1]):
        assert np.array_equal(_bits(out[:, t, :]), _bits(tabs[t][rq[:, t]])), "table %d" % t


@functools.lru_cache(maxsize=None)
def _bt_stream(policy, geom):
    """-> ((N_BATCHES, B, T) int32 rows, the model's flags); conflict-free, and for evlfu without a flush"""
    g = GEOMS[geom]
    if policy == "evlfu":
        rows, flags, _ = EM.conflict_free_rows_stream(g["cap"], list(g["n_rows"]), g["B"], N_BATCHES, SEED)
        m = EM.BagEvLFUModel(g["cap"], list(g["n_rows"]))
        for i in range(N_BATCHES):
            m.batch_bags(*EM.one_per_bag(rows[i]))
            assert m.top_bucket() < int(0.95 * g["cap"]), "the stream would flush"
        return rows, flags
    rows, flags, _ = M.conflict_free_stream(policy, g["cap"], list(g["n_rows"]), g["B"], N_BATCHES, SEED)
    return rows, flags


class _Account:
    """fetch_stats / batch_stats of one order-1 cache, call by call"""

    def __init__(self, c, used=False):
        self.c, self.f = c, c.fetch_stats()
        self.s = c.batch_stats() if used else {"size": 0, "n_evict": 0}
        self.calls = self.f["calls"]
        assert used or self.f == {"calls": 0, "repointed": 0, "in_place": 0}

    def step(self):
        """-> (re-pointed, in place, size + evictions) of the last call"""
        f, s = self.c.fetch_stats(), self.c.batch_stats()
        self.calls += 1
        assert f["calls"] == self.calls
        out = (f["repointed"] - self.f["repointed"], f["in_place"] - self.f["in_place"],
               s["size"] - self.s["size"] + s["n_evict"] - self.s["n_evict"])
        self.f, self.s = f, s
        return out


# ------------------------------------------------------------------------------------------- 1. twins on conflict-free streams
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("geom,codec,form", [("G1", 32, "batch"), ("G1", 8, "batch"), ("G1", 4, "batch"), ("G2", 32, "batch"),
                                             ("G2", 8, "batch"), ("G1", 32, "interact"), ("G2", 32, "interact")])
def test_twins_on_conflict_free_streams(E, policy, geom, codec, form):
    """No call brings two new keys to one set (and no flush fires), so the rule is deterministic.  After every call: flags equal
    across A, B, C and equal the model's; out / R bit-equal across the three, out bit-equal to the table rows; dump and
    statistics equal, the dump equal to the model's resident set and scores; A's and B's exported state equal but for the
    inline setting.  B and C: every missed position re-pointed and one installed way per distinct missed key -- the update is
    the only reader of the table -- except for a key the MODEL turns away (lru / lfu: every way of its set was touched by
    this very batch; under 1 % of the positions of these streams), whose positions are exactly the ones served in place."""
    g = GEOMS[geom]
    T, d, B = g["T"], g["d"], g["B"]
    reqs, want_flags = _bt_stream(policy, geom)
    caches, tabs, _dev_tabs = _three(E, policy, geom, codec)
    acct = [_Account(c) for c in caches[1:]]
    n_rows = list(g["n_rows"])
    model = EM.BagEvLFUModel(g["cap"], n_rows) if policy == "evlfu" else M.BatchedPolicyModel(policy, g["cap"], n_rows)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    n_turned = 0
    for i in range(N_BATCHES):
        rq = reqs[i]
        r = _dev(rq)
        if policy == "evlfu":
            model.batch_bags(*EM.one_per_bag(rq))
        else:
            model.batch(rq)
        resident = model.resident()
        if form == "batch":
            res = [c.lookup_batch(r) for c in caches]
        else:
            x = torch.empty(B, d, device="cuda").uniform_(-1, 1, generator=gen)
            res = [c.lookup_interact(r, x) for c in caches]
        flags = [h.cpu().numpy().astype(bool) for h, _ in res]
        outs = [o.cpu().numpy() for _, o in res]
        for k in range(3):
            assert np.array_equal(flags[k], want_flags[i]), "call %d, cache %s: %d flags differ from the model" % (
                i + 1, "ABC"[k], int((flags[k] != want_flags[i]).sum()))
            assert np.array_equal(_bits(outs[k]), _bits(outs[0])), "call %d: cache %s's output differs from A's" % (i + 1, "ABC"[k])
        if form == "batch":
            _rows_exact(outs[0], tabs, rq)
        dumps = [_dump(c) for c in caches]
        stats = [c.batch_stats() for c in caches]
        assert dumps[0] == dumps[1] == dumps[2] == resident, "call %d: resident sets" % (i + 1)
        assert stats[0] == stats[1] == stats[2], "call %d: statistics\n%s" % (i + 1, stats)
        assert stats[0]["n_flush"] == 0
        sa, sb = caches[0].export_state(), caches[1].export_state()
        assert np.array_equal(sa["entries"], sb["entries"]), "call %d: exported entries" % (i + 1)
        keep = np.arange(16) != 14                            # (state[14]: the inline-update setting)
        assert np.array_equal(sa["state"][keep], sb["state"][keep]), "call %d: exported state" % (i + 1)
        missed = [(t + 1, int(rq[b, t])) for b, t in zip(*np.nonzero(~want_flags[i]))]
        away = sum(k not in resident for k in missed)         # positions of the keys the model turned away
        n_turned += away
        for a in acct:
            assert a.step() == (len(missed) - away, away, len({k for k in missed if k in resident})), "call %d" % (i + 1)
    assert stats[0]["n_evict"] > 0 and stats[0]["n_hits"] > 0
    assert n_turned * 100 <= reqs.size and (policy != "evlfu" or n_turned == 0)    # (turned away: under 1 % of the positions)
    assert caches[0].fetch_stats() == {"calls": 0, "repointed": 0, "in_place": 0}


# ------------------------------------------------------------------------------------------------------- 2. bags, lru / lfu
@functools.lru_cache(maxsize=None)
def _bag_stream(policy):
    return BP.conflict_free_bag_stream(policy, G1["cap"], list(G1["n_rows"]), G1["B"], 5, N_BATCHES, SEED, alpha=BAG_ALPHA)[0]


def _np_pooled(ly):
    return torch.stack([t for t in ly]).cpu().numpy()


@pytest.mark.parametrize("policy", ["lru", "lfu"])
@pytest.mark.parametrize("form", ["bags", "bags_interact"])
def test_bag_twins_on_conflict_free_streams(E, policy, form):
    """Ragged bags of 0 .. 5 indices (empty bags among them) through the same three caches: flags equal the model's, pooled rows
    bit-equal to apply_emb over the HBM tables, R bit-equal across the three, dump (the model's), statistics and A's / B's
    exported state equal, and the same account of the re-point kernel as in the (B, T) form."""
    g = G1
    T, d, B = g["T"], g["d"], g["B"]
    calls = _bag_stream(policy)
    assert any((np.diff(np.append(o, len(ix))) == 0).any() for off, idx, _ in calls for o, ix in zip(off, idx)), "no empty bag"
    caches, _tabs, dev = _three(E, policy, "G1", 32)
    ev = E.EVTables(dev, d, 32)
    acct = [_Account(c) for c in caches[1:]]
    model = BP.BagPolicyModel(policy, g["cap"], list(g["n_rows"]))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(12)
    n_turned = 0
    for i, (off, idx, want_flags) in enumerate(calls):
        model.batch_bags(off, idx)
        resident = model.resident()
        lS_o, lS_i = [_dev(o) for o in off], [_dev(ix) for ix in idx]
        if form == "bags":
            res = [c.lookup_bags(lS_o, lS_i) for c in caches]
            outs = [_np_pooled(ly) for _, ly in res]
            assert np.array_equal(_bits(outs[0]), _bits(_np_pooled(E.apply_emb(lS_o, lS_i, ev, lazy=False)))), "call %d: pooled rows" % (i + 1)
        else:
            x = torch.empty(B, d, device="cuda").uniform_(-1, 1, generator=gen)
            res = [c.lookup_bags_interact(lS_o, lS_i, x) for c in caches]
            outs = [o.cpu().numpy() for _, o in res]
        for k in range(3):
            got = [h.cpu().numpy().astype(bool) for h in res[k][0]]
            assert all(np.array_equal(a, b) for a, b in zip(got, want_flags)), "call %d, cache %s: flags" % (i + 1, "ABC"[k])
            assert np.array_equal(_bits(outs[k]), _bits(outs[0])), "call %d: cache %s's output differs from A's" % (i + 1, "ABC"[k])
        dumps = [_dump(c) for c in caches]
        stats = [c.batch_stats() for c in caches]
        assert dumps[0] == dumps[1] == dumps[2] == resident, "call %d: resident sets" % (i + 1)
        assert stats[0] == stats[1] == stats[2], "call %d: statistics\n%s" % (i + 1, stats)
        sa, sb = caches[0].export_state(), caches[1].export_state()
        keep = np.arange(16) != 14
        assert np.array_equal(sa["entries"], sb["entries"]) and np.array_equal(sa["state"][keep], sb["state"][keep])
        missed = [(k + 1, int(r)) for k in range(T) for r, f in zip(idx[k], want_flags[k]) if not f]
        away = sum(k not in resident for k in missed)         # positions of the keys the model turned away
        n_turned += away
        for a in acct:
            assert a.step() == (len(missed) - away, away, len({k for k in missed if k in resident})), "call %d" % (i + 1)
    assert stats[0]["n_evict"] > 0 and stats[0]["n_perfect_hits"] > 0
    assert n_turned * 100 <= sum(len(ix) for _, idx, _ in calls for ix in idx)


# ------------------------------------------------------------------------------------------------- 3. directed cases, cache C
def _cache_c(E, policy, geom):
    raws, tabs = _tables(geom, 32)
    return _cache(E, policy, geom, 32, [_pin(r) for r in raws], order="fetch-first"), tabs


def _free_rows(n_rows, nset, bits, t, s, want_in):
    """rows of table t whose set is (want_in) / is not s"""
    rows = np.arange(n_rows[t])
    return rows[(M.set_of(t, rows, nset, list(n_rows), bits) == s) == want_in]


@pytest.mark.parametrize("policy", POLICIES)
def test_copies_of_one_fresh_key(E, policy):
    """Every sample names one fresh key of table 0 (the other columns hit): one way is installed and every copy is re-pointed at
    it -- only the compare-and-swap's winner knew the way."""
    g = G2
    c, tabs = _cache_c(E, policy, "G2")
    B, T = g["B"], g["T"]
    fill = np.tile(np.array([[0, 100, 7]], np.int32), (B, 1))
    hit, out = c.lookup_batch(_dev(fill))
    _rows_exact(out.cpu().numpy(), tabs, fill)
    acct = _Account(c, used=True)
    assert acct.calls == 1
    rq = fill.copy()
    rq[:, 0] = 3
    hit, out = c.lookup_batch(_dev(rq))
    hit = hit.cpu().numpy().astype(bool)
    assert not hit[:, 0].any() and hit[:, 1:].all()
    _rows_exact(out.cpu().numpy(), tabs, rq)
    assert acct.step() == (B, 0, 1)
    assert set(_dump(c)) == {(1, 0), (2, 100), (3, 7), (1, 3)}
    hit, out = c.lookup_batch(_dev(rq))
    assert hit.all()
    _rows_exact(out.cpu().numpy(), tabs, rq)


@pytest.mark.parametrize("policy", POLICIES)
def test_a_crowded_set(E, policy):
    """Twelve fresh keys of one set in one call (capacity 64: 8 sets): 8 are installed; the positions of the other four are the
    ones served in place from the pinned table, and every row is exact."""
    g = G1C
    B, T, n_rows = g["B"], g["T"], g["n_rows"]
    nset, bits = M.geometry(g["cap"], n_rows)
    c, tabs = _cache_c(E, policy, "G1C")
    s = 5
    away = [int(_free_rows(n_rows, nset, bits, t, s, False)[0]) for t in range(T)]    # one resident key per column, none in set s
    fill = np.tile(np.array([away], np.int32), (B, 1))
    c.lookup_batch(_dev(fill))
    c.lookup_batch(_dev(fill))
    assert set(_dump(c)) == {(t + 1, away[t]) for t in range(T)}
    fresh = _free_rows(n_rows, nset, bits, 0, s, True)[:12]
    assert len(fresh) == 12
    rq = fill.copy()
    rq[:, 0] = fresh[np.arange(B) % 12]
    f0, s0 = c.fetch_stats(), c.batch_stats()
    hit, out = c.lookup_batch(_dev(rq))
    hit = hit.cpu().numpy().astype(bool)
    assert not hit[:, 0].any() and hit[:, 1:].all()
    _rows_exact(out.cpu().numpy(), tabs, rq)
    f1, s1, after = c.fetch_stats(), c.batch_stats(), _dump(c)
    kept = {int(r) for r in fresh if (1, int(r)) in after}
    assert len(kept) == 8 and s1["size"] - s0["size"] + s1["n_evict"] - s0["n_evict"] == 8
    n_away = int(sum(int(r) not in kept for r in rq[:, 0]))
    assert f1["in_place"] - f0["in_place"] == n_away > 0
    assert f1["repointed"] - f0["repointed"] == B - n_away
    flags_after = np.array([(1, int(r)) in after for r in rq[:, 0]])
    hit, out = c.lookup_batch(_dev(rq))
    assert np.array_equal(hit.cpu().numpy().astype(bool)[:, 0], flags_after)
    _rows_exact(out.cpu().numpy(), tabs, rq)


@pytest.mark.parametrize("policy", POLICIES)
def test_an_index_out_of_range_bt(E, policy):
    """An index past its table and a negative one in the middle of a (B, T) batch: flag 0, a zero row, no key inserted and
    neither counter of the re-point kernel moved by them.  (The (B, T) probe raises no sticky flag under either order; the bag
    form, below, does.)"""
    g = G2
    c, tabs = _cache_c(E, policy, "G2")
    B = g["B"]
    rs = np.random.RandomState(4)
    rq = np.stack([rs.randint(0, n, B) for n in g["n_rows"]], 1).astype(np.int32)
    c.lookup_batch(_dev(rq))
    f0, before = c.fetch_stats(), _dump(c)
    rq2 = np.stack([rs.randint(0, n, B) for n in g["n_rows"]], 1).astype(np.int32)
    rq2[17, 1] = g["n_rows"][1]
    rq2[18, 2] = -1
    hit, out = c.lookup_batch(_dev(rq2))
    hit, out = hit.cpu().numpy().astype(bool), out.cpu().numpy()
    assert not hit[17, 1] and not hit[18, 2]
    assert not out[17, 1].any() and not out[18, 2].any()
    ok = np.ones(rq2.shape, bool)
    ok[17, 1] = ok[18, 2] = False
    for t in range(g["T"]):
        assert np.array_equal(_bits(out[ok[:, t], t]), _bits(tabs[t][rq2[ok[:, t], t]]))
        assert np.array_equal(hit[ok[:, t], t], np.array([(t + 1, int(r)) in before for r in rq2[ok[:, t], t]]))
    f1 = c.fetch_stats()
    assert f1["repointed"] - f0["repointed"] + f1["in_place"] - f0["in_place"] == int((~hit & ok).sum())
    assert all(0 <= r < g["n_rows"][t - 1] for t, r in _dump(c))


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_an_index_out_of_range_bags(E, policy):
    """The same through the bag form, one index per bag: flag 0, a zero pooled row, evs_check_index_errors raised once, and
    neither counter moved by the two positions."""
    g = G2
    L = E._lib
    c, tabs = _cache_c(E, policy, "G2")
    B, T = g["B"], g["T"]
    rs = np.random.RandomState(5)
    off = [_dev(np.arange(B, dtype=np.int64))] * T
    idx = [rs.randint(0, n, B).astype(np.int64) for n in g["n_rows"]]
    c.lookup_bags(off, [_dev(i) for i in idx])
    assert L.lib().evs_check_index_errors(None) == 0
    f0, before = c.fetch_stats(), _dump(c)
    idx = [rs.randint(0, n, B).astype(np.int64) for n in g["n_rows"]]
    idx[1][17] = g["n_rows"][1]
    idx[2][18] = -1
    hits, ly = c.lookup_bags(off, [_dev(i) for i in idx])
    assert L.lib().evs_check_index_errors(None) == L.EVS_EINDEX
    assert L.lib().evs_check_index_errors(None) == 0
    n_missed = 0
    for t in range(T):
        h, o = hits[t].cpu().numpy().astype(bool), ly[t].cpu().numpy()
        ok = np.ones(B, bool)
        if t == 1:
            ok[17] = False
        if t == 2:
            ok[18] = False
        assert not h[~ok].any() and not o[~ok].any()
        assert np.array_equal(_bits(o[ok]), _bits(tabs[t][idx[t][ok]]))
        assert np.array_equal(h[ok], np.array([(t + 1, int(r)) in before for r in idx[t][ok]]))
        n_missed += int((~h & ok).sum())
    f1 = c.fetch_stats()
    assert f1["repointed"] - f0["repointed"] + f1["in_place"] - f0["in_place"] == n_missed


@functools.lru_cache(maxsize=None)
def _victim_hit_case():
    """-> (rows (n, B, T), flags, the index of the call in which the model evicts a key that call also hits, that key, the key
    that takes its way, the model's resident set after that call).  Seeds are searched in order; the streams are conflict-free
    (a flatter Zipf than the twins': a request with a single hit raises its way to priority 1 only, which keeps it a victim)."""
    g = G2
    n_rows, cap, B, T = list(g["n_rows"]), g["cap"], g["B"], g["T"]
    for seed in range(40):
        try:
            rows, flags, _ = EM.conflict_free_rows_stream(cap, n_rows, B, 10, seed, alpha=1.2)
        except AssertionError:
            continue
        m = EM.BagEvLFUModel(cap, n_rows)
        for i in range(10):
            before = dict(m.where)
            fl = np.stack(m.batch_bags(*EM.one_per_bag(rows[i])), 1)
            if m.top_bucket() >= int(0.95 * cap):
                break                                          # (the flush is not modelled)
            hit_keys = {(t + 1, int(rows[i][b, t])) for b in range(B) for t in range(T) if fl[b, t]}
            both = (set(before) - set(m.where)) & hit_keys
            if both and i >= 1:
                old = sorted(both)[0]
                new = [k for k, at in m.where.items() if at == before[old]]
                return rows[:i + 1], flags[:i + 1], i, old, new[0], m.resident()
    raise AssertionError("no seed gives the case")


def test_evlfu_hit_way_is_the_same_batchs_victim(E):
    """The case the two-copy arena exists for.  The model says that the last call hits a key AND evicts it (its request has no
    other hit: the raise leaves it the lowest priority of its set).  The update runs in front of the consumers, so when they
    read, the way already names the new key: the evicted key's row must still be ITS table row (the old copy, intact), the new
    key's row its own, and the dump shows the new key only."""
    g = G2
    rows, flags, at, old, new, resident = _victim_hit_case()
    assert old not in resident and new in resident                      # the model says so ...
    b_old = [(b, t) for b in range(g["B"]) for t in range(g["T"]) if (t + 1, int(rows[at][b, t])) == old]
    b_new = [(b, t) for b in range(g["B"]) for t in range(g["T"]) if (t + 1, int(rows[at][b, t])) == new]
    assert b_old and all(flags[at][b, t] for b, t in b_old) and b_new and not any(flags[at][b, t] for b, t in b_new)   # ... hit and replaced
    c, tabs = _cache_c(E, "evlfu", "G2")
    for i in range(at + 1):
        hit, out = c.lookup_batch(_dev(rows[i]))
        assert np.array_equal(hit.cpu().numpy().astype(bool), flags[i]), "call %d: flags" % (i + 1)
        out = out.cpu().numpy()
        _rows_exact(out, tabs, rows[i])
    for b, t in b_old:
        assert np.array_equal(_bits(out[b, t]), _bits(tabs[t][old[1]]))
    for b, t in b_new:
        assert np.array_equal(_bits(out[b, t]), _bits(tabs[t][new[1]]))
    assert _dump(c) == resident
    assert c.batch_stats()["n_flush"] == 0


# ------------------------------------------------------------------------------------------- 4. crowded streams: invariants
@pytest.mark.parametrize("policy", POLICIES)
def test_crowded_streams_hold_the_invariants(E, policy):
    """Uniform rows over 8 sets: most calls bring several new keys to a set, so which of them wins a way is a matter of timing
    and C need not agree with A key for key.  Both serve every row exactly with flags = residency in the dump taken before the
    call, hold no key twice and never more than the capacity; per call C accounts for every missed position."""
    g = G1C
    B, T, cap = g["B"], g["T"], g["cap"]
    raws, tabs = _tables("G1C", 32)
    a = _cache(E, policy, "G1C", 32, [_dev(r) for r in raws], inline=False)
    c = _cache(E, policy, "G1C", 32, [_pin(r) for r in raws], order="fetch-first")
    rs = np.random.RandomState(9)
    f0 = c.fetch_stats()
    n_in_place = 0
    for i in range(30):
        rq = np.stack([rs.randint(0, n, B) for n in g["n_rows"]], 1).astype(np.int32)
        r = _dev(rq)
        for cache in (a, c):
            before = _dump(cache) if i else {}                 # (a fresh cache has no batched state to dump)
            hit, out = cache.lookup_batch(r)
            hit = hit.cpu().numpy().astype(bool)
            _rows_exact(out.cpu().numpy(), tabs, rq)
            want = np.array([[(t + 1, int(rq[b, t])) in before for t in range(T)] for b in range(B)])
            # (the dump runs a flush the last close asked for: it shows what this call's probe will see)
            assert np.array_equal(hit, want), "call %d: flags are not residency at arrival" % (i + 1)
            assert len(_dump(cache)) == cache.batch_stats()["size"] <= cap
        f1 = c.fetch_stats()
        assert f1["repointed"] - f0["repointed"] + f1["in_place"] - f0["in_place"] == int((~hit).sum()), "call %d" % (i + 1)
        n_in_place += f1["in_place"] - f0["in_place"]
        f0 = f1
    assert n_in_place > 0, "no set was ever crowded"


# ---------------------------------------------------------------------------------------------------- 5. the arena serves hits
@pytest.mark.parametrize("policy", POLICIES)
def test_the_arena_serves_hits(E, policy):
    """Three calls on one key set warm C; then the pinned tables are overwritten in place from the CPU.  The next call on the same
    keys returns the OLD bytes at every flag-1 position -- hits never touch the table -- (and the new ones at the others, which
    the update fetched just now), and after refresh_rows of those keys the new bytes everywhere."""
    g = G2
    raws, tabs = _tables("G2", 32)
    pinned = [_pin(r) for r in raws]
    c = _cache(E, policy, "G2", 32, pinned, order="fetch-first")
    rs = np.random.RandomState(6)
    rq = np.stack([rs.randint(0, n, g["B"]) for n in g["n_rows"]], 1).astype(np.int32)
    r = _dev(rq)
    for _ in range(3):
        c.lookup_batch(r)
    torch.cuda.synchronize()
    new_tabs = [(-2.0 * t - 1.0).astype(np.float32) for t in tabs]
    for p, n in zip(pinned, new_tabs):
        assert p.dtype == torch.float32 and tuple(p.shape) == n.shape
        p.copy_(torch.from_numpy(n))                           # in place: the cache holds the tensor's address
    hit, out = c.lookup_batch(r)
    hit, out = hit.cpu().numpy().astype(bool), out.cpu().numpy()
    assert hit.mean() > 0.5
    for t in range(g["T"]):
        h = hit[:, t]
        assert np.array_equal(_bits(out[h, t]), _bits(tabs[t][rq[h, t]])), "table %d: a hit was not served from the arena" % t
        assert np.array_equal(_bits(out[~h, t]), _bits(new_tabs[t][rq[~h, t]])), "table %d: misses" % t
    keys = sorted({(t, int(rq[b, t])) for b in range(g["B"]) for t in range(g["T"])})
    c.refresh_rows(np.array(keys, np.int64))
    hit, out = c.lookup_batch(r)
    _rows_exact(out.cpu().numpy(), new_tabs, rq)


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def _refused(E, code, policy, fn):
    """policy None: a refusal of today's whose wording does not name it"""
    with pytest.raises(E._lib.EvsError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    assert policy is None or policy in str(ei.value), str(ei.value)
    return str(ei.value)


def _serves(c, tabs, n_rows, B=5, seed=8):
    """two batches, the second the first again: rows exact, then all hits"""
    rs = np.random.RandomState(seed)
    rq = np.stack([rs.randint(0, n, B) for n in n_rows], 1).astype(np.int32)
    for i in range(2):
        hit, out = c.lookup_batch(_dev(rq))
        _rows_exact(out.cpu().numpy(), tabs, rq)
    assert hit.all()


@pytest.mark.parametrize("policy", POLICIES)
def test_refusals_of_the_switch(E, policy):
    g = G2
    L = E._lib
    raws, tabs = _tables("G2", 32)
    dev = [_dev(r) for r in raws]
    # after a batched call
    c = _cache(E, policy, "G2", 32, dev)
    _serves(c, tabs, g["n_rows"])
    _refused(E, L.EVS_ESTATE, policy, lambda: c.set_miss_order("fetch-first"))
    _serves(c, tabs, g["n_rows"], seed=9)
    assert c.fetch_stats()["calls"] == 0
    # an order outside {0, 1}
    c = _cache(E, policy, "G2", 32, dev)
    assert L.lib().evs_cache_set_miss_order(c._h, 2) == L.EVS_EINVAL and policy.encode() in L.lib().evs_last_error()
    assert L.lib().evs_cache_set_miss_order(c._h, -1) == L.EVS_EINVAL
    with pytest.raises(ValueError):
        c.set_miss_order("sideways")
    assert L.lib().evs_cache_fetch_stats(c._h, None, None) == L.EVS_EINVAL and b"NULL out4" in L.lib().evs_last_error()
    assert c.set_miss_order("consume-first") is c
    _serves(c, tabs, g["n_rows"])
    # against the inline update, in both orders (an lru / lfu cache refuses on = 1 by itself)
    c = _cache(E, policy, "G2", 32, dev, order="fetch-first")
    _refused(E, L.EVS_EINVAL, policy, lambda: c.set_inline_update(True))
    c.set_inline_update(False)
    _serves(c, tabs, g["n_rows"])
    assert c.fetch_stats()["calls"] == 2
    if policy == "evlfu":
        c = _cache(E, policy, "G2", 32, dev, inline=True)
        _refused(E, L.EVS_EINVAL, policy, lambda: c.set_miss_order("fetch-first"))
        _serves(c, tabs, g["n_rows"])
        assert c.fetch_stats()["calls"] == 0


def test_refusal_sampled_plus_fetch_first(E):
    g = G2
    L = E._lib
    raws, tabs = _tables("G2", 32)
    for policy_name in ("sampled", "plan"):
        c = _cache(E, "evlfu", "G2", 32, [_pin(r) for r in raws], order="fetch-first")
        c.set_batch_policy(policy_name)
        rq = _dev(np.zeros((4, 3), np.int32))
        assert policy_name in _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_batch(rq))
        c.set_batch_policy("setassoc")                         # (nothing was allocated: the policy may still be given)
        _serves(c, tabs, g["n_rows"])
        assert c.fetch_stats()["calls"] == 2


@pytest.mark.parametrize("policy", POLICIES)
def test_refusal_file_tier(E, policy, tmp_path):
    g = G2
    L = E._lib
    raws, tabs = _tables("G2", 32)
    paths = []
    for k, t in enumerate(tabs):
        p = tmp_path / ("ev-table-%d.bin" % (k + 1))
        t.tofile(p)
        paths.append(str(p))
    ft = E.FileTier(paths, g["d"] * 4, 1 << 30)
    c = E.GpuCache(policy, g["cap"], g["T"], g["d"], 32).set_miss_order("fetch-first")
    c.set_file_backing(ft)
    rq = _dev(np.zeros((4, 3), np.int32))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_batch(rq))
    assert c.fetch_stats()["calls"] == 0
    c = _cache(E, policy, "G2", 32, [_pin(r) for r in raws], order="fetch-first")    # a fresh one over pinned tables
    _serves(c, tabs, g["n_rows"])
    assert c.fetch_stats()["calls"] == 2


def test_refusal_evlfu_bags(E):
    g = G2
    L = E._lib
    raws, tabs = _tables("G2", 32)
    c = _cache(E, "evlfu", "G2", 32, [_pin(r) for r in raws], order="fetch-first").set_bag_rule("served-bags")
    off = [_dev(np.arange(4, dtype=np.int64))] * 3
    idx = [_dev(np.zeros(4, np.int64))] * 3
    msg = _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_bags(off, idx))
    assert "pooling" in msg
    x = torch.zeros(4, g["d"], device="cuda")
    _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_bags_interact(off, idx, x))
    _serves(c, tabs, g["n_rows"])
    assert c.fetch_stats()["calls"] == 2


def test_refusal_pair_member(E):
    g = G2
    L = E._lib
    raws, tabs = _tables("G2", 32)
    dev = [_dev(r) for r in raws]
    c1 = _cache(E, "evlfu", "G2", 32, dev, order="fetch-first")
    c2 = _cache(E, "evlfu", "G2", 32, dev)
    rq = _dev(np.zeros((4, 3), np.int32))
    out = torch.empty(4, 3, g["d"], device="cuda")
    tier = torch.empty(4, 3, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    for a, b in ((c1, c2), (c2, c1)):
        rc = L.lib().evs_cache_lookup_batch_c1c2(a._h, b._h, 4, rq.data_ptr(), out.data_ptr(), tier.data_ptr(), 2, st)
        assert rc == L.EVS_EINVAL and b"evlfu" in L.lib().evs_last_error() and b"fetch-first" in L.lib().evs_last_error()
    _serves(c1, tabs, g["n_rows"])
    assert c1.fetch_stats()["calls"] == 2
    _serves(c2, tabs, g["n_rows"])


@pytest.mark.parametrize("policy", POLICIES)
def test_order_0_over_pinned_tables_is_as_before(E, policy):
    """A cache that was not told otherwise: lru / lfu still refuse host-memory tables (EVS_ESTATE), evlfu still resolves to
    the sampled update there."""
    g = G2
    L = E._lib
    raws, tabs = _tables("G2", 32)
    c = _cache(E, policy, "G2", 32, [_pin(r) for r in raws])
    rq = _dev(np.zeros((4, 3), np.int32))
    if policy != "evlfu":
        _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_batch(rq))
        c = _cache(E, policy, "G2", 32, [_dev(r) for r in raws])
    _serves(c, tabs, g["n_rows"])
    assert c.fetch_stats() == {"calls": 0, "repointed": 0, "in_place": 0}
    if policy == "evlfu":
        _refused(E, L.EVS_ESTATE, None, lambda: c.set_batch_policy("setassoc"))      # (resolved at the first call: sampled)
        _refused(E, L.EVS_ESTATE, None, lambda: c.export_state())                    # (the warm start reads HBM tables)


def test_warm_start_of_an_order_1_cache(E):
    """Over HBM tables the warm start works as before; over host tables it keeps its EVS_ESTATE."""
    g = G2
    L = E._lib
    raws, tabs = _tables("G2", 32)
    dev = [_dev(r) for r in raws]
    c = _cache(E, "lru", "G2", 32, dev, order="fetch-first")
    _serves(c, tabs, g["n_rows"])
    state = c.export_state()
    c2 = _cache(E, "lru", "G2", 32, dev, order="fetch-first")
    c2.load_state(state)
    assert _dump(c2) == _dump(c)
    _refused(E, L.EVS_ESTATE, "lru", lambda: c2.set_miss_order("consume-first"))      # (a load is a batched call)
    _serves(c2, tabs, g["n_rows"])
    ch = _cache(E, "lru", "G2", 32, [_pin(r) for r in raws], order="fetch-first")
    _refused(E, L.EVS_ESTATE, None, lambda: ch.load_state(state))
    _serves(ch, tabs, g["n_rows"])
    _refused(E, L.EVS_ESTATE, None, lambda: ch.export_state())


def test_refusal_one_copy_arena_in_a_child():
    """EVS_SA_DUAL=0 is read once per process: an EvLFU cache then has one arena row per way and fetch-first refuses it, naming
    the switch; lru / lfu run over either arena (tests/_host_setassoc_env_child.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("EVS_SA_DUAL", "EVS_SA_WAYS", "EVS_CACHE_POLICY")}
    env["EVS_SA_DUAL"] = "0"
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_host_setassoc_env_child.py")], env=env, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
