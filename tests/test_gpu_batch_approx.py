"""The approximate-embedding mode of the batched set-associative EvLFU tier (evs_cache_set_batch_approx; the rule:
include/evstore_hip.h) against its restatement in Python (tests/_batch_approx_model.py): a sample whose agg_hit reaches the
threshold has every missed position served the row of its nearest earlier hit (the zero row when there is none), flagged 2, and
neither fetched nor inserted.  Directed cases from a hand-made state (loaded with the strict load_state), conflict-free streams
pinned flag for flag, bit for bit and way for way, lookup_interact against float64 over the served rows (tests/_accuracy.py),
twins (thres = T against the mode off; fetch-first over pinned tables against consume-first over HBM), a contended stream held to
the invariants, the setting toggled between calls and alternated with a bag call, and every refusal.

Two geometries (tests/_batch_approx_model.py: STREAMS): G26 -- 26 tables of 300 rows, d = 36, capacity 512, B = 40, thres = 20 --
and G4 -- 4 tables of 5 / 3000 / 70 / 400 rows, d = 16, capacity 64, B = 37, thres = 3; the contended stream runs B = 300 over
8 sets, the directed cases B = 6 and B = 1."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _accuracy as acc
import _bag_evlfu_model as EM
import _batch_approx_model as A
import _batched_policy_model as M

pytestmark = pytest.mark.gpu

ZERO = {"calls": 0, "samples": 0, "substituted": 0, "zero_rows": 0}


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
    g = A.STREAMS[geom]
    tabs = orc.kaggle_tables(list(g["n_rows"]), seed, g["d"])
    if codec == 32:
        return tabs, tabs
    raws = [orc.encode_table(np.clip(t * np.sqrt(len(t)), -1, 1), codec) for t in tabs]   # (spread over the codec's range: rows differ)
    return raws, [orc.decode(a, codec, g["d"]) for a in raws]


def _cache(E, geom, codec, backing, thres=None, order=None, inline=None, cap=None, policy="evlfu"):
    g = A.STREAMS[geom]
    c = E.GpuCache(policy, cap or g["cap"], g["T"], g["d"], codec)
    if order is not None:
        assert c.set_miss_order(order) is c
    if inline is not None:
        c.set_inline_update(inline)
    if thres is not None:
        assert c.set_batch_approx(thres) is c
    c.set_backing(backing)
    return c


def _dump(c):
    d = c.batch_dump()
    keys = [(int(t), int(r)) for _, t, r in d]
    assert len(set(keys)) == len(keys), "a key is resident twice"
    return {k: int(s) for k, (s, _, _) in zip(keys, d)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _base(stats):
    return {k: stats[k] for k in ("size", "n_evict", "n_requests", "n_perfect_hits", "n_hits", "hist")}


def _check_call(c, model, hit, out, flags, served, tabs, d, what):
    """one lookup_batch call against the model: flags, the served rows bit for bit, resident set, counters"""
    hit = hit.cpu().numpy()
    assert set(np.unique(hit)) <= {0, 1, 2}
    assert np.array_equal(hit, flags), "%s: %d flags differ from the model" % (what, int((hit != flags).sum()))
    if out is not None:
        want = A.served_rows(served, tabs, d)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), "%s: served rows" % what
    assert _dump(c) == model.resident(), "%s: resident set" % what
    assert _base(c.batch_stats()) == model.base_counters(), "%s: statistics" % what
    assert c.approx_stats() == model.approx_counters(), "%s: approx_stats" % what


# ------------------------------------------------------------------------------------------ 1. directed, from a hand-made state
def _rows_by_set(n_rows, nset, bits, t, s, skip=()):
    rows = np.arange(n_rows[t])
    return [int(r) for r in rows[M.set_of(t, rows, nset, list(n_rows), bits) == s] if int(r) not in skip]


@functools.lru_cache(maxsize=None)
def _directed():
    """G4, thres = 2.  Resident: table 0 row 0, one row of each other table, and eight rows of table 1 that fill set `full` at
    priorities 3, 1, 3, ... -- the way at 1 is what an insert into that set evicts.  Six samples:
      0  hits at tables 1 and 3: table 0 the zero row, table 2 the row of table 1
      1  one hit, below the threshold: three misses inserted at 1
      2  hits at tables 0 and 1: tables 2 and 3 both the row of table 1
      3  no hit: table 0's and table 2's keys, approximated by sample 0, are inserted here at 0; table 1's key goes into the
         full set and evicts
      4  an index out of range at table 0 inside an approximating sample: flag 0, a zero row, never approximated
      5  all four hit
    -> (the model holding the state, entries, state words, the request rows)"""
    g = A.STREAMS["G4"]
    n_rows, cap, T = list(g["n_rows"]), g["cap"], g["T"]
    m = A.BatchApproxModel(cap, n_rows)
    m.n = 9
    nset, bits = m.nset, m.bits
    set_of = lambda t, r: int(M.set_of(t, r, nset, n_rows, bits))
    full = (set_of(0, 0) + 1) % nset
    fill = _rows_by_set(n_rows, nset, bits, 1, full)[:9]
    assert len(fill) == 9
    for k, r in enumerate(fill[:8]):
        m.place((2, r), 1 if k == 1 else 3)
    used = {full}

    def pick(t, fresh_set, skip=()):
        """a row of table t that is not resident; fresh_set: its set holds no other key this call inserts"""
        for r in range(n_rows[t]):
            if (t + 1, r) in m.where or r in skip or (fresh_set and set_of(t, r) in used):
                continue
            if fresh_set:
                used.add(set_of(t, r))
            return r
        raise AssertionError("no row of table %d left" % t)

    a = [r for r in range(n_rows[1]) if set_of(1, r) != full][0]
    m.place((1, 0), 1), m.place((2, a), 1)
    b, r2 = pick(3, False), pick(2, False)
    m.place((4, b), 1), m.place((3, r2), 1)
    m0, m2 = pick(0, True), pick(2, True)                      # approximated by sample 0, inserted by sample 3
    s1 = [pick(0, True, (m0,)), a, pick(2, True, (m2,)), pick(3, True)]
    y3 = pick(3, True, (s1[3],))
    x1 = fill[8]                                               # into the full set
    m3x = pick(3, False, (s1[3], y3))
    rq = np.array([[m0, a, m2, b], s1, [0, a, m2, m3x], [m0, x1, m2, y3], [n_rows[0] + 2, a, m2, b], [0, a, r2, b]], np.int32)
    assert not A.insert_conflicts(m, rq, 2)
    entries = m.entries()
    S = M.stamp_bits_of("evlfu", cap, n_rows)[2]
    return m, entries, S, rq, (2, fill[1])


def _directed_state(codec):
    _m, entries, S, _rq, _victim = _directed()
    g = A.STREAMS["G4"]
    return {"entries": entries, "state": np.array([1, 0, g["cap"], g["T"], g["d"], codec, 9, 0, 0, 0, 0, 0, S, 0, -1, 0], np.int64),
            "n_rows": np.array(g["n_rows"], np.int64)}


def _fresh_directed_model():
    g = A.STREAMS["G4"]
    m0, entries, _S, rq, victim = _directed()
    m = A.BatchApproxModel(g["cap"], list(g["n_rows"]))
    m.n = 9
    for t1, row, score, _age, slot in entries.tolist():
        assert m.place((t1, row), score) == slot
    return m, rq, victim


@pytest.mark.parametrize("codec,order", [(32, None), (16, None), (8, None), (4, None), (32, "fetch-first"), (8, "fetch-first")])
def test_directed_from_a_hand_made_state(E, codec, order):
    g = A.STREAMS["G4"]
    d = g["d"]
    raws, tabs = _tables("G4", codec)
    model, rq, victim = _fresh_directed_model()
    c = _cache(E, "G4", codec, [_dev(r) for r in raws], thres=2, order=order, inline=False)
    got = c.load_state(_directed_state(codec))
    assert got["placed"] == len(model.where) and got["turned_away"] == 0
    assert _dump(c) == model.resident()
    flags, served = model.batch(rq, 2)
    assert flags.tolist() == [[2, 1, 2, 1], [0, 1, 0, 0], [1, 1, 2, 2], [0, 0, 0, 0], [0, 1, 2, 1], [1, 1, 1, 1]]
    assert served[0][0] is None and served[0][2] == served[0][1] and served[2][2] == served[2][3] == served[2][1]
    hit, out = c.lookup_batch(_dev(rq))
    _check_call(c, model, hit, out, flags, served, tabs, d, "directed")
    o = out.cpu().numpy()
    assert not _bits(o[0, 0]).any() and not _bits(o[4, 0]).any(), "the zero row is all +0.0f"
    res = _dump(c)
    assert (1, int(rq[0, 0])) in res and res[(1, int(rq[0, 0]))] == 0 and res[(3, int(rq[0, 2]))] == 0, "inserted once, at the missing sample's count"
    assert (4, int(rq[2, 3])) not in res, "a key that was only approximated is not resident"
    assert victim not in res and (2, int(rq[3, 1])) in res and c.batch_stats()["n_evict"] == 1
    assert c.approx_stats() == {"calls": 1, "samples": 3, "substituted": 4, "zero_rows": 1}
    assert c.batch_stats()["n_perfect_hits"] == 1 and c.batch_stats()["n_hits"] == 2 + 1 + 2 + 0 + 2 + 4
    if order:
        f = c.fetch_stats()
        assert f["calls"] == 1 and f["repointed"] + f["in_place"] == model.n_fetched == 7
    # the same rows again: what was inserted hits now, what was approximated is still missing
    flags, served = model.batch(rq, 2)
    assert flags[2].tolist() == [1, 1, 1, 2] and flags[3].tolist() == [1, 1, 1, 1]
    hit, out = c.lookup_batch(_dev(rq))
    _check_call(c, model, hit, out, flags, served, tabs, d, "directed, second call")


@pytest.mark.parametrize("thres,want", [(2, [2, 1, 2, 1]), (3, [0, 1, 0, 1])])
def test_one_sample(E, thres, want):
    """B = 1: one half-wave of one wave of one block, the other seven requests of the block off"""
    g = A.STREAMS["G4"]
    raws, tabs = _tables("G4", 32)
    model, rq, _victim = _fresh_directed_model()
    c = _cache(E, "G4", 32, [_dev(r) for r in raws], thres=thres)
    c.load_state(_directed_state(32))
    flags, served = model.batch(rq[:1], thres)
    assert flags.tolist() == [want]
    hit, out = c.lookup_batch(_dev(rq[:1]))
    _check_call(c, model, hit, out, flags, served, tabs, g["d"], "B = 1")


# --------------------------------------------------------------------------------------------------- 2. conflict-free streams
@pytest.mark.parametrize("geom,codec,order", [("G26", 32, None), ("G26", 8, "fetch-first"), ("G26", 4, None), ("G4", 32, "fetch-first"),
                                              ("G4", 16, None), ("G4", 8, None)])
def test_conflict_free_stream(E, geom, codec, order):
    """No call brings two inserted keys to one set and no flush fires (tests/test_batch_approx_model.py checks the streams'
    cover), so the rule is deterministic: flags, the served rows' bits, {key: priority}, the histogram, batch_stats and
    approx_stats equal the model's after every call.  Fetch-first caches stand over pinned tables: every position the model
    counts as a miss is re-pointed or served in place, and no other -- approximated rows never cross the bus."""
    g = A.STREAMS[geom]
    raws, tabs = _tables(geom, codec)
    rows, want_flags, want_served, _final, _top = A.stream(geom)
    backing = [_pin(r) for r in raws] if order else [_dev(r) for r in raws]
    c = _cache(E, geom, codec, backing, thres=g["thres"], order=order)
    model = A.BatchApproxModel(g["cap"], list(g["n_rows"]))
    for i in range(g["n_batches"]):
        flags, served = model.batch(rows[i], g["thres"])
        assert np.array_equal(flags, want_flags[i]) and served == want_served[i]
        hit, out = c.lookup_batch(_dev(rows[i]))
        _check_call(c, model, hit, out, flags, served, tabs, g["d"], "call %d" % (i + 1))
        if order:
            f = c.fetch_stats()
            assert f["calls"] == i + 1 and f["repointed"] + f["in_place"] == model.n_fetched, "call %d: fetched positions" % (i + 1)
            assert f["in_place"] == 0
    s = c.batch_stats()
    assert s["n_flush"] == 0 and s["n_evict"] > 0 and s["n_hits"] > 0
    a = c.approx_stats()
    assert a["samples"] > 0 and a["substituted"] > 0 and a["zero_rows"] > 0


# -------------------------------------------------------------------------------------------------------- 3. lookup_interact
@pytest.mark.parametrize("geom,codec", [("G26", 32), ("G4", 32), ("G26", 8), ("G26", 4)])
def test_lookup_interact(E, geom, codec):
    """The same flags and state through lookup_interact; R against interact_features in float64 over the rows the MODEL says
    are served (a zero row gives exact zeros), itself on and off."""
    g = A.STREAMS[geom]
    B, T, d = g["B"], g["T"], g["d"]
    raws, tabs = _tables(geom, codec)
    rows = A.stream(geom)[0]
    c = _cache(E, geom, codec, [_dev(r) for r in raws], thres=g["thres"])
    model = A.BatchApproxModel(g["cap"], list(g["n_rows"]))
    rs = np.random.RandomState(17)
    for i in range(6):
        flags, served = model.batch(rows[i], g["thres"])
        x = rs.uniform(-1, 1, (B, d)).astype(np.float32)
        hit, R = c.lookup_interact(_dev(rows[i]), _dev(x), itself=bool(i & 1))
        _check_call(c, model, hit, None, flags, served, tabs, d, "call %d" % (i + 1))
        feats = A.served_rows(served, tabs, d).astype(np.float64)
        ref = acc.Reference(x, [(feats[:, t], np.abs(feats[:, t])) for t in range(T)], bool(i & 1))
        acc.check(R.cpu().numpy(), ref, "%s codec %d call %d" % (geom, codec, i + 1), "approximating probe + pointer-table interaction, codec %d" % codec)
    assert c.approx_stats()["zero_rows"] > 0 and c.approx_stats()["substituted"] > 0


# ------------------------------------------------------------------------------------------------------------------ 4. twins
@pytest.mark.parametrize("geom,codec,form", [("G26", 32, "batch"), ("G4", 8, "batch"), ("G26", 32, "interact")])
def test_thres_T_is_the_mode_off(E, geom, codec, form):
    """A sample at thres = T has no miss: the new probe approximates nothing, and flags, outputs, dump, counters and the exported
    entries are those of the parent's chain (the mode off, set_inline_update(False)), byte for byte."""
    g = A.STREAMS[geom]
    B, T, d = g["B"], g["T"], g["d"]
    raws, _tabs = _tables(geom, codec)
    dev = [_dev(r) for r in raws]
    rows = EM.conflict_free_rows_stream(g["cap"], list(g["n_rows"]), B, 8, g["seed"])[0]
    on = _cache(E, geom, codec, dev, thres=T, inline=False)
    off = _cache(E, geom, codec, dev, thres=0, inline=False)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    for i in range(8):
        r = _dev(rows[i])
        if form == "batch":
            res = [c.lookup_batch(r) for c in (on, off)]
        else:
            x = torch.empty(B, d, device="cuda").uniform_(-1, 1, generator=gen)
            res = [c.lookup_interact(r, x) for c in (on, off)]
        assert torch.equal(res[0][0], res[1][0]) and int(res[0][0].max()) <= 1, "call %d: flags" % (i + 1)
        assert np.array_equal(_bits(res[0][1].cpu().numpy()), _bits(res[1][1].cpu().numpy())), "call %d: outputs" % (i + 1)
        assert _dump(on) == _dump(off) and on.batch_stats() == off.batch_stats(), "call %d" % (i + 1)
        so, sf = on.export_state(), off.export_state()
        assert np.array_equal(so["entries"], sf["entries"]) and np.array_equal(so["state"], sf["state"]), "call %d: exported state" % (i + 1)
    assert on.approx_stats() == {"calls": 8, "samples": 0, "substituted": 0, "zero_rows": 0} and off.approx_stats() == ZERO
    assert on.batch_stats()["n_hits"] > 0


@pytest.mark.parametrize("geom,codec", [("G26", 32), ("G4", 4)])
def test_fetch_first_over_pinned_tables_equals_consume_first_over_hbm(E, geom, codec):
    g = A.STREAMS[geom]
    raws, _tabs = _tables(geom, codec)
    rows = A.stream(geom)[0]
    a = _cache(E, geom, codec, [_dev(r) for r in raws], thres=g["thres"])
    b = _cache(E, geom, codec, [_pin(r) for r in raws], thres=g["thres"], order="fetch-first")
    model = A.BatchApproxModel(g["cap"], list(g["n_rows"]))
    for i in range(g["n_batches"]):
        model.batch(rows[i], g["thres"])
        r = _dev(rows[i])
        (ha, oa), (hb, ob) = a.lookup_batch(r), b.lookup_batch(r)
        assert torch.equal(ha, hb), "call %d: flags" % (i + 1)
        assert np.array_equal(_bits(oa.cpu().numpy()), _bits(ob.cpu().numpy())), "call %d: outputs" % (i + 1)
        assert _dump(a) == _dump(b) == model.resident() and a.batch_stats() == b.batch_stats() and a.approx_stats() == b.approx_stats()
        f = b.fetch_stats()
        assert f["repointed"] + f["in_place"] == model.n_fetched, "call %d: an approximated row was fetched (or a miss was not)" % (i + 1)
    assert a.fetch_stats() == {"calls": 0, "repointed": 0, "in_place": 0}


# ------------------------------------------------------------------------------------------------------- 5. contended stream
@pytest.mark.parametrize("order", [None, "fetch-first"])
def test_contended_stream_holds_the_invariants(E, order):
    """B = 300 over 8 sets (capacity 64), rows drawn from the first 20 of every table (about a third
    of the samples reach the threshold): most calls bring several new keys to a set,
    so which of them wins a way is a matter of timing.  The invariants: flag 1 = resident in the dump taken before the call and
    the table's row; flag 2 only in a sample at the threshold, on a key that was not resident, its output the row of the nearest
    earlier flag-1 position of its sample or zero; flag 0 the table's row; no key twice; size <= capacity."""
    g = A.STREAMS["G26"]
    T, d, B, cap, thres = g["T"], g["d"], 300, 64, 4
    raws, tabs = _tables("G26", 32)
    c = _cache(E, "G26", 32, [_pin(r) for r in raws] if order else [_dev(r) for r in raws], thres=thres, order=order, cap=cap)
    rs = np.random.RandomState(9)
    n2 = 0
    a0 = c.approx_stats()
    for i in range(8):
        rq = rs.randint(0, 20, (B, T)).astype(np.int32)
        before = _dump(c) if i else {}
        hit, out = c.lookup_batch(_dev(rq))
        hit, out = hit.cpu().numpy(), out.cpu().numpy()
        was = np.array([[(t + 1, int(rq[b, t])) in before for t in range(T)] for b in range(B)])
        assert np.array_equal(hit == 1, was), "call %d: flag 1 is not residency at arrival" % (i + 1)
        agg = was.sum(1)
        assert np.array_equal(hit == 2, ~was & (agg >= thres)[:, None]), "call %d: flag 2" % (i + 1)
        want = np.zeros((B, T, d), np.float32)
        for b in range(B):
            prev = None
            for t in range(T):
                if hit[b, t] == 2:
                    if prev is not None:
                        want[b, t] = tabs[prev][rq[b, prev]]
                else:
                    want[b, t] = tabs[t][rq[b, t]]
                    if hit[b, t] == 1:
                        prev = t
        assert np.array_equal(_bits(out), _bits(want)), "call %d: served rows" % (i + 1)
        assert len(_dump(c)) == c.batch_stats()["size"] <= cap
        a1 = c.approx_stats()
        two = hit == 2
        first_hit = np.where(was.any(1), was.argmax(1), T)
        zero = two & (np.arange(T)[None, :] < first_hit[:, None])
        assert (a1["samples"] - a0["samples"], a1["substituted"] - a0["substituted"], a1["zero_rows"] - a0["zero_rows"]) == (
            int(two.any(1).sum()), int((two & ~zero).sum()), int(zero.sum())), "call %d: approx_stats" % (i + 1)
        a0 = a1
        n2 += int(two.sum())
    assert n2 > 0 and c.batch_stats()["n_evict"] > 0


# ------------------------------------------------------------------------------ 6. toggled between calls, alternated with bags
def test_setting_toggled_and_alternated_with_a_bag_call(E):
    """One cache, one model: threshold on, off, a lookup_bags call (one index per bag; the bag forms ignore the setting, so its
    flags are residency and nothing is approximated), on at another value, ...  The batch number and the counters are shared."""
    g = A.STREAMS["G26"]
    T, d = g["T"], g["d"]
    raws, tabs = _tables("G26", 32)
    rows = A.toggle_stream()[0]
    c = _cache(E, "G26", 32, [_dev(r) for r in raws], inline=False).set_bag_rule("served-bags")
    model = A.BatchApproxModel(g["cap"], list(g["n_rows"]))
    for i, what in enumerate(A.TOGGLE_PLAN):
        rq = rows[i]
        if what != "bags":
            c.set_batch_approx(what)
            flags, served = model.batch(rq, what)
            hit, out = c.lookup_batch(_dev(rq))
            _check_call(c, model, hit, out, flags, served, tabs, d, "call %d (threshold %s)" % (i + 1, what))
            continue
        c.set_batch_approx(20)                                 # in force, and ignored
        off, idx = EM.one_per_bag(rq)
        want = np.stack(model.batch_bags(off, idx), 1)
        hits, ly = c.lookup_bags([_dev(o) for o in off], [_dev(ix) for ix in idx])
        got = torch.stack(hits, 1).cpu().numpy()
        assert np.array_equal(got, want.astype(np.uint8)), "call %d: bag flags" % (i + 1)
        pooled = torch.stack(ly, 1).cpu().numpy()
        for t in range(T):
            assert np.array_equal(_bits(pooled[:, t]), _bits(tabs[t][rq[:, t]])), "call %d: a bag call approximated" % (i + 1)
        assert _dump(c) == model.resident() and _base(c.batch_stats()) == model.base_counters(), "call %d" % (i + 1)
        assert c.approx_stats() == model.approx_counters(), "call %d: a bag call moved approx_stats" % (i + 1)
    a = c.approx_stats()
    assert a["calls"] == 4 and a["substituted"] > 0 and a["zero_rows"] > 0


# --------------------------------------------------------------------------------------------------------------- 7. refusals
def _refused(E, code, policy, fn):
    with pytest.raises(E._lib.EvsError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    assert policy is None or policy in str(ei.value), str(ei.value)
    return str(ei.value)


def _serves(c, geom="G4", seed=8, B=5):
    """two calls with a threshold that approximates nothing, the second the first again: rows exact, then all hits"""
    g = A.STREAMS[geom]
    _raws, tabs = _tables(geom, 32)
    rs = np.random.RandomState(seed)
    rq = np.stack([rs.randint(0, n, B) for n in g["n_rows"]], 1).astype(np.int32)
    for i in range(2):
        hit, out = c.lookup_batch(_dev(rq))
        o = out.cpu().numpy()
        for t in range(g["T"]):
            assert np.array_equal(_bits(o[:, t]), _bits(tabs[t][rq[:, t]]))
    assert bool((hit == 1).all())


def test_refusals_of_the_setter(E):
    L = E._lib
    g = A.STREAMS["G4"]
    raws, _tabs = _tables("G4", 32)
    dev = [_dev(r) for r in raws]
    c = _cache(E, "G4", 32, dev)
    msg = _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.set_batch_approx(g["T"] + 1))
    assert "4 tables" in msg
    assert L.lib().evs_cache_approx_stats(c._h, None, None) == L.EVS_EINVAL and b"NULL out4" in L.lib().evs_last_error()
    assert c.approx_stats() == ZERO
    for thres in (g["T"], 1, 0, -3, None):
        assert c.set_batch_approx(thres) is c
    c.set_batch_approx(g["T"])
    _serves(c)
    assert c.approx_stats() == {"calls": 2, "samples": 0, "substituted": 0, "zero_rows": 0}
    for policy in ("lru", "lfu"):
        p = _cache(E, "G4", 32, dev, policy=policy)
        msg = _refused(E, L.EVS_EINVAL, policy, lambda: p.set_batch_approx(1))
        assert "evlfu" in msg
        assert p.set_batch_approx(0) is p and p.set_batch_approx(-1) is p
        _serves(p)
        assert p.approx_stats() == ZERO
    # a row larger than the zero row of its codec: 4 KiB of fp32 zeros, 1 KiB of zero codes
    wide = E.GpuCache("evlfu", 64, 2, 1100, 32)
    msg = _refused(E, L.EVS_EINVAL, "evlfu", lambda: wide.set_batch_approx(1))
    assert "4400" in msg and "4096" in msg
    assert wide.set_batch_approx(0) is wide


def test_refusal_plan_and_sampled(E):
    L = E._lib
    raws, _tabs = _tables("G4", 32)
    for name in ("sampled", "plan"):
        c = _cache(E, "G4", 32, [_dev(r) for r in raws], thres=2)
        c.set_batch_policy(name)
        rq = _dev(np.zeros((4, 4), np.int32))
        assert name in _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_batch(rq))
        x = torch.zeros(4, 16, device="cuda")
        assert name in _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_interact(rq, x))
        assert c.approx_stats() == ZERO
        c.set_batch_policy("setassoc")                         # (nothing was allocated: the policy may still be given)
        _serves(c.set_batch_approx(4))
        assert c.approx_stats()["calls"] == 2
    # consume-first over pinned tables resolves to the sampled update: refused, and served once the threshold is off
    c = _cache(E, "G4", 32, [_pin(r) for r in raws], thres=2)
    rq = _dev(np.zeros((4, 4), np.int32))
    assert "sampled" in _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_batch(rq))
    _serves(c.set_batch_approx(0))
    assert c.approx_stats() == ZERO


def test_refusal_file_tier(E, tmp_path):
    L = E._lib
    g = A.STREAMS["G4"]
    raws, tabs = _tables("G4", 32)
    paths = []
    for k, t in enumerate(tabs):
        p = tmp_path / ("ev-table-%d.bin" % (k + 1))
        t.tofile(p)
        paths.append(str(p))
    ft = E.FileTier(paths, g["d"] * 4, 1 << 30)
    c = E.GpuCache("evlfu", g["cap"], g["T"], g["d"], 32).set_batch_approx(2)
    c.set_file_backing(ft)
    rq = _dev(np.zeros((4, 4), np.int32))
    _refused(E, L.EVS_ESTATE, "evlfu", lambda: c.lookup_batch(rq))
    assert c.approx_stats() == ZERO
    c.set_batch_approx(0)
    hit, out = c.lookup_batch(rq)                              # the file tier's own chain, as before
    assert np.array_equal(_bits(out.cpu().numpy()[0, 1]), _bits(tabs[1][0]))


def test_refusal_pair_member(E):
    """a cache with a threshold on as a member of a C1 + C2 lookup or of a pair bag call; alone it serves"""
    L = E._lib
    g = A.STREAMS["G4"]
    raws, _tabs = _tables("G4", 32)
    dev = [_dev(r) for r in raws]
    c1 = _cache(E, "G4", 32, dev, thres=2).set_bag_rule("served-bags")
    c2 = _cache(E, "G4", 32, dev).set_bag_rule("served-bags")
    rq = _dev(np.zeros((4, 4), np.int32))
    for a, b in ((c1, c2), (c2, c1)):
        msg = _refused(E, L.EVS_EINVAL, "evlfu", lambda: E.lookup_batch_c1c2(a, b, rq, threshold=2))
        assert "evs_cache_set_batch_approx" in msg and ("C1" if a is c1 else "C2") in msg
        off = [_dev(np.arange(4, dtype=np.int64))] * 4
        idx = [_dev(np.zeros(4, np.int64))] * 4
        msg = _refused(E, L.EVS_EINVAL, "evlfu", lambda: E.lookup_bags_c1c2(a, b, off, idx, threshold=2))
        assert "evs_cache_set_batch_approx" in msg
    _serves(c1.set_batch_approx(4))
    assert c1.approx_stats()["calls"] == 2
    _serves(c2)


def test_refusal_16_way_sets_in_a_child():
    """EVS_SA_WAYS=16 is read once per process (tests/_batch_approx_env_child.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("EVS_SA_DUAL", "EVS_SA_WAYS", "EVS_CACHE_POLICY")}
    env["EVS_SA_WAYS"] = "16"
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_batch_approx_env_child.py")], env=env, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_inline_update_is_not_refused_and_not_taken(E):
    """set_inline_update(True) with a threshold on: the call runs the unfolded chain (strict snapshot flags, the model's), and
    with the threshold off again the cache goes back to its one-launch form"""
    g = A.STREAMS["G26"]
    raws, tabs = _tables("G26", 32)
    rows = A.stream("G26")[0]
    c = _cache(E, "G26", 32, [_dev(r) for r in raws], thres=g["thres"], inline=True)
    model = A.BatchApproxModel(g["cap"], list(g["n_rows"]))
    rs = np.random.RandomState(3)
    for i in range(4):
        flags, served = model.batch(rows[i], g["thres"])
        x = _dev(rs.uniform(-1, 1, (g["B"], g["d"])).astype(np.float32))
        hit, _R = c.lookup_interact(_dev(rows[i]), x)
        _check_call(c, model, hit, None, flags, served, tabs, g["d"], "call %d" % (i + 1))
    c.set_batch_approx(0)
    hit, _R = c.lookup_interact(_dev(rows[4]), x)
    assert int(hit.max()) <= 1 and c.approx_stats()["calls"] == 4
