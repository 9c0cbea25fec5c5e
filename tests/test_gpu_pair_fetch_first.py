"""The C1 + C2 pair in fetch-first order (both tiers set_miss_order('fetch-first'): flush -> probe -> the pair's update ->
sa_repoint2 -> consumers -> close; include/evstore_hip.h at evs_cache_lookup_batch_c1c2) over tables in HBM and in pinned host
memory.  On conflict-free streams three pairs -- order 0 over HBM, order 1 over HBM, order 1 over pinned tables -- see the same
calls and must agree after every one of them; a hit whose way the call's own update takes, a key routed both ways and a key
turned away are built by hand and held to tests/_pair_fetch_model.py; contended streams are held to the invariants; every point
of the envelope is refused with the pair left usable."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _accuracy as A
import _bag_pair_model as BP
import _pair_fetch_model as F
import _pair_warm_model as P

pytestmark = pytest.mark.gpu

SHAPES = {"T3": [200, 1000, 4000], "T5": [200, 700, 1000, 2500, 4000]}
# (tables, d, codecs, capacities): 8 + 2 x 8 ways with the merged (36, 18)-byte update; the general mixed consumer with two update
# launches (64 / 16-byte rows); 6 + 2 x 8 ways -- the re-point kernel's general form; the (144, 36)-byte merged update
CASES = [("T3", 36, (8, 4), (64, 128)), ("T5", 16, (32, 8), (64, 128)), ("T3", 16, (8, 4), (36, 96)), ("T5", 36, (32, 8), (64, 128))]
# the calls of the twin streams: (B, new keys at most, "the resident picks walk every resident key"); the three covering calls in a
# row leave at most one way of a tier below priority T, which is what the flush waits for (95 % of the capacity)
B_CYCLE = [(1, 8, 0), (1, 1, 0), (7, 7, 0), (7, 7, 0), (64, 8, 0), (300, 8, 0), (7, 7, 0), (64, 8, 0), (300, 8, 0), (1, 1, 0), (64, 8, 0),
           (300, 8, 0), (7, 7, 0), (300, 8, 0), (300, 1, 1), (300, 1, 1), (300, 1, 1), (7, 7, 0), (64, 8, 0), (300, 8, 0), (1, 1, 0)]


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _new_tables(shape, codec, d, seed=0):
    g = torch.Generator(device="cuda")
    g.manual_seed(100 * len(SHAPES[shape]) + codec + d + seed)
    if codec == 32:
        return [torch.empty(n, d, device="cuda").uniform_(-1, 1, generator=g) for n in SHAPES[shape]]
    if codec == 4:   # (code 15 is not a value of the 4-bit codec -- it decodes to NaN --: nibbles 0 .. 14)
        return [(torch.randint(0, 15, (n, d // 2), device="cuda", generator=g) * 16 + torch.randint(0, 15, (n, d // 2), device="cuda", generator=g)).to(torch.uint8)
                for n in SHAPES[shape]]
    return [torch.randint(0, 256, (n, d * codec // 8), dtype=torch.uint8, device="cuda", generator=g) for n in SHAPES[shape]]


_made, _dec = {}, {}


def _tables(shape, codec, d):
    """tables in a tier's codec, shared by the tests that do not write them"""
    if (shape, codec, d) not in _made:
        _made[(shape, codec, d)] = _new_tables(shape, codec, d)
    return _made[(shape, codec, d)]


def _decode(E, tables, shape, codec, d):
    """the fp32 rows a tier of `codec` serves from `tables` (device or pinned), per table (numpy): read through the miss path of a
    fresh cache over device copies, once"""
    n_rows = SHAPES[shape]
    dev = [t if t.is_cuda else t.cuda() for t in tables]
    if codec == 32:
        return [t.cpu().numpy().copy() for t in dev]
    c = E.GpuCache("lru", 64, len(n_rows), d, codec, "python")
    c.set_backing(dev)
    rq = np.stack([np.minimum(np.arange(max(n_rows)), r - 1) for r in n_rows], 1).astype(np.int32)
    _h, out = c.lookup_batch(_dev(rq))
    out = out.cpu().numpy()
    return [out[:n_rows[t], t].copy() for t in range(len(n_rows))]


def _dec_shared(E, shape, codec, d):
    if (shape, codec, d) not in _dec:
        _dec[(shape, codec, d)] = _decode(E, _tables(shape, codec, d), shape, codec, d)
    return _dec[(shape, codec, d)]


def _pin(tables):
    return [t.cpu().pin_memory() for t in tables]


def _pair(E, shape, d, codecs, caps, order, pinned=(False, False), tables=None):
    """order: 0 | 1 for both tiers, or a pair of them"""
    T = len(SHAPES[shape])
    order = (order, order) if isinstance(order, int) else order
    cs = []
    for k in (0, 1):
        c = E.GpuCache("evlfu", caps[k], T, d, codecs[k], "cpp")
        if order[k]:
            assert c.set_miss_order("fetch-first") is c
        tab = tables[k] if tables else _tables(shape, codecs[k], d)
        c._tables_kept = _pin(tab) if pinned[k] else tab
        c.set_backing(c._tables_kept)
        cs.append(c)
    return tuple(cs)


def _twins(E, shape, d, codecs, caps):
    """order 0 over HBM, order 1 over HBM, order 1 over pinned tables"""
    return [_pair(E, shape, d, codecs, caps, 0), _pair(E, shape, d, codecs, caps, 1), _pair(E, shape, d, codecs, caps, 1, (True, True))]


def _dump(c):
    d = c.batch_dump()
    out = {(int(t), int(r)): int(s) for s, t, r in d}
    assert len(out) == len(d), "a key is resident twice in one tier"
    return out


def _same_export(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("entries", "state", "n_rows1", "n_rows2"))


def _expected(geom, in1, in2, rq, thr):
    """tier code and serve byte per position against the snapshot (the dumps): 1 / 2 = resident there; a double miss goes to C1
    while the key's own C1 set has a free way, else by the reference's rule (agg_hit below the threshold: odd table index -> C1,
    even -> C2; else C2); an index out of range: 0 / 0"""
    B, T = rq.shape
    occ = np.zeros(geom.nset, np.int64)
    for (t1, r) in in1:
        occ[geom.place(1, t1 - 1, r)[0]] += 1
    lim = [min(a, b) for a, b in zip(*geom.n_rows)]
    code, serve = np.zeros(rq.shape, np.uint8), np.zeros(rq.shape, np.uint8)
    for b in range(B):
        for t in range(T):
            key = (t + 1, int(rq[b, t]))
            if 0 <= rq[b, t] < lim[t]:
                code[b, t] = 1 if key in in1 else (2 if key in in2 else 0)
        agg = int((code[b] > 0).sum())
        for t in range(T):
            if code[b, t] or not 0 <= rq[b, t] < lim[t]:
                serve[b, t] = code[b, t]
            elif occ[geom.place(1, t, int(rq[b, t]))[0]] < geom.tiers[0].ways:
                serve[b, t] = 1
            else:
                serve[b, t] = (1 if t % 2 == 1 else 2) if agg < thr else 2
    return code, serve


def _quiet_call(rs, geom, resident, used, B, n_new, cover=False):
    """One (B, T) call whose outcome does not depend on timing: at most min(B, nset, n_new) new keys (never named before), each
    named by ONE position, in different set records and different samples; every other position names a resident key (cover:
    sample b the b-th of its table, round and round, so that every resident key is named).  From empty: B = 1, every position a new
    key."""
    T = geom.T
    lim = [min(a, b) for a, b in zip(*geom.n_rows)]
    by_table = [sorted(r for (t1, r) in resident if t1 == t + 1) for t in range(T)]
    if all(by_table):
        if cover:
            rq = np.stack([np.array(by_table[t])[np.arange(B) % len(by_table[t])] for t in range(T)], 1).astype(np.int32)
        else:
            rq = np.stack([rs.choice(by_table[t], B) for t in range(T)], 1).astype(np.int32)
        where = [(int(b), int(rs.randint(T))) for b in rs.permutation(B)[:min(B, geom.nset, n_new)]]
    else:
        assert B == 1 and T <= geom.nset
        rq = np.zeros((1, T), np.int32)
        where = [(0, t) for t in range(T)]
    recs = set()
    for b, t in where:
        for _try in range(100000):
            r = int(rs.randint(lim[t]))
            if (t + 1, r) not in used and geom.record(t, r) not in recs:
                break
        else:
            raise AssertionError("table %d has run out of new keys" % t)
        recs.add(geom.record(t, r))
        used.add((t + 1, r))
        rq[b, t] = r
    return rq


def _reference(x, rows):
    """rows (B, T, d) fp32 as served -> the fp64 reference of R"""
    return A.Reference(x, [A.pool64(rows[:, t])[:2] for t in range(rows.shape[1])], False)


# ------------------------------------------------------------------------------------------- 1. twins on conflict-free streams
@pytest.mark.parametrize("form", ["batch", "interact"])
@pytest.mark.parametrize("shape,d,codecs,caps", CASES)
def test_twins_on_conflict_free_streams(E, shape, d, codecs, caps, form):
    """The same calls from empty on the three pairs, B cycling over 1, 7, 64 and 300.  After every call: the tier codes are the
    snapshot's (the dumps taken before it), the rows are the serving tier's decode of its table row bit for bit -- on all three --,
    and both tiers' dumps and counters are equal.  Samples without a new key are served everywhere, so priorities reach T and the
    stream crosses EvLFU flushes (one block scans a tier this small: which ways go does not depend on timing).  interact: R is
    bit-equal between the two order-1 pairs (one consumer kernel over equal pointer tables' bytes) and held against fp64 on all
    three; order 0 runs the folded probe for 8 + 8 ways, which is another summation order."""
    n_rows = SHAPES[shape]
    T = len(n_rows)
    geom = P.Geometry(caps[0], caps[1], n_rows)
    thr = T                                              # a sample with a miss has agg_hit < T: odd tables -> C1, even -> C2
    dec1, dec2 = _dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d)
    pairs = _twins(E, shape, d, codecs, caps)
    rs = np.random.RandomState(caps[0] + T + d)
    used, in1, in2 = set(), {}, {}
    kernel = "interact_mixed84_kernel" if codecs == (8, 4) else "interact_mixed_rows_kernel"
    for i, (B, n_new, cover) in enumerate(B_CYCLE):
        rq = _quiet_call(rs, geom, set(in1) | set(in2), used, B, n_new, bool(cover))
        code, serve = _expected(geom, in1, in2, rq, thr)
        rows = F.expected_rows(serve, rq, dec1, dec2)
        x = rs.uniform(-1, 1, (B, d)).astype(np.float32)
        got_R = []
        for k, (c1, c2) in enumerate(pairs):
            if form == "batch":
                tier, out = E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=thr)
                assert np.array_equal(_bits(out.cpu().numpy()), _bits(rows)), "call %d pair %d: rows" % (i, k)
            else:
                tier, R = E.lookup_interact_c1c2(c1, c2, _dev(rq), _dev(x), threshold=thr)
                got_R.append(R.cpu().numpy())
                A.check(got_R[-1], _reference(x, rows), "call %d pair %d %s" % (i, k, shape), kernel)
            assert np.array_equal(tier.cpu().numpy(), code), "call %d pair %d: tier codes" % (i, k)
        if form == "interact":
            assert np.array_equal(_bits(got_R[1]), _bits(got_R[2])), "call %d: R of the two order-1 pairs" % i
        dumps = [(_dump(c1), _dump(c2)) for c1, c2 in pairs]
        stats = [(c1.batch_stats(), c2.batch_stats()) for c1, c2 in pairs]
        assert dumps[0] == dumps[1] == dumps[2], "call %d: dumps" % i
        assert stats[0] == stats[1] == stats[2], "call %d: counters" % i
        assert "hist" in stats[0][0] and not set(dumps[0][0]) & set(dumps[0][1])
        in1, in2 = dumps[0]
    assert stats[0][0]["n_flush"] >= 1, "the stream never crossed a flush"
    print("twins %s %s: C1 %s, C2 %s, re-point %s" % (shape, form, stats[1][0], stats[1][1], pairs[1][0].fetch_stats()))
    assert stats[0][0]["n_evict"] + stats[0][1]["size"] > 0, "C1 never filled a set"
    assert _same_export(E.export_state_c1c2(*pairs[0]), E.export_state_c1c2(*pairs[1]))
    f0, f1, f2 = (p[0].fetch_stats() for p in pairs)
    assert f0 == {"calls": 0, "repointed": 0, "in_place": 0}
    assert f1 == f2 and f1["calls"] == len(B_CYCLE) and f1["in_place"] == 0 and f1["repointed"] > 0
    assert pairs[1][1].fetch_stats() == {"calls": 0, "repointed": 0, "in_place": 0}      # (C2's own counters are not used)


# ------------------------------------------------------------------------------------------- 2. a hit whose way the update takes
def _rows_of_set(geom, tier, es, table0, count, skip=()):
    lim = min(geom.n_rows[0][table0], geom.n_rows[1][table0])
    out = [r for r in range(lim) if geom.place(tier, table0, r)[0] == es and (table0 + 1, r) not in skip]
    assert len(out) >= count
    return out[:count]


def _fresh_rows(geom, used_records, table0, count):
    out = []
    for r in range(min(geom.n_rows[0][table0], geom.n_rows[1][table0])):
        if geom.record(table0, r) not in used_records:
            used_records.add(geom.record(table0, r))
            out.append(r)
            if len(out) == count:
                return out
    raise AssertionError("too few records")


def _victim_case(geom):
    """C1 set 0: eight keys of table 2 (index 1), the first with the lowest priority; the judged call hits it from a sample with
    agg_hit 1 and brings a ninth key of the set from a sample with agg_hit 0 -> (the eight rows, the newcomer, the call)"""
    rows = _rows_of_set(geom, 1, 0, 1, 9)
    used = {0}
    a, b = _fresh_rows(geom, used, 0, 3), _fresh_rows(geom, used, 2, 3)
    rq = np.array([[a[1], rows[0], b[1]], [a[2], rows[8], b[2]]], np.int32)
    return rows[:8], rows[8], (a[0], b[0]), rq


def _check_victim_call(E, pair, rq, dec1, victim_hits_min):
    f0 = pair[0].fetch_stats()
    tier, out = E.lookup_batch_c1c2(pair[0], pair[1], _dev(rq), threshold=2)
    tier, out = tier.cpu().numpy(), out.cpu().numpy()
    assert tier.tolist() == [[0, 1, 0], [0, 0, 0]]
    assert np.array_equal(_bits(out), _bits(F.expected_rows(np.ones((2, 3), np.uint8), rq, dec1, dec1)))
    assert not np.array_equal(_bits(out[0, 1]), _bits(out[1, 1])), "the hit position got the newcomer's row"
    f1 = pair[0].fetch_stats()
    if getattr(pair[0], "_fetch_first", False):
        assert f1["victim_hits"] - f0.get("victim_hits", 0) >= victim_hits_min and f1["repointed"] - f0["repointed"] == 5
        assert f1["in_place"] == f0["in_place"]
    d1 = _dump(pair[0])
    assert (2, int(rq[1, 1])) in d1 and (2, int(rq[0, 1])) not in d1, "the newcomer did not take the hit key's way"


def test_a_hit_whose_way_the_update_takes(E):
    """A hand-made state (non-strict load) on an order-1 and an order-0 pair over HBM: C1 set 0 full, one way with the lowest
    priority.  The call hits that key (agg_hit 1: still the lowest) and routes a new key of the set to C1: the way goes to the
    newcomer inside the call, BEFORE the consumers of the order-1 pair run -- the hit position must still get its own key's C1
    table row.  The pinned pair cannot be loaded: it gets to the same set by scripted calls -- one sample each, the key of the set
    between two resident keys (agg_hit 2), the first of them alone among misses (agg_hit 0) -- and is held to the same bytes."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    geom = P.Geometry(caps[0], caps[1], SHAPES[shape])
    dec1 = _dec_shared(E, shape, codecs[0], d)
    rows, _newcomer, (a0, b0), rq = _victim_case(geom)
    entries = np.array([[1, 2, r, 0 if j == 0 else 2, 0, 0] for j, r in enumerate(rows)], np.int64)
    loaded = [_pair(E, shape, d, codecs, caps, 0), _pair(E, shape, d, codecs, caps, 1)]
    for pair in loaded:
        info = E.load_state_c1c2(pair[0], pair[1], {"entries": entries, "state": None}, strict=False)
        assert info["placed"] == (8, 0)
        _check_victim_call(E, pair, rq, dec1, 1)
    assert _same_export(E.export_state_c1c2(*loaded[0]), E.export_state_c1c2(*loaded[1]))
    assert loaded[1][0].fetch_stats()["victim_hits"] == 1
    scripted = [_pair(E, shape, d, codecs, caps, 0), _pair(E, shape, d, codecs, caps, 1, (True, True))]
    for pair in scripted:
        for r in rows:
            E.lookup_batch_c1c2(pair[0], pair[1], _dev(np.array([[a0, r, b0]], np.int32)), threshold=2)
        d1 = _dump(pair[0])
        assert [d1[(2, r)] for r in rows] == [0] + [2] * 7
        _check_victim_call(E, pair, rq, dec1, 1)
    assert (_dump(scripted[0][0]), _dump(scripted[0][1])) == (_dump(scripted[1][0]), _dump(scripted[1][1]))
    assert scripted[0][0].batch_stats() == scripted[1][0].batch_stats()
    assert scripted[1][0].fetch_stats()["victim_hits"] == 1


# --------------------------------------------------------------------------------------- 3. routed both ways, and turned away
def test_routed_both_ways_and_turned_away(E):
    """C1 set 3 full; an odd-table key of it is named by a sample without a hit (agg_hit 0 < 1: to C1) and by a sample with one
    (1 >= 1: to C2).  The route filter gives it to C1: the C2-routed position is served C2's decode of C2's table row, in place.
    Then nine new keys of the empty C1 set 5 in one call: eight get a way, the ninth is served in place, every row exact.  The
    totals of the re-point launch and the state after each call are the model's; the order-0 twin ends in the same state."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    n_rows = SHAPES[shape]
    geom = P.Geometry(caps[0], caps[1], n_rows)
    dec1, dec2 = _dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d)
    full = _rows_of_set(geom, 1, 3, 1, 9)
    x = full[8]
    entries = np.array([[1, 2, r, 2, 0, 0] for r in full[:8]] + [[2, 1, 0, 1, 0, 0]], np.int64)
    used = {3, 5, geom.record(0, 0)}
    a, b = _fresh_rows(geom, used, 0, 1), _fresh_rows(geom, used, 2, 2)
    rq1 = np.array([[a[0], x, b[0]], [0, x, b[1]]], np.int32)
    nine = [_rows_of_set(geom, 1, 5, t, 3) for t in range(3)]
    rq2 = np.array([[nine[0][i], nine[1][i], nine[2][i]] for i in range(3)], np.int32)
    pairs = [_pair(E, shape, d, codecs, caps, 0), _pair(E, shape, d, codecs, caps, 1), _pair(E, shape, d, codecs, caps, 1, (False, True))]
    for pair in pairs[:2]:
        E.load_state_c1c2(pair[0], pair[1], {"entries": entries, "state": None}, strict=False)
    # (a pair over host tables has no warm start: the third pair gets call 2 only, from empty -- its C1 set 5 is as empty)
    exports = []
    for k, pair in enumerate(pairs):
        ff = k > 0
        if k < 2:
            st = BP.State(geom, E.export_state_c1c2(*pair)["entries"])
            j, code, serve = F.judge_bt(st, rq1, 1)
            assert serve[0, 1] == 1 and serve[1, 1] == 2 and j.filtered == {(2, x)}
            f0 = pair[0].fetch_stats()
            tier, out = E.lookup_batch_c1c2(pair[0], pair[1], _dev(rq1), threshold=1)
            assert np.array_equal(tier.cpu().numpy(), code)
            out = out.cpu().numpy()
            assert np.array_equal(_bits(out), _bits(F.expected_rows(serve, rq1, dec1, dec2)))
            assert np.array_equal(_bits(out[1, 1]), _bits(dec2[1][x])) and not np.array_equal(_bits(out[1, 1]), _bits(out[0, 1]))
            BP.apply(st, j)
            after = E.export_state_c1c2(*pair)
            assert BP.State(geom, after["entries"]).triples() == st.triples()
            if ff:
                _src, totals = F.repoint(code, serve, rq1, st)
                f1 = pair[0].fetch_stats()
                assert {key: f1[key] - f0.get(key, 0) for key in totals} == totals == {"repointed": 4, "in_place": 1, "victim_hits": 0}
        st = BP.State(geom, E.export_state_c1c2(*pair)["entries"]) if k < 2 else BP.State(geom)
        j, code, serve = F.judge_bt(st, rq2, 2)
        assert not code.any() and (serve == 1).all()
        f0 = pair[0].fetch_stats()
        tier, out = E.lookup_batch_c1c2(pair[0], pair[1], _dev(rq2), threshold=2)
        assert not tier.any()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(F.expected_rows(serve, rq2, dec1, dec2)))
        d1 = _dump(pair[0])
        kept = [(t + 1, int(rq2[i, t])) for i in range(3) for t in range(3) if (t + 1, int(rq2[i, t])) in d1]
        assert len(kept) == 8 and pair[0].batch_stats()["size"] <= caps[0]
        if ff:
            after = BP.State(geom, [[1, t1, r, 0, 0, 5 * 8 + w] for w, (t1, r) in enumerate(kept)])
            _src, totals = F.repoint(code, serve, rq2, after)
            f1 = pair[0].fetch_stats()
            assert {key: f1[key] - f0.get(key, 0) for key in totals} == totals == {"repointed": 8, "in_place": 1, "victim_hits": 0}
        if k < 2:
            exports.append(E.export_state_c1c2(*pair))
    # (which eight of the nine stay is a matter of timing: the twins agree on everything but set 5)
    e0, e1 = (BP.State(geom, e["entries"]) for e in exports)
    in5 = {(1, t + 1, r) for t in range(3) for r in nine[t]}
    strip = lambda s: {q for q in s.triples() if q[:3] not in in5}
    assert strip(e0) == strip(e1)


# ------------------------------------------------------------------------------------------------------ 4. contended streams
@pytest.mark.parametrize("shape,d,codecs,caps,pinned", [("T3", 36, (8, 4), (64, 128), (True, True)), ("T5", 16, (32, 8), (64, 128), (False, True)),
                                                        ("T3", 16, (8, 4), (36, 96), (True, False))])
def test_contended_stream_invariants(E, shape, d, codecs, caps, pinned):
    """Zipf batches of 300 on an order-1 pair: many new keys per set and copies of a key in one call, so who wins a way is a matter
    of timing; the invariants are not.  Codes are residency at arrival; a hit position's row is its coded tier's table row, a missed
    position's row one of the two tiers' decodes of its table row; every missed position is either re-pointed or served in place;
    no key is resident twice, within or across the tiers; sizes stay within the capacities."""
    n_rows = SHAPES[shape]
    T = len(n_rows)
    dec = (_dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d))
    c1, c2 = _pair(E, shape, d, codecs, caps, 1, pinned)
    rs = np.random.RandomState(T + d)
    perms = [rs.permutation(n) for n in n_rows]
    in1, in2, f0, took = {}, {}, {"repointed": 0, "in_place": 0, "victim_hits": 0}, 0
    for i in range(12):
        B = 300
        rq = np.stack([perms[t][np.minimum(rs.zipf(1.3, B) - 1, n_rows[t] - 1)] for t in range(T)], 1).astype(np.int32)
        tier, out = E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=2)
        tier, out = tier.cpu().numpy(), out.cpu().numpy()
        for t in range(T):
            want = np.array([1 if (t + 1, int(r)) in in1 else (2 if (t + 1, int(r)) in in2 else 0) for r in rq[:, t]], np.uint8)
            assert np.array_equal(tier[:, t], want), "call %d table %d: codes are not residency at arrival" % (i, t)
            is1 = (_bits(out[:, t]) == _bits(dec[0][t][rq[:, t]])).all(1)
            is2 = (_bits(out[:, t]) == _bits(dec[1][t][rq[:, t]])).all(1)
            assert is1[want == 1].all() and is2[want == 2].all(), "call %d table %d: a hit row" % (i, t)
            assert (is1 | is2)[want == 0].all(), "call %d table %d: a missed row" % (i, t)
        f1 = c1.fetch_stats()
        assert f1["repointed"] - f0["repointed"] + f1["in_place"] - f0["in_place"] == int((tier == 0).sum()), "call %d" % i
        took += f1["victim_hits"] - f0["victim_hits"]
        f0 = f1
        in1, in2 = _dump(c1), _dump(c2)
        assert not set(in1) & set(in2), "call %d: a key in both tiers" % i
        s1, s2 = c1.batch_stats(), c2.batch_stats()
        assert len(in1) == s1["size"] <= caps[0] and len(in2) == s2["size"] <= caps[1] and sum(s1["hist"]) == s1["size"]
    assert f0["calls"] == 12 and f0["in_place"] > 0 and f0["repointed"] > 0 and took >= 0


# ---------------------------------------------------------------------------------------------------------- 5. bad indices
def test_an_index_out_of_range(E):
    """An index past its table and a negative one in a call of an order-1 pair over pinned tables: code 0, a zero row, the sticky
    flag raised (once), nothing inserted and none of the three totals moved by them."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    n_rows = SHAPES[shape]
    L = E._lib
    dec = (_dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d))
    c1, c2 = _pair(E, shape, d, codecs, caps, 1, (True, True))
    rs = np.random.RandomState(4)
    rq = np.stack([rs.randint(0, n, 64) for n in n_rows], 1).astype(np.int32)
    E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=2)
    assert L.lib().evs_check_index_errors(None) == 0
    f0 = c1.fetch_stats()
    rq2 = np.stack([rs.randint(0, n, 64) for n in n_rows], 1).astype(np.int32)
    rq2[17, 1] = n_rows[1]
    rq2[18, 2] = -1
    rq2[63, 0] = 1 << 30
    tier, out = E.lookup_batch_c1c2(c1, c2, _dev(rq2), threshold=2)
    tier, out = tier.cpu().numpy(), out.cpu().numpy()
    assert L.lib().evs_check_index_errors(None) == L.EVS_EINDEX
    assert L.lib().evs_check_index_errors(None) == 0
    ok = np.ones(rq2.shape, bool)
    ok[17, 1] = ok[18, 2] = ok[63, 0] = False
    assert not tier[~ok].any() and not out[~ok].any()
    for t in range(3):
        r = rq2[ok[:, t], t]
        got = _bits(out[ok[:, t], t])
        assert ((got == _bits(dec[0][t][r])).all(1) | (got == _bits(dec[1][t][r])).all(1)).all()
    f1 = c1.fetch_stats()
    assert f1["repointed"] - f0["repointed"] + f1["in_place"] - f0["in_place"] == int(((tier == 0) & ok).sum())
    assert all(0 <= r < n_rows[t - 1] for c in (c1, c2) for t, r in _dump(c))


# ----------------------------------------------------------------------------------- 6. alternation with row updates
@pytest.mark.parametrize("pinned", [(False, False), (True, True)])
def test_alternation_with_update_rows(E, pinned):
    """update_rows on each tier between the calls of an order-1 pair, over keys that are resident and keys that are not: the next
    call serves what the tables hold now -- a hit its coded tier's row, a miss one of the two tiers' rows."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    n_rows = SHAPES[shape]
    tables = (_new_tables(shape, codecs[0], d, seed=1), _new_tables(shape, codecs[1], d, seed=2))
    c1, c2 = _pair(E, shape, d, codecs, caps, 1, pinned, tables)
    rs = np.random.RandomState(6)
    in1, in2 = {}, {}
    for i in range(4):
        rq = np.stack([np.minimum(rs.zipf(1.5, 64) - 1, n - 1) for n in n_rows], 1).astype(np.int32)
        if i:
            keys = np.unique(np.stack([np.repeat(np.arange(3), 12), np.concatenate([rq[:12, t] for t in range(3)])], 1), axis=0)
            for c in (c1, c2):
                c.update_rows(torch.from_numpy(keys).cuda(), torch.from_numpy(rs.uniform(-1, 1, (len(keys), d)).astype(np.float32)).cuda())
        dec = [_decode(E, c._tables_kept, shape, codec, d) for c, codec in ((c1, codecs[0]), (c2, codecs[1]))]
        tier, out = E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=2)
        tier, out = tier.cpu().numpy(), out.cpu().numpy()
        for t in range(3):
            want = np.array([1 if (t + 1, int(r)) in in1 else (2 if (t + 1, int(r)) in in2 else 0) for r in rq[:, t]], np.uint8)
            assert np.array_equal(tier[:, t], want)
            is1 = (_bits(out[:, t]) == _bits(dec[0][t][rq[:, t]])).all(1)
            is2 = (_bits(out[:, t]) == _bits(dec[1][t][rq[:, t]])).all(1)
            assert is1[want == 1].all() and is2[want == 2].all() and (is1 | is2)[want == 0].all(), "call %d table %d" % (i, t)
        in1, in2 = _dump(c1), _dump(c2)
    assert in1 and c1.fetch_stats()["calls"] == 4


# ------------------------------------------------------------------------------------------------------------- 7. refusals
def _refused(E, code, word, call):
    with pytest.raises(E._lib.EvsError) as ei:
        call()
    assert ei.value.code == code and word in str(ei.value), str(ei.value)
    return str(ei.value)


SMALL = np.array([[3, 17, 150], [5, 18, 151]], np.int32)


def _serves(E, pair, dec, c3=None):
    """a pair nobody has used: the first call misses everywhere and serves table rows, the second hits"""
    tier, out = E.lookup_batch_c1c2(pair[0], pair[1], _dev(SMALL), threshold=2)
    assert not tier.any()
    out = out.cpu().numpy()
    for t in range(3):
        got = _bits(out[:, t])
        assert ((got == _bits(dec[0][t][SMALL[:, t]])).all(1) | (got == _bits(dec[1][t][SMALL[:, t]])).all(1)).all()
    tier, _out = E.lookup_batch_c1c2(pair[0], pair[1], _dev(SMALL), threshold=2)
    assert bool((tier > 0).all())


def test_refusals_of_the_envelope(E, tmp_path):
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    L = E._lib
    T = 3
    dec = (_dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d))
    rq = _dev(SMALL)
    x = torch.zeros(2, d, device="cuda")
    call = lambda p: (lambda: E.lookup_batch_c1c2(p[0], p[1], rq, threshold=2))
    # one tier at order 1 (either one): the pair / triple runs its own chains; setting the other makes it the fetch-first pair
    for which in (0, 1):
        order = (1, 0) if which == 0 else (0, 1)
        p = _pair(E, shape, d, codecs, caps, order, (False, False))
        _refused(E, L.EVS_EINVAL, "fetch-first", call(p))
        _refused(E, L.EVS_EINVAL, "fetch-first", lambda: E.lookup_interact_c1c2(p[0], p[1], rq, x, threshold=2))
        p[1 - which].set_miss_order("fetch-first")
        _serves(E, p, dec)
        assert p[0].fetch_stats()["calls"] == 2
    # plan / sampled given to a tier
    for name in ("sampled", "plan"):
        p = _pair(E, shape, d, codecs, caps, 1, (True, True))
        p[0].set_batch_policy(name)
        assert "evlfu" in _refused(E, L.EVS_EINVAL, name, call(p))
        p[0].set_batch_policy("setassoc")
        _serves(E, p, dec)
    # file-backed tables under a tier
    paths = []
    for t, tab in enumerate(_tables(shape, codecs[1], d)):
        path = tmp_path / ("ev-table-%d.bin" % (t + 1))
        tab.cpu().numpy().tofile(str(path))
        paths.append(str(path))
    ft = E.gpu_cache.FileTier(paths, d * 4 // 8, 1 << 30)
    p = _pair(E, shape, d, codecs, caps, 1)
    c2 = E.GpuCache("evlfu", caps[1], T, d, codecs[1], "cpp").set_miss_order("fetch-first")
    c2.set_file_backing(ft)
    assert "evlfu" in _refused(E, L.EVS_ESTATE, "file-backed", call((p[0], c2)))
    assert p[0].fetch_stats()["calls"] == 0
    _serves(E, p, dec)
    del c2
    ft.close()
    # the alt-key tier
    p = _pair(E, shape, d, codecs, caps, 1)
    alt = [torch.randint(0, 3, (n,), dtype=torch.int32, device="cuda") * 100 + (t % T) + 1 for t, n in enumerate(SHAPES[shape])]
    c3 = E.GpuAltKeyTier(64, alt)
    assert "evlfu" in _refused(E, L.EVS_EINVAL, "alt-key", lambda: E.lookup_batch_c1c2c3(p[0], p[1], c3, rq, threshold=2))
    _refused(E, L.EVS_EINVAL, "alt-key", lambda: E.lookup_interact_c1c2c3(p[0], p[1], c3, rq, x, threshold=2))
    _serves(E, p, dec)
    # an approximate threshold keeps its refusal
    p = _pair(E, shape, d, codecs, caps, 1)
    p[0].set_batch_approx(2)
    _refused(E, L.EVS_EINVAL, "approximate", call(p))
    p[0].set_batch_approx(0)
    _serves(E, p, dec)
    # tiers that did not start out together, and capacities without a shared record
    p = _pair(E, shape, d, codecs, caps, 1)
    hit, _o = p[0].lookup_batch(rq)
    assert not hit.any()
    assert "evlfu" in _refused(E, L.EVS_EINVAL, "shared set record", call(p))
    hit, _o = p[0].lookup_batch(rq)
    assert bool(hit.all()) and p[0].fetch_stats()["calls"] == 2
    hit, _o = p[1].lookup_batch(rq)                                                   # (C2 is as fresh as before: a tier alone now)
    assert not hit.any()
    p = _pair(E, shape, d, codecs, (16, 128), 1)
    _refused(E, L.EVS_EINVAL, "shared set record", call(p))
    for c in p:
        c.set_miss_order("consume-first")                                             # (nothing was allocated: the order may still be set)
    tier, _o = E.lookup_batch_c1c2(p[0], p[1], rq, threshold=2)
    assert not tier.any()
    # a member of a fetch-first pair is no tier alone; the pair's bag form keeps its refusal
    p = _pair(E, shape, d, codecs, caps, 1)
    for c in p:
        c.set_bag_rule("served-bags")
    _serves(E, p, dec)
    _refused(E, L.EVS_EINVAL, "C1 + C2", lambda: p[0].lookup_batch(rq))
    lo, li = [_dev(np.arange(2, dtype=np.int64))] * T, [_dev(np.zeros(2, np.int64))] * T
    _refused(E, L.EVS_EINVAL, "fetch-first", lambda: E.lookup_bags_c1c2(p[0], p[1], lo, li))
    tier, _o = E.lookup_batch_c1c2(p[0], p[1], rq, threshold=2)
    assert bool((tier > 0).all())


def test_warm_start_of_a_fetch_first_pair(E):
    """export / load accept a pair with both tiers at order 1 over HBM tables (the load launch does not depend on the order): a
    strict round trip, then the loaded pair and the exporter continue alike.  Host tables keep EVS_ESTATE, one tier at order 1
    EVS_EINVAL."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    L = E._lib
    dec = (_dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d))
    n_rows = SHAPES[shape]
    a, b = _pair(E, shape, d, codecs, caps, 1), _pair(E, shape, d, codecs, caps, 1)
    rs = np.random.RandomState(8)
    for _ in range(6):
        rq = np.stack([np.minimum(rs.zipf(1.3, 64) - 1, n - 1) for n in n_rows], 1).astype(np.int32)
        E.lookup_batch_c1c2(a[0], a[1], _dev(rq), threshold=2)
    sa = E.export_state_c1c2(*a)
    assert (sa["entries"][:, 0] == 2).any() and int(sa["state"][0]) == 3
    info = E.load_state_c1c2(b[0], b[1], sa)
    assert info["turned_away"] == (0, 0) and info["batch"] == 6
    assert _same_export(sa, E.export_state_c1c2(*b))
    rq = np.stack([np.minimum(rs.zipf(1.3, 8) - 1, n - 1) for n in n_rows], 1).astype(np.int32)
    ta, oa = E.lookup_batch_c1c2(a[0], a[1], _dev(rq), threshold=2)
    tb, ob = E.lookup_batch_c1c2(b[0], b[1], _dev(rq), threshold=2)
    assert torch.equal(ta, tb) and torch.equal(oa.view(torch.int32), ob.view(torch.int32))
    assert b[0].fetch_stats()["calls"] == 1
    good = {"entries": np.array([[1, 1, 5, 1, 0, 0], [2, 2, 17, 2, 1, 0]], np.int64), "state": None}
    p = _pair(E, shape, d, codecs, caps, 1, (True, False))
    _refused(E, L.EVS_ESTATE, "HBM", lambda: E.load_state_c1c2(p[0], p[1], good, strict=False))
    _serves(E, p, dec)
    _refused(E, L.EVS_ESTATE, "HBM", lambda: E.export_state_c1c2(*p))
    p = _pair(E, shape, d, codecs, caps, (0, 1))
    _refused(E, L.EVS_EINVAL, "fetch-first", lambda: E.load_state_c1c2(p[0], p[1], good, strict=False))
    p[0].set_miss_order("fetch-first")
    _serves(E, p, dec)


@pytest.mark.parametrize("switch,value", [("EVS_SA_PAIR", "0"), ("EVS_CACHE_POLICY", "sampled"), ("EVS_CACHE_POLICY", "plan")])
def test_refusals_behind_the_process_wide_switches(switch, value):
    """EVS_SA_PAIR and EVS_CACHE_POLICY are read once per process: checked in a child (tests/_pair_fetch_env_child.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env[switch] = value
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_pair_fetch_env_child.py"), switch], env=env, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
