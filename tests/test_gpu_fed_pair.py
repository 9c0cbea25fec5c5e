"""The fetch-first C1 + C2 pair over rows the caller supplies (include/evstore_hip.h at evs_cache_pair_fed_begin): begin -> the two
row sources -> finish.  On conflict-free streams a fed pair and an order-1 pair over the same tables in HBM see the same calls and
must agree after every one of them, with the lists, the sources and the stats of tests/_fed_pair_model.py; a hit whose way the
update takes must be served the row that was fed when its key was installed (the spill); a key routed both ways is in both lists;
an abort leaves no trace; every point of the envelope and of the protocol is refused with the pair, or the open call, left usable."""
import numpy as np
import pytest
import torch

import _accuracy as A
import _bag_pair_model as BP
import _fed_pair_common as K
import _fed_pair_model as M
import _pair_fetch_model as F
import _pair_warm_model as P
from _fed_pair_common import CASES, SHAPES, _bits, _dec_shared, _dev, _dump, _pair, _refused

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _state(geom, in1, in2):
    """a _bag_pair_model.State out of two dumps: every key in its own set, the ways filled in key order (a dump does not tell the
    way; the snapshot side of a call -- codes, serve bytes, lists -- does not depend on it)"""
    entries = []
    for tier, dump in ((1, in1), (2, in2)):
        fill = {}
        for (t1, r), s in sorted(dump.items()):
            es = geom.place(tier, t1 - 1, r)[0]
            w = fill.get(es, 0)
            fill[es] = w + 1
            entries.append([tier, t1, r, s, 0, es * geom.tiers[tier - 1].ways + w])
    return BP.State(geom, entries)


def _delta(a, b):
    return {k: a[k] - b.get(k, 0) for k in a}


def _call(E, pair, rq, thr, x=None):
    """one call through the one-call functions; a fed pair: begin -> sources -> finish inside them.  -> (tier, out or R) as numpy"""
    for c in pair:
        if hasattr(c, "source"):
            c.source.last = np.empty(0, np.uint64)
    if x is None:
        tier, out = E.lookup_batch_c1c2(pair[0], pair[1], _dev(rq), threshold=thr)
    else:
        tier, out = E.lookup_interact_c1c2(pair[0], pair[1], _dev(rq), _dev(x), threshold=thr)
    return tier.cpu().numpy(), out.cpu().numpy()


def _listed(c):
    keys = [int(k) for k in c.source.last]
    assert len(set(keys)) == len(keys), "a key is listed twice"
    return sorted(keys)


# ------------------------------------------------------------------------------------------- 1. twins on conflict-free streams
@pytest.mark.parametrize("shape,d,codecs,caps,mask", [c + ((1 << len(SHAPES[c[0]])) - 1,) for c in CASES] + [("T5", 16, (32, 8), (64, 128), 0b01101)])
def test_twins_on_conflict_free_streams(E, shape, d, codecs, caps, mask):
    """An order-1 pair over HBM and a fed pair (mask: the fed tables) see the same calls from empty, lookup_batch_c1c2 and
    lookup_interact_c1c2 alternating, B cycling over 1, 7, 64 and 300 across flushes.  After every call: equal tier codes (the
    snapshot's), equal bits of out / R, equal dumps, counters with hist and fetch_stats; R within the fp64 bound; the lists are the
    model's; pair_fed_stats is the model's."""
    n_rows = SHAPES[shape]
    T = len(n_rows)
    geom = P.Geometry(caps[0], caps[1], n_rows)
    thr = T
    dec1, dec2 = _dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d)
    hbm, fed = _pair(E, shape, d, codecs, caps, 1), _pair(E, shape, d, codecs, caps, 1, fed_mask=mask)
    rs = np.random.RandomState(caps[0] + T + d)
    used, in1, in2 = set(), {}, {}
    kernel = "interact_mixed84_kernel" if codecs == (8, 4) else "interact_mixed_rows_kernel"
    want8 = [0] * 8
    prev = [{"n_evict": 0, "n_flush": 0}, {"n_evict": 0, "n_flush": 0}]
    f_prev = fed[0].fetch_stats()
    s8_prev = E.fed_stats_c1c2(*fed)
    for i, (B, n_new, cover) in enumerate(K.B_CYCLE):
        rq = K._quiet_call(rs, geom, set(in1) | set(in2), used, B, n_new, bool(cover))
        j, code, serve = F.judge_bt(_state(geom, in1, in2), rq, thr)
        rows = F.expected_rows(serve, rq, dec1, dec2)
        x = rs.uniform(-1, 1, (B, d)).astype(np.float32) if i % 2 else None
        (th, oh), (tf, of) = _call(E, hbm, rq, thr, x), _call(E, fed, rq, thr, x)
        assert np.array_equal(th, code) and np.array_equal(tf, code), "call %d: tier codes" % i
        assert np.array_equal(_bits(oh), _bits(of)), "call %d: the twins' bits" % i
        if x is None:
            assert np.array_equal(_bits(of), _bits(rows)), "call %d: rows" % i
        else:
            A.check(of, K._reference(x, rows), "call %d %s" % (i, shape), kernel)
        k1, k2 = M.fed_lists(j, mask)
        assert _listed(fed[0]) == k1 and _listed(fed[1]) == k2, "call %d: the fed lists" % i
        dumps = [(_dump(c1), _dump(c2)) for c1, c2 in (hbm, fed)]
        stats = [(c1.batch_stats(), c2.batch_stats()) for c1, c2 in (hbm, fed)]
        assert dumps[0] == dumps[1], "call %d: dumps" % i
        assert stats[0] == stats[1] and "hist" in stats[1][0], "call %d: counters" % i
        fh, ff = hbm[0].fetch_stats(), fed[0].fetch_stats()
        assert fh == ff, "call %d: fetch_stats" % i
        in1, in2 = dumps[1]
        s8 = E.fed_stats_c1c2(*fed)
        evicted = sum(stats[1][k]["n_evict"] - prev[k]["n_evict"] for k in (0, 1))
        spilled = s8["spilled"] - s8_prev["spilled"]
        df = _delta(ff, f_prev)
        if any(stats[1][k]["n_flush"] != prev[k]["n_flush"] for k in (0, 1)):
            # (a flush was carried out between this call's update and the dumps: what the update itself left cannot be seen, so the
            #  model has no `after`; the totals are held to the twin's above and to each other)
            ds = _delta(s8, s8_prev)
            fedc = {k_: ds[k_] for k_ in ("missed", "from_block", "from_spill")}
            n_fed = int(((code == 0) & (serve > 0) & np.array([M.is_fed(mask, t) for t in range(T)])[None, :]).sum())
            assert fedc["missed"] == n_fed and fedc["from_block"] <= df["in_place"] and fedc["from_spill"] <= df["victim_hits"]
            assert mask != (1 << T) - 1 or (fedc["from_block"], fedc["from_spill"]) == (df["in_place"], df["victim_hits"])
            assert spilled <= evicted and (spilled == evicted or mask != (1 << T) - 1)
        else:
            _src, fetch, fedc = M.sources(code, serve, rq, _state(geom, in1, in2), mask)
            assert df == dict(fetch, calls=1), "call %d: re-point totals" % i
            served = len({(t, int(rq[b, t])) for b in range(B) for t in range(T) if _src[b, t] == M.SPILL})
            assert served <= spilled <= evicted and (spilled == evicted or mask != (1 << T) - 1), "call %d: %d rows spilled, %d evicted" % (i, spilled, evicted)
        want8 = M.stats_step(want8, j, mask, fedc, spilled)
        assert [s8[k] for k in ("calls", "keys1", "keys2", "missed", "from_block", "spilled", "from_spill")] == want8[:7], "call %d: pair_fed_stats" % i
        prev, f_prev, s8_prev = [stats[1][0], stats[1][1]], ff, s8
    assert stats[1][0]["n_flush"] >= 1, "the stream never crossed a flush"
    assert want8[5] > 0 and fed[0].source.calls > 0 and fed[1].source.calls > 0
    print("fed twins %s mask %x: %s, re-point %s" % (shape, mask, E.fed_stats_c1c2(*fed), fed[0].fetch_stats()))


# ------------------------------------------------------------------------------------------- 2. a hit whose way the update takes
def _altered(E, shape, d, codecs):
    """sources that feed ALTERED rows -- C1's bytes with bit 0 flipped, C2's nibbles swapped (codes stay valid) -- and what the
    tiers decode from them"""
    alter = (lambda b: b ^ np.uint8(1), lambda b: ((b << 4) | (b >> 4)).astype(np.uint8))
    decs = []
    for k in (0, 1):
        tabs = [torch.from_numpy(alter[k](t.cpu().numpy())).cuda() for t in K._tables(shape, codecs[k], d)]
        decs.append(K._decode(E, tabs, shape, codecs[k], d))
    return alter, decs


def test_a_hit_whose_way_the_update_takes(E):
    """The scripted branch of the addressed pair's test on a fed pair whose sources feed altered rows: C1 set 0 is filled by eight
    one-sample calls, the first key left at the lowest priority.  The judged call hits that key and routes a ninth key of the set to
    C1, whose update takes the hit key's way in front of the consumers.  The hit position must be served the altered row that was
    fed when its key was installed -- bytes no table holds, which only the spill can supply."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    geom = P.Geometry(caps[0], caps[1], SHAPES[shape])
    alter, (alt1, _alt2) = _altered(E, shape, d, codecs)
    dec1 = _dec_shared(E, shape, codecs[0], d)
    rows, _newcomer, (a0, b0), rq = K._victim_case(geom)
    pair = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111, alter=alter)
    for r in rows:
        _call(E, pair, np.array([[a0, r, b0]], np.int32), 2)
    d1 = _dump(pair[0])
    assert [d1[(2, r)] for r in rows] == [0] + [2] * 7
    f0, s0 = pair[0].fetch_stats(), E.fed_stats_c1c2(*pair)
    tier, out = _call(E, pair, rq, 2)
    assert tier.tolist() == [[0, 1, 0], [0, 0, 0]]
    assert np.array_equal(_bits(out), _bits(F.expected_rows(np.ones((2, 3), np.uint8), rq, alt1, alt1)))
    assert not np.array_equal(_bits(out[0, 1]), _bits(out[1, 1])), "the hit position got the newcomer's row"
    assert not np.array_equal(_bits(out[0, 1]), _bits(dec1[1][rq[0, 1]])), "the sources do not alter"
    f1, s1 = pair[0].fetch_stats(), E.fed_stats_c1c2(*pair)
    assert _delta(f1, f0) == {"calls": 1, "repointed": 5, "in_place": 0, "victim_hits": 1}
    ds = _delta(s1, s0)
    assert ds["spilled"] >= 1 and ds["from_spill"] == 1 and ds["missed"] == 5 and ds["from_block"] == 0 and ds["keys1"] == 5 and ds["keys2"] == 0
    d1 = _dump(pair[0])
    assert (2, int(rq[1, 1])) in d1 and (2, int(rq[0, 1])) not in d1, "the newcomer did not take the hit key's way"


# --------------------------------------------------------------------------------------- 3. routed both ways, and turned away
def _full_set3(E, pair, geom):
    """C1 set 3 filled with eight keys of table 2 by one-sample calls between two resident keys -> (the ninth key of the set, fresh
    rows of tables 1 and 3 in other records, the resident key of table 1)"""
    full = K._rows_of_set(geom, 1, 3, 1, 9)
    off = lambda t, n: [r for r in range(SHAPES["T3"][t]) if geom.record(t, r) not in (3, 5)][:n]   # (records 3 and 5 are the sets the test fills)
    a, b = off(0, 3), off(2, 4)
    for r in full[:8]:
        _call(E, pair, np.array([[a[0], r, b[0]]], np.int32), 2)
    d1 = _dump(pair[0])
    assert all((2, r) in d1 for r in full[:8]) and (1, a[0]) in d1
    return full[8], a, b


def test_routed_both_ways_and_turned_away(E):
    """C1 set 3 full; an odd-table key of it is named by a sample without a hit (to C1) and by a sample with one (to C2): it is in
    BOTH lists, its C1-routed position is served C1's fed row and its C2-routed position C2's fed row in C2's codec -- the route
    filter keeps it out of C2, so that row comes from fed2.  Then nine new keys of the empty C1 set 5: eight are in the arena, the
    ninth is served from the fed block.  Totals are the model's."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    geom = P.Geometry(caps[0], caps[1], SHAPES[shape])
    dec1, dec2 = _dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d)
    pair = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
    x, a, b = _full_set3(E, pair, geom)
    rq1 = np.array([[a[1], x, b[1]], [a[0], x, b[2]]], np.int32)
    st = _state(geom, _dump(pair[0]), _dump(pair[1]))
    j, code, serve = F.judge_bt(st, rq1, 1)
    assert serve[0, 1] == 1 and serve[1, 1] == 2 and j.filtered == {(2, x)} and code[1, 0] == 1
    f0, s0 = pair[0].fetch_stats(), E.fed_stats_c1c2(*pair)
    tier, out = _call(E, pair, rq1, 1)
    assert np.array_equal(tier, code)
    k1, k2 = M.fed_lists(j, 0b111)
    assert _listed(pair[0]) == k1 and _listed(pair[1]) == k2 and ((2 << 32) | x) in k1 and ((2 << 32) | x) in k2
    assert np.array_equal(_bits(out), _bits(F.expected_rows(serve, rq1, dec1, dec2)))
    assert np.array_equal(_bits(out[0, 1]), _bits(dec1[1][x])) and np.array_equal(_bits(out[1, 1]), _bits(dec2[1][x]))
    assert not np.array_equal(_bits(out[1, 1]), _bits(out[0, 1]))
    in1, in2 = _dump(pair[0]), _dump(pair[1])
    assert (2, x) in in1 and (2, x) not in in2
    _src, fetch, fedc = M.sources(code, serve, rq1, _state(geom, in1, in2), 0b111)
    assert _src[1, 1] == M.FED_BLOCK and fedc["from_block"] == 1
    f1, s1 = pair[0].fetch_stats(), E.fed_stats_c1c2(*pair)
    assert _delta(f1, f0) == dict(fetch, calls=1)
    ds = _delta(s1, s0)
    assert (ds["missed"], ds["from_block"], ds["from_spill"], ds["keys1"], ds["keys2"]) == (fedc["missed"], 1, 0, len(k1), len(k2))
    nine = [K._rows_of_set(geom, 1, 5, t, 3) for t in range(3)]
    rq2 = np.array([[nine[0][i], nine[1][i], nine[2][i]] for i in range(3)], np.int32)
    j, code, serve = F.judge_bt(_state(geom, in1, in2), rq2, 2)
    assert not code.any() and (serve == 1).all()
    tier, out = _call(E, pair, rq2, 2)
    assert not tier.any() and len(_listed(pair[0])) == 9 and _listed(pair[1]) == []
    assert np.array_equal(_bits(out), _bits(F.expected_rows(serve, rq2, dec1, dec2)))
    d1 = _dump(pair[0])
    kept = [(t + 1, int(rq2[i, t])) for i in range(3) for t in range(3) if (t + 1, int(rq2[i, t])) in d1]
    assert len(kept) == 8 and pair[0].batch_stats()["size"] <= caps[0]
    f2, s2 = pair[0].fetch_stats(), E.fed_stats_c1c2(*pair)
    assert _delta(f2, f1) == {"calls": 1, "repointed": 8, "in_place": 1, "victim_hits": 0}
    ds = _delta(s2, s1)
    assert (ds["missed"], ds["from_block"], ds["from_spill"], ds["keys1"], ds["keys2"]) == (9, 1, 0, 9, 0)


# ------------------------------------------------------------------------------------------------------------------ 4. abort
def test_abort_leaves_no_trace(E):
    """Twins over fed tables with C1 set 3 full.  One of them begins a call that hits three ways and a call that routes an odd-table
    key of the full set to C1, and drops each: dumps, counters with hist, fetch_stats and pair_fed_stats stay what they were, and
    the same begin lists the same keys.  Then both see a batch that routes that key to C2.  A begin that had raised a way shows in
    the dump; one that had stamped the route filter keeps the key out of C2 -- the dropped call's stamp is the next call's."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    geom = P.Geometry(caps[0], caps[1], SHAPES[shape])
    twins = [_pair(E, shape, d, codecs, caps, 1, fed_mask=0b111) for _ in range(2)]
    for pair in twins:
        x, a, b = _full_set3(E, pair, geom)
    pair = twins[0]
    snap = lambda: (_dump(pair[0]), _dump(pair[1]), pair[0].batch_stats(), pair[1].batch_stats(), pair[0].fetch_stats(), E.fed_stats_c1c2(*pair))
    before = snap()
    full0 = K._rows_of_set(geom, 1, 3, 1, 1)[0]
    for rq in (np.array([[a[0], full0, b[0]]] * 2, np.int32), np.array([[a[1], x, b[1]]], np.int32)):
        lists = []
        for _ in range(2):
            tier, k1, k2 = E.lookup_begin_c1c2(pair[0], pair[1], _dev(rq), threshold=1)
            lists.append((tier.cpu().numpy().copy(), sorted(k1.cpu().tolist()), sorted(k2.cpu().tolist())))
            E.lookup_abort_c1c2(*pair)
            assert snap() == before
        assert np.array_equal(lists[0][0], lists[1][0]) and lists[0][1:] == lists[1][1:]
    assert lists[0][1] == sorted([(1 << 32) | a[1], (2 << 32) | x, (3 << 32) | b[1]]) and lists[0][2] == []
    rqY = np.array([[a[0], x, b[2]]], np.int32)          # a hit: agg_hit 1 >= 1, the full set's key goes to C2
    got = [_call(E, p, rqY, 1) for p in twins]
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    assert (_dump(twins[0][0]), _dump(twins[0][1])) == (_dump(twins[1][0]), _dump(twins[1][1]))
    assert (2, x) in _dump(twins[0][1]), "the dropped call kept the key out of C2"
    assert [c.batch_stats() for c in twins[0]] == [c.batch_stats() for c in twins[1]]
    assert twins[0][0].fetch_stats() == twins[1][0].fetch_stats() and E.fed_stats_c1c2(*twins[0]) == E.fed_stats_c1c2(*twins[1])


# ---------------------------------------------------------------------------------------------------------- 5. bad indices
def test_an_index_out_of_range(E):
    """code 0, a zero row, in no list; the sticky flag is raised by the finish (once), not by the begin"""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    n_rows = SHAPES[shape]
    L = E._lib
    dec = (_dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d))
    c1, c2 = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
    rs = np.random.RandomState(4)
    rq = np.stack([rs.randint(0, n, 64) for n in n_rows], 1).astype(np.int32)
    _call(E, (c1, c2), rq, 2)
    assert L.lib().evs_check_index_errors(None) == 0
    f0 = c1.fetch_stats()
    rq2 = np.stack([rs.randint(0, n, 64) for n in n_rows], 1).astype(np.int32)
    rq2[17, 1] = n_rows[1]
    rq2[18, 2] = -1
    rq2[63, 0] = 1 << 30
    rows_dev = _dev(rq2)
    tier, k1, k2 = E.lookup_begin_c1c2(c1, c2, rows_dev, threshold=2)
    assert L.lib().evs_check_index_errors(None) == 0
    for keys in (k1, k2):
        for key in keys.cpu().tolist():
            assert 0 <= (key & 0xffffffff) < n_rows[(key >> 32) - 1]
    tier, out = E.lookup_finish_c1c2(c1, c2, c1._fetch_fed(k1), c2._fetch_fed(k2))
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


# ------------------------------------------------------------------------------------------------- 6. protocol and envelope
SMALL = np.array([[3, 17, 150], [5, 18, 151]], np.int32)


def _serves(E, pair, dec):
    """a fed pair nobody has used: the first call misses everywhere and serves fed rows, the second hits"""
    tier, out = _call(E, pair, SMALL, 2)
    assert not tier.any()
    for t in range(3):
        got = _bits(out[:, t])
        assert ((got == _bits(dec[0][t][SMALL[:, t]])).all(1) | (got == _bits(dec[1][t][SMALL[:, t]])).all(1)).all()
    tier, _out = _call(E, pair, SMALL, 2)
    assert bool((tier > 0).all())


def test_protocol(E):
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    L = E._lib
    dec = (_dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d))
    c1, c2 = pair = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
    other = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
    rq = _dev(SMALL)
    blk = lambda c: torch.zeros((8, c.dim * c.codec // 8), dtype=torch.uint8, device="cuda")
    # nothing open
    c1._fed_pair_call = (rq, torch.zeros((2, 3), dtype=torch.uint8, device="cuda"), 2, 0, 0, c2)
    _refused(E, L.EVS_ESTATE, "evs_cache_pair_fed_begin", lambda: E.lookup_finish_c1c2(c1, c2, None, None))
    _refused(E, L.EVS_ESTATE, "evs_cache_pair_fed_begin", lambda: E.lookup_abort_c1c2(c1, c2))
    tier, k1, k2 = E.lookup_begin_c1c2(c1, c2, rq, threshold=2)
    assert k1.numel() == 6 and k2.numel() == 0
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty((2, 3, d), device="cuda")
    # everything else on either cache waits
    for c in pair:
        assert "evlfu" in _refused(E, L.EVS_ESTATE, "fed pair call is open", lambda: c.lookup_begin(rq))
        assert L.lib().evs_cache_fed_finish(c._h, None, 0, out.data_ptr(), st) == L.EVS_ESTATE and b"fed pair call is open" in L.lib().evs_last_error()
        _refused(E, L.EVS_ESTATE, "fed pair call is open", c.lookup_abort)
        _refused(E, L.EVS_ESTATE, "fed pair call is open", c.batch_stats)
        _refused(E, L.EVS_ESTATE, "fed pair call is open", c.batch_dump)
        _refused(E, L.EVS_ESTATE, "fed pair call is open", c.fetch_stats)
        _refused(E, L.EVS_ESTATE, "fed pair call is open", c.fed_stats)
        _refused(E, L.EVS_ESTATE, "fed pair call is open", lambda: c.set_fed_backing([None] * 3, SHAPES[shape]))
        _refused(E, L.EVS_ESTATE, "fed pair call is open", lambda: c.update_rows(torch.zeros((1, 2), dtype=torch.int64, device="cuda"), torch.zeros((1, d), device="cuda")))
    _refused(E, L.EVS_ESTATE, "fed pair call is open", lambda: E.lookup_begin_c1c2(c1, c2, rq, threshold=2))
    _refused(E, L.EVS_ESTATE, "fed pair call is open", lambda: E.lookup_begin_c1c2(c1, other[1], rq, threshold=2))
    _refused(E, L.EVS_ESTATE, "fed pair call is open", lambda: E.fed_stats_c1c2(c1, c2))
    assert L.lib().evs_cache_lookup_batch_c1c2(c1._h, c2._h, 2, rq.data_ptr(), out.data_ptr(), tier.data_ptr(), 2, st) == L.EVS_ESTATE
    # another partner, the tiers the other way round
    assert L.lib().evs_cache_pair_fed_finish(c1._h, other[1]._h, blk(c1).data_ptr(), 36, None, 0, out.data_ptr(), st) == L.EVS_ESTATE
    assert b"evs_cache_pair_fed_begin" in L.lib().evs_last_error()
    assert L.lib().evs_cache_pair_fed_finish(c2._h, c1._h, None, 0, blk(c1).data_ptr(), 36, out.data_ptr(), st) == L.EVS_ESTATE
    assert b"partner" in L.lib().evs_last_error()
    assert L.lib().evs_cache_pair_fed_abort(c2._h, c1._h) == L.EVS_ESTATE
    # argument errors of a finish leave the call open
    _refused(E, L.EVS_EINVAL, "NULL fed1", lambda: E.lookup_finish_c1c2(c1, c2, None, None))
    assert L.lib().evs_cache_pair_fed_finish(c1._h, c2._h, blk(c1).data_ptr(), 20, None, 0, out.data_ptr(), st) == L.EVS_EINVAL
    assert L.lib().evs_cache_pair_fed_finish(c1._h, c2._h, blk(c1).data_ptr() + 2, 36, None, 0, out.data_ptr(), st) == L.EVS_EINVAL
    tier, got = E.lookup_finish_c1c2(c1, c2, c1._fetch_fed(k1), None)
    assert not tier.any() and np.array_equal(_bits(got.cpu().numpy()), _bits(F.expected_rows(np.ones((2, 3), np.uint8), SMALL, dec[0], dec[0])))
    _refused(E, L.EVS_ESTATE, "evs_cache_pair_fed_begin", lambda: E.lookup_abort_c1c2(c1, c2))
    tier, _o = _call(E, pair, SMALL, 2)
    assert bool((tier > 0).all()) and E.fed_stats_c1c2(c1, c2)["calls"] == 2
    # a source that fails leaves no call open; destroying a pair with an open call is fine
    c1.set_row_source(lambda keys: (_ for _ in ()).throw(RuntimeError("the store is down")))
    with pytest.raises(RuntimeError):
        E.lookup_batch_c1c2(c1, c2, _dev(SMALL + 10), threshold=2)
    c1.set_row_source(c1.source)
    assert E.fed_stats_c1c2(c1, c2)["calls"] == 2
    tier, _o = _call(E, pair, SMALL + 10, 2)
    assert not tier.any()
    E.lookup_begin_c1c2(other[0], other[1], rq, threshold=2)
    del other


def test_envelope(E):
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    L = E._lib
    n_rows = SHAPES[shape]
    dec = (_dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d))
    rq = _dev(SMALL)
    begin = lambda p: (lambda: E.lookup_begin_c1c2(p[0], p[1], rq, threshold=2))
    # one tier without fed tables, then another fed mask
    p = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
    tab = K._tables(shape, codecs[1], d)
    p[1].set_backing(tab)
    assert "evlfu" in _refused(E, L.EVS_EINVAL, "SAME fed tables", begin(p))
    p[1].set_fed_backing([None, tab[1], None], n_rows)
    _refused(E, L.EVS_EINVAL, "SAME fed tables", begin(p))
    p[1].set_fed_backing([None] * 3, n_rows)
    p[1].set_row_source(p[1].source)
    _serves(E, p, dec)
    # a tier at order 0
    p = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
    p[1].set_miss_order("consume-first")
    assert "evlfu" in _refused(E, L.EVS_EINVAL, "evs_cache_set_miss_order", begin(p))
    p[1].set_miss_order("fetch-first")
    _serves(E, p, dec)
    # plan / sampled given to a tier; an approximate threshold
    for name in ("sampled", "plan"):
        p = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
        p[0].set_batch_policy(name)
        assert "evlfu" in _refused(E, L.EVS_EINVAL, name, begin(p))
        p[0].set_batch_policy("setassoc")
        _serves(E, p, dec)
    p = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
    p[0].set_batch_approx(2)
    assert "evlfu" in _refused(E, L.EVS_EINVAL, "approximate", begin(p))
    p[0].set_batch_approx(0)
    _serves(E, p, dec)
    # no shared record: capacities too small, and a tier that ran alone
    p = _pair(E, shape, d, codecs, (16, 128), 1, fed_mask=0b111)
    assert "evlfu" in _refused(E, L.EVS_EINVAL, "shared set record", begin(p))
    p = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
    hit, _o = p[0].lookup_batch(rq)
    assert not hit.any()
    _refused(E, L.EVS_EINVAL, "shared set record", begin(p))
    hit, _o = p[0].lookup_batch(rq)
    assert bool(hit.all())
    # lru tiers
    cs = []
    for k in (0, 1):
        c = E.GpuCache("lru", caps[k], 3, d, codecs[k]).set_miss_order("fetch-first")
        c.set_fed_backing([None] * 3, n_rows)
        cs.append(c)
    _refused(E, L.EVS_EINVAL, "lru", begin(cs))
    # the interact finish: d in {16, 32, 36}; the refusal leaves the call open
    T = 3
    tabs = [[torch.randint(0, 15, (n, 8 * codec // 8), dtype=torch.uint8, device="cuda") for n in n_rows] for codec in codecs]
    p = []
    for k in (0, 1):
        c = E.GpuCache("evlfu", caps[k], T, 8, codecs[k], "cpp").set_miss_order("fetch-first")
        c.set_fed_backing([None] * 3, n_rows)
        c.source = K._Source(tabs[k])
        p.append(c)
    tier, k1, k2 = E.lookup_begin_c1c2(p[0], p[1], rq, threshold=2)
    x = torch.zeros((2, 8), device="cuda")
    _refused(E, L.EVS_EINVAL, "d must be", lambda: E.lookup_finish_interact_c1c2(p[0], p[1], _dev(p[0].source.rows(k1.cpu().numpy().view(np.uint64))), None, x))
    tier, out = E.lookup_finish_c1c2(p[0], p[1], _dev(p[0].source.rows(k1.cpu().numpy().view(np.uint64))), None)
    assert not tier.any() and out.shape == (2, 3, 8)
    # the other pair calls keep refusing a fed cache
    p = _pair(E, shape, d, codecs, caps, 1, fed_mask=0b111)
    for c in p:
        c.set_row_source(None)
    assert "evlfu" in _refused(E, L.EVS_EINVAL, "a fed cache is a tier alone", lambda: E.lookup_batch_c1c2(p[0], p[1], rq, threshold=2))
    _refused(E, L.EVS_EINVAL, "a fed cache is a tier alone", lambda: E.lookup_interact_c1c2(p[0], p[1], rq, torch.zeros((2, d), device="cuda"), threshold=2))
    for c in p:
        c.set_row_source(c.source)
    _serves(E, p, dec)


# ------------------------------------------------------------------------------------------------------ 7. contended stream
@pytest.mark.parametrize("shape,d,codecs,caps", [("T3", 36, (8, 4), (64, 128)), ("T5", 16, (32, 8), (64, 128)), ("T3", 16, (8, 4), (36, 96))])
def test_contended_stream_invariants(E, shape, d, codecs, caps):
    """Zipf batches of 300: many new keys per set and copies of a key in one call, so who wins a way is a matter of timing; the
    invariants are not.  Codes are residency at arrival; a hit position's row is the fed row of its key in its coded tier's codec
    -- from the arena, or from the spill when the call's own update took the way --, a missed position's row one of the two tiers'
    fed rows; list keys are distinct and each is a missed key; no key is resident twice; sizes stay within the capacities."""
    n_rows = SHAPES[shape]
    T = len(n_rows)
    dec = (_dec_shared(E, shape, codecs[0], d), _dec_shared(E, shape, codecs[1], d))
    c1, c2 = pair = _pair(E, shape, d, codecs, caps, 1, fed_mask=(1 << T) - 1)
    rs = np.random.RandomState(T + d)
    perms = [rs.permutation(n) for n in n_rows]
    in1, in2, f0 = {}, {}, {"repointed": 0, "in_place": 0, "victim_hits": 0}
    for i in range(12):
        B = 300
        rq = np.stack([perms[t][np.minimum(rs.zipf(1.3, B) - 1, n_rows[t] - 1)] for t in range(T)], 1).astype(np.int32)
        tier, out = _call(E, pair, rq, 2)
        missed = {((t + 1) << 32) | int(rq[b, t]) for b in range(B) for t in range(T) if tier[b, t] == 0}
        for t in range(T):
            want = np.array([1 if (t + 1, int(r)) in in1 else (2 if (t + 1, int(r)) in in2 else 0) for r in rq[:, t]], np.uint8)
            assert np.array_equal(tier[:, t], want), "call %d table %d: codes are not residency at arrival" % (i, t)
            is1 = (_bits(out[:, t]) == _bits(dec[0][t][rq[:, t]])).all(1)
            is2 = (_bits(out[:, t]) == _bits(dec[1][t][rq[:, t]])).all(1)
            assert is1[want == 1].all() and is2[want == 2].all(), "call %d table %d: a hit row" % (i, t)
            assert (is1 | is2)[want == 0].all(), "call %d table %d: a missed row" % (i, t)
        l1, l2 = _listed(c1), _listed(c2)
        assert set(l1) <= missed and set(l2) <= missed and set(l1) | set(l2) == missed, "call %d: the lists" % i
        f1 = c1.fetch_stats()
        assert f1["repointed"] - f0["repointed"] + f1["in_place"] - f0["in_place"] == int((tier == 0).sum()), "call %d" % i
        f0 = f1
        in1, in2 = _dump(c1), _dump(c2)
        assert not set(in1) & set(in2), "call %d: a key in both tiers" % i
        s1, s2 = c1.batch_stats(), c2.batch_stats()
        assert len(in1) == s1["size"] <= caps[0] and len(in2) == s2["size"] <= caps[1] and sum(s1["hist"]) == s1["size"]
    s8 = E.fed_stats_c1c2(c1, c2)
    assert s8["calls"] == 12 and s8["missed"] == f0["repointed"] + f0["in_place"] and s8["from_block"] == f0["in_place"]
    assert s8["from_spill"] == f0["victim_hits"] and s8["spilled"] >= (1 if s8["from_spill"] else 0)
    assert L_check(E) == 0
    print("contended %s: %s, re-point %s" % (shape, s8, f0))


def L_check(E):
    return E._lib.lib().evs_check_index_errors(None)
