"""The bag form of the C1 + C2 pair in fetch-first order (both tiers set_miss_order('fetch-first') and set_bag_count('count-first'):
flush -> bags_probe2 -> bags_count2 -> bags_route2 -> the pair's update -> bags_repoint2 -> bags_pool2 (-> interaction) -> close;
include/evstore_hip.h at evs_cache_lookup_bags_c1c2) over tables in HBM and in pinned host memory.  On conflict-free streams an
order-0 pair over HBM and order-1 pairs over HBM, pinned and mixed tables see the same calls and must agree with each other and
with tests/_bag_pair_model.py after every one of them; the re-point launch's totals are held to tests/_bag_pair_fetch_model.py;
directed states are built by hand; contended streams are held to the invariants; one call loops the grid; the two forms of the
pair alternate; every point of the envelope is refused with the pair left usable."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _accuracy as A
import _bag_pair_fetch_model as BF
import _bag_pair_model as BP
import _pair_warm_model as P
import test_gpu_pair_fetch_first as FF

pytestmark = pytest.mark.gpu

SHAPES, CASES = FF.SHAPES, FF.CASES
_dev, _bits, _dump = FF._dev, FF._bits, FF._dump


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _pair(E, shape, d, codecs, caps, order, pinned=(False, False), tables=None, count=True):
    """FF._pair with the bag rule told to both tiers and -- order 1 -- 'count-first' (count: both, or one flag per tier)"""
    p = FF._pair(E, shape, d, codecs, caps, order, pinned, tables)
    count = (count, count) if isinstance(count, bool) else count
    order = (order, order) if isinstance(order, int) else order
    for k, c in enumerate(p):
        c.set_bag_rule("served-bags")
        if order[k] and count[k]:
            assert c.set_bag_count("count-first") is c
    return p


def _flat(bags):
    T = len(bags)
    off = [np.cumsum([0] + [len(b) for b in bags[t][:-1]]).astype(np.int64) for t in range(T)]
    idx = [np.array([r for b in bags[t] for r in b], np.int64) for t in range(T)]
    return off, idx


def _call(E, pair, off, idx, thr, x=None, itself=False):
    lo, li = [_dev(o) for o in off], [_dev(i) for i in idx]
    if x is None:
        tiers, ly = E.lookup_bags_c1c2(pair[0], pair[1], lo, li, threshold=thr)
        return [t.cpu().numpy() for t in tiers], torch.stack(ly).cpu().numpy()
    tiers, R = E.lookup_bags_interact_c1c2(pair[0], pair[1], lo, li, _dev(x), threshold=thr, itself=itself)
    return [t.cpu().numpy() for t in tiers], R.cpu().numpy()


def _delta(f1, f0):
    return {k: f1[k] - f0.get(k, 0) for k in BF.TOTALS}


def _index_error_once(E):
    L = E._lib
    assert L.lib().evs_check_index_errors(None) == L.EVS_EINDEX
    assert L.lib().evs_check_index_errors(None) == 0


def _no_index_error(E):
    assert E._lib.lib().evs_check_index_errors(None) == 0


def _state_of_dumps(geom, d1, d2):
    """a State whose ways are filled in dump order (the model reads residency, scores and 'the set has room' from it)"""
    entries = []
    for tier, dump in ((1, d1), (2, d2)):
        n = {}
        w = geom.tiers[tier - 1].ways
        for (t1, r), s in sorted(dump.items()):
            es = geom.place(tier, t1 - 1, r)[0]
            entries.append([tier, t1, r, s, 0, es * w + n.get(es, 0)])
            n[es] = n.get(es, 0) + 1
            assert n[es] <= w
    return BP.State(geom, entries)


def _cover_call(st, B, T):
    """every bag one or two resident keys, walking every resident key of its table: every sample is served everywhere"""
    resident = sorted(set(st.keys(1)) | set(st.keys(2)))
    by_table = [[r for (t1, r) in resident if t1 == t + 1] for t in range(T)]
    bags = [[([by_table[t][b % len(by_table[t])], by_table[t][(3 * b + 1) % len(by_table[t])]][:1 + b % 2] if by_table[t] else [])
             for b in range(B)] for t in range(T)]
    return _flat(bags)


# ------------------------------------------------------------------------------------------- 1 / 3. twins on conflict-free streams
def _stream(E, shape, d, codecs, caps, pairs, exportable, form, label):
    """pairs[0]: the order-0 pair over HBM.  The same conflict-free ragged calls on every pair, B over 1, 7, 64 and 300, bags of
    0 .. 4 indices; new keys until C1 is full, then two covering calls (every resident key named by samples that are served
    everywhere: all priorities reach T, the close asks for the flush, the next dump runs it on every pair alike), then four more.
    After every call: codes and pooled bits (interact: R, bit-equal to the order-0 pair's and within the fp64 bound) are the
    model's from the exported snapshot, all dumps and counters agree with each other and -- size, hist, n_hits, n_requests,
    n_perfect_hits -- with the model, the exports of the HBM pairs are equal; the state is the model's after every call that no
    flush followed; fetch_stats() of every order-1 C1 is the model's running total."""
    n_rows = SHAPES[shape]
    T = len(n_rows)
    geom = P.Geometry(caps[0], caps[1], n_rows)
    thr = T
    dec1, dec2 = FF._dec_shared(E, shape, codecs[0], d), FF._dec_shared(E, shape, codecs[1], d)
    rs = np.random.RandomState(caps[0] + T + d)
    used, st = set(), BP.State(geom)
    running = {"calls": 0, "repointed": 0, "in_place": 0, "victim_hits": 0}
    plan = [(b, "new") for b in (1, 1, 7, 7, 64, 300, 7, 64, 300, 1, 64, 300)]
    fill, tail = 0, None
    n_flush, i = 0, 0
    cum = {"req": 0, "perfect": 0, "hits": [0, 0]}
    while plan:
        B, kind = plan.pop(0)
        if kind == "new":
            off, idx = BP.conflict_free_call(rs, st, used, B, n_new=min(B, 8, geom.nset))
        else:
            off, idx = _cover_call(st, B, T)
        j = BP.judge(st, B, off, idx, thr)
        assert BP.is_conflict_free(st, j) and not j.bad
        want = BP.pooled(j, idx, dec1, dec2, B)
        x = rs.uniform(-1, 1, (B, d)).astype(np.float32)
        itself = bool(i & 1)
        got = []
        for k, pair in enumerate(pairs):
            codes, res = _call(E, pair, off, idx, thr, x if form == "interact" else None, itself)
            for t in range(T):
                assert np.array_equal(codes[t], j.code[t]), "%s call %d pair %d table %d: codes" % (label, i, k, t)
            if form == "pooled":
                assert np.array_equal(_bits(res), _bits(want)), "%s call %d pair %d: pooled" % (label, i, k)
            else:
                got.append(res)
                w64 = want.astype(np.float64)
                A.check(res, A.Reference(x, [(w64[t], np.abs(w64[t])) for t in range(T)], itself, 1), "%s call %d pair %d" % (label, i, k),
                        "pair bags chain: pooling + dense interaction")
                assert np.array_equal(_bits(res), _bits(got[0])), "%s call %d pair %d: R is not the order-0 pair's" % (label, i, k)
        dumps = [(_dump(c1), _dump(c2)) for c1, c2 in pairs]
        stats = [(c1.batch_stats(), c2.batch_stats()) for c1, c2 in pairs]
        for k in range(1, len(pairs)):
            assert dumps[k] == dumps[0], "%s call %d pair %d: dumps" % (label, i, k)
            assert stats[k] == stats[0], "%s call %d pair %d: counters" % (label, i, k)
        assert "hist" in stats[0][0] and stats[0][0]["n_perfect_hits"] >= 0 and not set(dumps[0][0]) & set(dumps[0][1])
        exports = [E.export_state_c1c2(*pairs[k]) for k in exportable]
        assert all(FF._same_export(exports[0], e) for e in exports[1:]), "%s call %d: exports" % (label, i)
        after = BP.State(geom, exports[0]["entries"])
        assert after.keys(1).keys() == dumps[0][0].keys() and after.keys(2).keys() == dumps[0][1].keys()
        # the counters against the model: size and hist from the exported scores (the state the next call sees), the cumulative
        # hits per tier, requests and all-served samples from the judged calls
        cum["req"] += B
        cum["perfect"] += j.perfect
        for k in (0, 1):
            cum["hits"][k] += j.hits[k]
            scores = [e[2] for e in after.slots[k].values()]
            sk = stats[0][k]
            assert sk["size"] == len(scores) and list(sk["hist"]) == [scores.count(v) for v in range(T + 1)], "%s call %d C%d: size / hist" % (label, i, k + 1)
            assert sk["n_hits"] == cum["hits"][k] and sk["n_requests"] == cum["req"], "%s call %d C%d: n_hits / n_requests" % (label, i, k + 1)
        assert stats[0][0]["n_perfect_hits"] == cum["perfect"], "%s call %d: n_perfect_hits" % (label, i)
        flushed = stats[0][0]["n_flush"] + stats[0][1]["n_flush"]
        behind = BP.apply(st, j)                                     # the pair right behind the call's update: what the re-point launch saw
        if flushed == n_flush:                                       # (a flush runs later, at the dump; which ways it takes is not the model's business)
            assert behind.triples() == after.triples(), "%s call %d: the state is not the model's" % (label, i)
        n_flush = flushed
        BF.add_totals(running, BF.repoint_flat(j, idx, behind)[1])
        for k, pair in enumerate(pairs):
            f = pair[0].fetch_stats()
            if k == 0:
                assert f == {"calls": 0, "repointed": 0, "in_place": 0}
            else:
                assert f == running, "%s call %d pair %d: fetch_stats %s, the model %s" % (label, i, k, f, running)
        st = after
        i += 1
        if not plan and tail is None:
            if n_flush == 0 and stats[0][0]["size"] < caps[0] and fill < 10:   # C1 is not full yet: more new keys, one per set
                plan.append((64, "new"))
                fill += 1
            else:
                tail = [(300, "cover"), (300, "cover"), (7, "new"), (64, "new"), (300, "new"), (1, "new")]
                plan.extend(tail)
    assert stats[0][0]["size"] <= caps[0] and n_flush >= 1, "the stream never crossed a flush: %s" % (stats[0],)
    assert running["repointed"] > 0 and running["in_place"] == 0
    return pairs, running


@pytest.mark.parametrize("form", ["pooled", "interact"])
@pytest.mark.parametrize("shape,d,codecs,caps", CASES)
def test_twins_on_conflict_free_streams(E, shape, d, codecs, caps, form):
    """order 0 over HBM, order 1 + count-first over HBM, order 1 + count-first over pinned tables (see _stream); the export refuses
    the pair over host tables"""
    pairs = [_pair(E, shape, d, codecs, caps, 0), _pair(E, shape, d, codecs, caps, 1), _pair(E, shape, d, codecs, caps, 1, (True, True))]
    pairs, running = _stream(E, shape, d, codecs, caps, pairs, (0, 1), form, "%s %s" % (shape, form))
    FF._refused(E, E._lib.EVS_ESTATE, "HBM", lambda: E.export_state_c1c2(*pairs[2]))
    assert pairs[1][1].fetch_stats() == {"calls": 0, "repointed": 0, "in_place": 0}      # (C2's own counters are not used)
    print("bag twins %s %s: re-point %s" % (shape, form, running))
    _no_index_error(E)


@pytest.mark.parametrize("shape,d,codecs,caps", [CASES[0], CASES[2]])
def test_mixed_tables(E, shape, d, codecs, caps):
    """C1's tables in HBM and C2's pinned, and the other way round: the same stream, the same results as the twins'"""
    pairs = [_pair(E, shape, d, codecs, caps, 0), _pair(E, shape, d, codecs, caps, 1, (False, True)), _pair(E, shape, d, codecs, caps, 1, (True, False))]
    _stream(E, shape, d, codecs, caps, pairs, (0,), "pooled", "mixed %s" % shape)
    _no_index_error(E)


# ------------------------------------------------------------------------------------------------------------ 2. directed states
D_SHAPE, D_D, D_CODECS, D_CAPS, D_THR = "T3", 36, (8, 4), (64, 128), 1
BUSY_SETS = (0, 3, 5)                                                 # C1 sets the scenarios fill by hand


class _Ctx:
    def __init__(self, geom):
        self.geom, self.entries, self.taken, self.per_set = geom, [], {(1, 0)}, {}

    def fresh(self, table0, count):
        """new keys of C1 sets nobody fills by hand, at most six per set: each finds a free way, whatever the timing"""
        out = []
        for r in range(SHAPES[D_SHAPE][table0]):
            es = self.geom.place(1, table0, r)[0]
            if es in BUSY_SETS or (table0 + 1, r) in self.taken or self.per_set.get(es, 0) >= 6:
                continue
            self.taken.add((table0 + 1, r))
            self.per_set[es] = self.per_set.get(es, 0) + 1
            out.append(r)
            if len(out) == count:
                return out
        raise AssertionError("too few rows")


def _s_victim(c):
    """C1 set 0 full, way 0 the lowest; sample 0 hits it (agg_hit 1: still the lowest), sample 1 brings a ninth key of the set"""
    rows = FF._rows_of_set(c.geom, 1, 0, 1, 9)
    c.entries += [[1, 2, r, 0 if j == 0 else 2, 0, 0] for j, r in enumerate(rows[:8])]
    a, b = c.fresh(0, 2), c.fresh(2, 2)
    return dict(samples=[[[a[0]], [rows[0]], [b[0]]], [[a[1]], [rows[8]], [b[1]]]], expect=(5, 0, 1))


def _s_both_ways(c):
    """C1 set 3 full; its odd-table key x is named by a sample with agg_hit 0 (< 1: C1) and by one with agg_hit 1 (C2)"""
    full = FF._rows_of_set(c.geom, 1, 3, 1, 9)
    c.entries += [[1, 2, r, 2, 0, 0] for r in full[:8]] + [[2, 1, 0, 1, 0, 0]]
    a, b = c.fresh(0, 1), c.fresh(2, 2)
    return dict(samples=[[[a[0]], [full[8]], [b[0]]], [[0, 0], [full[8]], [b[1]]]], expect=(4, 1, 0), x=full[8])


def _s_turned_away(c):
    """nine new keys of the empty C1 set 5 in one call: one of them finds no way (which one is a matter of timing)"""
    nine = [FF._rows_of_set(c.geom, 1, 5, t, 3) for t in range(3)]
    return dict(samples=[[list(nine[0]), list(nine[1][:2]), list(nine[2])], [[], [nine[1][2]], []]], expect=(8, 1, 0), timing=True)


def _s_several(c):
    """one new key at four positions of three bags"""
    K = c.fresh(1, 1)[0]
    return dict(samples=[[[], [K], []], [[], [K, K], []], [[], [K], []]], expect=(4, 0, 0))


def _s_empty(c):
    """a sample of empty bags: served everywhere, no lookup (alone: a call without a position -- no launch over positions at all)"""
    return dict(samples=[[[], [], []]], expect=(0, 0, 0))


def _s_uncovered(c):
    """a leading position of table 0 that no bag covers: probed, routed with agg_hit 0, inserted, re-pointed, pooled nowhere"""
    return dict(samples=[[[], [], []]], lead={0: c.fresh(0, 1)}, expect=(1, 0, 0))


def _s_out_of_range(c):
    a, b = c.fresh(0, 1), c.fresh(2, 1)
    return dict(samples=[[[a[0]], [SHAPES[D_SHAPE][1]], [b[0], -1]]], expect=(2, 0, 0), bad=True)


def _s_backwards(c):
    """the last two bags of table 2 behind an offset that goes back: both empty (served), their positions uncovered.  Last."""
    p = c.fresh(2, 2)
    return dict(samples=[[[], [], [p[0]]], [[], [], [p[1]]]], backwards=2, expect=(2, 0, 0), bad=True)


SCENARIOS = {"victim": _s_victim, "both-ways": _s_both_ways, "turned-away": _s_turned_away, "several": _s_several, "empty": _s_empty,
             "uncovered": _s_uncovered, "out-of-range": _s_out_of_range, "backwards": _s_backwards}


@pytest.mark.parametrize("names", [(n,) for n in SCENARIOS] + [tuple(SCENARIOS)], ids=lambda n: n[0] if len(n) == 1 else "all-together")
def test_directed_states(E, names):
    """Hand-made states (non-strict load) on an order-0 and an order-1 pair over HBM, one bag call: codes, pooled bits and the
    three totals -- the model's repoint_flat over the exported state behind the call, and the figures worked out by hand -- for each
    scenario alone and for all of them in one call.  The sticky flag is raised exactly where an index is out of range or an offset
    goes back; the pair serves a second call; the twins end in the same state wherever timing has no say."""
    T = 3
    geom = P.Geometry(D_CAPS[0], D_CAPS[1], SHAPES[D_SHAPE])
    ctx = _Ctx(geom)
    built = [SCENARIOS[n](ctx) for n in names]
    samples = [s for b in built for s in b["samples"]]
    B = len(samples)
    off, idx = _flat([[s[t] for s in samples] for t in range(T)])
    for b in built:
        for t, rows in b.get("lead", {}).items():
            idx[t] = np.concatenate([rows, idx[t]]).astype(np.int64)
            off[t] = off[t] + len(rows)
    if "backwards" in built[-1]:
        off[built[-1]["backwards"]][B - 1] = -1
    expect = dict(zip(BF.TOTALS, np.sum([b["expect"] for b in built], 0).tolist()))
    bad = any(b.get("bad") for b in built)
    timing = any(b.get("timing") for b in built)
    dec1, dec2 = FF._dec_shared(E, D_SHAPE, D_CODECS[0], D_D), FF._dec_shared(E, D_SHAPE, D_CODECS[1], D_D)
    ends = []
    for order in (0, 1):
        pair = _pair(E, D_SHAPE, D_D, D_CODECS, D_CAPS, order)
        st = BP.State(geom)
        if ctx.entries:
            info = E.load_state_c1c2(pair[0], pair[1], {"entries": np.array(ctx.entries, np.int64), "state": None}, strict=False)
            assert sum(info["placed"]) == len(ctx.entries)
            st = BP.State(geom, E.export_state_c1c2(*pair)["entries"])
        j = BP.judge(st, B, off, idx, D_THR)
        assert j.bad == bad
        for b in built:
            if "x" in b:
                assert j.filtered == {(2, b["x"])} and {1, 2} <= set(j.serve[1].tolist())
        f0 = pair[0].fetch_stats()
        codes, ly = _call(E, pair, off, idx, D_THR)
        for t in range(T):
            assert np.array_equal(codes[t], j.code[t]), "table %d: codes" % t
        assert np.array_equal(_bits(ly), _bits(BP.pooled(j, idx, dec1, dec2, B)))
        _index_error_once(E) if bad else _no_index_error(E)
        after = BP.State(geom, E.export_state_c1c2(*pair)["entries"])
        _source, totals = BF.repoint_flat(j, idx, after)
        assert totals == expect, "%s: the model's totals %s, by hand %s" % (names, totals, expect)
        f1 = pair[0].fetch_stats()
        if order:
            assert _delta(f1, f0) == totals and f1["calls"] - f0["calls"] == 1
        else:
            assert f1 == {"calls": 0, "repointed": 0, "in_place": 0}
        assert all(0 <= r < SHAPES[D_SHAPE][t1 - 1] for t1, r in list(after.keys(1)) + list(after.keys(2))), "an index out of range was inserted"
        assert not set(after.keys(1)) & set(after.keys(2))
        # the pair stays usable: the same call again finds what the first one inserted
        j2 = BP.judge(after, B, off, idx, D_THR)
        codes2, ly2 = _call(E, pair, off, idx, D_THR)
        for t in range(T):
            assert np.array_equal(codes2[t], j2.code[t])
        assert np.array_equal(_bits(ly2), _bits(BP.pooled(j2, idx, dec1, dec2, B)))
        _index_error_once(E) if bad else _no_index_error(E)
        assert pair[0].fetch_stats()["calls"] == 2 * order
        ends.append(after.triples())
    if not timing:
        assert ends[0] == ends[1]
    else:
        in5 = {(1, t + 1, r) for t in range(3) for r in FF._rows_of_set(geom, 1, 5, t, 3)}
        assert {q for q in ends[0] if q[:3] not in in5} == {q for q in ends[1] if q[:3] not in in5}


# ------------------------------------------------------------------------------------------------------ 4. contended streams
@pytest.mark.parametrize("shape,d,codecs,caps,pinned", [("T3", 36, (8, 4), (64, 128), (False, False)), ("T3", 36, (8, 4), (64, 128), (True, True)),
                                                        ("T5", 16, (32, 8), (64, 128), (False, True)), ("T3", 16, (8, 4), (36, 96), (True, True))])
def test_contended_stream_invariants(E, shape, d, codecs, caps, pinned):
    """Zipf bags on an order-1 pair: copies of a key in one call, many new keys per set, keys routed both ways -- who wins a way is
    a matter of timing; these are not: codes are the strict snapshot of the dumps before the call, pooled is the model's from that
    snapshot, no key is resident twice, sizes stay within the capacities, and the three totals are repoint_flat's over the dumps
    after the call."""
    n_rows = SHAPES[shape]
    T = len(n_rows)
    geom = P.Geometry(caps[0], caps[1], n_rows)
    dec1, dec2 = FF._dec_shared(E, shape, codecs[0], d), FF._dec_shared(E, shape, codecs[1], d)
    pair = _pair(E, shape, d, codecs, caps, 1, pinned)
    rs = np.random.RandomState(T + d + caps[0])
    perms = [rs.permutation(n) for n in n_rows]
    d1, d2, f0 = {}, {}, pair[0].fetch_stats()
    seen = {name: 0 for name in BF.TOTALS}
    for i in range(10):
        B = (300, 64, 7, 300, 1)[i % 5]
        bags = [[[int(perms[t][min(z - 1, n_rows[t] - 1)]) for z in rs.zipf(1.3, rs.randint(0, 5))] for _b in range(B)] for t in range(T)]
        off, idx = _flat(bags)
        j = BP.judge(_state_of_dumps(geom, d1, d2), B, off, idx, 2)
        codes, ly = _call(E, pair, off, idx, 2)
        for t in range(T):
            assert np.array_equal(codes[t], j.code[t]), "call %d table %d: codes are not residency at arrival" % (i, t)
        assert np.array_equal(_bits(ly), _bits(BP.pooled(j, idx, dec1, dec2, B))), "call %d: pooled" % i
        d1, d2 = _dump(pair[0]), _dump(pair[1])
        assert not set(d1) & set(d2), "call %d: a key in both tiers" % i
        s1, s2 = pair[0].batch_stats(), pair[1].batch_stats()
        assert len(d1) == s1["size"] <= caps[0] and len(d2) == s2["size"] <= caps[1] and sum(s1["hist"]) == s1["size"]
        f1 = pair[0].fetch_stats()
        totals = BF.repoint_flat(j, idx, (d1.keys(), d2.keys()))[1]
        assert _delta(f1, f0) == totals, "call %d: re-point totals %s, the model over the dumps %s" % (i, _delta(f1, f0), totals)
        for name in BF.TOTALS:
            seen[name] += totals[name]
        f0 = f1
    assert f0["calls"] == 10 and seen["repointed"] > 0 and seen["in_place"] > 0
    _no_index_error(E)


# --------------------------------------------------------------------------------------------------------------- 5. looped grid
def test_a_call_that_loops_the_grid(E):
    """More than 256 x 8 192 positions in one call (T = 3, B = 300 000, bags of 1 .. 4), so that every block of the probe, the
    route launch and the re-point launch walks more than one stride: an order-1 pair against its order-0 twin over HBM, after small
    conflict-free warm-up calls -- the big call is hits plus a few new keys, each alone in its sample and its set record.  Codes,
    pooled bits and dumps are equal, pooled is the numpy sum (bags padded to 4 columns, added in order in fp32), and the totals are
    the rule's, evaluated with arrays."""
    shape, d, codecs, caps = "T3", 16, (8, 4), (64, 128)
    n_rows = SHAPES[shape]
    T, B, thr = 3, 300000, 3
    geom = P.Geometry(caps[0], caps[1], n_rows)
    dec = (FF._dec_shared(E, shape, codecs[0], d), FF._dec_shared(E, shape, codecs[1], d))
    pairs = [_pair(E, shape, d, codecs, caps, 0), _pair(E, shape, d, codecs, caps, 1)]
    rs = np.random.RandomState(11)
    used, st = set(), BP.State(geom)
    for Bw in (1, 7, 7, 64, 64, 64, 64, 64):
        off, idx = BP.conflict_free_call(rs, st, used, Bw, n_new=min(Bw, 8))
        for pair in pairs:
            _call(E, pair, off, idx, thr)
        st = BP.State(geom, E.export_state_c1c2(*pairs[0])["entries"])
    assert FF._same_export(E.export_state_c1c2(*pairs[0]), E.export_state_c1c2(*pairs[1]))
    in1, in2 = _dump(pairs[0][0]), _dump(pairs[0][1])
    by_table = [np.array(sorted(r for (t1, r) in list(in1) + list(in2) if t1 == t + 1), np.int64) for t in range(T)]
    assert all(len(b) for b in by_table)
    lens = rs.randint(1, 5, (T, B))
    off = [np.concatenate([[0], np.cumsum(lens[t])[:-1]]).astype(np.int64) for t in range(T)]
    idx = [by_table[t][rs.randint(0, len(by_table[t]), int(lens[t].sum()))] for t in range(T)]
    assert sum(len(i) for i in idx) > 256 * 8192
    new, recs = [], set()                                            # (sample, table, row): one new key per sample and record
    for b in (5, 70000, 150001, 299999):
        t = len(new) % T
        r = next(r for r in range(n_rows[t]) if (t + 1, r) not in used and geom.record(t, r) not in recs)
        recs.add(geom.record(t, r))
        used.add((t + 1, r))
        idx[t][off[t][b]] = r
        new.append((b, t, r))
    occ = np.zeros(geom.nset, np.int64)
    for (t1, r) in in1:
        occ[geom.place(1, t1 - 1, r)[0]] += 1
    tier_of = [np.zeros(n, np.uint8) for n in n_rows]
    for tier, keys in ((1, in1), (2, in2)):
        for (t1, r) in keys:
            tier_of[t1 - 1][r] = tier
    code = [tier_of[t][idx[t]] for t in range(T)]
    serve = [c.copy() for c in code]
    for b, t, r in new:                                              # agg_hit = T - 1 < thr: the key's set has room -> C1, else odd -> C1, even -> C2
        assert code[t][off[t][b]] == 0
        serve[t][off[t][b]] = 1 if occ[geom.place(1, t, r)[0]] < geom.tiers[0].ways else (1 if t % 2 == 1 else 2)
    want = np.zeros((T, B, d), np.float32)
    for t in range(T):
        rows = np.where((serve[t] == 1)[:, None], dec[0][t][idx[t]], dec[1][t][idx[t]])
        acc = np.zeros((B, d), np.float32)
        for c in range(4):
            on = lens[t] > c
            acc[on] = acc[on] + rows[(off[t] + c)[on]]
        want[t] = acc
    lo, li = [_dev(o) for o in off], [_dev(i) for i in idx]
    got = []
    f0 = pairs[1][0].fetch_stats()                                   # (the warm-up calls' totals)
    for pair in pairs:
        tiers, ly = E.lookup_bags_c1c2(pair[0], pair[1], lo, li, threshold=thr)
        got.append(([x.cpu().numpy() for x in tiers], torch.stack(ly).cpu().numpy()))
    for k in (0, 1):
        for t in range(T):
            assert np.array_equal(got[k][0][t], code[t]), "pair %d table %d: codes" % (k, t)
        assert np.array_equal(_bits(got[k][1]), _bits(want)), "pair %d: pooled" % k
    after = [(_dump(c1), _dump(c2)) for c1, c2 in pairs]
    assert after[0] == after[1] and all((t + 1, r) in after[0][0] or (t + 1, r) in after[0][1] for _b, t, r in new)
    assert [c.batch_stats() for c in pairs[0]] == [c.batch_stats() for c in pairs[1]]
    tier_after = [np.zeros(n, np.uint8) for n in n_rows]
    for tier, keys in ((1, after[1][0]), (2, after[1][1])):
        for (t1, r) in keys:
            tier_after[t1 - 1][r] = tier
    totals = dict.fromkeys(BF.TOTALS, 0)
    for t in range(T):
        there = tier_after[t][idx[t]] == serve[t]
        totals["repointed"] += int(((code[t] == 0) & there).sum())
        totals["in_place"] += int(((code[t] == 0) & ~there).sum())
        totals["victim_hits"] += int(((code[t] != 0) & ~there).sum())
    f = pairs[1][0].fetch_stats()
    assert totals["repointed"] == len(new) and totals["in_place"] == 0
    assert _delta(f, f0) == totals and f["calls"] == f0["calls"] + 1 == 9, "fetch_stats %s after %s, the rule %s" % (f, f0, totals)
    _no_index_error(E)


# ----------------------------------------------------------------------------------------------------------------- 6. alternation
@pytest.mark.parametrize("pinned", [(False, False), (True, True)])
def test_alternation_with_the_bt_form_and_update_rows(E, pinned):
    """One order-1 pair takes lookup_batch_c1c2 (its fetch-first chain), bag calls and update_rows on both tiers in turn; an order-0
    pair over HBM tables of its own gets the same calls.  Conflict-free calls: codes, served rows / pooled bits, dumps and counters
    agree after every call, and the order-1 pair's counters add up over both forms."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    n_rows = SHAPES[shape]
    T, thr = 3, 3
    geom = P.Geometry(caps[0], caps[1], n_rows)
    tabs = [(FF._new_tables(shape, codecs[0], d, seed=3), FF._new_tables(shape, codecs[1], d, seed=4)) for _ in range(2)]
    pairs = [_pair(E, shape, d, codecs, caps, 0, tables=tabs[0]), _pair(E, shape, d, codecs, caps, 1, pinned, tables=tabs[1])]
    rs = np.random.RandomState(13)
    used, st = set(), BP.State(geom)
    in1, in2 = {}, {}
    n_bt = n_bags = 0
    for i in range(12):
        if i % 3 == 2:                                               # new rows under resident and absent keys, on both tiers of both pairs
            keys = np.unique(np.stack([rs.randint(0, T, 40), rs.randint(0, 200, 40)], 1), axis=0)
            vals = torch.from_numpy(rs.uniform(-1, 1, (len(keys), d)).astype(np.float32)).cuda()
            for pair in pairs:
                for c in pair:
                    c.update_rows(torch.from_numpy(keys).cuda(), vals)
        B = (1, 7, 64, 300)[i % 4]
        if i % 2 == 0:
            rq = FF._quiet_call(rs, geom, set(in1) | set(in2), used, B, 8)
            res = [E.lookup_batch_c1c2(p[0], p[1], _dev(rq), threshold=thr) for p in pairs]
            res = [(a.cpu().numpy(), b.cpu().numpy()) for a, b in res]
            n_bt += 1
        else:
            off, idx = BP.conflict_free_call(rs, st, used, B, n_new=min(B, 8))
            res = [_call(E, p, off, idx, thr) for p in pairs]
            res = [(np.concatenate(a), b) for a, b in res]
            n_bags += 1
        assert np.array_equal(res[0][0], res[1][0]), "call %d: codes" % i
        assert np.array_equal(_bits(res[0][1]), _bits(res[1][1])), "call %d: served bits" % i
        dumps = [(_dump(c1), _dump(c2)) for c1, c2 in pairs]
        assert dumps[0] == dumps[1], "call %d: dumps" % i
        assert [c.batch_stats() for c in pairs[0]] == [c.batch_stats() for c in pairs[1]], "call %d: counters" % i
        in1, in2 = dumps[0]
        st = BP.State(geom, E.export_state_c1c2(*pairs[0])["entries"])
    f = pairs[1][0].fetch_stats()
    assert n_bt and n_bags and f["calls"] == n_bt + n_bags and f["repointed"] > 0 and "victim_hits" in f
    assert pairs[0][0].fetch_stats()["calls"] == 0
    _no_index_error(E)


def test_installed_rows_are_served_from_the_arena(E):
    """Within one call a re-pointed position's arena row and its table row hold the same bytes, so no output tells them apart; what
    can be seen is that the update installed the rows the re-point launch counted: after a call of new keys on an order-1 pair over
    HBM tables of its own every table is overwritten behind the cache's back, and the same call again hits everywhere and pools the
    OLD rows -- from the arenas -- with every position found in place by the re-point launch (no total moves)."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    T, thr = 3, 3
    geom = P.Geometry(caps[0], caps[1], SHAPES[shape])
    tabs = (FF._new_tables(shape, codecs[0], d, seed=5), FF._new_tables(shape, codecs[1], d, seed=6))
    old = [FF._decode(E, tabs[k], shape, codecs[k], d) for k in (0, 1)]
    pair = _pair(E, shape, d, codecs, caps, 1, tables=tabs)
    off, idx = BP.conflict_free_call(np.random.RandomState(2), BP.State(geom), set(), 7, n_new=7)
    j = BP.judge(BP.State(geom), 7, off, idx, thr)
    n_new = sum(len(i) for i in idx)
    assert n_new == 7 and not np.concatenate(j.code).any()
    codes, ly = _call(E, pair, off, idx, thr)
    assert not np.concatenate(codes).any() and np.array_equal(_bits(ly), _bits(BP.pooled(j, idx, old[0], old[1], 7)))
    f1 = pair[0].fetch_stats()
    assert (f1["repointed"], f1["in_place"], f1["victim_hits"]) == (n_new, 0, 0)
    torch.cuda.synchronize()
    for tab in tabs[0] + tabs[1]:
        tab.zero_()
    new = [FF._decode(E, tabs[k], shape, codecs[k], d) for k in (0, 1)]
    j2 = BP.judge(BP.State(geom, E.export_state_c1c2(*pair)["entries"]), 7, off, idx, thr)
    assert np.concatenate(j2.code).all()
    codes, ly = _call(E, pair, off, idx, thr)
    assert np.concatenate(codes).all()
    assert np.array_equal(_bits(ly), _bits(BP.pooled(j2, idx, old[0], old[1], 7))), "a hit was not served the row the update installed"
    assert not np.array_equal(_bits(ly), _bits(BP.pooled(j2, idx, new[0], new[1], 7)))
    f2 = pair[0].fetch_stats()
    assert f2["calls"] == 2 and _delta(f2, f1) == {"repointed": 0, "in_place": 0, "victim_hits": 0}
    _no_index_error(E)


# ------------------------------------------------------------------------------------------------------------------- 7. refusals
def _small(T=3):
    """(lS_o, lS_i): two samples, bags of 2 / 0 and 1 / 1 and 0 / 2 indices"""
    bags = [[[3, 5], []], [[17], [18]], [[], [150, 151]]][:T]
    off, idx = _flat(bags)
    return [_dev(o) for o in off], [_dev(i) for i in idx]


def _serves_bags(E, pair):
    """a pair nobody has used: the first bag call misses everywhere, the second hits everywhere"""
    lo, li = _small()
    tiers, _ly = E.lookup_bags_c1c2(pair[0], pair[1], lo, li, threshold=2)
    assert not torch.cat(tiers).any()
    tiers, _ly = E.lookup_bags_c1c2(pair[0], pair[1], lo, li, threshold=2)
    assert bool((torch.cat(tiers) > 0).all())


def test_refusals_of_the_envelope(E, tmp_path):
    """Every refusal comes before anything is allocated (the pair can still be told another order or policy, and serves), names the
    policy where the fetch-first envelope speaks, and leaves fetch_stats() untouched."""
    shape, d, codecs, caps = "T3", 36, (8, 4), (64, 128)
    L = E._lib
    T = 3
    lo, li = _small()
    x = torch.zeros(2, d, device="cuda")
    call = lambda p: (lambda: E.lookup_bags_c1c2(p[0], p[1], lo, li, threshold=2))
    icall = lambda p: (lambda: E.lookup_bags_interact_c1c2(p[0], p[1], lo, li, x, threshold=2))
    none = {"calls": 0, "repointed": 0, "in_place": 0}
    # one tier at order 1
    for which in (0, 1):
        p = _pair(E, shape, d, codecs, caps, (1, 0) if which == 0 else (0, 1))
        assert "evlfu" in FF._refused(E, L.EVS_EINVAL, "C%d runs fetch-first" % (which + 1), call(p))
        FF._refused(E, L.EVS_EINVAL, "fetch-first", icall(p))
        p[1 - which].set_miss_order("fetch-first").set_bag_count("count-first")
        _serves_bags(E, p)
        assert p[0].fetch_stats()["calls"] == 2
    # both at order 1, count-first on none or on one tier
    # (over pinned tables too: the refusal that names count-first comes before the one about host-memory tables)
    for count, pinned in (((False, False), (False, False)), ((True, False), (False, False)), ((False, True), (False, False)),
                          ((False, False), (True, True)), ((True, False), (False, True))):
        p = _pair(E, shape, d, codecs, caps, 1, pinned, count=count)
        msg = FF._refused(E, L.EVS_EINVAL, "fetch-first", call(p))
        assert "evlfu" in msg and "evs_cache_set_bag_count" in msg
        FF._refused(E, L.EVS_EINVAL, "fetch-first", icall(p))
        assert p[0].fetch_stats() == none
        for c in p:
            c.set_bag_count("count-first")
        _serves_bags(E, p)
    # file-backed tables
    paths = []
    for t, tab in enumerate(FF._tables(shape, codecs[1], d)):
        path = tmp_path / ("ev-table-%d.bin" % (t + 1))
        tab.cpu().numpy().tofile(str(path))
        paths.append(str(path))
    ft = E.gpu_cache.FileTier(paths, d * 4 // 8, 1 << 30)
    p = _pair(E, shape, d, codecs, caps, 1)
    c2 = E.GpuCache("evlfu", caps[1], T, d, codecs[1], "cpp").set_miss_order("fetch-first").set_bag_rule("served-bags").set_bag_count("count-first")
    c2.set_file_backing(ft)
    assert "evlfu" in FF._refused(E, L.EVS_ESTATE, "file-backed", call((p[0], c2)))
    assert p[0].fetch_stats() == none
    _serves_bags(E, p)
    del c2
    ft.close()
    # plan / sampled given to a tier
    for name in ("sampled", "plan"):
        p = _pair(E, shape, d, codecs, caps, 1, (True, True))
        p[0].set_batch_policy(name)
        assert "evlfu" in FF._refused(E, L.EVS_EINVAL, name, call(p))
        p[0].set_batch_policy("setassoc")
        _serves_bags(E, p)
    # capacities without a shared record; a tier that started alone
    p = _pair(E, shape, d, codecs, (16, 128), 1)
    assert "evlfu" in FF._refused(E, L.EVS_EINVAL, "shared set record", call(p))
    for c in p:
        c.set_miss_order("consume-first")                            # (nothing was allocated: the order may still be set)
    tier, _o = E.lookup_batch_c1c2(p[0], p[1], _dev(FF.SMALL), threshold=2)
    assert not tier.any()
    p = _pair(E, shape, d, codecs, caps, 1)
    hit, _o = p[0].lookup_batch(_dev(FF.SMALL))
    assert not hit.any()
    assert "evlfu" in FF._refused(E, L.EVS_EINVAL, "shared set record", call(p))
    hit, _o = p[0].lookup_batch(_dev(FF.SMALL))
    assert bool(hit.all())
    # alt-key history: an order-1 pair cannot acquire one -- the triple refuses it, and its bag form serves afterwards; on an order-0
    # pair that has run as a triple the bag form keeps its refusal
    alt = [torch.randint(0, 3, (n,), dtype=torch.int32, device="cuda") * 100 + (t % T) + 1 for t, n in enumerate(SHAPES[shape])]
    c3 = E.GpuAltKeyTier(64, alt)
    p = _pair(E, shape, d, codecs, caps, 1)
    assert "evlfu" in FF._refused(E, L.EVS_EINVAL, "alt-key", lambda: E.lookup_batch_c1c2c3(p[0], p[1], c3, _dev(FF.SMALL), threshold=2))
    _serves_bags(E, p)
    assert p[0].fetch_stats()["calls"] == 2
    p = _pair(E, shape, d, codecs, caps, 0)
    E.lookup_batch_c1c2c3(p[0], p[1], c3, _dev(FF.SMALL), threshold=2)
    FF._refused(E, L.EVS_EINVAL, "triple", call(p))
    E.lookup_batch_c1c2c3(p[0], p[1], c3, _dev(FF.SMALL), threshold=2)
    # a resident server on a tier (serve_start hands the cache to the exact path, which is what the batched path's own check names:
    # EVS_ESTATE before anything is allocated); the server is never sent a request here
    for which in (0, 1):
        p = _pair(E, shape, d, codecs, caps, 1)
        p[which].serve_start(n_slots=2)
        try:
            assert "evlfu" in FF._refused(E, L.EVS_ESTATE, "exact path", call(p))
            FF._refused(E, L.EVS_ESTATE, "exact path", icall(p))
            assert p[0].fetch_stats() == none
        finally:
            p[which].serve_stop()
        _serves_bags(E, _pair(E, shape, d, codecs, caps, 1))
    # an approximate threshold
    p = _pair(E, shape, d, codecs, caps, 1)
    p[1].set_batch_approx(2)
    FF._refused(E, L.EVS_EINVAL, "approximate", call(p))
    assert p[0].fetch_stats() == none
    p[1].set_batch_approx(0)
    _serves_bags(E, p)
    # an order-0 pair over pinned tables keeps its refusal, with or without count-first
    for which in (0, 1):
        p = _pair(E, shape, d, codecs, caps, 0, (which == 0, which == 1))
        FF._refused(E, L.EVS_ESTATE, "C%d sits over host-memory" % (which + 1), call(p))
        for c in p:
            c.set_bag_count("count-first")
        FF._refused(E, L.EVS_ESTATE, "C%d sits over host-memory" % (which + 1), call(p))
        p[which].set_backing(FF._tables(shape, codecs[which], d))
        _serves_bags(E, p)
        assert p[0].fetch_stats() == none                            # (an order-0 pair ignores the count setting: today's chain)
    _no_index_error(E)


@pytest.mark.parametrize("switch,value", [("EVS_SA_PAIR", "0"), ("EVS_CACHE_POLICY", "sampled"), ("EVS_CACHE_POLICY", "plan")])
def test_refusals_behind_the_process_wide_switches(switch, value):
    """EVS_SA_PAIR and EVS_CACHE_POLICY are read once per process: checked in a child (tests/_bag_pair_fetch_env_child.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env[switch] = value
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_bag_pair_fetch_env_child.py"), switch], env=env, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
