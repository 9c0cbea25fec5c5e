"""Ragged bags through the batched C1 + C2 pair (lookup_bags_c1c2 / lookup_bags_interact_c1c2; csrc/evs_cache_policy.hip:
bags_probe2_kernel -> bags_count2_kernel -> bags_route2_kernel -> bags_pool2_kernel, then the pair's own update launch) held to
the rule written down in include/evstore_hip.h at evs_cache_lookup_bags_c1c2: codes and pooled rows exact against the Python
restatement (tests/_bag_pair_model.py) from a hand-made state and on contended input, equal to the (B, T) form with one index
per bag, pinned entry by entry to the model on conflict-free ragged streams, and every point of the envelope refused with the
pair left usable."""
import functools

import numpy as np
import pytest
import torch

import _accuracy as acc
import _bag_pair_model as BP
import _pair_warm_model as P
import test_gpu_pair_warm_start as W

pytestmark = pytest.mark.gpu

N_ROWS, T = W.N_ROWS, W.T
CAPS = [(64, 128), (64, 96), (32, 128)]                  # 8 + 2 x 8 ways, 8 + 12, 4 + 2 x 8
SHAPES = [((64, 128), (8, 4), 36), ((64, 96), (8, 4), 16), ((32, 128), (32, 8), 36)]


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _tables(codec, d):
    """-> (the device tables set_backing takes, per table the fp32 rows the oracle decodes from them)"""
    from oracle import oracle as orc
    tabs = [np.ascontiguousarray(t[:, :d]) for t in orc.kaggle_tables(N_ROWS, 31)]
    if codec == 32:
        return [_dev(t) for t in tabs], tabs
    raws = [orc.encode_table(np.clip(t * np.sqrt(len(t)), -1, 1), codec) for t in tabs]
    return [_dev(r) for r in raws], [orc.decode(a, codec, d) for a in raws]


def _pair(E, caps, codecs=(8, 4), d=36, rule=True):
    c1, c2 = E.GpuCache("evlfu", caps[0], T, d, codecs[0], "cpp"), E.GpuCache("evlfu", caps[1], T, d, codecs[1], "cpp")
    c1.set_backing(_tables(codecs[0], d)[0])
    c2.set_backing(_tables(codecs[1], d)[0])
    if rule:
        c1.set_bag_rule("served-bags")
        c2.set_bag_rule("served-bags")
    return c1, c2


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _call(E, pair, off, idx, thr, **kw):
    tiers, ly = E.lookup_bags_c1c2(pair[0], pair[1], [_dev(o) for o in off], [_dev(i) for i in idx], threshold=thr, **kw)
    return [t.cpu().numpy() for t in tiers], torch.stack(ly).cpu().numpy()


def _index_error_once(E):
    L = E._lib
    assert L.lib().evs_check_index_errors(None) == L.EVS_EINDEX
    assert L.lib().evs_check_index_errors(None) == 0


def _no_index_error(E):
    assert E._lib.lib().evs_check_index_errors(None) == 0


def _hand_made(geom, rs, full_sets=(0, 1)):
    """entries (slot column 0) with C1 sets that are full and C1 sets that have room, and a C2 that is part full; an odd-table
    key K outside whose C1 set is full"""
    w1 = geom.tiers[0].ways
    K = next((2, r) for r in range(N_ROWS[1]) if geom.place(1, 1, r)[0] == full_sets[0])
    rows, keys = [], {K}
    for es in full_sets:
        for key in P.keys_of_set(geom, 1, es, w1, skip=keys):
            keys.add(key)
            rows.append([1, key[0], key[1], int(rs.randint(0, T + 1)), int(rs.randint(5)), 0])
    per = {}
    for tier, n in ((1, geom.tiers[0].cap // 3), (2, geom.tiers[1].cap // 2)):
        got = 0
        while got < n:
            t = int(rs.randint(T))
            r = int(rs.randint(N_ROWS[t]))
            es = geom.place(tier, t, r)[0]
            room = (w1 - 2) if tier == 1 else geom.tiers[1].ways
            if (t + 1, r) in keys or (tier == 1 and es in full_sets) or per.get((tier, es), 0) >= room:
                continue
            keys.add((t + 1, r))
            per[(tier, es)] = per.get((tier, es), 0) + 1
            rows.append([tier, t + 1, r, int(rs.randint(0, T + 1)), int(rs.randint(5)), 0])
            got += 1
    entries = np.array(rows, np.int64)
    rs.shuffle(entries)
    return entries, K


def _ragged(rs, resident, B, p_res=0.6, rows=N_ROWS, tables=range(T)):
    """bags of 0 .. 4 indices per sample for `tables` (the others: nnz = 0): resident keys with probability p_res, else any row"""
    by_table = [[r for (t1, r) in resident if t1 == t + 1] for t in range(T)]
    bags = [[[] for _ in range(B)] for _ in range(T)]
    for t in tables:
        for b in range(B):
            for _ in range(int(rs.randint(0, 5))):
                if by_table[t] and rs.rand() < p_res:
                    bags[t][b].append(int(by_table[t][rs.randint(len(by_table[t]))]))
                else:
                    bags[t][b].append(int(rs.randint(rows[t])))
    return bags


def _flat(bags):
    off = [np.cumsum([0] + [len(b) for b in bags[t][:-1]]).astype(np.int64) for t in range(T)]
    idx = [np.array([r for b in bags[t] for r in b], np.int64) for t in range(T)]
    return off, idx


def _state(E, geom, pair):
    return BP.State(geom, E.export_state_c1c2(*pair)["entries"])


# ------------------------------------------------------------------------------------- 1. snapshot exactness, hand-made state
@pytest.mark.parametrize("caps,codecs,d", SHAPES)
def test_snapshot_exactness_from_a_hand_made_state(E, caps, codecs, d):
    """load_state_c1c2 puts the pair into a hand-made state with full C1 sets and C1 sets with room; one bag call follows with an
    empty table (nnz = 0), empty bags, leading and trailing positions no bag covers, an index out of range, a backwards offset,
    an offset past nnz, sum(nnz) > 256, and an odd-table key K of a full C1 set named by a sample below the threshold (-> C1) and
    by one at it (-> C2).  Codes are membership in the exported lists; pooled is bit-equal to the model -- every position decoded
    by its serving tier with the oracle's decoders, added in index order -- although the input is contended (K is routed both
    ways, keys repeat); the sticky flag is read once."""
    thr, B = 2, 48
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    rs = np.random.RandomState(caps[0] + d)
    entries, K = _hand_made(geom, rs)
    pair = _pair(E, caps, codecs, d)
    info = E.load_state_c1c2(pair[0], pair[1], {"entries": entries, "state": None}, strict=False)
    assert info["placed"][0] > 0 and info["placed"][1] > 0
    st = _state(E, geom, pair)
    in1, in2 = st.keys(1), st.keys(2)
    assert K not in in1 and K not in in2 and not st.c1_room(1, K[1])
    resident = sorted(set(in1) | set(in2))
    res2 = [r for (t1, r) in resident if t1 == 3]
    absent2 = next(r for r in range(N_ROWS[2]) if (3, r) not in in1 and (3, r) not in in2)
    bags = _ragged(rs, resident, B, tables=(1, 2))                  # table 0: nnz = 0, every bag empty (served)
    for t in (1, 2):                                                # bags of 4 in the middle: sum(nnz) crosses 256
        for b in range(8, 40):
            while len(bags[t][b]) < 4:
                bags[t][b].append(int(rs.randint(N_ROWS[t])))
    bags[1][0], bags[2][0] = [K[1]], [res2[0]]                     # sample 0: only K missed, agg = 2 = thr -> C2
    bags[1][1], bags[2][1] = [K[1]], [absent2]                     # sample 1: agg = 1 < thr, table 1 is odd -> C1
    bags[1][5], bags[2][5] = [], []                                # an all-empty sample: served everywhere, no lookup
    bags[1][20][1] = N_ROWS[1]                                     # out of range: no key
    off, idx = _flat(bags)
    off[1][B - 1] = -1                                             # a backwards offset: bags B - 2 and B - 1 empty, what they held uncovered
    off[2] = off[2] + 2                                            # table 2: two leading positions nobody covers ...
    idx[2] = np.concatenate([[absent2, res2[-1]], idx[2]]).astype(np.int64)
    off[2][B - 1] = len(idx[2]) + 3                                # ... and an offset past nnz: trailing positions uncovered
    assert sum(len(i) for i in idx) > 256 and len(idx[0]) == 0
    j = BP.judge(st, B, off, idx, thr)
    assert j.bad and j.agg[0] == 2 and j.agg[1] == 1 and j.agg[5] == T
    assert K in j.listed[0] and K in j.listed[1] and (j.pos_sample[1] == -1).any() and (j.pos_sample[2][:2] == -1).all()
    assert {1, 2} <= set(np.concatenate(j.code).tolist()) and {0, 1, 2} <= set(np.concatenate(j.serve).tolist())
    tiers, ly = _call(E, pair, off, idx, thr)
    for t in range(T):
        assert np.array_equal(tiers[t], j.code[t]), "table %d: codes are membership in the exported lists" % t
    want = BP.pooled(j, idx, _tables(codecs[0], d)[1], _tables(codecs[1], d)[1], B)
    assert np.array_equal(_bits(ly), _bits(want)), "pooled differs from the model in %d elements" % int((_bits(ly) != _bits(want)).sum())
    _index_error_once(E)
    # the call counted what the rule says; K, routed both ways, is not in C2, and in C1 unless its set turned it away (more new
    # keys than ways)
    s1, s2 = pair[0].batch_stats(), pair[1].batch_stats()
    assert (s1["n_hits"], s2["n_hits"]) == j.hits and s1["n_requests"] == s2["n_requests"] == B and s1["n_perfect_hits"] == j.perfect
    after = _state(E, geom, pair)
    rivals = [key for key in j.insert[0] if geom.place(1, key[0] - 1, key[1])[0] == geom.place(1, 1, K[1])[0]]
    assert K in j.filtered and K not in after.keys(2)
    assert K in after.keys(1) or len(rivals) > geom.tiers[0].ways, "K is in neither tier; %d new keys for its C1 set: %s, the set now: %s" % (
        len(rivals), rivals, after.ways_of(1, geom.place(1, 1, K[1])[0]))
    assert not (set(after.keys(1)) & set(after.keys(2)))


# ----------------------------------------------------------------------------------- 2. one index per bag against the (B, T) form
def _fill_twins(E, caps, thr, rule_b=True):
    """pair a filled through the (B, T) form, pair b loaded strictly from a's export -> (a, b, geom, used keys, calls so far)"""
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    a, b = _pair(E, caps, rule=rule_b), _pair(E, caps)
    rs = np.random.RandomState(caps[0])
    used, k = set(), 0
    while True:
        rq = np.stack([rs.randint(0, n, 256) for n in N_ROWS], 1).astype(np.int32)
        used |= {(t + 1, int(r)) for t in range(T) for r in rq[:, t]}
        E.lookup_batch_c1c2(a[0], a[1], _dev(rq), threshold=thr)
        k += 1
        if a[0].batch_stats()["size"] >= 0.9 * caps[0] and a[1].batch_stats()["size"] >= 0.9 * caps[1]:
            break
        assert k < 200
    sa = E.export_state_c1c2(*a)
    assert E.load_state_c1c2(b[0], b[1], sa)["batch"] == k
    return a, b, geom, used, rs


@pytest.mark.parametrize("caps", CAPS)
def test_one_index_per_bag_is_the_bt_form(E, caps):
    """Twin pairs, the same 40-batch conflict-free stream (tests/test_gpu_pair_warm_start.py::_quiet_batch): pair a through
    lookup_batch_c1c2, pair b through lookup_bags_c1c2 with one index per bag -- from call 20 on the two forms alternate on BOTH
    pairs, out of step.  After every call: codes = tier, pooled[k][b] bit-equal to out[b, k], both tiers' counters equal; the
    exports are equal every eighth call and at the end."""
    thr = 3
    a, b, geom, used, rs = _fill_twins(E, caps, thr)
    B = min(16, geom.nset)
    lo = [torch.arange(B, dtype=torch.int64, device="cuda")] * T

    def bt(pair, rq):
        tier, out = E.lookup_batch_c1c2(pair[0], pair[1], rq, threshold=thr)
        return tier, out.permute(1, 0, 2).contiguous()

    def bags(pair, rq):
        tiers, ly = E.lookup_bags_c1c2(pair[0], pair[1], lo, [rq[:, t].long().contiguous() for t in range(T)], threshold=thr)
        return torch.stack(tiers, 1), torch.stack(ly)

    for i in range(40):
        resident = set(W._dump(a[0])) | set(W._dump(a[1]))
        rq = _dev(W._quiet_batch(rs, geom, resident, used, B))
        fa, fb = (bt, bags) if i < 20 or i % 2 == 0 else (bags, bt)
        (ta, ra), (tb, rb) = fa(a, rq), fb(b, rq)
        assert torch.equal(ta, tb), "call %d: codes" % (i + 1)
        assert int((ta == 0).sum()) == B
        assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)), "call %d: pooled[k][b] is not out[b, k]" % (i + 1)
        for k_ in (0, 1):
            assert a[k_].batch_stats() == b[k_].batch_stats(), "call %d: C%d counters" % (i + 1, k_ + 1)
        if i % 8 == 7:
            assert W._same_export(E.export_state_c1c2(*a), E.export_state_c1c2(*b)), "call %d: exports" % (i + 1)
    assert W._same_export(E.export_state_c1c2(*a), E.export_state_c1c2(*b))
    assert a[0].batch_stats()["n_flush"] == 0 and a[0].batch_stats()["n_evict"] + a[1].batch_stats()["n_evict"] > 0
    _no_index_error(E)


def test_twins_stay_equal_across_a_flush(E):
    """Both pairs start from one hand-made state whose C1 is full at priority T: the top bucket holds the whole capacity, so the
    first close asks for the flush and the next call of either form -- the (B, T) form on a, one index per bag on b -- runs it
    before its probe.  n_flush (>= 1), sizes, histograms and counters stay equal after every call; which top-priority ways leave
    is the flush's own business, so each pair's hits are only held to lie inside its own dump of before the call."""
    caps, thr, B = (64, 128), 2, 16
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    rows, keys = [], set()
    for es in range(geom.nset):                                    # per set 2 + 3 + 3 keys of the three tables
        for t, n in ((0, 2), (1, 3), (2, 3)):
            for r in [r for r in range(N_ROWS[t]) if geom.place(1, t, r)[0] == es][:n]:
                keys.add((t + 1, r))
                rows.append([1, t + 1, r, T, 0, 0])
    entries = np.array(rows, np.int64)
    a, b = _pair(E, caps, rule=False), _pair(E, caps)
    for p in (a, b):
        assert E.load_state_c1c2(p[0], p[1], {"entries": entries, "state": None}, strict=False)["placed"] == (caps[0], 0)
    rs = np.random.RandomState(4)
    lo = [torch.arange(B, dtype=torch.int64, device="cuda")] * T
    by_table = [[r for (t1, r) in sorted(keys) if t1 == t + 1] for t in range(T)]
    for call in range(3):
        rq = np.stack([rs.choice(by_table[t], B) for t in range(T)], 1).astype(np.int32)
        da, db = set(W._dump(a[0])), set(W._dump(b[0]))
        ta, _ = E.lookup_batch_c1c2(a[0], a[1], _dev(rq), threshold=thr)
        tb, _ = E.lookup_bags_c1c2(b[0], b[1], lo, [_dev(rq[:, t].astype(np.int64)) for t in range(T)], threshold=thr)
        for tiers, dump in ((ta.cpu().numpy(), da), (torch.stack(tb, 1).cpu().numpy(), db)):
            was = np.array([[(t + 1, int(rq[b_, t])) in dump for t in range(T)] for b_ in range(B)])
            assert not ((tiers == 1) & ~was).any() and not (tiers == 2).any()     # (a flush at entry only takes keys away)
        sa, sb = [c.batch_stats() for c in a], [c.batch_stats() for c in b]
        assert sa == sb, "call %d" % (call + 1)
    assert sa[0]["n_flush"] >= 1 and sa[0]["size"] < caps[0]


# ------------------------------------------------------------------------------------- 3. ragged, conflict-free, against the model
@pytest.mark.parametrize("caps", CAPS)
def test_ragged_conflict_free_stream_is_the_model(E, caps):
    """30 ragged calls of the model's conflict-free generator on a full pair: codes, pooled bits and -- after every call --
    every exported (tier, key, score) equal the model's.  (The model restates the route filter's hash: a C2-routed odd-table key
    whose word a C1-routed key stamped is in neither tier, there and here.)  Every sample names one new key, so agg_hit = T - 1
    everywhere, no priority reaches T and the flush -- whose victims the model does not restate -- never fires; the threshold
    alternates between T - 1 and T, so the new keys are routed on both sides of it."""
    B = 8
    _a, pair, geom, used, rs = _fill_twins(E, caps, 2)
    assert B <= geom.nset
    st = _state(E, geom, pair)
    dec1, dec2 = _tables(8, 36)[1], _tables(4, 36)[1]
    n_ins = 0
    for i in range(30):
        thr = T - 1 + (i & 1)
        off, idx = BP.conflict_free_call(rs, st, used, B, n_new=B, spread=True)
        j = BP.judge(st, B, off, idx, thr)
        assert BP.is_conflict_free(st, j) and (j.agg == T - 1).all()
        tiers, ly = _call(E, pair, off, idx, thr)
        for t in range(T):
            assert np.array_equal(tiers[t], j.code[t]), "call %d table %d: codes" % (i + 1, t)
        assert np.array_equal(_bits(ly), _bits(BP.pooled(j, idx, dec1, dec2, B))), "call %d: pooled" % (i + 1)
        BP.apply(st, j)
        n_ins += len(j.insert[0]) + len(j.insert[1])
        got = {(int(e[0]), int(e[1]), int(e[2]), int(e[3])) for e in E.export_state_c1c2(*pair)["entries"]}
        assert got == st.triples(), "call %d: %s" % (i + 1, sorted(got ^ st.triples())[:6])
    s1, s2 = pair[0].batch_stats(), pair[1].batch_stats()
    assert n_ins >= 30 and s1["n_flush"] == s2["n_flush"] == 0 and s1["n_evict"] + s2["n_evict"] > 0
    _no_index_error(E)


# --------------------------------------------------------------------------------------------------------- 4. ragged, contended
@pytest.mark.parametrize("caps,codecs,d", SHAPES)
def test_ragged_contended_calls_keep_the_invariants(E, caps, codecs, d):
    """Few rows per table (the calls draw from the first 30 / 120 / 300): many positions name one key, many new keys fall into one
    set, keys are routed both ways.  After every call no key is in both tiers, sizes stay within capacity, hist sums to size,
    every resident key was resident before or named by the call -- and codes and pooled are still exact, being functions of the
    snapshot and the input alone."""
    thr, B = 2, 48
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    pair = _pair(E, caps, codecs, d)
    rs = np.random.RandomState(caps[1] + d)
    dec1, dec2 = _tables(codecs[0], d)[1], _tables(codecs[1], d)[1]
    few = [30, 120, 300]
    st = BP.State(geom)
    for i in range(12):
        resident = sorted(set(st.keys(1)) | set(st.keys(2)))
        off, idx = _flat(_ragged(rs, resident, B, p_res=0.5, rows=few))
        j = BP.judge(st, B, off, idx, thr)
        tiers, ly = _call(E, pair, off, idx, thr)
        for t in range(T):
            assert np.array_equal(tiers[t], j.code[t]), "call %d table %d: codes" % (i + 1, t)
        assert np.array_equal(_bits(ly), _bits(BP.pooled(j, idx, dec1, dec2, B))), "call %d: pooled" % (i + 1)
        before = set(resident)
        st = _state(E, geom, pair)
        k1, k2 = set(st.keys(1)), set(st.keys(2))
        named = {(t + 1, int(r)) for t in range(T) for r in idx[t]}
        assert not (k1 & k2), "call %d: a key in both tiers" % (i + 1)
        assert (k1 | k2) <= (before | named), "call %d: a resident key nobody named" % (i + 1)
        for k_, keys in ((0, k1), (1, k2)):
            s = pair[k_].batch_stats()
            assert s["size"] == len(keys) <= caps[k_] and sum(s["hist"]) == s["size"], "call %d: C%d" % (i + 1, k_ + 1)
            assert all(0 <= e[2] <= T for e in st.slots[k_].values())
    assert len(k1) > 0 and len(k2) > 0
    _no_index_error(E)


# ------------------------------------------------------------------------------------------------------------ 5. the interact form
@pytest.mark.parametrize("caps,codecs,d", [((64, 128), (8, 4), 36), ((32, 128), (32, 8), 36), ((64, 96), (8, 4), 16)])
def test_interact_form(E, caps, codecs, d):
    """R against the fp64 interaction of the expected pooled block (the model's, bit-exact fp32) within the bound tests/_accuracy.py
    applies to evs_interact_dot; codes and the state after every call equal the pooled form's on a twin."""
    thr, B = 2, 24
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    a, b = _pair(E, caps, codecs, d), _pair(E, caps, codecs, d)
    rs = np.random.RandomState(d + caps[0])
    dec1, dec2 = _tables(codecs[0], d)[1], _tables(codecs[1], d)[1]
    st, used = BP.State(geom), set()
    for i in range(10):
        if i < 4:                                                   # the fill: fresh keys only, few per call
            off, idx = BP.conflict_free_call(rs, st, used, B, n_new=min(B, geom.nset))
        else:
            off, idx = BP.conflict_free_call(rs, st, used, B)
        j = BP.judge(st, B, off, idx, thr)
        x = rs.uniform(-1, 1, size=(B, d)).astype(np.float32)
        itself = bool(i & 1)
        lS_o, lS_i = [_dev(o) for o in off], [_dev(i_) for i_ in idx]
        ta, R = E.lookup_bags_interact_c1c2(a[0], a[1], lS_o, lS_i, _dev(x), threshold=thr, itself=itself)
        tb, _ly = E.lookup_bags_c1c2(b[0], b[1], lS_o, lS_i, threshold=thr)
        assert torch.equal(torch.cat(ta), torch.cat(tb)) and np.array_equal(torch.cat(ta).cpu().numpy(), np.concatenate(j.code))
        want = BP.pooled(j, idx, dec1, dec2, B).astype(np.float64)
        ref = acc.Reference(x, [(want[k], np.abs(want[k])) for k in range(T)], itself, 1)
        acc.check(R.cpu().numpy(), ref, "pair caps %s codecs %s d %d call %d" % (caps, codecs, d, i), "pair bags chain: pooling + dense interaction")
        assert W._same_export(E.export_state_c1c2(*a), E.export_state_c1c2(*b)), "call %d: state" % (i + 1)
        assert [c.batch_stats() for c in a] == [c.batch_stats() for c in b]
        st = _state(E, geom, a)
    assert len(st.keys(1)) > 0
    _no_index_error(E)


# ------------------------------------------------------------------------------------------------------------------- 6. refusals
def _probe_call(n_tables=T, B=4, row=0):
    """a tiny call every refusal is tried with: one index per bag, one row of every table -> (lS_o, lS_i, the (B, T) rows)"""
    lo = [torch.arange(B, dtype=torch.int64, device="cuda")] * n_tables
    li = [torch.full((B,), row, dtype=torch.int64, device="cuda")] * n_tables
    return lo, li, _dev(np.full((B, n_tables), row, np.int32))


def _refused(E, code, word, pair, x=None, B=4):
    """both forms refuse the pair with `code` and a message that holds `word`"""
    L = E._lib
    lo, li, _rq = _probe_call(pair[0].n_tables, B)
    x = torch.zeros((B, pair[0].dim), device="cuda") if x is None else x
    for fn in (lambda: E.lookup_bags_c1c2(pair[0], pair[1], lo, li), lambda: E.lookup_bags_interact_c1c2(pair[0], pair[1], lo, li, x)):
        with pytest.raises(L.EvsError) as ei:
            fn()
        assert ei.value.code == code and word in str(ei.value), str(ei.value)


def _still_serves(E, pair, dec=None, c3=None, row=0):
    """the pair serves lookup_batch_c1c2 afterwards: the second call finds what the first inserted, and the served row is its tier's"""
    _lo, _li, rq = _probe_call(pair[0].n_tables, row=row)
    for _ in range(2):
        tier, out = E.lookup_batch_c1c2(pair[0], pair[1], rq, c3=c3)
    assert bool((tier != 0).all())
    if dec is not None:
        assert np.array_equal(_bits(out[0, 1].cpu().numpy()), _bits(dec[int(tier[0, 1]) - 1][1][0]))


def _serves_alone(c):
    """a cache the (B, T) pair refuses too (an LRU tier, a fetch-first tier) still serves as what it is: a tier alone"""
    _lo, _li, rq = _probe_call(c.n_tables)
    for _ in range(2):
        hit, _out = c.lookup_batch(rq)
    assert bool(hit.all())


def test_refusals_leave_the_pair_usable(E):
    """Every point of the envelope that hangs on the two caches: the code, the cache named, and the pair serving
    lookup_batch_c1c2 afterwards (a tier the (B, T) pair refuses as well -- LRU, fetch-first -- serves lookup_batch alone)."""
    L = E._lib
    lo, li, rq = _probe_call()
    dec84 = (_tables(8, 36)[1], _tables(4, 36)[1])
    # the bag rule must be told to both tiers: the refusal names the one that lacks it
    for lacks in (0, 1):
        pair = _pair(E, (64, 128), rule=False)
        pair[1 - lacks].set_bag_rule("served-bags")
        _refused(E, L.EVS_EINVAL, "C%d has no bag rule" % (lacks + 1), pair)
        _still_serves(E, pair, dec84)
        pair[lacks].set_bag_rule("served-bags")                     # a started pair takes the bag form once both are told
        tiers, _ = E.lookup_bags_c1c2(pair[0], pair[1], lo, li)
        assert all(bool((t != 0).all()) for t in tiers)
    # an LRU tier, in either place
    for which in (0, 1):
        pair = list(_pair(E, (64, 128)))
        pair[which] = E.GpuCache("lru", (64, 128)[which], T, 36, (8, 4)[which])
        pair[which].set_backing(_tables((8, 4)[which], 36)[0])
        _refused(E, L.EVS_EINVAL, "C%d is an lru cache" % (which + 1), pair)
        _serves_alone(pair[0])
        _serves_alone(pair[1])
    # no shared set record: a tier would get fewer than 4 ways; plan-based and sampled pairs; tiers that started alone
    pair = _pair(E, (64, 16))
    _refused(E, L.EVS_EINVAL, "no shared set record", pair)
    _still_serves(E, pair, dec84)
    _refused(E, L.EVS_EINVAL, "set records", pair)                  # ... and started with records of their own since
    for policy in ("plan", "sampled"):
        for which in (0, 1):
            pair = _pair(E, (64, 128))
            pair[which].set_batch_policy(policy)
            _refused(E, L.EVS_EINVAL, policy, pair)
            _still_serves(E, pair, dec84)
            _refused(E, L.EVS_EINVAL, "set records", pair)
            _still_serves(E, pair, dec84)
    pair = _pair(E, (64, 128))
    pair[0].lookup_batch(rq)
    _refused(E, L.EVS_EINVAL, "set records", pair)
    _serves_alone(pair[0])
    # a pair of precisions the reference does not build
    pair = _pair(E, (64, 128), (8, 8))
    _refused(E, L.EVS_EINVAL, "8-bit C1 over a 8-bit C2", pair)
    _still_serves(E, pair, (_tables(8, 36)[1], _tables(8, 36)[1]))
    pair = _pair(E, (64, 128), (4, 8))
    _refused(E, L.EVS_EINVAL, "4-bit C1 over a 8-bit C2", pair)
    _still_serves(E, pair, (_tables(4, 36)[1], _tables(8, 36)[1]))
    # host-memory tables under a tier
    for which in (0, 1):
        pair = _pair(E, (64, 128))
        dev = _tables((8, 4)[which], 36)[0]
        pair[which].set_backing([t.cpu().pin_memory() for t in dev])
        _refused(E, L.EVS_ESTATE, "C%d sits over host-memory" % (which + 1), pair)
        pair[which].set_backing(dev)
        tiers, _ = E.lookup_bags_c1c2(pair[0], pair[1], lo, li)
        assert not torch.cat(tiers).any()
        _still_serves(E, pair, dec84)
    # fetch-first is a tier alone
    pair = _pair(E, (64, 128))
    pair[0].set_miss_order("fetch-first")
    _refused(E, L.EVS_EINVAL, "C1 runs fetch-first", pair)
    _serves_alone(pair[0])
    _serves_alone(pair[1])
    # a pair that has run as a triple: its evictions feed an alt-key tier the bag form does not have
    pair = _pair(E, (64, 128))
    alt = [torch.randint(0, 3, (n,), dtype=torch.int32, device="cuda") * 100 + (t % T) + 1 for t, n in enumerate(N_ROWS)]
    c3 = E.GpuAltKeyTier(64, alt)
    E.lookup_batch_c1c2c3(pair[0], pair[1], c3, rq)
    _refused(E, L.EVS_EINVAL, "C1 has run as a tier of a triple", pair)
    _still_serves(E, pair, c3=c3)
    # the same cache twice; tiers that do not agree (the wrapper's own check, then the library's)
    pair = _pair(E, (64, 128))
    _refused(E, L.EVS_EINVAL, "both tiers", (pair[0], pair[0]))
    with pytest.raises(ValueError):
        E.lookup_bags_c1c2(pair[0], _pair(E, (64, 128), d=16)[1], lo, li)
    _still_serves(E, pair, dec84)
    _no_index_error(E)


def _plain_pair(E, n_rows, d, codecs=(8, 4), caps=(64, 128)):
    """a pair over tables of any shape (random bytes / values: only codes are looked at)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(d)
    cs = []
    for cap, codec in zip(caps, codecs):
        c = E.GpuCache("evlfu", cap, len(n_rows), d, codec, "cpp")
        if codec == 32:
            c.set_backing([torch.rand((n, d), device="cuda", generator=g) for n in n_rows])
        else:
            c.set_backing([torch.randint(0, 256, (n, d * codec // 8), dtype=torch.uint8, device="cuda", generator=g) for n in n_rows])
        cs.append(c.set_bag_rule("served-bags"))
    return cs


def test_refusals_of_dim_and_feature_count(E):
    """dim must be a multiple of 4 up to 256 (both forms; d = 18 and d = 260 are caches evs_cache_create makes), the interact form
    additionally needs a fused-kernel dim and T + 1 <= 32 features.  All EVS_EINVAL before the device is touched; the pair serves
    lookup_batch_c1c2 afterwards, and the pooled form where only the interaction is out of reach."""
    L = E._lib
    B = 4
    st = torch.cuda.current_stream().cuda_stream
    # d = 18: the strides the wrappers would pass (18) are refused first, so the calls are made with padded ones
    pair = _plain_pair(E, N_ROWS, 18)
    lo, li, _rq = _probe_call()
    _B, idx_c, off_c, nnz_c, flat, _t, _keep = pair[0]._bags_call(lo, li)
    buf = torch.zeros((T, B, 20), device="cuda")
    assert L.lib().evs_cache_lookup_bags_c1c2(pair[0]._h, pair[1]._h, B, idx_c, off_c, nnz_c, buf.data_ptr(), B * 20, 20, flat.data_ptr(), 23, st) == L.EVS_EINVAL
    assert b"multiple of 4" in L.lib().evs_last_error() and b"18" in L.lib().evs_last_error()
    with pytest.raises(L.EvsError) as ei:
        E.lookup_bags_interact_c1c2(pair[0], pair[1], lo, li, torch.zeros((B, 20), device="cuda")[:, :18])
    assert ei.value.code == L.EVS_EINVAL and "multiple of 4" in str(ei.value)
    assert not buf.any()
    _still_serves(E, pair)
    # d = 260: past what a wave pools
    pair = _plain_pair(E, N_ROWS, 260, (32, 8))
    _refused(E, L.EVS_EINVAL, "multiple of 4 up to 256, not 260", pair)
    _still_serves(E, pair)
    # d = 20 pools but has no fused interaction
    assert not L.lib().evs_fused_dim_supported(20)
    pair = _plain_pair(E, N_ROWS, 20, (32, 8))
    with pytest.raises(L.EvsError) as ei:
        E.lookup_bags_interact_c1c2(pair[0], pair[1], lo, li, torch.zeros((B, 20), device="cuda"))
    assert ei.value.code == L.EVS_EINVAL and "interaction" in str(ei.value) and "d = 20" in str(ei.value)
    tiers, ly = E.lookup_bags_c1c2(pair[0], pair[1], lo, li)
    assert not torch.cat(tiers).any()
    _still_serves(E, pair)
    # T = 32 tables pool, but x + 32 features are more than the interaction takes.  (Row 1: of the 32 keys (table, 1) at most 6
    # share a C1 set of 8 ways; nine of the keys (table, 0) fall into one set, whose ninth is turned away.)
    pair = _plain_pair(E, [50] * 32, 16)
    assert max(np.bincount([P.Geometry(64, 128, [50] * 32).place(1, t, 1)[0] for t in range(32)])) <= 8
    lo32, li32, _rq = _probe_call(32, row=1)
    with pytest.raises(L.EvsError) as ei:
        E.lookup_bags_interact_c1c2(pair[0], pair[1], lo32, li32, torch.zeros((B, 16), device="cuda"))
    assert ei.value.code == L.EVS_EINVAL and "T = 32" in str(ei.value)
    tiers, ly = E.lookup_bags_c1c2(pair[0], pair[1], lo32, li32)
    assert len(tiers) == 32 and not torch.cat(tiers).any()
    tiers, ly = E.lookup_bags_c1c2(pair[0], pair[1], lo32, li32)
    assert bool(torch.cat(tiers).all())
    _still_serves(E, pair, row=1)
    _no_index_error(E)


def test_refusal_of_file_backed_tables(E, tmp_path):
    """a tier over file-backed tables: EVS_ESTATE naming it, and the pair serves lookup_batch_c1c2 (its plan-based chain)"""
    L = E._lib
    for which in (0, 1):
        codec = (8, 4)[which]
        paths = []
        for t, tab in enumerate(_tables(codec, 36)[0]):
            p = tmp_path / ("c%d-ev-table-%d.bin" % (which + 1, t + 1))
            tab.cpu().numpy().tofile(str(p))
            paths.append(str(p))
        ft = E.FileTier(paths, 36 * codec // 8, 1 << 30)
        pair = list(_pair(E, (64, 128)))
        pair[which] = E.GpuCache("evlfu", (64, 128)[which], T, 36, codec, "cpp").set_bag_rule("served-bags")
        pair[which].set_file_backing(ft)
        _refused(E, L.EVS_ESTATE, "C%d sits over host-memory / file-backed" % (which + 1), pair)
        _still_serves(E, pair, (_tables(8, 36)[1], _tables(4, 36)[1]))
        del pair
        ft.close()


def test_refusal_behind_the_process_wide_switch():
    """EVS_SA_PAIR=0 is read once per process, so the refusal is checked in a child (tests/_bag_pair_env_child.py)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EVS_SA_PAIR="0")
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_bag_pair_env_child.py")], env=env, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
