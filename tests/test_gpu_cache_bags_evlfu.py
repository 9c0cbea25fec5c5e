"""Ragged bags through the batched EvLFU cache tier (GpuCache.set_bag_rule("served-bags"), lookup_bags / lookup_bags_interact;
csrc/evs_cache_policy.hip: bags_probe_kernel<EVLFU>, bags_pool_kernel<.., EVLFU>, bags_raise_list_kernel, then
cache_batch_sa_list_kernel) held to the rule written down in include/evstore_hip.h at evs_cache_lookup_bags: equal to the
(B, T) chain with one index per bag, pinned position by position and priority by priority to the Python restatement
(tests/_bag_evlfu_model.py) on conflict-free ragged streams, held to the invariants on contended ones, the flush against a twin
cache driven through lookup_batch, and the pooled rows bit-equal to apply_emb over the backing tables everywhere."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _accuracy as acc
import _bag_evlfu_model as EM
import _bag_policy_model as BM
import _batched_policy_model as M

pytestmark = pytest.mark.gpu

N_ROWS = [2000] * 26
SHAPES = {"small": (1024, 4, 3, 300), "large": (2048, 8, 4, 200)}     # capacity, samples, largest bag, batches
SEED = 3                                                              # (tests/test_bag_evlfu_model.py: no flush on these)
KAGGLE_LIKE = [3000, 40, 20000, 700, 5, 9000, 1500, 12, 26000, 300, 8000, 64, 2200, 17000, 3, 450, 5000, 90, 13000,
               2, 7000, 30, 1000, 11000, 150, 4000]


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _stream(shape):
    cap, B, L, n_batches = SHAPES[shape]
    return EM.conflict_free_bag_stream(cap, N_ROWS, B, L, n_batches, SEED)[0]


@functools.lru_cache(maxsize=None)
def _tables(codec, n_rows=tuple(N_ROWS), seed=21, d=36):
    """-> (what set_backing takes (host arrays), the fp32 rows a lookup must return); tests/test_gpu_cache_bags.py::_tables"""
    from oracle import oracle as orc
    tabs = orc.kaggle_tables(list(n_rows), seed)
    if d != 36:
        tabs = [np.ascontiguousarray(t[:, :d]) for t in tabs]
    if codec == 32:
        return tabs, tabs
    raws = [orc.encode_table(np.clip(t * np.sqrt(len(t)), -1, 1), codec) for t in tabs]
    return raws, [orc.decode(a, codec, d) for a in raws]


def _cache(E, cap, T, d, codec, dev, rule="served-bags"):
    c = E.GpuCache("evlfu", cap, T, d, codec)
    c.set_backing(dev)
    return c.set_bag_rule(rule) if rule else c


def _dump(c):
    d = c.batch_dump()
    keys = [(int(t), int(r)) for _, t, r in d]
    assert len(set(keys)) == len(keys), "a key is resident twice"
    return {k: int(s) for k, (s, _, _) in zip(keys, d)}


def _hist_of(dump, T):
    return np.bincount(np.array(list(dump.values()), np.int64), minlength=T + 1).tolist()


def _upload(calls):
    """the offsets and indices of a list of calls as views of ONE device array each -> per call (lS_o, lS_i) lists"""
    flat = _dev(np.concatenate([a for off, idx in calls for a in list(off) + list(idx)] + [np.zeros(1, np.int64)]).astype(np.int64))
    out, at = [], 0
    for off, idx in calls:
        views = []
        for a in list(off) + list(idx):
            views.append(flat[at:at + len(a)])
            at += len(a)
        out.append((views[:len(off)], views[len(off):]))
    return out


def _np_flags(hits):
    return [h.cpu().numpy().astype(bool) for h in hits]


def _np_pooled(ly):
    return torch.stack([t for t in ly]).cpu().numpy()


def _apply_emb(E, ev, lS_o, lS_i):
    return _np_pooled(E.apply_emb(lS_o, lS_i, ev, lazy=False))


def _bit_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _index_error_once(E):
    L = E._lib
    assert L.lib().evs_check_index_errors(None) == L.EVS_EINDEX
    assert L.lib().evs_check_index_errors(None) == 0


def _refused(E, code, word, fn):
    with pytest.raises(E._lib.EvsError) as ei:
        fn()
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


# ------------------------------------------------------------------------------------------------ 1. the rule's setter, refusals
def test_bag_rule_setter_and_refusals(E):
    L = E._lib
    n_rows = [300] * 26
    tabs, _ = _tables(32, tuple(n_rows), 4)
    dev = [_dev(t) for t in tabs]
    rq = _dev(np.zeros((4, 26), np.int32))
    lo = [torch.arange(4, dtype=torch.int64, device="cuda")] * 26
    li = [torch.zeros(4, dtype=torch.int64, device="cuda")] * 26
    x = torch.zeros((4, 36), device="cuda")

    def still_serves(c):
        hit, out = c.lookup_batch(rq)
        assert _bit_equal(out.cpu().numpy()[:, 3], tabs[3][[0] * 4])

    # the default refuses; the setter is what turns the bag form on, and off again
    e = _cache(E, 512, 26, 36, 32, dev, rule=None)
    _refused(E, L.EVS_EINVAL, "evlfu", lambda: e.lookup_bags(lo, li))
    _refused(E, L.EVS_EINVAL, "evlfu", lambda: e.lookup_bags_interact(lo, li, x))
    assert L.lib().evs_cache_set_bag_rule(e._h, 2) == L.EVS_EINVAL and b"evlfu" in L.lib().evs_last_error()
    assert L.lib().evs_cache_set_bag_rule(e._h, -1) == L.EVS_EINVAL
    assert L.lib().evs_cache_set_bag_rule(None, 1) == L.EVS_EINVAL
    with pytest.raises(ValueError):
        e.set_bag_rule("hit-keys")
    assert e.set_bag_rule("served-bags") is e
    hits, ly = e.lookup_bags(lo, li)
    assert not torch.cat(hits).any() and _bit_equal(ly[3].cpu().numpy(), tabs[3][[0] * 4])
    hits, R = e.lookup_bags_interact(lo, li, x)
    assert torch.cat(hits).all()
    still_serves(e)
    e.set_bag_rule(None)
    _refused(E, L.EVS_EINVAL, "evlfu", lambda: e.lookup_bags(lo, li))
    still_serves(e)

    # LRU / LFU need no rule: 1 refused with the policy named, 0 accepted, their bag form as it was
    for policy in ("lru", "lfu"):
        c = E.GpuCache(policy, 512, 26, 36, 32)
        c.set_backing(dev)
        _refused(E, L.EVS_EINVAL, policy, lambda: c.set_bag_rule("served-bags"))
        assert c.set_bag_rule(None) is c
        hits, ly = c.lookup_bags(lo, li)
        assert _bit_equal(ly[3].cpu().numpy(), tabs[3][[0] * 4])

    # plan / sampled, explicit or by the geometry fall-back (a capacity below one set resolves to sampled): refused, and the
    # cache keeps serving lookup_batch under its policy
    for policy, cap in (("plan", 512), ("sampled", 512), (None, 7)):
        c = _cache(E, cap, 26, 36, 32, dev)
        if policy:
            c.set_batch_policy(policy)
        _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_bags(lo, li))
        _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_bags_interact(lo, li, x))
        if policy:
            still_serves(c)
            still_serves(c)
        else:                                                   # (seven entries: the exact engine, as test_gpu_cache_bags.py checks it)
            hit, out = c.request(rq)
            assert _bit_equal(out.cpu().numpy()[:, 3], tabs[3][[0] * 4])
    # a universe of 2^32 rows (declared: nothing is read before the refusal) has no set-associative form either
    c = _cache(E, 512, 26, 36, 32, dev)
    ptrs = (C.c_void_p * 26)(*[t.data_ptr() for t in dev])
    big = (C.c_int64 * 26)(*([1 << 31, 1 << 31] + [300] * 24))
    L.check(L.lib().evs_cache_set_backing(c._h, ptrs, big))
    _refused(E, L.EVS_EINVAL, "evlfu", lambda: c.lookup_bags(lo, li))
    c.set_backing(dev)                                          # the refusal resolved nothing for good: the true sizes are served
    hits, ly = c.lookup_bags(lo, li)
    assert _bit_equal(ly[3].cpu().numpy(), tabs[3][[0] * 4]) and _dump(c) == {(k + 1, 0): 0 for k in range(26)}

    # host-memory tables, the exact path: today's codes
    c = E.GpuCache("evlfu", 512, 26, 36, 32)
    c.set_backing([torch.from_numpy(np.ascontiguousarray(t)).pin_memory() for t in tabs])
    c.set_bag_rule("served-bags")
    _refused(E, L.EVS_ESTATE, "evlfu", lambda: c.lookup_bags(lo, li))
    c.set_backing(dev)
    hits, ly = c.lookup_bags(lo, li)
    assert _bit_equal(ly[3].cpu().numpy(), tabs[3][[0] * 4])
    c = _cache(E, 512, 26, 36, 32, dev)
    c.request(rq)
    _refused(E, L.EVS_ESTATE, "evlfu", lambda: c.lookup_bags(lo, li))
    hit, out = c.request(rq)
    assert hit.all() and _bit_equal(out.cpu().numpy()[:, 3], tabs[3][[0] * 4])


@pytest.mark.parametrize("switch,value,want", [("EVS_SA_WAYS", "16", "ways"), ("EVS_CACHE_POLICY", "plan", "plan"),
                                               ("EVS_CACHE_POLICY", "sampled", "sampled")])
def test_refusals_behind_a_process_wide_switch(switch, value, want):
    """16-way sets and a plan / sampled policy that comes from EVS_CACHE_POLICY: both switches are read once per process, so
    the refusal (EVS_EINVAL, the policy named, lookup_batch still serving) is checked in a child (tests/_bag_evlfu_env_child.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("EVS_SA_WAYS", "EVS_CACHE_POLICY")}
    env[switch] = value
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_bag_evlfu_env_child.py"), want], env=env, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


# ----------------------------------------------------------------------------------- 2. one index per bag = the (B, T) chain
def test_one_index_per_bag_is_lookup_batch(E):
    """Twin caches over one conflict-free stream: lookup_bags with arange offsets against lookup_batch as a chain of launches
    (set_inline_update(False)) -- flags, rows bit for bit, the dump and every counter, hist included, after every batch."""
    cap, B, n_batches = 512, 4, 400
    reqs, _, model = EM.conflict_free_rows_stream(cap, N_ROWS, B, n_batches, SEED)
    tabs, _ = _tables(32)
    dev = [_dev(t) for t in tabs]
    a = _cache(E, cap, 26, 36, 32, dev)
    b = _cache(E, cap, 26, 36, 32, dev, rule=None).set_inline_update(False)
    r32 = _dev(reqs.reshape(-1, 26))
    li_all = _dev(reqs.transpose(0, 2, 1).astype(np.int64))          # (batches, T, B)
    lo = torch.arange(B, dtype=torch.int64, device="cuda").repeat(26, 1)
    for i in range(n_batches):
        hits, ly = a.lookup_bags(lo, li_all[i])
        hit, out = b.lookup_batch(r32[i * B:(i + 1) * B])
        assert torch.equal(torch.stack(hits, 1), hit), "batch %d: flags" % (i + 1)
        assert torch.equal(torch.stack(ly, 1).view(torch.int32), out.view(torch.int32)), "batch %d: rows" % (i + 1)
        assert _dump(a) == _dump(b), "batch %d: resident set / priorities" % (i + 1)
        assert a.batch_stats() == b.batch_stats(), "batch %d: counters" % (i + 1)
    st = a.batch_stats()
    assert _dump(a) == model.resident()
    assert st["n_requests"] == B * n_batches and st["n_evict"] == model.n_evict > 5 * cap and st["n_flush"] == 0


# ------------------------------------------------------------------------------------------ 3. pinned on conflict-free streams
@pytest.mark.parametrize("shape,codec", [("small", 32), ("large", 32), ("small", 8)])
def test_rule_pinned_on_ragged_conflict_free_streams(E, shape, codec):
    """No call brings two new keys to one set and no flush fires, so the rule is deterministic: every flag equals the model's
    position by position, the dump IS the model's {key: priority}, the counters and the histogram are the model's, and the
    pooled rows are bit-equal to apply_emb over the same raw tables -- after every batch."""
    cap, B, L, n_batches = SHAPES[shape]
    calls = _stream(shape)
    raws, _ = _tables(codec)
    dev = [_dev(r) for r in raws]
    ev = E.EVTables(dev, 36, codec)
    c = _cache(E, cap, 26, 36, codec, dev)
    model = EM.BagEvLFUModel(cap, N_ROWS)
    on_dev = _upload([(off, idx) for off, idx, _ in calls])
    for i, (off, idx, want) in enumerate(calls):
        lS_o, lS_i = on_dev[i]
        hits, ly = c.lookup_bags(lS_o, lS_i)
        again = model.batch_bags(off, idx)
        got = _np_flags(hits)
        for k in range(26):
            assert np.array_equal(again[k], want[k])
            assert np.array_equal(got[k], want[k]), "batch %d table %d: %d flags differ from the model" % (i + 1, k, int((got[k] != want[k]).sum()))
        assert _bit_equal(_np_pooled(ly), _apply_emb(E, ev, lS_o, lS_i)), "batch %d: pooled rows" % (i + 1)
        assert _dump(c) == model.resident(), "batch %d: resident set / priorities" % (i + 1)
        st = c.batch_stats()
        assert (st["size"], st["n_hits"], st["n_requests"], st["n_evict"], st["n_perfect_hits"]) == \
            (model.size(), model.n_hits, model.n_requests, model.n_evict, model.n_perfect), "batch %d: counters" % (i + 1)
        assert st["hist"] == model.hist() and st["n_flush"] == 0, "batch %d: histogram" % (i + 1)
    assert model.n_evict > 2 * cap and model.size() == cap


def test_counters_folded_across_pending_batches(E):
    """The same stream with nothing read between the calls: the counters of several batches wait in the replica rows and are
    folded by the close every eighth call -- after 8, 13 and 60 calls the dump, the counters and the histogram are the model's."""
    cap, B, L, _ = SHAPES["small"]
    calls = _stream("small")[:60]
    raws, _ = _tables(32)
    dev = [_dev(r) for r in raws]
    c = _cache(E, cap, 26, 36, 32, dev)
    model = EM.BagEvLFUModel(cap, N_ROWS)
    on_dev = _upload([(off, idx) for off, idx, _ in calls])
    for i, (off, idx, _) in enumerate(calls):
        c.lookup_bags(*on_dev[i])
        model.batch_bags(off, idx)
        if i + 1 in (8, 13, 60):
            st = c.batch_stats()
            assert (st["size"], st["n_hits"], st["n_requests"], st["n_evict"], st["n_perfect_hits"], st["hist"], st["n_flush"]) == \
                (model.size(), model.n_hits, model.n_requests, model.n_evict, model.n_perfect, model.hist(), 0), "after %d calls" % (i + 1)
            assert _dump(c) == model.resident(), "after %d calls" % (i + 1)


# ----------------------------------------------------------------------------------- 4. shapes at which the kernels can go wrong
def _edge_batch(T, B, n_rows, rs):
    """One call with: an empty first and an empty last bag (table 0), a table without indices (table 1), a bag of 130 indices
    beside bags of 0 .. 10 (table T - 1), last bags that run to nnz, one key three times inside a bag and in another sample's
    bag, the indices -1 and n_rows[k]; T > 3: trailing positions no bag covers (table 3, or 2 when T = 4: three more indices
    and a last offset past nnz -- the last bag and the one in front of it are malformed, hence empty, and everything from the
    latter's start on is uncovered) and (B >= 5) a backwards offset in table 2 -- bag 1 = [.., 10^6) and bag 2 = [10^6, ..) are
    both empty, the positions between them uncovered.  No position is covered twice.  -> (offsets, indices)"""
    off, idx = [], []
    for k in range(T):
        sizes = rs.randint(0, 11, B)
        if k == 0:
            sizes[0] = sizes[-1] = 0
        elif k == 1:
            sizes[:] = 0
        else:
            sizes[-1] = max(sizes[-1], 1)
        if k == T - 1:
            sizes[B // 2] = 130
        bags = [rs.randint(0, n_rows[k], n).astype(np.int64) for n in sizes]
        if k == T - 1:
            hot = 7 % n_rows[k]
            bags[B // 2][[3, 60, 129]] = hot
            bags[-1][0] = hot
            bags[B // 2][[10, 11]] = [-1, n_rows[k]]
        off.append(np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int64))
        idx.append(np.concatenate(bags).astype(np.int64) if sizes.sum() else np.zeros(0, np.int64))
    if T > 3:
        if B >= 5:
            off[2][2] = 10 ** 6
        ku = 3 if T > 4 else 2
        idx[ku] = np.concatenate([idx[ku], rs.randint(0, n_rows[ku], 3)]).astype(np.int64)
        off[ku][-1] = len(idx[ku]) + 5                          # the last bag starts past nnz: empty, as is the bag in front of it
    return off, idx


def _edge_tables(E, T, d, codec, n_rows, tiny):
    if tiny:
        g = torch.Generator(device="cuda")
        g.manual_seed(9)
        dev = [torch.empty(n, d, device="cuda").uniform_(-1, 1, generator=g) for n in n_rows]
        return dev
    raws, _ = _tables(codec, tuple(n_rows), 5, d)
    return [_dev(r) for r in raws]


@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("T,d,codec,geom", [(26, 36, 32, None), (3, 16, 8, None), (26, 16, 4, None), (3, 36, 16, None), (4, 36, 32, "tiny")])
def test_shapes_and_edge_cases(E, T, d, codec, geom, B):
    """Flags equal to residency from the dump taken before the call, pooled output bit-equal to apply_emb, the counters and
    every priority equal to the model's (the caches are large enough that no set sees nine keys: nothing is evicted or turned
    away, so the rule is deterministic) over three calls -- a fresh cache, the same input again, a fresh draw -- with every
    edge of _edge_batch in each call.  `tiny` (2 sets, no two-copy arena, 4 stamp bits) evicts: invariants instead of the pin."""
    if geom:
        cap, n_rows, _ = M.WRAP_GEOMETRIES[geom]
        assert M.stamp_bits_of("evlfu", cap, n_rows)[1] == 0 and len(n_rows) == T     # one arena row per way
    else:
        n_rows = tuple(400 + 13 * k for k in range(T))
        cap = 65536 if T == 26 else 8192
    dev = _edge_tables(E, T, d, codec, n_rows, bool(geom))
    ev = E.EVTables(dev, d, codec)
    c = _cache(E, cap, T, d, codec, dev)
    model = EM.BagEvLFUModel(cap, n_rows)
    rs = np.random.RandomState(1000 * T + 10 * d + B)
    first = _edge_batch(T, B, n_rows, rs)
    judge = EM.BagEvLFUModel(cap, n_rows).judge
    resident, n_hits, n_perfect = {}, 0, 0
    for call, (off, idx) in enumerate([first, first, _edge_batch(T, B, n_rows, rs)]):
        lS_o, lS_i = [_dev(o) for o in off], [_dev(i) for i in idx]
        want_pooled = _apply_emb(E, ev, lS_o, lS_i)
        _index_error_once(E)
        hits, ly = c.lookup_bags(lS_o, lS_i)
        _index_error_once(E)
        got = _np_flags(hits)
        assert [len(g_) for g_ in got] == [len(i) for i in idx]
        for k in range(T):
            want = np.array([(k + 1, int(r)) in resident for r in idx[k]], bool)
            assert np.array_equal(got[k], want), "call %d table %d: flags != residency at arrival" % (call, k)
        pooled = _np_pooled(ly)
        assert _bit_equal(pooled, want_pooled), "call %d: pooled rows" % call
        assert not pooled[0, 0].any() and not pooled[0, -1].any() and not pooled[1].any()
        if T > 3:
            assert not pooled[3 if T > 4 else 2, -1].any()
        after = _dump(c)
        st = c.batch_stats()
        n_hits += int(sum(g_.sum() for g_ in got))
        agg, lookups, _ = judge(off, idx, got)
        n_perfect += int(((lookups > 0) & (agg == T)).sum())
        assert (T, -1) not in after and (T, n_rows[T - 1]) not in after
        assert st["hist"] == _hist_of(after, T) and st["size"] == len(after) <= cap and max(after.values()) <= T
        assert (st["n_hits"], st["n_perfect_hits"], st["n_requests"], st["n_flush"]) == (n_hits, n_perfect, (call + 1) * B, 0)
        assert all(after[k] >= p for k, p in resident.items() if k in after), "call %d: a priority fell" % call
        if not geom:
            model.batch_bags(off, idx)
            assert model.n_evict == 0 and model.n_turned == 0 and model.n_perfect == n_perfect
            assert after == model.resident(), "call %d: resident set / priorities" % call
        resident = after
    assert n_hits > 0


# -------------------------------------------------------------------------------------------------------- 5. contended batches
def _contended_calls(n_rows, B, max_bag, n_batches, seed, alpha=1.15):
    """Zipf bags of 0 .. max_bag indices per (sample, table), 30 % of the samples replaced by one of 64 hot samples"""
    rs = np.random.RandomState(seed)
    T = len(n_rows)
    perms = [rs.permutation(n) for n in n_rows]

    def sample():
        return [M.zipf_rows(rs, n_rows[t], rs.randint(0, max_bag + 1), alpha, perms[t]).astype(np.int64) for t in range(T)]
    hot = [sample() for _ in range(64)]
    calls = []
    for _ in range(n_batches):
        samples = [hot[rs.randint(0, 64)] if rs.rand() < 0.3 else sample() for _ in range(B)]
        idx = [np.concatenate([s[t] for s in samples]).astype(np.int64) for t in range(T)]
        off = [np.concatenate([[0], np.cumsum([len(s[t]) for s in samples[:-1]])]).astype(np.int64) for t in range(T)]
        calls.append((off, idx))
    return calls


@pytest.mark.parametrize("cap_frac", [0.02, 0.10])
def test_invariants_on_contended_batches(E, cap_frac):
    """Many new keys per set, hot keys named by many samples: which key takes which way depends on timing, the invariants do
    not -- flags = residency in the dump taken before, no key twice, size <= capacity, a key resident before and after never
    loses priority, priorities <= T, hist = the dump's histogram, n_hits and n_perfect_hits as the flags give them -- and
    the pooled rows stay bit-equal to apply_emb.  (A flush may fire here; it removes keys, it lowers none.)"""
    n_rows = KAGGLE_LIKE
    tabs, _ = _tables(32, tuple(n_rows))
    dev = [_dev(t) for t in tabs]
    ev = E.EVTables(dev, 36, 32)
    cap = int(cap_frac * sum(n_rows))
    calls = _contended_calls(n_rows, 64, 6, 48, 2)
    on_dev = _upload(calls)
    c = _cache(E, cap, 26, 36, 32, dev)
    judge = EM.BagEvLFUModel(cap, n_rows).judge
    resident, hits_total, perfect_total, raised = {}, 0, 0, 0
    for i, (off, idx) in enumerate(calls):
        lS_o, lS_i = on_dev[i]
        hits, ly = c.lookup_bags(lS_o, lS_i)
        flags = _np_flags(hits)
        got = np.concatenate(flags)
        keys = BM.keys_of(idx)
        assert np.array_equal(got, np.array([k in resident for k in keys], bool)), "batch %d: flags != residency at arrival" % i
        assert _bit_equal(_np_pooled(ly), _apply_emb(E, ev, lS_o, lS_i)), "batch %d: pooled rows" % i
        after = _dump(c)
        st = c.batch_stats()
        assert len(after) == st["size"] <= cap and st["hist"] == _hist_of(after, 26) and max(after.values()) <= 26
        assert all(after[k] >= p for k, p in resident.items() if k in after), "batch %d: a priority fell" % i
        raised += sum(1 for k, p in resident.items() if k in after and after[k] > p)
        agg, lookups, _ = judge(off, idx, flags)
        hits_total += int(got.sum())
        perfect_total += int(((lookups > 0) & (agg == 26)).sum())
        assert (st["n_hits"], st["n_perfect_hits"], st["n_requests"]) == (hits_total, perfect_total, 64 * (i + 1)), "batch %d: counters" % i
        if st["n_flush"] == 0:
            # every hit way carries at least the count of the samples that name it; a missed key that came in, exactly the largest
            _, _, pos_sample = judge(off, idx, flags)
            at, came_at = 0, {}
            for k in range(26):
                for p in range(len(idx[k])):
                    key, a = keys[at + p], int(agg[pos_sample[k][p]]) if pos_sample[k][p] >= 0 else 0
                    if got[at + p]:
                        assert key not in after or after[key] >= a, "batch %d: a hit way below its sample's count" % i
                    elif key[1] >= 0:
                        came_at[key] = max(came_at.get(key, 0), a)
                at += len(idx[k])
            assert all(after[key] == a for key, a in came_at.items() if key in after), "batch %d: a new key not at its largest count" % i
        resident = after
    assert hits_total > 0 and raised > 0
    print("evlfu cap %d: hit rate %.4f, perfect samples %d, flushes %d" % (cap, hits_total / sum(len(k) for _, ix in calls for k in ix),
                                                                            perfect_total, c.batch_stats()["n_flush"]))


# ------------------------------------------------------------------------------------------------------------------ 6. the flush
def test_flush_fires_as_in_the_bt_chain(E):
    """T = 4, capacity 64 = 8 sets of 8 ways, 64 distinct keys chosen so that every set receives exactly eight.  The same
    one-index-per-bag call twice: the first fills every way at priority 0, the second finds all and raises every way to T -- the
    top bucket holds the whole capacity, the close asks for the flush and batch_stats runs it.  A twin cache driven through
    lookup_batch is held against it: the same n_flush (>= 1), size and histogram; the call after that has flags = residency."""
    T, cap, B, n_rows = 4, 64, 16, [500] * 4
    nset, bits = M.geometry(cap, n_rows)
    reqs = np.zeros((B, T), np.int32)
    for t in range(T):
        rows = np.arange(n_rows[t])
        ss = M.set_of(t, rows, nset, n_rows, bits)
        reqs[:, t] = np.concatenate([rows[ss == s][:2] for s in range(nset)])       # two rows of every set per table
    assert (np.bincount(M.set_of(np.broadcast_to(np.arange(T), reqs.shape), reqs, nset, n_rows, bits).ravel(), minlength=nset) == 8).all()
    tabs, _ = _tables(32, tuple(n_rows), 6)
    dev = [_dev(t) for t in tabs]
    a = _cache(E, cap, T, 36, 32, dev)
    b = _cache(E, cap, T, 36, 32, dev, rule=None).set_inline_update(False)
    off, idx = EM.one_per_bag(reqs)
    lS_o, lS_i, r32 = [_dev(o) for o in off], [_dev(i) for i in idx], _dev(reqs)
    for call in range(2):
        hits, _ = a.lookup_bags(lS_o, lS_i)
        hit, _ = b.lookup_batch(r32)
        assert torch.equal(torch.stack(hits, 1), hit) and bool(hit.all()) == (call == 1)
        if call == 0:
            da = _dump(a)
            assert da == _dump(b) and len(da) == cap and set(da.values()) == {0}
    sa, sb = a.batch_stats(), b.batch_stats()
    assert sa["n_flush"] == sb["n_flush"] >= 1
    assert (sa["size"], sa["hist"], sa["n_perfect_hits"], sa["n_hits"]) == (sb["size"], sb["hist"], sb["n_perfect_hits"], sb["n_hits"])
    assert sa["n_perfect_hits"] == B and sa["size"] < cap
    da = _dump(a)
    assert set(da.values()) == {T} and sa["hist"] == _hist_of(da, T)
    hits, ly = a.lookup_bags(lS_o, lS_i)
    got = torch.stack(hits, 1).cpu().numpy().astype(bool)
    assert np.array_equal(got, np.array([[(t + 1, int(reqs[b_, t])) in da for t in range(T)] for b_ in range(B)]))
    assert not got.all() and _bit_equal(_np_pooled(ly), np.stack([tabs[t][reqs[:, t]] for t in range(T)]))


# ------------------------------------------------------------------------------------------------------ 7. the interaction form
@pytest.mark.parametrize("codec", [32, 8])
def test_lookup_bags_interact(E, codec):
    """probe -> pooling -> the dense interaction -> raise + list -> insert: R against float64 over the true rows
    (tests/_accuracy.py), itself on and off; flags, dump and counters equal to lookup_bags' on a twin cache and to the model
    (the stream is conflict-free)."""
    cap, T, d, B = 1024, 26, 36, 300
    raws, tabs = _tables(codec)
    rs = np.random.RandomState(11)
    perms = [rs.permutation(n) for n in N_ROWS]
    model = EM.BagEvLFUModel(cap, N_ROWS)
    backing = [_dev(r) for r in raws]
    a, b = _cache(E, cap, T, d, codec, backing), _cache(E, cap, T, d, codec, backing)
    x0 = torch.zeros((8, d), device="cuda")
    for i in range(30):
        off, idx, want, _ = BM.conflict_free_bags(model, rs, perms, 8, 4)
        lS_o, lS_i = [_dev(o) for o in off], [_dev(i_) for i_ in idx]
        ha, _ = a.lookup_bags_interact(lS_o, lS_i, x0)
        hb, _ = b.lookup_bags(lS_o, lS_i)
        assert torch.equal(torch.cat(ha), torch.cat(hb)) and np.array_equal(torch.cat(ha).cpu().numpy().astype(bool), np.concatenate(want))
    for i in range(4):
        off, idx, want, _ = BM.conflict_free_bags(model, rs, perms, B, 4)
        lS_o, lS_i = [_dev(o) for o in off], [_dev(i_) for i_ in idx]
        x = rs.uniform(-1, 1, size=(B, d)).astype(np.float32)
        ha, R = a.lookup_bags_interact(lS_o, lS_i, _dev(x), itself=bool(i & 1))
        hb, _ = b.lookup_bags(lS_o, lS_i)
        assert torch.equal(torch.cat(ha), torch.cat(hb)) and np.array_equal(torch.cat(ha).cpu().numpy().astype(bool), np.concatenate(want))
        ref = acc.reference_from_bags(x, tabs, off, idx, bool(i & 1))
        acc.check(R.cpu().numpy(), ref, "evlfu codec %d batch %d" % (codec, i), "bags chain: pooling + dense interaction, codec %d" % codec)
        if model.top_bucket() < int(0.95 * cap):               # (no flush: the priorities are pinned)
            assert _dump(a) == _dump(b) == model.resident()
            assert a.batch_stats() == b.batch_stats()
    assert model.n_evict > 0


# ------------------------------------------------------------------------------------------------------- 8. mixing, row updates
def test_the_forms_alternate_on_one_cache(E):
    """lookup_bags, lookup_interact (the default inline setting: its update runs inside the probe launch) and
    lookup_bags_interact in turn on one cache: they share the batch stamp and the counters.  After every call: no key twice,
    size <= capacity, priorities never fall and stay <= T, hist = the dump's histogram; the bag calls' flags are residency at
    arrival and their pooled rows exact."""
    cap, T, d, B = 1024, 26, 36, 32
    tabs, _ = _tables(32)
    dev = [_dev(t) for t in tabs]
    ev = E.EVTables(dev, d, 32)
    c = _cache(E, cap, T, d, 32, dev)
    rs = np.random.RandomState(8)
    perms = [rs.permutation(n) for n in N_ROWS]
    calls = _contended_calls(N_ROWS, B, 3, 40, 5, alpha=1.3)
    resident, n_req = {}, 0
    for i, (off, idx) in enumerate(calls):
        x = _dev(rs.uniform(-1, 1, size=(B, d)).astype(np.float32))
        if i % 3 == 1:
            rq = np.stack([M.zipf_rows(rs, N_ROWS[t], B, 1.3, perms[t]) for t in range(T)], 1).astype(np.int32)
            hit, R = c.lookup_interact(_dev(rq), x)
            hit = hit.cpu().numpy().astype(bool)
            was = np.array([[(t + 1, int(rq[b, t])) in resident for t in range(T)] for b in range(B)])
            assert not (hit & ~was).any(), "call %d: a hit flag on a key that was not resident" % i      # (inline: 1 => resident at arrival)
            o1, i1 = EM.one_per_bag(rq)
            acc.check(R.cpu().numpy(), acc.reference_from_bags(x.cpu().numpy(), tabs, o1, i1, False), "call %d" % i, "lookup_interact between bag calls")
        else:
            lS_o, lS_i = [_dev(o) for o in off], [_dev(i_) for i_ in idx]
            if i % 3 == 0:
                hits, ly = c.lookup_bags(lS_o, lS_i)
                assert _bit_equal(_np_pooled(ly), _apply_emb(E, ev, lS_o, lS_i)), "call %d: pooled rows" % i
            else:
                hits, R = c.lookup_bags_interact(lS_o, lS_i, x)
                acc.check(R.cpu().numpy(), acc.reference_from_bags(x.cpu().numpy(), tabs, off, idx, False), "call %d" % i,
                          "bags chain: pooling + dense interaction, codec 32")
            got = np.concatenate(_np_flags(hits))
            assert np.array_equal(got, np.array([k in resident for k in BM.keys_of(idx)], bool)), "call %d: flags != residency at arrival" % i
        n_req += B
        after = _dump(c)
        st = c.batch_stats()
        assert st["size"] == len(after) <= cap and st["hist"] == _hist_of(after, T) and max(after.values()) <= T
        assert st["n_requests"] == n_req
        assert all(after[k] >= p for k, p in resident.items() if k in after), "call %d: a priority fell" % i
        resident = after
    assert c.batch_stats()["n_evict"] > 0


def test_update_rows_between_two_bag_calls(E):
    """update_rows between two lookup_bags calls: the next call serves the new vectors from the arena (flag 1, new bits)"""
    n_rows = [300] * 26
    tabs = [t.copy() for t in _tables(32, tuple(n_rows), 8)[0]]
    dev = [_dev(t) for t in tabs]
    c = _cache(E, 16384, 26, 36, 32, dev)
    rs = np.random.RandomState(1)
    B = 20
    idx = [np.concatenate([[k % 100], rs.randint(0, 100, 3 * B - 1)]).astype(np.int64) for k in range(26)]
    off = [np.concatenate([[0, 1], np.arange(3, 3 * B - 3, 3)]).astype(np.int64)[:B] for _ in range(26)]
    lS_o, lS_i = [_dev(o) for o in off], [_dev(i) for i in idx]
    hits, _ = c.lookup_bags(lS_o, lS_i)
    assert not torch.cat(hits).any()
    keys = np.array([[k, k % 100] for k in range(26)], np.int64)
    vals = rs.uniform(-1, 1, size=(26, 36)).astype(np.float32)
    assert c.update_rows(keys, vals, count=True) == 26
    for (t, row), v in zip(keys, vals):
        tabs[t][row] = v
    hits, ly = c.lookup_bags(lS_o, lS_i)
    assert torch.cat(hits).all()
    pooled = _np_pooled(ly)
    assert _bit_equal(pooled[:, 0, :], vals)
    assert _bit_equal(pooled, _apply_emb(E, E.EVTables(dev, 36, 32), lS_o, lS_i))
    assert set(_dump(c).values()) == {26} and c.batch_stats()["n_perfect_hits"] == B
