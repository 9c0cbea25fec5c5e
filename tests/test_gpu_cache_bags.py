"""Ragged bags through the batched LRU / LFU cache tier (GpuCache.lookup_bags / lookup_bags_interact;
csrc/evs_cache_policy.hip: bags_probe_kernel, bags_pool_kernel) held to the rule written down in include/evstore_hip.h at
evs_cache_lookup_bags: equal to the (B, T) path with one index per bag, pinned position by position and way by way to the
Python restatement (tests/_bag_policy_model.py) on conflict-free ragged streams, held to the invariants on contended ones, and
the pooled rows bit-equal to apply_emb over the backing tables everywhere."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _accuracy as acc
import _bag_policy_model as BM
import _batched_policy_model as M

pytestmark = pytest.mark.gpu

N_ROWS = [2000] * 26
SHAPES = {"small": (1024, 4, 3, 300), "large": (2048, 8, 4, 200)}     # capacity, samples, largest bag, batches
KAGGLE_LIKE = [3000, 40, 20000, 700, 5, 9000, 1500, 12, 26000, 300, 8000, 64, 2200, 17000, 3, 450, 5000, 90, 13000,
               2, 7000, 30, 1000, 11000, 150, 4000]


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _stream(policy, shape):
    cap, B, L, n_batches = SHAPES[shape]
    return BM.conflict_free_bag_stream(policy, cap, N_ROWS, B, L, n_batches, 3)[0]


@functools.lru_cache(maxsize=None)
def _tables(codec, n_rows=tuple(N_ROWS), seed=21, d=36):
    """-> (what set_backing takes (host arrays), the fp32 rows a lookup must return); test_gpu_batched_lru_lfu.py::_tables"""
    from oracle import oracle as orc
    tabs = orc.kaggle_tables(list(n_rows), seed)
    if d != 36:
        tabs = [np.ascontiguousarray(t[:, :d]) for t in tabs]
    if codec == 32:
        return tabs, tabs
    raws = [orc.encode_table(np.clip(t * np.sqrt(len(t)), -1, 1), codec) for t in tabs]   # (spread over the codec's range: rows differ)
    return raws, [orc.decode(a, codec, d) for a in raws]


def _dump(c):
    d = c.batch_dump()
    keys = [(int(t), int(r)) for _, t, r in d]
    assert len(set(keys)) == len(keys), "a key is resident twice"
    return {k: int(s) for k, (s, _, _) in zip(keys, d)}


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
    """the uncached pooling over the same raw tables: (T, B, d) fp32"""
    return _np_pooled(E.apply_emb(lS_o, lS_i, ev, lazy=False))


def _bit_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _index_error_once(E):
    L = E._lib
    assert L.lib().evs_check_index_errors(None) == L.EVS_EINDEX
    assert L.lib().evs_check_index_errors(None) == 0


# ------------------------------------------------------------------------------------- 1. one index per bag = the (B, T) path
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_one_index_per_bag_is_lookup_batch(E, orc, policy):
    """Twin caches over one conflict-free stream: lookup_bags with arange offsets against lookup_batch -- flags, rows bit
    for bit, the dump and every counter after every batch."""
    cap, B, n_batches = 512, 4, 400
    reqs, _, _ = M.conflict_free_stream(policy, cap, N_ROWS, B, n_batches, 3)
    tabs = orc.kaggle_tables(N_ROWS, 21)
    dev = [_dev(t) for t in tabs]
    a, b = E.GpuCache(policy, cap, 26, 36, 32), E.GpuCache(policy, cap, 26, 36, 32)
    a.set_backing(dev)
    b.set_backing(dev)
    r32 = _dev(reqs.reshape(-1, 26))
    li_all = _dev(reqs.transpose(0, 2, 1).astype(np.int64))          # (batches, T, B)
    lo = torch.arange(B, dtype=torch.int64, device="cuda").repeat(26, 1)
    for i in range(n_batches):
        hits, ly = a.lookup_bags(lo, li_all[i])
        hit, out = b.lookup_batch(r32[i * B:(i + 1) * B])
        assert torch.equal(torch.stack(hits, 1), hit), "batch %d: flags" % (i + 1)
        assert torch.equal(torch.stack(ly, 1).view(torch.int32), out.view(torch.int32)), "batch %d: rows" % (i + 1)
        assert _dump(a) == _dump(b), "batch %d: resident set / scores" % (i + 1)
        assert a.batch_stats() == b.batch_stats(), "batch %d: counters" % (i + 1)
    st = a.batch_stats()
    assert st["n_requests"] == B * n_batches and st["n_evict"] > 10 * cap


# ------------------------------------------------------------------------------------------ 2. pinned on conflict-free streams
@pytest.mark.parametrize("policy,shape,codec", [(p, s, c) for p in ("lru", "lfu")
                                                for s, c in (("small", 32), ("large", 32), ("small", 16), ("small", 8), ("small", 4))])
def test_policy_pinned_on_ragged_conflict_free_streams(E, policy, shape, codec):
    """No call brings two new keys to one set, so the rule is deterministic: every flag equals the model's position by
    position, the dump IS the model's resident set (keys and scores), the counters are the model's, and the pooled rows are
    bit-equal to apply_emb over the same raw tables -- after every batch."""
    cap, B, L, n_batches = SHAPES[shape]
    calls = _stream(policy, shape)
    raws, _ = _tables(codec)
    dev = [_dev(r) for r in raws]
    ev = E.EVTables(dev, 36, codec)
    c = E.GpuCache(policy, cap, 26, 36, codec)
    c.set_backing(dev)
    model = BM.BagPolicyModel(policy, cap, N_ROWS)
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
        assert _dump(c) == model.resident(), "batch %d: resident set / scores" % (i + 1)
        st = c.batch_stats()
        assert (st["size"], st["n_hits"], st["n_requests"], st["n_evict"], st["n_perfect_hits"]) == \
            (model.size(), model.n_hits, model.n_requests, model.n_evict, model.n_perfect), "batch %d: counters" % (i + 1)
        assert st["hist"] == [st["size"]] + [0] * 26 and st["n_flush"] == 0
    assert model.n_evict > 5 * cap


# ----------------------------------------------------------------------------------- 3. shapes at which the kernels can go wrong
def _edge_batch(T, B, n_rows, rs):
    """One call with: an empty first and an empty last bag (table 0), a table without indices (table 1 when T > 1), a bag of
    130 indices beside bags of 0 .. 10, last bags that run to nnz, one key three times inside a bag and in bags of other
    samples, the indices -1 and n_rows[k], and (B >= 5) a backwards offset.  -> (offsets, indices, what is malformed)"""
    off, idx = [], []
    for k in range(T):
        sizes = rs.randint(0, 11, B)
        if k == 0:
            sizes[0] = sizes[-1] = 0
        elif k == 1:
            sizes[:] = 0
        else:
            sizes[-1] = max(sizes[-1], 1)                                  # the last bag runs to nnz
        if k == T - 1:
            sizes[B // 2] = 130
        bags = [rs.randint(0, n_rows[k], n).astype(np.int64) for n in sizes]
        if k == T - 1:
            hot = 7 % n_rows[k]
            bags[B // 2][[3, 60, 129]] = hot                               # three times inside one bag ...
            bags[-1][0] = hot                                              # ... and in another sample's bag
            bags[B // 2][[10, 11]] = [-1, n_rows[k]]                       # not keys
        off.append(np.concatenate([[0], np.cumsum(sizes[:-1])]).astype(np.int64))
        idx.append(np.concatenate(bags).astype(np.int64) if sizes.sum() else np.zeros(0, np.int64))
    backwards = False
    if B >= 5 and T > 3:                                                   # (T = 3: table 2 is the one with the long bag)
        k = 2
        if off[k][3] + 1 <= len(idx[k]):
            off[k][2] = off[k][3] + 1                                      # bag 2 = [off[3] + 1, off[3]): empty, flagged
            backwards = True
    return off, idx, backwards


@pytest.mark.parametrize("B", [1, 5, 67])
@pytest.mark.parametrize("policy,T,d,codec", [("lru", 26, 36, 32), ("lfu", 3, 36, 4), ("lfu", 26, 16, 8), ("lru", 3, 16, 32),
                                              ("lfu", 26, 36, 4), ("lru", 3, 36, 16)])
def test_shapes_and_edge_cases(E, policy, T, d, codec, B):
    """Pooled output bit-equal to apply_emb and flags equal to residency from the dump taken before the call, over three
    calls (a fresh cache, the same input again, a fresh draw), with every edge of _edge_batch in each call."""
    n_rows = tuple(400 + 13 * k for k in range(T))
    raws, _ = _tables(codec, n_rows, 5, d)
    dev = [_dev(r) for r in raws]
    ev = E.EVTables(dev, d, codec)
    cap = 65536 if T == 26 else 8192          # (under one key per set on average: no set sees nine)
    c = E.GpuCache(policy, cap, T, d, codec)
    c.set_backing(dev)
    rs = np.random.RandomState(1000 * T + 10 * d + B)
    first = _edge_batch(T, B, n_rows, rs)
    hot = (T, 7 % n_rows[T - 1])
    resident, n_hits, n_perfect = {}, 0, 0
    for call, (off, idx, backwards) in enumerate([first, first, _edge_batch(T, B, n_rows, rs)]):
        lS_o, lS_i = [_dev(o) for o in off], [_dev(i) for i in idx]
        want_pooled = _apply_emb(E, ev, lS_o, lS_i)
        _index_error_once(E)                                   # (the uncached pooling flags the same input)
        hits, ly = c.lookup_bags(lS_o, lS_i)
        _index_error_once(E)                                   # EVS_EINDEX once, then 0
        got = _np_flags(hits)
        assert [len(g) for g in got] == [len(i) for i in idx]
        for k in range(T):
            want = np.array([(k + 1, int(r)) in resident for r in idx[k]], bool)
            assert np.array_equal(got[k], want), "call %d table %d: flags != residency at arrival" % (call, k)
        pooled = _np_pooled(ly)
        assert _bit_equal(pooled, want_pooled), "call %d: pooled rows" % call
        assert not pooled[0, 0].any() and not pooled[0, -1].any()          # the empty first / last bag
        if T > 1:
            assert not pooled[1].any()                                         # the table without indices
        if backwards:
            assert not pooled[2, 2].any()
        after = _dump(c)
        keys = {key for key in BM.keys_of(idx) if 0 <= key[1] < n_rows[key[0] - 1]}
        assert set(after) == set(resident) | keys                          # (nothing is turned away, nothing evicted)
        assert (T, -1) not in after and (T, n_rows[T - 1]) not in after
        if policy == "lfu":                                                    # one count per batch, however many positions
            assert all(after[key] == resident.get(key, 0) + 1 for key in keys)
            assert all(after[key] == resident[key] for key in set(resident) - keys)
        else:
            assert all(after[key] == 0 for key in keys)
        assert hot in after
        n_hits += int(sum(g.sum() for g in got))
        n_perfect += BM.perfect_samples(off, idx, got)
        st = c.batch_stats()
        assert (st["n_hits"], st["n_perfect_hits"], st["n_requests"], st["size"]) == (n_hits, n_perfect, (call + 1) * B, len(after))
        resident = after
    # the second call found everything the first one brought: its all-hit samples are those with a lookup and no bad index
    assert n_hits > 0 and (B == 1 or n_perfect > 0)


def test_tensor_and_list_forms_agree(E, orc):
    """lS_o / lS_i as (T, B) / (T, n) tensors or as lists of T tensors: the same flags, rows and resident set"""
    T, B, n = 26, 33, 99
    tabs = orc.kaggle_tables(N_ROWS, 21)
    dev = [_dev(t) for t in tabs]
    rs = np.random.RandomState(4)
    idx = rs.randint(0, 300, (T, n)).astype(np.int64)
    off = np.sort(rs.randint(0, n + 1, (T, B)), 1).astype(np.int64)
    off[:, 0] = 0
    a, b = E.GpuCache("lfu", 65536, T, 36, 32), E.GpuCache("lfu", 65536, T, 36, 32)      # (8 192 sets for 2 600 keys)
    a.set_backing(dev)
    b.set_backing(dev)
    ev = E.EVTables(dev, 36, 32)
    for _ in range(2):
        ha, la = a.lookup_bags(_dev(off), _dev(idx))
        hb, lb = b.lookup_bags([_dev(o) for o in off], [_dev(i) for i in idx])
        assert torch.equal(torch.stack(ha), torch.stack(hb))
        assert _bit_equal(_np_pooled(la), _np_pooled(lb)) and _bit_equal(_np_pooled(la), _apply_emb(E, ev, _dev(off), _dev(idx)))
        assert _dump(a) == _dump(b)
    assert torch.stack(ha).all()


# -------------------------------------------------------------------------------------------------------- 4. contended batches
def _contended_calls(n_rows, B, max_bag, n_batches, seed, alpha=1.15):
    """Zipf bags of 0 .. max_bag indices per (sample, table), 30 % of the samples replaced by one of 64 hot samples
    (test_gpu_batched_lru_lfu.py: _zipf_requests, restated for bags)"""
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


@pytest.mark.parametrize("policy", ["lru", "lfu"])
@pytest.mark.parametrize("cap_frac", [0.02, 0.10])
def test_invariants_on_contended_batches(E, orc, policy, cap_frac):
    """Many new keys per set: which key takes which way depends on timing, the invariants do not -- flags = residency at
    arrival, no key resident twice, size <= capacity and <= 8 ways per set, a key the batch hit still resident, a missed key
    absent afterwards only if its set is full -- and the pooled rows stay bit-equal to apply_emb."""
    n_rows = KAGGLE_LIKE
    tabs = orc.kaggle_tables(n_rows, 21)
    dev = [_dev(t) for t in tabs]
    ev = E.EVTables(dev, 36, 32)
    cap = int(cap_frac * sum(n_rows))
    nset, bits = M.geometry(cap, n_rows)
    calls = _contended_calls(n_rows, 64, 6, 64, 2)
    on_dev = _upload(calls)
    c = E.GpuCache(policy, cap, 26, 36, 32)
    c.set_backing(dev)
    model = BM.BagPolicyModel(policy, cap, n_rows)
    resident, hits_total, n_pos = {}, 0, 0
    for i, (off, idx) in enumerate(calls):
        lS_o, lS_i = on_dev[i]
        hits, ly = c.lookup_bags(lS_o, lS_i)
        model.batch_bags(off, idx)
        got = np.concatenate(_np_flags(hits))
        keys = BM.keys_of(idx)
        assert np.array_equal(got, np.array([k in resident for k in keys], bool)), "batch %d: flags != residency at arrival" % i
        assert _bit_equal(_np_pooled(ly), _apply_emb(E, ev, lS_o, lS_i)), "batch %d: pooled rows" % i
        after = _dump(c)
        st = c.batch_stats()
        assert len(after) == st["size"] <= cap and st["hist"][0] == st["size"]
        kl = list(after)
        per_set = np.bincount(M.set_of([t - 1 for t, _ in kl], [rw for _, rw in kl], nset, n_rows, bits), minlength=nset)
        assert per_set.max() <= M.WAYS
        assert all(k in after for k, h in zip(keys, got) if h), "a key the batch hit is gone after it"
        gone = sorted({k for k, h in zip(keys, got) if not h and k not in after})
        if gone:
            assert (per_set[M.set_of([t - 1 for t, _ in gone], [rw for _, rw in gone], nset, n_rows, bits)] == M.WAYS).all()
        hits_total += int(got.sum())
        n_pos += len(keys)
        resident = after
    st = c.batch_stats()
    assert st["n_hits"] == hits_total and st["n_requests"] == 64 * len(calls) and st["n_flush"] == 0
    print("%s cap %d: hit rate over %d positions %.4f, the ragged model (first-appearance order) %.4f" %
          (policy, cap, n_pos, hits_total / n_pos, model.n_hits / n_pos))


# ------------------------------------------------------------------------------------------------------ 5. the interaction form
@pytest.mark.parametrize("policy", ["lru", "lfu"])
@pytest.mark.parametrize("codec", [32, 8])
def test_lookup_bags_interact(E, policy, codec):
    """probe -> pooling -> the dense interaction -> insert: R against float64 over the true rows (tests/_accuracy.py), flags
    and dump equal to lookup_bags' on a twin cache.  The stream is conflict-free (30 warm-up batches of 8 fill the sets,
    then four batches of 300), so both caches hold the same keys whatever the timing."""
    cap, T, d, B = 1024, 26, 36, 300
    raws, tabs = _tables(codec)
    rs = np.random.RandomState(11)
    perms = [rs.permutation(n) for n in N_ROWS]
    model = BM.BagPolicyModel(policy, cap, N_ROWS)
    a, b = E.GpuCache(policy, cap, T, d, codec), E.GpuCache(policy, cap, T, d, codec)
    backing = [_dev(r) for r in raws]
    a.set_backing(backing)
    b.set_backing(backing)
    x0 = torch.zeros((8, d), device="cuda")
    for i in range(30):
        off, idx, want, _ = BM.conflict_free_bags(model, rs, perms, 8, 4)
        lS_o, lS_i = [_dev(o) for o in off], [_dev(i_) for i_ in idx]
        ha, _ = a.lookup_bags_interact(lS_o, lS_i, x0)
        hb, _ = b.lookup_bags(lS_o, lS_i)
        assert torch.equal(torch.cat(ha), torch.cat(hb)) and np.array_equal(torch.cat(ha).cpu().numpy().astype(bool), np.concatenate(want))
    evict0 = model.n_evict
    for i in range(4):
        off, idx, want, _ = BM.conflict_free_bags(model, rs, perms, B, 4)
        lS_o, lS_i = [_dev(o) for o in off], [_dev(i_) for i_ in idx]
        x = rs.uniform(-1, 1, size=(B, d)).astype(np.float32)
        ha, R = a.lookup_bags_interact(lS_o, lS_i, _dev(x), itself=bool(i & 1))
        hb, _ = b.lookup_bags(lS_o, lS_i)
        assert torch.equal(torch.cat(ha), torch.cat(hb)) and np.array_equal(torch.cat(ha).cpu().numpy().astype(bool), np.concatenate(want))
        ref = acc.reference_from_bags(x, tabs, off, idx, bool(i & 1))
        acc.check(R.cpu().numpy(), ref, "%s codec %d batch %d" % (policy, codec, i), "bags chain: pooling + dense interaction, codec %d" % codec)
        assert _dump(a) == _dump(b) == model.resident()
        assert a.batch_stats() == b.batch_stats()
    assert model.n_evict > evict0


# ------------------------------------------------------------------------------------------------------ 6. mixing and refusals
def test_lookup_batch_and_lookup_bags_alternate(E, orc):
    """the two forms share the batch counter: alternating on one LRU cache against one model, ages and dump after each call"""
    cap, B = 1024, 4
    tabs = orc.kaggle_tables(N_ROWS, 21)
    c = E.GpuCache("lru", cap, 26, 36, 32)
    c.set_backing([_dev(t) for t in tabs])
    model = BM.BagPolicyModel("lru", cap, N_ROWS)
    rs = np.random.RandomState(6)
    perms = [rs.permutation(n) for n in N_ROWS]
    for i in range(120):
        if i % 3 == 1:
            rq, want = M.conflict_free_batch(model, rs, perms, B)
            hit, _ = c.lookup_batch(_dev(rq))
            assert np.array_equal(hit.cpu().numpy().astype(bool), want), "call %d (rows)" % i
        else:
            off, idx, want, _ = BM.conflict_free_bags(model, rs, perms, B, 3)
            hits, _ = c.lookup_bags([_dev(o) for o in off], [_dev(i_) for i_ in idx])
            assert np.array_equal(torch.cat(hits).cpu().numpy().astype(bool), np.concatenate(want)), "call %d (bags)" % i
        assert _dump(c) == model.resident(), "call %d: resident set / ages" % i
    assert model.n_evict > cap


def test_update_rows_between_two_bag_calls(E, orc):
    """update_rows between two lookup_bags calls: the next call serves the new vector from the arena (flag 1, new bits)"""
    n_rows = [300] * 26
    tabs = [t.copy() for t in orc.kaggle_tables(n_rows, 8)]
    dev = [_dev(t) for t in tabs]
    c = E.GpuCache("lru", 16384, 26, 36, 32)
    c.set_backing(dev)
    rs = np.random.RandomState(1)
    B = 20
    idx = [np.concatenate([[k % 100], rs.randint(0, 100, 3 * B - 1)]).astype(np.int64) for k in range(26)]     # bag 0 of table k starts with row k
    off = [np.concatenate([[0, 1], np.arange(3, 3 * B - 3, 3)]).astype(np.int64)[:B] for _ in range(26)]       # bag 0 = one index
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
    assert _bit_equal(pooled[:, 0, :], vals)                                   # bag 0 = the updated row alone
    assert _bit_equal(pooled, _apply_emb(E, E.EVTables(dev, 36, 32), lS_o, lS_i))
    for k in range(26):                                                        # index order, fp32, from +0
        want = np.zeros((B, 36), np.float32)
        ends = np.append(off[k][1:], len(idx[k]))
        for b_ in range(B):
            for r in idx[k][off[k][b_]:ends[b_]]:
                want[b_] = want[b_] + tabs[k][r]
        assert _bit_equal(pooled[k], want), "table %d" % k


def _refused(E, code, policy, fn):
    with pytest.raises(E._lib.EvsError) as ei:
        fn()
    assert ei.value.code == code and policy in str(ei.value), str(ei.value)


def _serves(c, tabs, seed=0):
    rs = np.random.RandomState(seed)
    T = len(tabs)
    idx = [rs.randint(0, 2, 40).astype(np.int64) for _ in range(T)]           # (2 T keys: they fit any cache used here)
    lo, li = [torch.arange(40, dtype=torch.int64, device="cuda")] * T, [_dev(i) for i in idx]
    for _ in range(2):
        hits, ly = c.lookup_bags(lo, li)
        for t in range(T):
            assert _bit_equal(ly[t].cpu().numpy(), tabs[t][idx[t]]), "table %d" % t
    assert torch.cat(hits).float().mean() > 0.9       # (the second call finds what the first one inserted)


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_refusals_leave_the_cache_serving(E, orc, policy, tmp_path):
    L = E._lib
    n_rows = [300] * 26
    tabs = orc.kaggle_tables(n_rows, 4)
    dev = [_dev(t) for t in tabs]
    rq = _dev(np.zeros((4, 26), np.int32))
    lo = [torch.arange(4, dtype=torch.int64, device="cuda")] * 26
    li = [torch.zeros(4, dtype=torch.int64, device="cuda")] * 26
    x = torch.zeros((4, 36), device="cuda")

    # an EvLFU cache has no bag form; its own batched path still serves
    e = E.GpuCache("evlfu", 512, 26, 36, 32)
    e.set_backing(dev)
    _refused(E, L.EVS_EINVAL, "evlfu", lambda: e.lookup_bags(lo, li))
    _refused(E, L.EVS_EINVAL, "evlfu", lambda: e.lookup_bags_interact(lo, li, x))
    hit, out = e.lookup_batch(rq)
    assert _bit_equal(out.cpu().numpy()[:, 3], tabs[3][[0] * 4])

    # host-memory and file-backed tables: refused, HBM tables afterwards: served
    c = E.GpuCache(policy, 512, 26, 36, 32)
    c.set_backing([torch.from_numpy(np.ascontiguousarray(t)).pin_memory() for t in tabs])
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags(lo, li))
    c.set_backing(dev)
    _serves(c, tabs)
    paths = []
    for k, t in enumerate(tabs):
        p = tmp_path / ("ev-table-%d.bin" % (k + 1))
        t.tofile(p)
        paths.append(str(p))
    ft = E.FileTier(paths, 144, 1 << 30)
    c = E.GpuCache(policy, 512, 26, 36, 32)
    c.set_file_backing(ft)
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags(lo, li))
    hit, out = c.request(rq)                   # (the exact engine still serves it)
    assert _bit_equal(out.cpu().numpy()[:, 3], tabs[3][[0] * 4])

    # a cache that has served request()
    c = E.GpuCache(policy, 512, 26, 36, 32)
    c.set_backing(dev)
    c.request(rq)
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags(lo, li))
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_bags_interact(lo, li, x))
    hit, out = c.request(rq)
    assert hit.all() and _bit_equal(out.cpu().numpy()[:, 3], tabs[3][[0] * 4])

    # a capacity below one set
    c = E.GpuCache(policy, 7, 26, 36, 32)
    c.set_backing(dev)
    _refused(E, L.EVS_EINVAL, policy, lambda: c.lookup_bags(lo, li))
    hit, out = c.request(rq)
    assert _bit_equal(out.cpu().numpy()[:, 3], tabs[3][[0] * 4])

    # a key universe of 2^32 rows (declared: nothing is read before the refusal), then the true sizes
    c = E.GpuCache(policy, 512, 26, 36, 32)
    ptrs = (C.c_void_p * 26)(*[t.data_ptr() for t in dev])
    big = (C.c_int64 * 26)(*([1 << 31, 1 << 31] + [300] * 24))
    L.check(L.lib().evs_cache_set_backing(c._h, ptrs, big))
    _refused(E, L.EVS_EINVAL, policy, lambda: c.lookup_bags(lo, li))
    c.set_backing(dev)
    _serves(c, tabs)

    # the argument checks that read the handle: all EVS_EINVAL before the device is touched, the cache serves afterwards
    lib = L.lib()
    idx_c = (C.c_void_p * 26)(*[t.data_ptr() for t in li])
    off_c = (C.c_void_p * 26)(*[t.data_ptr() for t in lo])
    nnz_c = (C.c_int64 * 26)(*([4] * 26))
    out = torch.empty((26, 4, 36), device="cuda")
    null_idx = (C.c_void_p * 26)(*([None] + [t.data_ptr() for t in li[1:]]))
    assert lib.evs_cache_lookup_bags(c._h, 4, null_idx, off_c, nnz_c, out.data_ptr(), 144, 36, None, None) == L.EVS_EINVAL
    assert b"indices[0]" in lib.evs_last_error()
    null_off = (C.c_void_p * 26)(*([t.data_ptr() for t in lo[:-1]] + [None]))
    assert lib.evs_cache_lookup_bags(c._h, 4, idx_c, null_off, nnz_c, out.data_ptr(), 144, 36, None, None) == L.EVS_EINVAL
    neg = (C.c_int64 * 26)(*([4] * 25 + [-1]))
    assert lib.evs_cache_lookup_bags(c._h, 4, idx_c, off_c, neg, out.data_ptr(), 144, 36, None, None) == L.EVS_EINVAL
    huge = (C.c_int64 * 26)(*([1 << 30, 1 << 30] + [4] * 24))
    assert lib.evs_cache_lookup_bags(c._h, 4, idx_c, off_c, huge, out.data_ptr(), 144, 36, None, None) == L.EVS_EINVAL
    assert b"2^31" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags(c._h, 4, idx_c, off_c, nnz_c, out.data_ptr() + 4, 144, 36, None, None) == L.EVS_EINVAL
    _serves(c, tabs, 1)
    hits, R = c.lookup_bags_interact(lo, li, x)           # (hit = NULL in the C call is allowed: flags are optional)
    assert lib.evs_cache_lookup_bags(c._h, 4, idx_c, off_c, nnz_c, out.data_ptr(), 144, 36, None, None) == 0
    assert _bit_equal(out.cpu().numpy()[3], tabs[3][[0] * 4])
    wide = E.GpuCache(policy, 512, 32, 36, 32)             # 33 features
    wide.set_backing([dev[k % 26] for k in range(32)])
    _refused(E, L.EVS_EINVAL, "features", lambda: wide.lookup_bags_interact(lo + lo[:6], li + li[:6], x))
    _serves(wide, [tabs[k % 26] for k in range(32)])
    odd = E.GpuCache(policy, 512, 2, 20, 32)               # a dim the pooling takes and the interaction does not
    t20 = [np.ascontiguousarray(t[:, :20]) for t in tabs[:2]]
    odd.set_backing([_dev(t) for t in t20])
    _refused(E, L.EVS_EINVAL, "d = 20", lambda: odd.lookup_bags_interact(lo[:2], li[:2], torch.zeros((4, 20), device="cuda")))
    _serves(odd, t20)
    odd = E.GpuCache(policy, 512, 2, 18, 32)               # a dim the pooling does not take
    odd.set_backing([_dev(np.ascontiguousarray(t[:, :18])) for t in tabs[:2]])
    assert lib.evs_cache_lookup_bags(odd._h, 4, idx_c, off_c, nnz_c, out.data_ptr(), 80, 20, None, None) == L.EVS_EINVAL
    assert b"multiple of 4" in lib.evs_last_error()
