"""Batched LRU and LFU on the set-associative cache tier (csrc/evs_cache_policy.hip) held to "the batched rule" of
include/evstore_hip.h (evs_cache_set_batch_policy): pinned flag by flag and way by way to the Python restatement
(tests/_batched_policy_model.py) on conflict-free streams, where the rule is deterministic; held to its invariants and to
the sequential oracle's hit rate on contended Zipf batches, where which key takes which way depends on timing; the
interaction consumer, the refusals and the row updates on such a tier."""
import functools

import numpy as np
import pytest
import torch

import _accuracy as acc
import _batched_policy_model as M

pytestmark = pytest.mark.gpu

N_ROWS = [2000] * 26
SHAPES = {"small": (512, 4, 400), "large": (1024, 8, 300)}     # capacity, batch, batches (tests/test_batched_policy_model.py)
KAGGLE_LIKE = [3000, 40, 20000, 700, 5, 9000, 1500, 12, 26000, 300, 8000, 64, 2200, 17000, 3, 450, 5000, 90, 13000,
               2, 7000, 30, 1000, 11000, 150, 4000]            # (test_batched_cache_invariants_and_hit_rate's tables)


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
    cap, batch, n_batches = SHAPES[shape]
    reqs, hits, _ = M.conflict_free_stream(policy, cap, N_ROWS, batch, n_batches, 3)
    return reqs, hits


@functools.lru_cache(maxsize=None)
def _tables(codec, n_rows=tuple(N_ROWS), seed=21):
    """-> (what set_backing takes (host arrays), the fp32 rows a lookup must return)"""
    from oracle import oracle as orc
    tabs = orc.kaggle_tables(list(n_rows), seed)
    if codec == 32:
        return tabs, tabs
    raws = [orc.encode_table(np.clip(t * np.sqrt(len(t)), -1, 1), codec) for t in tabs]   # (spread over the codec's range: rows differ)
    return raws, [orc.decode(a, codec, 36) for a in raws]


def _rows_exact(out, tabs, rq):
    for t in range(rq.shape[1]):
        assert np.array_equal(out[:, t, :].view(np.uint32), tabs[t][rq[:, t]].view(np.uint32)), "table %d" % t


def _dump(c):
    d = c.batch_dump()
    keys = [(int(t), int(r)) for _, t, r in d]
    assert len(set(keys)) == len(keys), "a key is resident twice"
    return {k: int(s) for k, (s, _, _) in zip(keys, d)}


# --------------------------------------------------------------------------------------------------------- 1. policy pinned
@pytest.mark.parametrize("policy,shape,codec", [(p, s, c) for p in ("lru", "lfu")
                                                for s, c in (("small", 32), ("large", 32), ("small", 8), ("small", 4))])
def test_policy_pinned_on_conflict_free_streams(E, policy, shape, codec):
    """No batch of the stream brings two new keys to one set, so the rule is deterministic: every hit flag equals the model's,
    rows are the table rows bit for bit, and after every batch the dump IS the model's resident set -- keys and scores (LRU:
    age in batches, LFU: the counter) -- with the statistics consistent."""
    cap, batch, n_batches = SHAPES[shape]
    reqs, hits = _stream(policy, shape)
    raws, tabs = _tables(codec)
    c = E.GpuCache(policy, cap, 26, 36, codec)
    c.set_backing([_dev(r) for r in raws])
    model = M.BatchedPolicyModel(policy, cap, N_ROWS)
    r = _dev(reqs.reshape(-1, 26))
    n_hits = 0
    for i in range(n_batches):
        hit, out = c.lookup_batch(r[i * batch:(i + 1) * batch])
        want = model.batch(reqs[i])
        assert np.array_equal(want, hits[i])
        hit = hit.cpu().numpy().astype(bool)
        assert np.array_equal(hit, want), "batch %d: %d flags differ from the model" % (i + 1, int((hit != want).sum()))
        _rows_exact(out.cpu().numpy(), tabs, reqs[i])
        n_hits += int(hit.sum())
        assert _dump(c) == model.resident(), "batch %d: resident set / scores" % (i + 1)
        if i % 25 == 0 or i == n_batches - 1:
            st = c.batch_stats()
            assert st["size"] == model.size() <= cap and st["n_hits"] == n_hits and st["n_requests"] == (i + 1) * batch
            assert st["n_flush"] == 0 and st["n_evict"] == model.n_evict
            assert st["hist"] == [st["size"]] + [0] * 26
    assert model.n_evict > 10 * cap


# ------------------------------------------------------------------------------------------- 1b. policy pinned across wraps
@pytest.fixture(scope="module")
def wrap_tables():
    """(geometry, codec) -> the tables of one of M.WRAP_GEOMETRIES, filled on the device: fp32 uniform in (-1, 1), or raw
    random bytes for a codec-8 tier.  Kept for the module, freed behind it."""
    made = {}

    def get(geom, codec):
        if (geom, codec) not in made:
            n_rows = M.WRAP_GEOMETRIES[geom][1]
            g = torch.Generator(device="cuda")
            g.manual_seed(len(geom) + codec)
            if codec == 32:
                made[geom, codec] = [torch.empty(n, 36, device="cuda").uniform_(-1, 1, generator=g) for n in n_rows]
            else:
                made[geom, codec] = [torch.randint(0, 256, (n, 36), dtype=torch.uint8, device="cuda", generator=g) for n in n_rows]
        return made[geom, codec]
    yield get
    made.clear()


@functools.lru_cache(maxsize=None)
def _wrap_case(policy, geom):
    return M.wrap_case(policy, geom)


@pytest.mark.parametrize("policy,geom,codec,bags", [("lfu", "tiny", 32, False), ("lfu", "tiny-dual", 32, True), ("lru", "tiny", 32, False),
                                                    ("lru", "tiny-dual", 32, False), ("lfu", "tiny-dual", 8, False)])
def test_policy_pinned_across_stamp_wraps(E, orc, wrap_tables, policy, geom, codec, bags):
    """Two sets of eight ways under a key universe of 2^22 / 2^19 rows: the tag leaves the batch stamp S = 4 / 6 bits under
    LFU and 10 / 12 under LRU (asserted: M.stamp_bits_of restates sa_make_geom), so a run of a few hundred batches wraps it
    many times.  M.wrap_stream leaves ways alone for 2^S batches and longer, re-hits them exactly 2^S batches after their
    last touch and brings new keys to sets whose only stale way is such a lapped one; the modular model
    (BatchedPolicyModel(stamp_bits=S)) says what "ages are CIRCULAR" of include/evstore_hip.h then means, and the cache is
    held to it after EVERY batch: hit flags, rows bit-equal to the table rows, the dump's keys and scores (LRU: the circular
    age), the statistics.  The stream parts from a plain-integer model (asserted from its event counts, as
    tests/test_batched_policy_model.py asserts them), so a geometry change cannot turn this back into a no-wrap run.
    LRU on `tiny-dual` (S = 12) does not wrap in 640 batches: there `last` carries from its 6-bit low field into the high
    one, across the copy-select bit, ten times while replacements flip that bit.  bags: every third batch goes through
    lookup_bags with one index per bag -- the two forms share the batch counter and count alike, the model is unchanged."""
    cap, n_rows, S = M.WRAP_GEOMETRIES[geom]
    S, T = S[policy], len(n_rows)
    assert M.stamp_bits_of(policy, cap, n_rows)[2] == S == {("lfu", "tiny"): 4, ("lfu", "tiny-dual"): 6, ("lru", "tiny"): 10,
                                                            ("lru", "tiny-dual"): 12}[policy, geom]
    batches, hits, _, parted = _wrap_case(policy, geom)
    n_batches = len(batches)
    if (policy, geom) == ("lru", "tiny-dual"):
        assert n_batches >= 600 and n_batches >> 6 >= 9 and parted["evictions"] >= 36
    else:
        assert n_batches >= (3 if policy == "lfu" else 2.5) * (1 << S)
        kinds = [k for k in M.EVENTS if policy == "lfu" or k != "count_skipped"]
        assert all(parted[k] >= 5 for k in kinds) and parted["flags"] >= 5 and parted["dumps"] >= 5, parted
    dev = wrap_tables(geom, codec)
    # the reference rows of the whole stream: the requested rows gathered on the device and copied back, once
    flat = np.concatenate(batches)
    rows = [dev[t][_dev(flat[:, t].astype(np.int64))].cpu().numpy() for t in range(T)]
    if codec != 32:
        rows = [orc.decode(a, codec, 36) for a in rows]
    want_rows = np.stack(rows, 1)                              # (all samples, T, 36)
    c = E.GpuCache(policy, cap, T, 36, codec)
    c.set_backing(dev)
    model = M.BatchedPolicyModel(policy, cap, n_rows, stamp_bits=S)
    arange = [_dev(np.arange(b, dtype=np.int64)) for b in range(5)]
    at = n_hits = n_req = 0
    for i, rq in enumerate(batches):
        B = len(rq)
        if bags and i % 3 == 2:
            hit, out = c.lookup_bags([arange[B]] * T, [_dev(rq[:, t].astype(np.int64)) for t in range(T)])
            hit, out = torch.stack(hit, 1), torch.stack(out, 1)
        else:
            hit, out = c.lookup_batch(_dev(rq))
        want = model.batch(rq)
        assert np.array_equal(want, hits[i])
        hit = hit.cpu().numpy().astype(bool)
        assert np.array_equal(hit, want), "batch %d (cur = %d): flags\n%s\nthe model's\n%s" % (i + 1, model._cur(), hit, want)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want_rows[at:at + B].view(np.uint32)), "batch %d: rows" % (i + 1)
        at, n_hits, n_req = at + B, n_hits + int(hit.sum()), n_req + B
        assert _dump(c) == model.resident(), "batch %d (cur = %d): resident set / scores" % (i + 1, model._cur())
        if i % 25 == 0 or i == n_batches - 1:
            st = c.batch_stats()
            assert st["size"] == model.size() <= cap and st["n_hits"] == n_hits and st["n_requests"] == n_req
            assert st["n_flush"] == 0 and st["n_evict"] == model.n_evict
            assert st["hist"] == [st["size"]] + [0] * T
    assert model.events == {k: parted[k] for k in M.EVENTS}


# ------------------------------------------------------------------------------------------------------ 2. contended batches
def _zipf_requests(n_rows, n_req, seed, alpha=1.15):
    """(tests/test_gpu_cache.py: _zipf_requests, restated)"""
    rs = np.random.RandomState(seed)
    perms = [rs.permutation(n) for n in n_rows]
    reqs = np.zeros((n_req, len(n_rows)), np.int32)
    for k, n in enumerate(n_rows):
        reqs[:, k] = perms[k][np.minimum(rs.zipf(alpha, n_req) - 1, n - 1)]
    hot = reqs[rs.randint(0, n_req, 64)]
    rep = rs.rand(n_req) < 0.3
    reqs[rep] = hot[rs.randint(0, 64, rep.sum())]
    return reqs


@pytest.mark.parametrize("policy", ["lru", "lfu"])
@pytest.mark.parametrize("cap_frac,batch,n_req,seed", [(0.02, 64, 4096, 2), (0.10, 256, 4096, 2), (0.02, 64, 8192, 5)])
def test_invariants_and_hit_rate_on_contended_batches(E, orc, policy, cap_frac, batch, n_req, seed):
    """Zipf batches with many new keys per set: which key takes which way depends on timing, the invariants do not -- rows
    exact, flags = residency at arrival, no duplicate keys, size <= capacity, no set above 8 ways, a missed key absent
    afterwards only if its set is full, no key the batch touched gone after it -- and the hit rate stays inside the band
    test_batched_cache_invariants_and_hit_rate holds EvLFU to, against oracle.LRU / oracle.LFU on the same requests."""
    n_rows = KAGGLE_LIKE
    tabs = orc.kaggle_tables(n_rows, 21)
    cap = int(cap_frac * sum(n_rows))
    nset, bits = M.geometry(cap, n_rows)
    reqs = _zipf_requests(n_rows, n_req, seed)
    c = E.GpuCache(policy, cap, 26, 36, 32)
    c.set_backing([_dev(t) for t in tabs])
    r = _dev(reqs)
    resident, hits_total = {}, 0
    for s in range(0, n_req, batch):
        rq = reqs[s:s + batch]
        hit, out = c.lookup_batch(r[s:s + batch])
        hit, out = hit.cpu().numpy().astype(bool), out.cpu().numpy()
        _rows_exact(out, tabs, rq)
        keys = [[(t + 1, int(rq[b, t])) for t in range(26)] for b in range(len(rq))]
        assert np.array_equal(hit, np.array([[k in resident for k in row] for row in keys])), "flags != residency at arrival"
        hits_total += int(hit.sum())
        after = _dump(c)
        st = c.batch_stats()
        assert len(after) == st["size"] <= cap and st["hist"][0] == st["size"]
        kl = list(after)
        per_set = np.bincount(M.set_of([t - 1 for t, _ in kl], [rw for _, rw in kl], nset, n_rows, bits), minlength=nset)
        assert per_set.max() <= M.WAYS
        touched = {k for row, hrow in zip(keys, hit) for k, h in zip(row, hrow) if h}
        assert all(k in after for k in touched), "a key the batch hit is gone after it"
        gone = sorted({k for row, hrow in zip(keys, hit) for k, h in zip(row, hrow) if not h and k not in after})
        if gone:
            assert (per_set[M.set_of([t - 1 for t, _ in gone], [rw for _, rw in gone], nset, n_rows, bits)] == M.WAYS).all()
        resident = after
    st = c.batch_stats()
    assert st["n_hits"] == hits_total and st["n_requests"] == n_req and st["n_flush"] == 0
    o = (orc.LRU if policy == "lru" else orc.LFU)(cap, tabs)
    seq_hits = sum(int(o.request(rq)[0].sum()) for rq in reqs)
    rate_b, rate_s = hits_total / reqs.size, seq_hits / reqs.size
    first_seen_in_batch, seen = 0, set()      # the snapshot cannot hit keys first inserted inside the same batch
    for s in range(0, n_req, batch):
        local = set()
        for rq in reqs[s:s + batch]:
            for k in range(26):
                key = (k, int(rq[k]))
                if key in local and key not in seen:
                    first_seen_in_batch += 1
                local.add(key)
        seen |= local
    print("%s cap %d batch %d: hit rate %.4f, sequential %.4f, first seen in batch %.4f" %
          (policy, cap, batch, rate_b, rate_s, first_seen_in_batch / reqs.size))
    assert rate_b >= rate_s - first_seen_in_batch / reqs.size - 0.05, (rate_b, rate_s)
    assert rate_b <= rate_s + 0.05, (rate_b, rate_s)


# ------------------------------------------------------------------------------------------------------- 3. lookup_interact
@pytest.mark.parametrize("policy", ["lru", "lfu"])
@pytest.mark.parametrize("codec", [32, 8])
def test_lookup_interact(E, policy, codec):
    """probe -> the row-id / pointer-table consumer -> insert: R against float64 over the true rows (tests/_accuracy.py), flags
    equal to lookup_batch's on a twin cache fed the same stream.  The stream is conflict-free (30 warm-up batches of 8 fill
    the sets, then four batches of 300), so both caches hold the same keys whatever the timing."""
    cap, T, d, B = 1024, 26, 36, 300
    raws, tabs = _tables(codec)
    rs = np.random.RandomState(11)
    perms = [rs.permutation(n) for n in N_ROWS]
    model = M.BatchedPolicyModel(policy, cap, N_ROWS)
    a, b = E.GpuCache(policy, cap, T, d, codec), E.GpuCache(policy, cap, T, d, codec)
    backing = [_dev(r) for r in raws]
    a.set_backing(backing)
    b.set_backing(backing)
    x0 = torch.zeros((8, d), device="cuda")
    for i in range(30):
        rq, want = M.conflict_free_batch(model, rs, perms, 8)
        ha, _ = a.lookup_interact(_dev(rq), x0)
        hb, _ = b.lookup_batch(_dev(rq))
        assert np.array_equal(ha.cpu().numpy().astype(bool), want) and torch.equal(ha, hb)
    evict0 = model.n_evict
    for i in range(4):
        rq, want = M.conflict_free_batch(model, rs, perms, B)
        x = rs.uniform(-1, 1, size=(B, d)).astype(np.float32)
        ha, R = a.lookup_interact(_dev(rq), _dev(x), itself=bool(i & 1))
        hb, out = b.lookup_batch(_dev(rq))
        assert torch.equal(ha, hb) and np.array_equal(ha.cpu().numpy().astype(bool), want)
        assert 0.3 < want.mean() < 1.0
        _rows_exact(out.cpu().numpy(), tabs, rq)
        ref = acc.Reference(x, [acc.pool64(tabs[k][rq[:, k]])[:2] for k in range(T)], bool(i & 1))
        acc.check(R.cpu().numpy(), ref, "%s codec %d batch %d" % (policy, codec, i), "policy chain consumer, codec %d" % codec)
        assert _dump(a) == _dump(b) == model.resident()
    assert model.n_evict > evict0


# ------------------------------------------------------------------------------------------------------------- 4. refusals
def _refused(E, code, policy, fn):
    with pytest.raises(E._lib.EvsError) as ei:
        fn()
    assert ei.value.code == code and policy in str(ei.value), str(ei.value)


def _serves(c, tabs, n_rows, seed=0):
    rs = np.random.RandomState(seed)
    rq = np.stack([rs.randint(0, 2, 40) for _ in n_rows], 1).astype(np.int32)      # (52 keys: they fit any cache used here)
    for _ in range(2):
        hit, out = c.lookup_batch(_dev(rq))
        _rows_exact(out.cpu().numpy(), tabs, rq)
    assert hit.cpu().numpy().mean() > 0.9       # (the second call finds what the first one inserted)


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_refusals_leave_the_cache_serving(E, orc, policy, tmp_path):
    from evstore_dlrm_amd import gpu_cache
    L = E._lib
    n_rows = [300] * 26
    tabs = orc.kaggle_tables(n_rows, 4)
    dev = [_dev(t) for t in tabs]
    rq = _dev(np.zeros((4, 26), np.int32))

    # the other batch policies, the one-launch form
    c = E.GpuCache(policy, 512, 26, 36, 32)
    c.set_backing(dev)
    _refused(E, L.EVS_EINVAL, policy, lambda: c.set_batch_policy("plan"))
    _refused(E, L.EVS_EINVAL, policy, lambda: c.set_batch_policy("sampled"))
    _refused(E, L.EVS_EINVAL, policy, lambda: c.set_inline_update(True))
    c.set_inline_update(False)
    c.set_batch_policy("setassoc")
    _serves(c, tabs, n_rows)
    _refused(E, L.EVS_EINVAL, policy, lambda: c.set_inline_update(True))
    with pytest.raises(L.EvsError) as ei:      # the exact and the batched path do not mix
        c.request(rq)
    assert ei.value.code == L.EVS_ESTATE
    _serves(c, tabs, n_rows, 1)
    c = E.GpuCache(policy, 512, 26, 36, 32)     # ... nor the other way round
    c.set_backing(dev)
    c.request(rq)
    with pytest.raises(L.EvsError) as ei:
        c.lookup_batch(rq)
    assert ei.value.code == L.EVS_ESTATE
    c.request(rq)

    # host-memory and file-backed tables: refused, HBM tables afterwards: served
    c = E.GpuCache(policy, 512, 26, 36, 32)
    c.set_backing([torch.from_numpy(np.ascontiguousarray(t)).pin_memory() for t in tabs])
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_batch(rq))
    c.set_backing(dev)
    _serves(c, tabs, n_rows)
    paths = []
    for k, t in enumerate(tabs):
        p = tmp_path / ("ev-table-%d.bin" % (k + 1))
        t.tofile(p)
        paths.append(str(p))
    ft = E.FileTier(paths, 144, 1 << 30)
    c = E.GpuCache(policy, 512, 26, 36, 32)
    c.set_file_backing(ft)
    _refused(E, L.EVS_ESTATE, policy, lambda: c.lookup_batch(rq))
    hit, out = c.request(rq)                   # (the exact engine still serves it)
    _rows_exact(out.cpu().numpy(), tabs, np.zeros((4, 26), np.int32))

    # a capacity below one set
    c = E.GpuCache(policy, 7, 26, 36, 32)
    c.set_backing(dev)
    _refused(E, L.EVS_EINVAL, policy, lambda: c.lookup_batch(rq))
    _refused(E, L.EVS_EINVAL, "set-associative", lambda: c.set_batch_policy("setassoc"))
    hit, out = c.request(rq)
    _rows_exact(out.cpu().numpy(), tabs, np.zeros((4, 26), np.int32))

    # a key universe of 2^32 rows (declared: nothing is read before the refusal), then the true sizes
    import ctypes as C
    c = E.GpuCache(policy, 512, 26, 36, 32)
    ptrs = (C.c_void_p * 26)(*[t.data_ptr() for t in dev])
    big = (C.c_int64 * 26)(*([1 << 31, 1 << 31] + [300] * 24))
    L.check(L.lib().evs_cache_set_backing(c._h, ptrs, big))
    _refused(E, L.EVS_EINVAL, policy, lambda: c.lookup_batch(rq))
    c.set_backing(dev)
    _serves(c, tabs, n_rows)

    # a tier pair / triple
    c1, c2, e = E.GpuCache(policy, 512, 26, 36, 32), E.GpuCache(policy, 1024, 26, 36, 32), E.GpuCache("evlfu", 1024, 26, 36, 32, "cpp")
    for t in (c1, c2, e):
        t.set_backing(dev)
    c3 = gpu_cache.GpuAltKeyTier(64, [torch.zeros(n, dtype=torch.int32, device="cuda") for n in n_rows])
    x = torch.zeros((4, 36), device="cuda")
    _refused(E, L.EVS_EINVAL, policy, lambda: gpu_cache.lookup_batch_c1c2(c1, e, rq))
    _refused(E, L.EVS_EINVAL, policy, lambda: gpu_cache.lookup_batch_c1c2(e, c2, rq))
    _refused(E, L.EVS_EINVAL, policy, lambda: gpu_cache.lookup_batch_c1c2(c1, c2, rq))
    _refused(E, L.EVS_EINVAL, policy, lambda: gpu_cache.lookup_batch_c1c2c3(c1, e, c3, rq))
    _refused(E, L.EVS_EINVAL, policy, lambda: gpu_cache.lookup_interact_c1c2(e, c2, rq, x))
    _serves(c1, tabs, n_rows)
    _serves(c2, tabs, n_rows)


def _serves_exact(c, dev, n_rows, seed):
    rs = np.random.RandomState(seed)
    rq = np.stack([rs.randint(0, 2, 5) for _ in n_rows], 1).astype(np.int32)
    for _ in range(2):
        hit, out = c.lookup_batch(_dev(rq))
        out = out.cpu().numpy()
        for t in range(rq.shape[1]):
            want = dev[t][_dev(rq[:, t].astype(np.int64))].cpu().numpy()
            assert np.array_equal(out[:, t].view(np.uint32), want.view(np.uint32))
    return hit.cpu().numpy()


def test_one_set_under_23_tag_bits_is_where_the_form_ends(E, wrap_tables):
    """The `tiny` tables (2^22 keys) with capacity 8 are one set: tag + 1 needs 23 bits and the way word has no room for a
    stamp of 4 (sa_make_geom).  An explicit "setassoc" on an EvLFU cache is refused (EVS_EINVAL) at the first batched call;
    an EvLFU cache that was given no policy resolves to another form and serves exact rows; LRU / LFU have no other form: refused
    with a message that names the policy, and served once set_backing brings smaller tables.  Capacity 16 is served by all."""
    L = E._lib
    _, n_rows, _ = M.WRAP_GEOMETRIES["tiny"]
    T = len(n_rows)
    dev = wrap_tables("tiny", 32)
    small = [t[:1000] for t in dev]
    with pytest.raises(ValueError):
        M.stamp_bits_of("evlfu", 8, n_rows)
    rq = _dev(np.zeros((2, T), np.int32))
    c = E.GpuCache("evlfu", 8, T, 36, 32, "python").set_batch_policy("setassoc")
    c.set_backing(dev)
    with pytest.raises(L.EvsError) as ei:
        c.lookup_batch(rq)
    assert ei.value.code == L.EVS_EINVAL and "set-associative" in str(ei.value)
    c = E.GpuCache("evlfu", 8, T, 36, 32, "python")
    c.set_backing(dev)
    assert _serves_exact(c, dev, n_rows, 0).mean() > 0.5                 # (the second call finds what the first one inserted)
    for policy in ("lru", "lfu"):
        c = E.GpuCache(policy, 8, T, 36, 32)
        c.set_backing(dev)
        with pytest.raises(L.EvsError) as ei:
            c.lookup_batch(rq)
        assert ei.value.code == L.EVS_EINVAL and policy in str(ei.value), str(ei.value)
        c.set_backing(small)
        assert _serves_exact(c, small, [1000] * T, 1).mean() > 0.5
    for policy in ("evlfu", "lru", "lfu"):
        assert M.stamp_bits_of(policy, 16, n_rows)[:2] == (22, 0)
        c = E.GpuCache(policy, 16, T, 36, 32)
        if policy == "evlfu":
            c.set_batch_policy("setassoc")
        c.set_backing(dev)
        assert _serves_exact(c, dev, n_rows, 2).mean() > 0.5


# ----------------------------------------------------------------------------------------------------------- 5. row updates
def test_row_updates_on_an_lru_tier(E, orc):
    """update_rows between two batches: the next batch serves the new vector from the arena (flag 1, new bits);
    refresh_rows counts the resident copies."""
    n_rows = [300] * 26
    tabs = [t.copy() for t in orc.kaggle_tables(n_rows, 8)]
    dev = [_dev(t) for t in tabs]
    c = E.GpuCache("lru", 16384, 26, 36, 32)
    c.set_backing(dev)
    rs = np.random.RandomState(1)
    rq = np.stack([rs.randint(0, 100, 50) for _ in n_rows], 1).astype(np.int32)      # rows 0..99 only
    hit, _ = c.lookup_batch(_dev(rq))
    assert not hit.any()
    res = _dump(c)
    assert set(res) == {(t + 1, int(rq[b, t])) for b in range(50) for t in range(26)}    # (2 048 sets for <= 1 300 keys)
    keys = np.array([[t, int(rq[0, t])] for t in range(26)] + [[t, 200 + t] for t in range(26)], np.int64)   # 26 resident, 26 not
    vals = rs.uniform(-1, 1, size=(len(keys), 36)).astype(np.float32)
    assert c.update_rows(keys, vals, count=True) == 26
    for (t, row), v in zip(keys, vals):
        tabs[t][row] = v
    hit, out = c.lookup_batch(_dev(rq))
    assert hit.all()                               # everything from the arena, the updated rows included
    _rows_exact(out.cpu().numpy(), tabs, rq)
    assert np.array_equal(out[0].cpu().numpy().view(np.uint32), vals[:26].view(np.uint32))
    assert c.refresh_rows(keys, count=True) == 26
    assert c.refresh_rows(np.array([[0, int(r)] for r in range(300)], np.int64), count=True) == len({int(v) for v in rq[:, 0]})
    assert _dump(c) == {k: 0 for k in res}         # residency did not move; every way was touched by the latest batch
