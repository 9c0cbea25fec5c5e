"""Warm start of the exact batch-1 DEVICE engine (evs_cache_exact_export / evs_cache_exact_load: one parallel launch builds the
map, the entry records, the lists and the arena): cut a golden trace of the imported reference anywhere, export, load into a
fresh cache, continue -- hit flags, rows, final list order and counters are those of the uncut golden trace, bit for bit.
Also: the resident server behind a load, reduced-precision and pinned-host tables, host <-> device exchange of states, the
C1 + C2 pair, the refusals, the cache modules and the cache manager."""
import numpy as np
import pytest
import torch

import _exact_warm as W
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available()
    E._lib.lib()
    return E


@pytest.fixture(scope="module")
def dev_tabs():
    return [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in W.tables()]


def _gpu(E, policy, cap, tabs, codec=32, variant="python"):
    c = E.GpuCache(policy, cap, 26, 36, codec, variant)
    c.set_backing(tabs)
    return c


def _replay(c, reqs, chunk=64, approx=-1):
    """-> (hit flags, rows) of reqs through request() in launches of `chunk` requests, read back once"""
    n = len(reqs)
    r = torch.from_numpy(np.ascontiguousarray(reqs, dtype=np.int32)).cuda()
    out = torch.empty((n, 26, 36), dtype=torch.float32, device="cuda")
    hit = torch.empty((n, 26), dtype=torch.uint8, device="cuda")
    for s in range(0, n, chunk):
        c.request(r[s:s + chunk], approx, out=out[s:s + chunk], hit=hit[s:s + chunk])
    return hit.cpu().numpy().astype(bool), out.cpu().numpy()


def _rows_are_table_rows(outs, reqs, tabs=None):
    tabs = W.tables() if tabs is None else tabs
    for k in range(26):
        assert np.array_equal(outs[:, k, :].view(np.uint32), tabs[k][reqs[:, k]].view(np.uint32)), k


@pytest.mark.parametrize("chunk", [1, 64])
@pytest.mark.parametrize("policy,cap,cut", W.CASES)
def test_cut_export_load_continue_is_the_uncut_trace(E, dev_tabs, policy, cap, cut, chunk):
    reqs = W.trace(cap)
    a = _gpu(E, policy, cap, dev_tabs)
    _replay(a, reqs[:cut])
    state = a.export_exact_state()
    assert state["entries"].shape == (a.stats()["size"], 3) and int(state["state"][0]) == 2
    b = _gpu(E, policy, cap, dev_tabs).load_exact_state(state)
    assert W.same_export(b.export_exact_state(), state)          # the export of the loaded cache, taken at once
    assert b.stats() == a.stats()
    hits, outs = _replay(b, reqs[cut:], chunk)
    _rows_are_table_rows(outs, reqs[cut:])
    W.check_final(policy, cap, b, hits, cut)


def test_approx_mode_continues_to_the_golden_trace(E, dev_tabs):
    reqs, cut = W.trace(768), 400
    a = _gpu(E, "evlfu", 768, dev_tabs)
    _replay(a, reqs[:cut], approx=20)
    b = _gpu(E, "evlfu", 768, dev_tabs).load_exact_state(a.export_exact_state())
    hits, outs = _replay(b, reqs[cut:], approx=20)
    W.check_final("evlfu", 768, b, hits, cut, tag="_approx20")
    _, a_outs = _replay(a, reqs[cut:], approx=20)
    assert np.array_equal(outs.view(np.uint32), a_outs.view(np.uint32))


def test_the_resident_server_continues_a_loaded_cache(E, dev_tabs):
    reqs, cut = W.trace(768), 120
    a = _gpu(E, "evlfu", 768, dev_tabs)
    _replay(a, reqs[:cut])
    b = _gpu(E, "evlfu", 768, dev_tabs).load_exact_state(a.export_exact_state())
    b.serve_start(n_slots=4, idle_us=200)
    rest = reqs[cut:]
    out = torch.empty((len(rest), 26, 36), dtype=torch.float32, device="cuda")
    hits = np.zeros((len(rest), 26), bool)
    torch.cuda.synchronize()
    for i, rq in enumerate(rest):
        hits[i] = b.serve_request_to(rq, out[i]).astype(bool)
    b.serve_stop()
    _rows_are_table_rows(out.cpu().numpy(), rest)
    W.check_final("evlfu", 768, b, hits, cut)


@pytest.mark.parametrize("cut", [30, 700])
@pytest.mark.parametrize("codec", [8, 4])
def test_reduced_precision_rows_come_back_from_the_arena(E, codec, cut):
    """a hit is served from the arena, so the decoded rows of the continuation check the load's row copy (36- and 18-byte rows:
    the 4-byte and the byte-wise pieces of the copy)"""
    reqs = W.trace(300)
    raws = [orc.encode_table(np.clip(w * 8, -1, 1), codec) for w in W.tables()]
    dev = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in raws]
    a = _gpu(E, "evlfu", 300, dev, codec)
    _replay(a, reqs[:cut])
    b = _gpu(E, "evlfu", 300, dev, codec).load_exact_state(a.export_exact_state())
    hits, outs = _replay(b, reqs[cut:])
    assert hits[:50].any()
    _rows_are_table_rows(outs, reqs[cut:], [orc.decode(r, codec, 36) for r in raws])
    W.check_final("evlfu", 300, b, hits, cut)


def test_pinned_host_tables(E):
    reqs, cut = W.trace(64), 700
    host = [torch.from_numpy(np.ascontiguousarray(t)).pin_memory() for t in W.tables()]
    a = _gpu(E, "lru", 64, host)
    _replay(a, reqs[:cut])
    b = _gpu(E, "lru", 64, host).load_exact_state(a.export_exact_state())
    hits, outs = _replay(b, reqs[cut:])
    _rows_are_table_rows(outs, reqs[cut:])
    W.check_final("lru", 64, b, hits, cut)


def test_registered_file_tables_are_accepted_and_staged_ones_refused(E, dev_tabs, tmp_path):
    reqs, cut = W.trace(80), 9
    paths = []
    for k, w in enumerate(W.tables()):
        w.tofile(tmp_path / ("ev-table-%d.bin" % (k + 1)))
        paths.append(str(tmp_path / ("ev-table-%d.bin" % (k + 1))))
    a = _gpu(E, "evlfu", 80, dev_tabs)
    _replay(a, reqs[:cut])
    ex = a.export_exact_state()
    ex = {"entries": ex["entries"], "state": ex["state"]}
    staged = E.FileTier(paths, 144, 0)
    assert not any(staged.registered)
    c = E.GpuCache("evlfu", 80, 26, 36, 32)
    c.set_file_backing(staged)
    with pytest.raises(E.EvsError) as e:
        c.load_exact_state(ex)
    assert e.value.code == E._lib.EVS_ESTATE and "staged" in str(e.value)
    reg = E.FileTier(paths, 144, 1 << 30)
    assert all(reg.registered)
    b = E.GpuCache("evlfu", 80, 26, 36, 32)
    b.set_file_backing(reg)
    b.load_exact_state(ex)
    hits, outs = _replay(b, reqs[cut:])
    _rows_are_table_rows(outs, reqs[cut:])
    W.check_final("evlfu", 80, b, hits, cut)


@pytest.mark.parametrize("policy,cap,cut", [("evlfu", 80, 7), ("lfu", 768, 700)])
def test_host_and_device_states_are_interchangeable(E, dev_tabs, policy, cap, cut):
    from evstore_dlrm_amd import host_cache as H
    reqs = W.trace(cap)
    g = _gpu(E, policy, cap, dev_tabs)
    _replay(g, reqs[:cut])
    h = H.HostCache(policy, cap, 26, 36, 32, "python").set_backing(W.tables())
    h.request(reqs[:cut])
    ge, he = g.export_exact_state(), h.export_exact_state()
    assert W.same_export(ge, he)
    g2 = _gpu(E, policy, cap, dev_tabs).load_exact_state(he)     # host -> device
    hits, outs = _replay(g2, reqs[cut:])
    _rows_are_table_rows(outs, reqs[cut:])
    W.check_final(policy, cap, g2, hits, cut)
    h2 = H.HostCache(policy, cap, 26, 36, 32, "python").set_backing(W.tables()).load_exact_state(ge)   # device -> host
    hh, ho = h2.request(reqs[cut:])
    _rows_are_table_rows(ho, reqs[cut:])
    W.check_final(policy, cap, h2, hh.astype(bool), cut)


@pytest.mark.parametrize("cut", [2, 40, 400])
def test_tier_pair(E, cut):
    """request_c1c2 over a C1 (u8, 96 entries) + C2 (u4, 192 entries) pair: each cache exported and loaded on its own, the
    continuation = the uncut run on the same engine = oracle.C1C2.  (cut 2: C1 still filling.)"""
    from evstore_dlrm_amd import gpu_cache
    rs = np.random.RandomState(3)
    ws = [rs.uniform(-1, 1, size=(400, 36)).astype(np.float32) for _ in range(26)]
    raw8, raw4 = [orc.encode_table(w, 8) for w in ws], [orc.encode_table(w, 4) for w in ws]
    dec8, dec4 = [orc.decode(r, 8, 36) for r in raw8], [orc.decode(r, 4, 36) for r in raw4]
    reqs = np.zeros((600, 26), np.int32)
    for i in range(len(reqs)):
        reqs[i] = rs.randint(0, 400, 26)
        if i > 20 and rs.rand() < 0.4:
            reqs[i] = reqs[i - 1 - rs.randint(15)]
            reqs[i] = np.where(rs.rand(26) < 0.07, rs.randint(0, 400, 26), reqs[i])
    cap1, cap2 = 96, 192
    o = orc.C1C2(cap1, cap2, dec8, dec4)
    want_tier, want_out, perfect = [], [], 0
    for rq in reqs:
        t, out, p = o.request(rq)
        want_tier.append(t.copy()); want_out.append(out.copy()); perfect += p
    want_tier, want_out = np.stack(want_tier), np.stack(want_out)
    d8, d4 = [torch.from_numpy(r).cuda() for r in raw8], [torch.from_numpy(r).cuda() for r in raw4]
    r = torch.from_numpy(reqs).cuda()

    def pair():
        return _gpu(E, "evlfu", cap1, d8, 8, "cpp"), _gpu(E, "evlfu", cap2, d4, 4, "cpp")

    def run(c1, c2, lo, hi):
        t, out = gpu_cache.request_c1c2(c1, c2, r[lo:hi].contiguous())
        return t.cpu().numpy(), out.cpu().numpy()

    u1, u2 = pair()                                              # the uncut run on the same engine
    ut, uo = run(u1, u2, 0, len(reqs))
    a1, a2 = pair()
    run(a1, a2, 0, cut)
    if cut == 2:
        assert a1.stats()["size"] < cap1
    e1, e2 = a1.export_exact_state(), a2.export_exact_state()
    b1, b2 = pair()
    b1.load_exact_state(e1)
    b2.load_exact_state(e2)
    bt, bo = run(b1, b2, cut, len(reqs))
    assert np.array_equal(bt, ut[cut:]) and np.array_equal(bt, want_tier[cut:])
    assert np.array_equal(bo.view(np.uint32), uo[cut:].view(np.uint32)) and np.array_equal(bo.view(np.uint32), want_out[cut:].view(np.uint32))
    for got, same_engine, oracle_tier in ((b1, u1, o.c1), (b2, u2, o.c2)):
        np.testing.assert_array_equal(got.dump(), same_engine.dump())
        np.testing.assert_array_equal(got.dump(), oracle_tier.dump())
        assert got.stats() == same_engine.stats()
    assert b1.stats()["n_perfect_hits"] == perfect


def test_refusals_leave_the_cache_usable(E, dev_tabs):
    reqs = W.trace(80)
    a = _gpu(E, "evlfu", 80, dev_tabs)
    _replay(a, reqs[:9])
    ex = a.export_exact_state()

    def refused(c, state, code, word=None):
        with pytest.raises(E.EvsError) as e:
            c.load_exact_state(state)
        assert e.value.code == code and (word is None or word in str(e.value)), str(e.value)

    def still_serves(c):
        h, o = _replay(c, reqs[:3])
        _rows_are_table_rows(o, reqs[:3])

    refused(a, ex, E._lib.EVS_ESTATE, "not fresh")               # a cache that has served a request
    still_serves(a)
    bat = _gpu(E, "evlfu", 80, dev_tabs)                         # a cache on the batched path
    bat.lookup_batch(torch.from_numpy(reqs[:4].astype(np.int32)).cuda())
    refused(bat, ex, E._lib.EVS_ESTATE, "batched")
    with pytest.raises(E.EvsError) as e:
        bat.export_exact_state()
    assert e.value.code == E._lib.EVS_ESTATE
    bat.lookup_batch(torch.from_numpy(reqs[:4].astype(np.int32)).cuda())
    srv = _gpu(E, "evlfu", 80, dev_tabs)                         # a server is armed
    srv.serve_start(n_slots=2, idle_us=200)
    refused(srv, ex, E._lib.EVS_ESTATE, "server")
    hit, _ = srv.serve_request(reqs[0])
    assert not hit.any()
    srv.serve_stop()
    nob = E.GpuCache("evlfu", 80, 26, 36, 32)                    # no backing
    refused(nob, ex, E._lib.EVS_ESTATE)
    c = _gpu(E, "evlfu", 80, dev_tabs)
    bad = dict(ex, entries=ex["entries"].copy())
    bad["entries"][3, 2] = 10 ** 6                               # a row outside its table
    refused(c, bad, E._lib.EVS_EINVAL, "row outside")
    dup = dict(ex, entries=ex["entries"].copy())
    dup["entries"][4, 1:] = dup["entries"][3, 1:]
    refused(c, dup, E._lib.EVS_EINVAL, "duplicate")
    refused(_gpu(E, "evlfu", 81, dev_tabs), ex, E._lib.EVS_EINVAL, "capacity")      # strict: the exporter's capacity
    refused(_gpu(E, "evlfu", 80, dev_tabs, variant="cython"), ex, E._lib.EVS_EINVAL, "constants")
    refused(_gpu(E, "lru", 80, dev_tabs), ex, E._lib.EVS_EINVAL, "another policy")
    still_serves(c)                                              # the refused loads loaded nothing: an empty cache serves table rows
    ok = _gpu(E, "evlfu", 80, dev_tabs).load_exact_state(ex)
    with pytest.raises(E.EvsError) as e:                         # an exact-path cache: the batched lookups are refused as ever
        ok.lookup_batch(torch.from_numpy(reqs[:4].astype(np.int32)).cuda())
    assert e.value.code == E._lib.EVS_ESTATE
    refused(ok, ex, E._lib.EVS_ESTATE, "not fresh")
    with pytest.raises(E.EvsError) as e:                         # ... and its state is not the batched tier's
        ok.load_state(ex)
    hits, _ = _replay(ok, reqs[9:])
    W.check_final("evlfu", 80, ok, hits, 9)


def test_non_strict_load_into_a_larger_cache(E, dev_tabs):
    reqs = W.trace(768)
    a = _gpu(E, "evlfu", 768, dev_tabs)
    _replay(a, reqs[:900])
    entries = a.export_exact_state()["entries"]
    b = _gpu(E, "evlfu", 1000, dev_tabs).load_exact_state({"entries": entries, "state": None}, strict=False)
    st = b.stats()
    assert st["min_c1"] == int(entries[:, 0].min()) and st["n_perfect"] == int((entries[:, 0] == 26).sum()) and st["size"] == len(entries)
    assert [st[k] for k in ("n_flush", "n_evict", "n_requests", "n_perfect_hits", "n_hits")] == [0] * 5
    np.testing.assert_array_equal(b.dump(), entries)
    per_table = [entries[entries[:, 1] == k + 1][:, 2] for k in range(26)]
    n_req = max(len(p) for p in per_table)
    rq = np.stack([np.concatenate([p, np.full(n_req - len(p), p[-1])]) for p in per_table], 1).astype(np.int32)
    hits, outs = _replay(b, rq, chunk=16)
    assert hits.all() and b.stats()["size"] == len(entries)
    _rows_are_table_rows(outs, rq)
    # 1000 - n free entries are there to be taken: new keys go in without an eviction until the cache is full
    free = 1000 - len(entries)
    new = np.stack([np.arange(free // 26 + 1) % int(n) for n in W.golden()["n_rows"]], 1).astype(np.int32)
    _replay(b, new)
    assert b.stats()["size"] <= 1000 and len(np.unique(b.dump()[:, 1:], axis=0)) == b.stats()["size"]


def test_the_unpacked_map_form(E):
    """capacity > 2^25: the map keeps the entry beside the key (slot_entry[]) instead of inside the key's word.  1 000 entries
    into a cache of 2^25 + 8, then 200 requests against oracle.LRU (the oracle with a smaller capacity: nothing is evicted on
    either side, so the capacity is not observable)"""
    rs = np.random.RandomState(8)
    T, d = 4, 4
    tabs = [rs.uniform(-1, 1, size=(2000, d)).astype(np.float32) for _ in range(T)]
    o = orc.LRU(1 << 16, tabs, d)
    for j in range(250):
        o.request(np.full(T, j, np.int32))
    entries = np.concatenate([np.zeros((1000, 1), np.int64), o.dump()], 1)
    assert entries.shape == (1000, 3)
    c = E.GpuCache("lru", (1 << 25) + 8, T, d, 32)
    c.set_backing([torch.from_numpy(t).cuda() for t in tabs])
    c.load_exact_state({"entries": entries, "state": None}, strict=False)
    assert c.stats()["size"] == 1000
    reqs = rs.randint(0, 400, size=(200, T)).astype(np.int32)
    want_hit, want_out = [], []
    for rq in reqs:
        h, v = o.request(rq)
        want_hit.append(h.copy()); want_out.append(v.copy())
    hit, out = c.request(torch.from_numpy(reqs).cuda())
    assert np.array_equal(hit.cpu().numpy().astype(bool), np.stack(want_hit)) and 0 < np.stack(want_hit).sum() < reqs.size
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.stack(want_out).view(np.uint32))
    np.testing.assert_array_equal(c.dump()[:, 1:], o.dump())
    st = c.stats()
    assert st["n_evict"] == 0 and st["n_requests"] == 200 and st["n_hits"] == int(np.stack(want_hit).sum())


def test_cache_modules_save_and_load_under_both_engines(E, tmp_path):
    """cache_algo.EvLFU_C1: init -> requests -> save_state -> re-init -> load_state -> requests = the golden hit lists, under
    engine="host" and engine="gpu", and with the state saved under one engine and loaded under the other"""
    from evstore_dlrm_amd.cache_algo import EvLFU_C1
    from evstore_dlrm_amd.emb_storage import storage_manager as sm
    reqs, hits = W.trace(768), W.want("evlfu", 768)[0]
    sm.use_device_tables([torch.from_numpy(np.ascontiguousarray(t)).pin_memory() for t in W.tables()], 32, storage=sm.EmbStorage.PINNED)
    cut, n = 130, 260
    try:
        for save_engine, load_engine, use_gpu in (("host", "host", False), ("gpu", "gpu", False), ("gpu", "gpu", True),
                                                  ("host", "gpu", True), ("gpu", "host", False)):
            EvLFU_C1.init(768, engine=save_engine)
            for i in range(cut):
                assert EvLFU_C1.request_to_ev_lfu([int(v) for v in reqs[i]], use_gpu=use_gpu)[0] == hits[i].tolist(), i
            path = str(tmp_path / ("%s_%s_%d.npz" % (save_engine, load_engine, use_gpu)))
            EvLFU_C1.save_state(path)
            EvLFU_C1.init(768, engine=load_engine)
            EvLFU_C1.load_state(path)
            assert EvLFU_C1._m.engine == load_engine
            for i in range(cut, n):
                h, ly = EvLFU_C1.request_to_ev_lfu([int(v) for v in reqs[i]], use_gpu=use_gpu)
                assert h == hits[i].tolist(), (save_engine, load_engine, i)
                assert np.array_equal(ly[7].detach().cpu().numpy()[0], W.tables()[7][reqs[i][7]])
            assert EvLFU_C1.stats()["n_requests"] == n
    finally:
        sm.close_any_db_conn()


@pytest.mark.parametrize("layers,serve", [(1, False), (1, True), (2, True)])
def test_the_manager_on_the_device_engine(tmp_path, layers, serve):
    """ev_lookup on the GPU engine -- launched per request, and behind the resident server, which is taken off the tiers
    for the load and armed again: a second process loads the first one's state and continues"""
    W.check_two_processes(tmp_path, layers, backing="hbm", env_extra={"EVS_MANAGER_SERVE": "1"} if serve else None,
                          engine=3 if serve else 2)
