"""Warm start of the exact batch-1 HOST engine (evs_hostcache_export / evs_hostcache_load): cut a golden trace of the imported
reference anywhere, export, load the export into a fresh cache, continue -- hit flags, rows, final list order and counters are
those of the uncut golden trace, bit for bit.  No GPU involved."""
import numpy as np
import pytest

import _exact_warm as W
from oracle import oracle as orc

import evstore_dlrm_amd as E
from evstore_dlrm_amd import host_cache as H


def _fresh(policy, cap):
    return H.HostCache(policy, cap, 26, 36, 32, "python").set_backing(W.tables())


def _replay(c, reqs, approx=-1, chunk=64):
    hits, outs = [np.zeros((0, 26), bool)], [np.zeros((0, 26, 36), np.float32)]
    for s in range(0, len(reqs), chunk):
        h, o = c.request(reqs[s:s + chunk], approx)
        hits.append(h.astype(bool))
        outs.append(o)
    return np.concatenate(hits), np.concatenate(outs)


@pytest.mark.parametrize("policy,cap,cut", W.CASES)
def test_cut_export_load_continue_is_the_uncut_trace(policy, cap, cut):
    reqs, tabs = W.trace(cap), W.tables()
    a = _fresh(policy, cap)
    _replay(a, reqs[:cut])
    state = a.export_exact_state()
    assert state["entries"].shape == (a.stats()["size"], 3) and state["state"].shape == (20,) and int(state["state"][0]) == 2
    b = _fresh(policy, cap).load_exact_state(state)
    assert W.same_export(b.export_exact_state(), state)          # the export of the loaded cache, taken at once
    assert b.stats() == a.stats()
    hits, outs = _replay(b, reqs[cut:])
    for k in range(26):
        assert np.array_equal(outs[:, k, :], tabs[k][reqs[cut:, k]])
    W.check_final(policy, cap, b, hits, cut)
    a_hits, _ = _replay(a, reqs[cut:])                           # ... and of the exporter, had it gone on
    assert np.array_equal(a_hits, hits) and a.stats() == b.stats()


def test_approx_mode_continues_to_the_golden_trace():
    reqs, cut = W.trace(768), 400
    a = _fresh("evlfu", 768)
    _replay(a, reqs[:cut], approx=20)
    b = _fresh("evlfu", 768).load_exact_state(a.export_exact_state())
    hits, outs = _replay(b, reqs[cut:], approx=20)
    W.check_final("evlfu", 768, b, hits, cut, tag="_approx20")
    _, a_outs = _replay(a, reqs[cut:], approx=20)                # (approx rows are the previous hit's: the exporter's own)
    assert np.array_equal(outs.view(np.uint32), a_outs.view(np.uint32))


def test_state_file_round_trip(tmp_path):
    reqs = W.trace(768)
    a = _fresh("lfu", 768)
    _replay(a, reqs[:700])
    a.save_exact_state(tmp_path / "s.npz")
    b = _fresh("lfu", 768).load_exact_state(tmp_path / "s.npz")
    hits, _ = _replay(b, reqs[700:])
    W.check_final("lfu", 768, b, hits, 700)
    with pytest.raises(E.EvsError) as e:
        _fresh("lfu", 768).load_exact_state(tmp_path / "missing.npz")
    assert e.value.code == E._lib.EVS_EIO


def test_non_strict_load_into_a_larger_cache_derives_the_scalars():
    reqs = W.trace(768)
    a = _fresh("evlfu", 768)
    _replay(a, reqs[:900])
    ex = a.export_exact_state()
    entries = ex["entries"]
    with pytest.raises(E.EvsError) as e:                         # strict: the capacity is the exporter's
        _fresh("evlfu", 1000).load_exact_state(ex)
    assert e.value.code == E._lib.EVS_EINVAL
    b = _fresh("evlfu", 1000).load_exact_state({"entries": entries, "state": None}, strict=False)
    st = b.stats()
    assert st["min_c1"] == int(entries[:, 0].min()) and st["n_perfect"] == int((entries[:, 0] == 26).sum()) and st["size"] == len(entries)
    assert [st[k] for k in ("n_flush", "n_evict", "n_requests", "n_perfect_hits", "n_hits")] == [0] * 5
    np.testing.assert_array_equal(b.dump(), entries)            # before any request: the dump IS the entries
    # every key of the export hits on its first request: request j asks every table for its j-th resident row (a table that
    # has run out repeats its last one, also a hit)
    per_table = [entries[entries[:, 1] == k + 1][:, 2] for k in range(26)]
    assert all(len(p) for p in per_table)
    n_req = max(len(p) for p in per_table)
    rq = np.stack([np.concatenate([p, np.full(n_req - len(p), p[-1])]) for p in per_table], 1).astype(np.int32)
    hits, outs = _replay(b, rq)
    assert hits.all() and b.stats()["size"] == len(entries) and b.stats()["n_evict"] == 0
    for k in range(26):
        assert np.array_equal(outs[:, k, :], W.tables()[k][rq[:, k]])
    # LFU: the lowest frequency present
    l = _fresh("lfu", 768)
    _replay(l, reqs[:700])
    le = l.export_exact_state()
    l2 = _fresh("lfu", 900).load_exact_state({"entries": le["entries"], "state": None}, strict=False)
    assert l2.stats()["min_c1"] == int(le["entries"][:, 0].min())   # (evs_hostcache_stats reports least_freq there)
    np.testing.assert_array_equal(l2.dump(), le["entries"])


def test_load_refusals_leave_the_cache_usable():
    reqs = W.trace(80)
    a = _fresh("evlfu", 80)
    _replay(a, reqs[:9])
    ex = a.export_exact_state()
    with pytest.raises(E.EvsError) as e:                         # not fresh: it has served requests
        a.load_exact_state(ex)
    assert e.value.code == E._lib.EVS_ESTATE
    with pytest.raises(E.EvsError) as e:                         # no backing
        H.HostCache("evlfu", 80).load_exact_state(ex)
    assert e.value.code == E._lib.EVS_ESTATE
    b = _fresh("evlfu", 80)
    bad = dict(ex, entries=ex["entries"].copy())
    bad["entries"][3, 2] = 10 ** 6                               # a row outside its table
    with pytest.raises(E.EvsError) as e:
        b.load_exact_state(bad)
    assert e.value.code == E._lib.EVS_EINVAL and "row outside" in str(e.value)
    with pytest.raises(E.EvsError) as e:                         # other tables than the exporter's
        H.HostCache("evlfu", 80, 26, 36, 32).set_backing([t[:-1] for t in W.tables()]).load_exact_state(ex)
    assert e.value.code == E._lib.EVS_EINVAL
    with pytest.raises(E.EvsError) as e:                         # the batched tier's state is not this one's
        b.load_exact_state({"entries": np.zeros((1, 5), np.int64), "state": np.ones(16, np.int64)})
    assert e.value.code == E._lib.EVS_EINVAL
    b.load_exact_state(ex)                                       # nothing was loaded by the refused calls: still fresh
    hits, _ = _replay(b, reqs[9:])
    W.check_final("evlfu", 80, b, hits, 9)
    with pytest.raises(E.EvsError) as e:                         # ... and a loaded cache is not
        b.load_exact_state(ex)
    assert e.value.code == E._lib.EVS_ESTATE


def test_cache_modules_save_and_load_on_the_host_engine(tmp_path):
    """cache_algo: init -> requests -> save_state -> re-init -> load_state -> requests = the golden hit lists (engine="host")"""
    import torch
    from evstore_dlrm_amd.cache_algo import EvLFU, EvLFU_C1, LFU, LRU
    from evstore_dlrm_amd.emb_storage import storage_manager as sm
    sm.use_device_tables([torch.from_numpy(t) for t in W.tables()], 32, storage=sm.EmbStorage.DUMMY)
    try:
        for mod, init, req, policy, cap, cut in ((EvLFU_C1, lambda: EvLFU_C1.init(768, engine="host"), EvLFU_C1.request_to_ev_lfu, "evlfu", 768, 120),
                                                 (LRU, lambda: LRU.init(64, engine="host"), LRU.request_to_lru, "lru", 64, 100),
                                                 (LFU, lambda: LFU.init(80, engine="host"), LFU.request_to_lfu, "lfu", 80, 100)):
            reqs, hits = W.trace(cap), W.want(policy, cap)[0]
            init()
            for i in range(cut):
                assert req([int(v) for v in reqs[i]])[0] == hits[i].tolist()
            mod.save_state(str(tmp_path / "m.npz"))
            init()
            mod.load_state(str(tmp_path / "m.npz"))
            for i in range(cut, cut + 150):
                assert req([int(v) for v in reqs[i]])[0] == hits[i].tolist(), i
        assert callable(EvLFU.save_state) and callable(EvLFU.load_state)
    finally:
        sm.close_any_db_conn()


def test_inference_loop_loads_instead_of_replaying(tmp_path):
    """inference(..., warm_state=path): the state is loaded before the first stamp, through the cache module by default;
    without it nothing changes"""
    import torch
    from evstore_dlrm_amd import inference_loop as IL
    from evstore_dlrm_amd.cache_algo import EvLFU_C1
    from evstore_dlrm_amd.emb_storage import storage_manager as sm
    ld = [(None, None, i) for i in range(5)]
    seen, loaded = [], []
    fwd = lambda X, lS_o, lS_i: seen.append((lS_i, list(loaded)))
    stamps = IL.inference(ld, fwd, use_gpu=False, device="cpu", warm_state="w.npz", load_state=loaded.append)
    assert [s[0] for s in seen] == list(range(5)) and seen[0][1] == ["w.npz"] and loaded == ["w.npz"] and len(stamps) == 6
    del seen[:]
    IL.inference(ld, fwd, use_gpu=False, device="cpu")
    assert len(seen) == 5 and loaded == ["w.npz"]
    # the default loader is the EvLFU_C1 module's: the loop's requests continue the saved cache's golden trace
    reqs, hits = W.trace(768), W.want("evlfu", 768)[0]
    sm.use_device_tables([torch.from_numpy(t) for t in W.tables()], 32, storage=sm.EmbStorage.DUMMY)
    try:
        EvLFU_C1.init(768, engine="host")
        for i in range(120):
            EvLFU_C1.request_to_ev_lfu([int(v) for v in reqs[i]])
        EvLFU_C1.save_state(str(tmp_path / "c1.npz"))
        EvLFU_C1.init(768, engine="host")
        got = []
        IL.inference([(None, None, reqs[i]) for i in range(120, 200)], lambda X, lS_o, lS_i: got.append(EvLFU_C1.request_to_ev_lfu([int(v) for v in lS_i])[0]),
                     use_gpu=False, device="cpu", warm_state=str(tmp_path / "c1.npz"))
        assert got == [hits[i].tolist() for i in range(120, 200)]
    finally:
        sm.close_any_db_conn()
