"""Online row updates, the part that needs no GPU: the argument checks of the four entry points, and the host engine's
refresh_rows held to the golden traces -- a delta written into the tables between the two halves of the recorded stream
must leave every hit flag and the final lists where the reference's policies put them (the update moves no policy state)
while every served row equals the table contents at the time of its request.  All comparisons are bit-exact."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from oracle import oracle as orc

import evstore_dlrm_amd as E
from evstore_dlrm_amd import host_cache as H

from _row_updates import D, T, golden_final as _golden_final, make_delta, unpack as _unpack


def test_argument_checks_without_a_gpu():
    L = E._lib.lib()
    EINVAL = E._lib.EVS_EINVAL
    one = (C.c_void_p * 1)(None)
    rows = (C.c_int64 * 1)(0)
    # evs_table_update_rows(codec, d, n_tables, tables, n_rows, n, keys, values, values_stride, stream)
    assert L.evs_table_update_rows(7, 36, 1, one, rows, 4, None, None, 36, None) == EINVAL and b"codec" in L.evs_last_error()
    assert L.evs_table_update_rows(4, 35, 1, one, rows, 4, None, None, 35, None) == EINVAL and b"even" in L.evs_last_error()
    assert L.evs_table_update_rows(8, 36, 1, one, rows, -1, None, None, 36, None) == EINVAL and b"n = -1" in L.evs_last_error()
    assert L.evs_table_update_rows(8, 36, 1, one, rows, 4, None, None, 36, None) == EINVAL and b"NULL" in L.evs_last_error()
    assert L.evs_table_update_rows(8, 36, 0, one, rows, 4, None, None, 36, None) == EINVAL and b"n_tables" in L.evs_last_error()
    assert L.evs_table_update_rows(8, 36, 1, one, rows, 0, None, None, 36, None) == 0
    # keys not 8-byte aligned, a value stride below d: refused before the device is touched (fake addresses, never followed)
    fake = (C.c_void_p * 1)(4096)
    rows1 = (C.c_int64 * 1)(10)
    assert L.evs_table_update_rows(8, 36, 1, fake, rows1, 4, 4100, 8192, 36, None) == EINVAL and b"aligned" in L.evs_last_error()
    assert L.evs_table_update_rows(8, 36, 1, fake, rows1, 4, 4104, 8192, 35, None) == EINVAL and b"values_stride" in L.evs_last_error()
    assert L.evs_table_update_rows(8, 36, 1, fake, rows1, 4, 4104, 8192, -36, None) == EINVAL and b"values_stride" in L.evs_last_error()
    # evs_cache_update_rows(c, n, keys, values, values_stride, n_resident, stream)
    assert L.evs_cache_update_rows(None, 4, None, None, 36, None, None) == EINVAL and b"NULL" in L.evs_last_error()
    assert L.evs_cache_update_rows(None, -2, None, None, 36, None, None) == EINVAL and b"n = -2" in L.evs_last_error()
    assert L.evs_cache_update_rows(None, 0, None, None, 36, None, None) == 0
    # evs_cache_refresh_rows(c, n, keys, n_resident, stream)
    assert L.evs_cache_refresh_rows(None, 4, None, None, None) == EINVAL and b"NULL" in L.evs_last_error()
    assert L.evs_cache_refresh_rows(None, -1, None, None, None) == EINVAL and b"n = -1" in L.evs_last_error()
    assert L.evs_cache_refresh_rows(None, 0, None, None, None) == 0
    # evs_hostcache_refresh_rows(c, n, keys_host, n_resident_host)
    assert L.evs_hostcache_refresh_rows(None, 4, None, None) == EINVAL and b"NULL" in L.evs_last_error()
    assert L.evs_hostcache_refresh_rows(None, -1, None, None) == EINVAL and b"n = -1" in L.evs_last_error()
    cnt = C.c_int64(7)
    assert L.evs_hostcache_refresh_rows(None, 0, None, C.byref(cnt)) == 0 and cnt.value == 0
    # a key array without a cache, a cache without backing
    keys = np.zeros((4, 2), np.int32)
    assert L.evs_hostcache_refresh_rows(None, 4, keys.ctypes.data, None) == EINVAL
    c = H.HostCache("lru", 8, 1, 16, 32)
    assert L.evs_hostcache_refresh_rows(c._h, 4, keys.ctypes.data, None) == E._lib.EVS_ESTATE and b"backing" in L.evs_last_error()


def test_host_refresh_skips_keys_out_of_range():
    tab = np.arange(10 * 16, dtype=np.float32).reshape(10, 16)
    c = H.HostCache("lru", 8, 1, 16, 32).set_backing([tab])
    c.request(np.array([[3]], np.int32))
    c.backing_tables()[0][3] = -1.0
    with pytest.raises(E.EvsError) as e:
        c.refresh_rows([[0, 3], [0, 10], [1, 0], [0, -1]])
    assert e.value.code == E._lib.EVS_EINDEX
    _, out = c.request(np.array([[3]], np.int32))   # the key in range was refreshed all the same
    assert np.array_equal(out[0, 0], np.full(16, -1.0, np.float32))


def test_backing_tables_are_what_the_engine_reads():
    big = np.arange(20 * 16, dtype=np.float32).reshape(10, 32)
    view = big[:, :16]   # not contiguous: set_backing copies it
    c = H.HostCache("lru", 4, 1, 16, 32).set_backing([view])
    bt = c.backing_tables()
    assert len(bt) == 1 and bt[0].flags["C_CONTIGUOUS"] and not np.shares_memory(bt[0], big)
    bt[0][5] = 7.0
    _, out = c.request(np.array([[5]], np.int32))
    assert np.array_equal(out[0, 0], np.full(16, 7.0, np.float32))


def test_dedup_keeps_the_last_occurrence():
    import torch
    from evstore_dlrm_amd import dlrm_ops
    keys = torch.tensor([[0, 5], [1, 5], [0, 5], [2, 9], [1, 5], [0, 6]], dtype=torch.int32)
    vals = torch.arange(6, dtype=torch.float32).reshape(6, 1).repeat(1, 4)
    k, v = dlrm_ops.dedup_last(keys, vals)
    assert k.tolist() == [[0, 5], [2, 9], [1, 5], [0, 6]] and v[:, 0].tolist() == [2.0, 3.0, 4.0, 5.0]
    k, v = dlrm_ops.delta_tensors([[3, 1], [3, 1]], [[1.0] * 4, [2.0] * 4], "cpu", 4)
    assert k.dtype == torch.int32 and k.tolist() == [[3, 1]] and v.tolist() == [[2.0] * 4]
    k, v = dlrm_ops.delta_tensors(np.zeros((0, 2), np.int64), None, "cpu", 4)
    assert tuple(k.shape) == (0, 2) and v is None


# ---- the golden-trace protocol ------------------------------------------------------------------------------------------------
def _replay_with_delta(policy, cap, codec, refresh):
    """-> (hits, final dump, wrong rows as a list of (request, table, resident-in-delta))"""
    t = load_golden("cache_traces")
    n_rows = [int(n) for n in t["n_rows"]]
    fp32 = orc.kaggle_tables(n_rows, int(t["table_seed"]))
    if codec == 32:
        raws = [np.array(w, np.float32) for w in fp32]
    else:
        raws = [orc.encode_table(np.clip(w * 8, -1, 1), codec) for w in fp32]
    reqs = t["requests"]
    half = len(reqs) // 2
    c = H.HostCache(policy, cap, T, D, codec).set_backing(raws)
    bt = c.backing_tables()

    def current(k, rows):
        return orc.decode(bt[k][rows], codec, D) if codec != 32 else bt[k][rows]

    wrong, hits = [], []
    h, o = c.request(reqs[:half])
    hits.append(h.astype(bool))
    for k in range(T):
        assert np.array_equal(o[:, k, :].view(np.uint32), current(k, reqs[:half, k]).view(np.uint32))
    dump0, stats0 = c.dump(), c.stats()
    rs = np.random.RandomState(5)
    keys, n_res, n_non, n_later = make_delta(dump0, reqs[half:], n_rows, rs)
    assert n_res >= 64 and n_non >= 64 and n_later >= 1
    vals = rs.uniform(-1, 1, size=(len(keys), D)).astype(np.float32)
    enc = vals if codec == 32 else orc.encode_table(vals, codec)
    for (k, r), v in zip(keys, enc):
        bt[k][r] = v
    if refresh:
        assert c.refresh_rows(keys) == n_res
        np.testing.assert_array_equal(c.dump(), dump0)
        assert c.stats() == stats0
    res_set = {(int(k), int(r)) for k, r in keys[:n_res]}
    h, o = c.request(reqs[half:])
    hits.append(h.astype(bool))
    for k in range(T):
        bad = np.nonzero((o[:, k, :].view(np.uint32) != current(k, reqs[half:, k]).view(np.uint32)).any(1))[0]
        wrong += [(half + int(i), k, (k, int(reqs[half + i, k])) in res_set) for i in bad]
    return t, np.concatenate(hits), c.dump(), wrong


@pytest.mark.parametrize("codec", [32, 8])
@pytest.mark.parametrize("policy", ["evlfu", "lru", "lfu"])
def test_host_engine_refresh_keeps_trace_and_rows(policy, codec):
    cap = 300
    t, hits, final, wrong = _replay_with_delta(policy, cap, codec, refresh=True)
    assert np.array_equal(hits, _unpack(t["%s_cap%d_hits" % (policy, cap)], len(hits)))
    _golden_final(t, policy, cap, final)
    assert wrong == []


@pytest.mark.parametrize("codec", [32, 8])
@pytest.mark.parametrize("policy", ["evlfu", "lru", "lfu"])
def test_without_refresh_the_stale_copy_is_seen(policy, codec):
    """the same run with the refresh_rows call left out: the policy is none the wiser (same trace), but a resident key of the
    delta is served its OLD row -- the defect this feature exists for, and proof that the comparison above can see it"""
    cap = 300
    t, hits, final, wrong = _replay_with_delta(policy, cap, codec, refresh=False)
    assert np.array_equal(hits, _unpack(t["%s_cap%d_hits" % (policy, cap)], len(hits)))
    assert any(res for _, _, res in wrong), "no stale row was served without the refresh"
    assert all(res for _, _, res in wrong)   # (and only resident delta keys can be stale)


def test_module_cache_update_rows_on_the_host_engine():
    """cache_algo's module surface: a delta through _ModuleCache.update_rows with the host engine bound"""
    from evstore_dlrm_amd.cache_algo import _common
    m = _common._ModuleCache("lru")
    tabs = [np.random.RandomState(k).rand(50, m.dim).astype(np.float32) for k in range(m.n_tables)]
    m.init(100, engine="host")
    m._make_host(tabs)
    m._bound = True
    ids = [k % 50 for k in range(m.n_tables)]
    m.request_rows(ids)
    new = np.full((2, m.dim), 3.5, np.float32)
    assert m.update_rows([[0, ids[0]], [1, 49]], new) == 1   # (1, 49) is not resident
    hit, rows = m.request_rows(ids)
    assert all(hit) and np.array_equal(rows[0], new[0]) and np.array_equal(rows[1], tabs[1][ids[1]])
    assert np.array_equal(m.cache.backing_tables()[1][49], new[1])
    m8 = _common._ModuleCache("lru")
    m8.init(100, engine="host")
    from evstore_dlrm_amd.emb_storage import storage_manager
    old = storage_manager.ev_precs
    try:
        storage_manager.ev_precs = 8
        m8._make_host([np.zeros((50, m.dim), np.uint8) for _ in range(m.n_tables)])
        m8._bound = True
        with pytest.raises(NotImplementedError):
            m8.update_rows([[0, 0]], new[:1])
    finally:
        storage_manager.ev_precs = old


def test_module_cache_update_rows_skips_and_reports_keys_out_of_range():
    """host engine: a negative row must not wrap round to another row of the table, a bad table index is skipped like a bad
    row; the keys in range are applied and the call then reports EVS_EINDEX"""
    from evstore_dlrm_amd.cache_algo import _common
    m = _common._ModuleCache("lru")
    tabs = [np.random.RandomState(k).rand(50, m.dim).astype(np.float32) for k in range(m.n_tables)]
    before = [t.copy() for t in tabs]
    m.init(100, engine="host")
    m._make_host(tabs)
    m._bound = True
    new = np.full((5, m.dim), 2.25, np.float32)
    with pytest.raises(E.EvsError) as e:
        m.update_rows([[0, -1], [m.n_tables, 0], [-1, 3], [2, 50], [3, 7]], new)
    assert e.value.code == E._lib.EVS_EINDEX
    bt = m.cache.backing_tables()
    before[3][7] = new[4]
    for k in range(m.n_tables):
        assert np.array_equal(bt[k], before[k]), k


class _StubTables:
    """what _deferred_result needs of an EVTables, without a device"""
    d, device = 4, "cpu"

    def __init__(self):
        self._pending = []

    def __len__(self):
        return 3


def test_materialize_pending_computes_only_what_somebody_can_still_see(monkeypatch):
    """update_rows computes pending deferred apply_emb results first -- but only those a caller can still look at and that
    can still be computed.  A result the fused interact_features consumed whose list has died (what every step of a serving
    loop leaves behind) is skipped, also when the loop has since refilled its index buffer in place: no gather is launched
    for it and nothing is raised.  A held result is computed once; a held result whose indices were rewritten is left to
    raise on its own first use; a fifth simultaneous result of one shape (not pooled) is covered like the others."""
    import torch
    from evstore_dlrm_amd import dlrm_ops
    if not dlrm_ops.DEFER_POOLING:   # (a torch build without the two internals the deferred list needs: nothing is ever pending)
        return
    calls = []

    def fake_apply_emb(lS_o, lS_i, ev, v_W_l=None, out=None, lazy=None, one_index_per_bag=False, _into=None, **kw):
        calls.append(_into)
        _into.fill_(float(len(calls)))

    monkeypatch.setattr(dlrm_ops, "apply_emb", fake_apply_emb)
    monkeypatch.setattr(dlrm_ops, "_defer_pool", {})
    ev = _StubTables()
    B = 8
    off = torch.arange(B).repeat(3, 1)

    def result():
        idx = torch.zeros((3, B), dtype=torch.int64)
        return dlrm_ops._deferred_result(off, idx, ev, True, B), idx

    # consumed by the fused path, list dropped, index buffer refilled in place: invisible
    ly, idx = result()
    ly._evs_defer.consumed = True
    del ly
    idx.add_(1)
    dlrm_ops.materialize_pending(ev)
    assert calls == []
    # never consumed, list dropped: nobody can look either
    ly, idx = result()
    del ly
    dlrm_ops.materialize_pending(ev)
    assert calls == []
    # held: computed once, before the write; a second update has nothing left to do
    ly, idx = result()
    st = ly._evs_defer
    dlrm_ops.materialize_pending(ev)
    assert len(calls) == 1 and st.done and calls[0] is st.buf
    dlrm_ops.materialize_pending(ev)
    assert len(calls) == 1
    # held, indices rewritten in place: not computable -- update_rows stays silent, the first use raises its own error
    ly2, idx2 = result()
    idx2.add_(1)
    dlrm_ops.materialize_pending(ev)
    assert len(calls) == 1 and not ly2._evs_defer.done
    with pytest.raises(RuntimeError, match="modified in place"):
        ly2._evs_defer.materialize()
    # a row that escaped a dead list is still a way to look at the result
    ly3, _ = result()
    row = ly3[1]
    del ly3
    dlrm_ops.materialize_pending(ev)
    assert len(calls) == 2
    del row
    # more simultaneous results of one shape than the pool keeps: every one of them is covered
    held = [result() for _ in range(7)]
    assert len({id(h[0]._evs_defer) for h in held}) == 7
    n0 = len(calls)
    dlrm_ops.materialize_pending(ev)
    assert len(calls) == n0 + 7 and all(h[0]._evs_defer.done for h in held)
    # a result of OTHER tables is not this update's business
    other = _StubTables()
    idx = torch.zeros((3, B), dtype=torch.int64)
    ly4 = dlrm_ops._deferred_result(off, idx, other, True, B)
    dlrm_ops.materialize_pending(ev)
    assert not ly4._evs_defer.done
