"""Online row updates on the GPU (include/evstore_hip.h: evs_table_update_rows / evs_cache_update_rows /
evs_cache_refresh_rows): a delta of (table, row) -> new fp32 vector is encoded, written into the table and into every
cached copy, in stream order, and the policy state does not move by one bit.  Every value comparison is bit-exact (raw
bytes / view(np.uint32)); only the interaction result goes through the accuracy helper of the cache tests."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

import _row_updates as ru
from _row_updates import D, T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available()
    E._lib.lib()
    return E


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    return torch.cuda.current_stream().cuda_stream


SPECIAL = np.array([0.0, 1.0, -1.0, 0.65, -0.65, 0.8, -0.8, 0.6, 0.4, 0.25, 0.015, 0.00025, -0.00025, 0.66, -0.66, 0.999],
                   np.float32)


def _values(rs, n, d, neg_zero=False):
    """(-0.0 only where raw bytes are compared: a bag sum starts from +0.0, so pooling -0.0 alone gives +0.0 on any engine)"""
    v = rs.uniform(-1, 1, size=(n, d)).astype(np.float32)   # (inside [-1, 1]: the u4 code of v < -1 decodes to NaN)
    m = rs.rand(n, d) < 0.15
    v[m] = SPECIAL[rs.randint(0, len(SPECIAL), int(m.sum()))]
    if neg_zero:
        v[rs.rand(n, d) < 0.05] = -0.0
    return v


def _distinct_keys(rs, n_rows, n):
    keys = set()
    while len(keys) < n:
        k = int(rs.randint(0, len(n_rows)))
        keys.add((k, int(rs.randint(0, n_rows[k]))))
    return np.array(sorted(keys), np.int64)[rs.permutation(n)]


# ---- tables ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec,d", [(32, 36), (16, 36), (8, 36), (4, 36), (32, 16), (32, 64), (8, 20), (16, 12)])
def test_table_update_rows(E, orc, codec, d):
    """EVTables.update_rows: the WHOLE raw table equals a host mirror byte for byte (untouched rows included), the mirror
    built with the oracle's encoders and cross-checked against evs_encode_table over the modified fp32 tables; apply_emb
    over the updated tables equals the oracle.  ((8, 20) and (16, 12): row sizes without a compiled shape -- table bytes only.)"""
    rs = np.random.RandomState(codec * 100 + d)
    n_rows = [500, 3, 2000, 17, 64, 1]
    w = [_values(rs, n, d) for n in n_rows]
    ev32 = E.EVTables.from_fp32([torch.from_numpy(x) for x in w])
    ev = ev32 if codec == 32 else ev32.encode(codec)
    keys = _distinct_keys(rs, n_rows, 700)
    vals = _values(rs, len(keys), d)
    w2 = [x.copy() for x in w]
    for (k, r), v in zip(keys, vals):
        w2[k][r] = v
    mirror = [orc.encode_table(x, codec) for x in w2]
    ev.update_rows(_dev(keys), _dev(vals))
    for k in range(len(n_rows)):
        assert np.array_equal(ev.raw[k].cpu().numpy(), mirror[k].reshape(n_rows[k], -1)), "table %d" % k
    if codec != 32:
        again = E.EVTables.from_fp32([torch.from_numpy(x) for x in w2]).encode(codec)
        for k in range(len(n_rows)):
            assert torch.equal(again.raw[k], ev.raw[k]), "table %d against evs_encode_table" % k
    if d not in (16, 36, 64):
        return
    B = 300
    idx = np.stack([rs.randint(0, n, B) for n in n_rows]).astype(np.int64)
    for k in range(len(n_rows)):   # (half of the bags ask for updated rows)
        mine = keys[keys[:, 0] == k][:, 1]
        if len(mine):
            idx[k, ::2] = mine[rs.randint(0, len(mine), len(idx[k, ::2]))]
    off = np.tile(np.arange(B, dtype=np.int64), (len(n_rows), 1))
    ly = E.apply_emb(_dev(off), _dev(idx), ev, lazy=False, check_indices=True)
    got = torch.stack(list(ly)).cpu().numpy()
    want = np.stack(orc.apply_emb(list(off), list(idx), w2 if codec == 32 else mirror, None, codec, d))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_table_update_duplicates_unaligned_values_and_host_input(E, orc):
    """through the Python wrapper the LAST of duplicate keys wins; plain Python lists are accepted; values whose rows are not
    16-byte aligned (a column slice) take the scalar loads and give the same bytes"""
    rs = np.random.RandomState(3)
    n_rows, d = [40, 9], 36
    w = [_values(rs, n, d) for n in n_rows]
    for codec in (32, 8, 4):
        ev32 = E.EVTables.from_fp32([torch.from_numpy(x) for x in w])
        ev = ev32 if codec == 32 else ev32.encode(codec)
        keys = np.array([[0, 5], [1, 2], [0, 5], [0, 7], [1, 2], [0, 5]], np.int64)
        vals = _values(rs, len(keys), d, neg_zero=True)
        w2 = [x.copy() for x in w]
        for (k, r), v in zip(keys, vals):
            w2[k][r] = v
        ev.update_rows(keys.tolist(), vals.tolist())
        for k in range(2):
            assert np.array_equal(ev.raw[k].cpu().numpy(), orc.encode_table(w2[k], codec).reshape(n_rows[k], -1))
        # unaligned value rows straight through the C ABI: base + 4 bytes, row stride d + 1
        wide = _dev(np.concatenate([np.zeros((3, 1), np.float32), _values(rs, 3, d)], 1))
        k3 = _dev(np.array([[0, 1], [0, 2], [1, 8]], np.int32))
        E._lib.check(E._lib.lib().evs_table_update_rows(codec, d, 2, ev._tables_c, ev._n_rows_c, 3, k3.data_ptr(),
                                                        wide.data_ptr() + 4, d + 1, _stream()))
        v3 = wide.cpu().numpy()[:, 1:]
        w2[0][1], w2[0][2], w2[1][8] = v3[0], v3[1], v3[2]
        for k in range(2):
            assert np.array_equal(ev.raw[k].cpu().numpy(), orc.encode_table(w2[k], codec).reshape(n_rows[k], -1))


def test_table_update_skips_and_reports_keys_out_of_range(E, orc):
    rs = np.random.RandomState(4)
    n_rows, d = [40, 9], 36
    w = [_values(rs, n, d) for n in n_rows]
    ev = E.EVTables.from_fp32([torch.from_numpy(x) for x in w])
    L = E._lib.lib()
    assert L.evs_check_index_errors(_stream()) == 0
    keys = np.array([[0, 40], [2, 0], [1, -1], [-1, 3], [1, 8], [0, 0]], np.int64)
    vals = _values(rs, len(keys), d)
    ev.update_rows(keys, vals)
    assert L.evs_check_index_errors(_stream()) == E._lib.EVS_EINDEX
    assert L.evs_check_index_errors(_stream()) == 0          # (the flag is cleared by the report)
    w[1][8], w[0][0] = vals[4], vals[5]
    for k in range(2):
        assert np.array_equal(ev.raw[k].cpu().numpy().view(np.float32), w[k])


def test_deferred_apply_emb_result_keeps_the_rows_of_its_call(E, orc):
    """a deferred apply_emb result (the default) taken BEFORE an update and first touched AFTER it holds the pre-update
    rows; the next call sees the new ones"""
    rs = np.random.RandomState(6)
    n_rows = [200] * T
    w = [_values(rs, n, D) for n in n_rows]
    ev = E.EVTables.from_fp32([torch.from_numpy(x) for x in w])
    B = 64
    idx = np.stack([rs.randint(0, n, B) for n in n_rows]).astype(np.int64)
    off = np.tile(np.arange(B, dtype=np.int64), (T, 1))
    offd, idxd = _dev(off), _dev(idx)
    ly = E.apply_emb(offd, idxd, ev)
    st = getattr(ly, "_evs_defer", None)
    from evstore_dlrm_amd import dlrm_ops
    if dlrm_ops.DEFER_POOLING and not dlrm_ops.LAZY_POOLING:
        assert st is not None and not st.done, "the result was expected to be deferred"
    keys = np.array([(k, int(idx[k, b])) for k in range(T) for b in range(0, B, 2)], np.int64)
    keys = np.unique(keys, axis=0)
    vals = _values(rs, len(keys), D)
    ev.update_rows(keys, vals)
    if st is not None:
        assert st.done, "update_rows must compute pending deferred results first"
    got = torch.stack([t.clone() for t in ly]).cpu().numpy()
    want = np.stack([w[k][idx[k]] for k in range(T)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "a pre-update call returned post-update rows"
    for (k, r), v in zip(keys, vals):
        w[k][r] = v
    got2 = torch.stack([t.clone() for t in E.apply_emb(offd, idxd, ev)]).cpu().numpy()
    want2 = np.stack([w[k][idx[k]] for k in range(T)])
    assert np.array_equal(got2.view(np.uint32), want2.view(np.uint32)) and not np.array_equal(got, got2)


def test_update_between_batches_of_a_loop_that_refills_its_index_buffer(E, orc):
    """the serving loop: apply_emb (deferred) -> interact_features (the fused launch consumes the result) -> the NEXT batch's
    indices copied into the same buffer in place -> update_rows.  The consumed result is nobody's to look at any more:
    update_rows neither raises "modified in place" nor launches a gather for it, and the next batch sees the new rows."""
    from evstore_dlrm_amd import dlrm_ops
    rs = np.random.RandomState(16)
    n_rows = [200] * T
    w = [_values(rs, n, D) for n in n_rows]
    ev = E.EVTables.from_fp32([torch.from_numpy(x) for x in w])
    B = 64
    off = _dev(np.tile(np.arange(B, dtype=np.int64), (T, 1)))
    slot = torch.empty((T, B), dtype=torch.int64, device="cuda")      # the loop's one index buffer
    x = _dev(rs.uniform(-1, 1, size=(B, D)).astype(np.float32))
    idx0 = np.stack([rs.randint(0, n, B) for n in n_rows]).astype(np.int64)
    idx1 = np.stack([rs.randint(0, n, B) for n in n_rows]).astype(np.int64)
    slot.copy_(_dev(idx0))
    ly = E.apply_emb(off, slot, ev)
    st = getattr(ly, "_evs_defer", None)
    R0 = E.interact_features(x, ly)
    want0 = orc.interact_features(x.cpu().numpy(), [w[k][idx0[k]] for k in range(T)])
    np.testing.assert_allclose(R0.cpu().numpy(), want0, rtol=1e-5, atol=2e-6)
    deferred = st is not None and not st.done
    if dlrm_ops.DEFER_POOLING and not dlrm_ops.LAZY_POOLING:
        assert deferred and st.consumed, "the fused path was expected to consume the deferred result"
    del ly
    slot.copy_(_dev(idx1))                                            # in place: the old result can no longer be computed
    keys = np.unique(np.array([(k, int(idx1[k, b])) for k in range(T) for b in range(0, B, 2)], np.int64), axis=0)
    vals = _values(rs, len(keys), D)
    ev.update_rows(keys, vals)                                        # (raised RuntimeError before)
    if deferred:
        assert not st.done, "a gather was launched for a result nobody can look at"
    for (k, r), v in zip(keys, vals):
        w[k][r] = v
    R1 = E.interact_features(x, E.apply_emb(off, slot, ev))
    want1 = orc.interact_features(x.cpu().numpy(), [w[k][idx1[k]] for k in range(T)])
    np.testing.assert_allclose(R1.cpu().numpy(), want1, rtol=1e-5, atol=2e-6)
    # the enqueue-only form: device tensors, distinct keys on the caller's word
    vals2 = _values(rs, len(keys), D)
    ev.update_rows(_dev(keys.astype(np.int32)), _dev(vals2), assume_distinct=True)
    for (k, r), v in zip(keys, vals2):
        w[k][r] = v
    for k in range(T):
        assert np.array_equal(ev.raw[k].cpu().numpy().view(np.float32), w[k])


def test_module_cache_update_rows_on_the_gpu_engine(E, orc):
    """cache_algo's module surface with the GPU engine bound (the resident server path of request(use_gpu=True)): a delta
    through _ModuleCache.update_rows, then the rows served"""
    from evstore_dlrm_amd.cache_algo import _common
    m = _common._ModuleCache("evlfu")
    rs = np.random.RandomState(18)
    tabs = [rs.uniform(-1, 1, size=(50, m.dim)).astype(np.float32) for _ in range(m.n_tables)]
    dev = [_dev(t) for t in tabs]
    m.init(100, engine="gpu")
    m._make_gpu(dev)
    m._bound = True
    ids = [k % 50 for k in range(m.n_tables)]
    for use_gpu in (True, False):          # the resident server, then launch + synchronise
        m.request(ids, use_gpu)
        new = rs.uniform(-1, 1, size=(3, m.dim)).astype(np.float32)
        assert m.update_rows([[0, ids[0]], [1, 49], [2, ids[2]]], new) is None    # (0, .) and (2, .) are resident, (1, 49) is not
        tabs[0][ids[0]], tabs[1][49], tabs[2][ids[2]] = new[0], new[1], new[2]
        hit, ly = m.request(ids, use_gpu)
        assert all(hit)
        got = torch.cat([t.detach() for t in ly]).cpu().numpy()
        want = np.stack([tabs[k][ids[k]] for k in range(m.n_tables)])
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(dev[1].cpu().numpy(), tabs[1])
    m.cache.serve_stop()


# ---- exact engines --------------------------------------------------------------------------------------------------------------
def _trace_setup(orc, codec):
    t = load_golden("cache_traces")
    n_rows = [int(n) for n in t["n_rows"]]
    fp32 = orc.kaggle_tables(n_rows, int(t["table_seed"]))
    if codec == 32:
        mirror = [np.array(w, np.float32).view(np.uint8).reshape(len(w), -1) for w in fp32]
    else:
        mirror = [orc.encode_table(np.clip(w * 8, -1, 1), codec) for w in fp32]
    return t, n_rows, mirror, [_dev(m.copy()) for m in mirror]


def _rows_equal(orc, mirror, codec, out, rq):
    """out (n, T, D) fp32 against the CURRENT table contents, bit for bit"""
    for k in range(T):
        want = orc.decode(mirror[k][rq[:, k]], codec, D)
        if not np.array_equal(out[:, k, :].view(np.uint32), want.view(np.uint32)):
            return False
    return True


@pytest.mark.parametrize("codec", [32, 8])
@pytest.mark.parametrize("policy", ["evlfu", "lru", "lfu"])
def test_exact_engines_keep_trace_and_serve_current_rows(E, orc, policy, codec):
    """the golden-trace protocol of tests/test_row_updates_host.py through GpuCache.request / update_rows"""
    cap = 300
    t, n_rows, mirror, dev = _trace_setup(orc, codec)
    reqs = t["requests"]
    half = len(reqs) // 2
    c = E.GpuCache(policy, cap, T, D, codec, "python")
    c.set_backing(dev)
    r = _dev(reqs.astype(np.int32))
    h1, o1 = c.request(r[:half].contiguous())
    assert _rows_equal(orc, mirror, codec, o1.cpu().numpy(), reqs[:half])
    dump0, stats0 = c.dump(), c.stats()
    rs = np.random.RandomState(5)
    keys, n_res, n_non, n_later = ru.make_delta(dump0, reqs[half:], n_rows, rs)
    assert n_res >= 64 and n_non >= 64 and n_later >= 1
    vals = rs.uniform(-1, 1, size=(len(keys), D)).astype(np.float32)
    enc = orc.encode_table(vals, codec)
    for (k, rw), e in zip(keys, enc):
        mirror[k][rw] = e
    assert c.update_rows(keys, vals, count=True) == n_res
    np.testing.assert_array_equal(c.dump(), dump0)
    assert c.stats() == stats0
    for k in range(T):
        assert np.array_equal(dev[k].cpu().numpy(), mirror[k]), "table %d" % k
    h2, o2 = c.request(r[half:].contiguous())
    assert _rows_equal(orc, mirror, codec, o2.cpu().numpy(), reqs[half:])
    hits = np.concatenate([h1.cpu().numpy(), h2.cpu().numpy()]).astype(bool)
    assert np.array_equal(hits, ru.unpack(t["%s_cap%d_hits" % (policy, cap)], len(reqs)))
    ru.golden_final(t, policy, cap, c.dump())


@pytest.mark.parametrize("codec", [32, 8])
@pytest.mark.parametrize("policy", ["evlfu", "lru", "lfu"])
def test_exact_resident_server_is_sent_home_and_serves_the_new_rows(E, orc, policy, codec):
    """the same through serve_start / serve_request: the server is RUNNING when update_rows is called (it answered a request
    a moment ago and its idle window is 20 ms); the next serve_request returns the new rows with the golden hit flags"""
    cap = 300
    t, n_rows, mirror, dev = _trace_setup(orc, codec)
    reqs = t["requests"]
    half = len(reqs) // 2
    want = ru.unpack(t["%s_cap%d_hits" % (policy, cap)], len(reqs))
    c = E.GpuCache(policy, cap, T, D, codec, "python")
    c.set_backing(dev)
    c.serve_start(n_slots=3, idle_us=20000)
    for i in range(half):
        hit, _ = c.serve_request(reqs[i])
        assert np.array_equal(hit.astype(bool), want[i]), i
    dump0 = c.dump()                      # (sends the server home; the next request starts it again)
    rs = np.random.RandomState(7)
    nxt = [(k, int(reqs[half + 1, k])) for k in range(T)]
    keys, n_res, n_non, _ = ru.make_delta(dump0, reqs[half + 1:], n_rows, rs, must=nxt)
    assert n_res >= 64 and n_non >= 64
    vals = rs.uniform(-1, 1, size=(len(keys), D)).astype(np.float32)
    enc = orc.encode_table(vals, codec)
    hit, _ = c.serve_request(reqs[half])
    assert np.array_equal(hit.astype(bool), want[half])
    c.update_rows(keys, vals)             # the server answered microseconds ago: it is resident now
    for (k, rw), e in zip(keys, enc):
        mirror[k][rw] = e
    hit, rows = c.serve_request(reqs[half + 1])
    assert np.array_equal(hit.astype(bool), want[half + 1])
    assert _rows_equal(orc, mirror, codec, rows.cpu().numpy()[None], reqs[half + 1:half + 2]), "the request after the update"
    for i in range(half + 2, len(reqs)):
        hit, rows = c.serve_request(reqs[i])
        assert np.array_equal(hit.astype(bool), want[i]), i
        if i % 41 == 0:
            assert _rows_equal(orc, mirror, codec, rows.cpu().numpy()[None], reqs[i:i + 1]), i
    c.serve_stop()
    ru.golden_final(t, policy, cap, c.dump())
    for k in range(T):
        assert np.array_equal(dev[k].cpu().numpy(), mirror[k])


def test_fresh_cache_only_has_its_table_written(E, orc):
    t, n_rows, mirror, dev = _trace_setup(orc, 32)
    c = E.GpuCache("evlfu", 300, T, D, 32, "python")
    c.set_backing(dev)
    rs = np.random.RandomState(2)
    keys = _distinct_keys(rs, n_rows, 100)
    vals = rs.uniform(-1, 1, size=(100, D)).astype(np.float32)
    assert c.update_rows(keys, vals, count=True) == 0
    for (k, rw), v in zip(keys, vals):
        mirror[k][rw] = v.view(np.uint8)
    for k in range(T):
        assert np.array_equal(dev[k].cpu().numpy(), mirror[k])
    c.set_batch_policy("setassoc")        # still fresh: the batched path (and its policy) can still be chosen
    rq = np.stack([keys[keys[:, 0] == k][:1, 1].repeat(8) if (keys[:, 0] == k).any() else np.zeros(8, np.int64) for k in range(T)], 1)
    hit, out = c.lookup_batch(_dev(rq.astype(np.int32)))
    assert not hit.cpu().numpy().any() and _rows_equal(orc, mirror, 32, out.cpu().numpy(), rq)
    nb = E.GpuCache("evlfu", 300, T, D, 32, "python")   # no backing at all
    with pytest.raises(E.EvsError) as e:
        nb.update_rows(keys, vals)
    assert e.value.code == E._lib.EVS_ESTATE


# ---- batched tiers --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [32, 8])
@pytest.mark.parametrize("policy,inline", [("plan", None), ("sampled", None), ("setassoc", True), ("setassoc", False)])
def test_batched_tier(E, orc, policy, inline, codec):
    ru.batched_case(E, orc, policy, inline, codec)


def test_batched_set_associative_tier_with_16_ways():
    """EVS_SA_WAYS=16 is read once per process: the same case in a child"""
    env = dict(os.environ, EVS_SA_WAYS="16")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_row_updates_child.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


# ---- tier pairs -----------------------------------------------------------------------------------------------------------------
def _pair_tables(orc, rs, n):
    ws = [rs.uniform(-1, 1, size=(n, D)).astype(np.float32) for _ in range(T)]
    m8 = [orc.encode_table(w, 8) for w in ws]
    m4 = [orc.encode_table(w, 4) for w in ws]
    return m8, m4, [_dev(m.copy()) for m in m8], [_dev(m.copy()) for m in m4]


def _pair_delta(res1, res2, n, rs, n_each=128):
    """keys resident in C1, in C2 and in neither"""
    r1, r2 = sorted(res1), sorted(res2)
    k1 = [r1[i] for i in rs.choice(len(r1), min(n_each, len(r1)), replace=False)]
    k2 = [r2[i] for i in rs.choice(len(r2), min(n_each, len(r2)), replace=False)]
    both = set(res1) | set(res2)
    non = []
    while len(non) < n_each:
        kr = (int(rs.randint(0, T)), int(rs.randint(0, n)))
        if kr not in both and kr not in non:
            non.append(kr)
    return k1, k2, non


def _pair_apply(orc, c1, c2, keys, m8, m4, rs):
    vals = rs.uniform(-1, 1, size=(len(keys), D)).astype(np.float32)
    e8, e4 = orc.encode_table(vals, 8), orc.encode_table(vals, 4)
    for (k, rw), a, b in zip(keys, e8, e4):
        m8[k][rw] = a
        m4[k][rw] = b
    kd, vd = _dev(np.array(keys, np.int64)), _dev(vals)
    return c1.update_rows(kd, vd, count=True), c2.update_rows(kd, vd, count=True)


def _pair_rows_ok(orc, tier, out, rq, m8, m4, alt=None):
    """every served row at the precision of the tier that served it, from the CURRENT tables: code 1 -> u8, 2 -> u4, 0 (a
    miss: the routing's choice of destination) -> one of the two, 3 -> the alt key's row in one of the two"""
    u8 = [orc.decode(m, 8, D).view(np.uint32) for m in m8]
    u4 = [orc.decode(m, 4, D).view(np.uint32) for m in m4]
    for b in range(len(rq)):
        for k in range(T):
            kk, rw = k, int(rq[b, k])
            if tier[b, k] == 3:
                a = int(alt[k][rw])
                kk, rw = a % 100 - 1, a // 100
            got = out[b, k].view(np.uint32)
            is8, is4 = np.array_equal(got, u8[kk][rw]), np.array_equal(got, u4[kk][rw])
            if not (is8 if tier[b, k] == 1 else is4 if tier[b, k] == 2 else (is8 or is4)):
                return (b, k, int(tier[b, k]))
    return None


@pytest.mark.parametrize("policy", ["setassoc", "sampled"])
def test_batched_tier_pair_u8_u4(E, orc, policy):
    """a u8 C1 + u4 C2 pair on the batched path (setassoc: the shared-record form), each tier updated from the same fp32
    delta in its own codec on its own backing"""
    from evstore_dlrm_amd import gpu_cache
    rs = np.random.RandomState(31)
    n = 300
    m8, m4, d8, d4 = _pair_tables(orc, rs, n)
    c1 = E.GpuCache("evlfu", 500, T, D, 8, "cpp").set_batch_policy(policy)
    c2 = E.GpuCache("evlfu", 900, T, D, 4, "cpp").set_batch_policy(policy)
    c1.set_backing(d8)
    c2.set_backing(d4)
    reqs = np.minimum(rs.zipf(1.25, size=(3000, T)) - 1, n - 1).astype(np.int32)
    r = _dev(reqs)
    for s in range(0, len(reqs), 250):
        gpu_cache.lookup_batch_c1c2(c1, c2, r[s:s + 250].contiguous())
    res1 = {(int(t) - 1, int(rw)) for _, t, rw in c1.batch_dump()}
    res2 = {(int(t) - 1, int(rw)) for _, t, rw in c2.batch_dump()}
    assert len(res1) >= 128 and len(res2) >= 128 and not (res1 & res2)
    k1, k2, non = _pair_delta(res1, res2, n, rs)
    # a resident-only batch: every position a key of C1 or C2 (delta keys first)
    by_t = [[rw for t, rw in k1 + k2 if t == k] or [rw for t, rw in sorted(res1 | res2) if t == k][:4] for k in range(T)]
    assert all(len(b) for b in by_t)
    rq, _ = ru.batch_of(by_t, by_t, max(64, max(len(b) for b in by_t)), rs)   # (every updated resident key is read back)
    assert {(k, int(v)) for k in range(T) for v in rq[:, k]} >= set(k1 + k2)
    rqd = _dev(rq)
    tier0, _ = gpu_cache.lookup_batch_c1c2(c1, c2, rqd)
    tier0 = tier0.cpu().numpy()
    assert (tier0 > 0).all()
    dumps0 = [c1.batch_dump(), c2.batch_dump()]
    stats0 = [c1.batch_stats(), c2.batch_stats()]
    n1, n2 = _pair_apply(orc, c1, c2, k1 + k2 + non, m8, m4, rs)
    assert (n1, n2) == (len(k1), len(k2))
    for c, d0, s0 in zip((c1, c2), dumps0, stats0):
        assert {tuple(v) for v in c.batch_dump().tolist()} == {tuple(v) for v in d0.tolist()} and c.batch_stats() == s0
    for k in range(T):
        assert np.array_equal(d8[k].cpu().numpy(), m8[k]) and np.array_equal(d4[k].cpu().numpy(), m4[k])
    tier1, out = gpu_cache.lookup_batch_c1c2(c1, c2, rqd)
    tier1, out = tier1.cpu().numpy(), out.cpu().numpy()
    assert np.array_equal(tier1, tier0), "the tier codes of a resident-only batch moved"
    assert _pair_rows_ok(orc, tier1, out, rq, m8, m4) is None
    # the delta keys neither tier holds: from the destination tier's table, new bytes
    by_n = [[rw for t, rw in non if t == k] for k in range(T)]
    rq2, mask = ru.batch_of(by_n, by_t, max(32, max(len(b) for b in by_n)), rs)
    tier2, out2 = gpu_cache.lookup_batch_c1c2(c1, c2, _dev(rq2))
    tier2, out2 = tier2.cpu().numpy(), out2.cpu().numpy()
    assert mask.any() and (tier2[mask] == 0).all()
    assert _pair_rows_ok(orc, tier2, out2, rq2, m8, m4) is None


@pytest.mark.parametrize("with_c3", [False, True])
def test_exact_tier_pair_and_triple(E, orc, with_c3):
    """request_c1c2 / request_c1c2c3 (exact): the tier codes of the whole stream stay the oracle's, rows come from the
    current tables at the serving tier's precision; the alt-key tier stores no rows and needs nothing"""
    from evstore_dlrm_amd import gpu_cache
    rs = np.random.RandomState(8)
    n = 300
    m8, m4, d8, d4 = _pair_tables(orc, rs, n)
    alt = [(rs.randint(0, n, size=n) * 100 + (k + 1)).astype(np.uint32) for k in range(T)]
    cap1, cap2, cap3 = 400, 800, 200
    reqs = np.minimum(rs.zipf(1.3, size=(1600, T)) - 1, n - 1).astype(np.int32)
    dec8, dec4 = [orc.decode(m, 8, D) for m in m8], [orc.decode(m, 4, D) for m in m4]
    o = orc.C1C2C3(cap1, cap2, cap3, dec8, dec4, alt) if with_c3 else orc.C1C2(cap1, cap2, dec8, dec4)
    want_tier = np.stack([o.request(rq)[0].copy() for rq in reqs])
    c1 = E.GpuCache("evlfu", cap1, T, D, 8, "cpp")
    c2 = E.GpuCache("evlfu", cap2, T, D, 4, "cpp")
    c1.set_backing(d8)
    c2.set_backing(d4)
    c3 = gpu_cache.GpuAltKeyTier(cap3, [_dev(a.view(np.int32)) for a in alt]) if with_c3 else None
    r = _dev(reqs)
    half = len(reqs) // 2

    def run(lo, hi):
        tiers, outs = [], []
        for s in range(lo, hi, 173):
            e = min(s + 173, hi)
            tr, out = gpu_cache.request_c1c2c3(c1, c2, c3, r[s:e].contiguous())
            tiers.append(tr.cpu().numpy()); outs.append(out.cpu().numpy())
        return np.concatenate(tiers), np.concatenate(outs)

    t1, o1 = run(0, half)
    assert np.array_equal(t1, want_tier[:half]) and _pair_rows_ok(orc, t1, o1, reqs[:half], m8, m4, alt) is None
    dumps0, stats0 = [c1.dump(), c2.dump()], [c1.stats(), c2.stats()]
    c3s0 = c3.stats() if with_c3 else None
    res1 = {(int(t) - 1, int(rw)) for _, t, rw in dumps0[0]}
    res2 = {(int(t) - 1, int(rw)) for _, t, rw in dumps0[1]}
    k1, k2, non = _pair_delta(res1, res2, n, rs)
    assert len(k1) >= 64 and len(k2) >= 64
    n1, n2 = _pair_apply(orc, c1, c2, k1 + k2 + non, m8, m4, rs)
    assert (n1, n2) == (len(k1), len(k2))
    for c, d0, s0 in zip((c1, c2), dumps0, stats0):
        np.testing.assert_array_equal(c.dump(), d0)
        assert c.stats() == s0
    if with_c3:
        assert c3.stats() == c3s0
    t2, o2 = run(half, len(reqs))
    assert np.array_equal(t2, want_tier[half:])
    assert _pair_rows_ok(orc, t2, o2, reqs[half:], m8, m4, alt) is None
    assert (t2 == 1).sum() > 50 and (t2 == 2).sum() > 50 and (not with_c3 or (np.concatenate([t1, t2]) == 3).sum() > 0)


def test_tier_server_is_sent_home_and_serves_the_new_rows(E, orc):
    from evstore_dlrm_amd import gpu_cache
    rs = np.random.RandomState(12)
    n = 300
    m8, m4, d8, d4 = _pair_tables(orc, rs, n)
    cap1, cap2 = 400, 800
    reqs = np.minimum(rs.zipf(1.3, size=(600, T)) - 1, n - 1).astype(np.int32)
    o = orc.C1C2(cap1, cap2, [orc.decode(m, 8, D) for m in m8], [orc.decode(m, 4, D) for m in m4])
    want_tier = np.stack([o.request(rq)[0].copy() for rq in reqs])
    c1 = E.GpuCache("evlfu", cap1, T, D, 8, "cpp")
    c2 = E.GpuCache("evlfu", cap2, T, D, 4, "cpp")
    c1.set_backing(d8)
    c2.set_backing(d4)
    ts = gpu_cache.TierServer(c1, c2, None, n_slots=3, idle_us=20000)
    half = len(reqs) // 2
    for i in range(half):
        tier, _ = ts.request(reqs[i])
        assert np.array_equal(tier, want_tier[i]), i
    res1 = {(int(t) - 1, int(rw)) for _, t, rw in c1.dump()}     # (sends the server home)
    res2 = {(int(t) - 1, int(rw)) for _, t, rw in c2.dump()}
    k1, k2, non = _pair_delta(res1, res2, n, rs)
    keys = list(dict.fromkeys([(k, int(reqs[half + 1, k])) for k in range(T)] + k1 + k2 + non))
    tier, _ = ts.request(reqs[half])                              # the server is resident again ...
    assert np.array_equal(tier, want_tier[half])
    _pair_apply(orc, c1, c2, keys, m8, m4, rs)                    # ... when the update arrives
    tier, rows = ts.request(reqs[half + 1])
    assert np.array_equal(tier, want_tier[half + 1])
    assert _pair_rows_ok(orc, tier[None], rows.cpu().numpy()[None], reqs[half + 1:half + 2], m8, m4) is None
    for i in range(half + 2, len(reqs)):
        tier, rows = ts.request(reqs[i])
        assert np.array_equal(tier, want_tier[i]), i
        if i % 29 == 0:
            assert _pair_rows_ok(orc, tier[None], rows.cpu().numpy()[None], reqs[i:i + 1], m8, m4) is None, i
    ts.stop()
    ts.close()


# ---- refusals, and tables the kernels must not write ------------------------------------------------------------------------------
def test_update_rows_refuses_a_file_backed_cache(E, orc, tmp_path):
    rs = np.random.RandomState(9)
    n_rows = [50] * T
    paths = []
    for k, nr in enumerate(n_rows):
        p = tmp_path / ("ev-table-%d.bin" % (k + 1))
        rs.uniform(-1, 1, size=(nr, D)).astype(np.float32).tofile(p)
        paths.append(str(p))
    ft = E.FileTier(paths, 4 * D, 10 ** 9)
    c = E.GpuCache("evlfu", 200, T, D, 32)
    c.set_file_backing(ft)
    with pytest.raises(E.EvsError) as e:
        c.update_rows([[0, 1]], [[0.5] * D])
    assert e.value.code == E._lib.EVS_ESTATE and "read-only" in str(e.value)
    del c
    ft.close()


def test_refresh_rows_over_pinned_host_tables(E, orc):
    """tables in pinned host memory written by the HOST, then refresh_rows: the cache serves the new rows"""
    rs = np.random.RandomState(10)
    n_rows = [400] * T
    tabs = [torch.from_numpy(rs.uniform(-1, 1, size=(nr, D)).astype(np.float32)).pin_memory() for nr in n_rows]
    c = E.GpuCache("evlfu", 2000, T, D, 32).set_batch_policy("sampled")
    c.set_backing(tabs)
    reqs = np.minimum(rs.zipf(1.2, size=(1024, T)) - 1, 399).astype(np.int32)
    for s in range(0, 1024, 256):
        c.lookup_batch(_dev(reqs[s:s + 256]))
    dump0, stats0 = c.batch_dump(), c.batch_stats()
    resident = sorted({(int(t) - 1, int(rw)) for _, t, rw in dump0})
    res = [resident[i] for i in rs.choice(len(resident), 300, replace=False)]
    for k in range(T):
        if not any(t == k for t, _ in res):
            res.append(next(kr for kr in resident if kr[0] == k))
    non = [(k, 399 - j) for k in range(T) for j in range(3) if (k, 399 - j) not in set(resident)]
    keys = np.array(res + non, np.int64)
    vals = rs.uniform(-1, 1, size=(len(keys), D)).astype(np.float32)
    torch.cuda.synchronize()
    for (k, rw), v in zip(keys, vals):
        tabs[k][rw] = torch.from_numpy(v)
    assert c.refresh_rows(keys, count=True) == len(res)
    assert {tuple(v) for v in c.batch_dump().tolist()} == {tuple(v) for v in dump0.tolist()} and c.batch_stats() == stats0
    res_by_t = [[rw for t, rw in res if t == k] for k in range(T)]
    rq, _ = ru.batch_of(res_by_t, [[0]] * T, max(64, max(len(v) for v in res_by_t)), rs)   # (every refreshed key is read back)
    assert {(k, int(v)) for k in range(T) for v in rq[:, k]} == set(res)
    hit, out = c.lookup_batch(_dev(rq))
    assert bool(hit.cpu().numpy().all())
    out = out.cpu().numpy()
    for k in range(T):
        assert np.array_equal(out[:, k, :].view(np.uint32), tabs[k].numpy()[rq[:, k]].view(np.uint32))
