"""GPU: the tier pair / triple as a resident server (evs_tiers_serve_*, gpu_cache.TierServer) and ev_lookup through the
servers (EVS_MANAGER_SERVE=1) -- every request's tier codes and rows bit-exact against the oracle, the tiers' final state
equal to the oracle's whatever interrupts the server on the way."""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


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


def _tiers(E, cap1, cap2, raw8, raw4, alt=None, cap3=0):
    from evstore_dlrm_amd import gpu_cache
    c1 = E.GpuCache("evlfu", cap1, 26, 36, 8, "cpp")
    c2 = E.GpuCache("evlfu", cap2, 26, 36, 4, "cpp")
    c1.set_backing([torch.from_numpy(r).cuda() for r in raw8])
    c2.set_backing([torch.from_numpy(r).cuda() for r in raw4])
    c3 = gpu_cache.GpuAltKeyTier(cap3, [torch.from_numpy(a.view(np.int32)).cuda() for a in alt]) if alt is not None else None
    return c1, c2, c3


def _drive(E, c1, c2, c3, reqs, want_tier, want_out, c3_stats_at=None):
    """every request through a TierServer, alternating the three ways a request can be posted, with the interruptions of
    (c); -> the tier codes served, one row per request"""
    from evstore_dlrm_amd import gpu_cache
    srv = E.TierServer(c1, c2, c3, n_slots=3, idle_us=300)
    tiers = np.zeros((len(reqs), 26), np.uint8)
    held = None   # (request index, ring view) of the last ring request
    try:
        i = 0
        while i < len(reqs):
            if i == 300:      # the server goes home for these and is started again by the next request
                assert c1.stats()["n_requests"] == 300
                assert len(c2.dump()) == c2.stats()["size"]
            if i == 500:      # past the idle time-out: the server has left by itself
                time.sleep(0.01)
            if c3_stats_at is not None and i == c3_stats_at:
                assert c3.stats()["error"] == 0
            if i == 600:      # one chunk launched the old way in between
                r = torch.from_numpy(np.ascontiguousarray(reqs[600:711])).cuda()
                t, out = gpu_cache.request_c1c2c3(c1, c2, c3, r) if c3 is not None else gpu_cache.request_c1c2(c1, c2, r)
                tiers[600:711] = t.cpu().numpy()
                assert np.array_equal(tiers[600:711], want_tier[600:711])
                assert np.array_equal(out.cpu().numpy().view(np.uint32), want_out[600:711].view(np.uint32))
                i = 711
                held = None
                continue
            rq, way = reqs[i], i % 3
            if way == 0:
                t, rows = srv.request(rq)
            elif way == 1:
                rows = torch.full((26, 36), -7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                t = srv.request_to(rq, rows)
            else:
                ids = torch.from_numpy(np.stack([rq.astype(np.int64), np.full(26, -1, np.int64)], 1)).cuda()   # (T, 2)
                rows = torch.full((26, 1, 36), -7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                t = srv.request_to(ids, rows)
            tiers[i] = t
            assert np.array_equal(tiers[i], want_tier[i]), (i, way)
            got = rows.reshape(26, 36).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want_out[i].view(np.uint32)), (i, way)
            if held is not None and held[0] == i - 1:   # a held ring slot is intact one request later (n_slots = 3)
                assert np.array_equal(held[1].cpu().numpy().view(np.uint32), want_out[held[0]].view(np.uint32)), i
            held = (i, rows) if way == 0 else None
            i += 1
        srv.stop()
        with pytest.raises(E.EvsError):
            srv.request(reqs[0])
    finally:
        srv.close()
    return tiers


def test_pair_vs_oracle_with_interruptions(E, orc):
    """(a) + (c): the construction of test_two_tier_c1c2_vs_oracle, every request through the server."""
    rs = np.random.RandomState(3)
    ws = [rs.uniform(-1, 1, size=(400, 36)).astype(np.float32) for _ in range(26)]
    raw8 = [orc.encode_table(w, 8) for w in ws]
    raw4 = [orc.encode_table(w, 4) for w in ws]
    dec8 = [orc.decode(r, 8, 36) for r in raw8]
    dec4 = [orc.decode(r, 4, 36) for r in raw4]
    cap1, cap2 = 600, 1200
    reqs = np.zeros((900, 26), np.int32)
    for i in range(len(reqs)):
        reqs[i] = rs.randint(0, 400, 26)
        if i > 20 and rs.rand() < 0.4:
            reqs[i] = reqs[i - 1 - rs.randint(15)]
            reqs[i] = np.where(rs.rand(26) < 0.07, rs.randint(0, 400, 26), reqs[i])
    o = orc.C1C2(cap1, cap2, dec8, dec4)
    want_tier, want_out, perfect = [], [], 0
    for rq in reqs:
        t, out, p = o.request(rq)
        want_tier.append(t.copy()); want_out.append(out.copy()); perfect += p
    want_tier, want_out = np.stack(want_tier), np.stack(want_out)
    c1, c2, _ = _tiers(E, cap1, cap2, raw8, raw4)
    tiers = _drive(E, c1, c2, None, reqs, want_tier, want_out)
    assert np.array_equal(tiers, want_tier)
    np.testing.assert_array_equal(c1.dump(), o.c1.dump())
    np.testing.assert_array_equal(c2.dump(), o.c2.dump())
    st = c1.stats()
    assert st["n_perfect_hits"] == perfect and st["n_requests"] == len(reqs)
    assert (tiers == 2).sum() > 100 and (tiers == 1).sum() > 100  # both tiers actually serve


def test_triple_vs_oracle_with_interruptions(E, orc):
    """(b) + (c): the construction of test_three_tier_c1c2c3_vs_oracle, every request through the server."""
    rs = np.random.RandomState(8)
    n = 300
    ws = [rs.uniform(-1, 1, size=(n, 36)).astype(np.float32) for _ in range(26)]
    raw8 = [orc.encode_table(w, 8) for w in ws]
    raw4 = [orc.encode_table(w, 4) for w in ws]
    dec8 = [orc.decode(r, 8, 36) for r in raw8]
    dec4 = [orc.decode(r, 4, 36) for r in raw4]
    alt = [(rs.randint(0, n, size=n) * 100 + (k + 1)).astype(np.uint32) for k in range(26)]
    cap1, cap2, cap3 = 400, 800, 200
    reqs = np.minimum(rs.zipf(1.3, size=(2500, 26)) - 1, n - 1).astype(np.int32)
    o = orc.C1C2C3(cap1, cap2, cap3, dec8, dec4, alt)
    want_tier, want_out = [], []
    for rq in reqs:
        t, out, _ = o.request(rq)
        want_tier.append(t.copy()); want_out.append(out.copy())
    want_tier, want_out = np.stack(want_tier), np.stack(want_out)
    c1, c2, c3 = _tiers(E, cap1, cap2, raw8, raw4, alt, cap3)
    tiers = _drive(E, c1, c2, c3, reqs, want_tier, want_out, c3_stats_at=1500)
    assert np.array_equal(tiers, want_tier)
    np.testing.assert_array_equal(c1.dump(), o.c1.dump())
    np.testing.assert_array_equal(c2.dump(), o.c2.dump())
    st, so = c3.stats(), o.c3_state()
    assert st == so and st["n_hit"] > 50 and st["error"] == 0
    assert (tiers == 3).sum() == st["n_hit"]


def test_reference_traffic_through_the_server(E, orc):
    """(d): the compiled reference's 11 000-request stream (tests/golden/c1c2_ref.npz): codes and rows of every request equal
    the oracle's, nothing served at the secondary precision before the reference's first such request.  Driven through
    ctypes with the pointers built once (the Python wrapper's per-request cost is not what is tested here)."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden as G
    g = load_golden("c1c2_ref")
    _, tabs = G.c1c2_tables(orc)
    raw8, raw4 = [t[0] for t in tabs], [t[1] for t in tabs]
    dec8, dec4 = [orc.decode(r, 8, 36) for r in raw8], [orc.decode(r, 4, 36) for r in raw4]
    reqs = np.ascontiguousarray(g["requests"], dtype=np.int32)
    cap1, cap2 = int(g["cap_c1"]), int(g["cap_c2"])
    o = orc.C1C2(cap1, cap2, dec8, dec4)
    c1, c2, _ = _tiers(E, cap1, cap2, raw8, raw4)
    n_slots = 8
    srv = E.TierServer(c1, c2, None, n_slots=n_slots, idle_us=300)
    tier = np.zeros((len(reqs), 26), np.uint8)
    try:
        fn = E._lib.lib().evs_tiers_serve_request
        slot = C.c_int(0)
        sp = C.byref(slot)
        block = n_slots - 1      # a slot stays valid until n_slots - 1 more requests are posted: copy the ring out in time
        got = np.zeros((block, 26, 36), np.float32)
        for a in range(0, len(reqs), block):
            b = min(a + block, len(reqs))
            slots = []
            for i in range(a, b):
                rc = fn(srv._h, reqs[i].ctypes.data, tier[i].ctypes.data, sp)
                assert rc == 0, (i, E._lib.lib().evs_last_error())
                slots.append(slot.value)
            got[:b - a] = srv.ring[slots].cpu().numpy()
            for i in range(a, b):
                t_o, v_o, _ = o.request(reqs[i])
                assert np.array_equal(tier[i], t_o), i
                assert np.array_equal(got[i - a].view(np.uint32), v_o.view(np.uint32)), i
        srv.stop()
    finally:
        srv.close()
    np.testing.assert_array_equal(c1.dump(), o.c1.dump())
    np.testing.assert_array_equal(c2.dump(), o.c2.dump())
    ref = g["served_bits"]
    first_ref = int(np.argmax((ref == 4).any(1)))
    assert (tier[:first_ref] != 2).all() and first_ref > 9000


def _serve_env():
    env = dict(os.environ)
    env["EVS_MANAGER_SERVE"] = "1"
    return env


def _result(out):
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, out.stdout[-2000:] + out.stderr[-2000:]
    return json.loads(line[0][7:])


@pytest.mark.parametrize("var", ["2-32-4-4000", "2-8-4-4000", "1-32-4-3000"])
def test_ev_lookup_precision_builds_through_the_servers(E, orc, tmp_path, var):
    """(e): test_cabi_precision_builds_vs_compiled_reference's child, unchanged, with EVS_MANAGER_SERVE=1: every row of every
    request is compared on the host, bit for bit, right behind the sequence number."""
    child = os.path.join(HERE, "_ev_lookup_variant_child.py")
    out = subprocess.run([sys.executable, child, str(tmp_path), var], capture_output=True, text=True, timeout=600, env=_serve_env())
    r = _result(out)
    assert r["exact_vs_oracle"] and r["no_garbage"], r
    assert r["caps"][:2] == r["caps_ref"], r
    assert r["perfect_prefix_equal"] and r["nb"] >= 1, r
    if var.startswith("2-"):
        assert r["first_mine"] == r["first_ref"] and r["prefill_equal"] and r["min_block_agreement"] >= 0.99, r
    else:
        assert abs(r["perfect"][0] - r["perfect"][1]) <= max(8, 0.4 * r["perfect"][1]), r


@pytest.mark.parametrize("prec,layers", [(8, 2), (8, 3)])
def test_ev_lookup_reference_cabi_through_the_servers(E, orc, tmp_path, prec, layers):
    """(e): test_reference_cabi_ev_lookup's child, unchanged (its default backing: pinned host tables), with the switch."""
    t = load_golden("cache_traces")
    tabs = orc.kaggle_tables([int(n) for n in t["n_rows"]], int(t["table_seed"]))
    sub = {32: "ev-table", 16: "ev-table-16", 8: "ev-table-8", 4: "ev-table-4"}[prec]
    (tmp_path / sub / "binary").mkdir(parents=True)
    for k, w in enumerate(tabs):
        orc.encode_table(np.clip(w * 8, -1, 1), prec).tofile(tmp_path / sub / "binary" / ("ev-table-%d.bin" % (k + 1)))
    if layers == 3:
        (tmp_path / "altkeys").mkdir()
        rs = np.random.RandomState(4)
        for k, w in enumerate(tabs):
            ((rs.randint(0, len(w), size=len(w)) * 100 + (k + 1)).astype(">u4")).tofile(tmp_path / "altkeys" / ("ev-table-%d.bin" % (k + 1)))
    (tmp_path / "ev-table-4" / "binary").mkdir(parents=True)
    for k, w in enumerate(tabs):
        orc.encode_table(np.clip(w * 8, -1, 1), 4).tofile(tmp_path / "ev-table-4" / "binary" / ("ev-table-%d.bin" % (k + 1)))
    np.save(tmp_path / "reqs.npy", t["requests"][:1200] if layers == 3 else t["requests"][:250])
    child = os.path.join(HERE, "_ev_lookup_child.py")
    out = subprocess.run([sys.executable, child, str(tmp_path), str(prec), "40" if layers == 3 else "100", str(layers)],
                         capture_output=True, text=True, timeout=300, env=_serve_env())
    r = _result(out)
    assert r["ok"] and r["same_buf"] and r["rc_dead"] == -1
    assert r["perfect_oracle"] <= r["counter"] <= r["perfect_oracle"] + 1 and r["after_print"] == 0
    assert "Perfect hit" in out.stdout
    if layers == 3:
        assert r["aprx"][1] <= r["aprx"][0] <= r["aprx"][1] + 26 and "C3 Indiv-Hit" in out.stdout


@pytest.mark.parametrize("switch,engine", [("1", 3), (None, 2)])
def test_manager_engine_says_which_path_served(E, tmp_path, switch, engine):
    """(e): the switch is honoured -- evs_manager_engine() is 3 with EVS_MANAGER_SERVE=1 and 2 without, same rows either way."""
    env = {k: v for k, v in os.environ.items() if k != "EVS_MANAGER_SERVE"}
    if switch is not None:
        env["EVS_MANAGER_SERVE"] = switch
    out = subprocess.run([sys.executable, os.path.join(HERE, "_tier_serve_child.py"), str(tmp_path)], capture_output=True,
                         text=True, timeout=300, env=env)
    r = _result(out)
    assert r["before"] == 0 and r["engine"] == engine and r["ok"], r
    assert r["counter"] == r["perfect_oracle"], r


def test_refusals(E, orc):
    """(f): what the server does not do is an EvsError, never undefined behaviour."""
    rs = np.random.RandomState(5)
    ws = [rs.uniform(-1, 1, size=(64, 36)).astype(np.float32) for _ in range(27)]
    raw8 = [orc.encode_table(w, 8) for w in ws]
    raw4 = [orc.encode_table(w, 4) for w in ws]
    c1, c2, _ = _tiers(E, 100, 200, raw8[:26], raw4[:26])
    srv = E.TierServer(c1, c2, idle_us=100)
    try:
        srv.request(np.zeros(26, np.int32))
        with pytest.raises(E.EvsError):          # a member cannot run a single-tier server of its own
            c1.serve_start()
        with pytest.raises(E.EvsError):          # two servers over one cache
            E.TierServer(c1, c2)
        c4, c5, _ = _tiers(E, 100, 200, raw8[:26], raw4[:26])
        with pytest.raises(E.EvsError):
            E.TierServer(c4, c2)
        with pytest.raises(E.EvsError):          # C1 == C2
            E.TierServer(c4, c4)
        r = torch.zeros((4, 26), dtype=torch.int32, device="cuda")
        c5.lookup_batch(r)                       # a cache on the batched path
        with pytest.raises(E.EvsError):
            E.TierServer(c4, c5)
        # a member destroyed under the server: the server is dead, the handle still answers
        srv.request(np.ones(26, np.int32))
        E._lib.check(E._lib.lib().evs_cache_destroy(c2._h))
        c2._h = None
        with pytest.raises(E.EvsError):
            srv.request(np.zeros(26, np.int32))
    finally:
        srv.close()
    # 27 tables: the destination address rides in the id words of tables 26 and 27
    a = E.GpuCache("evlfu", 100, 27, 36, 8, "cpp")
    b = E.GpuCache("evlfu", 200, 27, 36, 4, "cpp")
    a.set_backing([torch.from_numpy(r).cuda() for r in raw8])
    b.set_backing([torch.from_numpy(r).cuda() for r in raw4])
    s27 = E.TierServer(a, b, n_slots=2, idle_us=100)
    try:
        t, rows = s27.request(np.zeros(27, np.int32))
        assert rows.shape == (27, 36) and (t == 0).all()   # an empty pair: 27 misses
        with pytest.raises(E.EvsError):
            s27.request_to(np.zeros(27, np.int32), torch.zeros((27, 36), dtype=torch.float32, device="cuda"))
    finally:
        s27.stop()
        s27.close()
