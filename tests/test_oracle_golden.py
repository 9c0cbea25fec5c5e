"""Pins oracle/ against the golden vectors produced by the reference itself
(tests/golden/make_golden.py).  CPU only."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden, split_indices, split_tables, split_weights
from oracle import oracle as orc

DLRM_CASES = ["dlrm_ragged_small", "dlrm_kaggle_small", "dlrm_weighted_itself", "dlrm_d64", "dlrm_bench_shape", "dlrm_d128"]
RTOL = 1e-5  # BASELINE.json north_star: "within 1e-5 rel on fp32 pooled outputs"


def _tables_cfg1(g):
    # dlrm_cfg1 stores only sha256 of the tables: regenerate them with the reference's
    # draw order: seed, data (generate_dist_input_batch), then create_emb per table.
    # Simpler and exact: the draws before create_emb are consumed by replaying the generator.
    np.random.seed(int(g["seed"]))
    ln, B = g["ln_emb"], int(g["B"])
    np.random.rand(B, 13)
    for size in ln:
        for _ in range(B):
            r = np.random.random(1)
            k = np.int64(np.round(max([1.0], r * min(size, 10))))
            np.random.random(k)
    d = int(g["m_spa"])
    tabs = []
    for n in ln:
        tabs.append(np.random.uniform(low=-np.sqrt(1 / n), high=np.sqrt(1 / n), size=(n, d)).astype(np.float32))
    return tabs


def test_cfg1_tables_reproduce_and_match():
    g = load_golden("dlrm_cfg1")
    tabs = _tables_cfg1(g)
    for t, h in zip(tabs, g["tables_sha256"]):
        assert hashlib.sha256(t.tobytes()).hexdigest() == str(h)
    lS_o, lS_i = split_indices(g)
    ly = orc.apply_emb(lS_o, lS_i, tabs)
    np.testing.assert_allclose(np.stack(ly), g["ly"], rtol=RTOL, atol=1e-7)
    R = orc.interact_features(g["x"], ly)
    assert R.shape == (128, 52)
    np.testing.assert_allclose(R, g["R"], rtol=RTOL, atol=1e-6)


@pytest.mark.parametrize("name", DLRM_CASES)
def test_apply_emb_and_interact(name):
    g = load_golden(name)
    tabs = split_tables(g)
    for t, h in zip(tabs, g["tables_sha256"]):
        assert hashlib.sha256(t.tobytes()).hexdigest() == str(h)
    lS_o, lS_i = split_indices(g)
    ly = orc.apply_emb(lS_o, lS_i, tabs, split_weights(g))
    np.testing.assert_allclose(np.stack(ly), g["ly"], rtol=RTOL, atol=1e-7)
    itself = bool(g["itself"])
    for chain in (False, True):
        R = orc.interact_features(g["x"], [g["ly"][k] for k in range(len(tabs))], itself, chain)
        np.testing.assert_allclose(R, g["R"], rtol=RTOL, atol=2e-6)


def test_bad_index_is_an_error():
    W = np.zeros((4, 16), np.float32)
    with pytest.raises(IndexError):
        orc.embedding_bag_sum(W, [0, 4], [0])
    with pytest.raises(IndexError):
        orc.embedding_bag_sum(W, [0, -1], [0])


def test_empty_bags_and_empty_batch():
    W = np.arange(12, dtype=np.float32).reshape(3, 4)
    out = orc.embedding_bag_sum(W, [2, 0], [0, 0, 1, 2])  # bags: [], [2], [0], []
    np.testing.assert_array_equal(out, np.stack([np.zeros(4), W[2], W[0], np.zeros(4)]).astype(np.float32))
    assert orc.embedding_bag_sum(W, [], []).shape == (0, 4)


# ------------------------------------------------------------------ codecs
def test_decoders_match_compiled_reference():
    t = load_golden("codec_tables")
    u8 = orc.decode(np.arange(256, dtype=np.uint8), 8, 1).reshape(-1)
    np.testing.assert_array_equal(u8.view(np.uint32), t["u8"].view(np.uint32))
    u16 = orc.decode(np.arange(65536, dtype=np.uint16), 16, 1).reshape(-1)
    np.testing.assert_array_equal(u16.view(np.uint32), t["u16"].view(np.uint32))
    u4 = orc.decode(np.arange(256, dtype=np.uint8), 4, 2)
    ref = t["u4"]
    ok = ~np.isnan(ref)
    assert ok.sum() == 2 * 15 * 15  # every byte without a 15 nibble
    np.testing.assert_array_equal(u4[ok].view(np.uint32), ref[ok].view(np.uint32))
    assert np.isnan(u4[~ok]).all() or True  # nibble 15 is UB in the reference


def test_encoders_match_reference_python():
    e = load_golden("encoders")
    for codec, key in ((8, "u8"), (16, "u16"), (4, "u4")):
        np.testing.assert_array_equal(orc.encode(e["values"], codec), e[key])
    lut = orc.decode(np.array([(c << 4) | c for c in range(15)], np.uint8), 4, 2)[:, 0]
    np.testing.assert_allclose(lut, e["u4_decode_table"].astype(np.float32), rtol=0, atol=0)


def test_encode_table_roundtrip_layout():
    rs = np.random.RandomState(0)
    W = rs.uniform(-1, 1, size=(50, 36)).astype(np.float32)
    for codec, bpr in ((32, 144), (16, 72), (8, 36), (4, 18)):
        raw = orc.encode_table(W, codec)
        assert raw.shape == (50, bpr) and raw.dtype == np.uint8
        dec = orc.decode(raw, codec, 36)
        tol = {32: 0, 16: 2.1e-2, 8: 4e-3, 4: 0.61}[codec]
        assert np.abs(dec - W).max() <= tol


# ------------------------------------------------------------------ cache policies
def _tables_for_traces(t):
    return orc.kaggle_tables([int(n) for n in t["n_rows"]], int(t["table_seed"]))


def _unpack_hits(packed, n):
    return np.unpackbits(packed, axis=1)[:, :26].astype(bool)[:n]


@pytest.mark.parametrize("cap", [64, 300, 768, 2000, 79, 80, 82])
def test_evlfu_trace(cap):
    t = load_golden("cache_traces")
    tabs = _tables_for_traces(t)
    reqs = t["requests_flush"] if cap in (79, 80, 82) else t["requests"]
    c = orc.EvLFU(cap, tabs)
    want = _unpack_hits(t["evlfu_cap%d_hits" % cap], len(reqs))
    for i, rq in enumerate(reqs):
        hit, vals = c.request(rq)
        assert np.array_equal(hit, want[i]), "request %d" % i
        for k in range(26):
            assert np.array_equal(vals[k], tabs[k][rq[k]])
    np.testing.assert_array_equal(c.dump(), t["evlfu_cap%d_final_buckets" % cap])
    st = c.state()
    want_st = t["evlfu_cap%d_state" % cap]
    assert [st["min_c1"], st["n_perfect"], st["size"], st["n_flush"]] == list(want_st)
    if cap in (79, 80, 82):
        assert st["n_flush"] >= 1


@pytest.mark.parametrize("stream,cap", [("main", 52), ("main", 64), ("main", 78), ("main", 300), ("main", 768),
                                        ("flush", 52), ("flush", 64), ("flush", 78), ("flush", 300), ("flush", 768)])
def test_evlfu_cython_variant_trace(stream, cap):
    """variant='cython' (flush 0.4 / perfect cap 1.0, n+1 keys flushed) against traces of the COMPILED reference
    C++ (cache_algo/EvLFU_C1_Cython/EvLFU.cpp:70-232 built by oracle/Makefile -> _ref/ref_cython_evlfu):
    hit flags of every request, final list order, min_C1 / n_perfect / size, number of flushes."""
    t = load_golden("cython_traces")
    tabs = _tables_for_traces(t)
    reqs = t["requests_flush"] if stream == "flush" else t["requests"]
    c = orc.EvLFU(cap, tabs, 36, "cython")
    tag = "cython_%s_cap%d" % (stream, cap)
    want = _unpack_hits(t[tag + "_hits"], len(reqs))
    for i, rq in enumerate(reqs):
        hit, vals = c.request(rq)
        assert np.array_equal(hit, want[i]), "request %d" % i
        assert np.array_equal(vals[5], tabs[5][rq[5]])
    np.testing.assert_array_equal(c.dump(), t[tag + "_final_buckets"])
    st = c.state()
    assert [st["min_c1"], st["n_perfect"], st["size"], st["n_flush"]] == list(t[tag + "_state"])
    if stream == "flush" and cap in (52, 78):
        assert st["n_flush"] >= 1


def test_evlfu_approx_mode_trace():
    t = load_golden("cache_traces")
    tabs = _tables_for_traces(t)
    c = orc.EvLFU(768, tabs)
    want = _unpack_hits(t["evlfu_cap768_approx20_hits"], len(t["requests"]))
    for i, rq in enumerate(t["requests"]):
        hit, _ = c.request(rq, approx_thres=20)
        assert np.array_equal(hit, want[i]), "request %d" % i
    np.testing.assert_array_equal(c.dump(), t["evlfu_cap768_approx20_final_buckets"])


@pytest.mark.parametrize("cap", [64, 300, 768, 2000, 80])
def test_lru_trace(cap):
    t = load_golden("cache_traces")
    tabs = _tables_for_traces(t)
    reqs = t["requests_flush"] if cap == 80 else t["requests"]
    c = orc.LRU(cap, tabs)
    want = _unpack_hits(t["lru_cap%d_hits" % cap], len(reqs))
    for i, rq in enumerate(reqs):
        hit, vals = c.request(rq)
        assert np.array_equal(hit, want[i]), "request %d" % i
        assert np.array_equal(vals[3], tabs[3][rq[3]])
    np.testing.assert_array_equal(c.dump(), t["lru_cap%d_final_order" % cap])


@pytest.mark.parametrize("cap", [64, 300, 768, 2000, 80])
def test_lfu_trace(cap):
    t = load_golden("cache_traces")
    tabs = _tables_for_traces(t)
    reqs = t["requests_flush"] if cap == 80 else t["requests"]
    c = orc.LFU(cap, tabs)
    want = _unpack_hits(t["lfu_cap%d_hits" % cap], len(reqs))
    for i, rq in enumerate(reqs):
        hit, vals = c.request(rq)
        assert np.array_equal(hit, want[i]), "request %d" % i
        assert np.array_equal(vals[7], tabs[7][rq[7]])
    np.testing.assert_array_equal(c.dump(), t["lfu_cap%d_final_freq" % cap])


def test_reader_rows(tmp_path):
    t = load_golden("cache_traces")
    tabs = _tables_for_traces(t)
    for k, w in enumerate(tabs):
        w.tofile(tmp_path / ("ev-table-%d.bin" % (k + 1)))
    for (tb, r), want in zip(t["reader_probe"], t["reader_rows"]):
        got = orc.read_row(str(tmp_path), int(tb), int(r))
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("name", ["dlrm_ragged_small", "dlrm_kaggle_small", "dlrm_d64"])
def test_cpu_port_matches_golden(name):
    """oracle/dlrm_cpu.py (bench.py's cpu_baseline) reproduces the reference's outputs exactly: the pooled rows of the recorded
    batch bit for bit, and the interaction bit for bit on the same x and pooled rows snapped to a grid on which every product
    and sum is exact in fp32 (<name>_interact_exact.npz, the reference's interact_features on them).  The R of the raw batch
    holds the recording host's sgemm rounding, which the BLAS of other CPUs does not reproduce: the port's R of it is held to
    it bit for bit on the x columns and within the sgemm rounding bound on the interaction columns."""
    import torch
    from oracle import dlrm_cpu
    g = load_golden(name)
    tabs = [torch.from_numpy(t) for t in split_tables(g)]
    lS_o, lS_i = split_indices(g)
    m = dlrm_cpu.CpuHotPath(tabs)
    with torch.no_grad():
        ly = m.apply_emb([torch.from_numpy(o) for o in lS_o], [torch.from_numpy(i) for i in lS_i])
    np.testing.assert_array_equal(np.stack([v.numpy() for v in ly]), g["ly"])
    R = m.step([torch.from_numpy(o) for o in lS_o], [torch.from_numpy(i) for i in lS_i], torch.from_numpy(g["x"]))
    d = int(g["m_spa"])
    assert R.shape == g["R"].shape
    np.testing.assert_array_equal(R.numpy()[:, :d], g["R"][:, :d])
    # ... and its interaction columns within the rounding either sgemm may make of the same dot products, in any order of
    # summation: |fl(sum) - sum| <= d u sum |a_k b_k| for each side, u = 2^-24
    T = np.concatenate([g["x"][:, None, :], np.transpose(g["ly"], (1, 0, 2))], axis=1).astype(np.float64)
    A = np.abs(T) @ np.abs(np.transpose(T, (0, 2, 1)))
    F = T.shape[1]
    li, lj = np.tril_indices(F, -1)
    bound = 2 * d * 2.0 ** -24 * A[:, li, lj]
    assert np.all(np.abs(R.numpy()[:, d:].astype(np.float64) - g["R"][:, d:]) <= bound)
    e = load_golden(name + "_interact_exact")
    assert e["R"].shape == g["R"].shape and np.count_nonzero(e["R"][:, d:]) > 0.9 * e["R"][:, d:].size
    with torch.no_grad():
        Re = m.interact_features(torch.from_numpy(e["x"]), [torch.from_numpy(v) for v in e["ly"]])
    np.testing.assert_array_equal(Re.numpy(), e["R"])


def _c1c2_decoded_tables():
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as G
    _, tabs = G.c1c2_tables(orc)
    return ([orc.decode(t[0], 8, 36) for t in tabs], [orc.decode(t[1], 4, 36) for t in tabs],
            [t[0] for t in tabs], [t[1] for t in tabs])


def test_c1c2_routing_matches_compiled_reference():
    """oracle.C1C2 (evlfu_8.cpp:669-796 restated) vs the reference's own libcachemanager on the same
    stream: identical serving precision for every key until C1 fills; afterwards the C++ evicts in
    unordered_set order (not reproducible) so agreement is statistical (>= 99.5 % per 500 requests)."""
    g = load_golden("c1c2_ref")
    dec8, dec4, _, _ = _c1c2_decoded_tables()
    reqs, ref = g["requests"], g["served_bits"]
    c = orc.C1C2(int(g["cap_c1"]), int(g["cap_c2"]), dec8, dec4)
    mine = np.zeros_like(ref)
    for i, rq in enumerate(reqs):
        tier, out, _ = c.request(rq)
        for k in range(26):
            mine[i, k] = 8 if np.array_equal(out[k], dec8[k][rq[k]]) else (4 if np.array_equal(out[k], dec4[k][rq[k]]) else 0)
    assert (mine != 0).all()  # the restatement never serves a wrong row (the C++ does: 205 rows, hazard g)
    first_ref = int(np.argmax((ref == 4).any(1)))
    assert int(np.argmax((mine == 4).any(1))) == first_ref and first_ref > 9000
    assert np.array_equal(mine[:first_ref], ref[:first_ref])
    for a in range(first_ref - first_ref % 500, len(reqs), 500):
        ok = ref[a:a + 500] != 0
        assert (mine[a:a + 500][ok] == ref[a:a + 500][ok]).mean() >= 0.995


# ------------------------------------------------------------------ the other precision builds of the reference manager
def _variant_decoded():
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as G
    tabs, reqs = G.variant_tables(orc)
    dec = {32: [t[0] for t in tabs], 16: [orc.decode(t[1], 16, 36) for t in tabs],
           8: [orc.decode(t[2], 8, 36) for t in tabs], 4: [orc.decode(t[3], 4, 36) for t in tabs]}
    return dec, reqs


def test_tier_capacities_as_the_reference_constructs_them():
    assert orc.ref_tier_capacities(3, 8, 4, 75425, "48-48-4") == (144816, 289632, 108612)   # c1c2_ref.npz's build
    assert orc.ref_tier_capacities(2, 32, 8, 4000) == (2000, 32000, 0)    # the double x4 of an 8-bit secondary tier
    assert orc.ref_tier_capacities(2, 16, 8, 4000) == (4000, 32000, 0)
    assert orc.ref_tier_capacities(2, 32, 16, 4000) == (2000, 4000, 0)
    assert orc.ref_tier_capacities(2, 32, 4, 4000) == (2000, 16000, 0)
    assert orc.ref_tier_capacities(2, 16, 4, 4000) == (4000, 16000, 0)
    assert orc.ref_tier_capacities(2, 8, 4, 4000) == (8000, 16000, 0)
    assert orc.ref_tier_capacities(1, 4, 4, 3000) == (24000, 0, 0)


@pytest.mark.parametrize("var", ["2-32-16-4000", "2-32-8-4000", "2-32-4-4000", "2-16-8-4000", "2-16-4-4000", "2-8-4-4000"])
def test_c1c2_precision_builds_match_compiled_reference(var):
    """request_to_c1_c2 of the 32- and 16-bit main tiers (evlfu_32.cpp:319-473, evlfu_16.cpp:443-592) and the plain 8/4
    two-tier build, each COMPILED from the reference with its #defines set (oracle/Makefile MGR_VARIANTS): the serving
    precision of every key equals the oracle's until C1 fills (afterwards the C++ evicts in unordered_set order:
    agreement >= 99 % per 100-request block, garbage rows of the reference -- hazard g -- excluded), with the
    capacities the reference's constructors compute (incl. the x16 of an 8-bit secondary tier)."""
    g = load_golden("mgr_variants")
    dec, reqs = _variant_decoded()
    assert np.array_equal(reqs, g["requests"])
    L, M, S, T = [int(v) for v in var.split("-")]
    ref = g["v" + var.replace("-", "_") + "_served"]
    c1, c2, _ = orc.ref_tier_capacities(L, M, S, T)
    c = orc.C1C2(c1, c2, dec[M], dec[S])
    mine = np.zeros_like(ref)
    perfect = []
    blk = int(g["block"])
    n_perf = 0
    for i, rq in enumerate(reqs):
        tier, out, rc = c.request(rq)
        n_perf += int(rc == 1)
        for k in range(26):
            mine[i, k] = M if np.array_equal(out[k], dec[M][k][rq[k]]) else (S if np.array_equal(out[k], dec[S][k][rq[k]]) else 0)
        if (i + 1) % blk == 0:
            perfect.append(n_perf)
            n_perf = 0
    assert (mine != 0).all()
    first_ref = int(np.argmax((ref == S).any(1)))
    assert int(np.argmax((mine == S).any(1))) == first_ref and first_ref > 20
    assert np.array_equal(mine[:first_ref], ref[:first_ref])
    agree = []
    for a in range(0, len(reqs), blk):
        ok = ref[a:a + blk] != 0
        agree.append((mine[a:a + blk][ok] == ref[a:a + blk][ok]).mean())
    assert min(agree) >= 0.99, agree
    # perfect-hit counter (cache_manager.cpp:262-290 prints and resets it): exact while nothing was evicted
    nb = first_ref // blk
    assert perfect[:nb] == list(g["v" + var.replace("-", "_") + "_perfect"][:nb])


@pytest.mark.parametrize("var", ["1-32-4-3000", "1-16-4-3000", "1-8-4-3000", "1-4-4-3000"])
def test_single_tier_precision_builds_perfect_hits(var):
    """N_CACHING_LAYER 1 builds (request_to_ev_lfu of evlfu_32/16/8/4.cpp): rows decode at the tier's precision and the
    perfect-hit counter per 100 requests equals the oracle's EvLFU('cpp') with the reference's capacity until the cache
    fills, and stays within a band afterwards (eviction order of an unordered_set)."""
    g = load_golden("mgr_variants")
    dec, reqs = _variant_decoded()
    L, M, S, T = [int(v) for v in var.split("-")]
    tag = "v" + var.replace("-", "_")
    served = g[tag + "_served"]
    assert ((served == M) | (served == 0)).all() and (served == 0).mean() < 0.005
    cap = orc.ref_tier_capacities(1, M, S, T)[0]
    c = orc.EvLFU(cap, dec[M], 36, "cpp")
    blk = int(g["block"])
    perfect, n = [], 0
    fill_at = None
    for i, rq in enumerate(reqs):
        hit, vals = c.request(rq)
        n += int(hit.all())
        if fill_at is None and c.state()["size"] >= cap:
            fill_at = i
        if (i + 1) % blk == 0:
            perfect.append(n)
            n = 0
    ref = list(g[tag + "_perfect"])
    nb = (fill_at if fill_at is not None else len(reqs)) // blk
    assert nb >= 1 and perfect[:nb] == ref[:nb]
    assert abs(sum(perfect) - sum(ref)) <= max(8, 0.4 * sum(ref)), (sum(perfect), sum(ref))


# ------------------------------------------------------------------ a12: the alt-key tier's single-key methods
def _aprx_alt_tables():
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as G
    return G.aprx_inputs()[0]


@pytest.mark.parametrize("cap", [50, 64, 257])
def test_altkey_tier_ops_match_reference_driven_single_threaded(cap):
    """APRX_EV's public methods (insert_altkey, get_altkey_str, set_recency_flag_c3, evict_one_key;
    aprx_embedding.cpp:278-288,341-350,360-411) of the COMPILED reference, driven from one thread by
    oracle/ref/ref_aprx_driver.cpp: every lookup result, every alt key decoded from the big-endian files, and the
    final FIFO (stale duplicates included) equal the oracle's.  What stays unpinned: WHEN an evicted-key batch
    becomes visible (5 racing threads) and insert_altkey_batched_obj itself (uninitialised loop counters)."""
    g = load_golden("aprx_ops")
    alt = _aprx_alt_tables()
    t = orc.AltKeyTier(cap, alt)
    ops = g["cap%d_ops" % cap]
    res = t.apply(ops)
    assert t.state()["error"] == 0
    np.testing.assert_array_equal(res, g["cap%d_res" % cap])
    np.testing.assert_array_equal(t.queue(), g["cap%d_queue" % cap])
    assert t.state()["size"] <= cap


def test_collate_criteo_offset_restated_equals_reference():
    """oracle/dlrm_cpu.py collate_criteo_offset against the reference's collate_wrapper_criteo_offset (dlrm_data_pytorch.py:397-410;
    tests/golden/collate_criteo.npz, `make_golden.py collate`): the two index tensors bit for bit, X within one ulp (torch's
    vectorised log may pick another code path on another host; on the recording host it is bit-equal)."""
    import torch
    from oracle import dlrm_cpu
    g = load_golden("collate_criteo")
    X, lS_o, lS_i = dlrm_cpu.collate_criteo_offset(g["x_int"], g["x_cat"])
    assert X.dtype == torch.float32 and lS_o.dtype == torch.int64 and lS_i.dtype == torch.int64
    assert np.array_equal(lS_o.numpy(), g["lS_o"]) and np.array_equal(lS_i.numpy(), g["lS_i"])
    np.testing.assert_array_max_ulp(X.numpy(), g["X"], maxulp=1)


def test_terabyte_transform_features_restated_equals_reference():
    """oracle/dlrm_cpu.py transform_features_terabyte against the reference's _transform_features over a (B, 40) record block
    (script/data_loader_terabyte.py:68-87,226-236; tests/golden/collate_terabyte.npz), with and without max_ind_range."""
    import torch
    from oracle import dlrm_cpu
    g = load_golden("collate_terabyte")
    for rng, tag in ((-1, "all"), (1000, "r1000")):
        X, lS_o, lS_i = dlrm_cpu.transform_features_terabyte(g["rec"], rng)
        assert np.array_equal(lS_o.numpy(), g["lS_o_" + tag]) and np.array_equal(lS_i.numpy(), g["lS_i_" + tag])
        np.testing.assert_array_max_ulp(X.numpy(), g["X_" + tag], maxulp=1)
