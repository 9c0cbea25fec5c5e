"""Warm start of the batched set-associative cache tier (GpuCache.export_state / load_state / save_state over
evs_cache_batch_export / evs_cache_batch_load; csrc/evs_cache_warm.hip) held to the contract in include/evstore_hip.h: a cache
loaded strictly from an export continues exactly as the exporter does -- flags, rows, counters and the next export, under every
entry point of the tier --, a load with strict=False places what the Python restatement of the plan (tests/_warm_start_model.py)
says, the rows really are copied into the arena, and everything out of scope is refused with the cache left usable.
Streams are conflict-free (tests/_batched_policy_model.py, tests/_bag_evlfu_model.py), so the rule is deterministic."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _bag_evlfu_model as EM
import _batched_policy_model as M
import _warm_start_model as W

pytestmark = pytest.mark.gpu

N_ROWS = [40, 1000, 5000]
T = len(N_ROWS)
D = 36
GROUPS_PER_BLOCK = 16       # csrc/evs_cache_warm.hip: 16 lanes per entry, blocks of 256 threads


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_made = {}


def _tables(codec=32, d=D, n_rows=N_ROWS):
    """tables in the tier's codec, filled on the device: fp32 uniform in (-1, 1), else raw random bytes; shared by the tests
    that do not write them"""
    key = (codec, d, tuple(n_rows))
    if key not in _made:
        g = torch.Generator(device="cuda")
        g.manual_seed(7 + codec + d)
        if codec == 32:
            _made[key] = [torch.empty(n, d, device="cuda").uniform_(-1, 1, generator=g) for n in n_rows]
        else:
            _made[key] = [torch.randint(0, 256, (n, d * codec // 8), dtype=torch.uint8, device="cuda", generator=g) for n in n_rows]
    return _made[key]


def _cache(E, policy, cap, dev, codec=32, d=D):
    c = E.GpuCache(policy, cap, len(dev), d, codec, "python")
    c.set_backing(dev)
    return c


def _dump(c):
    d = c.batch_dump()
    out = {(int(t), int(r)): int(s) for s, t, r in d}
    assert len(out) == len(d)
    return out


def _step(c, form, call, x=None):
    """one batched call -> (flags, rows / R / pooled bags) as tensors"""
    if form == "batch":
        return c.lookup_batch(call)
    if form == "interact":
        return c.lookup_interact(call, x)
    hits, ly = c.lookup_bags(*call)
    return torch.cat(hits), torch.stack(ly)


def _same_export(a, b):
    return np.array_equal(a["entries"], b["entries"]) and np.array_equal(a["state"], b["state"]) and np.array_equal(a["n_rows"], b["n_rows"])


def _stream(policy, cap, B, n_batches, seed, n_rows=N_ROWS):
    """-> ((n_batches, B, T) int32 rows, the model's strict snapshot flags)"""
    if policy == "evlfu":
        reqs, flags, _model = EM.conflict_free_rows_stream(cap, n_rows, B, n_batches, seed)
    else:
        reqs, flags, _model = M.conflict_free_stream(policy, cap, n_rows, B, n_batches, seed)
    return reqs, flags


def quiet_stream(cap, n_rows, B, n_batches, seed):
    """EvLFU's one-launch form raises hit ways and claims victims in ONE launch, so its outcome is pinned only when no set sees
    both in a batch: every batch splits the sets into those that get exactly one new key and those whose resident keys are
    requested.  Every request names at least one new key, so no priority reaches T and nothing flushes (the flush's victims are
    a matter of timing).  -> (rows, the model's flags, the model, the largest top bucket)"""
    rs = np.random.RandomState(seed)
    model = EM.BagEvLFUModel(cap, n_rows)
    nt, nset = len(n_rows), model.nset
    sets_of = [M.set_of(t, np.arange(n_rows[t]), nset, n_rows, model.bits) for t in range(nt)]
    rows, flags, top = np.zeros((n_batches, B, nt), np.int32), np.zeros((n_batches, B, nt), bool), 0
    for n in range(n_batches):
        order = rs.permutation(nset)
        new_sets, hit_sets = order[:max(nt, nset // 2)], set(order[max(nt, nset // 2):].tolist())
        new, options = [[] for _ in range(nt)], [[] for _ in range(nt)]
        for i, s in enumerate(new_sets):
            t = i % nt
            cand = [int(r) for r in np.nonzero(sets_of[t] == s)[0] if (t + 1, int(r)) not in model.where]
            if cand:
                new[t].append(cand[rs.randint(len(cand))])
        for (t1, r), (s, _j) in model.where.items():
            if s in hit_sets:
                options[t1 - 1].append(r)
        options = [o + w for o, w in zip(options, new)]
        with_new = [t for t in range(nt) if new[t]]
        assert all(options) and with_new, "batch %d: a table without a key to ask for" % n
        rows[n] = np.stack([rs.choice(options[t], B) for t in range(nt)], 1)
        for b in range(B):
            t = with_new[rs.randint(len(with_new))]
            rows[n, b, t] = new[t][rs.randint(len(new[t]))]
        f = model.batch_bags(*EM.one_per_bag(rows[n]))
        flags[n] = np.stack(f, 1)
        top = max(top, model.top_bucket())
    return rows, flags, model, top


def _twin(E, policy, form, cap, B, k, m, seed, codec=32, prepare=None, calls=None, want_flags=None, x=None):
    """k calls on A, export, strict load into a fresh B (the round trip), m more calls on both (the continuation)"""
    dev = _tables(codec)
    a, b = _cache(E, policy, cap, dev, codec), _cache(E, policy, cap, dev, codec)
    if prepare:
        prepare(a)                                    # (B is told nothing: load_state applies what the export carries)
    for i in range(k):
        _step(a, form, calls[i], x)
    sa = a.export_state()
    info = b.load_state(sa)
    sb = b.export_state()
    st = a.batch_stats()
    assert info == {"placed": len(sa["entries"]), "turned_away": 0, "batch": k} and sa["state"][6] == k
    assert sa["entries"].shape == (st["size"], 5) and np.all(np.diff(sa["entries"][:, 4]) > 0)
    assert _same_export(sa, sb), "the export of the loaded cache differs"
    assert _dump(a) == _dump(b)
    assert st == b.batch_stats() and sum(st["hist"]) == st["size"]
    for i in range(k, k + m):
        fa, ra = _step(a, form, calls[i], x)
        fb, rb = _step(b, form, calls[i], x)
        assert torch.equal(fa, fb), "call %d: flags" % (i + 1)
        if want_flags is not None:
            assert np.array_equal(fa.cpu().numpy().astype(bool).reshape(-1), np.asarray(want_flags[i]).reshape(-1)), "call %d: flags against the model" % (i + 1)
        assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)), "call %d: rows" % (i + 1)
        assert a.batch_stats() == b.batch_stats(), "call %d: counters" % (i + 1)
    assert _same_export(a.export_state(), b.export_state())
    return a, b, st, a.batch_stats()


# ------------------------------------------------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("codec", [32, 8])
@pytest.mark.parametrize("policy", ["evlfu", "lru", "lfu"])
def test_round_trip(E, policy, codec):
    cap, B, k = 128, 16, 24
    reqs, flags = _stream(policy, cap, B, k + 2, 40)
    a, b, st0, st1 = _twin(E, policy, "batch", cap, B, k, 2, 40, codec, calls=_dev(reqs), want_flags=flags)
    assert st0["size"] > cap // 2 and st0["n_hits"] > 0


# ------------------------------------------------------------------------------------------------- 2. twin continuation
def test_twin_continuation_evlfu_one_launch_form(E):
    """lookup_interact of an fp32 EvLFU tier makes its update inside the probe launch (14 stamp bits here)"""
    cap, B, k, m = 64, 32, 28, 8
    reqs, flags, model, top = quiet_stream(cap, N_ROWS, B, k + m, 3)
    assert top == 0, "the stream must stay clear of the flush"
    x = torch.empty(B, D, device="cuda").uniform_(-1, 1)
    a, b, st0, st1 = _twin(E, "evlfu", "interact", cap, B, k, m, 3, calls=_dev(reqs), want_flags=flags, x=x)
    assert st0["size"] == cap and st1["n_evict"] > st0["n_evict"] and st1["n_flush"] == 0     # full sets: victims by restored priority
    assert a.export_state()["state"][14] == 1
    assert _dump(a) == model.resident()


def test_twin_continuation_evlfu_chain(E):
    """set_inline_update(False): probe, consumer and update as launches of their own; the loaded cache learns it from the state"""
    cap, B, k, m = 64, 32, 28, 8
    reqs, flags = _stream("evlfu", cap, B, k + m, 41)
    x = torch.empty(B, D, device="cuda").uniform_(-1, 1)
    a, b, st0, st1 = _twin(E, "evlfu", "interact", cap, B, k, m, 41, prepare=lambda c: c.set_inline_update(False), calls=_dev(reqs), want_flags=flags, x=x)
    assert st0["size"] == cap and st1["n_evict"] > st0["n_evict"] and st1["n_flush"] == 0
    assert b.export_state()["state"][14] == 0


def test_twin_continuation_evlfu_bags(E):
    """ragged bags under the "served bags" rule; the loaded cache learns the rule from the state"""
    cap, B, k, m = 64, 16, 28, 8
    calls, model, top = EM.conflict_free_bag_stream(cap, N_ROWS, B, 3, k + m, 42)
    assert top < int(cap * 0.95)
    dev_calls = [([_dev(o) for o in off], [_dev(i) for i in idx]) for off, idx, _f in calls]
    want = [np.concatenate(f) for _o, _i, f in calls]
    a, b, st0, st1 = _twin(E, "evlfu", "bags", cap, B, k, m, 42, prepare=lambda c: c.set_bag_rule("served-bags"), calls=dev_calls, want_flags=want)
    assert st0["size"] == cap and st1["n_evict"] > st0["n_evict"] and st1["n_flush"] == 0
    assert b.export_state()["state"][13] == 1 and _dump(a) == model.resident()


@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_twin_continuation_lru_lfu(E, policy):
    cap, B, k, m = 64, 32, 28, 8
    reqs, flags = _stream(policy, cap, B, k + m, 43)
    a, b, st0, st1 = _twin(E, policy, "batch", cap, B, k, m, 43, calls=_dev(reqs), want_flags=flags)
    assert st0["size"] == cap and st1["n_evict"] > st0["n_evict"]       # full sets: victims by restored age / counter


# ------------------------------------------------------------------------------------------- 3. the rows are in the arena
@pytest.mark.parametrize("n_entries", [1, 7, 2 * GROUPS_PER_BLOCK + 1, 4 * GROUPS_PER_BLOCK * 4 + 1])
@pytest.mark.parametrize("codec,d", [(32, 36), (8, 36), (4, 36), (32, 64), (32, 4)])
def test_loaded_rows_are_served_from_the_arena(E, codec, d, n_entries):
    """A resident key's backing row is overwritten behind the cache's back: the lookup still serves the loaded copy, and the new
    row after refresh_rows.  u4 rows of d = 36 are 18 bytes (one 16-byte piece + the 2-byte tail), u8 36, fp32 d = 4 one piece."""
    cap = 512
    g = torch.Generator(device="cuda")
    g.manual_seed(n_entries + d)
    if codec == 32:
        dev = [torch.empty(n, d, device="cuda").uniform_(-1, 1, generator=g) for n in N_ROWS]
    else:
        dev = [torch.randint(0, 256, (n, d * codec // 8), dtype=torch.uint8, device="cuda", generator=g) for n in N_ROWS]
    rs = np.random.RandomState(n_entries)
    nset, bits = M.geometry(cap, N_ROWS)
    pool, per_set, take = W.random_entries(rs, "lru", N_ROWS, 3 * n_entries, 5), np.zeros(nset, int), []
    for i, e in enumerate(pool):                       # at most 6 of a set: every entry is placed and the sets keep room
        s_ = int(M.set_of(e[0] - 1, e[1], nset, N_ROWS, bits))
        if per_set[s_] < 6 and len(take) < n_entries:
            per_set[s_] += 1
            take.append(i)
    entries = pool[take]
    dest, _words, out4 = W.plan("lru", cap, N_ROWS, entries)
    assert out4[0] == n_entries == len(entries)
    c = _cache(E, "lru", cap, dev, codec, d)
    assert c.load_state({"entries": entries, "state": None}, strict=False) == {"placed": n_entries, "turned_away": 0, "batch": int(entries[:, 3].max())}
    keys = [(int(t), int(r)) for t, r in entries[:, :2]]
    # one request per loaded key, the other columns filled with rows nothing has loaded (they miss, are served from the table
    # and take free ways)
    room = np.bincount(dest // M.WAYS, minlength=nset) < M.WAYS - 1
    spare = [next(r for r in range(N_ROWS[t]) if (t + 1, r) not in keys and room[int(M.set_of(t, r, nset, N_ROWS, bits))]) for t in range(T)]
    rq = np.array([[r if t + 1 == t1 else spare[t] for t in range(T)] for t1, r in keys], np.int32)
    col = np.array([t1 - 1 for t1, _ in keys])
    hit0, out0 = c.lookup_batch(_dev(rq))
    picked0 = out0[torch.arange(len(keys)), _dev(col)].clone()
    assert bool(hit0[torch.arange(len(keys)), _dev(col)].all()), "a loaded key is not resident"
    fresh = _cache(E, "lru", cap, dev, codec, d)      # the same rows through the miss path: the tables as they are
    _h, ref0 = fresh.lookup_batch(_dev(rq))
    assert torch.equal(out0.view(torch.int32), ref0.view(torch.int32))
    for (t1, r) in keys:                               # written directly, not through update_rows
        if codec == 32:
            dev[t1 - 1][r] += 1.0
        else:
            dev[t1 - 1][r] = dev[t1 - 1][r] ^ 0x5A
    torch.cuda.synchronize()
    _h, out1 = c.lookup_batch(_dev(rq))
    assert torch.equal(out1[torch.arange(len(keys)), _dev(col)].view(torch.int32), picked0.view(torch.int32)), "the old row is not served from the arena"
    n_res = c.refresh_rows(np.array([[t1 - 1, r] for t1, r in keys], np.int64), count=True)
    assert n_res == n_entries
    _h, out2 = c.lookup_batch(_dev(rq))
    fresh2 = _cache(E, "lru", cap, dev, codec, d)
    _h, ref2 = fresh2.lookup_batch(_dev(rq))
    got, want = out2[torch.arange(len(keys)), _dev(col)], ref2[torch.arange(len(keys)), _dev(col)]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and not torch.equal(got.view(torch.int32), picked0.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- 4. stamp wrap
def test_lfu_across_stamp_wraps(E):
    """`tiny` (tests/test_gpu_stamp_wrap.py): two sets, 22 tag bits, S = 4 -- the stamp wraps every 16 batches.  40 batches on A
    (two wraps), export, load, and both run on across seven more wraps, held to the modular model's flags all along."""
    cap, n_rows, S = M.WRAP_GEOMETRIES["tiny"]
    assert M.stamp_bits_of("lfu", cap, n_rows)[2] == S["lfu"] == 4
    batches, hits, model, parted = M.wrap_case("lfu", "tiny")
    dev = _tables(32, 4, n_rows)
    a, b = _cache(E, "lfu", cap, dev, 32, 4), _cache(E, "lfu", cap, dev, 32, 4)
    k = 40
    for i in range(k):
        a.lookup_batch(_dev(batches[i]))
    sa = a.export_state()
    assert sa["state"][12] == 4 and sa["state"][6] == k and sa["entries"][:, 3].max() < 16
    assert b.load_state(sa)["batch"] == k
    assert _same_export(sa, b.export_state())
    for i in range(k, len(batches)):
        fa, ra = a.lookup_batch(_dev(batches[i]))
        fb, rb = b.lookup_batch(_dev(batches[i]))
        assert torch.equal(fa, fb) and np.array_equal(fb.cpu().numpy().astype(bool), hits[i]), "batch %d" % (i + 1)
        assert torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    assert _same_export(a.export_state(), b.export_state()) and a.batch_stats() == b.batch_stats()
    assert _dump(b) == model.resident() and len(batches) - k > 6 * 16


def test_evlfu_across_stamp_wraps(E):
    """the same geometry under EvLFU (the two-launch chain: S = 4 is below the one-launch form's 8 bits): the exporter is 21
    batches old, so stamps of both sides of the wrap are resident; both run on over two more wraps"""
    cap, n_rows, S = M.WRAP_GEOMETRIES["tiny"]
    assert M.stamp_bits_of("evlfu", cap, n_rows)[2] == S["evlfu"] == 4
    dev = _tables(32, 4, n_rows)
    rs = np.random.RandomState(9)
    perms = [rs.permutation(n)[:24] for n in n_rows]
    k, m, B = 21, 36, 4
    reqs = [np.stack([M.zipf_rows(rs, 24, B, 1.2, perms[t]) for t in range(len(n_rows))], 1).astype(np.int32) for _ in range(k + m)]
    a, b = _cache(E, "evlfu", cap, dev, 32, 4), _cache(E, "evlfu", cap, dev, 32, 4)
    for i in range(k):
        a.lookup_batch(_dev(reqs[i]))
    sa = a.export_state()
    assert sa["state"][12] == 4 and 0 <= sa["entries"][:, 3].min() and sa["entries"][:, 3].max() < 16
    b.load_state(sa)
    assert _same_export(sa, b.export_state()) and _dump(a) == _dump(b)
    # (the stream is not conflict-free -- 16 ways under Zipf rows --, so which of two new keys of a set stays is the kernels'
    #  choice: the twins are compared on what the rule pins -- strict snapshot flags against each twin's own residents)
    for i in range(k, k + m):
        for c in (a, b):
            res = _dump(c)
            f, _r = c.lookup_batch(_dev(reqs[i]))
            was = np.array([[(t + 1, int(r)) in res for t, r in enumerate(row)] for row in reqs[i]])
            assert np.array_equal(f.cpu().numpy().astype(bool), was), "batch %d" % (i + 1)
    assert a.batch_stats()["n_requests"] == b.batch_stats()["n_requests"] == (k + m) * B


# -------------------------------------------------------------------------------------------------------- 5. re-placement
@pytest.mark.parametrize("cap_to", [64, 256])
@pytest.mark.parametrize("policy", ["evlfu", "lru", "lfu"])
def test_replacement_into_another_capacity(E, policy, cap_to):
    cap, B, k = 128, 16, 24
    reqs, _flags = _stream(policy, cap, B, k + 1, 44)
    dev = _tables()
    a = _cache(E, policy, cap, dev)
    for i in range(k):
        a.lookup_batch(_dev(reqs[i]))
    sa = a.export_state()
    dest, words, out4 = W.plan(policy, cap_to, N_ROWS, sa["entries"], sa["state"], strict=False)
    b = _cache(E, policy, cap_to, dev)
    with pytest.raises(E._lib.EvsError):               # a strict load holds the cache to the exporter's capacity
        b.load_state(sa)
    info = b.load_state(sa, strict=False)
    assert info == {"placed": out4[0], "turned_away": out4[1], "batch": k}
    if cap_to < cap:
        assert info["turned_away"] > 0
    else:
        assert info["turned_away"] == 0
    sb = b.export_state()
    keep = dest >= 0
    order = np.argsort(dest[keep])
    want = sa["entries"][keep][order].copy()
    want[:, 4] = dest[keep][order]
    want[:, 3] = np.minimum(want[:, 3], (1 << out4[2]) - 2)
    assert np.array_equal(sb["entries"], want)         # the resident set, scores, ages and ways the model says
    assert len(_dump(b)) == info["placed"] <= cap_to
    st = b.batch_stats()
    assert st["size"] == info["placed"] and st["n_free"] == cap_to - info["placed"] and sum(st["hist"]) == st["size"]
    assert [st[n] for n in ("n_flush", "n_evict", "n_requests", "n_perfect_hits", "n_hits")] == [int(v) for v in sa["state"][7:12]]
    res = {(int(t), int(r)) for t, r in want[:, :2]}
    f, out = b.lookup_batch(_dev(reqs[k]))
    was = np.array([[(t + 1, int(r)) in res for t, r in enumerate(row)] for row in reqs[k]])
    assert np.array_equal(f.cpu().numpy().astype(bool), was)
    for t in range(T):
        assert torch.equal(out[:, t].view(torch.int32), dev[t][_dev(reqs[k][:, t].astype(np.int64))].view(torch.int32))


@pytest.mark.parametrize("policy", ["evlfu", "lru", "lfu"])
def test_hand_made_list_without_a_state(E, policy):
    cap = 64
    rs = np.random.RandomState(5)
    entries = W.random_entries(rs, policy, N_ROWS, 90, 300)
    dest, words, out4 = W.plan(policy, cap, N_ROWS, entries)
    assert out4[1] > 0
    c = _cache(E, policy, cap, _tables())
    assert c.load_state({"entries": entries, "state": None}, strict=False) == {"placed": out4[0], "turned_away": out4[1], "batch": int(entries[:, 3].max())}
    st = c.batch_stats()
    assert [st[n] for n in ("n_tomb", "n_flush", "n_evict", "n_requests", "n_perfect_hits", "n_hits")] == [0] * 6 and st["size"] == out4[0]
    if policy == "evlfu":
        assert st["hist"] == np.bincount(entries[dest >= 0][:, 2], minlength=T + 1).tolist()
    else:
        assert st["hist"] == [out4[0]] + [0] * T
    s = c.export_state()
    assert s["state"][6] == entries[:, 3].max() and np.array_equal(s["entries"][:, 4], np.sort(dest[dest >= 0]))
    assert {(int(t), int(r)) for t, r in s["entries"][:, :2]} == set(W.resident_after(entries, dest))


# ------------------------------------------------------------------------------------------------------ 6. flush on load
def test_evlfu_flush_is_asked_for_by_the_load(E):
    """cap 64: max_perfect = int(0.95 * 64) = 60, flush_n = int(0.3 * 64) + 1 = 20.  60 keys at the top priority (sets 0 .. 3
    keep a free way) ask for the flush as a close would; the next batched call runs it before its probe: 20 top entries go,
    its three new keys (sets 0 .. 2, priority 0) take free ways."""
    cap = 64
    nset, bits = M.geometry(cap, N_ROWS)
    per_set = {s: [] for s in range(nset)}
    for t in (1, 2):
        for r in range(N_ROWS[t]):
            per_set[int(M.set_of(t, r, nset, N_ROWS, bits))].append((t + 1, r))
    keys = [k for s in range(nset) for k in per_set[s][:7 if s < 4 else 8]]
    assert len(keys) == 60
    entries = np.array([[t1, r, T, 1, 0] for t1, r in keys], np.int64)
    c = _cache(E, "evlfu", cap, _tables())
    assert c.load_state({"entries": entries, "state": None}, strict=False)["placed"] == 60
    new = []
    for t in range(T):                                 # one new key per table, in sets 0, 1, 2
        r = next(r for r in range(N_ROWS[t]) if int(M.set_of(t, r, nset, N_ROWS, bits)) == t and (t + 1, r) not in keys)
        new.append(r)
    f, _out = c.lookup_batch(_dev(np.array([new], np.int32)))
    assert not f.any()
    st = c.batch_stats()
    assert st["n_flush"] == 1 and st["hist"] == [3, 0, 0, 40] and st["size"] == 43 and st["n_evict"] == 0
    d = _dump(c)
    assert sum(1 for k in keys if k in d) == 40 and all(d[(t + 1, r)] == 0 for t, r in enumerate(new))
    # below max_perfect nothing is asked for
    c2 = _cache(E, "evlfu", cap, _tables())
    c2.load_state({"entries": entries[:59], "state": None}, strict=False)
    c2.lookup_batch(_dev(np.array([new], np.int32)))
    assert c2.batch_stats()["n_flush"] == 0 and c2.batch_stats()["hist"][T] == 59


# ----------------------------------------------------------------------------------------------------------- 7. refusals
def _refused(E, call, code, word):
    with pytest.raises(E._lib.EvsError) as ei:
        call()
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def _serves(c, dev, rq=((3, 17, 4000), (3, 17, 4000))):
    """two batches through lookup_batch: the rows are the tables', the second batch hits"""
    rq = torch.tensor(rq, dtype=torch.int32, device="cuda")
    for i in range(2):
        hit, out = c.lookup_batch(rq)
        for t in range(T):
            assert torch.equal(out[:, t].view(torch.int32), dev[t][rq[:, t].long()].view(torch.int32))
    assert bool(hit.all())


def test_refusals_of_the_scope_table(E, tmp_path):
    L = E._lib
    dev = _tables()
    good = {"entries": np.array([[1, 5, 0, 0, 0]], np.int64), "state": None}
    good_evlfu = {"entries": np.array([[1, 5, 1, 0, 0]], np.int64), "state": None}
    # a tier of a C1 + C2 lookup
    c1, c2 = E.GpuCache("evlfu", 64, T, D, 32, "cpp"), E.GpuCache("evlfu", 128, T, D, 32, "cpp")
    c1.set_backing(dev)
    c2.set_backing(dev)
    rq = torch.tensor([[3, 17, 4000]], dtype=torch.int32, device="cuda")
    E.lookup_batch_c1c2(c1, c2, rq, threshold=2)
    for c in (c1, c2):
        _refused(E, lambda: c.load_state(good_evlfu, strict=False), L.EVS_EINVAL, "C1 + C2")
        _refused(E, c.export_state, L.EVS_EINVAL, "C1 + C2")
    tier, out = E.lookup_batch_c1c2(c1, c2, rq, threshold=2)
    assert torch.equal(out[0, 1].view(torch.int32), dev[1][17].view(torch.int32))
    # a batch policy that is plan / sampled
    for name in ("plan", "sampled"):
        c = _cache(E, "evlfu", 64, dev).set_batch_policy(name)
        _refused(E, lambda: c.load_state(good_evlfu, strict=False), L.EVS_EINVAL, name)
        _serves(c, dev)
        _refused(E, c.export_state, L.EVS_EINVAL, name)
    # a geometry that resolves to sampled: a capacity below one set
    c = _cache(E, "evlfu", 4, dev)
    _refused(E, lambda: c.load_state(good_evlfu, strict=False), L.EVS_EINVAL, "sampled")
    # host-memory and file-backed tables
    host = [t.cpu().pin_memory() for t in dev]
    for policy, state in (("evlfu", good_evlfu), ("lru", good)):
        c = E.GpuCache(policy, 64, T, D, 32, "python")
        c.set_backing(host)
        _refused(E, lambda: c.load_state(state, strict=False), L.EVS_ESTATE, "HBM")
    paths = []
    for t in range(T):
        p = tmp_path / ("ev-table-%d.bin" % (t + 1))
        dev[t].cpu().numpy().tofile(str(p))
        paths.append(str(p))
    ft = E.gpu_cache.FileTier(paths, D * 4, 1 << 30)
    c = E.GpuCache("evlfu", 64, T, D, 32, "python")
    c.set_file_backing(ft)
    _refused(E, lambda: c.load_state(good_evlfu, strict=False), L.EVS_ESTATE, "HBM")
    hit, out = c.lookup_batch(rq)
    assert torch.equal(out[0, 1].view(torch.int32), dev[1][17].view(torch.int32))
    del c
    ft.close()
    # no backing yet; a cache driven by the exact path; a resident server
    c = E.GpuCache("lru", 64, T, D, 32, "python")
    _refused(E, lambda: c.load_state(good, strict=False), L.EVS_ESTATE, "set_backing")
    c.set_backing(dev)
    c.request(rq)
    _refused(E, lambda: c.load_state(good, strict=False), L.EVS_ESTATE, "exact")
    hit, out = c.request(rq)
    assert bool(hit.all()) and torch.equal(out[0, 2].view(torch.int32), dev[2][4000].view(torch.int32))
    c = _cache(E, "evlfu", 64, dev)
    c.serve_start(n_slots=2)
    try:
        with pytest.raises(L.EvsError) as ei:
            c.load_state(good_evlfu, strict=False)
        assert ei.value.code == L.EVS_ESTATE
        hit, view = c.serve_request([3, 17, 4000])
        assert torch.equal(view[1].view(torch.int32), dev[1][17].view(torch.int32))
    finally:
        c.serve_stop()


@pytest.mark.parametrize("switch,value,want", [("EVS_SA_WAYS", "16", "ways"), ("EVS_CACHE_POLICY", "sampled", "sampled")])
def test_refusals_behind_a_process_wide_switch(switch, value, want):
    """16-way sets and a policy that comes from EVS_CACHE_POLICY: both switches are read once per process, so the refusal is
    checked in a child (tests/_warm_start_env_child.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("EVS_SA_WAYS", "EVS_CACHE_POLICY")}
    env[switch] = value
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_warm_start_env_child.py"), want], env=env, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


@pytest.mark.parametrize("policy", ["evlfu", "lru", "lfu"])
def test_refusals_of_the_input_load_nothing(E, policy):
    L = E._lib
    cap = 64
    dev = _tables()
    sc = {"evlfu": 1, "lru": 0, "lfu": 5}[policy]
    good = np.array([[1, 3, sc, 2, 0], [2, 17, sc, 0, 0], [3, 4000, sc, 7, 0]], np.int64)
    dest, _w, _o = W.plan(policy, cap, N_ROWS, good)
    S = M.stamp_bits_of(policy, cap, N_ROWS)[2]
    state = np.array([1, W.POLICY_ID[policy], cap, T, D, 32, 9, 0, 0, 0, 0, 0, S, 0, -1, 0], np.int64)
    c = _cache(E, policy, cap, dev)

    def with_(i, col, v, base=good):
        e = base.copy()
        e[i, col] = v
        return e

    def st_(pos, v):
        s = state.copy()
        s[pos] = v
        return s

    strict_good = good.copy()
    strict_good[:, 4] = dest
    other = [p for p in ("evlfu", "lru", "lfu") if p != policy][0]
    bad_score = {"evlfu": T + 1, "lru": 1, "lfu": 0}[policy]
    cases = [(with_(0, 0, 0), None, False, "table"), (with_(0, 0, T + 1), None, False, "table"), (with_(1, 1, 1000), None, False, "row"),
             (with_(1, 1, -1), None, False, "row"), (np.concatenate([good, good[:1]]), None, False, "duplicate"),
             (with_(0, 2, bad_score), None, False, "score"), (with_(2, 3, -1), None, False, "age"),
             (good, st_(0, 2), False, "version"), (good, st_(1, W.POLICY_ID[other]), False, "policy"),
             (strict_good, None, True, "strict"), (strict_good, st_(2, 128), True, "capacity"), (strict_good, st_(3, 2), True, "capacity"),
             (strict_good, st_(12, S - 1), True, "capacity"), (with_(0, 4, (dest[0] + 8) % 64, strict_good), state, True, "slot")]
    for entries, st, strict, word in cases:
        with pytest.raises(L.EvsError) as ei:
            c.load_state({"entries": entries, "state": st}, strict=strict)
        assert ei.value.code == L.EVS_EINVAL and word in str(ei.value), (word, str(ei.value))
    # a strict load checks the tables' row counts too
    with pytest.raises(L.EvsError):
        c.load_state({"entries": strict_good, "state": state, "n_rows": np.array([40, 1000, 4999])}, strict=True)
    # nothing was loaded and the cache is as fresh as before: the good list goes in, strictly
    assert c.load_state({"entries": strict_good, "state": state, "n_rows": np.array(N_ROWS)}) == {"placed": 3, "turned_away": 0, "batch": 9}
    assert set(_dump(c)) == {(1, 3), (2, 17), (3, 4000)}
    # ... and a second load finds the batched path in use
    with pytest.raises(L.EvsError) as ei:
        c.load_state({"entries": strict_good, "state": state})
    assert ei.value.code == L.EVS_ESTATE and "already" in str(ei.value)
    rq = _dev(np.array([[3, 17, 4000], [4, 18, 4001]], np.int32))
    hit, out = c.lookup_batch(rq)
    assert hit.cpu().numpy().tolist() == [[1, 1, 1], [0, 0, 0]]
    for t in range(T):
        assert torch.equal(out[:, t].view(torch.int32), dev[t][rq[:, t].long()].view(torch.int32))
    st = c.batch_stats()
    assert st["size"] == 6 and st["n_requests"] == 2 and st["n_hits"] == 3
    # an empty load is a load: it needs no launch and leaves a usable, empty batched path
    e = _cache(E, policy, cap, dev)
    assert e.load_state({"entries": np.zeros((0, 5), np.int64), "state": None}, strict=False) == {"placed": 0, "turned_away": 0, "batch": 0}
    assert e.batch_stats()["size"] == 0 and len(e.export_state()["entries"]) == 0
    # a used cache refuses a load
    with pytest.raises(L.EvsError) as ei:
        e.load_state({"entries": good, "state": None}, strict=False)
    assert ei.value.code == L.EVS_ESTATE
    # an export before anything batched happened
    with pytest.raises(L.EvsError):
        _cache(E, policy, cap, dev).export_state()


# ------------------------------------------------------------------------------------------------ 8. lives with the rest
@pytest.mark.parametrize("policy", ["lru", "lfu"])
def test_a_loaded_cache_lives_with_the_other_entry_points(E, policy):
    """after a load: update_rows finds the loaded keys, the dump is the export's, and lookup_batch / lookup_bags (one index per
    bag: the same rule) alternate on the loaded twin exactly as on the replayed one"""
    cap, B, k, m = 64, 16, 20, 8
    reqs, flags = _stream(policy, cap, B, k + m, 45)
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    dev = [torch.empty(n, D, device="cuda").uniform_(-1, 1, generator=g) for n in N_ROWS]      # (written below: not shared)
    a, b = _cache(E, policy, cap, dev), _cache(E, policy, cap, dev)
    for i in range(k):
        a.lookup_batch(_dev(reqs[i]))
    sa = a.export_state()
    b.load_state(sa)
    d = _dump(b)
    assert set(d) == {(int(t), int(r)) for t, r in sa["entries"][:, :2]} and d == _dump(a)
    keys = np.array([[t - 1, r] for t, r in sa["entries"][:, :2]] + [[2, 4999]], np.int64)      # every loaded key + one that is not
    assert (2 + 1, 4999) not in d
    vals = torch.empty(len(keys), D, device="cuda").uniform_(-1, 1, generator=g)
    assert b.update_rows(keys, vals, count=True) == len(sa["entries"])
    assert a.refresh_rows(keys, count=True) == len(sa["entries"])                               # (the twin shares the tables)
    lo = [torch.arange(B, dtype=torch.int64, device="cuda")] * T
    for i in range(k, k + m):
        rq = _dev(reqs[i])
        if i & 1:
            (ha, la), (hb, lb) = a.lookup_bags(lo, list(rq.long().t().contiguous())), b.lookup_bags(lo, list(rq.long().t().contiguous()))
            fa, fb, ra, rb = torch.stack(ha, 1), torch.stack(hb, 1), torch.stack(la, 1), torch.stack(lb, 1)
        else:
            (fa, ra), (fb, rb) = a.lookup_batch(rq), b.lookup_batch(rq)
        assert torch.equal(fa, fb) and np.array_equal(fb.cpu().numpy().astype(bool), flags[i]), "call %d" % (i + 1)
        assert torch.equal(ra.view(torch.int32), rb.view(torch.int32))
        for t in range(T):
            assert torch.equal(rb[:, t].view(torch.int32), dev[t][rq[:, t].long()].view(torch.int32)), "call %d: a stale row" % (i + 1)
        assert a.batch_stats() == b.batch_stats()
    assert _same_export(a.export_state(), b.export_state())


# ------------------------------------------------------------------------------------------------------ 9. file round trip
def test_file_round_trip(E, tmp_path):
    L = E._lib
    cap, B, k, m = 64, 16, 20, 3
    reqs, flags = _stream("lfu", cap, B, k + m, 46)
    dev = _tables()
    a, b = _cache(E, "lfu", cap, dev), _cache(E, "lfu", cap, dev)
    for i in range(k):
        a.lookup_batch(_dev(reqs[i]))
    path = str(tmp_path / "tier.npz")
    a.save_state(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["entries", "n_rows", "state"] and z["state"][0] == 1
    assert b.load_state(path)["batch"] == k
    for i in range(k, k + m):
        (fa, ra), (fb, rb) = a.lookup_batch(_dev(reqs[i])), b.lookup_batch(_dev(reqs[i]))
        assert torch.equal(fa, fb) and np.array_equal(fb.cpu().numpy().astype(bool), flags[i])
        assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)) and a.batch_stats() == b.batch_stats()
    assert _same_export(a.export_state(), b.export_state())
    # a truncated file, a file of version 2, a file without the table sizes
    raw = open(path, "rb").read()
    cut = str(tmp_path / "cut.npz")
    open(cut, "wb").write(raw[:len(raw) // 2])
    s = a.export_state()
    v2 = str(tmp_path / "v2.npz")
    st2 = s["state"].copy()
    st2[0] = 2
    np.savez(v2, entries=s["entries"], state=st2, n_rows=s["n_rows"])
    part = str(tmp_path / "part.npz")
    np.savez(part, entries=s["entries"], state=s["state"])
    for p in (cut, v2, part, str(tmp_path / "none.npz")):
        c = _cache(E, "lfu", cap, dev)
        with pytest.raises(L.EvsError):
            c.load_state(p)
        assert c.load_state(path)["batch"] == k                                # the refusal left the cache fresh
