"""Warm start of the batched C1 + C2 pair (export_state_c1c2 / load_state_c1c2 / save_state_c1c2 over evs_cache_pair_export /
evs_cache_pair_load; the pair form of csrc/evs_cache_warm.hip) held to the contract in include/evstore_hip.h: a pair loaded
strictly from an export continues exactly as the exporter does -- tier codes, rows, both tiers' counters, the next export --, a
non-strict load places what the Python restatement of the plan (tests/_pair_warm_model.py) says, the rows really are copied
into both arenas, and everything out of scope is refused with both caches left fresh."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _pair_warm_model as P

pytestmark = pytest.mark.gpu

N_ROWS = [40, 1000, 5000]
T = len(N_ROWS)
D = 36
GROUPS_PER_BLOCK = 16       # csrc/evs_cache_warm.hip: 16 lanes per entry, blocks of 256 threads, 4 entries in flight per group


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _new_tables(codec, d=D, seed=0):
    g = torch.Generator(device="cuda")
    g.manual_seed(11 + codec + d + seed)
    if codec == 32:
        return [torch.empty(n, d, device="cuda").uniform_(-1, 1, generator=g) for n in N_ROWS]
    return [torch.randint(0, 256, (n, d * codec // 8), dtype=torch.uint8, device="cuda", generator=g) for n in N_ROWS]


_made = {}


def _tables(codec, d=D):
    """tables in a tier's codec, shared by the tests that do not write them"""
    if (codec, d) not in _made:
        _made[(codec, d)] = _new_tables(codec, d)
    return _made[(codec, d)]


def _decoded(E, tables, codec, d=D):
    """the fp32 rows a tier of `codec` serves from `tables`, per table: read through the miss path of a fresh cache, once"""
    c = E.GpuCache("lru", 64, T, d, codec, "python")
    c.set_backing(tables)
    n = max(N_ROWS)
    rq = np.stack([np.minimum(np.arange(n), r - 1) for r in N_ROWS], 1).astype(np.int32)
    _h, out = c.lookup_batch(_dev(rq))
    return [out[:N_ROWS[t], t].clone() for t in range(T)]


_dec = {}


def _dec_shared(E, codec, d=D):
    if (codec, d) not in _dec:
        _dec[(codec, d)] = _decoded(E, _tables(codec, d), codec, d)
    return _dec[(codec, d)]


def _pair(E, caps, codecs=(8, 4), d=D, tables=None):
    t1, t2 = tables or (_tables(codecs[0], d), _tables(codecs[1], d))
    c1, c2 = E.GpuCache("evlfu", caps[0], T, d, codecs[0], "cpp"), E.GpuCache("evlfu", caps[1], T, d, codecs[1], "cpp")
    c1.set_backing(t1)
    c2.set_backing(t2)
    return c1, c2


def _dump(c):
    d = c.batch_dump()
    out = {(int(t), int(r)): int(s) for s, t, r in d}
    assert len(out) == len(d)
    return out


def _same_export(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("entries", "state", "n_rows1", "n_rows2"))


def _keys(export, tier):
    e = export["entries"]
    return {(int(t), int(r)) for t, r in e[e[:, 0] == tier][:, 1:3]}


def _warm(E, pair, B, thr, seed, min_c2=1, max_batches=400, uniform=False):
    """Zipf (or uniform) batches until C2 holds at least min_c2 entries -> the number of calls"""
    rs = np.random.RandomState(seed)
    k = 0
    while True:
        if uniform:
            rq = np.stack([rs.randint(0, n, B) for n in N_ROWS], 1).astype(np.int32)
        else:
            rq = np.stack([np.minimum(rs.zipf(1.15, B) - 1, n - 1) for n in N_ROWS], 1).astype(np.int32)
        E.lookup_batch_c1c2(pair[0], pair[1], _dev(rq), threshold=thr)
        k += 1
        if k % 4 == 0 and pair[1].batch_stats()["size"] >= min_c2:
            return k
        assert k < max_batches, "C2 never filled"


def _round_trip(E, caps, B=32, thr=2, seed=5, min_c2=1, uniform=False):
    """k calls on pair A, export, strict load into a fresh pair B -> (a, b, export of A, k); asserts the round trip"""
    a, b = _pair(E, caps), _pair(E, caps)
    k = _warm(E, a, B, thr, seed, min_c2, uniform=uniform)
    sa = E.export_state_c1c2(*a)
    n1, n2 = int((sa["entries"][:, 0] == 1).sum()), int((sa["entries"][:, 0] == 2).sum())
    assert n2 >= min_c2 and n1 > 0, "the exporter's C2 holds nothing"
    info = E.load_state_c1c2(b[0], b[1], sa)
    assert info == {"placed": (n1, n2), "turned_away": (0, 0), "batch": k}
    sb = E.export_state_c1c2(*b)
    assert _same_export(sa, sb), "the export of the loaded pair differs"
    e = sa["entries"]
    assert e.shape[1] == 6 and np.all(np.diff(e[:, 0] * (1 << 32) + e[:, 5]) > 0), "sorted by (tier, slot)"
    for k_ in (0, 1):
        assert _dump(a[k_]) == _dump(b[k_]) and set(_dump(a[k_])) == _keys(sa, k_ + 1)
        st = a[k_].batch_stats()
        assert st == b[k_].batch_stats() and sum(st["hist"]) == st["size"] == (n1, n2)[k_]
    return a, b, sa, k


def _expected(geom, export, rq, thr):
    """tier code and serving tier per position of a batch against the exported snapshot: 1 / 2 = resident there; a double miss
    is routed to C1 while the key's own C1 set has a free way, else by the reference's rule (agg_hit below the threshold: odd
    table index -> C1, even -> C2; else C2)"""
    in1, in2 = _keys(export, 1), _keys(export, 2)
    e = export["entries"]
    occ = np.bincount(e[e[:, 0] == 1][:, 5] // geom.tiers[0].ways, minlength=geom.nset)
    code, serve = np.zeros(rq.shape, np.uint8), np.zeros(rq.shape, np.uint8)
    for b in range(rq.shape[0]):
        h1 = [(t + 1, int(rq[b, t])) in in1 for t in range(T)]
        h2 = [(t + 1, int(rq[b, t])) in in2 for t in range(T)]
        agg = sum(h1) + sum(h2)
        for t in range(T):
            if h1[t]:
                code[b, t] = serve[b, t] = 1
            elif h2[t]:
                code[b, t] = serve[b, t] = 2
            else:
                full = occ[geom.record(t, int(rq[b, t]))] >= geom.tiers[0].ways
                serve[b, t] = 1 if not full else ((1 if t % 2 == 1 else 2) if agg < thr else 2)
    return code, serve


def _check_rows(out, rq, serve, dec1, dec2, what=""):
    rq_t = _dev(rq).long()
    for t in range(T):
        want = torch.where(_dev(serve[:, t] == 1)[:, None], dec1[t][rq_t[:, t]], dec2[t][rq_t[:, t]])
        assert torch.equal(out[:, t].view(torch.int32), want.view(torch.int32)), "%s table %d: rows" % (what, t)


# ------------------------------------------------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("caps", [(64, 128), (64, 96), (32, 128)])
def test_round_trip(E, caps):
    """(64, 128): 8 + 2 x 8 ways; (64, 96): 8 + 12 and (32, 128): 4 + 2 x 8 -- the shapes that take the unfolded chain"""
    a, b, sa, k = _round_trip(E, caps)
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    st = sa["state"]
    assert list(st[:4]) == [3, T, D, geom.nset] and not st[28:].any()
    for i, t in enumerate(geom.tiers):
        blk = st[P.TIER0 + i * P.BLOCK:P.TIER0 + (i + 1) * P.BLOCK]
        assert list(blk[:6]) == [caps[i], (8, 4)[i], t.ways, 1 << t.sub_shift, t.S, k] and blk[P.B_REQ] == 32 * k and blk[11] == 0
    # every exported slot lies in its key's effective set, and the export is what the model's strict plan takes
    dest, _w, out8 = P.plan(geom, sa["entries"], st, strict=True)
    assert np.array_equal(dest, sa["entries"][:, 5]) and out8[6] == k


# ---------------------------------------------------------------------------------------- 2. the first batch after the load
@pytest.mark.parametrize("caps", [(64, 128), (64, 96)])
def test_first_batch_after_the_load(E, caps):
    thr = 2
    a, b, sa, k = _round_trip(E, caps)
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    rs = np.random.RandomState(9)
    e = sa["entries"]
    B = 48
    rq = np.stack([rs.randint(0, n, B) for n in N_ROWS], 1).astype(np.int32)
    for b_ in range(B):                                  # two columns of three name an exported key where the table has one
        for t in rs.permutation(T)[:2]:
            rows = e[e[:, 1] == t + 1][:, 2]
            if len(rows):
                rq[b_, t] = rows[rs.randint(len(rows))]
    code, serve = _expected(geom, sa, rq, thr)
    assert (code == 1).any() and (code == 2).any() and (code == 0).any()
    dec1, dec2 = _dec_shared(E, 8), _dec_shared(E, 4)
    for name, pair in (("exporter", a), ("loaded", b)):
        tier, out = E.lookup_batch_c1c2(pair[0], pair[1], _dev(rq), threshold=thr)
        assert np.array_equal(tier.cpu().numpy(), code), name + ": tier codes are membership in the exported lists"
        _check_rows(out, rq, serve, dec1, dec2, name)


# ------------------------------------------------------------------------------------------- 3. the rows are in the arenas
@pytest.mark.parametrize("n_entries", [1, 7, 2 * GROUPS_PER_BLOCK + 1, 4 * GROUPS_PER_BLOCK * 4 + 1])
@pytest.mark.parametrize("codecs,d", [((8, 4), 36), ((32, 8), 36), ((8, 4), 16)])
def test_loaded_rows_are_served_from_the_arenas(E, codecs, d, n_entries):
    """n_entries per tier (one below, across and well past a block's 16 groups x 4 in flight) from a hand-made list without a
    state.  The loaded keys' backing rows are overwritten in both tiers' tables behind the caches' back: the pair still serves
    the loaded copies, and the new rows after refresh_rows on both tiers.  Row widths: u8 d = 36 is 2 x 16 + 4 bytes, u4 16 + 2,
    fp32 9 x 16; d = 16: u8 one piece, u4 8 bytes (a tail alone)."""
    caps, thr = (512, 1024), 2
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    tabs = (_new_tables(codecs[0], d, n_entries), _new_tables(codecs[1], d, n_entries + 1))
    dec_old = (_decoded(E, tabs[0], codecs[0], d), _decoded(E, tabs[1], codecs[1], d))
    rs = np.random.RandomState(n_entries + d)
    # at most 5 keys per C1 set and 6 per effective C2 set: every entry is placed, and the three spare keys below find free ways
    # even if they fall into one set
    per_set, rows, keys = (np.zeros(geom.nset, int), np.zeros(geom.n_slots(2) // geom.tiers[1].ways, int)), [], set()
    for tier in (1, 2):
        got = 0
        while got < n_entries:
            t = int(rs.randint(T))
            r = int(rs.randint(N_ROWS[t]))
            es = geom.place(tier, t, r)[0]
            if (t + 1, r) in keys or per_set[tier - 1][es] >= 7 - tier or r == N_ROWS[t] - 1:      # (the last row of a table: its spare)
                continue
            keys.add((t + 1, r))
            per_set[tier - 1][es] += 1
            rows.append([tier, t + 1, r, int(rs.randint(0, T)), int(rs.randint(5)), 0])
            got += 1
    entries = np.array(rows, np.int64)
    rs.shuffle(entries)
    dest, _w, out8 = P.plan(geom, entries)
    assert out8[0] == out8[3] == n_entries and out8[1] == out8[4] == 0
    c1, c2 = _pair(E, caps, codecs, d, tabs)
    info = E.load_state_c1c2(c1, c2, {"entries": entries, "state": None}, strict=False)
    assert info == {"placed": (n_entries, n_entries), "turned_away": (0, 0), "batch": int(entries[:, 4].max())}
    # one request per loaded key; the other columns name one spare row per table that nothing has loaded
    spare = [n - 1 for n in N_ROWS]
    rq = np.array([[e[2] if t + 1 == e[1] else spare[t] for t in range(T)] for e in entries], np.int32)
    col, tier_of = _dev(entries[:, 1] - 1), entries[:, 0]
    idx = torch.arange(len(entries), device="cuda")

    def picked(dec):
        d1 = torch.stack([dec[0][e[1] - 1][e[2]] for e in entries.tolist()])
        d2 = torch.stack([dec[1][e[1] - 1][e[2]] for e in entries.tolist()])
        return torch.where(_dev(tier_of == 1)[:, None], d1, d2)

    tier0, out0 = E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=thr)
    assert np.array_equal(tier0[idx, col].cpu().numpy(), tier_of), "a loaded key is not resident in its tier"
    want_old = picked(dec_old)
    assert torch.equal(out0[idx, col].view(torch.int32), want_old.view(torch.int32))
    for tab, codec in zip(tabs, codecs):                # written directly, not through update_rows
        for (t1, r) in keys:
            tab[t1 - 1][r] = tab[t1 - 1][r] + 1.0 if codec == 32 else tab[t1 - 1][r] ^ 0x5A
    torch.cuda.synchronize()
    tier1, out1 = E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=thr)
    assert np.array_equal(tier1[idx, col].cpu().numpy(), tier_of)
    assert torch.equal(out1[idx, col].view(torch.int32), want_old.view(torch.int32)), "the old row is not served from the arena"
    kk = np.array([[t1 - 1, r] for t1, r in sorted(keys)], np.int64)
    assert c1.refresh_rows(kk, count=True) == n_entries and c2.refresh_rows(kk, count=True) == n_entries
    _t, out2 = E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=thr)
    want_new = picked((_decoded(E, tabs[0], codecs[0], d), _decoded(E, tabs[1], codecs[1], d)))
    assert torch.equal(out2[idx, col].view(torch.int32), want_new.view(torch.int32))
    assert not torch.equal(want_new.view(torch.int32), want_old.view(torch.int32))


# ------------------------------------------------------------------------------------------------- 4. twin continuation
def _quiet_batch(rs, geom, resident, used, B):
    """One batch whose outcome does not depend on timing: every request names exactly one new key (a key never asked for
    before, so in neither tier) and resident keys in its other columns; the B new keys fall into B different set records."""
    by_table = [[r for (t1, r) in resident if t1 == t + 1] for t in range(T)]
    assert all(by_table), "a table without a resident key"
    rq = np.stack([rs.choice(by_table[t], B) for t in range(T)], 1).astype(np.int32)
    recs = set()
    for b in range(B):
        while True:
            t = int(rs.choice([1, 2, 0], p=[0.45, 0.45, 0.1]))            # (table 0 has 40 rows: it runs out of new keys first)
            r = int(rs.randint(N_ROWS[t]))
            rec = geom.record(t, r)
            if (t + 1, r) not in used and rec not in recs:
                break
        recs.add(rec)
        used.add((t + 1, r))
        rq[b, t] = r
    return rq


@pytest.mark.parametrize("caps,form", [((512, 1024), "batch"), ((512, 1024), "interact"), ((64, 128), "interact")])
def test_twin_continuation(E, caps, form):
    """After the strict load, m = 8 more batches on both pairs: tier codes, rows / R bits, both tiers' counters after every call
    and the final exports are equal.  (64, 128) and (512, 1024) are 8 + 2 x 8 ways: lookup_interact_c1c2 runs the folded probe.

    The stream makes the pair's rule independent of timing.  Per batch at most one new key per set RECORD: the routing reads
    "a free way in the key's own C1 set" off the snapshot and C1 and C2 share the record index, so two new keys of one record
    could race for a way.  Every new key is named by exactly one request (no two requests route it differently), and every
    request names a new key, so its agg_hit stays below T: no priority reaches T and nothing flushes (the flush's victims are
    a matter of timing).  The raises run in the probe launch and the inserts in the update launch behind it, so victims are
    chosen among settled priorities.  The stream is built batch by batch from the exporter's dumps: a key is "new" when no
    batch has named it, "resident" when the exporter's dump holds it."""
    thr, m = 3, 8                                        # agg_hit = 2 < 3: a full C1 set sends odd tables to C1, even ones to C2
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    B = min(16, geom.nset)
    a, b = _pair(E, caps), _pair(E, caps)
    rs = np.random.RandomState(caps[0])
    used = set()
    k = 0
    while True:                                          # the fill: uniform batches until both tiers are nearly full
        rq = np.stack([rs.randint(0, n, 256) for n in N_ROWS], 1).astype(np.int32)
        used |= {(t + 1, int(r)) for t in range(T) for r in rq[:, t]}
        E.lookup_batch_c1c2(a[0], a[1], _dev(rq), threshold=thr)
        k += 1
        if a[0].batch_stats()["size"] >= 0.9 * caps[0] and a[1].batch_stats()["size"] >= 0.9 * caps[1]:
            break
        assert k < 200
    sa = E.export_state_c1c2(*a)
    assert E.load_state_c1c2(b[0], b[1], sa)["batch"] == k
    assert _same_export(sa, E.export_state_c1c2(*b))
    st0 = [c.batch_stats() for c in a]
    x = torch.empty(B, D, device="cuda").uniform_(-1, 1)
    for i in range(m):
        resident = set(_dump(a[0])) | set(_dump(a[1]))
        rq = _dev(_quiet_batch(rs, geom, resident, used, B))
        if form == "batch":
            (ta, ra), (tb, rb) = E.lookup_batch_c1c2(a[0], a[1], rq, threshold=thr), E.lookup_batch_c1c2(b[0], b[1], rq, threshold=thr)
        else:
            (ta, ra), (tb, rb) = E.lookup_interact_c1c2(a[0], a[1], rq, x, threshold=thr), E.lookup_interact_c1c2(b[0], b[1], rq, x, threshold=thr)
        assert torch.equal(ta, tb), "call %d: tier codes" % (i + 1)
        assert int((ta == 0).sum()) == B, "call %d: one new key per request" % (i + 1)
        assert torch.equal(ra.view(torch.int32), rb.view(torch.int32)), "call %d: rows" % (i + 1)
        for k_ in (0, 1):
            assert a[k_].batch_stats() == b[k_].batch_stats(), "call %d: counters of C%d" % (i + 1, k_ + 1)
            assert _dump(a[k_]) == _dump(b[k_]), "call %d: residents of C%d" % (i + 1, k_ + 1)
    assert _same_export(E.export_state_c1c2(*a), E.export_state_c1c2(*b))
    for k_ in (0, 1):
        st = a[k_].batch_stats()
        assert st["n_evict"] > st0[k_]["n_evict"], "the continuation did not evict in C%d" % (k_ + 1)
        assert st["n_flush"] == st0[k_]["n_flush"]


# ------------------------------------------------------------------------------------------------------ 5. re-placement
@pytest.mark.parametrize("caps_to", [(128, 256), (48, 40)])
def test_replacement_into_another_geometry(E, caps_to):
    a, _b, sa, k = _round_trip(E, (64, 128))
    geom = P.Geometry(caps_to[0], caps_to[1], N_ROWS)
    dest, _w, out8 = P.plan(geom, sa["entries"], sa["state"], strict=False)
    c1, c2 = _pair(E, caps_to)
    with pytest.raises(E._lib.EvsError):                # another geometry: not strictly
        E.load_state_c1c2(c1, c2, sa)
    info = E.load_state_c1c2(c1, c2, sa, strict=False)
    assert info == {"placed": (out8[0], out8[3]), "turned_away": (out8[1], out8[4]), "batch": k}
    if caps_to == (48, 40):
        assert out8[4] > 0, "the smaller pair must turn entries away"
    e = sa["entries"]
    for tier, c in ((1, c1), (2, c2)):
        want = {(int(r[1]), int(r[2])): int(r[3]) for r, d_ in zip(e, dest) if r[0] == tier and d_ >= 0}
        assert _dump(c) == want, "C%d: the resident keys (and their priorities) are the plan's" % tier
        assert set(want) <= _keys(sa, tier), "a key changed tier"
    ex = E.export_state_c1c2(c1, c2)
    m = dest >= 0
    order = np.lexsort((dest[m], e[m][:, 0]))
    assert np.array_equal(ex["entries"][:, [0, 1, 2, 3, 5]], np.column_stack([e[m][:, :4], dest[m]])[order])
    rs = np.random.RandomState(3)
    for i in range(6):                                   # every batch afterwards keeps the pair's invariants
        rq = np.stack([np.minimum(rs.zipf(1.15, 32) - 1, n - 1) for n in N_ROWS], 1).astype(np.int32)
        E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=2)
        d1, d2, s1, s2 = c1.batch_dump(), c2.batch_dump(), c1.batch_stats(), c2.batch_stats()
        n1, n2 = _dump(c1), _dump(c2)
        assert len(n1) == s1["size"] <= caps_to[0] and len(n2) == s2["size"] <= caps_to[1]
        assert not (set(n1) & set(n2)), "a key lives in one tier"
        assert np.array_equal(np.bincount(d1[:, 0], minlength=T + 1), s1["hist"]) and np.array_equal(np.bincount(d2[:, 0], minlength=T + 1), s2["hist"])


# ------------------------------------------------------------------------------------------------------ 6. flush on load
@pytest.mark.parametrize("tier", [1, 2])
def test_flush_is_asked_for_by_the_load(E, tier):
    """max_perfect = int(0.95 * capacity): 60 of C1's 64, 121 of C2's 128.  A hand-made list gives ONE tier that many entries at
    priority T: the next pair call runs that tier's flush (n_flush + 1) and leaves the other tier's alone; one entry fewer asks
    for nothing."""
    caps = (64, 128)
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    want = int(0.95 * caps[tier - 1])
    t = geom.tiers[tier - 1]
    n_eff = geom.nset << t.sub_shift
    per_set = {s: [] for s in range(n_eff)}
    for tab in (1, 2):
        for r in range(N_ROWS[tab]):
            per_set[geom.place(tier, tab, r)[0]].append((tab + 1, r))
    keys = [k for j in range(t.ways) for s in range(n_eff) for k in per_set[s][j:j + 1]][:want]
    other = [[3 - tier, 1, r, 1, 0, 0] for r in range(5)]             # a few entries of the other tier, low priority
    for n_top, flushes in ((want, 1), (want - 1, 0)):
        entries = np.array([[tier, t1, r, T, 1, 0] for t1, r in keys[:n_top]] + other, np.int64)
        c = _pair(E, caps)
        info = E.load_state_c1c2(c[0], c[1], {"entries": entries, "state": None}, strict=False)
        assert info["placed"][tier - 1] == n_top and info["turned_away"] == (0, 0)
        assert c[tier - 1].batch_stats()["hist"][T] == n_top or flushes     # (batch_stats runs a wanted flush itself)
        c = _pair(E, caps)
        E.load_state_c1c2(c[0], c[1], {"entries": entries, "state": None}, strict=False)
        E.lookup_batch_c1c2(c[0], c[1], _dev(np.array([[39, 999, 4999]], np.int32)), threshold=2)
        st = [x.batch_stats() for x in c]
        assert st[tier - 1]["n_flush"] == flushes and st[2 - tier]["n_flush"] == 0
        if flushes:
            assert st[tier - 1]["hist"][T] < n_top


# ----------------------------------------------------------------------------------------------------------- 7. refusals
def _refused(E, call, code, word):
    with pytest.raises(E._lib.EvsError) as ei:
        call()
    assert ei.value.code == code and word in str(ei.value), str(ei.value)


def _serves_cold(E, c1, c2, dec1, dec2, all_kept=True):
    """a cold pair: the first batch misses everywhere and is served from the tables, the second hits (all_kept=False: a tier too
    small to keep the first batch's six keys)"""
    rq = np.array([[3, 17, 4000], [5, 18, 4001]], np.int32)
    tier, out = E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=2)
    assert not tier.any()
    for t in range(T):
        rows = _dev(rq[:, t]).long()
        ok1, ok2 = out[:, t].view(torch.int32) == dec1[t][rows].view(torch.int32), out[:, t].view(torch.int32) == dec2[t][rows].view(torch.int32)
        assert bool((ok1.all(1) | ok2.all(1)).all())
    tier, _out = E.lookup_batch_c1c2(c1, c2, _dev(rq), threshold=2)
    assert bool((tier > 0).all()) or not all_kept
    assert c1.batch_stats()["n_requests"] == 4 and (c1.batch_stats()["size"] + c2.batch_stats()["size"] == 6 or not all_kept)


def test_refusals_of_the_envelope(E, tmp_path):
    L = E._lib
    dec1, dec2 = _dec_shared(E, 8), _dec_shared(E, 4)
    t8, t4 = _tables(8), _tables(4)
    good = {"entries": np.array([[1, 1, 5, 1, 0, 0], [2, 2, 17, 2, 1, 0]], np.int64), "state": None}

    def load(c1, c2, state=good, strict=False):
        return lambda: E.load_state_c1c2(c1, c2, state, strict=strict)

    # one fresh and one used cache (either way round); the used one keeps serving alone
    for used_first in (False, True):
        c1, c2 = _pair(E, (64, 128))
        used = c1 if used_first else c2
        used.lookup_batch(_dev(np.array([[3, 17, 4000]], np.int32)))
        _refused(E, load(c1, c2), L.EVS_ESTATE, "fresh")
        hit, _o = used.lookup_batch(_dev(np.array([[3, 17, 4000]], np.int32)))
        assert bool(hit.all())
    # an LRU cache
    c1 = E.GpuCache("lru", 64, T, D, 8, "cpp")
    c1.set_backing(t8)
    _c, c2 = _pair(E, (64, 128))
    _refused(E, load(c1, c2), L.EVS_EINVAL, "EvLFU")
    # tiers that disagree on dim
    c1, _c = _pair(E, (64, 128))
    c2 = E.GpuCache("evlfu", 128, T, 16, 4, "cpp")
    c2.set_backing(_tables(4, 16))
    _refused(E, load(c1, c2), L.EVS_EINVAL, "agree")
    # no backing yet
    c1, c2 = _pair(E, (64, 128))
    c2 = E.GpuCache("evlfu", 128, T, D, 4, "cpp")
    _refused(E, load(c1, c2), L.EVS_ESTATE, "set_backing")
    c2.set_backing(t4)
    _serves_cold(E, c1, c2, dec1, dec2)
    # a batch policy that is plan / sampled, on either tier
    for name in ("sampled", "plan"):
        for which in (0, 1):
            c = _pair(E, (64, 128))
            c[which].set_batch_policy(name)
            _refused(E, load(*c), L.EVS_EINVAL, name)
            _serves_cold(E, c[0], c[1], dec1, dec2)
    # ... or resolves to sampled: a tier below one set of 8 entries
    c = _pair(E, (4, 128))
    _refused(E, load(*c), L.EVS_EINVAL, "sampled")
    _serves_cold(E, c[0], c[1], dec1, dec2, all_kept=False)
    # capacities without a shared record: a tier would get fewer than 4 ways
    c = _pair(E, (16, 128))
    _refused(E, load(*c), L.EVS_EINVAL, "4 ways")
    _serves_cold(E, c[0], c[1], dec1, dec2)
    # pinned-host and file-backed tables
    c = _pair(E, (64, 128), tables=([t.cpu().pin_memory() for t in t8], t4))
    _refused(E, load(*c), L.EVS_ESTATE, "HBM")
    _serves_cold(E, c[0], c[1], dec1, dec2)
    paths = []
    for t in range(T):
        p = tmp_path / ("ev-table-%d.bin" % (t + 1))
        t4[t].cpu().numpy().tofile(str(p))
        paths.append(str(p))
    ft = E.gpu_cache.FileTier(paths, D * 4 // 8, 1 << 30)
    c1, _c = _pair(E, (64, 128))
    c2 = E.GpuCache("evlfu", 128, T, D, 4, "cpp")
    c2.set_file_backing(ft)
    _refused(E, load(c1, c2), L.EVS_ESTATE, "HBM")
    _serves_cold(E, c1, c2, dec1, dec2)
    del c2
    ft.close()
    # a tier set to fetch-first (a tier alone)
    c = _pair(E, (64, 128))
    c[0].set_miss_order("fetch-first")
    _refused(E, load(*c), L.EVS_EINVAL, "fetch-first")
    hit, _o = c[0].lookup_batch(_dev(np.array([[3, 17, 4000]], np.int32)))
    assert not hit.any()
    # a resident server running on a tier
    c = _pair(E, (64, 128))
    c[0].serve_start(n_slots=2)
    try:
        with pytest.raises(L.EvsError) as ei:
            load(*c)()
        assert ei.value.code == L.EVS_ESTATE
        hit, view = c[0].serve_request([3, 17, 4000])
        assert torch.equal(view[1].view(torch.int32), dec1[1][17].view(torch.int32))
    finally:
        c[0].serve_stop()
    # the exact path has served a tier
    c = _pair(E, (64, 128))
    c[1].request(_dev(np.array([[3, 17, 4000]], np.int32)))
    _refused(E, load(*c), L.EVS_ESTATE, "exact")
    # an export before the pair has run, and of two tiers that keep records of their own
    c = _pair(E, (64, 128))
    _refused(E, lambda: E.export_state_c1c2(*c), L.EVS_EINVAL, "pair")
    c = _pair(E, (16, 128))
    E.lookup_batch_c1c2(c[0], c[1], _dev(np.array([[3, 17, 4000]], np.int32)), threshold=2)
    _refused(E, lambda: E.export_state_c1c2(*c), L.EVS_EINVAL, "records of its own")


def test_refusal_behind_the_process_wide_switch():
    """EVS_SA_PAIR=0 is read once per process, so the refusal is checked in a child (tests/_pair_warm_env_child.py)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, EVS_SA_PAIR="0")
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "_pair_warm_env_child.py")], env=env, cwd=root,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def test_refusals_of_the_input_load_nothing(E):
    """every refusal of the plan comes back through the load, and behind each the two caches are as fresh as before: at the end
    a cold lookup starts the pair, or -- on a second pair -- the good list goes in strictly"""
    L = E._lib
    caps = (64, 128)
    geom = P.Geometry(caps[0], caps[1], N_ROWS)
    good = np.array([[1, 1, 3, 1, 2, 0], [1, 2, 999, 0, 0, 0], [2, 3, 4999, 3, 7, 0], [2, 2, 17, 2, 1, 0]], np.int64)
    dest, _w, _o = P.plan(geom, good)
    strict_good = good.copy()
    strict_good[:, 5] = dest
    state = P.state_of(geom, n=9, counters=(0, 0, 0, 0, 0))

    def with_(i, col, v, base=good):
        e = base.copy()
        e[i, col] = v
        return e

    def st_(pos, v):
        s = state.copy()
        s[pos] = v
        return s

    both = good[1:2].copy()
    both[0, 0] = 2
    cases = [(with_(0, 0, 3), None, False, "tier"), (with_(0, 1, T + 1), None, False, "table"), (with_(1, 2, 1000), None, False, "row"),
             (with_(2, 3, T + 1), None, False, "score"), (with_(3, 4, -1), None, False, "age"),
             (np.concatenate([good, good[:1]]), None, False, "duplicate"), (np.concatenate([good, both]), None, False, "both tiers"),
             (strict_good, None, True, "strict"), (strict_good, st_(P.TIER0 + P.B_CAP, 128), True, "geometry"),
             (strict_good, st_(P.TIER0 + P.BLOCK + P.B_SUBS, 1), True, "geometry"), (strict_good, st_(2, 16), True, "dim"),
             (with_(0, 5, (dest[0] + 8) % 64, strict_good), state, True, "slot")]
    pairs = [_pair(E, caps), _pair(E, caps)]
    for c in pairs:
        for entries, st, strict, word in cases:
            _refused(E, lambda: E.load_state_c1c2(c[0], c[1], {"entries": entries, "state": st}, strict=strict), L.EVS_EINVAL, word)
        # states of the other formats, at the Python surface and below it
        for version in (1, 2):
            _refused(E, lambda: E.load_state_c1c2(c[0], c[1], {"entries": good, "state": st_(0, version)}, strict=False), L.EVS_EINVAL, "version")
        out8 = np.zeros(8, np.int64)
        rc = L.lib().evs_cache_pair_load(c[0]._h, c[1]._h, 4, good.ctypes.data, st_(0, 1).ctypes.data, 0, out8.ctypes.data, None)
        assert rc == L.EVS_EINVAL and b"version" in L.lib().evs_last_error() and not out8.any()
        # a strict load checks the tables' row counts too
        with pytest.raises(L.EvsError):
            E.load_state_c1c2(c[0], c[1], {"entries": strict_good, "state": state, "n_rows1": np.array(N_ROWS), "n_rows2": np.array([40, 1000, 4999])})
        # wrong shapes
        _refused(E, lambda: E.load_state_c1c2(c[0], c[1], {"entries": good[:, :5], "state": None}, strict=False), L.EVS_EINVAL, "(n, 6)")
    # pair 0: as if the load had never been called
    _serves_cold(E, pairs[0][0], pairs[0][1], _dec_shared(E, 8), _dec_shared(E, 4))
    # pair 1: the good list goes in, strictly; a second load finds the pair in use; the single tier's calls still refuse a member
    c1, c2 = pairs[1]
    assert E.load_state_c1c2(c1, c2, {"entries": strict_good, "state": state}) == {"placed": (2, 2), "turned_away": (0, 0), "batch": 9}
    assert set(_dump(c1)) == {(1, 3), (2, 999)} and set(_dump(c2)) == {(3, 4999), (2, 17)}
    _refused(E, lambda: E.load_state_c1c2(c1, c2, {"entries": strict_good, "state": state}), L.EVS_ESTATE, "fresh")
    single = {"entries": np.array([[1, 5, 1, 0, 0]], np.int64), "state": None}
    for c in (c1, c2):
        _refused(E, lambda: c.load_state(single, strict=False), L.EVS_EINVAL, "C1 + C2")
        _refused(E, c.export_state, L.EVS_EINVAL, "C1 + C2")
    tier, _o = E.lookup_batch_c1c2(c1, c2, _dev(np.array([[3, 17, 4999], [4, 999, 4001]], np.int32)), threshold=2)
    assert tier.cpu().numpy().tolist() == [[1, 2, 2], [0, 1, 0]]
    # an empty load is a load: no launch, a usable empty pair, and the caches are no longer fresh
    e1, e2 = _pair(E, caps)
    assert E.load_state_c1c2(e1, e2, {"entries": np.zeros((0, 6), np.int64), "state": None}, strict=False) == {"placed": (0, 0), "turned_away": (0, 0), "batch": 0}
    assert e1.batch_stats()["size"] == 0 and len(E.export_state_c1c2(e1, e2)["entries"]) == 0
    _refused(E, lambda: E.load_state_c1c2(e1, e2, {"entries": good, "state": None}, strict=False), L.EVS_ESTATE, "fresh")


# ------------------------------------------------------------------------------------------------ 8. lives with the rest
def test_a_loaded_pair_lives_with_the_other_entry_points(E):
    caps, thr = (64, 128), 2
    tabs = (_new_tables(8, D, 77), _new_tables(4, D, 78))
    a, b = _pair(E, caps, tables=tabs), _pair(E, caps, tables=tabs)
    k = _warm(E, a, 32, thr, 6)
    sa = E.export_state_c1c2(*a)
    E.load_state_c1c2(b[0], b[1], sa)
    # batch_dump / batch_stats agree with the export
    e = sa["entries"]
    for i, c in enumerate(b):
        mine = e[e[:, 0] == i + 1]
        assert _dump(c) == {(int(r[1]), int(r[2])): int(r[3]) for r in mine}
        st = c.batch_stats()
        blk = sa["state"][P.TIER0 + i * P.BLOCK:P.TIER0 + (i + 1) * P.BLOCK]
        assert st["size"] == len(mine) and st["hist"] == np.bincount(mine[:, 3], minlength=T + 1).tolist()
        assert [st["n_flush"], st["n_evict"], st["n_requests"], st["n_perfect_hits"], st["n_hits"]] == list(blk[P.B_FLUSH:P.B_HITS + 1])
    # update_rows on both tiers changes the served rows of resident keys (checked against each tier's own re-decoded table)
    keys = np.array([[r[1] - 1, r[2]] for r in e] + [[2, 4999]] * ((3, 4999) not in {(int(r[1]), int(r[2])) for r in e}), np.int64)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    vals = torch.empty(len(keys), D, device="cuda").uniform_(-1, 1, generator=g)
    n1, n2 = b[0].update_rows(keys, vals, count=True), b[1].update_rows(keys, vals, count=True)
    assert (n1, n2) == (int((e[:, 0] == 1).sum()), int((e[:, 0] == 2).sum()))
    dec1, dec2 = _decoded(E, tabs[0], 8), _decoded(E, tabs[1], 4)
    rs = np.random.RandomState(2)
    rq = np.stack([rs.choice(e[e[:, 1] == t + 1][:, 2], 24) for t in range(T)], 1).astype(np.int32)
    code, serve = _expected(P.Geometry(caps[0], caps[1], N_ROWS), sa, rq, thr)
    assert code.all()
    tier, out = E.lookup_batch_c1c2(b[0], b[1], _dev(rq), threshold=thr)
    assert np.array_equal(tier.cpu().numpy(), code)
    _check_rows(out, rq, serve, dec1, dec2, "after update_rows")
    # the pair runs as a triple with a fresh alt-key tier: its membership starts empty, the codes stay 0 / 1 / 2 for this batch
    alt = [torch.randint(0, 3, (n,), dtype=torch.int32, device="cuda") * 100 + (t % T) + 1 for t, n in enumerate(N_ROWS)]
    c3 = E.GpuAltKeyTier(64, alt)
    rq2 = np.stack([rs.randint(0, n, 24) for n in N_ROWS], 1).astype(np.int32)
    t3, _o3 = E.lookup_batch_c1c2c3(b[0], b[1], c3, _dev(rq2), threshold=thr)
    assert int(t3.max()) <= 2 and c3.stats() is not None
    t3b, _o = E.lookup_batch_c1c2c3(b[0], b[1], c3, _dev(rq2), threshold=thr)
    n1, n2 = _dump(b[0]), _dump(b[1])
    assert not (set(n1) & set(n2)) and len(n1) == b[0].batch_stats()["size"] and len(n2) == b[1].batch_stats()["size"]


# ------------------------------------------------------------------------------------------------------ 9. file round trip
def test_file_round_trip(E, tmp_path):
    L = E._lib
    caps, thr = (64, 128), 2
    a, b, c = _pair(E, caps), _pair(E, caps), _pair(E, caps)
    k = _warm(E, a, 32, thr, 8)
    path = str(tmp_path / "pair.npz")
    E.save_state_c1c2(a[0], a[1], path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ["entries", "n_rows1", "n_rows2", "state"] and z["state"][0] == 3 and z["state"].shape == (32,)
    sa = E.export_state_c1c2(*a)
    assert E.load_state_c1c2(b[0], b[1], path) == E.load_state_c1c2(c[0], c[1], sa) and E.load_state_c1c2.__doc__
    assert _same_export(E.export_state_c1c2(*b), E.export_state_c1c2(*c)) and _same_export(E.export_state_c1c2(*b), sa)
    # a truncated file, a file without 'state', without the table sizes, a missing file
    raw = open(path, "rb").read()
    cut = str(tmp_path / "cut.npz")
    open(cut, "wb").write(raw[:len(raw) // 2])
    part = str(tmp_path / "part.npz")
    np.savez(part, entries=sa["entries"], n_rows1=sa["n_rows1"], n_rows2=sa["n_rows2"])
    rows = str(tmp_path / "rows.npz")
    np.savez(rows, entries=sa["entries"], state=sa["state"])
    d = _pair(E, caps)
    _refused(E, lambda: E.load_state_c1c2(d[0], d[1], cut), L.EVS_EIO, "readable")
    _refused(E, lambda: E.load_state_c1c2(d[0], d[1], str(tmp_path / "none.npz")), L.EVS_EIO, "readable")
    _refused(E, lambda: E.load_state_c1c2(d[0], d[1], part), L.EVS_EINVAL, "'state'")
    _refused(E, lambda: E.load_state_c1c2(d[0], d[1], rows), L.EVS_EINVAL, "n_rows")
    assert E.load_state_c1c2(d[0], d[1], path)["batch"] == k          # ... and the pair was fresh all along
