"""Warm start of the set-associative cache tier against the replay it replaces: for EvLFU, LRU and LFU in one run, on the
bench's cache shape (10 % of the Criteo-Kaggle rows, B = 16 384, Zipf 0.75), the time of
  replay   the --warmup fill batches bench.py pushes through a fresh tier before it measures (device events, batches ready)
  export   GpuCache.export_state of the filled tier (host clock around a call that ends in a synchronise)
  plan     evs_cache_load_plan over the exported entries, strict (host clock: pure host code)
  load     evs_cache_batch_load into a fresh twin -- the same plan, the upload of the packed entry list, the launch (host clock
           around the call, which returns when the load has run)
  launch   the load's kernel alone over the same record list, into set words and an arena of the tool's own (the library's
           developer entry evs_x_warm_launch), by device events
  copy     a device-to-device copy of the bytes the launch moves (placed entries x row bytes), the yardstick of the launch
and the hit rate of ten further batches on the original and on the loaded twin (the stream has set conflicts, so the flags are
not bit-equal; the rates must lie within 0.01 of each other, the band tests/test_gpu_fullsize.py holds the tier to against the
sequential oracle).  Acceptance: load (plan included) is shorter than the replay, host clock against host clock, per policy.
ONE JSON line, also written to --out.  Every tier runs the form bench.py runs: EvLFU its one-launch update, LRU / LFU the probe / consumer / insert chain.

    python tools/warm_start_bench.py [--max-rows 200000 --batch 2048] [--out profiles/warm_start.json]

--exact runs the EXACT batch-1 engine's leg instead (recorded, not gated; profiles/exact_warm_start.json): for the same tier
(10 % of the Criteo-Kaggle rows = 3 376 257 entries, fp32, d = 36) the wall time of evs_cache_exact_load -- the host checks, the
host plan and upload + launch + wait separately, and the kernel alone by device events -- against the time evs_cache_request
needs to replay, in ONE launch, the requests that put the same number of keys into the tier (n / 26 requests of new keys: the
in-kernel replay the load replaces, at its cheapest -- a workload that has to reach a warm steady state replays many more).

    python tools/warm_start_bench.py --exact [--max-rows 200000] [--out profiles/exact_warm_start.json]

--pair runs the batched C1 + C2 pair's leg (recorded; profiles/warm_start_pair.json) at the bench's mixed-precision tier shape
(Kaggle cardinalities, u8 + u4, d = 36, B = 16 384, the 48-48 split of 2 % of the rows): the replay fill bench.py runs before it
measures, the export, evs_cache_pair_load_plan (host clock), the load into a fresh pair (host clock around evs_cache_pair_load:
plan + upload + allocation + launch), the tool's own upload of the record list and allocation of records and arenas (host
clock), the load's kernel alone over that list (developer entry evs_x_warm_pair_launch, device events) -- and the steady state:
us per batch of the LOADED pair beside the replay-warmed pair it was exported from and beside a SECOND replay-warmed pair (the
A/A twin), on the same batches in the same process, chunk by chunk in rotating order.  The one comparison with a margin: the
loaded pair may be slower than its replay-warmed twin by no more than the two replay-warmed twins differ from each other.

    python tools/warm_start_bench.py --pair [--max-rows 200000 --batch 2048] [--out profiles/warm_start_pair.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import bench
import evstore_dlrm_amd as E

POLICIES = ("evlfu", "lru", "lfu")
POLICY_ID = {"evlfu": 0, "lru": 1, "lfu": 2}


def ms_since(t0):
    return round((time.perf_counter() - t0) * 1e3, 3)


def exact_leg(args):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    x_load = C.CDLL(E._lib.LIB_PATH).evs_x_exact_load_timed   # evs_cache_exact_load's three steps with a clock between them
    x_load.restype, x_load.argtypes = C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    ln = [min(n, args.max_rows) if args.max_rows else n for n in bench.KAGGLE_LN]
    T, d = len(ln), args.dim
    cap = int(args.frac * sum(ln))
    ev = bench.make_tables(ln, d, seed=0, device=dev)
    rs = np.random.RandomState(5)
    # a state of `cap` distinct keys, every table holding its share (small tables whole), EvLFU buckets drawn and sorted
    share = np.minimum(np.asarray(ln, np.int64), np.maximum(1, (np.asarray(ln, np.float64) / sum(ln) * cap).astype(np.int64)))
    while share.sum() < cap:
        room = np.asarray(ln, np.int64) - share
        k = int(np.argmax(room))
        share[k] += min(int(room[k]), cap - int(share.sum()))
    keys = np.concatenate([np.stack([np.full(int(m), k + 1, np.int64), rs.permutation(ln[k])[:int(m)].astype(np.int64)], 1) for k, m in enumerate(share)])
    keys = keys[rs.permutation(len(keys))][:cap]
    n = len(keys)
    entries = np.ascontiguousarray(np.concatenate([np.sort(rs.randint(0, T + 1, size=n)).astype(np.int64)[:, None], keys], 1))
    n_req = (n + T - 1) // T
    # the replay: n / T requests, request j asks table k for a row it has not asked for before (small tables wrap around)
    reqs = torch.from_numpy(np.stack([(np.arange(n_req, dtype=np.int64) * 7919 + 13 * k) % ln[k] for k in range(T)], 1).astype(np.int32)).to(dev)
    out = torch.empty((n_req, T, d), dtype=torch.float32, device=dev)
    hit = torch.empty((n_req, T), dtype=torch.uint8, device=dev)

    def fresh():
        c = E.GpuCache("evlfu", cap, T, d, 32, "python", dev)
        c.set_backing(ev)
        return c

    w = fresh()                                   # every kernel has run once before anything is timed
    w.load_exact_state({"entries": entries[:1000], "state": None}, strict=False)
    w.request(reqs[:8].contiguous(), out=out[:8], hit=hit[:8])
    del w
    torch.cuda.synchronize()
    r = {"load_ms": [], "check_ms": [], "plan_ms": [], "upload_launch_wait_ms": [], "kernel_ms": [], "replay_ms": [], "replay_wall_ms": []}
    for rnd in range(args.rounds):
        c = fresh()
        torch.cuda.synchronize()
        t4 = (C.c_double * 4)()
        t0 = time.perf_counter()
        E._lib.check(x_load(c._h, n, entries.ctypes.data, None, 0, torch.cuda.current_stream(dev).cuda_stream, t4))
        r["load_ms"].append(ms_since(t0))
        for k, name in enumerate(("check_ms", "plan_ms", "upload_launch_wait_ms", "kernel_ms")):
            r[name].append(round(float(t4[k]), 3))
        if rnd == 0:   # what was loaded is what comes back, in order, and it is served from the arena
            assert np.array_equal(c.dump(), entries)
            probe = np.zeros((64, T), np.int32)
            for k in range(T):
                mine = entries[entries[:, 1] == k + 1][:, 2]
                probe[:, k] = mine[np.arange(64) % len(mine)]
            h, o = c.request(torch.from_numpy(probe).to(dev))
            assert bool(h.all()) and all(torch.equal(o[:, k], ev.raw[k].view(torch.float32).view(-1, d)[torch.from_numpy(probe[:, k]).to(dev).long()]) for k in range(T))
        del c
        c = fresh()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        c.request(reqs, out=out, hit=hit)
        e1.record()
        torch.cuda.synchronize()
        r["replay_wall_ms"].append(ms_since(t0))
        r["replay_ms"].append(round(e0.elapsed_time(e1), 3))
        r["replay_entries"] = c.stats()["size"]
        del c
    r["replay_us_per_request"] = round(min(r["replay_ms"]) * 1e3 / n_req, 3)
    r["replay_ms_n_requests_extrapolated"] = round(r["replay_us_per_request"] * n / 1e3, 1)
    r["replay_over_load"] = round(min(r["replay_wall_ms"]) / min(r["load_ms"]), 2)
    line = json.dumps({"tool": "warm_start_bench --exact",
                       "shape": {"rows": int(sum(ln)), "capacity": cap, "entries": n, "frac": args.frac, "dim": d, "codec": 32, "policy": "evlfu",
                                 "replay_requests": n_req, "rounds": args.rounds},
                       "what": {"load_ms": "host clock around the load (evs_cache_exact_load's steps: checks + plan + upload + one launch + wait)",
                                "check_ms": "evs_exact_load_check inside it (host)", "plan_ms": "records, list heads, run list (host)",
                                "upload_launch_wait_ms": "record upload, state copy, the launch, the synchronise (host clock)",
                                "kernel_ms": "the load kernel alone, device events",
                                "replay_ms": "evs_cache_request over replay_requests requests of new keys in ONE launch, device events",
                                "replay_wall_ms": "host clock around it, ending in a synchronise",
                                "replay_entries": "keys resident after the replay (small tables wrap around, so fewer than entries)",
                                "replay_ms_n_requests_extrapolated": "replay_us_per_request x entries: what as many REQUESTS as the tier has entries would take (not run)",
                                "replay_over_load": "min replay_wall_ms / min load_ms (recorded, not gated)"},
                       "exact": r})
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


def pair_leg(args):
    from evstore_dlrm_amd import gpu_cache
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    lib = E._lib.lib()
    x_launch = C.CDLL(E._lib.LIB_PATH).evs_x_warm_pair_launch
    x_launch.restype = C.c_int
    x_launch.argtypes = [C.c_void_p, C.c_longlong, C.c_longlong, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ln = [min(n, args.max_rows) if args.max_rows else n for n in bench.KAGGLE_LN]
    T, d, B = len(ln), args.dim, args.batch
    fill, steps, chunks = args.pair_fill, args.pair_steps, args.pair_chunks
    ev = bench.make_tables(ln, d, seed=0, device=dev)
    ev8, ev4 = ev.encode(8), ev.encode(4)
    del ev
    budget = int(0.02 * sum(ln))
    caps = (int(0.48 * budget) * 4, int(0.48 * budget) * 8)
    row_bytes = (d, d // 2)
    rq = [b[1].t().contiguous().to(torch.int32) for b in
          bench.make_batches(ln, B, fill + steps * chunks, seed=21, device=dev, dist="zipf", alpha=args.alpha)]
    x = torch.rand((B, d), device=dev)
    tier = torch.empty((B, T), dtype=torch.uint8, device=dev)
    n_rows = np.asarray(ln, np.int64)
    table_ptr = (np.array([t.data_ptr() for t in ev8.raw], np.uint64), np.array([t.data_ptr() for t in ev4.raw], np.uint64))

    def fresh():
        c1, c2 = E.GpuCache("evlfu", caps[0], T, d, 8, "cpp", dev), E.GpuCache("evlfu", caps[1], T, d, 4, "cpp", dev)
        c1.set_backing(ev8)
        c2.set_backing(ev4)
        return c1, c2

    def run(pair, lo, hi):
        for r in rq[lo:hi]:
            gpu_cache.lookup_interact_c1c2(pair[0], pair[1], r, x, tier=tier)

    def timed(pair, lo, hi):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        run(pair, lo, hi)
        e1.record()
        torch.cuda.synchronize()
        return ms_since(t0), e0.elapsed_time(e1)

    w = fresh()                                   # every kernel has run once before anything is timed
    run(w, 0, 2)
    w2 = fresh()
    gpu_cache.load_state_c1c2(w2[0], w2[1], gpu_cache.export_state_c1c2(*w))
    run(w2, 2, 3)
    del w, w2
    torch.cuda.synchronize()

    r = {}
    a, a2 = fresh(), fresh()
    r["replay_wall_ms"], r["replay_ms"] = [round(v, 3) for v in timed(a, 0, fill)]
    r["replay_twin_wall_ms"], r["replay_twin_ms"] = [round(v, 3) for v in timed(a2, 0, fill)]
    t0 = time.perf_counter()
    s = gpu_cache.export_state_c1c2(*a)
    r["export_ms"] = ms_since(t0)
    n = len(s["entries"])
    n1 = int((s["entries"][:, 0] == 1).sum())
    dest, words, out8 = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.uint32), np.zeros(8, np.int64)
    t0 = time.perf_counter()
    E._lib.check(lib.evs_cache_pair_load_plan(caps[0], caps[1], T, n_rows.ctypes.data, n_rows.ctypes.data, n, s["entries"].ctypes.data,
                                              s["state"].ctypes.data, 1, dest.ctypes.data, words.ctypes.data, out8.ctypes.data))
    r["plan_ms"] = ms_since(t0)
    r["load_ms"] = []
    loaded = None
    for rnd in range(args.rounds):
        w = fresh()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        info = gpu_cache.load_state_c1c2(w[0], w[1], s)
        r["load_ms"].append(ms_since(t0))
        assert info["placed"] == (n1, n - n1) and info["turned_away"] == (0, 0) and info["batch"] == fill
        if loaded is None:
            loaded = w
    # the launch alone: the record list the load builds, set records and arenas of the tool's own
    st = s["state"]
    geo = np.array([st[4 + 2], 0, 0, row_bytes[0], st[16 + 2], (st[4 + 2] + 3) // 4 * 4, int(st[16 + 3]).bit_length() - 1, row_bytes[1]], np.int32)
    slots = np.array([caps[0], caps[1]], np.int64)
    e = s["entries"]
    recs = np.zeros(n, np.dtype([("src", "<u8"), ("slot", "<u4"), ("word", "<u4")]))
    for k in (0, 1):
        m = e[:, 0] == k + 1
        recs["src"][m] = table_ptr[k][e[m, 1] - 1] + e[m, 2].astype(np.uint64) * np.uint64(row_bytes[k])
    recs["slot"], recs["word"] = dest[:n], words[:n]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    recs_dev = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev)
    tags = torch.zeros(int(st[3]) * 32, dtype=torch.int32, device=dev)
    arenas = [torch.empty(caps[k] * row_bytes[k], dtype=torch.uint8, device=dev) for k in (0, 1)]
    torch.cuda.synchronize()
    r["upload_alloc_ms"] = ms_since(t0)
    nbytes = n1 * row_bytes[0] + (n - n1) * row_bytes[1]
    src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for rep_ in range(4):          # (the first one warms the buffers' pages; a copy in front of each pushes the rows out of the caches)
        dst.copy_(src)
        torch.cuda.synchronize()
        e0.record()
        assert x_launch(recs_dev.data_ptr(), n1, n - n1, tags.data_ptr(), arenas[0].data_ptr(), arenas[1].data_ptr(), geo.ctypes.data,
                        slots.ctypes.data, torch.cuda.current_stream(dev).cuda_stream) == 0
        e1.record()
        torch.cuda.synchronize()
        if rep_:
            best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
    r["load_launch_ms"] = round(best, 4)
    assert int((tags != 0).sum()) == n, "the launch did not store every way word"
    dst.copy_(src)
    torch.cuda.synchronize()
    e0.record()
    dst.copy_(src)
    e1.record()
    torch.cuda.synchronize()
    r["copy_ms"] = round(e0.elapsed_time(e1), 4)
    del recs_dev, tags, arenas, src, dst
    r.update(entries_c1=n1, entries_c2=n - n1, bytes_moved=nbytes)
    # steady state: the loaded pair, its replay-warmed twin and the second replay-warmed pair on the same batches, chunk by chunk
    pairs = {"twin": a, "twin_aa": a2, "loaded": loaded}
    us = {k: [] for k in pairs}
    names = list(pairs)
    for c in range(chunks):
        lo = fill + c * steps
        for k in names[c % 3:] + names[:c % 3]:
            us[k].append(round(timed(pairs[k], lo, lo + steps)[1] * 1e3 / steps, 3))
    med = {k: float(np.median(v)) for k, v in us.items()}
    spread = abs(med["twin_aa"] - med["twin"])
    hits = {k: sum(c.batch_stats()["n_hits"] for c in p) for k, p in pairs.items()}
    r.update(us_per_batch=us, loaded_us_per_batch=round(med["loaded"], 3), twin_us_per_batch=round(med["twin"], 3),
             twin_aa_us_per_batch=round(med["twin_aa"], 3), aa_spread_us=round(spread, 3),
             loaded_minus_twin_us=round(med["loaded"] - med["twin"], 3), n_hits=hits,
             loaded_within_aa_spread=bool(med["loaded"] - med["twin"] <= spread),
             load_shorter_than_replay=bool(min(r["load_ms"]) < r["replay_wall_ms"]))
    line = json.dumps({"tool": "warm_start_bench --pair",
                       "shape": {"rows": int(sum(ln)), "capacities": caps, "batch": B, "dim": d, "codecs": [8, 4], "zipf_alpha": args.alpha,
                                 "replay_batches": fill, "steady_chunks": chunks, "batches_per_chunk": steps, "rounds": args.rounds},
                       "what": {"replay_ms": "device events around the fill batches (lookup_interact_c1c2)", "replay_wall_ms": "host clock around them, ending in a synchronise",
                                "export_ms": "host clock around export_state_c1c2", "plan_ms": "evs_cache_pair_load_plan, strict (host clock: pure host code)",
                                "load_ms": "host clock around load_state_c1c2 into a fresh pair: plan + upload + allocation + launch, per round",
                                "upload_alloc_ms": "host clock around the tool's own upload of the record list and allocation of records and arenas",
                                "load_launch_ms": "device events around the load's kernel alone (evs_x_warm_pair_launch, best of 3)",
                                "copy_ms": "device-to-device copy of bytes_moved",
                                "loaded_us_per_batch / twin_us_per_batch / twin_aa_us_per_batch": "median over the chunks of device-event time per batch",
                                "aa_spread_us": "|twin_aa - twin|: what two replay-warmed pairs differ by in this run",
                                "loaded_within_aa_spread": "loaded - twin <= aa_spread_us (the verdict); load_shorter_than_replay is recorded, not gated"},
                       "pair": r, "accepted": r["loaded_within_aa_spread"]})
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pair", action="store_true", help="the batched C1 + C2 pair's leg (evs_cache_pair_load against the replay fill; steady state beside replay-warmed twins)")
    ap.add_argument("--pair-fill", type=int, default=180, help="--pair: fill batches (bench.py's mixed-tier fill)")
    ap.add_argument("--pair-steps", type=int, default=20, help="--pair: batches per steady-state chunk")
    ap.add_argument("--pair-chunks", type=int, default=9, help="--pair: steady-state chunks per pair")
    ap.add_argument("--exact", action="store_true", help="the exact batch-1 engine's leg (evs_cache_exact_load against the in-kernel replay)")
    ap.add_argument("--frac", type=float, default=0.10)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--warmup", type=int, default=60, help="fill batches: bench.py's replay")
    ap.add_argument("--cmp", type=int, default=10, help="further batches on which the two hit rates are taken")
    ap.add_argument("--rounds", type=int, default=3, help="loads per policy, each into a fresh twin")
    ap.add_argument("--max-rows", type=int, default=0, help="clamp every table to this many rows (0: full size)")
    ap.add_argument("--dim", type=int, default=36)
    ap.add_argument("--out", default=None, help="default: profiles/warm_start.json (--exact: profiles/exact_warm_start.json)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "exact_warm_start.json" if args.exact else "warm_start_pair.json" if args.pair else "warm_start.json")
    assert torch.cuda.is_available(), "warm_start_bench measures on the GPU"
    if args.exact:
        return exact_leg(args)
    if args.pair:
        return pair_leg(args)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    lib = E._lib.lib()
    x_launch = C.CDLL(E._lib.LIB_PATH).evs_x_warm_launch
    x_launch.restype, x_launch.argtypes = C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_void_p]
    ln = [min(n, args.max_rows) if args.max_rows else n for n in bench.KAGGLE_LN]
    T, d, B = len(ln), args.dim, args.batch
    cap = int(args.frac * sum(ln))
    ev = bench.make_tables(ln, d, seed=0, device=dev)
    rows = [b[1].t().contiguous().to(torch.int32) for b in
            bench.make_batches(ln, B, args.warmup + args.cmp, seed=3, device=dev, dist="zipf", alpha=args.alpha)]
    x = torch.rand((B, d), device=dev)
    F = T + 1
    out = torch.empty((B, d + F * (F - 1) // 2), device=dev)
    hit = torch.empty((B, T), dtype=torch.uint8, device=dev)
    n_rows = np.asarray(ln, np.int64)
    table_ptr = np.array([ev.raw[k].data_ptr() for k in range(T)], np.uint64)

    def fresh(policy):
        c = E.GpuCache(policy, cap, T, d, 32, "python", dev)
        c.set_backing(ev)
        return c

    def replay(c, lo, hi):
        for i in range(lo, hi):
            c.lookup_interact(rows[i], x, out=out, hit=hit)

    # every kernel of the three chains has run once before anything is timed
    for p in POLICIES:
        c = fresh(p)
        replay(c, 0, 2)
        w = fresh(p)
        w.load_state(c.export_state())
        del c, w
    torch.cuda.synchronize()

    res, ok = {}, True
    for p in POLICIES:
        r = {"replay_ms": [], "replay_wall_ms": [], "export_ms": [], "plan_ms": [], "load_ms": [], "load_launch_ms": [], "copy_ms": []}
        state = orig = None
        for rnd in range(args.rounds):
            c = fresh(p)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            replay(c, 0, args.warmup)
            e1.record()
            torch.cuda.synchronize()
            r["replay_wall_ms"].append(ms_since(t0))
            r["replay_ms"].append(round(e0.elapsed_time(e1), 3))
            t0 = time.perf_counter()
            s = c.export_state()
            r["export_ms"].append(ms_since(t0))
            n = len(s["entries"])
            dest, words, out4 = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.uint32), np.zeros(4, np.int64)
            t0 = time.perf_counter()
            E._lib.check(lib.evs_cache_load_plan(POLICY_ID[p], cap, T, n_rows.ctypes.data, n, s["entries"].ctypes.data, s["state"].ctypes.data,
                                                 1, dest.ctypes.data, words.ctypes.data, out4.ctypes.data))
            r["plan_ms"].append(ms_since(t0))
            w = fresh(p)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = w.load_state(s)
            r["load_ms"].append(ms_since(t0))
            assert info["placed"] == n and info["turned_away"] == 0
            # the launch alone: the record list the load builds (row address, slot, word), buffers of the tool's own
            recs = np.zeros(n, np.dtype([("src", "<u8"), ("slot", "<u4"), ("word", "<u4")]))
            recs["src"] = table_ptr[s["entries"][:, 0] - 1] + s["entries"][:, 1].astype(np.uint64) * np.uint64(d * 4)
            recs["slot"], recs["word"] = dest[:n], words[:n]
            recs_dev = torch.from_numpy(recs.view(np.uint8).reshape(-1)).to(dev)
            n_slots = cap // 8 * 8
            tags, arena = torch.zeros(n_slots, dtype=torch.int32, device=dev), torch.empty(2 * n_slots * d * 4, dtype=torch.uint8, device=dev)
            st_ = torch.cuda.current_stream(dev).cuda_stream
            best = None
            nbytes = n * d * 4
            src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
            for rep_ in range(4):          # (the first one warms the buffers' pages; a copy in front of each pushes the rows out of the caches)
                dst.copy_(src)
                torch.cuda.synchronize()
                e0.record()
                assert x_launch(recs_dev.data_ptr(), n, tags.data_ptr(), arena.data_ptr(), 1, d * 4, st_) == 0
                e1.record()
                torch.cuda.synchronize()
                if rep_:
                    best = e0.elapsed_time(e1) if best is None else min(best, e0.elapsed_time(e1))
            r["load_launch_ms"].append(round(best, 4))
            assert torch.equal(tags.view(torch.int32)[torch.from_numpy(dest[:n]).to(dev)], torch.from_numpy(words[:n].view(np.int32)).to(dev))
            del recs_dev, tags, arena
            dst.copy_(src)
            torch.cuda.synchronize()
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            r["copy_ms"].append(round(e0.elapsed_time(e1), 4))
            del src, dst
            if rnd == 0:
                state, orig, twin = s, c, w
            else:
                del c, w
        # ten further batches on the original and on the restored twin
        rates = []
        for c in (orig, twin):
            s0 = c.batch_stats()
            replay(c, args.warmup, args.warmup + args.cmp)
            s1 = c.batch_stats()
            rates.append((s1["n_hits"] - s0["n_hits"]) / float(T * B * args.cmp))
        n = len(state["entries"])
        r.update(entries=n, bytes_moved=n * d * 4, hit_rate_original=round(rates[0], 5), hit_rate_restored=round(rates[1], 5),
                 hit_rate_gap=round(abs(rates[0] - rates[1]), 5))
        r["launch_rate_of_copy"] = round(min(r["copy_ms"]) / min(r["load_launch_ms"]), 3)
        r["load_shorter_than_replay"] = bool(min(r["load_ms"]) < min(r["replay_wall_ms"]))
        r["hit_rates_within_0.01"] = bool(r["hit_rate_gap"] <= 0.01)
        ok = ok and r["load_shorter_than_replay"] and r["hit_rates_within_0.01"]
        res[p] = r
        print("warm_start_bench: %s replay %.2f ms, export %.1f, plan %.1f, load %.1f (launch %.3f, copy %.3f), hit rate %.4f / %.4f"
              % (p, min(r["replay_ms"]), min(r["export_ms"]), min(r["plan_ms"]), min(r["load_ms"]), min(r["load_launch_ms"]), min(r["copy_ms"]),
                 rates[0], rates[1]), file=sys.stderr, flush=True)
        del orig, twin, state
    line = json.dumps({"tool": "warm_start_bench",
                       "shape": {"rows": int(sum(ln)), "capacity": cap, "frac": args.frac, "batch": B, "dim": d, "codec": 32, "zipf_alpha": args.alpha,
                                 "replay_batches": args.warmup, "hit_rate_batches": args.cmp, "rounds": args.rounds},
                       "what": {"replay_ms": "device events around the fill batches", "replay_wall_ms": "host clock around them, ending in a synchronise",
                                "load_ms": "host clock around evs_cache_batch_load: plan + upload + launch",
                                "load_launch_ms": "device events around the load's kernel alone (evs_x_warm_launch, best of 3)",
                                "copy_ms": "device-to-device copy of bytes_moved", "launch_rate_of_copy": "copy_ms / load_launch_ms, best of each",
                                "load_shorter_than_replay": "min load_ms < min replay_wall_ms: host clock against host clock"},
                       "policies": res, "accepted": ok})
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
