#!/usr/bin/env python3
"""The set-associative cache tier over caller-fed rows (GpuCache.set_fed_backing; lookup_begin / lookup_finish_interact) beside the
fetch-first chain it is cut from, as ONE JSON file.

Shape (tools/policy_compare.py's): the Criteo-Kaggle cardinalities, fp32, d = 36, a 10 % EvLFU tier, B = 16 384, rows Zipf(0.75),
the interaction as the consumer.  Every configuration is warmed until its size stops growing; then --steps batches are timed, the
configurations alternating on the SAME batches in one process:
    a  fetch-first over HBM tables                      -- the yardstick
    b  fetch-first over pinned host tables
    c  fed, a DEVICE source: one index_select from the HBM tables (what a GPU-side store would do)
    d  fed, a HOST source: a numpy gather and one host-to-device copy (what a file, a key-value store or a remote server would do)
A begin synchronises, so every call is timed by the host clock between two synchronises (a and b too: `wall_us`); a and b are
also timed by a pair of device events as everywhere else (`median_us`).  c and d are split into begin (flush, probe, list launch,
the synchronise and the 4-byte copy of the count), source and finish (update, re-point, consumer), and report the keys listed
and the positions served straight from the fed block per batch.  `begin_over_a_us` is what the seam costs over the yardstick
before a single row is fetched: c's begin + finish against a's call.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import evstore_dlrm_amd as E  # noqa: E402
from tools.host_setassoc_bench import pinned_tables  # noqa: E402

NAMES = ("a_fetch_first_hbm", "b_fetch_first_pinned", "c_fed_device_source", "d_fed_host_source")
BAG_NAMES = ("a_bags_count_first_fetch_first_hbm", "b_fed_bags_device_source", "c_fed_bags_host_source")


def main_bags(args):
    """--bags: the bag form (lookup_bags_begin / lookup_bags_finish_interact) beside the order-1 count-first bag chain it is cut from
    -> profiles/fed_bags.json.  tools/bags_cache_bench.py's ragged stream (bags of 1 .. --max-bag indices, rows Zipf) at this tool's
    shape; a: lookup_bags_interact over HBM tables, the yardstick; b: fed, a device index_select source; c: fed, a host source.
    Timed as above: the host clock between two synchronises, b and c split into begin / source / finish."""
    from tools.bags_cache_bench import make_batch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    d, B = args.dim, args.batch
    ln, ev, pinned, scale = pinned_tables(bench.KAGGLE_LN, d, args.scale, dev)
    T = len(ln)
    cap = int(args.frac * sum(ln))
    rb = d * 4
    base_np = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    base_dev = torch.from_numpy(base_np).to(dev)
    all_dev = torch.cat([ev.fp32_view(k) for k in range(T)])
    all_host = np.concatenate([p.numpy() for p in pinned])

    def device_source(keys):
        return all_dev.index_select(0, base_dev[(keys >> 32) - 1] + (keys & 0xffffffff))

    def host_source(keys):
        k = keys.cpu().numpy()
        return torch.from_numpy(all_host[base_np[(k >> 32) - 1] + (k & 0xffffffff)]).to(dev)

    sources = {"b_fed_bags_device_source": device_source, "c_fed_bags_host_source": host_source}
    x = torch.rand((B, d), device=dev)
    F = T + 1
    out = torch.empty((B, d + F * (F - 1) // 2), device=dev)

    def call(name, c, lo, li, split=None):
        if name in sources:
            t0 = time.perf_counter()
            _, keys = c.lookup_bags_begin(lo, li)           # (synchronises)
            t1 = time.perf_counter()
            fed = sources[name](keys) if keys.numel() else None
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            c.lookup_bags_finish_interact(fed, x, out=out)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if split is not None:
                split.append((t1 - t0, t2 - t1, t3 - t2, int(keys.numel())))
        else:
            c.lookup_bags_interact(lo, li, x, out=out)

    caches, warm = {}, {}
    for name in BAG_NAMES:
        c = E.GpuCache("evlfu", cap, T, d, 32, "python", dev).set_miss_order("fetch-first")
        c.set_bag_rule("served-bags").set_bag_count("count-first")
        if name in sources:
            c.set_fed_backing([None] * T, ln)
        else:
            c.set_backing(ev)
        g = torch.Generator(device=dev).manual_seed(7)       # (every configuration warms on the same batches)
        size = -1
        for i in range(args.max_warm):
            call(name, c, *make_batch(ln, B, g, dev, args.max_bag, args.alpha))
            if i % 10 == 9:
                s = c.batch_stats()["size"]
                if s - size < 0.002 * cap:
                    break
                size = s
        caches[name], warm[name] = c, i + 1
        print("fed_backing_bench: %s warm after %d batches, size %d of %d" % (name, i + 1, c.batch_stats()["size"], cap), file=sys.stderr, flush=True)
    g = torch.Generator(device=dev).manual_seed(11)
    timed = [make_batch(ln, B, g, dev, args.max_bag, args.alpha) for _ in range(args.steps)]
    n_pos = sum(int(t.numel()) for _, li in timed for t in li)
    s0 = {n: (caches[n].batch_stats(), caches[n].fetch_stats(), caches[n].fed_stats()) for n in BAG_NAMES}
    events, wall, split = {n: [] for n in BAG_NAMES}, {n: [] for n in BAG_NAMES}, {n: [] for n in sources}
    for lo, li in timed:
        for n in BAG_NAMES:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            call(n, caches[n], lo, li, split.get(n))
            e1.record()
            torch.cuda.synchronize()
            wall[n].append(time.perf_counter() - t0)
            events[n].append((e0, e1))
    res = {}
    for n in BAG_NAMES:
        s1, f1, fs1 = caches[n].batch_stats(), caches[n].fetch_stats(), caches[n].fed_stats()
        w = np.array(wall[n]) * 1e6
        res[n] = {"wall_us": round(float(np.median(w)), 2), "wall_p95_us": round(float(np.percentile(w, 95)), 2),
                  "hit_rate": round((s1["n_hits"] - s0[n][0]["n_hits"]) / n_pos, 4), "size": s1["size"], "warm_batches": warm[n],
                  "flushes": s1["n_flush"] - s0[n][0]["n_flush"], "fetch_stats_delta": {k: f1[k] - s0[n][1][k] for k in f1}}
        if n in sources:
            sp = np.array(split[n], np.float64)
            res[n].update({"begin_us": round(float(np.median(sp[:, 0])) * 1e6, 2), "source_us": round(float(np.median(sp[:, 1])) * 1e6, 2),
                           "finish_us": round(float(np.median(sp[:, 2])) * 1e6, 2), "keys_per_batch": round(float(sp[:, 3].mean()), 1),
                           "fed_bytes_per_batch": round(float(sp[:, 3].mean()) * rb),
                           "fed_stats_delta": {k: fs1[k] - s0[n][2][k] for k in fs1}})
        else:
            us = np.array([a.elapsed_time(b) * 1e3 for a, b in events[n]])
            res[n].update({"median_us": round(float(np.median(us)), 2), "p95_us": round(float(np.percentile(us, 95)), 2)})
        print("fed_backing_bench: %s %s" % (n, res[n]), file=sys.stderr, flush=True)
    a = res[BAG_NAMES[0]]["wall_us"]
    b_ = res[BAG_NAMES[1]]
    doc = {"tool": "fed_backing_bench --bags", "device": torch.cuda.get_device_name(0),
           "shape": {"rows": sum(ln), "table_scale": scale, "capacity": cap, "frac": args.frac, "batch": B, "dim": d, "row_bytes": rb,
                     "zipf_alpha": args.alpha, "bags": "1 .. %d" % args.max_bag, "lookups_per_call": round(n_pos / len(timed), 1),
                     "timed_batches": len(timed), "policy": "evlfu (served bags, count first)",
                     "consumer": "lookup_bags_interact / lookup_bags_finish_interact (pooling, then the dense interaction)"},
           "chains": {"a": "bags_probe -> bags_count -> bags_raise_list -> cache_batch_sa_list -> sa_repoint (flat) -> bags_pool -> dense interaction",
                      "b, c": "begin: bags_fed_probe -> bags_count -> bags_fed_list -> fed_list -> synchronise | source | finish: fold -> bags_fed_hits -> "
                              "cache_batch_sa_list_fed -> bags_repoint_fed -> bags_pool -> dense interaction"},
           "timing": "host clock between two synchronises around every call (wall_us; begin / source / finish each end on a synchronise); a also by a "
                     "pair of device events (median_us); the configurations alternate on the same batches in one process; one run on one box",
           "configs": res,
           "begin_plus_finish_over_a_us": round(b_["begin_us"] + b_["finish_us"] - a, 2),
           "b_over_a": round(b_["wall_us"] / a, 3), "c_over_a": round(res[BAG_NAMES[2]]["wall_us"] / a, 3)}
    path = args.out or os.path.join(ROOT, "profiles", "fed_bags.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"tool": doc["tool"], "a_wall_us": a, "b_over_a": doc["b_over_a"], "c_over_a": doc["c_over_a"],
                      "begin_plus_finish_over_a_us": doc["begin_plus_finish_over_a_us"], "out": path}))


PAIR_NAMES = ("a_pair_fetch_first_hbm", "b_pair_fetch_first_pinned", "c_fed_pair_device_source")


def main_pair(args):
    """--pair: the fed C1 + C2 pair (lookup_begin_c1c2 / lookup_finish_interact_c1c2) beside the fetch-first pair it is cut from ->
    profiles/fed_pair_bench.json.  tools/c2_pair_bench.py's Kaggle pair geometry (a u8 C1 and a u4 C2, 2 % of the rows between
    them, d = 36, B = 16 384) and one Zipf(0.75) stream: --fill batches fill every pair, then --steps batches are timed, the pairs
    alternating on the same batches in one process.  a: the fetch-first pair over HBM tables, b: over pinned tables, c: the fed
    pair with a device-resident gather source per tier (one index_select each), split into begin / sources / finish, each ended
    by a synchronise.  Times are the host clock between two synchronises (wall_us); a and b also by device events (median_us)."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ln, d, B = bench.KAGGLE_LN, 36, args.batch
    T = len(ln)
    ev = bench.make_tables(ln, d)
    ev8, ev4 = ev.encode(8), ev.encode(4)
    del ev
    pin8, pin4 = [t.cpu().pin_memory() for t in ev8.raw], [t.cpu().pin_memory() for t in ev4.raw]
    budget = int(0.02 * sum(ln))
    caps = (int(0.48 * budget) * 4, int(0.48 * budget) * 8)
    base_dev = torch.from_numpy(np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)).to(dev)
    all8, all4 = torch.cat([t.reshape(t.shape[0], -1) for t in ev8.raw]), torch.cat([t.reshape(t.shape[0], -1) for t in ev4.raw])

    def gather(table, keys):
        return table.index_select(0, base_dev[(keys >> 32) - 1] + (keys & 0xffffffff)) if keys.numel() else None

    tier = torch.empty((B, T), dtype=torch.uint8, device=dev)
    x = torch.rand((B, d), device=dev)
    F = T + 1
    out = torch.empty((B, d + F * (F - 1) // 2), device=dev)
    rq = [b[1].t().contiguous().to(torch.int32) for b in bench.make_batches(ln, B, args.fill + args.steps, seed=21, device=dev, dist="zipf", alpha=args.alpha)]

    def call(name, pair, r, split=None):
        c1, c2 = pair
        if name.startswith("c_"):
            t0 = time.perf_counter()
            _, k1, k2 = E.lookup_begin_c1c2(c1, c2, r, tier=tier)       # (synchronises)
            t1 = time.perf_counter()
            f1, f2 = gather(all8, k1), gather(all4, k2)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            E.lookup_finish_interact_c1c2(c1, c2, f1, f2, x, out=out)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if split is not None:
                split.append((t1 - t0, t2 - t1, t3 - t2, int(k1.numel()), int(k2.numel())))
        else:
            E.lookup_interact_c1c2(c1, c2, r, x, tier=tier, fused=True)

    pairs = {}
    for name in PAIR_NAMES:
        c1, c2 = E.GpuCache("evlfu", caps[0], T, d, 8, "cpp", dev), E.GpuCache("evlfu", caps[1], T, d, 4, "cpp", dev)
        for c, hbm, pin in ((c1, ev8, pin8), (c2, ev4, pin4)):
            c.set_miss_order("fetch-first")
            if name.startswith("c_"):
                c.set_fed_backing([None] * T, ln)
            else:
                c.set_backing(pin if name.startswith("b_") else hbm)
        for r in rq[:args.fill]:
            call(name, (c1, c2), r)
        pairs[name] = (c1, c2)
        print("fed_backing_bench: %s filled, C1 %d C2 %d resident" % (name, c1.batch_stats()["size"], c2.batch_stats()["size"]), file=sys.stderr, flush=True)
    timed = rq[args.fill:]
    s0 = {n: (p[0].batch_stats(), p[1].batch_stats(), p[0].fetch_stats()) for n, p in pairs.items()}
    fs0 = E.fed_stats_c1c2(*pairs[PAIR_NAMES[2]])
    events, wall, split = {n: [] for n in PAIR_NAMES}, {n: [] for n in PAIR_NAMES}, []
    for r in timed:
        for n in PAIR_NAMES:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            call(n, pairs[n], r, split if n.startswith("c_") else None)
            e1.record()
            torch.cuda.synchronize()
            wall[n].append(time.perf_counter() - t0)
            events[n].append((e0, e1))
    res = {}
    for n, (c1, c2) in pairs.items():
        s1 = (c1.batch_stats(), c2.batch_stats(), c1.fetch_stats())
        w = np.array(wall[n]) * 1e6
        res[n] = {"wall_us": round(float(np.median(w)), 2), "wall_p95_us": round(float(np.percentile(w, 95)), 2),
                  "hit_rate": round(sum(s1[k]["n_hits"] - s0[n][k]["n_hits"] for k in (0, 1)) / (T * B * len(timed)), 4),
                  "size": (s1[0]["size"], s1[1]["size"]),
                  "repoint_per_batch": {k: round((s1[2][k] - s0[n][2].get(k, 0)) / len(timed), 2) for k in s1[2] if k != "calls"}}
        if n.startswith("c_"):
            sp = np.array(split, np.float64)
            fs1 = E.fed_stats_c1c2(c1, c2)
            res[n].update({"begin_us": round(float(np.median(sp[:, 0])) * 1e6, 2), "sources_us": round(float(np.median(sp[:, 1])) * 1e6, 2),
                           "finish_us": round(float(np.median(sp[:, 2])) * 1e6, 2),
                           "keys_per_batch": (round(float(sp[:, 3].mean()), 1), round(float(sp[:, 4].mean()), 1)),
                           "fed_bytes_per_batch": round(float(sp[:, 3].mean()) * d + float(sp[:, 4].mean()) * d / 2),
                           "fed_stats_delta": {k: fs1[k] - fs0[k] for k in fs1}})
        else:
            us = np.array([a.elapsed_time(b) * 1e3 for a, b in events[n]])
            res[n].update({"median_us": round(float(np.median(us)), 2), "p95_us": round(float(np.percentile(us, 95)), 2)})
        print("fed_backing_bench: %s %s" % (n, res[n]), file=sys.stderr, flush=True)
    a, b_, c_ = (res[n] for n in PAIR_NAMES)
    doc = {"tool": "fed_backing_bench --pair", "device": torch.cuda.get_device_name(0),
           "shape": {"rows": sum(ln), "capacities": caps, "codecs": (8, 4), "batch": B, "dim": d, "zipf_alpha": args.alpha, "fill_batches": args.fill,
                     "timed_batches": len(timed), "consumer": "lookup_interact_c1c2 / lookup_finish_interact_c1c2"},
           "chains": {"a, b": "cache_batch_probe2 -> cache_batch_sa_list2 -> sa_repoint2 -> interaction",
                      "c": "begin: cache_batch_probe2<fed> -> fed_list x 2 -> synchronise | sources | finish: fold x 2 -> pair_fed_hits -> "
                           "cache_batch_sa_list_fed_spill x 2 -> sa_repoint2_fed -> interaction"},
           "timing": "host clock between two synchronises around every call (wall_us; begin / sources / finish each end on a synchronise); a and b also "
                     "by a pair of device events (median_us); the pairs alternate on the same batches in one process; one run on one box",
           "configs": res,
           "begin_plus_finish_over_a_us": round(c_["begin_us"] + c_["finish_us"] - a["wall_us"], 2),
           "begin_plus_finish_over_a": round((c_["begin_us"] + c_["finish_us"]) / a["wall_us"], 3),
           "c_over_a": round(c_["wall_us"] / a["wall_us"], 3), "c_over_b": round(c_["wall_us"] / b_["wall_us"], 3),
           "b_over_a": round(b_["wall_us"] / a["wall_us"], 3)}
    path = args.out or os.path.join(ROOT, "profiles", "fed_pair_bench.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"tool": doc["tool"], "a_wall_us": a["wall_us"], "c_over_a": doc["c_over_a"], "c_over_b": doc["c_over_b"],
                      "begin_plus_finish_over_a": doc["begin_plus_finish_over_a"], "out": path}))


AHEAD_DEPTHS, AHEAD_LATENCIES_US = (1, 2, 4), (0, 200, 1000)


def main_ahead(args):
    """--ahead D: case d (fed, a host source) through GpuCache.lookup_stream with up to D calls open -> profiles/fed_ahead.json.
    The source is the numpy gather of case d plus a sleep of L microseconds -- the store's latency --, run by lookup_stream's worker
    threads; the main thread copies each answer to the device and finishes the calls oldest first.  Per depth in {1, 2, 4} (and D)
    one cache is warmed through the stream at L = 0; then, per L in {0, 200, 1000} (and --source-latency-us), --steps batches are
    timed as ONE stream between two synchronises: per_call_us = wall / batches.  Depth 1 at the largest L is timed three times: the
    spread the gain is held against.  begin_us / finish_us at depth 1 and 2 (L = 0) come from a hand-driven loop -- begin k + 1,
    finish k -- whose finish ends on a synchronise (the begin synchronises by itself): the cost of the hold stores and hold loads.
    Per depth the hit rate and the three fed_ahead_stats words per call, over the timed batches of all latencies together.  Only case d
    runs here: a device source is GPU work, which the driver's worker threads do not do.  The depth-1 comparison with the parent
    commit is NOT made by this tool: --baseline takes the case-c wall_us of three plain runs of this tool on each commit (same box,
    same session, alternating) from a file and records them beside the parent's spread."""
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    d, B = args.dim, args.batch
    ln, ev, pinned, scale = pinned_tables(bench.KAGGLE_LN, d, args.scale, dev)
    T = len(ln)
    cap = int(args.frac * sum(ln))
    base_np = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    all_host = np.concatenate([p.numpy() for p in pinned])
    del ev
    depths = sorted(set(AHEAD_DEPTHS) | {args.ahead})
    lats = sorted(set(AHEAD_LATENCIES_US) | {args.source_latency_us})
    n_warm = args.max_warm
    n_b = n_warm + args.steps
    rows = [b[1].t().contiguous().to(torch.int32) for b in bench.make_batches(ln, B, n_b, seed=3, device=dev, dist="zipf", alpha=args.alpha)]
    x = torch.rand((B, d), device=dev)
    timed = rows[n_warm:]

    def source(lat_us):
        def fn(keys):                                       # keys: uint64 numpy, on a worker thread: host work only
            k = keys.astype(np.int64)
            got = all_host[base_np[(k >> 32) - 1] + (k & 0xffffffff)]
            if lat_us:
                time.sleep(lat_us * 1e-6)
            return got
        return fn

    def stream_us(c, depth, lat_us):
        c.set_row_source(source(lat_us))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in c.lookup_stream(((r, x) for r in timed), depth=depth):
            pass
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / len(timed)

    def halves_us(c, depth):
        """begin and finish of a hand-driven loop at `depth` (1 or 2), L = 0: medians over the timed batches"""
        fn = source(0)
        tb, tf, open_calls = [], [], []

        def begin(r):
            t0 = time.perf_counter()
            _, keys = c.lookup_begin(r)                     # (synchronises)
            tb.append(time.perf_counter() - t0)
            open_calls.append(torch.from_numpy(fn(keys.cpu().numpy().view(np.uint64))).to(dev) if keys.numel() else None)

        def finish():
            fed = open_calls.pop(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c.lookup_finish_interact(fed, x)
            torch.cuda.synchronize()
            tf.append(time.perf_counter() - t0)

        for r in timed:
            begin(r)
            if len(open_calls) == depth:
                finish()
        while open_calls:
            finish()
        return round(float(np.median(tb)) * 1e6, 2), round(float(np.median(tf)) * 1e6, 2)

    res = {}
    for depth in depths:
        c = E.GpuCache("evlfu", cap, T, d, 32, "python", dev).set_miss_order("fetch-first")
        c.set_fed_backing([None] * T, ln).set_fed_depth(depth)
        c.set_row_source(source(0))
        for _ in c.lookup_stream(((r, x) for r in rows[:n_warm]), depth=depth):
            pass
        print("fed_backing_bench: depth %d warm, size %d of %d" % (depth, c.batch_stats()["size"], cap), file=sys.stderr, flush=True)
        s0, a0 = c.batch_stats(), c.fed_ahead_stats()
        per = {str(lat): round(stream_us(c, depth, lat), 2) for lat in lats}
        s1, a1 = c.batch_stats(), c.fed_ahead_stats()
        n_calls = len(lats) * len(timed)
        res[str(depth)] = {"per_call_us": per, "hit_rate": round((s1["n_hits"] - s0["n_hits"]) / (T * B * n_calls), 4),
                           "fed_ahead_stats_per_call": {k: round((a1[k] - a0[k]) / n_calls, 2) for k in a1}, "flushes": s1["n_flush"] - s0["n_flush"]}
        if depth == 1:
            res["1"]["repeats_at_%d_us" % lats[-1]] = [per[str(lats[-1])]] + [round(stream_us(c, 1, lats[-1]), 2) for _ in range(2)]
        if depth in (1, 2):
            res[str(depth)]["begin_us"], res[str(depth)]["finish_us"] = halves_us(c, depth)
        print("fed_backing_bench: depth %d %s" % (depth, res[str(depth)]), file=sys.stderr, flush=True)
        del c
    rep = res["1"]["repeats_at_%d_us" % lats[-1]]
    G = res["1"]["begin_us"] + res["1"]["finish_us"]
    L = float(lats[-1])
    doc = {"tool": "fed_backing_bench --ahead", "device": torch.cuda.get_device_name(0),
           "shape": {"rows": sum(ln), "table_scale": scale, "capacity": cap, "frac": args.frac, "batch": B, "dim": d, "zipf_alpha": args.alpha,
                     "warm_batches": n_warm, "timed_batches": len(timed), "policy": "evlfu", "consumer": "lookup_finish_interact",
                     "source": "numpy gather from host tables + sleep(L), on lookup_stream's worker threads"},
           "timing": "per_call_us: one lookup_stream over the timed batches between two synchronises, wall / batches; begin_us / finish_us: medians of "
                     "a hand-driven loop (begin k + 1, finish k) at L = 0, the finish between two synchronises; one run on one box",
           "depths": res,
           "depth_1_spread_us": round(max(rep) - min(rep), 2),
           "gain_at_%d_us" % lats[-1]: {str(D): round(res[str(D)]["per_call_us"][str(lats[-1])] / res["1"]["per_call_us"][str(lats[-1])], 3) for D in depths if D > 1},
           "model_at_%d_us" % lats[-1]: {str(D): round(max(G, (L + G) / D) / (L + G), 3) for D in depths if D > 1},
           "G_us": round(G, 2),
           "hold_cost_us": {"begin": round(res["2"]["begin_us"] - res["1"]["begin_us"], 2), "finish": round(res["2"]["finish_us"] - res["1"]["finish_us"], 2)}}
    if args.baseline:   # case c of this tool on the parent commit and on this one, three runs each in one session (wall_us per call)
        with open(args.baseline) as f:
            base = json.load(f)
        par, new = base["parent_c_wall_us"], base["this_c_wall_us"]
        spread = round(max(par) - min(par), 2)
        doc["depth_1_regression"] = {"case": "c_fed_device_source, wall_us per call, runs alternating in one session on one box",
                                     "parent_c_wall_us": par, "this_c_wall_us": new, "parent_spread_us": spread,
                                     "bound_us": round(max(par) + spread, 2), "within_bound": bool(max(new) <= max(par) + spread)}
    path = args.out or os.path.join(ROOT, "profiles", "fed_ahead.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"tool": doc["tool"], "per_call_us": {D: res[D]["per_call_us"] for D in res}, "depth_1_spread_us": doc["depth_1_spread_us"],
                      "hold_cost_us": doc["hold_cost_us"], "out": path}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ahead", type=int, default=0, help="case d through lookup_stream with up to this many calls open (1 .. 4) -> profiles/fed_ahead.json")
    ap.add_argument("--source-latency-us", type=int, default=0, help="--ahead: a store latency measured beside 0, 200 and 1000 us")
    ap.add_argument("--baseline", default="", help="--ahead: a JSON file {parent_c_wall_us: [..], this_c_wall_us: [..]} of case c timed on the parent commit "
                                                   "and on this one, recorded into the output beside the parent's spread")
    ap.add_argument("--frac", type=float, default=0.10)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--steps", type=int, default=100, help="timed batches")
    ap.add_argument("--max-warm", type=int, default=150, help="at most this many warm-up batches")
    ap.add_argument("--scale", type=float, default=1.0, help="every table's rows times this")
    ap.add_argument("--dim", type=int, default=36)
    ap.add_argument("--bags", action="store_true", help="the bag form beside the count-first fetch-first bag chain -> profiles/fed_bags.json")
    ap.add_argument("--max-bag", type=int, default=10, help="--bags: bags of 1 .. this many indices")
    ap.add_argument("--pair", action="store_true", help="the fed C1 + C2 pair beside the fetch-first pair -> profiles/fed_pair_bench.json")
    ap.add_argument("--fill", type=int, default=180, help="--pair: batches that fill the tiers")
    ap.add_argument("--out", default="", help="default: profiles/fed_backing.json (--bags: profiles/fed_bags.json, --pair: profiles/fed_pair_bench.json, "
                                              "--ahead: profiles/fed_ahead.json)")
    args = ap.parse_args()
    if args.ahead:
        return main_ahead(args)
    if args.bags:
        return main_bags(args)
    if args.pair:
        return main_pair(args)
    args.out = args.out or os.path.join(ROOT, "profiles", "fed_backing.json")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    d, B = args.dim, args.batch
    ln, ev, pinned, scale = pinned_tables(bench.KAGGLE_LN, d, args.scale, dev)
    T = len(ln)
    cap = int(args.frac * sum(ln))
    rb = d * 4
    # the sources: every table behind one base offset, on the device and on the host
    base_np = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int64)
    base_dev = torch.from_numpy(base_np).to(dev)
    all_dev = torch.cat([ev.fp32_view(k) for k in range(T)])
    all_host = np.concatenate([p.numpy() for p in pinned])

    def device_source(keys):   # keys: int64 device tensor
        return all_dev.index_select(0, base_dev[(keys >> 32) - 1] + (keys & 0xffffffff))

    def host_source(keys):
        k = keys.cpu().numpy()
        return torch.from_numpy(all_host[base_np[(k >> 32) - 1] + (k & 0xffffffff)]).to(dev)

    sources = {"c_fed_device_source": device_source, "d_fed_host_source": host_source}
    n_b = args.max_warm + args.steps
    rows = [b[1].t().contiguous().to(torch.int32) for b in bench.make_batches(ln, B, n_b, seed=3, device=dev, dist="zipf", alpha=args.alpha)]
    x = torch.rand((B, d), device=dev)
    F = T + 1
    out = torch.empty((B, d + F * (F - 1) // 2), device=dev)
    hit = torch.empty((B, T), dtype=torch.uint8, device=dev)

    def call(name, c, r, split=None):
        if name in sources:
            t0 = time.perf_counter()
            _, keys = c.lookup_begin(r, hit)                # (synchronises)
            t1 = time.perf_counter()
            fed = sources[name](keys) if keys.numel() else None
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            c.lookup_finish_interact(fed, x, out=out)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            if split is not None:
                split.append((t1 - t0, t2 - t1, t3 - t2, int(keys.numel())))
        else:
            c.lookup_interact(r, x, out=out, hit=hit)

    caches, warm = {}, {}
    for name in NAMES:
        c = E.GpuCache("evlfu", cap, T, d, 32, "python", dev).set_miss_order("fetch-first")
        if name in sources:
            c.set_fed_backing([None] * T, ln)
        else:
            c.set_backing(pinned if name.startswith("b_") else ev)
        size = -1
        for i in range(args.max_warm):
            call(name, c, rows[i])
            if i % 10 == 9:
                s = c.batch_stats()["size"]
                if s <= size:
                    break
                size = s
        caches[name], warm[name] = c, i + 1
        print("fed_backing_bench: %s warm after %d batches, size %d of %d" % (name, i + 1, c.batch_stats()["size"], cap), file=sys.stderr, flush=True)
    timed = rows[args.max_warm:]
    s0 = {n: (caches[n].batch_stats(), caches[n].fetch_stats(), caches[n].fed_stats()) for n in NAMES}
    events, wall, split = {n: [] for n in NAMES}, {n: [] for n in NAMES}, {n: [] for n in sources}
    for r in timed:
        for n in NAMES:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            call(n, caches[n], r, split.get(n))
            e1.record()
            torch.cuda.synchronize()
            wall[n].append(time.perf_counter() - t0)
            events[n].append((e0, e1))
    res = {}
    for n in NAMES:
        s1, f1, fs1 = caches[n].batch_stats(), caches[n].fetch_stats(), caches[n].fed_stats()
        w = np.array(wall[n]) * 1e6
        res[n] = {"wall_us": round(float(np.median(w)), 2), "wall_p95_us": round(float(np.percentile(w, 95)), 2),
                  "hit_rate": round((s1["n_hits"] - s0[n][0]["n_hits"]) / (T * B * len(timed)), 4), "size": s1["size"],
                  "warm_batches": warm[n], "fetch_stats_delta": {k: f1[k] - s0[n][1][k] for k in f1}}
        if n in sources:
            sp = np.array(split[n], np.float64)
            res[n].update({"begin_us": round(float(np.median(sp[:, 0])) * 1e6, 2), "source_us": round(float(np.median(sp[:, 1])) * 1e6, 2),
                           "finish_us": round(float(np.median(sp[:, 2])) * 1e6, 2), "keys_per_batch": round(float(sp[:, 3].mean()), 1),
                           "fed_bytes_per_batch": round(float(sp[:, 3].mean()) * rb),
                           "fed_stats_delta": {k: fs1[k] - s0[n][2][k] for k in fs1}})
        else:
            us = np.array([a.elapsed_time(b) * 1e3 for a, b in events[n]])
            res[n].update({"median_us": round(float(np.median(us)), 2), "p95_us": round(float(np.percentile(us, 95)), 2)})
        print("fed_backing_bench: %s %s" % (n, res[n]), file=sys.stderr, flush=True)
    a = res["a_fetch_first_hbm"]["wall_us"]
    c_ = res["c_fed_device_source"]
    doc = {"tool": "fed_backing_bench", "device": torch.cuda.get_device_name(0),
           "shape": {"rows": sum(ln), "table_scale": scale, "capacity": cap, "frac": args.frac, "batch": B, "dim": d, "row_bytes": rb,
                     "zipf_alpha": args.alpha, "timed_batches": len(timed), "policy": "evlfu",
                     "consumer": "lookup_interact / lookup_finish_interact (the fused interaction through the address table)"},
           "timing": "host clock between two synchronises around every call (wall_us; begin / source / finish each end on a synchronise); "
                     "a and b also by a pair of device events (median_us); the configurations alternate on the same batches in one process",
           "configs": res,
           "begin_over_a_us": round(c_["begin_us"] + c_["finish_us"] - a, 2),
           "c_over_a": round(c_["wall_us"] / a, 3), "d_over_a": round(res["d_fed_host_source"]["wall_us"] / a, 3),
           "b_over_a": round(res["b_fetch_first_pinned"]["wall_us"] / a, 3)}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"tool": "fed_backing_bench", "a_wall_us": a, "c_over_a": doc["c_over_a"], "d_over_a": doc["d_over_a"],
                      "begin_over_a_us": doc["begin_over_a_us"], "out": args.out}))


if __name__ == "__main__":
    main()
