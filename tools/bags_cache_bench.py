#!/usr/bin/env python3
"""Multi-hot bags behind the LRU / LFU / EvLFU cache tier: the chain  probe -> pooling -> dense interaction -> insert
(GpuCache.lookup_bags_interact; EvLFU under set_bag_rule("served-bags"): probe -> pooling -> dense interaction -> raise + list
-> insert) beside the uncached apply_emb_interact on the same batches, as ONE JSON file.  Every policy's leg draws the same
batches (one seed), so the LRU chain of the same run is the yardstick for the EvLFU one.

Shape: the Criteo-Kaggle cardinalities with the 10 % tier, bags of 1 .. 10 indices drawn as tools/multihot_bench.py draws them,
rows Zipf(0.75) as bench.make_batches draws them, B = 2 048 and 16 384.  The tier is warmed until its size stops growing;
then, in one run with the two alternating batch by batch, every batch is timed by a pair of device events around the chain and
another around the uncached call (dispatch gaps included: what a caller sees).  Hit rate = hit positions / positions over the
timed batches.

The per-kernel split comes from a profiler run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bags_cache_bench.py --chain-only --batch 2048
    python tools/bags_cache_bench.py --kernel-stats 2048=DIR/.../..._kernel_stats.csv evlfu:16384=... --out profiles/bags_cache.json
(--chain-only runs the warm-up and the chain alone, one --policy per profiler run; --kernel-stats folds the library's rows of
those files into the JSON under kernel_split[policy], the policy named in front of the batch size, lru when it is left out.)

--pair: the bag form of the mixed-precision C1 + C2 pair (lookup_bags_interact_c1c2: probe2 -> count -> route + raise + list ->
pool2 -> dense interaction -> the pair's update) at the reference's flagship shape -- u8 C1 + u4 C2 at the 48-48-4 split of 2 %
of the Kaggle rows (1 296 480 + 2 592 960 entries), d = 36, B = 16 384, Zipf 0.75, both pairs warmed until their sizes stop
growing -- into profiles/bags_pair.json:
  (a) one index per bag beside lookup_interact_c1c2(fused=False) on a twin pair: the same batches, alternating, one process;
  (b) ragged bags of mean length --pair-mean-bag (0 .. 2 x mean indices) on the first pair.
Its per-kernel times come from a profiler run of its own, as above:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bags_cache_bench.py --pair --chain-only
    python tools/bags_cache_bench.py --pair --pair-timing profiles/bags_pair.json --kernel-stats one_index_per_bag=DIR/.../..._kernel_stats.csv

--pair --fetch-first [--host-tables]: the pair's fetch-first bag chain (both tiers set_miss_order("fetch-first") and
set_bag_count("count-first"): probe2 -> count -> route + raise + list -> the pair's update -> bags_repoint2 -> pool2 -> dense
interaction) at the --pair shape, into profiles/bag_pair_fetch_first.json.  Without --host-tables: over HBM, alternating with the
order-0 chain on a twin pair (section "hbm").  With it: both tiers' tables in pinned host memory, alternating -- one index per bag
-- with the (B, T) fetch-first pair on a twin (section "pinned"), with the rows fetched, the positions read in place and the bus
bytes per call.  --chain-only runs the fetch-first chain alone for a profiler, as above (--pair-profile one | ragged), and
    python tools/bags_cache_bench.py --pair --fetch-first --pair-timing profiles/bag_pair_fetch_first.json --kernel-stats NAME=CSV
folds the profiler's rows into the JSON under kernel_split[NAME] (no GPU needed).

--host-tables: the count-first EvLFU bag chain (GpuCache.set_bag_count("count-first")) at this tool's shape, into
profiles/bags_count_first.json -- (a) EvLFU bags, order 0, the default chain, HBM tables: today's form; (b) the same count-first;
(c) EvLFU bags, count-first, fetch-first, PINNED host tables; (d) LRU and LFU bags, fetch-first, pinned tables.  Per
configuration: median / p95 us per call, hit rate, and the bytes that crossed the bus per call as tools/host_setassoc_bench.py
accounts them.  The five alternate on the same batches in one process.  (a) as the PARENT commit runs it on the same machine is
b's yardstick: this file run from the parent commit's tree with --host-configs a (a needs nothing new), beside b alone from this
tree, folded in by --yardstick:
    python tools/bags_cache_bench.py --host-tables --host-configs a --out PARENT_A.json        (the parent commit's library)
    python tools/bags_cache_bench.py --host-tables --host-configs b --out B.json
    python tools/bags_cache_bench.py --host-tables --batch 2048 16384 --yardstick parent_a=PARENT_A.json b=B.json
Where the count pass's time goes comes from profiler runs of single configurations (--kernel-stats NAME=CSV folds them in):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bags_cache_bench.py --host-tables --host-configs b --chain-only --batch 16384
Needs a GPU."""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import evstore_dlrm_amd as E  # noqa: E402


def make_batch(ln, B, g, dev, max_bag, alpha):
    """-> (lS_o, lS_i): per table B bag starts and the indices; bag sizes max(1, round(U * min(n, max_bag))), rows Zipf"""
    lo, li = [], []
    e = 1.0 - alpha
    for n in ln:
        sizes = torch.clamp(torch.round(torch.rand((B,), device=dev, generator=g) * min(n, max_bag)), min=1).to(torch.int64)
        ends = torch.cumsum(sizes, 0)
        nnz = int(ends[-1])
        u = torch.rand((nnz,), device=dev, generator=g, dtype=torch.float64)
        r = (((float(n) ** e - 1.0) * u + 1.0) ** (1.0 / e)).to(torch.int64).clamp_(1, n) - 1
        lo.append((ends - sizes).contiguous())
        li.append((r * 2654435761 % n).to(torch.int64))
    return lo, li


def warm(c, ln, B, g, dev, x, args):
    """batches until the tier's size grows by less than 0.2 % of its capacity over ten of them -> batches used"""
    n, last = 0, -1
    while n < args.max_warmup:
        for _ in range(10):
            lo, li = make_batch(ln, B, g, dev, args.max_bag, args.alpha)
            c.lookup_bags_interact(lo, li, x)
        n += 10
        size = c.batch_stats()["size"]
        if last >= 0 and size - last < 0.002 * c.capacity:
            break
        last = size
    return n


def run(policy, B, ev, ln, dev, args):
    T, d = len(ln), args.dim
    cap = int(args.frac * sum(ln))
    c = E.GpuCache(policy, cap, T, d, 32, "python", dev)
    c.set_backing(ev)
    if policy == "evlfu":
        c.set_bag_rule("served-bags")
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand((B, d), device=dev)
    n_warm = warm(c, ln, B, g, dev, x, args)
    batches = [make_batch(ln, B, g, dev, args.max_bag, args.alpha) for _ in range(args.steps)]
    n_pos = sum(int(t.numel()) for _, li in batches for t in li)
    F = T + 1
    R = torch.empty((B, d + F * (F - 1) // 2), device=dev)
    s0 = c.batch_stats()
    if args.chain_only:
        for lo, li in batches:
            c.lookup_bags_interact(lo, li, x, out=R)
        torch.cuda.synchronize()
        return {"policy": policy, "batch": B, "warmup_batches": n_warm, "batches": args.steps}
    for lo, li in batches[:5]:                       # the uncached path's first launches
        E.apply_emb_interact(x, lo, li, ev)
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.steps)]
    torch.cuda.synchronize()
    for (lo, li), e4 in zip(batches, evs):
        e4[0].record()
        c.lookup_bags_interact(lo, li, x, out=R)
        e4[1].record()
        e4[2].record()
        E.apply_emb_interact(x, lo, li, ev)
        e4[3].record()
    torch.cuda.synchronize()
    s1 = c.batch_stats()
    chain = np.array([e4[0].elapsed_time(e4[1]) for e4 in evs]) * 1e3
    plain = np.array([e4[2].elapsed_time(e4[3]) for e4 in evs]) * 1e3
    return {"policy": policy, "batch": B, "capacity": cap, "warmup_batches": n_warm, "timed_batches": args.steps,
            "lookups_per_batch": round(n_pos / args.steps, 1), "size": s1["size"],
            "hit_rate": round((s1["n_hits"] - s0["n_hits"]) / n_pos, 4),
            "all_hit_samples": s1["n_perfect_hits"] - s0["n_perfect_hits"], "evictions": s1["n_evict"] - s0["n_evict"],
            "flushes": s1["n_flush"] - s0["n_flush"],
            "chain_us_per_batch": {"mean": round(float(chain.mean()), 2), "median": round(float(np.median(chain)), 2)},
            "uncached_apply_emb_interact_us_per_batch": {"mean": round(float(plain.mean()), 2), "median": round(float(np.median(plain)), 2)}}


def make_pair_batch(ln, B, g, dev, mean_bag, alpha):
    """-> (lS_o, lS_i, rq): bags of exactly one index (mean_bag == 1; rq = the (B, T) int32 rows of the same batch) or of
    0 .. 2 * mean_bag indices (rq None); rows Zipf as make_batch draws them"""
    lo, li = [], []
    e = 1.0 - alpha
    for n in ln:
        if mean_bag == 1:
            sizes = torch.ones((B,), dtype=torch.int64, device=dev)
        else:
            sizes = torch.randint(0, 2 * mean_bag + 1, (B,), device=dev, generator=g, dtype=torch.int64)
        ends = torch.cumsum(sizes, 0)
        nnz = int(ends[-1])
        u = torch.rand((nnz,), device=dev, generator=g, dtype=torch.float64)
        r = (((float(n) ** e - 1.0) * u + 1.0) ** (1.0 / e)).to(torch.int64).clamp_(1, n) - 1
        lo.append((ends - sizes).contiguous())
        li.append((r * 2654435761 % n).to(torch.int64))
    rq = torch.stack(li, 1).to(torch.int32).contiguous() if mean_bag == 1 else None
    return lo, li, rq


def run_pair(ln, dev, args):
    """the pair's bag form at the flagship shape -> the JSON's "pair" section (or, --chain-only, the profiled chain alone)"""
    T, d, B = len(ln), args.dim, args.pair_batch
    ev = bench.make_tables(ln, d, seed=0, device=dev)
    ev8, ev4 = ev.encode(8), ev.encode(4)
    budget = int(0.02 * sum(ln))
    caps = (int(0.48 * budget) * 4, int(0.48 * budget) * 8)

    def pair(rule):
        c1, c2 = E.GpuCache("evlfu", caps[0], T, d, 8, "cpp", dev), E.GpuCache("evlfu", caps[1], T, d, 4, "cpp", dev)
        c1.set_backing(ev8)
        c2.set_backing(ev4)
        if rule:
            c1.set_bag_rule("served-bags")
            c2.set_bag_rule("served-bags")
        return c1, c2

    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand((B, d), device=dev)
    F = T + 1
    R = torch.empty((B, d + F * (F - 1) // 2), device=dev)
    a = pair(True)
    b = None if args.chain_only else pair(False)
    n_warm, last = 0, -1
    while n_warm < args.max_warmup:                   # one index per bag on both pairs until the sizes stop growing
        for _ in range(10):
            lo, li, rq = make_pair_batch(ln, B, g, dev, 1, args.alpha)
            E.lookup_bags_interact_c1c2(a[0], a[1], lo, li, x, out=R)
            if b:
                E.lookup_interact_c1c2(b[0], b[1], rq, x, fused=False)
        n_warm += 10
        size = a[0].batch_stats()["size"] + a[1].batch_stats()["size"]
        if last >= 0 and size - last < 0.002 * (caps[0] + caps[1]):
            break
        last = size
    one = [make_pair_batch(ln, B, g, dev, 1, args.alpha) for _ in range(args.steps)]
    rag = [make_pair_batch(ln, B, g, dev, args.pair_mean_bag, args.alpha) for _ in range(args.steps)]
    if args.chain_only:
        for lo, li, _ in (rag if args.pair_profile == "ragged" else one):
            E.lookup_bags_interact_c1c2(a[0], a[1], lo, li, x, out=R)
        torch.cuda.synchronize()
        return {"batch": B, "warmup_batches": n_warm, "batches": args.steps, "profiled": args.pair_profile}

    def stats(p):
        return [c.batch_stats() for c in p]

    out = {"batch": B, "capacities": list(caps), "codecs": [8, 4], "dim": d, "warmup_batches": n_warm,
           "sizes_after_warmup": [s["size"] for s in stats(a)], "timed_batches": args.steps}
    # (a) one index per bag: the bag form on pair a, the (B, T) form + dense interaction on its twin, alternating
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(args.steps)]
    s0, t0 = stats(a), stats(b)
    torch.cuda.synchronize()
    for (lo, li, rq), e4 in zip(one, evs):
        e4[0].record()
        E.lookup_bags_interact_c1c2(a[0], a[1], lo, li, x, out=R)
        e4[1].record()
        e4[2].record()
        E.lookup_interact_c1c2(b[0], b[1], rq, x, fused=False)
        e4[3].record()
    torch.cuda.synchronize()
    s1, t1 = stats(a), stats(b)
    bag = np.array([e4[0].elapsed_time(e4[1]) for e4 in evs]) * 1e3
    bt = np.array([e4[2].elapsed_time(e4[3]) for e4 in evs]) * 1e3
    n_pos = args.steps * B * T
    out["one_index_per_bag"] = {
        "bag_form_us_per_call": {"mean": round(float(bag.mean()), 2), "median": round(float(np.median(bag)), 2)},
        "bt_form_unfused_us_per_call": {"mean": round(float(bt.mean()), 2), "median": round(float(np.median(bt)), 2)},
        "ratio_bag_over_bt_median": round(float(np.median(bag) / np.median(bt)), 3),
        "hit_rate_bag_form": round(sum(s1[k]["n_hits"] - s0[k]["n_hits"] for k in (0, 1)) / n_pos, 4),
        "hit_rate_bt_form": round(sum(t1[k]["n_hits"] - t0[k]["n_hits"] for k in (0, 1)) / n_pos, 4)}
    # (b) ragged bags on pair a
    for lo, li, _ in rag[:10]:
        E.lookup_bags_interact_c1c2(a[0], a[1], lo, li, x, out=R)
    ev2 = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(args.steps)]
    s0 = stats(a)
    torch.cuda.synchronize()
    for (lo, li, _), e2 in zip(rag, ev2):
        e2[0].record()
        E.lookup_bags_interact_c1c2(a[0], a[1], lo, li, x, out=R)
        e2[1].record()
    torch.cuda.synchronize()
    s1 = stats(a)
    t = np.array([e2[0].elapsed_time(e2[1]) for e2 in ev2]) * 1e3
    n_pos = sum(int(v.numel()) for _, li, _ in rag for v in li)
    out["ragged"] = {"mean_bag": args.pair_mean_bag, "lookups_per_call": round(n_pos / args.steps, 1),
                     "bag_form_us_per_call": {"mean": round(float(t.mean()), 2), "median": round(float(np.median(t)), 2)},
                     "hit_rate": round(sum(s1[k]["n_hits"] - s0[k]["n_hits"] for k in (0, 1)) / n_pos, 4),
                     "all_served_samples": s1[0]["n_perfect_hits"] - s0[0]["n_perfect_hits"],
                     "flushes": [s1[k]["n_flush"] - s0[k]["n_flush"] for k in (0, 1)]}
    return out


def run_pair_fetch(ln, dev, args):
    """--pair --fetch-first: the pair's fetch-first bag chain (both tiers set_miss_order("fetch-first") + set_bag_count("count-first"))
    at the --pair shape -> the JSON's "hbm" section, or, with --host-tables, its "pinned" section.  Over HBM it alternates with the order-0 chain on a twin pair;
    with --host-tables both tiers' tables are pinned host tensors and it alternates, one index per bag, with the (B, T) fetch-first
    pair (lookup_interact_c1c2(fused=False)) on a twin.  All pairs see the same batches, call by call, in one process."""
    T, d, B = len(ln), args.dim, args.pair_batch
    ev = bench.make_tables(ln, d, seed=0, device=dev)
    ev8, ev4 = ev.encode(8), ev.encode(4)
    del ev
    rbs = (d, d // 2)                                 # row bytes of the u8 and the u4 tier
    tabs = ([t.cpu().pin_memory() for t in ev8.raw], [t.cpu().pin_memory() for t in ev4.raw]) if args.host_tables else (ev8, ev4)
    budget = int(0.02 * sum(ln))
    caps = (int(0.48 * budget) * 4, int(0.48 * budget) * 8)

    def pair(order):
        p = E.GpuCache("evlfu", caps[0], T, d, 8, "cpp", dev), E.GpuCache("evlfu", caps[1], T, d, 4, "cpp", dev)
        for c, tab in zip(p, tabs):
            if order:
                c.set_miss_order("fetch-first").set_bag_count("count-first")
            c.set_bag_rule("served-bags").set_backing(tab)
        return p

    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand((B, d), device=dev)
    F = T + 1
    R = torch.empty((B, d + F * (F - 1) // 2), device=dev)
    bags = lambda p: (lambda lo, li, rq: E.lookup_bags_interact_c1c2(p[0], p[1], lo, li, x, out=R))
    bt = lambda p: (lambda lo, li, rq: E.lookup_interact_c1c2(p[0], p[1], rq, x, fused=False))
    if args.chain_only:
        pairs = {"fetch_first": pair(1)}
        calls = {"fetch_first": bags(pairs["fetch_first"])}
    elif args.host_tables:
        pairs = {"fetch_first_pinned": pair(1), "bt_fetch_first_pinned": pair(1)}
        calls = {"fetch_first_pinned": bags(pairs["fetch_first_pinned"]), "bt_fetch_first_pinned": bt(pairs["bt_fetch_first_pinned"])}
    else:
        pairs = {"order0_hbm": pair(0), "fetch_first_hbm": pair(1)}
        calls = {n: bags(p) for n, p in pairs.items()}
    first = next(iter(pairs.values()))
    n_warm, last = 0, -1
    while n_warm < args.max_warmup:                   # one index per bag on every pair until the sizes stop growing
        for _ in range(10):
            batch = make_pair_batch(ln, B, g, dev, 1, args.alpha)
            for call in calls.values():
                call(*batch)
        n_warm += 10
        size = first[0].batch_stats()["size"] + first[1].batch_stats()["size"]
        if last >= 0 and size - last < 0.002 * (caps[0] + caps[1]):
            break
        last = size
    draws = {"one_index_per_bag": [make_pair_batch(ln, B, g, dev, 1, args.alpha) for _ in range(args.steps)],
             "ragged": [make_pair_batch(ln, B, g, dev, args.pair_mean_bag, args.alpha) for _ in range(args.steps)]}
    if args.chain_only:
        for batch in draws["ragged" if args.pair_profile == "ragged" else "one_index_per_bag"]:
            calls["fetch_first"](*batch)
        torch.cuda.synchronize()
        return {"batch": B, "warmup_batches": n_warm, "batches": args.steps, "profiled": args.pair_profile}
    out = {"batch": B, "capacities": list(caps), "codecs": [8, 4], "dim": d, "tables": "pinned host memory" if args.host_tables else "HBM",
           "warmup_batches": n_warm, "sizes_after_warmup": [c.batch_stats()["size"] for c in first], "timed_batches": args.steps}

    def snap(p):
        return [c.batch_stats() for c in p], p[0].fetch_stats()

    for section, batches in draws.items():
        names = [n for n in calls if section == "one_index_per_bag" or not n.startswith("bt_")]
        for batch in batches[:10]:                    # settle on the timed draw before the clock starts
            for n in names:
                calls[n](*batch)
        s0 = {n: snap(pairs[n]) for n in names}
        events = {n: [] for n in names}
        torch.cuda.synchronize()
        for batch in batches:
            for n in names:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                calls[n](*batch)
                e1.record()
                events[n].append((e0, e1))
        torch.cuda.synchronize()
        n_pos = sum(int(v.numel()) for _, li, _ in batches for v in li)
        res = {}
        for n in names:
            us = np.array([a.elapsed_time(b) * 1e3 for a, b in events[n]])
            (st0, f0), (st1, f1) = s0[n], snap(pairs[n])
            hits = sum(st1[k]["n_hits"] - st0[k]["n_hits"] for k in (0, 1))
            fetched = [st1[k]["size"] - st0[k]["size"] + st1[k]["n_evict"] - st0[k]["n_evict"] for k in (0, 1)]
            fd = {k: f1[k] - f0.get(k, 0) for k in f1}
            res[n] = {"median_us": round(float(np.median(us)), 2), "p95_us": round(float(np.percentile(us, 95)), 2),
                      "hit_rate": round(hits / n_pos, 4), "miss_positions_per_call": round((n_pos - hits) / args.steps, 1),
                      "rows_fetched_per_call": [round(f / args.steps, 1) for f in fetched], "fetch_stats_delta": fd,
                      "flushes": [st1[k]["n_flush"] - st0[k]["n_flush"] for k in (0, 1)]}
            if args.host_tables:                      # the update's fetches, plus the positions the pooling reads in place (their tier is not
                rest = fd.get("in_place", 0) + fd.get("victim_hits", 0)   # counted: bounded by the u4 and the u8 row)
                res[n]["bus_bytes_per_call"] = [round((fetched[0] * rbs[0] + fetched[1] * rbs[1] + rest * rb) / args.steps) for rb in (rbs[1], rbs[0])]
                res[n]["positions_read_from_host_by_the_consumer_per_call"] = round(rest / args.steps, 1)
            print("bags_cache_bench: %s %s %s" % (section, n, res[n]), file=sys.stderr, flush=True)
        entry = {"lookups_per_call": round(n_pos / args.steps, 1), "configs": res}
        if "order0_hbm" in res:
            entry["fetch_first_over_order0_median"] = round(res["fetch_first_hbm"]["median_us"] / res["order0_hbm"]["median_us"], 3)
        if "bt_fetch_first_pinned" in res:
            entry["bag_form_over_bt_form_median"] = round(res["fetch_first_pinned"]["median_us"] / res["bt_fetch_first_pinned"]["median_us"], 3)
        out[section] = entry
    return out


HOST_CONFIGS = {   # name -> (policy, tables, how the cache is told)
    "a_evlfu_default_hbm": ("evlfu", "hbm", lambda c: c.set_bag_rule("served-bags")),
    "b_evlfu_count_first_hbm": ("evlfu", "hbm", lambda c: c.set_bag_rule("served-bags").set_bag_count("count-first")),
    "c_evlfu_count_first_fetch_first_pinned": ("evlfu", "pinned", lambda c: c.set_miss_order("fetch-first").set_bag_rule("served-bags")
                                               .set_bag_count("count-first")),
    "d_lru_fetch_first_pinned": ("lru", "pinned", lambda c: c.set_miss_order("fetch-first")),
    "d_lfu_fetch_first_pinned": ("lfu", "pinned", lambda c: c.set_miss_order("fetch-first")),
}


def run_host(ln, dev, args):
    """--host-tables: the EvLFU bag chain count-first, over HBM and over pinned tables in fetch-first order, beside today's chain
    and beside the LRU / LFU fetch-first bag chains -> the JSON's "host_tables" section, one entry per batch size.  Every
    configuration is warmed on the same warm-up batches until its size stops growing; the timed batches are the same for all,
    the configurations alternating call by call.  If the machine refuses the pinned memory every table is halved until it fits
    (tools/host_setassoc_bench.py's rule) and the factor is recorded."""
    d, T = args.dim, len(ln)
    scale = 1.0
    while True:
        lns = [max(1, int(n * scale)) for n in ln]
        ev = bench.make_tables(lns, d, seed=0, device=dev)
        try:
            pinned = [ev.fp32_view(k).cpu().pin_memory() for k in range(T)]
            break
        except RuntimeError as e:
            print("bags_cache_bench: pinning %.2f GB failed (%s); halving every table" % (sum(lns) * d * 4 / 1e9, e), file=sys.stderr, flush=True)
            del ev
            scale *= 0.5
    cap = int(args.frac * sum(lns))
    rb = d * 4
    out = {"rows": sum(lns), "table_scale": scale, "capacity": cap, "row_bytes": rb, "pinned_bytes": sum(lns) * rb, "batches": {}}
    F = T + 1
    for B in args.batch:
        x = torch.rand((B, d), device=dev)
        R = torch.empty((B, d + F * (F - 1) // 2), device=dev)
        caches, warmed = {}, {}
        for name, (policy, where, tell) in HOST_CONFIGS.items():
            if not name.startswith(tuple(args.host_configs)):
                continue
            c = E.GpuCache(policy, cap, T, d, 32, "python", dev)
            tell(c)
            c.set_backing(pinned if where == "pinned" else ev)
            caches[name] = c
            warmed[name] = warm(c, lns, B, torch.Generator(device=dev).manual_seed(7), dev, x, args)
        g = torch.Generator(device=dev).manual_seed(11)
        batches = [make_batch(lns, B, g, dev, args.max_bag, args.alpha) for _ in range(args.steps)]
        n_pos = sum(int(t.numel()) for _, li in batches for t in li)
        if args.chain_only:                          # the run a profiler wraps: the selected chains alone, untimed
            for lo, li in batches:
                for c in caches.values():
                    c.lookup_bags_interact(lo, li, x, out=R)
            torch.cuda.synchronize()
            out["batches"]["B=%d" % B] = {"chain_only": list(caches), "warmup_batches": warmed, "batches": args.steps}
            continue
        for lo, li in batches[:10]:                  # settle: every configuration on the timed draw before the clock starts
            for c in caches.values():
                c.lookup_bags_interact(lo, li, x, out=R)
        s0 = {n: (c.batch_stats(), c.fetch_stats()) for n, c in caches.items()}
        events = {n: [] for n in caches}
        torch.cuda.synchronize()
        for lo, li in batches:
            for n, c in caches.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                c.lookup_bags_interact(lo, li, x, out=R)
                e1.record()
                events[n].append((e0, e1))
        torch.cuda.synchronize()
        res = {}
        for n, c in caches.items():
            us = np.array([a.elapsed_time(b) * 1e3 for a, b in events[n]])
            s1, f1 = c.batch_stats(), c.fetch_stats()
            fd = {k: f1[k] - s0[n][1][k] for k in f1}
            fetched = s1["size"] - s0[n][0]["size"] + s1["n_evict"] - s0[n][0]["n_evict"]
            res[n] = {"median_us": round(float(np.median(us)), 2), "p95_us": round(float(np.percentile(us, 95)), 2),
                      "hit_rate": round((s1["n_hits"] - s0[n][0]["n_hits"]) / n_pos, 4), "size": s1["size"], "warmup_batches": warmed[n],
                      "flushes": s1["n_flush"] - s0[n][0]["n_flush"], "fetch_stats_delta": fd,
                      "bus_bytes_per_call": None if HOST_CONFIGS[n][1] == "hbm" else round((fetched + fd["in_place"]) * rb / args.steps)}
            print("bags_cache_bench: B=%d %s %s" % (B, n, res[n]), file=sys.stderr, flush=True)
        entry = {"lookups_per_call": round(n_pos / args.steps, 1), "timed_batches": args.steps, "configs": res}
        med = {k[0]: v["median_us"] for k, v in res.items() if k[0] in "abc"}
        if "a" in med and "b" in med:
            entry["b_over_a"] = round(med["b"] / med["a"], 3)
        for k in ("d_lru_fetch_first_pinned", "d_lfu_fetch_first_pinned"):
            if "c" in med and k in res:
                entry["c_over_" + k[:5]] = round(med["c"] / res[k]["median_us"], 3)
        out["batches"]["B=%d" % B] = entry
        del caches
    return out


def kernel_split(path):
    """the library's rows of a rocprofv3 kernel_stats.csv: name, calls, average microseconds, share of the traced time"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "evs::" in r["Name"]:
                rows.append({"kernel": r["Name"][:160], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                             "percent": float(r["Percentage"])})
    return rows


def finish_pair(res, args):
    """the --pair JSON: the profiler's rows folded in (--kernel-stats), written (not for --chain-only) and printed"""
    if args.kernel_stats:
        res["kernel_split"] = {"source": "rocprofv3 --kernel-trace --stats over a --pair --chain-only run (warm-up launches included in the averages)"}
        for item in args.kernel_stats:
            b, path = item.split("=", 1)
            res["kernel_split"][b] = kernel_split(path)
    line = json.dumps(res)
    if not args.chain_only:
        with open(args.out or os.path.join(ROOT, "profiles", "bags_pair.json"), "w") as f:
            f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[2048, 16384])
    ap.add_argument("--policy", nargs="+", default=["lru", "lfu", "evlfu"])
    ap.add_argument("--frac", type=float, default=0.10)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--max-bag", type=int, default=10)
    ap.add_argument("--steps", type=int, default=200, help="timed batches (at least 200 for a figure that is quoted)")
    ap.add_argument("--max-warmup", type=int, default=400)
    ap.add_argument("--max-rows", type=int, default=0, help="clamp every table to this many rows (0: full size)")
    ap.add_argument("--dim", type=int, default=36)
    ap.add_argument("--chain-only", action="store_true", help="warm-up and the chain alone: the run a profiler wraps")
    ap.add_argument("--kernel-stats", nargs="*", default=[], metavar="[POLICY:]B=CSV", help="kernel_stats.csv of a --chain-only profiler run per batch size")
    ap.add_argument("--pair", action="store_true", help="the bag form of the u8 + u4 pair at the flagship shape (see above)")
    ap.add_argument("--pair-batch", type=int, default=16384)
    ap.add_argument("--pair-mean-bag", type=int, default=4)
    ap.add_argument("--pair-timing", default="", metavar="JSON", help="--pair --kernel-stats: fold the profiler's rows into this timing run's JSON "
                    "instead of timing again (no GPU needed)")
    ap.add_argument("--pair-profile", choices=["one", "ragged"], default="one", help="--pair --chain-only: which batches the profiled run draws")
    ap.add_argument("--fetch-first", action="store_true", help="--pair: the pair's fetch-first bag chain beside the order-0 chain over HBM, or "
                    "(with --host-tables) over pinned host tables beside the (B, T) fetch-first pair (see above)")
    ap.add_argument("--host-tables", action="store_true", help="the count-first EvLFU bag chain over HBM and pinned host tables (see above)")
    ap.add_argument("--host-configs", nargs="+", default=["a", "b", "c", "d"], metavar="PREFIX", help="--host-tables: only the configurations whose "
                    "names start so (a configuration alone in its process: the form the parent-commit yardstick is taken in)")
    ap.add_argument("--yardstick", nargs="*", default=[], metavar="NAME=JSON", help="--host-tables: JSON files of `--host-tables --host-configs X` "
                    "runs on the same machine (this tool run from the parent commit's tree for configuration a), folded in under alone[NAME]")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.fetch_first and not args.pair:
        ap.error("--fetch-first is the pair's bag chain: give --pair with it (--host-tables alone is the single-tier bench)")
    if args.pair and args.pair_profile == "ragged" and args.pair_mean_bag < 2:
        ap.error("--pair-profile ragged needs --pair-mean-bag of 2 or more")
    if args.pair and args.fetch_first and args.pair_timing:   # ... of --pair --fetch-first: --kernel-stats NAME=CSV into kernel_split[NAME]
        with open(args.pair_timing) as f:
            res = json.load(f)
        res.setdefault("kernel_split", {"source": "rocprofv3 --kernel-trace --stats over --pair --fetch-first --chain-only runs (warm-up launches "
                                                  "included in the averages)"})
        for item in args.kernel_stats:
            name, path = item.split("=", 1)
            res["kernel_split"][name] = kernel_split(path)
        with open(args.out or args.pair_timing, "w") as f:
            f.write(json.dumps(res) + "\n")
        return
    if args.pair and args.pair_timing:                # fold the profiler's rows into an earlier timing run's JSON: no GPU needed
        with open(args.pair_timing) as f:
            finish_pair(json.load(f), args)
        return
    if not torch.cuda.is_available():
        sys.exit("bags_cache_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ln = [min(n, args.max_rows) if args.max_rows else n for n in bench.KAGGLE_LN]
    if args.pair and args.fetch_first:
        path = args.out or os.path.join(ROOT, "profiles", "bag_pair_fetch_first.json")
        res = {}
        if not args.chain_only and os.path.exists(path):   # the HBM run and the --host-tables run share one file
            with open(path) as f:
                res = json.load(f)
        res.update({"tool": "bags_cache_bench --pair --fetch-first [--host-tables]",
                    "chain": "bags_probe2_kernel -> bags_count2_kernel -> bags_route2_kernel -> cache_batch_sa_list2_kernel -> "
                             "bags_repoint2_kernel -> bags_pool2_kernel -> dense interaction",
                    "device": torch.cuda.get_device_name(0),
                    "shape": {"rows": sum(ln), "dim": args.dim, "zipf_alpha": args.alpha},
                    "timing": "one pair of device events around every call (dispatch gaps included); the compared pairs alternate on the same "
                              "batches in one process; rows fetched = size delta + eviction delta per tier; bus bytes per call = rows fetched x "
                              "the tier's row bytes + (in_place + victim_hits) x [u4, u8] row bytes (lower and upper figure)"})
        res["pinned" if args.host_tables else "hbm"] = run_pair_fetch(ln, dev, args)
        line = json.dumps(res)
        if not args.chain_only:
            with open(path, "w") as f:
                f.write(line + "\n")
        print(line)
        return
    if args.pair:
        res = {"tool": "bags_cache_bench --pair",
               "chain": "bags_probe2_kernel -> bags_count2_kernel -> bags_route2_kernel -> bags_pool2_kernel -> dense interaction -> "
                        "cache_batch_sa_list2_kernel",
               "device": torch.cuda.get_device_name(0),
               "shape": {"rows": sum(ln), "dim": args.dim, "zipf_alpha": args.alpha},
               "timing": "device events around every call, the two forms alternating batch by batch; dispatch gaps included",
               "pair": run_pair(ln, dev, args)}
        finish_pair(res, args)
        return
    if args.host_tables:
        res = {"tool": "bags_cache_bench --host-tables", "device": torch.cuda.get_device_name(0),
               "chains": {"a": "bags_probe_kernel -> bags_pool_kernel (+ counts) -> dense interaction -> bags_raise_list_kernel -> cache_batch_sa_list_kernel",
                          "b": "bags_probe_kernel -> bags_count_kernel -> bags_pool_kernel (pooling alone) -> dense interaction -> bags_raise_list_kernel -> "
                               "cache_batch_sa_list_kernel",
                          "c": "bags_probe_kernel -> bags_count_kernel -> bags_raise_list_kernel -> cache_batch_sa_list_kernel -> sa_repoint_kernel -> "
                               "bags_pool_kernel (pooling alone) -> dense interaction",
                          "d": "bags_probe_kernel -> policy_insert_kernel -> sa_repoint_kernel -> bags_pool_kernel -> dense interaction"},
               "shape": {"frac": args.frac, "dim": args.dim, "zipf_alpha": args.alpha, "bags": "1 .. %d" % args.max_bag},
               "timing": "one pair of device events around every call (dispatch gaps included); the configurations alternate on the same batches "
                         "in one process; bus bytes per call = (size delta + eviction delta + positions served in place) x row bytes",
               "host_tables": run_host(ln, dev, args)}
        for path in args.yardstick:                 # runs of single configurations, each alone in its process: NAME=JSON
            name, path = path.split("=", 1)
            with open(path) as f:
                alone = json.load(f)
            res.setdefault("alone", {})[name] = {k: {c: {m: r[m] for m in ("median_us", "p95_us", "hit_rate")} for c, r in v["configs"].items()}
                                                 for k, v in alone["host_tables"]["batches"].items()}
        if args.kernel_stats:                       # rocprofv3 --kernel-trace --stats over `--host-tables --host-configs X --chain-only` runs: NAME=CSV
            res["kernel_split"] = {"source": "rocprofv3 --kernel-trace --stats over --host-tables --host-configs X --chain-only --batch B runs, one "
                                             "configuration and batch size per run (warm-up launches included in the averages)"}
            for item in args.kernel_stats:
                name, path = item.split("=", 1)
                res["kernel_split"][name] = kernel_split(path)
        if args.chain_only:
            print(json.dumps(res["host_tables"]["batches"]))
            return
        with open(args.out or os.path.join(ROOT, "profiles", "bags_count_first.json"), "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"tool": res["tool"], "batches": {k: {r: v[r] for r in v if r.startswith(("b_over", "c_over"))}
                                                            for k, v in res["host_tables"]["batches"].items()}, "alone": res.get("alone")}))
        return
    ev = bench.make_tables(ln, args.dim, seed=0, device=dev)
    runs = []
    for B in args.batch:
        for p in args.policy:
            runs.append(run(p, B, ev, ln, dev, args))
            print("bags_cache_bench: %s" % json.dumps(runs[-1]), file=sys.stderr, flush=True)
    res = {"tool": "bags_cache_bench", "chain": "bags_probe_kernel -> bags_pool_kernel -> dense interaction -> policy_insert_kernel"
           " (evlfu: ... -> bags_raise_list_kernel -> cache_batch_sa_list_kernel)",
           "shape": {"rows": sum(ln), "frac": args.frac, "dim": args.dim, "zipf_alpha": args.alpha, "bags": "1 .. %d" % args.max_bag},
           "timing": "device events around every call, the chain and the uncached call alternating batch by batch; dispatch gaps included",
           "runs": runs}
    if args.kernel_stats:
        res["kernel_split"] = {"source": "rocprofv3 --kernel-trace --stats over a --chain-only run (warm-up launches included in the averages)"}
        for item in args.kernel_stats:
            b, path = item.split("=", 1)
            policy, b = b.split(":", 1) if ":" in b else ("lru", b)
            res["kernel_split"].setdefault(policy, {})["B=%s" % b] = kernel_split(path)
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
