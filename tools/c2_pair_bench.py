#!/usr/bin/env python3
"""Developer: the two-tier (configs[4] pair: u8 C1 + u4 C2, the reference's 48-48-4 split of 2 % of the rows) batched lookup +
interaction ALONE -- 180 batches fill both tiers, then argv[1] (default 200) unseen batches at capacity, per-batch stream time
by HIP events.  The profile target of tools/prof_r06.sh: every dispatch of the two kernels behind the fill is a steady-state one.
argv[2] = 3: with the alt-key tier (three tiers).

--fetch-first [--steps N] [--out FILE]: the fetch-first pair (both tiers set_miss_order("fetch-first"): probe -> the pair's update ->
sa_repoint2 -> consumer) beside the forms there were before it, at the same shape, as ONE JSON file (profiles/pair_fetch_first.json).
Every pair is filled by the same 180 batches; then N (default 200) unseen batches are timed, each call by a pair of device events, the
four pairs alternating on the SAME batches in one process:
    a  the hashed `sampled` pair over pinned tables           -- the only host-memory form of the pair before: the yardstick
    b  the fetch-first pair over pinned tables
    c  the fetch-first pair over HBM
    d  the set-associative pair, consume first, over HBM, with EVS_CACHE_FOLD2=0 (the unfolded probe: c's twin)   -- c's yardstick
Per pair: median and p95 us per batch, the hit rate over the timed batches, the three re-point totals per batch, and the bytes that
crossed the bus per batch = per tier (size delta + eviction delta) x its row bytes, + the positions served in place (misses left in
place and hits whose way was taken) x C1's row bytes, the larger of the two.  (The hashed pair serves positions in place as well and
does not count them: a's figure is a lower bound.)  b above 1.10 x a, or c above 1.10 x d, asks for an account by kernel."""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FETCH_FIRST = "--fetch-first" in sys.argv
if FETCH_FIRST:
    os.environ["EVS_CACHE_FOLD2"] = "0"   # (read once per process, at the first pair call: only d would fold)
import numpy as np
import torch
import bench
import evstore_dlrm_amd as E
from evstore_dlrm_amd import gpu_cache

dev = torch.device("cuda")
ln, d, T, B = bench.KAGGLE_LN, 36, 26, 16384


def fetch_first_leg():
    import argparse
    import json
    ap = argparse.ArgumentParser()
    ap.add_argument("--fetch-first", action="store_true")
    ap.add_argument("--steps", type=int, default=200, help="timed batches")
    ap.add_argument("--fill", type=int, default=180, help="batches that fill the tiers")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_fetch_first.json"))
    ap.add_argument("--chain-only", default=None, metavar="NAME", help="this pair alone, filled and then run untimed (for a profiler run)")
    args = ap.parse_args()
    ev = bench.make_tables(ln, d)
    ev8, ev4 = ev.encode(8), ev.encode(4)
    del ev
    pin8, pin4 = [t.cpu().pin_memory() for t in ev8.raw], [t.cpu().pin_memory() for t in ev4.raw]
    budget = int(0.02 * sum(ln))
    caps = (int(0.48 * budget) * 4, int(0.48 * budget) * 8)
    configs = {   # name -> (tables, how a tier is told)
        "a_sampled_pinned": ("pinned", lambda c: c.set_batch_policy("sampled")),
        "b_fetch_first_pinned": ("pinned", lambda c: c.set_miss_order("fetch-first")),
        "c_fetch_first_hbm": ("hbm", lambda c: c.set_miss_order("fetch-first")),
        "d_setassoc_unfolded_hbm": ("hbm", lambda c: c.set_batch_policy("setassoc")),
    }
    tier = torch.empty((B, T), dtype=torch.uint8, device=dev)
    x = torch.rand((B, d), device=dev)
    rq = [b[1].t().contiguous().to(torch.int32) for b in bench.make_batches(ln, B, args.fill + args.steps, seed=21, device=dev, dist="zipf", alpha=0.75)]
    pairs = {}
    if args.chain_only:
        configs = {args.chain_only: configs[args.chain_only]}
    for name, (where, tell) in configs.items():
        c1, c2 = E.GpuCache("evlfu", caps[0], T, d, 8, "cpp", dev), E.GpuCache("evlfu", caps[1], T, d, 4, "cpp", dev)
        tell(c1); tell(c2)
        c1.set_backing(pin8 if where == "pinned" else ev8); c2.set_backing(pin4 if where == "pinned" else ev4)
        for r in rq[:args.fill]:
            gpu_cache.lookup_interact_c1c2(c1, c2, r, x, tier=tier, fused=True)
        pairs[name] = (c1, c2)
        print("c2_pair_bench: %s filled, C1 %d C2 %d resident" % (name, c1.batch_stats()["size"], c2.batch_stats()["size"]), file=sys.stderr, flush=True)
    timed = rq[args.fill:]
    if args.chain_only:
        c1, c2 = pairs[args.chain_only]
        for r in timed:
            gpu_cache.lookup_interact_c1c2(c1, c2, r, x, tier=tier, fused=True)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "c2_pair_bench --fetch-first", "chain_only": args.chain_only, "batches": len(timed), "fetch_stats": c1.fetch_stats()}))
        return
    s0 = {n: (p[0].batch_stats(), p[1].batch_stats(), p[0].fetch_stats()) for n, p in pairs.items()}
    events = {n: [] for n in pairs}
    for r in timed:
        for n, (c1, c2) in pairs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gpu_cache.lookup_interact_c1c2(c1, c2, r, x, tier=tier, fused=True)
            e1.record()
            events[n].append((e0, e1))
    torch.cuda.synchronize()
    rb = (d, d // 2)
    res = {}
    for n, (c1, c2) in pairs.items():
        us = np.array([a.elapsed_time(b) * 1e3 for a, b in events[n]])
        s1 = (c1.batch_stats(), c2.batch_stats(), c1.fetch_stats())
        fd = {k: (s1[2][k] - s0[n][2].get(k, 0)) / len(timed) for k in s1[2] if k != "calls"}
        fetched = sum((s1[k]["size"] - s0[n][k]["size"] + s1[k]["n_evict"] - s0[n][k]["n_evict"]) * rb[k] for k in (0, 1))
        in_place = (fd.get("in_place", 0) + fd.get("victim_hits", 0)) * rb[0]
        res[n] = {"median_us": round(float(np.median(us)), 2), "p95_us": round(float(np.percentile(us, 95)), 2),
                  "hit_rate": round(sum(s1[k]["n_hits"] - s0[n][k]["n_hits"] for k in (0, 1)) / (T * B * len(timed)), 4),
                  "size": (s1[0]["size"], s1[1]["size"]), "repoint_per_batch": {k: round(v, 2) for k, v in fd.items()},
                  "bus_bytes_per_batch": None if configs[n][0] == "hbm" else round(fetched / len(timed) + in_place)}
        print("c2_pair_bench: %s %s" % (n, res[n]), file=sys.stderr, flush=True)
    ba = res["b_fetch_first_pinned"]["median_us"] / res["a_sampled_pinned"]["median_us"]
    cd = res["c_fetch_first_hbm"]["median_us"] / res["d_setassoc_unfolded_hbm"]["median_us"]
    verdict = "b / a = %.3f, c / d = %.3f: %s" % (ba, cd, "an account by kernel is owed" if ba > 1.10 or cd > 1.10 else "within the 1.10 x that asks for no account")
    doc = {"tool": "c2_pair_bench --fetch-first", "device": torch.cuda.get_device_name(0),
           "shape": {"rows": sum(ln), "capacities": caps, "codecs": (8, 4), "batch": B, "dim": d, "zipf_alpha": 0.75, "fill_batches": args.fill,
                     "timed_batches": len(timed), "pinned_bytes": sum(ln) * (rb[0] + rb[1]), "consumer": "lookup_interact_c1c2"},
           "timing": "one pair of device events around every call; the four pairs alternate on the same batches in one process; EVS_CACHE_FOLD2=0",
           "configs": res, "b_over_a": round(ba, 3), "c_over_d": round(cd, 3), "verdict": verdict}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"tool": "c2_pair_bench --fetch-first", "b_over_a": doc["b_over_a"], "c_over_d": doc["c_over_d"], "verdict": verdict, "out": args.out}))


if FETCH_FIRST:
    fetch_first_leg()
    sys.exit(0)

n_timed = int(sys.argv[1]) if len(sys.argv) > 1 else 200
tiers = int(sys.argv[2]) if len(sys.argv) > 2 else 2
ev = bench.make_tables(ln, d)
ev8, ev4 = ev.encode(8), ev.encode(4)
budget = int(0.02 * sum(ln))
c1 = E.GpuCache("evlfu", int(0.48 * budget) * 4, T, d, 8, "cpp", dev)
c2 = E.GpuCache("evlfu", int(0.48 * budget) * 8, T, d, 4, "cpp", dev)
c1.set_backing(ev8); c2.set_backing(ev4)
c3 = None
if tiers == 3:
    alt = [torch.from_numpy(((np.arange(n, dtype=np.int64) % min(n, 4096)) * 100 + (t + 1)).astype(np.uint32).view(np.int32)).to(dev)
           for t, n in enumerate(ln)]
    c3 = E.GpuAltKeyTier(int(0.04 * budget) * 8 + 64, alt, dev)
tier = torch.empty((B, T), dtype=torch.uint8, device=dev)
x = torch.rand((B, d), device=dev)
P = (T + 1) * T // 2
R = torch.empty((B, d + P), device=dev)
n_fill = 180
bs = bench.make_batches(ln, B, n_fill + n_timed, seed=21, device=dev, dist="zipf", alpha=0.75)
rq = [b[1].t().contiguous().to(torch.int32) for b in bs]
del bs


def step(r):
    if c3 is None:
        gpu_cache.lookup_interact_c1c2(c1, c2, r, x, tier=tier, fused=True)
    else:
        gpu_cache.lookup_interact_c1c2c3(c1, c2, c3, r, x, tier=tier)


for r in rq[:n_fill]:
    step(r)
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record(); b.record()
torch.cuda.synchronize()
t0 = time.perf_counter()
a.record()
for r in rq[n_fill:]:
    step(r)
b.record()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("%d-tier batched + interaction: %.2f us per batch by events, %.2f wall (%d unseen batches at capacity); C1 %d C2 %d resident"
      % (tiers, a.elapsed_time(b) / n_timed * 1e3, dt / n_timed * 1e6, n_timed, c1.batch_stats()["size"], c2.batch_stats()["size"]))
