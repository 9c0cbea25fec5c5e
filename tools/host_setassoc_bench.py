#!/usr/bin/env python3
"""The set-associative cache tier over tables in PINNED HOST memory, in fetch-first order (GpuCache.set_miss_order("fetch-first"):
probe -> update -> sa_repoint -> consumer), beside the only host-memory form there was before it and beside the HBM floor, as ONE
JSON file.

Shape (tools/policy_compare.py's): the Criteo-Kaggle cardinalities, fp32, d = 36, a 10 % tier, B = 16 384, rows Zipf(0.75), the
interaction as the consumer (lookup_interact).  Every configuration is warmed until its size stops growing; then --steps batches
are timed, each call by a pair of device events, the configurations alternating on the SAME batches in one process:
    a  evlfu, `sampled` update, pinned tables        -- the hashed host tier: the yardstick
    b  evlfu, set-associative, fetch-first, pinned tables
    c  lru and lfu, fetch-first, pinned tables
    d  evlfu, set-associative, consume-first, the two-launch chain (set_inline_update(False)), HBM copies -- the floor
Per configuration: median and p95 us per batch, hit rate over the timed batches, the fetch_stats deltas, and the bytes that
crossed the bus per batch = (size delta + eviction delta + positions served in place) x row bytes.  (The hashed tier serves the
positions of a key its update dropped in place as well; it does not count them, so a's figure is a lower bound.)
The verdict is b's median against a's: above 1.10 x it asks for an account by kernel, which comes from a profiler run of its own,
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/host_setassoc_bench.py --chain-only
(--chain-only runs b's warm-up and b's chain alone).  If the machine refuses the 4.86 GB of pinned memory, every table is scaled
by the same factor (halved until the allocation succeeds) and the factor is recorded.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import evstore_dlrm_amd as E  # noqa: E402

CONFIGS = {   # name -> (policy, tables, how the cache is told)
    "a_evlfu_sampled_pinned": ("evlfu", "pinned", lambda c: c.set_batch_policy("sampled")),
    "b_evlfu_setassoc_fetch_first_pinned": ("evlfu", "pinned", lambda c: c.set_miss_order("fetch-first")),
    "c_lru_fetch_first_pinned": ("lru", "pinned", lambda c: c.set_miss_order("fetch-first")),
    "c_lfu_fetch_first_pinned": ("lfu", "pinned", lambda c: c.set_miss_order("fetch-first")),
    "d_evlfu_setassoc_chain_hbm": ("evlfu", "hbm", lambda c: c.set_batch_policy("setassoc").set_inline_update(False)),
}


def pinned_tables(ln, d, scale, dev):
    """-> (ln scaled, the HBM tables, pinned copies of them, scale); halves the scale while pinning fails"""
    while True:
        lns = [max(1, int(n * scale)) for n in ln]
        ev = bench.make_tables(lns, d, seed=0, device=dev)
        try:
            pinned = [ev.fp32_view(k).cpu().pin_memory() for k in range(len(lns))]
            return lns, ev, pinned, scale
        except RuntimeError as e:
            print("host_setassoc_bench: pinning %.2f GB failed (%s); halving every table" % (sum(lns) * d * 4 / 1e9, e), file=sys.stderr, flush=True)
            del ev
            scale *= 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=0.10)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--steps", type=int, default=200, help="timed batches")
    ap.add_argument("--max-warm", type=int, default=150, help="at most this many warm-up batches")
    ap.add_argument("--scale", type=float, default=1.0, help="every table's rows times this")
    ap.add_argument("--dim", type=int, default=36)
    ap.add_argument("--chain-only", action="store_true", help="configuration b alone, untimed (for a profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "host_tier_setassoc.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    d, B = args.dim, args.batch
    ln, ev, pinned, scale = pinned_tables(bench.KAGGLE_LN, d, args.scale, dev)
    T = len(ln)
    cap = int(args.frac * sum(ln))
    n_b = args.max_warm + args.steps
    rows = [b[1].t().contiguous().to(torch.int32) for b in bench.make_batches(ln, B, n_b, seed=3, device=dev, dist="zipf", alpha=args.alpha)]
    x = torch.rand((B, d), device=dev)
    F = T + 1
    out = torch.empty((B, d + F * (F - 1) // 2), device=dev)
    hit = torch.empty((B, T), dtype=torch.uint8, device=dev)
    names = ["b_evlfu_setassoc_fetch_first_pinned"] if args.chain_only else list(CONFIGS)
    caches, warm = {}, {}
    for name in names:
        policy, where, tell = CONFIGS[name]
        c = E.GpuCache(policy, cap, T, d, 32, "python", dev)
        tell(c)
        c.set_backing(pinned if where == "pinned" else ev)
        size = -1
        for i in range(args.max_warm):
            c.lookup_interact(rows[i], x, out=out, hit=hit)
            if i % 10 == 9:
                s = c.batch_stats()["size"]
                if s <= size:
                    break
                size = s
        caches[name], warm[name] = c, i + 1
        print("host_setassoc_bench: %s warm after %d batches, size %d of %d" % (name, i + 1, c.batch_stats()["size"], cap), file=sys.stderr, flush=True)
    timed = rows[args.max_warm:]
    if args.chain_only:
        c = caches[names[0]]
        for r in timed:
            c.lookup_interact(r, x, out=out, hit=hit)
        torch.cuda.synchronize()
        print(json.dumps({"tool": "host_setassoc_bench", "chain_only": names[0], "batches": len(timed), "fetch_stats": c.fetch_stats()}))
        return
    s0 = {n: (caches[n].batch_stats(), caches[n].fetch_stats()) for n in names}
    events = {n: [] for n in names}
    for r in timed:
        for n in names:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            caches[n].lookup_interact(r, x, out=out, hit=hit)
            e1.record()
            events[n].append((e0, e1))
    torch.cuda.synchronize()
    rb = d * 4
    res = {}
    for n in names:
        us = np.array([a.elapsed_time(b) * 1e3 for a, b in events[n]])
        s1, f1 = caches[n].batch_stats(), caches[n].fetch_stats()
        fd = {k: f1[k] - s0[n][1][k] for k in f1}
        fetched = s1["size"] - s0[n][0]["size"] + s1["n_evict"] - s0[n][0]["n_evict"]
        res[n] = {"median_us": round(float(np.median(us)), 2), "p95_us": round(float(np.percentile(us, 95)), 2),
                  "hit_rate": round((s1["n_hits"] - s0[n][0]["n_hits"]) / (T * B * len(timed)), 4), "size": s1["size"],
                  "warm_batches": warm[n], "fetch_stats_delta": fd,
                  "bus_bytes_per_batch": None if CONFIGS[n][1] == "hbm" else round((fetched + fd["in_place"]) * rb / len(timed))}
        print("host_setassoc_bench: %s %s" % (n, res[n]), file=sys.stderr, flush=True)
    a, b = res["a_evlfu_sampled_pinned"]["median_us"], res["b_evlfu_setassoc_fetch_first_pinned"]["median_us"]
    verdict = ("b (set-associative, fetch-first) %.2f us against a (sampled) %.2f us per batch: %.3f x -- " % (b, a, b / a)) + (
        "above 1.10 x: an account by kernel is owed" if b > 1.10 * a else
        "at or below the yardstick" if b <= a else "above the yardstick, within the 1.10 x that asks for no account")
    doc = {"tool": "host_setassoc_bench", "device": torch.cuda.get_device_name(0),
           "shape": {"rows": sum(ln), "table_scale": scale, "capacity": cap, "frac": args.frac, "batch": B, "dim": d, "row_bytes": rb,
                     "zipf_alpha": args.alpha, "timed_batches": len(timed), "pinned_bytes": sum(ln) * rb,
                     "consumer": "lookup_interact (the fused interaction through the address table)"},
           "timing": "one pair of device events around every call; the configurations alternate on the same batches in one process",
           "configs": res, "b_over_a": round(b / a, 3), "verdict": verdict}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"tool": "host_setassoc_bench", "b_over_a": doc["b_over_a"], "verdict": verdict, "out": args.out}))


if __name__ == "__main__":
    main()
