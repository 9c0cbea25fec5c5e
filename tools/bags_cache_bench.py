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


def kernel_split(path):
    """the library's rows of a rocprofv3 kernel_stats.csv: name, calls, average microseconds, share of the traced time"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "evs::" in r["Name"]:
                rows.append({"kernel": r["Name"][:160], "calls": int(r["Calls"]), "avg_us": round(float(r["AverageNs"]) / 1e3, 2),
                             "percent": float(r["Percentage"])})
    return rows


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
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bags_cache_bench: needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ln = [min(n, args.max_rows) if args.max_rows else n for n in bench.KAGGLE_LN]
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
