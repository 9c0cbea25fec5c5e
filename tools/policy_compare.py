"""EvLFU, LRU and LFU side by side on the set-associative cache tier: one Zipf stream through three tiers of the same shape,
hit rate and event-timed microseconds per batch for each, as ONE JSON line.

All three run the same separate-launch chain in this process -- probe, interaction consumer, insert / update as launches of
their own (EvLFU: EVS_CACHE_FOLD=0 and set_inline_update(False); LRU / LFU have no other form) -- so the figures compare the
policies, not the launch structure: per key one set line, at most one compare-and-swap, one row copy per new key.  EvLFU's
folded one-launch form is what bench.py measures.

Default: the bench's cache shape (10 % of the Criteo-Kaggle rows, B = 16 384, Zipf 0.75, 60 fill batches, then batches the
tiers have not seen).  Smaller: --max-rows clamps every table, --batch / --steps / --warmup as usual.  Hit rates are taken
over --cmp batches behind the fill and reported beside the sequential oracle's on the same history (--no-oracle skips it).

    python tools/policy_compare.py [--max-rows 200000 --batch 2048 --steps 50]"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("EVS_CACHE_FOLD", "0")   # read once by the library: EvLFU's probe as a launch of its own, like the others'
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
import evstore_dlrm_amd as E

POLICIES = ("evlfu", "lru", "lfu")


def make_cache(policy, cap, T, d, ev, dev):
    c = E.GpuCache(policy, cap, T, d, 32, "python", dev)
    if policy == "evlfu":
        c.set_batch_policy("setassoc").set_inline_update(False)
    c.set_backing(ev)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=0.10)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--cmp", type=int, default=10, help="batches behind the fill on which the hit rates are taken")
    ap.add_argument("--steps", type=int, default=200, help="timed batches")
    ap.add_argument("--rounds", type=int, default=2, help="timed regions per policy (fresh tier each, policies interleaved)")
    ap.add_argument("--max-rows", type=int, default=0, help="clamp every table to this many rows (0: full size)")
    ap.add_argument("--dim", type=int, default=36)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ln = [min(n, args.max_rows) if args.max_rows else n for n in bench.KAGGLE_LN]
    T, d, B = len(ln), args.dim, args.batch
    cap = int(args.frac * sum(ln))
    ev = bench.make_tables(ln, d, seed=0, device=dev)
    n_b = args.warmup + args.cmp + args.steps
    rows = [b[1].t().contiguous().to(torch.int32) for b in bench.make_batches(ln, B, n_b, seed=3, device=dev, dist="zipf", alpha=args.alpha)]
    x = torch.rand((B, d), device=dev)
    F = T + 1
    out = torch.empty((B, d + F * (F - 1) // 2), device=dev)
    hit = torch.empty((B, T), dtype=torch.uint8, device=dev)
    res = {p: {"us_per_batch": []} for p in POLICIES}
    for rnd in range(args.rounds):
        for p in POLICIES:
            c = make_cache(p, cap, T, d, ev, dev)
            for i in range(args.warmup):
                c.lookup_interact(rows[i], x, out=out, hit=hit)
            s0 = c.batch_stats()
            for i in range(args.cmp):
                c.lookup_interact(rows[args.warmup + i], x, out=out, hit=hit)
            s1 = c.batch_stats()
            if rnd == 0 and args.cmp:
                res[p]["hit_rate"] = (s1["n_hits"] - s0["n_hits"]) / (T * B * args.cmp)
            # clock settle on a scratch tier of the same kind (bench.cache_tier_section does the same)
            scratch = make_cache(p, cap, T, d, ev, dev)
            t_s = time.perf_counter()
            while time.perf_counter() - t_s < 0.35:
                for i in range(20):
                    scratch.lookup_interact(rows[i % args.warmup], x, out=out, hit=hit)
                torch.cuda.synchronize()
            del scratch
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for i in range(args.steps):
                c.lookup_interact(rows[args.warmup + args.cmp + i], x, out=out, hit=hit)
            e1.record()
            torch.cuda.synchronize()
            s2 = c.batch_stats()
            res[p]["us_per_batch"].append(round(e0.elapsed_time(e1) / args.steps * 1e3, 2))
            print("policy_compare: round %d %s %.2f us per batch" % (rnd, p, res[p]["us_per_batch"][-1]), file=sys.stderr, flush=True)
            if rnd == 0:
                res[p]["hit_rate_timed"] = (s2["n_hits"] - s1["n_hits"]) / (T * B * args.steps)
                res[p]["size"] = s2["size"]
            del c
    base = min(res["evlfu"]["us_per_batch"])
    for p in POLICIES:
        res[p]["ratio_to_evlfu_chain"] = round(min(res[p]["us_per_batch"]) / base, 3)
    if not args.no_oracle and args.cmp:
        from oracle import oracle as orc
        tabs = [ev.fp32_view(k).cpu().numpy() for k in range(T)]
        host_rows = [r.cpu().numpy() for r in rows[:args.warmup + args.cmp]]
        for p in POLICIES:
            t0 = time.perf_counter()
            o = orc.EvLFU(cap, tabs, d, "python") if p == "evlfu" else (orc.LRU if p == "lru" else orc.LFU)(cap, tabs, d)
            oh = 0
            for i, rq in enumerate(host_rows):
                for q in rq:
                    h = o.request(q)[0]
                    if i >= args.warmup:
                        oh += int(h.sum())
            res[p]["oracle_hit_rate"] = oh / (T * B * args.cmp)
            res[p]["oracle_seconds"] = round(time.perf_counter() - t0, 1)
            print("policy_compare: sequential oracle %s %.4f (%.0f s)" % (p, res[p]["oracle_hit_rate"], res[p]["oracle_seconds"]), file=sys.stderr, flush=True)
            del o
    print(json.dumps({"tool": "policy_compare", "chain": "probe -> consumer -> insert, separate launches (EVS_CACHE_FOLD=0, inline update off)",
                      "shape": {"rows": sum(ln), "capacity": cap, "frac": args.frac, "batch": B, "dim": d, "zipf_alpha": args.alpha,
                                "fill_batches": args.warmup, "hit_rate_batches": args.cmp, "timed_batches": args.steps},
                      "policies": res}))


if __name__ == "__main__":
    main()
