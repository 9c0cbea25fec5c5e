#!/usr/bin/env python3
"""The approximate-embedding mode of the batched set-associative EvLFU tier (GpuCache.set_batch_approx) on the bench's cache
shape, as ONE JSON file: what the new probe costs when it approximates nothing, and what the mode saves when it does.

Shape (tools/host_setassoc_bench.py's): the Criteo-Kaggle cardinalities, fp32, d = 36, a 10 % tier, B = 16 384, rows
Zipf(0.75), the interaction as the consumer (lookup_interact).  Three placements, each measured on its own:
    pinned           fetch-first over tables in pinned host memory (probe -> update -> sa_repoint -> consumer)
    hbm              consume-first over tables in HBM (probe -> consumer -> update); with the threshold off this chain folds
                     the probe into the consumer and hands it 4-byte row ids, with a threshold on it does neither, so b against
                     a is here the price of the unfolded pointer-mode chain AND of the new probe
    hbm_fetch_first  fetch-first over tables in HBM: unfolded and in pointer mode with or without a threshold, so b against a
                     is the new probe against the old one and nothing else, at a call short enough to show it
and in each four caches that see the SAME batches, alternating call by call in one process:
    a, a2   threshold off, set_inline_update(False): the chain as it was before the mode existed, twice -- the A/A spread
    b       thres = T: the new probe, approximating nothing
    c       thres = T - 3
Every cache is warmed until its size stops growing; then --steps batches are timed, each call by a pair of device events.
Per cache: median and p95 us per batch, the hit rate (true hits) over the timed batches, the approx_stats and fetch_stats
deltas, and for c the rows per batch that did not cross the bus (pinned) / were not read from the table (hbm) -- the
approximated positions.  The verdict per placement is b's median against a's beside |a2 - a| / a: above 1.10 x it asks for an
account.  If the machine refuses the 4.86 GB of pinned memory every table is scaled by the same factor (halved until the
allocation succeeds) and the factor is recorded.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import evstore_dlrm_amd as E  # noqa: E402
from host_setassoc_bench import pinned_tables  # noqa: E402

MODES = ("a", "a2", "b", "c")


def run_placement(where, tables, ln, cap, d, rows, x, out, hit, args, dev):
    T = len(ln)
    thres = {"a": 0, "a2": 0, "b": T, "c": T - 3}
    caches, warm = {}, {}
    for m in MODES:
        c = E.GpuCache("evlfu", cap, T, d, 32, "python", dev)
        if where in ("pinned", "hbm_fetch_first"):
            c.set_miss_order("fetch-first")
        else:
            c.set_batch_policy("setassoc")
        c.set_inline_update(False).set_batch_approx(thres[m])
        c.set_backing(tables)
        size = -1
        for i in range(args.max_warm):
            c.lookup_interact(rows[i], x, out=out, hit=hit)
            if i % 10 == 9:
                s = c.batch_stats()["size"]
                if s <= size:
                    break
                size = s
        caches[m], warm[m] = c, i + 1
        print("batch_approx_bench: %s/%s warm after %d batches, size %d of %d" % (where, m, i + 1, c.batch_stats()["size"], cap), file=sys.stderr, flush=True)
    timed = rows[args.max_warm:]
    s0 = {m: (caches[m].batch_stats(), caches[m].fetch_stats(), caches[m].approx_stats()) for m in MODES}
    events = {m: [] for m in MODES}
    for r in timed:
        for m in MODES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            caches[m].lookup_interact(r, x, out=out, hit=hit)
            e1.record()
            events[m].append((e0, e1))
    torch.cuda.synchronize()
    n = len(timed)
    res = {}
    for m in MODES:
        us = np.array([a.elapsed_time(b) * 1e3 for a, b in events[m]])
        s1, f1, a1 = caches[m].batch_stats(), caches[m].fetch_stats(), caches[m].approx_stats()
        fd = {k: f1[k] - s0[m][1][k] for k in f1}
        ad = {k: a1[k] - s0[m][2][k] for k in a1}
        hits = s1["n_hits"] - s0[m][0]["n_hits"]
        inserted = s1["size"] - s0[m][0]["size"] + s1["n_evict"] - s0[m][0]["n_evict"]
        res[m] = {"threshold": thres[m], "median_us": round(float(np.median(us)), 2), "p95_us": round(float(np.percentile(us, 95)), 2),
                  "hit_rate": round(hits / (T * B_of(rows) * n), 4), "size": s1["size"], "warm_batches": warm[m],
                  "approx_stats_delta": ad, "fetch_stats_delta": fd, "rows_inserted_per_batch": round(inserted / n, 1),
                  "samples_approximated_per_batch": round(ad["samples"] / n, 1),
                  "rows_not_fetched_per_batch": round((ad["substituted"] + ad["zero_rows"]) / n, 1),
                  "positions_not_hit_per_batch": round((T * B_of(rows) * n - hits) / n, 1)}
        print("batch_approx_bench: %s/%s %s" % (where, m, res[m]), file=sys.stderr, flush=True)
    a, a2, b, c = (res[m]["median_us"] for m in MODES)
    spread = abs(a2 - a) / a
    verdict = ("b (thres = T) %.2f us against a (off) %.2f us per batch: %.3f x, A/A spread %.3f -- " % (b, a, b / a, spread)) + (
        "above 1.10 x: an account is owed" if b > 1.10 * a else "held: within the 1.10 x that asks for no account")
    return {"configs": res, "b_over_a": round(b / a, 3), "a2_over_a": round(a2 / a, 3), "c_over_a": round(c / a, 3), "verdict": verdict}


def B_of(rows):
    return int(rows[0].shape[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frac", type=float, default=0.10)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--steps", type=int, default=200, help="timed batches")
    ap.add_argument("--max-warm", type=int, default=150, help="at most this many warm-up batches")
    ap.add_argument("--scale", type=float, default=1.0, help="every table's rows times this")
    ap.add_argument("--dim", type=int, default=36)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_approx.json"))
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
    placements = {}
    for where, tables in (("pinned", pinned), ("hbm", ev), ("hbm_fetch_first", ev)):
        placements[where] = run_placement(where, tables, ln, cap, d, rows, x, out, hit, args, dev)
        torch.cuda.empty_cache()
    doc = {"tool": "batch_approx_bench", "device": torch.cuda.get_device_name(0),
           "shape": {"rows": sum(ln), "table_scale": scale, "capacity": cap, "frac": args.frac, "batch": B, "dim": d, "row_bytes": d * 4,
                     "n_tables": T, "zipf_alpha": args.alpha, "timed_batches": args.steps, "pinned_bytes": sum(ln) * d * 4,
                     "consumer": "lookup_interact (the fused interaction through the address table)"},
           "modes": {"a": "threshold off, set_inline_update(False)", "a2": "the same again (A/A)", "b": "thres = T: the new probe, nothing approximated",
                     "c": "thres = T - 3"},
           "timing": "one pair of device events around every call; the four caches alternate on the same batches in one process",
           "placements": placements}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"tool": "batch_approx_bench", "out": args.out,
                      **{w: {"b_over_a": p["b_over_a"], "a2_over_a": p["a2_over_a"], "c_over_a": p["c_over_a"], "verdict": p["verdict"]} for w, p in placements.items()}}))


if __name__ == "__main__":
    main()
