#!/usr/bin/env python3
"""Developer: what an online row update costs at the Kaggle shape (26 tables, d = 36) -> profiles/row_updates.json.

  table     evs_table_update_rows at n = 1 024 / 65 536 / 1 048 576 distinct uniform keys, codec 32 and 8: us per call and
            keys/s, and the yardstick measured in the same run: apply_emb (one index per bag) READING the same number of rows
            of the same tables -- the random-row read this write mirrors.
  cache     evs_cache_update_rows on the 10 % fp32 set-associative tier, and on the u8 + u4 pair with one call per tier: the
            same n, the resident fraction, the ratio to the table-only call.
  steady    the batched tier at B = 16 384: us per batch with no updates, and with a 16 384-key delta applied between
            consecutive batches -- both in this process, alternating.

All times are device events around warmed work of at least --min-s seconds per figure; the calls timed are the C entry
points (the Python wrappers add the de-duplication of the keys, a torch.unique).  No pass thresholds.
--merge-bench parent=FILE branch=FILE records the headline ms_per_step of two bench.py runs made in the same GPU call."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import evstore_dlrm_amd as E  # noqa: E402
from evstore_dlrm_amd import _lib, gpu_cache  # noqa: E402

T, D = 26, 36


def timed(fn, min_s):
    """us per call of fn() by device events: warmed, then repeated until the timed window holds >= min_s of work"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, total_ms, total_n = 8, 0.0, 0
    while True:
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_s * 1e3:
            return ms * 1e3 / reps, reps
        total_ms, total_n = total_ms + ms, total_n + reps
        reps = int(min(max(reps * 2, reps * min_s * 1e3 / max(ms, 1e-3) * 1.2), 4e6))


def uniform_keys(ln, n, n_sets, seed, dev):
    """n_sets sets of n DISTINCT keys, uniform over all rows of all tables -> list of (n, 2) int32 device tensors"""
    g = torch.Generator(device=dev).manual_seed(seed)
    total = int(sum(ln))
    base = torch.tensor(np.concatenate([[0], np.cumsum(ln)]), device=dev, dtype=torch.int64)
    out = []
    for _ in range(n_sets):
        gid = torch.randperm(total, device=dev, generator=g)[:n]
        t = torch.searchsorted(base, gid, right=True) - 1
        out.append(torch.stack([t, gid - base[t]], 1).to(torch.int32).contiguous())
    return out


def stream():
    return torch.cuda.current_stream().cuda_stream


def table_section(evs, ln, sizes, min_s, dev):
    L = _lib.lib()
    out = {}
    for codec, ev in evs.items():
        for n in sizes:
            sets = uniform_keys(ln, n, 4, 100 + n % 97, dev)
            vals = torch.empty((n, D), device=dev).uniform_(-0.05, 0.05)
            it = [0]

            def upd():
                k = sets[it[0] % len(sets)]
                it[0] += 1
                _lib.check(L.evs_table_update_rows(codec, D, T, ev._tables_c, ev._n_rows_c, n, k.data_ptr(), vals.data_ptr(), D, stream()))

            us, reps = timed(upd, min_s)
            # the yardstick: apply_emb, one index per bag, reading as many rows of the same tables
            B = max(n // T, 1)
            bs = bench.make_batches(ln, B, 4, seed=7, device=dev)
            buf = torch.empty((T, B, D), device=dev)

            def read():
                off, idx = bs[it[0] % len(bs)]
                it[0] += 1
                E.apply_emb(off, idx, ev, lazy=False, one_index_per_bag=True, _into=buf)

            us_r, reps_r = timed(read, min_s)
            out["codec%d_n%d" % (codec, n)] = {
                "us_per_call": us, "keys_per_s": n / us * 1e6, "calls_timed": reps,
                "apply_emb_read": {"rows": B * T, "us_per_call": us_r, "rows_per_s": B * T / us_r * 1e6, "calls_timed": reps_r},
                "write_over_read_per_row": (us / n) / (us_r / (B * T))}
            print("table codec %2d n %7d: %9.2f us/call %8.1f M keys/s | read %9.2f us for %d rows" % (codec, n, us, n / us, us_r, B * T), flush=True)
    return out


def cache_calls(L, caches, n, sets, vals):
    it = [0]

    def upd():
        k = sets[it[0] % len(sets)]
        it[0] += 1
        for c in caches:
            _lib.check(L.evs_cache_update_rows(c._h, n, k.data_ptr(), vals.data_ptr(), D, None, stream()))
    return upd


def cache_section(evs, ln, sizes, min_s, dev, table, fill):
    L = _lib.lib()
    out = {}
    B = 16384
    bs = bench.make_batches(ln, B, fill, seed=21, device=dev, dist="zipf", alpha=0.75)
    rq = [b[1].t().contiguous().to(torch.int32) for b in bs]
    del bs
    x = torch.rand((B, D), device=dev)
    # the 10 % fp32 set-associative tier
    c = E.GpuCache("evlfu", int(0.10 * sum(ln)), T, D, 32, "python", dev).set_batch_policy("setassoc")
    c.set_backing(evs[32])
    for r in rq:
        c.lookup_interact(r, x)
    # the u8 + u4 pair (the reference's 48-48-4 split of 2 % of the rows), warmed together
    ev8, ev4 = evs[8], evs[4]
    budget = int(0.02 * sum(ln))
    c1 = E.GpuCache("evlfu", int(0.48 * budget) * 4, T, D, 8, "cpp", dev)
    c2 = E.GpuCache("evlfu", int(0.48 * budget) * 8, T, D, 4, "cpp", dev)
    c1.set_backing(ev8)
    c2.set_backing(ev4)
    tier = torch.empty((B, T), dtype=torch.uint8, device=dev)
    for r in rq:
        gpu_cache.lookup_interact_c1c2(c1, c2, r, x, tier=tier, fused=True)
    out["fp32_tier_entries"] = c.batch_stats()["size"]
    out["pair_entries"] = [c1.batch_stats()["size"], c2.batch_stats()["size"]]
    for n in sizes:
        sets = uniform_keys(ln, n, 4, 300 + n % 97, dev)
        vals = torch.empty((n, D), device=dev).uniform_(-0.05, 0.05)
        res = c.update_rows(sets[0], vals, count=True)
        us, reps = timed(cache_calls(L, [c], n, sets, vals), min_s)
        t_us = table["codec32_n%d" % n]["us_per_call"]
        out["fp32_setassoc_n%d" % n] = {"us_per_call": us, "keys_per_s": n / us * 1e6, "resident_fraction": res / n,
                                       "ratio_to_table_only": us / t_us, "calls_timed": reps}
        print("cache fp32 10%% setassoc n %7d: %9.2f us/call, resident %.3f, x%.2f of the table-only call" % (n, us, res / n, us / t_us), flush=True)
        r1, r2 = c1.update_rows(sets[0], vals, count=True), c2.update_rows(sets[0], vals, count=True)
        us, reps = timed(cache_calls(L, [c1, c2], n, sets, vals), min_s)
        # the table-only counterpart of the pair: the same delta into a u8 and a u4 table set
        it = [0]

        def two_tables():
            k = sets[it[0] % len(sets)]
            it[0] += 1
            for codec, ev in ((8, ev8), (4, ev4)):
                _lib.check(L.evs_table_update_rows(codec, D, T, ev._tables_c, ev._n_rows_c, n, k.data_ptr(), vals.data_ptr(), D, stream()))

        t2_us, _ = timed(two_tables, min_s)
        out["u8_u4_pair_n%d" % n] = {"us_per_delta": us, "keys_per_s": n / us * 1e6, "resident_fraction": [r1 / n, r2 / n],
                                    "table_only_us": t2_us, "ratio_to_table_only": us / t2_us, "calls_timed": reps}
        print("cache u8+u4 pair        n %7d: %9.2f us/delta, resident %.3f + %.3f, x%.2f of the two table-only calls" % (n, us, r1 / n, r2 / n, us / t2_us), flush=True)
    return out, c, rq, x


def steady_section(c, ln, rq, x, min_s, dev):
    """the 10 % fp32 tier at B = 16 384: blocks of batches without and with a 16 384-key delta in front of every batch,
    alternating in one process"""
    L = _lib.lib()
    B, n = 16384, 16384
    sets = uniform_keys(ln, n, 8, 555, dev)
    # the delta a serving loop would see: the keys its traffic asks for (Zipf) -- de-duplicated, padded with uniform keys
    hot = []
    for r in rq[:8]:
        k = torch.stack([torch.arange(T, device=dev, dtype=torch.int32).repeat(B), r.reshape(-1)], 1)
        k = torch.unique(k[torch.randperm(k.shape[0], device=dev)[:4 * n]], dim=0)[:n]
        hot.append(k.contiguous() if k.shape[0] == n else None)
    vals = torch.empty((n, D), device=dev).uniform_(-0.05, 0.05)
    hit = torch.empty((B, T), dtype=torch.uint8, device=dev)
    R = torch.empty((B, D + (T + 1) * T // 2), device=dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    tot = {"none": [0.0, 0], "uniform_delta": [0.0, 0], "traffic_delta": [0.0, 0]}
    block, i = 25, 0
    for r in rq[:20]:
        c.lookup_interact(r, x, out=R, hit=hit)
    torch.cuda.synchronize()
    modes = ["none", "uniform_delta"] + (["traffic_delta"] if all(h is not None for h in hot) else [])
    while min(tot[m][0] for m in modes) < min_s * 1e3:
        for mode in modes:
            a.record()
            for _ in range(block):
                if mode != "none":
                    k = (sets if mode == "uniform_delta" else hot)[i % 8]
                    _lib.check(L.evs_cache_update_rows(c._h, n, k.data_ptr(), vals.data_ptr(), D, None, stream()))
                c.lookup_interact(rq[i % len(rq)], x, out=R, hit=hit)
                i += 1
            b.record()
            torch.cuda.synchronize()
            tot[mode][0] += a.elapsed_time(b)
            tot[mode][1] += block
    out = {"batch": B, "delta_keys": n}
    for m in modes:
        out["us_per_batch_" + m] = tot[m][0] * 1e3 / tot[m][1]
        out["batches_timed_" + m] = tot[m][1]
    out["resident_fraction_uniform"] = c.update_rows(sets[0], vals, count=True) / n
    if "traffic_delta" in modes:
        out["resident_fraction_traffic"] = c.update_rows(hot[0], vals, count=True) / n
    print("steady state B 16384: " + ", ".join("%s %.2f us" % (m, out["us_per_batch_" + m]) for m in modes), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "row_updates.json"))
    ap.add_argument("--min-s", type=float, default=0.5, help="device time per figure, at least")
    ap.add_argument("--sizes", default="1024,65536,1048576")
    ap.add_argument("--fill", type=int, default=120, help="Zipf batches that warm the tiers")
    ap.add_argument("--merge-bench", nargs="*", default=[], metavar="NAME=FILE")
    args = ap.parse_args()
    res = {}
    if os.path.exists(args.out):
        try:
            res = json.load(open(args.out))
        except ValueError:
            res = {}
    if args.merge_bench:
        hl = {}
        for item in args.merge_bench:
            name, path = item.split("=", 1)
            line = [ln for ln in open(path).read().splitlines() if ln.startswith("{")][-1]
            j = json.loads(line)
            hl[name] = {"ms_per_step": j["ms_per_step"], "value": j["value"], "unit": j.get("unit")}
        res["bench_headline_same_gpu_call"] = hl
        json.dump(res, open(args.out, "w"), indent=1)
        print(json.dumps(hl))
        return
    assert torch.cuda.is_available(), "row_update_bench needs the GPU: it has no other way to produce a time"
    dev = torch.device("cuda")
    ln = bench.KAGGLE_LN
    sizes = [int(s) for s in args.sizes.split(",")]
    ev = bench.make_tables(ln, D)
    evs = {32: ev, 8: ev.encode(8), 4: ev.encode(4)}
    res.update({"shape": {"tables": T, "d": D, "rows": int(sum(ln))}, "min_seconds_per_figure": args.min_s,
                "device": torch.cuda.get_device_name(0)})
    res["table_update_rows"] = table_section({32: evs[32], 8: evs[8]}, ln, sizes, args.min_s, dev)
    # (the u4 table-only figures the pair's ratio needs are taken inside the cache section)
    res["cache_update_rows"], c, rq, x = cache_section(evs, ln, sizes, args.min_s, dev, res["table_update_rows"], args.fill)
    res["batched_steady_state"] = steady_section(c, ln, rq, x, args.min_s, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote " + args.out)


if __name__ == "__main__":
    main()
