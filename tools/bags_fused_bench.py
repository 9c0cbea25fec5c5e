"""apply_emb_interact_bags (one launch: csrc/evs_fused_bags.hip) against apply_emb_interact (bag_sum_flat / bag_sum_long into a
(T, B, d) block, then the interaction: two launches) on the same seeded multi-hot batches, in one process, alternating the two,
device events around every call, after a warm-up of every shape.  Writes profiles/bags_fused.json (--out).

    python tools/bags_fused_bench.py [--reps 200] [--out profiles/bags_fused.json]

A kernel split (rocprofv3 --kernel-trace --stats -- python tools/bags_fused_bench.py --reps 20 --out /dev/null) belongs in a run of
its own.  A second build of the library (single- against double-buffered stages) is timed by running this tool once per build with
EVS_LIB_PATH set."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evstore_dlrm_amd as E  # noqa: E402

KAGGLE_LN = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593,
             3194, 27, 14992, 5461306, 10, 5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572]
# blocks of 256 threads per CU of each instantiation, from the build's resource report (512 VGPRs per SIMD lane, 160 KiB of LDS per
# CU): (d, nt) -> (VGPRs, LDS bytes per block)
RESOURCES = {(16, 1): (83, 29312), (16, 2): (111, 33152), (32, 1): (87, 34432), (32, 2): (121, 41344),
             (36, 1): (98, 34432), (36, 2): (129, 41344), (64, 1): (95, 44672), (64, 2): (134, 57728)}

SHAPES = [("kaggle_T26_d36_bags1to10_B2048", KAGGLE_LN, 36, 2048, (1, 10)),
          ("kaggle_T26_d36_bags1to10_B16384", KAGGLE_LN, 36, 16384, (1, 10)),
          ("bench_T8_1M_d64_bags100_B2048", [1000000] * 8, 64, 2048, (100, 100))]


def blocks_per_cu(d, T):
    vgprs, lds = RESOURCES[(d, 1 if T + 1 <= 16 else 2)]
    return min(512 // ((vgprs + 7) // 8 * 8), (160 * 1024) // lds)


def batch(ln, B, lo, hi, seed):
    """one seeded batch: per table, bag lengths uniform in [lo, hi] (the reference's random loader), indices uniform over the table"""
    rs = np.random.RandomState(seed)
    lS_o, lS_i = [], []
    for n in ln:
        lens = rs.randint(lo, hi + 1, size=B)
        lS_o.append(torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).cuda())
        lS_i.append(torch.from_numpy(rs.randint(0, n, size=int(lens.sum())).astype(np.int64)).cuda())
    return lS_o, lS_i


def algorithmic_bytes(T, d, B, lookups):
    F = T + 1
    fused = lookups * (4 * d + 8) + T * B * 8 + B * d * 4 + B * (d + F * (F - 1) // 2) * 4
    return {"fused": fused, "two_launch": fused + 2 * T * B * d * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bags_fused.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    torch.manual_seed(0)
    out = {"library": os.path.basename(E._lib.LIB_PATH), "reps": a.reps, "shapes": {}}
    for name, ln, d, B, (lo, hi) in SHAPES:
        T = len(ln)
        ev = E.EVTables.from_fp32([torch.rand((n, d), device="cuda") * 2 - 1 for n in ln])
        data = [(torch.rand((B, d), device="cuda") * 2 - 1,) + batch(ln, B, lo, hi, 100 + k) for k in range(a.batches)]
        calls = {"fused": lambda x, o, i: E.apply_emb_interact_bags(x, o, i, ev),
                 "two_launch": lambda x, o, i: E.apply_emb_interact(x, o, i, ev)}
        for x, o, i in data:   # warm-up of every shape and path; the two paths agree within the interaction's own rounding
            Ra, Rb = calls["fused"](x, o, i), calls["two_launch"](x, o, i)
            torch.testing.assert_close(Ra, Rb, rtol=1e-4, atol=1e-4)
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for r in range(a.reps):
            x, o, i = data[r % len(data)]
            for k in (("fused", "two_launch") if r % 2 == 0 else ("two_launch", "fused")):
                ev0.record()
                calls[k](x, o, i)
                ev1.record()
                ev1.synchronize()
                ms[k].append(ev0.elapsed_time(ev1))
        lookups = int(np.mean([sum(int(t.numel()) for t in i) for _, _, i in data]))
        rec = {"T": T, "d": d, "B": B, "lookups_per_batch": lookups, "blocks_per_cu": blocks_per_cu(d, T),
               "algorithmic_bytes": algorithmic_bytes(T, d, B, lookups)}
        for k, v in ms.items():
            p = np.percentile(v, [10, 50, 90]) * 1000.0
            rec[k + "_us"] = {"p10": round(float(p[0]), 2), "median": round(float(p[1]), 2), "p90": round(float(p[2]), 2)}
        rec["fused_over_two_launch"] = round(rec["fused_us"]["median"] / rec["two_launch_us"]["median"], 3)
        out["shapes"][name] = rec
        print(name, json.dumps(rec), flush=True)
        del ev, data
        torch.cuda.empty_cache()
    out["double_buffered_stage"] = "not measured"
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
