"""apply_emb_long (csrc/evs_gather_longq.hip: K raw rows of a bag in flight per lane, decode after arrival) against
apply_emb(..., lazy=False) -- the grid-stride vec kernel, what multi-hot batches over u16 / u8 / u4 tables run on by default -- on
the same seeded multi-hot batches, per codec, in one process, alternating the two, device events around every call, after a
warm-up of every shape that also compares the two outputs as bits.  The routes are confirmed from the two dispatch records.
Writes profiles/long_q.json (--out).

    python tools/long_q_bench.py [--reps 200] [--out profiles/long_q.json]

A kernel split (rocprofv3 --kernel-trace --stats -- python tools/long_q_bench.py --reps 20 --out /dev/null) belongs in a run of
its own."""
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

SHAPES = [("bench_T8_1M_d64_bags100_B2048", [1000000] * 8, 64, 2048, (100, 100)),
          ("kaggle_T26_d36_bags1to10_B2048", KAGGLE_LN, 36, 2048, (1, 10)),
          ("kaggle_T26_d36_bags1to10_B16384", KAGGLE_LN, 36, 16384, (1, 10))]


def batch(ln, B, lo, hi, seed):
    """one seeded batch: per table, bag lengths uniform in [lo, hi] (the reference's random loader), indices uniform over the table"""
    rs = np.random.RandomState(seed)
    lS_o, lS_i = [], []
    for n in ln:
        lens = rs.randint(lo, hi + 1, size=B)
        lS_o.append(torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).cuda())
        lS_i.append(torch.from_numpy(rs.randint(0, n, size=int(lens.sum())).astype(np.int64)).cuda())
    return lS_o, lS_i


def went_up(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--codecs", type=int, nargs="+", default=[16, 8, 4])
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "long_q.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    torch.manual_seed(0)
    L = E._lib.lib()
    out = {"library": os.path.basename(E._lib.LIB_PATH), "reps": a.reps, "shapes": {}}
    for name, ln, d, B, (lo, hi) in SHAPES:
        T = len(ln)
        ev32 = E.EVTables.from_fp32([torch.rand((n, d), device="cuda") * 2 - 1 for n in ln])
        data = [batch(ln, B, lo, hi, 100 + k) for k in range(a.batches)]
        lookups = int(np.mean([sum(int(t.numel()) for t in i) for _, i in data]))
        out["shapes"][name] = {"T": T, "d": d, "B": B, "lookups_per_batch": lookups, "codecs": {}}
        for codec in a.codecs:
            ev = ev32.encode(codec)
            calls = {"long_q": lambda o, i: E.apply_emb_long(o, i, ev), "vec": lambda o, i: E.apply_emb(o, i, ev, lazy=False)}
            seen = {}
            for o, i in data:   # warm-up of every batch and path; the route of each; the two paths agree as bits
                g0, q0 = E._lib.gather_kernels_seen(), E._lib.long_q_kernels_seen()
                ya = torch.stack(list(calls["long_q"](o, i)))
                g1, q1 = E._lib.gather_kernels_seen(), E._lib.long_q_kernels_seen()
                yb = torch.stack(list(calls["vec"](o, i)))
                g2, q2 = E._lib.gather_kernels_seen(), E._lib.long_q_kernels_seen()
                seen = {"long_q": went_up(q0, q1), "vec": went_up(g1, g2)}
                assert g0 == g1 and q1 == q2 and seen["long_q"] == {"longq_c%d_lpr%d" % (codec, d // 4): 1}, seen
                assert seen["vec"] == {"vec_c%d_lpr%d_offsets" % (codec, d // 4): 1}, seen
                assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), "the two paths differ"
            torch.cuda.synchronize()
            ms = {k: [] for k in calls}
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for r in range(a.reps):
                o, i = data[r % len(data)]
                for k in (("long_q", "vec") if r % 2 == 0 else ("vec", "long_q")):
                    ev0.record()
                    calls[k](o, i)
                    ev1.record()
                    ev1.synchronize()
                    ms[k].append(ev0.elapsed_time(ev1))
            # what the algorithm has to move: the encoded rows, 8-byte indices and offsets in, the pooled fp32 rows out
            rec = {"chunk_K": L.evs_long_q_chunk(codec, d), "route": seen,
                   "algorithmic_bytes": lookups * (d * codec // 8 + 8) + T * B * 8 + T * B * d * 4}
            for k, v in ms.items():
                p = np.percentile(v, [10, 50, 90]) * 1000.0
                rec[k + "_us"] = {"p10": round(float(p[0]), 2), "median": round(float(p[1]), 2), "p90": round(float(p[2]), 2)}
            rec["long_q_over_vec"] = round(rec["long_q_us"]["median"] / rec["vec_us"]["median"], 3)
            rec["long_q_p90_below_vec_p10"] = rec["long_q_us"]["p90"] < rec["vec_us"]["p10"]
            out["shapes"][name]["codecs"]["c%d" % codec] = rec
            print(name, "c%d" % codec, json.dumps(rec), flush=True)
            del ev
        del ev32, data
        torch.cuda.empty_cache()
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
