"""The wide interaction kernel (csrc/evs_fused_wide.hip) at F in {33, 64, 128}, d in {36, 64}, B = 16 384, three routes to the same R
on the same seeded batches, in one process, in rotating order, device events around every call, after a warm-up of every shape
that also compares the outputs and confirms the routes from the dispatch records:
    gather       apply_emb_interact(..., one_index_per_bag=True): rows from the tables to the matrix cores, one launch
    two_launch   apply_emb (the (T, B, d) block) then interact_features' dense form of the same kernel
    generic      apply_emb then evs_interact_dot's generic kernel: the only route there was before the wide kernel
Bytes moved (what the algorithm has to move, from the shapes) over time stand beside the run's own copy calibration: a
device-to-device copy of 1 GiB, read + written bytes over its time.  Writes profiles/wide.json (--out).

    python tools/wide_bench.py [--reps 2000] [--generic-reps 60] [--out profiles/wide.json]
    python tools/wide_bench.py --codec 16,8,4 [--reps 500]      the encoded kernel (measure_encoded), writes profiles/wide_q.json

The two wide routes take tens to hundreds of microseconds a call, so they are timed --reps times each (a good second of device
time per shape); the generic route takes milliseconds and joins every (reps / generic-reps)-th round.

A kernel split (rocprofv3 --kernel-trace --stats -- python tools/wide_bench.py --reps 10 --out /dev/null) belongs in a run of its own."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import evstore_dlrm_amd as E  # noqa: E402

B, ROWS = 16384, 100000
SHAPES = [(F, d) for F in (33, 64, 128) for d in (36, 64)]


def went_up(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def timed(call, ev0, ev1):
    ev0.record()
    call()
    ev1.record()
    ev1.synchronize()
    return ev0.elapsed_time(ev1)


def stats_us(v):
    p = np.percentile(v, [10, 50, 90]) * 1000.0
    return {"p10": round(float(p[0]), 2), "median": round(float(p[1]), 2), "p90": round(float(p[2]), 2)}


def generic(x, ly):
    """evs_interact_dot past 32 features: its generic kernel (pointer tables through a device buffer, a synchronise per call)"""
    fs = [x] + list(ly)
    F, d = len(fs), int(x.shape[1])
    R = torch.empty((B, d + F * (F - 1) // 2), dtype=torch.float32, device="cuda")
    ptrs = (C.c_void_p * F)(*[f.data_ptr() for f in fs])
    strides = (C.c_int64 * F)(*[int(f.stride(0)) for f in fs])
    E._lib.check(E._lib.lib().evs_interact_dot(B, F, d, ptrs, strides, 0, R.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return R


def encoded_tables(codec, T, d, gen):
    """T tables of ROWS random rows of `codec`-bit codes (u16 up to 65 000: the main range of trained tables; u4 never nibble 15)"""
    if codec == 16:
        v = torch.randint(0, 65001, (T, ROWS, d), device="cuda", generator=gen, dtype=torch.int32)
        raw = torch.stack((v & 255, v >> 8), -1).to(torch.uint8)   # little-endian ushorts
    elif codec == 8:
        raw = torch.randint(0, 256, (T, ROWS, d), device="cuda", generator=gen).to(torch.uint8)
    else:
        nib = torch.randint(0, 15, (T, ROWS, d), device="cuda", generator=gen)
        raw = (nib[..., 0::2] * 16 + nib[..., 1::2]).to(torch.uint8)
    return E.EVTables(list(raw.reshape(T, ROWS, -1).unbind(0)), d, codec)


def measure_encoded(a, codecs, out, copy_gbs, ev0, ev1):
    """--codec: the wide kernel over encoded tables (csrc/evs_fused_wide_q.hip), three routes per codec and shape, rotating:
        one_launch    apply_emb_interact(..., one_index_per_bag=True) over the encoded tables
        two_launch    the same call with lS_o given and nothing declared: apply_emb decodes the (T, B, d) block, the dense form reads it
        fp32_gather   the gather form over fp32 tables of the same shape, the yardstick"""
    for codec in codecs:
        for F, d in SHAPES:
            T, P = F - 1, F * (F - 1) // 2
            gen = torch.Generator(device="cuda").manual_seed(100 * F + d + codec)
            evq = encoded_tables(codec, T, d, gen)
            ev32 = E.EVTables.from_fp32(list((torch.rand((T, ROWS, d), device="cuda") * 2 - 1).unbind(0)))
            data = [(torch.randn((B, d), device="cuda", generator=gen), torch.randint(0, ROWS, (T, B), device="cuda", generator=gen))
                    for _ in range(a.batches)]
            lS_o = torch.arange(B, device="cuda").repeat(T, 1)
            calls = {"one_launch": lambda x, i: E.apply_emb_interact(x, None, i, evq, one_index_per_bag=True),
                     "two_launch": lambda x, i: E.apply_emb_interact(x, lS_o, i, evq),
                     "fp32_gather": lambda x, i: E.apply_emb_interact(x, None, i, ev32, one_index_per_bag=True)}
            route, same = {}, True
            for x, i in data:   # warm-up of every batch and route; the routes from the records; do the two encoded routes agree bit for bit
                R = {}
                for k, f in calls.items():
                    q0, w0 = E._lib.wide_q_kernels_seen(), E._lib.wide_kernels_seen()
                    R[k] = f(x, i)
                    route[k] = {"wide_q": went_up(q0, E._lib.wide_q_kernels_seen()), "wide": went_up(w0, E._lib.wide_kernels_seen())}
                assert len(route["one_launch"]["wide_q"]) == 1 and not route["one_launch"]["wide"], route
                assert not route["two_launch"]["wide_q"] and list(route["two_launch"]["wide"])[0].startswith("wide_dense"), route
                assert list(route["fp32_gather"]["wide"])[0].startswith("wide_gather"), route
                same = same and torch.equal(R["one_launch"].view(torch.int32), R["two_launch"].view(torch.int32))
            torch.cuda.synchronize()
            ms = {k: [] for k in calls}
            order = list(calls)
            for r in range(a.reps):
                x, i = data[r % len(data)]
                for k in order[r % 3:] + order[:r % 3]:
                    ms[k].append(timed(lambda: calls[k](x, i), ev0, ev1))
            # what each route has to move: rows, indices and x in, R out; two launches write the fp32 (T, B, d) block and read it back
            rest = B * (T * 8 + d * 4 + (d + P) * 4)
            nbytes = {"one_launch": rest + B * T * d * codec // 8, "two_launch": rest + B * T * d * codec // 8 + 2 * T * B * d * 4,
                      "fp32_gather": rest + B * T * d * 4}
            rec = {"codec": codec, "T": T, "d": d, "route": route, "routes_bit_equal": same}
            for k, v in ms.items():
                s = stats_us(v)
                gbs = nbytes[k] / s["median"] / 1e3
                rec[k] = {"us": s, "algorithmic_bytes": nbytes[k], "GB_per_s": round(gbs, 1), "of_copy_rate": round(gbs / copy_gbs, 3)}
            rec["one_over_two_launch"] = round(rec["one_launch"]["us"]["median"] / rec["two_launch"]["us"]["median"], 4)
            rec["one_launch_over_fp32_gather"] = round(rec["one_launch"]["us"]["median"] / rec["fp32_gather"]["us"]["median"], 4)
            out["shapes"]["u%d_F%d_d%d" % (codec, F, d)] = rec
            print("u%d_F%d_d%d" % (codec, F, d), json.dumps(rec), flush=True)
            del evq, ev32, data
            torch.cuda.empty_cache()


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--generic-reps", type=int, default=60)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--codec", default=None, help="16, 8, 4 or a comma list: measure the encoded kernel instead (profiles/wide_q.json)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    codecs = [int(c) for c in a.codec.split(",")] if a.codec else []
    assert all(c in (16, 8, 4) for c in codecs), "--codec takes 16, 8, 4"
    a.out = a.out or os.path.join(root, "profiles", "wide_q.json" if codecs else "wide.json")
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    torch.manual_seed(0)
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    copy_ms = float(np.median([timed(lambda: dst.copy_(src), ev0, ev1) for _ in range(20)]))
    copy_gbs = 2 * src.numel() * 4 / copy_ms / 1e6
    del src, dst
    out = {"library": os.path.basename(E._lib.LIB_PATH), "reps": a.reps, "generic_reps": a.generic_reps, "B": B, "rows_per_table": ROWS,
           "copy_calibration": {"bytes": 2 << 30, "median_ms": round(copy_ms, 4), "GB_per_s": round(copy_gbs, 1)}, "shapes": {}}
    print("copy calibration", json.dumps(out["copy_calibration"]), flush=True)
    if codecs:
        measure_encoded(a, codecs, out, copy_gbs, ev0, ev1)
    for F, d in SHAPES if not codecs else []:
        T, P = F - 1, F * (F - 1) // 2
        ev = E.EVTables.from_fp32(list((torch.rand((T, ROWS, d), device="cuda") * 2 - 1).unbind(0)))
        gen = torch.Generator(device="cuda").manual_seed(100 * F + d)
        data = [(torch.randn((B, d), device="cuda", generator=gen), torch.randint(0, ROWS, (T, B), device="cuda", generator=gen))
                for _ in range(a.batches)]
        lS_o = torch.arange(B, device="cuda").repeat(T, 1)
        pool = lambda i: E.apply_emb(lS_o, i, ev, lazy=False, one_index_per_bag=True)
        calls = {"gather": lambda x, i: E.apply_emb_interact(x, None, i, ev, one_index_per_bag=True),
                 "two_launch": lambda x, i: E.interact_features(x, pool(i)),
                 "generic": lambda x, i: generic(x, pool(i))}
        route = {}
        for x, i in data:   # warm-up of every batch and route; the routes from the records; the outputs agree
            R = {}
            for k, f in calls.items():
                w0, g0 = E._lib.wide_kernels_seen(), E._lib.gather_kernels_seen()
                R[k] = f(x, i)
                route[k] = {"wide": went_up(w0, E._lib.wide_kernels_seen()), "pooling_launches": sum(went_up(g0, E._lib.gather_kernels_seen()).values())}
            assert len(route["gather"]["wide"]) == 1 and route["gather"]["pooling_launches"] == 0, route
            assert len(route["two_launch"]["wide"]) == 1 and route["two_launch"]["pooling_launches"] > 0 and not route["generic"]["wide"], route
            assert torch.equal(R["gather"].view(torch.int32), R["two_launch"].view(torch.int32)), "the two forms differ"
            scale = float(R["gather"].abs().max())
            assert float((R["gather"] - R["generic"]).abs().max()) <= 1e-4 * scale, "the wide kernel and the generic kernel differ"
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        order = list(calls)
        every = max(1, a.reps // a.generic_reps)
        for r in range(a.reps):
            x, i = data[r % len(data)]
            for k in order[r % 3:] + order[:r % 3]:
                if k != "generic" or r % every == 0:
                    ms[k].append(timed(lambda: calls[k](x, i), ev0, ev1))
        # what each route has to move: rows, indices and x in, R out; the two-launch routes write the (T, B, d) block and read it back
        fused = B * (T * (d * 4 + 8) + d * 4 + (d + P) * 4)
        nbytes = {"gather": fused, "two_launch": fused + 2 * T * B * d * 4, "generic": fused + 2 * T * B * d * 4}
        rec = {"T": T, "d": d, "route": route, "mfma_flop": 2 * B * 16 * 16 * d * sum(t + 1 for t in range((F + 15) // 16))}
        for k, v in ms.items():
            s = stats_us(v)
            gbs = nbytes[k] / s["median"] / 1e3
            rec[k] = {"us": s, "algorithmic_bytes": nbytes[k], "GB_per_s": round(gbs, 1), "of_copy_rate": round(gbs / copy_gbs, 3)}
        rec["gather_over_generic"] = round(rec["gather"]["us"]["median"] / rec["generic"]["us"]["median"], 4)
        rec["two_launch_over_generic"] = round(rec["two_launch"]["us"]["median"] / rec["generic"]["us"]["median"], 4)
        rec["gather_over_two_launch"] = round(rec["gather"]["us"]["median"] / rec["two_launch"]["us"]["median"], 4)
        out["shapes"]["F%d_d%d" % (F, d)] = rec
        print("F%d_d%d" % (F, d), json.dumps(rec), flush=True)
        del ev, data
        torch.cuda.empty_cache()
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
