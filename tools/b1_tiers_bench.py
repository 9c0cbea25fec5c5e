#!/usr/bin/env python3
"""Developer micro-benchmark: batch-1 latency of the tier pair / triple (u8 C1 + u4 C2, optionally the alt-key tier) on the
GPU engine -- one launch + synchronise per request (evs_cache_request_c1c2[c3], the only form before the tier server) against
the resident server (evs_tiers_serve_*), and the per-request cost of the kernel body alone (2 000 requests in one launch).
Kaggle tables (bench.make_tables), the Zipf(1.05) stream of bench.py's batch1_exact, 1 000 warm-up + 2 000 timed requests.

The capacities are chosen so that C1 is full before the timed window and BOTH tiers evict inside it (bench.py --full's
two-tier capacities are sized for 16 384-request batches: this stream would never fill C1, and until C1 is full every miss
goes to C1 and C2 idles).  `--plan` checks a choice without a GPU: the same stream formula on the CPU generator, row ids
renamed to their rank among the ids the stream uses (the policy sees key identity only), through the host engine.
A run in which a tier evicted nothing in the timed window, or tier code 1 or 2 has under 5 % of the keys, is void.

  python tools/b1_tiers_bench.py --plan                 # CPU: shares and evictions for the capacities below
  python tools/b1_tiers_bench.py [--out profiles/b1_tiers_serve.json]
  EVS_LIB_PATH=<another build> python tools/b1_tiers_bench.py --replay-only     # the kernel body of another build
"""
import argparse, ctypes as C, datetime, json, os, socket, subprocess, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np, torch

CAP1, CAP2, CAP3 = 2000, 4000, 1800     # entries; --plan prints what they do to the stream
N_WARM, N_TIMED, T, D = 1000, 2000, 26, 36
ap = argparse.ArgumentParser()
ap.add_argument("--plan", action="store_true"); ap.add_argument("--replay-only", action="store_true")
ap.add_argument("--out", default=""); ap.add_argument("--idle-us", type=int, default=200)
a = ap.parse_args()
import bench


def stream(device):
    n = N_WARM + N_TIMED
    b1s = bench.make_batches(bench.KAGGLE_LN, 256, (n + 255) // 256, seed=13, device=device, dist="zipf", alpha=1.05)
    return torch.cat([b[1].t().contiguous().to(torch.int32) for b in b1s])[:n].contiguous().cpu().numpy()


def void_reason(tier_timed, ev1, ev2):
    s1, s2 = float((tier_timed == 1).mean()), float((tier_timed == 2).mean())
    if ev1 <= 0 or ev2 <= 0: return "a tier evicted nothing in the timed window (C1 %d, C2 %d)" % (ev1, ev2)
    if s1 < 0.05 or s2 < 0.05: return "tier code 1 / 2 has %.1f %% / %.1f %% of the keys (< 5 %%)" % (100 * s1, 100 * s2)
    return ""


if a.plan:
    from evstore_dlrm_amd import host_cache as H
    req = stream("cpu")
    ren = np.zeros_like(req); n_u = []
    for k in range(T):
        u, inv = np.unique(req[:, k], return_inverse=True); ren[:, k] = inv; n_u.append(len(u))
    rs = np.random.RandomState(1)
    raw8 = [rs.randint(0, 255, (n, D), dtype=np.uint8) for n in n_u]; raw4 = [rs.randint(0, 255, (n, D // 2), dtype=np.uint8) & 0xEE for n in n_u]
    for with_c3 in (False, True):
        c1 = H.HostCache("evlfu", CAP1, T, D, 8, "cpp").set_backing(raw8); c2 = H.HostCache("evlfu", CAP2, T, D, 4, "cpp").set_backing(raw4)
        c3 = H.HostAltKeyTier(CAP3, [(rs.randint(0, n, n) * 100 + k + 1).astype(np.uint32) for k, n in enumerate(n_u)]) if with_c3 else None
        rq = (lambda r: H.request_c1c2c3(c1, c2, c3, r)) if with_c3 else (lambda r: H.request_c1c2(c1, c2, r))
        rq(ren[:N_WARM]); s1, s2 = c1.stats(), c2.stats()
        tier, _ = rq(ren[N_WARM:]); e1, e2 = c1.stats()["n_evict"] - s1["n_evict"], c2.stats()["n_evict"] - s2["n_evict"]
        print("plan c3=%d caps %d/%d/%d: C1 size at the window's start %d of %d; timed shares miss %.3f c1 %.3f c2 %.3f c3 %.3f; evictions C1 %d C2 %d; %s"
              % (with_c3, CAP1, CAP2, CAP3, s1["size"], CAP1, *[float((tier == v).mean()) for v in range(4)], e1, e2, void_reason(tier, e1, e2) or "valid"))
    sys.exit(0)

import evstore_dlrm_amd as E
if a.replay_only:   # an older build (EVS_LIB_PATH) lacks the newer entry points: bind what it has, this mode calls evs_cache_request_c1c2c3 only
    _raw = C.CDLL(E._lib.LIB_PATH)
    for _k in [k for k in E._lib._PROTOS if not hasattr(_raw, k)]: del E._lib._PROTOS[_k]
from evstore_dlrm_amd import gpu_cache
from evstore_dlrm_amd.gpu_cache import _dev_ptr
dev = torch.device("cuda"); L = E._lib.lib()
ev = bench.make_tables(bench.KAGGLE_LN, D)
ev8, ev4 = ev.encode(8), ev.encode(4); del ev
g = torch.Generator(device=dev).manual_seed(5)
alt = [(torch.randint(0, n, (n,), device=dev, generator=g, dtype=torch.int64) * 100 + k + 1).to(torch.int32) for k, n in enumerate(bench.KAGGLE_LN)]
req = stream(dev); n_all = len(req)
has_serve = hasattr(L, "evs_tiers_serve_start") and not a.replay_only
st = torch.cuda.current_stream(dev).cuda_stream


def tiers(with_c3):
    c1 = E.GpuCache("evlfu", CAP1, T, D, 8, "cpp", dev); c2 = E.GpuCache("evlfu", CAP2, T, D, 4, "cpp", dev)
    c1.set_backing(ev8); c2.set_backing(ev4)
    return c1, c2, (gpu_cache.GpuAltKeyTier(CAP3, alt) if with_c3 else None)


def run(mode, with_c3):
    c1, c2, c3 = tiers(with_c3); h3 = c3._h if c3 is not None else None
    lat = np.zeros(n_all); tier = np.zeros((n_all, T), np.uint8); ev0 = None
    def mark():    # the tiers' eviction counters where the timed window starts (pauses a server: outside every timed request)
        return c1.stats()["n_evict"], c2.stats()["n_evict"]
    if mode == "replay":
        r = torch.from_numpy(req).to(dev); out = torch.empty((N_TIMED, T, D), dtype=torch.float32, device=dev); td = torch.empty((n_all, T), dtype=torch.uint8, device=dev)
        E._lib.check(L.evs_cache_request_c1c2c3(c1._h, c2._h, h3, N_WARM, r.data_ptr(), out.data_ptr(), td.data_ptr(), 23, st)); torch.cuda.synchronize(); ev0 = mark()
        t1 = time.perf_counter()
        E._lib.check(L.evs_cache_request_c1c2c3(c1._h, c2._h, h3, N_TIMED, r[N_WARM:].data_ptr(), out.data_ptr(), td[N_WARM:].data_ptr(), 23, st)); torch.cuda.synchronize()
        lat[N_WARM:] = (time.perf_counter() - t1) * 1e6 / N_TIMED; tier = td.cpu().numpy()
    elif mode == "launch":
        pr = torch.empty((1, T), dtype=torch.int32).pin_memory(); po = torch.empty((1, T, D), dtype=torch.float32).pin_memory(); pt = torch.empty((1, T), dtype=torch.uint8).pin_memory()
        prn, ptn = pr.numpy(), pt.numpy(); args = (c1._h, c2._h, h3, 1, _dev_ptr(pr), _dev_ptr(po), _dev_ptr(pt), 23, st); fn = L.evs_cache_request_c1c2c3; sync = torch.cuda.synchronize
        for i in range(n_all):
            if i == N_WARM: ev0 = mark()
            t1 = time.perf_counter(); prn[0] = req[i]; rc = fn(*args); sync(); lat[i] = (time.perf_counter() - t1) * 1e6
            assert rc == 0; tier[i] = ptn[0]
    else:
        srv = E.TierServer(c1, c2, c3, n_slots=4, idle_us=a.idle_us)
        try:
            if mode == "serve":
                slot = C.c_int(0); fn = L.evs_tiers_serve_request; h = srv._h; sp = C.byref(slot)
                ptr = [(req[i].ctypes.data, tier[i].ctypes.data) for i in range(n_all)]
                for i in range(n_all):
                    if i == N_WARM: ev0 = mark()
                    rp, tp = ptr[i]; t1 = time.perf_counter(); rc = fn(h, rp, tp, sp); lat[i] = (time.perf_counter() - t1) * 1e6
                    assert rc == 0
            else:
                for i in range(n_all):
                    if i == N_WARM: ev0 = mark()
                    t1 = time.perf_counter(); t, rows = srv.request(req[i]); lat[i] = (time.perf_counter() - t1) * 1e6; tier[i] = t
            srv.stop()
        finally:
            srv.close()
    ev1 = mark(); l = lat[N_WARM:]; tt = tier[N_WARM:]
    return {"mode": mode, "c3": with_c3, "p50_us": float(np.percentile(l, 50)), "p95_us": float(np.percentile(l, 95)), "mean_us": float(l.mean()),
            "hits": int((tt != 0).sum()), "share": [float((tt == v).mean()) for v in range(4)], "n_evict_c1": ev1[0] - ev0[0], "n_evict_c2": ev1[1] - ev0[1],
            "void": void_reason(tt, ev1[0] - ev0[0], ev1[1] - ev0[1])}


modes = ["replay", "replay"] if not has_serve else ["launch", "serve", "serve_py", "replay"] * 2
runs = []
for with_c3 in (False, True):
    for m in modes:
        r = run(m, with_c3); runs.append(r)
        print("%-8s c3=%d  p50 %6.1f us  p95 %6.1f us  mean %6.1f us  hits %d  shares %s  evict %d/%d %s" % (
            m, with_c3, r["p50_us"], r["p95_us"], r["mean_us"], r["hits"], ["%.3f" % v for v in r["share"]], r["n_evict_c1"], r["n_evict_c2"], r["void"] and "VOID: " + r["void"]), flush=True)
void = [r["void"] for r in runs if r["void"]]
for with_c3 in (False, True):
    if len({r["hits"] for r in runs if r["c3"] == with_c3}) != 1: void.append("hits differ between the modes (c3=%d)" % with_c3)
try:
    commit = subprocess.check_output(["git", "-C", R, "rev-parse", "--short", "HEAD"], text=True, stderr=subprocess.DEVNULL).strip()
except Exception:
    commit = "unknown"
rec = {"tool": "tools/b1_tiers_bench.py", "lib": E._lib.LIB_PATH if os.environ.get("EVS_LIB_PATH") else "in-tree", "box": socket.gethostname(), "gpu": torch.cuda.get_device_name(0),
       "date": datetime.date.today().isoformat(), "commit": commit, "caps": [CAP1, CAP2, CAP3], "warmup": N_WARM, "timed": N_TIMED,
       "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "unset (runtime default 4)"),
       "note": "the server shares the process's hardware queues as the machine sets them (configure_runtime() is the integrator's call)",
       "void": void, "runs": runs}
print("RECORD " + json.dumps(rec))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rec, open(a.out, "w"), indent=1)
