"""Shared by tests/test_exact_warm_host.py and tests/test_gpu_exact_warm.py: the cut / export / load / continue check of the
exact engines' warm start against the golden traces of the imported reference (tests/golden/cache_traces.npz).  The exact
policies are deterministic, so everything is array_equal: no tolerance anywhere."""
import functools
import json
import os
import subprocess
import sys

import numpy as np

from conftest import load_golden
from oracle import oracle as orc

# (policy, capacity, cut).  EvLFU 80 runs requests_flush, where the CPU oracle shows the one flush at request 6 and the tier
# full from request 8: empty / before the flush / after it with free entries left / just full / steady.  768 is full from
# request 119, 2000 from request 651.
CASES = ([("evlfu", 80, c) for c in (0, 5, 7, 9, 600)] + [("evlfu", 768, c) for c in (50, 120, 900)] +
         [("evlfu", 2000, c) for c in (300, 1000)] + [("lru", cap, c) for cap in (64, 80) for c in (5, 700)] +
         [("lfu", cap, c) for cap in (768, 80) for c in (5, 700)])


@functools.lru_cache(maxsize=None)
def golden():
    t = load_golden("cache_traces")
    return {k: t[k] for k in t.files}


@functools.lru_cache(maxsize=None)
def tables():
    t = golden()
    return orc.kaggle_tables([int(n) for n in t["n_rows"]], int(t["table_seed"]))


def unpack(packed, n):
    return np.unpackbits(packed, axis=1)[:, :26].astype(bool)[:n]


def trace(cap):
    t = golden()
    return t["requests_flush"] if cap == 80 else t["requests"]


def want(policy, cap, tag=""):
    """-> (hit flags of the uncut trace, final dump, [min_c1, n_perfect, size, n_flush] or None)"""
    t = golden()
    reqs = trace(cap)
    key = "%s_cap%d%s" % (policy, cap, tag)
    hits = unpack(t[key + "_hits"], len(reqs))
    final = t[key + {"evlfu": "_final_buckets", "lru": "_final_order", "lfu": "_final_freq"}[policy]]
    state = [int(v) for v in t[key + "_state"]] if policy == "evlfu" and not tag else None
    return hits, final, state


def check_final(policy, cap, cache, hits_cont, cut, tag=""):
    """the loaded cache after the continuation against the golden of the UNCUT trace: flags, final dump, scalars, counters"""
    hits, final, state = want(policy, cap, tag)
    reqs = trace(cap)
    assert np.array_equal(hits_cont, hits[cut:])
    d = cache.dump()
    np.testing.assert_array_equal(d[:, 1:] if policy == "lru" else d, final)
    st = cache.stats()
    if state is not None:
        assert [st["min_c1"], st["n_perfect"], st["size"], st["n_flush"]] == state
    assert st["size"] == len(final)
    assert st["n_requests"] == len(reqs) and st["n_hits"] == int(hits.sum()) and st["n_perfect_hits"] == int(hits.all(1).sum())


def same_export(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("entries", "state", "n_rows")) and a["entries"].shape == b["entries"].shape


# ---- the cache manager behind ev_lookup: a process-wide singleton, hence child processes (tests/_ev_lookup_warm_child.py) ----
HERE = os.path.dirname(os.path.abspath(__file__))


def manager_child(tmp_path, layers, start, stop, load, save, out, backing="host", env_extra=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="") if backing == "host" else dict(os.environ)
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(HERE, "_ev_lookup_warm_child.py"), str(tmp_path), "8", "60", str(layers), backing,
                        str(start), str(stop), str(load), str(save), str(out)], capture_output=True, text=True, timeout=300, env=env)
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(line[0][7:])


def write_tables(tmp_path, n_req):
    for prec, sub in ((8, "ev-table-8"), (4, "ev-table-4")):
        (tmp_path / sub / "binary").mkdir(parents=True)
        for k, w in enumerate(tables()):
            orc.encode_table(np.clip(w * 8, -1, 1), prec).tofile(tmp_path / sub / "binary" / ("ev-table-%d.bin" % (k + 1)))
    np.save(tmp_path / "reqs.npy", golden()["requests"][:n_req])


def check_two_processes(tmp_path, layers, backing="host", env_extra=None, engine=1):
    n, cut = 400, 150
    write_tables(tmp_path, n)
    whole = manager_child(tmp_path, layers, 0, n, "-", "-", tmp_path / "whole.npy", backing, env_extra)
    first = manager_child(tmp_path, layers, 0, cut, "-", tmp_path / "state.npz", tmp_path / "first.npy", backing, env_extra)
    second = manager_child(tmp_path, layers, cut, n, tmp_path / "state.npz", "-", tmp_path / "second.npy", backing, env_extra)
    assert whole["engine"] == first["engine"] == second["engine"] == engine
    assert first["refused"] == -5                       # EVS_ESTATE: a manager that has served requests is not fresh
    got = np.concatenate([np.load(tmp_path / "first.npy"), np.load(tmp_path / "second.npy")])
    assert np.array_equal(got.view(np.uint32), np.load(tmp_path / "whole.npy").view(np.uint32))
    assert second["perfect"] == whole["perfect"] >= first["perfect"] and whole["perfect"] > 0
    with np.load(tmp_path / "state.npz", allow_pickle=False) as z:
        assert sorted(z.files) == (["entries1", "entries2", "state1", "state2"] if layers == 2 else ["entries1", "state1"])
        assert int(z["state1"][0]) == 2 and z["entries1"].shape[1] == 3 and len(z["entries1"]) > 0
