"""What tests/test_gpu_fed_backing.py shares with the fetch-first tests of the set-associative tier (tests/test_gpu_host_setassoc.py),
restated here so that neither test file depends on the other: the geometries G1 / G1C / G2, the tables, the conflict-free (B, T)
streams of the Python models (tests/_batched_policy_model.py, _bag_evlfu_model.py), the directed EvLFU hit-and-victim case and the
small helpers around a GpuCache.  Every reference is computed once per process (lru_cache)."""
import functools

import numpy as np
import pytest
import torch

import _bag_evlfu_model as EM
import _batched_policy_model as M

G1 = dict(T=26, n_rows=tuple([300] * 26), d=36, cap=512, B=40)
G1C = dict(T=26, n_rows=tuple([300] * 26), d=36, cap=64, B=64)      # the crowded form: 8 sets
G2 = dict(T=3, n_rows=(5, 3000, 70), d=16, cap=64, B=37)
GEOMS = {"G1": G1, "G1C": G1C, "G2": G2}
POLICIES = ("evlfu", "lru", "lfu")
N_BATCHES = 12
SEED = 3


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()

@functools.lru_cache(maxsize=None)
def _tables(geom, codec, seed=21):
    """-> (what set_backing takes (host arrays), the fp32 rows a lookup must return)"""
    from oracle import oracle as orc
    g = GEOMS[geom]
    tabs = orc.kaggle_tables(list(g["n_rows"]), seed, g["d"])
    if codec == 32:
        return tabs, tabs
    raws = [orc.encode_table(np.clip(t * np.sqrt(len(t)), -1, 1), codec) for t in tabs]   # (spread over the codec's range: rows differ)
    return raws, [orc.decode(a, codec, g["d"]) for a in raws]

def _cache(E, policy, geom, codec, backing, order=None, inline=None):
    g = GEOMS[geom]
    c = E.GpuCache(policy, g["cap"], g["T"], g["d"], codec)
    if order is not None:
        assert c.set_miss_order(order) is c
    if inline is not None:
        c.set_inline_update(inline)
    c.set_backing(backing)
    return c

def _dump(c):
    d = c.batch_dump()
    keys = [(int(t), int(r)) for _, t, r in d]
    assert len(set(keys)) == len(keys), "a key is resident twice"
    return {k: int(s) for k, (s, _, _) in zip(keys, d)}

def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)

def _rows_exact(out, tabs, rq):
    for t in range(rq.shape[1]):
        assert np.array_equal(_bits(out[:, t, :]), _bits(tabs[t][rq[:, t]])), "table %d" % t

@functools.lru_cache(maxsize=None)
def _bt_stream(policy, geom):
    """-> ((N_BATCHES, B, T) int32 rows, the model's flags); conflict-free, and for evlfu without a flush"""
    g = GEOMS[geom]
    if policy == "evlfu":
        rows, flags, _ = EM.conflict_free_rows_stream(g["cap"], list(g["n_rows"]), g["B"], N_BATCHES, SEED)
        m = EM.BagEvLFUModel(g["cap"], list(g["n_rows"]))
        for i in range(N_BATCHES):
            m.batch_bags(*EM.one_per_bag(rows[i]))
            assert m.top_bucket() < int(0.95 * g["cap"]), "the stream would flush"
        return rows, flags
    rows, flags, _ = M.conflict_free_stream(policy, g["cap"], list(g["n_rows"]), g["B"], N_BATCHES, SEED)
    return rows, flags

@functools.lru_cache(maxsize=None)
def _victim_hit_case():
    """-> (rows (n, B, T), flags, the index of the call in which the model evicts a key that call also hits, that key, the key
    that takes its way, the model's resident set after that call).  Seeds are searched in order; the streams are conflict-free
    (a flatter Zipf than the twins': a request with a single hit raises its way to priority 1 only, which keeps it a victim)."""
    g = G2
    n_rows, cap, B, T = list(g["n_rows"]), g["cap"], g["B"], g["T"]
    for seed in range(40):
        try:
            rows, flags, _ = EM.conflict_free_rows_stream(cap, n_rows, B, 10, seed, alpha=1.2)
        except AssertionError:
            continue
        m = EM.BagEvLFUModel(cap, n_rows)
        for i in range(10):
            before = dict(m.where)
            fl = np.stack(m.batch_bags(*EM.one_per_bag(rows[i])), 1)
            if m.top_bucket() >= int(0.95 * cap):
                break                                          # (the flush is not modelled)
            hit_keys = {(t + 1, int(rows[i][b, t])) for b in range(B) for t in range(T) if fl[b, t]}
            both = (set(before) - set(m.where)) & hit_keys
            if both and i >= 1:
                old = sorted(both)[0]
                new = [k for k, at in m.where.items() if at == before[old]]
                return rows[:i + 1], flags[:i + 1], i, old, new[0], m.resident()
    raise AssertionError("no seed gives the case")

def _refused(E, code, policy, fn):
    """policy None: a refusal of today's whose wording does not name it"""
    with pytest.raises(E._lib.EvsError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    assert policy is None or policy in str(ei.value), str(ei.value)
    return str(ei.value)
