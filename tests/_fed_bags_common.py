"""What tests/test_gpu_fed_bags.py computes once per process: the geometries of tests/test_gpu_bags_count_first.py (G1, G1C, G2,
G3), their tables, the conflict-free bag streams of the two Python models (tests/_bag_evlfu_model.py, _bag_policy_model.py) with
the parameters the existing bag tests use for these geometries, numpy pooling and the key list a begin must give."""
import functools

import numpy as np

import _bag_evlfu_model as EM
import _bag_policy_model as BP
import _batched_policy_model as M

G1 = dict(T=26, n_rows=tuple([300] * 26), d=36, cap=512, B=40)
G1C = dict(T=26, n_rows=tuple([300] * 26), d=36, cap=64, B=64)      # the crowded form: 8 sets
G2 = dict(T=3, n_rows=(5, 3000, 70), d=16, cap=64, B=37)
G3 = dict(T=3, n_rows=(400, 413, 426), d=16, cap=8192, B=37)        # long bags: a cache in which nothing is evicted
GEOMS = {"G1": G1, "G1C": G1C, "G2": G2, "G3": G3}
POLICIES = ("evlfu", "lru", "lfu")
N_BATCHES = 12
SEED = 3
STREAM_KW = {"G1": dict(max_bag=5, alpha=2.0), "G2": dict(max_bag=4, alpha=1.3)}


@functools.lru_cache(maxsize=None)
def tables(geom, codec, seed=21):
    """-> (what set_backing takes (host arrays), the fp32 rows a lookup must return)"""
    from oracle import oracle as orc
    g = GEOMS[geom]
    tabs = orc.kaggle_tables(list(g["n_rows"]), seed, g["d"])
    if codec == 32:
        return tabs, tabs
    raws = [orc.encode_table(np.clip(t * np.sqrt(len(t)), -1, 1), codec) for t in tabs]   # (spread over the codec's range: rows differ)
    return raws, [orc.decode(a, codec, g["d"]) for a in raws]


def new_model(policy, geom):
    g = GEOMS[geom]
    if policy == "evlfu":
        return EM.BagEvLFUModel(g["cap"], list(g["n_rows"]))
    return BP.BagPolicyModel(policy, g["cap"], list(g["n_rows"]))


def samples_of(off, idx):
    """per table: the sample whose valid bag covers each position, -1 = none"""
    out = []
    B = len(off[0])
    for o, ix in zip(off, idx):
        ps = np.full(len(ix), -1, np.int64)
        for b in range(B):
            st, en = int(o[b]), int(o[b + 1]) if b + 1 < B else len(ix)
            if 0 <= st <= en <= len(ix):
                ps[st:en] = b
        out.append(ps)
    return out


def want_keys(idx, flags, n_rows, fed):
    """the distinct table_1based << 32 | row with flag 0 and a valid index, over the fed tables"""
    want = set()
    for t in fed:
        col = np.asarray(idx[t], np.int64)
        ok = (col >= 0) & (col < n_rows[t]) & ~np.asarray(flags[t], bool)
        want |= {((t + 1) << 32) | int(r) for r in col[ok]}
    return want


@functools.lru_cache(maxsize=None)
def stream(policy, geom):
    """-> the N_BATCHES calls (offsets, indices, flags) of the conflict-free stream.  Held to: at least one eviction, no flush, and
    at least one listed key that two or more positions of different samples name."""
    g = GEOMS[geom]
    kw = STREAM_KW[geom]
    n_rows = list(g["n_rows"])
    if policy == "evlfu":
        calls, model, top = EM.conflict_free_bag_stream(g["cap"], n_rows, g["B"], kw["max_bag"], N_BATCHES, SEED, alpha=kw["alpha"])
        assert top < int(0.95 * g["cap"]), "the stream would flush"
    else:
        calls, model, _ = BP.conflict_free_bag_stream(policy, g["cap"], n_rows, g["B"], kw["max_bag"], N_BATCHES, SEED, alpha=kw["alpha"])
    assert model.n_evict > 0, "no eviction"
    shared = 0
    for off, idx, flags in calls:
        ps = samples_of(off, idx)
        named = {}
        for t in range(g["T"]):
            for p in np.nonzero(~np.asarray(flags[t], bool))[0]:
                named.setdefault((t, int(idx[t][p])), set()).add(int(ps[t][p]))
        shared += sum(len(s) >= 2 for s in named.values())
    assert shared > 0, "no missed key is named by two samples"
    return calls


@functools.lru_cache(maxsize=None)
def mixed_stream(policy, geom, n_calls=N_BATCHES):
    """-> calls ("bags", offsets, indices, flags) and ("rows", (B, T) int32 rows, (B, T) flags) alternating, conflict-free against
    ONE model: a (B, T) call is the bag call with one index per bag, under either rule"""
    g = GEOMS[geom]
    kw = STREAM_KW[geom]
    n_rows, B, T = list(g["n_rows"]), g["B"], g["T"]
    rs = np.random.RandomState(SEED + 1)
    perms = [rs.permutation(n) for n in n_rows]
    model = new_model(policy, geom)
    calls = []
    for i in range(n_calls):
        if i % 2 == 0:
            off, idx, flags, _ = BP.conflict_free_bags(model, rs, perms, B, kw["max_bag"], kw["alpha"])
            calls.append(("bags", off, idx, flags))
            continue
        reqs = np.stack([M.zipf_rows(rs, n_rows[t], B, kw["alpha"], perms[t]) for t in range(T)], 1).astype(np.int32)
        owner = {}
        for b in range(B):
            for t in range(T):
                for attempt in range(1000):
                    key = (t + 1, int(reqs[b, t]))
                    if key in model.where:
                        break
                    s = int(M.set_of(t, reqs[b, t], model.nset, n_rows, model.bits))
                    if owner.setdefault(s, key) == key:
                        break
                    reqs[b, t] = M.zipf_rows(rs, n_rows[t], 1, kw["alpha"], perms[t])[0]
                else:
                    raise AssertionError("no conflict-free row for table %d in 1000 draws" % t)
        flags = np.stack(model.batch_bags(*EM.one_per_bag(reqs)), 1)
        calls.append(("rows", reqs, flags))
    assert model.n_evict > 0, "no eviction"
    if policy == "evlfu":
        assert model.top_bucket() < int(0.95 * g["cap"]), "the stream would flush"
    return calls


def np_pool(tabs, off, idx, B):
    """(T, B, d) fp32: every valid bag's rows added in index order from +0 (unfused fp32 adds); an index out of range pools
    nothing, a bad bag is empty"""
    T, d = len(tabs), tabs[0].shape[1]
    out = np.zeros((T, B, d), np.float32)
    for t in range(T):
        n = len(idx[t])
        for b in range(B):
            st, en = int(off[t][b]), int(off[t][b + 1]) if b + 1 < B else n
            if not (0 <= st <= en <= n):
                continue
            acc = np.zeros(d, np.float32)
            for r in idx[t][st:en]:
                if 0 <= r < len(tabs[t]):
                    acc = acc + tabs[t][int(r)]
            out[t, b] = acc
    return out


def set_of(geom, key):
    g = GEOMS[geom]
    nset, bits = M.geometry(g["cap"], g["n_rows"])
    return int(M.set_of(key[0] - 1, key[1], nset, list(g["n_rows"]), bits))


def call_of(B, T, bags):
    """{(sample, table): [rows]} -> (offsets, indices) with every other bag empty"""
    off, idx = [], []
    for t in range(T):
        per = [np.asarray(bags.get((b, t), []), np.int64) for b in range(B)]
        off.append(np.concatenate([[0], np.cumsum([len(p) for p in per[:-1]])]).astype(np.int64))
        idx.append(np.concatenate(per + [np.zeros(0, np.int64)]).astype(np.int64))
    return off, idx
