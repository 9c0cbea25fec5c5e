"""The approximate-embedding mode of the batched EvLFU rule restated in Python (test infrastructure; imported like
_bag_evlfu_model.py, on whose BagEvLFUModel -- sets, victim choice, resident(), hist(), counters -- it builds).  The rule is
written down in include/evstore_hip.h at evs_cache_set_batch_approx:

  one (B, T) call = batch n of the batched EvLFU rule, everything judged on the snapshot:
    hit         key (t + 1, rows[b, t]) was resident when the call started; an index out of range is no key (flag 0, a zero
                row, never inserted, never approximated)
    agg_hit(b)  the number of sample b's T keys that hit; an approximated position never counts
    raise       every hit way: priority = max(old, agg_hit(b))
    approx      thres > 0 and agg_hit(b) >= thres: every missed position (b, t) is flagged 2 and served what sample b's
                nearest hit position t' < t is served, key (t' + 1, rows[b, t']); none below t: the zero row.  It is no miss.
    insert      every distinct key missed by a position that was NOT approximated, once, priority = the maximum agg_hit
                over those positions, by BagEvLFUModel's victim rule, priorities as they stand after all raises
    counters    n_requests += B, n_hits += true hits, n_perfect += samples with agg_hit = T; with thres > 0: calls += 1,
                samples += samples with at least one approximated position, substituted / zero_rows += such positions

The flush is not modelled (top_bucket() says how near a stream comes).  When two new keys of one call fall into one set the
kernels' outcome depends on timing: conflict_free_approx_stream draws calls that bring no two INSERTED keys to one set, judged
against this model -- under approximation fewer keys are inserted, so the non-approximating generator's state diverges."""
import numpy as np

import _bag_evlfu_model as EM
import _batched_policy_model as M


class BatchApproxModel(EM.BagEvLFUModel):
    def __init__(self, cap, n_rows, stamp_bits=None):
        super().__init__(cap, n_rows, stamp_bits)
        self.a_calls = self.a_samples = self.a_sub = self.a_zero = 0
        self.n_fetched = 0        # positions that were misses (neither hit nor approximated), cumulative

    def judge_rows(self, rows, thres):
        """-> (flags (B, T) uint8 in {0, 1, 2}, served: B lists of T keys or None, agg (B,), valid (B, T) bool); no state moves"""
        rows = np.asarray(rows)
        B, T = rows.shape
        assert T == self.T
        valid = np.array([[self.is_key((t + 1, int(rows[b, t]))) for t in range(T)] for b in range(B)], bool).reshape(B, T)
        hit = np.array([[valid[b, t] and (t + 1, int(rows[b, t])) in self.where for t in range(T)] for b in range(B)], bool).reshape(B, T)
        agg = hit.sum(1)
        flags = hit.astype(np.uint8)
        served = []
        for b in range(B):
            approx = thres > 0 and agg[b] >= thres
            prev, line = None, []
            for t in range(T):
                key = (t + 1, int(rows[b, t]))
                if not valid[b, t]:
                    line.append(None)
                elif hit[b, t]:
                    line.append(key)
                    prev = key
                elif approx:
                    flags[b, t] = 2
                    line.append(prev)
                else:
                    line.append(key)
            served.append(line)
        return flags, served, agg, valid

    def batch(self, rows, thres=0):
        """one (B, T) call with the threshold `thres` in force (<= 0: the mode off) -> (flags, served)"""
        rows = np.asarray(rows)
        B, T = rows.shape
        flags, served, agg, valid = self.judge_rows(rows, thres)
        self.n += 1
        missed = {}                                            # key -> priority, in order of first appearance (table-major)
        for t in range(T):
            for b in range(B):
                if not valid[b, t] or flags[b, t] == 2:
                    continue
                key, a = (t + 1, int(rows[b, t])), int(agg[b])
                if flags[b, t] == 1:                           # raise
                    s, j = self.where[key]
                    w = self.sets[s][j]
                    w[1] = max(w[1], a)
                else:
                    missed[key] = max(missed.get(key, 0), a)
                    self.n_fetched += 1
        for key, a in missed.items():                          # insert: priorities as the raises left them
            s = int(M.set_of(key[0] - 1, key[1], self.nset, self.n_rows, self.bits))
            ways = self.sets[s]
            j = self._victim(ways)
            if j is None:
                self.n_turned += 1
                continue
            if ways[j] is not None:
                del self.where[ways[j][0]]
                self.n_evict += 1
            ways[j] = [key, a, self.n]
            self.where[key] = (s, j)
        self.n_requests += B
        self.n_hits += int((flags == 1).sum())
        self.n_perfect += int((agg == T).sum())
        if thres > 0:
            two = flags == 2
            zero = np.array([[two[b, t] and served[b][t] is None for t in range(T)] for b in range(B)], bool).reshape(B, T)
            self.a_calls += 1
            self.a_samples += int(two.any(1).sum())
            self.a_sub += int((two & ~zero).sum())
            self.a_zero += int(zero.sum())
        return flags, served

    def approx_counters(self):
        """as GpuCache.approx_stats reports them"""
        return {"calls": self.a_calls, "samples": self.a_samples, "substituted": self.a_sub, "zero_rows": self.a_zero}

    def base_counters(self):
        """the counters of GpuCache.batch_stats the model keeps"""
        return {"size": self.size(), "n_evict": self.n_evict, "n_requests": self.n_requests, "n_perfect_hits": self.n_perfect,
                "n_hits": self.n_hits, "hist": self.hist()}

    def place(self, key, prio):
        """hand-made states: key into the lowest free way of its set at priority prio, filled before any batch"""
        assert self.is_key(key) and key not in self.where
        s = int(M.set_of(key[0] - 1, key[1], self.nset, self.n_rows, self.bits))
        j = self.sets[s].index(None)
        self.sets[s][j] = [key, prio, self.n - 1]
        self.where[key] = (s, j)
        return s * M.WAYS + j

    def entries(self):
        """the resident set as the rows evs_cache_batch_export writes: (table_1based, row, score, age, slot), sorted by slot"""
        out = []
        for s, ways in enumerate(self.sets):
            for j, w in enumerate(ways):
                if w is not None:
                    out.append([w[0][0], w[0][1], w[1], self.n - w[2], s * M.WAYS + j])
        return np.array(out, np.int64).reshape(-1, 5)


def served_rows(served, tabs, d):
    """(B, T, d) fp32: the rows the model says are served, out of the fp32 tables `tabs`; None is the zero row"""
    B, T = len(served), len(served[0])
    out = np.zeros((B, T, d), np.float32)
    for b in range(B):
        for t in range(T):
            if served[b][t] is not None:
                t1, r = served[b][t]
                out[b, t] = tabs[t1 - 1][r]
    return out


def insert_conflicts(model, reqs, thres):
    """positions (b, t) whose key this call would INSERT (missed and not approximated) and which shares its set with a DIFFERENT
    inserted key of the call"""
    flags, _served, _agg, valid = model.judge_rows(reqs, thres)
    owner, bad = {}, []
    for b in range(reqs.shape[0]):
        for t in range(reqs.shape[1]):
            if flags[b, t] != 0 or not valid[b, t]:
                continue
            key = (t + 1, int(reqs[b, t]))
            s = int(M.set_of(t, reqs[b, t], model.nset, model.n_rows, model.bits))
            if owner.setdefault(s, key) != key:
                bad.append((b, t))
    return bad


def conflict_free_call(model, rs, perms, batch, thres, alpha=1.3):
    """One more (batch, T) call for `model` under `thres` (the model does NOT run it): Zipf rows per table; every position whose
    key would be the second inserted key of its set is drawn again and the call judged anew, until none is left"""
    n_rows, T = model.n_rows, model.T
    reqs = np.stack([M.zipf_rows(rs, n_rows[t], batch, alpha, perms[t]) for t in range(T)], 1).astype(np.int32)
    for attempt in range(1000):
        bad = insert_conflicts(model, reqs, thres)
        if not bad:
            return reqs
        for b, t in bad:
            reqs[b, t] = M.zipf_rows(rs, n_rows[t], 1, alpha, perms[t])[0]
    raise AssertionError("no conflict-free call in 1000 rounds of redraws")


def conflict_free_approx_stream(cap, n_rows, batch, n_batches, seed, thres, alpha=1.3):
    """-> (rows (n_batches, batch, T) int32, flags (n_batches, batch, T) uint8, served: per batch what BatchApproxModel.batch
    returned, the model after the last call, the largest top bucket any call left).  Zipf rows; a position whose key would be the
    second inserted key of its set in the call is drawn again and the call judged anew, against THIS model under `thres`: a
    redraw can only add hits to its sample, so the set of approximating samples only grows and the loop ends."""
    rs = np.random.RandomState(seed)
    perms = [rs.permutation(n) for n in n_rows]
    model = BatchApproxModel(cap, n_rows)
    T = len(n_rows)
    rows, flags = np.zeros((n_batches, batch, T), np.int32), np.zeros((n_batches, batch, T), np.uint8)
    served, top = [], 0
    for i in range(n_batches):
        reqs = conflict_free_call(model, rs, perms, batch, thres, alpha)
        rows[i] = reqs
        flags[i], sv = model.batch(reqs, thres)
        served.append(sv)
        top = max(top, model.top_bucket())
    return rows, flags, served, model, top


# The streams the GPU tests run (tests/test_gpu_batch_approx.py); tests/test_batch_approx_model.py asserts their cover without a
# GPU.  G26 -- the reference's 26 tables, d = 36, B = 40: neither a full block nor an even count of half-waves per wave pair;
# G4 -- four tables of very different sizes, d = 16, B = 37: an odd half-wave and a tiny table that puts many positions on one
# way.  Seeds and exponents are picked so that every stream approximates and fetches, evicts, and stays clear of the flush.
STREAMS = {
    "G26": dict(T=26, n_rows=tuple([300] * 26), d=36, cap=512, B=40, n_batches=10, seed=3, thres=20, alpha=1.3),
    "G4": dict(T=4, n_rows=(5, 3000, 70, 400), d=16, cap=64, B=37, n_batches=10, seed=3, thres=3, alpha=1.3),
}
# the toggled stream (G26): the threshold of each call, "bags" = the call goes through lookup_bags with one index per bag
TOGGLE_PLAN = (20, 0, "bags", 20, "bags", 14, 0, 22)
_stream_cache = {}


def toggle_stream():
    """-> (rows (len(TOGGLE_PLAN), B, T) int32, the model after the last call): every call conflict-free under ITS threshold
    (a bag call: none), drawn against one model that runs the plan"""
    if "toggle" not in _stream_cache:
        g = STREAMS["G26"]
        rs = np.random.RandomState(g["seed"] + 1)
        perms = [rs.permutation(n) for n in g["n_rows"]]
        model = BatchApproxModel(g["cap"], list(g["n_rows"]))
        rows = np.zeros((len(TOGGLE_PLAN), g["B"], g["T"]), np.int32)
        for i, what in enumerate(TOGGLE_PLAN):
            rows[i] = conflict_free_call(model, rs, perms, g["B"], 0 if what == "bags" else what, g["alpha"])
            if what == "bags":
                model.batch_bags(*EM.one_per_bag(rows[i]))
            else:
                model.batch(rows[i], what)
        _stream_cache["toggle"] = (rows, model)
    return _stream_cache["toggle"]


def stream(name):
    """conflict_free_approx_stream of STREAMS[name], drawn once per process"""
    if name not in _stream_cache:
        g = STREAMS[name]
        _stream_cache[name] = conflict_free_approx_stream(g["cap"], list(g["n_rows"]), g["B"], g["n_batches"], g["seed"], g["thres"], g["alpha"])
    return _stream_cache[name]
