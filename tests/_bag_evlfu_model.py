"""The batched EvLFU rule over ragged bags ("served bags") restated in Python (test infrastructure; imported like
_bag_policy_model.py).  The rule is written down in include/evstore_hip.h at evs_cache_lookup_bags:

  one call = batch n, the counter shared with the (B, T) form:
    a lookup    one POSITION of one table's index array, all positions numbered table-major
    probe       hit[p] = key (k + 1, indices[k][p]) was resident when the call started; an index out of range is no key (flag 0,
                never inserted); no way word is written
    served bag  a valid bag none of whose positions is a miss or out of range; an empty bag is served, a bag with backwards
                offsets (or offsets past the index array) is empty, hence served
    agg_hit(b)  the number of sample b's T bags that are served
    raise       every hit way named by a position of sample b: priority = max(old, agg_hit(b)); the stamp stays
    insert      every distinct missed key once, priority = the maximum of agg_hit over the samples that name it, into its own
                set: a free way first (lowest index), else the lowest priority among the ways the running batch has not
                filled, lowest index among equals; none: turned away.  Priorities as they stand after ALL raises.
    uncovered   a position no valid bag covers counts 0: a hit is not raised, a miss is inserted at priority 0
    counters    n_requests += B, n_hits += hit positions, n_perfect += samples with at least one lookup and agg_hit = T

Ways are [key, priority, filling batch] lists (None = free); keys are (table_1based, row).  The flush (the top bucket reaching
95 % of the capacity) is NOT modelled: its victims depend on timing.  top_bucket() says how near a stream comes.

A position that two valid bags of DIFFERENT samples cover (offsets that go back) counts for one of them, which one the rule
leaves open: batch_bags refuses such a call (AssertionError) instead of guessing.

When two new keys of one call fall into one set the kernels' outcome depends on timing; the model inserts in order of first
appearance, one of the allowed outcomes.  conflict_free_bag_stream draws calls that bring no two new keys to one set
(_bag_policy_model.conflict_free_bags, run against this model), so every flag and the whole {key: priority} set are pinned."""
import numpy as np

import _bag_policy_model as BM
import _batched_policy_model as M


class BagEvLFUModel:
    def __init__(self, cap, n_rows, stamp_bits=None):
        assert cap >= M.WAYS
        self.cap, self.n_rows, self.T = cap, [int(n) for n in n_rows], len(n_rows)
        self.nset, self.bits = M.geometry(cap, n_rows)
        self.stamp_bits = stamp_bits           # None: plain batch numbers; S: compared modulo 2^S, as the way words hold them
        self.sets = [[None] * M.WAYS for _ in range(self.nset)]
        self.where = {}                        # key -> (set, way)
        self.n = 0
        self.n_evict = self.n_requests = self.n_hits = self.n_perfect = self.n_turned = 0

    def is_key(self, key):
        return 0 <= key[1] < self.n_rows[key[0] - 1]

    def _filled_now(self, w):
        d = self.n - w[2]
        return d == 0 if self.stamp_bits is None else d % (1 << self.stamp_bits) == 0

    def _victim(self, ways):
        for j, w in enumerate(ways):
            if w is None:
                return j
        best = None
        for j, w in enumerate(ways):
            if self._filled_now(w):
                continue
            if best is None or w[1] < ways[best][1]:          # (strict: ties go to the lowest way index)
                best = j
        return best

    def judge(self, offsets, indices, flags):
        """-> (agg: B served-bag counts, lookups: B position counts over the valid bags, pos_sample: per table the sample
        that covers each position, -1 = none)"""
        T, B = len(indices), len(offsets[0])
        agg, lookups = np.zeros(B, np.int64), np.zeros(B, np.int64)
        pos_sample = [np.full(len(indices[k]), -1, np.int64) for k in range(T)]
        for k in range(T):
            nnz = len(indices[k])
            for b in range(B):
                st = int(offsets[k][b])
                en = int(offsets[k][b + 1]) if b + 1 < B else nnz
                if not (0 <= st <= en <= nnz):
                    agg[b] += 1                                # an empty bag is served
                    continue
                taken = pos_sample[k][st:en]
                assert ((taken == -1) | (taken == b)).all(), "table %d: samples %s and %d cover one position" % (k, set(taken[taken >= 0]), b)
                pos_sample[k][st:en] = b
                lookups[b] += en - st
                agg[b] += int(np.asarray(flags[k][st:en], bool).all())   # (an out-of-range index has flag 0)
        return agg, lookups, pos_sample

    def batch_bags(self, offsets, indices):
        """one call over per-table offsets (B,) and index arrays -> per-table bool flag arrays; keeps the counters"""
        T, B = len(indices), len(offsets[0])
        assert T == self.T
        self.n += 1
        flags = [np.array([(k + 1, int(r)) in self.where for r in indices[k]], bool) for k in range(T)]
        agg, lookups, pos_sample = self.judge(offsets, indices, flags)
        missed = {}                                            # key -> priority, in order of first appearance
        for k in range(T):
            for p, r in enumerate(indices[k]):
                key = (k + 1, int(r))
                if not self.is_key(key):
                    continue
                a = int(agg[pos_sample[k][p]]) if pos_sample[k][p] >= 0 else 0
                if flags[k][p]:                                # raise
                    s, j = self.where[key]
                    w = self.sets[s][j]
                    w[1] = max(w[1], a)
                else:
                    missed[key] = max(missed.get(key, 0), a)
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
        self.n_hits += int(sum(f.sum() for f in flags))
        self.n_perfect += int(((lookups > 0) & (agg == T)).sum())
        return flags

    def resident(self):
        """{key: priority} as evs_cache_batch_dump reports it"""
        return {w[0]: w[1] for ways in self.sets for w in ways if w is not None}

    def hist(self):
        """resident entries per priority 0 .. T, as evs_cache_batch_stats reports them"""
        h = [0] * (self.T + 1)
        for ways in self.sets:
            for w in ways:
                if w is not None:
                    h[w[1]] += 1
        return h

    def top_bucket(self):
        return self.hist()[self.T]

    def size(self):
        return len(self.where)


def one_per_bag(reqs):
    """(B, T) rows -> (offsets, indices) of the same call with one index per bag"""
    reqs = np.asarray(reqs)
    B, T = reqs.shape
    return [np.arange(B, dtype=np.int64) for _ in range(T)], [reqs[:, t].astype(np.int64) for t in range(T)]


def conflict_free_bag_stream(cap, n_rows, batch, max_bag, n_batches, seed, alpha=1.3):
    """-> (calls: n_batches tuples (offsets, indices, flags), the model after the last call, the largest top bucket any call
    left): _bag_policy_model.conflict_free_bags against this model -- bag sizes uniform in 0 .. max_bag, Zipf rows, and a row
    whose key would be the second new key of its set in the call drawn again"""
    rs = np.random.RandomState(seed)
    perms = [rs.permutation(n) for n in n_rows]
    model = BagEvLFUModel(cap, n_rows)
    calls, top = [], 0
    for _ in range(n_batches):
        off, idx, flags, _ = BM.conflict_free_bags(model, rs, perms, batch, max_bag, alpha)
        calls.append((off, idx, flags))
        top = max(top, model.top_bucket())
    return calls, model, top


def conflict_free_rows_stream(cap, n_rows, batch, n_batches, seed, alpha=1.3):
    """the same with one index per bag -> ((n_batches, batch, T) int32 rows, flags (n_batches, batch, T) bool, the model):
    _batched_policy_model.conflict_free_batch's draw, run against this model"""
    rs = np.random.RandomState(seed)
    perms = [rs.permutation(n) for n in n_rows]
    model = BagEvLFUModel(cap, n_rows)
    T = len(n_rows)
    rows, flags = np.zeros((n_batches, batch, T), np.int32), np.zeros((n_batches, batch, T), bool)
    for i in range(n_batches):
        reqs = np.stack([M.zipf_rows(rs, n_rows[t], batch, alpha, perms[t]) for t in range(T)], 1).astype(np.int32)
        owner = {}                                             # set -> the one new key this call brings to it
        for b in range(batch):
            for t in range(T):
                for attempt in range(1000):
                    key = (t + 1, int(reqs[b, t]))
                    if key in model.where:
                        break
                    s = int(M.set_of(t, reqs[b, t], model.nset, n_rows, model.bits))
                    if owner.setdefault(s, key) == key:
                        break
                    reqs[b, t] = M.zipf_rows(rs, n_rows[t], 1, alpha, perms[t])[0]
                else:
                    raise AssertionError("no conflict-free row for table %d in 1000 draws" % t)
        rows[i] = reqs
        flags[i] = np.stack(model.batch_bags(*one_per_bag(reqs)), 1)
    return rows, flags, model
