"""The batched LRU / LFU rule over ragged bags restated in Python (test infrastructure; imported like _batched_policy_model.py).
The rule is written down in include/evstore_hip.h at evs_cache_lookup_bags:

  one call = batch n, the counter shared with the (B, T) form:
    a lookup  one POSITION of one table's index array, all positions numbered table-major
    probe     hit[p] = key (k + 1, indices[k][p]) was resident when the call started; an index out of range is no key (flag 0,
              never inserted)
    touch     every way hit at least once: last = n; LFU: counter + 1 ONCE per batch
    insert    every distinct missed key once (BatchedPolicyModel's victim rule)
    counters  n_requests += B, n_hits += hit positions, n_perfect += samples with at least one lookup and none missed or out of
              range over all their bags (a bag with backwards offsets is empty)

Also a conflict-free ragged generator: no batch brings two new keys to one set, so the kernels' outcome is deterministic."""
import numpy as np

import _batched_policy_model as M


class BagPolicyModel(M.BatchedPolicyModel):
    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.n_requests = self.n_hits = self.n_perfect = 0

    def is_key(self, key):
        return 0 <= key[1] < self.n_rows[key[0] - 1]

    def batch_keys(self, keys):
        """one call over a position-ordered list of (table_1based, row) -> bool flags, one per position"""
        self.n += 1
        cur = self._cur()
        flags = np.zeros(len(keys), bool)
        missed, seen = [], set()
        for p, key in enumerate(keys):
            if not self.is_key(key):
                continue
            if key in self.where:
                flags[p] = True
            elif key not in seen:
                seen.add(key)
                missed.append(key)
        for p in np.nonzero(flags)[0]:                      # touch: once per way and batch
            s, j = self.where[keys[p]]
            w = self.sets[s][j]
            if w[2] != cur:
                w[2] = cur
                w[1] = w[1] + 1 if self.cnt_max is None else min(w[1] + 1, self.cnt_max)
            elif w[3] != self.n and self.policy == "lfu" and (self.cnt_max is None or w[1] < self.cnt_max):
                self.events["count_skipped"] += 1           # (only with stamp_bits, as in BatchedPolicyModel.batch)
            w[3] = self.n
        if missed:                                          # insert: every distinct missed key once
            sets = M.set_of([t - 1 for t, _ in missed], [r for _, r in missed], self.nset, self.n_rows, self.bits)
            for key, s in zip(missed, sets):
                ways = self.sets[int(s)]
                j = self._victim(ways)
                if j is None:
                    continue                                # turned away
                if ways[j] is not None:
                    del self.where[ways[j][0]]
                    self.n_evict += 1
                ways[j] = [key, 1, cur, self.n]           # [key, counter, last, true_last], BatchedPolicyModel's ways
                self.where[key] = (int(s), j)
        return flags

    def batch_bags(self, offsets, indices):
        """one call over per-table offsets (B,) and index arrays -> per-table bool flag arrays; keeps the counters"""
        T, B = len(indices), len(offsets[0])
        keys = [(k + 1, int(r)) for k in range(T) for r in indices[k]]
        flags = self.batch_keys(keys)
        cuts = np.cumsum([len(i) for i in indices])[:-1]
        per_table = np.split(flags, cuts)
        self.n_requests += B
        self.n_hits += int(flags.sum())
        self.n_perfect += perfect_samples(offsets, indices, per_table)
        return per_table


def perfect_samples(offsets, indices, flags):
    """the samples that have at least one lookup and none missed or out of range, over all their bags (flags: per table,
    one per position; a bag whose offsets are backwards or past the index array is empty)"""
    T, B = len(indices), len(offsets[0])
    n = 0
    for b in range(B):
        n_lookups, n_bad = 0, 0
        for k in range(T):
            nnz = len(indices[k])
            st = int(offsets[k][b])
            en = int(offsets[k][b + 1]) if b + 1 < B else nnz
            if not (0 <= st <= en <= nnz):
                continue
            n_lookups += en - st
            n_bad += int((~np.asarray(flags[k][st:en], bool)).sum())
        n += int(n_lookups > 0 and n_bad == 0)
    return n


def keys_of(indices):
    """the position-ordered (table-major) key list of a call"""
    return [(k + 1, int(r)) for k in range(len(indices)) for r in indices[k]]


def new_key_conflicts(model, keys):
    """positions of `keys` whose key is new to `model` and shares its set with a DIFFERENT new key of the call"""
    owner, bad = {}, []
    for p, key in enumerate(keys):
        if key in model.where or not model.is_key(key):
            continue
        s = int(M.set_of(key[0] - 1, key[1], model.nset, model.n_rows, model.bits))
        if owner.setdefault(s, key) != key:
            bad.append(p)
    return bad


def conflict_free_bags(model, rs, perms, batch, max_bag, alpha=1.3):
    """One more call for `model` (which runs it) -> (offsets, indices: T int64 arrays each, flags: T bool arrays, redrawn
    positions).  Bag sizes uniform in 0 .. max_bag per (sample, table), rows Zipf through per-table permutations, drawn in
    (sample, table) order; a row whose key would be the second new key of its set in this call is drawn again against the
    model's own state.  (Table-major draws starve the late tables: the sets are taken by the time they come up.)"""
    n_rows, T = model.n_rows, len(model.n_rows)
    sizes = rs.randint(0, max_bag + 1, size=(batch, T))
    bags = [[None] * T for _ in range(batch)]
    owner, redrawn = {}, 0
    for b in range(batch):
        for t in range(T):
            rows = M.zipf_rows(rs, n_rows[t], int(sizes[b, t]), alpha, perms[t]).astype(np.int64)
            for i in range(len(rows)):
                for attempt in range(1000):
                    key = (t + 1, int(rows[i]))
                    if key in model.where:
                        break
                    s = int(M.set_of(t, rows[i], model.nset, n_rows, model.bits))
                    if owner.setdefault(s, key) == key:
                        break
                    rows[i] = M.zipf_rows(rs, n_rows[t], 1, alpha, perms[t])[0]
                    redrawn += attempt == 0
                else:
                    raise AssertionError("no conflict-free row for table %d in 1000 draws" % t)
            bags[b][t] = rows
    indices = [np.concatenate([bags[b][t] for b in range(batch)]).astype(np.int64) for t in range(T)]
    offsets = [np.concatenate([[0], np.cumsum(sizes[:-1, t])]).astype(np.int64) for t in range(T)]
    assert not new_key_conflicts(model, keys_of(indices))
    return offsets, indices, model.batch_bags(offsets, indices), redrawn


def conflict_free_bag_stream(policy, cap, n_rows, batch, max_bag, n_batches, seed, alpha=1.3):
    """-> (calls: n_batches tuples (offsets, indices, flags), the model after the last call, the fraction of positions that
    were drawn again)"""
    rs = np.random.RandomState(seed)
    perms = [rs.permutation(n) for n in n_rows]
    model = BagPolicyModel(policy, cap, n_rows)
    calls, redrawn, total = [], 0, 0
    for _ in range(n_batches):
        off, idx, flags, r = conflict_free_bags(model, rs, perms, batch, max_bag, alpha)
        calls.append((off, idx, flags))
        redrawn += r
        total += sum(len(i) for i in idx)
    return calls, model, redrawn / max(total, 1)
