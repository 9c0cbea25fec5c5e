"""The batched LRU / LFU rule of the set-associative cache tier restated in Python (test infrastructure; imported like
_accuracy.py).  The rule itself is written down in include/evstore_hip.h (evs_cache_set_batch_policy, "the batched rule"):

  one call = batch n (1, 2, ...):
    probe    hit[b, t] = key (t + 1, rows[b, t]) was resident when the call started
    touch    every way hit at least once: last = n; LFU: counter + 1 ONCE per batch, saturating
    insert   every distinct missed key once, into its own set: a free way first (lowest index); else, among the ways with
             last != n, LRU the oldest last, LFU the lowest counter then the oldest last, then the lowest way index; no
             eligible way: turned away.  A new way: last = n, counter 1.

When two new keys of one batch fall into one set the kernels' outcome depends on timing; the model inserts in order of first
appearance, which is ONE of the allowed outcomes.  On a conflict-free stream (conflict_free_stream below) no batch brings two
new keys to one set, the rule is deterministic and the model predicts every hit flag and the whole resident set.

The set function restates csrc/evs_hash.h (sa_perm / sa_split) and csrc/evs_cache.hip (sa_single_feasible): the dense row
number over all tables through two rounds of odd multiply + xorshift on `bits` bits, modulo capacity // 8 sets."""
import numpy as np

WAYS = 8
CNT_MAX = 63      # the 6-bit counter of a way word


def geometry(cap, n_rows):
    """-> (nset, bits): capacity // 8 sets of 8 ways; the key universe is 2^bits >= all rows of all tables."""
    total = int(sum(n_rows))
    bits = 1
    while (1 << bits) < total:
        bits += 1
    return cap // WAYS, bits


def set_of(table0, row, nset, n_rows, bits):
    """Set index of keys (table 0-based, row); scalars or arrays."""
    base = np.concatenate([[0], np.cumsum(np.asarray(n_rows, np.uint64))]).astype(np.uint64)
    x = base[np.asarray(table0, np.int64)] + np.asarray(row, np.int64).astype(np.uint64)
    mask, half = np.uint64((1 << bits) - 1), np.uint64((bits + 1) // 2)
    x = (x * np.uint64(0x9E3779B1)) & mask
    x = x ^ (x >> half)
    x = (x * np.uint64(0x85EBCA6B)) & mask
    x = x ^ (x >> half)
    return (x % np.uint64(nset)).astype(np.int64)


class BatchedPolicyModel:
    """policy 'lru' | 'lfu'.  Ways are [key, counter, last] lists (None = free); keys are (table_1based, row).
    cnt_max: where the LFU counter saturates (None: never).  stamp_bits: ages are taken modulo 2^stamp_bits like the
    kernels' (None: plain integers -- the same thing while every resident way was touched within 2^stamp_bits - 1 batches)."""

    def __init__(self, policy, cap, n_rows, cnt_max=CNT_MAX, stamp_bits=None):
        assert policy in ("lru", "lfu") and cap >= WAYS
        self.policy, self.n_rows = policy, [int(n) for n in n_rows]
        self.nset, self.bits = geometry(cap, n_rows)
        self.cnt_max, self.stamp_bits = cnt_max, stamp_bits
        self.sets = [[None] * WAYS for _ in range(self.nset)]
        self.where = {}     # key -> (set, way)
        self.n = 0
        self.n_evict = 0

    def sets_of(self, reqs):
        """(B, T) rows -> (B, T) set indices"""
        reqs = np.asarray(reqs)
        t = np.broadcast_to(np.arange(reqs.shape[1]), reqs.shape)
        return set_of(t, reqs, self.nset, self.n_rows, self.bits)

    def _age(self, last):
        a = self.n - last
        return a if self.stamp_bits is None else a % (1 << self.stamp_bits)

    def _victim(self, ways):
        """index of the way a new key takes, or None"""
        for j, w in enumerate(ways):
            if w is None:
                return j
        best, best_rank = None, None
        for j, w in enumerate(ways):
            age = self._age(w[2])
            if age == 0:
                continue        # touched or filled by the running batch
            rank = (-age,) if self.policy == "lru" else (w[1], -age)
            if best_rank is None or rank < best_rank:     # (strict: ties go to the lowest way index)
                best, best_rank = j, rank
        return best

    def batch(self, reqs):
        """one call over (B, T) rows -> (B, T) bool hit flags"""
        reqs = np.asarray(reqs)
        B, T = reqs.shape
        self.n += 1
        sets = self.sets_of(reqs)
        hit = np.zeros((B, T), bool)
        missed, seen = [], set()
        for b in range(B):
            for t in range(T):
                key = (t + 1, int(reqs[b, t]))
                at = self.where.get(key)
                if at is not None:
                    hit[b, t] = True
                elif key not in seen:
                    seen.add(key)
                    missed.append((key, int(sets[b, t])))
        for b, t in zip(*np.nonzero(hit)):                # touch
            s, j = self.where[(t + 1, int(reqs[b, t]))]
            w = self.sets[s][j]
            if w[2] != self.n:
                w[2] = self.n
                w[1] = w[1] + 1 if self.cnt_max is None else min(w[1] + 1, self.cnt_max)
        for key, s in missed:                             # insert
            ways = self.sets[s]
            j = self._victim(ways)
            if j is None:
                continue                                  # turned away
            if ways[j] is not None:
                del self.where[ways[j][0]]
                self.n_evict += 1
            ways[j] = [key, 1, self.n]
            self.where[key] = (s, j)
        return hit

    def resident(self):
        """{key: score} as evs_cache_batch_dump reports it: LRU the age in batches (0 = the latest batch), LFU the counter"""
        out = {}
        for ways in self.sets:
            for w in ways:
                if w is not None:
                    out[w[0]] = self._age(w[2]) if self.policy == "lru" else w[1]
        return out

    def size(self):
        return len(self.where)


def zipf_rows(rs, n, size, alpha, perm):
    return perm[np.minimum(rs.zipf(alpha, size) - 1, n - 1)]


def new_key_conflicts(model, reqs):
    """positions (b, t) of `reqs` whose key is new to `model` and shares its set with a DIFFERENT new key of the batch"""
    reqs = np.asarray(reqs)
    sets = model.sets_of(reqs)
    owner, bad = {}, []
    for b in range(reqs.shape[0]):
        for t in range(reqs.shape[1]):
            key = (t + 1, int(reqs[b, t]))
            if key in model.where:
                continue
            s = int(sets[b, t])
            if owner.setdefault(s, key) != key:
                bad.append((b, t))
    return bad


def conflict_free_batch(model, rs, perms, batch, alpha=1.3):
    """One more batch for `model` (which runs it) -> (reqs (batch, T) int32, hits (batch, T) bool).  Zipf rows per table; a
    position whose key would be the second new key of its set in this batch has its row drawn again, against the model's own
    state, so the batch brings no two new keys to one set."""
    n_rows, T = model.n_rows, len(model.n_rows)
    reqs = np.stack([zipf_rows(rs, n_rows[t], batch, alpha, perms[t]) for t in range(T)], 1).astype(np.int32)
    owner = {}       # set -> the one new key this batch brings to it
    for b in range(batch):
        for t in range(T):
            for attempt in range(1000):
                key = (t + 1, int(reqs[b, t]))
                if key in model.where:
                    break
                s = int(set_of(t, reqs[b, t], model.nset, n_rows, model.bits))
                if owner.setdefault(s, key) == key:
                    break
                reqs[b, t] = zipf_rows(rs, n_rows[t], 1, alpha, perms[t])[0]
            else:
                raise AssertionError("no conflict-free row for table %d in 1000 draws" % t)
    assert not new_key_conflicts(model, reqs)
    return reqs, model.batch(reqs)


def conflict_free_stream(policy, cap, n_rows, batch, n_batches, seed, alpha=1.3, cnt_max=CNT_MAX):
    """-> (reqs (n_batches, batch, T) int32, hits (n_batches, batch, T) bool, model after the last batch): n_batches
    conflict_free_batch draws from one seed."""
    rs = np.random.RandomState(seed)
    perms = [rs.permutation(n) for n in n_rows]
    model = BatchedPolicyModel(policy, cap, n_rows, cnt_max)
    all_reqs = np.zeros((n_batches, batch, len(n_rows)), np.int32)
    all_hits = np.zeros((n_batches, batch, len(n_rows)), bool)
    for i in range(n_batches):
        all_reqs[i], all_hits[i] = conflict_free_batch(model, rs, perms, batch, alpha)
    return all_reqs, all_hits, model
