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

The kernels keep `last` modulo 2^S in the bits the tag leaves free and compare it circularly; BatchedPolicyModel(stamp_bits=S)
does the same (stamp_bits_of gives S for a geometry), and wrap_stream drives a tier of a few sets through many wraps of it.

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


def stamp_bits_of(policy, cap, n_rows, dual=1):
    """-> (tag_bits, dual, S): the tag width, whether the tier keeps the two-copy arena (bit 25 = the copy-select bit) and the
    width of the batch stamp a way word carries, for a tier ALONE of `cap` entries over tables of `n_rows` rows.  Restates
    csrc/evs_cache.hip, sa_make_universe (2^b >= all rows) and sa_make_geom:
        max_tag1 = (2^b - 1) / nset + 1;  tb = its bit length;  tb > 22: refused (ValueError here);  tb > 21: dual = 0;
        stamp_mask = 2^(26 - dual - tb) - 1
    and csrc/evs_cache_policy.h, pol_layout / pol_stamp_bits: LFU keeps `last` in that field, LRU adds the six bits of the
    counter field, EvLFU ('evlfu') stamps the filling batch into the field as it is (csrc/evs_hash.h: sa_word / sa_stamp)."""
    assert policy in ("lru", "lfu", "evlfu")
    nset, bits = geometry(cap, n_rows)
    tb = (((1 << bits) - 1) // nset + 1).bit_length()
    if tb > 22:
        raise ValueError("tag of %d bits: sa_make_geom refuses the geometry" % tb)
    if tb > 21:
        dual = 0
    return tb, dual, 26 - dual - tb + (6 if policy == "lru" else 0)


EVENTS = ("victim", "passed_over", "count_skipped", "turned_away")


class BatchedPolicyModel:
    """policy 'lru' | 'lfu'.  Ways are [key, counter, last, true_last] lists (None = free); keys are (table_1based, row).
    cnt_max: where the LFU counter saturates (None: never).
    stamp_bits = None: plain integers, last = the batch number itself.
    stamp_bits = S: what the kernels do (csrc/evs_cache_policy.hip).  `last` is held reduced modulo 2^S; the running batch is
    cur = n mod 2^S; a hit way whose stored last equals cur is NOT touched (policy_probe_key: pol_last(L, w) != cur) -- so a
    way last touched exactly k 2^S batches ago keeps its word, the LFU counter included; age = (cur - last) mod 2^S and age 0
    means "not eligible" (policy_insert_one).  true_last is the unreduced number of the batch that hit or filled the way last
    -- what a plain-integer model holds in the same place; last = true_last mod 2^S always.  It decides nothing: `events`
    counts, against the plain rule applied to the SAME ways (same counters, true_last for last), where the modular rule parts:
      victim         a new key takes another way than the plain rule's victim
      passed_over    a set without a free way ranks a victim while one of its ways has age 0 but was not touched by this batch
      count_skipped  (LFU) a hit leaves the counter alone because the stored last equals cur from 2^S batches ago
      turned_away    a new key is turned away though the plain rule had a victim"""

    def __init__(self, policy, cap, n_rows, cnt_max=CNT_MAX, stamp_bits=None):
        assert policy in ("lru", "lfu") and cap >= WAYS
        self.policy, self.n_rows = policy, [int(n) for n in n_rows]
        self.nset, self.bits = geometry(cap, n_rows)
        self.cnt_max, self.stamp_bits = cnt_max, stamp_bits
        self.sets = [[None] * WAYS for _ in range(self.nset)]
        self.where = {}     # key -> (set, way)
        self.n = 0
        self.n_evict = 0
        self.events = dict.fromkeys(EVENTS, 0)

    def sets_of(self, reqs):
        """(B, T) rows -> (B, T) set indices"""
        reqs = np.asarray(reqs)
        t = np.broadcast_to(np.arange(reqs.shape[1]), reqs.shape)
        return set_of(t, reqs, self.nset, self.n_rows, self.bits)

    def _cur(self, n=None):
        n = self.n if n is None else n
        return n if self.stamp_bits is None else n % (1 << self.stamp_bits)

    def _age(self, last):
        a = self._cur() - last
        return a if self.stamp_bits is None else a % (1 << self.stamp_bits)

    def _rank(self, ways, age_of):
        """index of the way a new key takes under the ages age_of(way) gives, or None"""
        for j, w in enumerate(ways):
            if w is None:
                return j
        best, best_rank = None, None
        for j, w in enumerate(ways):
            age = age_of(w)
            if age == 0:
                continue        # touched or filled by the running batch (or, modulo 2^S, looking like it)
            rank = (-age,) if self.policy == "lru" else (w[1], -age)
            if best_rank is None or rank < best_rank:     # (strict: ties go to the lowest way index)
                best, best_rank = j, rank
        return best

    def _victim(self, ways):
        """index of the way a new key takes, or None"""
        j = self._rank(ways, lambda w: self._age(w[2]))
        if self.stamp_bits is not None and all(w is not None for w in ways):
            plain = self._rank(ways, lambda w: self.n - w[3])
            if any(self._age(w[2]) == 0 and w[3] != self.n for w in ways):
                self.events["passed_over"] += 1
            if j is None and plain is not None:
                self.events["turned_away"] += 1
            elif j != plain:
                self.events["victim"] += 1
        return j

    def batch(self, reqs):
        """one call over (B, T) rows -> (B, T) bool hit flags"""
        reqs = np.asarray(reqs)
        B, T = reqs.shape
        self.n += 1
        cur = self._cur()
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
            if w[2] != cur:
                w[2] = cur
                w[1] = w[1] + 1 if self.cnt_max is None else min(w[1] + 1, self.cnt_max)
            elif w[3] != self.n and self.policy == "lfu" and (self.cnt_max is None or w[1] < self.cnt_max):
                self.events["count_skipped"] += 1         # (only with stamp_bits: last == cur from 2^S batches ago)
            w[3] = self.n
        for key, s in missed:                             # insert
            ways = self.sets[s]
            j = self._victim(ways)
            if j is None:
                continue                                  # turned away
            if ways[j] is not None:
                del self.where[ways[j][0]]
                self.n_evict += 1
            ways[j] = [key, 1, cur, self.n]
            self.where[key] = (s, j)
        return hit

    def resident(self):
        """{key: score} as evs_cache_batch_dump reports it: LRU the age in batches (0 = the latest batch; with stamp_bits the
        CIRCULAR age, as the dump computes it with pol_age), LFU the counter"""
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


def wrap_stream(policy, cap, n_rows, S, n_batches, seed, new_key_rate=None, min_batch=2, max_batch=4):
    """A directed conflict-free stream for a tier of a FEW sets whose stamps wrap every 2^S batches
    -> (batches: a list of n_batches (B, T) int32 arrays, min_batch <= B <= max_batch; hits: the modular model's flags per
        batch; model: the modular model after the last batch; parted: its `events` plus 'flags' / 'dumps', the number of
        batches whose flags / resident set and scores differ from a plain-integer model's run side by side on the same
        stream, 'first' the first such batch (None: never), 'wraps' = n_batches / 2^S, 'evictions' and 'turned' (keys
        turned away, lapped way or not)).
    Batch 1 brings one ANCHOR key per table, table t's to set t mod nset.  That is the one batch with two new keys in a set
    (T columns cannot be filled from an empty cache otherwise); the anchors are requested by every batch, so they fill the
    columns, are never eligible, and which of the first ways each took never enters a ranking.  From batch 2 on a batch
    brings at most one new key per set.  Ways behind the anchors: two WARM ways per set (hit in 6 batches of 10), the rest
    SLEEPERS, left alone but for a rare hit (1 batch in 4 * 2^S) -- by way index, whichever key holds the way.  New keys arrive
    at `new_key_rate` per set and batch (default 0.5 / 2^S: sleepers outlive 2^S batches).  When a way's true age reaches a
    multiple of 2^S (it LAPS: the kernels see age 0) its set does one of
      rehit    request the lapped key: the touch is skipped (LFU: the counter stays)
      newkey   bring a new key and touch nothing else: the lapped way is passed over, another way goes
      squeeze  bring a new key and hit every other way: the only stale way is the lapped one, the key is turned away
    -- rehit (3 in 10) or newkey while another way of the set is about to lap, squeeze for the last of such a group: a
    squeeze stamps the whole set with one batch number, so it ends the set's laps for 2^S batches.  Sleepers that share a
    stamp afterwards are hit one per batch until their stamps differ, so each of them laps in a batch of its own.
    A new key has the table of the way it is about to replace, so the tables a set holds stay as the fill left them and a
    column of max_batch cells has room for what a set's action needs; an action that does not fit is left out."""
    rs = np.random.RandomState(seed)
    T, P = len(n_rows), 1 << S
    model = BatchedPolicyModel(policy, cap, n_rows, stamp_bits=S)
    plain = BatchedPolicyModel(policy, cap, n_rows)
    nset = model.nset
    n_anchor = -(-T // nset)
    assert nset <= T and n_anchor + 2 < WAYS and max_batch >= 2, "wrap_stream is for a few sets: anchors must leave ways to fight over"
    rate = 0.5 / P if new_key_rate is None else new_key_rate
    # rows of every (table, set), in a random order, handed out once each
    pools = {}
    for t in range(T):
        rows = np.arange(min(n_rows[t], 4096 * nset))
        ss = set_of(t, rows, nset, n_rows, model.bits)
        for s in range(nset):
            pools[t, s] = list(rs.permutation(rows[ss == s]))
    anchors = [(t + 1, int(pools[t, t % nset].pop())) for t in range(T)]
    gone = {}                                   # (table0, set) -> evicted keys, to come back now and then

    def fresh(t, s):
        g = gone.get((t, s))
        if g and rs.rand() < 0.3:
            return g.pop(rs.randint(len(g)))
        return (t + 1, int(pools[t, s].pop()))

    def lapped(w, n):
        return w is not None and n > w[3] and (n - w[3]) % P == 0

    batches, hits = [], []
    diff = {"flags": 0, "dumps": 0, "first": None}
    turned = 0
    for n in range(1, n_batches + 1):
        cols = [[anchors[t]] for t in range(T)]

        def fits(keys):
            need = [0] * T
            for k in keys:
                need[k[0] - 1] += 1
            return all(len(cols[t]) + need[t] <= max_batch for t in range(T))

        def put(keys):
            for k in keys:
                cols[k[0] - 1].append(k)

        if n > 1:
            for s in rs.permutation(nset):
                ways = model.sets[s]
                others = [j for j, w in enumerate(ways) if w is not None and w[0] not in anchors]
                free = [j for j, w in enumerate(ways) if w is None]
                lap = [j for j in others if lapped(ways[j], n)]
                touch, bring = [], False
                if free:                                           # the fill: one new key per set and batch
                    bring = True
                elif lap:
                    # a squeeze stamps every way of the set with this batch, so the next lap of the set is 2^S batches off:
                    # it is kept for the last way of a group that laps in consecutive batches
                    soon = [j for j in others if j not in lap and (n - ways[j][2]) % P >= P - min(8, P // 4)]
                    act = rs.choice(["rehit", "newkey"], p=[0.3, 0.7]) if soon else "squeeze"
                    if act == "rehit":
                        touch = [lap[rs.randint(len(lap))]]
                    else:
                        bring = True
                        touch = [j for j in others if j not in lap] if act == "squeeze" else []
                else:
                    for j in others:
                        warm = j < n_anchor + 2
                        if rs.rand() < (0.6 if warm else 0.25 / P):
                            touch.append(j)
                    # sleepers that share a stamp (a squeeze touched them together) would lap together: one of them is
                    # hit per batch until their stamps differ again, so every one of them laps in a batch of its own
                    same = {}
                    for j in others:
                        if j >= n_anchor + 2:
                            same.setdefault(ways[j][2], []).append(j)
                    crowd = max(same.values(), key=len) if same else []
                    if len(crowd) > 1 and crowd[-1] not in touch:
                        touch.append(crowd[-1])
                    bring = rs.rand() < rate
                keys = [ways[j][0] for j in touch]
                new = None
                if bring:
                    if free:
                        t0 = (free[0] + s) % T
                    else:      # the table of the way the key will take (the batch's touches known), else of a lapped way
                        was = model.n
                        model.n = n
                        cur = model._cur()
                        hold = [w if (j not in touch and w[0] not in anchors) else [w[0], w[1], cur, n] for j, w in enumerate(ways)]
                        v = model._rank(hold, lambda w: model._age(w[2]))
                        model.n = was
                        t0 = ways[v if v is not None else (lap[0] if lap else others[0])][0][0] - 1
                    new = fresh(t0, s)
                if fits(keys + ([new] if new else [])):
                    put(keys + ([new] if new else []))
                elif new is not None:
                    gone.setdefault((new[0] - 1, s), []).append(new)     # (not brought after all: keep it for later)
        B = max(min_batch, max(len(c) for c in cols))
        reqs = np.array([[c[b % len(c)][1] for c in cols] for b in range(B)], np.int32)
        if n > 1:
            assert not new_key_conflicts(model, reqs), "batch %d" % n
        before = set(model.where)
        h = model.batch(reqs)
        hp = plain.batch(reqs)
        new_keys = {(t + 1, int(reqs[b, t])) for b in range(B) for t in range(T) if not h[b, t]}
        turned += sum(1 for k in new_keys if k not in model.where)
        for k in before - set(model.where):
            gone.setdefault((k[0] - 1, int(set_of(k[0] - 1, k[1], nset, n_rows, model.bits))), []).append(k)
        d_flags, d_dump = not np.array_equal(h, hp), model.resident() != plain.resident()
        diff["flags"] += d_flags
        diff["dumps"] += d_dump
        if (d_flags or d_dump) and diff["first"] is None:
            diff["first"] = n
        batches.append(reqs)
        hits.append(h)
    parted = dict(model.events)
    parted.update(diff)
    parted.update(wraps=n_batches / float(P), evictions=model.n_evict, turned=turned)
    return batches, hits, model, parted


# The geometries whose stamps wrap within a test-sized run (a tier alone): name -> (capacity, rows per table, S per policy as
# sa_make_geom gives it -- the tests assert stamp_bits_of against these), and the streams the GPU tests replay over them:
# (policy, geometry) -> (batches, seed, new_key_rate).  Lengths: LFU ten wraps; LRU on `tiny` a little over four (a squeeze,
# the only source of 'turned_away', comes once per set and wrap); LRU on `tiny-dual` does not wrap in a test-sized run
# (S = 12) -- its 640 batches carry the 6-bit low field of `last` into the high one, across the copy-select bit, ten times
# while a new key per set every 16 batches keeps that bit flipping.  Seeds: tests/test_batched_policy_model.py asserts what
# each stream covers.
WRAP_GEOMETRIES = {
    "tiny": (16, [1040000] * 4, {"evlfu": 4, "lfu": 4, "lru": 10}),
    "tiny-dual": (16, [130000] * 4, {"evlfu": 6, "lfu": 6, "lru": 12}),
    "inline": (128, [40000] * 26, {"evlfu": 8, "lfu": 8, "lru": 14}),
}
WRAP_CASES = {
    ("lfu", "tiny"): (160, 0, None),
    ("lfu", "tiny-dual"): (640, 4, None),
    ("lru", "tiny"): (4200, 0, None),
    ("lru", "tiny-dual"): (640, 0, 1.0 / 16),
}


def wrap_case(policy, geom):
    """-> wrap_stream's results for one of WRAP_CASES"""
    cap, n_rows, S = WRAP_GEOMETRIES[geom]
    n_batches, seed, rate = WRAP_CASES[policy, geom]
    return wrap_stream(policy, cap, n_rows, S[policy], n_batches, seed, new_key_rate=rate)
