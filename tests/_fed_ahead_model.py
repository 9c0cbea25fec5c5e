"""Several fed calls open at once (evs_cache_set_fed_depth; include/evstore_hip.h there) restated in Python (test infrastructure;
imported like _batched_policy_model.py).  FedAheadModel wraps BatchedPolicyModel ('lru' / 'lfu') or BagEvLFUModel ('evlfu', its
(B, T) form through one_per_bag) and cuts the wrapped model's one call in two:

  begin(reqs)   batch n = the next one.  Flags = residency in the tier as it stands (every finished call applied, no open one);
                the call records the ways it hit as (set, way) -- they are HELD until it ends --, its distinct missed keys in order
                of first appearance (evlfu: with the largest agg_hit of the requests that name them) and a record per missed position
  finish(call)  the OLDEST open call, on its own batch number: the touch (lru / lfu) or the raise (evlfu) of the ways it hit, then
                every missed key once: a key that is resident by now -- an earlier call installed it -- is skipped (evlfu: its
                priority folded to the maximum) and counted once per record in `found_installed`; else the wrapped model's
                ranking with the ways the OTHER open calls hold left out; no way left: turned away
  abort()       the NEWEST open call is forgotten; its batch number is given back

Driven begin, finish, begin, finish it is the wrapped model, flag for flag and way for way.  `passed_over` counts the inserts
whose way differs from the one the ranking without holds would have taken (a turned-away key included).

ahead_stream draws a stream for a given depth whose outcome does not depend on timing: a batch is drawn at its begin and judged on
a deep copy of the model on which the begin is made and the older open calls are finished first; positions are drawn again until
the batch's own finish meets at most one of its missed keys in any set -- conflict_free_batch's rule, judged at the state the
finish will see (a key found installed there counts: a new key of its set could take its way first).  For evlfu the top bucket stays below 95 % of the capacity (no flush), asserted as _fed_backing_common._bt_stream asserts it."""
import copy
import functools

import numpy as np

import _bag_evlfu_model as EM
import _batched_policy_model as M


class FedAheadModel:
    def __init__(self, policy, cap, n_rows):
        assert policy in ("evlfu", "lru", "lfu")
        self.policy, self.cap, self.n_rows, self.T = policy, cap, [int(n) for n in n_rows], len(n_rows)
        self.m = EM.BagEvLFUModel(cap, n_rows) if policy == "evlfu" else M.BatchedPolicyModel(policy, cap, n_rows)
        self.open = []                         # the open calls, oldest first
        self.found_installed = 0
        self.passed_over = 0
        self.ahead_begins = 0
        self.n_requests = self.n_hits = self.n_perfect = 0   # of the finished calls, as evs_cache_batch_stats counts them

    # ---- the wrapped model's state
    def resident(self):
        return self.m.resident()

    def _set_of(self, key):
        return int(M.set_of(key[0] - 1, key[1], self.m.nset, self.n_rows, self.m.bits))

    def _is_key(self, key):
        return 0 <= key[1] < self.n_rows[key[0] - 1]

    def held_by_others(self, call):
        held = set()
        for c in self.open:
            if c is not call:
                held |= c["hits"]
        return held

    # ---- begin / finish / abort
    def begin(self, reqs):
        reqs = np.asarray(reqs)
        B, T = reqs.shape
        m = self.m
        m.n += 1
        flags = np.zeros((B, T), bool)
        hits, hit_pos, missed, records = set(), [], {}, []
        for b in range(B):
            keys = [(t + 1, int(reqs[b, t])) for t in range(T)]
            at = [m.where.get(k) if self._is_key(k) else None for k in keys]
            agg = sum(a is not None for a in at)
            for t in range(T):
                if at[t] is not None:
                    flags[b, t] = True
                    hits.add(at[t])
                    hit_pos.append((keys[t], at[t], agg))
                elif self._is_key(keys[t]):
                    missed[keys[t]] = max(missed.get(keys[t], 0), agg)
                    records.append(keys[t])
        call = dict(n=m.n, reqs=reqs, flags=flags, hits=hits, hit_pos=hit_pos, missed=missed, records=records)
        if self.open:
            self.ahead_begins += 1
        self.open.append(call)
        return flags, call

    def _rank(self, ways, s, held, n):
        """the way a new key of set s takes in batch n with the ways in `held` left out, or None"""
        for j, w in enumerate(ways):
            if w is None:
                return j                                   # (a free way is never held)
        m = self.m
        if self.policy == "evlfu":
            best = None
            for j, w in enumerate(ways):
                if w[2] == n or (s, j) in held:
                    continue
                if best is None or w[1] < ways[best][1]:
                    best = j
            return best
        ids = {id(ways[j]) for (ss, j) in held if ss == s}
        return m._rank(ways, lambda w: 0 if id(w) in ids else m._age(w[2]))

    def finish(self, call):
        assert self.open and call is self.open[0], "finishes come oldest first"
        m = self.m
        held = self.held_by_others(call)
        latest, m.n = m.n, call["n"]
        n = call["n"]
        try:
            for key, (s, j), agg in call["hit_pos"]:          # the touch / the raise of the ways the begin hit
                w = m.sets[s][j]
                assert w is not None and w[0] == key, "a way the call hit is gone: %r" % (key,)
                if self.policy == "evlfu":
                    w[1] = max(w[1], agg)
                elif w[2] != n:
                    w[2] = n
                    w[1] = w[1] + 1 if m.cnt_max is None else min(w[1] + 1, m.cnt_max)
                if self.policy != "evlfu":
                    w[3] = n
            seen_installed = {k for k in call["missed"] if k in m.where}
            self.found_installed += sum(1 for k in call["records"] if k in seen_installed)
            new_sets = {}                                     # set -> the missed keys the finish meets there, installed or new
            for key, agg in call["missed"].items():
                if key in seen_installed:
                    new_sets.setdefault(self._set_of(key), []).append(key)
                    assert key in m.where, "a new key of this call took the way of %r first" % (key,)
                    if self.policy == "evlfu":
                        s, j = m.where[key]
                        m.sets[s][j][1] = max(m.sets[s][j][1], agg)
                    continue
                s = self._set_of(key)
                new_sets.setdefault(s, []).append(key)
                ways = m.sets[s]
                j = self._rank(ways, s, held, n)
                if j != self._rank(ways, s, set(), n):
                    self.passed_over += 1
                if j is None:
                    if self.policy == "evlfu":
                        m.n_turned += 1
                    continue
                if ways[j] is not None:
                    del m.where[ways[j][0]]
                    m.n_evict += 1
                ways[j] = [key, agg, n] if self.policy == "evlfu" else [key, 1, n, n]
                m.where[key] = (s, j)
            self.n_requests += call["reqs"].shape[0]
            self.n_hits += int(call["flags"].sum())
            self.n_perfect += int((call["flags"].sum(1) == self.T).sum())
        finally:
            m.n = latest
        self.open.pop(0)
        call["new_sets"] = new_sets
        return new_sets

    def abort(self):
        call = self.open.pop()
        assert self.m.n == call["n"], "the newest call holds the last batch number"
        self.m.n -= 1                                         # (ahead_begins stays: evs_cache_fed_ahead_stats is cumulative)
        return call


def schedule(n_calls, depth):
    """-> [('begin' | 'finish', call index)]: begins until `depth` calls are open, then finish k / begin k + depth alternate, then
    the drain"""
    ops, begun, done = [], 0, 0
    while done < n_calls:
        if begun < n_calls and begun - done < depth:
            ops.append(("begin", begun))
            begun += 1
        else:
            ops.append(("finish", done))
            done += 1
    return ops


def _settle(model, reqs, rs, perms, alpha):
    """Draws positions of `reqs` again, in place, until the batch's own finish meets at most one of its missed keys in any set.
    Judged on a deep copy of `model` on which the begin is made and the older open calls are finished first: a position that hit at
    the begin is free; every other key -- new at the finish, or found installed there: a new key of the same set could take its
    way first, and which of the two records runs first is timing -- must be the only one its set sees.  A draw changes what the
    begin holds, and with that what the older finishes leave, so the copy is made again until a round changes nothing."""
    n_rows, (B, T) = model.n_rows, reqs.shape
    for rounds in range(50):
        trial = copy.deepcopy(model)
        _, call = trial.begin(reqs)
        while trial.open[0] is not call:
            trial.finish(trial.open[0])
        owner, changed = {}, False
        for b in range(B):
            for t in range(T):
                for attempt in range(1000):
                    key = (t + 1, int(reqs[b, t]))
                    if key in model.m.where:                  # a hit at the begin
                        break
                    if owner.setdefault(trial._set_of(key), key) == key:
                        break
                    reqs[b, t] = M.zipf_rows(rs, n_rows[t], 1, alpha, perms[t])[0]
                    changed = True
                else:
                    raise AssertionError("no conflict-free row for table %d in 1000 draws" % t)
        if not changed:
            return
    raise AssertionError("the batch did not settle in 50 rounds")


def ahead_stream(policy, cap, n_rows, batch, n_calls, depth, seed, alpha=1.3):
    """-> (reqs (n_calls, batch, T) int32, flags (n_calls, batch, T) bool, the model after the drain, info): the calls in the order of
    schedule(n_calls, depth).  info: 'passed_over', 'found_installed', 'ahead_begins', 'both_missed' (keys two open calls both
    listed) and 'held_checked' (held ways looked at behind a finish).  AssertionError where a seed does not give such a stream."""
    rs = np.random.RandomState(seed)
    n_rows = [int(n) for n in n_rows]
    T = len(n_rows)
    perms = [rs.permutation(n) for n in n_rows]
    model = FedAheadModel(policy, cap, n_rows)
    all_reqs = np.zeros((n_calls, batch, T), np.int32)
    all_flags = np.zeros((n_calls, batch, T), bool)
    calls = {}
    info = dict(both_missed=0, held_checked=0)
    for op, i in schedule(n_calls, depth):
        if op == "begin":
            reqs = np.stack([M.zipf_rows(rs, n_rows[t], batch, alpha, perms[t]) for t in range(T)], 1).astype(np.int32)
            _settle(model, reqs, rs, perms, alpha)
            all_reqs[i] = reqs
            all_flags[i], calls[i] = model.begin(reqs)
            for older in model.open[:-1]:
                info["both_missed"] += len(set(older["missed"]) & set(calls[i]["missed"]))
        else:
            call = calls[i]
            others = [c for c in model.open if c is not call]
            new_sets = model.finish(call)
            assert all(len(v) == 1 for v in new_sets.values()), "call %d's finish meets two of its missed keys in one set" % (i + 1)
            for c in others:                                  # every way held at a finish is still there after it
                for key, (s, j), _ in c["hit_pos"]:
                    w = model.m.sets[s][j]
                    assert w is not None and w[0] == key
                    info["held_checked"] += 1
            keys = [w[0] for ways in model.m.sets for w in ways if w is not None]
            assert len(set(keys)) == len(keys) == len(model.m.where), "a key is resident twice"
            if policy == "evlfu":
                assert model.m.top_bucket() < int(0.95 * cap), "the stream would flush"
    assert not model.open
    info.update(passed_over=model.passed_over, found_installed=model.found_installed, ahead_begins=model.ahead_begins)
    return all_reqs, all_flags, model, info


@functools.lru_cache(maxsize=None)
def searched_stream(policy, cap, n_rows, batch, n_calls, depth):
    """ahead_stream over the first seed whose stream exercises the feature: at least one held way passed over by an update and at
    least one record found installed.  n_rows: a tuple.  Computed once per process."""
    for seed in range(80):
        try:
            reqs, flags, model, info = ahead_stream(policy, cap, list(n_rows), batch, n_calls, depth, seed)
        except AssertionError:
            continue
        if info["passed_over"] >= 1 and info["found_installed"] >= 1:
            return reqs, flags, model, info
    raise AssertionError("no seed gives the stream")
