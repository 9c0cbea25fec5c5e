"""The bag form of the batched C1 + C2 pair (include/evstore_hip.h: evs_cache_lookup_bags_c1c2) restated in Python over
tests/_pair_warm_model.py's Geometry (test infrastructure).

  state     per tier {slot: [table_1based, row, score]}, made from the 'entries' of an export (export_state_c1c2)
  judge     one call against the state as a snapshot: per position the tier code (1 | 2 | 0) and the serve byte, per sample
            agg_hit = its served bags, per tier the missed keys listed for it with the maximum of agg_hit over their positions,
            the route filter restated (mix64 of the key into 2^20 words: a C2-listed odd-table key whose word a C1-routed
            odd-table key of the call stamped is not inserted)
  pooled    per bag the fp32 sum, in index order from +0, of the rows decoded by the serving tier of each position
  apply     the state after the call ON A CONFLICT-FREE CALL: every hit way to max(old, agg_hit), then every listed key into
            its own set -- the free way of the lowest index, else the way of the lowest score, lowest index among equals
  stream    conflict-free ragged calls: every new key is named by ONE position of the call and the new keys of a call fall
            into different set records (so at most one per C1 set and per effective C2 set, and none is routed both ways);
            every other position names a resident key"""
import numpy as np

ROUTE_WORDS = 1 << 20
M64 = (1 << 64) - 1


def mix64(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def route_word(table1, row):
    return mix64((table1 << 32) | row) & (ROUTE_WORDS - 1)


class State:
    def __init__(self, geom, entries=()):
        self.geom = geom
        self.slots = ({}, {})
        for tier, t1, row, score, _age, slot in np.asarray(entries, np.int64).reshape(-1, 6).tolist():
            assert slot not in self.slots[tier - 1]
            self.slots[tier - 1][slot] = [t1, row, score]

    def keys(self, tier):
        """{(table_1based, row): slot}"""
        return {(e[0], e[1]): s for s, e in self.slots[tier - 1].items()}

    def triples(self):
        return {(k + 1, e[0], e[1], e[2]) for k in (0, 1) for e in self.slots[k].values()}

    def ways_of(self, tier, es):
        w = self.geom.tiers[tier - 1].ways
        return [self.slots[tier - 1].get(es * w + j) for j in range(w)]

    def c1_room(self, table0, row):
        return any(e is None for e in self.ways_of(1, self.geom.place(1, table0, row)[0]))


class Judged:
    pass


def judge(state, B, offsets, indices, thr):
    """offsets: T arrays of B bag starts; indices: T int arrays.  -> Judged: .code / .serve / .pos_sample (T arrays), .agg (B,),
    .bad, .hits (h1, h2), .perfect, .listed ({key: priority} per tier, before the route filter), .insert (after it),
    .bags (T lists of B (start, end))"""
    g = state.geom
    T = g.T
    in1, in2 = state.keys(1), state.keys(2)
    j = Judged()
    j.code, j.serve, j.pos_sample, j.bags = [], [], [], []
    j.bad = False
    missed = np.zeros(B, np.int64)
    looked = np.zeros(B, bool)
    ok_of = []
    for k in range(T):
        idx = np.asarray(indices[k], np.int64)
        off = np.asarray(offsets[k], np.int64)
        n = len(idx)
        lim = min(g.n_rows[0][k], g.n_rows[1][k])
        ok = (idx >= 0) & (idx < lim)
        j.bad = j.bad or bool((~ok).any())
        code = np.zeros(n, np.uint8)
        for p in range(n):
            if ok[p]:
                key = (k + 1, int(idx[p]))
                code[p] = 1 if key in in1 else (2 if key in in2 else 0)
        ps = np.full(n, -1, np.int64)
        bags = []
        for b in range(B):
            st, en = int(off[b]), (int(off[b + 1]) if b + 1 < B else n)
            if not (st >= 0 and en >= st and en <= n):
                j.bad = True
                st = en = 0
            bags.append((st, en))
            ps[st:en] = b
            looked[b] = looked[b] or en > st
            if (code[st:en] == 0).any():
                missed[b] += 1
        j.code.append(code)
        j.serve.append(code.copy())
        j.pos_sample.append(ps)
        j.bags.append(bags)
        ok_of.append(ok)
    j.agg = T - missed
    j.perfect = int((looked & (j.agg == T)).sum())
    j.hits = (int(sum((c == 1).sum() for c in j.code)), int(sum((c == 2).sum() for c in j.code)))
    j.listed = ({}, {})
    j.raise_to = ({}, {})                  # per tier {slot: the largest agg_hit of a position that names it}
    for k in range(T):
        idx = np.asarray(indices[k], np.int64)
        for p in range(len(idx)):
            a = int(j.agg[j.pos_sample[k][p]]) if j.pos_sample[k][p] >= 0 else 0
            key = (k + 1, int(idx[p]))
            if j.code[k][p]:
                tier = int(j.code[k][p])
                slot = (in1 if tier == 1 else in2)[key]
                j.raise_to[tier - 1][slot] = max(j.raise_to[tier - 1].get(slot, 0), a)
            elif ok_of[k][p]:
                dest = 1 if state.c1_room(k, key[1]) else ((1 if k % 2 == 1 else 2) if a < thr else 2)
                j.serve[k][p] = dest
                j.listed[dest - 1][key] = max(j.listed[dest - 1].get(key, -1), a)
    stamped = {route_word(*key) for key in j.listed[0] if (key[0] - 1) % 2 == 1}
    j.filtered = {key for key in j.listed[1] if (key[0] - 1) % 2 == 1 and route_word(*key) in stamped}
    j.insert = (dict(j.listed[0]), {k_: v for k_, v in j.listed[1].items() if k_ not in j.filtered})
    return j


def is_conflict_free(state, j):
    """at most one listed key per C1 set and per effective C2 set, and no key routed both ways"""
    g = state.geom
    if set(j.listed[0]) & set(j.listed[1]):
        return False
    for tier in (1, 2):
        sets = [g.place(tier, t1 - 1, row)[0] for (t1, row) in j.listed[tier - 1]]
        if len(set(sets)) != len(sets):
            return False
    return True


def pooled(j, indices, dec1, dec2, B):
    """dec1 / dec2: per table the (n_rows, d) fp32 rows each tier serves -> (T, B, d) fp32"""
    T, d = len(indices), dec1[0].shape[1]
    out = np.zeros((T, B, d), np.float32)
    for k in range(T):
        idx = np.asarray(indices[k], np.int64)
        for b, (st, en) in enumerate(j.bags[k]):
            acc = np.zeros(d, np.float32)
            for p in range(st, en):
                if j.serve[k][p] == 1:
                    acc = acc + dec1[k][idx[p]]
                elif j.serve[k][p] == 2:
                    acc = acc + dec2[k][idx[p]]
            out[k, b] = acc
    return out


def apply(state, j):
    """the state after a conflict-free call (in place)"""
    g = state.geom
    for k in (0, 1):
        for slot, a in j.raise_to[k].items():
            e = state.slots[k][slot]
            e[2] = max(e[2], a)
    for k in (0, 1):
        t = g.tiers[k]
        for (t1, row), prio in j.insert[k].items():
            es = g.place(k + 1, t1 - 1, row)[0]
            ways = state.ways_of(k + 1, es)
            free = [w for w, e in enumerate(ways) if e is None]
            way = free[0] if free else min(range(t.ways), key=lambda w: (ways[w][2], w))
            state.slots[k][es * t.ways + way] = [t1, row, prio]
    return state


def conflict_free_call(rs, state, used, B, max_len=4, n_new=None, spread=False):
    """One ragged call whose outcome does not depend on timing -> (offsets, indices): T int64 arrays each.  Bags of 0 .. max_len
    resident keys (a table without a resident key gets empty bags); n_new keys nobody has named yet (`used`, updated), in
    different set records, each put into one bag of its table at a random place.  spread: the new keys go to different samples
    (n_new <= B) -- with n_new = B no sample is served everywhere, no priority reaches T and nothing ever flushes."""
    g = state.geom
    T = g.T
    rows = [min(a, b) for a, b in zip(*g.n_rows)]
    resident = sorted(set(state.keys(1)) | set(state.keys(2)))
    by_table = [[r for (t1, r) in resident if t1 == t + 1] for t in range(T)]
    bags = [[[int(r) for r in rs.choice(by_table[t], rs.randint(0, max_len + 1))] if by_table[t] else [] for _b in range(B)]
            for t in range(T)]
    n_new = min(B, g.nset) // 2 if n_new is None else n_new
    assert not spread or n_new <= B
    order = rs.permutation(B)
    recs = set()
    for _ in range(n_new):
        for _try in range(10000):
            t = int(rs.randint(T))
            r = int(rs.randint(rows[t]))
            rec = g.record(t, r)
            if (t + 1, r) not in used and rec not in recs:
                break
        else:
            break
        if spread:                                     # new key i into a bag of sample order[i]: no sample is served everywhere
            bag = bags[t][order[len(recs) % B]]
            if len(bag) >= max_len:
                bag.pop()
        else:
            short = [bag for bag in bags[t] if len(bag) < max_len]
            if not short:
                continue
            bag = short[int(rs.randint(len(short)))]
        recs.add(rec)
        used.add((t + 1, r))
        bag.insert(int(rs.randint(len(bag) + 1)), r)
    used |= {(t + 1, r) for t in range(T) for bag in bags[t] for r in bag}
    offsets = [np.cumsum([0] + [len(b) for b in bags[t][:-1]]).astype(np.int64) for t in range(T)]
    indices = [np.array([r for b in bags[t] for r in b], np.int64) for t in range(T)]
    return offsets, indices
