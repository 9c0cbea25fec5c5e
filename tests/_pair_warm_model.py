"""The geometry of a C1 + C2 pair that shares its set records (csrc/evs_cache.hip: sa_pair_geometry, csrc/evs_hash.h) and the
placement rule of its warm start (include/evstore_hip.h: evs_cache_pair_load_plan) restated in Python (test infrastructure).

  records   nset = max(cap1 // 8, ceil(cap2 / 16)) records of 32 words; C1 min(cap1 // nset, 16) ways at word 0; C2
            min(cap2 // nset, 16) ways behind them (from the next multiple of 4 words), 16 as TWO sub-sets of 8; a tier with
            fewer than 4 ways: no shared record
  universe  the dense row number over tables of max(n_rows1, n_rows2) rows, permuted by two rounds of odd multiply + xorshift
  key       x = P(gid); set = x % nset, q = x // nset; effective set = (set << s) | (q & (2^s - 1)), tag + 1 = (q >> s) + 1,
            s = log2 of the tier's sub-sets; slot = effective set * ways + way
  word      tag + 1 | stamp << tag_bits | priority << 26, stamp bits S = 26 - tag_bits (one arena row per way: no select bit);
            batch n is stamped (n mod 0x7ffffffe) + 1 mod 2^S
  entries   rows of (tier 1 | 2, table_1based, row, score, age, slot); state: the exporter's 32 words or None
  strict    every entry to its own slot of its own tier (which must lie in the key's effective set), ages as they are
  else      a key stays in its tier; its effective set in THIS geometry, ages clamped to 2^S - 2, per effective set the `ways`
            best of (score descending, age ascending, table, row) take ways 0 .. ways - 1, the rest are turned away
  n         per tier the state's, or without a state the largest clamped age over both tiers"""
import numpy as np

VERSION = 3
TIER0, BLOCK = 4, 12          # state32: the first tier block and its length
B_CAP, B_CODEC, B_WAYS, B_SUBS, B_S, B_N, B_FLUSH, B_EVICT, B_REQ, B_PERFECT, B_HITS = range(11)


class Refused(ValueError):
    pass


class Tier:
    def __init__(self, cap, ways, sub_shift, w_off, tag_bits):
        self.cap, self.ways, self.sub_shift, self.w_off, self.tag_bits = cap, ways, sub_shift, w_off, tag_bits
        self.S = 26 - tag_bits


class Geometry:
    """-> .nset, .bits, .base (gid of row 0 per table), .tiers = (Tier, Tier); None-like (raises Refused) without a shared record"""

    def __init__(self, cap1, cap2, n_rows1, n_rows2=None):
        n_rows2 = n_rows1 if n_rows2 is None else n_rows2
        rows = [max(a, b) for a, b in zip(n_rows1, n_rows2)]
        self.n_rows = (list(n_rows1), list(n_rows2))
        self.T = len(rows)
        self.base = [0] + list(np.cumsum(rows)[:-1].astype(int))
        total = int(sum(rows))
        self.bits = 1
        while (1 << self.bits) < total:
            self.bits += 1
        nset = max(cap1 // 8, (cap2 + 15) // 16, 1)
        w1, w2, sub2 = min(cap1 // nset, 16), min(cap2 // nset, 16), 0
        if w2 == 16:
            w2, sub2 = 8, 1
        if w1 < 4 or w2 < 4:
            raise Refused("no shared record")
        self.nset = nset

        def tag_bits(sub_shift):
            max_tag1 = ((((1 << self.bits) - 1) // nset) >> sub_shift) + 1
            tb = 1
            while tb < 32 and (max_tag1 >> tb):
                tb += 1
            return tb

        self.tiers = (Tier(cap1, w1, 0, 0, tag_bits(0)), Tier(cap2, w2, sub2, (w1 + 3) // 4 * 4, tag_bits(sub2)))

    def perm(self, table0, row):
        mask, half = (1 << self.bits) - 1, (self.bits + 1) // 2
        x = ((self.base[table0] + int(row)) * 0x9E3779B1) & mask
        x ^= x >> half
        x = (x * 0x85EBCA6B) & mask
        x ^= x >> half
        return x

    def record(self, table0, row):
        return self.perm(table0, row) % self.nset

    def place(self, tier, table0, row):
        """-> (effective set, tag + 1) of the key in tier 1 | 2"""
        t = self.tiers[tier - 1]
        x = self.perm(table0, row)
        s, q = x % self.nset, x // self.nset
        return (s << t.sub_shift) | (q & ((1 << t.sub_shift) - 1)), (q >> t.sub_shift) + 1

    def n_slots(self, tier):
        t = self.tiers[tier - 1]
        return (self.nset << t.sub_shift) * t.ways

    def word_index(self, tier, slot):
        """where the way word of a slot sits in the shared records (words)"""
        t = self.tiers[tier - 1]
        es, way = divmod(slot, t.ways)
        return (es >> t.sub_shift) * 32 + t.w_off + (es & ((1 << t.sub_shift) - 1)) * t.ways + way


def cur_stamp(S, n):
    return ((n % 0x7ffffffe) + 1) & ((1 << S) - 1)


def word(tier, n, tag1, score, age):
    stamp = (cur_stamp(tier.S, n) - age) & ((1 << tier.S) - 1)
    return tag1 | (stamp << tier.tag_bits) | (score << 26)


def state_of(geom, n=0, dim=36, codecs=(8, 4), counters=(0, 0, 0, 0, 0), version=VERSION):
    st = np.zeros(32, np.int64)
    st[:4] = [version, geom.T, dim, geom.nset]
    for k, t in enumerate(geom.tiers):
        st[TIER0 + k * BLOCK:TIER0 + k * BLOCK + 11] = [t.cap, codecs[k], t.ways, 1 << t.sub_shift, t.S, n] + list(counters)
    return st


def plan(geom, entries, state=None, strict=False):
    """-> (dest (n,) int64: slot in the entry's tier or -1, words (n,) uint32, out8); Refused(reason) for what the plan refuses"""
    entries = np.asarray(entries, np.int64).reshape(-1, 6)
    T = geom.T
    if strict and state is None:
        raise Refused("strict without a state")
    n_of = [0, 0]
    if state is not None:
        if state[0] != VERSION:
            raise Refused("version")
        for k, t in enumerate(geom.tiers):
            b = state[TIER0 + k * BLOCK:TIER0 + (k + 1) * BLOCK]
            if b[B_N] < 0:
                raise Refused("batch number")
            n_of[k] = int(b[B_N])
            if strict and (state[1] != T or state[3] != geom.nset or b[B_CAP] != t.cap or b[B_WAYS] != t.ways
                           or b[B_SUBS] != 1 << t.sub_shift or b[B_S] != t.S):
                raise Refused("geometry")
    cands, seen, age_max = ([], []), (set(), set()), 0
    for i, (tier, t1, row, score, age, slot) in enumerate(entries.tolist()):
        if tier not in (1, 2):
            raise Refused("tier")
        if not 1 <= t1 <= T:
            raise Refused("table")
        if not 0 <= row < geom.n_rows[tier - 1][t1 - 1]:
            raise Refused("row")
        if not 0 <= score <= T:
            raise Refused("score")
        if age < 0:
            raise Refused("age")
        if (t1, row) in seen[tier - 1]:
            raise Refused("duplicate")
        if (t1, row) in seen[2 - tier]:
            raise Refused("both tiers")
        seen[tier - 1].add((t1, row))
        es, tag1 = geom.place(tier, t1 - 1, row)
        if not strict:
            age = min(age, (1 << geom.tiers[tier - 1].S) - 2)
        age_max = max(age_max, age)
        cands[tier - 1].append((es, -score, age, t1, row, i, tag1, slot))
    if state is None:
        n_of = [age_max, age_max]
    dest = np.full(len(entries), -1, np.int64)
    words = np.zeros(len(entries), np.uint32)
    placed = [0, 0]
    for k, t in enumerate(geom.tiers):
        if strict:
            taken = set()
            for es, _ms, _age, _t1, _row, i, _tag1, slot in cands[k]:
                if not 0 <= slot < geom.n_slots(k + 1) or slot // t.ways != es:
                    raise Refused("slot")
                if slot in taken:
                    raise Refused("slot taken twice")
                taken.add(slot)
                dest[i] = slot
        else:
            rank = {}
            for es, _ms, _age, _t1, _row, i, _tag1, _slot in sorted(cands[k]):
                r = rank.get(es, 0)
                rank[es] = r + 1
                if r < t.ways:
                    dest[i] = es * t.ways + r
        for es, ms, age, _t1, _row, i, tag1, _slot in cands[k]:
            if dest[i] >= 0:
                words[i] = word(t, n_of[k], tag1, -ms, age)
                placed[k] += 1
    out8 = [placed[0], len(cands[0]) - placed[0], geom.tiers[0].S, placed[1], len(cands[1]) - placed[1], geom.tiers[1].S, n_of[0], 0]
    return dest, words, out8


def random_entries(rs, geom, n1, n2, max_age):
    """n1 + n2 distinct keys, the first n1 in tier 1, with in-range scores and ages below max_age (slot column 0), shuffled"""
    T = geom.T
    rows = [min(a, b) for a, b in zip(*geom.n_rows)]
    keys = set()
    while len(keys) < n1 + n2:
        t = int(rs.randint(T))
        keys.add((t + 1, int(rs.randint(rows[t]))))
    keys = sorted(keys)
    rs.shuffle(keys)
    out = [[1 if i < n1 else 2, t1, row, rs.randint(0, T + 1), rs.randint(max_age), 0] for i, (t1, row) in enumerate(keys)]
    rs.shuffle(out)
    return np.array(out, np.int64).reshape(-1, 6)


def keys_of_set(geom, tier, es, count, skip=()):
    """the first `count` keys, in (table, row) order, whose effective set in `tier` is es"""
    out = []
    for t in range(geom.T):
        for row in range(min(geom.n_rows[0][t], geom.n_rows[1][t])):
            if (t + 1, row) not in skip and geom.place(tier, t, row)[0] == es:
                out.append((t + 1, row))
                if len(out) == count:
                    return out
    raise AssertionError("too few keys in effective set %d of tier %d" % (es, tier))
