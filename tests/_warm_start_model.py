"""The placement rule of a warm start (include/evstore_hip.h: evs_cache_load_plan) restated in Python (test infrastructure;
imported like _batched_policy_model.py, on whose geometry / set_of / stamp_bits_of it builds).

  entries  rows of (table_1based, row, score, age, slot); state: the exporter's 16 words or None
  strict   every entry to its own slot (which must lie in the key's set), ages as they are
  else     each key's set in THIS geometry, ages clamped to 2^S - 2, sorted by (set, score descending, age ascending, table,
           row); the first 8 of a set take ways 0 .. 7, the rest are turned away
  word     tag + 1 | stamp << tag_bits | high field << 26, select bit 0, stamp = (stamp of batch n - age) mod 2^S:
           EvLFU stamps batch n with (n mod 0x7ffffffe) + 1, priority in the high field; LFU with n, counter in the high field;
           LRU with n, whose bits above the low field go into the high field
  n        state[6], or without a state the largest (clamped) age"""
import numpy as np

from _batched_policy_model import CNT_MAX, WAYS, geometry, set_of, stamp_bits_of

POLICY_ID = {"evlfu": 0, "lru": 1, "lfu": 2}


class Refused(ValueError):
    pass


def place(table0, row, nset, n_rows, bits):
    """-> (set, tag + 1) of key (table 0-based, row): the permuted key modulo / over the set count (set_of's arithmetic)"""
    base = int(np.sum(np.asarray(n_rows[:table0], np.int64)))
    mask, half = (1 << bits) - 1, (bits + 1) // 2
    x = ((base + int(row)) * 0x9E3779B1) & mask
    x ^= x >> half
    x = (x * 0x85EBCA6B) & mask
    x ^= x >> half
    assert x % nset == int(set_of(table0, row, nset, n_rows, bits))
    return x % nset, x // nset + 1


def cur_stamp(policy, S, n):
    return ((n % 0x7ffffffe) + 1 if policy == "evlfu" else n) & ((1 << S) - 1)


def word(policy, cap, n_rows, n, tag1, score, age):
    tb, dual, S = stamp_bits_of(policy, cap, n_rows)
    low_bits = 26 - dual - tb
    stamp = (cur_stamp(policy, S, n) - age) & ((1 << S) - 1)
    high = score if policy != "lru" else stamp >> low_bits
    return tag1 | ((stamp & ((1 << low_bits) - 1)) << tb) | (high << 26)


def plan(policy, cap, n_rows, entries, state=None, strict=False):
    """-> (dest (n,) int64: slot or -1, words (n,) uint32, [placed, turned away, S, n]); Refused(reason) for what the plan refuses"""
    entries = np.asarray(entries, np.int64).reshape(-1, 5)
    T = len(n_rows)
    nset, bits = geometry(cap, n_rows)
    _tb, _dual, S = stamp_bits_of(policy, cap, n_rows)
    if strict and state is None:
        raise Refused("strict without a state")
    if state is not None:
        if state[0] != 1:
            raise Refused("version")
        if state[1] != POLICY_ID[policy]:
            raise Refused("policy")
        if strict and (state[2] != cap or state[3] != T or state[12] != S):
            raise Refused("geometry")
    lo, hi = {"evlfu": (0, T), "lru": (0, 0), "lfu": (1, CNT_MAX)}[policy]
    cands, seen = [], set()
    n = int(state[6]) if state is not None else 0
    for i, (t1, row, score, age, slot) in enumerate(entries.tolist()):
        if not 1 <= t1 <= T:
            raise Refused("table")
        if not 0 <= row < n_rows[t1 - 1]:
            raise Refused("row")
        if not lo <= score <= hi:
            raise Refused("score")
        if age < 0:
            raise Refused("age")
        if (t1, row) in seen:
            raise Refused("duplicate")
        seen.add((t1, row))
        s, tag1 = place(t1 - 1, row, nset, n_rows, bits)
        if not strict:
            age = min(age, (1 << S) - 2)
        if state is None:
            n = max(n, age)
        cands.append((s, -score, age, t1, row, i, tag1, slot))
    dest = np.full(len(cands), -1, np.int64)
    if strict:
        for s, _ms, _age, _t1, _row, i, _tag1, slot in cands:
            if not 0 <= slot < nset * WAYS or slot // WAYS != s:
                raise Refused("slot")
            dest[i] = slot
        if len(set(dest.tolist())) != len(cands):
            raise Refused("slot taken twice")
    else:
        rank = {}
        for s, _ms, _age, _t1, _row, i, _tag1, _slot in sorted(cands):
            k = rank.get(s, 0)
            rank[s] = k + 1
            if k < WAYS:
                dest[i] = s * WAYS + k
    words = np.zeros(len(cands), np.uint32)
    for s, ms, age, _t1, _row, i, tag1, _slot in cands:
        if dest[i] >= 0:
            words[i] = word(policy, cap, n_rows, n, tag1, -ms, age)
    placed = int((dest >= 0).sum())
    return dest, words, [placed, len(cands) - placed, S, n]


def resident_after(entries, dest):
    """{(table_1based, row): (score, slot)} of what a plan placed"""
    entries = np.asarray(entries, np.int64).reshape(-1, 5)
    return {(int(e[0]), int(e[1])): (int(e[2]), int(d)) for e, d in zip(entries, dest) if d >= 0}


def random_entries(rs, policy, n_rows, n, max_age):
    """n distinct keys with in-range scores and ages below max_age (slot column 0)"""
    T = len(n_rows)
    keys = set()
    while len(keys) < n:
        t = int(rs.randint(T))
        keys.add((t + 1, int(rs.randint(n_rows[t]))))
    lo, hi = {"evlfu": (0, T), "lru": (0, 0), "lfu": (1, CNT_MAX)}[policy]
    keys = sorted(keys)
    rs.shuffle(keys)
    return np.array([[t1, row, rs.randint(lo, hi + 1), rs.randint(max_age), 0] for t1, row in keys], np.int64).reshape(-1, 5)
