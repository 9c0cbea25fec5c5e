"""The refusals of the fed begin / finish calls (evs_cache_fed_begin[_bags], evs_cache_fed_finish[_interact],
evs_cache_fed_finish_bags[_interact], evs_cache_fed_abort) and of the other calls on a fed cache, as a table of (name, build) in the
pattern of tests/_batched_refusal_cases.py, whose shapes and helpers it takes: build(E) sets the situation up and returns
(call, after) -- call() must raise EvsError; after(), where there is one, checks what the refusal must have left behind.
tests/golden/make_golden_refusals.py _fed_refusal_cases records code and text of every case into tests/golden/fed_refusals.json;
tests/test_gpu_fed_refusals.py replays the table against that record.

Every refusal of the five entry points that needs no environment switch is here.  Not reachable, and so not in the table:
  - batch_check's "at most 32 tables", "call evs_cache_set_backing first" and an lru / lfu cache over host-memory tables at order
    0: evs_cache_set_fed_backing refuses more than 32 tables, a cache without backing has no fed table, and order 0 is refused
    first; a capacity above the batched maximum would need the arena of such a cache;
  - an approximate threshold on an lru / lfu cache: evs_cache_set_batch_approx refuses it (evlfu: approx_threshold below);
  - everything behind the point where a begin has counted the call (a failed allocation, clear or launch).  No refusal that takes
    the call's ordinal back is reachable without one of these failing, so the twin check stands on the refusals that leave a call
    OPEN instead: after() ends that call with the right finish, and the call after it must give the hit flags and the
    batch_stats of a twin cache that never saw the refusal.

4 tables, d = 16, B = 2, two sets of 8 ways; all four tables fed unless a case says otherwise."""
import ctypes as C
import os
import tempfile

import numpy as np
import torch

import _batched_refusal_cases as BC
from _batched_refusal_cases import B, D, ROWS, RQ, T, _dev, refusal  # noqa: F401  (refusal: what the recorder and the replay call)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _fed_tier(E, policy="lru", cap=16, d=D, order=1, fed=(0, 1, 2, 3), rule=False, count=False, given=None, approx=0, n_rows=ROWS,
              table_offset=0):
    """a tier alone whose tables `fed` have no address; table_offset: the addressed tables start that many bytes into their tensors"""
    c = E.GpuCache(policy, cap, T, d, 32, "cpp")
    if order:
        c.set_miss_order("fetch-first")
    c._kept = [None if k in fed else torch.zeros(n * d + 4, device="cuda")[table_offset // 4:] for k, n in enumerate(n_rows)]
    c.set_fed_backing(c._kept, n_rows)
    if rule:
        c.set_bag_rule("served-bags")
    if count:
        c.set_bag_count("count-first")
    if given:
        c.set_batch_policy(given)
    if approx:
        c.set_batch_approx(approx)
    return c


def _evlfu(E, **kw):
    return _fed_tier(E, "evlfu", rule=True, count=True, **kw)


def _begin(E, c, **bad):
    """evs_cache_fed_begin through the C ABI, one argument made bad -> the number of keys listed"""
    rows, hit = _dev(RQ), torch.empty(B * T, dtype=torch.uint8, device="cuda")
    keys, n = torch.empty(B * T + 1, dtype=torch.int64, device="cuda"), C.c_int64()
    a = {"c": c._h if c is not None else None, "rows": rows.data_ptr(), "hit": hit.data_ptr(),
         "keys": keys.data_ptr() + bad.get("keys_offset", 0), "n": C.byref(n)}
    if "null" in bad:
        a[bad["null"]] = None
    rc = E._lib.lib().evs_cache_fed_begin(a["c"], bad.get("B", B), a["rows"], a["hit"], a["keys"], a["n"], _st())
    E._lib.check(rc)
    c._call = (rows, hit, keys)   # (alive until the finish)
    return int(n.value)


def _begin_bags(E, c, **bad):
    """evs_cache_fed_begin_bags through the C ABI, one argument made bad -> the number of keys listed"""
    idx = [_dev(RQ[:, t].astype(np.int64)) for t in range(T)]
    off = [_dev(np.arange(B, dtype=np.int64)) for _ in range(T)]
    nnz = [B] * T
    ip, op = [t.data_ptr() for t in idx], [t.data_ptr() for t in off]
    if "null_index" in bad:
        ip[bad["null_index"]] = None
    if "null_offset" in bad:
        op[bad["null_offset"]] = None
    for k, v in bad.get("nnz_k", {}).items():
        nnz[k] = v
    hit = torch.empty(B * T, dtype=torch.uint8, device="cuda")
    keys, n = torch.empty(B * T + 1, dtype=torch.int64, device="cuda"), C.c_int64()
    a = {"c": c._h if c is not None else None, "indices": (C.c_void_p * T)(*ip), "offsets": (C.c_void_p * T)(*op),
         "nnz": (C.c_int64 * T)(*nnz), "keys": keys.data_ptr() + bad.get("keys_offset", 0), "n": C.byref(n)}
    if "null" in bad:
        a[bad["null"]] = None
    rc = E._lib.lib().evs_cache_fed_begin_bags(a["c"], bad.get("B", B), a["indices"], a["offsets"], a["nnz"], hit.data_ptr(), a["keys"],
                                                a["n"], _st())
    E._lib.check(rc)
    c._call = (idx, off, hit, keys)
    return int(n.value)


def _finish(E, c, n, bags=False, interact=False, **bad):
    """the finish of either form through the C ABI over a block of n zero rows, one argument made bad"""
    L = E._lib.lib()
    d = c.dim if c is not None else D
    rb, F = d * 4, T + 1
    fed = torch.zeros((n + 2) * (rb + 16), dtype=torch.uint8, device="cuda")
    x, R = torch.zeros(B * d + 4, device="cuda"), torch.zeros(B, d + F * (F - 1) // 2, device="cuda")
    out = torch.zeros(T * B * d + 4, device="cuda")
    a = {"c": c._h if c is not None else None, "fed": fed.data_ptr() + bad.get("fed_offset", 0), "x": x.data_ptr() + bad.get("x_offset", 0),
         "R": R.data_ptr(), "out": out.data_ptr() + bad.get("out_offset", 0)}
    if "null" in bad:
        a[bad["null"]] = None
    stride = bad.get("stride", rb)
    if interact:
        fn = L.evs_cache_fed_finish_bags_interact if bags else L.evs_cache_fed_finish_interact
        rc = fn(a["c"], a["fed"], stride, a["x"], bad.get("x_stride", d), 0, a["R"], _st())
    elif bags:
        rc = L.evs_cache_fed_finish_bags(a["c"], a["fed"], stride, a["out"], bad.get("tstride", B * d), bad.get("bstride", d), _st())
    else:
        rc = L.evs_cache_fed_finish(a["c"], a["fed"], stride, a["out"], _st())
    torch.cuda.synchronize()
    E._lib.check(rc)


def _serves(E, c, bags=False):
    """one call of the form, begin to finish -> its hit flags"""
    n = (_begin_bags if bags else _begin)(E, c)
    flags = c._call[-2].cpu().numpy().copy()
    _finish(E, c, n, bags)
    return flags


def _plain(make, call):
    """a refusal on a cache with no call open; make(E) -> cache (None: the NULL cache)"""
    def build(E):
        c = make(E) if make else None
        return (lambda: call(E, c)), None
    return build


def _open(make, bags, call):
    """a refusal while a call of the form is open: it stays open, the right finish then serves, and the call after it is the twin's"""
    def build(E):
        c = make(E)
        n = (_begin_bags if bags else _begin)(E, c)

        def after():
            twin = make(E)
            _finish(E, c, n, bags)
            _serves(E, twin, bags)
            mine, theirs = _serves(E, c, bags), _serves(E, twin, bags)
            assert np.array_equal(mine, theirs) and mine.any()
            assert c.batch_stats() == twin.batch_stats() and c.fed_stats() == twin.fed_stats()
        return (lambda: call(E, c, n)), after
    return build


def _given(name, bags):
    def build(E):
        c = _evlfu(E, given=name)

        def after():
            assert c.set_batch_policy("setassoc") is c
            _serves(E, c, bags)
        return (lambda: (_begin_bags if bags else _begin)(E, c)), after
    return build


def _ordinary(E, policy="lru"):
    return BC._tier(E, policy, order=1)


def _file_backed(policy):
    def make(E):
        c = E.GpuCache(policy, 16, T, D, 32, "cpp").set_miss_order("fetch-first")
        c._tmp = tempfile.TemporaryDirectory()   # (goes with the cache)
        paths = []
        for k, n in enumerate(ROWS):
            paths.append(os.path.join(c._tmp.name, "ev-table-%d.bin" % (k + 1)))
            np.zeros((n, D), np.float32).tofile(paths[-1])
        c._tier = E.FileTier(paths, D * 4, 0)
        c.set_file_backing(c._tier)
        c.set_fed_backing([None] * T, ROWS)
        return c
    return make


def _tier_of_a_pair(E):
    p = BC._pair(E, 1)
    BC._bt2(E, p)()
    p[0]._partner = p[1]
    return p[0].set_fed_backing([None] * T, ROWS)


def _used_exactly(E):
    c = BC._tier(E, "lru")
    c.request(_dev(RQ))
    c.set_miss_order("fetch-first")
    return c.set_fed_backing([None] * T, ROWS)


def _pair_call(E, c, first):
    other = BC._tier(E, cap=BC.PAIR_CAPS[1], order=1)
    return E.lookup_batch_c1c2(*((c, other) if first else (other, c)), _dev(RQ), threshold=2)


def _bags_call(E, c):
    return BC._bags(E, (c,))


HUGE = [1 << 31] * T   # (2^33 rows over all tables)

BEGIN = [
    ("null_cache", _plain(None, lambda E, c: _begin(E, c))),
    ("null_rows", _plain(_fed_tier, lambda E, c: _begin(E, c, null="rows"))),
    ("null_hit", _plain(_fed_tier, lambda E, c: _begin(E, c, null="hit"))),
    ("null_keys", _plain(_fed_tier, lambda E, c: _begin(E, c, null="keys"))),
    ("null_n_keys", _plain(_fed_tier, lambda E, c: _begin(E, c, null="n"))),
    ("B_zero", _plain(_fed_tier, lambda E, c: _begin(E, c, B=0))),
    ("B_negative", _plain(_fed_tier, lambda E, c: _begin(E, c, B=-3))),
    ("B_too_large", _plain(_fed_tier, lambda E, c: _begin(E, c, B=1 << 26))),
    ("misaligned_keys", _plain(_fed_tier, lambda E, c: _begin(E, c, keys_offset=4))),
    ("no_fed_table", _plain(_ordinary, lambda E, c: _begin(E, c))),
    ("order_0", _plain(lambda E: _fed_tier(E, order=0), lambda E, c: _begin(E, c))),
    ("approx_threshold", _plain(lambda E: _evlfu(E, approx=2), lambda E, c: _begin(E, c))),
    ("capacity_below_a_set", _plain(lambda E: _fed_tier(E, cap=4), lambda E, c: _begin(E, c))),
    ("universe_lru", _plain(lambda E: _fed_tier(E, n_rows=HUGE), lambda E, c: _begin(E, c))),
    ("universe_evlfu", _plain(lambda E: _evlfu(E, n_rows=HUGE), lambda E, c: _begin(E, c))),
    ("used_through_the_exact_path", _plain(_used_exactly, lambda E, c: _begin(E, c))),
    ("file_backed_lru", _plain(_file_backed("lru"), lambda E, c: _begin(E, c))),
    ("file_backed_evlfu", _plain(_file_backed("evlfu"), lambda E, c: _begin(E, c))),
    ("tier_of_a_started_pair", _plain(_tier_of_a_pair, lambda E, c: _begin(E, c))),
    ("plan", _given("plan", False)), ("sampled", _given("sampled", False)),
    ("second_begin", _open(_fed_tier, False, lambda E, c, n: _begin(E, c))),
    ("bag_call_open", _open(_fed_tier, True, lambda E, c, n: _begin(E, c))),
]

BEGIN_BAGS = [
    ("null_cache", _plain(None, lambda E, c: _begin_bags(E, c))),
    ("null_indices", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, null="indices"))),
    ("null_offsets", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, null="offsets"))),
    ("null_nnz", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, null="nnz"))),
    ("null_keys", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, null="keys"))),
    ("null_n_keys", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, null="n"))),
    ("B_zero", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, B=0))),
    ("B_too_large", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, B=1 << 31))),
    ("misaligned_keys", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, keys_offset=4))),
    ("no_fed_table", _plain(_ordinary, lambda E, c: _begin_bags(E, c))),
    ("order_0", _plain(lambda E: _fed_tier(E, order=0), lambda E, c: _begin_bags(E, c))),
    ("approx_threshold", _plain(lambda E: _evlfu(E, approx=2), lambda E, c: _begin_bags(E, c))),
    ("universe_lru", _plain(lambda E: _fed_tier(E, n_rows=HUGE), lambda E, c: _begin_bags(E, c))),
    ("universe_evlfu", _plain(lambda E: _evlfu(E, n_rows=HUGE), lambda E, c: _begin_bags(E, c))),
    ("file_backed_evlfu", _plain(lambda E: _file_backed("evlfu")(E).set_bag_rule("served-bags").set_bag_count("count-first"),
                                 lambda E, c: _begin_bags(E, c))),
    ("tier_of_a_started_pair", _plain(_tier_of_a_pair, lambda E, c: _begin_bags(E, c))),
    ("plan", _given("plan", True)), ("sampled", _given("sampled", True)),
    ("no_bag_rule", _plain(lambda E: _fed_tier(E, "evlfu"), lambda E, c: _begin_bags(E, c))),
    ("no_bag_count", _plain(lambda E: _fed_tier(E, "evlfu", rule=True), lambda E, c: _begin_bags(E, c))),
    ("negative_nnz", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, nnz_k={2: -1}))),
    ("null_indices_k", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, null_index=3))),
    ("null_offsets_k", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, null_offset=1))),
    ("too_many_lookups", _plain(_fed_tier, lambda E, c: _begin_bags(E, c, nnz_k={0: 1 << 30, 1: 1 << 30}))),
    ("dim_pooling", _plain(lambda E: _fed_tier(E, d=18), lambda E, c: _begin_bags(E, c))),
    ("misaligned_table", _plain(lambda E: _fed_tier(E, fed=(0, 1, 3), table_offset=4), lambda E, c: _begin_bags(E, c))),
    ("second_begin", _open(_fed_tier, True, lambda E, c, n: _begin_bags(E, c))),
    ("rows_call_open", _open(_fed_tier, False, lambda E, c, n: _begin_bags(E, c))),
]


def _finishes(bags, interact):
    """the refusals of one finish entry point: no call open, the other form's call open, then the argument errors on its own call"""
    def fin(**bad):
        return lambda E, c, n: _finish(E, c, n, bags, interact, **bad)
    cases = [
        ("null_cache", _plain(None, lambda E, c: _finish(E, c, 0, bags, interact))),
        ("nothing_open", _plain(_fed_tier, lambda E, c: _finish(E, c, 0, bags, interact))),
        ("nothing_open_evlfu", _plain(_evlfu, lambda E, c: _finish(E, c, 0, bags, interact))),
        ("other_form_open", _open(_fed_tier, not bags, fin())),
        ("null_fed", _open(_fed_tier, bags, fin(null="fed"))),
        ("stride_below_the_row", _open(_fed_tier, bags, fin(stride=D * 4 - 16))),
        ("misaligned_fed", _open(_fed_tier, bags, fin(fed_offset=4))),
        ("misaligned_stride", _open(_fed_tier, bags, fin(stride=D * 4 + 4))),
    ]
    if interact:
        cases += [
            ("null_x", _plain(_fed_tier, lambda E, c: _finish(E, c, 0, bags, interact, null="x"))),
            ("null_R", _plain(_fed_tier, lambda E, c: _finish(E, c, 0, bags, interact, null="R"))),
            ("misaligned_x", _open(_fed_tier, bags, fin(x_offset=8))),
            ("x_stride", _open(_fed_tier, bags, fin(x_stride=D + 2))),
            ("interaction_shape", _open(lambda E: _fed_tier(E, d=20), bags, fin())),
        ]
    else:
        cases += [("null_out", _plain(_fed_tier, lambda E, c: _finish(E, c, 0, bags, interact, null="out")))]
        if bags:
            cases += [
                ("table_stride", _open(_fed_tier, bags, fin(tstride=B * D + 2))),
                ("bag_stride", _open(_fed_tier, bags, fin(bstride=D + 1))),
                ("misaligned_pooled", _open(_fed_tier, bags, fin(out_offset=4))),
            ]
    return cases


def _abort(E, c, *_n):
    E._lib.check(E._lib.lib().evs_cache_fed_abort(c._h if c is not None else None))


def _set_backing(E, c, *_n):
    c.set_backing(BC._tables(32))


OTHERS = [
    ("abort/null_cache", _plain(None, _abort)), ("abort/nothing_open", _plain(_fed_tier, _abort)),
    ("abort/nothing_open_evlfu", _plain(_evlfu, _abort)),
    # the one-call lookups on a cache with fed tables
    ("fed_cache/lookup_batch", _plain(_fed_tier, lambda E, c: c.lookup_batch(_dev(RQ)))),
    ("fed_cache/lookup_interact", _plain(_fed_tier, lambda E, c: c.lookup_interact(_dev(RQ), torch.zeros(B, D, device="cuda")))),
    ("fed_cache/lookup_bags", _plain(_fed_tier, _bags_call)),
    ("fed_cache/lookup_bags_evlfu", _plain(_evlfu, _bags_call)),
    ("fed_cache/first_tier_of_a_pair", _plain(_evlfu, lambda E, c: _pair_call(E, c, True))),
    ("fed_cache/second_tier_of_a_pair", _plain(_evlfu, lambda E, c: _pair_call(E, c, False))),
    ("fed_cache/tier_of_a_bag_pair", _plain(_evlfu, lambda E, c: BC._bags(E, (c, BC._tier(E, cap=BC.PAIR_CAPS[1], rule=True))))),
    # ... and while a call is open
    ("open_call/lookup_batch", _open(_fed_tier, False, lambda E, c, n: c.lookup_batch(_dev(RQ)))),
    ("open_call/lookup_bags", _open(_fed_tier, False, lambda E, c, n: _bags_call(E, c))),
    ("open_bag_call/lookup_batch", _open(_fed_tier, True, lambda E, c, n: c.lookup_batch(_dev(RQ)))),
    ("open_bag_call/lookup_bags", _open(_fed_tier, True, lambda E, c, n: _bags_call(E, c))),
    ("open_call/tier_of_a_pair", _open(_evlfu, False, lambda E, c, n: _pair_call(E, c, True))),
    ("open_call/set_backing", _open(_fed_tier, False, _set_backing)),
    ("open_bag_call/set_backing", _open(_fed_tier, True, _set_backing)),
    ("open_call/set_fed_backing", _open(_fed_tier, False, lambda E, c, n: c.set_fed_backing([None] * T, ROWS))),
]

CASES = ([("begin/" + n, b) for n, b in BEGIN] + [("begin_bags/" + n, b) for n, b in BEGIN_BAGS] +
         [("%s/%s" % (ep, n), b) for ep, bags, interact in (("finish", False, False), ("finish_interact", False, True),
                                                            ("finish_bags", True, False), ("finish_bags_interact", True, True))
          for n, b in _finishes(bags, interact)] + OTHERS)
