"""The refusals of the batched cache calls that are made before anything is launched, as a table of (name, build): build(E) sets
the situation up and returns (call, after) -- call() must raise EvsError; after(), where there is one, tells the cache(s) the
opposite batch policy, mends what was refused and checks that they serve (a refusal that resolved a policy must have forgotten it
and must not have marked the cache as used).  tests/golden/make_golden_refusals.py records code and text of every case into
tests/golden/batched_refusals.json; tests/test_gpu_batched_refusals.py replays the table against that record.

4 tables, d = 16, B = 2; a tier alone has two sets of 8 ways, a pair 64 + 128 entries (the shared set record)."""
import ctypes as C

import numpy as np
import torch

T, D, B = 4, 16, 2
ROWS = [40, 60, 80, 100]
RQ = np.array([[3, 17, 50, 7], [5, 18, 51, 9]], np.int32)
PAIR_CAPS = (64, 128)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tables(codec, d=D, pinned=False):
    """rows of a tier's codec (their values do not matter here: nibbles stay below 15, the 4-bit codec's NaN code)"""
    if codec == 32:
        tabs = [(torch.arange(n * d, dtype=torch.float32) % 7 - 3).reshape(n, d) for n in ROWS]
    else:
        tabs = [(torch.arange(n * d * codec // 8) % 14 * 17 % 224).to(torch.uint8).reshape(n, d * codec // 8) for n in ROWS]
    return [t.pin_memory() for t in tabs] if pinned else [t.cuda() for t in tabs]


def _tier(E, policy="evlfu", cap=16, codec=32, d=D, pinned=False, order=0, rule=False, count=False, given=None, approx=0):
    c = E.GpuCache(policy, cap, T, d, codec, "cpp")
    if order:
        c.set_miss_order("fetch-first")
    c._kept = _tables(codec, d, pinned)
    c.set_backing(c._kept)
    if rule:
        c.set_bag_rule("served-bags")
    if count:
        c.set_bag_count("count-first")
    if given:
        c.set_batch_policy(given)
    if approx:
        c.set_batch_approx(approx)
    return c


def _pair(E, order=0, codecs=(32, 8), caps=PAIR_CAPS, d=D, pinned=(False, False), rule=(True, True), count=None, policy=("evlfu", "evlfu")):
    order = (order, order) if isinstance(order, int) else order
    count = order if count is None else count
    return tuple(_tier(E, policy[k], caps[k], codecs[k], d, pinned[k], order[k], rule[k] and policy[k] == "evlfu", bool(count[k]))
                 for k in (0, 1))


def _bt(c):
    return lambda: c.lookup_batch(_dev(RQ))


def _bt2(E, p, c3=None):
    return lambda: E.lookup_batch_c1c2(p[0], p[1], _dev(RQ), threshold=2, c3=c3)


def _serves(c):
    """a tier nobody has used: the first call misses everywhere, the second hits"""
    hit, _o = c.lookup_batch(_dev(RQ))
    assert not hit.any()
    hit, _o = c.lookup_batch(_dev(RQ))
    assert bool(hit.all())


def _serves2(E, p):
    tier, _o = E.lookup_batch_c1c2(p[0], p[1], _dev(RQ), threshold=2)
    assert not tier.any()
    tier, _o = E.lookup_batch_c1c2(p[0], p[1], _dev(RQ), threshold=2)
    assert bool((tier > 0).all())


def _then(cs, policy, serve, mend=None):
    """after(): every cache still takes `policy` (the opposite of what the refused call saw or resolved), then serves"""
    def after():
        for c in cs:
            assert c.set_batch_policy(policy) is c
        if mend:
            mend()
        serve()
    return after


def _bags(E, cs, interact=False, **bad):
    """one bag call through the C ABI, single tier (cs = (c,)) or pair (cs = (c1, c2)), with one argument made bad"""
    d = cs[0].dim
    L = E._lib.lib()
    idx = [_dev(RQ[:, t].astype(np.int64)) for t in range(T)]
    off = [_dev(np.arange(B, dtype=np.int64)) for _ in range(T)]
    nnz = [B] * T
    ip, op = [t.data_ptr() for t in idx], [t.data_ptr() for t in off]
    if "null_index" in bad:
        ip[bad["null_index"]] = None
    if "null_offset" in bad:
        op[bad["null_offset"]] = None
    if "neg_nnz" in bad:
        nnz[bad["neg_nnz"]] = -1
    idx_c = None if bad.get("indices") == "null" else (C.c_void_p * T)(*ip)
    off_c = None if bad.get("offsets") == "null" else (C.c_void_p * T)(*op)
    nnz_c = None if bad.get("nnz") == "null" else (C.c_int64 * T)(*nnz)
    flags = torch.empty(B * T, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    hs = [c._h for c in cs]
    tail = [flags.data_ptr()] + ([2] if len(cs) == 2 else []) + [st]
    if interact:
        F = T + 1
        x = torch.zeros(B * d + 4, device="cuda")
        R = torch.zeros(B, d + F * (F - 1) // 2, device="cuda")
        xp = x.data_ptr() + bad.get("x_offset", 0)
        fn = L.evs_cache_lookup_bags_interact if len(cs) == 1 else L.evs_cache_lookup_bags_interact_c1c2
        rc = fn(*hs, B, idx_c, off_c, nnz_c, xp, bad.get("x_stride", d), 0, R.data_ptr(), *tail)
    else:
        out = torch.zeros(T * B * d + 4, device="cuda")
        outp = None if bad.get("pooled") == "null" else out.data_ptr() + bad.get("pooled_offset", 0)
        fn = L.evs_cache_lookup_bags if len(cs) == 1 else L.evs_cache_lookup_bags_c1c2
        rc = fn(*hs, B, idx_c, off_c, nnz_c, outp, bad.get("tstride", B * d), bad.get("bstride", d), *tail)
    torch.cuda.synchronize()
    E._lib.check(rc)


# the argument checks both bag forms share: (name, interact, the bad argument); "dim" cases make their caches with that dim
SHARED = [
    ("table_stride", False, {"tstride": B * D + 2}), ("bag_stride", False, {"bstride": D + 1}), ("x_stride", True, {"x_stride": D + 2}),
    ("null_indices", False, {"indices": "null"}), ("null_offsets", False, {"offsets": "null"}), ("null_nnz", False, {"nnz": "null"}),
    ("null_pooled", False, {"pooled": "null"}), ("misaligned_pooled", False, {"pooled_offset": 4}), ("misaligned_x", True, {"x_offset": 8}),
    ("negative_nnz", False, {"neg_nnz": 2}), ("null_offsets_k", False, {"null_offset": 1}), ("null_indices_k", False, {"null_index": 3}),
    ("dim_pooling", False, {"dim": 18, "tstride": B * 20, "bstride": 20}),("dim_interaction", True, {"dim": 20}),
]


def _shared(form, interact, bad):
    def build(E):
        bad_ = dict(bad)
        d = bad_.pop("dim", D)
        cs = (_tier(E, "lru", d=d),) if form == "alone" else _pair(E, d=d)
        return (lambda: _bags(E, cs, interact, **bad_)), None
    return build


def _alt_tier(E):
    alt = [(torch.arange(n, dtype=torch.int32) % 3 * 100 + (t % T) + 1).cuda() for t, n in enumerate(ROWS)]
    return E.GpuAltKeyTier(64, alt)


def _ff_given(name):
    def build(E):
        c = _tier(E, order=1, given=name)
        return _bt(c), _then((c,), "setassoc", lambda: _serves(c))
    return build


def _ff_tier_of_pair(E):
    p = _pair(E, 1)
    _bt2(E, p)()
    return _bt(p[0]), None


def _ff_bags_without_count(E):
    c = _tier(E, order=1, rule=True)
    return (lambda: _bags(E, (c,))), _then((c,), "sampled", lambda: _serves(c), lambda: c.set_miss_order("consume-first"))


def _apx_given(name):
    def build(E):
        c = _tier(E, given=name, approx=2)
        return _bt(c), _then((c,), "setassoc", lambda: _serves(c))
    return build


def _apx_tier_of_pair(E):
    p = _pair(E, 0)
    _bt2(E, p)()
    p[0].set_batch_approx(2)
    return _bt(p[0]), None


def _apx_consume_first_pinned(E):
    c = _tier(E, pinned=True, approx=2)   # (resolves to the sampled update: host-memory tables at order 0)
    return _bt(c), _then((c,), "setassoc", lambda: _serves(c), lambda: c.set_miss_order("fetch-first"))


def _bags_no_rule(E):
    c = _tier(E)
    return (lambda: _bags(E, (c,))), None


def _bags_pinned(E):
    c = _tier(E, pinned=True, rule=True)
    return (lambda: _bags(E, (c,))), None


def _bags_pinned_cf_only(E):
    c = _tier(E, pinned=True, rule=True, count=True)
    return (lambda: _bags(E, (c,))), None


def _bags_pinned_ff_only(E):
    c = _tier(E, pinned=True, rule=True, order=1)
    return (lambda: _bags(E, (c,))), None


def _bags_policy_not_2(E):
    c = _tier(E, rule=True, given="sampled")
    return (lambda: _bags(E, (c,))), _then((c,), "setassoc", lambda: _serves(c))


def _pairff_alt_key(E):
    p = _pair(E, 1)
    c3 = _alt_tier(E)
    return _bt2(E, p, c3), None


def _pairff_one_tier(E):
    return _bt2(E, _pair(E, (1, 0))), None


def _pairff_given(name):
    def build(E):
        p = _pair(E, 1, pinned=(True, True))
        p[0].set_batch_policy(name)
        return _bt2(E, p), _then(p[:1], "setassoc", lambda: _serves2(E, p))
    return build


def _pairff_ran_alone(E):
    p = _pair(E, 1)
    _bt(p[0])()
    return _bt2(E, p), None


def _pb(E, p):
    return lambda: _bags(E, p)


def _pairbags_non_evlfu(E):
    return _pb(E, _pair(E, policy=("evlfu", "lru"))), None


def _pairbags_no_rule(E):
    return _pb(E, _pair(E, rule=(True, False))), None


def _pairbags_one_without_count(E):
    return _pb(E, _pair(E, 1, count=(1, 0))), None


def _pairbags_pinned_order0(E):
    return _pb(E, _pair(E, 0, pinned=(False, True))), None


def _pairbags_approx(E):
    p = _pair(E)
    p[1].set_batch_approx(2)
    return _pb(E, p), None


def _pairbags_triple(E):
    p = _pair(E)
    c3 = _alt_tier(E)
    _bt2(E, p, c3)()
    return _pb(E, p), None


def _pairbags_same_cache(E):
    c = _tier(E, cap=PAIR_CAPS[0], rule=True)
    return _pb(E, (c, c)), None


def _pairbags_precisions(E):
    return _pb(E, _pair(E, codecs=(8, 16))), None


def _pairbags_not_together(E):
    p = _pair(E)
    _bt(p[0])()
    _bt(p[1])()
    return _pb(E, p), None


def _pairbags_ran_hashed(E):
    p = _pair(E)
    for c in p:
        c.set_batch_policy("sampled")
    _bt2(E, p)()
    return _pb(E, p), None


def _pairbags_given(name):
    def build(E):
        p = _pair(E)
        p[1].set_batch_policy(name)
        return _pb(E, p), _then(p[1:], "setassoc", lambda: _serves2(E, p))
    return build


def _pairbags_no_shared_record(E):
    p = _pair(E, caps=(16, 128))   # (C1 would get fewer than 4 ways of the shared record)
    return _pb(E, p), _then(p, "sampled", lambda: _serves2(E, p))


def _pairbags_ff_given(name):
    def build(E):
        p = _pair(E, 1, pinned=(True, True))
        p[0].set_batch_policy(name)
        return _pb(E, p), _then(p[:1], "setassoc", lambda: _serves2(E, p))
    return build


def _pairbags_ff_no_shared_record(E):
    p = _pair(E, 1, caps=(16, 128))
    return _pb(E, p), _then(p, "sampled", lambda: _serves2(E, p), lambda: [c.set_miss_order("consume-first") for c in p])


CASES = [("%s_bags/%s" % (form, name), _shared(form, interact, bad)) for form in ("alone", "pair") for name, interact, bad in SHARED] + [
    ("fetch_first/plan", _ff_given("plan")), ("fetch_first/sampled", _ff_given("sampled")),
    ("fetch_first/tier_of_a_started_pair", _ff_tier_of_pair), ("fetch_first/evlfu_bags_without_count_first", _ff_bags_without_count),
    ("approx/plan", _apx_given("plan")), ("approx/sampled", _apx_given("sampled")),
    ("approx/tier_of_a_started_pair", _apx_tier_of_pair), ("approx/consume_first_over_pinned_tables", _apx_consume_first_pinned),
    ("evlfu_bags/no_bag_rule", _bags_no_rule), ("evlfu_bags/pinned_tables", _bags_pinned),
    ("evlfu_bags/pinned_tables_count_first_without_fetch_first", _bags_pinned_cf_only),
    ("evlfu_bags/pinned_tables_fetch_first_without_count_first", _bags_pinned_ff_only), ("evlfu_bags/policy_not_2", _bags_policy_not_2),
    ("pair_fetch_first/alt_key_tier", _pairff_alt_key), ("pair_fetch_first/one_tier_at_order_1", _pairff_one_tier),
    ("pair_fetch_first/plan", _pairff_given("plan")), ("pair_fetch_first/sampled", _pairff_given("sampled")),
    ("pair_fetch_first/a_tier_ran_alone_first", _pairff_ran_alone),
    ("pair_bags/non_evlfu_tier", _pairbags_non_evlfu), ("pair_bags/tier_without_bag_rule", _pairbags_no_rule),
    ("pair_bags/order_1_one_tier_without_count_first", _pairbags_one_without_count), ("pair_bags/pinned_tables_at_order_0", _pairbags_pinned_order0),
    ("pair_bags/approximate_threshold", _pairbags_approx), ("pair_bags/ran_in_a_triple", _pairbags_triple),
    ("pair_bags/one_cache_given_twice", _pairbags_same_cache), ("pair_bags/precision_pair", _pairbags_precisions),
    ("pair_bags/tiers_did_not_start_out_together", _pairbags_not_together), ("pair_bags/tiers_ran_the_sampled_update", _pairbags_ran_hashed),
    ("pair_bags/plan", _pairbags_given("plan")), ("pair_bags/sampled", _pairbags_given("sampled")),
    ("pair_bags/no_shared_record", _pairbags_no_shared_record),
    ("pair_bags/fetch_first_plan", _pairbags_ff_given("plan")), ("pair_bags/fetch_first_sampled", _pairbags_ff_given("sampled")),
    ("pair_bags/fetch_first_no_shared_record", _pairbags_ff_no_shared_record),
]


def refusal(E, call):
    """-> (code, the full evs_last_error() text) of the refusal call() raises"""
    try:
        call()
    except E._lib.EvsError as e:
        return e.code, E._lib.lib().evs_last_error().decode("utf-8", "replace")
    raise AssertionError("the call was not refused")
