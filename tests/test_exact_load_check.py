"""evs_exact_load_check alone: the one function both exact loaders (device and host) run on a state before they touch
anything -- pure host code, no GPU.  One case per refusal, each changing one field of a good export."""
import numpy as np
import pytest

import _exact_warm as W

import evstore_dlrm_amd as E
from evstore_dlrm_amd import host_cache as H

MAX_FREQ = 1 << 22   # the device engine's lfu_max_freq


def _export(policy, cap, cut):
    c = H.HostCache(policy, cap, 26, 36, 32, "python").set_backing(W.tables())
    c.request(W.trace(cap)[:cut])
    return c.export_exact_state()


@pytest.fixture(scope="module")
def good():
    return {"evlfu": _export("evlfu", 768, 900), "lru": _export("lru", 64, 700), "lfu": _export("lfu", 768, 700)}


def _check(policy, cap, entries, state, strict=1, max_freq=MAX_FREQ, n_rows=None, n_tables=26, n=None):
    n_rows = np.ascontiguousarray(W.golden()["n_rows"] if n_rows is None else n_rows, np.int64)
    entries = np.ascontiguousarray(entries, np.int64)
    state = None if state is None else np.ascontiguousarray(state, np.int64)
    rc = E._lib.lib().evs_exact_load_check({"evlfu": 0, "lru": 1, "lfu": 2}[policy], cap, n_tables, n_rows.ctypes.data,
                                           len(entries) if n is None else n, entries.ctypes.data if len(entries) else None,
                                           None if state is None else state.ctypes.data, strict, max_freq)
    return rc, E._lib.lib().evs_last_error().decode()


@pytest.mark.parametrize("policy,cap", [("evlfu", 768), ("lru", 64), ("lfu", 768)])
def test_a_good_export_passes(good, policy, cap):
    ex = good[policy]
    assert 0 < len(ex["entries"]) <= cap
    for strict, state, mf in ((1, ex["state"], MAX_FREQ), (0, ex["state"], MAX_FREQ), (0, None, MAX_FREQ), (1, ex["state"], 0)):
        assert _check(policy, cap, ex["entries"], state, strict, mf)[0] == 0
    assert _check(policy, cap + 100, ex["entries"], ex["state"], strict=0)[0] == 0   # any capacity >= n without strict
    assert _check(policy, cap, ex["entries"][:0], ex["state"])[0] == 0              # nothing to load


def _edit(a, i, j, v):
    a = a.copy()
    a[i, j] = v
    return a


def test_every_refusal(good):
    ev, lru, lfu = good["evlfu"], good["lru"], good["lfu"]
    e, s = ev["entries"], ev["state"]
    last = len(e) - 1
    cases = {
        "table 0": ("evlfu", 768, _edit(e, 5, 1, 0), s, 1, "table outside"),
        "table T + 1": ("evlfu", 768, _edit(e, 5, 1, 27), s, 1, "table outside"),
        "row < 0": ("evlfu", 768, _edit(e, 5, 2, -1), s, 1, "row outside"),
        "row = n_rows": ("evlfu", 768, _edit(e, 5, 2, int(W.golden()["n_rows"][e[5, 1] - 1])), s, 1, "row outside"),
        "duplicate key": ("evlfu", 768, np.concatenate([e[:7], [[e[7, 0], e[3, 1], e[3, 2]]], e[8:]]), s, 1, "duplicate key"),
        "evlfu score > T": ("evlfu", 768, _edit(e, last, 0, 27), s, 1, "score outside"),
        "evlfu score < 0": ("evlfu", 768, _edit(e, 0, 0, -1), s, 1, "score outside"),
        "lru score 1": ("lru", 64, _edit(lru["entries"], 63, 0, 1), lru["state"], 1, "score outside"),
        "lfu score 0": ("lfu", 768, _edit(lfu["entries"], 0, 0, 0), lfu["state"], 1, "score outside"),
        "lfu score max_freq - 1": ("lfu", 768, _edit(lfu["entries"], 767, 0, MAX_FREQ - 1), lfu["state"], 1, "score outside"),
        "scores go down": ("evlfu", 768, np.concatenate([e[1:], e[:1]]) if e[0, 0] < e[last, 0] else None, s, 1, "go down"),
        "n > capacity": ("evlfu", 767, e, s, 0, "capacity"),
        "version 3": ("evlfu", 768, e, np.concatenate([[3], s[1:]]), 1, "version"),
        "another policy": ("lru", 768, e[:0], s, 0, "another policy"),
        "strict without a state": ("evlfu", 768, e, None, 1, "needs the exported state"),
        "strict, another capacity": ("evlfu", 800, e, s, 1, "capacity"),
        "strict, another table count": ("evlfu", 768, e[:0], s, 1, "table count"),
        "min_C1 out of range": ("evlfu", 768, e, np.concatenate([s[:6], [27], s[7:]]), 1, "min_C1"),
        "least_freq 0": ("lfu", 768, lfu["entries"], np.concatenate([lfu["state"][:8], [0], lfu["state"][9:]]), 1, "least_freq"),
        "a negative counter": ("evlfu", 768, e, np.concatenate([s[:11], [-1], s[12:]]), 1, "negative counter"),
    }
    for name, (policy, cap, entries, state, strict, word) in cases.items():
        assert entries is not None, name
        kw = {"n_tables": 30, "n_rows": np.concatenate([W.golden()["n_rows"], [5] * 4])} if name == "strict, another table count" else {}
        rc, msg = _check(policy, cap, entries, state, strict, **kw)
        assert rc == E._lib.EVS_EINVAL and word in msg, (name, rc, msg)
    assert _check("lfu", 768, _edit(lfu["entries"], 767, 0, MAX_FREQ - 1), lfu["state"], 1, max_freq=0)[0] == 0   # the host engine: unbounded
    assert _check("evlfu", 768, e, s, n=-1)[0] == E._lib.EVS_EINVAL


def test_the_batched_tiers_state16_is_refused(good):
    """version 1 is evs_cache_batch_export's state16: refused on its first field, whatever else it holds"""
    e = good["evlfu"]["entries"]
    state16 = np.zeros(16, np.int64)
    state16[:6] = [1, 0, 768, 26, 36, 32]
    for strict in (0, 1):
        rc, msg = _check("evlfu", 768, e, state16, strict)
        assert rc == E._lib.EVS_EINVAL and "version" in msg
