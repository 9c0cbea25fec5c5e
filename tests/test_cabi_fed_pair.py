"""CPU: the exports of the fed C1 + C2 pair (include/evstore_hip.h: evs_cache_pair_fed_begin, _pair_fed_finish,
_pair_fed_finish_interact, _pair_fed_abort, _pair_fed_stats) exist, are bound, and reject a NULL cache and every NULL argument with
EVS_EINVAL, naming the call, before they touch the device."""
import ctypes as C

import pytest

NEW = ("evs_cache_pair_fed_begin", "evs_cache_pair_fed_finish", "evs_cache_pair_fed_finish_interact", "evs_cache_pair_fed_abort",
       "evs_cache_pair_fed_stats")


@pytest.fixture(scope="module")
def L():
    import evstore_dlrm_amd as E
    return E._lib


def test_the_exports_are_bound(L):
    import evstore_dlrm_amd as E
    lib = L.lib()
    for name in NEW:
        assert name in L.exported_symbols() and hasattr(lib, name), name
    for name in ("lookup_begin_c1c2", "lookup_finish_c1c2", "lookup_finish_interact_c1c2", "lookup_abort_c1c2", "fed_stats_c1c2"):
        assert callable(getattr(E, name)) and name in E.__all__, name


def _einval(L, cases):
    lib = L.lib()
    for name, fn in cases:
        assert fn() == L.EVS_EINVAL, name
        msg = lib.evs_last_error()
        assert name.encode() in msg and b"NULL" in msg, (name, msg)


def test_a_null_cache_is_einval(L):
    """either tier NULL, the other a handle that is never dereferenced"""
    lib = L.lib()
    one = (C.c_int64 * 8)()
    ptr = C.cast(one, C.c_void_p)
    fake = C.c_void_p(0x1000)
    cases = []
    for c1, c2 in ((None, fake), (fake, None), (None, None)):
        cases += [
            ("evs_cache_pair_fed_begin", lambda c1=c1, c2=c2: lib.evs_cache_pair_fed_begin(c1, c2, 1, ptr, ptr, 2, ptr, one, ptr, one, None)),
            ("evs_cache_pair_fed_finish", lambda c1=c1, c2=c2: lib.evs_cache_pair_fed_finish(c1, c2, ptr, 16, ptr, 16, ptr, None)),
            ("evs_cache_pair_fed_finish_interact",
             lambda c1=c1, c2=c2: lib.evs_cache_pair_fed_finish_interact(c1, c2, ptr, 16, ptr, 16, ptr, 4, 0, ptr, None)),
            ("evs_cache_pair_fed_abort", lambda c1=c1, c2=c2: lib.evs_cache_pair_fed_abort(c1, c2)),
            ("evs_cache_pair_fed_stats", lambda c1=c1, c2=c2: lib.evs_cache_pair_fed_stats(c1, c2, one, None)),
        ]
    assert sorted({name for name, _ in cases}) == sorted(NEW)
    _einval(L, cases)


def test_null_arguments_are_einval(L):
    """Cache handles that are never dereferenced: every call must stop at its NULL argument.  (fed1 / fed2 may be NULL: an empty
    list needs no block -- that is judged against the open call.)"""
    lib = L.lib()
    one = (C.c_int64 * 8)()
    ptr = C.cast(one, C.c_void_p)
    fake = C.c_void_p(0x1000)
    begin = [ptr, ptr, 2, ptr, one, ptr, one]        # rows, tier, threshold, keys1, n_keys1_host, keys2, n_keys2_host
    cases = []
    for i in (0, 1, 3, 4, 5, 6):
        args = list(begin)
        args[i] = None
        cases.append(("evs_cache_pair_fed_begin", lambda args=args: lib.evs_cache_pair_fed_begin(fake, fake, 1, *args, None)))
    cases += [
        ("evs_cache_pair_fed_finish", lambda: lib.evs_cache_pair_fed_finish(fake, fake, ptr, 16, ptr, 16, None, None)),
        ("evs_cache_pair_fed_finish_interact", lambda: lib.evs_cache_pair_fed_finish_interact(fake, fake, ptr, 16, ptr, 16, None, 4, 0, ptr, None)),
        ("evs_cache_pair_fed_finish_interact", lambda: lib.evs_cache_pair_fed_finish_interact(fake, fake, ptr, 16, ptr, 16, ptr, 4, 0, None, None)),
        ("evs_cache_pair_fed_stats", lambda: lib.evs_cache_pair_fed_stats(fake, fake, None, None)),
    ]
    _einval(L, cases)
