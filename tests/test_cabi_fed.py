"""CPU: the fed-backing exports of the cache tier (include/evstore_hip.h: evs_cache_set_fed_backing, evs_cache_fed_begin,
_fed_finish, _fed_finish_interact, _fed_abort, _fed_stats) exist, are bound, and reject a NULL cache and NULL arguments with
EVS_EINVAL before they touch the device."""
import ctypes as C

import pytest

NEW = ("evs_cache_set_fed_backing", "evs_cache_fed_begin", "evs_cache_fed_finish", "evs_cache_fed_finish_interact",
       "evs_cache_fed_abort", "evs_cache_fed_stats")


@pytest.fixture(scope="module")
def L():
    import evstore_dlrm_amd as E
    return E._lib


def test_the_exports_are_bound(L):
    lib = L.lib()
    for name in NEW:
        assert name in L.exported_symbols() and hasattr(lib, name), name


def test_a_null_cache_is_einval(L):
    lib = L.lib()
    one = (C.c_int64 * 4)()
    ptr = C.cast(one, C.c_void_p)
    tabs = (C.c_void_p * 1)(None)
    calls = {
        "evs_cache_set_fed_backing": lambda: lib.evs_cache_set_fed_backing(None, tabs, one),
        "evs_cache_fed_begin": lambda: lib.evs_cache_fed_begin(None, 1, ptr, ptr, ptr, one, None),
        "evs_cache_fed_finish": lambda: lib.evs_cache_fed_finish(None, ptr, 16, ptr, None),
        "evs_cache_fed_finish_interact": lambda: lib.evs_cache_fed_finish_interact(None, ptr, 16, ptr, 4, 0, ptr, None),
        "evs_cache_fed_abort": lambda: lib.evs_cache_fed_abort(None),
        "evs_cache_fed_stats": lambda: lib.evs_cache_fed_stats(None, one, None),
    }
    assert sorted(calls) == sorted(NEW)
    for name, fn in calls.items():
        assert fn() == L.EVS_EINVAL, name
        msg = lib.evs_last_error()
        assert name.encode() in msg and b"NULL" in msg, (name, msg)


def test_null_arguments_are_einval(L):
    """A cache handle that is never dereferenced: every call must stop at its NULL argument."""
    lib = L.lib()
    one = (C.c_int64 * 4)()
    ptr = C.cast(one, C.c_void_p)
    fake = C.c_void_p(0x1000)
    tabs = (C.c_void_p * 1)(None)
    cases = [
        ("evs_cache_set_fed_backing", lambda: lib.evs_cache_set_fed_backing(fake, None, one)),
        ("evs_cache_set_fed_backing", lambda: lib.evs_cache_set_fed_backing(fake, tabs, None)),
        ("evs_cache_fed_begin", lambda: lib.evs_cache_fed_begin(fake, 1, None, ptr, ptr, one, None)),
        ("evs_cache_fed_begin", lambda: lib.evs_cache_fed_begin(fake, 1, ptr, None, ptr, one, None)),
        ("evs_cache_fed_begin", lambda: lib.evs_cache_fed_begin(fake, 1, ptr, ptr, None, one, None)),
        ("evs_cache_fed_begin", lambda: lib.evs_cache_fed_begin(fake, 1, ptr, ptr, ptr, None, None)),
        ("evs_cache_fed_finish", lambda: lib.evs_cache_fed_finish(fake, ptr, 16, None, None)),
        ("evs_cache_fed_finish_interact", lambda: lib.evs_cache_fed_finish_interact(fake, ptr, 16, None, 4, 0, ptr, None)),
        ("evs_cache_fed_finish_interact", lambda: lib.evs_cache_fed_finish_interact(fake, ptr, 16, ptr, 4, 0, None, None)),
        ("evs_cache_fed_stats", lambda: lib.evs_cache_fed_stats(fake, None, None)),
    ]
    for name, fn in cases:
        assert fn() == L.EVS_EINVAL, name
        msg = lib.evs_last_error()
        assert name.encode() in msg and b"NULL" in msg, (name, msg)
