"""CPU: the bag form of the fed-backing exports (include/evstore_hip.h: evs_cache_fed_begin_bags, _fed_finish_bags,
_fed_finish_bags_interact) exist, are bound, and reject a NULL cache and NULL arguments with EVS_EINVAL before they touch the
device."""
import ctypes as C

import pytest

NEW = ("evs_cache_fed_begin_bags", "evs_cache_fed_finish_bags", "evs_cache_fed_finish_bags_interact")


@pytest.fixture(scope="module")
def L():
    import evstore_dlrm_amd as E
    return E._lib


def _args():
    one = (C.c_int64 * 4)()
    return one, C.cast(one, C.c_void_p), (C.c_void_p * 1)(None)


def test_the_exports_are_bound(L):
    lib = L.lib()
    for name in NEW:
        assert name in L.exported_symbols() and hasattr(lib, name), name


def test_a_null_cache_is_einval(L):
    lib = L.lib()
    one, ptr, arr = _args()
    calls = {
        "evs_cache_fed_begin_bags": lambda: lib.evs_cache_fed_begin_bags(None, 1, arr, arr, one, ptr, ptr, one, None),
        "evs_cache_fed_finish_bags": lambda: lib.evs_cache_fed_finish_bags(None, ptr, 16, ptr, 4, 4, None),
        "evs_cache_fed_finish_bags_interact": lambda: lib.evs_cache_fed_finish_bags_interact(None, ptr, 16, ptr, 4, 0, ptr, None),
    }
    assert sorted(calls) == sorted(NEW)
    for name, fn in calls.items():
        assert fn() == L.EVS_EINVAL, name
        msg = lib.evs_last_error()
        assert name.encode() in msg and b"NULL" in msg, (name, msg)


def test_null_arguments_are_einval(L):
    """A cache handle that is never dereferenced: every call must stop at its NULL argument (hit may be NULL: the cache's own flag
    bytes; fed may be NULL: an empty list)."""
    lib = L.lib()
    one, ptr, arr = _args()
    fake = C.c_void_p(0x1000)
    cases = [
        ("evs_cache_fed_begin_bags", lambda: lib.evs_cache_fed_begin_bags(fake, 1, None, arr, one, ptr, ptr, one, None)),
        ("evs_cache_fed_begin_bags", lambda: lib.evs_cache_fed_begin_bags(fake, 1, arr, None, one, ptr, ptr, one, None)),
        ("evs_cache_fed_begin_bags", lambda: lib.evs_cache_fed_begin_bags(fake, 1, arr, arr, None, ptr, ptr, one, None)),
        ("evs_cache_fed_begin_bags", lambda: lib.evs_cache_fed_begin_bags(fake, 1, arr, arr, one, ptr, None, one, None)),
        ("evs_cache_fed_begin_bags", lambda: lib.evs_cache_fed_begin_bags(fake, 1, arr, arr, one, ptr, ptr, None, None)),
        ("evs_cache_fed_finish_bags", lambda: lib.evs_cache_fed_finish_bags(fake, ptr, 16, None, 4, 4, None)),
        ("evs_cache_fed_finish_bags_interact", lambda: lib.evs_cache_fed_finish_bags_interact(fake, ptr, 16, None, 4, 0, ptr, None)),
        ("evs_cache_fed_finish_bags_interact", lambda: lib.evs_cache_fed_finish_bags_interact(fake, ptr, 16, ptr, 4, 0, None, None)),
    ]
    for name, fn in cases:
        assert fn() == L.EVS_EINVAL, name
        msg = lib.evs_last_error()
        assert name.encode() in msg and b"NULL" in msg, (name, msg)
