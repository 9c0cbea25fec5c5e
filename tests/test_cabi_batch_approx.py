"""CPU: the approximate-embedding mode of the batched EvLFU tier (evs_cache_set_batch_approx / evs_cache_approx_stats) is exported
with the header's signatures and refuses bad arguments before it touches the device.  A cache handle needs a GPU, so the refusals
that read the handle -- a threshold above n_tables, a threshold on an LRU / LFU cache -- are exercised by
tests/test_gpu_batch_approx.py (test_refusals_of_the_setter)."""
import ctypes as C
import os
import re

NAMES = ("evs_cache_set_batch_approx", "evs_cache_approx_stats")


def _lib():
    import evstore_dlrm_amd as E
    return E._lib, E._lib.lib()


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "evstore_hip.h")).read()


def _declared():
    """name -> (return type, [parameter types]) as include/evstore_hip.h declares the two symbols"""
    src = _header()
    out = {}
    for name in NAMES:
        m = re.search(r"EVS_API\s+(\w+)\s+" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, "not declared: " + name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(2).split(",")]
        out[name] = (m.group(1), [re.sub(r"\s*\w+$", "", p).replace("const ", "").strip() for p in params])
    return out


def test_symbols_are_exported_and_bound_with_the_headers_signatures():
    L, lib = _lib()
    raw = C.CDLL(L.LIB_PATH)
    d = _declared()
    for name in NAMES:
        assert hasattr(raw, name), "missing export: " + name
        assert name in L.exported_symbols()
        res, args = L._PROTOS[name]
        assert res is C.c_int and len(args) == len(d[name][1]), name
    assert d["evs_cache_set_batch_approx"] == ("int", ["evs_cache *", "int"])
    assert d["evs_cache_approx_stats"] == ("int", ["evs_cache *", "int64_t *", "void *"])
    assert L._PROTOS["evs_cache_set_batch_approx"][1] == [C.c_void_p, C.c_int]
    a = L._PROTOS["evs_cache_approx_stats"][1]
    assert a[0] is C.c_void_p and a[1] in (C.c_void_p, C.POINTER(C.c_int64)) and a[2] is C.c_void_p
    assert lib.evs_abi_version() == 1


def test_the_rule_stands_beside_the_batched_switches():
    """include/evstore_hip.h writes the rule down where the setter is declared, behind the fetch-first switch it composes with"""
    src = _header()
    at_fetch = src.index("EVS_API int evs_cache_fetch_stats")
    at_set = src.index("EVS_API int evs_cache_set_batch_approx")
    at_stats = src.index("EVS_API int evs_cache_approx_stats")
    assert at_fetch < at_set < at_stats < src.index("EVS_API int evs_cache_batch_stats")
    text = src[at_fetch:at_stats]
    for word in ("agg_hit", "nearest hit", "+0.0f", "hit[b, t] = 2", "sa_repoint", "n_perfect_hits", "bag forms", "warm-start",
                 "EVS_EINVAL", "EVS_ESTATE", "EVS_SA_WAYS", "evs_cache_set_inline_update", "thres <= 0"):
        assert word in text, word


def test_bad_arguments_come_back_without_a_gpu():
    L, lib = _lib()
    EINVAL = L.EVS_EINVAL
    assert lib.evs_cache_set_batch_approx(None, 1) == EINVAL
    assert b"evs_cache_set_batch_approx" in lib.evs_last_error() and b"NULL cache" in lib.evs_last_error()
    assert lib.evs_cache_set_batch_approx(None, 0) == EINVAL and b"NULL cache" in lib.evs_last_error()
    out4 = (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.evs_cache_approx_stats(None, out4, None) == EINVAL
    assert b"evs_cache_approx_stats" in lib.evs_last_error() and b"NULL cache" in lib.evs_last_error()
    assert list(out4) == [7, 7, 7, 7]
    assert lib.evs_cache_approx_stats(None, None, None) == EINVAL
    assert b"evs_cache_approx_stats" in lib.evs_last_error() and b"NULL out4" in lib.evs_last_error()
