"""CPU: the fetch-first switch of the set-associative cache tier (evs_cache_set_miss_order / evs_cache_fetch_stats) is exported
with the header's signatures and refuses bad arguments before it touches the device.  A cache handle needs a GPU, so what reads
the handle is exercised by tests/test_gpu_host_setassoc.py."""
import ctypes as C
import os
import re

NAMES = ("evs_cache_set_miss_order", "evs_cache_fetch_stats")


def _lib():
    import evstore_dlrm_amd as E
    return E._lib, E._lib.lib()


def _declared():
    """name -> (return type, [parameter types]) as include/evstore_hip.h declares the two symbols"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "evstore_hip.h")).read()
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
    ctype = {"int": C.c_int, "int64_t": C.c_int64}
    d = _declared()
    for name, (ret, params) in d.items():
        assert hasattr(raw, name), "missing export: " + name
        assert name in L.exported_symbols()
        res, args = L._PROTOS[name]
        assert res is ctype[ret], name
        assert len(args) == len(params), name
        for a, p in zip(args, params):
            if p == "int64_t *":
                assert a in (C.c_void_p, C.POINTER(C.c_int64)), (name, p)
            elif p.endswith("*"):
                assert a is C.c_void_p, (name, p)            # every other pointer travels as an address
            else:
                assert a is ctype[p], (name, p)
    assert d["evs_cache_set_miss_order"] == ("int", ["evs_cache *", "int"])
    assert d["evs_cache_fetch_stats"] == ("int", ["evs_cache *", "int64_t *", "void *"])
    assert lib.evs_abi_version() == 1


def test_the_contract_stands_beside_the_inline_setting():
    """include/evstore_hip.h says what order 1 is where evs_cache_set_inline_update is declared"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "evstore_hip.h")).read()
    at_inline = src.index("EVS_API int evs_cache_set_inline_update")
    at_order = src.index("EVS_API int evs_cache_set_miss_order")
    at_stats = src.index("EVS_API int evs_cache_fetch_stats")
    assert at_inline < at_order < at_stats < src.index("EVS_API int evs_cache_batch_stats")
    text = src[at_inline:at_stats]
    for word in ("consume first", "fetch first", "sa_repoint", "EVS_ESTATE", "EVS_EINVAL", "EVS_SA_DUAL", "EVS_SA_WAYS"):
        assert word in text, word


def test_bad_arguments_come_back_without_a_gpu():
    L, lib = _lib()
    EINVAL = L.EVS_EINVAL
    out4 = (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.evs_cache_set_miss_order(None, 1) == EINVAL
    assert b"evs_cache_set_miss_order" in lib.evs_last_error() and b"NULL cache" in lib.evs_last_error()
    assert lib.evs_cache_set_miss_order(None, 5) == EINVAL
    assert lib.evs_cache_fetch_stats(None, out4, None) == EINVAL
    assert b"evs_cache_fetch_stats" in lib.evs_last_error() and b"NULL cache" in lib.evs_last_error()
    assert list(out4) == [7, 7, 7, 7]
    assert lib.evs_cache_fetch_stats(None, None, None) == EINVAL and b"evs_cache_fetch_stats" in lib.evs_last_error()
