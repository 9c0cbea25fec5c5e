"""CPU: the count-first switch of the EvLFU bag chain (evs_cache_set_bag_count) is exported with the header's signature, bound
in _lib, documented where the bag rule is, and refuses bad arguments before it touches the device.  A cache handle needs a GPU,
so what reads the handle is exercised by tests/test_gpu_bags_count_first.py."""
import ctypes as C
import os
import re

NAME = "evs_cache_set_bag_count"


def _lib():
    import evstore_dlrm_amd as E
    return E._lib, E._lib.lib()


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "evstore_hip.h")).read()


def test_symbol_is_exported_and_bound_with_the_headers_signature():
    L, lib = _lib()
    m = re.search(r"EVS_API\s+(\w+)\s+" + NAME + r"\s*\(([^;]*)\)\s*;", _header())
    assert m, "not declared: " + NAME
    assert m.group(1) == "int"
    assert [re.sub(r"\s+", " ", p).strip() for p in m.group(2).split(",")] == ["evs_cache *c", "int when"]
    assert hasattr(C.CDLL(L.LIB_PATH), NAME), "missing export"
    assert NAME in L.exported_symbols()
    assert L._PROTOS[NAME] == (C.c_int, [C.c_void_p, C.c_int])
    assert lib.evs_abi_version() == 1


def test_the_contract_stands_beside_the_bag_rule():
    """include/evstore_hip.h names both values, both orders and what stays as it was, between the bag rule's setter and this one"""
    src = _header()
    at_rule = src.index("EVS_API int evs_cache_set_bag_rule")
    at_count = src.index("EVS_API int " + NAME)
    assert at_rule < at_count < src.index("EVS_API int evs_cache_set_miss_order")
    text = src[at_rule:at_count]
    for word in ('0 "in the pooling walk"', '1 "count first"', "consume first", "fetch first", "sa_repoint", "EVS_EINVAL", "EVS_ESTATE",
                 "warm-start", "evs_cache_lookup_bags_c1c2", "evs_cache_fetch_stats"):
        assert word in text, word
    served = src[src.index("EVS_API int evs_cache_set_inline_update"):src.index("EVS_API int evs_cache_set_miss_order")]
    assert NAME in served, "the fetch-first 'served' line does not name the new form"


def test_bad_arguments_come_back_without_a_gpu():
    L, lib = _lib()
    for when in (1, 5):
        assert lib.evs_cache_set_bag_count(None, when) == L.EVS_EINVAL
        assert NAME.encode() in lib.evs_last_error() and b"NULL cache" in lib.evs_last_error()


def test_python_setter_carries_the_contract():
    import inspect

    import evstore_dlrm_amd as E
    doc = inspect.getdoc(E.GpuCache.set_bag_count)
    for word in ("count-first", "pooling-walk", "fetch-first", "evs_cache_set_bag_count", "EVS_EINVAL"):
        assert word in doc, word
