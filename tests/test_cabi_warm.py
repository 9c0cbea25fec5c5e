"""CPU: the warm start of the batched cache tier (evs_cache_batch_export / evs_cache_batch_load / evs_cache_load_plan) is
exported with the header's signatures and refuses bad arguments before it touches the device.  A cache handle needs a GPU, so
what reads the handle is exercised by tests/test_gpu_warm_start.py; the plan itself by tests/test_warm_start_plan.py."""
import ctypes as C
import os
import re

NAMES = ("evs_cache_batch_export", "evs_cache_batch_load", "evs_cache_load_plan")


def _lib():
    import evstore_dlrm_amd as E
    return E._lib, E._lib.lib()


def _declared():
    """name -> (return type, [parameter types]) as include/evstore_hip.h declares the three symbols"""
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
    for name, (ret, params) in _declared().items():
        assert hasattr(raw, name), "missing export: " + name
        assert name in L.exported_symbols()
        res, args = L._PROTOS[name]
        assert res is ctype[ret], name
        assert len(args) == len(params), name
        for a, p in zip(args, params):
            if p.endswith("*"):
                assert a is C.c_void_p, (name, p)            # every pointer travels as an address
            else:
                assert a is ctype[p], (name, p)
    d = _declared()
    assert d["evs_cache_batch_export"] == ("int64_t", ["evs_cache *", "int64_t *", "int64_t", "int64_t *", "void *"])
    assert d["evs_cache_batch_load"] == ("int", ["evs_cache *", "int64_t", "int64_t *", "int64_t *", "int", "int64_t *", "void *"])
    assert d["evs_cache_load_plan"][1][:4] == ["int", "int64_t", "int", "int64_t *"]
    assert lib.evs_abi_version() == 1


def test_bad_arguments_come_back_without_a_gpu():
    L, lib = _lib()
    EINVAL = L.EVS_EINVAL
    buf = (C.c_int64 * 16)()
    assert lib.evs_cache_batch_export(None, None, 0, None, None) == EINVAL and b"evs_cache_batch_export" in lib.evs_last_error()
    assert lib.evs_cache_batch_load(None, 0, None, None, 0, None, None) == EINVAL and b"NULL cache" in lib.evs_last_error()
    assert lib.evs_cache_batch_load(None, -1, buf, None, 0, None, None) == EINVAL and b"negative" in lib.evs_last_error()
    assert lib.evs_cache_batch_load(None, 3, None, None, 0, None, None) == EINVAL
    assert lib.evs_cache_batch_load(None, 1, buf, buf, 2, None, None) == EINVAL and b"strict" in lib.evs_last_error()
