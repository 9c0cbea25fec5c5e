"""CPU: the bag form of the batched C1 + C2 pair (evs_cache_lookup_bags_c1c2 / _lookup_bags_interact_c1c2) is exported, bound,
and refuses bad arguments before it touches the device -- the checks of tests/test_cabi_bags.py, which the pair's calls share.
A cache handle needs a GPU, so what reads the handles (the envelope: bag rules, geometry, codecs, table placement) is exercised
by tests/test_gpu_cache_bags_pair.py; the checks in front of the handles are held here."""
import ctypes as C


def _lib():
    import evstore_dlrm_amd as E
    return E, E._lib, E._lib.lib()


def test_symbols_are_exported_bound_and_wrapped():
    E, L, lib = _lib()
    raw = C.CDLL(L.LIB_PATH)
    for name in ("evs_cache_lookup_bags_c1c2", "evs_cache_lookup_bags_interact_c1c2"):
        assert hasattr(raw, name), "missing export: " + name
        assert name in L.exported_symbols()
        assert getattr(lib, name).argtypes is not None
    for name in ("lookup_bags_c1c2", "lookup_bags_interact_c1c2"):
        assert callable(getattr(E, name)) and name in E.__all__


def test_bad_arguments_come_back_without_a_gpu():
    E, L, lib = _lib()
    EINVAL = L.EVS_EINVAL
    T = 2
    ptrs = (C.c_void_p * T)(None, None)
    nnz = (C.c_int64 * T)(0, 0)
    buf = C.c_void_p(0x1000)        # a well-aligned address nothing reads: every call below is refused first
    odd = C.c_void_p(0x1004)
    pooled, interact = lib.evs_cache_lookup_bags_c1c2, lib.evs_cache_lookup_bags_interact_c1c2
    err = lib.evs_last_error
    # B == 0 is success, B < 0 is not -- whatever else is passed
    assert pooled(None, None, 0, None, None, None, None, 0, 0, None, 23, None) == 0
    assert interact(None, None, 0, None, None, None, None, 0, 0, None, None, 23, None) == 0
    assert pooled(None, None, -1, ptrs, ptrs, nnz, buf, 72, 36, None, 23, None) == EINVAL and b"B" in err()
    assert interact(None, None, -1, ptrs, ptrs, nnz, buf, 36, 0, buf, None, 23, None) == EINVAL
    # strides that are not multiples of 4 floats
    assert pooled(None, None, 4, ptrs, ptrs, nnz, buf, 145, 36, None, 23, None) == EINVAL and b"strides" in err()
    assert pooled(None, None, 4, ptrs, ptrs, nnz, buf, 144, 37, None, 23, None) == EINVAL and b"strides" in err()
    assert interact(None, None, 4, ptrs, ptrs, nnz, buf, 37, 0, buf, None, 23, None) == EINVAL and b"strides" in err()
    # NULL host arrays, NULL outputs, outputs that are not 16-byte aligned
    assert pooled(None, None, 4, None, ptrs, nnz, buf, 144, 36, None, 23, None) == EINVAL and b"NULL" in err()
    assert pooled(None, None, 4, ptrs, None, nnz, buf, 144, 36, None, 23, None) == EINVAL and b"NULL" in err()
    assert pooled(None, None, 4, ptrs, ptrs, None, buf, 144, 36, None, 23, None) == EINVAL and b"NULL" in err()
    assert pooled(None, None, 4, ptrs, ptrs, nnz, None, 144, 36, None, 23, None) == EINVAL and b"pooled" in err()
    assert pooled(None, None, 4, ptrs, ptrs, nnz, odd, 144, 36, None, 23, None) == EINVAL and b"aligned" in err()
    assert interact(None, None, 4, ptrs, ptrs, nnz, None, 36, 0, buf, None, 23, None) == EINVAL and b"x / R" in err()
    assert interact(None, None, 4, ptrs, ptrs, nnz, buf, 36, 0, None, None, 23, None) == EINVAL and b"x / R" in err()
    assert interact(None, None, 4, ptrs, ptrs, nnz, odd, 36, 0, buf, None, 23, None) == EINVAL and b"aligned" in err()
    # a NULL cache, either one
    assert pooled(None, None, 4, ptrs, ptrs, nnz, buf, 144, 36, None, 23, None) == EINVAL and b"NULL cache" in err()
    assert interact(None, None, 4, ptrs, ptrs, nnz, buf, 36, 0, buf, None, 23, None) == EINVAL and b"NULL cache" in err()
