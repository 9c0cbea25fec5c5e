"""CPU: the bag form of the batched cache lookup (evs_cache_lookup_bags / _bags_interact) is exported and refuses bad
arguments before it touches the device.  A cache handle needs a GPU, so the checks that read the handle (a NULL indices[k]
with nnz[k] > 0, 2^31 lookups, the feature count and the dimension of the interact form) are exercised by
tests/test_gpu_cache_bags.py; the ones in front of the handle are held here."""
import ctypes as C


def _lib():
    import evstore_dlrm_amd as E
    return E._lib, E._lib.lib()


def test_symbols_are_exported_and_bound():
    L, lib = _lib()
    raw = C.CDLL(L.LIB_PATH)
    for name in ("evs_cache_lookup_bags", "evs_cache_lookup_bags_interact"):
        assert hasattr(raw, name), "missing export: " + name
        assert name in L.exported_symbols()
    assert lib.evs_abi_version() == 1


def test_bad_arguments_come_back_without_a_gpu():
    L, lib = _lib()
    EINVAL = L.EVS_EINVAL
    T = 2
    ptrs = (C.c_void_p * T)(None, None)
    nnz = (C.c_int64 * T)(0, 0)
    buf = C.c_void_p(0x1000)        # a well-aligned address nothing reads: every call below is refused first
    # B == 0 is success, B < 0 is not -- whatever else is passed
    assert lib.evs_cache_lookup_bags(None, 0, None, None, None, None, 0, 0, None, None) == 0
    assert lib.evs_cache_lookup_bags_interact(None, 0, None, None, None, None, 0, 0, None, None, None) == 0
    assert lib.evs_cache_lookup_bags(None, -1, ptrs, ptrs, nnz, buf, 72, 36, None, None) == EINVAL and b"B" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags_interact(None, -1, ptrs, ptrs, nnz, buf, 36, 0, buf, None, None) == EINVAL
    # strides that are not multiples of 4 floats
    assert lib.evs_cache_lookup_bags(None, 4, ptrs, ptrs, nnz, buf, 145, 36, None, None) == EINVAL and b"strides" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags(None, 4, ptrs, ptrs, nnz, buf, 144, 37, None, None) == EINVAL and b"strides" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags_interact(None, 4, ptrs, ptrs, nnz, buf, 37, 0, buf, None, None) == EINVAL and b"strides" in lib.evs_last_error()
    # NULL host arrays, NULL outputs
    assert lib.evs_cache_lookup_bags(None, 4, None, ptrs, nnz, buf, 144, 36, None, None) == EINVAL and b"NULL" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags(None, 4, ptrs, None, nnz, buf, 144, 36, None, None) == EINVAL and b"NULL" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags(None, 4, ptrs, ptrs, None, buf, 144, 36, None, None) == EINVAL and b"NULL" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags(None, 4, ptrs, ptrs, nnz, None, 144, 36, None, None) == EINVAL and b"pooled" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags_interact(None, 4, ptrs, ptrs, nnz, None, 36, 0, buf, None, None) == EINVAL and b"x / R" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags_interact(None, 4, ptrs, ptrs, nnz, buf, 36, 0, None, None, None) == EINVAL and b"x / R" in lib.evs_last_error()
    # a NULL cache
    assert lib.evs_cache_lookup_bags(None, 4, ptrs, ptrs, nnz, buf, 144, 36, None, None) == EINVAL and b"NULL cache" in lib.evs_last_error()
    assert lib.evs_cache_lookup_bags_interact(None, 4, ptrs, ptrs, nnz, buf, 36, 0, buf, None, None) == EINVAL and b"NULL cache" in lib.evs_last_error()
