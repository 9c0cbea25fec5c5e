"""Mirror of the reference's cache_algo/cpp_socket_client.py: the ctypes front end of the C++
cache manager (init_ctypes_lib :63-83, cache_lookup_via_ctypes :119, request_to_cpp_cache
:129-157, print_n_reset_perfect_hit :85-87).  The socket transport (:89-117) is out of scope."""
import ctypes

import torch

from .. import _lib

N_EVTable = 26
EV_DIMENSION = 36
cache_manager_cpp = None
emb_weights_in_tensor = [None] * N_EVTable  # module-global list reused across calls, as in the reference (:18)


def init_ctypes_lib(ev_table_root=None, main_precision=32, total_size=75425, n_caching_layer=1,
                    secondary_precision=4, size_proportion="", backing="hbm", altkey_dir=None):
    """Loads libevstore_hip.so.  With ev_table_root the manager is configured here; without it the
    library reads the EVS_* environment variables on the first lookup."""
    global cache_manager_cpp
    print("Initiating ctypes cache_manager_cpp library (libevstore_hip.so) ...")
    cache_manager_cpp = _lib.lib()
    if altkey_dir is not None:
        _lib.check(cache_manager_cpp.evs_manager_set_altkey_dir(str(altkey_dir).encode()))
    if ev_table_root is not None:
        _lib.check(cache_manager_cpp.evs_manager_configure(
            n_caching_layer, main_precision, secondary_precision, total_size, size_proportion.encode(),
            str(ev_table_root).encode(), 1 if backing == "pinned" else 0))


def print_n_reset_perfect_hit():
    if cache_manager_cpp is not None:
        cache_manager_cpp.print_perfect_hit()


def establish_socket_conn():
    print("ERROR: the loopback-socket transport is not part of this build; use the ctypes path")
    exit(-1)


def cache_lookup_via_ctypes(group_rowIds):
    return cache_manager_cpp.ev_lookup((ctypes.c_int * N_EVTable)(*group_rowIds))


def request_to_cpp_cache(group_rowIds, use_gpu=False, use_socket=False, evstore_gpu_id=0):
    if use_socket:
        establish_socket_conn()
    clean_arr_floats = cache_lookup_via_ctypes(group_rowIds)
    if not clean_arr_floats:
        print("ERROR: ev_lookup failed: " + _lib.lib().evs_last_error().decode())
        exit(-1)
    flat = torch.frombuffer((ctypes.c_float * (N_EVTable * EV_DIMENSION)).from_address(
        ctypes.addressof(clean_arr_floats.contents)), dtype=torch.float32).clone()
    if use_gpu:
        flat = flat.to(torch.device("cuda:" + str(evstore_gpu_id)))  # ONE copy instead of 26 (:148-150)
    for table_idx in range(N_EVTable):
        emb_weights_in_tensor[table_idx] = flat[table_idx * EV_DIMENSION:(table_idx + 1) * EV_DIMENSION].view(1, -1)
    return emb_weights_in_tensor


def save_state(path):
    """warm start of the manager's tiers (evs_manager_export; no reference counterpart -- the reference's manager is warmed
    by replaying the workload): one .npz with 'entries1' / 'state1' (and 'entries2' / 'state2' of a two-layer manager)."""
    import numpy as np
    L = _lib.lib() if cache_manager_cpp is None else cache_manager_cpp
    arrays = {}
    for tier in (1, 2):
        if tier == 2 and L.evs_manager_tier_capacity(2) <= 0:
            break
        n = L.evs_manager_export(tier, None, 0, None)
        if n < 0:
            _lib.check(int(n))
        entries, state = np.zeros((max(n, 1), 3), np.int64), np.zeros(20, np.int64)
        n2 = L.evs_manager_export(tier, entries.ctypes.data, n, state.ctypes.data)
        if n2 < 0:
            _lib.check(int(n2))
        arrays["entries%d" % tier], arrays["state%d" % tier] = entries[:n], state
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def load_state(path):
    """a save_state file into the manager's tiers (evs_manager_load, strict), before the first lookup"""
    import numpy as np
    L = _lib.lib() if cache_manager_cpp is None else cache_manager_cpp
    try:
        with np.load(path, allow_pickle=False) as z:
            d = {k: np.ascontiguousarray(z[k], np.int64) for k in z.files}
    except Exception as e:
        raise _lib.EvsError(_lib.EVS_EIO, "load_state: %s is not a readable state file (%s)" % (path, e))
    if "entries1" not in d or "state1" not in d:
        raise _lib.EvsError(_lib.EVS_EINVAL, "load_state: the file lacks 'entries1' / 'state1'")
    for tier in (1, 2):
        if "entries%d" % tier not in d:
            break
        entries, state = d["entries%d" % tier], d.get("state%d" % tier)
        if entries.ndim != 2 or entries.shape[1] != 3 or state is None or state.shape != (20,):
            raise _lib.EvsError(_lib.EVS_EINVAL, "load_state: tier %d needs (n, 3) entries and a (20,) state" % tier)
        _lib.check(L.evs_manager_load(tier, int(entries.shape[0]), entries.ctypes.data if entries.shape[0] else None, state.ctypes.data))
