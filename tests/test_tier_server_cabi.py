"""CPU: the tier pair / triple server's C ABI (evs_tiers_serve_*, evs_manager_engine) is exported, bound by _lib, and checks
its arguments before it touches a device."""
import ctypes as C

NEW = ["evs_tiers_serve_start", "evs_tiers_serve_request", "evs_tiers_serve_request_to", "evs_tiers_serve_consumed",
       "evs_tiers_serve_stop", "evs_tiers_serve_destroy", "evs_manager_engine"]


def test_library_exports_and_binds_the_tier_server():
    import evstore_dlrm_amd as E
    raw = C.CDLL(E._lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), "missing export: " + name
        assert name in E._lib.exported_symbols(), "not bound: " + name
    L = E._lib.lib()
    for name in NEW:
        assert getattr(L, name).argtypes is not None
    assert L.evs_abi_version() == 1
    assert hasattr(E, "TierServer") and E.TierServer is E.gpu_cache.TierServer


def test_bad_arguments_are_rejected_without_a_gpu():
    import evstore_dlrm_amd as E
    L = E._lib.lib()
    EINVAL = E._lib.EVS_EINVAL
    h = C.c_void_p()
    # the first check looks at the pointers' values only: these stand-ins are never dereferenced
    fake1, fake2 = C.create_string_buffer(64), C.create_string_buffer(64)
    c1, c2, ring = C.addressof(fake1), C.addressof(fake2), C.addressof(fake1)
    cases = {"NULL out": (None, c1, c2, None, 23, ring, 4, 200),
             "NULL c1": (C.byref(h), None, c2, None, 23, ring, 4, 200),
             "NULL ring": (C.byref(h), c1, c2, None, 23, None, 4, 200),
             "n_slots 0": (C.byref(h), c1, c2, None, 23, ring, 0, 200),
             "idle_us 0": (C.byref(h), c1, c2, None, 23, ring, 4, 0)}
    for what, args in cases.items():
        assert L.evs_tiers_serve_start(*args) == EINVAL, what
        assert b"evs_tiers_serve_start" in L.evs_last_error(), what
        assert not h.value, what
    slot = C.c_int(0)
    assert L.evs_tiers_serve_request(None, c1, c2, C.byref(slot)) == EINVAL and b"evs_tiers_serve_request" in L.evs_last_error()
    assert L.evs_tiers_serve_request_to(None, c1, None, 0, ring, c2) == EINVAL and b"evs_tiers_serve_request_to" in L.evs_last_error()
    assert L.evs_tiers_serve_consumed(None, 0, None) == EINVAL
    assert L.evs_tiers_serve_stop(None) == EINVAL
    assert L.evs_tiers_serve_destroy(None) == 0


def test_manager_engine_is_zero_before_configuration():
    """in a process of its own: the manager is a process-wide singleton another test of this run may have configured"""
    import os
    import subprocess
    import sys
    import evstore_dlrm_amd as E
    code = ("import ctypes, sys; L = ctypes.CDLL(sys.argv[1]); L.evs_manager_engine.restype = ctypes.c_int; "
            "print('ENGINE', L.evs_manager_engine())")
    env = {k: v for k, v in os.environ.items() if not k.startswith("EVS_")}
    out = subprocess.run([sys.executable, "-c", code, E._lib.LIB_PATH], capture_output=True, text=True, timeout=120, env=env)
    assert "ENGINE 0" in out.stdout, out.stdout[-1000:] + out.stderr[-1000:]
