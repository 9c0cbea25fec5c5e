"""Child process of tests/test_ev_lookup_warm.py (the cache manager is a process-wide singleton): the manager behind
cache_algo/cpp_socket_client.py serves reqs[start:stop] through ev_lookup, after load_state(load) when a state file is given
and before save_state(save) when one is asked for; the served rows and the perfect-hit counter go to `out`."""
import json
import os
import sys

import numpy as np

root, prec, total, layers, backing, start, stop, load, save, out = sys.argv[1:11]
start, stop = int(start), int(stop)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
os.environ["EVS_EV_TABLE_ROOT"] = root            # zero-argument path: configuration from the environment
os.environ["EVS_MAIN_PRECISION"] = prec
os.environ["EVS_TOTAL_SIZE"] = total
os.environ["EVS_BACKING"] = backing
os.environ["EVS_N_CACHING_LAYER"] = layers
os.environ["EVS_SECONDARY_PRECISION"] = "4"

import evstore_dlrm_amd  # noqa: E402,F401  (import shim)
from evstore_dlrm_amd import _lib  # noqa: E402
from evstore_dlrm_amd.cache_algo import cpp_socket_client as M  # noqa: E402

M.init_ctypes_lib()
refused = None
if layers == "3":   # the alt-key tier has no export: both directions are refused, the manager stays usable
    refused_load = None
    try:
        M.save_state(save)
    except _lib.EvsError as e:
        refused = e.code
    try:
        M.load_state(load)
    except _lib.EvsError as e:
        refused_load = e.code
    served = bool(M.request_to_cpp_cache([0] * 26))
    print("RESULT " + json.dumps({"refused": refused, "refused_load": refused_load, "served": served}))
    sys.exit(0)
if load != "-":
    M.load_state(load)
reqs = np.load(os.path.join(root, "reqs.npy"))[start:stop]
rows = np.zeros((len(reqs), 26, 36), np.float32)
for i, rq in enumerate(reqs):
    ly = M.request_to_cpp_cache([int(v) for v in rq])
    rows[i] = np.concatenate([t.numpy() for t in ly])
perfect = int(_lib.lib().evs_manager_perfect_hit())
if save != "-":
    M.save_state(save)
    # a manager that has served requests is no target of a load
    try:
        M.load_state(save)
    except _lib.EvsError as e:
        refused = e.code
np.save(out, rows)
print("RESULT " + json.dumps({"perfect": perfect, "refused": refused, "engine": int(_lib.lib().evs_manager_engine())}))
