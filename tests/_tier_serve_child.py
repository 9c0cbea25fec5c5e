"""Child process of tests/test_gpu_tier_server.py: two caching layers over HBM tables through ev_lookup, with or without
EVS_MANAGER_SERVE in the environment; prints which engine the manager chose (evs_manager_engine) and whether every row
equals the oracle's.  The manager is a process-wide singleton, hence a process of its own."""
import ctypes
import json
import os
import sys

import numpy as np

root = sys.argv[1]
_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
from oracle import oracle as orc  # noqa: E402

L = ctypes.CDLL(os.path.join(_repo, "ev-store-dlrm_amd", "lib", "libevstore_hip.so"))
L.ev_lookup.argtypes = [ctypes.POINTER(ctypes.c_int)]
L.ev_lookup.restype = ctypes.POINTER(ctypes.c_float)
L.evs_manager_engine.restype = ctypes.c_int
L.evs_manager_perfect_hit.restype = ctypes.c_longlong

rs = np.random.RandomState(11)
n, total = 120, 20
ws = [rs.uniform(-1, 1, size=(n, 36)).astype(np.float32) for _ in range(26)]
raw8 = [orc.encode_table(w, 8) for w in ws]
raw4 = [orc.encode_table(w, 4) for w in ws]
for sub, raws in (("ev-table-8", raw8), ("ev-table-4", raw4)):
    os.makedirs(os.path.join(root, sub, "binary"))
    for k, r in enumerate(raws):
        r.tofile(os.path.join(root, sub, "binary", "ev-table-%d.bin" % (k + 1)))
os.environ.update({"EVS_EV_TABLE_ROOT": root, "EVS_MAIN_PRECISION": "8", "EVS_SECONDARY_PRECISION": "4",
                   "EVS_TOTAL_SIZE": str(total), "EVS_N_CACHING_LAYER": "2", "EVS_BACKING": "hbm"})
before = int(L.evs_manager_engine())
o = orc.C1C2((total // 2) * 4, (total // 2) * 8, [orc.decode(r, 8, 36) for r in raw8], [orc.decode(r, 4, 36) for r in raw4])
reqs = np.minimum(rs.zipf(1.2, size=(50, 26)) - 1, n - 1).astype(np.int32)
ok, perfect = True, 0
for rq in reqs:
    ptr = L.ev_lookup((ctypes.c_int * 26)(*[int(v) for v in rq]))
    if not ptr:
        print("ev_lookup returned NULL")
        sys.exit(3)
    got = np.ctypeslib.as_array(ptr, shape=(26, 36)).copy()
    _, vals, p = o.request(rq)
    perfect += p
    ok = ok and np.array_equal(got.view(np.uint32), vals.view(np.uint32))
print("RESULT " + json.dumps({"before": before, "engine": int(L.evs_manager_engine()), "ok": bool(ok),
                              "counter": int(L.evs_manager_perfect_hit()), "perfect_oracle": int(perfect)}))
