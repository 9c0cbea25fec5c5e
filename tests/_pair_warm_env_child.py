"""Child process of tests/test_gpu_pair_warm_start.py: the refusal of the pair's warm start that hangs on a switch the library
reads once per process -- EVS_SA_PAIR=0 (each tier keeps set records of its own: there is no shared record to load).
EVS_EINVAL with the reason named, both caches left fresh: the pair goes on serving lookup_batch_c1c2 with records of its own,
and has nothing to export either."""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

assert os.environ.get("EVS_SA_PAIR") == "0"
import numpy as np  # noqa: E402
import torch  # noqa: E402

import evstore_dlrm_amd as E  # noqa: E402

L = E._lib
n_rows = [40, 1000, 5000]
g = torch.Generator(device="cuda")
g.manual_seed(5)
t8 = [torch.randint(0, 256, (n, 36), dtype=torch.uint8, device="cuda", generator=g) for n in n_rows]
t4 = [torch.randint(0, 256, (n, 18), dtype=torch.uint8, device="cuda", generator=g) for n in n_rows]
c1, c2 = E.GpuCache("evlfu", 64, 3, 36, 8, "cpp"), E.GpuCache("evlfu", 128, 3, 36, 4, "cpp")
c1.set_backing(t8)
c2.set_backing(t4)
entries = np.array([[1, 1, 3, 1, 0, 0], [2, 2, 17, 2, 1, 0]], np.int64)
try:
    E.load_state_c1c2(c1, c2, {"entries": entries, "state": None}, strict=False)
except L.EvsError as e:
    assert e.code == L.EVS_EINVAL and "EVS_SA_PAIR" in str(e), str(e)
else:
    raise AssertionError("the load was accepted")
rq = torch.tensor([[3, 17, 4000], [5, 18, 4001]], dtype=torch.int32, device="cuda")
for i in range(2):
    tier, out = E.lookup_batch_c1c2(c1, c2, rq, threshold=2)
    assert bool((tier > 0).all()) == (i == 1)          # nothing was loaded: the first batch misses, the second hits
assert c1.batch_stats()["size"] + c2.batch_stats()["size"] == 6
try:
    E.export_state_c1c2(c1, c2)
except L.EvsError as e:
    assert e.code == L.EVS_EINVAL and "records of its own" in str(e), str(e)
else:
    raise AssertionError("the export was accepted")
print("RESULT ok")
