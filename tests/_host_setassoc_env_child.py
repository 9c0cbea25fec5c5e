"""Child process of tests/test_gpu_host_setassoc.py: EVS_SA_DUAL=0 is read once per process.  With one arena row per way an
EvLFU cache in fetch-first order is refused -- EVS_EINVAL, the switch named, before anything is allocated -- and goes on
serving once told "consume-first"; an LRU cache runs fetch-first over pinned tables on the one-copy arena."""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

assert os.environ.get("EVS_SA_DUAL") == "0"
import numpy as np  # noqa: E402
import torch  # noqa: E402

import evstore_dlrm_amd as E  # noqa: E402

L = E._lib
n_rows = [5, 3000, 70]
rs = np.random.RandomState(5)
tabs = [rs.uniform(-1, 1, size=(n, 16)).astype(np.float32) for n in n_rows]
dev = [torch.from_numpy(t).cuda() for t in tabs]
rq_np = np.stack([rs.randint(0, n, 9) for n in n_rows], 1).astype(np.int32)
rq = torch.from_numpy(rq_np).cuda()


def serves(c):
    for i in range(2):
        hit, out = c.lookup_batch(rq)
        for t in range(3):
            assert np.array_equal(out[:, t].cpu().numpy().view(np.uint32), tabs[t][rq_np[:, t]].view(np.uint32))
    assert bool(hit.all())


c = E.GpuCache("evlfu", 64, 3, 16, 32).set_miss_order("fetch-first")
c.set_backing(dev)
try:
    c.lookup_batch(rq)
except L.EvsError as e:
    assert e.code == L.EVS_EINVAL, str(e)
    assert "EVS_SA_DUAL" in str(e) and "evlfu" in str(e), str(e)
else:
    raise AssertionError("the call was accepted")
assert c.fetch_stats() == {"calls": 0, "repointed": 0, "in_place": 0}
c.set_miss_order("consume-first")                  # (nothing was allocated: the order may still be set)
serves(c)
assert c.fetch_stats()["calls"] == 0

c = E.GpuCache("lru", 64, 3, 16, 32).set_miss_order("fetch-first")
c.set_backing([torch.from_numpy(t.copy()).pin_memory() for t in tabs])
serves(c)
f = c.fetch_stats()
assert f["calls"] == 2 and f["repointed"] == rq_np.size and f["in_place"] == 0, f
print("RESULT ok")
