"""Child process of tests/test_gpu_batch_approx.py: EVS_SA_WAYS=16 is read once per process.  With 16-way sets a batched call
with an approximate threshold in force is refused -- EVS_EINVAL, the switch and the policy named, before anything is allocated --
and the cache goes on serving once the threshold is off."""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

assert os.environ.get("EVS_SA_WAYS") == "16"
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

c = E.GpuCache("evlfu", 64, 3, 16, 32).set_batch_approx(2)
c.set_backing(dev)
try:
    c.lookup_batch(rq)
except L.EvsError as e:
    assert e.code == L.EVS_EINVAL, str(e)
    assert "EVS_SA_WAYS" in str(e) and "evlfu" in str(e), str(e)
else:
    raise AssertionError("the call was accepted")
assert c.approx_stats() == {"calls": 0, "samples": 0, "substituted": 0, "zero_rows": 0}
c.set_batch_approx(0)
for i in range(2):
    hit, out = c.lookup_batch(rq)
    for t in range(3):
        assert np.array_equal(out[:, t].cpu().numpy().view(np.uint32), tabs[t][rq_np[:, t]].view(np.uint32))
assert bool((hit == 1).all())
assert c.approx_stats()["calls"] == 0
print("RESULT ok")
