"""Child process of tests/test_gpu_warm_start.py: the refusals of a warm-start load that hang on a switch the library reads
once per process -- EVS_SA_WAYS=16 (the load places into 8-way sets) and EVS_CACHE_POLICY=plan | sampled (a cache that was given
no batch policy resolves to it).  Each: EVS_EINVAL with the reason named, before anything is allocated, and the cache goes on
serving lookup_batch under what the switch selects."""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

want = sys.argv[1]
assert (os.environ.get("EVS_SA_WAYS") == "16") if want == "ways" else (os.environ.get("EVS_CACHE_POLICY") == want)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import evstore_dlrm_amd as E  # noqa: E402

L = E._lib
n_rows = [40, 1000, 5000]
g = torch.Generator(device="cuda")
g.manual_seed(5)
dev = [torch.empty(n, 36, device="cuda").uniform_(-1, 1, generator=g) for n in n_rows]
c = E.GpuCache("evlfu", 64, 3, 36, 32)
c.set_backing(dev)
entries = np.array([[1, 3, 1, 0, 0], [2, 17, 2, 1, 0]], np.int64)
try:
    c.load_state({"entries": entries, "state": None}, strict=False)
except L.EvsError as e:
    assert e.code == L.EVS_EINVAL, str(e)
    assert ("16 ways" if want == "ways" else want) in str(e), str(e)
else:
    raise AssertionError("the load was accepted")
rq = torch.tensor([[3, 17, 4000], [3, 17, 4000]], dtype=torch.int32, device="cuda")
for i in range(2):
    hit, out = c.lookup_batch(rq)
    assert bool(hit.all()) == (i == 1)                 # nothing was loaded: the first batch misses, the second hits
    for t in range(3):
        assert torch.equal(out[:, t].view(torch.int32), dev[t][rq[:, t].long()].view(torch.int32))
assert c.batch_stats()["size"] == 3
print("RESULT ok")
