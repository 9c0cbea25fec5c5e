"""Child process of tests/test_gpu_cache_bags_evlfu.py: the refusals of the EvLFU bag form that hang on a switch the library
reads once per process -- EVS_SA_WAYS=16 (the bag kernels are compiled for 8-way sets) and EVS_CACHE_POLICY=plan | sampled (a
cache that was given no batch policy resolves to it).  Each: EVS_EINVAL with the policy named, before anything is allocated,
and the cache goes on serving lookup_batch under what the switch selects."""
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
from oracle import oracle as orc  # noqa: E402

L = E._lib
tabs = orc.kaggle_tables([300] * 26, 4)
dev = [torch.from_numpy(t).cuda() for t in tabs]
rq = torch.zeros((4, 26), dtype=torch.int32, device="cuda")
lo = [torch.arange(4, dtype=torch.int64, device="cuda")] * 26
li = [torch.zeros(4, dtype=torch.int64, device="cuda")] * 26
x = torch.zeros((4, 36), device="cuda")
c = E.GpuCache("evlfu", 512, 26, 36, 32)
c.set_backing(dev)
c.set_bag_rule("served-bags")
for call in (lambda: c.lookup_bags(lo, li), lambda: c.lookup_bags_interact(lo, li, x)):
    try:
        call()
    except L.EvsError as e:
        assert e.code == L.EVS_EINVAL and "evlfu" in str(e), str(e)
        assert ("8 ways" if want == "ways" else want) in str(e), str(e)
    else:
        raise AssertionError("the bag call was accepted")
for _ in range(2):
    hit, out = c.lookup_batch(rq)
    assert np.array_equal(out.cpu().numpy()[:, 3].view(np.uint32), tabs[3][[0] * 4].view(np.uint32))
assert hit.all()
st = c.batch_stats()
assert st["size"] == 26 and st["n_requests"] == 8
print("RESULT ok")
