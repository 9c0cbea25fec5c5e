"""Child process of tests/test_gpu_bags_count_first.py: EVS_SA_DUAL and EVS_SA_WAYS are read once per process.
argv[1] = EVS_SA_DUAL (the parent set it to 0): an order-1 count-first EvLFU bag call is refused -- EVS_EINVAL, the switch named,
nothing allocated, the cache serving once told "consume-first" -- and over the one-copy arena an order-0 count-first cache equals
the default chain call by call.  argv[1] = EVS_SA_WAYS (16): the order-1 call is refused with that switch named."""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

switch = sys.argv[1]
assert os.environ.get(switch) == {"EVS_SA_DUAL": "0", "EVS_SA_WAYS": "16"}[switch]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import _bag_evlfu_model as EM  # noqa: E402
import evstore_dlrm_amd as E  # noqa: E402

L = E._lib
n_rows = [5, 3000, 70]
rs = np.random.RandomState(5)
tabs = [rs.uniform(-1, 1, size=(n, 16)).astype(np.float32) for n in n_rows]
dev = [torch.from_numpy(t).cuda() for t in tabs]
calls = EM.conflict_free_bag_stream(64, n_rows, 9, 3, 6, 4)[0]


def up(off, idx):
    return [torch.from_numpy(o).cuda() for o in off], [torch.from_numpy(i).cuda() for i in idx]


def cache(order=None, count=None, backing=dev):
    c = E.GpuCache("evlfu", 64, 3, 16, 32)
    if order:
        c.set_miss_order(order)
    c.set_backing(backing)
    c.set_bag_rule("served-bags")
    return c.set_bag_count(count) if count else c


c = cache("fetch-first", "count-first", [torch.from_numpy(t.copy()).pin_memory() for t in tabs])
try:
    c.lookup_bags(*up(*calls[0][:2]))
except L.EvsError as e:
    assert e.code == L.EVS_EINVAL, str(e)
    assert switch in str(e) and "evlfu" in str(e), str(e)
else:
    raise AssertionError("the call was accepted")
assert c.fetch_stats() == {"calls": 0, "repointed": 0, "in_place": 0}

if switch == "EVS_SA_DUAL":
    c.set_miss_order("consume-first")              # (nothing was allocated: the order may still be set)
    c.set_backing(dev)
    a = cache()
    for off, idx, want in calls:
        lS_o, lS_i = up(off, idx)
        (ha, la), (hc, lc) = a.lookup_bags(lS_o, lS_i), c.lookup_bags(lS_o, lS_i)
        assert torch.equal(torch.cat(ha), torch.cat(hc))
        assert np.array_equal(torch.cat(hc).cpu().numpy().astype(bool), np.concatenate(want))
        assert torch.equal(torch.stack(la).view(torch.int32), torch.stack(lc).view(torch.int32))
        assert sorted(map(tuple, a.batch_dump())) == sorted(map(tuple, c.batch_dump()))
        assert a.batch_stats() == c.batch_stats()
    assert c.fetch_stats()["calls"] == 0 and a.batch_stats()["n_hits"] > 0
print("RESULT ok")
