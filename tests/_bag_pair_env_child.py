"""Child process of tests/test_gpu_cache_bags_pair.py: the refusal of the pair's bag form that hangs on a switch the library
reads once per process -- EVS_SA_PAIR=0 (each tier keeps set records of its own: there is no shared record for the bag probe to
read).  EVS_EINVAL with the switch named by both forms, nothing allocated; the pair goes on serving lookup_batch_c1c2 with
records of its own, and is refused again -- as a pair that did not start out over one record -- once it has started."""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

assert os.environ.get("EVS_SA_PAIR") == "0"
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
c1.set_bag_rule("served-bags")
c2.set_bag_rule("served-bags")
lo = [torch.arange(2, dtype=torch.int64, device="cuda")] * 3
li = [torch.tensor([r, r + 1], dtype=torch.int64, device="cuda") for r in (3, 17, 4000)]
x = torch.zeros((2, 36), device="cuda")


def refused(word):
    for fn in (lambda: E.lookup_bags_c1c2(c1, c2, lo, li, threshold=2), lambda: E.lookup_bags_interact_c1c2(c1, c2, lo, li, x, threshold=2)):
        try:
            fn()
        except L.EvsError as e:
            assert e.code == L.EVS_EINVAL and word in str(e), str(e)
        else:
            raise AssertionError("the bag call was accepted")


refused("EVS_SA_PAIR")
rq = torch.tensor([[3, 17, 4000], [4, 18, 4001]], dtype=torch.int32, device="cuda")
for i in range(2):
    tier, out = E.lookup_batch_c1c2(c1, c2, rq, threshold=2)
    assert bool((tier > 0).all()) == (i == 1)          # the refusals inserted nothing: the first batch misses, the second hits
assert c1.batch_stats()["size"] + c2.batch_stats()["size"] == 6
refused("set records")
tier, out = E.lookup_batch_c1c2(c1, c2, rq, threshold=2)
assert bool((tier > 0).all())
print("RESULT ok")
