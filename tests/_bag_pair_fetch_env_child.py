"""Child process of tests/test_gpu_bag_pair_fetch_first.py: the refusals of the fetch-first bag form of the C1 + C2 pair that hang
on switches the library reads once per process.  argv[1] names the switch the parent has set:
  EVS_SA_PAIR=0                   each tier would keep set records of its own -- EVS_EINVAL naming the policy and the switch;
                                  nothing was allocated, so both tiers can be set back to consume-first and serve as that pair
  EVS_CACHE_POLICY=sampled|plan   the process-wide policy is not the set-associative one -- EVS_EINVAL naming it; a policy given
                                  to the tiers themselves outranks the switch, and the pair then serves bags fetch-first"""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

switch = sys.argv[1]
value = os.environ.get(switch)
assert value, switch
import torch  # noqa: E402

import evstore_dlrm_amd as E  # noqa: E402

L = E._lib
n_rows = [200, 1000, 4000]
g = torch.Generator(device="cuda")
g.manual_seed(5)
t8 = [torch.randint(0, 256, (n, 36), dtype=torch.uint8, device="cuda", generator=g) for n in n_rows]
t4 = [torch.randint(0, 256, (n, 18), dtype=torch.uint8, device="cuda", generator=g) for n in n_rows]
keep = [[t.cpu().pin_memory() for t in t8], [t.cpu().pin_memory() for t in t4]]
c1 = E.GpuCache("evlfu", 64, 3, 36, 8, "cpp").set_miss_order("fetch-first").set_bag_rule("served-bags").set_bag_count("count-first")
c2 = E.GpuCache("evlfu", 128, 3, 36, 4, "cpp").set_miss_order("fetch-first").set_bag_rule("served-bags").set_bag_count("count-first")
lo = [torch.tensor(o, dtype=torch.int64, device="cuda") for o in ([0, 2], [0, 1], [0, 0])]
li = [torch.tensor(i, dtype=torch.int64, device="cuda") for i in ([3, 5], [17, 18], [150, 151])]
if switch == "EVS_SA_PAIR":
    c1.set_backing(t8)                                 # (over HBM: what the tiers fall back on must serve these tables)
    c2.set_backing(t4)
    word = "EVS_SA_PAIR"
else:
    c1.set_backing(keep[0])
    c2.set_backing(keep[1])
    word = value
try:
    E.lookup_bags_c1c2(c1, c2, lo, li, threshold=2)
except L.EvsError as e:
    assert e.code == L.EVS_EINVAL and word in str(e) and "evlfu" in str(e), str(e)
else:
    raise AssertionError("the call was accepted")
assert c1.fetch_stats() == {"calls": 0, "repointed": 0, "in_place": 0}
if switch == "EVS_SA_PAIR":
    # (nothing was allocated: the order may still be set; without the shared record the pair has no bag form at all, so it serves
    #  the (B, T) form)
    c1.set_miss_order("consume-first")
    c2.set_miss_order("consume-first")
    rq = torch.tensor([[3, 17, 150], [5, 18, 151]], dtype=torch.int32, device="cuda")
    for i in range(2):
        tier, out = E.lookup_batch_c1c2(c1, c2, rq, threshold=2)
        assert bool((tier > 0).all()) == (i == 1)      # the first batch misses, the second hits
    assert c1.fetch_stats()["calls"] == 0
else:
    c1.set_batch_policy("setassoc")
    c2.set_batch_policy("setassoc")
    for i in range(2):
        tiers, ly = E.lookup_bags_c1c2(c1, c2, lo, li, threshold=2)
        assert bool((torch.cat(tiers) > 0).all()) == (i == 1)
    assert c1.fetch_stats()["calls"] == 2
assert c1.batch_stats()["size"] + c2.batch_stats()["size"] == 6
print("RESULT ok")
