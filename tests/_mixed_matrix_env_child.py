"""Child process of tests/test_gpu_mixed_matrix.py::test_rows_kernel_takes_the_u8_u4_pair_when_the_switch_is_off, under EVS_MIXED_RFQ=0 (read
once per process): mixed84_supported() then turns every shape away, so the (8, 4) cases and the one-hot decode probe of the parent run through
interact_mixed_rows_kernel -- its u8 and u4 chunk decoders at full code range, two classes inside one wave -- under the parent's assertions
(tests/_mixed_matrix.py).  The record must show rows_* names only, and the library must have read the switch as set."""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

assert os.environ.get("EVS_MIXED_RFQ") == "0"
import evstore_dlrm_amd as E  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import _mixed_matrix as MM  # noqa: E402

start = E._lib.mixed_kernels_seen()
assert sorted(start) == sorted(MM.ALL_NAMES) and not any(start.values())

for d in MM.DIMS:
    for case in MM.cases((8, 4), d):
        MM.run_case(E, orc, case, rfq_on=False)
    for cls in (1, 2):
        for NT in (1, 2):
            MM.run_probe(E, orc, d, cls, NT, itself=NT - 1, rfq_on=False)

end = E._lib.mixed_kernels_seen()
r84 = [k for k in end if end[k] and k.startswith("r84")]
assert not r84, r84
idle = [k for k in end if k.startswith("rows") and not end[k]]
assert not idle, idle
seen = E._lib.env_switches_seen()
assert seen.get("EVS_MIXED_RFQ") is True, seen
print("RESULT ok %d cases, %d launches" % (MM.N_CASES[0], MM.N_LAUNCHES[0]))
