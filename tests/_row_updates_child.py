"""Child process of tests/test_gpu_row_updates.py: the batched set-associative tier with 16 ways per set (EVS_SA_WAYS=16 is
read once per process, hence a process of its own) through the same case as the 8-way tier."""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

assert os.environ.get("EVS_SA_WAYS") == "16"
import evstore_dlrm_amd as E  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import _row_updates as ru  # noqa: E402

for codec in (32, 8):
    n = ru.batched_case(E, orc, "setassoc", None, codec, log=print)
    print("codec %d: %d resident keys updated" % (codec, n))
print("RESULT ok")
