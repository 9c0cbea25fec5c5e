"""Child process of tests/test_gpu_pooling_matrix.py::test_forms_the_default_environment_cannot_reach, under EVS_GATHER_LONG=0
EVS_GATHER_RF=0 (read once per process).  argv: the parent's CHILD_ONLY names.  Every case under the parent's two assertions
(tests/_pooling_matrix.py:check_case: the intended name of the dispatch record went up by the intended count, the output is the oracle's
bits):

  * bag_sum_flat_kernel<LPRD, true>, d = 16, 32, 36, 64: bags of 0..40 and one of 300 (above a tile at every d), mean above 16, B = 70 (a
    chunk of 64 bags and a partial one); once more over a row range;
  * the fp32 grid-stride kernels without weights, one (d, T) per compiled lanes per row: one index per bag declared.  With offsets =
    arange the same batches go to the tile kernel's plain form under these switches (asserted: the offsets form of the fp32 grid-stride
    kernel is the weighted batches' at d <= 64), and at d = 128 multi-hot bags of any mean reach the offsets form."""
import os
import sys

_repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, _repo)
sys.path.insert(0, os.path.join(_repo, "tests"))

assert os.environ.get("EVS_GATHER_LONG") == "0" and os.environ.get("EVS_GATHER_RF") == "0"
child_only = sys.argv[1:]
assert child_only
import numpy as np  # noqa: E402

import evstore_dlrm_amd as E  # noqa: E402
from oracle import oracle as orc  # noqa: E402

import _pooling_matrix as PM  # noqa: E402

start = E._lib.gather_kernels_seen()
assert not any(start.values())

for d in (16, 32, 36, 64):
    T, B = 3, 70
    rs = np.random.RandomState(500 + d)
    tabs = PM.make_tables(orc, rs, T, d, 32)
    lens = rs.randint(0, 41, size=(T, B))
    lens[:, 5] = 0
    lens[np.arange(T), [0, 33, 69]] = 300
    assert 16 * B * T < lens.sum() <= 128 * B * T
    idx, off = PM.make_bags(rs, tabs, lens)
    PM.check_case(E, orc, {PM.flat_name(d, True): 1}, B, d, 32, tabs, idx, off)
    PM.check_case(E, orc, {PM.flat_name(d, True): 1}, B, d, 32, tabs, idx, off, ranges=PM.mid_ranges(tabs))

for d, T in ((16, 5), (32, 5), (36, 5), (64, 5), (128, 3)):
    B = 4 * (64 // (d // 4)) + 3
    rs = np.random.RandomState(600 + d)
    tabs = PM.make_tables(orc, rs, T, d, 32)
    idx = PM.one_index_bags(rs, tabs, B)
    PM.check_case(E, orc, {PM.vec_name(32, d, True): 1}, B, d, 32, tabs, idx, None)
    arange = [np.arange(B, dtype=np.int64) for _ in range(T)]
    PM.check_case(E, orc, {PM.vec_name(32, d, False) if d == 128 else PM.flat_name(d, False): 1}, B, d, 32, tabs, idx, arange)
    if d == 128:
        idx, off = PM.make_bags(rs, tabs, rs.randint(0, 6, size=(T, B)))
        PM.check_case(E, orc, {PM.vec_name(32, d, False): 1}, B, d, 32, tabs, idx, off)

end = E._lib.gather_kernels_seen()
flat_rows_long = [k for k in end if end[k] and k.startswith(("rows_", "long_"))]
assert not flat_rows_long, flat_rows_long
missing = [k for k in child_only if end.get(k, 0) <= start.get(k, 0)]
assert not missing, "CHILD_ONLY names this child did not launch: %s" % missing
print("RESULT ok")
