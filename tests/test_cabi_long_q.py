"""CPU: evs_embedding_bag_sum_long refuses what it has no kernel for before it touches a device; the chunk query and the dispatch record."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["longq_c%d_lpr%d" % (c, l) for c in (16, 8, 4) for l in (4, 8, 9, 16, 32)]


def _call(L, T=2, B=4, d=36, codec=8, table=0x1000, n_rows=7, idx=0x4000, off=0x3000, nnz=5, out=0x5000, tstride=144, bstride=36):
    """the call over made-up device addresses (a refused call reads none of them)"""
    arr = lambda ty, v: (ty * max(T, 1))(*([v] * max(T, 1)))
    return L.evs_embedding_bag_sum_long(T, B, d, codec, arr(C.c_void_p, table), arr(C.c_int64, n_rows), arr(C.c_void_p, idx),
                                        arr(C.c_void_p, off), arr(C.c_int64, nnz), out, tstride, bstride, None)


@pytest.mark.parametrize("kw,word", [(dict(codec=32), b"codec 32"), (dict(codec=2), b"codec 2"), (dict(d=48), b"d=48"), (dict(d=0), b"d=0"),
                                     (dict(off=None), b"offsets"), (dict(nnz=1 << 31), b"2^31"), (dict(n_rows=1 << 31), b"2^31"),
                                     (dict(B=1 << 31), b"2^31"), (dict(out=0x5008), b"aligned"), (dict(tstride=146), b"multiples of 4"),
                                     (dict(bstride=38), b"multiples of 4"), (dict(table=0x1008), b"aligned"), (dict(table=None), b"is NULL"),
                                     (dict(idx=None), b"is NULL")])
def test_refusals_without_a_device(kw, word):
    import evstore_dlrm_amd as E
    L = E._lib.lib()
    before = E._lib.long_q_kernels_seen()
    assert _call(L, **kw) == E._lib.EVS_EINVAL and word in L.evs_last_error()
    assert E._lib.long_q_kernels_seen() == before


def test_empty_calls_and_the_chunk():
    import evstore_dlrm_amd as E
    L = E._lib.lib()
    assert _call(L, B=0) == 0 and _call(L, T=0) == 0
    assert all(L.evs_long_q_chunk(c, d) > 0 for c in (16, 8, 4) for d in (16, 32, 36, 64, 128))
    assert [L.evs_long_q_chunk(c, d) for c, d in ((32, 36), (8, 48), (8, 0))] == [0, 0, 0]


def test_record_lists_the_fifteen_names_at_zero_in_a_fresh_process():
    code = "import evstore_dlrm_amd as E; print(E._lib.long_q_kernels_seen())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True, timeout=120).stdout
    assert eval(out) == {n: 0 for n in NAMES} and list(eval(out)) == NAMES
