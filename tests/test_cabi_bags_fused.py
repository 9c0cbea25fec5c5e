"""CPU: evs_emb_interact_bags refuses what it has no kernel for before it touches a device; the stage size and the dispatch record."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _call(L, B=4, T=2, d=36, table=0x1000, x=0x2000, off=0x3000, nnz=5, n_rows=7, off_len=None):
    """the call over made-up device addresses (a refused call reads none of them)"""
    arr = lambda ty, v: (ty * T)(*([v] * T))
    return L.evs_emb_interact_bags(B, T, d, arr(C.c_void_p, table), arr(C.c_int64, n_rows), x, d, arr(C.c_void_p, 0x4000),
                                   arr(C.c_int64, nnz), arr(C.c_void_p, off), arr(C.c_int64, B if off_len is None else off_len),
                                   0, 0x5000, None)


@pytest.mark.parametrize("kw,word", [(dict(d=48), b"d=48"), (dict(d=128), b"d=128"), (dict(T=28), b"T=28"), (dict(T=0), b"T=0"),
                                     (dict(off=None), b"offsets"), (dict(table=0x1008), b"aligned"), (dict(x=0x2004), b"aligned"),
                                     (dict(B=1 << 31), b"2^31"), (dict(nnz=1 << 31), b"2^31"), (dict(n_rows=1 << 31), b"2^31"),
                                     (dict(nnz=(1 << 30) + 1), b"lookups"), (dict(off_len=6), b"offsets_len")])
def test_refusals_without_a_device(kw, word):
    import evstore_dlrm_amd as E
    L = E._lib.lib()
    before = E._lib.bags_fused_kernels_seen()
    assert _call(L, **kw) == E._lib.EVS_EINVAL and word in L.evs_last_error()
    assert E._lib.bags_fused_kernels_seen() == before


def test_empty_batch_and_stage_rows():
    import evstore_dlrm_amd as E
    L = E._lib.lib()
    assert _call(L, B=0) == 0
    assert [L.evs_bags_fused_stage_rows(d) for d in (16, 32, 36, 64, 48, 128, 0)] == [64, 32, 28, 16, 0, 0, 0]


def test_record_lists_the_eight_names_at_zero_in_a_fresh_process():
    code = "import evstore_dlrm_amd as E; print(E._lib.bags_fused_kernels_seen())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True, timeout=120).stdout
    assert eval(out) == {"bagsf_d%d_nt%d" % (d, nt): 0 for d in (16, 32, 36, 64) for nt in (1, 2)}
    assert list(eval(out)) == ["bagsf_d%d_nt%d" % (d, nt) for d in (16, 32, 36, 64) for nt in (1, 2)]
