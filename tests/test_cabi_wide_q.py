"""CPU: evs_emb_interact_wide_q_stacked refuses what it has no kernel for before it touches a device; B = 0; the dispatch record."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wideq_c%d_d%d_nt%d" % (c, d, n) for c in (16, 8, 4) for d in (16, 32, 36, 64) for n in (3, 4, 6, 8)]


def _arr(ty, n, v, at):
    a = (ty * max(n, 1))(*([v] * max(n, 1)))
    for k, w in at.items():
        a[k] = w
    return a


def _call(L, B=4, T=39, d=36, codec=8, table=0x1000, n_rows=7, x=0x2000, x_stride=36, idx=0x4000, R=0x9000, at_table={}, at_rows={}):
    """the call over made-up device addresses (a refused call reads none of them)"""
    ts = None if table is None else _arr(C.c_void_p, T, table, at_table)
    return L.evs_emb_interact_wide_q_stacked(B, T, d, codec, ts, _arr(C.c_int64, T, n_rows, at_rows), x, x_stride, idx, B, 0, R, None)


@pytest.mark.parametrize("kw,word", [
    (dict(codec=32), b"evs_emb_interact_wide_stacked"), (dict(codec=7), b"codec 7"), (dict(codec=0), b"codec 0"),
    (dict(T=31), b"F=32"), (dict(T=128), b"F=129"), (dict(d=48), b"d=48"),
    (dict(table=None), b"NULL"), (dict(x=None), b"NULL"), (dict(idx=None), b"NULL"), (dict(R=None), b"NULL"),
    (dict(at_table={2: None}), b"table 2 is NULL"), (dict(at_table={38: 0x1004}), b"table 38 is not 16-byte aligned"),
    (dict(x=0x2004), b"x is not"), (dict(R=0x9004), b"R is not"), (dict(at_rows={1: 1 << 31}), b"2^31"), (dict(B=1 << 31), b"2^31")])
def test_refusals_without_a_device(kw, word):
    import evstore_dlrm_amd as E
    L = E._lib.lib()
    before = E._lib.wide_q_kernels_seen()
    assert _call(L, **kw) == E._lib.EVS_EINVAL and word in L.evs_last_error()
    assert E._lib.wide_q_kernels_seen() == before


def test_empty_batch_succeeds():
    import evstore_dlrm_amd as E
    L = E._lib.lib()
    before = E._lib.wide_q_kernels_seen()
    assert all(_call(L, B=0, codec=c) == 0 for c in (16, 8, 4)) and _call(L, B=0, table=None, x=None, R=None) == 0
    assert E._lib.wide_q_kernels_seen() == before


def test_record_lists_the_names_at_zero_in_a_fresh_process():
    code = "import evstore_dlrm_amd as E; print(E._lib.wide_q_kernels_seen())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True, timeout=120).stdout
    assert eval(out) == {n: 0 for n in NAMES} and list(eval(out)) == NAMES
