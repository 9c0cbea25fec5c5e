"""CPU: evs_interact_dot_wide and evs_emb_interact_wide_stacked refuse what they have no kernel for before they touch a device; B = 0; the dispatch record."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["wide_%s_d%d_nt%d" % (f, d, n) for f in ("dense", "gather") for d in (16, 32, 36, 64) for n in (3, 4, 6, 8)]


def _arr(ty, n, v, at):
    a = (ty * max(n, 1))(*([v] * max(n, 1)))
    for k, w in at.items():
        a[k] = w
    return a


def _dense(L, B=4, F=40, d=36, feats=0x1000, stride=36, R=0x9000, at_feats={}, at_stride={}):
    """the dense call over made-up device addresses (a refused call reads none of them)"""
    fs = None if feats is None else _arr(C.c_void_p, F, feats, at_feats)
    return L.evs_interact_dot_wide(B, F, d, fs, _arr(C.c_int64, F, stride, at_stride), 0, R, None)


def _gather(L, B=4, T=39, d=36, table=0x1000, n_rows=7, x=0x2000, x_stride=36, idx=0x4000, R=0x9000, at_table={}, at_rows={}):
    ts = None if table is None else _arr(C.c_void_p, T, table, at_table)
    return L.evs_emb_interact_wide_stacked(B, T, d, ts, _arr(C.c_int64, T, n_rows, at_rows), x, x_stride, idx, B, 0, R, None)


@pytest.mark.parametrize("call,kw,word", [
    (_dense, dict(F=32), b"F=32"), (_dense, dict(F=129), b"F=129"), (_dense, dict(d=48), b"d=48"), (_dense, dict(d=0), b"d=0"),
    (_dense, dict(feats=None), b"NULL"), (_dense, dict(R=None), b"NULL"), (_dense, dict(at_feats={3: None}), b"feats[3] is NULL"),
    (_dense, dict(at_feats={39: 0x1008}), b"feats[39] is not 16-byte aligned"), (_dense, dict(at_stride={5: 38}), b"multiple of 4"),
    (_dense, dict(R=0x9008), b"R is not 16-byte aligned"), (_dense, dict(B=1 << 31), b"2^31"),
    (_gather, dict(T=31), b"F=32"), (_gather, dict(T=128), b"F=129"), (_gather, dict(d=20), b"d=20"), (_gather, dict(table=None), b"NULL"),
    (_gather, dict(x=None), b"NULL"), (_gather, dict(idx=None), b"NULL"), (_gather, dict(R=None), b"NULL"),
    (_gather, dict(at_table={2: None}), b"table 2 is NULL"), (_gather, dict(at_table={38: 0x1004}), b"table 38 is not 16-byte aligned"),
    (_gather, dict(x=0x2004), b"x is not"), (_gather, dict(x_stride=38), b"multiple of 4"), (_gather, dict(R=0x9004), b"R is not"),
    (_gather, dict(at_rows={1: 1 << 31}), b"2^31"), (_gather, dict(B=1 << 31), b"2^31")])
def test_refusals_without_a_device(call, kw, word):
    import evstore_dlrm_amd as E
    L = E._lib.lib()
    before = E._lib.wide_kernels_seen()
    assert call(L, **kw) == E._lib.EVS_EINVAL and word in L.evs_last_error()
    assert E._lib.wide_kernels_seen() == before


def test_empty_batches_succeed():
    import evstore_dlrm_amd as E
    L = E._lib.lib()
    assert _dense(L, B=0) == 0 and _gather(L, B=0) == 0 and _dense(L, B=0, feats=None, R=None) == 0
    assert E.wide_supported(33, 36) and E.wide_supported(128, 64) and not E.fused_supported(33, 36)
    assert not any(E.wide_supported(F, d) for F, d in ((32, 36), (129, 36), (40, 48), (40, 128)))


def test_record_lists_the_names_at_zero_in_a_fresh_process():
    code = "import evstore_dlrm_amd as E; print(E._lib.wide_kernels_seen())"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True, timeout=120).stdout
    assert eval(out) == {n: 0 for n in NAMES} and list(eval(out)) == NAMES
