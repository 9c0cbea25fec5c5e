"""CPU: the dispatch record of the mixed-precision interaction consumers (evs_mixed_kernels_seen) in a fresh process -- it parses, it lists
the 18 instantiations in their fixed order, and nothing has been launched; and evs_interact_rows_by_address turns bad arguments away before
it touches a device.  The text contract is evs_env_switches_seen's."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C
import re
import sys
sys.path.insert(0, %r)
import evstore_dlrm_amd as E
L = E._lib.lib()
n = L.evs_mixed_kernels_seen(None, 0)
buf = C.create_string_buffer(n + 1)
assert L.evs_mixed_kernels_seen(buf, n + 1) == n and len(buf.value) == n
text = buf.value.decode()
assert text.endswith("\n") and all(re.fullmatch(r"[a-z0-9_]+=\d+", ln) for ln in text.splitlines()), text
short = C.create_string_buffer(b"x" * 64, 64)
assert L.evs_mixed_kernels_seen(short, 30) == n and len(short.value) <= 29 and text.startswith(short.value.decode())
rec = E._lib.mixed_kernels_seen()
want = ["%%s_d%%d_nt%%d%%s" %% (f, d, nt, s) for f, s in (("rows", ""), ("r84", ""), ("r84", "_probe")) for d in (16, 32, 36) for nt in (1, 2)]
assert [ln.split("=")[0] for ln in text.splitlines()] == want == list(rec), "the 18 names, each once, in the fixed order"
assert not any(rec.values()), "nothing has been launched yet"

EINVAL = E._lib.EVS_EINVAL
def call(B=4, T=26, d=36, x=16, xs=36, ptrs=16, cls=None, c1=8, c2=4, itself=0, dflt=1, R=16):
    return L.evs_interact_rows_by_address(B, T, d, x, xs, ptrs, cls, c1, c2, itself, dflt, R, None)
assert call(d=20) == EINVAL and b"d=20" in L.evs_last_error()
assert call(d=64) == EINVAL
assert call(T=0) == EINVAL and b"T=0" in L.evs_last_error()
assert call(T=32) == EINVAL
assert call(c1=7) == EINVAL and b"codec" in L.evs_last_error()
assert call(c2=2) == EINVAL
assert call(B=-1) == EINVAL
assert call(dflt=0) == EINVAL and call(dflt=3) == EINVAL
assert call(x=None) == EINVAL and b"NULL" in L.evs_last_error()
assert call(R=None) == EINVAL and call(ptrs=None) == EINVAL
assert call(x=20) == EINVAL and call(R=8) == EINVAL and call(xs=38) == EINVAL and call(xs=32) == EINVAL
assert call(B=0, x=None, R=None, ptrs=None) == 0, "B == 0 is a no-op"
assert call(B=0, d=20) == EINVAL
assert not any(E._lib.mixed_kernels_seen().values()), "a refused call launches nothing"
print("RECORD ok %%d" %% len(rec))
""" % ROOT


def test_the_mixed_record_and_the_entry_checks_in_a_fresh_process():
    import evstore_dlrm_amd as E
    if not os.path.exists(E._lib.LIB_PATH):
        E.build()
    p = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "RECORD ok 18" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
