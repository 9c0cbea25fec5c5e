"""CPU: the gather's dispatch record (evs_gather_kernels_seen) in a fresh process -- it parses, it lists every kernel family for every
codec the family is built for, and nothing has been launched.  The text contract is evs_env_switches_seen's."""
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
n = L.evs_gather_kernels_seen(None, 0)
buf = C.create_string_buffer(n + 1)
assert L.evs_gather_kernels_seen(buf, n + 1) == n and len(buf.value) == n
text = buf.value.decode()
assert text.endswith("\n") and all(re.fullmatch(r"[a-z0-9_]+=\d+", ln) for ln in text.splitlines()), text
short = C.create_string_buffer(b"x" * 64, 64)
assert L.evs_gather_kernels_seen(short, 30) == n and len(short.value) <= 29 and text.startswith(short.value.decode())
rec = E._lib.gather_kernels_seen()
assert len(rec) == len(text.splitlines()), "a name is listed once"
assert not any(rec.values()), "nothing has been launched yet"
pat = {"rows": r"rows_c%%d_lpr(4|8|9|16)_nj\d_(check|declared)", "vec": r"vec_c%%d_lpr(0|4|8|9|16|32)_(bag1|offsets)", "scalar": r"scalar_c%%d"}
for fam, p in pat.items():
    for c in (32, 16, 8, 4):
        assert [k for k in rec if re.fullmatch(p %% c, k)], (fam, c)
assert sorted(k for k in rec if k.startswith("long_")) == sorted("long_c32_lpr%%d_k%%d" %% lk for lk in ((4, 8), (8, 8), (9, 9), (16, 16), (32, 16)))
assert sorted(k for k in rec if k.startswith("flat_")) == sorted("flat_c32_lpr%%d_%%s" %% (l, f) for l in (4, 8, 9, 16) for f in ("select", "plain"))
for c in (32, 16, 8, 4):
    assert len([k for k in rec if k.startswith("rows_c%%d_" %% c)]) == 26 and len([k for k in rec if k.startswith("vec_c%%d_" %% c)]) == 12
assert all(k.split("_")[0] in ("rows", "long", "flat", "vec", "scalar") for k in rec)
print("RECORD ok %%d" %% len(rec))
""" % ROOT


def test_the_gather_record_in_a_fresh_process():
    import evstore_dlrm_amd as E
    if not os.path.exists(E._lib.LIB_PATH):
        E.build()
    p = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "RECORD ok 169" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
