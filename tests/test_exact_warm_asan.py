"""The host engine's warm start (evs_hostcache_export / evs_hostcache_load / evs_exact_load_check) under AddressSanitizer +
UBSan on the CPU: csrc/evs_hostcache.hip compiled host-only with hipcc's clang together with a stand-alone driver with its own
main (tools/exact_warm_asan.cpp) and run as a program of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_host_warm_start_is_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "exact_warm_asan")
    csrc = os.path.join(ROOT, "ev-store-dlrm_amd", "csrc")
    cmd = [HIPCC, "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "evs_hostcache.hip"),
           os.path.join(csrc, "evs_api.hip"), os.path.join(ROOT, "tools", "exact_warm_asan.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "exact warm start sanitizer run ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
