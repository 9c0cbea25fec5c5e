"""The host half of the resident servers' mailbox protocol (csrc/evs_mailbox.h: MailboxLayout, MailboxHost) on the CPU, under
AddressSanitizer + UBSan: the header compiled WITHOUT HIP by g++ together with a stand-alone driver with its own main
(tools/mailbox_host_check.cpp) and run as a program of its own.  A second thread plays the device with the header's own layout
constants.  The driver checks, and fails on the first miss:
  * T in {1, 7, 8, 14, 26, 27, 28}: the fake server reads back exactly the ids posted, table t from word t + t / 7, no id in a
    guard word; for T <= 26 the destination from words 29 / 30; by address the id address, stride and destination from words
    0..4 with bit 31 of every guard set; for T in {27, 28} words 29 / 30 are ids;
  * a line with only three of the four guards updated is not accepted (each guard in turn left out);
  * slot order is want % n_slots for n_slots in {1, 4};
  * the sequence number passes 0x7fffffff -> 0 -> 1 with host and fake server agreeing;
  * on_idle is called while nobody is alive and not otherwise; an error from it comes back as the return code with seq reset
    to the number last answered;
  * the stop word makes the fake server leave and clear `alive`."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")


@pytest.mark.skipif(GXX is None, reason="g++ not installed")
def test_mailbox_host_protocol_against_a_fake_server_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "mailbox_host_check")
    cmd = [GXX, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "ev-store-dlrm_amd", "csrc"),
           os.path.join(ROOT, "tools", "mailbox_host_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "mailbox host check ok" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
