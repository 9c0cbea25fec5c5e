"""The descriptor cache behind the lean fused launch (csrc/evs_desc_cache.h) on the host: the key and its equality, the
least-recently-used order, and the pinning of slots a captured graph holds.  The header is plain C++, so the test compiles a
small stand-alone program around it (host compiler, address + undefined-behaviour sanitizers) and runs it: no device."""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ev-store-dlrm_amd", "csrc")

PROGRAM = r"""
#include "evs_desc_cache.h"
#include <stdio.h>
#include <stdlib.h>
using namespace evs;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

static DescKey model(int dev, int d, int T, uintptr_t base, int64_t rows) {
    DescKey k;
    k.dev = dev; k.d = d; k.codec = 32; k.T = T;
    for (int i = 0; i < T; i++) { k.table[i] = (const void *)(base + 4096 * (uintptr_t)i); k.n_rows[i] = rows + i; }
    return k;
}

int main() {
    static_assert(kDescCacheSlots == 8, "the cache holds eight models");
    // ---- the key: every field counts; entries past T do not
    const DescKey a = model(0, 36, 26, 0x10000, 100);
    DescKey b = a;
    CHECK(a == b);
    b.table[27] = (const void *)8; b.n_rows[30] = 5;            // past T: ignored
    CHECK(a == b);
    b = a; b.dev = 1; CHECK(!(a == b));
    b = a; b.d = 32; CHECK(!(a == b));
    b = a; b.codec = 16; CHECK(!(a == b));
    b = a; b.T = 25; CHECK(!(a == b));
    b = a; b.table[25] = (const void *)0x20000; CHECK(!(a == b));
    b = a; b.n_rows[0] += 1; CHECK(!(a == b));                  // the same addresses handed out again, other row counts
    // ---- an empty cache, then eight models fill the eight slots in order
    DescLru lru;
    bool ev = true;
    CHECK(lru.find(a) == -1);
    for (int m = 0; m < 8; m++) {
        const DescKey k = model(0, 16, 8, 0x100000 * (uintptr_t)(m + 1), 10);
        CHECK(lru.find(k) == -1);
        const int s = lru.victim(&ev);
        CHECK(s == m && !ev);
        lru.put(s, k);
        CHECK(lru.find(k) == m);
    }
    // ---- the ninth takes the least recently used: model 0; then model 0 again takes model 1's slot
    const DescKey k0 = model(0, 16, 8, 0x100000, 10), k1 = model(0, 16, 8, 0x200000, 10), k8 = model(0, 16, 8, 0x900000, 10);
    CHECK(lru.find(k8) == -1);
    int s = lru.victim(&ev);
    CHECK(s == 0 && ev);
    lru.drop(s); CHECK(!lru.used(s)); lru.put(s, k8);
    CHECK(lru.find(k0) == -1 && lru.find(k8) == 0);
    s = lru.victim(&ev);
    CHECK(s == 1 && ev);
    lru.put(s, k0);
    CHECK(lru.find(k1) == -1 && lru.find(k0) == 1);
    // ---- a look-up refreshes: after touching model 2 the victim is model 3
    CHECK(lru.find(model(0, 16, 8, 0x300000, 10)) == 2);
    CHECK(lru.victim(&ev) == 3 && ev);
    // ---- pinned slots are never victims; all pinned: no slot
    lru.pin(3);
    CHECK(lru.pinned(3) && lru.victim(&ev) == 4);
    for (int i = 0; i < 8; i++) lru.pin(i);
    CHECK(lru.victim(&ev) == -1 && !ev);
    CHECK(lru.find(k0) == 1);                                    // ... and are still found
    // ---- a dropped slot is free again and loses its pin
    lru.drop(5);
    CHECK(lru.victim(&ev) == 5 && !ev);
    lru.put(5, k1);
    CHECK(!lru.pinned(5) && lru.find(k1) == 5);
    printf("OK\n");
    return 0;
}
"""


def test_descriptor_cache_logic(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src, exe = tmp_path / "desc_cache_test.cpp", tmp_path / "desc_cache_test"
    src.write_text(PROGRAM)
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:   # (a host without the sanitizer runtimes: the same program, plain)
        subprocess.run(base, check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout + r.stderr
