"""CPU: the names of the EVS_* switches cannot drift.  Three lists are held to each other --

  code      every EVS_* literal the library (csrc/*.hip, *.h, *.cpp: getenv / env_switch / env_switch_on / env_switch_range), the package's
            *.py and bench.py (os.environ, os.getenv) read, plus the EVS_* build flags the README documents (#if / #ifndef in csrc/)
  README    the first column of the "Environment switches" table
  SWITCHES  the entries of tests/test_gpu_switches.py (one child process per switch setting), or EXEMPT below with a reason

-- the library's record of the switches it has read (evs_env_switches_seen) and the range check of the numeric switches are
exercised through the manager and the file tier, which need no GPU, and so is EVS_REQUIRE_EXT."""
import glob
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "ev-store-dlrm_amd")
NAME = r"EVS_[A-Z0-9_]+"


def _csrc_files():
    return sorted(f for pat in ("*.hip", "*.h", "*.cpp") for f in glob.glob(os.path.join(PKG, "csrc", pat)))


def names_read_by_the_code():
    names = set()
    for f in _csrc_files():
        names |= set(re.findall(r'(?:getenv|env_switch|env_switch_on|env_switch_range)\(\s*"(%s)"' % NAME, open(f).read()))
    py = [os.path.join(dp, f) for dp, _, fs in os.walk(PKG) for f in fs if f.endswith(".py")] + [os.path.join(ROOT, "bench.py")]
    for f in py:
        text = open(f).read()
        names |= set(re.findall(r'\benviron(?:\.get|\.pop|\.setdefault)?\s*[\(\[]\s*["\'](%s)["\']' % NAME, text))    # os.environ, _os.environ
        names |= set(re.findall(r'\bgetenv\(\s*["\'](%s)["\']' % NAME, text))
        names |= set(re.findall(r'["\'](%s)["\']\s+(?:not\s+)?in\s+\w*\.?environ\b' % NAME, text))
    return names


# Names that no entry of SWITCHES sets, each with its reason.  Of the names no test used to set, only EVS_P2P_SPINS and
# EVS_REQUIRE_EXT may stand here.
EXEMPT = {
    "EVS_SA_WAYS": "covered: test_gpu_row_updates.py::test_batched_set_associative_tier_with_16_ways (a child of its own)",
    "EVS_CACHE_INLINE": "covered: test_gpu_cache.py and test_gpu_fullsize.py pin both values",
    "EVS_SERVE_PUBLISH": "covered: test_gpu_serve.py",
    "EVS_NO_EXT": "covered: test_gpu_parity.py (the ctypes call path in a child)",
    "EVS_LAZY_POOLING": "covered: test_gpu_parity.py",
    "EVS_DEFER_POISON": "covered: test_gpu_parity.py::test_this_file_is_green_under_the_poisoned_deferred_default",
    "EVS_MANAGER_SERVE": "covered: test_gpu_tier_server.py",
    "EVS_BACKING": "covered: test_ev_lookup_host.py and the ev_lookup children",
    "EVS_LIB_PATH": "covered: test_gpu_parity.py; it selects a library file, not a kernel path",
    "EVS_BENCH_P2P": "needs two ranks; its set-up failure path is covered by test_p2p_exchange.py",
    "EVS_BENCH_MASTER_PORT": "the rendezvous port of bench.py's ranks: no kernel path",
    "EVS_P2P_SPINS": "needs two ranks and a timeout path",
    "EVS_P2P_INJECT_FAIL": "test-only hook of test_p2p_exchange.py",
    "EVS_DIRECT_A2A": "needs more than one rank (the sharded op's exchange)",
    "EVS_DIRECT_A2A_V": "needs more than one rank; the world-1 child of test_gpu_nccl sets it",
    "EVS_REQUIRE_EXT": "no GPU needed: test_require_ext_turns_a_failed_extension_build_into_an_error below",
    # the manager's configuration, the environment form of the reference's #defines (the ev_lookup children set them)
    "EVS_N_CACHING_LAYER": "manager #define equivalent", "EVS_MAIN_PRECISION": "manager #define equivalent",
    "EVS_SECONDARY_PRECISION": "manager #define equivalent", "EVS_TOTAL_SIZE": "manager #define equivalent",
    "EVS_SIZE_PROPORTION": "manager #define equivalent", "EVS_EV_TABLE_ROOT": "manager #define equivalent",
    "EVS_ALTKEY_DIR": "manager #define equivalent",
    # build flags: a variant library each, and EVS_LIB_PATH turns the extension off
    "EVS_RFQ_FOLD": "build flag: needs a variant library", "EVS_MIXED_FOLD": "build flag: needs a variant library",
    "EVS_MIXED_LB_PROBE": "build flag: needs a variant library",
}
NEVER_SET_BEFORE = """EVS_FUSED_RF EVS_FUSED_RF_CHECK EVS_FUSED_RF_MAX_B EVS_FUSED_RF_PADLDS EVS_FUSED_RFQ EVS_FUSED_RFQ_MAX_B
    EVS_FUSED_RFQ_CHECK_MIN_B EVS_FUSED_TILE EVS_FUSED_TILE_MIN_B EVS_FUSED_TILE_ALIGN EVS_FUSED_LDS EVS_FUSED_OPTIMISTIC EVS_FUSED_MULTI
    EVS_INTERACT_RF EVS_GATHER_RF EVS_GATHER_FLAT EVS_GATHER_FLAT_MAXAVG EVS_GATHER_LONG EVS_GATHER_LONG_MINAVG EVS_GATHER_BLOCKS_PER_CU
    EVS_MIXED_RFQ EVS_SA_DUAL EVS_SA_PAIR EVS_CACHE_FOLD EVS_CACHE_FOLDQ EVS_CACHE_FOLD2 EVS_CACHE_PAIR EVS_CACHE_ROUTEFILTER
    EVS_CACHE_LAZY2 EVS_CACHE_C3INLINE EVS_CACHE_LIST2 EVS_CACHE_LIST_WAVES EVS_CACHE_HASH_SCALE EVS_CACHE_POLICY
    EVS_DEFER_POOLING EVS_REQUIRE_EXT EVS_P2P_SPINS""".split()


def switches_table():
    import test_gpu_switches
    return test_gpu_switches.SWITCHES


def readme_table():
    """-> (environment names, build-flag names) of the first column of the switch table"""
    text = open(os.path.join(ROOT, "README.md")).read()
    start = text.index("Environment switches")
    env, flags = set(), set()
    for line in text[start:].splitlines():
        if not line.startswith("|"):
            continue
        first = line.split("|")[1]
        for dash, name in re.findall(r"(-D)?(%s)" % NAME, first):
            (flags if dash else env).add(name)
    return env, flags


def build_flags_in_the_code():
    src = "\n".join(open(f).read() for f in _csrc_files())
    return set(re.findall(r"#\s*if(?:n?def)?\s+!?\s*(?:defined\s*\(\s*)?(%s)" % NAME, src))


def test_the_scan_finds_the_switches():
    code = names_read_by_the_code()
    assert {"EVS_FUSED_RF", "EVS_CACHE_FOLD", "EVS_GATHER_RF", "EVS_DEFER_POOLING", "EVS_LIB_PATH", "EVS_BENCH_P2P"} <= code and len(code) >= 60
    env, flags = readme_table()
    assert "EVS_FUSED_RF" in env and flags == {"EVS_RFQ_FOLD", "EVS_MIXED_FOLD", "EVS_MIXED_LB_PROBE"}


def test_no_read_of_the_environment_bypasses_the_record():
    """every EVS_* read of the library goes through evs::env_switch (csrc/evs_api.hip holds the one getenv)"""
    for f in _csrc_files():
        for n, line in enumerate(open(f), 1):
            if re.search(r"(?<!\w)getenv\(", line):
                assert f.endswith("evs_api.hip") and "getenv(name)" in line, (f, n, line)


def test_every_switch_the_code_reads_is_in_the_readme_table():
    env, flags = readme_table()
    assert sorted(names_read_by_the_code() - env) == []
    assert sorted(flags - build_flags_in_the_code()) == []


def test_every_readme_switch_is_read_somewhere():
    env, _ = readme_table()
    assert sorted(env - names_read_by_the_code()) == []


def test_every_switch_is_exercised_or_exempt_with_a_reason():
    env, flags = readme_table()
    exercised = {name for _, e, _, _, _ in switches_table() for name in e}
    every = names_read_by_the_code() | env | flags
    assert sorted(every - exercised - set(EXEMPT)) == [], "neither an entry of SWITCHES nor in EXEMPT"
    assert sorted(set(EXEMPT) - every) == [] and sorted(exercised - every) == [], "a name nothing reads"
    assert sorted(set(EXEMPT) & exercised) == []
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in EXEMPT.values())
    assert sorted(set(EXEMPT) & set(NEVER_SET_BEFORE)) == ["EVS_P2P_SPINS", "EVS_REQUIRE_EXT"]


def test_the_switches_table_is_well_formed():
    """ids are unique, every node id names a test function that exists in its file, a switch that the library reads is proved
    by the record (seen), and every entry's environment sets what its id says"""
    table = switches_table()
    assert len({s[0] for s in table}) == len(table)
    python_side = {"EVS_DEFER_POOLING"}
    for ident, e, nodes, seen, group in table:
        assert nodes and len(set(nodes)) == len(nodes), ident
        assert seen == set(e) - python_side, ident
        for n in nodes:
            path, func = n.split("::")
            assert re.search(r"^def %s\(" % re.escape(func.split("[")[0]), open(os.path.join(ROOT, path)).read(), re.M), n


_RECORD_CHILD = """
import ctypes, sys
import evstore_dlrm_amd as E
L = E._lib.lib()
assert E._lib.env_switches_seen() == {}, "nothing has been read yet"
h = ctypes.c_void_p()
paths = (ctypes.c_char_p * 1)(sys.argv[1].encode())               # an empty table file, nothing pinned: no GPU call
assert L.evs_filetier_open(ctypes.byref(h), 1, paths, 4, 0) == 0  # reads EVS_FILETIER_THREADS
L.evs_filetier_close(h)
first = E._lib.env_switches_seen()
L.ev_lookup.restype, L.ev_lookup.argtypes = ctypes.c_void_p, [ctypes.POINTER(ctypes.c_int)]
arr = (ctypes.c_int * 26)()
assert L.ev_lookup(arr) is None                                   # the manager reads its configuration, then refuses: no table root
rec = E._lib.env_switches_seen()
print("FIRST", sorted(first.items()))
print("ORDER", list(rec))
print("REC", sorted(rec.items()))
n = L.evs_env_switches_seen(None, 0)
buf = ctypes.create_string_buffer(n + 1)
assert L.evs_env_switches_seen(buf, n + 1) == n and len(buf.value) == n
print("LINES", buf.value.decode().count(chr(10)), len(rec))
short = ctypes.create_string_buffer(8)
assert L.evs_env_switches_seen(short, 8) == n and len(short.value) <= 7
assert L.ev_lookup(arr) is None
assert list(E._lib.env_switches_seen()) == list(rec), "a second read of a name adds no line"
"""


def test_the_library_records_the_switches_it_reads(tmp_path):
    """In a fresh process, without a GPU: the file tier reads EVS_FILETIER_THREADS (set here), the manager reads its
    configuration (EVS_N_CACHING_LAYER set, EVS_EV_TABLE_ROOT unset).  The record holds each name once, in the order of the
    first read, with whether it was set."""
    import subprocess
    import sys
    env = dict(os.environ, EVS_FILETIER_THREADS="3", EVS_N_CACHING_LAYER="2")
    for k in ("EVS_EV_TABLE_ROOT", "EVS_MAIN_PRECISION"):
        env.pop(k, None)
    (tmp_path / "t0.bin").write_bytes(b"")
    p = subprocess.run([sys.executable, "-c", _RECORD_CHILD, str(tmp_path / "t0.bin")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    out = dict(ln.split(" ", 1) for ln in p.stdout.splitlines() if ln.split(" ", 1)[0] in ("FIRST", "ORDER", "REC", "LINES"))
    assert eval(out["FIRST"]) == [("EVS_FILETIER_THREADS", True)]
    order, rec = eval(out["ORDER"]), dict(eval(out["REC"]))
    assert order[0] == "EVS_FILETIER_THREADS" and len(order) == len(set(order))
    assert order.index("EVS_N_CACHING_LAYER") < order.index("EVS_EV_TABLE_ROOT")
    assert rec["EVS_FILETIER_THREADS"] is True and rec["EVS_N_CACHING_LAYER"] is True
    assert rec["EVS_EV_TABLE_ROOT"] is False and rec["EVS_MAIN_PRECISION"] is False
    assert out["LINES"] == "%d %d" % (len(rec), len(rec))


def test_require_ext_turns_a_failed_extension_build_into_an_error(monkeypatch, tmp_path):
    """EVS_REQUIRE_EXT=1: a failed build of the C++ extension raises; without it the failure is a warning and the ctypes path
    stays (the extension's output path points into tmp_path here, so the real one is not touched)."""
    import evstore_dlrm_amd as E
    from evstore_dlrm_amd import _ext_build
    _lib = E._lib
    if not os.path.exists(_lib.LIB_PATH):
        E.build()
    monkeypatch.setattr(_lib.subprocess, "check_call", lambda *a, **k: 0)      # (the library is built: no make here)
    monkeypatch.setattr(_ext_build, "OUT", str(tmp_path / "_evs_torch_ext.so"))

    def fail(**kw):
        raise RuntimeError("forced extension build failure")
    monkeypatch.setattr(_ext_build, "build", fail)
    monkeypatch.setenv("EVS_REQUIRE_EXT", "1")
    with pytest.raises(RuntimeError, match="forced extension build failure"):
        _lib.build()
    monkeypatch.delenv("EVS_REQUIRE_EXT")
    with pytest.warns(UserWarning, match="ctypes call path"):
        _lib.build()
