"""Every runtime switch's alternative kernel path under the contract of the default path.

The EVS_* switches are read once per process, so each entry of SWITCHES is one child process: `python -m pytest <node ids>
tests/_switch_seen.py -q -m gpu` under the entry's environment, over EXISTING tests -- bit-exact pooled rows against the oracle,
_accuracy.check against fp64 for R, exact rows plus the residency / no-duplicate / size / histogram invariants and RATE_BAND
for the tiers.  No case and no tolerance is new here; the work is the choice of nodes that reach each dispatch site.  The parent
asserts, per child,

  * return code 0 and passed == selected (an id that no longer exists is a pytest usage error, not a smaller run);
  * every name of `seen` is in the library's record of switches read (evs_env_switches_seen) AS SET: the dispatch site was
    reached with the value in force.  (EVS_DEFER_POOLING is read by the package at import and needs no such proof.)

Children run one after another.  Once a child has ended by signal, abort or timeout, no later child is started: its entry
fails with "not started" and the GPU is left alone.

Nodes left out on purpose (they assert the default's structure, not its result):
  * test_default_result_defers_the_gather_until_it_is_touched and the other deferral tests under EVS_DEFER_POOLING=0.

Timeouts: 3 x the time of the entry's nodes under the default environment + 60 s for the interpreter and the library (the slowest
documented alternative, the dense hash, is 2.3 x its default in kernel time; host time dominates either way).  The default
times are written next to the node lists below (DEFAULT_S).  Wall time on an MI355X: this module 6 min 13 s (59 children of 4 to 9 s
each, most of it the interpreter and the library start).  -s prints a table of worst err/bound and median per switch at the end
(INTEGRATION.md carries it)."""
import os
import re
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, P, C, U, H = ("tests/test_gpu_%s.py::" % m for m in ("accuracy", "parity", "cache", "row_updates", "tiers_host"))
SEEN_NODE = "tests/_switch_seen.py::test_print_the_switches_seen"

# ---- the nodes -------------------------------------------------------------------------------------------------------------------
a_b1, a_off, a_rag = (A + "test_apply_emb_interact_fp32[17-36-%s]" % k for k in ("bag1", "offsets", "ragged"))
a_big, a_bigoff = (A + "test_apply_emb_interact_fp32[16385-36-%s]" % k for k in ("bag1", "offsets"))
a_list = A + "test_multi_hot_list_form[36-26-2100-2-40]"
a_w, a_w64 = A + "test_weighted_bags_itself[32-36]", A + "test_weighted_bags_itself[32-64]"
a_multi = A + "test_apply_emb_interact_multi[3]"
p_gold, p_rag, p_d64 = (P + "test_fused_gather_interact_vs_golden[dlrm_%s]" % k for k in ("kaggle_small", "ragged_small", "d64"))
p_large, p_large64 = P + "test_fused_fp32_large_batch[36-40007]", P + "test_fused_fp32_large_batch[64-16417]"
p_opt, p_opt8 = P + "test_fused_optimistic_offsets_pair[32-4101]", P + "test_fused_optimistic_offsets_pair[8-8269]"
p_tile = P + "test_fused_index_tile_kernel[32-26-5003-36]"
# d = 32 above one resident generation of the rows-in-registers kernel (16 384 samples): the shapes the index-tile loop serves by default
TILED = [A + "test_apply_emb_interact_fp32[16385-32-bag1]", A + "test_apply_emb_interact_fp32[16385-32-offsets]",
         P + "test_fused_fp32_large_batch[32-33000]"]
p_slices = P + "test_fused_offsets_bet_on_batch_slices"
p_multi = P + "test_multi_batch_call_equals_single_launches[3-1000-True-36]"
p_tiny = [P + "test_fused_tiny_batches[%d]" % c for c in (32, 16, 8, 4)]

# default environment, all of them in one process: see DEFAULT_S
FUSED_Q = [A + "test_reduced_precision[36-27-%d]" % c for c in (16, 8, 4)] + [A + "test_reduced_precision[16-9-8]"] + \
          [P + "test_fused_codec_tiers[36-%d]" % c for c in (16, 8, 4)] + \
          [P + "test_fused_codec_26_tables_one_index_per_bag[%d]" % c for c in (8, 4)] + \
          [P + "test_fused_codec_large_batch[8-36-33000]", P + "test_u8_integer_pipe_on_the_extreme_codes", p_opt8] + p_tiny[1:]
DENSE = [A + "test_interact_features_dense[%s]" % k for k in ("27-36", "27-64", "17-16", "2-32")] + \
        [A + "test_interact_features_generic[27-36-True]", A + "test_interact_features_generic[33-36-False]"] + \
        [P + "test_apply_emb_and_interact_vs_golden_and_oracle[dlrm_%s]" % k for k in ("kaggle_small", "d64")]
GATHER = [P + "test_rows_in_registers_gather_vs_oracle[%s]" % k for k in ("36-26-5003", "64-26-3001", "16-32-2049")] + \
         [P + "test_rows_in_registers_gather_reduced_precision_vs_oracle[36-26-5003-%d]" % c for c in (8, 4)] + \
         [P + "test_multi_hot_gather_through_lds_vs_oracle[%s]" % k for k in ("36-26-1003-10", "36-2-64-300", "36-3-200-100")] + \
         [P + "test_edge_cases"] + [P + "test_codec_tiers_bit_exact[36-%d]" % c for c in (16, 8, 4)] + \
         [P + "test_bag_sum_null_offsets_is_the_one_index_row_gather[%s]" % k for k in ("32-36-16389", "8-36-4099")] + \
         [P + "test_sharded_hip_world8_and_rowsplit_virtual_ranks[%s-long]" % k for k in ("8-rows", "2-rowsplit")] + \
         [P + "test_apply_emb_returns_a_real_list_by_default"]
POLICIES = ("sampled", "plan", "setassoc")
TIER1 = [C + "test_batched_cache_invariants_and_hit_rate[0.1-256-%s]" % p for p in POLICIES] + \
        [C + "test_cache_lookup_interact_equals_rows_then_interact[%s]" % p for p in POLICIES] + \
        [C + "test_single_tier_reduced_precision_interaction_consumer[8-36-26-%s]" % p for p in POLICIES] + \
        [C + "test_batched_cache_smaller_than_one_batch[%s]" % p for p in POLICIES] + \
        [C + "test_batched_cache_over_host_memory_backing[sampled]"] + \
        [A + "test_cache_lookup_interact[%s]" % k for k in ("setassoc-32", "sampled-32", "plan-32", "setassoc-8")] + \
        [U + "test_batched_tier[%s]" % k for k in ("plan-None-32", "sampled-None-8", "setassoc-True-32", "setassoc-False-8")]
# the update inside the probe launch: what it asserts is the contract (R over the true rows, flag => resident on arrival, the
# invariants behind every batch), not the launch structure, so it runs under the switches that take the update out of the launch too
TIER1_SA = [n for n in TIER1 if "setassoc" in n] + \
           [C + "test_update_inside_the_probe_launch_of_the_set_associative_tier[%s]" % k for k in ("0.1-512-32", "0.1-512-8")]
TIER1_LIST = [n for n in TIER1 if "sampled" in n]
TIER2 = [C + "test_batched_two_tier_c1c2[23-%s]" % p for p in POLICIES] + \
        [C + "test_two_tier_mixed_codec_interaction_consumer[codecs0-36-26-%s]" % p for p in POLICIES] + \
        [C + "test_batched_three_tier_c1c2c3[codecs0-36-%s]" % p for p in POLICIES] + \
        [A + "test_cache_lookup_interact_c1c2[sampled-codecs0]", A + "test_cache_lookup_interact_c1c2[plan-codecs1]"] + \
        [U + "test_batched_tier_pair_u8_u4[setassoc]", U + "test_batched_tier_pair_u8_u4[sampled]"] + \
        [H + "test_batched_tiers_over_host_and_file_miss_tiers[pinned-40-60-True]",
         H + "test_batched_tiers_over_host_and_file_miss_tiers[file0-40-60-False]",
         H + "test_tier_pairs_over_host_tables_refuse_what_they_cannot_serve"]
UNSET_POLICY = [H + "test_batched_tiers_over_host_and_file_miss_tiers[%s]" % k for k in ("pinned-40-60-False", "pinned-40-60-True", "file0-40-60-False")]
TIER2_SA = [n for n in TIER2 if "setassoc" in n]
TIER2_LIST = [n for n in TIER2 if "sampled" in n or "plan" in n]

# seconds of each node list under the default environment (one process, interpreter and library start included), measured on an
# MI355X; an entry that runs a part of a list takes the list's figure
DEFAULT_S = {"fused": 12.1, "fused_q": 5.8, "dense": 6.2, "gather": 4.9, "tier1": 6.3, "tier2": 6.1}


def _e(name, value, nodes, group, seen=True, tag=None):
    return ("%s=%s" % (name, value) + ("-" + tag if tag else ""), {name: str(value)}, list(nodes), {name} if seen else set(), group)


# (id, env, node ids, seen, timing group)
SWITCHES = [
    # ---- fused fp32 ---------------------------------------------------------------------------------------------------------
    _e("EVS_FUSED_RF", 0, [a_b1, a_off, a_big, p_gold, p_large, p_tiny[0]], "fused"),
    _e("EVS_FUSED_RF_CHECK", 0, [a_off, a_bigoff, p_opt, p_gold], "fused"),
    _e("EVS_FUSED_RF_MAX_B", 64, [a_b1, a_off, a_big, p_large, p_tiny[0]], "fused"),
    _e("EVS_FUSED_RF_MAX_B", 2048, [a_b1, a_big, p_large, p_tile], "fused"),
    _e("EVS_FUSED_RF_MAX_B", -1, [a_b1, a_big, p_large], "fused"),                       # out of range: the default, one warning
    _e("EVS_FUSED_RF_PADLDS", 20480, [a_b1, a_off, a_big, p_gold], "fused"),
    _e("EVS_FUSED_RF_PADLDS", 1000000, [a_b1, a_off, a_big, p_gold], "fused"),           # beyond a block's LDS: refused on the host
    _e("EVS_FUSED_RF_TILE", 4, [a_b1, a_off, a_big, p_gold, p_tiny[0]], "fused"),
    _e("EVS_FUSED_RF_TILE", 8, [a_b1, a_big], "fused"),
    _e("EVS_FUSED_RF_TILE", 12, [a_b1, a_big], "fused"),
    # the PROBE / IDS launches of the tiers keep 16 samples per block under it (a_big, p_large: plain launches, which read the switch)
    _e("EVS_FUSED_RF_TILE", 4, TIER1 + [a_big, p_large], "tier1", tag="tiers"),
    _e("EVS_FUSED_RF_D64", 0, [p_d64, p_large64, a_w64], "fused"),
    _e("EVS_FUSED_TILE", 0, TILED + [p_tile, a_bigoff, p_opt], "fused"),
    _e("EVS_FUSED_TILE_MIN_B", 20000, TILED + [p_tile, p_opt], "fused"),
    _e("EVS_FUSED_TILE_ALIGN", 1, TILED, "fused"),
    # ... and at d = 36, F = 27, where the index-tile loop runs once the rows-in-registers kernel is off
    ("EVS_FUSED_TILE_ALIGN=1-EVS_FUSED_RF=0", {"EVS_FUSED_TILE_ALIGN": "1", "EVS_FUSED_RF": "0"}, [p_tile, a_big, a_bigoff],
     {"EVS_FUSED_TILE_ALIGN", "EVS_FUSED_RF"}, "fused"),
    _e("EVS_FUSED_LDS", 0, [a_rag, a_list, a_w, p_rag], "fused"),
    _e("EVS_FUSED_OPTIMISTIC", 0, [p_opt, p_slices, a_bigoff], "fused"),
    _e("EVS_FUSED_STK", 0, [a_b1, a_list, p_gold, p_tile], "fused"),
    _e("EVS_FUSED_MULTI", 0, [a_multi, p_multi], "fused"),
    # ---- fused, reduced precision (under EVS_FUSED_RFQ=0 the u8 rows no longer take the integer pipe: the tests' i8 terms only
    # loosen the bound, and none asserts that the pipe was taken) ---------------------------------------------------------------
    _e("EVS_FUSED_RFQ", 0, FUSED_Q, "fused_q"),
    _e("EVS_FUSED_RFQ_MAX_B", 64, FUSED_Q, "fused_q"),
    _e("EVS_FUSED_RFQ_MAX_B", -1, FUSED_Q[:4], "fused_q"),                              # out of range
    _e("EVS_FUSED_RFQ_CHECK_MIN_B", 1, FUSED_Q, "fused_q"),
    _e("EVS_FUSED_RFQ_CHECK_MIN_B", 1000000, [p_opt8, FUSED_Q[9]], "fused_q"),
    # ---- dense interaction --------------------------------------------------------------------------------------------------
    _e("EVS_INTERACT_RF", 0, DENSE, "dense"),
    # ---- gather alone -------------------------------------------------------------------------------------------------------
    _e("EVS_GATHER_RF", 0, GATHER, "gather"),
    _e("EVS_GATHER_BLOCKS_PER_CU", 1, GATHER, "gather"),
    _e("EVS_GATHER_BLOCKS_PER_CU", 0, GATHER, "gather"),                             # out of range
    # the flat bag sum takes the bags the long-bag kernel leaves (fewer than 2 indices on average: the two-call side of the fused
    # tests, offsets == arange) -- and every multi-hot shape once the long-bag kernel is off
    _e("EVS_GATHER_FLAT", 0, [p_opt, p_tile, p_slices] + GATHER[5:9], "gather"),
    ("EVS_GATHER_FLAT=0-EVS_GATHER_LONG=0", {"EVS_GATHER_FLAT": "0", "EVS_GATHER_LONG": "0"}, GATHER[5:9] + GATHER[14:16],
     {"EVS_GATHER_FLAT", "EVS_GATHER_LONG"}, "gather"),
    ("EVS_GATHER_FLAT_MAXAVG=4-EVS_GATHER_LONG=0", {"EVS_GATHER_FLAT_MAXAVG": "4", "EVS_GATHER_LONG": "0"}, GATHER[5:9] + GATHER[14:16],
     {"EVS_GATHER_FLAT_MAXAVG", "EVS_GATHER_LONG"}, "gather"),
    _e("EVS_GATHER_LONG", 0, GATHER[5:9] + GATHER[14:16], "gather"),
    _e("EVS_GATHER_LONG_MINAVG", 1000, GATHER[5:9] + GATHER[14:16], "gather"),
    _e("EVS_DEFER_POOLING", 0, GATHER, "gather", seen=False),
    # ---- a single tier ------------------------------------------------------------------------------------------------------
    _e("EVS_CACHE_FOLD", 0, TIER1 + TIER1_SA[-2:], "tier1"),
    _e("EVS_CACHE_FOLDQ", 0, TIER1 + TIER1_SA[-2:], "tier1"),
    _e("EVS_SA_DUAL", 0, TIER1_SA, "tier1"),
    _e("EVS_SA_PAD_MB", 2, TIER1_SA, "tier1"),
    _e("EVS_CACHE_HASH_SCALE", 1, TIER1, "tier1"),
    _e("EVS_CACHE_LIST_WAVES", 1, TIER1_LIST, "tier1"),
    _e("EVS_CACHE_LIST_WAVES", 2, TIER1_LIST, "tier1"),
    _e("EVS_CACHE_LIST_WAVES", 3, TIER1_LIST, "tier1"),
    _e("EVS_CACHE_LIST_WAVES", 4, TIER1_LIST, "tier1"),
    _e("EVS_CACHE_LIST_WAVES", 9, TIER1_LIST, "tier1"),                                  # out of range
    # the tests' own set_batch_policy calls stay: the explicit call wins over the variable, which only a cache that was given
    # no policy reads (the tiers over host and file miss tiers)
    _e("EVS_CACHE_POLICY", "plan", TIER1 + TIER2[:3] + UNSET_POLICY, "tier1"),
    _e("EVS_CACHE_POLICY", "sampled", TIER1 + TIER2[:3] + UNSET_POLICY, "tier1"),
    _e("EVS_CACHE_POLICY", "setassoc", TIER1 + TIER2[:3] + UNSET_POLICY, "tier1"),
    # ---- tier pairs and triples ---------------------------------------------------------------------------------------------
    _e("EVS_CACHE_PAIR", 0, TIER2, "tier2"),
    _e("EVS_CACHE_ROUTEFILTER", 0, TIER2, "tier2"),
    _e("EVS_CACHE_LAZY2", 0, TIER2, "tier2"),
    _e("EVS_CACHE_C3INLINE", 0, TIER2, "tier2"),
    _e("EVS_CACHE_FOLD2", 0, TIER2, "tier2"),
    _e("EVS_CACHE_LIST2", 0, TIER2_LIST, "tier2"),
    _e("EVS_MIXED_RFQ", 0, TIER2, "tier2"),
    _e("EVS_SA_PAIR", 0, TIER2_SA, "tier2"),
    _e("EVS_FILETIER_THREADS", 2, [n for n in TIER2 if "file0" in n], "tier2"),
]

# out-of-range values fall back to the default with ONE warning line (the PADLDS check is made once per kernel)
WARNS = {"EVS_FUSED_RF_MAX_B=-1": (r"EVS_FUSED_RF_MAX_B=-1 is outside", 1), "EVS_FUSED_RFQ_MAX_B=-1": (r"EVS_FUSED_RFQ_MAX_B=-1 is outside", 1),
         "EVS_GATHER_BLOCKS_PER_CU=0": (r"EVS_GATHER_BLOCKS_PER_CU=0 is outside", 1), "EVS_CACHE_LIST_WAVES=9": (r"EVS_CACHE_LIST_WAVES=9 is outside", 1),
         "EVS_FUSED_RF_PADLDS=1000000": (r"EVS_FUSED_RF_PADLDS=1000000 ignored", None)}

_ABNORMAL = (134, 139, 124, 137)
_ended_abnormally = []      # the id of the first child that ended by signal, abort or timeout
_headroom = {}              # entry id -> {kernel: (worst err / bound, median, checks)}


def run_child(env, nodes, timeout):
    """-> (return code or None on timeout, output, seconds)"""
    full = dict(os.environ, **env)
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, "-m", "pytest"] + list(nodes) + [SEEN_NODE, "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"],
                           env=full, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode("utf-8", "replace")
        return None, out, time.time() - t0
    return p.returncode, p.stdout + p.stderr, time.time() - t0


def judge(out, n_selected, seen):
    """what the parent asserts of a child that ended normally -> list of complaints"""
    bad = []
    m = re.search(r"(\d+) passed", out)
    passed = int(m.group(1)) if m else 0
    if passed != n_selected or re.search(r"\d+ (failed|error|errors|skipped|deselected|xfailed|xpassed)\b", out):
        bad.append("passed %d of %d selected" % (passed, n_selected))
    record = dict(re.findall(r"^SWITCH_SEEN (\w+)=(\d)$", out, re.M))
    for name in sorted(seen):
        if record.get(name) != "1":
            bad.append("%s is not in the record of switches read as set (%s): its dispatch site was not reached" %
                       (name, "read as unset" if name in record else "never read"))
    return bad


@pytest.fixture(scope="module", autouse=True)
def headroom_per_switch():
    yield
    print("\n| switch | kernel | worst err/bound | median | checks |\n|---|---|---|---|---|")
    for ident, st in _headroom.items():
        for k, (w, m, n) in sorted(st.items()):
            print("| %s | %s | %.3f | %.3f | %d |" % (ident, k, w, m, n))


@pytest.mark.parametrize("ident,env,nodes,seen,group", SWITCHES, ids=[s[0] for s in SWITCHES])
def test_contract_under_switch(ident, env, nodes, seen, group):
    if _ended_abnormally:
        pytest.fail("not started: %s ended abnormally" % _ended_abnormally[0], pytrace=False)
    rc, out, dt = run_child(env, nodes, timeout=3 * DEFAULT_S[group] + 60)
    print("\n%s: %d nodes, %.1f s, rc %s" % (ident, len(nodes) + 1, dt, rc))
    if rc is None or rc in _ABNORMAL or rc < 0:
        _ended_abnormally.append(ident)
        pytest.fail("%s ended abnormally (%s)\n%s" % (ident, "timeout" if rc is None else "rc %d" % rc, out[-4000:]), pytrace=False)
    bad = judge(out, len(nodes) + 1, seen)
    if ident in WARNS:
        pat, count = WARNS[ident]
        n = len(re.findall(pat, out))
        if n == 0 or (count is not None and n != count):
            bad.append("%d warning lines /%s/" % (n, pat))
    assert rc == 0 and not bad, "%s: rc %d %s\n%s" % (ident, rc, "; ".join(bad), out[-4000:])
    _headroom[ident] = {k: (float(w), float(m), int(n)) for k, w, m, n in re.findall(r"^HEADROOM\t(.*)\t(.*)\t(.*)\t(\d+)$", out, re.M)}


if __name__ == "__main__":      # python tests/test_gpu_switches.py: the node lists under the default environment, timed
    for g, nodes in (("fused", sorted({n for s in SWITCHES if s[4] == "fused" for n in s[2]})), ("fused_q", FUSED_Q), ("dense", DENSE),
                     ("gather", GATHER), ("tier1", TIER1 + TIER1_SA[-2:]), ("tier2", TIER2)):
        rc, out, dt = run_child({}, nodes, timeout=900)
        print("DEFAULT %-8s %3d nodes %6.1f s rc %s %s" % (g, len(nodes) + 1, dt, rc, judge(out, len(nodes) + 1, ())), flush=True)
        for k, w, m, n in re.findall(r"^HEADROOM\t(.*)\t(.*)\t(.*)\t(\d+)$", out, re.M):
            print("| default | %s | %.3f | %.3f | %s |" % (k, float(w), float(m), n))
        if rc != 0:
            print(out[-3000:])
            sys.exit(1)
