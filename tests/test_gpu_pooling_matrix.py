"""Pooling alone: every gather kernel instantiation that bag_sum_impl (csrc/evs_gather.hip) can launch, against the oracle's bits.

bag_sum_impl picks one of five kernel families from (codec, d, T, bag form, weights, alignment); each is a template with many
instantiations.  Every case here is ONE call straight through the C ABI (evs_embedding_bag_sum_sharded / _p2p: eager, default
stream) under two assertions (tests/_pooling_matrix.py:check_case):

  * the dispatch record (evs_gather_kernels_seen) taken before and after the call: exactly the intended name went up, by the intended
    number of launches -- so the case ran the kernel it is about, and a change of the dispatch that routes it elsewhere fails here;
  * the whole output buffer, as uint32, equals the oracle's pooled rows laid out like the call's output (index order, unfused fp32
    multiply and add; entries of another shard's rows removed and offsets rebuilt for row ranges; the peer-major / peer_delta layout
    rebuilt in numpy), and still holds a sentinel wherever the call has nothing to write.  There is no tolerance in this file.

Tables have 1, 3, 40 and 700 rows; reduced-precision tables come from orc.encode_table with a few u16 tail codes patched in.

The forms the default environment cannot reach run in one child process (tests/_pooling_matrix_env_child.py, EVS_GATHER_LONG=0
EVS_GATHER_RF=0) under the same two assertions.  The closing test reads the whole record: a name this module left at 0 must be in
CHILD_ONLY, and the child proves those.

Cases beyond the planned list, which the closing test asked for: the record does not tell a weighted launch from an unweighted one, so
the grid-stride kernels that unweighted batches never reach by default -- fp32 at d = 16, 32, 64 in both forms, and the one-index form
of every codec at d = 16 and 32 -- ARE reachable, through weights.  test_vec_weighted_other_compiled_dims runs them here instead of
listing them in CHILD_ONLY, which holds the tile kernel's select form alone.

Wall time on an MI355X: this module 5.5 s for 282 cases (about 800 pooling calls of at most a few hundred bags each), of which the child 2.1 s,
most of it the interpreter and the library start."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _pooling_matrix as PM
from _pooling_matrix import check_case, flat_name, long_name, rows_name, scalar_name, vec_name

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODECS = (32, 16, 8, 4)

# Names the default environment cannot launch; each entry: the line of bag_sum_impl that keeps it out of reach.
CHILD_ONLY = [
    # `if (codec == 32 && !bag1 && launch_bag_sum_long(a, vec_ok, st)) { ...; continue; }` stands in front of the launch_bag_sum_flat line and
    # takes every average >= 2 at d = 16; the select form needs an average above 16
    "flat_c32_lpr4_select",
    # the same line, d = 32
    "flat_c32_lpr8_select",
    # the same line, d = 36
    "flat_c32_lpr9_select",
    # the same line, d = 64
    "flat_c32_lpr16_select",
]


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    assert not [k for k in os.environ if k.startswith("EVS_GATHER_")], "this module pins the DEFAULT dispatch: unset the EVS_GATHER_* switches"
    return E


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module", autouse=True)
def record_at_start(E):
    """the record before this module's first case: the closing test counts this module's launches only"""
    return dict(E._lib.gather_kernels_seen())


def _rs(*key):
    return np.random.RandomState(sum(int(v) * 7919 ** i for i, v in enumerate(key)) % (2 ** 31))


def _short_lens(rs, T, B):
    """bag lengths 0..3 with a mean of 1.1: below what the long-bag kernel takes"""
    return rs.choice(4, size=(T, B), p=[0.3, 0.4, 0.2, 0.1])


def _vec_B(d):
    """four full wave items of the grid-stride kernel's unroll slots and a partial one"""
    return 4 * (64 // (d // 4)) + 3


# ------------------------------------------------------------------------------------------------------------------------------ rows
ROWS_PAIRS = [(16, 16), (16, 17), (32, 8), (32, 9), (32, 16), (32, 17), (32, 24), (32, 25), (36, 7), (36, 8), (36, 14), (36, 15), (36, 21),
              (36, 22), (36, 28), (64, 8), (64, 9), (64, 16), (64, 17), (64, 28)]


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("d,T", ROWS_PAIRS)
def test_rows_every_instruction_count(E, orc, d, T, codec):
    """gather_rows_kernel<CODEC, LPRD, NJ, CHECK> on both sides of every NJ boundary of every d: offsets = arange (checked per block) and
    one index per bag declared; B = 53 = three full blocks of 16 samples and a partial one."""
    B = 53
    rs = _rs(1, d, T, codec)
    tabs = PM.make_tables(orc, rs, T, d, codec)
    idx = PM.one_index_bags(rs, tabs, B)
    off = [np.arange(B, dtype=np.int64) for _ in range(T)]
    check_case(E, orc, {rows_name(codec, d, T, False): 1}, B, d, codec, tabs, idx, off)
    check_case(E, orc, {rows_name(codec, d, T, True): 1}, B, d, codec, tabs, idx, None)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("d,T", [(16, 17), (32, 9), (36, 15), (64, 9)])
def test_rows_ragged_block_tile_and_sharded_layouts(E, orc, d, T, codec):
    """Once per d and codec: a block that finds ragged bags (nnz = B: a two-index bag next to an empty one, in block 1 of table 1 only)
    pools the general way while the other blocks keep the fast path; the (B, F, d) tile as `out` takes the sample-major store mapping;
    a row range with row_lo > 0; the peer-major layout with 20 bags per peer (B = 53: the last peer is short), plain and through
    peer_delta."""
    B = 53
    rs = _rs(2, d, T, codec)
    tabs = PM.make_tables(orc, rs, T, d, codec)
    idx = PM.one_index_bags(rs, tabs, B)
    off = [np.arange(B, dtype=np.int64) for _ in range(T)]
    check, declared = {rows_name(codec, d, T, False): 1}, {rows_name(codec, d, T, True): 1}
    ragged = [o.copy() for o in off]
    ragged[1][20] = 21                                     # bag 19 = [19, 21), bag 20 = [21, 21)
    plain = check_case(E, orc, check, B, d, codec, tabs, idx, off)
    got = check_case(E, orc, check, B, d, codec, tabs, idx, ragged)
    assert not np.array_equal(got, plain)
    check_case(E, orc, check, B, d, codec, tabs, idx, off, layout="tile")
    check_case(E, orc, declared, B, d, codec, tabs, idx, None, layout="tile")
    rg = PM.mid_ranges(tabs)
    assert all(lo > 0 for (lo, _), t in zip(rg, tabs) if t.shape[0] > 1)
    check_case(E, orc, check, B, d, codec, tabs, idx, off, ranges=rg)
    check_case(E, orc, declared, B, d, codec, tabs, idx, None, layout="peer", bpp=20)
    check_case(E, orc, check, B, d, codec, tabs, idx, off, ranges=rg, layout="peer", bpp=20, delta=True)


# ------------------------------------------------------------------------------------------------------------------------------ long
def _long_case(rs, orc, d, T):
    """B = 2 G + 1 bags (G = bags per wave); per table one bag of 150; table 1's first wave item all empty; the other bags cycle through
    0, 1, K - 1, K, K + 1, 2 K, 2 K + 1, 3 K + 5"""
    K, G = PM.LONG_K[d], 64 // (d // 4)
    B = 2 * G + 1
    cycle = [0, 1, K - 1, K, K + 1, 2 * K, 2 * K + 1, 3 * K + 5]
    lens = -np.ones((T, B), np.int64)
    for k in range(T):
        lens[k, 2 * G if k % 2 else 0] = 150
    lens[1, :G] = 0
    free = np.argwhere(lens < 0)
    for i, (k, b) in enumerate(free):
        lens[k, b] = cycle[i % 8]
    assert set(cycle) | {150} <= set(lens.reshape(-1).tolist()) and len(free) >= 8 and (lens == 150).sum(axis=1).all()
    assert not lens[1, :G].any()
    for k0 in range(0, T, 32):   # every launch of the call: the average the long-bag kernel asks for
        assert lens[k0:k0 + 32].sum() >= 2 * B * lens[k0:k0 + 32].shape[0]
    tabs = PM.make_tables(orc, rs, T, d, 32)
    idx, off = PM.make_bags(rs, tabs, lens)
    return B, G, tabs, idx, off


@pytest.mark.parametrize("T", [3, 33])
@pytest.mark.parametrize("d", [16, 32, 36, 64, 128])
def test_long_bags(E, orc, d, T):
    """bag_sum_long_kernel<LPR, K>, d = 128 (K < LPR, two bags per wave, index lanes 16..31 idle) included: bag lengths around every multiple
    of K, a bag of 150, a wave item of empty bags; T = 33 is two launches, the second with one table."""
    B, G, tabs, idx, off = _long_case(_rs(3, d, T), orc, d, T)
    check_case(E, orc, {long_name(d): 1 if T <= 32 else 2}, B, d, 32, tabs, idx, off)


@pytest.mark.parametrize("d", [16, 32, 36, 64, 128])
def test_long_bags_sharded_layouts(E, orc, d):
    B, G, tabs, idx, off = _long_case(_rs(4, d), orc, d, 3)
    want = {long_name(d): 1}
    check_case(E, orc, want, B, d, 32, tabs, idx, off, ranges=PM.mid_ranges(tabs))
    check_case(E, orc, want, B, d, 32, tabs, idx, off, layout="peer", bpp=G + 1)
    check_case(E, orc, want, B, d, 32, tabs, idx, off, ranges=PM.mid_ranges(tabs), layout="peer", bpp=G + 1, delta=True)


# ------------------------------------------------------------------------------------------------------------------------------ flat
@pytest.mark.parametrize("d", [16, 32, 36, 64])
def test_flat_plain_form(E, orc, d):
    """bag_sum_flat_kernel<LPRD, false>: bags of 0..3 with a mean below 2 and nnz != B (neither the rows nor the long-bag kernel takes
    them), B = 137 = two chunks of 64 bags and a partial one; a row range and the peer-major layout."""
    T, B = 3, 137
    rs = _rs(5, d)
    tabs = PM.make_tables(orc, rs, T, d, 32)
    lens = _short_lens(rs, T, B)
    assert lens.sum() < 2 * B * T and any(lens[k].sum() != B for k in range(T))
    idx, off = PM.make_bags(rs, tabs, lens)
    want = {flat_name(d, False): 1}
    check_case(E, orc, want, B, d, 32, tabs, idx, off)
    check_case(E, orc, want, B, d, 32, tabs, idx, off, ranges=PM.mid_ranges(tabs))
    check_case(E, orc, want, B, d, 32, tabs, idx, off, layout="peer", bpp=50)
    check_case(E, orc, want, B, d, 32, tabs, idx, off, ranges=PM.mid_ranges(tabs), layout="peer", bpp=50, delta=True)


# ------------------------------------------------------------------------------------------------------------------------------- vec
@pytest.mark.parametrize("codec", [16, 8, 4])
@pytest.mark.parametrize("d", [16, 32, 36, 64])
def test_vec_compiled_lanes_offsets_form(E, orc, d, codec):
    """embedding_bag_sum_kernel<CODEC, LPR, 4, false>: multi-hot bags of 0..5 over reduced-precision tables"""
    T, B = 3, _vec_B(d)
    rs = _rs(6, d, codec)
    tabs = PM.make_tables(orc, rs, T, d, codec)
    idx, off = PM.make_bags(rs, tabs, rs.randint(0, 6, size=(T, B)))
    check_case(E, orc, {vec_name(codec, d, False): 1}, B, d, codec, tabs, idx, off)


@pytest.mark.parametrize("codec", CODECS)
def test_vec_d128_offsets_form(E, orc, codec):
    """d = 128 with a mean bag length below 2: unweighted fp32 included, which neither the long-bag nor the tile kernel takes"""
    T, d = 3, 128
    B = _vec_B(d)
    rs = _rs(7, codec)
    tabs = PM.make_tables(orc, rs, T, d, codec)
    lens = _short_lens(rs, T, B)
    assert lens.sum() < 2 * B * T
    idx, off = PM.make_bags(rs, tabs, lens)
    check_case(E, orc, {vec_name(codec, d, False): 1}, B, d, codec, tabs, idx, off)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("d,T", [(36, 29), (36, 30), (36, 31), (36, 32), (64, 29), (64, 30), (64, 31), (64, 32), (128, 3)])
def test_vec_compiled_lanes_bag1_form(E, orc, d, T, codec):
    """embedding_bag_sum_kernel<CODEC, LPR, 4, true>: one-index bags declared where launch_gather_rows turns the launch away (d = 36 and
    d = 64 with T = 29..32), and d = 128"""
    B = 53
    rs = _rs(8, d, T, codec)
    tabs = PM.make_tables(orc, rs, T, d, codec)
    idx = PM.one_index_bags(rs, tabs, B)
    check_case(E, orc, {vec_name(codec, d, True): 1}, B, d, codec, tabs, idx, None)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("d", [8, 20, 24, 40, 48, 100, 136, 256])
def test_vec_run_time_lanes(E, orc, d, big, codec):
    """embedding_bag_sum_kernel<CODEC, 0, 4, *>: lanes per row read at run time -- d whose d / 4 does not divide 64 (the top lanes of a wave
    are off), d = 256 (one row per wave), multi-hot bags of 0..5 and one-index bags; B = 1 and four full wave items plus three bags."""
    T, B = 3, (_vec_B(d) if big else 1)
    rs = _rs(9, d, big, codec)
    tabs = PM.make_tables(orc, rs, T, d, codec)
    lens = rs.randint(0, 6, size=(T, B))
    if B == 1:
        lens[:, 0] = [5, 0, 3]
    idx, off = PM.make_bags(rs, tabs, lens)
    check_case(E, orc, {vec_name(codec, d, False): 1}, B, d, codec, tabs, idx, off)
    check_case(E, orc, {vec_name(codec, d, True): 1}, B, d, codec, tabs, PM.one_index_bags(rs, tabs, B), None)


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("d", [36, 20])
def test_vec_weighted(E, orc, d, codec):
    """Per-row weights (one weighted table sends the whole launch to the grid-stride kernel): reduced-precision rows, weights for some tables
    of the list only, one-index bags declared, T = 40 with a weighted table in the second launch (row_weights[k0 + k]), a row range (the
    weights of the local rows), the peer-major layout."""
    B = _vec_B(d)
    rs = _rs(10, d, codec)
    tabs = PM.make_tables(orc, rs, 3, d, codec)
    idx, off = PM.make_bags(rs, tabs, rs.randint(0, 6, size=(3, B)))
    offs, bag1 = {vec_name(codec, d, False): 1}, {vec_name(codec, d, True): 1}
    w = PM.make_weights(rs, tabs, {0, 2})
    check_case(E, orc, offs, B, d, codec, tabs, idx, off, weights=w)
    check_case(E, orc, bag1, B, d, codec, tabs, PM.one_index_bags(rs, tabs, B), None, weights=PM.make_weights(rs, tabs, {1}))
    w3 = PM.make_weights(rs, tabs, {0, 1, 2})
    check_case(E, orc, offs, B, d, codec, tabs, idx, off, weights=w3, ranges=PM.mid_ranges(tabs))
    check_case(E, orc, offs, B, d, codec, tabs, idx, off, weights=w, layout="peer", bpp=20)
    check_case(E, orc, bag1, B, d, codec, tabs, PM.one_index_bags(rs, tabs, B), None, weights=w3, ranges=PM.mid_ranges(tabs), layout="peer",
               bpp=20, delta=True)
    tabs40 = PM.make_tables(orc, rs, 40, d, codec)
    idx40, off40 = PM.make_bags(rs, tabs40, rs.randint(0, 6, size=(40, B)))
    check_case(E, orc, {vec_name(codec, d, False): 2}, B, d, codec, tabs40, idx40, off40, weights=PM.make_weights(rs, tabs40, {2, 35}))


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("d", [16, 32, 64])
def test_vec_weighted_other_compiled_dims(E, orc, d, codec):
    """The grid-stride kernels of the other compiled widths that only a weighted batch reaches by default (see the module docstring):
    fp32 in both forms, and the one-index form of every codec at d = 16 and d = 32, where the rows kernel takes every T <= 32."""
    B = _vec_B(d)
    rs = _rs(11, d, codec)
    tabs = PM.make_tables(orc, rs, 3, d, codec)
    idx, off = PM.make_bags(rs, tabs, rs.randint(0, 6, size=(3, B)))
    w = PM.make_weights(rs, tabs, {0})
    check_case(E, orc, {vec_name(codec, d, False): 1}, B, d, codec, tabs, idx, off, weights=w)
    check_case(E, orc, {vec_name(codec, d, True): 1}, B, d, codec, tabs, PM.one_index_bags(rs, tabs, B), None, weights=w)


# ---------------------------------------------------------------------------------------------------------------------------- scalar
SCALAR = [(d, c) for d in (2, 10, 66, 258) for c in CODECS] + [(7, c) for c in (32, 16, 8)] + [(260, 32), (260, 8)]


@pytest.mark.parametrize("d,codec", SCALAR)
def test_scalar_kernel(E, orc, d, codec):
    """embedding_bag_sum_scalar_kernel<CODEC>: the reduced codecs (the nibble order of the u4 decode), d > 64 (a second trip of the column
    loop), d > 256 -- d = 260 is a multiple of 4 the grid-stride kernel does not take; offsets and one-index forms, weighted and not, a
    row range, the peer-major layout."""
    T = 3
    rs = _rs(12, d, codec)
    tabs = PM.make_tables(orc, rs, T, d, codec)
    want = {scalar_name(codec): 1}
    w = PM.make_weights(rs, tabs, {0, 2})
    for B in (5, 70):
        idx, off = PM.make_bags(rs, tabs, rs.randint(0, 4, size=(T, B)))
        idx1 = PM.one_index_bags(rs, tabs, B)
        for ww in (None, w):
            check_case(E, orc, want, B, d, codec, tabs, idx, off, weights=ww)
            check_case(E, orc, want, B, d, codec, tabs, idx1, None, weights=ww)
    check_case(E, orc, want, B, d, codec, tabs, idx, off, weights=w, ranges=PM.mid_ranges(tabs))
    check_case(E, orc, want, B, d, codec, tabs, idx1, None, layout="peer", bpp=20)


# ---------------------------------------------------------------------------------------------------------------------------- guards
GUARDS = [("long", 128, 32)] + [("vec", 20, c) for c in CODECS] + [("scalar", 10, c) for c in (16, 8, 4)]


@pytest.mark.parametrize("family,d,codec", GUARDS)
def test_guards_of_the_kernels_no_earlier_test_reached(E, orc, family, d, codec):
    """The two guard cases of the existing gather tests, for long at d = 128, vec with run-time lanes per row and scalar with a reduced
    codec.  (1) one index equal to n_rows and one negative: skipped, the other rows of their bags still summed, evs_check_index_errors
    raises once and is then clear.  (2) one offset past nnz: that bag and the one before it are empty, every other bag unchanged."""
    T, B = 4, {"long": 5, "vec": 51, "scalar": 20}[family]
    name = long_name(d) if family == "long" else vec_name(codec, d, False) if family == "vec" else scalar_name(codec)
    rs = _rs(13, d, codec)
    tabs = PM.make_tables(orc, rs, T, d, codec)
    idx, off = PM.make_bags(rs, tabs, rs.randint(2, 6, size=(T, B)))
    good = check_case(E, orc, {name: 1}, B, d, codec, tabs, idx, off).reshape(T, B, d)
    EINDEX = E._lib.EVS_EINDEX

    def run(idx_, off_):
        before = E._lib.gather_kernels_seen()
        got = PM.pool(E, B, d, codec, tabs, idx_, off_)
        after = E._lib.gather_kernels_seen()
        assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}
        assert PM.index_flag(E) == EINDEX and PM.index_flag(E) == 0, "the flag is raised once and then clear"
        return got.reshape(T, B, d)

    k = 2                                                   # the table of 40 rows
    bad = [i.copy() for i in idx]
    b_hi, b_neg = 1, B - 2
    bad[k][off[k][b_hi]] = tabs[k].shape[0]                 # the first entry of a bag of >= 2
    bad[k][off[k][b_neg + 1] - 1] = -1                      # the last entry of another
    want = np.stack(PM.reference(orc, B, d, codec, tabs, bad, off)).view(np.uint32)
    got = run(bad, off)
    assert np.array_equal(got, want)
    assert not np.array_equal(got[k, b_hi], good[k, b_hi]) and got[k, b_hi].any() and got[k, b_neg].any()

    off2 = [o.copy() for o in off]
    b_bad = B // 2
    off2[k][b_bad] = idx[k].size + 7
    got = run(idx, off2)
    others = np.ones(B, bool)
    others[[b_bad - 1, b_bad]] = False
    assert np.array_equal(got[k][others], good[k][others]) and not got[k][~others].any()
    assert np.array_equal(np.delete(got, k, axis=0), np.delete(good, k, axis=0))


# ------------------------------------------------------------------------------------------------------- behind switches: one child
def test_forms_the_default_environment_cannot_reach():
    """The select form of the tile kernel and the unweighted fp32 grid-stride kernels, in one child process under EVS_GATHER_LONG=0
    EVS_GATHER_RF=0 (the switches are read once per process): the same two assertions per case there; the child also asserts that every
    CHILD_ONLY name went up.  A child that ends by signal, abort or timeout fails this test; nothing else is started here."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("EVS_GATHER_")}
    env.update(EVS_GATHER_LONG="0", EVS_GATHER_RF="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_pooling_matrix_env_child.py")] + CHILD_ONLY, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])


# --------------------------------------------------------------------------------------------------------------------------- closing
def test_every_default_reachable_instantiation_was_launched(E, record_at_start):
    """The whole record: every name this module's cases left at 0 is in CHILD_ONLY (runs last; it speaks about the module as a whole)."""
    seen = E._lib.gather_kernels_seen()
    assert set(seen) == set(record_at_start) and set(CHILD_ONLY) <= set(seen)
    never = sorted(k for k in seen if seen[k] == record_at_start[k])
    print("gather kernels in the record: %d, launched by this module: %d, child only: %d" % (len(seen), len(seen) - len(never), len(CHILD_ONLY)))
    assert never == sorted(CHILD_ONLY), "default-reachable gather kernels this module did not launch: %s" % sorted(set(never) - set(CHILD_ONLY))
