"""The stage pipeline of emb_interact_bags_kernel (csrc/evs_fused_bags.hip) at every edge, by construction: tests/_bags_edges.py lays the
sample totals on both sides of every multiple of the stage size S, table boundaries on stage boundaries, a bag over three stages, empty
samples between and behind multi-stage ones of the same wave, an empty chunk and a one-sample chunk into ONE call of 33 samples
(tests/test_bags_edges_layout.py asserts that from the lengths, without a GPU).  Here that call runs

  * against float64 under the contract of tests/_accuracy.py, L the longest bag (2 S + 1), for every d, T on both sides of the NT edge and
    T = 1, itself both ways, each under the dispatch record: exactly the one name, by exactly 1;
  * for every element of every pooled row as bits: x = e_c in every sample turns column (t + 1, 0) of R into element c of the pooled row of
    table t, which must be the fp32 sum in index order -- d launches per d, no tolerance;
  * through the rest of the call's surface: out=, a strided x, B and B + 1 offsets in one call, a call without any lookup;
  * with one bad bag in the second half of the head (table 20) and one bad index in the second stage of a multi-stage sample: the flag is
    raised, every other sample keeps its bits, the bad sample is the reference with a row of zeros.

The closing test reads the record: all eight instantiations went up within this module.

Wall time on an MI355X: this module 1.3 s for 29 tests (193 launches of at most 33 samples each, 148 of them the one-column launches of the
bit check)."""
import numpy as np
import pytest
import torch

import _accuracy as acc
import _bags_edges as BE
from test_gpu_bags_fused import _pooled_seq

pytestmark = pytest.mark.gpu

DIMS = (16, 32, 36, 64)


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    for d in DIMS:
        assert E._lib.lib().evs_bags_fused_stage_rows(d) == BE.STAGE_ROWS[d]
    return E


@pytest.fixture(scope="module", autouse=True)
def record_at_start(E):
    """the record before this module's first case: the closing test counts this module's launches only"""
    return dict(E._lib.bags_fused_kernels_seen())


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _name(d, T):
    return "bagsf_d%d_nt%d" % (d, 1 if T + 1 <= 16 else 2)


def _tables(E, tables):
    return E.EVTables.from_fp32([torch.from_numpy(t) for t in tables], device="cuda:0")


def _run(E, name, x, ev, lS_o, lS_i, itself, check_indices=True, out=None):
    """one call under the record: exactly `name` goes up, by 1.  x: numpy, or a device tensor (a view).  -> R (numpy)"""
    before = E._lib.bags_fused_kernels_seen()
    R = E.apply_emb_interact_bags(x if torch.is_tensor(x) else _dev(x), [_dev(o) for o in lS_o], [_dev(i) for i in lS_i], ev, itself,
                                  check_indices, out=out)
    torch.cuda.synchronize()
    after = E._lib.bags_fused_kernels_seen()
    assert len(after) == 8 and {k: after[k] - before[k] for k in after} == {k: int(k == name) for k in after}
    assert out is None or R is out
    return R.cpu().numpy()


@pytest.mark.parametrize("d,T", [(d, T) for d in DIMS for T in (15, 16, 27)] + [(16, 1), (64, 1)])
def test_against_float64(E, d, T):
    """T = 15: the last NT = 1 (F = 16); T = 16: NT = 2 at F = 17; T = 27: the most tables; T = 1: every edge inside one table"""
    x, tables, lS_o, lS_i = BE.edge_inputs(d, T, seed=1000 * d + T)
    ev = _tables(E, tables)
    for itself in (False, True):
        label = "edges d=%d T=%d itself=%d" % (d, T, itself)
        ref = acc.reference_from_bags(x, tables, lS_o, lS_i, itself)
        assert ref.L == 2 * BE.STAGE_ROWS[d] + 1
        e = acc.check(_run(E, _name(d, T), x, ev, lS_o, lS_i, itself), ref, label, _name(d, T))
        print("%s [%s]: worst err/bound %.3g, median %.3g" % (label, _name(d, T), e["worst"], e["median"]))


@pytest.mark.parametrize("d", DIMS)
def test_every_pooled_element_is_the_sum_in_index_order(E, d):
    """x = e_c: Z[t + 1][0] = 0 + 1.0 * pooled[t][c] + 0 ... = pooled[t][c], whatever the chain's order -- the bits of the accumulators
    that the stages carry, for every bag of the edge lengths and every element of its row"""
    T = 3
    _, tables, lS_o, lS_i = BE.edge_inputs(d, T, seed=d, mixed=True)
    B = len(lS_o[0])
    want = _pooled_seq(tables, lS_o, lS_i, B)            # (B, T, d)
    ev = _tables(E, tables)
    li, lj = acc.pair_index(T + 1, False)
    cols = [d + int(np.flatnonzero((li == t + 1) & (lj == 0))[0]) for t in range(T)]
    o_dev, i_dev = [_dev(o) for o in lS_o], [_dev(i) for i in lS_i]
    name = _name(d, T)
    before = E._lib.bags_fused_kernels_seen()
    for c in range(d):
        x = torch.zeros((B, d), dtype=torch.float32, device="cuda")
        x[:, c] = 1.0
        R = E.apply_emb_interact_bags(x, o_dev, i_dev, ev, False, True).cpu().numpy()
        assert np.array_equal(R[:, cols], want[:, :, c]), "element %d: a pooled sum is not the sequential fp32 sum in index order" % c
    after = E._lib.bags_fused_kernels_seen()
    assert {k: after[k] - before[k] for k in after} == {k: d * int(k == name) for k in after}


def test_out_is_written_whole(E):
    d, T = 36, 16
    x, tables, lS_o, lS_i = BE.edge_inputs(d, T, seed=11)
    out = torch.full((len(x), d + (T + 1) * T // 2), float("nan"), dtype=torch.float32, device="cuda")
    R = _run(E, _name(d, T), x, _tables(E, tables), lS_o, lS_i, False, out=out)     # (R is out: _run)
    acc.check(R, acc.reference_from_bags(x, tables, lS_o, lS_i, False), "out=", _name(d, T))


def test_strided_x(E):
    """x is a column slice: rows 16-byte aligned, d + 12 floats apart, NaN around them"""
    d, T = 16, 27
    x, tables, lS_o, lS_i = BE.edge_inputs(d, T, seed=12)
    wide = torch.full((len(x), d + 12), float("nan"), dtype=torch.float32, device="cuda")
    xv = wide[:, 4:4 + d]
    xv.copy_(_dev(x))
    assert xv.data_ptr() % 16 == 0 and xv.stride(0) == d + 12 and xv.stride(1) == 1
    R = _run(E, _name(d, T), xv, _tables(E, tables), lS_o, lS_i, True)
    acc.check(R, acc.reference_from_bags(x, tables, lS_o, lS_i, True), "strided x", _name(d, T))


def test_offsets_of_B_and_of_B_plus_1_in_one_call(E):
    """even tables: B offsets, the last bag ends at nnz; odd tables: B + 1 offsets, the last one in front of indices no bag refers to"""
    d, T = 64, 15
    x, tables, lS_o, lS_i = BE.edge_inputs(d, T, seed=13)
    ref = acc.reference_from_bags(x, tables, lS_o, lS_i, False)
    for k in range(1, T, 2):
        lS_o[k] = np.append(lS_o[k], len(lS_i[k]))
        lS_i[k] = np.append(lS_i[k], np.arange(1 + k % 3) % len(tables[k]))
    assert {len(o) for o in lS_o} == {len(x), len(x) + 1} and any(o[-1] < len(i) for o, i in zip(lS_o[1::2], lS_i[1::2]))
    acc.check(_run(E, _name(d, T), x, _tables(E, tables), lS_o, lS_i, False), ref, "B | B + 1 offsets", _name(d, T))


@pytest.mark.parametrize("d,T", [(32, 16), (36, 15)])
def test_a_call_without_any_lookup(E, d, T):
    """every index tensor empty (its data_ptr() is NULL): R is x, then exact zeros -- but x . x with itself"""
    B = 33
    x, tables, _, _ = BE.edge_inputs(d, T, seed=14)
    lS_o, lS_i = [np.zeros(B, np.int64)] * T, [np.zeros(0, np.int64)] * T
    assert _dev(lS_i[0]).data_ptr() == 0
    ev = _tables(E, tables)
    for itself in (False, True):
        R = _run(E, _name(d, T), x, ev, lS_o, lS_i, itself)
        ref = acc.reference_from_bags(x, tables, lS_o, lS_i, itself)
        acc.check(R, ref, "no lookup, itself=%d" % itself, _name(d, T))      # x bit for bit, M == 0 -> exactly 0, (0, 0) within the bound
        xx = (ref.li == 0) & (ref.lj == 0)
        assert xx.sum() == int(itself) and (ref.M[:, ~xx] == 0).all() and not R[:, d:][:, ~xx].any() and (R[:, d:][:, xx] > 0).all()


BAD = ["decreasing_offsets", -1, "n_rows", 2 ** 32 + 1, 2 ** 63 - 1]


@pytest.mark.parametrize("kind", BAD, ids=[str(k) for k in BAD])
def test_bad_input_at_the_edges_stays_local(E, kind):
    """d = 36, T = 27, the first 20 samples of the edge lengths, B + 1 offsets.
    decreasing_offsets: bag (table 20, sample 9) -- the half of the head that reads the offsets of tables 16 to 26 -- holds two indices and
    its end is lowered below its start.  The offset is also the start of bag (20, 10), a valid bag that now begins three indices earlier,
    inside a two-stage sample: those indices point at a row of zeros, so sample 10 keeps its bits and only the verdict on bag 9 is in play.
    an index: lookup S + 5 of sample 7, whose 2 S + 1 lookups are all in table 26: the second stage.  2**32 + 1 has valid low 32 bits."""
    d, T, B, S = 36, 27, 20, 28
    rs = np.random.RandomState(21)
    lens = BE.edge_lens(S, T)[:, :B].copy()
    k, m = (20, 9) if kind == "decreasing_offsets" else (26, 7)
    lens[20, 9] = 2
    lens[20, 10] = max(lens[20, 10], 1)
    n_rows = rs.randint(3, 201, size=T)
    tables = [rs.uniform(-1, 1, size=(n, d)).astype(np.float32) for n in n_rows]
    lS_o, lS_i = BE.bags(rs, lens, n_rows)
    lS_o = [np.append(o, len(i)) for o, i in zip(lS_o, lS_i)]
    lS_i[20] = np.maximum(lS_i[20], 1)                  # row 0 of table 20 is the row of zeros; nothing else points at it
    tables[20][0] = 0.0
    x = rs.uniform(-1, 1, size=(B, d)).astype(np.float32)
    j = int(lS_o[k][m])
    if kind == "decreasing_offsets":
        assert j >= 1 and lS_o[k][m + 1] == j + 2
        lS_i[k][j - 1:j + 2] = 0
    else:
        assert lens[k, m] == lens[:, m].sum() == 2 * S + 1
        j += S + 5
    ev = _tables(E, tables)
    name = _name(d, T)
    clean = _run(E, name, x, ev, lS_o, lS_i, False)
    want_tables, want_i = list(tables), [i.copy() for i in lS_i]
    lS_o, lS_i = [o.copy() for o in lS_o], [i.copy() for i in lS_i]
    if kind == "decreasing_offsets":
        lS_o[k][m + 1] = j - 1                          # bag m = [j, j - 1): empty
    else:                                               # a zero row: the reference reads a row of zeros appended to the table
        lS_i[k][j] = len(tables[k]) if kind == "n_rows" else kind
        want_tables[k] = np.concatenate([tables[k], np.zeros((1, d), np.float32)])
        want_i[k][j] = len(tables[k])
    R = _run(E, name, x, ev, lS_o, lS_i, False, check_indices=False)
    with pytest.raises(E.EvsError) as err:
        E._lib.check(E._lib.lib().evs_check_index_errors(None))
    assert err.value.code == E._lib.EVS_EINDEX
    acc.check(R, acc.reference_from_bags(x, want_tables, lS_o, want_i, False), str(kind), name)
    others = np.arange(B) != m
    assert np.array_equal(R[others].view(np.uint32), clean[others].view(np.uint32)), "another sample changed"
    if kind != "decreasing_offsets":
        assert not np.array_equal(R[m].view(np.uint32), clean[m].view(np.uint32))


def test_every_instantiation_was_launched(E, record_at_start):
    """runs last: it speaks about the module as a whole"""
    seen = E._lib.bags_fused_kernels_seen()
    assert len(seen) == 8 and set(seen) == set(record_at_start)
    never = sorted(k for k in seen if seen[k] == record_at_start[k])
    assert not never, "instantiations of the fused multi-hot kernel this module did not launch: %s" % never
