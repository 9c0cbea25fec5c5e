"""tests/_bags_edges.py holds what tests/test_gpu_bags_edges.py relies on: every stage edge of the fused multi-hot kernel is in edge_lens by
construction, asserted here from the lengths alone, and the accuracy contract's median cap is met by the reference alone -- the sequential
fp32 evaluation of the same inputs passes tests/_accuracy.py.  No GPU."""
import numpy as np
import pytest

import _accuracy as acc
import _bags_edges as BE
from test_gpu_bags_fused import _pooled_seq

CASES = [(d, T) for d in (16, 32, 36, 64) for T in (1, 15, 16, 27)]


def _stages(total, S):
    return max(1, -(-total // S))   # an all-empty sample is one stage of zero rows


@pytest.mark.parametrize("d,T", CASES + [(d, 3) for d in (16, 32, 36, 64)])
def test_every_edge_is_in_the_lengths(d, T):
    S = BE.STAGE_ROWS[d]
    assert S == 4 * (64 // (d // 4))
    lens = BE.edge_lens(S, T)
    assert lens.shape == (T, 33) and lens.dtype == np.int64 and (lens >= 0).all()
    assert np.array_equal(lens, BE.edge_lens(S, T)), "the lengths are a function of (S, T)"
    pre = np.concatenate([np.zeros((1, 33), np.int64), np.cumsum(lens, axis=0)])     # pre[t, b]: lookups of sample b in front of table t
    tot = pre[T]
    assert {0, 1, S - 1, S, S + 1, 2 * S, 2 * S + 1} <= set(tot.tolist())
    st = [_stages(t, S) for t in tot]
    if T >= 2:
        # a bag from flattened position S - 1 with S + 2 lookups: stages 0, 1 and 2
        assert ((pre[:T] == S - 1) & (lens == S + 2)).any() and (S - 1) // S == 0 and ((S - 1) + (S + 2) - 1) // S == 2
        # tables 0..j sum to exactly S and table j + 1 is not empty: the stage boundary is a table boundary
        assert any(pre[j + 1, b] == S and lens[j + 1, b] > 0 for b in range(33) for j in range(T - 1))
    if T >= 5:
        # a run of three empty tables whose prefix is S, and a lookup behind it
        assert any(pre[t, b] == S and not lens[t:t + 3, b].any() and tot[b] > S for b in range(33) for t in range(1, T - 2))
    assert any(tot[b] > 0 and lens[0, b] == tot[b] for b in range(33)), "no sample with all its lookups in table 0"
    assert any(tot[b] > 0 and lens[T - 1, b] == tot[b] for b in range(33)), "no sample with all its lookups in table T - 1"
    # wave w of chunk 0 takes samples w, w + 4, w + 8, w + 12
    waves = [[(tot[w + 4 * u], st[w + 4 * u]) for u in range(4)] for w in range(4)]
    assert any(a[0] == 0 and b[1] > 1 and c[0] == 0 and e[0] > 0 and e[1] == 1 for a, b, c, e in waves), "empty, multi-stage, empty, single-stage"
    assert any(a[1] > 1 and b[1] > 1 and c[0] > 0 and c[1] == 1 and e[0] == 0 for a, b, c, e in waves), \
        "multi-stage, multi-stage, single-stage, then an empty last sample"
    assert not tot[16:32].any(), "the second chunk is all empty"
    assert tot[32] == S + 1


@pytest.mark.parametrize("d,T", CASES)
def test_the_sequential_fp32_evaluation_meets_the_contract(d, T):
    """the "seq_fp32" pre-check of test_gpu_bags_fused.py::test_against_float64: pooled in index order from +0.0f, then d rank-one updates"""
    x, tables, lS_o, lS_i = BE.edge_inputs(d, T, seed=1000 * d + T)
    Tm = np.concatenate([x[:, None, :], _pooled_seq(tables, lS_o, lS_i, len(x))], 1)
    Z = np.zeros((len(x), T + 1, T + 1), np.float32)
    for c in range(d):
        Z = Z + Tm[:, :, None, c] * Tm[:, None, :, c]
    for itself in (False, True):
        ref = acc.reference_from_bags(x, tables, lS_o, lS_i, itself)
        assert ref.L == 2 * BE.STAGE_ROWS[d] + 1
        e = acc.check(np.concatenate([x, Z[:, ref.li, ref.lj]], 1), ref, "d=%d T=%d itself=%d edges" % (d, T, itself), "seq_fp32")
        print("d=%d T=%d itself=%d: worst err/bound %.3g, median %.3g" % (d, T, itself, e["worst"], e["median"]))
