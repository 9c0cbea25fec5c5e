"""apply_emb_interact_bags (csrc/evs_fused_bags.hip: multi-hot bags pooled and interacted in one launch) against float64 at the
smallest shapes where the kernel can go wrong, under its dispatch record; pooled sums keep index order; bad input stays local."""
import numpy as np
import pytest
import torch

import _accuracy as acc

pytestmark = pytest.mark.gpu

#        d   T  itself  B  profile
CASES = [(16, 1, False, 1, "plus1"),
         (16, 15, True, 15, "short"),
         (16, 16, False, 17, "stage"),
         (32, 15, False, 16, "stage"),
         (32, 16, True, 33, "short"),
         (32, 27, False, 15, "plus1"),
         (36, 27, False, 33, "stage"),
         (36, 26, True, 17, "short"),
         (36, 15, False, 16, "plus1"),
         (64, 16, False, 33, "stage"),
         (64, 27, True, 1, "short"),
         (64, 1, False, 17, "stage"),
         (64, 15, True, 16, "plus1")]


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(E, d, T, B, profile, seed, mixed=False):
    """-> x, tables, lS_o, lS_i (numpy).  short: lengths 0..3, table 1 all empty behind two indices no bag refers to, the last table
    passed with nnz == 0; stage: four bags of S - 1, S, S + 1, 2 S + 1 among short ones; plus1: B + 1 offsets, the last one in
    front of nnz."""
    rs = np.random.RandomState(seed)
    S = E._lib.lib().evs_bags_fused_stage_rows(d)
    assert S == 4 * (64 // (d // 4))
    n_rows = rs.randint(3, 201, size=T)
    tables = [rs.uniform(-1, 1, size=(n, d)).astype(np.float32) for n in n_rows]
    if mixed:
        tables = [(t * 10.0 ** rs.uniform(-3, 3, size=t.shape)).astype(np.float32) for t in tables]
    lens = rs.randint(0, 4, size=(T, B))
    if profile == "stage":
        where = rs.choice(T * B, 4, replace=False)
        lens.reshape(-1)[where] = [S - 1, S, S + 1, 2 * S + 1]
    lS_o, lS_i = [], []
    for k in range(T):
        lead, trail = 0, 0
        if profile == "short" and T >= 3 and k in (1, T - 1):
            lens[k] = 0
            lead = 2 if k == 1 else 0
        if profile == "plus1":
            trail = k % 3
        starts = lead + np.concatenate([[0], np.cumsum(lens[k])]).astype(np.int64)
        lS_o.append(starts if profile == "plus1" else starts[:-1])
        lS_i.append(rs.randint(0, n_rows[k], size=lead + lens[k].sum() + trail).astype(np.int64))
    x = rs.uniform(-1, 1, size=(B, d)).astype(np.float32)
    return x, tables, lS_o, lS_i


def _pooled_seq(tables, lS_o, lS_i, B):
    """(B, T, d) fp32: every bag summed in index order from +0.0f"""
    out = np.zeros((B, len(tables), tables[0].shape[1]), np.float32)
    for k, t in enumerate(tables):
        ends = np.append(lS_o[k][1:], len(lS_i[k]))
        for b in range(B):
            for j in range(lS_o[k][b], ends[b]):
                out[b, k] = out[b, k] + t[lS_i[k][j]]
    return out


def _run(E, x, tables, lS_o, lS_i, itself, check_indices=True):
    ev = E.EVTables.from_fp32([torch.from_numpy(t) for t in tables], device="cuda:0")
    R = E.apply_emb_interact_bags(_dev(x), [_dev(o) for o in lS_o], [_dev(i) for i in lS_i], ev, itself, check_indices)
    torch.cuda.synchronize()
    return R.cpu().numpy()


@pytest.mark.parametrize("d,T,itself,B,profile", CASES)
def test_against_float64(E, d, T, itself, B, profile):
    label = "d=%d T=%d itself=%d B=%d %s" % (d, T, itself, B, profile)
    name = "bagsf_d%d_nt%d" % (d, 1 if T + 1 <= 16 else 2)
    x, tables, lS_o, lS_i = _inputs(E, d, T, B, profile, seed=1000 * d + 10 * T + B)
    ref = acc.reference_from_bags(x, tables, lS_o, lS_i, itself)
    # the cap is met by the reference alone: the sequential fp32 evaluation of the same inputs
    Tm = np.concatenate([x[:, None, :], _pooled_seq(tables, lS_o, lS_i, B)], 1)
    Z = np.zeros((B, T + 1, T + 1), np.float32)
    for c in range(d):
        Z = Z + Tm[:, :, None, c] * Tm[:, None, :, c]
    acc.check(np.concatenate([x, Z[:, ref.li, ref.lj]], 1), ref, label, "seq_fp32")
    before = E._lib.bags_fused_kernels_seen()
    R = _run(E, x, tables, lS_o, lS_i, itself)
    after = E._lib.bags_fused_kernels_seen()
    e = acc.check(R, ref, label, name)
    print("%s [%s]: worst err/bound %.3g, median %.3g" % (label, name, e["worst"], e["median"]))
    assert len(after) == 8 and {k: after[k] - before[k] for k in after} == {k: int(k == name) for k in after}


@pytest.mark.parametrize("d", [36, 64])
def test_pooled_sums_keep_index_order(E, d):
    T, B = 3, d + 5
    x, tables, lS_o, lS_i = _inputs(E, d, T, B, "stage", seed=d, mixed=True)
    x = np.zeros((B, d), np.float32)
    x[np.arange(B), np.arange(B) % d] = 1.0
    R = _run(E, x, tables, lS_o, lS_i, False)
    want = _pooled_seq(tables, lS_o, lS_i, B)[np.arange(B), :, np.arange(B) % d]       # (B, T)
    li, lj = acc.pair_index(T + 1, False)
    for t in range(T):
        col = d + int(np.flatnonzero((li == t + 1) & (lj == 0))[0])
        assert np.array_equal(R[:, col], want[:, t]), "table %d: the pooled sum is not the sequential fp32 sum in index order" % t


@pytest.mark.parametrize("kind", ["index_past_end", "negative_index", "decreasing_offsets"])
def test_bad_input_stays_local(E, kind):
    """One bad bag, (table k, sample m).  An offset belongs to two bags: lowering offsets[m + 1] below offsets[m] also moves the start
    of bag m + 1 (still a valid bag) over the indices from offsets[m] - 1 on.  Those point at a row of zeros here, so that sample m + 1
    keeps its bits and only the verdict on bag m is in play."""
    d, T, B, k, m = 36, 5, 20, 2, 9
    x, tables, lS_o, lS_i = _inputs(E, d, T, B, "plus1", seed=7)
    lS_o, lS_i, tables = [o.copy() for o in lS_o], [i.copy() for i in lS_i], [t.copy() for t in tables]
    grow = 2 - (lS_o[k][m + 1] - lS_o[k][m])            # bag (k, m) holds exactly two indices
    lS_o[k][m + 1:] += grow
    lS_i[k] = np.random.RandomState(3).randint(1, len(tables[k]), size=lS_o[k][-1] + 1).astype(np.int64)
    j = int(lS_o[k][m])
    assert j >= 1
    if kind == "decreasing_offsets":
        tables[k][0] = 0.0
        lS_i[k][j - 1:j + 2] = 0
    clean = _run(E, x, tables, lS_o, lS_i, False)
    want_tables = list(tables)
    want_i = [i.copy() for i in lS_i]
    if kind == "decreasing_offsets":
        lS_o[k][m + 1] = j - 1                          # bag m = [j, j - 1): empty
    else:                                               # a zero row: the reference reads a row of zeros appended to the table
        lS_i[k][j] = len(tables[k]) + 3 if kind == "index_past_end" else -1
        want_tables[k] = np.concatenate([tables[k], np.zeros((1, d), np.float32)])
        want_i[k][j] = len(tables[k])
    R = _run(E, x, tables, lS_o, lS_i, False, check_indices=False)
    with pytest.raises(E.EvsError) as err:
        E._lib.check(E._lib.lib().evs_check_index_errors(None))
    assert err.value.code == E._lib.EVS_EINDEX
    acc.check(R, acc.reference_from_bags(x, want_tables, lS_o, want_i, False), kind, "bagsf_d36_nt1")
    others = np.arange(B) != m
    assert np.array_equal(R[others].view(np.uint32), clean[others].view(np.uint32)), "another sample changed"
    if kind != "decreasing_offsets":
        assert not np.array_equal(R[m].view(np.uint32), clean[m].view(np.uint32))
