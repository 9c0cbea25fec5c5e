"""The wide interaction kernel (csrc/evs_fused_wide.hip, 33 <= F <= 128): the dense form through interact_features and the gather
form through apply_emb_interact against float64 under the contract of tests/_accuracy.py -- hard bound (d + 2 L + 2) u M with
L = 1, exact zeros where M = 0, x bit for bit, median cap -- on both sides of every row-tile edge, under its own dispatch record."""
import numpy as np
import pytest
import torch

import _accuracy as acc
import _accuracy_data as data

pytestmark = pytest.mark.gpu

EDGES = [33, 48, 49, 64, 65, 96, 97, 128]   # both sides of every NT edge (48 | 64 | 96), the first and the last width
SHAPES = [(F, 36) for F in EDGES] + [(F, d) for F in (33, 128) for d in (16, 32, 64)]
KINDS = ("unit", "samesign", "dlrm", "cancel")


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _name(form, F, d):
    return "wide_%s_d%d_nt%d" % (form, d, 3 if F <= 48 else 4 if F <= 64 else 6 if F <= 96 else 8)


def _ran(E, call):
    """call() -> (its result, the names of the wide record that went up, with by how much)"""
    before = E._lib.wide_kernels_seen()
    out = call()
    torch.cuda.synchronize()
    return out, {k: v - before[k] for k, v in E._lib.wide_kernels_seen().items() if v != before[k]}


def _dense(E, F, d, B, itself, kind, tile=False, pad=0):
    rs = np.random.RandomState(1000 * F + d)
    v = np.stack([data.values(kind, rs, (B, d), j) for j in range(F)])   # (F, B, d)
    # views of a (B, F, d) tile | rows; pad floats in front of every row of the tile take the rows off the 16-byte grid
    fs = list(_dev(np.pad(v.transpose(1, 0, 2), ((0, 0), (0, 0), (pad, 0))))[:, :, pad:].unbind(1)) if tile else list(_dev(v).unbind(0))
    R, went_up = _ran(E, lambda: E.interact_features(fs[0], fs[1:], "dot", itself))
    assert went_up == ({} if pad else {_name("dense", F, d): 1})
    case = "dense F=%d d=%d B=%d itself=%d %s%s" % (F, d, B, itself, kind, " tile" if tile else "")
    acc.check(R.cpu().numpy(), acc.Reference(v[0], [data.sub(v[j]) for j in range(1, F)], itself), case, "interact_wide_kernel")


@pytest.mark.parametrize("F,d", SHAPES)
def test_dense_form(E, F, d):
    """B = 37: two full blocks and a tail of 5"""
    for itself in (False, True):
        for kind in KINDS:
            _dense(E, F, d, 37, itself, kind)


@pytest.mark.parametrize("B,tile", [(37, True), (1, False), (1, True)])
def test_dense_form_strided_views_and_one_sample(E, B, tile):
    for F in (33, 128):
        _dense(E, F, 36, B, False, "unit", tile)


def test_rows_off_the_16_byte_grid_keep_the_generic_kernel(E):
    """not the wide kernel's to address: evs_interact_dot's generic kernel answers, under the same contract, and the record stands"""
    _dense(E, 33, 36, 5, False, "unit", tile=True, pad=1)


def _model(E, F, d, B, kind):
    """x, T = F - 1 fp32 tables of a few hundred rows (different counts), one index per bag; every table is read at index 0
    (sample 0) and at its index n - 1 (the last sample); with one sample the even tables at 0 and the odd ones at n - 1"""
    T, rs = F - 1, np.random.RandomState(2000 * F + d + B)
    n = [200 + 31 * (k % 5) for k in range(T)]
    tabs = [data.values(kind, rs, (n[k], d), k + 1) for k in range(T)]
    x = data.values(kind, rs, (B, d), 0)
    idx = np.stack([rs.randint(0, n[k], B) for k in range(T)]).astype(np.int64)
    idx[:, B - 1] = np.array(n) - 1
    idx[slice(None, None, 2 if B == 1 else 1), 0] = 0
    ev = E.EVTables.from_fp32(list(torch.split(_dev(np.concatenate(tabs)), n)))
    return x, tabs, idx, ev


def _gather_ref(x, tabs, idx, itself, absent=()):
    rows = [tabs[k][np.minimum(idx[k], len(tabs[k]) - 1)].copy() for k in range(len(tabs))]
    for k, s in absent:
        rows[k][s] = 0   # an index out of range is a zero row
    return acc.Reference(x, [data.sub(r) for r in rows], itself)


@pytest.mark.parametrize("B", [1, 16, 17])
@pytest.mark.parametrize("F,d", SHAPES[:8] + SHAPES[11:])
def test_gather_form(E, F, d, B):
    for itself in (False, True):
        for kind in KINDS:
            x, tabs, idx, ev = _model(E, F, d, B, kind)
            R, went_up = _ran(E, lambda: E.apply_emb_interact(_dev(x), None, _dev(idx), ev, None, itself, one_index_per_bag=True))
            assert went_up == {_name("gather", F, d): 1}
            acc.check(R.cpu().numpy(), _gather_ref(x, tabs, idx, itself), "gather F=%d d=%d B=%d itself=%d %s" % (F, d, B, itself, kind),
                      "interact_wide_kernel")


def test_gather_form_writes_out(E):
    x, tabs, idx, ev = _model(E, 65, 36, 17, "unit")
    out = torch.full((17, 36 + 65 * 32), float("nan"), dtype=torch.float32, device="cuda")
    R, went_up = _ran(E, lambda: E.apply_emb_interact(_dev(x), None, _dev(idx), ev, out=out, one_index_per_bag=True))
    assert R is out and went_up == {_name("gather", 65, 36): 1}
    acc.check(out.cpu().numpy(), _gather_ref(x, tabs, idx, False), "gather out=", "interact_wide_kernel")


def test_gather_form_index_out_of_range(E):
    """one index = n: EVS_EINDEX with check_indices, that sample's pairs with the feature exactly 0 (M = 0), the rest within the bound"""
    x, tabs, idx, ev = _model(E, 97, 36, 17, "unit")
    idx[70, 16] = len(tabs[70])
    out = torch.full((17, 36 + 97 * 48), float("nan"), dtype=torch.float32, device="cuda")
    name, before = _name("gather", 97, 36), E._lib.wide_kernels_seen()
    with pytest.raises(E.EvsError) as e:
        E.apply_emb_interact(_dev(x), None, _dev(idx), ev, check_indices=True, out=out, one_index_per_bag=True)
    assert e.value.code == E._lib.EVS_EINDEX and E._lib.wide_kernels_seen()[name] == before[name] + 1
    ref = _gather_ref(x, tabs, idx, False, absent=[(70, 16)])
    assert (ref.M[16][(ref.li == 71) | (ref.lj == 71)] == 0).all()
    acc.check(out.cpu().numpy(), ref, "gather, index out of range", "interact_wide_kernel")


def test_offsets_given_and_not_declared_go_two_launch(E):
    """apply_emb (any T) then the dense form over its (T, B, d) buffer: the same R within the bound"""
    x, tabs, idx, ev = _model(E, 49, 36, 17, "dlrm")
    lS_o = torch.arange(17, device="cuda").repeat(48, 1)
    pooled = E._lib.gather_kernels_seen()
    R, went_up = _ran(E, lambda: E.apply_emb_interact(_dev(x), lS_o, _dev(idx), ev))
    assert went_up == {_name("dense", 49, 36): 1} and E._lib.gather_kernels_seen() != pooled
    acc.check(R.cpu().numpy(), _gather_ref(x, tabs, idx, False), "two-launch", "interact_wide_kernel")
    with pytest.raises(ValueError, match="pass lS_o"):   # no offsets and not the gather form's to take (int32 indices): refused by name
        E.apply_emb_interact(_dev(x), None, _dev(idx).int(), ev)
