"""Every instantiation of interact_wide_kernel (csrc/evs_fused_wide.hip: d in 16, 32, 36, 64 x NT in 3, 4, 6, 8), in the dense form
(interact_features) AND the gather form (apply_emb_interact, one index per bag), against float64 under the contract of tests/_accuracy.py
with L = 1, each call under the dispatch record: exactly the one name, by exactly 1.

  * F = 48 | 49 and 96 | 97 are the two sides of an NT edge for every d; d = 64 also runs F = 64 | 65, the two sides of the switch between
    two generations of rows in registers (NT KS <= 64) and the serial form.  F = 47, 95 and 127 are there for the run phases (below).
  * dense form B = 37; gather form B = 21: one full block, then a tail in which wave 1 has one sample and waves 2 and 3 have none.
    Tables of one row sit among the others.
  * run phases: a band's run starts at float (b out_row + (0 | d + tri(16 ti))) mod 4 of a 16-byte piece, and the band buffer, the masks and
    the partial first and last piece all move with it.  Every case notes the phases of its (sample, band)s; the test in front of the closing
    one asserts that band 0 and band NT - 1 of each NT saw all four.  out_row is a multiple of 4 for every planned F but 49 | 65 | 97 with
    itself, which never reach band NT - 1 of NT = 6 or 8, nor NT = 3 at all: hence F = 47, 95, 127 (out_row odd, every phase in any four
    consecutive samples).
  * the gather form with a strided x AND a stacked index tensor whose stride(0) > B, out-of-range values in the padding of both.
  * four bad indices in one call (-1, n, 2**32 + 1, 2**63 - 1), in samples of different waves, the call's last sample among them, in a
    serial and in an ahead instantiation.

The closing test reads the record: all 32 names went up within this module.

Wall time on an MI355X: this module 2.6 s for 48 tests (174 launches of at most 37 samples each, and their float64 references)."""
import numpy as np
import pytest
import torch

import _accuracy as acc
import _accuracy_data as data
from test_gpu_wide import _dev, _gather_ref, _name, _ran

pytestmark = pytest.mark.gpu

DIMS = (16, 32, 36, 64)
SHAPES = [(F, d) for d in DIMS for F in (48, 49, 96, 97)] + [(64, 64), (65, 64)] + [(47, 36), (95, 16), (127, 32)]
KINDS = ("dlrm", "cancel")
PHASES = {}   # (NT, band) -> the run phases its cases had


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


@pytest.fixture(scope="module", autouse=True)
def record_at_start(E):
    """the record before this module's first case: the closing test counts this module's launches only"""
    return dict(E._lib.wide_kernels_seen())


def _nt(F):
    return 3 if F <= 48 else 4 if F <= 64 else 6 if F <= 96 else 8


def _tri(i, itself):
    return i * (i - 1 + 2 * itself) // 2   # pairs in front of row i of the packed triangle


def _note_phases(R, F, d, itself):
    """sh of every (sample, band) of one call, recomputed on the host (R's first row is on a 16-byte boundary)"""
    B, out_row = R.shape
    assert R.data_ptr() % 16 == 0 and out_row == d + _tri(F, itself)
    for ti in range((F + 15) // 16):
        first = 0 if ti == 0 else d + _tri(16 * ti, itself)
        PHASES.setdefault((_nt(F), ti), set()).update((b * out_row + first) % 4 for b in range(B))


@pytest.mark.parametrize("F,d", SHAPES)
def test_dense_form(E, F, d):
    """B = 37: two full blocks and a tail of 5"""
    B = 37
    for kind in KINDS:
        rs = np.random.RandomState(3000 * F + d)
        v = np.stack([data.values(kind, rs, (B, d), j) for j in range(F)])   # (F, B, d)
        fs = list(_dev(v).unbind(0))
        for itself in (False, True):
            R, went_up = _ran(E, lambda: E.interact_features(fs[0], fs[1:], "dot", itself))
            assert went_up == {_name("dense", F, d): 1}
            _note_phases(R, F, d, itself)
            acc.check(R.cpu().numpy(), acc.Reference(v[0], [data.sub(v[j]) for j in range(1, F)], itself),
                      "dense F=%d d=%d B=%d itself=%d %s" % (F, d, B, itself, kind), "interact_wide_kernel")


def _model(E, F, d, B, kind):
    """x, T = F - 1 fp32 tables, one index per bag: every eleventh table has ONE row, the others a few hundred (different counts) and are
    read at index 0 (sample 0) and at index n - 1 (the last sample)"""
    T, rs = F - 1, np.random.RandomState(4000 * F + d + B)
    n = [1 if k % 11 == 5 else 200 + 31 * (k % 5) for k in range(T)]
    tabs = [data.values(kind, rs, (n[k], d), k + 1) for k in range(T)]
    x = data.values(kind, rs, (B, d), 0)
    idx = np.stack([rs.randint(0, n[k], B) for k in range(T)]).astype(np.int64)
    idx[:, B - 1] = np.array(n) - 1
    idx[:, 0] = 0
    ev = E.EVTables.from_fp32(list(torch.split(_dev(np.concatenate(tabs)), n)))
    return x, tabs, idx, ev


def _gather(E, F, d, x, idx, ev, itself, strided=False):
    """one call of the gather form under the record.  strided: x is a column slice of a wider tensor (rows 16-byte aligned, d + 12 floats
    apart, NaN around them), the indices a [:, :B] view of a (T, B + 3) tensor whose padding no table holds.  -> R (device)"""
    xd, idxd = _dev(x), _dev(idx)
    if strided:
        B, T = idx.shape[1], idx.shape[0]
        xw = torch.full((B, d + 12), float("nan"), dtype=torch.float32, device="cuda")
        iw = torch.full((T, B + 3), 2 ** 40, dtype=torch.int64, device="cuda")
        xw[:, 4:4 + d], iw[:, :B] = xd, idxd
        xd, idxd = xw[:, 4:4 + d], iw[:, :B]
        assert xd.data_ptr() % 16 == 0 and xd.stride(0) == d + 12 and idxd.stride(0) == B + 3
    R, went_up = _ran(E, lambda: E.apply_emb_interact(xd, None, idxd, ev, None, itself, check_indices=True, one_index_per_bag=True))
    assert went_up == {_name("gather", F, d): 1}
    _note_phases(R, F, d, itself)
    return R


@pytest.mark.parametrize("F,d", SHAPES)
def test_gather_form(E, F, d):
    """B = 21: a full block; in the tail block wave 0 has four samples, wave 1 one, waves 2 and 3 none"""
    B = 21
    for kind in KINDS:
        x, tabs, idx, ev = _model(E, F, d, B, kind)
        assert 1 in [len(t) for t in tabs]
        for itself in (False, True):
            R = _gather(E, F, d, x, idx, ev, itself)
            acc.check(R.cpu().numpy(), _gather_ref(x, tabs, idx, itself), "gather F=%d d=%d B=%d itself=%d %s" % (F, d, B, itself, kind),
                      "interact_wide_kernel")


@pytest.mark.parametrize("F,d", [(96, 64), (49, 16)])
def test_gather_form_strides(E, F, d):
    """x_stride and idx_stride, in a serial (d = 64, NT = 6) and in an ahead (d = 16, NT = 4) instantiation"""
    x, tabs, idx, ev = _model(E, F, d, 21, "dlrm")
    for itself in (False, True):
        R = _gather(E, F, d, x, idx, ev, itself, strided=True)
        acc.check(R.cpu().numpy(), _gather_ref(x, tabs, idx, itself), "gather, strided, F=%d d=%d itself=%d" % (F, d, itself), "interact_wide_kernel")


@pytest.mark.parametrize("F,d", [(96, 64), (49, 32)])
def test_gather_form_bad_indices(E, F, d):
    """Four bad indices in one call, each one sample of one table, in four row-tiles' features and four waves: -1 (block 0, wave 1), n (wave
    2), 2**32 + 1 whose low 32 bits are a valid index (wave 3), 2**63 - 1 in the call's last sample (block 1, wave 1).  Serial (d = 64,
    NT = 6) and ahead (d = 32, NT = 4).  EVS_EINDEX with check_indices; out was NaN; those samples' pairs with those features are exactly 0
    (M = 0), everything else within the bound."""
    B, T = 21, F - 1
    x, tabs, idx, ev = _model(E, F, d, B, "dlrm")
    bad = [(1, 5, -1), (17, 9, None), (40, 14, 2 ** 32 + 1), (T - 1, B - 1, 2 ** 63 - 1)]
    for k, s, i in bad:
        assert len(tabs[k]) > 1
        idx[k, s] = len(tabs[k]) if i is None else i
    out = torch.full((B, d + _tri(F, 0)), float("nan"), dtype=torch.float32, device="cuda")
    name, before = _name("gather", F, d), E._lib.wide_kernels_seen()
    with pytest.raises(E.EvsError) as e:
        E.apply_emb_interact(_dev(x), None, _dev(idx), ev, check_indices=True, out=out, one_index_per_bag=True)
    after = E._lib.wide_kernels_seen()
    assert e.value.code == E._lib.EVS_EINDEX and {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}
    _note_phases(out, F, d, 0)
    ref = _gather_ref(x, tabs, idx, False, absent=[(k, s) for k, s, _ in bad])
    for k, s, _ in bad:
        assert (ref.M[s][(ref.li == k + 1) | (ref.lj == k + 1)] == 0).all()
    acc.check(out.cpu().numpy(), ref, "gather, bad indices, F=%d d=%d" % (F, d), "interact_wide_kernel")


def test_every_run_phase_was_seen():
    """runs behind every case (PHASES is what they noted): band 0 and band NT - 1 of each NT started at every float of a 16-byte piece"""
    for nt in (3, 4, 6, 8):
        for band in (0, nt - 1):
            assert PHASES.get((nt, band), set()) == {0, 1, 2, 3}, "NT = %d, band %d: run phases %s" % (nt, band, sorted(PHASES.get((nt, band), ())))


def test_every_instantiation_was_launched_in_both_forms(E, record_at_start):
    """runs last: it speaks about the module as a whole"""
    seen = E._lib.wide_kernels_seen()
    assert len(seen) == 32 and set(seen) == set(record_at_start)
    assert set(seen) == {"wide_%s_d%d_nt%d" % (form, d, nt) for form in ("dense", "gather") for d in DIMS for nt in (3, 4, 6, 8)}
    never = sorted(k for k in seen if seen[k] == record_at_start[k])
    assert not never, "instantiations of the wide kernel this module did not launch: %s" % never
