"""The wide kernel over encoded tables (csrc/evs_fused_wide_q.hip, 33 <= F <= 128, u16 / u8 / u4) through apply_emb_interact against
float64 over the oracle's decoded rows, under the contract of tests/_accuracy.py -- hard bound (d + 4) u M (L = 1, extra = 0), exact
zeros where M = 0, x bit for bit, median cap 4 -- at every row-tile edge, under its own dispatch record."""
import numpy as np
import pytest
import torch

import _accuracy as acc
import _accuracy_data as data

pytestmark = pytest.mark.gpu

SHAPES = [(F, 36) for F in (33, 48, 49, 64, 65, 96, 97, 128)] + [(F, d) for F in (33, 128) for d in (16, 32, 64)]
KERNEL = "interact_wide_q_kernel"


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _name(codec, F, d):
    return "wideq_c%d_d%d_nt%d" % (codec, d, 3 if F <= 48 else 4 if F <= 64 else 6 if F <= 96 else 8)


def _ran(E, call):
    """call() -> (its result, what went up in the encoded record); the fp32 wide record must not move"""
    before, fp32 = E._lib.wide_q_kernels_seen(), E._lib.wide_kernels_seen()
    out = call()
    torch.cuda.synchronize()
    assert E._lib.wide_kernels_seen() == fp32
    return out, {k: v - before[k] for k, v in E._lib.wide_q_kernels_seen().items() if v != before[k]}


def _sizes(F):
    return [200 + 31 * (k % 5) for k in range(F - 1)]   # a few hundred rows, different counts


def _indices(rs, n, B):
    """one index per bag; every table is read at row 0 (sample 0) and at its last row (the last sample); with one sample the
    even tables at 0 and the odd ones at n - 1"""
    idx = np.stack([rs.randint(0, m, B) for m in n]).astype(np.int64)
    idx[:, B - 1] = np.array(n) - 1
    idx[slice(None, None, 2 if B == 1 else 1), 0] = 0
    return idx


def _model(orc, codec, F, d, B, kind="unit", n=None):
    """-> x, the codes of T = F - 1 tables, indices"""
    rs, n = np.random.RandomState(3000 * F + 10 * d + codec), n or _sizes(F)
    codes = [data.codes(orc, codec, kind, rs, (m, d), k + 1) for k, m in enumerate(n)]
    return data.values(kind, rs, (B, d), 0), codes, _indices(rs, n, B)


def _ev(E, codec, codes):
    return E.EVTables([_dev(data.raw(codec, c)) for c in codes], codes[0].shape[1], codec)


def _ref(orc, codec, x, codes, idx, itself, absent=()):
    """float64 over the rows as the oracle decodes them"""
    dec = data.decode_all(orc, codec)
    rows = [dec[c[np.minimum(idx[k], len(c) - 1)]].astype(np.float32) for k, c in enumerate(codes)]
    for k, s in absent:
        rows[k][s] = 0   # an index out of range is a zero row
    return acc.Reference(x, [data.sub(r) for r in rows], itself)


@pytest.mark.parametrize("codec", [16, 8, 4])
@pytest.mark.parametrize("F,d", SHAPES)
def test_main_matrix(E, orc, codec, F, d):
    """B = 1, and B = 17: one full block and a tail block of one sample.  u16: `unit` reaches tail codes above 65 000, `dlrm`
    stays on the packed main-range path"""
    for kind in ("unit", "dlrm") + (("samesign", "cancel") if d == 36 else ()):
        _, codes, _ = _model(orc, codec, F, d, 1, kind)
        ev, rs = _ev(E, codec, codes), np.random.RandomState(F + d)
        for B in (1, 17):
            x, idx = data.values(kind, rs, (B, d), 0), _indices(rs, _sizes(F), B)
            for itself in (False, True):
                R, went_up = _ran(E, lambda: E.apply_emb_interact(_dev(x), None, _dev(idx), ev, None, itself, one_index_per_bag=True))
                assert went_up == {_name(codec, F, d): 1}
                case = "u%d F=%d d=%d B=%d itself=%d %s" % (codec, F, d, B, itself, kind)
                acc.check(R.cpu().numpy(), _ref(orc, codec, x, codes, idx, itself), case, KERNEL)


@pytest.mark.parametrize("codec", [16, 8, 4])
def test_every_start_phase_of_a_row(E, orc, codec):
    """d = 36, 9-row tables, idx[k, b] = (b + k) % 9: rows of 72 / 36 / 18 bytes start at every phase inside a 16-byte piece"""
    x, codes, _ = _model(orc, codec, 33, 36, 17, n=[9] * 32)
    idx = (np.arange(17)[None, :] + np.arange(32)[:, None]) % 9
    R, went_up = _ran(E, lambda: E.apply_emb_interact(_dev(x), None, _dev(idx), _ev(E, codec, codes), one_index_per_bag=True))
    assert went_up == {_name(codec, 33, 36): 1}
    acc.check(R.cpu().numpy(), _ref(orc, codec, x, codes, idx, False), "u%d start phases" % codec, KERNEL)


def test_u8_extreme_codes(E, orc):
    """rows made of one code -- 0, 127, 128, 254, 255 -- as rows 0..4 of every table, each of them indexed"""
    x, codes, idx = _model(orc, 8, 49, 36, 17)
    for c in codes:
        c[:5] = np.array([0, 127, 128, 254, 255])[:, None]
    idx[:, :10] = (np.arange(10)[None, :] + np.arange(48)[:, None]) % 5
    R, went_up = _ran(E, lambda: E.apply_emb_interact(_dev(x), None, _dev(idx), _ev(E, 8, codes), one_index_per_bag=True))
    assert went_up == {_name(8, 49, 36): 1}
    acc.check(R.cpu().numpy(), _ref(orc, 8, x, codes, idx, False), "u8 extreme codes", KERNEL)


@pytest.mark.parametrize("codec", [16, 8, 4])
def test_no_offsets_and_nothing_declared(E, orc, codec):
    """lS_o=None without one_index_per_bag: a ValueError before the encoded kernel existed.  With out=: written into and returned"""
    x, codes, idx = _model(orc, codec, 65, 36, 17)
    out = torch.full((17, 36 + 65 * 32), float("nan"), dtype=torch.float32, device="cuda")
    R, went_up = _ran(E, lambda: E.apply_emb_interact(_dev(x), None, _dev(idx), _ev(E, codec, codes), out=out))
    assert R is out and went_up == {_name(codec, 65, 36): 1}
    acc.check(out.cpu().numpy(), _ref(orc, codec, x, codes, idx, False), "u%d lS_o=None, out=" % codec, KERNEL)


@pytest.mark.parametrize("codec", [16, 8, 4])
def test_index_out_of_range(E, orc, codec):
    """one index = n: EVS_EINDEX with check_indices, that sample's pairs with the feature exactly 0 (M = 0), the rest within the bound"""
    x, codes, idx = _model(orc, codec, 97, 36, 17)
    idx[70, 16] = len(codes[70])
    ev, out = _ev(E, codec, codes), torch.full((17, 36 + 97 * 48), float("nan"), dtype=torch.float32, device="cuda")
    name, before = _name(codec, 97, 36), E._lib.wide_q_kernels_seen()
    with pytest.raises(E.EvsError) as e:
        E.apply_emb_interact(_dev(x), None, _dev(idx), ev, check_indices=True, out=out, one_index_per_bag=True)
    assert e.value.code == E._lib.EVS_EINDEX and E._lib.wide_q_kernels_seen()[name] == before[name] + 1
    ref = _ref(orc, codec, x, codes, idx, False, absent=[(70, 16)])
    assert (ref.M[16][(ref.li == 71) | (ref.lj == 71)] == 0).all()
    acc.check(out.cpu().numpy(), ref, "u%d index out of range" % codec, KERNEL)


def test_other_calls_keep_their_route(E, orc):
    """offsets given and not declared, or row weights: apply_emb then the dense form, the same R within the bound; int32 indices
    without offsets: refused by name.  The encoded record stands"""
    x, codes, idx = _model(orc, 8, 49, 36, 17, "dlrm")
    ev, lS_o, before = _ev(E, 8, codes), torch.arange(17, device="cuda").repeat(48, 1), E._lib.wide_q_kernels_seen()
    ones = [torch.ones(len(c), device="cuda") for c in codes]
    for kw in (dict(), dict(v_W_l=ones, one_index_per_bag=True)):
        dense = sum(E._lib.wide_kernels_seen().values())
        R = E.apply_emb_interact(_dev(x), lS_o, _dev(idx), ev, **kw)
        assert sum(E._lib.wide_kernels_seen().values()) == dense + 1
        acc.check(R.cpu().numpy(), _ref(orc, 8, x, codes, idx, False), "two-launch %s" % sorted(kw), "interact_wide_kernel")
    with pytest.raises(ValueError, match="pass lS_o"):
        E.apply_emb_interact(_dev(x), None, _dev(idx).int(), ev)
    assert E._lib.wide_q_kernels_seen() == before
