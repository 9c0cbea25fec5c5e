"""Every interaction path against float64 with a scale-aware bound (tests/_accuracy.py): each case names the kernel its
launcher conditions are meant to reach and runs over the data kinds

  unit      U(-1, 1)
  dlrm      rows U(+-sqrt(1/n)), n from the Kaggle cardinalities (one batch spans 2^-12 .. 2^-1); x >= 0 around 0.1
  cancel    pairs whose exact dot is 0: "even" rows repeat each value twice, "odd" rows carry (b, -b); x is even
  samesign  every value positive (the largest honest error of an fp32 chain)
  scaled    the dlrm kind with the tables (or weights) and x times 2^s, s = -24 / +24: the bound again, and bit-exact
            power-of-two equivariance against the unscaled run (codec cases: x only)

The reference is computed on at most 2 048 sampled rows per call (rows 0, B - 1 and the last 16-sample block always)."""
import numpy as np
import pytest
import torch

import _accuracy as acc
from _accuracy_data import KAGGLE_LN, codes as _codes, decode_all as _decode_all, raw as _raw, sub as _sub, values as _values   # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = ("unit", "dlrm", "cancel", "samesign")
S = (-24, 24)


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


@pytest.fixture(scope="module", autouse=True)
def headroom():
    """per kernel: the worst err / bound and the largest median statistic seen (printed at the end: pytest -s)"""
    yield
    for k, (w, m, n) in sorted(acc.STATS.items()):
        print("\nheadroom %-55s worst err/bound %.3f  median <= %.3f  (%d checks)" % (k, w, m, n))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------------------ data
def _ref_dense(x, feats, rows, itself):
    return acc.Reference(x[rows], [_sub(f[rows]) for f in feats], itself)


def _tables(kind, rs, T, d, n_max=3000):
    ns = [min(KAGGLE_LN[k % 26], n_max) | 1 for k in range(T)]
    return [_values(kind, rs, (n, d), k + 1) for k, n in enumerate(ns)], ns


def _equivariant(R, Rs, d, s, F=None, x_only=False):
    """R_s[:, d:] == 2^(2s) R[:, d:] (x_only: x pairs 2^s, row x row pairs unchanged), x columns 2^s x, bitwise."""
    f = np.float32(2.0 ** s)
    assert np.array_equal(Rs[:, :d].view(np.uint32), (R[:, :d] * f).view(np.uint32)), "x columns under 2^%d" % s
    if not x_only:
        want = R[:, d:] * f * f
        assert np.array_equal(Rs[:, d:].view(np.uint32), want.view(np.uint32)), "pairs are not 2^(2s) times (s = %d)" % s
        return
    li, lj = acc.pair_index(F, False)
    xp, rr = d + np.nonzero(lj == 0)[0], d + np.nonzero(lj != 0)[0]
    assert np.array_equal(Rs[:, xp].view(np.uint32), (R[:, xp] * f).view(np.uint32)), "x pairs under 2^%d" % s
    assert np.array_equal(Rs[:, rr].view(np.uint32), R[:, rr].view(np.uint32)), "row x row pairs moved under 2^%d" % s


# ------------------------------------------------------------------------------------------- interact_features, dense
@pytest.mark.parametrize("d", [16, 32, 36, 48, 64, 128])
@pytest.mark.parametrize("F", [2, 16, 17, 27, 28, 29, 32])
def test_interact_features_dense(E, d, F):
    """aligned dense features, B >= the tile threshold: emb_interact_rf_kernel (F <= 28, d in 16 / 32 / 36 / 64),
    emb_interact_dot_lds_kernel otherwise"""
    B = 2048 + 37
    kernel = "emb_interact_rf_kernel" if F <= 28 and d in (16, 32, 36, 64) else "emb_interact_dot_lds_kernel"
    rs = np.random.RandomState(d * 100 + F)
    rows = acc.sample_rows(B, seed=F)
    for kind in KINDS:
        x = _values(kind, rs, (B, d), 0)
        feats = [_values(kind, rs, (B, d), j + 1) for j in range(F - 1)]
        for itself in (False, True):
            R = E.interact_features(_dev(x), [_dev(f) for f in feats], "dot", itself).cpu().numpy()
            case = "dense d=%d F=%d itself=%d %s" % (d, F, itself, kind)
            acc.check(R[rows], _ref_dense(x, feats, rows, itself), case, kernel, rows)
            if kind != "dlrm":
                continue
            for s in S:
                f = np.float32(2.0 ** s)
                Rs = E.interact_features(_dev(x * f), [_dev(v * f) for v in feats], "dot", itself).cpu().numpy()
                acc.check(Rs[rows], _ref_dense(x * f, [v * f for v in feats], rows, itself), case + " scaled 2^%d" % s, kernel, rows)
                _equivariant(R, Rs, d, s)


def _interact(E, x, feats, itself):
    """interact_features; past 32 features (which the extension refuses) the C ABI's evs_interact_dot itself"""
    if len(feats) + 1 <= 32:
        return E.interact_features(x, feats, "dot", itself)
    import ctypes as C
    fs = [x] + list(feats)
    B, d, F = int(x.shape[0]), int(x.shape[1]), len(fs)
    P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    R = torch.empty((B, d + P), dtype=torch.float32, device="cuda")
    ptrs = (C.c_void_p * F)(*[f.data_ptr() for f in fs])
    strides = (C.c_int64 * F)(*[int(f.stride(0)) for f in fs])
    E._lib.check(E._lib.lib().evs_interact_dot(B, F, d, ptrs, strides, int(itself), R.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream))
    return R


@pytest.mark.parametrize("F,d,misaligned", [(33, 36, False), (40, 16, False), (33, 10, False), (40, 20, False), (33, 256, False),
                                            (17, 10, False), (27, 20, False), (9, 256, False), (27, 36, True)])
def test_interact_features_generic(E, F, d, misaligned):
    """F > 32, d outside the fused set, or a feature that is not 16-byte aligned: interact_dot_generic_kernel"""
    B = 777
    rs = np.random.RandomState(F * 1000 + d)
    rows = np.arange(B)
    for kind in KINDS:
        if kind == "cancel" and d % 2:
            continue
        x = _values(kind, rs, (B, d), 0)
        feats = [_values(kind, rs, (B, d), j + 1) for j in range(F - 1)]
        dev = [_dev(f) for f in feats]
        if misaligned:   # feature 5 as a view 4 bytes into a wider buffer
            buf = torch.zeros((B, d + 1), device="cuda")
            buf[:, 1:] = dev[5]
            dev[5] = buf[:, 1:]
            assert dev[5].data_ptr() % 16 != 0
        for itself in (False, True):
            R = _interact(E, _dev(x), dev, itself).cpu().numpy()
            case = "generic F=%d d=%d%s itself=%d %s" % (F, d, " misaligned" if misaligned else "", itself, kind)
            acc.check(R, _ref_dense(x, feats, rows, itself), case, "interact_dot_generic_kernel", rows)


# ------------------------------------------------------------------------------------------ apply_emb_interact, fp32
def _stacked_indices(rs, ns, B, mode):
    """-> (lS_o (T, B) or None, lS_i (T, N), bag lengths (T, B)).  ragged: B indices per table (a stacked tensor) thrown
    into B bags at random -- empty bags and bags of several indices: the offsets bet lost."""
    T = len(ns)
    if mode != "ragged":
        idx = np.stack([rs.randint(0, n, B) for n in ns]).astype(np.int64)
        idx[:, -1] = np.array(ns) - 1
        idx[:, 0] = 0
        lens = np.ones((T, B), np.int64)
        return (None if mode == "bag1" else np.tile(np.arange(B), (T, 1))), idx, lens
    lens = np.stack([np.bincount(rs.randint(0, B, B), minlength=B) for _ in range(T)]).astype(np.int64)
    off = np.concatenate([np.zeros((T, 1), np.int64), np.cumsum(lens, 1)[:, :-1]], 1)
    idx = np.stack([rs.randint(0, n, B) for n in ns]).astype(np.int64)
    return off, idx, lens


def _pooled_ref(x, tabs, off, idx, rows, itself, weights=None):
    """Reference over the sampled rows of stacked / list indices (off None: one index per bag)."""
    if off is not None:
        return acc.reference_from_bags(x, tabs, off, idx, itself, weights, rows)
    feats = [_sub(t[np.asarray(idx[k])[rows]]) for k, t in enumerate(tabs)]
    return acc.Reference(x[rows], feats, itself)


@pytest.mark.parametrize("mode", ["bag1", "offsets", "ragged"])
@pytest.mark.parametrize("B,d", [(1, 36), (15, 36), (16, 36), (17, 36), (16384, 36), (16385, 36), (16384, 32), (16385, 32)])
def test_apply_emb_interact_fp32(E, mode, B, d):
    """one index per bag declared: emb_interact_rf_kernel (F <= 28, B from the tile threshold up to rf_max_batch),
    emb_interact_dot_lds_kernel (small B, F > 28, d = 32 past rf_max_batch); lS_o given: the rf CHECK form; ragged bags
    (the offsets bet lost): the general loop"""
    Fs = [16, 17, 27, 28, 29, 32] if B < 1000 else [17, 27, 29]
    for F in Fs:
        T = F - 1
        if mode == "bag1":
            kernel = "emb_interact_rf_kernel" if (B >= 2048 and F <= 28 and (d != 32 or B <= 16384)) else "emb_interact_dot_lds_kernel"
        else:
            kernel = "emb_interact_rf_kernel (CHECK)" if (mode == "offsets" and B >= 2048 and F <= 28) else "emb_interact_dot_lds_kernel"
        rs = np.random.RandomState(B + F + d)
        rows = acc.sample_rows(B, seed=F)
        for kind in KINDS:
            tabs, ns = _tables(kind, rs, T, d)
            ev = E.EVTables.from_fp32([torch.from_numpy(t) for t in tabs])
            off, idx, lens = _stacked_indices(rs, ns, B, mode)
            x = _values(kind, rs, (B, d), 0)
            o = None if off is None else _dev(off)
            R = E.apply_emb_interact(_dev(x), o, _dev(idx), ev, check_indices=True, one_index_per_bag=(mode == "bag1")).cpu().numpy()
            case = "apply_emb_interact %s B=%d F=%d d=%d %s" % (mode, B, F, d, kind)
            acc.check(R[rows], _pooled_ref(x, tabs, off, idx, rows, False), case, kernel, rows)
            if kind != "dlrm":
                continue
            for s in S:
                f = np.float32(2.0 ** s)
                evs = E.EVTables.from_fp32([torch.from_numpy(t * f) for t in tabs])
                Rs = E.apply_emb_interact(_dev(x * f), o, _dev(idx), evs, one_index_per_bag=(mode == "bag1")).cpu().numpy()
                acc.check(Rs[rows], _pooled_ref(x * f, [t * f for t in tabs], off, idx, rows, False), case + " 2^%d" % s, kernel, rows)
                _equivariant(R, Rs, d, s)


# ------------------------------------------------------------------------------------------------------- multi-hot
def _list_bags(rs, ns, B, lo, hi):
    lens = [rs.randint(lo, hi + 1, B) for _ in ns]
    off = [np.concatenate([[0], np.cumsum(l)[:-1]]).astype(np.int64) for l in lens]
    idx = [rs.randint(0, n, int(l.sum())).astype(np.int64) for n, l in zip(ns, lens)]
    return off, idx


@pytest.mark.parametrize("d,T,B,lo,hi", [(36, 26, 2100, 2, 40), (16, 8, 300, 2, 40), (64, 5, 2049, 2, 40), (32, 27, 513, 2, 40),
                                          (36, 26, 2100, 1, 2), (16, 8, 300, 1, 2), (64, 5, 2049, 1, 2)])
def test_multi_hot_list_form(E, d, T, B, lo, hi):
    """multi-hot bags in list form, fp32, pooled by the gather kernels then the dense interaction: bags of 2 - 40 (from an
    average of 2 indices per bag) bag_sum_long_kernel, bags of 1 - 2 bag_sum_flat_kernel"""
    kernel = "bag_sum_long_kernel + interaction" if lo >= 2 else "bag_sum_flat_kernel + interaction"
    rs = np.random.RandomState(d + T + lo)
    rows = acc.sample_rows(B, seed=T)
    for kind in KINDS:
        tabs, ns = _tables(kind, rs, T, d)
        ev = E.EVTables.from_fp32([torch.from_numpy(t) for t in tabs])
        off, idx = _list_bags(rs, ns, B, lo, hi)
        x = _values(kind, rs, (B, d), 0)
        R = E.apply_emb_interact(_dev(x), [_dev(v) for v in off], [_dev(v) for v in idx], ev, check_indices=True).cpu().numpy()
        case = "multi-hot bags %d-%d d=%d T=%d B=%d %s" % (lo, hi, d, T, B, kind)
        acc.check(R[rows], _pooled_ref(x, tabs, off, idx, rows, False), case, kernel, rows)
        if kind != "dlrm":
            continue
        for s in S:
            f = np.float32(2.0 ** s)
            evs = E.EVTables.from_fp32([torch.from_numpy(t * f) for t in tabs])
            Rs = E.apply_emb_interact(_dev(x * f), [_dev(v) for v in off], [_dev(v) for v in idx], evs).cpu().numpy()
            _equivariant(R, Rs, d, s)


@pytest.mark.parametrize("codec,d", [(32, 36), (32, 16), (32, 64), (8, 36), (16, 32), (4, 16)])
def test_weighted_bags_itself(E, orc, codec, d):
    """bags of 0 - 12 with itself, list form: the general loops -- weighted fp32 rows (weighted pooling is built for fp32
    tables only): emb_interact_dot_lds_kernel, unweighted encoded rows: emb_interact_dot_lds_kernel<CODEC>"""
    T, B = 9, 700
    rs = np.random.RandomState(codec + d)
    kernel = "emb_interact_dot_lds_kernel" if codec == 32 else "emb_interact_dot_lds_kernel<%d>" % codec
    rows = np.arange(B)
    for kind in KINDS:
        tabs, ns = _tables(kind, rs, T, d, 500)
        if codec != 32:
            raws = [orc.encode_table(np.clip(t, -1, 1), codec) for t in tabs]
            tabs = [orc.decode(r, codec, d) for r in raws]
            ev = E.EVTables([_dev(r) for r in raws], d, codec)
        else:
            ev = E.EVTables.from_fp32([torch.from_numpy(t) for t in tabs])
        wts = [(_values("samesign" if kind == "samesign" else "unit", rs, (n,), 1) * 2).astype(np.float32) for n in ns] \
            if codec == 32 else None
        off, idx = _list_bags(rs, ns, B, 0, 12)
        x = _values(kind, rs, (B, d), 0)
        R = E.apply_emb_interact(_dev(x), [_dev(v) for v in off], [_dev(v) for v in idx], ev,
                                 None if wts is None else [_dev(w) for w in wts], True, check_indices=True).cpu().numpy()
        case = "weighted codec=%d d=%d %s" % (codec, d, kind)
        acc.check(R, _pooled_ref(x, tabs, off, idx, rows, True, wts), case, kernel, rows)
        if kind != "dlrm" or codec != 32:
            continue
        for s in S:
            f = np.float32(2.0 ** s)
            Rs = E.apply_emb_interact(_dev(x * f), [_dev(v) for v in off], [_dev(v) for v in idx], ev,
                                      [_dev(w * f) for w in wts], True).cpu().numpy()
            _equivariant(R, Rs, d, s)


# ------------------------------------------------------------------------------------------ apply_emb_interact_multi
@pytest.mark.parametrize("K", [3, 9])
def test_apply_emb_interact_multi(E, K):
    """K batches in one launch: the rf multi-grid"""
    d, T, B = 36, 26, 2048 + 5
    rs = np.random.RandomState(K)
    rows = acc.sample_rows(B, 1024, seed=K)
    for kind in KINDS:
        tabs, ns = _tables(kind, rs, T, d)
        ev = E.EVTables.from_fp32([torch.from_numpy(t) for t in tabs])
        xs = [_values(kind, rs, (B, d), 0) for _ in range(K)]
        idxs = [_stacked_indices(rs, ns, B, "bag1")[1] for _ in range(K)]
        Rs = E.apply_emb_interact_multi([_dev(x) for x in xs], None, [_dev(i) for i in idxs], ev, one_index_per_bag=True)
        for k in range(K):
            case = "multi K=%d batch %d %s" % (K, k, kind)
            acc.check(Rs[k].cpu().numpy()[rows], _pooled_ref(xs[k], tabs, None, idxs[k], rows, False), case, "emb_interact_rf_kernel (multi)", rows)


# ------------------------------------------------------------------------------------------------- reduced precision
@pytest.mark.parametrize("codec", [16, 8, 4])
@pytest.mark.parametrize("d,F", [(16, 9), (16, 27), (32, 9), (32, 27), (36, 9), (36, 27), (36, 17), (64, 27)])
def test_reduced_precision(E, orc, codec, d, F):
    """one index per bag declared and lS_o given: emb_interact_rfq_kernel (d in 16 / 32 / 36; u8 at d = 36, F > 16: the
    integer pipe, I8), emb_interact_dot_lds_kernel<CODEC> at d = 64"""
    T, B = F - 1, 1000 + 3
    i8 = codec == 8 and d == 36 and F > 16
    kernel = "emb_interact_rfq_kernel%s" % (" (I8)" if i8 else "") if d != 64 else "emb_interact_dot_lds_kernel<%d>" % codec
    rs = np.random.RandomState(codec * 7 + d + F)
    dec = _decode_all(orc, codec)
    rows = np.arange(B)
    for kind in KINDS:
        ns = [max(min(KAGGLE_LN[k % 26], 400), 7) | 1 for k in range(T)]
        codes = [_codes(orc, codec, kind, rs, (n, d), k + 1) for k, n in enumerate(ns)]
        if codec == 8 and kind == "unit":   # the extreme codes, and rows of one code (0, 127, 128, 254, 255) as rows 0..4
            for c in codes:
                c[:5] = np.array([0, 127, 128, 254, 255])[:, None]
                c[5:] = np.where(rs.rand(*c[5:].shape) < 0.2, rs.choice([0, 127, 128, 254, 255], c[5:].shape), c[5:])
        raws = [_raw(codec, c) for c in codes]
        tabs = [orc.decode(r, codec, d) for r in raws]
        assert all(np.array_equal(t, dec[c].astype(np.float32)) for t, c in zip(tabs, codes))
        ev = E.EVTables([_dev(r) for r in raws], d, codec)
        x = _values("unit" if kind == "unit" else kind, rs, (B, d), 0)
        _, idx, _ = _stacked_indices(rs, ns, B, "bag1")
        if codec == 8 and kind == "unit":
            idx[:, :40] = np.arange(40) % 5
        xd, idd = _dev(x), _dev(idx)
        off = torch.arange(B, device="cuda").repeat(T, 1)
        for mode in ("bag1", "offsets"):
            R = E.apply_emb_interact(xd, None if mode == "bag1" else off, idd, ev, check_indices=True,
                                     one_index_per_bag=(mode == "bag1")).cpu().numpy()
            feats = [_sub(tabs[k][idx[k]]) for k in range(T)]
            cc = np.stack([codes[k][idx[k]] for k in range(T)], 1)   # (B, T, d) the codes behind the rows
            ref = acc.Reference(x, feats, False, 1, acc.u8_delta()[cc] if i8 else None, cc)
            case = "codec %d d=%d F=%d %s %s" % (codec, d, F, mode, kind)
            acc.check(R, ref, case, kernel, rows)
            if kind != "dlrm" or mode != "bag1":
                continue
            for s in S:
                Rs = E.apply_emb_interact(xd * float(2.0 ** s), None, idd, ev, one_index_per_bag=True).cpu().numpy()
                _equivariant(R, Rs, d, s, F, x_only=True)


# ------------------------------------------------------------------------------------------------ cache-tier consumers
@pytest.mark.parametrize("policy,codec", [("setassoc", 32), ("sampled", 32), ("plan", 32), ("setassoc", 8)])
def test_cache_lookup_interact(E, orc, policy, codec):
    """GpuCache.lookup_interact: rf PROBE (set-associative fp32 tier), rf IDS (sampled / plan), rfq PROBE (u8 tier); the
    reference is float64 over the table rows served"""
    T, d, B = 26, 36, 600
    kernel = {("setassoc", 32): "emb_interact_rf_kernel (PROBE)", ("sampled", 32): "emb_interact_rf_kernel (IDS)",
              ("plan", 32): "emb_interact_rf_kernel (IDS)", ("setassoc", 8): "emb_interact_rfq_kernel (PROBE)"}[(policy, codec)]
    rs = np.random.RandomState(len(policy) + codec)
    rows = np.arange(B)
    for kind in KINDS:
        ns = [min(n, 2000) | 1 for n in KAGGLE_LN]
        if codec == 32:
            tabs = [_values(kind, rs, (n, d), k + 1) for k, n in enumerate(ns)]
            backing = [_dev(t) for t in tabs]
        else:
            raws = [_raw(8, _codes(orc, 8, kind, rs, (n, d), k + 1)) for k, n in enumerate(ns)]
            tabs = [orc.decode(r, 8, d) for r in raws]
            backing = [_dev(r) for r in raws]
        c = E.GpuCache("evlfu", 4000, T, d, codec, "python").set_batch_policy(policy)
        c.set_backing(backing)
        for it in range(3):
            hot = rs.rand(B, T) < 0.5
            rq = np.where(hot, rs.randint(0, 3, (B, T)), np.stack([rs.randint(0, n, B) for n in ns], 1)).astype(np.int32)
            x = _values(kind, rs, (B, d), 0)
            _, R = c.lookup_interact(_dev(rq), _dev(x), itself=bool(it & 1))
            R = R.cpu().numpy()
            ref = acc.Reference(x, [_sub(tabs[k][rq[:, k]]) for k in range(T)], bool(it & 1))
            if codec == 8:
                cc = np.stack([np.asarray(raws[k])[rq[:, k]] for k in range(T)], 1).astype(np.int64)
                ref = acc.Reference(x, [_sub(tabs[k][rq[:, k]]) for k in range(T)], bool(it & 1), 1, acc.u8_delta()[cc], cc)
            acc.check(R, ref, "cache %s codec %d it %d %s" % (policy, codec, it, kind), kernel, rows)
        assert c.batch_stats()["n_hits"] > 0


@pytest.mark.parametrize("policy,codecs", [("sampled", (8, 4)), ("plan", (8, 4)), ("sampled", (32, 8)), ("plan", (32, 4))])
def test_cache_lookup_interact_c1c2(E, orc, policy, codecs):
    """lookup_interact_c1c2 over two tiers: interact_mixed84_kernel for (u8, u4) (the probe folded in),
    interact_mixed_rows_kernel for the other pairs.  The tier that serves a miss is the routing's choice, so the rows hold values both codecs
    decode exactly (-1, 0, 1: the row x row pairs are exact integers) and x carries the arithmetic of the x pairs."""
    from evstore_dlrm_amd import gpu_cache
    T, d, B = 26, 36, 400
    rs = np.random.RandomState(len(policy))
    kernel = "interact_mixed84_kernel" if codecs == (8, 4) else "interact_mixed_rows_kernel"
    rows = np.arange(B)
    for kind in KINDS:
        if kind == "cancel":   # even rows (v, v), odd rows (v, -v) over {-1, 0, 1}; x even: x x odd row is exactly 0
            ws = [np.repeat(rs.randint(-1, 2, (300, d // 2)), 2, 1).astype(np.float32) for _ in range(T)]
            for k in range(0, T, 2):
                ws[k][:, 1::2] *= -1
        else:
            lo = 0 if kind == "samesign" else -1
            ws = [rs.randint(lo, 2, (300, d)).astype(np.float32) for _ in range(T)]
        raws = {c: [orc.encode_table(w, c) for w in ws] for c in codecs}
        c1 = E.GpuCache("evlfu", 400, T, d, codecs[0], "cpp").set_batch_policy(policy)
        c2 = E.GpuCache("evlfu", 900, T, d, codecs[1], "cpp").set_batch_policy(policy)
        c1.set_backing([_dev(a) for a in raws[codecs[0]]])
        c2.set_backing([_dev(a) for a in raws[codecs[1]]])
        for it in range(4):
            hot = rs.rand(B, T) < 0.7
            rq = np.where(hot, rs.randint(0, 12, (B, T)), rs.randint(0, 300, (B, T))).astype(np.int32)
            x = _values(kind, rs, (B, d), 0)
            _, R = gpu_cache.lookup_interact_c1c2(c1, c2, _dev(rq), _dev(x), itself=bool(it & 1))
            ref = acc.Reference(x, [_sub(ws[k][rq[:, k]]) for k in range(T)], bool(it & 1))
            acc.check(R.cpu().numpy(), ref, "c1c2 %s %s it %d %s" % (policy, codecs, it, kind), kernel, rows)


# ------------------------------------------------------------------------------------------------------- full size
def test_bench_data_full_size(E):
    """The bench's own tables and batches at B = 16 384 through the headline launch (one index per bag declared) and the
    lS_o-given launch; 1 024 sampled rows against float64."""
    from bench import KAGGLE_LN as LN, make_batches, make_tables
    d, B = 36, 16384
    ev = make_tables(LN, d, seed=0)
    (off, idx), = make_batches(LN, B, 1, seed=29, device="cuda")
    torch.manual_seed(2)
    x = torch.rand((B, d), device="cuda")
    rows = acc.sample_rows(B, 1024, seed=3)
    rt = torch.from_numpy(rows).cuda()
    feats = [_sub(ev.fp32_view(k)[idx[k, rt]].cpu().numpy()) for k in range(26)]
    ref = acc.Reference(x[rt].cpu().numpy(), feats, False)
    a = E.apply_emb_interact(x, None, idx, ev, one_index_per_bag=True)
    b = E.apply_emb_interact(x, off, idx, ev, check_indices=True)
    acc.check(a[rt].cpu().numpy(), ref, "bench data, one index per bag", "emb_interact_rf_kernel", rows)
    acc.check(b[rt].cpu().numpy(), ref, "bench data, lS_o given", "emb_interact_rf_kernel (CHECK)", rows)
