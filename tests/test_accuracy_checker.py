"""The accuracy checker of tests/_accuracy.py has teeth (CPU only): honest fp32 evaluations of the interaction pass it,
at unit scale and at the scale of DLRM's own tables; each way of being subtly wrong fails the check named for it.
This is what makes the GPU sweep (tests/test_gpu_accuracy.py) trustworthy from a machine without a GPU."""
import numpy as np
import pytest

import _accuracy as acc
from oracle import oracle as orc

D, N = 36, 384


def _kaggle_ln():
    from bench import KAGGLE_LN
    return KAGGLE_LN


def _inputs(scale, d=D, n=N, seed=0):
    """x (n, d), 26 features (n, d), one row per bag: "unit" U(-1, 1); "kaggle" rows U(+-sqrt(1/n_k)) over the Kaggle
    cardinalities, x ~ randn (as the full-size test draws it); "kaggle_relu" the same rows, x >= 0 around 0.1."""
    rs = np.random.RandomState(seed)
    if scale == "unit":
        return (rs.uniform(-1, 1, (n, d)).astype(np.float32),
                [rs.uniform(-1, 1, (n, d)).astype(np.float32) for _ in range(26)])
    fs = [rs.uniform(-1, 1, (n, d)).astype(np.float32) * np.float32(np.sqrt(1.0 / m)) for m in _kaggle_ln()]
    if scale == "kaggle":
        x = rs.randn(n, d).astype(np.float32)
    else:
        x = (np.maximum(rs.randn(n, d), 0) * 0.1).astype(np.float32)
    return x, fs


def _ref(x, fs, itself=False):
    return acc.Reference(x, [acc.pool64(f)[:2] for f in fs], itself)


def _mfma_order(d):
    """k in the order the f32 MFMA chain of the rows-in-registers kernels consumes it: instruction t takes element t of
    each of the four k-slots (slot q owns 4 d // 16 consecutive elements, the 4-element tail chunks one element each)."""
    cq, rem = d // 16, (d % 16) // 4
    main = [4 * cq * q + t for t in range(4 * cq) for q in range(4)]
    tail = [16 * cq + 4 * t + q for t in range(rem) for q in range(4)]
    return np.array(main + tail)


def _chain(T, itself, order, terms=None):
    """fp32 fma chain over k in `order` for every pair (emulated: the exact product plus the fp32 accumulator, rounded
    to fp32 once).  terms(a, b) -> list of (a', b') operand pairs fed per k (default: the operands themselves)."""
    n, F, d = T.shape
    li, lj = acc.pair_index(F, itself)
    a, b = T[:, li, :], T[:, lj, :]
    parts = [(a, b)] if terms is None else terms(a, b)
    s = np.zeros(a.shape[:2], np.float32)
    for k in order:
        for pa, pb in parts:
            s = (s.astype(np.float64) + pa[..., k].astype(np.float64) * pb[..., k].astype(np.float64)).astype(np.float32)
    return np.concatenate([T[:, 0, :], s], 1)


def _tile(x, fs):
    return np.ascontiguousarray(np.stack([x] + list(fs), 1), np.float32)


def _round_mantissa(a, bits):
    """round-to-nearest-even to `bits` explicit mantissa bits (tf32: 10, bf16: 7)"""
    u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
    sh = 23 - bits
    u = (u + ((1 << (sh - 1)) - 1) + ((u >> sh) & 1)) & ~np.uint64((1 << sh) - 1)
    return u.astype(np.uint32).view(np.float32)


def _bf16x3(a, b):
    ah, bh = _round_mantissa(a, 7), _round_mantissa(b, 7)
    al, bl = _round_mantissa(a - ah, 7), _round_mantissa(b - bh, 7)
    return [(al, bh), (ah, bl), (ah, bh)]


def _exact_from(T, itself):
    """R from float64 dot products of the fp32 tile T, rounded once (the orc.interact_features arithmetic)."""
    n, F, d = T.shape
    li, lj = acc.pair_index(F, itself)
    T64 = T.astype(np.float64)
    Z = np.matmul(T64, T64.transpose(0, 2, 1))[:, li, lj]
    return np.concatenate([T[:, 0, :], Z.astype(np.float32)], 1)


SCALES = ["unit", "kaggle", "kaggle_relu"]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("itself", [False, True])
def test_honest_fp32_evaluations_pass(scale, itself):
    x, fs = _inputs(scale)
    ref = _ref(x, fs, itself)
    T = _tile(x, fs)
    e1 = acc.check(orc.interact_features(x, fs, itself, f32chain=True), ref, "f32chain " + scale, "oracle")
    e2 = acc.check(_chain(T, itself, _mfma_order(D)), ref, "mfma order " + scale, "emulation")
    e3 = acc.check(orc.interact_features(x, fs, itself), ref, "double " + scale, "oracle")
    assert e3["median"] <= 0.5 and e3["worst"] <= 1.0 / ref.K + 1e-12   # one rounding of the exact value: <= u |R64| / 2
    assert e1["median"] < 2.5 and e2["median"] < 2.5


def test_same_sign_data_is_the_largest_honest_error():
    """Same-sign data at d = 128: the chain's errors all point one way; still within the cap (the emulation gives ~1.8)."""
    rs = np.random.RandomState(3)
    d = 128
    x = rs.uniform(0, 1, (128, d)).astype(np.float32)
    fs = [rs.uniform(0, 1, (128, d)).astype(np.float32) for _ in range(15)]
    e = acc.check(_chain(_tile(x, fs), False, _mfma_order(d)), _ref(x, fs), "same sign d=128", "emulation")
    assert 1.0 < e["median"] <= acc.CAP


@pytest.mark.parametrize("scale", SCALES)
def test_tf32_operands_fail_the_hard_bound(scale):
    x, fs = _inputs(scale)
    T = _round_mantissa(_tile(x, fs), 10)
    R = _exact_from(T, False)
    R[:, :D] = x
    e = acc.evaluate(R, _ref(x, fs))
    assert not e["hard_ok"] and not e["cap_ok"] and e["median"] > 100


@pytest.mark.parametrize("scale", SCALES)
def test_bf16x3_split_fails_the_hard_bound_and_the_cap(scale):
    x, fs = _inputs(scale)
    R = _chain(_tile(x, fs), False, _mfma_order(D), _bf16x3)
    e = acc.evaluate(R, _ref(x, fs))
    assert not e["hard_ok"], e
    assert not e["cap_ok"], e


@pytest.mark.parametrize("scale", SCALES)
def test_one_dropped_k_element_fails_the_hard_bound(scale):
    x, fs = _inputs(scale)
    T = _tile(x, fs)
    T2 = T.copy()
    T2[:, 1:, D - 1] = 0   # (the tail element of the rows lost; x kept: the x columns still pass)
    R = _exact_from(T2, False)
    R[:, :D] = x
    e = acc.evaluate(R, _ref(x, fs))
    assert e["x_ok"] and not e["hard_ok"]


@pytest.mark.parametrize("scale", SCALES)
def test_two_swapped_pair_columns_fail_the_hard_bound(scale):
    x, fs = _inputs(scale)
    ref = _ref(x, fs)
    R = _chain(_tile(x, fs), False, _mfma_order(D))
    assert acc.evaluate(R, ref)["hard_ok"]
    R[:, [D + 40, D + 200]] = R[:, [D + 200, D + 40]]
    e = acc.evaluate(R, ref)
    assert e["x_ok"] and not e["hard_ok"]


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("col", [0, 7, 150, 350])
def test_one_pair_column_of_zeros_fails_the_hard_bound(scale, col):
    """Under the old rtol 1e-5 / atol 2e-6 a column of small outputs written as zeros passes at DLRM scale; not here."""
    x, fs = _inputs(scale)
    ref = _ref(x, fs)
    R = _chain(_tile(x, fs), False, _mfma_order(D))
    R[:, D + col] = 0
    e = acc.evaluate(R, ref)
    assert e["x_ok"] and not e["hard_ok"]


def test_the_old_tolerance_lets_a_zeroed_column_through_at_dlrm_scale():
    """The gap this checker closes: the same zeroed column, against the double oracle with rtol 1e-5, atol 1e-5."""
    x, fs = _inputs("kaggle_relu")
    R = _chain(_tile(x, fs), False, _mfma_order(D))
    Ro = orc.interact_features(x, fs)
    small = int(np.argmin(np.abs(Ro[:, D:]).max(0)))
    R[:, D + small] = 0
    np.testing.assert_allclose(R, Ro, rtol=1e-5, atol=1e-5)
    assert not acc.evaluate(R, _ref(x, fs))["hard_ok"]


def test_mutations_at_unit_scale_are_caught_by_the_old_check_too():
    """(sanity of the emulations: the old check was sharp on unit-scale data)"""
    x, fs = _inputs("unit")
    R = _chain(_tile(x, fs), False, _mfma_order(D))
    R[:, D + 7] = 0
    with pytest.raises(AssertionError):
        np.testing.assert_allclose(R, orc.interact_features(x, fs), rtol=1e-5, atol=2e-6)


def _u8_case(codes_rows, x, F):
    """x and F - 1 u8 features with the given (n, F - 1, d) codes; -> (x, decoded features, codes)."""
    dec = acc.dec_u8_values().astype(np.float32)[codes_rows]
    return [np.ascontiguousarray(dec[:, k]) for k in range(F - 1)]


def _u8_affine(x, codes):
    """What the u8 integer-pipe path computes: row x row = fl(N fl(1/127^2)), N = sum (c_i - 127)(c_j - 127) exact;
    x x row = sum x fl(1/127) ((c - 128) + 1) as the kernel folds it (one fp32 chain over the 36 elements)."""
    n, T, d = codes.shape
    s = codes.astype(np.int64) - 128
    F = T + 1
    li, lj = acc.pair_index(F, False)
    rz = np.float32(1.0 / 16129.0)
    r127 = np.float32(1.0 / 127.0)
    Z = np.zeros((n, len(li)), np.float32)
    xs = (x * r127).astype(np.float32)
    for p, (i, j) in enumerate(zip(li, lj)):
        if j == 0:
            t = xs.sum(1, dtype=np.float32)
            for k in range(d):
                t = (t.astype(np.float64) + xs[:, k].astype(np.float64) * s[:, i - 1, k]).astype(np.float32)
            Z[:, p] = t
        else:
            N = ((s[:, i - 1] + 1) * (s[:, j - 1] + 1)).sum(1)
            Z[:, p] = (N.astype(np.float32) * rz).astype(np.float32)
    return np.concatenate([x, Z], 1)


def _u8_ref(x, codes, with_extra):
    fs = _u8_case(codes, x, codes.shape[1] + 1)
    delta = acc.u8_delta()[codes] if with_extra else None
    return acc.Reference(x, [acc.pool64(f)[:2] for f in fs], False, delta=delta, i8_codes=codes)


def test_u8_affine_result_needs_its_decoder_term():
    """Rows of constant code 128: the integer path's exact affine value sits ~15.7 u M from the reference decoder's --
    inside the hard bound, far over the distribution cap, unless the path's own term is given."""
    rs = np.random.RandomState(8)
    n, T = 256, 26
    codes = np.full((n, T, D), 128, np.int64)
    x = rs.uniform(-1, 1, (n, D)).astype(np.float32)
    R = _u8_affine(x, codes)
    e = acc.evaluate(R, _u8_ref(x, codes, False))
    assert e["hard_ok"] and not e["cap_ok"] and 12 < e["median"] < 20, e
    acc.check(R, _u8_ref(x, codes, True), "u8 affine, code 128", "emulation")


@pytest.mark.parametrize("kind", ["random", "extreme", "dlrm"])
def test_u8_affine_result_passes_with_its_term(kind):
    """The integer path on random codes, on the extreme codes (0, 127, 128, 254, 255 and constant rows, code-127 rows
    included: they decode to zeros, their x pair is the folded sum's residue) and on DLRM-scale codes (near 127)."""
    rs = np.random.RandomState(9)
    n, T = 256, 26
    if kind == "random":
        codes = rs.randint(0, 256, (n, T, D))
    elif kind == "extreme":
        codes = rs.choice([0, 127, 128, 254, 255], (n, T, D))
        for k, c in enumerate([0, 127, 128, 254, 255]):
            codes[k::5, k] = c
    else:
        codes = orc.encode(rs.uniform(-1, 1, (n, T, D)) * 0.03, 8)
    x = (np.maximum(rs.randn(n, D), 0) * 0.1).astype(np.float32) if kind == "dlrm" else rs.uniform(-1, 1, (n, D)).astype(np.float32)
    R = _u8_affine(x, codes)
    acc.check(R, _u8_ref(x, codes, True), "u8 affine " + kind, "emulation")
    if kind == "extreme":   # the x pair of a code-127 row is not exactly 0 in this arithmetic: the term is what admits it
        e = acc.evaluate(R, _u8_ref(x, codes, False))
        assert not e["zero_ok"] or not e["hard_ok"]


def test_zero_outputs_must_be_exact_and_x_bit_exact():
    x, fs = _inputs("unit", n=64)
    fs[3][:] = 0   # (an empty bag)
    ref = _ref(x, fs)
    R = orc.interact_features(x, fs)
    acc.check(R, ref, "zero feature", "oracle")
    li, lj = acc.pair_index(27, False)
    p = int(np.nonzero((li == 4) & (lj == 1))[0][0])
    R2 = R.copy()
    R2[5, D + p] = 1e-30
    assert not acc.evaluate(R2, ref)["zero_ok"]
    R3 = R.copy()
    R3[5, 3] = np.nextafter(R3[5, 3], np.float32(2))
    assert not acc.evaluate(R3, ref)["x_ok"]


def test_pooled_reference_and_the_bag_length_term():
    """pool64 over weighted multi-hot bags: the oracle's fp32 pooling (then its double interaction) is inside the bound
    with L = the longest bag, and the failure message names the case, the kernel and the worst element."""
    rs = np.random.RandomState(4)
    n, d, T = 200, 16, 5
    tabs = [rs.uniform(-1, 1, (50, d)).astype(np.float32) for _ in range(T)]
    lens = rs.randint(0, 12, (T, n))
    lS_o = [np.concatenate([[0], np.cumsum(l)[:-1]]).astype(np.int64) for l in lens]
    lS_i = [rs.randint(0, 50, l.sum()).astype(np.int64) for l in lens]
    vW = [rs.uniform(0, 2, 50).astype(np.float32) for _ in range(T)]
    x = rs.uniform(-1, 1, (n, d)).astype(np.float32)
    ly = orc.apply_emb(lS_o, lS_i, tabs, vW)
    feats, L = [], 0
    for k in range(T):
        v, a, l = acc.pool64(tabs[k][lS_i[k]], vW[k][lS_i[k]], lS_o[k], n)
        feats.append((v, a))
        L = max(L, l)
    assert L == 11
    ref = acc.Reference(x, feats, True, L)
    acc.check(orc.interact_features(x, ly, True), ref, "weighted bags", "oracle")
    R = orc.interact_features(x, ly, True)
    R[17, d + 0] *= 1.01
    with pytest.raises(AssertionError, match=r"weighted bags \[oracle\]: worst at sample 17 pair \(0, 0\)"):
        acc.check(R, ref, "weighted bags", "oracle")
