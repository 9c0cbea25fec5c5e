"""CPU: the generators of tests/test_gpu_mixed_matrix.py (tests/_mixed_matrix.py) cover what that module says they cover -- checked here so
that a change of a generator cannot quietly thin the GPU module out."""
import numpy as np
import pytest

import _mixed_matrix as MM


@pytest.mark.parametrize("d", MM.DIMS)
def test_the_decode_probe_reaches_every_code_at_every_position_in_both_halves(d):
    for codec, n_codes in ((8, 256), (4, 16)):
        for NT in (1, 2):
            codes = MM.probe_codes(d, codec, NT)
            B, T, dd = codes.shape
            assert dd == d and T == MM.PROBE_T[NT] and B % d == 0 and codes.min() >= 0 and codes.max() == n_codes - 1
            cov = MM.probe_coverage(codes, d, codec)
            assert len(cov) == NT and all(c.shape == (d, n_codes) and c.all() for c in cov), "a code is not probed at some position of a half"
            # the same over the rows' whole contents: every code at every element position of some row of each half
            for lo, hi in [(0, 15), (15, T)][:NT]:
                for c in range(d):
                    assert len(np.unique(codes[:, lo:hi, c])) == n_codes
            # a neighbour of the probed element never holds the probed code, and u4's NaN code stands at probed positions only
            b = np.arange(B)
            probed = codes[b, :, b % d]
            other = np.ones((B, T, d), bool)
            other[b, :, b % d] = False
            assert not (other & (codes == probed[:, :, None])).any()
            if codec == 4:
                assert not (other & (codes == 15)).any() and (probed == 15).any()


def test_the_case_lists_cover_the_matrix():
    names = set()
    total = 0
    for codecs in ((8, 4),) + MM.ROWS_PAIRS:
        for d in MM.DIMS:
            cs = MM.cases(codecs, d)
            total += len(cs)
            assert len({(c["T"], c["B"], c["itself"], c["pattern"]) for c in cs}) == len(cs), "a case is listed once"
            rand = [c for c in cs if c["pattern"] == "rand"]
            for c in rand:
                names.add((MM.kernel_name(c["T"], d, codecs), c["B"]))
            assert {c["T"] for c in cs} >= set(MM.KEY_T) and {c["itself"] for c in cs} == {0, 1}
            assert {c["pattern"] for c in cs} == set(MM.PATTERNS)
            assert any(c["x_stride"] > d for c in cs) and any(c["x_stride"] == d for c in cs)
            big = [c for c in cs if c["B"] == MM.BIG_B]
            assert all((d, c["T"]) in MM.BIG_AT for c in big)
            if codecs == (8, 4):
                assert {(c["T"], c["B"]) for c in rand} >= {(T, B) for T in range(1, 32) for B in MM.BATCHES}
                assert all({c["itself"] for c in rand if c["T"] == T and c["B"] == B} == {0, 1} for T in MM.KEY_T for B in MM.BATCHES)
                assert len(big) == sum(dd == d for dd, _ in MM.BIG_AT)
            if codecs in MM.SWEEP_PAIRS:
                assert {c["T"] for c in rand} == set(range(1, 32)) and len(big) == sum(dd == d for dd, _ in MM.BIG_AT)
    # every record name but the folded probe's, by a random-class case at each of B = 1, 17 and 67
    want = {(n, B) for n in MM.ALL_NAMES if not n.endswith("_probe") for B in (1, 17, 67)}
    assert want <= names, sorted(want - names)
    assert MM.BIG_B > 4 * 256 * 8, "past the grid cap of interact_mixed_rows_kernel for any occupancy <= 8"
    assert 1500 < total < 3000, total


def test_the_random_classes_hold_what_the_cases_ask_of_them():
    """zeros of both sorts in every sizeable draw (class 0; address 0 under a live class), and both classes in every half of 2 or 3 rows"""
    for T in range(1, 32):
        rs = np.random.RandomState(T)
        cls, dflt, null = MM.classes(rs, 67, T, "rand")
        assert cls.shape == null.shape == (67, T) and set(np.unique(cls)) <= {0, 1, 2} and not (null & (cls == 0)).any()
        if T >= 4:
            assert (cls == 0).any() and null.any()
        eff = np.where(null, 0, cls)
        shares = MM.both_classes_share(eff, T)
        for (lo, hi), share in zip(MM.HALVES(T), shares):
            assert (share is None) == (hi - lo < 2)
            if 2 <= hi - lo < 4:
                assert share == 1.0
            elif share is not None:
                assert share >= 0.5
    for p in MM.PATTERNS[1:]:
        cls, dflt, null = MM.classes(np.random.RandomState(0), 5, 7, p)
        assert not null.any() and dflt in (1, 2) and (cls is None) == p.startswith("d")


def test_the_dispatch_rule_of_the_names():
    assert MM.kernel_name(27, 36, (8, 4)) == "r84_d36_nt2" and MM.kernel_name(28, 36, (8, 4)) == "rows_d36_nt2"
    assert MM.kernel_name(15, 16, (8, 4)) == "r84_d16_nt1" and MM.kernel_name(16, 16, (8, 4)) == "r84_d16_nt2"
    assert MM.kernel_name(15, 32, (32, 8)) == "rows_d32_nt1" and MM.kernel_name(9, 32, (8, 4), rfq_on=False) == "rows_d32_nt1"
    assert len(MM.ALL_NAMES) == 18 == len(set(MM.ALL_NAMES))
