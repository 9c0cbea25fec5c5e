"""CPU: the case table of the fused first top-MLP layer (tests/_mlp1_matrix.py) covers what it claims, its cap is what the fp32
emulation measures, its checker has teeth, and the launcher's dispatch record (evs_mlp1_kernels_seen) parses in a fresh process.
This is what makes tests/test_gpu_mlp1_matrix.py trustworthy from a machine without a GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _mlp1_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_table_covers_every_edge_it_is_meant_to():
    assert len(set(M.CASES)) == len(M.CASES)
    sh = {c: M.shape(c) for c in M.CASES}
    for d, T, itself, n1, B in M.CASES:
        assert d in (16, 32, 36) and 1 <= T <= 27 and 1 <= n1 <= 512 and 1 <= B <= 300
    assert {s[5] for s in sh.values()} == set(M.NAMES), "all six instantiations"
    for d in (16, 32, 36):
        assert {16, 17} <= {sh[c][0] for c in M.CASES if c[0] == d}, "F = 16 and F = 17 at d = %d" % d
    nj = {s[4] for s in sh.values()}
    assert {2, 3, 4, 5, 6, 28} <= nj and {n % 5 for n in nj} == {0, 1, 2, 3, 4}
    assert sh[(16, 1, False, 1, 1)][2:5] == (17, 32, 2) and sh[(36, 7, False, 16, 16)][2:5] == (64, 64, 4)
    assert sh[(36, 26, False, 512, 293)][2:5] == (387, 400, 25) and sh[(36, 27, True, 80, 47)][2:5] == (442, 448, 28)
    assert {0, 15} <= {s[3] - s[2] for s in sh.values()}, "padding kp - K of 0 and of 15"
    assert max(s[3] for s in sh.values()) == 448
    assert {1, 15, 16, 17, 65, 80, 512} <= {c[3] for c in M.CASES}
    Bs = {c[4] for c in M.CASES}
    assert {1, 15, 16, 17, 33} <= Bs and any(200 <= b <= 300 and b % 16 for b in Bs)
    rows = [M.table_rows(c) for c in M.CASES]
    assert any(1 in r for r in rows) and all(1 <= n <= 500 for r in rows for n in r)
    assert M.SINGLE_ROW_CASE in M.CASES and M.SINGLE_ROW_CASE[4] > 1


def test_the_data_kinds_are_what_they_say():
    case = (32, 10, False, 65, 33)
    for kind in M.KINDS:
        x, tabs, idx, W, b = M.inputs(case, kind)
        x2, _, idx2, W2, _ = M.inputs(case, kind)
        assert np.array_equal(x, x2) and np.array_equal(idx, idx2) and np.array_equal(W, W2)
        assert W.shape == (65, 87) and b.shape == (65,) and W.dtype == b.dtype == x.dtype == np.float32 and idx.shape == (10, 33)
        assert not np.array_equal(W, M.inputs(case, kind, seed=1)[3])
    _, _, _, W, b = M.inputs(case, "samesign")
    assert (W > 0).all() and (b > 0).all()
    x, tabs, idx, W, b = M.inputs(case, "cancel")
    R = M.interact32(x, tabs, idx, False)
    Z64, Mz = M.reference(R, W, b)
    assert (Mz[:, 64] == 0).all() and (Mz[:, :64] > 0).all(), "the cancel kind carries one output with Mz == 0"
    _, _, _, W, _ = M.inputs(case, "dlrm")
    assert np.abs(W).min() >= np.sqrt(2.0 / (87 + 65)) / 64 * (1 - 1e-6)


@pytest.fixture(scope="module")
def honest():
    """(case, kind) -> (R, W, b, Z1 linear, Z1 relu) of the honest emulation, computed once"""
    out = {}
    for case in M.CASES:
        for kind in M.KINDS:
            x, tabs, idx, W, b = M.inputs(case, kind)
            R = M.interact32(x, tabs, idx, case[2])
            out[case, kind] = (R, W, b, M.emulate(R, W, b, False), M.emulate(R, W, b, True))
    return out


def test_the_honest_emulation_passes_and_the_cap_is_twice_its_largest_median(honest):
    worst = {k: (0.0, None) for k in M.KINDS}
    for (case, kind), (R, W, b, lin, rel) in honest.items():
        e = M.check(lin, R, W, b, False, M.case_id(case) + " " + kind, "emulation")
        M.check(rel, R, W, b, True, M.case_id(case) + " " + kind + " relu", "emulation")
        if e["median"] > worst[kind][0]:
            worst[kind] = (e["median"], case)
    for kind in M.KINDS:
        print("emulated median, %-8s %.4f at %s" % (kind, worst[kind][0], worst[kind][1]))
        assert worst[kind][1] == M.MEDIANS[kind][1] and abs(worst[kind][0] - M.MEDIANS[kind][0]) <= 0.005 * M.MEDIANS[kind][0], (kind, worst[kind])
    assert M.CAP == 2.0 * max(m for m, _ in M.MEDIANS.values()) and 1.8 < M.CAP < 1.95
    M.STATS.pop("emulation", None)


def _fails(case, kind, Z_lin, Z_relu, R, W, b):
    """the names of the checks the pair of outputs fails"""
    bad = set()
    for relu, Z in ((False, Z_lin), (True, Z_relu)):
        e = M.evaluate(Z, R, W, b, relu)
        bad |= {k for k in ("zero_ok", "hard_ok", "cap_ok") if not e[k]}
    return bad


FAULTS = ["tf32", "bf16", "dropped_piece", "bias_omitted", "stale_padding", "nonzero_padding", "stale_weight", "zeros"]


@pytest.mark.parametrize("fault", FAULTS)
def test_each_emulated_fault_fails_a_check(honest, fault):
    """Every way the kernel could be subtly wrong, at every case it can show at, fails at least one check on at least one kind (the
    honest emulation of the same case passes them all: the test above)."""
    hit = {}
    for case in M.CASES:
        F, P, K, kp, nj, name = M.shape(case)
        n1 = case[3]
        if fault == "bias_omitted" and n1 % 16 == 0:
            continue   # (no partial last tile)
        if fault in ("stale_padding", "nonzero_padding") and kp == K:
            continue   # (no padding columns)
        caught = {}
        for kind in M.KINDS:
            R, W, b, _, _ = honest[case, kind]
            kw, Wk = {}, W
            if fault in ("tf32", "bf16"):
                kw = {"bits": 10 if fault == "tf32" else 7}
            elif fault == "dropped_piece":
                kw = {"drop_last_piece": True}
            elif fault == "bias_omitted":
                kw = {"bias_until": 16 * (n1 // 16)}
            elif fault == "stale_padding":      # the A operand's padding columns hold what LDS held before: any bits at all
                kw = {"a_pad": np.inf}
            elif fault == "nonzero_padding":    # neither operand's padding zeroed
                kw = {"a_pad": 1.0, "w_pad": 1.0}
            elif fault == "stale_weight":       # the padded copy is of the weight before its last update
                Wk = M.inputs(case, kind, seed=1)[3]
            if fault == "zeros":
                Zl = Zr = np.zeros((R.shape[0], n1), np.float32)
            else:
                Zl, Zr = M.emulate(R, Wk, b, False, **kw), M.emulate(R, Wk, b, True, **kw)
            bad = _fails(case, kind, Zl, Zr, R, W, b)
            if bad:
                caught[kind] = sorted(bad)
        assert caught, "%s at %s passes every check on every kind" % (fault, M.case_id(case))
        hit[case] = caught
    assert hit
    if fault in ("tf32", "bf16"):   # reduced-precision operands fail on EVERY kind, hard bound and distribution both
        for case, caught in hit.items():
            if case[4] * case[3] >= 16:
                assert set(caught) == set(M.KINDS) and all("hard_ok" in v for v in caught.values()), (M.case_id(case), caught)


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_a_relu_that_turns_nan_into_zero_is_caught(honest, poison):
    """The rule the GPU test applies to a sample that read a NaN / +Inf table row: Z1 is NaN wherever float64 Linear + ReLU over its R
    is.  The ReLU written z > 0 ? z : 0 hides every one of them (with ReLU only); z <= 0 ? 0 : z hides none."""
    case = (32, 10, False, 65, 33)
    R, W, b, _, _ = honest[case, "unit"]
    R = R[20:21].copy()
    R[0, 40:44] = poison
    for relu in (False, True):
        hidden, n_nan = M.hidden_nans(M.emulate(R, W, b, relu), R, W, b, relu)
        assert n_nan >= 32 and len(hidden) == 0
        hidden, n_nan = M.hidden_nans(M.emulate(R, W, b, relu, nan_to_zero=True), R, W, b, relu)
        assert n_nan >= 32 and len(hidden) == (n_nan if relu else 0)
    hidden, n_nan = M.hidden_nans(M.emulate(honest[case, "unit"][0], W, b, True), honest[case, "unit"][0], W, b, True)
    assert n_nan == 0 and len(hidden) == 0


CHILD = r"""
import ctypes as C
import re
import sys
sys.path.insert(0, %r)
import evstore_dlrm_amd as E
L = E._lib.lib()
n = L.evs_mlp1_kernels_seen(None, 0)
buf = C.create_string_buffer(n + 1)
assert L.evs_mlp1_kernels_seen(buf, n + 1) == n and len(buf.value) == n
text = buf.value.decode()
assert text.endswith("\n") and all(re.fullmatch(r"[a-z0-9_]+=\d+", ln) for ln in text.splitlines()), text
short = C.create_string_buffer(b"x" * 64, 64)
assert L.evs_mlp1_kernels_seen(short, 30) == n and len(short.value) <= 29 and text.startswith(short.value.decode())
rec = E._lib.mlp1_kernels_seen()
want = ["mlp1_d%%d_nt%%d" %% (d, nt) for d in (16, 32, 36) for nt in (1, 2)]
assert [ln.split("=")[0] for ln in text.splitlines()] == want == list(rec), "the six names, each once, in the fixed order"
assert not any(rec.values()), "nothing has been launched yet"

EINVAL = E._lib.EVS_EINVAL
def call(B=4, T=26, d=36, itself=0, w1=16, kp=400, n1=8, x=16, xs=36):
    tabs = (C.c_void_p * 32)(*([16] * 32))
    nr = (C.c_int64 * 32)(*([5] * 32))
    return L.evs_emb_interact_mlp1_stacked(B, T, d, tabs, nr, x, xs, 16, B, itself, w1, kp, 16, n1, 1, 16, None, None)
assert call(d=64) == EINVAL and b"d=64" in L.evs_last_error()
assert call(T=28) == EINVAL and b"T=28" in L.evs_last_error()
assert call(T=0) == EINVAL and call(B=-1) == EINVAL
assert call(kp=384) == EINVAL and b"kp" in L.evs_last_error()
assert call(kp=416) == EINVAL and call(kp=387) == EINVAL
assert call(w1=20) == EINVAL and b"aligned" in L.evs_last_error()
assert call(x=20) == EINVAL and call(xs=38) == EINVAL
assert call(n1=0) == EINVAL
assert call(w1=None) == EINVAL and b"NULL" in L.evs_last_error()
assert call(B=0) == 0 and call(B=0, w1=None, x=None) == 0, "B == 0 is a no-op"
assert call(B=0, d=64) == EINVAL
assert not any(E._lib.mlp1_kernels_seen().values()), "a refused call launches nothing"
print("RECORD ok %%d" %% len(rec))
""" % ROOT


def test_the_mlp1_record_and_the_entry_checks_in_a_fresh_process():
    import evstore_dlrm_amd as E
    if not os.path.exists(E._lib.LIB_PATH):
        E.build()
    p = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "RECORD ok 6" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
