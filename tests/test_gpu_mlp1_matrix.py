"""The fused gather + interaction + first top-MLP layer (apply_emb_interact_mlp1 / evs_emb_interact_mlp1_stacked: the MLP form of
emb_interact_rf_kernel) against float64 at every shape edge of tests/_mlp1_matrix.py, under the launcher's dispatch record
(evs_mlp1_kernels_seen).  Per case and data kind (unit, dlrm, cancel, samesign; W1 and b1 drawn per kind):

  * R (return_R=True) is the plain fused launch's R bit for bit and passes tests/_accuracy.py's checks against float64;
  * Z1, linear and with ReLU, passes _mlp1_matrix.check over the kernel's own R (hard bound (K + 2) u Mz, Mz == 0 -> 0, median <= CAP);
    Z1 with R = NULL is Z1 with R written, bit for bit;
  * the record's count for the case's instantiation rose by exactly the launches made, no other count moved;
  * dlrm kind: W1 and b1 times 2^+-24 give Z1 times 2^+-24 bit for bit.

Then: x and lS_i with row strides above d and B; a NaN / +Inf table row stays inside its sample and shows in that sample's Z1 with and
without ReLU (torch.relu keeps NaN); bad indices raise the flag, read a zero row and leave the other samples alone; pad_top_layer's cache
follows copy_ / mul_ / load_state_dict, alternating weights, more weights than it holds, a replaced weight, a transposed view and a bf16
weight (writes through .data do not move _version: unsupported, not tested); refused calls launch nothing.  The closing test reads the
record: all six instantiations ran.  pytest -s prints a headroom line per instantiation."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import _accuracy as acc
import _mlp1_matrix as M

pytestmark = pytest.mark.gpu

TINY = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


@pytest.fixture(scope="module", autouse=True)
def record_at_start(E):
    """the record before this module's first case: the closing test counts this module's launches only"""
    return dict(E._lib.mlp1_kernels_seen())


@pytest.fixture(scope="module", autouse=True)
def headroom():
    """per instantiation: the worst err / bound and the largest median statistic of Z1 (and of R) seen (pytest -s)"""
    yield
    for k, (w, m, n) in sorted(M.STATS.items()):
        print("\nheadroom Z1 %-14s worst err/bound %.3f  median <= %.3f of cap %.3f  (%d checks)" % (k, w, m, M.CAP, n))
    for k, (w, m, n) in sorted(acc.STATS.items()):
        if k.startswith("mlp1_"):
            print("\nheadroom R  %-14s worst err/bound %.3f  median <= %.3f  (%d checks)" % (k, w, m, n))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


class Run:
    """one case and kind on the device; mlp1() counts its launches"""

    def __init__(self, E, case, kind, tables=None, idx=None):
        self.E, self.case, self.kind = E, case, kind
        d, T, itself, n1, B = case
        self.x, self.tabs, self.idx, self.W, self.b = M.inputs(case, kind)
        if tables is not None:
            self.tabs = tables
        if idx is not None:
            self.idx = idx
        self.ev = E.EVTables.from_fp32([torch.from_numpy(t) for t in self.tabs])
        self.xd, self.idxd, self.Wd, self.bd = _dev(self.x), _dev(self.idx), _dev(self.W), _dev(self.b)
        self.off = torch.arange(B, device="cuda").repeat(T, 1)
        self.launches = 0

    def mlp1(self, relu, return_R=True, x=None, idx=None, W=None, b=None):
        self.launches += 1
        out = self.E.apply_emb_interact_mlp1(self.xd if x is None else x, self.off, self.idxd if idx is None else idx, self.ev,
                                            self.Wd if W is None else W, self.bd if b is None else b, relu=relu,
                                            arch_interaction_itself=self.case[2], return_R=return_R)
        if return_R:
            return out[0].cpu().numpy(), out[1].cpu().numpy()
        return out.cpu().numpy()

    def plain(self, idx=None):
        return self.E.apply_emb_interact(self.xd, self.off, self.idxd if idx is None else idx, self.ev, None, self.case[2],
                                         one_index_per_bag=True).cpu().numpy()

    def ref_R(self):
        d, T, itself, n1, B = self.case
        return acc.reference_from_bags(self.x, self.tabs, [np.arange(B, dtype=np.int64)] * T, list(self.idx), itself)


def _record_moved(E, before, name, launches):
    after = E._lib.mlp1_kernels_seen()
    assert list(after) == M.NAMES
    moved = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert moved == ({name: launches} if launches else {}), (name, launches, moved)


# ------------------------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("kind", M.KINDS)
@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_case_against_float64(E, case, kind):
    """One case and kind: the bit identities, the record and (dlrm) the power-of-two scale first, then R and Z1 against float64.

    The distribution check is what made the kernel deal its fma chain to four accumulators.  With ONE accumulator over all kp columns (Z1
    had the bits of _mlp1_matrix.emulate(order="mfma") at all 60 pairs) five same-sign cases measured, on an MI355X, a median err / (u Mz)
    above CAP = 1.8708 -- d16-T16 1.994, d32-T16 2.040, d36-T15 2.550, d36-T26 3.197, d36-T27 3.161, at hard-bound ratios of 0.04 - 0.08:
    on same-sign data the running sum of one chain is four times as large over four times as many steps.  With four (Z1 has the bits of
    emulate(order="kernel") at all 60 pairs; the line this test prints says so) the same five measure 0.76 - 0.91 and the largest median
    of any pair is 1.27 (d36-T16-strict-n17-B1, same sign: 17 outputs)."""
    d, T, itself, n1, B = case
    F, P, K, kp, nj, name = M.shape(case)
    label = "%s %s" % (M.case_id(case), kind)
    before = E._lib.mlp1_kernels_seen()
    r = Run(E, case, kind)
    R0 = r.plain()
    Z = {}
    for relu in (False, True):
        Z[relu], R = r.mlp1(relu)
        assert _same(R, R0), label + ": R is not the plain fused launch's R (relu=%d)" % relu
        assert _same(r.mlp1(relu, return_R=False), Z[relu]), label + ": Z1 with R = NULL differs (relu=%d)" % relu
    if kind == "dlrm":
        nzR, nzW = np.abs(R0[R0 != 0]).min(), np.abs(r.W).min()
        for s in (-24, 24):
            f = np.float32(2.0 ** s)
            # every intermediate value is a sum of products R_k W_nk 2^s: a multiple of the smallest product's last bit
            assert float(nzR) * float(nzW) * 2.0 ** (min(s, 0) - 46) >= TINY and np.abs((r.b * f)[r.b != 0]).min() >= TINY
            for relu in (False, True):
                Zs = r.mlp1(relu, return_R=False, W=_dev(r.W * f), b=_dev(r.b * f))
                assert _same(Zs, Z[relu] * f), label + ": Z1 is not 2^%d times under W1, b1 times 2^%d (relu=%d)" % (s, s, relu)
    _record_moved(E, before, name, r.launches)
    e = acc.evaluate(R0, r.ref_R())
    el, er = M.evaluate(Z[False], R0, r.W, r.b, False), M.evaluate(Z[True], R0, r.W, r.b, True)
    chain = _same(M.emulate(R0, r.W, r.b, False, order="kernel"), Z[False])
    print("\n%-36s %s  R worst %.3f median %.3f | Z1 linear worst %.3f median %.3f | relu worst %.3f median %.3f (cap %.3f) | bits of the four-chain emulation: %s" % (
        label, name, e["worst"], e["median"], el["worst"], el["median"], er["worst"], er["median"], M.CAP, "yes" if chain else "no"))
    acc.check(R0, r.ref_R(), label, name)
    assert el["zero_ok"] and el["hard_ok"] and er["zero_ok"] and er["hard_ok"], (label, el, er)
    M.check(Z[False], R0, r.W, r.b, False, label + " linear", name)
    M.check(Z[True], R0, r.W, r.b, True, label + " relu", name)


# --------------------------------------------------------------------------------------------------------------------------- strides
@pytest.mark.parametrize("case", [(32, 10, False, 65, 33), (16, 16, False, 80, 33), (36, 27, True, 80, 47), (36, 16, False, 17, 1)], ids=M.case_id)
def test_row_strides_above_d_and_B(E, case):
    """x as a 16-byte-aligned column slice of a wider tensor, lS_i as a slice of a (T, B + 9) tensor: the bits of the contiguous call"""
    d, T, itself, n1, B = case
    r = Run(E, case, "unit")
    Z0, R0 = r.mlp1(True)
    wide = torch.full((B, d + 12), 7.0, device="cuda")
    wide[:, 4:4 + d] = r.xd
    xs = wide[:, 4:4 + d]
    big = torch.full((T, B + 9), -5, dtype=torch.int64, device="cuda")
    big[:, 5:5 + B] = r.idxd
    ids = big[:, 5:5 + B]
    assert xs.data_ptr() % 16 == 0 and xs.stride(0) == d + 12 and ids.stride(0) == B + 9
    for kw in ({"x": xs}, {"idx": ids}, {"x": xs, "idx": ids}):
        Z, R = r.mlp1(True, **kw)
        assert _same(Z, Z0) and _same(R, R0), (M.case_id(case), sorted(kw))
        assert _same(r.mlp1(False, return_R=False, **kw), r.mlp1(False, return_R=False))
    E._lib.check(E._lib.lib().evs_check_index_errors(None))


# ------------------------------------------------------------------------------------------------- isolation, non-finite values
ISOLATION = [(32, 10, False, 65, 33), (16, 16, False, 80, 33), (36, 26, False, 512, 293)]


def _own_row(case, kind):
    """-> sample s in the middle of a 16-sample chunk, table t, row r that only sample s reads, and the indices arranged so"""
    d, T, itself, n1, B = case
    _, tabs, idx, _, _ = M.inputs(case, kind)
    s, t = 16 * ((B // 16) // 2) + 7, T // 2
    n = tabs[t].shape[0]
    assert n >= 3 and s < B
    idx = idx.copy()
    r = int(idx[t, s])
    others = np.arange(B) != s
    idx[t, others & (idx[t] == r)] = (r + 1) % n
    return s, t, r, idx


@pytest.mark.parametrize("poison", ["nan", "inf"])
@pytest.mark.parametrize("case", ISOLATION, ids=M.case_id)
def test_a_non_finite_row_stays_in_its_sample_and_shows_in_Z1(E, case, poison):
    """NaN in a whole table row / +Inf in one element of it, read by one sample in the middle of a chunk: every other sample's Z1 and R
    keep the bits of the clean run, and the sample's Z1 is NaN wherever float64 nn.Linear (+ ReLU: torch.relu(nan) is nan) over its R is."""
    d, T, itself, n1, B = case
    s, t, row, idx = _own_row(case, "unit")
    clean = Run(E, case, "unit", idx=idx)
    tabs = [a.copy() for a in clean.tabs]
    if poison == "nan":
        tabs[t][row, :] = np.nan
    else:
        tabs[t][row, 5] = np.inf
    bad = Run(E, case, "unit", tables=tabs, idx=idx)
    others = np.arange(B) != s
    for relu in (False, True):
        Zc, Rc = clean.mlp1(relu)
        Zb, Rb = bad.mlp1(relu)
        assert np.isfinite(Zc).all() and np.isfinite(Rc).all()
        assert _same(Zb[others], Zc[others]) and _same(Rb[others], Rc[others]), "a non-finite row leaked into other samples (relu=%d)" % relu
        assert _same(Zb, bad.mlp1(relu, return_R=False))
        assert not np.isfinite(Rb[s]).all(), "the row does not show in R"
        hidden, n_nan = M.hidden_nans(Zb[s:s + 1], Rb[s:s + 1], bad.W, bad.b, relu)
        assert n_nan, "float64 gives no NaN here: the case checks nothing"
        assert len(hidden) == 0, "%s relu=%d: Z1[%d] hides the NaN of float64 at %d of %d outputs (first: output %d = %r)" % (
            M.case_id(case), relu, s, len(hidden), n_nan, hidden[0][1], Zb[s][hidden[0][1]])


# ----------------------------------------------------------------------------------------------------------------------- bad indices
@pytest.mark.parametrize("which", ["past_the_end", "negative"])
@pytest.mark.parametrize("case", ISOLATION[:2], ids=M.case_id)
def test_a_bad_index_raises_the_flag_and_reads_a_zero_row(E, case, which):
    d, T, itself, n1, B = case
    F, P, K, kp, nj, name = M.shape(case)
    s, t, row, idx = _own_row(case, "unit")
    r = Run(E, case, "unit", idx=idx)
    L = E._lib.lib()
    E._lib.check(L.evs_check_index_errors(None))
    Zc, Rc = r.mlp1(True)
    E._lib.check(L.evs_check_index_errors(None))
    badidx = idx.copy()
    badidx[t, s] = r.tabs[t].shape[0] if which == "past_the_end" else -1
    bd = _dev(badidx)
    Zb, Rb = r.mlp1(True, idx=bd)
    with pytest.raises(E.EvsError):
        E._lib.check(L.evs_check_index_errors(None))
    Rp = r.plain(idx=bd)
    with pytest.raises(E.EvsError):
        E._lib.check(L.evs_check_index_errors(None))
    E._lib.check(L.evs_check_index_errors(None))
    assert _same(Rb, Rp), "R over a bad index is not the plain launch's"
    li, lj = acc.pair_index(F, itself)
    touched = d + np.nonzero((li == t + 1) | (lj == t + 1))[0]
    assert (Rb[s, touched] == 0).all() and _same(np.delete(Rb[s], touched), np.delete(Rc[s], touched)), "the bad index is not a zero row"
    others = np.arange(B) != s
    assert _same(Zb[others], Zc[others]) and _same(Rb[others], Rc[others])
    M.check(Zb[s:s + 1], Rb[s:s + 1], r.W, r.b, True, "%s bad index %s" % (M.case_id(case), which), name)
    Zl = r.mlp1(False, return_R=False, idx=bd)
    with pytest.raises(E.EvsError):
        E._lib.check(L.evs_check_index_errors(None))
    M.check(Zl[s:s + 1], Rb[s:s + 1], r.W, r.b, False, "%s bad index %s linear" % (M.case_id(case), which), name)


# ------------------------------------------------------------------------------------------------------------- pad_top_layer's cache
def test_the_padded_weight_follows_its_weight(E):
    """Every way a top layer's weight changes between two calls, each result against float64 over the kernel's own R (a stale padded
    copy is wrong by whole weights, not by roundings).  Writes through W1.data do not move W1._version and are not supported."""
    case = (36, 4, False, 15, 15)
    d, T, itself, n1, B = case
    F, P, K, kp, nj, name = M.shape(case)
    r = Run(E, case, "unit")
    rs = np.random.RandomState(5)
    new = lambda: rs.uniform(-1, 1, (n1, K)).astype(np.float32)

    def ok(Wt, W_np, what, b=None):
        Z, R = r.mlp1(False, W=Wt, b=b)
        M.check(Z, R, W_np, r.b, False, "pad_top_layer " + what, name)

    W = _dev(new())
    ok(W, W.cpu().numpy(), "first use")
    W.copy_(_dev(new()))
    ok(W, W.cpu().numpy(), "after copy_")
    W.mul_(-1.75)
    ok(W, W.cpu().numpy(), "after mul_")
    lin = torch.nn.Linear(K, n1).cuda()
    ok(lin.weight, lin.weight.detach().cpu().numpy(), "nn.Linear.weight", b=r.bd)
    lin.load_state_dict({"weight": _dev(new()), "bias": r.bd.clone()})
    ok(lin.weight, lin.weight.detach().cpu().numpy(), "after load_state_dict", b=r.bd)
    A, Bw = _dev(new()), _dev(new())
    for i in range(6):
        ok(A if i % 2 == 0 else Bw, (A if i % 2 == 0 else Bw).cpu().numpy(), "alternating %d" % i)
    many = [_dev(new()) for _ in range(18)]   # (the cache is cleared past 16 entries)
    for rep in range(2):
        for i, Wi in enumerate(many):
            ok(Wi, Wi.cpu().numpy(), "weight %d of 18, round %d" % (i, rep))
    shape = tuple(many[3].shape)
    del many, Wi
    gc.collect()
    fresh = _dev(new())
    assert tuple(fresh.shape) == shape
    ok(fresh, fresh.cpu().numpy(), "a new tensor in place of a deleted one")
    Wt = _dev(np.ascontiguousarray(new().T))      # (K, n1): its transpose is a (n1, K) view with strides (1, n1)
    assert not Wt.t().is_contiguous()
    ok(Wt.t(), Wt.cpu().numpy().T, "transposed view")
    Wb = _dev(new()).to(torch.bfloat16)
    ok(Wb, Wb.to(torch.float32).cpu().numpy(), "bf16 weight")


# -------------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(E):
    """EVS_EINVAL, no launch (the record), Z1 and R untouched: d = 64; T = 28; kp not K rounded up to 16; a misaligned w1_padded;
    n1 = 0.  B = 0 is success and touches nothing."""
    L = E._lib.lib()
    T, d, B, n1 = 26, 36, 4, 8
    K, kp = 387, 400
    tabs = [torch.zeros((5, 64), device="cuda") for _ in range(32)]
    x = torch.zeros((B, 64), device="cuda")
    idx = torch.zeros((32, B), dtype=torch.int64, device="cuda")
    w1 = torch.zeros((16, 464 + 4), device="cuda")
    b1 = torch.zeros((16,), device="cuda")
    Z1 = torch.full((B, 16), 3.0, device="cuda")
    R = torch.full((B, 512), 3.0, device="cuda")
    tp = (C.c_void_p * 32)(*[t.data_ptr() for t in tabs])
    nr = (C.c_int64 * 32)(*([5] * 32))
    before = E._lib.mlp1_kernels_seen()

    def call(**kw):
        a = dict(B=B, T=T, d=d, kp=kp, n1=n1, w1=w1.data_ptr(), xs=64)
        a.update(kw)
        return L.evs_emb_interact_mlp1_stacked(a["B"], a["T"], a["d"], tp, nr, x.data_ptr(), a["xs"], idx.data_ptr(), B, 0, a["w1"], a["kp"],
                                               b1.data_ptr(), a["n1"], 1, Z1.data_ptr(), R.data_ptr(), None)

    EINVAL = E._lib.EVS_EINVAL
    assert call(d=64) == EINVAL
    assert call(T=28) == EINVAL
    assert call(kp=384) == EINVAL and call(kp=416) == EINVAL and call(kp=K) == EINVAL
    assert call(w1=w1.data_ptr() + 4) == EINVAL
    assert call(n1=0) == EINVAL
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert E._lib.mlp1_kernels_seen() == before, "a refused call launched a kernel"
    assert bool((Z1 == 3.0).all()) and bool((R == 3.0).all())


# --------------------------------------------------------------------------------------------------------------------------- closing
def test_every_instantiation_was_launched(E, record_at_start):
    """All six names went up in this module.  It reads what the tests above left in this process: it runs last and only with the whole
    module -- under -k, another order or several workers it fails, as the other matrices' closing tests do."""
    seen = E._lib.mlp1_kernels_seen()
    assert list(seen) == M.NAMES
    never = sorted(k for k in seen if seen[k] == record_at_start[k])
    print("\nmlp1 record: " + "  ".join("%s=%d" % (k, seen[k] - record_at_start[k]) for k in seen))
    assert not never, "instantiations this module did not launch: %s" % never
