"""The lean entry of the fused launch (csrc/evs_fused_rf_lean.hip: scalar kernel arguments, per-model descriptor in device
memory) against the SAME call in list form -- lS_o / lS_i as lists of per-table tensors, which never is the stacked form and
runs the FusedArgs entry, the arithmetic the parity tests hold to the oracle.  Same arithmetic, so every comparison is
torch.equal.  Tables are tiny (3 .. 5 000 rows); the shapes are the smallest at which the kernel is chosen and can go wrong."""
import ctypes
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(26, 36), (8, 16), (26, 32), (26, 64)]     # NT = 2 / CQ = 2 / REM = 1;  F <= 16: NT = 1;  REM = 0;  CQ = 4


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _model(E, T, d, seed, lo=3, hi=5000):
    rs = np.random.RandomState(seed)
    ns = [int(n) for n in rs.randint(lo, hi + 1, T)]
    ns[0], ns[-1] = lo, hi
    tabs = [torch.from_numpy(rs.uniform(-1, 1, (n, d)).astype(np.float32)) for n in ns]
    return E.EVTables.from_fp32(tabs), ns


def _batch(ns, B, d, seed):
    rs = np.random.RandomState(seed)
    idx = np.stack([rs.randint(0, n, B) for n in ns]).astype(np.int64)
    idx[:, 0] = 0
    idx[:, -1] = np.array(ns) - 1
    x = rs.uniform(-1, 1, (B, d)).astype(np.float32)
    off = np.tile(np.arange(B, dtype=np.int64), (len(ns), 1))
    return torch.from_numpy(x).cuda(), torch.from_numpy(off).cuda(), torch.from_numpy(idx).cuda()


def _as_list(t):
    """the rows of a (T, B) tensor as T tensors at IRREGULAR distances in one buffer: never the stacked form's fixed stride"""
    T, B = t.shape
    buf = torch.empty(T * (B + 64) + 64, dtype=t.dtype, device=t.device)
    out = []
    for k in range(T):
        at = k * (B + 64) + 8 * (k % 3)
        buf[at:at + B] = t[k]
        out.append(buf[at:at + B])
    return out


def _ref(E, ev, x, off, idx, **kw):
    n = _lean(E)
    want = E.apply_emb_interact(x.contiguous(), _as_list(off), _as_list(idx), ev, **kw)
    assert _lean(E) == n, "the reference must run the FusedArgs entry"
    return want


def _lean(E):
    """launches that took the lean entry so far: a call that silently declines computes the same results, so every test
    below also counts (evs_x_lean_launches: a developer symbol of the library, outside the header's ABI)"""
    fn = E._lib.lib().evs_x_lean_launches
    fn.restype, fn.argtypes = ctypes.c_ulonglong, []
    return int(fn())


@pytest.mark.parametrize("one", [False, True], ids=["lS_o", "declared"])
@pytest.mark.parametrize("T,d", SHAPES)
@pytest.mark.parametrize("B", [2048, 2053])
def test_lean_equals_list_form(E, B, T, d, one):
    """the tile path's minimum batch, and a last block of 5 samples (waves with 2 / 1 / 1 / 1: the phantom-sample path)"""
    ev, ns = _model(E, T, d, 100 * T + d)
    x, off, idx = _batch(ns, B, d, B + d)
    want = _ref(E, ev, x, off, idx, check_indices=True)
    n = _lean(E)
    got = E.apply_emb_interact(x, None if one else off, idx, ev, check_indices=True, one_index_per_bag=one)
    assert torch.equal(got, want)
    want = _ref(E, ev, x, off, idx, arch_interaction_itself=True)
    got = E.apply_emb_interact(x, None if one else off, idx, ev, arch_interaction_itself=True, one_index_per_bag=one)
    assert torch.equal(got, want)
    assert _lean(E) == n + 2


@pytest.mark.parametrize("one", [False, True], ids=["lS_o", "declared"])
def test_lean_one_full_generation(E, one):
    T, d, B = 26, 36, 16384
    ev, ns = _model(E, T, d, 7)
    x, off, idx = _batch(ns, B, d, 8)
    want = _ref(E, ev, x, off, idx, check_indices=True)
    n = _lean(E)
    got = E.apply_emb_interact(x, None if one else off, idx, ev, check_indices=True, one_index_per_bag=one)
    assert torch.equal(got, want) and _lean(E) == n + 1


@pytest.mark.parametrize("one", [False, True], ids=["lS_o", "declared"])
@pytest.mark.parametrize("T,d", [(26, 36), (8, 16)])
def test_lean_strided_inputs(E, T, d, one):
    """row strides that are not B, x rows that are not d apart, out= given and not given"""
    B = 2053
    ev, ns = _model(E, T, d, 11 * T + d)
    x, off, idx = _batch(ns, B, d, 12)
    wide_i = torch.full((T, B + 64), -7, dtype=torch.int64, device="cuda")
    wide_o = torch.full((T, B + 64), -7, dtype=torch.int64, device="cuda")
    wide_x = torch.full((B, d + 4), 9.0, dtype=torch.float32, device="cuda")
    wide_i[:, :B], wide_o[:, :B], wide_x[:, :d] = idx, off, x
    si, so, sx = wide_i[:, :B], wide_o[:, :B], wide_x[:, :d]
    assert si.stride(0) != B and sx.stride(0) != d
    want = _ref(E, ev, x, off, idx, check_indices=True)
    got = E.apply_emb_interact(sx, None if one else so, si, ev, check_indices=True, one_index_per_bag=one)
    assert torch.equal(got, want)
    out = torch.full_like(want, float("nan"))
    n = _lean(E)
    ret = E.apply_emb_interact(sx, None if one else so, si, ev, out=out, one_index_per_bag=one)
    assert ret.data_ptr() == out.data_ptr() and torch.equal(out, want) and _lean(E) == n + 1


def test_lean_slow_block(E):
    """one 16-sample chunk with an empty bag followed by a bag of two indices: only that block takes the general loop"""
    T, d, B = 26, 36, 2048
    ev, ns = _model(E, T, d, 21)
    x, off, idx = _batch(ns, B, d, 22)
    b = 16 * 5 + 3
    off[:, b + 1] = b          # bag b = [b, b): empty;  bag b + 1 = [b, b + 2): two indices
    want = _ref(E, ev, x, off, idx, check_indices=True)
    n = _lean(E)
    got = E.apply_emb_interact(x, off, idx, ev, check_indices=True)
    assert torch.equal(got, want) and _lean(E) == n + 1


@pytest.mark.parametrize("last", ["B", "B-1"])
def test_lean_offsets_with_the_last_offset_included(E, last):
    """B + 1 offsets per table (EmbeddingBag's include_last_offset form): lists whose tensors are the rows of ONE array at a
    fixed distance are the stacked form, so the lean entry runs with B + 1 readable offsets per row.  The last entry ends the
    last bag: B, or B - 1 -- then the last bag is empty and the last block pools the slow way."""
    T, d, B = 26, 36, 2053
    ev, ns = _model(E, T, d, 23)
    x, off, idx = _batch(ns, B, d, 24)
    off1 = torch.cat([off, torch.full((T, 1), B if last == "B" else B - 1, dtype=torch.int64, device="cuda")], dim=1).contiguous()
    idx = idx.contiguous()
    want = _ref(E, ev, x, off1, idx, check_indices=True)
    n = _lean(E)
    got = E.apply_emb_interact(x, list(off1.unbind(0)), list(idx.unbind(0)), ev, check_indices=True)
    assert torch.equal(got, want) and _lean(E) == n + 1
    if last == "B":      # (the same bags as B offsets give)
        assert torch.equal(got, _ref(E, ev, x, off, idx, check_indices=True))


def test_lean_bad_index(E):
    """an index >= n_rows in a fast block: the same error as the list form, the row counted as zeros"""
    T, d, B = 26, 36, 2048
    ev, ns = _model(E, T, d, 31)
    x, off, idx = _batch(ns, B, d, 32)
    idx[3, 16 * 7 + 5] = ns[3]
    want = torch.full((B, d + (T + 1) * T // 2), float("nan"), device="cuda")
    got = torch.full_like(want, float("nan"))
    with pytest.raises(E._lib.EvsError) as e_list:
        _ref(E, ev, x, off, idx, check_indices=True, out=want)
    n = _lean(E)
    for one, o in ((False, off), (True, None)):
        got.fill_(float("nan"))
        with pytest.raises(E._lib.EvsError) as e_lean:
            E.apply_emb_interact(x, o, idx, ev, check_indices=True, out=got, one_index_per_bag=one)
        assert e_lean.value.code == e_list.value.code and str(e_lean.value) == str(e_list.value)
        assert torch.equal(got, want)
    assert _lean(E) == n + 2
    idx[3, 16 * 7 + 5] = 0     # the flag is cleared by the check: the next call is clean
    assert torch.equal(E.apply_emb_interact(x, off, idx, ev, check_indices=True), _ref(E, ev, x, off, idx, check_indices=True))


def test_descriptor_cache_two_models_alternately(E):
    B = 2048
    a, b = _model(E, 26, 36, 41), _model(E, 8, 16, 42)
    for it in range(3):
        for (ev, ns), d in ((a, 36), (b, 16)):
            x, off, idx = _batch(ns, B, d, 43 + it)
            n = _lean(E)
            assert torch.equal(E.apply_emb_interact(x, off, idx, ev), _ref(E, ev, x, off, idx))
            assert _lean(E) == n + 1


def test_descriptor_cache_eviction(E):
    """nine distinct models in turn -- the ninth takes the first one's slot -- then the first again"""
    B, T, d = 2048, 8, 16
    models = [_model(E, T, d, 50 + k, hi=200) for k in range(9)]
    batches = [_batch(ns, B, d, 60 + k) for k, (_, ns) in enumerate(models)]
    want = [_ref(E, ev, *batches[k]) for k, (ev, _) in enumerate(models)]
    n = _lean(E)
    for k in list(range(9)) + [0, 8, 1]:
        assert torch.equal(E.apply_emb_interact(*batches[k], models[k][0]), want[k]), "model %d" % k
    assert _lean(E) == n + 12     # (an evicted model gets a descriptor again: none of the calls declined)


def test_descriptor_cache_model_replaced(E):
    """a model dropped and one of other row counts allocated after it: the allocator may hand the addresses out again"""
    B, T, d = 2048, 8, 16
    for k in range(4):
        ev, ns = _model(E, T, d, 70 + k, lo=3 + k, hi=300 + 10 * k)
        x, off, idx = _batch(ns, B, d, 80 + k)
        n = _lean(E)
        assert torch.equal(E.apply_emb_interact(x, off, idx, ev, check_indices=True), _ref(E, ev, x, off, idx, check_indices=True))
        assert _lean(E) == n + 1
        del ev
        torch.cuda.synchronize()


def _capture_and_replay(E, ev, ns, B, d, warm):
    x, off, idx = _batch(ns, B, d, 90)
    out = torch.zeros((B, d + (len(ns) + 1) * len(ns) // 2), device="cuda")
    if warm:
        E.apply_emb_interact(x, off, idx, ev, out=out)
        torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    n = _lean(E)
    with torch.cuda.graph(g):     # one kernel, no parallel branches
        E.apply_emb_interact(x, off, idx, ev, out=out)
    # a known model's capture holds the lean entry; one first seen inside the capture the FusedArgs entry (nothing is allocated there)
    assert _lean(E) == n + (1 if warm else 0)
    for it in range(3):
        _, _, idx2 = _batch(ns, B, d, 91 + it)
        idx.copy_(idx2)
        want = _ref(E, ev, x, off, idx)
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want), "replay %d" % it


def test_graph_capture_of_a_warmed_model(E):
    ev, ns = _model(E, 26, 36, 95)
    _capture_and_replay(E, ev, ns, 2048, 36, warm=True)


def test_graph_capture_of_a_model_first_seen_in_the_capture(E):
    ev, ns = _model(E, 26, 36, 96)
    _capture_and_replay(E, ev, ns, 2048, 36, warm=False)


def test_two_threads_two_streams(E):
    T, d, B = 26, 36, 2048
    ev, ns = _model(E, T, d, 97)
    batches = [_batch(ns, B, d, 98 + t) for t in range(2)]
    want = [_ref(E, ev, *b) for b in batches]
    torch.cuda.synchronize()
    wrong, errors = [], []
    n = _lean(E)

    def work(t):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for it in range(10):
                    got = E.apply_emb_interact(*batches[t], ev)
                    s.synchronize()
                    if not torch.equal(got, want[t]):
                        wrong.append((t, it))
        except Exception as e:   # noqa: BLE001 -- reported below, in the test's own thread
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors and not wrong, (errors, wrong)
    assert _lean(E) == n + 20
