"""The mixed-precision interaction consumers (csrc/evs_mixed.hip), every instantiation, at the full code range, against float64.

interact_mixed84_kernel<CQ, REM, NT, PROBE> (the (u8, u4) pair: rows in registers, clamped windows, the 12-byte FOLD load at d = 36, one
decode table picked per lane by the class mask) and interact_mixed_rows_kernel<CQ, REM, NT> (every other pair: per-chunk dispatch on the
codec, a capped grid-stride loop).  The cache tests reach them only with rows of -1 / 0 / 1, because there the tier that serves a miss is the
routing's choice.  Here every case is one call of evs_interact_rows_by_address -- several calls of one shape over fresh draws where one
call has fewer than 64 pair elements (tests/_mixed_matrix.py:run_case), each under the first two assertions below and all of them under one
check -- and the test picks each row's address and class itself, so rows of any code go to either class inside one wave.  Class 0 comes with
a live address and address 0 with a live class: either alone must give a row of exact zeros.  Every case asserts

  * the dispatch record (evs_mixed_kernels_seen) before and after: exactly the intended name went up by one;
  * R was filled with a NaN sentinel and has a guard band behind it: the band is untouched, and every element of R passes
  * tests/_accuracy.py's check with L = 1 and no extra: x columns bit for bit, exact zeros where the magnitude is zero (class 0, null address),
    the hard bound (d + 4) u M, median err / (u M) <= 4 -- against fp64 over the oracle's bit-exact decode of the rows addressed.

The one-hot probe (x[b] = e_c: R[b, pair(i, 0)] is one decoded element times 1.0 plus exact zeros) compares single elements with the
oracle's decode, bit for bit: all 256 u8 codes and 16 u4 nibbles at every element position, in both halves of the feature rows.

EVS_MIXED_RFQ=0 runs in one child process (tests/_mixed_matrix_env_child.py): the (8, 4) cases and the probe again, through
interact_mixed_rows_kernel.  The folded probe (the *_probe names) runs through lookup_interact_c1c2 on tiers of full-range rows, every cell's
precision decided from the two dumps taken before the call.  The closing test reads the whole record: all 18 names went up.

Wall time on an MI355X: this module 7.8 s -- 2 094 by-address cases (3 882 launches) and 24 probe runs here, 896 cases (1 412 launches) and 12
probe runs in the child, which takes 3.0 s of it."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _accuracy as acc
import _mixed_matrix as MM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    assert "EVS_MIXED_RFQ" not in os.environ and "EVS_CACHE_FOLD2" not in os.environ, "this module pins the DEFAULT dispatch"
    return E


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module", autouse=True)
def record_at_start(E):
    """the record before this module's first case: the closing test counts this module's launches only"""
    return dict(E._lib.mixed_kernels_seen())


@pytest.fixture(scope="module", autouse=True)
def headroom():
    """per kernel: the worst err / bound and the largest median statistic seen (printed at the end: pytest -s)"""
    yield
    for k, (w, m, n) in sorted(acc.STATS.items()):
        if k.startswith("interact_mixed"):
            print("\nheadroom %-45s worst err/bound %.3f  median <= %.3f  (%d checks)" % (k, w, m, n))
    print("\nmixed matrix: %d cases, %d launches in this process" % (MM.N_CASES[0], MM.N_LAUNCHES[0]))


# --------------------------------------------------------------------------------------------------------- the consumers by address
@pytest.mark.parametrize("d", MM.DIMS)
@pytest.mark.parametrize("codecs", ((8, 4),) + MM.ROWS_PAIRS)
def test_consumer_by_address(E, orc, codecs, d):
    """the covering subset of (T, B, itself, class pattern, x stride) for one codec pair and d: tests/_mixed_matrix.py:cases"""
    for case in MM.cases(codecs, d):
        MM.run_case(E, orc, case)


@pytest.mark.parametrize("NT", (1, 2))
@pytest.mark.parametrize("cls", (1, 2))
@pytest.mark.parametrize("d", MM.DIMS)
def test_decode_probe_one_hot(E, orc, d, cls, NT):
    """every code at every element position of both row halves, one element at a time, against the oracle's decode bit for bit"""
    for itself in (0, 1):
        MM.run_probe(E, orc, d, cls, NT, itself)


def test_refusals_launch_nothing(E):
    before = E._lib.mixed_kernels_seen()
    x = torch.zeros((4, 36), device="cuda")
    R = torch.zeros((4, 36 + 351), device="cuda")
    p = torch.zeros((4, 26), dtype=torch.int64, device="cuda")
    L = E._lib.lib()
    for bad in (dict(d=20), dict(T=0), dict(T=32), dict(c1=5), dict(B=-1)):
        a = dict(B=4, T=26, d=36, c1=8)
        a.update(bad)
        assert L.evs_interact_rows_by_address(a["B"], a["T"], a["d"], x.data_ptr(), 36, p.data_ptr(), None, a["c1"], 4, 0, 1, R.data_ptr(), None) \
            == E._lib.EVS_EINVAL
    assert L.evs_interact_rows_by_address(0, 26, 36, x.data_ptr(), 36, p.data_ptr(), None, 8, 4, 0, 1, R.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert E._lib.mixed_kernels_seen() == before and not R.any()


# ------------------------------------------------------------------------------------------------ the folded probe, full code range
LEFT_OUT = {}    # (policy, d, T) -> the largest share of a call's samples left out of the reference


def _pair(E, orc, policy, d, T, seed):
    """A (u8, u4) tier pair over the SAME uniform(-1, 1) fp32 tables, so a key's two rows decode to different values.  The key universe U is
    rows 0 .. u - 1 of every table (576 keys at T = 9, 832 at T = 26): cap1 = |U| / 2 < |U| <= cap2 / 4.
    With these capacities a set-associative pair gets no shared record (C1 would have fewer than 4 ways of it), so each tier
    keeps 8-way sets of its own -- the geometry the folded probe is compiled for."""
    rs = np.random.RandomState(seed)
    n, u = 300, {9: 64, 26: 32}[T]
    ws = [rs.uniform(-1, 1, size=(n, d)).astype(np.float32) for _ in range(T)]
    raw8 = [np.ascontiguousarray(orc.encode_table(w, 8)) for w in ws]
    raw4 = [np.ascontiguousarray(orc.encode_table(w, 4)) for w in ws]
    dec = {1: np.stack([orc.decode(r, 8, d) for r in raw8]), 2: np.stack([orc.decode(r, 4, d) for r in raw4])}   # (T, n, d) per class
    cap1 = (T * u // 2) // 8 * 8
    cap2 = -(-4 * T * u // 8) * 8
    assert cap1 < T * u <= cap2 // 4
    c1 = E.GpuCache("evlfu", cap1, T, d, 8, "cpp").set_batch_policy(policy)
    c2 = E.GpuCache("evlfu", cap2, T, d, 4, "cpp").set_batch_policy(policy)
    c1.set_backing([torch.from_numpy(r).cuda() for r in raw8])
    c2.set_backing([torch.from_numpy(r).cuda() for r in raw4])
    return rs, c1, c2, dec, cap1, n, u


def _dumps(c1, c2):
    in1 = {(int(t) - 1, int(rw)) for _, t, rw in c1.batch_dump()}
    in2 = {(int(t) - 1, int(rw)) for _, t, rw in c2.batch_dump()}
    assert not (in1 & in2), "a key lives in one tier"
    return in1, in2


def _probe_call(E, c1, c2, dec, rq, fresh_cls, rs, d, T, threshold, itself, what, name):
    """One lookup_interact_c1c2 under the record.  The class of every cell comes from facts known BEFORE the call: the two dumps for a key of
    U, fresh_cls (B, T) (0: not fresh) for a key no earlier call has named.  A sample with a cell in neither is left out of the reference.
    -> (share of the samples left out, share of the checked samples that hold both classes)"""
    from evstore_dlrm_amd import gpu_cache
    B = rq.shape[0]
    in1, in2 = _dumps(c1, c2)
    res = np.array([[1 if (k, int(rq[b, k])) in in1 else 2 if (k, int(rq[b, k])) in in2 else 0 for k in range(T)] for b in range(B)])
    assert not (res.astype(bool) & fresh_cls.astype(bool)).any(), "a fresh key is resident"
    cls = np.where(fresh_cls > 0, fresh_cls, res)
    x = rs.uniform(-1, 1, size=(B, d)).astype(np.float32)
    before = E._lib.mixed_kernels_seen()
    tier, R = gpu_cache.lookup_interact_c1c2(c1, c2, torch.from_numpy(rq).cuda(), torch.from_numpy(x).cuda(), threshold=threshold, itself=bool(itself))
    tier, R = tier.cpu().numpy(), R.cpu().numpy()
    after = E._lib.mixed_kernels_seen()
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {name: 1}, (name, before, after)
    assert np.array_equal(tier, res), "tier codes: residency when the call began, on every cell"
    keep = (cls > 0).all(1)
    rows = np.zeros((B, T, d), np.float32)
    kk = np.broadcast_to(np.arange(T), (B, T))
    for c in (1, 2):
        rows[cls == c] = dec[c][kk[cls == c], rq[cls == c]]
    assert keep.any()
    ref = acc.Reference(x[keep], [MM.AD.sub(rows[keep][:, k]) for k in range(T)], bool(itself))
    acc.check(R[keep], ref, what, "interact_mixed84_kernel " + name, np.nonzero(keep)[0])
    both = ((cls[keep] == 1).any(1) & (cls[keep] == 2).any(1)).mean()
    return 1.0 - keep.mean(), float(both)


@pytest.mark.parametrize("policy", ["sampled", "setassoc"])
@pytest.mark.parametrize("T", [9, 26])
@pytest.mark.parametrize("d", MM.DIMS)
def test_folded_probe_full_code_range(E, orc, d, T, policy):
    """interact_mixed84_kernel<.., PROBE> through lookup_interact_c1c2 on tiers whose rows use the whole code range.

    Hits: warmed at threshold 0 (a miss goes to C1 only while C1 -- set-associative: the key's own C1 set -- has room, everything else to C2)
    until the two dumps cover U; then B = 1, 17 and 333 drawn from U.  Misses (sampled policy, C1 at capacity): half of the cells name keys
    no call has named; at threshold 0 they are served from C2's table (u4), at threshold T + 1 from C1's table (u8) for an odd zero-based
    table index and from C2's otherwise.  The dumps are rebuilt before every call.
    At most 10 % of a call's samples may be left out of the reference (a cell of U in neither dump), and half of the checked samples must hold
    both precisions.  Observed on an MI355X with these capacities (cap1 = |U| / 2, cap2 = 4 |U|): two warm rounds cover U, and the share left out
    is 0.000 in every call of all twelve cases (sampled: C1 ends at capacity, 288 / 416 entries; set-associative: 202 of 288 and 292 of 416,
    the keys whose C1 set was full sit in C2)."""
    rs, c1, c2, dec, cap1, n, u = _pair(E, orc, policy, d, T, 7 * d + T)
    name = "r84_d%d_nt%d_probe" % (d, 2 if T + 1 > 16 else 1)
    U = {(k, r) for k in range(T) for r in range(u)}
    no_fresh = lambda B: np.zeros((B, T), np.int64)   # noqa: E731
    from evstore_dlrm_amd import gpu_cache
    for rnd in range(40):   # warm: every key of U once per round; bounded
        rq = ((np.arange(u)[:, None] + rnd * np.arange(T)[None, :]) % u).astype(np.int32)
        gpu_cache.lookup_interact_c1c2(c1, c2, torch.from_numpy(rq).cuda(), torch.rand(u, d, device="cuda"), threshold=0)
        in1, in2 = _dumps(c1, c2)
        if U <= (in1 | in2):
            break
    worst = 0.0
    for B in (1, 17, 333):
        for _ in range(200):   # (B = 1: a sample that holds both classes, chosen from the dumps -- facts known before the call)
            rq = rs.randint(0, u, size=(B, T)).astype(np.int32)
            res = np.array([[1 if (k, int(rq[b, k])) in in1 else 2 if (k, int(rq[b, k])) in in2 else 0 for k in range(T)] for b in range(B)])
            if B > 1 or ((res == 1).any() and (res == 2).any()):
                break
        out, both = _probe_call(E, c1, c2, dec, rq, no_fresh(B), rs, d, T, 0, B & 1, "folded probe hits %s d=%d T=%d B=%d" % (policy, d, T, B), name)
        assert out <= 0.10 and both >= 0.5, (out, both)
        worst = max(worst, out)
        in1, in2 = _dumps(c1, c2)
    if policy == "sampled":
        # a batch whose misses outnumber C1's room leaves C1 short of its capacity (the update turns the surplus away): fill it one key per
        # call, keys of rows 200 .. that nothing else names, each a lone miss among hits.  Bounded.
        for it in range(2 * cap1):
            if c1.batch_stats()["size"] >= cap1:
                break
            rq = rs.randint(0, u, size=(1, T)).astype(np.int32)
            rq[0, it % T] = 200 + it // T
            gpu_cache.lookup_interact_c1c2(c1, c2, torch.from_numpy(rq).cuda(), torch.rand(1, d, device="cuda"), threshold=0)
        nxt = u
        for thr in (0, T + 1):   # (the second call's odd-table misses go INTO the full C1 and evict keys of U: it comes last)
            B = 17
            assert c1.batch_stats()["size"] == cap1, "C1 at capacity: a miss is routed by the threshold rule alone"
            fresh = rs.rand(B, T) < 0.5
            in1, in2 = _dumps(c1, c2)   # the other cells: keys of U resident now, so that a sample holds rows of both precisions
            held = [sorted(r for kk, r in (in1 | in2) if kk == k and r < u) for k in range(T)]
            assert all(held)
            hits = np.stack([np.asarray(h)[rs.randint(0, len(h), B)] for h in held], 1)
            rq = np.where(fresh, nxt + np.arange(B)[:, None], hits).astype(np.int32)
            nxt += B
            assert nxt <= n
            odd = (np.arange(T) & 1)[None, :]
            fc = np.where(fresh, 2 if thr == 0 else np.where(odd == 1, 1, 2), 0)
            out, both = _probe_call(E, c1, c2, dec, rq, fc, rs, d, T, thr, 1, "folded probe misses thr=%d d=%d T=%d" % (thr, d, T), name)
            assert out <= 0.10 and both >= 0.5, (thr, out, both)
            worst = max(worst, out)
    LEFT_OUT[(policy, d, T)] = worst
    print("left out %s d=%d T=%d: %.3f (warm rounds %d, resident %d + %d of |U| = %d, C1 size %d of %d)" % (
        policy, d, T, worst, rnd + 1, len(in1 & U), len(in2 & U), len(U), c1.batch_stats()["size"], cap1))


# ------------------------------------------------------------------------------------------------------- behind the switch: one child
def test_rows_kernel_takes_the_u8_u4_pair_when_the_switch_is_off():
    """EVS_MIXED_RFQ=0 in one child process (the switch is read once per process): the (8, 4) cases and the probe through
    interact_mixed_rows_kernel.  A child that ends by signal, abort or timeout fails this test; nothing else is started here."""
    env = {k: v for k, v in os.environ.items() if k != "EVS_MIXED_RFQ"}
    env["EVS_MIXED_RFQ"] = "0"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_mixed_matrix_env_child.py")], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    print(p.stdout.strip().splitlines()[-1])


# --------------------------------------------------------------------------------------------------------------------------- closing
def test_every_instantiation_was_launched(E, record_at_start):
    """The whole record: all 18 names went up, and every name but the folded probe's was hit by a random-class case at each of B = 1, 17 and
    67.  It speaks about the module as a whole and reads what the tests above left in this process (the record, MM.HITS): it runs last and
    only with the whole module -- under -k, another order or several workers it fails, as the pooling matrix's closing test does."""
    seen = E._lib.mixed_kernels_seen()
    assert list(seen) == MM.ALL_NAMES
    never = sorted(k for k in seen if seen[k] == record_at_start[k])
    assert not never, "instantiations this module did not launch: %s" % never
    want = {(n, B) for n in MM.ALL_NAMES if not n.endswith("_probe") for B in (1, 17, 67)}
    assert want <= MM.HITS, sorted(want - MM.HITS)
