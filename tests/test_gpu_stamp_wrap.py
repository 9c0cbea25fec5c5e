"""EvLFU on the set-associative cache tier across wraps of the batch stamp.  A way word keeps the batch that FILLED the way
modulo 2^S in the bits its tag leaves free (csrc/evs_hash.h: sa_word / sa_stamp; S = 26 - dual - tag bits, restated by
tests/_batched_policy_model.py: stamp_bits_of).  Two rules read it: sa_pick8 does not take a way whose stamp equals the running
batch's as a victim, and the one-launch form of evs_cache_lookup_interact (csrc/evs_fused_rf.hip, csrc/evs_fused_rfq.hip:
sa_find(..., pend_stamp)) hides such a way from its probers.  Modulo 2^S both also meet a way filled k 2^S batches ago.  The
geometries here (M.WRAP_GEOMETRIES) make 2^S 16 and 256 batches, so a run of a few hundred batches wraps many times:
  * the two-launch chain (S = 4: the one-launch form is not taken below 8 stamp bits) keeps strict snapshot flags and every
    invariant of include/evstore_hip.h ("WHAT IS THE SAME") on every batch;
  * the one-launch form (S = 8) reports a resident key as a miss in exactly the cases the header lists, the third one -- a way
    filled k 256 batches ago -- pinned deterministically on keys that never leave the cache.
Where the form ends (23 tag bits): tests/test_gpu_batched_lru_lfu.py, beside the other refusals."""
import numpy as np
import pytest
import torch

import _accuracy as acc
import _batched_policy_model as M

pytestmark = pytest.mark.gpu

D = 36


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


@pytest.fixture(scope="module")
def tables():
    """(geometry, codec) -> the tables of one of M.WRAP_GEOMETRIES, filled on the device (fp32 uniform in (-1, 1); codec 8: raw
    random bytes); freed behind the module"""
    made = {}

    def get(geom, codec=32):
        if (geom, codec) not in made:
            g = torch.Generator(device="cuda")
            g.manual_seed(7 + codec)
            n_rows = M.WRAP_GEOMETRIES[geom][1]
            if codec == 32:
                made[geom, codec] = [torch.empty(n, D, device="cuda").uniform_(-1, 1, generator=g) for n in n_rows]
            else:
                made[geom, codec] = [torch.randint(0, 256, (n, D), dtype=torch.uint8, device="cuda", generator=g) for n in n_rows]
        return made[geom, codec]
    yield get
    made.clear()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _gather(dev, rq):
    """the requested rows of every table, gathered on the device and copied back: T arrays of (B, ...)"""
    return [dev[t][_dev(rq[:, t].astype(np.int64))].cpu().numpy() for t in range(rq.shape[1])]


def _residents(c, cap, nset, n_rows, bits):
    """-> ({key: priority}, statistics), the dump held to them: no duplicate keys, size <= capacity, the histogram, no set
    above its ways"""
    d = c.batch_dump()
    keys = [(int(t), int(rw)) for _, t, rw in d]
    st = c.batch_stats()
    assert len(set(keys)) == len(keys) == st["size"] <= cap
    assert np.array_equal(np.bincount(d[:, 0], minlength=len(n_rows) + 1), np.array(st["hist"]))
    if keys:
        per_set = np.bincount(M.set_of([t - 1 for t, _ in keys], [r for _, r in keys], nset, n_rows, bits), minlength=nset)
        assert per_set.max() <= M.WAYS
    return {k: int(p) for k, p in zip(keys, d[:, 0])}, st


def _keys_of(rq):
    return [[(t + 1, int(rq[b, t])) for t in range(rq.shape[1])] for b in range(len(rq))]


# ------------------------------------------------------------------------------------------------- the two-launch chain
@pytest.mark.parametrize("form", ["lookup_batch", "lookup_interact"])
def test_evlfu_chain_keeps_snapshot_flags_across_wraps(E, tables, form):
    """`tiny`: two sets of 8 ways, 22 tag bits, S = 4 -- the stamp wraps every 16 batches, 96 batches wrap it six times.  An
    explicit "setassoc" tier; lookup_interact has fewer than 8 stamp bits here, so it must NOT take the one-launch form: under
    either entry point the flags equal residency at arrival on every batch.  Zipf rows over a few hot keys per table (they
    fight over 16 ways: the stream is not conflict-free), and a last column that never repeats a row, so no request is a
    perfect hit and nothing flushes.  Behind every batch: no duplicate keys, size <= capacity, histogram = dump, priorities
    of the keys that stayed never fall, a missed key is absent only if its set is full; lookup_batch's rows are the table
    rows bit for bit, lookup_interact's R meets the float64 reference."""
    cap, n_rows, S = M.WRAP_GEOMETRIES["tiny"]
    T, n_batches, B = len(n_rows), 96, 6
    assert M.stamp_bits_of("evlfu", cap, n_rows) == (22, 0, 4) == (22, 0, S["evlfu"]) and n_batches >= 80
    nset, bits = M.geometry(cap, n_rows)
    dev = tables("tiny")
    rs = np.random.RandomState(17)
    perms = [rs.permutation(n)[:64] for n in n_rows]
    c = E.GpuCache("evlfu", cap, T, D, 32, "python").set_batch_policy("setassoc")
    c.set_backing(dev)
    x_np = rs.uniform(-1, 1, size=(B, D)).astype(np.float32)
    x = _dev(x_np)
    res, st = {}, {"n_evict": 0}
    n_hits = 0
    for n in range(1, n_batches + 1):
        rq = np.stack([M.zipf_rows(rs, 64, B, 1.2, perms[t]) for t in range(T)], 1).astype(np.int32)
        rq[:, T - 1] = 1000 + (n - 1) * B + np.arange(B)                # never the same row twice
        rows = _gather(dev, rq)
        if form == "lookup_batch":
            hit, out = c.lookup_batch(_dev(rq))
            out = out.cpu().numpy()
            for t in range(T):
                assert np.array_equal(out[:, t].view(np.uint32), rows[t].view(np.uint32)), "batch %d table %d" % (n, t)
        else:
            hit, R = c.lookup_interact(_dev(rq), x, itself=bool(n & 1))
            ref = acc.Reference(x_np, [acc.pool64(r)[:2] for r in rows], bool(n & 1))
            acc.check(R.cpu().numpy(), ref, "evlfu tiny batch %d" % n, "the chain's interaction consumer")
        hit = hit.cpu().numpy().astype(bool)
        keys = _keys_of(rq)
        was = np.array([[k in res for k in row] for row in keys])
        assert np.array_equal(hit, was), "batch %d (stamp residue %d): flags != residency at arrival" % (n, (n + 1) % 16)
        n_hits += int(hit.sum())
        after, st = _residents(c, cap, nset, n_rows, bits)
        assert all(after[k] >= p for k, p in res.items() if k in after), "batch %d: a priority fell" % n
        gone = sorted({k for row in keys for k in row if k not in after})
        if gone:
            per_set = np.bincount(M.set_of([t - 1 for t, _ in after], [r for _, r in after], nset, n_rows, bits), minlength=nset)
            assert (per_set[M.set_of([t - 1 for t, _ in gone], [r for _, r in gone], nset, n_rows, bits)] == M.WAYS).all()
        res = after
    assert st["n_flush"] == 0 and st["n_hits"] == n_hits and st["n_requests"] == n_batches * B
    assert n_hits > n_batches and st["n_evict"] > 4 * cap            # (hits and replacements all along)


# -------------------------------------------------------------------------------------------------- the one-launch form
@pytest.mark.parametrize("codec", [32, 8])
def test_evlfu_one_launch_form_hides_a_way_filled_256_batches_ago(E, orc, tables, codec):
    """`inline`: 26 x 40 000 rows under 16 sets, 17 tag bits, two-copy arena, S = 8 -- stamp_mask = 255, the smallest for
    which evs_cache_lookup_interact makes the update inside its launch (codec 8: csrc/evs_fused_rfq.hip).  820 batches of 16
    wrap the stamp three times.  Sample 0 of every batch asks for the same 20 ANCHOR keys; they live in sets 0..7 beside at
    most three of the 50 HOT keys all other columns draw from, so those sets never need a victim: the anchors reach priority
    20 and more and never leave.  (An EvLFU victim is the lowest priority among the ways the running batch has not filled;
    a set that takes more new keys in a batch than it has other ways gives up its best key too -- so the stream keeps the
    new keys away from the anchors' sets.)  Sets 8..15 hold the other hot keys and take sixteen new keys per batch.
    The last column never repeats a row: no perfect hit, no flush.  The fill batch of every resident key is tracked from
    the dumps (a resident key flagged 0 is, hidden or retired and inserted again, stamped like batch n afterwards).
      flag = 1  => resident at arrival;
      a resident key flagged 0 was retired by this batch's inserts -- at most as many keys as the batch evicted -- or was
                filled k 256 batches ago: (n - fill) % 256 == 0;
      every anchor is flagged 0 at exactly the batches with (n - fill) % 256 == 0 and 1 at all others;
      R meets the float64 reference over the true rows every 50th batch and on the wrap batches; n_hits = the flags seen."""
    cap, n_rows, S = M.WRAP_GEOMETRIES["inline"]
    T, B, n_batches, n_anchor = len(n_rows), 16, 820, 20
    assert M.stamp_bits_of("evlfu", cap, n_rows) == (17, 1, 8) == (17, 1, S["evlfu"]) and n_batches >= 800
    nset, bits = M.geometry(cap, n_rows)
    dev = tables("inline", codec)
    rs = np.random.RandomState(23)
    # anchor t: a row of table t in set t mod 8.  Hot keys: two rows per column 0..24, at most three of them in any of the sets
    # 0..7 (with at most three anchors that leaves two ways free) and at most four in any of the sets 8..15.  The last
    # column: rows of sets 8..15, each row once.
    sets_of_table = [M.set_of(t, np.arange(n_rows[t]), nset, n_rows, bits) for t in range(T)]
    anchor_rows = [int(np.nonzero(sets_of_table[t][:2000] == t % 8)[0][0]) for t in range(n_anchor)]
    anchors = [(t + 1, r) for t, r in enumerate(anchor_rows)]
    slots = rs.permutation(list(range(8)) * 3 + list(range(8, 16)) * 4)[:2 * (T - 1)].reshape(T - 1, 2)
    hot = np.array([[2000 + int(np.nonzero(sets_of_table[t][2000:4000] == s)[0][k]) for k, s in enumerate(slots[t])] for t in range(T - 1)])
    fresh = iter((4000 + np.nonzero(sets_of_table[T - 1][4000:] >= 8)[0]).tolist())
    c = E.GpuCache("evlfu", cap, T, D, codec, "python").set_batch_policy("setassoc")
    c.set_backing(dev)
    x_np = rs.uniform(-1, 1, size=(B, D)).astype(np.float32)
    x = _dev(x_np)
    res, st = {}, {"n_evict": 0}
    fill, flags_seen, hidden_seen, retired_seen, wrap_batches = {}, 0, 0, 0, []
    for n in range(1, n_batches + 1):
        rq = np.zeros((B, T), np.int32)
        rq[:, :T - 1] = np.take_along_axis(hot.T, rs.randint(0, 2, size=(B, T - 1)), 0)
        rq[0, :n_anchor] = anchor_rows
        rq[:, T - 1] = [next(fresh) for _ in range(B)]                  # never the same row twice: no perfect hit, no flush
        hit, R = c.lookup_interact(_dev(rq), x)
        hit = hit.cpu().numpy().astype(bool)
        flags_seen += int(hit.sum())
        keys = _keys_of(rq)
        was = np.array([[k in res for k in row] for row in keys])
        assert not (hit & ~was).any(), "batch %d: a hit flag on a key that was not resident" % n
        lost = {k for row, hrow, wrow in zip(keys, hit, was) for k, h, w in zip(row, hrow, wrow) if w and not h}
        lapped = {k for k in lost if (n - fill[k]) % 256 == 0}
        after, st1 = _residents(c, cap, nset, n_rows, bits)
        assert len(lost - lapped) <= st1["n_evict"] - st["n_evict"], "batch %d: %s" % (n, sorted(lost - lapped))
        hidden_seen += len(lapped)
        retired_seen += len(lost - lapped)
        for a in anchors:                                               # the deterministic pin
            if n == 1:
                continue
            assert a in res and a in after, "batch %d: anchor %s left the cache" % (n, a)
            want_hidden = (n - fill[a]) % 256 == 0
            assert hit[0, a[0] - 1] == (not want_hidden), "batch %d: anchor %s filled by batch %d, flag %d" % (n, a, fill[a], hit[0, a[0] - 1])
        if any((n - fill[a]) % 256 == 0 for a in anchors if a in fill):
            wrap_batches.append(n)
        if n % 50 == 0 or wrap_batches[-1:] == [n]:
            rows = _gather(dev, rq)
            if codec == 32:
                ref = acc.Reference(x_np, [acc.pool64(r)[:2] for r in rows], False)
            else:   # (the integer pipe of the u8 consumer: its own term of the bound, as tests/test_gpu_accuracy.py holds it)
                cc = np.stack(rows, 1).astype(np.int64)
                ref = acc.Reference(x_np, [acc.pool64(orc.decode(r, 8, D))[:2] for r in rows], False, 1, acc.u8_delta()[cc], cc)
            acc.check(R.cpu().numpy(), ref, "evlfu inline codec %d batch %d" % (codec, n), "the one-launch form, codec %d" % codec)
        for k in after:
            if k not in res or k in lost:
                fill[k] = n
        for k in res:
            if k not in after:
                del fill[k]
        res, st = after, st1
    assert wrap_batches == [257, 513, 769], wrap_batches                # (anchors: filled by batch 1, hidden every 256 batches)
    assert all(res[a] >= 15 for a in anchors)
    assert st["n_hits"] == flags_seen and st["n_requests"] == n_batches * B and st["n_flush"] == 0
    assert hidden_seen >= 3 * n_anchor and st["n_evict"] > 10 * cap
    print("codec %d: resident keys reported as misses: %d because their fill residue matched, %d retired by the batch's own inserts"
          % (codec, hidden_seen, retired_seen))
