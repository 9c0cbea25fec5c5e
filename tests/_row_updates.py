"""Shared pieces of the row-update tests (tests/test_row_updates_host.py, tests/test_gpu_row_updates.py and its
EVS_SA_WAYS=16 child process): the delta of the golden-trace protocol, and the batched-tier case."""
import numpy as np

T, D = 26, 36


def unpack(packed, n):
    return np.unpackbits(packed, axis=1)[:, :T].astype(bool)[:n]


def golden_final(t, policy, cap, dump):
    if policy == "evlfu":
        np.testing.assert_array_equal(dump, t["evlfu_cap%d_final_buckets" % cap])
    elif policy == "lru":
        np.testing.assert_array_equal(dump[:, 1:], t["lru_cap%d_final_order" % cap])
    else:
        np.testing.assert_array_equal(dump, t["lfu_cap%d_final_freq" % cap])


def make_delta(dump, reqs2, n_rows, rs, n_res=96, n_non=96, must=()):
    """-> keys (n, 2) int64 of (table 0-based, row): resident ones first (from `dump`; keys that reqs2 asks for in front),
    then non-resident ones (`must` first); and the three counts the protocol asserts: resident, non-resident, requested later"""
    resident = {(int(a) - 1, int(b)) for a, b in dump[:, 1:]}
    later = [(k, int(r)) for rq in reqs2 for k, r in enumerate(rq)]
    res_later = [kr for kr in later if kr in resident]
    res = list(dict.fromkeys(res_later[:8] + sorted(resident)))[:n_res]
    non = [kr for kr in dict.fromkeys(must) if kr not in resident]
    res += [kr for kr in dict.fromkeys(must) if kr in resident and kr not in res]
    while len(non) < n_non:
        k = int(rs.randint(0, len(n_rows)))
        r = int(rs.randint(0, n_rows[k]))
        if (k, r) not in resident and (k, r) not in non:
            non.append((k, r))
    keys = np.array(res + non, np.int64)
    later = set(later)
    return keys, len(res), len(non), sum(1 for kr in res + non if kr in later)


def zipf_requests(n_rows, n_req, seed, alpha=1.15):
    rs = np.random.RandomState(seed)
    perms = [rs.permutation(n) for n in n_rows]
    reqs = np.zeros((n_req, len(n_rows)), np.int32)
    for k, n in enumerate(n_rows):
        reqs[:, k] = perms[k][np.minimum(rs.zipf(alpha, n_req) - 1, n - 1)]
    hot = reqs[rs.randint(0, n_req, 64)]
    rep = rs.rand(n_req) < 0.3
    reqs[rep] = hot[rs.randint(0, 64, rep.sum())]
    return reqs


def batch_of(keys_by_table, fill_by_table, B, rs):
    """(B, T) int32 requests whose position (b, k) is a row of keys_by_table[k] (cycled through, so every one is asked for
    when B allows) or, where that list is empty, of fill_by_table[k]; and the mask of the positions of the first kind"""
    n_t = len(keys_by_table)
    rq = np.zeros((B, n_t), np.int32)
    mask = np.zeros((B, n_t), bool)
    for k in range(n_t):
        src = keys_by_table[k]
        if len(src):
            rq[:, k] = np.resize(np.asarray(src, np.int32), B)
            mask[:, k] = True
        else:
            rq[:, k] = np.asarray(fill_by_table[k], np.int32)[rs.randint(0, len(fill_by_table[k]), B)]
    return rq, mask


def batched_case(E, orc, policy, inline, codec, log=None):
    """One batched tier (codec 32 or 8, T = 26, d = 36) over a Zipf stream warmed past its capacity; a delta of >= 256 resident
    and >= 256 non-resident keys through GpuCache.update_rows: the resident count, the policy state (batch_dump as a set,
    batch_stats) unchanged, the table bytes, then lookups of resident-only and of non-resident delta keys through
    lookup_batch and lookup_interact: the new rows bit for bit, hit 1 / hit 0."""
    import torch
    import _accuracy as acc
    n_rows = [3000, 40, 20000, 700, 5, 9000, 1500, 12, 26000, 300, 8000, 64, 2200, 17000, 3, 450, 5000, 90, 13000,
              2, 7000, 30, 1000, 11000, 150, 4000]
    fp32 = orc.kaggle_tables(n_rows, 21)
    if codec == 32:
        mirror = [np.array(w, np.float32).view(np.uint8).reshape(len(w), -1) for w in fp32]
    else:
        mirror = [orc.encode_table(np.clip(w * 8, -1, 1), codec) for w in fp32]
    dev = [torch.from_numpy(m.copy()).cuda() for m in mirror]
    reqs = zipf_requests(n_rows, 4096, 2, alpha=1.08)
    uniq = {(k, int(r)) for rq in reqs for k, r in enumerate(rq)}
    cap = max(4096, len(uniq) // 2 // 16 * 16)
    assert len(uniq) > cap, "the stream does not run past the capacity"
    c = E.GpuCache("evlfu", cap, T, D, codec, "python").set_batch_policy(policy)
    if inline is not None:
        c.set_inline_update(inline)
    c.set_backing(dev)
    r = torch.from_numpy(reqs).cuda()
    xw = torch.rand(512, D, device="cuda")
    for i, s in enumerate(range(0, len(reqs), 512)):   # both consumers take part in the warm-up
        if i % 2:
            c.lookup_batch(r[s:s + 512].contiguous())
        else:
            c.lookup_interact(r[s:s + 512].contiguous(), xw)
    dump0, stats0 = c.batch_dump(), c.batch_stats()
    assert stats0["n_evict"] > 0 or stats0["size"] >= cap * 0.6, stats0
    resident = sorted({(int(t) - 1, int(rw)) for _, t, rw in dump0})
    rs = np.random.RandomState(11)
    res = [resident[i] for i in rs.choice(len(resident), 384, replace=False)]
    # every table takes part in the resident-only batch: at least one resident key of each in the delta
    for k in range(T):
        if not any(t == k for t, _ in res):
            res.append(next(kr for kr in resident if kr[0] == k))
    rset = set(resident)
    non = []
    while len(non) < 384:
        k = int(rs.randint(0, T))
        rw = int(rs.randint(0, n_rows[k]))
        if (k, rw) not in rset and (k, rw) not in non:
            non.append((k, rw))
    assert len(res) >= 256 and len(non) >= 256
    keys = np.array(res + non, np.int64)
    vals = rs.uniform(-1, 1, size=(len(keys), D)).astype(np.float32)
    vals[0, :3] = [0.0, 1.0, -1.0]
    enc = orc.encode_table(vals, codec)
    for (k, rw), e in zip(keys, enc):
        mirror[k][rw] = e
    n_res = c.update_rows(torch.from_numpy(keys).cuda(), torch.from_numpy(vals).cuda(), count=True)
    if log is not None:
        log("resident count %d (want %d)" % (n_res, len(res)))
    assert n_res == len(res)
    dump1, stats1 = c.batch_dump(), c.batch_stats()
    assert {tuple(v) for v in dump1.tolist()} == {tuple(v) for v in dump0.tolist()} and len(dump1) == len(dump0)
    assert stats1 == stats0
    for k in range(T):
        assert np.array_equal(dev[k].cpu().numpy(), mirror[k]), "table %d" % k

    def rows_of(k, ids):
        return orc.decode(mirror[k][ids], codec, D)

    def check_interact(R, x, rq, case):
        feats = [acc.pool64(rows_of(k, rq[:, k]))[:2] for k in range(T)]
        if codec == 8:
            cc = np.stack([mirror[k][rq[:, k]] for k in range(T)], 1).astype(np.int64)
            ref = acc.Reference(x, feats, False, 1, acc.u8_delta()[cc], cc)
        else:
            ref = acc.Reference(x, feats, False)
        acc.check(R, ref, case, "GpuCache.lookup_interact after update_rows")

    # every updated resident key is read back: the batch is as long as the longest per-table list of them
    res_by_t = [[rw for t, rw in res if t == k] for k in range(T)]
    B = max(64, max(len(v) for v in res_by_t))
    rq, _ = batch_of(res_by_t, [[0]] * T, B, rs)
    assert {(k, int(v)) for k in range(T) for v in rq[:, k]} == set(res)
    x = rs.uniform(-1, 1, size=(B, D)).astype(np.float32)
    hit, out = c.lookup_batch(torch.from_numpy(rq).cuda())
    assert bool(hit.cpu().numpy().all()), "a resident key was not a hit"
    out = out.cpu().numpy()
    for k in range(T):
        assert np.array_equal(out[:, k, :].view(np.uint32), rows_of(k, rq[:, k]).view(np.uint32)), "resident rows, table %d" % k
    hit, R = c.lookup_interact(torch.from_numpy(rq).cuda(), torch.from_numpy(x).cuda())
    assert bool(hit.cpu().numpy().all())
    check_interact(R.cpu().numpy(), x, rq, "%s inline=%s codec %d resident-only" % (policy, inline, codec))
    # the non-resident delta keys: served from the table, which holds the new rows
    other = [[rw for t, rw in resident if t == k][:4] for k in range(T)]
    non_by_t = [[rw for t, rw in non if t == k] for k in range(T)]
    B = max(64, max(len(v) for v in non_by_t))
    rq, mask = batch_of(non_by_t, other, B, rs)
    assert {(k, int(v)) for k in range(T) for v in rq[:, k] if mask[0, k]} == set(non)
    hit, out = c.lookup_batch(torch.from_numpy(rq).cuda())
    hit, out = hit.cpu().numpy().astype(bool), out.cpu().numpy()
    assert mask.sum() >= 256 and not hit[mask].any(), "a non-resident key was a hit"
    for k in range(T):
        assert np.array_equal(out[:, k, :].view(np.uint32), rows_of(k, rq[:, k]).view(np.uint32)), "non-resident rows, table %d" % k
    return n_res
