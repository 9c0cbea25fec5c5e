"""GPU: the request line of both resident servers (csrc/evs_mailbox.h) at the table counts where its layout changes -- T = 1,
7 / 8 (the first sector boundary), 26 (the last count at which a destination address rides in words 29 / 30, also driven with
request_to from host ids and from device ids) and 28 (words 29 / 30 carry the ids of tables 26 and 27).  Every request's hit
flags / tier codes and rows bit-equal to a twin cache driven by the launch-per-call form (request / request_c1c2, which the
oracle tests hold), and the final stats() equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ROWS, D, N_REQ = 64, 36, 48
CASES = [(1, "ring"), (7, "ring"), (8, "ring"), (26, "ring"), (28, "ring"), (26, "to_host"), (26, "to_dev")]


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available()
    E._lib.lib()
    return E


@pytest.fixture(scope="module")
def data():
    """tables of 64 rows x 36 for 28 tables (fp32 and their 8- / 4-bit encodings) and 48 requests: half the ids from 8 hot rows"""
    from oracle import oracle as orc
    rs = np.random.RandomState(26)
    ws = [rs.uniform(-1, 1, size=(N_ROWS, D)).astype(np.float32) for _ in range(28)]
    hot = rs.randint(0, 8, size=(N_REQ, 28))
    reqs = np.where(rs.rand(N_REQ, 28) < 0.5, hot, rs.randint(0, N_ROWS, size=(N_REQ, 28))).astype(np.int32)
    return dict(fp32=ws, raw8=[orc.encode_table(w, 8) for w in ws], raw4=[orc.encode_table(w, 4) for w in ws], reqs=reqs)


def _post(request, request_to, T, mode, rq):
    """one request the way `mode` says -> (flags, (T, D) rows on the device)"""
    if mode == "ring":
        return request(rq)
    if mode == "to_host":
        rows = torch.full((T, D), -7.0, dtype=torch.float32, device="cuda")
        ids = rq
    else:
        rows = torch.full((T, 1, D), -7.0, dtype=torch.float32, device="cuda")
        ids = torch.from_numpy(np.stack([rq.astype(np.int64), np.full(T, -1, np.int64)], 1)).cuda()   # (T, 2): element 0 is the id
    torch.cuda.synchronize()
    return request_to(ids, rows), rows.reshape(T, D)


def _compare(T, mode, reqs, want_flags, want_rows, request, request_to):
    for i, rq in enumerate(reqs):
        flags, rows = _post(request, request_to, T, mode, rq)
        assert np.array_equal(np.asarray(flags), want_flags[i]), (i, flags, want_flags[i])
        assert np.array_equal(rows.cpu().numpy().view(np.uint32), want_rows[i].view(np.uint32)), i


@pytest.mark.parametrize("T,mode", CASES)
def test_single_tier_server_equals_the_launch_per_call_twin(E, data, T, mode):
    reqs = np.ascontiguousarray(data["reqs"][:, :T])

    def make():
        c = E.GpuCache("evlfu", 40, T, D, 32, "python")
        c.set_backing([torch.from_numpy(w).cuda() for w in data["fp32"][:T]])
        return c
    twin, c = make(), make()
    hit, out = twin.request(torch.from_numpy(reqs).cuda())
    torch.cuda.synchronize()
    want_stats = twin.stats()
    assert want_stats["n_evict"] + want_stats["n_flush"] > 0 or T == 1   # (capacity 40: T x 48 keys over 64 rows per table do not fit)
    c.serve_start(n_slots=3, idle_us=300)
    try:
        _compare(T, mode, reqs, hit.cpu().numpy(), out.cpu().numpy(), c.serve_request, c.serve_request_to)
    finally:
        c.serve_stop()
    assert c.stats() == want_stats


@pytest.mark.parametrize("T,mode", CASES)
def test_tier_pair_server_equals_the_launch_per_call_twin(E, data, T, mode):
    from evstore_dlrm_amd import gpu_cache
    reqs = np.ascontiguousarray(data["reqs"][:, :T])
    thr = max(1, (3 * T) // 4)

    def make():
        c1 = E.GpuCache("evlfu", 32, T, D, 8, "cpp")
        c2 = E.GpuCache("evlfu", 48, T, D, 4, "cpp")
        c1.set_backing([torch.from_numpy(r).cuda() for r in data["raw8"][:T]])
        c2.set_backing([torch.from_numpy(r).cuda() for r in data["raw4"][:T]])
        return c1, c2
    (t1, t2), (c1, c2) = make(), make()
    tier, out = gpu_cache.request_c1c2(t1, t2, torch.from_numpy(reqs).cuda(), threshold=thr)
    torch.cuda.synchronize()
    want1, want2 = t1.stats(), t2.stats()
    srv = E.TierServer(c1, c2, None, threshold=thr, n_slots=3, idle_us=300)
    try:
        _compare(T, mode, reqs, tier.cpu().numpy(), out.cpu().numpy(), srv.request, srv.request_to)
        srv.stop()
        assert c1.stats() == want1 and c2.stats() == want2
    finally:
        srv.close()
