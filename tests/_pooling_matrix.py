"""Shared by tests/test_gpu_pooling_matrix.py and its child (tests/_pooling_matrix_env_child.py): tables, bags, one pooling call
straight through the C ABI under the dispatch record (evs_gather_kernels_seen), and the oracle's result laid out like the call's
output.  Everything is compared as bits; there is no tolerance here."""
import ctypes as C

import numpy as np
import torch

N_ROWS = (1, 3, 40, 700)
SENTINEL = 0x7FC0DEAD          # (a NaN no sum produces: what the output holds where the call must not write)
LONG_K = {16: 8, 32: 8, 36: 9, 64: 16, 128: 16}
ROWS_NJ = {16: (1, 2), 32: (1, 2, 3, 4), 36: (1, 2, 3, 4), 64: (2, 4, 7)}   # the instruction counts gather_rows_kernel is compiled for
VEC_LPR = (4, 8, 9, 16, 32)                                                 # the lanes per row embedding_bag_sum_kernel is compiled for


# ---- the names of the record, from the dispatch rules as include/evstore_hip.h states them ----------------------------------------
def rows_name(codec, d, T, declared):
    need = -(-T // (64 // (d // 4)))
    return "rows_c%d_lpr%d_nj%d_%s" % (codec, d // 4, min(n for n in ROWS_NJ[d] if n >= need), "declared" if declared else "check")


def long_name(d):
    return "long_c32_lpr%d_k%d" % (d // 4, LONG_K[d])


def flat_name(d, select):
    return "flat_c32_lpr%d_%s" % (d // 4, "select" if select else "plain")


def vec_name(codec, d, bag1):
    return "vec_c%d_lpr%d_%s" % (codec, d // 4 if d // 4 in VEC_LPR else 0, "bag1" if bag1 else "offsets")


def scalar_name(codec):
    return "scalar_c%d" % codec


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def make_tables(orc, rs, T, d, codec):
    """T tables of 1, 3, 40, 700, 1, ... rows: fp32 (n, d) arrays, or the raw rows of the codec (a few u16 tail codes patched in)"""
    tabs = []
    for k in range(T):
        w = rs.uniform(-1, 1, size=(N_ROWS[k % 4], d)).astype(np.float32)
        if codec == 32:
            tabs.append(w)
            continue
        raw = np.ascontiguousarray(orc.encode_table(w, codec))
        if codec == 16:
            codes = raw.reshape(-1).view(np.uint16)
            m = min(4, codes.size)
            codes[:m] = [0, 65000, 65001, 65535][:m]
        tabs.append(raw)
    return tabs


def make_bags(rs, tabs, lens):
    """lens: (T, B) bag lengths -> (idx, off) lists"""
    idx, off = [], []
    for k, t in enumerate(tabs):
        ln = np.asarray(lens[k], np.int64)
        o = np.zeros(ln.size, np.int64)
        o[1:] = np.cumsum(ln)[:-1]
        off.append(o)
        idx.append(rs.randint(0, t.shape[0], size=int(ln.sum())).astype(np.int64))
    return idx, off


def one_index_bags(rs, tabs, B):
    return [rs.randint(0, t.shape[0], size=B).astype(np.int64) for t in tabs]


def make_weights(rs, tabs, which):
    """per-row weights for the tables of `which`, None for the others: 0, -1, 2^-20 and values above 1 among them"""
    out = []
    for k, t in enumerate(tabs):
        if k not in which:
            out.append(None)
            continue
        w = rs.choice(np.array([0.0, -1.0, 2.0 ** -20, 1.5, 3.25, 0.75, -2.5], np.float32), size=t.shape[0]).astype(np.float32)
        out.append(w)
    return out


def mid_ranges(tabs):
    """a row range per table with row_lo > 0 wherever the table has more than one row"""
    out = []
    for t in tabs:
        n = t.shape[0]
        lo = n // 4 + (1 if n > 1 else 0)
        out.append((lo, max(1, min(n - lo, n // 2))))
    return out


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def reference(orc, B, d, codec, tabs, idx, off, weights=None, ranges=None):
    """The oracle's pooled rows, list of T (B, d): index order, unfused fp32 multiply and add.  Entries outside the table's row range
    (another shard's rows -- or, in the guard cases, indices outside the table) are removed from their bags first and the offsets
    rebuilt, the way the existing multi-hot test drops entries."""
    out = []
    for k, t in enumerate(tabs):
        o = np.arange(B, dtype=np.int64) if off is None else off[k]
        i = idx[k][:B] if off is None else idx[k]
        lo, nl = (0, t.shape[0]) if ranges is None else ranges[k]
        keep = (i >= lo) & (i < lo + nl)
        before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
        w = None if weights is None or weights[k] is None else weights[k][lo:lo + nl]
        out.append(orc.embedding_bag_sum(t[lo:lo + nl], i[keep] - lo, before[o], w, codec, d))
    return out


def lay_out(ref, B, d, layout, bpp=0, delta=False):
    """the flat output buffer a call with this layout must leave behind (uint32 bits; SENTINEL where nothing is written),
    and (float offset of `out`, table stride, bag stride, peer stride, peer deltas or None)"""
    T = len(ref)
    if layout == "list":
        buf = np.stack(ref).view(np.uint32).reshape(-1).copy()
        return buf, (0, B * d, d, 0, None)
    if layout == "tile":                       # the (B, F, d) interaction tile, F = T + 1: feature 0 is not the gather's
        buf = np.full((B, T + 1, d), SENTINEL, np.uint32)
        for k in range(T):
            buf[:, k + 1, :] = ref[k].view(np.uint32)
        return buf.reshape(-1), (d, d, (T + 1) * d, 0, None)
    assert layout == "peer" and 0 < bpp < B
    P = -(-B // bpp)
    buf = np.full((2 if delta else 1, P, T, bpp, d), SENTINEL, np.uint32)
    dl = [(P + (P - 1 - 2 * q)) * T * bpp * d for q in range(P)] if delta else None   # peer q's block: the second half, peers reversed
    for b in range(B):
        q = b // bpp
        for k in range(T):
            if delta:
                buf[1, P - 1 - q, k, b % bpp] = ref[k][b].view(np.uint32)
            else:
                buf[0, q, k, b % bpp] = ref[k][b].view(np.uint32)
    return buf.reshape(-1), (0, bpp * d, d, T * bpp * d, dl)


# ---- one call ---------------------------------------------------------------------------------------------------------------------
def pool(E, B, d, codec, tabs, idx, off, weights=None, ranges=None, layout="list", bpp=0, delta=False):
    """evs_embedding_bag_sum_sharded (evs_embedding_bag_sum_p2p with peer deltas) on the default stream -> the whole output buffer as
    uint32 bits.  off None: one index per bag declared.  The sticky index flag is NOT read here."""
    L = E._lib.lib()
    T = len(tabs)
    hold = []

    def up(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        hold.append(t)
        return t

    def ptrs(ts):
        return (C.c_void_p * T)(*[None if (t is None or t.numel() == 0) else t.data_ptr() for t in ts])

    rg = [(0, t.shape[0]) for t in tabs] if ranges is None else ranges
    tab_c = ptrs([up(t[lo:lo + nl]) for t, (lo, nl) in zip(tabs, rg)])
    idx_c = ptrs([up(i) for i in idx])
    off_c = None if off is None else ptrs([up(o) for o in off])
    w_c = None if weights is None else ptrs([None if w is None else up(w[lo:lo + nl]) for w, (lo, nl) in zip(weights, rg)])
    i64 = lambda v: (C.c_int64 * T)(*[int(x) for x in v])
    n_rows_c, nnz_c = i64([nl for _, nl in rg]), i64([i.size for i in idx])
    lo_c = None if ranges is None else i64([lo for lo, _ in rg])
    tot_c = None if ranges is None else i64([t.shape[0] for t in tabs])
    want_shape, (foff, tstride, bstride, pstride, dl) = lay_out([np.zeros((B, d), np.float32)] * T, B, d, layout, bpp, delta)
    buf = torch.full((want_shape.size,), SENTINEL, dtype=torch.int32, device="cuda")
    out_p = buf.data_ptr() + 4 * foff
    if dl is None:
        rc = L.evs_embedding_bag_sum_sharded(T, B, d, codec, tab_c, n_rows_c, lo_c, tot_c, idx_c, off_c, nnz_c, w_c, out_p, tstride, bstride,
                                             pstride, bpp, None)
    else:
        dl_t = up(np.asarray(dl, np.int64))
        rc = L.evs_embedding_bag_sum_p2p(T, B, d, codec, tab_c, n_rows_c, lo_c, tot_c, idx_c, off_c, nnz_c, w_c, out_p, tstride, bstride,
                                         pstride, bpp, dl_t.data_ptr(), None)
    E._lib.check(rc)
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint32)


def index_flag(E):
    """evs_check_index_errors on the default stream: the return code (reading a raised flag clears it)"""
    return E._lib.lib().evs_check_index_errors(None)


def check_case(E, orc, want_names, B, d, codec, tabs, idx, off, weights=None, ranges=None, layout="list", bpp=0, delta=False):
    """One case under the module's two rules: exactly `want_names` ({name: launches}) went up in the record, and the output buffer holds
    the oracle's bits (and is untouched everywhere else).  No index error may be flagged."""
    before = E._lib.gather_kernels_seen()
    got = pool(E, B, d, codec, tabs, idx, off, weights, ranges, layout, bpp, delta)
    after = E._lib.gather_kernels_seen()
    went_up = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert went_up == want_names, (went_up, want_names)
    assert index_flag(E) == 0, "a valid batch raised the index flag"
    want, _ = lay_out(reference(orc, B, d, codec, tabs, idx, off, weights, ranges), B, d, layout, bpp, delta)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError("%d of %d output words differ from the oracle's bits, first at %d: %08x != %08x (%s)" % (
            bad.size, want.size, bad[0], got[bad[0]], want[bad[0]], sorted(want_names)))
    return got
