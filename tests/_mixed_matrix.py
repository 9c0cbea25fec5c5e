"""Shared by tests/test_gpu_mixed_matrix.py, its child (tests/_mixed_matrix_env_child.py) and the CPU test of the generators
(tests/test_mixed_matrix_cases.py): the case lists of the mixed-precision interaction consumers (csrc/evs_mixed.hip), one call through
evs_interact_rows_by_address under the dispatch record (evs_mixed_kernels_seen), and the one-hot decode probe.

The test chooses every row address and every class itself, so nothing about a result is the cache routing's choice: rows of the full
code range go to either class, inside one wave.  No GPU and no torch are needed to import this module or to build the case lists."""
import numpy as np

import _accuracy as acc
import _accuracy_data as AD

SENTINEL = 0x7FC0DEAD          # (a NaN no dot product produces: what R holds where the call must not write)
GUARD = 1024                   # floats behind R that must keep the sentinel
DIMS = (16, 32, 36)
KEY_T = (1, 14, 15, 16, 26, 27, 28, 31)
BATCHES = (1, 3, 15, 16, 17, 67)      # partial 16-sample blocks; waves of a block holding 0 .. 4 real samples
# interact_mixed_rows_kernel's grid is capped at kNumCu (256) * the blocks per CU the runtime reports, 4 samples (waves) per block: this B
# is past the cap for any occupancy <= 8 (the kernel's LDS use allows fewer), so waves take a second trip of the grid-stride loop
BIG_B = 4 * 256 * 8 + 5
BIG_AT = ((36, 26), (16, 1))
PATTERNS = ("rand", "c1", "c2", "d1", "d2")   # random class per (b, k) with zeros and null addresses; all 1; all 2; row_class NULL, default 1 / 2
KINDS = ("dlrm", "cancel", "samesign")
ROWS_PAIRS = ((32, 8), (32, 4), (16, 8), (16, 4), (32, 16), (16, 16))
SWEEP_PAIRS = ((32, 8), (16, 4))              # every T from 1 to 31 through interact_mixed_rows_kernel: each of its four chunk decoders
N_ROWS = 61                                   # rows per class buffer


def kernel_name(T, d, codecs, rfq_on=True):
    """the record name the dispatch rule (mixed84_supported: EVS_MIXED_RFQ, the pair (8, 4), T + 1 <= 28; NT = 2 from T + 1 > 16) gives"""
    r84 = rfq_on and tuple(codecs) == (8, 4) and T + 1 <= 28
    return "%s_d%d_nt%d" % ("r84" if r84 else "rows", d, 2 if T + 1 > 16 else 1)


ALL_NAMES = ["%s_d%d_nt%d%s" % (f, d, nt, s) for f, s in (("rows", ""), ("r84", ""), ("r84", "_probe")) for d in DIMS for nt in (1, 2)]


def row_bytes(codec, d):
    return d * codec // 8


# ---- the case lists ---------------------------------------------------------------------------------------------------------------
def _case(codecs, d, T, B, itself, pattern):
    return dict(codecs=tuple(codecs), d=d, T=T, B=B, itself=int(itself), pattern=pattern, kind=KINDS[(T + B) % 3],
                x_stride=d + 4 * (T % 3))       # (two of three T: x rows 16 / 32 bytes apart from dense)


def cases(codecs, d):
    """The covering subset for one codec pair and d (the full cross product is 39 060 calls):
    (8, 4), which the rows-in-registers kernel takes up to T = 27 and interact_mixed_rows_kernel from T = 28 (and, in the child, at every T):
      every T in 1 .. 31 x every B, random classes, itself = (T + B) & 1; at the key T also the other itself; at the key T, B = 16 and 67, the
      four uniform class patterns; the B past the grid cap at (d, T) = (36, 26) and (16, 1).
    the six pairs interact_mixed_rows_kernel takes: the key T x B = 1, 17, 67 with random classes, the key T at B = 16 with the uniform patterns;
      (32, 8) and (16, 4) -- all four chunk decoders -- also every T at B = 17; the big B as above for (32, 8) and (16, 4)."""
    out, seen = [], set()

    def add(T, B, itself, pattern):
        key = (T, B, int(itself), pattern)
        if key not in seen:
            seen.add(key)
            out.append(_case(codecs, d, T, B, itself, pattern))

    if tuple(codecs) == (8, 4):
        for T in range(1, 32):
            for B in BATCHES:
                add(T, B, (T + B) & 1, "rand")
        for T in KEY_T:
            for B in BATCHES:
                add(T, B, 1 - ((T + B) & 1), "rand")
            for B in (16, 67):
                for p in PATTERNS[1:]:
                    add(T, B, T & 1, p)
    else:
        for T in KEY_T:
            for B in (1, 17, 67):
                add(T, B, (T + B) & 1, "rand")
            for p in PATTERNS[1:]:
                add(T, 16, T & 1, p)
        if tuple(codecs) in SWEEP_PAIRS:
            for T in range(1, 32):
                add(T, 17, T & 1, "rand")
    if tuple(codecs) == (8, 4) or tuple(codecs) in SWEEP_PAIRS:
        for dd, T in BIG_AT:
            if dd == d:
                add(T, BIG_B, 1, "rand")
    return out


def classes(rs, B, T, pattern):
    """-> (row_class (B, T) uint8 or None, default_class, null (B, T) bool: the address is 0 although the class is not)"""
    null = np.zeros((B, T), bool)
    if pattern == "rand":
        cls = rs.choice(3, size=(B, T), p=[0.10, 0.45, 0.45]).astype(np.uint8)
        null = (rs.rand(B, T) < 0.05) & (cls != 0)
        for lo, hi in HALVES(T):   # a half of 2 or 3 rows: a draw seldom holds both classes there, so its first two rows are a chosen split
            if 2 <= hi - lo < 4:
                cls[0::2, lo], cls[0::2, lo + 1] = 1, 2
                cls[1::2, lo], cls[1::2, lo + 1] = 2, 1
                null[:, lo:lo + 2] = False
        return cls, 1, null
    if pattern in ("c1", "c2"):
        return np.full((B, T), int(pattern[1]), np.uint8), 1, null
    return None, int(pattern[1]), null


def HALVES(T):
    """the halves of the feature rows as ranges of k: rows 0 .. 15 = x and k < 15; rows 16 .. 31 = k >= 15"""
    return ((0, min(T, 15)), (15, T))


def both_classes_share(eff, T):
    """eff (B, T): the class a row is really read as (0: zeros).  -> per half of the feature rows, the share of samples that hold a row of
    each class there -- or None for a half of fewer than 2 rows (T = 1; T = 16, whose second half is one row), which cannot hold both.
    (A half of 2 or 3 rows holds both by construction, see classes(); from 4 rows on P(both) of a draw is 1 - 2 * 0.55^n + 0.1^n >= 0.82.)"""
    shares = []
    for lo, hi in HALVES(T):
        if hi - lo < 2:
            shares.append(None)
            continue
        h = eff[:, lo:hi]
        shares.append(float(((h == 1).any(1) & (h == 2).any(1)).mean()))
    return shares


# ---- rows: one device buffer of encoded rows per (d, codec, kind, class) ----------------------------------------------------------------
_ROWS = {}


class RowBuffer:
    def __init__(self, raw, dec, dev):
        self.raw, self.dec, self.dev = raw, dec, dev
        self.base = dev.data_ptr()
        self.row_bytes = raw.shape[1]
        assert self.base % 16 == 0, "a 16-byte aligned base: rows are then aligned as arena and backing rows are"


def row_buffer(orc, d, codec, kind, which):
    """N_ROWS rows of the kind's values (row r as feature r + 1), encoded by the oracle; .dec = the oracle's bit-exact decode of those bytes"""
    import torch
    key = (d, codec, kind, which)
    if key not in _ROWS:
        rs = np.random.RandomState(1000 * d + 10 * codec + which + 100000 * KINDS.index(kind))
        W = np.stack([AD.values(kind, rs, (d,), r + 1) for r in range(N_ROWS)])
        raw = np.ascontiguousarray(orc.encode_table(np.clip(W, -1, 1), codec))
        assert raw.shape == (N_ROWS, row_bytes(codec, d))
        _ROWS[key] = RowBuffer(raw, orc.decode(raw, codec, d), torch.from_numpy(raw).cuda())
    return _ROWS[key]


# ---- one call ----------------------------------------------------------------------------------------------------------------------
def out_row(d, T, itself):
    F = T + 1
    return d + (F * (F + 1) // 2 if itself else F * (F - 1) // 2)


def call(E, B, T, d, x, ptrs, cls, codecs, itself, default_class, want_name):
    """x (B, x_stride) fp32 and ptrs (B, T) int64 numpy, cls (B, T) uint8 or None -> R (B, out_row) numpy.  Asserts that exactly `want_name` of
    the record went up, by one, and that the guard band behind R still holds the sentinel."""
    import torch
    n = B * out_row(d, T, itself)
    Rbuf = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    xd, pd = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.ascontiguousarray(ptrs)).cuda()
    cd = None if cls is None else torch.from_numpy(np.ascontiguousarray(cls)).cuda()
    before = E._lib.mixed_kernels_seen()
    E._lib.check(E._lib.lib().evs_interact_rows_by_address(B, T, d, xd.data_ptr(), x.shape[1], pd.data_ptr(), None if cd is None else cd.data_ptr(),
                                                           codecs[0], codecs[1], itself, default_class, Rbuf.data_ptr(),
                                                           torch.cuda.current_stream().cuda_stream))
    after = E._lib.mixed_kernels_seen()
    got = Rbuf.cpu().numpy()
    assert {k: after[k] - before[k] for k in after if after[k] != before[k]} == {want_name: 1}, (want_name, before, after)
    assert (got[n:] == SENTINEL).all(), "the call wrote behind R"
    return got[:n].view(np.float32).reshape(B, -1)


HITS = set()     # (record name, B) of the random-class cases run in this process
N_CASES = [0]
N_LAUNCHES = [0]


MIN_ELEMENTS = 64   # pair elements under one check (see run_case)


def run_case(E, orc, case, rfq_on=True):
    """One case of cases(): the record, the guard band, and tests/_accuracy.py's check (L = 1, no extra) of the whole of R -- which was filled
    with a NaN sentinel, so an element the call left alone fails the bound -- against fp64 over the oracle's decode of the rows addressed.

    The check's fourth clause is a statistic of a distribution (the median of err / (u M) over the pair elements, at most 4); a call of B = 1
    and T = 1 has ONE pair element, whose honest error is above 4 u M now and then.  A case of fewer than MIN_ELEMENTS pair elements is
    therefore that many launches of its shape over fresh draws, each under the record and guard-band assertions, and ONE check over all
    their samples: the per-element clauses (x bits, exact zeros, the hard bound) hold for every launch, the median is taken over >= 64 elements."""
    d, T, B, itself, codecs = case["d"], case["T"], case["B"], case["itself"], case["codecs"]
    rs = np.random.RandomState((d * 1009 + T * 101 + B * 7 + itself * 3 + PATTERNS.index(case["pattern"]) + 131 * codecs[0] + codecs[1]) % 2 ** 31)
    bufs = {c: row_buffer(orc, d, codecs[c - 1], case["kind"], c) for c in (1, 2)}
    name = kernel_name(T, d, codecs, rfq_on)
    xs = case["x_stride"]
    launches = -(-MIN_ELEMENTS // (B * (out_row(d, T, itself) - d)))
    X, ROWS, RS = [], [], []
    for _ in range(launches):
        for _ in range(50):   # (a small B can miss "both classes in half of the samples" by chance: draw again, a bounded number of times)
            cls, dflt, null = classes(rs, B, T, case["pattern"])
            eff = np.where(null, 0, cls if cls is not None else dflt).astype(np.int64)
            shares = both_classes_share(eff, T) if case["pattern"] == "rand" else []
            if all(s is None or s >= 0.5 for s in shares):
                break
        for half, share in enumerate(shares):
            assert share is None or share >= 0.5, "half %d of the feature rows: both classes in %.2f of the samples" % (half, share)
        idx = rs.randint(0, N_ROWS, (B, T))
        ptrs = np.zeros((B, T), np.int64)
        rows = np.zeros((B, T, d), np.float32)
        for c in (1, 2):
            m = (cls if cls is not None else np.full((B, T), dflt)) == c
            ptrs[m] = bufs[c].base + idx[m] * bufs[c].row_bytes
            rows[eff == c] = bufs[c].dec[idx[eff == c]]
        # class 0 with a LIVE address (a row of either buffer): zeros all the same, by the class alone.  (Class 0 together with address 0 is
        # not drawn: both guards agree there, so it can tell nothing that these two cells do not.)
        if cls is not None:
            for c in (1, 2):
                m = (cls == 0) & (idx % 2 == c - 1)
                ptrs[m] = bufs[c].base + idx[m] * bufs[c].row_bytes
            assert (ptrs[cls == 0] != 0).all()
        ptrs[null] = 0                                            # address 0 with a class of 1 or 2: zeros by the address alone
        assert not (null & (eff != 0)).any() and (ptrs[eff != 0] != 0).all()
        x = np.full((B, xs), np.nan, np.float32)                  # (what lies between two samples' x is not the call's to read)
        x[:, :d] = AD.values(case["kind"], rs, (B, d), 0)
        RS.append(call(E, B, T, d, x, ptrs, cls, codecs, itself, dflt, name))
        X.append(x[:, :d])
        ROWS.append(rows)
    x, rows, R = np.concatenate(X), np.concatenate(ROWS), np.concatenate(RS)
    ref = acc.Reference(x, [AD.sub(rows[:, k]) for k in range(T)], bool(itself))
    what = "mixed %s d=%d T=%d B=%d itself=%d %s %s stride=%d (%d launches)" % (codecs, d, T, B, itself, case["pattern"], case["kind"], xs, launches)
    kernel = ("interact_mixed84_kernel" if name.startswith("r84") else "interact_mixed_rows_kernel") + " " + name
    acc.check(R, ref, what, kernel)
    if case["pattern"] == "rand":
        HITS.add((name, B))
    N_CASES[0] += 1
    N_LAUNCHES[0] += launches
    return R


# ---- the exact decode probe -----------------------------------------------------------------------------------------------------------
PROBE_T = {1: 15, 2: 27}     # NT -> T: 15 rows in the first half; 15 + 12 rows, the most the rows-in-registers kernel takes


def probe_codes(d, codec, NT):
    """One-hot probe: B = G d samples, x[b] = e_c with c = b % d, so R[b, d + pair(i, 0)] = dec(code of element c of row i of sample b) * 1.0
    plus exact zeros -- the element, its window, shift and nibble, and its table entry, pinned one at a time.

    -> codes (B, T, d) int64 such that, per half of the feature rows (rows 1 .. 15; rows 16 .. T) and per element position c, the PROBED codes
    codes[b, i - 1, b % d] run over every code of the codec (256 u8 codes; 16 u4 nibbles, 15 = NaN included).  The other elements of a row hold
    codes that differ from the probed one (a kernel that reads a neighbouring element returns another value) and are never u4's 15, whose NaN
    would reach every pair of the row.  G groups of d samples: B = d alone cannot do it -- at d = 16 the first half has 16 x 15 = 240 rows in
    all, fewer than the 256 codes that one position must see."""
    T, nc = PROBE_T[NT], 256 if codec == 8 else 16
    halves = [(0, min(T, 15))] + ([(15, T)] if T > 15 else [])
    G = max(-(-nc // (hi - lo)) for lo, hi in halves)
    B = G * d
    codes = np.zeros((B, T, d), np.int64)
    b = np.arange(B)
    g, c = b // d, b % d
    k = (np.arange(d)[None, :] - c[:, None]) % d                      # distance of an element from the probed one
    for lo, hi in halves:
        for j in range(hi - lo):
            probed = (g * (hi - lo) + j + 37 * c) % nc                # (g (hi - lo) + j runs over 0 .. G (hi - lo) - 1 >= nc: every code, for every c)
            if codec == 8:
                row = (probed[:, None] + 1 + 5 * k) % 256             # 5 k + 1 != 0 mod 256 for k < 51
            else:
                row = (probed[:, None] + 1 + k % 13) % 16
                row = np.where(row == 15, (probed[:, None] + 14) % 16, row)
            row[b, c] = probed
            codes[:, lo + j] = row
    return codes


def probe_coverage(codes, d, codec):
    """-> per half: bool (d, n_codes): code v was probed at element position c in that half"""
    B, T, _ = codes.shape
    nc = 256 if codec == 8 else 16
    c = np.arange(B) % d
    probed = codes[np.arange(B), :, c]                                # (B, T)
    out = []
    for lo, hi in [(0, min(T, 15))] + ([(15, T)] if T > 15 else []):
        cov = np.zeros((d, nc), bool)
        for kk in range(lo, hi):
            cov[c, probed[:, kk]] = True
        out.append(cov)
    return out


def run_probe(E, orc, d, cls, NT, itself, rfq_on=True):
    """the probe for rows of one class (1: u8, 2: u4) of the pair (8, 4); asserts the record, the guard band, and every probed cell"""
    import torch
    codec = (8, 4)[cls - 1]
    T = PROBE_T[NT]
    codes = probe_codes(d, codec, NT)
    B = codes.shape[0]
    raw = np.ascontiguousarray(AD.raw(codec, codes.reshape(B * T, d)))
    dec = orc.decode(raw, codec, d).reshape(B, T, d)
    dev = torch.from_numpy(raw).cuda()
    assert dev.data_ptr() % 16 == 0
    ptrs = dev.data_ptr() + np.arange(B * T, dtype=np.int64).reshape(B, T) * raw.shape[1]
    x = np.zeros((B, d), np.float32)
    c = np.arange(B) % d
    x[np.arange(B), c] = 1.0
    name = kernel_name(T, d, (8, 4), rfq_on)
    R = call(E, B, T, d, x, ptrs, np.full((B, T), cls, np.uint8), (8, 4), itself, 1, name)
    li, lj = acc.pair_index(T + 1, bool(itself))
    for i in range(1, T + 1):
        col = d + int(np.nonzero((li == i) & (lj == 0))[0][0])
        want, got = dec[np.arange(B), i - 1, c], R[:, col]
        nan = np.isnan(want)
        assert nan.any() == (codec == 4)
        bad = np.nonzero(~np.where(nan, np.isnan(got), (got == want) & ((want == 0) | (got.view(np.uint32) == want.view(np.uint32)))))[0]
        assert not len(bad), "%s class %d: row %d, sample %d (element %d, code %d): got %r, the oracle decodes %r" % (
            name, cls, i, bad[0], c[bad[0]], codes[bad[0], i - 1, c[bad[0]]], got[bad[0]], want[bad[0]])
    assert np.array_equal(R[:, :d].view(np.uint32), x.view(np.uint32))
    N_CASES[0] += 1
    N_LAUNCHES[0] += 1


def mixed_record(E):
    return dict(E._lib.mixed_kernels_seen())

