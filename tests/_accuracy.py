"""The accuracy contract of the interaction output R (test infrastructure; imported like _dist_helpers.py).

R = [x | Z] with Z the packed lower triangle of T T^T, T = (x, f_1, ..., f_T) per sample.  The reference is float64 on the
host from the fp32 inputs: pooled features recomputed as sum_l w_l row_l, codec rows decoded with the oracle's bit-exact
decoders.  Alongside it, the magnitude matrix M_ij = sum_c P_ic P_jc with P = sum_l |w_l row_l| for a pooled feature and
P = |x| for x.  The checks, per element of every sample checked:

  * hard bound   |R - R64| <= (d + 2L + 2) u M_ij + extra_ij,   u = 2^-24, L = the longest bag.
                 A pooled feature summed in fp32 in any order is within L u P of its exact value, a dot product of d
                 terms in any order within d u sum |a||b| of its exact value (first order); the two compose to
                 (d + 2L) u M, and the + 2 covers the second-order terms.  The k-ordered fma chain of the f32 MFMA,
                 split sums over k-slots and shuffles included, is one evaluation order among those.
  * M_ij == 0    (empty bags, absent rows, zero rows) -> R_ij is exactly 0;
  * x columns    bit for bit equal to x;
  * distribution median over the pair elements of |R - R64| / (u M + extra) <= 4 (an honest fp32 chain gives 0.2 - 1.8;
                 a bf16 x 3 split 9.4, tf32 or bf16 operands thousands: tests/test_accuracy_checker.py).

extra is zero except on the u8 integer-pipe path (csrc/evs_fused_rfq.hip, EVS_RFQ_I8: u8 rows, d = 36, F > 16, rows in
registers), which computes a different arithmetic, derived in i8_extra() below.
"""
import numpy as np

U = 2.0 ** -24
CAP = 4.0
STATS = {}   # kernel -> [worst err / bound, largest median, checks] over the checks made (the headroom of each path)


def pair_index(F, itself):
    """(i, j) of the packed lower triangle in R's column order (j < i, j <= i with itself)."""
    off = 1 if itself else 0
    li = [i for i in range(F) for j in range(i + off)]
    lj = [j for i in range(F) for j in range(i + off)]
    return np.array(li, np.int64), np.array(lj, np.int64)


def dec_u8_values():
    """dec_u8(code) for all 256 codes (the oracle's bit-exact decoder), float64."""
    from oracle import oracle as orc
    return orc.decode(np.arange(256, dtype=np.uint8), 8, 1).reshape(-1).astype(np.float64)


def u8_delta():
    """delta(code) = dec_u8(code) - (code - 127) / 127: what separates the reference decoder from the affine one
    (|delta| <= 5.9e-8)."""
    return dec_u8_values() - (np.arange(256, dtype=np.float64) - 127.0) / 127.0


def pool64(rows, weights=None, offsets=None, n_bags=None):
    """Pooled features in float64 from fp32 rows.  rows (nnz, d) fp32 (decoded), weights (nnz,) or None, offsets = bag
    starts (n_bags,) (None: one row per bag).  -> (value (n, d), magnitude P (n, d), longest bag)."""
    r = np.asarray(rows, np.float64)
    if weights is not None:
        r = r * np.asarray(weights, np.float32).astype(np.float64)[:, None]
    if offsets is None:
        return r, np.abs(r), 1
    off = np.asarray(offsets, np.int64)
    nb = len(off) if n_bags is None else n_bags
    ends = np.append(off[1:], len(r))[:nb]
    starts = off[:nb]
    seg = np.repeat(np.arange(nb), ends - starts)
    val = np.zeros((nb, r.shape[1]))
    mag = np.zeros((nb, r.shape[1]))
    if len(seg):
        take = np.concatenate([np.arange(s, e) for s, e in zip(starts, ends)])
        np.add.at(val, seg, r[take])
        np.add.at(mag, seg, np.abs(r[take]))
    L = int((ends - starts).max()) if nb else 0
    return val, mag, L


class Reference:
    """R64, M and extra over the sampled rows of one call.

    x (n, d) fp32; feats: list of T (value, magnitude) float64 (n, d) pairs (pool64's first two results); L the longest
    bag; delta: None, or (n, T, d) float64 per-element delta of the feature rows for the u8 integer-pipe path."""

    def __init__(self, x, feats, itself, L=1, delta=None, i8_codes=None):
        self.x = np.ascontiguousarray(x, np.float32)
        n, d = self.x.shape
        V = np.stack([self.x.astype(np.float64)] + [v for v, _ in feats], 1)      # (n, F, d)
        A = np.stack([np.abs(self.x.astype(np.float64))] + [a for _, a in feats], 1)
        self.F = V.shape[1]
        self.d, self.L, self.itself = d, int(L), bool(itself)
        self.li, self.lj = pair_index(self.F, itself)
        self.R64 = np.matmul(V, V.transpose(0, 2, 1))[:, self.li, self.lj]
        self.M = np.matmul(A, A.transpose(0, 2, 1))[:, self.li, self.lj]
        self.K = d + 2 * self.L + 2
        self.extra = np.zeros_like(self.M)
        if delta is not None:
            self.extra = i8_extra(V, delta, i8_codes, self.li, self.lj, self.K)

    def bound(self):
        return self.K * U * self.M + self.extra


def i8_extra(V, delta, codes, li, lj, K):
    """The u8 integer-pipe path's own term (csrc/evs_fused_rfq.hip, I8).

    Row x row: it computes the EXACT value of the affine decoder, a_ic a_jc summed over c with a = (code - 127) / 127, in
    int32, then two roundings (N -> fp32 exact, times fl(1/127^2)): 2 u |sum a_i a_j| <= 2 u M (to first order).  With
    T = dec = a + delta, sum a_i a_j - sum T_i T_j = -sum (delta_i T_j + T_i delta_j - delta_i delta_j), so
        extra_ij = sum_c (|delta_ic| |T_jc| + |T_ic| |delta_jc| + |delta_ic| |delta_jc|).
    x x row: sum_c x_c a_jc, evaluated in fp32 as sum_c x'_c + sum_c x'_c s_jc (x' = x fl(1/127), s = code - 128: the
    "+ 1" of a = (s + 1) / 127 folded into one sum of x'), so besides sum_c |x_c| |delta_jc| the rounding error scales with
    sum_c |x'_c| (1 + |s_jc|), not with sum_c |x'_c| |s_jc + 1| = sum |x_c| |a_jc|.  The two differ by 2 |x'_c| exactly where
    s_jc <= -1 (code <= 127), so the x column carries
        extra_0j = sum_c |x_c| |delta_jc| + K u sum_{c: code_jc <= 127} 2 |x_c| / 127.
    (A row of code 127 decodes to exact zeros -- M = 0 -- but its pair with x is the residue of that folded sum.)
    V (n, F, d) float64 with V[:, 0] = x; delta (n, T, d); codes (n, T, d) the u8 codes of the rows."""
    n, F, d = V.shape
    Dl = np.concatenate([np.zeros((n, 1, d)), np.abs(delta)], 1)
    A = np.abs(V)
    rr = np.matmul(Dl, A.transpose(0, 2, 1))
    ex = rr + rr.transpose(0, 2, 1) + np.matmul(Dl, Dl.transpose(0, 2, 1))
    neg = np.concatenate([np.zeros((n, 1, d)), (np.asarray(codes) <= 127).astype(np.float64)], 1)
    fold = K * U * 2.0 / 127.0 * np.matmul(neg, A[:, :1, :].transpose(0, 2, 1))[:, :, 0]   # (n, F): x against row j
    ex[:, :, 0] += fold
    ex[:, 0, :] += fold
    ex[:, 0, 0] = 0.0   # x . x (itself): 127^2 sum x'^2, a fp32 chain with four more roundings -- inside K
    return ex[:, li, lj]


def evaluate(R, ref):
    """R (n, d + P) fp32 at the sampled rows.  -> dict of the four checks and the statistics."""
    R = np.asarray(R, np.float32)
    d = ref.d
    assert R.shape == (ref.x.shape[0], d + len(ref.li)), (R.shape, ref.x.shape, len(ref.li))
    Z = R[:, d:].astype(np.float64)
    err = np.abs(Z - ref.R64)
    err[~np.isfinite(Z)] = np.inf
    bnd = ref.bound()
    zero = (ref.M == 0) & (ref.extra == 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), np.where(err > 0, np.inf, 0.0))
        den = U * ref.M + ref.extra
        stat = err[den > 0] / den[den > 0]
    out = {"x_ok": bool(np.array_equal(R[:, :d].view(np.uint32), ref.x.view(np.uint32))),
           "zero_ok": bool((Z[zero] == 0).all()),
           "hard_ok": bool((err <= bnd).all()),
           "median": float(np.median(stat)) if stat.size else 0.0,
           "worst": float(ratio.max()) if ratio.size else 0.0}
    out["cap_ok"] = out["median"] <= CAP
    if ratio.size:
        s, p = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        out["at"] = (int(s), int(ref.li[p]), int(ref.lj[p]), float(err[s, p]), float(bnd[s, p]))
    return out


def check(R, ref, case, kernel, rows=None):
    """evaluate() and assert every check; the message names the case, the kernel it is meant for, the worst
    (sample, i, j), its error, its bound and their ratio.  -> the statistics (worst err / bound, median)."""
    e = evaluate(R, ref)
    s, i, j, err, bnd = e.get("at", (0, 0, 0, 0.0, 0.0))
    sample = int(rows[s]) if rows is not None else s
    where = "%s [%s]: worst at sample %d pair (%d, %d): |R - R64| = %.3g, bound %.3g, ratio %.3g; median %.3g" % (
        case, kernel, sample, i, j, err, bnd, e["worst"], e["median"])
    assert e["x_ok"], "x columns are not x bit for bit: " + where
    assert e["zero_ok"], "an output with M == 0 is not exactly 0: " + where
    assert e["hard_ok"], "hard bound (d + 2L + 2) u M + extra exceeded: " + where
    assert e["cap_ok"], "median err / (u M + extra) above %g: %s" % (CAP, where)
    st = STATS.setdefault(kernel, [0.0, 0.0, 0])
    st[0], st[1], st[2] = max(st[0], e["worst"]), max(st[1], e["median"]), st[2] + 1
    return e


def sample_rows(B, n_max=2048, seed=0):
    """At most n_max sample ids of a batch of B: always 0, B - 1 and the rows of the last 16-sample block."""
    if B <= n_max:
        return np.arange(B)
    must = np.unique(np.concatenate([[0, B - 1], np.arange((B - 1) // 16 * 16, B)]))
    rest = np.setdiff1d(np.random.RandomState(seed).choice(B, n_max, replace=False), must)[:n_max - len(must)]
    return np.sort(np.concatenate([must, rest]))


def reference_from_bags(x, tables, lS_o, lS_i, itself=False, weights=None, rows=None):
    """Reference of interact_features(x, apply_emb(lS_o, lS_i, tables, weights)) over the sample ids `rows` (all when
    None): fp32 (decoded) tables, lS_o bag starts per table, lS_i indices per table, weights per table row or None."""
    x = np.asarray(x, np.float32)
    rows = np.arange(x.shape[0]) if rows is None else np.asarray(rows)
    feats, L = [], 1
    for k, t in enumerate(tables):
        ik, o = np.asarray(lS_i[k], np.int64), np.asarray(lS_o[k], np.int64)
        e = np.append(o[1:], len(ik))
        take = [np.arange(o[r], e[r]) for r in rows]
        flat = np.concatenate(take).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum([len(q) for q in take])[:-1]]).astype(np.int64)
        w = None if weights is None else np.asarray(weights[k], np.float32)[ik[flat]]
        v, a, l = pool64(np.asarray(t, np.float32)[ik[flat]], w, starts, len(rows))
        feats.append((v, a))
        L = max(L, l)
    return Reference(x[rows], feats, itself, L)
