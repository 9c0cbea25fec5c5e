"""The case table, the data, the float64 reference and the bound of the fused first top-MLP layer (evs_emb_interact_mlp1_stacked,
Python: apply_emb_interact_mlp1): Z1 = act(R W1^T + b1) behind the fused gather + interaction, the MLP form of emb_interact_rf_kernel.
Test infrastructure for tests/test_mlp1_matrix_cases.py (CPU) and tests/test_gpu_mlp1_matrix.py; numpy only, no GPU, no torch.

A case is (d, T, itself, n1, B): F = T + 1 features, K = d + P columns of R, kp = K rounded up to 16 floats per padded row of W1,
nj = kp / 16 sixteen-byte pieces per k-slot of the GEMM's k loop (software-pipelined in groups of 5).  CASES reaches all six kernel
instantiations (mlp1_d<16|32|36>_nt<1|2>), F = 16 and F = 17 for every d, nj mod 5 = 0..4, nj = 2..6 and 28 (kp = 448, the size the
staged rows are built for), padding kp - K of 0 and of 15, n1 = 1 / 15 / 16 / 17 / 65 / 80 / 512, B = 1 / 15 / 16 / 17 / 33 / 293,
and one table of a single row.

The contract of Z1 follows tests/_accuracy.py, with the kernel's own fp32 R as the GEMM operand:

  Z64 = R W1^T + b1 in float64,  Mz = sum_k |R_k| |W_nk| + |b_n|
  * hard bound    |Z1 - act(Z64)| <= (K + 2) u Mz, u = 2^-24: a K-term fp32 dot in any order is within K u sum |a||b| to first order,
                  the + 2 covers the bias add and the second-order terms, ReLU is 1-Lipschitz;
  * Mz == 0       -> Z1 is exactly 0;
  * distribution  the median over a case's outputs of |Z1 - act(Z64)| / (u Mz) <= CAP.

CAP is not acc.CAP (argued for chains of d <= 128 terms) and is not taken from any kernel: it is twice the largest median of
emulate() -- np.float32, one fma chain per k-slot over its kp / 4 columns, the four slots added in turn, then the bias -- over CASES
x KINDS, linear output, R from interact32().  Measured (test_mlp1_matrix_cases.py re-measures and compares):

  kind       largest median   at case
  unit       %(unit)s
  dlrm       %(dlrm)s
  cancel     %(cancel)s
  samesign   %(samesign)s

so CAP = 2 x 0.9354 = 1.8708.  The factor 2 is the allowance for other honest orders.  For information only (no check uses them):
emulate(order="mfma") -- element t of all four slots in instruction t, ONE fma chain of kp terms -- gives 1.49 / 0.84 / 0.34 / 3.21
as its largest medians for the four kinds: same-sign data over the long rows (kp >= 160) is where a single accumulator passes CAP
(the kernel had one, and measured 1.99 - 3.20 there).  emulate(order="kernel") is the order the kernel has now: that order dealt to
four accumulators (tests/test_gpu_mlp1_matrix.py:test_case_against_float64 prints whether Z1 has its bits)."""
import numpy as np

import _accuracy as acc
from _accuracy_data import KAGGLE_LN, values

U = acc.U
KINDS = ("unit", "dlrm", "cancel", "samesign")
NAMES = ["mlp1_d%d_nt%d" % (d, nt) for d in (16, 32, 36) for nt in (1, 2)]   # evs_mlp1_kernels_seen's lines, in its order

#        d   T  itself  n1   B         K   nj
CASES = [
    (16, 1, False, 1, 1),        # 17    2   padding 15
    (36, 4, False, 15, 15),      # 46    3   (table 1 has a single row)
    (36, 7, False, 16, 16),      # 64    4   padding 0
    (32, 8, False, 17, 17),      # 68    5
    (32, 10, False, 65, 33),     # 87    6
    (32, 11, False, 80, 33),     # 98    7
    (16, 14, False, 17, 15),     # 121   8
    (16, 15, False, 65, 17),     # 136   9   F = 16
    (16, 16, False, 80, 33),     # 152   10  F = 17
    (32, 15, False, 15, 16),     # 152   10  F = 16
    (32, 16, False, 16, 293),    # 168   11  F = 17
    (36, 15, True, 1, 33),       # 172   11  F = 16, diagonal kept
    (36, 16, False, 17, 1),      # 172   11  F = 17
    (36, 26, False, 512, 293),   # 387   25  the Kaggle model's own first top layer
    (36, 27, True, 80, 47),      # 442   28  kp = 448
]
SINGLE_ROW_CASE, SINGLE_ROW_TABLE = (36, 4, False, 15, 15), 1

# the largest median of emulate() per kind over CASES (linear output), and the case it was measured at
MEDIANS = {
    "unit": (0.2323, (36, 15, True, 1, 33)),
    "dlrm": (0.5888, (16, 1, False, 1, 1)),
    "cancel": (0.1835, (36, 7, False, 16, 16)),
    "samesign": (0.9354, (36, 26, False, 512, 293)),
}
CAP = 2.0 * max(m for m, _ in MEDIANS.values())   # 1.8708
__doc__ = __doc__ % {k: "%-16.3f %s" % v for k, v in MEDIANS.items()}

STATS = {}   # record name -> [worst err / bound, largest median, checks]


def shape(case):
    """-> F, P, K, kp, nj, record name"""
    d, T, itself, n1, B = case
    F = T + 1
    P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    K = d + P
    kp = (K + 15) // 16 * 16
    return F, P, K, kp, kp // 16, "mlp1_d%d_nt%d" % (d, 2 if F > 16 else 1)


def case_id(case):
    return "d%d-T%d-%s-n%d-B%d" % (case[0], case[1], "itself" if case[2] else "strict", case[3], case[4])


def table_rows(case):
    ns = [min(KAGGLE_LN[k % 26], 498) | 1 for k in range(case[1])]
    if case == SINGLE_ROW_CASE:
        ns[SINGLE_ROW_TABLE] = 1
    return ns


def weights(kind, rs, n1, K):
    """W1 (n1, K), b1 (n1,) fp32 of the kind: unit U(-1, 1); dlrm as create_mlp draws them (dlrm_s_pytorch.py:205-245: N(0, 2 / (K + n1)),
    N(0, 1 / n1)), no weight closer to zero than 2^-6 standard deviations (the scale test keeps every product normal); cancel: values in
    equal pairs, odd rows with the second of each pair negated, no bias on even rows, and the last row (n1 > 1) all zero with no bias
    (Mz == 0); samesign: all positive."""
    if kind == "unit":
        return rs.uniform(-1, 1, (n1, K)).astype(np.float32), rs.uniform(-1, 1, n1).astype(np.float32)
    if kind == "samesign":
        return rs.uniform(0, 1, (n1, K)).astype(np.float32), rs.uniform(0, 1, n1).astype(np.float32)
    if kind == "dlrm":
        sd = np.sqrt(2.0 / (K + n1))
        W = rs.normal(0.0, sd, (n1, K))
        W = np.where(np.abs(W) < sd / 64, np.where(W < 0, -sd / 64, sd / 64), W)
        return W.astype(np.float32), rs.normal(0.0, np.sqrt(1.0 / n1), n1).astype(np.float32)
    assert kind == "cancel"
    W = values("cancel", rs, (n1, K + K % 2), 0)[:, :K].copy()
    W[1::2, 1::2] *= -1
    b = rs.uniform(-1, 1, n1).astype(np.float32)
    b[0::2] = 0
    if n1 > 1:
        W[n1 - 1] = 0
        b[n1 - 1] = 0
    return W, b


def inputs(case, kind, seed=0):
    """-> x (B, d), tables [(n_k, d)], idx (T, B) int64, W1 (n1, K), b1 (n1,): fp32 of the kind, the same for the same arguments"""
    d, T, itself, n1, B = case
    K = shape(case)[2]
    rs = np.random.RandomState([seed, d, T, int(itself), n1, B, KINDS.index(kind)])
    ns = table_rows(case)
    x = values(kind, rs, (B, d), 0)
    tables = [values(kind, rs, (n, d), k + 1) for k, n in enumerate(ns)]
    idx = np.stack([rs.randint(0, n, B) for n in ns]).astype(np.int64)
    W, b = weights(kind, rs, n1, K)
    return x, tables, idx, W, b


def interact32(x, tables, idx, itself):
    """R (B, K) fp32: the interaction in float64, rounded once (the CPU tests' stand-in for the kernel's R)."""
    V = np.stack([x] + [t[idx[k]] for k, t in enumerate(tables)], 1).astype(np.float64)
    li, lj = acc.pair_index(V.shape[1], itself)
    Z = np.matmul(V, V.transpose(0, 2, 1))[:, li, lj]
    return np.concatenate([x, Z.astype(np.float32)], 1)


def reference(R, W, b):
    """-> Z64 (n, n1), Mz (n, n1) from fp32 R (n, K), W (n1, K), b (n1,)"""
    R64, W64, b64 = np.asarray(R, np.float32).astype(np.float64), np.asarray(W, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return R64 @ W64.T + b64, np.abs(R64) @ np.abs(W64).T + np.abs(b64)


def evaluate(Z1, R, W, b, relu, cap=None):
    """Z1 (n, n1) fp32 against the float64 layer over fp32 R.  -> dict of the checks and the statistics."""
    Z1 = np.asarray(Z1, np.float32)
    Z64, Mz = reference(R, W, b)
    K = np.asarray(W).shape[1]
    assert Z1.shape == Z64.shape, (Z1.shape, Z64.shape)
    want = np.maximum(Z64, 0) if relu else Z64
    err = np.abs(Z1.astype(np.float64) - want)
    err[~np.isfinite(Z1)] = np.inf
    bnd = (K + 2) * U * Mz
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), np.where(err > 0, np.inf, 0.0))
        stat = err[Mz > 0] / (U * Mz[Mz > 0])
    out = {"zero_ok": bool((Z1[Mz == 0] == 0).all()),
           "hard_ok": bool((err <= bnd).all()),
           "median": float(np.median(stat)) if stat.size else 0.0,
           "worst": float(ratio.max()) if ratio.size else 0.0}
    out["cap_ok"] = out["median"] <= (CAP if cap is None else cap)
    out["ok"] = out["zero_ok"] and out["hard_ok"] and out["cap_ok"]
    if ratio.size:
        s, n = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        out["at"] = (int(s), int(n), float(err[s, n]), float(bnd[s, n]))
    return out


def check(Z1, R, W, b, relu, case, name):
    """evaluate() and assert every check; the message names the case and the worst (sample, output).  -> the statistics"""
    e = evaluate(Z1, R, W, b, relu)
    s, n, err, bnd = e.get("at", (0, 0, 0.0, 0.0))
    where = "%s [%s]: worst at sample %d output %d: |Z1 - Z64| = %.3g, bound %.3g, ratio %.3g; median %.3g" % (
        case, name, s, n, err, bnd, e["worst"], e["median"])
    assert e["zero_ok"], "an output with Mz == 0 is not exactly 0: " + where
    assert e["hard_ok"], "hard bound (K + 2) u Mz exceeded: " + where
    assert e["cap_ok"], "median err / (u Mz) above %g: %s" % (CAP, where)
    st = STATS.setdefault(name, [0.0, 0.0, 0])
    st[0], st[1], st[2] = max(st[0], e["worst"]), max(st[1], e["median"]), st[2] + 1
    return e


def round_mantissa(a, bits):
    """round-to-nearest-even to `bits` explicit mantissa bits (tf32: 10, bf16: 7)"""
    u = np.asarray(a, np.float32).view(np.uint32).astype(np.uint64)
    sh = 23 - bits
    u = (u + ((1 << (sh - 1)) - 1) + ((u >> sh) & 1)) & ~np.uint64((1 << sh) - 1)
    return u.astype(np.uint32).view(np.float32)


def _fma(s, a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return (s.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def emulate(R, W, b, relu, order="slots", bits=None, drop_last_piece=False, bias_until=None, a_pad=0.0, w_pad=0.0, nan_to_zero=False):
    """The layer in np.float32 over the padded operands (kp columns, k-slot q owning columns [q kp/4, (q+1) kp/4)).
    order "slots": one fma chain per k-slot, the four sums added in turn, then the bias (what CAP is measured on); "mfma": element t
    of the four slots in turn, ONE chain (the matrix unit's order under a single accumulator); "kernel": the same order dealt to four
    accumulators, element t to accumulator t mod 4, added as (0 + 1) + (2 + 3) -- what the kernel does.  The faults a kernel could have: bits = operands rounded to that
    many mantissa bits; drop_last_piece = the last 16-byte piece of every k-slot never accumulated; bias_until = outputs n >= it get
    no bias; a_pad / w_pad = what the padding columns [K, kp) of the two operands hold (0: as they should); nan_to_zero = the ReLU
    written as z > 0 ? z : 0."""
    R, W, b = np.asarray(R, np.float32), np.asarray(W, np.float32), np.asarray(b, np.float32)
    n, K = R.shape
    n1 = W.shape[0]
    kp = (K + 15) // 16 * 16
    kq = kp // 4
    A = np.full((n, kp), a_pad, np.float32)
    Bw = np.full((n1, kp), w_pad, np.float32)
    A[:, :K], Bw[:, :K] = R, W
    if bits is not None:
        A, Bw = round_mantissa(A, bits), round_mantissa(Bw, bits)
    steps = kq - 4 if drop_last_piece else kq
    if order == "slots":
        parts = []
        for q in range(4):
            s = np.zeros((n, n1), np.float32)
            for t in range(steps):
                s = _fma(s, A[:, q * kq + t, None], Bw[None, :, q * kq + t])
            parts.append(s)
        with np.errstate(invalid="ignore", over="ignore"):
            z = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    elif order == "kernel":
        parts = [np.zeros((n, n1), np.float32) for _ in range(4)]
        for t in range(steps):
            for q in range(4):
                parts[t % 4] = _fma(parts[t % 4], A[:, q * kq + t, None], Bw[None, :, q * kq + t])
        with np.errstate(invalid="ignore", over="ignore"):
            z = (parts[0] + parts[1]) + (parts[2] + parts[3])
    else:
        z = np.zeros((n, n1), np.float32)
        for t in range(steps):
            for q in range(4):
                z = _fma(z, A[:, q * kq + t, None], Bw[None, :, q * kq + t])
    bias = b.copy()
    if bias_until is not None:
        bias[bias_until:] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        z = (z + bias[None, :]).astype(np.float32)
        if relu and nan_to_zero:
            return np.where(z > 0, z, np.float32(0))     # z > 0 ? z : 0 -- a NaN compares false and leaves as 0
        return np.where(z <= 0, np.float32(0), z) if relu else z


def hidden_nans(Z1, R, W, b, relu):
    """Outputs where float64 nn.Linear (+ ReLU: torch.relu(nan) is nan, np.maximum keeps it too) over fp32 R is NaN and Z1 is not.
    -> (their (sample, output) indices, how many float64 NaNs there are)"""
    Z64 = reference(R, W, b)[0]
    with np.errstate(invalid="ignore"):
        want = np.maximum(Z64, 0) if relu else Z64
    isnan = np.isnan(want)
    return np.argwhere(isnan & ~np.isnan(np.asarray(Z1, np.float32))), int(isnan.sum())
