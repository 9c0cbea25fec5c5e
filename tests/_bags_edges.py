"""Bag lengths that hold every stage edge of the fused multi-hot kernel (csrc/evs_fused_bags.hip) by construction, and the inputs of one
call over them (test infrastructure; imported like _accuracy.py.  No GPU, no torch).

A wave of the kernel walks the flattened lookups of samples w, w + 4, w + 8, w + 12 of a 16-sample chunk as ONE sequence of stages of S
rows: what decides is every sample's total over the tables relative to the multiples of S, where the table boundaries fall inside a stage,
and which samples follow each other in a wave.  tests/test_bags_edges_layout.py asserts each property below from the lengths alone."""
import numpy as np

B = 33                                            # chunk 0 holds the edges, chunk 1 is empty, sample 32 is alone in chunk 2
STAGE_ROWS = {16: 64, 32: 32, 36: 28, 64: 16}     # d -> S (evs_bags_fused_stage_rows)


def edge_lens(S, T):
    """-> (T, B) bag lengths.  Sample by sample (T >= 2 unless said otherwise; with T == 1 every sample keeps its total, in table 0):

    wave 0   0 empty | 4 table 0 = S - 1, table 1 = S + 2: a bag from flattened position S - 1 over three stages | 8 empty
             | 12 one lookup, in table T - 1
    wave 1   1 tables 0..j sum to S (j = min(2, T - 2)), table j + 1 = S: total 2 S, both stage boundaries on table boundaries
             | 5 prefix S, then three empty tables, then 2 (T >= 6: 3, S - 3, three empty, 2; T < 6: S in table 0, 2 in table T - 1)
             | 9 S - 1 spread at random | 13 empty: the wave's last sample
    wave 2   2 S, all in table 0 | 6 S + 1 spread | 10 2 S spread | 14 one lookup, in table 0
    wave 3   3 S spread | 7 2 S + 1, all in table T - 1 | 11 0..3 per table | 15 2 S + 1 spread
    16..31   empty: a whole chunk without a lookup
    32       S + 1 spread: one sample in the third chunk"""
    rs = np.random.RandomState(1000 * S + T)
    lens = np.zeros((T, B), np.int64)

    def only(t, n):
        lens_b = np.zeros(T, np.int64)
        lens_b[t] = n
        return lens_b

    def spread(n):
        return np.bincount(rs.randint(0, T, size=n), minlength=T)

    lens[:, 12] = only(T - 1, 1)
    lens[:, 9] = spread(S - 1)
    lens[:, 2] = only(0, S)
    lens[:, 6] = spread(S + 1)
    lens[:, 10] = spread(2 * S)
    lens[:, 14] = only(0, 1)
    lens[:, 3] = spread(S)
    lens[:, 7] = only(T - 1, 2 * S + 1)
    lens[:, 11] = rs.randint(0, 4, size=T)
    lens[:, 15] = spread(2 * S + 1)
    lens[:, 32] = spread(S + 1)
    if T == 1:
        lens[0, 4], lens[0, 1], lens[0, 5] = 2 * S + 1, 2 * S, S + 2
        return lens
    lens[0, 4], lens[1, 4] = S - 1, S + 2
    j = min(2, T - 2)
    lens[:j + 1, 1] = 1
    lens[0, 1] = S - j
    lens[j + 1, 1] = S
    if T >= 6:
        lens[0, 5], lens[1, 5], lens[5, 5] = 3, S - 3, 2
    else:
        lens[0, 5], lens[T - 1, 5] = S, 2
    return lens


def bags(rs, lens, n_rows):
    """-> lS_o (one start per bag), lS_i (indices inside their tables) of the given lengths"""
    lS_o = [np.concatenate([[0], np.cumsum(l)[:-1]]).astype(np.int64) for l in lens]
    lS_i = [rs.randint(0, n, size=l.sum()).astype(np.int64) for l, n in zip(lens, n_rows)]
    return lS_o, lS_i


def edge_inputs(d, T, seed, mixed=False):
    """-> x, tables, lS_o, lS_i (numpy) over edge_lens(STAGE_ROWS[d], T); mixed: the magnitudes of the rows span six decades"""
    rs = np.random.RandomState(seed)
    lens = edge_lens(STAGE_ROWS[d], T)
    n_rows = rs.randint(3, 201, size=T)
    tables = [rs.uniform(-1, 1, size=(n, d)).astype(np.float32) for n in n_rows]
    if mixed:
        tables = [(t * 10.0 ** rs.uniform(-3, 3, size=t.shape)).astype(np.float32) for t in tables]
    lS_o, lS_i = bags(rs, lens, n_rows)
    x = rs.uniform(-1, 1, size=(lens.shape[1], d)).astype(np.float32)
    return x, tables, lS_o, lS_i
