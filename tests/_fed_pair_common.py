"""What tests/test_gpu_fed_pair.py and tests/test_fed_pair_model.py share, restated from tests/test_gpu_pair_fetch_first.py so that
no test file depends on another: the geometries, the tables and their decodes (computed once per process), the pair constructor
(addressed or fed), the conflict-free (B, T) call, the hand-made victim case and a row source per codec.  Nothing here touches the
GPU at import."""
import numpy as np
import pytest
import torch

import _accuracy as A

SHAPES = {"T3": [200, 1000, 4000], "T5": [200, 700, 1000, 2500, 4000]}
# (tables, d, codecs, capacities): tests/test_gpu_pair_fetch_first.py's CASES -- 8 + 2 x 8 ways, 6 + 2 x 8 ways, both update row widths
CASES = [("T3", 36, (8, 4), (64, 128)), ("T5", 16, (32, 8), (64, 128)), ("T3", 16, (8, 4), (36, 96)), ("T5", 36, (32, 8), (64, 128))]
# (B, new keys at most, "the resident picks walk every resident key"): B cycling 1, 7, 64, 300; the covering calls reach a flush
B_CYCLE = [(1, 8, 0), (1, 1, 0), (7, 7, 0), (7, 7, 0), (64, 8, 0), (300, 8, 0), (7, 7, 0), (64, 8, 0), (300, 8, 0), (1, 1, 0), (64, 8, 0),
           (300, 8, 0), (7, 7, 0), (300, 8, 0), (300, 1, 1), (300, 1, 1), (300, 1, 1), (7, 7, 0), (64, 8, 0), (300, 8, 0), (1, 1, 0)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _new_tables(shape, codec, d, seed=0):
    g = torch.Generator(device="cuda")
    g.manual_seed(100 * len(SHAPES[shape]) + codec + d + seed)
    if codec == 32:
        return [torch.empty(n, d, device="cuda").uniform_(-1, 1, generator=g) for n in SHAPES[shape]]
    if codec == 4:   # (code 15 is not a value of the 4-bit codec -- it decodes to NaN --: nibbles 0 .. 14)
        return [(torch.randint(0, 15, (n, d // 2), device="cuda", generator=g) * 16 + torch.randint(0, 15, (n, d // 2), device="cuda", generator=g)).to(torch.uint8)
                for n in SHAPES[shape]]
    return [torch.randint(0, 256, (n, d * codec // 8), dtype=torch.uint8, device="cuda", generator=g) for n in SHAPES[shape]]


_made, _dec = {}, {}


def _tables(shape, codec, d):
    """tables in a tier's codec, shared by the tests (none writes them)"""
    if (shape, codec, d) not in _made:
        _made[(shape, codec, d)] = _new_tables(shape, codec, d)
    return _made[(shape, codec, d)]


def _decode(E, tables, shape, codec, d):
    """the fp32 rows a tier of `codec` serves from `tables`, per table (numpy): read through the miss path of a fresh cache, once"""
    n_rows = SHAPES[shape]
    dev = [t if t.is_cuda else t.cuda() for t in tables]
    if codec == 32:
        return [t.cpu().numpy().copy() for t in dev]
    c = E.GpuCache("lru", 64, len(n_rows), d, codec, "python")
    c.set_backing(dev)
    rq = np.stack([np.minimum(np.arange(max(n_rows)), r - 1) for r in n_rows], 1).astype(np.int32)
    _h, out = c.lookup_batch(_dev(rq))
    out = out.cpu().numpy()
    return [out[:n_rows[t], t].copy() for t in range(len(n_rows))]


def _dec_shared(E, shape, codec, d):
    if (shape, codec, d) not in _dec:
        _dec[(shape, codec, d)] = _decode(E, _tables(shape, codec, d), shape, codec, d)
    return _dec[(shape, codec, d)]


class _Source:
    """A row source of one tier (GpuCache.set_row_source): the rows of `tables` (that tier's codec) as bytes, through `alter`
    (bytes -> bytes) when given.  Remembers the keys of its last call (`last`) and counts its calls."""

    def __init__(self, tables, alter=None):
        self.raw = [t.cpu().contiguous().view(torch.uint8).reshape(t.shape[0], -1).numpy() for t in tables]
        self.alter = alter
        self.last = np.empty(0, np.uint64)
        self.calls = 0

    def rows(self, keys):
        keys = np.asarray(keys, np.uint64)
        t, r = (keys >> np.uint64(32)).astype(np.int64) - 1, (keys & np.uint64(0xffffffff)).astype(np.int64)
        out = np.empty((len(keys), self.raw[0].shape[1]), np.uint8)
        for k in range(len(self.raw)):
            m = t == k
            out[m] = self.raw[k][r[m]]
        return self.alter(out) if self.alter is not None else out

    def __call__(self, keys):
        self.calls += 1
        self.last = np.array(keys, np.uint64)
        return self.rows(keys)


def _pair(E, shape, d, codecs, caps, order, fed_mask=0, tables=None, alter=(None, None)):
    """order: 0 | 1 for both tiers.  fed_mask != 0: both tiers fed caches over those tables, each with a _Source over its own tables
    (c.source); the other tables addressed in HBM"""
    n_rows = SHAPES[shape]
    T = len(n_rows)
    cs = []
    for k in (0, 1):
        c = E.GpuCache("evlfu", caps[k], T, d, codecs[k], "cpp")
        if order:
            assert c.set_miss_order("fetch-first") is c
        tab = tables[k] if tables else _tables(shape, codecs[k], d)
        c._tables_kept = tab
        if fed_mask:
            c.set_fed_backing([None if (fed_mask >> t) & 1 else tab[t] for t in range(T)], n_rows)
            c.source = _Source(tab, alter[k])
            c.set_row_source(c.source)
        else:
            c.set_backing(tab)
        cs.append(c)
    return tuple(cs)


def _dump(c):
    d = c.batch_dump()
    out = {(int(t), int(r)): int(s) for s, t, r in d}
    assert len(out) == len(d), "a key is resident twice in one tier"
    return out


def _quiet_call(rs, geom, resident, used, B, n_new, cover=False):
    """One (B, T) call whose outcome does not depend on timing: at most min(B, nset, n_new) new keys (never named before), each
    named by ONE position, in different set records and different samples; every other position names a resident key (cover:
    sample b the b-th of its table, round and round, so that every resident key is named).  From empty: B = 1, every position a new
    key."""
    T = geom.T
    lim = [min(a, b) for a, b in zip(*geom.n_rows)]
    by_table = [sorted(r for (t1, r) in resident if t1 == t + 1) for t in range(T)]
    if all(by_table):
        if cover:
            rq = np.stack([np.array(by_table[t])[np.arange(B) % len(by_table[t])] for t in range(T)], 1).astype(np.int32)
        else:
            rq = np.stack([rs.choice(by_table[t], B) for t in range(T)], 1).astype(np.int32)
        where = [(int(b), int(rs.randint(T))) for b in rs.permutation(B)[:min(B, geom.nset, n_new)]]
    else:
        assert B == 1 and T <= geom.nset
        rq = np.zeros((1, T), np.int32)
        where = [(0, t) for t in range(T)]
    recs = set()
    for b, t in where:
        for _try in range(100000):
            r = int(rs.randint(lim[t]))
            if (t + 1, r) not in used and geom.record(t, r) not in recs:
                break
        else:
            raise AssertionError("table %d has run out of new keys" % t)
        recs.add(geom.record(t, r))
        used.add((t + 1, r))
        rq[b, t] = r
    return rq


def _reference(x, rows):
    """rows (B, T, d) fp32 as served -> the fp64 reference of R"""
    return A.Reference(x, [A.pool64(rows[:, t])[:2] for t in range(rows.shape[1])], False)


def _rows_of_set(geom, tier, es, table0, count, skip=()):
    lim = min(geom.n_rows[0][table0], geom.n_rows[1][table0])
    out = [r for r in range(lim) if geom.place(tier, table0, r)[0] == es and (table0 + 1, r) not in skip]
    assert len(out) >= count
    return out[:count]


def _fresh_rows(geom, used_records, table0, count):
    out = []
    for r in range(min(geom.n_rows[0][table0], geom.n_rows[1][table0])):
        if geom.record(table0, r) not in used_records:
            used_records.add(geom.record(table0, r))
            out.append(r)
            if len(out) == count:
                return out
    raise AssertionError("too few records")


def _victim_case(geom):
    """C1 set 0: eight keys of table 2 (index 1), the first with the lowest priority; the judged call hits it from a sample with
    agg_hit 1 and brings a ninth key of the set from a sample with agg_hit 0 -> (the eight rows, the newcomer, the two resident keys
    of the scripted calls, the call)"""
    rows = _rows_of_set(geom, 1, 0, 1, 9)
    used = {0}
    a, b = _fresh_rows(geom, used, 0, 3), _fresh_rows(geom, used, 2, 3)
    rq = np.array([[a[1], rows[0], b[1]], [a[2], rows[8], b[2]]], np.int32)
    return rows[:8], rows[8], (a[0], b[0]), rq


def _refused(E, code, word, call):
    with pytest.raises(E._lib.EvsError) as ei:
        call()
    assert ei.value.code == code and word in str(ei.value), str(ei.value)
    return str(ei.value)
