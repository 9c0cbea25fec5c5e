"""The data kinds of the accuracy tests (tests/test_gpu_accuracy.py, tests/_mixed_matrix.py): fp32 values, and the codes and raw rows
of a reduced-precision feature.  Test infrastructure; imported like _accuracy.py.  No GPU, no torch."""
import numpy as np

import _accuracy as acc

KAGGLE_LN = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306, 10,
             5652, 2173, 4, 7046547, 18, 15, 286181, 105, 142572]   # (bench.KAGGLE_LN)


def values(kind, rs, shape, j):
    """fp32 values of feature j (0 = x) of the given kind, shape (..., d)."""
    d = shape[-1]
    if kind == "unit":
        return rs.uniform(-1, 1, shape).astype(np.float32)
    if kind == "samesign":
        return rs.uniform(0, 1, shape).astype(np.float32)
    if kind == "dlrm":
        if j == 0:
            return (np.maximum(rs.randn(*shape), 0) * 0.1).astype(np.float32)
        a = np.sqrt(1.0 / KAGGLE_LN[(j - 1) % 26])
        return rs.uniform(-a, a, shape).astype(np.float32)
    assert kind == "cancel" and d % 2 == 0
    h = rs.uniform(-1, 1, shape[:-1] + (d // 2,)).astype(np.float32)
    v = np.repeat(h, 2, axis=-1)
    if j % 2:
        v[..., 1::2] *= -1
    return v


def sub(v):
    return acc.pool64(v)[:2]


def decode_all(orc, codec):
    if codec == 16:
        return orc.decode(np.arange(65536, dtype=np.uint16).view(np.uint8), 16, 1).reshape(-1)
    if codec == 8:
        return orc.decode(np.arange(256, dtype=np.uint8), 8, 1).reshape(-1)
    return np.array([orc.decode(np.array([c * 16], np.uint8), 4, 2)[0, 0] for c in range(15)], np.float32)


def codes(orc, codec, kind, rs, shape, j):
    """codes of a reduced-precision feature (int64, one per element; u4 never 15)."""
    dec = decode_all(orc, codec)
    nc = len(dec)
    if kind == "unit":
        return rs.randint(0, nc, shape)
    if kind == "samesign":
        pos = np.nonzero(dec > 0)[0]
        return pos[rs.randint(0, len(pos), shape)]
    if kind == "dlrm":
        a = np.sqrt(1.0 / KAGGLE_LN[(j - 1) % 26])
        return orc.encode(rs.uniform(-a, a, shape), codec)
    # cancel: value pairs (v, v) in even rows, (v, -v) in odd ones, over the codes whose negation is a code
    where = {float(v): c for c, v in enumerate(dec)}
    sym = np.array([c for c, v in enumerate(dec) if np.isfinite(v) and float(-v) in where])
    h = sym[rs.randint(0, len(sym), shape[:-1] + (shape[-1] // 2,))]
    c = np.repeat(h, 2, axis=-1)
    if j % 2:
        c[..., 1::2] = np.vectorize(lambda q: where[float(-dec[q])])(c[..., 1::2])
    return c


def raw(codec, codes):
    if codec == 16:
        return codes.astype(np.uint16).view(np.uint8).reshape(codes.shape[0], -1)
    if codec == 8:
        return codes.astype(np.uint8)
    return (codes[:, 0::2] * 16 + codes[:, 1::2]).astype(np.uint8)
