"""apply_emb_long (csrc/evs_gather_longq.hip: long-bag pooling of u16 / u8 / u4 tables) against the oracle's index-order fp32 loop,
as BITS, at the bag lengths around the kernel's chunk K, under its own dispatch record; bad input stays local and is flagged."""
import numpy as np
import pytest
import torch

from _pooling_matrix import SENTINEL, index_flag, make_bags, make_tables, reference
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import evstore_dlrm_amd as E
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    E._lib.lib()
    return E


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cycle(K, T, B):
    """bag lengths around the chunk, a different starting point per table: one wave holds bags of different lengths"""
    c = (0, 1, K - 1, K, K + 1, 2 * K + 1, 3)
    return np.array([[c[(b + 2 * k) % 7] for b in range(B)] for k in range(T)])


def _bits(E, d, codec, tabs, idx, off, **kw):
    """apply_emb_long over numpy inputs -> (T, B, d) uint32, the launches of both records"""
    ev = E.EVTables([_dev(t) for t in tabs], d, codec)
    seen = E._lib.long_q_kernels_seen(), E._lib.gather_kernels_seen()
    ly = E.apply_emb_long([_dev(o) for o in off], [_dev(i) for i in idx], ev, **kw)
    torch.cuda.synchronize()
    now = E._lib.long_q_kernels_seen()
    assert E._lib.gather_kernels_seen() == seen[1]
    return torch.stack(list(ly)).cpu().numpy().view(np.uint32), {k: now[k] - v for k, v in seen[0].items() if now[k] != v}


def _want(B, d, codec, tabs, idx, off):
    return np.stack(reference(orc, B, d, codec, tabs, idx, off)).view(np.uint32)


@pytest.mark.parametrize("codec,d", [(c, d) for c in (16, 8, 4) for d in (16, 32, 36, 64, 128)])
def test_bits_at_the_chunk_edges(E, codec, d):
    K, G = E._lib.lib().evs_long_q_chunk(codec, d), 64 // (d // 4)
    B, rs = 2 * G + 1, np.random.RandomState(1000 * codec + d)
    tabs = make_tables(orc, rs, 3, d, codec)
    lens = _cycle(K, 3, B)
    lens[1] = 0
    idx, off = make_bags(rs, tabs, lens)
    got, went_up = _bits(E, d, codec, tabs, idx, off)
    assert went_up == {"longq_c%d_lpr%d" % (codec, d // 4): 1} and index_flag(E) == 0
    assert np.array_equal(got, _want(B, d, codec, tabs, idx, off))


@pytest.mark.parametrize("d", [36, 64])
def test_one_bag_and_the_tile_layout(E, d):
    K, G, rs = E._lib.lib().evs_long_q_chunk(8, d), 64 // (d // 4), np.random.RandomState(d)
    tabs = make_tables(orc, rs, 3, d, 8)
    idx, off = make_bags(rs, tabs, np.full((3, 1), 2 * K + 1))
    got, _ = _bits(E, d, 8, tabs, idx, off)
    assert np.array_equal(got, _want(1, d, 8, tabs, idx, off))
    B = G + 1
    lens = _cycle(K, 3, B)
    lens[:, 0] = 2 * K + 1
    idx, off = make_bags(rs, tabs, lens)
    tile = torch.full((B, 4, d), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    _bits(E, d, 8, tabs, idx, off, out=tile)
    got = tile.view(torch.int32).cpu().numpy().view(np.uint32)
    assert (got[:, 0] == SENTINEL).all() and index_flag(E) == 0
    assert np.array_equal(got[:, 1:].transpose(1, 0, 2), _want(B, d, 8, tabs, idx, off))


def test_more_tables_than_one_launch(E):
    rs = np.random.RandomState(33)
    tabs = make_tables(orc, rs, 33, 16, 4)
    idx, off = make_bags(rs, tabs, rs.randint(0, 4, size=(33, 5)))
    got, went_up = _bits(E, 16, 4, tabs, idx, off)
    assert went_up == {"longq_c4_lpr4": 2} and index_flag(E) == 0
    assert np.array_equal(got, _want(5, 16, 4, tabs, idx, off))


def _batch(E, d=64, codec=8):
    K, G, rs = E._lib.lib().evs_long_q_chunk(codec, d), 64 // (d // 4), np.random.RandomState(7)
    tabs = make_tables(orc, rs, 3, d, codec)
    lens = _cycle(K, 3, G + 2)
    lens[2, 0], lens[2, G] = K + 1, 3
    return (d, codec, tabs) + make_bags(rs, tabs, lens), K, G + 2


def test_indices_outside_the_table_are_dropped_and_flagged(E):
    (d, codec, tabs, idx, off), K, B = _batch(E)
    idx[2][K // 2], idx[2][K // 2 + 2] = tabs[2].shape[0], -1
    got, _ = _bits(E, d, codec, tabs, idx, off)
    assert index_flag(E) != 0 and index_flag(E) == 0
    assert np.array_equal(got, _want(B, d, codec, tabs, idx, off))
    with pytest.raises(E.EvsError):
        _bits(E, d, codec, tabs, idx, off, check_indices=True)


def test_an_offset_behind_the_indices_empties_its_two_bags(E):
    (d, codec, tabs, idx, off), K, B = _batch(E)
    want = _want(B, d, codec, tabs, idx, off)
    assert want[2, B - 2].any() and want[2, B - 1].any()
    want[2, B - 2:] = 0
    off[2][B - 1] = idx[2].size + 1
    got, _ = _bits(E, d, codec, tabs, idx, off)
    assert index_flag(E) != 0 and np.array_equal(got, want)


def test_fp32_tables_are_refused(E):
    rs = np.random.RandomState(3)
    tabs = make_tables(orc, rs, 3, 36, 32)
    idx, off = make_bags(rs, tabs, np.full((3, 4), 2))
    before = E._lib.long_q_kernels_seen()
    with pytest.raises(E.EvsError) as e:
        _bits(E, 36, 32, tabs, idx, off)
    assert e.value.code == E._lib.EVS_EINVAL and E._lib.long_q_kernels_seen() == before
