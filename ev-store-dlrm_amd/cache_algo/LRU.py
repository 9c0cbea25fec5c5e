"""LRU cache module -- call surface of the reference's cache_algo/LRU.py (init :10, request_to_lru :38)."""
from ._common import _ModuleCache

_m = _ModuleCache("lru")


def init(capacity, device="cuda", engine="auto"):
    _m.init(capacity, "python", device, engine)


def request_to_lru(group_row_ids, use_gpu=False):
    return _m.request(group_row_ids, use_gpu)


def update_rows(keys, values):
    """online row update (no reference counterpart): (table index 0-based, row) -> new fp32 vector into the tables and into
    the cache's copies, whichever engine is bound (_common._ModuleCache.update_rows)"""
    return _m.update_rows(keys, values)
