"""LFU cache module -- call surface of the reference's cache_algo/LFU.py (init :12, request_to_lfu :69)."""
from ._common import _ModuleCache

_m = _ModuleCache("lfu")


def init(capacity, device="cuda", engine="auto"):
    _m.init(capacity, "python", device, engine)


def request_to_lfu(group_row_ids, use_gpu=False):
    return _m.request(group_row_ids, use_gpu)


def update_rows(keys, values):
    """online row update (no reference counterpart): (table index 0-based, row) -> new fp32 vector into the tables and into
    the cache's copies, whichever engine is bound (_common._ModuleCache.update_rows)"""
    return _m.update_rows(keys, values)


def save_state(path):
    """warm start (no reference counterpart: the reference warms the tier by replaying the workload): the cache's exact
    state into an .npz file (_common._ModuleCache.save_state)"""
    _m.save_state(path)


def load_state(path, strict=True):
    """... and back into a cache that has not served a request since its init, under either engine"""
    _m.load_state(path, strict)
