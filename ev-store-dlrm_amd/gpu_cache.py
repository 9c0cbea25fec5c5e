"""GPU-resident cache tier (EvLFU / LRU / LFU) -- Python handle over the C ABI (evs_cache_*).

Reference policies: cache_algo/EvLFU_C1.py, LRU.py, LFU.py; C++/Cython EvLFU variants differ
only in three constants (see include/evstore_hip.h).  All state (hash table, priority lists,
row arena) lives in HBM; this class only owns device buffers and marshals pointers.
"""
import collections
import ctypes as C

import torch

from . import _ext, _lib

POLICY = {"evlfu": 0, "lru": 1, "lfu": 2}
# (flush_rate, perfect_item_cap, flush_extra, perfect_mode)
EVLFU_VARIANTS = {"python": (0.3, 0.95, 1, 0), "cpp": (0.3, 0.95, 0, 2), "cython": (0.4, 1.0, 1, 1)}


def _dev_ptr(t):
    """Device-side address of a device tensor or of a pinned host tensor."""
    if t.is_cuda:
        return t.data_ptr()
    assert t.is_pinned() and t.is_contiguous(), "host tensors must be pinned (torch.Tensor.pin_memory) and contiguous"
    p = _lib.lib().evs_host_device_pointer(t.data_ptr())
    if not p:
        raise _lib.EvsError(_lib.EVS_EINVAL, "pinned tensor is not device-accessible")
    return p


def _check_batch(cache, rows, out=None, hit=None, out_cols=None, pinned_ok=False):
    """Shapes the kernels rely on (a wrong one is an out-of-bounds device access, not an exception): rows (B, n_tables)
    int32 contiguous; out fp32 contiguous with B * out_cols elements (default n_tables * dim); hit / tier uint8 contiguous
    with B * n_tables elements.  Device tensors -- or, for the exact path, pinned host tensors.  -> B"""
    def where(t):
        return t.is_cuda or (pinned_ok and t.is_pinned())
    if not (rows.dtype == torch.int32 and rows.dim() == 2 and rows.shape[1] == cache.n_tables and rows.is_contiguous() and where(rows)):
        raise ValueError("rows must be a contiguous (B, %d) int32 %s tensor, got %s %s" %
                         (cache.n_tables, "device or pinned host" if pinned_ok else "device", tuple(rows.shape), rows.dtype))
    B = int(rows.shape[0])
    if out is not None:
        n = B * (out_cols if out_cols is not None else cache.n_tables * cache.dim)
        if not (out.dtype == torch.float32 and out.is_contiguous() and out.numel() == n and where(out)):
            raise ValueError("out must be a contiguous fp32 tensor of %d elements, got %s %s" % (n, tuple(out.shape), out.dtype))
    if hit is not None:
        if not (hit.dtype == torch.uint8 and hit.is_contiguous() and hit.numel() == B * cache.n_tables and where(hit)):
            raise ValueError("hit / tier must be a contiguous uint8 tensor of %d elements, got %s %s" %
                             (B * cache.n_tables, tuple(hit.shape), hit.dtype))
    return B


class FileTier:
    """File-backed miss tier (evs_filetier_*): ev-table-N.bin files mapped read-only; tables registered with the GPU
    smallest first while they fit pinned_budget_bytes (read zero-copy by the kernels), the rest served through the
    host's reader pool (mmap_file_read.py:32-40 semantics: row r at byte row_bytes * r)."""

    def __init__(self, paths, row_bytes, pinned_budget_bytes):
        self.paths, self.row_bytes, self.n_tables = list(paths), int(row_bytes), len(paths)
        arr = (C.c_char_p * self.n_tables)(*[p.encode() for p in self.paths])
        h = C.c_void_p()
        _lib.check(_lib.lib().evs_filetier_open(C.byref(h), self.n_tables, arr, self.row_bytes, int(pinned_budget_bytes)))
        self._h = h
        rows = (C.c_int64 * self.n_tables)()
        ptrs = (C.c_void_p * self.n_tables)()
        reg = (C.c_int * self.n_tables)()
        pinned = C.c_int64()
        _lib.check(_lib.lib().evs_filetier_info(self._h, rows, ptrs, reg, C.byref(pinned)))
        self.n_rows = [int(v) for v in rows]
        self.registered = [bool(v) for v in reg]
        self.pinned_bytes = int(pinned.value)

    def fetch(self, keys):
        """the reader pool: keys (n,) uint64 numpy array of (table_1based << 32 | row) -> (n, row_bytes) uint8"""
        import numpy as np
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.zeros((len(keys), self.row_bytes), np.uint8)
        _lib.check(_lib.lib().evs_filetier_fetch(self._h, len(keys), keys.ctypes.data, out.ctypes.data, 0))
        return out

    def close(self):
        if self._h:
            _lib.lib().evs_filetier_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_exact_state(state_or_path, who="load_exact_state"):
    """what export_exact_state returned, or the path of a save_exact_state file (read with allow_pickle=False) ->
    (entries (n, 3) int64, state (20,) int64 or None, n_rows int64 array or None); shared by GpuCache and HostCache"""
    import numpy as np
    if isinstance(state_or_path, dict):
        d = state_or_path
    else:
        try:
            with np.load(state_or_path, allow_pickle=False) as z:
                d = {k: z[k] for k in z.files}
        except Exception as e:
            raise _lib.EvsError(_lib.EVS_EIO, "%s: %s is not a readable state file (%s)" % (who, state_or_path, e))
    missing = [k for k in ("entries", "state") + (() if isinstance(state_or_path, dict) else ("n_rows",)) if k not in d]
    if missing:
        raise _lib.EvsError(_lib.EVS_EINVAL, "%s: the state lacks %s" % (who, ", ".join(repr(k) for k in missing)))
    entries = np.ascontiguousarray(d["entries"], np.int64)
    state = None if d["state"] is None else np.ascontiguousarray(d["state"], np.int64)
    if entries.ndim != 2 or entries.shape[1] != 3:
        raise _lib.EvsError(_lib.EVS_EINVAL, "%s: 'entries' must be (n, 3) rows of (score, table_1based, row) -- is this a state of the "
                                             "batched tier (export_state / load_state)?" % who)
    if state is not None and int(state.reshape(-1)[0] if state.size else 0) != 2:
        raise _lib.EvsError(_lib.EVS_EINVAL, "%s: unknown format version (the exact engines take version 2)" % who)
    if state is not None and state.shape != (20,):
        raise _lib.EvsError(_lib.EVS_EINVAL, "%s: 'state' must be (20,)" % who)
    n_rows = d.get("n_rows")
    return entries, state, None if n_rows is None else np.asarray(n_rows).astype(np.int64)


def check_exact_rows(n_rows, mine, strict, who="load_exact_state"):
    """a strict load needs backing tables of the exporter's row counts"""
    if strict and n_rows is not None and n_rows.size and mine is not None and list(n_rows) != [int(v) for v in mine]:
        raise _lib.EvsError(_lib.EVS_EINVAL, "%s: a strict load needs backing tables of the exporter's row counts" % who)


_hwq_warned = False


def _warn_hw_queues():
    """the resident server wants a hardware queue nothing else is folded onto (evstore_dlrm_amd.configure_runtime): say so ONCE
    when the process runs on the runtime's default of four -- the package no longer sets the knob at import"""
    global _hwq_warned
    if _hwq_warned:
        return
    _hwq_warned = True
    import os
    try:
        n = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    except ValueError:
        n = 4
    if n < 8:
        import warnings
        warnings.warn("GpuCache.serve_start: GPU_MAX_HW_QUEUES=%d -- a copy or kernel of the caller's that HIP folds onto the resident "
                      "server's hardware queue waits until the server goes home idle (up to idle_us per request); call "
                      "evstore_dlrm_amd.configure_runtime() before the first GPU call, or export GPU_MAX_HW_QUEUES=8" % n)


class GpuCache:
    def __init__(self, policy, capacity, n_tables=26, dim=36, codec=32, variant="python", device="cuda"):
        self.policy, self.capacity, self.n_tables, self.dim, self.codec = policy, int(capacity), n_tables, dim, codec
        self.device = torch.device(device)
        fr, pc, ex, pm = EVLFU_VARIANTS[variant]
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().evs_cache_create(C.byref(h), POLICY[policy], self.capacity, n_tables, dim, codec,
                                                   fr, pc, ex, pm))
        self._h = h
        self._backing = None

    def __del__(self):
        try:
            if self._h:
                _lib.lib().evs_cache_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _dev_index(self):
        return torch.cuda.current_device() if self.device.index is None else self.device.index

    def set_backing(self, tables):
        """tables: EVTables, or a list of uint8/float tensors (HBM or pinned host memory) in the cache's codec."""
        raws = tables.raw if hasattr(tables, "raw") else list(tables)
        assert len(raws) == self.n_tables
        rb = self.dim * self.codec // 8
        n_rows = [int(t.numel() * t.element_size() // rb) for t in raws]
        self._backing = raws  # keep alive
        self._n_rows = n_rows
        self._backing_ev = tables if hasattr(tables, "raw") else None   # (update_rows: deferred apply_emb results of these tables)
        ptrs = (C.c_void_p * self.n_tables)(*[_dev_ptr(t) for t in raws])   # pinned host tables: their device-side address
        rows = (C.c_int64 * self.n_tables)(*n_rows)
        _lib.check(_lib.lib().evs_cache_set_backing(self._h, ptrs, rows))
        self._fed = False   # (an ordinary cache again: the one-call lookups go straight to the library)

    def set_file_backing(self, tier):
        """tier: FileTier -- the miss tier is a set of .bin files (registered tables zero-copy, the rest staged by the
        host's reader pool; batched lookups only when any table is staged)."""
        assert tier.n_tables == self.n_tables and tier.row_bytes == self.dim * self.codec // 8
        self._backing = tier  # keep alive
        self._backing_ev = None
        _lib.check(_lib.lib().evs_cache_set_file_backing(self._h, tier._h))
        self._fed = False

    def staged_rows(self):
        return int(_lib.lib().evs_cache_staged_rows(self._h))

    def set_batch_policy(self, policy):
        """'sampled' (one update kernel, victim = lowest priority of 8 sampled entries), 'plan' (insert / plan / evict /
        assign, clock-hand window) or 'setassoc' (8-way set-associative: one 64-byte line of key words per set, the
        victim is the lowest priority of the key's own set; single tier, tables in HBM); before the first batched lookup.
        An 'lru' / 'lfu' cache has the set-associative form only (its default): 'plan' and 'sampled' raise EVS_EINVAL."""
        _lib.check(_lib.lib().evs_cache_set_batch_policy(self._h, {"plan": 0, "sampled": 1, "setassoc": 2}[policy]))
        return self

    def request(self, rows, approx_thres=-1, out=None, hit=None):
        """rows: (B, n_tables) int32 tensor.  Requests are replayed strictly in order.
        Returns (hit (B,T) uint8, out (B,T,dim) fp32).
        rows / out / hit may be device tensors or PINNED host tensors (torch pin_memory): pinned buffers are
        read and written by the kernel itself, so the reference's one-request-at-a-time loop costs one launch
        and one synchronise per request instead of two copies around it (synchronise before reading them)."""
        B = _check_batch(self, rows, out, hit, pinned_ok=True)
        if out is None:
            out = torch.empty((B, self.n_tables, self.dim), dtype=torch.float32, device=self.device)
        if hit is None:
            hit = torch.empty((B, self.n_tables), dtype=torch.uint8, device=self.device)
        X = _ext.ext()
        if X is not None:
            X.cache_request(self._h.value, rows, out, hit, int(approx_thres), self._dev_index())
            return hit, out
        _lib.check(_lib.lib().evs_cache_request(self._h, B, _dev_ptr(rows), _dev_ptr(out), _dev_ptr(hit),
                                                int(approx_thres), torch.cuda.current_stream(self.device).cuda_stream))
        return hit, out

    # ---- the exact policy as a resident server (include/evstore_hip.h: evs_cache_serve_*) ----
    def serve_start(self, approx_thres=-1, n_slots=4, idle_us=200):
        """Arm the mailbox server: batch-1 requests then cost two cache-line hand-overs over the bus instead of a launch and a
        synchronise each.  The rows of request i land in self.serve_ring[slot] on the DEVICE."""
        import ctypes as C
        import numpy as np
        _warn_hw_queues()
        self.serve_ring = torch.empty((n_slots, self.n_tables, self.dim), dtype=torch.float32, device=self.device)
        self._srv_views = [self.serve_ring[k] for k in range(n_slots)]   # (a tensor index per request is 2 us of a 15 us request)
        self._srv_rows = np.zeros(self.n_tables, np.int32)
        self._srv_hit = np.zeros(self.n_tables, np.uint8)
        self._srv_slot = C.c_int(0)
        self._srv_call = (_lib.lib().evs_cache_serve_request, self._h, self._srv_rows.ctypes.data, self._srv_hit.ctypes.data, C.byref(self._srv_slot))
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().evs_cache_serve_start(self._h, int(approx_thres), self.serve_ring.data_ptr(), int(n_slots), int(idle_us)))
        return self

    def serve_request(self, row_ids):
        """row_ids: n_tables ints (host).  -> (hit flags: a numpy uint8 view valid until the next request, the (T, dim) fp32
        rows as a DEVICE tensor view of a ring slot).  Same results as request() one at a time.
        The server overwrites a slot when the request n_slots later is POSTED (host order): a caller that only ENQUEUES its
        reads of the view (a clone, a kernel) calls serve_consumed() behind them -- the slot is then handed out again only
        after they have run; otherwise the rows must have been read before n_slots - 1 more requests are posted."""
        self._srv_rows[:] = row_ids
        fn, h, rp, hp, sp = self._srv_call
        rc = fn(h, rp, hp, sp)
        if rc:
            _lib.check(rc)
        return self._srv_hit, self._srv_views[self._srv_slot.value]

    def serve_request_to(self, row_ids, out):
        """the same request with the rows written by the server into `out` (a contiguous (T, dim) fp32 DEVICE tensor of the
        caller's, not in use by pending work) instead of a ring slot; row_ids: n_tables ints on the host, or a (T, ...) int64
        device tensor whose element 0 of each row is the id (the reference's lS_i on the GPU).  -> hit flags (numpy uint8 view)"""
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == self.n_tables * self.dim):
            raise ValueError("out must be a contiguous fp32 device tensor of %d elements" % (self.n_tables * self.dim))
        L = _lib.lib()
        if torch.is_tensor(row_ids) and row_ids.is_cuda:
            if row_ids.dtype != torch.int64 or row_ids.shape[0] != self.n_tables:
                raise ValueError("device ids: a (T, ...) int64 tensor")
            _lib.check(L.evs_cache_serve_request_to(self._h, None, row_ids.data_ptr(), int(row_ids.stride(0)), out.data_ptr(), self._srv_hit.ctypes.data))
        else:
            self._srv_rows[:] = row_ids
            _lib.check(L.evs_cache_serve_request_to(self._h, self._srv_rows.ctypes.data, None, 0, out.data_ptr(), self._srv_hit.ctypes.data))
        return self._srv_hit

    def serve_consumed(self, slot=None, stream=None):
        """the reads of ring slot `slot` (default: the last request's) have been enqueued on `stream` (default: the current one)"""
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        _lib.check(_lib.lib().evs_cache_serve_consumed(self._h, int(self._srv_slot.value if slot is None else slot), st.cuda_stream))

    def set_inline_update(self, on=True):
        """the set-associative tier's policy update inside the probe + interaction launch (the default where it applies; hit
        flags then mean "served from the cache") or, on=False, the two-launch chain with strict snapshot flags
        (include/evstore_hip.h: evs_cache_set_inline_update).  An 'lru' / 'lfu' cache always runs the chain: on=True raises
        EVS_EINVAL, on=False is accepted."""
        _lib.check(_lib.lib().evs_cache_set_inline_update(self._h, 1 if on else 0))
        self._inline_told = True
        return self

    def set_miss_order(self, order):
        """Which runs first on the set-associative batched path: 'consume-first' (the default: probe, consumers, update --
        tables in HBM only) or 'fetch-first' (probe, update, a kernel that re-points the installed misses at the arena, then the
        consumers: every missing row is read once, by the update, so the tables may live in pinned host memory as well as in
        HBM).  Before the first batched call or load; 'fetch-first' against set_inline_update(True) raises EVS_EINVAL
        (include/evstore_hip.h: evs_cache_set_miss_order)."""
        if order not in ("consume-first", "fetch-first"):
            raise ValueError("order must be 'consume-first' or 'fetch-first', got %r" % (order,))
        _lib.check(_lib.lib().evs_cache_set_miss_order(self._h, 1 if order == "fetch-first" else 0))
        self._fetch_first = order == "fetch-first"
        return self

    def fetch_stats(self):
        """Counters of the fetch-first chain, cumulative since creation: 'calls' (batched calls that ran it), 'repointed'
        (missed positions served from the arena row the update installed) and 'in_place' (missed positions served from their
        table: the key's set took 8 new keys in that batch).  On C1 of a fetch-first C1 + C2 pair (both tiers set to
        'fetch-first') they count the pair's calls, (B, T) and bag form alike -- 'in_place' then includes a key routed both ways that C1 took -- and
        'victim_hits' counts the hit positions whose way the call's own update took (served from their table row, the same
        bytes).  That key exists only on a cache that has run as C1 of such a pair: a tier alone has no such position.
        Synchronises."""
        s = (C.c_int64 * 4)()
        _lib.check(_lib.lib().evs_cache_fetch_stats(self._h, s, torch.cuda.current_stream(self.device).cuda_stream))
        d = {"calls": int(s[0]), "repointed": int(s[1]), "in_place": int(s[2])}
        if getattr(self, "_pair_fetch_first", False):
            d["victim_hits"] = int(s[3])
        return d

    # ---- fed backing: the tier over rows the caller supplies (include/evstore_hip.h: evs_cache_fed_begin) ----
    def set_fed_backing(self, tables, n_rows):
        """set_backing where tables[k] may be None: table k is then FED -- the GPU never reads it, and the rows of its missing
        keys come from the caller between lookup_begin and lookup_finish (or from set_row_source's function).  n_rows: the row
        count of every table.  Tensors that are given are read in place (HBM or pinned host memory), as set_backing reads
        them.  A fed cache runs 'fetch-first' (set_miss_order) and serves lookup_begin / lookup_finish[_interact] and their bag
        form, lookup_bags_begin / lookup_bags_finish[_interact], only."""
        tables, n_rows = list(tables), [int(v) for v in n_rows]
        assert len(tables) == self.n_tables and len(n_rows) == self.n_tables
        rb = self.dim * self.codec // 8
        for t, n in zip(tables, n_rows):
            assert t is None or t.numel() * t.element_size() // rb >= n, "a table is shorter than its n_rows"
        self._backing = tables   # keep alive
        self._n_rows = n_rows
        self._backing_ev = None
        ptrs = (C.c_void_p * self.n_tables)(*[None if t is None else _dev_ptr(t) for t in tables])
        rows = (C.c_int64 * self.n_tables)(*n_rows)
        _lib.check(_lib.lib().evs_cache_set_fed_backing(self._h, ptrs, rows))
        self._fed = any(t is None and n > 0 for t, n in zip(tables, n_rows))
        return self

    def set_row_source(self, fn, bags=False):
        """fn(keys) -> rows: keys a uint64 numpy array of table_1based << 32 | row, rows (n, row_bytes) uint8 in the cache's
        codec -- numpy or tensor, host or device (FileTier.fetch is such a function).  With a source set, lookup_batch /
        lookup_interact on a fed cache run lookup_begin -> fn -> a copy into a device block this object owns -> lookup_finish.
        bags=True: lookup_bags / lookup_bags_interact run lookup_bags_begin -> fn -> lookup_bags_finish[_interact] as well
        (the default leaves them the library's refusal, as before the bag form existed).  None takes the source away."""
        self._row_source = fn
        self._row_source_bags = bool(bags) and fn is not None
        return self

    def _fetch_fed(self, keys):
        """the source's rows for `keys` in this object's device block (None for an empty list)"""
        import numpy as np
        n = int(keys.numel())
        if n == 0:
            return None
        return self._into_fed_block(self._row_source(keys.cpu().numpy().view(np.uint64)), n)

    def _into_fed_block(self, got, n, which=0):
        """what the row source answered for n keys, copied into device block `which` of this object (lookup_stream: one per open call)"""
        import numpy as np
        rb = self.dim * self.codec // 8
        got = got if isinstance(got, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(got))
        if got.dtype != torch.uint8:
            got = got.contiguous().view(torch.uint8)
        if got.numel() != n * rb:
            raise _lib.EvsError(_lib.EVS_EINVAL, "the row source returned %d bytes for %d keys of %d-byte rows" % (got.numel(), n, rb))
        name = "_fed_block" if which == 0 else "_fed_block%d" % which
        blk = getattr(self, name, None)
        if blk is None or blk.shape[0] < n:
            blk = torch.empty((max(n, 256), rb), dtype=torch.uint8, device=self.device)
            setattr(self, name, blk)
        blk[:n].copy_(got.reshape(n, rb), non_blocking=False)
        return blk[:n]

    def _via_source(self, rows, hit, finish, begin=None):
        """begin -> the row source -> finish; whatever fails in between leaves no call open -- at depth > 1 that includes calls
        the caller opened by hand with lookup_begin before this one: every open call is dropped, newest first.  begin: the bag
        form's (rows and hit are then unused)"""
        hit, keys = begin() if begin is not None else self.lookup_begin(rows, hit)
        try:
            return hit, finish(self._fetch_fed(keys))
        except BaseException:
            self._abort_open_calls()
            raise

    def _open_calls(self):
        """the open calls, oldest first: (rows, hit, B, listed keys, the key buffer) -- kept alive until the call ends"""
        q = getattr(self, "_fed_call", None)
        if q is None:
            q = self._fed_call = collections.deque()
        return q

    def _abort_open_calls(self):
        """drops every open call, newest first (a call the library had already spent is only forgotten)"""
        q = self._open_calls()
        while q:
            try:
                self.lookup_abort()
            except _lib.EvsError:
                q.clear()

    def set_fed_depth(self, n):
        """How many (B, n_tables) calls may be open at once on a fed cache, 1 (the default) .. 4: lookup_begin is accepted while
        fewer are open, lookup_finish[_interact] end the OLDEST open call, lookup_abort drops the NEWEST (include/evstore_hip.h:
        evs_cache_set_fed_depth).  Not while a call is open.  lookup_stream is the driver that keeps the calls open."""
        _lib.check(_lib.lib().evs_cache_set_fed_depth(self._h, int(n)))
        self._fed_depth = int(n)
        return self

    def fed_open_calls(self):
        return int(_lib.lib().evs_cache_fed_open_calls(self._h))

    def fed_ahead_stats(self):
        """Counters of the calls that overlapped, cumulative: 'ahead_begins' (begins made with another call open), 'hold_bits'
        (ways such a begin held) and 'found_installed' (miss records whose key an earlier call had installed by the finish:
        keys fetched twice).  Synchronises."""
        s = (C.c_int64 * 4)()
        _lib.check(_lib.lib().evs_cache_fed_ahead_stats(self._h, s, torch.cuda.current_stream(self.device).cuda_stream))
        return {"ahead_begins": int(s[0]), "hold_bits": int(s[1]), "found_installed": int(s[2])}

    def lookup_stream(self, batches, x=None, itself=False, depth=None):
        """The pipelined driver of a fed cache with a row source (set_row_source): a generator over `batches` -- items `rows` or
        `(rows, x)` -- that yields (hit, out) per item, in order: lookup_batch's out for an item without x, lookup_interact's for
        one with (the argument x: the dense features of every item that carries none).  Up to `depth` calls (default: the
        depth set_fed_depth gave; another value is set first) are open at a time: each begin hands its keys to a pool of `depth`
        threads that run the source -- host work only --, the main thread copies each answer into that call's own device block
        and finishes the calls oldest first; when no call can begin it waits for the oldest fetch.  Whatever fails -- the source,
        a finish, the consumer closing the generator -- every open call is dropped, newest first, before it propagates (calls
        the caller had opened by hand before the stream included).  At depth 1 this is a loop over lookup_batch / lookup_interact.
        An 'evlfu' cache's flush waits for a begin that finds no call open: in steady state the pipe never drains, so a flush
        request stands until the stream ends -- end the stream now and then (a stream per epoch, say) where the tier fills its
        top priority."""
        import numpy as np
        from concurrent.futures import ThreadPoolExecutor
        if getattr(self, "_row_source", None) is None or not getattr(self, "_fed", False):
            raise _lib.EvsError(_lib.EVS_ESTATE, "lookup_stream: a fed cache with a row source (set_fed_backing, set_row_source)")
        depth = int(getattr(self, "_fed_depth", 1) if depth is None else depth)
        if depth != getattr(self, "_fed_depth", 1):
            self.set_fed_depth(depth)

        def split(item):
            rows, xi = item if isinstance(item, (tuple, list)) else (item, None)
            return rows, (x if xi is None else xi)

        if depth == 1:
            for item in batches:
                rows, xi = split(item)
                finish = (lambda fed: self.lookup_finish(fed)) if xi is None else (lambda fed: self.lookup_finish_interact(fed, xi, itself))
                yield self._via_source(rows, None, finish)
            return
        pool = ThreadPoolExecutor(max_workers=depth)
        fetches = collections.deque()          # per open call, oldest first: (the source's future or None, keys listed, hit, x, block)
        it, more, seq = iter(batches), True, 0
        try:
            while True:
                while more and len(fetches) < depth:
                    item = next(it, None)
                    if item is None:
                        more = False
                        break
                    rows, xi = split(item)
                    hit, keys = self.lookup_begin(rows)
                    n = int(keys.numel())
                    fut = pool.submit(self._row_source, keys.cpu().numpy().view(np.uint64)) if n else None
                    fetches.append((fut, n, hit, xi, seq % depth))
                    seq += 1
                if not fetches:
                    break
                fut, n, hit, xi, which = fetches.popleft()
                fed = self._into_fed_block(fut.result(), n, which) if fut is not None else None
                out = self.lookup_finish(fed) if xi is None else self.lookup_finish_interact(fed, xi, itself)
                yield hit, out
        except BaseException:
            self._abort_open_calls()
            raise
        finally:
            for f in fetches:
                if f[0] is not None:
                    f[0].cancel()
            pool.shutdown(wait=True)

    def lookup_begin(self, rows, hit=None):
        """First half of a lookup on a fed cache: the probe.  -> (hit, keys): hit the (B, n_tables) strict snapshot flags, keys
        an int64 device tensor (a view of a buffer this object owns, valid until the next begin) with every distinct missing
        key of a fed table once, as table_1based << 32 | row, in no particular order.  Synchronises.  `rows` and `hit` must
        stay alive until the finish; everything else on this cache is refused until lookup_finish[_interact] or lookup_abort."""
        B = _check_batch(self, rows, None, hit)
        if hit is None:
            hit = torch.empty((B, self.n_tables), dtype=torch.uint8, device=self.device)
        if getattr(self, "_fed_depth", 1) > 1:
            # every open call keeps a key buffer of its own: the view stays valid until that call ends
            busy = {id(call[4]) for call in self._open_calls()}
            bufs = self.__dict__.setdefault("_fed_key_bufs", [])
            kb = next((b for b in bufs if id(b) not in busy and b.numel() >= B * self.n_tables), None)
            if kb is None:
                kb = torch.empty(B * self.n_tables, dtype=torch.int64, device=self.device)
                bufs[:] = [b for b in bufs if id(b) in busy] + [kb]
        else:
            kb = getattr(self, "_fed_keys", None)
            if kb is None or kb.numel() < B * self.n_tables:
                kb = self._fed_keys = torch.empty(B * self.n_tables, dtype=torch.int64, device=self.device)
        n = C.c_int64()
        _lib.check(_lib.lib().evs_cache_fed_begin(self._h, B, rows.data_ptr(), hit.data_ptr(), kb.data_ptr(), C.byref(n),
                                                  torch.cuda.current_stream(self.device).cuda_stream))
        self._open_calls().append((rows, hit, B, int(n.value), kb))   # keep alive
        return hit, kb[:int(n.value)]

    def _fed_args(self, fed):
        if not self._open_calls():
            raise _lib.EvsError(_lib.EVS_ESTATE, "lookup_finish: no call is open on this cache (lookup_begin)")
        _, _, B, n = self._open_calls()[0][:4]   # (the oldest open call: the one a finish ends)
        rb = self.dim * self.codec // 8
        if fed is None:
            return B, 0, 0
        if not (fed.is_cuda and fed.dim() == 2 and fed.shape[0] >= n and fed.shape[1] * fed.element_size() == rb and
                fed.stride(1) == 1):
            raise ValueError("fed must be a device tensor of at least %d rows of %d bytes with unit inner stride, got %s %s" %
                             (n, rb, tuple(fed.shape), fed.dtype))
        return B, fed.data_ptr(), int(fed.stride(0)) * fed.element_size() if fed.shape[0] > 1 else rb

    def lookup_finish(self, fed, out=None):
        """Second half: fed[i] is the row of keys[i] (device tensor, (n, row_bytes) uint8 or (n, dim) fp32 for codec 32; None
        when the list was empty).  Runs the update, the re-point and the row consumer -> out (B, n_tables, dim) fp32.  `fed`
        must stay unchanged until this call's kernels have run on the stream."""
        B, ptr, stride = self._fed_args(fed)
        if out is None:
            out = torch.empty((B, self.n_tables, self.dim), dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * self.n_tables * self.dim):
            raise ValueError("out must be a contiguous fp32 device tensor of %d elements" % (B * self.n_tables * self.dim))
        _lib.check(_lib.lib().evs_cache_fed_finish(self._h, ptr, stride, out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))
        self._open_calls().popleft()
        return out

    def lookup_finish_interact(self, fed, x, itself=False, out=None):
        """lookup_finish with the fused interaction as the consumer -> out (B, dim + P), as lookup_interact returns it."""
        B, ptr, stride = self._fed_args(fed)
        F = self.n_tables + 1
        P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
        if out is None:
            out = torch.empty((B, self.dim + P), dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * (self.dim + P)):
            raise ValueError("out must be a contiguous fp32 device tensor of %d elements" % (B * (self.dim + P)))
        if not (x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (B, self.dim) and x.stride(1) == 1):
            raise ValueError("x must be a (B, %d) fp32 device tensor with unit inner stride" % self.dim)
        _lib.check(_lib.lib().evs_cache_fed_finish_interact(
            self._h, ptr, stride, x.data_ptr(), int(x.stride(0)) if B > 1 else self.dim, int(bool(itself)), out.data_ptr(),
            torch.cuda.current_stream(self.device).cuda_stream))
        self._open_calls().popleft()
        return out

    def lookup_abort(self):
        """Drops the open call: nothing was inserted, the batch is not counted, the same begin lists the same keys."""
        _lib.check(_lib.lib().evs_cache_fed_abort(self._h))
        self._open_calls().pop()

    def fed_stats(self):
        """Counters of the fed form, cumulative: 'calls' (finished), 'keys' (listed), 'missed' (missed positions of fed
        tables) and 'from_block' (of those, served straight from the fed block: the key's set took 8 new keys in that call).
        Synchronises."""
        s = (C.c_int64 * 4)()
        _lib.check(_lib.lib().evs_cache_fed_stats(self._h, s, torch.cuda.current_stream(self.device).cuda_stream))
        return {"calls": int(s[0]), "keys": int(s[1]), "missed": int(s[2]), "from_block": int(s[3])}

    def set_batch_approx(self, thres):
        """The approximate-embedding mode of lookup_batch / lookup_interact on an 'evlfu' set-associative tier: a sample with at
        least `thres` of its T keys resident has every missed position served the row of its nearest earlier hit (a row of
        +0.0 when there is none), flagged 2, and neither fetched nor inserted.  thres <= 0 (or None) switches it off, the
        default; may be set between calls.  thres > n_tables, or thres > 0 on an 'lru' / 'lfu' cache, raises EVS_EINVAL
        (include/evstore_hip.h: evs_cache_set_batch_approx).  The bag forms ignore it."""
        _lib.check(_lib.lib().evs_cache_set_batch_approx(self._h, 0 if thres is None else int(thres)))
        return self

    def approx_stats(self):
        """Counters of the approximate mode, cumulative since creation: 'calls' (batched calls run with a threshold in force),
        'samples' (samples at or above it that had at least one miss), 'substituted' (positions served an earlier hit's row)
        and 'zero_rows' (positions served the zero row).  Synchronises."""
        s = (C.c_int64 * 4)()
        _lib.check(_lib.lib().evs_cache_approx_stats(self._h, s, torch.cuda.current_stream(self.device).cuda_stream))
        return {"calls": int(s[0]), "samples": int(s[1]), "substituted": int(s[2]), "zero_rows": int(s[3])}

    def serve_stop(self):
        _lib.check(_lib.lib().evs_cache_serve_stop(self._h))

    def lookup_batch(self, rows, out=None, hit=None):
        """Batched lookup, snapshot semantics (see include/evstore_hip.h: evs_cache_lookup_batch).  EvLFU under any batch
        policy; an 'lru' / 'lfu' cache as a single set-associative tier over tables in HBM, by "the batched rule" written
        down at evs_cache_set_batch_policy: flags = residency at arrival, every way hit in the batch stamped with the batch
        number (LFU: counter + 1 once per batch), every distinct missed key inserted into its own set over a free way, else
        the least recently touched / least frequently counted way the running batch has not touched."""
        B = _check_batch(self, rows, out, hit)
        if getattr(self, "_row_source", None) is not None and getattr(self, "_fed", False):
            return self._via_source(rows, hit, lambda fed: self.lookup_finish(fed, out))
        if out is None:
            out = torch.empty((B, self.n_tables, self.dim), dtype=torch.float32, device=self.device)
        if hit is None:
            hit = torch.empty((B, self.n_tables), dtype=torch.uint8, device=self.device)
        _lib.check(_lib.lib().evs_cache_lookup_batch(self._h, B, rows.data_ptr(), out.data_ptr(), hit.data_ptr(),
                                                     torch.cuda.current_stream(self.device).cuda_stream))
        return hit, out

    def lookup_interact(self, rows, x, itself=False, out=None, hit=None):
        """R = interact_features(x, cached rows of the B requests): probe + fused MFMA kernel reading the
        rows through a pointer table (no (B,T,d) intermediate), then the batched policy update.  An 'lru' / 'lfu' cache
        runs probe + touch, the row-id / pointer-table consumer and the insert as three launches (strict snapshot flags);
        fp32 or 16 / 8 / 4-bit tiers."""
        F = self.n_tables + 1
        P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
        B = _check_batch(self, rows, out, hit, out_cols=self.dim + P)
        if getattr(self, "_row_source", None) is not None and getattr(self, "_fed", False):
            return self._via_source(rows, hit, lambda fed: self.lookup_finish_interact(fed, x, itself, out))
        if out is None:
            out = torch.empty((B, self.dim + P), dtype=torch.float32, device=self.device)
        if hit is None:
            hit = torch.empty((B, self.n_tables), dtype=torch.uint8, device=self.device)
        if not (x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (B, self.dim) and x.stride(1) == 1):
            raise ValueError("x must be a (B, %d) fp32 device tensor with unit inner stride" % self.dim)
        X = _ext.ext()
        if X is not None:
            X.cache_lookup_interact(self._h.value, rows, x, bool(itself), out, hit)
            return hit, out
        _lib.check(_lib.lib().evs_cache_lookup_interact(
            self._h, B, rows.data_ptr(), x.data_ptr(), int(x.stride(0)) if B > 1 else self.dim, int(bool(itself)),
            out.data_ptr(), hit.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))
        return hit, out

    # ---- ragged bags through an 'lru' / 'lfu' / 'evlfu' tier (include/evstore_hip.h: evs_cache_lookup_bags) ----
    def set_bag_rule(self, rule):
        """What a request's hit count is over ragged bags, for an 'evlfu' cache: 'served-bags' (agg_hit of a sample = the number
        of its T bags without a missed or out-of-range position; empty bags count) or None (the default: lookup_bags /
        lookup_bags_interact refuse an 'evlfu' cache).  An 'lru' / 'lfu' cache needs no rule: 'served-bags' raises EVS_EINVAL,
        None is accepted (include/evstore_hip.h: evs_cache_set_bag_rule)."""
        if rule not in (None, "served-bags"):
            raise ValueError("rule must be 'served-bags' or None, got %r" % (rule,))
        _lib.check(_lib.lib().evs_cache_set_bag_rule(self._h, 1 if rule else 0))
        self._bag_rule_told = True
        return self

    def set_bag_count(self, when):
        """When an 'evlfu' bag call computes its samples' served-bag counts: 'pooling-walk' (the default: the pooling kernel
        judges every sample as a by-product -- today's chain and refusals, tables in HBM only) or 'count-first' (a launch of its
        own between the probe and everything that needs a count; the pooling then only pools).  The rule and every result are
        the same.  On a 'consume-first' cache 'count-first' is the twin of the default chain; on a 'fetch-first' cache
        (set_miss_order) it is what gives 'evlfu' a bag form at all: probe, count, raise + list, update, re-point, pooling -- every
        missing row is read once, by the update, so the tables may live in pinned host memory as well as in HBM.  The C1 + C2
        pair's bag form (lookup_bags_c1c2 / lookup_bags_interact_c1c2) always counts first; there the setting is a statement: told
        to BOTH tiers of a pair whose tiers are both 'fetch-first', it lets the pair's update run in front of the pooling (the
        fetch-first bag chain, tables in HBM or pinned); a 'consume-first' pair ignores it.  May be set
        between calls.  'count-first' on an 'lru' / 'lfu' cache raises EVS_EINVAL (their bag form needs no count),
        'pooling-walk' is accepted (include/evstore_hip.h: evs_cache_set_bag_count)."""
        if when not in ("count-first", "pooling-walk"):
            raise ValueError("when must be 'count-first' or 'pooling-walk', got %r" % (when,))
        _lib.check(_lib.lib().evs_cache_set_bag_count(self._h, 1 if when == "count-first" else 0))
        return self

    def _bags_call(self, lS_o, lS_i):
        """lS_o / lS_i as apply_emb takes them -- a (T, B) int64 tensor or a list of T 1-D int64 tensors, on the device ->
        (B, the C arrays of the call, the flat flag tensor and its per-table views, what must stay alive)"""
        T = self.n_tables
        for name, t in (("lS_o", lS_o), ("lS_i", lS_i)):
            if torch.is_tensor(t):
                if not (t.dim() == 2 and t.shape[0] == T):
                    raise ValueError("%s must be a (%d, n) tensor or a list of %d tensors, got %s" % (name, T, T, tuple(t.shape)))
            elif len(t) != T:
                raise ValueError("%s must hold %d tensors, got %d" % (name, T, len(t)))
        lo, li = [lS_o[k] for k in range(T)], [lS_i[k] for k in range(T)]
        for t in lo + li:
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int64 and t.dim() == 1 and (t.numel() == 0 or t.stride(0) == 1)):
                raise ValueError("offsets and indices must be 1-D int64 device tensors with unit stride")
        B = int(lo[0].shape[0])
        if any(int(t.shape[0]) != B for t in lo):
            raise ValueError("every table needs %d bag offsets" % B)
        nnz = [int(t.numel()) for t in li]
        flat = torch.empty((sum(nnz),), dtype=torch.uint8, device=self.device)
        hits = list(torch.split(flat, nnz))
        idx_c = (C.c_void_p * T)(*[t.data_ptr() if t.numel() else None for t in li])
        off_c = (C.c_void_p * T)(*[t.data_ptr() for t in lo])
        nnz_c = (C.c_int64 * T)(*nnz)
        return B, idx_c, off_c, nnz_c, flat, hits, (lo, li)

    # ---- ragged bags over fed backing (include/evstore_hip.h: evs_cache_fed_begin_bags) ----
    def lookup_bags_begin(self, lS_o, lS_i):
        """First half of lookup_bags on a fed cache: the probe (an 'evlfu' cache: and the count pass; it needs
        set_bag_rule('served-bags') and set_bag_count('count-first')).  -> (hits, keys): hits as lookup_bags gives them, keys an
        int64 device tensor (a view of a buffer this object owns, valid until the next begin) with every distinct missing key of
        a fed table once, as table_1based << 32 | row, in no particular order.  Synchronises.  Everything else on this cache is
        refused until lookup_bags_finish[_interact] or lookup_abort."""
        B, idx_c, off_c, nnz_c, flat, hits, keep = self._bags_call(lS_o, lS_i)
        n_pos = int(flat.numel())
        kb = getattr(self, "_fed_keys", None)
        if kb is None or kb.numel() < max(n_pos, 1):
            kb = self._fed_keys = torch.empty(max(n_pos, 1), dtype=torch.int64, device=self.device)
        n = C.c_int64()
        _lib.check(_lib.lib().evs_cache_fed_begin_bags(self._h, B, idx_c, off_c, nnz_c, flat.data_ptr(), kb.data_ptr(), C.byref(n),
                                                       torch.cuda.current_stream(self.device).cuda_stream))
        self._open_calls().append(((keep, hits, "bags"), flat, B, int(n.value), kb))   # keep alive
        return hits, kb[:int(n.value)]

    def lookup_bags_finish(self, fed, out=None):
        """Second half: fed[i] is the row of keys[i], as lookup_finish takes it.  Touches / raises the ways the begin hit, runs the
        update, the re-point and the pooling -> ly: T (B, dim) fp32 tensors, views of one (T, B, dim) block -- `out`, when given."""
        B, ptr, stride = self._fed_args(fed)
        T, d = self.n_tables, self.dim
        if out is None:
            out = torch.empty((T, B, d), dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (T, B, d)):
            raise ValueError("out must be a contiguous (%d, %d, %d) fp32 device tensor" % (T, B, d))
        _lib.check(_lib.lib().evs_cache_fed_finish_bags(self._h, ptr, stride, out.data_ptr(), B * d, d,
                                                        torch.cuda.current_stream(self.device).cuda_stream))
        self._open_calls().popleft()
        return list(out.unbind(0))

    def lookup_bags_finish_interact(self, fed, x, itself=False, out=None):
        """lookup_bags_finish with the dense interaction behind the pooling -> R (B, dim + P), as lookup_bags_interact returns it."""
        B, ptr, stride = self._fed_args(fed)
        F = self.n_tables + 1
        P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
        if not (x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (B, self.dim) and x.stride(1) == 1):
            raise ValueError("x must be a (B, %d) fp32 device tensor with unit inner stride" % self.dim)
        if out is None:
            out = torch.empty((B, self.dim + P), dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * (self.dim + P)):
            raise ValueError("out must be a contiguous fp32 device tensor of %d elements" % (B * (self.dim + P)))
        _lib.check(_lib.lib().evs_cache_fed_finish_bags_interact(
            self._h, ptr, stride, x.data_ptr(), int(x.stride(0)) if B > 1 else self.dim, int(bool(itself)), out.data_ptr(),
            torch.cuda.current_stream(self.device).cuda_stream))
        self._open_calls().popleft()
        return out

    def lookup_bags(self, lS_o, lS_i, out=None):
        """Multi-hot lookup on an 'lru' / 'lfu' tier: every position of every index array is one lookup of "the batched rule"
        (flags = residency at arrival, one touch per way and batch, every distinct missed key inserted once), the bags pool the
        served rows bit-equal to apply_emb over the backing tables (include/evstore_hip.h: evs_cache_lookup_bags).
        An 'evlfu' tier (set-associative, after set_bag_rule('served-bags')): strict snapshot flags, every hit way raised to
        the served-bag count of the samples that name it, every distinct missed key inserted once at the largest such count.
        -> (hits: T uint8 tensors, one flag per index, views of one flat array; ly: T (B, dim) fp32 tensors, views of one
        (T, B, dim) block -- `out`, when given).  A fed cache with a row source for bags (set_row_source(fn, bags=True)) runs
        lookup_bags_begin -> the source -> lookup_bags_finish."""
        if getattr(self, "_row_source_bags", False) and getattr(self, "_fed", False):
            return self._via_source(None, None, lambda fed: self.lookup_bags_finish(fed, out), begin=lambda: self.lookup_bags_begin(lS_o, lS_i))
        B, idx_c, off_c, nnz_c, flat, hits, _keep = self._bags_call(lS_o, lS_i)
        T, d = self.n_tables, self.dim
        if out is None:
            out = torch.empty((T, B, d), dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (T, B, d)):
            raise ValueError("out must be a contiguous (%d, %d, %d) fp32 device tensor" % (T, B, d))
        _lib.check(_lib.lib().evs_cache_lookup_bags(self._h, B, idx_c, off_c, nnz_c, out.data_ptr(), B * d, d, flat.data_ptr(),
                                                    torch.cuda.current_stream(self.device).cuda_stream))
        return hits, list(out.unbind(0))

    def lookup_bags_interact(self, lS_o, lS_i, x, itself=False, out=None):
        """R = interact_features(x, the T pooled bags of lookup_bags): probe, pooling into a (T, B, dim) block the cache owns,
        the dense interaction, insert ('evlfu': raise + list, then the insert) -- the rule and the flags of lookup_bags
        (include/evstore_hip.h: evs_cache_lookup_bags_interact).  -> (hits as lookup_bags gives them, R (B, dim + F (F - 1) / 2) with F = T + 1)."""
        if getattr(self, "_row_source_bags", False) and getattr(self, "_fed", False):
            return self._via_source(None, None, lambda fed: self.lookup_bags_finish_interact(fed, x, itself, out),
                                    begin=lambda: self.lookup_bags_begin(lS_o, lS_i))
        B, idx_c, off_c, nnz_c, flat, hits, _keep = self._bags_call(lS_o, lS_i)
        F = self.n_tables + 1
        P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
        if not (x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (B, self.dim) and x.stride(1) == 1):
            raise ValueError("x must be a (B, %d) fp32 device tensor with unit inner stride" % self.dim)
        if out is None:
            out = torch.empty((B, self.dim + P), dtype=torch.float32, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * (self.dim + P)):
            raise ValueError("out must be a contiguous fp32 device tensor of %d elements" % (B * (self.dim + P)))
        _lib.check(_lib.lib().evs_cache_lookup_bags_interact(
            self._h, B, idx_c, off_c, nnz_c, x.data_ptr(), int(x.stride(0)) if B > 1 else self.dim, int(bool(itself)),
            out.data_ptr(), flat.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))
        return hits, out

    def batch_stats(self):
        """Counters of the batched path and the resident-entry histogram per priority.  An 'lru' / 'lfu' cache: n_flush stays
        0, n_perfect_hits counts all-hit requests, hist[0] = size and the rest 0.  After lookup_bags on an 'evlfu' cache
        n_perfect_hits counts the samples with a lookup whose T bags were all served, hist the priorities 0 .. T."""
        s = (C.c_int64 * 8)()
        hist = (C.c_int64 * (self.n_tables + 1))()
        _lib.check(_lib.lib().evs_cache_batch_stats(self._h, s, hist, torch.cuda.current_stream(self.device).cuda_stream))
        keys = ("size", "n_free", "n_tomb", "n_flush", "n_evict", "n_requests", "n_perfect_hits", "n_hits")
        d = dict(zip(keys, [int(v) for v in s]))
        d["hist"] = [int(v) for v in hist]
        return d

    def batch_dump(self):
        """Resident keys of the batched path, unordered: rows of (score, table_1based, row).  score: EvLFU the priority, 'lru'
        the way's age in batches (0 = touched by the latest batch), 'lfu' its counter (1..63, one count per batch)."""
        import numpy as np
        st = torch.cuda.current_stream(self.device).cuda_stream
        n = _lib.lib().evs_cache_batch_dump(self._h, None, 0, st)
        if n < 0:
            _lib.check(int(n))
        out = np.zeros((max(n, 1), 3), np.int64)
        _lib.lib().evs_cache_batch_dump(self._h, out.ctypes.data, n, st)
        return out[:n]

    # ---- warm start (include/evstore_hip.h: evs_cache_batch_export / evs_cache_batch_load) ----
    def export_state(self):
        """What the batched set-associative tier holds, at rest (pending closes folded, a wanted EvLFU flush run) -> a dict of
        numpy arrays: 'entries' (n, 5) int64 rows of (table_1based, row, score, age, slot) sorted by slot, 'state' (16,) int64
        (format version, policy, capacity, n_tables, dim, codec, batch number, five counters, stamp bits S, bag rule,
        inline-update setting, 0) and 'n_rows' (T,) int64, the rows of the backing tables."""
        import numpy as np
        L, st = _lib.lib(), torch.cuda.current_stream(self.device).cuda_stream
        state = np.zeros(16, np.int64)
        with torch.cuda.device(self.device):
            n = L.evs_cache_batch_export(self._h, None, 0, None, st)
            if n < 0:
                _lib.check(int(n))
            entries = np.zeros((max(n, 1), 5), np.int64)
            n2 = L.evs_cache_batch_export(self._h, entries.ctypes.data, n, state.ctypes.data, st)
        if n2 != n:
            raise _lib.EvsError(_lib.EVS_ESTATE, "export_state: the cache changed between the count and the export")
        return {"entries": entries[:n], "state": state, "n_rows": np.asarray(getattr(self, "_n_rows", []), np.int64)}

    def save_state(self, path):
        """export_state() into an .npz file (np.savez; read back by load_state with allow_pickle=False)"""
        import numpy as np
        with open(path, "wb") as f:
            np.savez(f, **self.export_state())

    def load_state(self, state_or_path, strict=True):
        """Warm start: the exported entries into this cache, which must be fresh with its backing set -- one launch copies every
        entry's row from the backing table into the arena and stores its way word; the host decides every placement.
        state_or_path: what export_state returned, or the path of a save_state file.  strict=True: the cache must have the
        exporter's capacity, tables and key universe, and continues exactly as the exporter would have; strict=False: the
        entries are placed anew in this cache's geometry (another capacity: per set the 8 highest scores, youngest first, the
        rest turned away); 'state' may then be None (batch number = the largest age, counters 0).  The exported bag rule and
        inline-update setting are applied through set_bag_rule / set_inline_update unless this cache was told already.
        -> {'placed', 'turned_away', 'batch'}"""
        import numpy as np
        if isinstance(state_or_path, dict):
            d = state_or_path
        else:
            try:
                with np.load(state_or_path, allow_pickle=False) as z:
                    d = {k: z[k] for k in z.files}
            except Exception as e:
                raise _lib.EvsError(_lib.EVS_EIO, "load_state: %s is not a readable state file (%s)" % (state_or_path, e))
        missing = [k for k in ("entries", "state") + (() if isinstance(state_or_path, dict) else ("n_rows",)) if k not in d]
        if missing:
            raise _lib.EvsError(_lib.EVS_EINVAL, "load_state: the state lacks %s" % ", ".join(repr(k) for k in missing))
        entries = np.ascontiguousarray(d["entries"], np.int64)
        state = None if d["state"] is None else np.ascontiguousarray(d["state"], np.int64)
        if entries.ndim != 2 or entries.shape[1] != 5 or (state is not None and state.shape != (16,)):
            raise _lib.EvsError(_lib.EVS_EINVAL, "load_state: 'entries' must be (n, 5) and 'state' (16,)")
        if state is not None and int(state[0]) != 1:
            raise _lib.EvsError(_lib.EVS_EINVAL, "load_state: unknown format version %d" % int(state[0]))
        if strict and d.get("n_rows") is not None and hasattr(self, "_n_rows") and list(np.asarray(d["n_rows"]).astype(np.int64)) != list(self._n_rows):
            raise _lib.EvsError(_lib.EVS_EINVAL, "load_state: a strict load needs backing tables of the exporter's row counts")
        out4 = np.zeros(4, np.int64)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().evs_cache_batch_load(self._h, int(entries.shape[0]), entries.ctypes.data if entries.shape[0] else None,
                                                       None if state is None else state.ctypes.data, 1 if strict else 0, out4.ctypes.data,
                                                       torch.cuda.current_stream(self.device).cuda_stream))
        if state is not None:
            if int(state[13]) == 1 and not getattr(self, "_bag_rule_told", False):
                self.set_bag_rule("served-bags")
            if int(state[14]) >= 0 and not getattr(self, "_inline_told", False) and (self.policy == "evlfu" or int(state[14]) == 0) \
                    and not (getattr(self, "_fetch_first", False) and int(state[14]) == 1):   # (a fetch-first cache has the chain only)
                self.set_inline_update(bool(state[14]))
        return {"placed": int(out4[0]), "turned_away": int(out4[1]), "batch": int(out4[3])}

    # ---- warm start of the exact path (include/evstore_hip.h: evs_cache_exact_export / evs_cache_exact_load) ----
    def export_exact_state(self):
        """What the exact (batch-1) engine holds -> a dict of numpy arrays: 'entries' (n, 3) int64 = dump()'s rows in list
        order, 'state' (20,) int64 (format version 2, policy, capacity, n_tables, dim, codec, min_C1, n_perfect, least_freq,
        five counters, max_perfect, flush_n, perfect_mode, 0, 0, 0) and 'n_rows' (T,) int64, the rows of the backing tables.
        A resident server is sent home first.  HostCache.export_exact_state gives the same arrays for the same requests."""
        import numpy as np
        L, st = _lib.lib(), torch.cuda.current_stream(self.device).cuda_stream
        state = np.zeros(20, np.int64)
        with torch.cuda.device(self.device):
            n = L.evs_cache_exact_export(self._h, None, 0, None, st)
            if n < 0:
                _lib.check(int(n))
            entries = np.zeros((max(n, 1), 3), np.int64)
            n2 = L.evs_cache_exact_export(self._h, entries.ctypes.data, n, state.ctypes.data, st)
        if n2 != n:
            if n2 < 0:
                _lib.check(int(n2))
            raise _lib.EvsError(_lib.EVS_ESTATE, "export_exact_state: the cache changed between the count and the export")
        return {"entries": entries[:n], "state": state, "n_rows": np.asarray(getattr(self, "_n_rows", []), np.int64)}

    def save_exact_state(self, path):
        """export_exact_state() into an .npz file (read back by load_exact_state with allow_pickle=False)"""
        import numpy as np
        with open(path, "wb") as f:
            np.savez(f, **self.export_exact_state())

    def load_exact_state(self, state_or_path, strict=True):
        """Warm start of the exact path: the exported entries into this cache, which must be fresh with its backing set -- ONE
        parallel launch builds the map, the entry records, the lists and the arena; no request is replayed.  state_or_path:
        what export_exact_state returned (of a GpuCache or a HostCache), or the path of a save_exact_state file.
        strict=True: the cache must have the exporter's policy, capacity, tables and EvLFU constants, and continues exactly
        as the exporter would have; strict=False: any capacity >= n, 'state' may be None (scalars derived, counters 0)."""
        entries, state, n_rows = read_exact_state(state_or_path)
        check_exact_rows(n_rows, getattr(self, "_n_rows", None), strict)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().evs_cache_exact_load(self._h, int(entries.shape[0]), entries.ctypes.data if entries.shape[0] else None,
                                                       None if state is None else state.ctypes.data, 1 if strict else 0,
                                                       torch.cuda.current_stream(self.device).cuda_stream))
        return self

    # ---- online row updates (include/evstore_hip.h: evs_cache_update_rows / evs_cache_refresh_rows) ----
    def _rows_call(self, keys, values, count, assume_distinct=False):
        from . import dlrm_ops
        if getattr(self, "_backing_ev", None) is not None:
            dlrm_ops.materialize_pending(self._backing_ev)   # deferred apply_emb results keep the rows of their own call
        keys, values = dlrm_ops.delta_tensors(keys, values, self.device, self.dim, assume_distinct)
        n = int(keys.shape[0])
        cnt = torch.zeros((1,), dtype=torch.int64, device=self.device) if count else None
        st = torch.cuda.current_stream(self.device).cuda_stream
        with torch.cuda.device(self.device):
            if values is None:
                _lib.check(_lib.lib().evs_cache_refresh_rows(self._h, n, keys.data_ptr(), cnt.data_ptr() if count else None, st))
            else:
                _lib.check(_lib.lib().evs_cache_update_rows(self._h, n, keys.data_ptr(), values.data_ptr(), int(values.stride(0)) if n else self.dim,
                                                            cnt.data_ptr() if count else None, st))
        return int(cnt.item()) if count else None

    def update_rows(self, keys, values, count=False, assume_distinct=False):
        """A delta of (table index 0-based, row) -> new fp32 vector, in ONE launch on the current stream: every vector is
        encoded in this tier's codec, stored at its row of the BACKING table and into the arena row of every key that is
        resident -- a lookup issued on this stream afterwards serves the new rows from either place.  Residency, priorities,
        lists and counters do not move.  keys (n, 2), values (n, dim): device tensors or anything torch.as_tensor takes;
        duplicate keys: the last one wins.  A resident server (serve_start / TierServer) is sent home first and started again
        by the next request.  A tier pair / triple: one call per cache, each over its own backing in its own codec.
        count=True: returns how many keys were resident WHEN THE CALL RAN (an EvLFU flush the last batch's close asked for
        runs with the next batched call, not here).  The de-duplication of the keys, host inputs and count=True make the
        call wait for the stream; assume_distinct=True with device tensors and count=False only enqueues (the keys are then
        distinct on the caller's word).  EvsError(EVS_ESTATE) over a FileTier."""
        return self._rows_call(keys, values, count, assume_distinct)

    def refresh_rows(self, keys, count=False, assume_distinct=False):
        """The arena row of every resident key of `keys` re-copied from its backing row: for callers that wrote the table
        themselves (pinned host tables written by the host, the files under a FileTier's registered tables)."""
        return self._rows_call(keys, None, count, assume_distinct)

    def stats(self):
        s = (C.c_int64 * 8)()
        _lib.check(_lib.lib().evs_cache_stats(self._h, s, torch.cuda.current_stream(self.device).cuda_stream))
        keys = ("min_c1", "n_perfect", "size", "n_flush", "n_evict", "n_requests", "n_perfect_hits", "n_hits")
        return dict(zip(keys, [int(v) for v in s]))

    def reset_counters(self):
        _lib.check(_lib.lib().evs_cache_reset_counters(self._h, torch.cuda.current_stream(self.device).cuda_stream))

    def dump(self):
        """Resident keys in list order: rows of (bucket | frequency | 0, table_1based, row)."""
        import numpy as np
        st = torch.cuda.current_stream(self.device).cuda_stream
        n = _lib.lib().evs_cache_dump(self._h, None, 0, st)
        if n < 0:
            _lib.check(int(n))
        out = np.zeros((max(n, 1), 3), np.int64)
        _lib.lib().evs_cache_dump(self._h, out.ctypes.data, n, st)
        return out[:n]


def request_c1c2(c1, c2, rows, threshold=23, out=None, tier=None):
    """Two-tier request (mixed_precs_caching/evlfu_8.cpp:669-796): c1 = main-precision GpuCache, c2 =
    secondary-precision GpuCache (both variant="cpp").  Returns (tier (B,T) uint8, out (B,T,dim) fp32)."""
    B = _check_batch(c1, rows, out, tier)
    if out is None:
        out = torch.empty((B, c1.n_tables, c1.dim), dtype=torch.float32, device=c1.device)
    if tier is None:
        tier = torch.empty((B, c1.n_tables), dtype=torch.uint8, device=c1.device)
    _lib.check(_lib.lib().evs_cache_request_c1c2(c1._h, c2._h, B, rows.data_ptr(), out.data_ptr(), tier.data_ptr(),
                                                 int(threshold), torch.cuda.current_stream(c1.device).cuda_stream))
    return tier, out


def lookup_batch_c1c2(c1, c2, rows, threshold=23, out=None, tier=None, c3=None):
    """Batched two-tier lookup with snapshot semantics (include/evstore_hip.h: evs_cache_lookup_batch_c1c2): the
    throughput form of request_c1c2.  Returns (tier (B,T) uint8: 1 = C1 hit, 2 = C2 hit, 0 = miss; out (B,T,dim) fp32).
    c3 (GpuAltKeyTier): the three-tier form (evs_cache_lookup_batch_c1c2c3) -- tier code 3 = the alt row was served.
    Both tiers set_miss_order('fetch-first'): the fetch-first pair -- the set-associative tiers over the shared set record with
    the update in front of the consumers, so either tier's tables may be pinned host tensors; same results as the default
    order (c1.fetch_stats() counts its re-point launch).  No c3 there."""
    B = _check_batch(c1, rows, out, tier)
    if c3 is None and _fed_pair_with_sources(c1, c2):
        return _pair_via_sources(c1, c2, rows, threshold, tier, lambda f1, f2: lookup_finish_c1c2(c1, c2, f1, f2, out))
    if out is None:
        out = torch.empty((B, c1.n_tables, c1.dim), dtype=torch.float32, device=c1.device)
    if tier is None:
        tier = torch.empty((B, c1.n_tables), dtype=torch.uint8, device=c1.device)
    st = torch.cuda.current_stream(c1.device).cuda_stream
    if c3 is None:
        _lib.check(_lib.lib().evs_cache_lookup_batch_c1c2(c1._h, c2._h, B, rows.data_ptr(), out.data_ptr(), tier.data_ptr(),
                                                          int(threshold), st))
    else:
        _lib.check(_lib.lib().evs_cache_lookup_batch_c1c2c3(c1._h, c2._h, c3._h, B, rows.data_ptr(), out.data_ptr(),
                                                            tier.data_ptr(), int(threshold), st))
    _ran_pair(c1, c2)
    return tier, out


# ---- fed backing of the fetch-first pair (include/evstore_hip.h: evs_cache_pair_fed_begin) ----
def lookup_begin_c1c2(c1, c2, rows, threshold=23, tier=None):
    """First half of a lookup on a fed pair (both tiers set_fed_backing over the same fed tables, each in its own codec, both
    'fetch-first'): the pair's probe.  -> (tier, keys1, keys2): tier the (B, n_tables) strict snapshot codes, keys_d an int64
    device tensor (a view of a buffer c_d owns, valid until its next begin) with every distinct missing key of a fed table that a
    missed position routed to tier d names, once, as table_1based << 32 | row.  A key routed both ways is in both lists.
    Synchronises.  `rows` and `tier` must stay alive until the finish; everything else on either cache is refused until
    lookup_finish[_interact]_c1c2 or lookup_abort_c1c2."""
    B = _check_batch(c1, rows, None, tier)
    if tier is None:
        tier = torch.empty((B, c1.n_tables), dtype=torch.uint8, device=c1.device)
    kbs = []
    for c in (c1, c2):
        kb = getattr(c, "_fed_keys", None)
        if kb is None or kb.numel() < B * c1.n_tables:
            kb = c._fed_keys = torch.empty(B * c1.n_tables, dtype=torch.int64, device=c1.device)
        kbs.append(kb)
    n1, n2 = C.c_int64(), C.c_int64()
    _lib.check(_lib.lib().evs_cache_pair_fed_begin(c1._h, c2._h, B, rows.data_ptr(), tier.data_ptr(), int(threshold), kbs[0].data_ptr(),
                                                   C.byref(n1), kbs[1].data_ptr(), C.byref(n2),
                                                   torch.cuda.current_stream(c1.device).cuda_stream))
    c1._fed_pair_call = (rows, tier, B, int(n1.value), int(n2.value), c2)   # keep alive
    return tier, kbs[0][:int(n1.value)], kbs[1][:int(n2.value)]


def _fed_pair_args(c1, c2, fed1, fed2):
    call = getattr(c1, "_fed_pair_call", None)
    if call is None or call[5] is not c2:
        raise _lib.EvsError(_lib.EVS_ESTATE, "lookup_finish_c1c2: no call is open on this pair (lookup_begin_c1c2)")
    _, tier, B, n1, n2, _ = call
    args = []
    for c, fed, n in ((c1, fed1, n1), (c2, fed2, n2)):
        rb = c.dim * c.codec // 8
        if fed is None:
            args += [0, 0]
            continue
        if not (fed.is_cuda and fed.dim() == 2 and fed.shape[0] >= n and fed.shape[1] * fed.element_size() == rb and fed.stride(1) == 1):
            raise ValueError("fed must be a device tensor of at least %d rows of %d bytes with unit inner stride, got %s %s" %
                             (n, rb, tuple(fed.shape), fed.dtype))
        args += [fed.data_ptr(), int(fed.stride(0)) * fed.element_size() if fed.shape[0] > 1 else rb]
    return B, tier, args


def lookup_finish_c1c2(c1, c2, fed1, fed2, out=None):
    """Second half: fed_d[i] is the row of keys_d[i] in tier d's codec (device tensor (n, row_bytes) uint8, or (n, dim) fp32 for
    codec 32; None where the list was empty) -> (tier, out (B, n_tables, dim) fp32)."""
    B, tier, a = _fed_pair_args(c1, c2, fed1, fed2)
    if out is None:
        out = torch.empty((B, c1.n_tables, c1.dim), dtype=torch.float32, device=c1.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * c1.n_tables * c1.dim):
        raise ValueError("out must be a contiguous fp32 device tensor of %d elements" % (B * c1.n_tables * c1.dim))
    _lib.check(_lib.lib().evs_cache_pair_fed_finish(c1._h, c2._h, a[0], a[1], a[2], a[3], out.data_ptr(),
                                                    torch.cuda.current_stream(c1.device).cuda_stream))
    c1._fed_pair_call = None
    _ran_pair(c1, c2)
    return tier, out


def lookup_finish_interact_c1c2(c1, c2, fed1, fed2, x, itself=False, out=None):
    """lookup_finish_c1c2 with the fused interaction as the consumer -> (tier, R (B, dim + P))."""
    B, tier, a = _fed_pair_args(c1, c2, fed1, fed2)
    F = c1.n_tables + 1
    P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    if out is None:
        out = torch.empty((B, c1.dim + P), dtype=torch.float32, device=c1.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * (c1.dim + P)):
        raise ValueError("out must be a contiguous fp32 device tensor of %d elements" % (B * (c1.dim + P)))
    if not (x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (B, c1.dim) and x.stride(1) == 1):
        raise ValueError("x must be a (B, %d) fp32 device tensor with unit inner stride" % c1.dim)
    _lib.check(_lib.lib().evs_cache_pair_fed_finish_interact(
        c1._h, c2._h, a[0], a[1], a[2], a[3], x.data_ptr(), int(x.stride(0)) if B > 1 else c1.dim, int(bool(itself)), out.data_ptr(),
        torch.cuda.current_stream(c1.device).cuda_stream))
    c1._fed_pair_call = None
    _ran_pair(c1, c2)
    return tier, out


def lookup_abort_c1c2(c1, c2):
    """Drops the open pair call: nothing was inserted or raised, the batch is not counted, the same begin lists the same keys."""
    _lib.check(_lib.lib().evs_cache_pair_fed_abort(c1._h, c2._h))
    c1._fed_pair_call = None


def fed_stats_c1c2(c1, c2):
    """Counters of the fed pair, cumulative: 'calls' (finished), 'keys1' / 'keys2' (listed per tier), 'missed' (missed positions of
    fed tables), 'from_block' (of those, served from a fed block), 'spilled' (rows the update spilled) and 'from_spill' (hit
    positions served from the spill).  Synchronises."""
    s = (C.c_int64 * 8)()
    _lib.check(_lib.lib().evs_cache_pair_fed_stats(c1._h, c2._h, s, torch.cuda.current_stream(c1.device).cuda_stream))
    return {"calls": int(s[0]), "keys1": int(s[1]), "keys2": int(s[2]), "missed": int(s[3]), "from_block": int(s[4]),
            "spilled": int(s[5]), "from_spill": int(s[6])}


def _fed_pair_with_sources(c1, c2):
    return all(getattr(c, "_fed", False) and getattr(c, "_row_source", None) is not None for c in (c1, c2))


def _pair_via_sources(c1, c2, rows, threshold, tier, finish):
    """begin -> the two row sources -> finish; whatever fails in between leaves no call open (GpuCache._via_source's guard)"""
    tier, k1, k2 = lookup_begin_c1c2(c1, c2, rows, threshold, tier)
    try:
        return finish(c1._fetch_fed(k1), c2._fetch_fed(k2))
    except BaseException:
        if getattr(c1, "_fed_pair_call", None) is not None:
            try:
                lookup_abort_c1c2(c1, c2)
            except _lib.EvsError:   # (the library had already spent the call)
                c1._fed_pair_call = None
        raise


def _ran_pair(c1, c2):
    """a pair call went through: C1 of a fetch-first pair reports the pair's fourth counter from here on (fetch_stats)"""
    if getattr(c1, "_fetch_first", False) and getattr(c2, "_fetch_first", False):
        c1._pair_fetch_first = True


# ---- ragged bags through the pair (include/evstore_hip.h: evs_cache_lookup_bags_c1c2) ----
def _check_bag_pair(c1, c2):
    if not (c1.n_tables == c2.n_tables and c1.dim == c2.dim):
        raise ValueError("the tiers must agree on n_tables and dim")


def lookup_bags_c1c2(c1, c2, lS_o, lS_i, threshold=23, out=None):
    """Multi-hot lookup through the batched C1 + C2 pair (both 'evlfu' after set_bag_rule('served-bags'); the pair that shares its
    set records): every position is probed against both tiers as they stand when the call starts (code 1 = in C1, 2 = in C2,
    0 = neither), a sample's agg_hit is the number of its T bags without a missed position, every hit way is raised to it, a
    missed position is routed by the reference's rule on the snapshot and served from its destination tier's table at that
    tier's precision, every distinct missed key is inserted once; the bags pool the served rows in index order, each decoded at
    the precision of the tier that serves it (include/evstore_hip.h: evs_cache_lookup_bags_c1c2).  lS_o / lS_i as
    GpuCache.lookup_bags takes them.
    Both tiers set_miss_order('fetch-first') AND set_bag_count('count-first'): the fetch-first bag chain -- probe, count, route +
    raise + list, the pair's update, a kernel that re-points every position at where its row is now, then the pooling -- so every
    distinct missing row is read once, by the update, and either tier's tables may be pinned host tensors.  Codes, pooled bits
    and the tier state equal the default order's; c1.fetch_stats() counts the call and its 'repointed' / 'in_place' /
    'victim_hits' positions.  Both at 'fetch-first' without 'count-first' on both, or one tier alone at 'fetch-first': EVS_EINVAL;
    a 'consume-first' pair over pinned tables: EVS_ESTATE, as before.
    -> (tiers: T uint8 tensors, one code per index, views of one flat array; ly: T (B, dim) fp32 tensors, views of one
    (T, B, dim) block -- `out`, when given)."""
    _check_bag_pair(c1, c2)
    B, idx_c, off_c, nnz_c, flat, tiers, _keep = c1._bags_call(lS_o, lS_i)
    T, d = c1.n_tables, c1.dim
    if out is None:
        out = torch.empty((T, B, d), dtype=torch.float32, device=c1.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (T, B, d)):
        raise ValueError("out must be a contiguous (%d, %d, %d) fp32 device tensor" % (T, B, d))
    _lib.check(_lib.lib().evs_cache_lookup_bags_c1c2(c1._h, c2._h, B, idx_c, off_c, nnz_c, out.data_ptr(), B * d, d, flat.data_ptr(),
                                                     int(threshold), torch.cuda.current_stream(c1.device).cuda_stream))
    _ran_pair(c1, c2)
    return tiers, list(out.unbind(0))


def lookup_bags_interact_c1c2(c1, c2, lS_o, lS_i, x, threshold=23, itself=False, out=None):
    """R = interact_features(x, the T pooled bags of lookup_bags_c1c2): the same rule and codes, the pooling into a (T, B, dim)
    block C1 owns, the dense interaction, then the pair's update (include/evstore_hip.h: evs_cache_lookup_bags_interact_c1c2).
    A pair with both tiers at 'fetch-first' and 'count-first' runs the fetch-first bag chain of lookup_bags_c1c2 (update and
    re-point in front of the pooling; tables in HBM or pinned host memory; same codes, R bits and tier state).  There the batch is
    already inserted when the interaction refuses its arguments; in the default order nothing is inserted then.
    -> (tiers as lookup_bags_c1c2 gives them, R (B, dim + F (F - 1) / 2) with F = T + 1)."""
    _check_bag_pair(c1, c2)
    B, idx_c, off_c, nnz_c, flat, tiers, _keep = c1._bags_call(lS_o, lS_i)
    F = c1.n_tables + 1
    P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    if not (x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (B, c1.dim) and x.stride(1) == 1):
        raise ValueError("x must be a (B, %d) fp32 device tensor with unit inner stride" % c1.dim)
    if out is None:
        out = torch.empty((B, c1.dim + P), dtype=torch.float32, device=c1.device)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == B * (c1.dim + P)):
        raise ValueError("out must be a contiguous fp32 device tensor of %d elements" % (B * (c1.dim + P)))
    _lib.check(_lib.lib().evs_cache_lookup_bags_interact_c1c2(
        c1._h, c2._h, B, idx_c, off_c, nnz_c, x.data_ptr(), int(x.stride(0)) if B > 1 else c1.dim, int(bool(itself)),
        out.data_ptr(), flat.data_ptr(), int(threshold), torch.cuda.current_stream(c1.device).cuda_stream))
    _ran_pair(c1, c2)
    return tiers, out


# ---- warm start of the pair (include/evstore_hip.h: evs_cache_pair_export / evs_cache_pair_load) ----
def export_state_c1c2(c1, c2):
    """What the batched C1 + C2 pair holds, at rest (pending closes folded, a wanted flush run on either tier) -> a dict of
    numpy arrays: 'entries' (n, 6) int64 rows of (tier 1 | 2, table_1based, row, score, age, slot) sorted by (tier, slot),
    'state' (32,) int64 (format version 3, n_tables, dim, nset, then per tier capacity, codec, ways, sub-sets, stamp bits S,
    batch number, five counters, 0) and 'n_rows1' / 'n_rows2' (T,) int64, the rows of each tier's backing tables.  The pair
    must share its set records (the default geometry of lookup_batch_c1c2 on two set-associative tiers)."""
    import numpy as np
    L, st = _lib.lib(), torch.cuda.current_stream(c1.device).cuda_stream
    state = np.zeros(32, np.int64)
    with torch.cuda.device(c1.device):
        n = L.evs_cache_pair_export(c1._h, c2._h, None, 0, None, st)
        if n < 0:
            _lib.check(int(n))
        entries = np.zeros((max(n, 1), 6), np.int64)
        n2 = L.evs_cache_pair_export(c1._h, c2._h, entries.ctypes.data, n, state.ctypes.data, st)
    if n2 != n:
        if n2 < 0:
            _lib.check(int(n2))
        raise _lib.EvsError(_lib.EVS_ESTATE, "export_state_c1c2: the pair changed between the count and the export")
    return {"entries": entries[:n], "state": state, "n_rows1": np.asarray(getattr(c1, "_n_rows", []), np.int64),
            "n_rows2": np.asarray(getattr(c2, "_n_rows", []), np.int64)}


def save_state_c1c2(c1, c2, path):
    """export_state_c1c2() into an .npz file (np.savez; read back by load_state_c1c2 with allow_pickle=False)"""
    import numpy as np
    with open(path, "wb") as f:
        np.savez(f, **export_state_c1c2(c1, c2))


def load_state_c1c2(c1, c2, state_or_path, strict=True):
    """Warm start of the pair: the exported entries into two caches that must BOTH be fresh with their backing set -- the pair
    starts as its first lookup would start it, then one launch copies every entry's row from its tier's table into its tier's
    arena and stores its way word; the host decides every placement.  state_or_path: what export_state_c1c2 returned, or the
    path of a save_state_c1c2 file.  strict=True: the pair must have the exporter's capacities, tables and geometry, and
    continues exactly as the exporter would have; strict=False: every key is placed anew in its own tier of this pair's
    geometry (per effective set the highest scores, youngest first, the rest turned away); 'state' may then be None (batch
    number = the largest age, counters 0).  An alt-key tier's membership is not carried.
    -> {'placed': (p1, p2), 'turned_away': (t1, t2), 'batch'}"""
    import numpy as np
    if isinstance(state_or_path, dict):
        d = state_or_path
    else:
        try:
            with np.load(state_or_path, allow_pickle=False) as z:
                d = {k: z[k] for k in z.files}
        except Exception as e:
            raise _lib.EvsError(_lib.EVS_EIO, "load_state_c1c2: %s is not a readable state file (%s)" % (state_or_path, e))
    missing = [k for k in ("entries", "state") + (() if isinstance(state_or_path, dict) else ("n_rows1", "n_rows2")) if k not in d]
    if missing:
        raise _lib.EvsError(_lib.EVS_EINVAL, "load_state_c1c2: the state lacks %s" % ", ".join(repr(k) for k in missing))
    entries = np.ascontiguousarray(d["entries"], np.int64)
    state = None if d["state"] is None else np.ascontiguousarray(d["state"], np.int64)
    if entries.ndim != 2 or entries.shape[1] != 6 or (state is not None and state.shape != (32,)):
        raise _lib.EvsError(_lib.EVS_EINVAL, "load_state_c1c2: 'entries' must be (n, 6) and 'state' (32,)")
    if state is not None and int(state[0]) != 3:
        raise _lib.EvsError(_lib.EVS_EINVAL, "load_state_c1c2: unknown format version %d (the pair's state is version 3)" % int(state[0]))
    for c, key in ((c1, "n_rows1"), (c2, "n_rows2")):
        if strict and d.get(key) is not None and hasattr(c, "_n_rows") and list(np.asarray(d[key]).astype(np.int64)) != list(c._n_rows):
            raise _lib.EvsError(_lib.EVS_EINVAL, "load_state_c1c2: a strict load needs backing tables of the exporter's row counts (%s)" % key)
    out8 = np.zeros(8, np.int64)
    with torch.cuda.device(c1.device):
        _lib.check(_lib.lib().evs_cache_pair_load(c1._h, c2._h, int(entries.shape[0]), entries.ctypes.data if entries.shape[0] else None,
                                                  None if state is None else state.ctypes.data, 1 if strict else 0, out8.ctypes.data,
                                                  torch.cuda.current_stream(c1.device).cuda_stream))
    return {"placed": (int(out8[0]), int(out8[3])), "turned_away": (int(out8[1]), int(out8[4])), "batch": int(out8[6])}


def lookup_batch_c1c2c3(c1, c2, c3, rows, threshold=23, out=None, tier=None):
    return lookup_batch_c1c2(c1, c2, rows, threshold, out, tier, c3=c3)


def lookup_interact_c1c2c3(c1, c2, c3, rows, x, threshold=23, itself=False, out=None, tier=None, fused=True):
    return lookup_interact_c1c2(c1, c2, rows, x, threshold, itself, out, tier, fused, c3=c3)


def lookup_interact_c1c2(c1, c2, rows, x, threshold=23, itself=False, out=None, tier=None, fused=True, c3=None):
    """The two-tier snapshot lookup with interact_features as its consumer -> (tier, R).  fused (default): every row is
    decoded from the precision of the tier that serves it inside the interaction kernel (evs_cache_lookup_interact_c1c2);
    fused=False: lookup_batch_c1c2 into fp32 (B,T,dim) rows (`out`), then the dense interaction over them."""
    if not fused or c1.dim not in (16, 32, 36):
        from .dlrm_ops import interact_features
        tier, rows_fp32 = lookup_batch_c1c2(c1, c2, rows, threshold, out, tier, c3=c3)
        return tier, interact_features(x, list(rows_fp32.unbind(1)), "dot", itself)
    B = _check_batch(c1, rows, None, tier)
    if c3 is None and _fed_pair_with_sources(c1, c2):
        return _pair_via_sources(c1, c2, rows, threshold, tier, lambda f1, f2: lookup_finish_interact_c1c2(c1, c2, f1, f2, x, itself))
    F = c1.n_tables + 1
    P = F * (F + 1) // 2 if itself else F * (F - 1) // 2
    R = torch.empty((B, c1.dim + P), dtype=torch.float32, device=c1.device)
    if tier is None:
        tier = torch.empty((B, c1.n_tables), dtype=torch.uint8, device=c1.device)
    if not (x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (B, c1.dim) and x.stride(1) == 1):
        raise ValueError("x must be a (B, %d) fp32 device tensor with unit inner stride" % c1.dim)
    xs = int(x.stride(0)) if B > 1 else c1.dim
    st = torch.cuda.current_stream(c1.device).cuda_stream
    if c3 is None:
        _lib.check(_lib.lib().evs_cache_lookup_interact_c1c2(
            c1._h, c2._h, B, rows.data_ptr(), x.data_ptr(), xs, int(bool(itself)), R.data_ptr(), tier.data_ptr(), int(threshold), st))
    else:
        _lib.check(_lib.lib().evs_cache_lookup_interact_c1c2c3(
            c1._h, c2._h, c3._h, B, rows.data_ptr(), x.data_ptr(), xs, int(bool(itself)), R.data_ptr(), tier.data_ptr(),
            int(threshold), st))
    _ran_pair(c1, c2)
    return tier, R


class GpuAltKeyTier:
    """C3: key -> alt-key map with second-chance FIFO (deterministic re-specification of
    mixed_precs_caching/aprx_embedding.cpp).  alt_tables: per table a device uint32 tensor (viewed as int32 is fine)
    with alt_key[row] = alt_row*100 + alt_table_1based."""

    def __init__(self, capacity, alt_tables, device="cuda"):
        self.device = torch.device(device)
        self.n_tables = len(alt_tables)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().evs_aprx_create(C.byref(h), int(capacity), self.n_tables))
        self._h = h
        self._alt = [t.contiguous() for t in alt_tables]
        ptrs = (C.c_void_p * self.n_tables)(*[t.data_ptr() for t in self._alt])
        rows = (C.c_int64 * self.n_tables)(*[int(t.numel()) for t in self._alt])
        _lib.check(_lib.lib().evs_aprx_set_altkeys(self._h, ptrs, rows))

    def __del__(self):
        try:
            if self._h:
                _lib.lib().evs_aprx_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def stats(self):
        s = (C.c_int64 * 4)()
        _lib.check(_lib.lib().evs_aprx_stats(self._h, s, torch.cuda.current_stream(self.device).cuda_stream))
        return dict(size=int(s[0]), n_hit=int(s[1]), n_pending=int(s[2]), error=int(s[3]))

    def batch_dump(self):
        """Batched form: (members as an (n,3) int64 array of (table_1based, row, recency flag), stats dict)."""
        import numpy as np
        st = torch.cuda.current_stream(self.device).cuda_stream
        o4 = (C.c_int64 * 4)()
        n = _lib.lib().evs_aprx_batch_dump(self._h, None, 0, o4, st)
        if n < 0:
            _lib.check(int(n))
        out = np.zeros((max(n, 1), 3), np.int64)
        _lib.lib().evs_aprx_batch_dump(self._h, out.ctypes.data_as(C.POINTER(C.c_int64)), n, o4, st)
        return out[:n], dict(members=int(o4[0]), n_hit=int(o4[1]), capacity=int(o4[2]))

    def apply_ops(self, ops):
        """APRX_EV's single-key methods in order: ops (n,3) int32 device tensor of (op, table_1based, row) with op 0
        insert_altkey | 1 get_altkey | 2 set_recency_flag | 3 evict_one_key (aprx_embedding.cpp:278-288,341-350,390-411).
        -> uint32-valued int64 tensor: the alt key for op 0 / 1 (0xffffffff = miss), else 0."""
        assert ops.dtype == torch.int32 and ops.is_cuda and ops.is_contiguous() and ops.dim() == 2 and ops.shape[1] == 3
        res = torch.zeros((ops.shape[0],), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().evs_aprx_apply_ops(self._h, int(ops.shape[0]), ops.data_ptr(), res.data_ptr(),
                                                 torch.cuda.current_stream(self.device).cuda_stream))
        return res.to(torch.int64) & 0xffffffff

    def queue(self):
        """the FIFO front to back as (n,2) int64 (table_1based, row), stale duplicates included"""
        st = torch.cuda.current_stream(self.device).cuda_stream
        n = int(_lib.lib().evs_aprx_dump_queue(self._h, None, 0, st))
        if n < 0:
            _lib.check(n)
        out = (C.c_int64 * (2 * max(n, 1)))()
        _lib.lib().evs_aprx_dump_queue(self._h, out, n, st)
        return torch.tensor(list(out)[:2 * n], dtype=torch.int64).view(n, 2)


def request_c1c2c3(c1, c2, c3, rows, threshold=23, out=None, tier=None):
    """request_to_c1_c2_c3 (evlfu_8.cpp:492-667): tier codes 1 C1 hit, 2 C2 hit, 3 alt-key hit, 0 miss."""
    assert rows.dtype == torch.int32 and rows.is_cuda and rows.is_contiguous()
    B = int(rows.shape[0])
    if out is None:
        out = torch.empty((B, c1.n_tables, c1.dim), dtype=torch.float32, device=c1.device)
    if tier is None:
        tier = torch.empty((B, c1.n_tables), dtype=torch.uint8, device=c1.device)
    _lib.check(_lib.lib().evs_cache_request_c1c2c3(c1._h, c2._h, c3._h if c3 is not None else None, B, rows.data_ptr(),
                                                   out.data_ptr(), tier.data_ptr(), int(threshold),
                                                   torch.cuda.current_stream(c1.device).cuda_stream))
    return tier, out


class TierServer:
    """The tier pair / triple as a resident server (include/evstore_hip.h: evs_tiers_serve_*): request_c1c2 / request_c1c2c3
    one request at a time without a launch and a synchronise per request.  c1, c2: GpuCache (variant="cpp", backing set),
    c3: GpuAltKeyTier or None.  Keeps its members alive; any call on a member that reads or writes its exact state
    (stats, dump, request, ...) sends the server home first and the next request starts it again."""

    def __init__(self, c1, c2, c3=None, threshold=23, n_slots=4, idle_us=200):
        import numpy as np
        _warn_hw_queues()
        self.c1, self.c2, self.c3 = c1, c2, c3
        self.n_tables, self.dim, self.device = c1.n_tables, c1.dim, c1.device
        self.ring = torch.empty((n_slots, self.n_tables, self.dim), dtype=torch.float32, device=self.device)
        self._views = [self.ring[k] for k in range(n_slots)]   # (a tensor index per request is 2 us)
        self._rows = np.zeros(self.n_tables, np.int32)
        self._tier = np.zeros(self.n_tables, np.uint8)
        self._slot = C.c_int(0)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().evs_tiers_serve_start(C.byref(h), c1._h, c2._h, c3._h if c3 is not None else None, int(threshold),
                                                        self.ring.data_ptr(), int(n_slots), int(idle_us)))
        self._h = h
        self._call = (_lib.lib().evs_tiers_serve_request, self._h, self._rows.ctypes.data, self._tier.ctypes.data, C.byref(self._slot))

    def request(self, row_ids):
        """row_ids: n_tables ints (host) -> (tier codes: a numpy uint8 view valid until the next request; the (T, dim) fp32
        rows as a DEVICE view of a ring slot, valid until n_slots - 1 more requests are posted -- see consumed())."""
        self._rows[:] = row_ids
        fn, h, rp, tp, sp = self._call
        rc = fn(h, rp, tp, sp)
        if rc:
            _lib.check(rc)
        return self._tier, self._views[self._slot.value]

    def request_to(self, row_ids, out):
        """the same request with the rows written into `out` (a contiguous (T, dim) fp32 DEVICE tensor, not in use by pending
        work); row_ids: n_tables ints on the host, or a (T, ...) int64 device tensor whose element 0 of each row is the id.
        -> tier codes (numpy uint8 view)"""
        if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == self.n_tables * self.dim):
            raise ValueError("out must be a contiguous fp32 device tensor of %d elements" % (self.n_tables * self.dim))
        L = _lib.lib()
        if torch.is_tensor(row_ids) and row_ids.is_cuda:
            if row_ids.dtype != torch.int64 or row_ids.shape[0] != self.n_tables:
                raise ValueError("device ids: a (T, ...) int64 tensor")
            _lib.check(L.evs_tiers_serve_request_to(self._h, None, row_ids.data_ptr(), int(row_ids.stride(0)), out.data_ptr(), self._tier.ctypes.data))
        else:
            self._rows[:] = row_ids
            _lib.check(L.evs_tiers_serve_request_to(self._h, self._rows.ctypes.data, None, 0, out.data_ptr(), self._tier.ctypes.data))
        return self._tier

    def consumed(self, slot=None, stream=None):
        """the reads of ring slot `slot` (default: the last request's) have been enqueued on `stream` (default: the current one)"""
        st = torch.cuda.current_stream(self.device) if stream is None else stream
        _lib.check(_lib.lib().evs_tiers_serve_consumed(self._h, int(self._slot.value if slot is None else slot), st.cuda_stream))

    def stop(self):
        """send the server home for good (the members' state is back in HBM); later requests raise"""
        if self._h:
            _lib.check(_lib.lib().evs_tiers_serve_stop(self._h))

    def close(self):
        if self._h:
            _lib.lib().evs_tiers_serve_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
