// The mailbox of the two batch-1 resident servers: the single-tier exact server (evs_cache_serve_*, cache_serve_kernel) and
// the tier pair / triple server (evs_tiers_serve_*, cache_c1c2_serve_kernel).  Layout, host protocol, host server state and
// the device side of the protocol, once.  (evs_rf_server in evs_fused_rf.hip speaks another protocol and is not described here.)
//
// A server is ONE wavefront that stays resident and takes one request at a time from three 128-byte lines in mapped host
// memory -- the reference's operating point is batch 1 (cache_algo/EvLFU_C1.py:97-166, dlrm_s_pytorch_C1.py:227-275), where
// a launch and a synchronise per request cost twice what the request does.
//   request line  (host -> device): four 32-byte sectors of seven row ids and a guard word (the sequence number) -- the host
//                 writes the ids, then the four guards; the device reads the line as one load (bus reads of 32 or 64 bytes
//                 that may be taken at different times) and accepts it when ALL guards hold the number it waits for: every
//                 sector was then read after its guard, hence after its ids, was written -- whatever the granularity the
//                 fabric delivers the line in.  The id of table t rides in word t + t / 7.
//                 Ids by ADDRESS (bit 31 of every guard set): the first words of the line carry the address of table 0's
//                 id (int64, device memory), the elements between two tables' ids and the destination; the server reads
//                 the ids itself (the reference's loop has them on the DEVICE -- dlrm_wrap moved lS_i there -- and
//                 fetching them back costs a copy and a synchronise per request).
//                 Destination: a DEVICE address of the caller's for the T x d fp32 rows, 0 = this request's ring slot.
//                 Beside ids it rides in the id words of tables 26 and 27, hence at most 26 tables there.
//   control line  (host -> device): word 0 = stop; the server reads it with the same load (lane 32).
//   answer line   (device -> host): the T flag bytes first, then `done` (the sequence number served) and `alive`.
// Without a destination the rows go to slot (sequence % n_slots) of a ring in HBM: the caller gets DEVICE rows with no launch,
// copy or synchronise.  An idle server leaves by itself after idle_ticks of the 100 MHz wall clock (a device-wide synchronise
// elsewhere in the process waits no longer than that); the host starts it again with the next request.
#pragma once
#include <stdint.h>
#include <string.h>

namespace evs {

struct MailboxLayout {
    static constexpr int kLineWords = 32;                                  // a line: 128 bytes
    static constexpr int kReqLine = 0, kCtlLine = 32, kAnsLine = 64;       // word offsets into the block
    static constexpr int kBlockBytes = 3 * kLineWords * 4;
    static constexpr int kIdsPerSector = 7;
    static constexpr int kGuardWords[4] = {7, 15, 23, 31};                 // the last word of every 32-byte sector
    static constexpr unsigned long long kGuardLanes = 0x80808080ull;       // ... as lanes of the server's one load
    static constexpr int kStopWord = kCtlLine;                             // from the request line's base: lane 32 of that load
    static constexpr int kDoneWord = 16, kAliveWord = 17;                  // of the answer line (bytes 0..63: the flags)
    static constexpr unsigned kSeqMask = 0x7fffffffu, kByAddrBit = 0x80000000u;   // of a guard
    static constexpr int id_word(int t) { return t + t / kIdsPerSector; }
    static constexpr int kIdsAddrLo = 0, kIdsAddrHi = 1, kIdsStride = 2;   // by address: where the ids are ...
    static constexpr int kOutByAddrLo = 3, kOutByAddrHi = 4;               // ... and where the rows go
    static constexpr int kOutLo = 29, kOutHi = 30;                         // beside ids: where the rows go
    static constexpr int kMaxTables = 4 * kIdsPerSector;                   // 28
    static constexpr int kMaxTablesTo = 26;                                // with a destination beside ids
};
static_assert(MailboxLayout::id_word(MailboxLayout::kMaxTables - 1) == MailboxLayout::kGuardWords[3] - 1, "28 ids fill the line");
static_assert(MailboxLayout::id_word(MailboxLayout::kMaxTablesTo) == MailboxLayout::kOutLo &&
              MailboxLayout::id_word(MailboxLayout::kMaxTablesTo + 1) == MailboxLayout::kOutHi, "the destination rides in the id words of tables 26, 27");
static_assert(MailboxLayout::kAliveWord * 4 >= 64 && MailboxLayout::kDoneWord * 4 >= 64, "behind the flag bytes");

// ---- the host's half of the protocol: no HIP call in it ---------------------------------------------------------------------
struct MailboxHost {
    using L = MailboxLayout;
    volatile unsigned *line = nullptr;   // the host's view of the block
    unsigned seq = 0;                    // the number last posted
    int slots = 0;
    struct Posted { unsigned want; int slot; };

    unsigned next_want() const { return (seq + 1u) & L::kSeqMask; }
    int next_slot() const { return (int)(next_want() % (unsigned)slots); }
    void set_stop(bool on) {
        line[L::kStopWord] = on ? 1u : 0u;
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
    }
    // exactly one of rows (host ids) / ids_dev (their device address) is given; out_dev: 0 = the ring
    Posted post(int T, const int32_t *rows, const void *ids_dev, long long ids_stride, const void *out_dev) {
        volatile unsigned *req = line + L::kReqLine;
        const unsigned want = next_want();
        const int slot = (int)(want % (unsigned)slots);
        seq = want;
        const unsigned long long oa = (unsigned long long)reinterpret_cast<uintptr_t>(out_dev);
        unsigned guard = want;
        if (rows) {
            for (int t = 0; t < T; t++) req[L::id_word(t)] = (unsigned)rows[t];
            if (T <= L::kMaxTablesTo) { req[L::kOutLo] = (unsigned)oa; req[L::kOutHi] = (unsigned)(oa >> 32); }
        } else {
            const unsigned long long pa = (unsigned long long)reinterpret_cast<uintptr_t>(ids_dev);
            req[L::kIdsAddrLo] = (unsigned)pa; req[L::kIdsAddrHi] = (unsigned)(pa >> 32); req[L::kIdsStride] = (unsigned)ids_stride;
            req[L::kOutByAddrLo] = (unsigned)oa; req[L::kOutByAddrHi] = (unsigned)(oa >> 32);
            guard |= L::kByAddrBit;
        }
        __atomic_thread_fence(__ATOMIC_RELEASE);
        for (int g : L::kGuardWords) req[g] = guard;
        __atomic_thread_fence(__ATOMIC_SEQ_CST);
        return {want, slot};
    }
    // Spins until the server has answered `want`, then copies the T flag bytes.  Every 64 spins, while nobody is alive (never
    // started, went home idle, or was paused), on_idle(false) may start a server: 0 to go on, else the code to return.  After
    // 2^31 spins on_idle(true) sends home whoever may still be there and names the code.  A request that fails leaves host
    // and device agreeing on the sequence number: the one the device last ANSWERED.
    template <class OnIdle>
    int await(unsigned want, unsigned char *flags, int T, OnIdle on_idle) {
        volatile unsigned *ans = line + L::kAnsLine;
        long long spins = 0;
        auto fail = [&](int rc) { seq = ans[L::kDoneWord]; return rc; };
        while (ans[L::kDoneWord] != want) {
            if ((spins & 63) == 0 && ans[L::kAliveWord] == 0u) {
                const int rc = on_idle(false);
                if (rc) return fail(rc);
            }
            if (++spins > (1ll << 31)) return fail(on_idle(true));
            __builtin_ia32_pause();
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        const volatile unsigned char *fl = reinterpret_cast<const volatile unsigned char *>(ans);
        for (int t = 0; t < T; t++) flags[t] = fl[t];
        return 0;
    }
};

}  // namespace evs

#ifdef __HIPCC__
#include "evs_common.h"
#include <vector>

namespace evs {

struct ServeArgs {
    volatile unsigned *req;     // request line (device address of the mapped host block)
    volatile unsigned *ctl;     // control line (directly behind it: the server reads both with one load)
    volatile unsigned *ans;     // answer line
    float *ring; int n_slots;
    long long idle_ticks;
};

// ---- the host's server state: the mapped block, the server's stream, the ring, and the events that order the server ----------
// against everything else that touches the exact state or reads the ring:
//   exact_done: recorded behind every exact-path launch on the CALLER's stream; a server started afterwards waits for it
//               on its own stream (two kernels must never mutate the lists / the map / the free stack at once);
//   slot_done[s]: recorded by consumed() on the stream that READS ring slot s; the request that is about to hand slot s out
//               again waits for it on the host (the server overwrites the slot in host order).
// (Round 6 tried the request + control lines in DEVICE memory, written by the host through the large-BAR aperture:
//  tools/mailbox_probe.hip's bare echo makes a round trip in 1.8 us against 2.4, the server's p50 did not move -- 14.3-14.9
//  against 14.4-14.8 us over four runs each --, so the lines stay where an ordinary store reaches them.)
struct ServeHost {
    unsigned *block = nullptr, *block_dev = nullptr;
    MailboxHost mb;
    hipStream_t stream = nullptr;
    float *ring = nullptr;
    long long idle_ticks = 0;
    hipEvent_t exact_done = nullptr; bool exact_pending = false;
    std::vector<hipEvent_t> slot_done; std::vector<char> slot_busy;

    bool is_open() const { return block != nullptr; }
    // all or nothing: a failure leaves the object closed
    int open(const char *who) {
        auto fail = [&](int rc) { (void)hipGetLastError(); close(); return rc; };
        if (hipHostMalloc(reinterpret_cast<void **>(&block), MailboxLayout::kBlockBytes, hipHostMallocMapped) != hipSuccess) { block = nullptr; set_error("%s: no mailbox", who); return fail(EVS_ENOMEM); }
        memset(block, 0, MailboxLayout::kBlockBytes);
        if (hipHostGetDevicePointer(reinterpret_cast<void **>(&block_dev), block, 0) != hipSuccess) { set_error("%s: the mailbox is not device-accessible", who); return fail(EVS_EHIP); }
        // a stream of the highest priority: streams share a handful of hardware queues, round-robin per priority level, and a
        // queue runs its commands in order -- a copy or a kernel of the caller's that lands on the queue of the resident server
        // waits until the server goes home idle (measured through the plug-in loop: 299 us per request instead of 104 once a
        // process had made a few more streams).  Nothing else of this library uses the level.
        int prio_lo = 0, prio_hi = 0;
        if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess || hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio_hi) != hipSuccess) {
            stream = nullptr; set_error("%s: no stream", who); return fail(EVS_EHIP);
        }
        mb.line = block; mb.seq = 0;
        return EVS_OK;
    }
    // a new ring: whoever still reads the old one finishes first
    void rearm(float *ring_, int n_slots, long long idle_us) {
        for (size_t k = 0; k < slot_busy.size(); k++)
            if (slot_busy[k]) { (void)hipEventSynchronize(slot_done[k]); slot_busy[k] = 0; }
        for (size_t k = (size_t)n_slots; k < slot_done.size(); k++)
            if (slot_done[k]) (void)hipEventDestroy(slot_done[k]);
        slot_done.resize((size_t)n_slots, nullptr); slot_busy.assign((size_t)n_slots, 0);
        ring = ring_; mb.slots = n_slots;
        idle_ticks = idle_us * 100;   // wall_clock64(): 100 MHz
    }
    // send the server home (it writes the state back on its way out); the next request starts it again
    int pause(const char *who) {
        if (!block || !stream) return EVS_OK;
        if (hipStreamQuery(stream) == hipSuccess) return EVS_OK;   // nothing running
        (void)hipGetLastError();
        mb.set_stop(true);
        const hipError_t e = hipStreamSynchronize(stream);
        mb.set_stop(false);
        if (e != hipSuccess) { set_error("%s: the server's stream failed: %s", who, hipGetErrorString(e)); return EVS_EHIP; }
        return EVS_OK;
    }
    // behind every exact-path launch: where a server started later has to wait (only caches that have a server pay the record)
    int launched(hipStream_t st) {
        if (!stream) return EVS_OK;
        if (!exact_done) EVS_HIP_CHECK(hipEventCreateWithFlags(&exact_done, hipEventDisableTiming));
        EVS_HIP_CHECK(hipEventRecord(exact_done, st));
        exact_pending = true;
        return EVS_OK;
    }
    // a launch on another stream that touches the state goes behind the pending exact-path launch as well
    int wait_exact(hipStream_t st) {
        if (exact_pending && exact_done) EVS_HIP_CHECK(hipStreamWaitEvent(st, exact_done, 0));
        return EVS_OK;
    }
    // an exact-path launch of the caller's may still be running on ITS stream: the server starts behind it
    ServeArgs before_launch() {
        if (exact_pending) { (void)hipStreamWaitEvent(stream, exact_done, 0); exact_pending = false; }
        ServeArgs sv;
        sv.req = block_dev + MailboxLayout::kReqLine; sv.ctl = block_dev + MailboxLayout::kCtlLine; sv.ans = block_dev + MailboxLayout::kAnsLine;
        sv.ring = ring; sv.n_slots = mb.slots; sv.idle_ticks = idle_ticks;
        return sv;
    }
    // The caller has ENQUEUED its reads of ring slot `slot` (a copy, a kernel) on `st`: the slot is handed out again only
    // after they have finished.
    int consumed(int slot, hipStream_t st) {
        hipEvent_t &e = slot_done[(size_t)slot];
        if (!e) EVS_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        EVS_HIP_CHECK(hipEventRecord(e, st));
        slot_busy[(size_t)slot] = 1;
        return EVS_OK;
    }
    // One request -> T flag bytes on the host, the rows in out_dev or in ring slot *slot_out (-1 with out_dev).  Blocks until
    // the server has answered (no launch, no copy, no synchronise: two cache-line hand-overs over the bus).
    // launch(sv, stream) starts the caller's server kernel; it is the only thing the two servers differ in.
    template <class Launch>
    int request(const char *who, int T, const int32_t *rows, const int64_t *ids_dev, int64_t ids_stride, float *out_dev,
                uint8_t *flags, int *slot_out, Launch launch) {
        const int slot = mb.next_slot();
        if (!out_dev && slot_busy[(size_t)slot]) {   // whoever still READS the slot (consumed()) finishes first
            EVS_HIP_CHECK(hipEventSynchronize(slot_done[(size_t)slot]));
            slot_busy[(size_t)slot] = 0;
        }
        const MailboxHost::Posted p = mb.post(T, rows, ids_dev, ids_stride, out_dev);
        const int rc = mb.await(p.want, flags, T, [&](bool gave_up) -> int {
            if (gave_up) {   // (a server sent home re-reads the answer line's number when it starts again)
                (void)pause(who);
                set_error("%s: the server did not answer", who);
                return EVS_EHIP;
            }
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) {
                launch(before_launch(), stream);
                if (hipGetLastError() != hipSuccess) { set_error("%s: the server could not be started", who); return EVS_EHIP; }
            }
            else if (q != hipErrorNotReady) { (void)hipGetLastError(); set_error("%s: the server's stream failed", who); return EVS_EHIP; }
            else (void)hipGetLastError();
            return EVS_OK;
        });
        if (rc) return rc;
        *slot_out = out_dev ? -1 : p.slot;
        return EVS_OK;
    }
    void close() {
        (void)pause("close");
        if (stream) { (void)hipStreamSynchronize(stream); (void)hipStreamDestroy(stream); stream = nullptr; }
        if (block) { (void)hipHostFree(block); block = nullptr; block_dev = nullptr; mb.line = nullptr; }
        if (exact_done) { (void)hipEventDestroy(exact_done); exact_done = nullptr; }
        for (hipEvent_t e : slot_done) if (e) (void)hipEventDestroy(e);
        slot_done.clear(); slot_busy.clear();
    }
};

// ---- the device's half: one wavefront, requests strictly in order -----------------------------------------------------------
// developer A/B of what stands between the flags and `done`: 0 a wait for the wave's own stores (the rows were written THROUGH,
// agent scope: a fence here is an L2 write-back per request), 1 a system-scope fence, 2 an agent-scope one
#ifndef EVS_X_SERVE_FENCE
#define EVS_X_SERVE_FENCE 0
#endif
// -> the sequence number last served (the host's and the device's numbers meet in the answer line)
__device__ __forceinline__ unsigned mbox_enter(const ServeArgs &sv, int lane) {
    const unsigned seq = __hip_atomic_load(const_cast<unsigned *>(sv.ans) + MailboxLayout::kDoneWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (lane == 0) __hip_atomic_store(const_cast<unsigned *>(sv.ans) + MailboxLayout::kAliveWord, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    return seq;
}
// Waits for request seq + 1.  false: stop word or idle time-out, the server leaves.  true: row = the id of this lane's table
// (0 for a lane past T), out = where the T x d rows go.
__device__ __forceinline__ bool mbox_next(const ServeArgs &sv, int lane, int T, int d, unsigned seq, int &row, float *&out) {
    using L = MailboxLayout;
    const unsigned want = (seq + 1u) & L::kSeqMask;
    const long long t0 = (long long)wall_clock64();
    unsigned word = 0u;
    for (;;) {
        // ONE load per poll (the control word as a second dependent load made the request wait out both): lanes 0..31 the
        // request line, lane 32 the stop word in the line behind it
        word = __hip_atomic_load(const_cast<unsigned *>(sv.req) + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if ((__ballot((word & L::kSeqMask) == want) & L::kGuardLanes) == L::kGuardLanes) break;
        const unsigned stop = (unsigned)__builtin_amdgcn_readlane((int)word, L::kStopWord);
        if (stop != 0u || (long long)wall_clock64() - t0 > sv.idle_ticks) return false;
        __builtin_amdgcn_s_sleep(4);
    }
    auto w = [&](int i) { return (unsigned)__builtin_amdgcn_readlane((int)word, i); };
    row = __shfl((int)word, L::id_word(lane) & (L::kLineWords - 1));
    const bool by_addr = (w(L::kGuardWords[0]) & L::kByAddrBit) != 0u;
    unsigned long long out_a = 0ull;
    if (by_addr) {   // one agent-scope load per lane
        const unsigned long long pa = ((unsigned long long)w(L::kIdsAddrHi) << 32) | w(L::kIdsAddrLo);
        const long long stride = (long long)w(L::kIdsStride);
        const long long *ip = reinterpret_cast<const long long *>((uintptr_t)pa) + (long long)(lane < T ? lane : 0) * stride;
        row = (int)__hip_atomic_load(ip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out_a = ((unsigned long long)w(L::kOutByAddrHi) << 32) | w(L::kOutByAddrLo);
    } else if (T <= L::kMaxTablesTo) out_a = ((unsigned long long)w(L::kOutHi) << 32) | w(L::kOutLo);
    if (lane >= T) row = 0;
    out = out_a ? reinterpret_cast<float *>((uintptr_t)out_a) : sv.ring + (long long)(want % (unsigned)sv.n_slots) * T * d;
    return true;
}
// The answer: this lane's flag byte, then -- behind a wait that also puts the rows where every later launch sees them -- the
// sequence number the host is polling for.  -> that number.
__device__ __forceinline__ unsigned mbox_answer(const ServeArgs &sv, int lane, int T, unsigned char flag, unsigned seq) {
    seq = (seq + 1u) & MailboxLayout::kSeqMask;
    if (lane < T) const_cast<volatile unsigned char *>(reinterpret_cast<volatile unsigned char *>(sv.ans))[lane] = flag;
    unsigned *done = const_cast<unsigned *>(sv.ans) + MailboxLayout::kDoneWord;
#if EVS_X_SERVE_FENCE == 1
    __threadfence_system();
    if (lane == 0) __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
#elif EVS_X_SERVE_FENCE == 2
    __threadfence();
    if (lane == 0) __hip_atomic_store(done, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
#else
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    if (lane == 0) __hip_atomic_store(done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // (a release here would be the write-back again)
#endif
    return seq;
}
// the state is back in HBM: only now may the host start another server (or anything else) on it
__device__ __forceinline__ void mbox_leave(const ServeArgs &sv, int lane) {
    __threadfence_system();
    if (lane == 0) __hip_atomic_store(const_cast<unsigned *>(sv.ans) + MailboxLayout::kAliveWord, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace evs
#endif  // __HIPCC__
