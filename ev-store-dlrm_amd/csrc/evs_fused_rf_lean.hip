// The lean entry of the rows-in-registers fused kernel (evs_fused_rf.hip) for the STACKED call: x + T fp32 tables behind one
// (T, B) index array and, lS_o given, one (T, B) offsets array -- what evs_emb_interact_dot_stacked passes (FusedArgs::stk).
//
// The FusedArgs entry hands every block a 3 KB by-value struct: the scalars the first index load needs sit 2 KB into the
// kernel-argument segment and arrive by scalar loads from lines the host wrote microseconds earlier, and lanes 0..31 of every
// block read seven 256-byte arrays out of the same lines before the block barrier in front of the row requests -- two of the
// dependent round trips in the head of the one generation of co-resident blocks (docs/HISTORY.md 3.2b, round 7).  Here
//   * the kernel arguments are a dozen scalars, ordered so that what tile_load(0) needs comes first: this unit alone is built
//     with -mllvm -amdgpu-kernarg-preload-count=14 (csrc/Makefile), so the leading 14 dwords are in SGPRs when a wave starts
//     and the index loads are arithmetic on registers (where the firmware does not preload, the compiler's compatibility
//     prologue loads the same values itself: correct either way);
//   * what is a constant of the model -- table addresses, row counts -- comes from a descriptor in device memory (RfModelDesc),
//     one 16-byte load per lane, built once per distinct model and kept in a small cache below.
// The body is rf_body<..., LEAN>: the same arithmetic, the same bits.
//
// Build-time A/B (tools/variants.sh name@evs_fused_rf_lean:"-D..."):  -DEVS_RF_LEAN=0: launch_rf_lean always declines (the
// FusedArgs entry everywhere);  -DEVS_RF_LEAN_PRELOAD=0: the same scalars behind a by-value struct, which is never preloaded.
#define EVS_PT_TABLE g_pt_lean
#include "evs_fused_rf_body.h"
#include "evs_desc_cache.h"

#include <atomic>
#include <mutex>
#include <stdio.h>

#ifndef EVS_RF_LEAN
#define EVS_RF_LEAN 1
#endif
#ifndef EVS_RF_LEAN_PRELOAD
#define EVS_RF_LEAN_PRELOAD 1
#endif

namespace evs {

// the kernel's arguments, in the order of the preloaded form: 14 dwords up to and including R, 64 bytes in all.  Everything the
// index / offsets loads of tile_load(0) need is inside the 14 (the readable length of an offsets row is B or B + 1: one bit of fti)
struct RfLeanArgs {
    const int64_t *idx;        // (T, B) indices, row 0
    const int64_t *off;        // (T, B) offsets, row 0; nullptr: one index per bag declared
    int idx_stride, off_stride;   // elements between the rows of two tables
    int B;
    unsigned fti;              // F | tile_per << 8 | itself << 16 | (offsets row has B + 1 entries) << 17
    const RfModelDesc *md;
    const float *x;
    float *R;
    int x_stride, P;
};

template <int CQ, int REM, int NT, int D, bool CHECK>
__device__ __forceinline__ void rf_lean_run(const RfLeanArgs &la) {
    // what rf_body reads of a FusedArgs, filled in registers (the arrays are never touched: `ka` is not read by the LEAN body)
    FusedArgs a;
    a.F = (int)(la.fti & 0xffu); a.tile_per = (int)((la.fti >> 8) & 0xffu); a.itself = (int)((la.fti >> 16) & 1u);
    a.P = la.P; a.B = la.B; a.R = la.R;
    a.stk = 1; a.stk_idx = la.idx; a.stk_off = la.off; a.stk_idx_stride = la.idx_stride; a.stk_off_stride = la.off_stride;
    a.stk_off_len = (int64_t)la.B + (int64_t)((la.fti >> 17) & 1u);
    a.multi_n = 0; a.multi_cpb = 0;
    a.dummy_i64 = la.idx;      // (entry 0 of the index array: readable, and an address the scalars already hold)
    a.zeros = nullptr; a.err = nullptr;   // (LEAN: from the descriptor)
    rf_body<CQ, REM, NT, D, false, false, false, CHECK, false, true>(a, nullptr, RfServeDesc{}, (int)blockIdx.x, false,
                                                                      RfLeanX{la.md, la.x, la.x_stride});
}

// (the stem and the leading template arguments are the FusedArgs entry's: the profile summaries and the bench's label find both)
#if EVS_RF_LEAN_PRELOAD
template <int CQ, int REM, int NT, int D, bool MLP, bool IDS, bool PROBE, bool CHECK, bool LEAN>
__global__ void __launch_bounds__(256, (CQ >= 4 ? 2 : EVS_RF_LB))
emb_interact_rf_kernel(const int64_t *idx, const int64_t *off, int idx_stride, int off_stride, int B, unsigned fti, const RfModelDesc *md,
                       const float *x, float *R, int x_stride, int P) {
    static_assert(LEAN && !MLP && !IDS && !PROBE, "the lean entry of the plain / CHECK launch");
    rf_lean_run<CQ, REM, NT, D, CHECK>(RfLeanArgs{idx, off, idx_stride, off_stride, B, fti, md, x, R, x_stride, P});
}
template <auto K>
static void lean_launch(const RfLeanArgs &la, unsigned blocks, hipStream_t st) {
    hipLaunchKernelGGL(K, dim3(blocks), dim3(256), 0, st, la.idx, la.off, la.idx_stride, la.off_stride, la.B, la.fti, la.md, la.x, la.R,
                       la.x_stride, la.P);
}
#else
template <int CQ, int REM, int NT, int D, bool MLP, bool IDS, bool PROBE, bool CHECK, bool LEAN>
__global__ void __launch_bounds__(256, (CQ >= 4 ? 2 : EVS_RF_LB)) emb_interact_rf_kernel(const RfLeanArgs la) {
    static_assert(LEAN && !MLP && !IDS && !PROBE, "the lean entry of the plain / CHECK launch");
    rf_lean_run<CQ, REM, NT, D, CHECK>(la);
}
template <auto K>
static void lean_launch(const RfLeanArgs &la, unsigned blocks, hipStream_t st) {
    hipLaunchKernelGGL(K, dim3(blocks), dim3(256), 0, st, la);
}
#endif

// ---- the descriptors: one allocation per cache slot, made on first use and kept for the life of the process like the
// library's other lazily made buffers (zero page, error flag); a slot that changes hands is overwritten in place.
namespace {
std::mutex g_desc_mu;
DescLru g_desc_lru;
RfModelDesc *g_desc_dev[kDescCacheSlots] = {};
int g_desc_devno[kDescCacheSlots] = {};     // the device each slot's allocation lives on
}

// a thread that allocates or copies while ANOTHER thread captures in global mode (the default of torch.cuda.graph) invalidates that
// capture; in relaxed mode this thread's calls are its own business -- what torch's allocator does around its hipMalloc
struct RelaxedCaptureMode {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    bool ok;
    RelaxedCaptureMode() { ok = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess; if (!ok) (void)hipGetLastError(); }
    ~RelaxedCaptureMode() { if (ok && hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) (void)hipGetLastError(); }
};

// the descriptor of the model in `a` (device memory), or nullptr: unknown while `st` is capturing, every slot pinned, or a HIP error
// (called with g_desc_mu held; the caller keeps it until its launch is enqueued, so that a slot cannot change hands between the
//  look-up and the launch that reads it)
static const RfModelDesc *model_desc(const FusedArgs &a, hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    DescKey key;
    key.dev = dev; key.d = a.d; key.codec = 32; key.T = a.F - 1;
    for (int k = 0; k < key.T; k++) { key.table[k] = a.src[k + 1]; key.n_rows[k] = a.n_rows[k + 1]; }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    const bool capturing = cs != hipStreamCaptureStatusNone;
    int slot = g_desc_lru.find(key);
    if (slot >= 0) {
        if (capturing) g_desc_lru.pin(slot);   // the graph keeps the address: this slot never changes hands again
        return g_desc_dev[slot];
    }
    if (capturing) return nullptr;             // (no allocation, no copy, no synchronisation inside a capture)
    bool evicts = false;
    slot = g_desc_lru.victim(&evicts);
    if (slot < 0) {
        // every slot belongs to a captured graph: new models keep the FusedArgs entry, about a microsecond slower per launch
        static bool told = false;
        if (!told) fprintf(stderr, "libevstore_hip: all %d model descriptors are held by captured graphs; further models run the fused launch without one\n", kDescCacheSlots);
        told = true;
        return nullptr;
    }
    RfModelDesc h;
    memset(&h, 0, sizeof h);
    for (int k = 0; k < key.T; k++) {
        h.feat[k + 1].base = (unsigned long long)reinterpret_cast<uintptr_t>(a.src[k + 1]);
        h.feat[k + 1].n_rows = (unsigned)a.n_rows[k + 1];
        h.feat[k + 1].row_bytes = (unsigned)(a.d * 4);
    }
    h.zeros = a.zeros; h.err = a.err;
    RelaxedCaptureMode relaxed;
    // a slot that held another model: launches of that model may still be reading it -- rare (more than kDescCacheSlots
    // models in turn), so the plain answer is to wait for the device.  An allocation that lives on another device goes, and
    // this device makes its own below.  After a failure the slot either still holds its old model, whole, or is free -- with
    // no allocation, or (the copy below failed) with its own device's allocation still attached, which the next model to take the
    // slot overwrites: the wait for the device has already happened, and a free slot is handed out without one.
    const int was = g_desc_devno[slot];
    const bool foreign = g_desc_dev[slot] && was != dev;
    if (evicts || foreign) {
        bool ok = !foreign || hipSetDevice(was) == hipSuccess;
        ok = ok && hipDeviceSynchronize() == hipSuccess;
        if (ok && foreign) {
            ok = hipFree(g_desc_dev[slot]) == hipSuccess;
            if (ok) { g_desc_dev[slot] = nullptr; g_desc_lru.drop(slot); }
        }
        if (foreign) ok = hipSetDevice(dev) == hipSuccess && ok;
        if (!ok) { (void)hipGetLastError(); return nullptr; }
        g_desc_lru.drop(slot);
    }
    if (!g_desc_dev[slot]) {
        void *p = nullptr;
        if (hipMalloc(&p, sizeof(RfModelDesc)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        g_desc_dev[slot] = static_cast<RfModelDesc *>(p);
        g_desc_devno[slot] = dev;
    }
    if (hipMemcpy(g_desc_dev[slot], &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    g_desc_lru.put(slot, key);
    return g_desc_dev[slot];
}

// how many launches took the lean entry in this process (tests: a silent decline computes the same results)
static std::atomic<unsigned long long> g_lean_launches{0};

int rf_lean_pt_add(unsigned long long *h, int reset) {
#ifdef EVS_X_PT
    static unsigned long long l[1024 * 16], z[1024 * 16];
    if (hipMemcpyFromSymbol(l, HIP_SYMBOL(evs::g_pt_lean), sizeof l) != hipSuccess) return -2;
    for (int i = 0; i < 1024 * 16; i++) h[i] += l[i];
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(evs::g_pt_lean), z, sizeof z) != hipSuccess) return -3;
#else
    (void)h; (void)reset;
#endif
    return 0;
}

bool launch_rf_lean(const FusedArgs &a, int tile_per, hipStream_t st) {
#if !EVS_RF_LEAN
    return false;
#else
    if (!a.stk || a.multi_n != 0 || !(a.bag1 == 1 || a.bag1 == 3) || a.F < 2 || a.F > kTileMaxF) return false;
    if (tile_per < 1 || tile_per > 16) return false;
    const auto fits = [](int64_t v) { return v >= INT32_MIN && v <= INT32_MAX; };
    if (!fits(a.stk_idx_stride) || !fits(a.stk_off_stride) || !fits(a.B) || !fits(a.stride[0]) || a.B < 1) return false;
    // (the entry's checks have passed -- evs_emb_interact_dot: alignment, ranges, NULLs; what the descriptor records of the
    //  model was checked there on this very call, and an equal key means equal values.  The host side of the call is NOT leaner
    //  than before: the stacked call still fills its evs_feature[] and FusedArgs and runs every check per call, and this function
    //  adds a lock, two HIP queries and the key compare -- a host path of its own for the stacked call is left for later.)
    const bool check = a.bag1 == 3;
    if (check && (!a.stk_off || !(a.stk_off_len == a.B || a.stk_off_len == a.B + 1))) return false;   // (whole batches: B or B + 1 offsets)
    switch (a.d) { case 16: case 32: case 36: case 64: break; default: return false; }
    std::lock_guard<std::mutex> lk(g_desc_mu);
    const RfModelDesc *md = model_desc(a, st);
    if (!md) return false;
    RfLeanArgs la;
    la.idx = a.stk_idx; la.off = check ? a.stk_off : nullptr;
    la.idx_stride = (int)a.stk_idx_stride; la.off_stride = check ? (int)a.stk_off_stride : 0;
    la.B = (int)a.B; la.fti = (unsigned)a.F | ((unsigned)tile_per << 8) | ((unsigned)(a.itself ? 1 : 0) << 16) |
             ((check && a.stk_off_len == a.B + 1) ? 1u << 17 : 0u);
    la.md = md; la.x = reinterpret_cast<const float *>(a.src[0]); la.R = a.R;
    la.x_stride = (int)a.stride[0]; la.P = a.P;
    const unsigned blocks = (unsigned)((a.B + tile_per - 1) / tile_per);
    const bool nt2 = a.F > 16;
#define EVS_RF_LEAN_GO(CQ_, REM_)                                                                                        \
    do {                                                                                                                 \
        if (check) {                                                                                                     \
            if (nt2) lean_launch<emb_interact_rf_kernel<CQ_, REM_, 2, EVS_RF_DEPTH, false, false, false, true, true>>(la, blocks, st);   \
            else lean_launch<emb_interact_rf_kernel<CQ_, REM_, 1, EVS_RF_DEPTH, false, false, false, true, true>>(la, blocks, st);       \
        } else {                                                                                                         \
            if (nt2) lean_launch<emb_interact_rf_kernel<CQ_, REM_, 2, EVS_RF_DEPTH, false, false, false, false, true>>(la, blocks, st);  \
            else lean_launch<emb_interact_rf_kernel<CQ_, REM_, 1, EVS_RF_DEPTH, false, false, false, false, true>>(la, blocks, st);      \
        }                                                                                                                \
    } while (0)
    switch (a.d) {
    case 16: EVS_RF_LEAN_GO(1, 0); break;
    case 32: EVS_RF_LEAN_GO(2, 0); break;
    case 36: EVS_RF_LEAN_GO(2, 1); break;
    default: EVS_RF_LEAN_GO(4, 0); break;
    }
#undef EVS_RF_LEAN_GO
    g_lean_launches.fetch_add(1, std::memory_order_relaxed);
    return true;
#endif
}

}  // namespace evs

// developer / test hook, not part of the header's ABI (as evs_x_pt)
extern "C" __attribute__((visibility("default"))) unsigned long long evs_x_lean_launches(void) {
    return evs::g_lean_launches.load(std::memory_order_relaxed);
}
