// Fused embedding gather + pairwise-dot interaction, "rows in flight in registers" form of the bag-1 index-tile loop.
//
// Same computation and the same bits as emb_interact_dot_lds_kernel<..., BAG1, TILE> (evs_fused.hip):
//     R[b] = [ x[b] | strict-lower(T[b] T[b]^T) ],  T[b] = [x[b]; W_0[idx_0[b]]; ...; W_{F-2}[idx_{F-2}[b]]]
// (dlrm_s_pytorch.py:407-461 apply_emb with one index per bag -- the Criteo collate, dlrm_data_pytorch.py:407-408 --
//  followed by :483-516 interact_features), one wavefront per sample, MFMA 16x16x4 f32 chains, output row staged
// in LDS and written one iteration later.  What changes is WHERE a sample's rows wait while they travel:
//
//   LDS-DMA loop:  the rows of sample k+1 are DMA'd into the wave's single 4 KiB LDS slot while sample k computes: one
//                  sample in flight per wave, and a 16 384-sample launch (4 samples per wave) is a chain of 4 memory
//                  round trips per wave plus fill and drain.
//   this kernel:   a block owns ONE 16-sample chunk; the rows of all 4 samples of a wave are requested at once and
//                  travel in REGISTERS, in the DMA-shaped mapping (LPRD = d/4 consecutive lanes fetch one row as d*4
//                  contiguous bytes with one global_load_dwordx4 each; 64/LPRD rows per instruction, every line
//                  requested once): 16 VGPRs hold one d=36 sample.  The LDS slot is only the transpose buffer between
//                  that mapping and the MFMA operand mapping (ds_write_b128 x 4, ds_read_b128 x 6 per sample).  The
//                  code is straight-line, so hipcc's own counted s_waitcnt vmcnt(15..12) consumes sample u while
//                  samples u+1.. stay in flight (with any branch around a memory operation the waitcnt pass takes the
//                  minimum over paths and drains everything: measured, see docs/HISTORY.md 3.2b).
// Used for batches whose blocks are all resident at once (B <= 16 x 4 x 256 = 16 384); larger batches keep the LDS-DMA
// loop, whose steady state is bound by the per-CU vector-memory / LDS pipes rather than by latency (docs/HISTORY.md 3.2).
// Measured (same box, A/B by EVS_FUSED_RF): B = 16 384: 20.5 -> 18.9 us, B = 8 192: 12.5 -> 11.4 us.
//
// Row addresses need no cross-lane traffic here: the index tile in LDS has one row PER FEATURE (x and dense features
// carry the sample number as their "index"), and a lane of the DMA mapping reads the tile entry of the row it fetches.
#include <fcntl.h>
#include <unistd.h>
#include "evs_fused.h"

#include <stdlib.h>
#include <string.h>
#include <atomic>
#include "evs_fused_rf_body.h"

namespace evs {

template <int CQ, int REM, int NT, int D, bool MLP = false, bool IDS = false, bool PROBE = false, bool CHECK = false>
__global__ void __launch_bounds__(256, (MLP ? 3 : (CQ >= 4 ? 2 : EVS_RF_LB))) emb_interact_rf_kernel(const FusedArgs args) {
    rf_body<CQ, REM, NT, D, MLP, IDS, PROBE, CHECK, false>(args, (const FusedArgs *)__builtin_amdgcn_kernarg_segment_ptr(), RfServeDesc{}, (int)blockIdx.x);
}

static int rf_mode() {
    static int v = -1;
    if (v < 0) { const char *e = evs::env_switch("EVS_FUSED_RF"); v = e ? atoi(e) : 1; }   // developer switch: 0 = the LDS-DMA loop
    return v;
}

// developer switch: bytes of dynamic LDS added to every block, i.e. fewer blocks per CU (27 KB static: 4 per CU; +20 KB: 3;
// +40 KB: 2) -- does a launch whose blocks arrive in two waves overlap its own fill and drain?
// Checked on the host, once per kernel: static + dynamic LDS beyond the device's limit per block would fail the launch and leave
// R unwritten, so such a value is refused here (one warning line, no padding) and never reaches the launch.
static long long rf_pad_lds_env() {
    static const long long v = env_switch_range("EVS_FUSED_RF_PADLDS", 0, 0, 1ll << 30);
    return v;
}
template <auto K>
static unsigned rf_pad_lds() {
    if (rf_pad_lds_env() == 0) return 0u;
    static const unsigned v = [] {
        hipFuncAttributes fa;
        int dev = 0, limit = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
            hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(K)) != hipSuccess) {
            (void)hipGetLastError();
            fprintf(stderr, "libevstore_hip: EVS_FUSED_RF_PADLDS ignored: the LDS limit of the device could not be read\n");
            return 0u;
        }
        if (rf_pad_lds_env() + (long long)fa.sharedSizeBytes > (long long)limit) {
            fprintf(stderr, "libevstore_hip: EVS_FUSED_RF_PADLDS=%lld ignored: with %zu bytes of static LDS it exceeds the %d bytes a block may use\n",
                    rf_pad_lds_env(), (size_t)fa.sharedSizeBytes, limit);
            return 0u;
        }
        return (unsigned)rf_pad_lds_env();
    }();
    return v;
}
// developer switch: samples per block (16: one generation of co-resident blocks at B = 16 384; 8 / 4: the grid arrives in two / four
// generations whose heads and bodies can overlap -- the per-block timeline of tools/probe_stage_probe.py asked for the experiment.
// Measured on the plain launch, B = 16 384: 19.2 us at 16, 28.8 at 8, 48.7 at 4 -- but a wave still issues four samples' worth of
// requests (the missing ones against the zero page; the body does not build at a depth of 2), so this prices a block's fixed cost,
// not two generations as such: EVS_FUSED_RF_PADLDS -- the same blocks, fewer per CU -- is the fair form of that question.
// Plain and CHECK launches only (launch_rf, launch_rf_check pass it): the cache tier's per-block buffers (PROBE), and the IDS / MLP
// forms, are sized for 16 samples per block and always get 16.)
static int rf_tile_per() {
    static int v = -1;
    if (v < 0) { const char *e = evs::env_switch("EVS_FUSED_RF_TILE"); v = e ? atoi(e) : 16; if (v != 4 && v != 8 && v != 12) v = 16; }
    return v;
}
template <auto K>
static void launch_rf_grid(FusedArgs a, hipStream_t st, int tile_per = 16) {
    a.tile_per = tile_per;   // (default 16) one 16-sample chunk per block: 4 samples per wave, all requested at once
    hipLaunchKernelGGL(K, dim3((unsigned)((a.B + a.tile_per - 1) / a.tile_per)), dim3(256), rf_pad_lds<K>(), st, a);
}

// the batch sizes this form is for: every block resident at once (4 blocks of 256 threads per CU at 128 VGPRs)
// (-1 from the read: unset, or a value that was refused -- both mean the default behaviour)
static int64_t rf_max_batch_env() {
    static const int64_t v = env_switch_range("EVS_FUSED_RF_MAX_B", -1, 0, 1ll << 40);
    return v;
}
static int64_t rf_max_batch() {
    return rf_max_batch_env() >= 0 ? rf_max_batch_env() : 16ll * kNumCu * EVS_RF_LB;
}

// the dispatch record of the MLP form (evs_mlp1_kernels_seen, include/evstore_hip.h): one counter per instantiation, bumped next to
// its launch.  id = (d: 16 / 32 / 36) * 2 + (NT - 1)
constexpr int kMlp1Count = 6;
static std::atomic<long long> g_mlp1_seen[kMlp1Count];

bool launch_rf_mlp(const FusedArgs &a, hipStream_t st) {
    if (a.F > kTileMaxF || a.bag1 != 1 || a.kp > kMlpRowStride - 4 || (a.kp & 15) || a.kp < a.d + a.P) return false;
    const bool nt2 = a.F > 16;
    switch (a.d) {
    case 16:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<1, 0, 2, 4, true>>(a, st); else launch_rf_grid<emb_interact_rf_kernel<1, 0, 1, 4, true>>(a, st);
        g_mlp1_seen[0 + nt2].fetch_add(1, std::memory_order_relaxed);
        return true;
    case 32:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 0, 2, 4, true>>(a, st); else launch_rf_grid<emb_interact_rf_kernel<2, 0, 1, 4, true>>(a, st);
        g_mlp1_seen[2 + nt2].fetch_add(1, std::memory_order_relaxed);
        return true;
    case 36:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 1, 2, 4, true>>(a, st); else launch_rf_grid<emb_interact_rf_kernel<2, 1, 1, 4, true>>(a, st);
        g_mlp1_seen[4 + nt2].fetch_add(1, std::memory_order_relaxed);
        return true;
    default:
        return false;
    }
}

bool rf_ids_supported(int64_t B, int F, int d) {
    return rf_mode() && F <= kTileMaxF && B <= rf_max_batch() && (d == 16 || d == 32 || d == 36);
}
bool launch_rf_ids(const FusedArgs &a, hipStream_t st) {
    if (!rf_ids_supported(a.B, a.F, a.d) || !a.row_ids || !a.arena) return false;
    const bool nt2 = a.F > 16;
    switch (a.d) {
    case 16:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<1, 0, 2, EVS_RF_DEPTH, false, true>>(a, st); else launch_rf_grid<emb_interact_rf_kernel<1, 0, 1, EVS_RF_DEPTH, false, true>>(a, st);
        return true;
    case 32:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 0, 2, EVS_RF_DEPTH, false, true>>(a, st); else launch_rf_grid<emb_interact_rf_kernel<2, 0, 1, EVS_RF_DEPTH, false, true>>(a, st);
        return true;
    default:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 1, 2, EVS_RF_DEPTH, false, true>>(a, st); else launch_rf_grid<emb_interact_rf_kernel<2, 1, 1, EVS_RF_DEPTH, false, true>>(a, st);
        return true;
    }
}

bool launch_rf_probe(const FusedArgs &a, hipStream_t st) {
    if (!rf_ids_supported(a.B, a.F, a.d) || (!a.probe.slots && !a.probe.sa.tags) || !a.arena) return false;
    const bool nt2 = a.F > 16;
    switch (a.d) {
    case 16:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<1, 0, 2, EVS_RF_DEPTH, false, false, true>>(a, st); else launch_rf_grid<emb_interact_rf_kernel<1, 0, 1, EVS_RF_DEPTH, false, false, true>>(a, st);
        return true;
    case 32:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 0, 2, EVS_RF_DEPTH, false, false, true>>(a, st); else launch_rf_grid<emb_interact_rf_kernel<2, 0, 1, EVS_RF_DEPTH, false, false, true>>(a, st);
        return true;
    default:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 1, 2, EVS_RF_DEPTH, false, false, true>>(a, st); else launch_rf_grid<emb_interact_rf_kernel<2, 1, 1, EVS_RF_DEPTH, false, false, true>>(a, st);
        return true;
    }
}

// the same launch with lS_o given (whole batches, FusedArgs::bag1 == 3): the kernel checks the offsets of its 16 samples itself
// d = 64 (the Terabyte scripts' width, round 3): the same kernel with CQ = 4 -- 16 lanes per row, 4 rows per load, 7 loads
// per sample, 135 VGPRs (three blocks per CU).  Same box, B = 16 384: one index per bag declared 30.4 -> 25.6 us (0.59 -> 0.70 of
// peak), lS_o given 33.2 -> 27.5 us; B = 65 536: 91.5 -> 89.5 us.
static bool rf_d64() {
    static const bool on = evs::env_switch_on("EVS_FUSED_RF_D64");
    return on;
}

// the lean entry (evs_fused_rf_lean.hip) takes the stacked call at the widths this unit has kernels for; the developer switches that
// reshape the launch keep their meaning (EVS_FUSED_RF_TILE is passed on, EVS_FUSED_RF_PADLDS keeps the FusedArgs entry it pads)
static bool rf_lean_shape(const FusedArgs &a) {
    return a.stk != 0 && a.multi_n == 0 && rf_pad_lds_env() == 0 && (a.d == 16 || a.d == 32 || a.d == 36 || (a.d == 64 && rf_d64()));
}

bool launch_rf_check(const FusedArgs &a, hipStream_t st) {
    static const bool on = evs::env_switch_on("EVS_FUSED_RF_CHECK");
    if (!on || !rf_mode() || a.F > kTileMaxF || a.bag1 != 3 || a.B > rf_max_batch()) return false;
    if (rf_lean_shape(a) && launch_rf_lean(a, rf_tile_per(), st)) return true;   // the stacked call: scalar arguments + model descriptor
    const bool nt2 = a.F > 16;
    switch (a.d) {
    case 16:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<1, 0, 2, EVS_RF_DEPTH, false, false, false, true>>(a, st, rf_tile_per()); else launch_rf_grid<emb_interact_rf_kernel<1, 0, 1, EVS_RF_DEPTH, false, false, false, true>>(a, st, rf_tile_per());
        return true;
    case 32:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 0, 2, EVS_RF_DEPTH, false, false, false, true>>(a, st, rf_tile_per()); else launch_rf_grid<emb_interact_rf_kernel<2, 0, 1, EVS_RF_DEPTH, false, false, false, true>>(a, st, rf_tile_per());
        return true;
    case 36:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 1, 2, EVS_RF_DEPTH, false, false, false, true>>(a, st, rf_tile_per()); else launch_rf_grid<emb_interact_rf_kernel<2, 1, 1, EVS_RF_DEPTH, false, false, false, true>>(a, st, rf_tile_per());
        return true;
    case 64:
        if (!rf_d64()) return false;
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<4, 0, 2, EVS_RF_DEPTH, false, false, false, true>>(a, st, rf_tile_per()); else launch_rf_grid<emb_interact_rf_kernel<4, 0, 1, EVS_RF_DEPTH, false, false, false, true>>(a, st, rf_tile_per());
        return true;
    default:
        return false;
    }
}

// K batches in one launch: K * ceil(B / 16) one-chunk blocks; the hardware hands a CU the next block as one retires, so the
// drain of a batch's last blocks runs under the fill of the next batch's first ones (what two alternating streams give a
// caller, without any stream: cross-stream event waits cost more here than they return -- measured, docs/HISTORY.md 3.2d)
bool rf_multi_supported(int64_t B, int F, int d) {
    return rf_mode() && F <= kTileMaxF && B >= 1 && (d == 16 || d == 32 || d == 36 || (d == 64 && rf_d64()));
}
template <auto K>
static void launch_rf_multi_grid(FusedArgs a, hipStream_t st) {
    a.tile_per = 16;
    a.multi_cpb = (int)((a.B + 15) / 16);
    hipLaunchKernelGGL(K, dim3((unsigned)(a.multi_cpb * a.multi_n)), dim3(256), 0, st, a);
}
bool launch_rf_multi(const FusedArgs &a, hipStream_t st) {
    if (!rf_multi_supported(a.B, a.F, a.d) || a.multi_n < 1 || a.multi_n > kMultiMax || !(a.bag1 == 1 || a.bag1 == 3)) return false;
    const bool nt2 = a.F > 16;
#define EVS_RF_MULTI(CQ_, REM_)                                                                                              \
    do {                                                                                                                     \
        if (a.bag1 == 1) {                                                                                                   \
            if (nt2) launch_rf_multi_grid<emb_interact_rf_kernel<CQ_, REM_, 2, EVS_RF_DEPTH>>(a, st);                        \
            else launch_rf_multi_grid<emb_interact_rf_kernel<CQ_, REM_, 1, EVS_RF_DEPTH>>(a, st);                            \
        } else {                                                                                                             \
            if (nt2) launch_rf_multi_grid<emb_interact_rf_kernel<CQ_, REM_, 2, EVS_RF_DEPTH, false, false, false, true>>(a, st); \
            else launch_rf_multi_grid<emb_interact_rf_kernel<CQ_, REM_, 1, EVS_RF_DEPTH, false, false, false, true>>(a, st);     \
        }                                                                                                                    \
    } while (0)
    switch (a.d) {
    case 16: EVS_RF_MULTI(1, 0); return true;
    case 32: EVS_RF_MULTI(2, 0); return true;
    case 36: EVS_RF_MULTI(2, 1); return true;
    case 64: EVS_RF_MULTI(4, 0); return true;
    default: return false;
    }
#undef EVS_RF_MULTI
}

// The plain launch (one index per bag declared) also takes batches ABOVE one resident generation for d = 36 and 16: with
// the round-3 head the one-chunk blocks beat the LDS-DMA loop there too (same box, d = 36: B = 32 768 36.2 -> 32.4 us,
// 65 536 62.1 -> 60.0, 131 072 120.0 -> 114.6, 262 144 235 -> 227; d = 16 at 65 536: 42.0 -> 38.5; d = 32 loses, 48.6 ->
// 50.6, and keeps the loop).  The checked / probing / row-id forms stay at one generation (no gain measured for the
// checked form: 65.6 vs 65.7 us at 65 536).  EVS_FUSED_RF_MAX_B, when set to a valid value, bounds every form.
static int64_t rf_max_batch_plain(int d) {
    const bool bounded = rf_max_batch_env() >= 0;   // (a refused value does not bound: it falls back to the unset behaviour)
    if (bounded || d == 32) return rf_max_batch();
    if (d == 64) return 1ll << 22;
    return 1ll << 22;
}

bool launch_rf(const FusedArgs &a, hipStream_t st) {
    if (!rf_mode() || a.F > kTileMaxF || a.bag1 != 1 || a.B > rf_max_batch_plain(a.d)) return false;
    if (rf_lean_shape(a) && launch_rf_lean(a, rf_tile_per(), st)) return true;   // the stacked call: scalar arguments + model descriptor
    const bool nt2 = a.F > 16;
    switch (a.d) {
    case 16:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<1, 0, 2, EVS_RF_DEPTH>>(a, st, rf_tile_per()); else launch_rf_grid<emb_interact_rf_kernel<1, 0, 1, EVS_RF_DEPTH>>(a, st, rf_tile_per());
        return true;
    case 32:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 0, 2, EVS_RF_DEPTH>>(a, st, rf_tile_per()); else launch_rf_grid<emb_interact_rf_kernel<2, 0, 1, EVS_RF_DEPTH>>(a, st, rf_tile_per());
        return true;
    case 36:
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<2, 1, 2, EVS_RF_DEPTH>>(a, st, rf_tile_per()); else launch_rf_grid<emb_interact_rf_kernel<2, 1, 1, EVS_RF_DEPTH>>(a, st, rf_tile_per());
        return true;
    case 64:   // 28 VGPRs per sample in flight (135 in all: three blocks per CU); EVS_FUSED_RF_D64=0: the LDS-DMA loop
        if (!rf_d64()) return false;
        if (nt2) launch_rf_grid<emb_interact_rf_kernel<4, 0, 2, EVS_RF_DEPTH>>(a, st, rf_tile_per()); else launch_rf_grid<emb_interact_rf_kernel<4, 0, 1, EVS_RF_DEPTH>>(a, st, rf_tile_per());
        return true;
    default:   // (d = 128 was built the same way -- CQ = 8, 14 loads per sample, 248 VGPRs, one or two blocks per CU -- and lost to the
               //  LDS-DMA loop: 57.5 vs 52.5 us at B = 16 384, 220 vs 182 us at 65 536; removed)
        return false;
    }
}


// ======================================================================================================================
// The fused launch as a RESIDENT DISPATCHER (round 6; evs_emb_interact_serve_*).  BASELINE's metric is "lookups/sec + p50 batch
// latency", and a launch that is waited for spends 12 of its 31 us (B = 16 384) outside the kernel: ~6 us of host time in the
// launch call, ~3 us until the command processor has dispatched 1 024 blocks, ~3 us until the completion signal is visible;
// below ~4 000 samples a launch IS that floor (7-8 us per batch whatever B).  Here the grid stays on the device and takes
// batches from a mailbox in pinned host memory (the reference's loop calls the pair once per batch: dlrm_s_pytorch.py:596-601,
// the inference loop :801-836):
//   request ring   (host -> device) kSrvSlots descriptors of 64 bytes: x, (T, B) indices, (T, B) offsets, R, B, strides, the block the
//                  batch's first chunk goes to; each 32-byte sector closed by the sequence number (written last: a sector is
//                  accepted only when its guard holds the number awaited, whatever granularity the bus delivers it in);
//   leader         block 0, one wavefront: polls the next FOUR ring slots as one 64-lane system-scope load, copies every
//                  descriptor that has arrived into device memory (agent-scope write-through stores) and publishes its number
//                  in kSrvReplicas replica lines (a thousand blocks polling ONE word cost more than the work: r04_atomic_probe);
//   workers        blocks 1 .. G-1: lane 0 polls its replica line; a new number -> an agent-scope acquire (inputs written by
//                  other launches), the descriptor, then rf_body<..., SERVE> for every chunk c of the batch with
//                  (first_block + c) % (G - 1) == this worker -- consecutive small batches land on different blocks and overlap;
//                  R leaves as agent-scope write-through stores (a resident kernel has no end-of-kernel release), every wave
//                  waits for its stores (vmcnt(0)), then ONE arrival atomic per block; the block that completes the batch
//                  writes the batch's number into the ANSWER ring in host memory, which the caller spins on;
//   leaving        the leader publishes "stop" after idle_ticks without a request (or when the host's control word says so):
//                  every block returns; the next post starts the grid again.  While it is resident the grid holds its CUs
//                  (G = 4 blocks per CU by default): kernels of other streams run when it has left.
// Same bits as the launch form (the same rf_body).  Rules for the caller: the inputs of a batch are complete when it is posted
// (post on the host after the producer's stream has been synchronised), and R may be read by anything started after evs_emb_interact_serve_wait has returned.
constexpr int kSrvSlots = 64;
constexpr int kSrvReplicas = 32;
#ifndef EVS_SRV_SUB
#define EVS_SRV_SUB 32
#endif
constexpr unsigned kSrvSub = EVS_SRV_SUB;         // sub-counters a batch's arrivals are spread over (a power of two; developer A/B: 128 -- a quarter of
                                                  // the arrivals per counter, but 128 answer words written by 128 blocks for the host to collect -- 31.2 us
                                                  // waited for at B = 16 384 against 26.0, 19.6 against 14.2 at B = 2 048; 8: 26.9 / 14.7)
constexpr unsigned kSrvAnsLine = kSrvSub;  // words per slot of the answer ring: one per sub-counter of the batch's arrivals
struct SrvDesc { unsigned w[16]; };   // w0-1 x, w2-3 idx, w4-5 off, w6 B, w7 seq | w8-9 R, w10 x_stride, w11 first block, w12 idx stride, w13 off stride, w14 -, w15 seq
struct SrvState {
    unsigned pub[kSrvReplicas][32];       // line r: word 0 = the last published sequence number, word 1 = the generation (launch number) of the grid that has LEFT behind it
    SrvDesc desc[kSrvSlots];              // the leader's copies of the descriptors
    // per slot: chunks finished (a thousand arrivals on ONE word serialise at the memory-side atomic unit: ~6 us,
    // r04_atomic_probe, and the blocks of a full batch all finish together): chunk c arrives at sub-counter c % 32 (a line each);
    // whoever completes sub-counter r writes the batch's number into word r of the slot's ANSWER line in host memory, and the
    // host takes the batch as answered when all of them hold it (the first form had a top counter the 32 completers arrived at:
    // one more dependent atomic round trip, ~1 us, in front of every answer)
    unsigned arrived[kSrvSlots][kSrvSub][32];
    unsigned prog[4096];                  // host-published front end: the last batch block b has looked at (kept across launches)
};
// HOST-PUBLISHED front end (round 6; parts whose device memory the host can address -- large BAR): the host writes a batch's
// descriptor straight into device memory through the PCIe aperture -- into its slot of a descriptor ring and into the first half
// of every replica line -- and every block's poll of its line is the whole way in: no leader reading the mailbox over the bus
// and republishing (tools/mailbox_probe.hip: post -> 32 pollers -> arrival counter -> answer 3.0 us; the leader's hop alone
// was ~3).  Fine-grained device memory (a poll of plain device memory is served by the polling XCD's L2 once the line is in it).
//   line r, words 0..15   the descriptor of the LATEST batch posted; its guards (words 7, 15) are its number    [host, through the aperture]
//           word 16       the launch number of a grid that is leaving                                           [the leader]
//   line 0, word 18       the host's request to leave                                                           [host]
// Nobody publishes "up to here" when the grid leaves -- the host posts whenever it likes, a block may have seen a batch the
// leader has not --: every block keeps ITS OWN count of batches looked at (SrvState::prog), stores it on its way out, and its
// successor in the next launch goes on from there; a batch is answered when every chunk has arrived, whichever launch ran it.
struct SrvFront {
    unsigned line[kSrvReplicas][32];
    SrvDesc desc[kSrvSlots];
};
struct SrvArgs {
    const FusedArgs *tmpl;                // tables, shapes (device memory; written before the grid starts, never while it runs)
    SrvState *st;
    SrvFront *front;                      // the host-published front end, or nullptr: the leader reads the mailbox in host memory
    volatile unsigned *req;               // request ring (device address of the mapped host block)
    volatile unsigned *ctl;               // word 0: stop
    volatile unsigned *ans;               // answer ring: kSrvSlots lines of kSrvAnsLine words (word r = the number of the batch whose sub-counter r is complete);
                                          // behind them the status line: word 0 = alive, word 1 = the last published number
    unsigned start_seq;                   // the last number published by an earlier run of the grid
    unsigned gen;                         // this launch's number (>= 1): "stop" is the leader writing it into word 1 of the replica lines --
                                          // what an earlier launch left there never matches, so nothing has to be cleared between launches
    long long idle_ticks;
};

// which block runs chunk c of a batch (the same rule on both sides).  A batch with fewer chunks than the grid has blocks goes to the
// WORKERS only (blocks 1 .. G-1, starting at the batch's `first`: consecutive small batches land on different blocks), so the
// leader stays at its mailbox; a batch with at least G chunks uses every block, the leader's too (at B = 16 384 = 1 024 chunks a
// grid of 1 024 blocks would otherwise hand one worker two chunks: the batch's tail)
__device__ __forceinline__ unsigned srv_block_of(unsigned c, unsigned n_chunks, unsigned first, unsigned G) {
    return n_chunks >= G ? (first + c) % G : 1u + (first + c) % (G - 1u);
}
// the chunks of one batch that fall to block `me`, then the arrival: every wave waits for its stores of R (written through),
// ONE atomic per block, and the block that completes the batch writes its number into the answer ring in host memory
// a batch whose chunks this block has run but not yet reported: the report (srv_arrive) waits until the block's stores of R are
// known to be complete -- which the worker learns for free from its NEXT poll (vector-memory operations complete in issue
// order: a load that has returned has every earlier store of its wave behind it), so the drain of a batch's stores runs under
// the poll for the next one instead of in front of it
struct SrvPending { unsigned k, c0, step, n_chunks; };
__device__ __forceinline__ void srv_arrive(const SrvArgs &sv, const SrvPending &p) {
    const unsigned slot = p.k % (unsigned)kSrvSlots, n_chunks = p.n_chunks;
    unsigned *ans = const_cast<unsigned *>(sv.ans) + slot * kSrvAnsLine;
    if (n_chunks == 1u) {             // (a batch of one chunk: nobody else to wait for)
        __hip_atomic_store(ans, p.k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    for (unsigned c = p.c0; c < n_chunks; c += p.step) {
        const unsigned r = c & (kSrvSub - 1u), expect = n_chunks / kSrvSub + (r < (n_chunks & (kSrvSub - 1u)) ? 1u : 0u);
        const unsigned before = __hip_atomic_fetch_add(&sv.st->arrived[slot][r][0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1u == expect) {
            __hip_atomic_store(&sv.st->arrived[slot][r][0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // back to zero for the slot's next use
            __hip_atomic_store(ans + r, p.k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// the chunks of one batch that fall to block `me`; -> true: it ran some (pend says which: report them with srv_arrive once the
// stores are known to be complete)
template <int CQ, int REM, int NT>
__device__ __forceinline__ bool srv_run_batch(const SrvArgs &sv, const FusedArgs &la, const unsigned (&w)[16], unsigned k, unsigned me, unsigned G, bool &first, SrvPending &pend) {
    RfServeDesc sd;
    sd.x = reinterpret_cast<const float *>((uintptr_t)(((unsigned long long)w[1] << 32) | w[0]));
    sd.idx = reinterpret_cast<const int64_t *>((uintptr_t)(((unsigned long long)w[3] << 32) | w[2]));
    sd.off = reinterpret_cast<const int64_t *>((uintptr_t)(((unsigned long long)w[5] << 32) | w[4]));
    sd.R = reinterpret_cast<float *>((uintptr_t)(((unsigned long long)w[9] << 32) | w[8]));
    sd.B = (int64_t)w[6]; sd.x_stride = (int64_t)w[10]; sd.idx_stride = (int64_t)w[12]; sd.off_stride = (int64_t)w[13];
    const unsigned n_chunks = (w[6] + 15u) >> 4;
    unsigned c0, step;
    if (n_chunks >= G) { c0 = (me + G - w[11] % G) % G; step = G; }
    else { if (me == 0u) return false; c0 = (me - 1u + (G - 1u) - w[11] % (G - 1u)) % (G - 1u); step = G - 1u; }
    unsigned mine = 0u;
    for (unsigned c = c0; c < n_chunks; c += step) {
        rf_body<CQ, REM, NT, EVS_RF_DEPTH, false, false, false, true, true>(la, sv.tmpl, sd, (int)c, first);
        first = false;
        mine++;
        __syncthreads();
    }
    pend.k = k; pend.c0 = c0; pend.step = step; pend.n_chunks = n_chunks;
    return mine != 0u;
}

template <int CQ, int REM, int NT>
__global__ void __launch_bounds__(256, (CQ >= 4 ? 2 : EVS_RF_LB)) emb_interact_rf_serve_kernel(const SrvArgs sv) {
    SrvState *st = sv.st;
    const int lane = threadIdx.x & 63;
    const unsigned G = gridDim.x, me = blockIdx.x;
    // the scalar fields of the template (constant address space: scalar loads; the template is not written while the grid runs)
    typedef const __attribute__((address_space(4))) FusedArgs *tmpl4_t;
    const tmpl4_t t4 = reinterpret_cast<tmpl4_t>(reinterpret_cast<uintptr_t>(sv.tmpl));
    FusedArgs la;
    la.F = t4->F; la.d = t4->d; la.itself = t4->itself; la.P = t4->P; la.err = t4->err; la.zeros = t4->zeros;
    la.dummy_i64 = t4->dummy_i64; la.dummy_f32 = t4->dummy_f32; la.tile_per = 16; la.multi_n = 0; la.multi_cpb = 0;
    la.multi_idx_stride = 0; la.multi_off_stride = 0; la.R = nullptr; la.B = 0; la.bag1 = 3;
    bool first = true;     // (block-uniform) this block has not run a chunk yet: the body's one read of the template
    // what the block's wave 0 brought back from its poll: [0..63] descriptor words (leader: up to four new batches; worker: its
    // replica line -- number, stop word, the descriptor of batch `number`), [64] = batches to look at, [65] = leave afterwards
    __shared__ unsigned s_line[66];
    const bool hostpub = sv.front != nullptr;      // (grid-uniform)
    const unsigned *my_line = hostpub ? &sv.front->line[me % (unsigned)kSrvReplicas][0] : &st->pub[me % (unsigned)kSrvReplicas][0];
    // the last batch this block has looked at (host-published lines: its own count, kept in device memory across launches)
    unsigned my = hostpub ? __hip_atomic_load(&st->prog[me & 4095u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : sv.start_seq;
    SrvPending pend{0u, 0u, 1u, 0u};
    bool have_pend = false;          // (block-uniform) chunks run, their stores possibly still on their way, not yet reported
    if (me == 0u && threadIdx.x == 0) __hip_atomic_store(const_cast<unsigned *>(sv.ans) + kSrvSlots * kSrvAnsLine, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // alive
    for (;;) {
        if (threadIdx.x < 64 && hostpub) {
            // ---------------- host-published lines: every block's wave 0 at its line (the leader's too) ----------------
            const long long t0 = (long long)wall_clock64();
            unsigned v = 0u, n_new = 0u;
            bool leave_now = false;
            for (;;) {
                v = __hip_atomic_load(my_line + (lane & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                const unsigned g7 = (unsigned)__builtin_amdgcn_readlane((int)v, 7), g15 = (unsigned)__builtin_amdgcn_readlane((int)v, 15);
                const unsigned gn = (unsigned)__builtin_amdgcn_readlane((int)v, 16);
                // the line's number: both guards (a line caught between its two halves' arrival shows nothing new yet)
                const unsigned sq = (g7 == g15 && (int)(g7 - my) > 0) ? g7 : my;
                if (sq != my) { n_new = sq - my; break; }
                if (have_pend) break;     // nothing new, but chunks to report: the load above has returned, so have this wave's stores
                if (gn == sv.gen) { leave_now = true; break; }       // the leader has gone (idle, or asked to): so does this block
                if (me == 0u) {
                    const unsigned stopreq = (unsigned)__builtin_amdgcn_readlane((int)v, 18);
                    if (stopreq != 0u || (long long)wall_clock64() - t0 > sv.idle_ticks) {
                        if (lane < kSrvReplicas) __hip_atomic_store(&sv.front->line[lane][16], sv.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                        leave_now = true;
                        break;
                    }
                }
                __builtin_amdgcn_s_sleep(1);
            }
            if (lane < 16) s_line[lane] = v;       // the latest descriptor (the look below checks whose it is)
            if (lane == 0) { s_line[64] = n_new; s_line[65] = leave_now ? 1u : 0u; }
        } else if (threadIdx.x < 64) {
            if (me == 0u) {
                // ---------------- the leader: wave 0 at the mailbox ----------------
                const long long t0 = (long long)wall_clock64();
                int n_new = 0;
                unsigned word = 0u;
                bool pend_only = false;
                for (;;) {
                    // the next four ring slots in one load: lane = 16 * (slot in the group) + word
                    const unsigned slot0 = (my + 1u) % (unsigned)kSrvSlots;
                    const unsigned sl = (slot0 + (unsigned)(lane >> 4)) % (unsigned)kSrvSlots;
                    word = __hip_atomic_load(const_cast<unsigned *>(sv.req) + sl * 16u + (unsigned)(lane & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    // (the control word asked for WITH the ring, not behind it: it was a second round trip over the bus per poll)
                    const unsigned stop = __hip_atomic_load(const_cast<unsigned *>(sv.ctl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    // group g holds descriptor my + 1 + g when both its guards say so
                    const unsigned want = my + 1u + (unsigned)(lane >> 4);
                    const unsigned long long gm = __ballot(((lane & 7) == 7) && word == want);   // lanes 7, 15 of every group
#pragma unroll
                    for (int g = 0; g < 4; g++) {
                        const bool okg = ((gm >> (16 * g + 7)) & 1ull) && ((gm >> (16 * g + 15)) & 1ull);
                        if (okg && n_new == g) n_new = g + 1;    // consecutive ones only
                    }
                    if (n_new > 0) {
                        // the descriptors into the ring in device memory (what a worker reads when a poll brought it more than one
                        // new number), the LAST of them into every replica line behind the line's number (a worker's poll brings the
                        // descriptor with the number: one round trip less per batch) -- all without a wait in between: a reader checks
                        // the guards of what it reads against the number it is after (older: not there yet, read again)
                        if ((lane >> 4) < n_new) __hip_atomic_store(&st->desc[sl].w[lane & 15], word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        const unsigned wl = (unsigned)__shfl((int)word, 16 * (n_new - 1) + (lane & 15));
#pragma unroll 4
                        for (int r = 0; r < kSrvReplicas; r += 4)
                            __hip_atomic_store(&st->pub[r + (lane >> 4)][2 + (lane & 15)], wl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (lane < kSrvReplicas) __hip_atomic_store(&st->pub[lane][0], my + (unsigned)n_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        break;
                    }
                    if (have_pend) { pend_only = true; break; }   // nothing new, but chunks to report: the load above has returned, so have this wave's stores
                    if (stop != 0u || (long long)wall_clock64() - t0 > sv.idle_ticks) break;
                    __builtin_amdgcn_s_sleep(2);
                }
                s_line[lane] = word;
                if (lane == 0) { s_line[64] = (unsigned)n_new; s_line[65] = (n_new == 0 && !pend_only) ? 1u : 0u; }
            } else {
                // ---------------- a worker: the whole replica line in one 32-lane load ----------------
                unsigned v, sq, gn;
                for (;;) {
                    v = __hip_atomic_load(my_line + (lane & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    sq = (unsigned)__builtin_amdgcn_readlane((int)v, 0); gn = (unsigned)__builtin_amdgcn_readlane((int)v, 1);   // (not __shfl: that is the LDS crossbar)
                    if (sq != my || gn == sv.gen) break;
                    if (have_pend) break;     // nothing new, but chunks to report: the load above has returned, so have this wave's stores
                    __builtin_amdgcn_s_sleep((EVS_X_SRV & 4) ? 16 : 1);
                }
                if (lane >= 2 && lane < 18) s_line[lane - 2] = v;
                if (lane == 0) { s_line[64] = sq - my; s_line[65] = gn == sv.gen ? 1u : 0u; }
            }
        }
        // (waves 1..3: nothing to poll for, their stores of the batch before drain meanwhile; wave 0's poll has returned: so have its stores)
        if (have_pend && threadIdx.x >= 64) __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        if (have_pend) { if (threadIdx.x == 0) srv_arrive(sv, pend); have_pend = false; }
        const unsigned n_look = s_line[64], leave = s_line[65];
        for (unsigned g = 0; g < n_look; g++) {
            const unsigned k = my + 1u + g;
            unsigned w[16];
            bool have;
            if ((me == 0u && !hostpub) || g + 1u == n_look) {     // the leader's own copies / the descriptor that came with the line
#pragma unroll
                for (int i = 0; i < 16; i++) w[i] = (unsigned)__builtin_amdgcn_readfirstlane((int)s_line[((me == 0u && !hostpub) ? 16 * g : 0) + i]);
                have = w[7] == k && w[15] == k;
            } else have = false;
            if (!have && (me != 0u || hostpub)) {
                // an earlier batch of a burst (or a line caught between its words and its number): the ring in device memory.  Its
                // guards say which batch the slot holds: k -- take it (both guards); an OLDER number -- the leader's copy is still on its way: read again; a LATER one -- this worker
                // lags, batch k completed without it and the ring has come round: k owed it nothing (a batch is only answered,
                // and its slot only reused, when every chunk of it has arrived).
                const unsigned *dw = hostpub ? sv.front->desc[k % (unsigned)kSrvSlots].w : st->desc[k % (unsigned)kSrvSlots].w;
                for (int tries = 0; tries < (1 << 20); tries++) {
                    // ONE load instruction for the sixteen words (lane = word): a 32-byte sector -- seven words and the guard behind
                    // them -- is sampled at one time, so a guard that holds k vouches for the words in front of it (sixteen separate
                    // loads could take words 0..6 before a write lands and the guard after it)
                    const unsigned dv = hostpub ? __hip_atomic_load(dw + (lane & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                                : __hip_atomic_load(dw + (lane & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                    for (int i = 0; i < 16; i++) w[i] = (unsigned)__builtin_amdgcn_readlane((int)dv, i);
                    if (w[7] == k && w[15] == k) { have = true; break; }     // (the leader writes a descriptor as ONE 64-byte store)
                    if ((int)(w[7] - k) > 0 || (int)(w[15] - k) > 0) break;    // overwritten by a later batch
                }
            }
            if (have) {
                if (have_pend) {   // a second batch inside one look: the first one's stores are waited for in place (rare: a burst)
                    __builtin_amdgcn_s_waitcnt(0x0F70);
                    __syncthreads();
                    if (threadIdx.x == 0) srv_arrive(sv, pend);
                    have_pend = false;
                }
                have_pend = srv_run_batch<CQ, REM, NT>(sv, la, w, k, me, G, first, pend);
            }
        }
        my += n_look;
        __syncthreads();
        if (leave) break;
    }
    if (have_pend) {
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        if (threadIdx.x == 0) srv_arrive(sv, pend);
    }
    if (hostpub && threadIdx.x == 0) __hip_atomic_store(&st->prog[me & 4095u], my, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (me == 0u) {
        // leaving: every worker sees the stop word behind the last number; the host learns how far the grid got
        if (!hostpub && threadIdx.x < kSrvReplicas) __hip_atomic_store(&st->pub[threadIdx.x][1], sv.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (threadIdx.x == 0) {
            __hip_atomic_store(const_cast<unsigned *>(sv.ans) + kSrvSlots * kSrvAnsLine + 1, my, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(const_cast<unsigned *>(sv.ans) + kSrvSlots * kSrvAnsLine, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

}  // namespace evs

extern "C" int evs_mlp1_kernels_seen(char *buf, int n) {
    constexpr int kD[3] = {16, 32, 36};
    int len = 0;
    if (buf && n > 0) buf[0] = 0;
    for (int id = 0; id < evs::kMlp1Count; id++) {
        char line[64];
        const int k = snprintf(line, sizeof line, "mlp1_d%d_nt%d=%lld\n", kD[id / 2], (id & 1) + 1, evs::g_mlp1_seen[id].load(std::memory_order_relaxed));
        if (buf && len + k < n) memcpy(buf + len, line, (size_t)k + 1);
        len += k;
    }
    return len;
}

struct evs_rf_server {
    evs::FusedArgs tmpl{};
    evs::FusedArgs *tmpl_dev = nullptr;
    evs::SrvState *st_dev = nullptr;
    evs::SrvFront *front = nullptr;  // host-published front end: fine-grained device memory the host writes through the aperture (same address on both sides), or nullptr
    unsigned *mbox = nullptr, *mbox_dev = nullptr;   // host block: request ring | control line | answer ring + status line
    hipStream_t stream = nullptr;
    unsigned posted = 0;            // the last sequence number posted
    unsigned gen = 0;               // launches of the grid so far
    unsigned next_first = 0;        // the worker the next batch's first chunk goes to
    unsigned slot_words[evs::kSrvSlots] = {};   // answer words the slot's batch in flight is answered through (min(chunks, 32))
    int n_blocks = 0, T = 0, d = 0;
    long long idle_ticks = 0;
    bool nt2 = false;
};
namespace {
constexpr size_t kSrvReqWords = (size_t)evs::kSrvSlots * 16, kSrvCtlWords = 32, kSrvAnsWords = (size_t)evs::kSrvSlots * evs::kSrvAnsLine + 16;
constexpr size_t kSrvStatus = (size_t)evs::kSrvSlots * evs::kSrvAnsLine;   // the status line behind the answer ring
// batch k of ring slot `slot` has been answered: every sub-counter's completer has written its number
inline bool srv_answered(evs_rf_server *s, unsigned slot, unsigned k) {
    volatile unsigned *a = s->mbox + kSrvReqWords + kSrvCtlWords + (size_t)slot * evs::kSrvAnsLine;
    const unsigned n = s->slot_words[slot] ? s->slot_words[slot] : 1u;
    for (unsigned r = 0; r < n; r++) if (a[r] != k) return false;
    return true;
}
inline volatile unsigned *srv_req(evs_rf_server *s) { return s->mbox; }
inline volatile unsigned *srv_ctl(evs_rf_server *s) { return s->mbox + kSrvReqWords; }
inline volatile unsigned *srv_ans(evs_rf_server *s) { return s->mbox + kSrvReqWords + kSrvCtlWords; }
void srv_launch(evs_rf_server *s) {
    using namespace evs;
    SrvArgs a;
    a.tmpl = s->tmpl_dev; a.st = s->st_dev; a.front = s->front;
    a.req = s->mbox_dev; a.ctl = s->mbox_dev + kSrvReqWords; a.ans = s->mbox_dev + kSrvReqWords + kSrvCtlWords;
    a.start_seq = srv_ans(s)[kSrvStatus + 1];   // how far the last run got (0 at first)
    a.idle_ticks = s->idle_ticks;
    a.gen = ++s->gen;
    const dim3 grid((unsigned)s->n_blocks), block(256);
    const bool nt2 = s->nt2;
    switch (s->d) {
    case 16: if (nt2) hipLaunchKernelGGL((emb_interact_rf_serve_kernel<1, 0, 2>), grid, block, 0, s->stream, a); else hipLaunchKernelGGL((emb_interact_rf_serve_kernel<1, 0, 1>), grid, block, 0, s->stream, a); break;
    case 32: if (nt2) hipLaunchKernelGGL((emb_interact_rf_serve_kernel<2, 0, 2>), grid, block, 0, s->stream, a); else hipLaunchKernelGGL((emb_interact_rf_serve_kernel<2, 0, 1>), grid, block, 0, s->stream, a); break;
    case 36: if (nt2) hipLaunchKernelGGL((emb_interact_rf_serve_kernel<2, 1, 2>), grid, block, 0, s->stream, a); else hipLaunchKernelGGL((emb_interact_rf_serve_kernel<2, 1, 1>), grid, block, 0, s->stream, a); break;
    default: if (nt2) hipLaunchKernelGGL((emb_interact_rf_serve_kernel<4, 0, 2>), grid, block, 0, s->stream, a); else hipLaunchKernelGGL((emb_interact_rf_serve_kernel<4, 0, 1>), grid, block, 0, s->stream, a); break;
    }
}
// Can this process STORE to p?  The attribute says the part has a large BAR; whether this allocation is mapped writable here is
// asked of the kernel, not found out by a fault: read(2) from /dev/zero INTO p copies four zero bytes to it, or fails with
// EFAULT -- no signal either way (the block has just been zeroed: nothing changes).
bool host_can_store(void *p) {
    const int fd = open("/dev/zero", O_RDONLY);
    if (fd < 0) return false;
    const ssize_t n = read(fd, p, 4);
    (void)close(fd);
    return n == 4;
}
// send the grid home (it leaves by itself when idle) and wait until it has gone
int srv_pause(evs_rf_server *s) {
    if (!s->stream) return EVS_OK;
    if (hipStreamQuery(s->stream) == hipSuccess) return EVS_OK;
    (void)hipGetLastError();
    // (the host-published front end: the request is a word of line 0, written through the aperture and never read back)
    volatile unsigned *stop = s->front ? reinterpret_cast<volatile unsigned *>(&s->front->line[0][18]) : srv_ctl(s);
    *stop = 1u;
    __builtin_ia32_sfence();
    const hipError_t e = hipStreamSynchronize(s->stream);
    *stop = 0u;
    __builtin_ia32_sfence();
    return e == hipSuccess ? EVS_OK : EVS_EHIP;
}
}  // namespace

extern "C" int evs_emb_interact_serve_start(evs_rf_server **out, int T, int d, const void *const *tables, const int64_t *n_rows,
                                            int itself, int n_blocks, int64_t idle_us) {
    using namespace evs;
    EVS_REQUIRE(out && tables && n_rows, "evs_emb_interact_serve_start: NULL argument");
    EVS_REQUIRE(T >= 1 && T + 1 <= kTileMaxF, "evs_emb_interact_serve_start: T=%d (the rows-in-registers kernel takes x + at most %d tables)", T, kTileMaxF - 1);
    EVS_REQUIRE(d == 16 || d == 32 || d == 36 || d == 64, "evs_emb_interact_serve_start: d=%d (16, 32, 36 or 64; fp32 tables)", d);
    EVS_REQUIRE(idle_us >= 1 && n_blocks >= 0, "evs_emb_interact_serve_start: bad argument");
    for (int t = 0; t < T; t++)
        EVS_REQUIRE(n_rows[t] >= 0 && n_rows[t] < (1ll << 31) && (n_rows[t] == 0 || (tables[t] && reinterpret_cast<uintptr_t>(tables[t]) % 16 == 0)),
                    "evs_emb_interact_serve_start: table %d (16-byte aligned, fewer than 2^31 rows)", t);
    evs_rf_server *s = new evs_rf_server();
    s->T = T; s->d = d; s->nt2 = T + 1 > 16;
    const int per_cu = d == 64 ? 2 : EVS_RF_LB;
    s->n_blocks = n_blocks > 0 ? n_blocks : kNumCu * per_cu;
    if (s->n_blocks < 2) s->n_blocks = 2;
    s->idle_ticks = idle_us * 100;   // wall_clock64(): 100 MHz
    FusedArgs &a = s->tmpl;
    const int F = T + 1;
    for (int f = 0; f < EVS_MAX_FEATURES; f++) {
        a.src[f] = nullptr; a.stride[f] = 0; a.indices[f] = nullptr; a.offsets[f] = nullptr; a.nnz[f] = 0;
        a.n_rows[f] = 0; a.row_w[f] = nullptr; a.off_len[f] = 0;
    }
    a.zeros = zero_page();
    a.err = index_error_flag();
    if (!a.zeros || !a.err) { delete s; return EVS_EHIP; }
    const int64_t *any_i64 = reinterpret_cast<const int64_t *>(a.zeros);
    for (int t = 0; t < T; t++) {
        a.src[t + 1] = n_rows[t] == 0 ? a.zeros : tables[t];
        a.indices[t + 1] = any_i64;       // (non-NULL marks a table: the kernel reads the descriptor's arrays)
        a.offsets[t + 1] = any_i64;
        a.n_rows[t + 1] = n_rows[t];
    }
    a.src[0] = a.zeros;
    a.B = 0; a.F = F; a.d = d; a.itself = itself ? 1 : 0; a.P = itself ? F * (F + 1) / 2 : F * (F - 1) / 2;
    a.dummy_i64 = any_i64; a.dummy_f32 = reinterpret_cast<const float *>(a.zeros); a.bag1 = 3; a.enc_lds = 0; a.opt_flag = nullptr; a.opt_id = 0;
    a.tile_per = 16; a.row_ids = nullptr; a.arena = nullptr; a.w1p = nullptr; a.b1 = nullptr; a.z1 = nullptr; a.n1 = 0; a.kp = 0; a.relu = 0; a.write_r = 1;
    a.zero_codes = nullptr; a.multi_n = 0; a.multi_cpb = 0; a.multi_idx_stride = 0; a.multi_off_stride = 0; a.R = nullptr;
    auto fail = [&](int rc) { (void)evs_emb_interact_serve_destroy(s); return rc; };
    if (hipMalloc(reinterpret_cast<void **>(&s->tmpl_dev), sizeof(FusedArgs)) != hipSuccess) return fail(EVS_ENOMEM);
    if (hipMalloc(reinterpret_cast<void **>(&s->st_dev), sizeof(SrvState)) != hipSuccess) return fail(EVS_ENOMEM);
    if (hipMemcpy(s->tmpl_dev, &a, sizeof(FusedArgs), hipMemcpyHostToDevice) != hipSuccess) return fail(EVS_EHIP);
    if (hipMemset(s->st_dev, 0, sizeof(SrvState)) != hipSuccess) return fail(EVS_EHIP);
    {   // The host-published front end where the host can address device memory (EVS_SERVE_PUBLISH=leader keeps the leader's
        // mailbox: developer A/B, and what parts without a large BAR run)
        const char *how = evs::env_switch("EVS_SERVE_PUBLISH");
        int dev_id = 0, large_bar = 0;
        if (!(how && !strcmp(how, "leader")) && s->n_blocks <= 4096 && hipGetDevice(&dev_id) == hipSuccess &&
            hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, dev_id) == hipSuccess && large_bar) {
            void *p = nullptr;
            if (hipExtMallocWithFlags(&p, sizeof(SrvFront), hipDeviceMallocFinegrained) == hipSuccess && hipMemset(p, 0, sizeof(SrvFront)) == hipSuccess &&
                hipDeviceSynchronize() == hipSuccess && host_can_store(p))
                s->front = reinterpret_cast<SrvFront *>(p);
            else { if (p) (void)hipFree(p); (void)hipGetLastError(); }
        } else (void)hipGetLastError();
    }
    const size_t words = kSrvReqWords + kSrvCtlWords + kSrvAnsWords;
    if (hipHostMalloc(reinterpret_cast<void **>(&s->mbox), words * 4, hipHostMallocMapped) != hipSuccess) return fail(EVS_ENOMEM);
    memset(s->mbox, 0, words * 4);
    if (hipHostGetDevicePointer(reinterpret_cast<void **>(&s->mbox_dev), s->mbox, 0) != hipSuccess) return fail(EVS_EHIP);
    int prio_lo = 0, prio_hi = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) return fail(EVS_EHIP);
    if (hipStreamCreateWithPriority(&s->stream, hipStreamNonBlocking, prio_hi) != hipSuccess) return fail(EVS_EHIP);
    if (hipDeviceSynchronize() != hipSuccess) return fail(EVS_EHIP);   // (the template and the state are in place before the grid's first read)
    *out = s;
    return EVS_OK;
}

// Post one batch: R = interact_features(x, apply_emb(lS_o, lS_i, tables)), lS_o given and checked per 16-sample block exactly as
// evs_emb_interact_dot_stacked does.  Returns at once; *ticket names the batch for evs_emb_interact_serve_wait.
extern "C" int evs_emb_interact_serve_post(evs_rf_server *s, int64_t B, const float *x, int64_t x_stride, const int64_t *indices_base,
                                           int64_t indices_row_stride, const int64_t *offsets_base, int64_t offsets_row_stride,
                                           float *R, uint64_t *ticket) {
    using namespace evs;
    EVS_REQUIRE(s && x && indices_base && offsets_base && R && ticket, "evs_emb_interact_serve_post: NULL argument");
    EVS_REQUIRE(B >= 1 && B < (1ll << 31), "evs_emb_interact_serve_post: B=%lld", (long long)B);
    EVS_REQUIRE(x_stride >= 0 && x_stride % 4 == 0 && x_stride < (1ll << 31) && reinterpret_cast<uintptr_t>(x) % 16 == 0,
                "evs_emb_interact_serve_post: x must be 16-byte aligned with a row stride that is a multiple of 4 floats");
    EVS_REQUIRE(indices_row_stride >= 0 && indices_row_stride < (1ll << 31) && offsets_row_stride >= 0 && offsets_row_stride < (1ll << 31),
                "evs_emb_interact_serve_post: row strides of the (T, B) arrays must fit 31 bits");
    const unsigned k = s->posted + 1u;
    const unsigned slot = k % (unsigned)kSrvSlots;
    volatile unsigned *ans = srv_ans(s), *req = srv_req(s) + (size_t)slot * 16;
    // the ring holds kSrvSlots batches in flight: the slot's previous user (k - kSrvSlots) must have been answered
    if (k > (unsigned)kSrvSlots) {
        const unsigned prev = k - (unsigned)kSrvSlots;
        uint64_t t = prev;
        if (!srv_answered(s, slot, prev)) { const int rc = evs_emb_interact_serve_wait(s, t); if (rc) return rc; }
    }
    {   const uint64_t n_chunks = (uint64_t)((B + 15) / 16);
        s->slot_words[slot] = (unsigned)(n_chunks < kSrvSub ? n_chunks : kSrvSub); }
    const unsigned long long px = (unsigned long long)reinterpret_cast<uintptr_t>(x), pi = (unsigned long long)reinterpret_cast<uintptr_t>(indices_base),
                             po = (unsigned long long)reinterpret_cast<uintptr_t>(offsets_base), pr = (unsigned long long)reinterpret_cast<uintptr_t>(R);
    if (s->front) {
        // host-published: the descriptor into its ring slot in DEVICE memory, then into the first half of every replica line --
        // 64-byte lines written whole through the write-combining aperture (one bus write each), a store fence between the ring
        // and the lines (a block that finds a number in its line reads the ring for the batches before it), nothing read back
        const unsigned dsc[16] = {(unsigned)px, (unsigned)(px >> 32), (unsigned)pi, (unsigned)(pi >> 32), (unsigned)po, (unsigned)(po >> 32), (unsigned)B, k,
                                  (unsigned)pr, (unsigned)(pr >> 32), (unsigned)x_stride, s->next_first, (unsigned)indices_row_stride, (unsigned)offsets_row_stride, 0u, k};
        volatile unsigned *ring = reinterpret_cast<volatile unsigned *>(s->front->desc[slot].w);
        for (int i = 0; i < 16; i++) ring[i] = dsc[i];
        __builtin_ia32_sfence();
        for (int r = 0; r < kSrvReplicas; r++) {
            volatile unsigned *l = reinterpret_cast<volatile unsigned *>(s->front->line[r]);
            for (int i = 0; i < 16; i++) l[i] = dsc[i];
        }
        __builtin_ia32_sfence();
    } else {
    req[0] = (unsigned)px; req[1] = (unsigned)(px >> 32); req[2] = (unsigned)pi; req[3] = (unsigned)(pi >> 32);
    req[4] = (unsigned)po; req[5] = (unsigned)(po >> 32); req[6] = (unsigned)B;
    req[8] = (unsigned)pr; req[9] = (unsigned)(pr >> 32); req[10] = (unsigned)x_stride; req[11] = s->next_first;
    req[12] = (unsigned)indices_row_stride; req[13] = (unsigned)offsets_row_stride; req[14] = 0u;
    __atomic_thread_fence(__ATOMIC_RELEASE);
    req[7] = k; req[15] = k;
    __atomic_thread_fence(__ATOMIC_SEQ_CST);
    }
    s->posted = k;
    s->next_first = (unsigned)(((uint64_t)s->next_first + (uint64_t)((B + 15) / 16)) % (uint64_t)(1u << 30));
    *ticket = k;
    if (ans[kSrvStatus] == 0u) {   // nobody there (never started, or gone home idle): start the grid
        const hipError_t q = hipStreamQuery(s->stream);
        if (q == hipSuccess) { srv_launch(s); if (hipGetLastError() != hipSuccess) { set_error("evs_emb_interact_serve_post: the grid could not be started"); return EVS_EHIP; } }
        else if (q != hipErrorNotReady) { (void)hipGetLastError(); return EVS_EHIP; }
        else (void)hipGetLastError();
    }
    return EVS_OK;
}

// Spin until batch `ticket` has been answered (R complete: anything started afterwards may read it)
extern "C" int evs_emb_interact_serve_wait(evs_rf_server *s, uint64_t ticket) {
    using namespace evs;
    EVS_REQUIRE(s && ticket >= 1 && ticket <= s->posted, "evs_emb_interact_serve_wait: no such batch");
    // (only the last kSrvSlots batches have an answer word of their own: an older one was answered when its slot was re-posted)
    if ((uint64_t)s->posted - ticket >= (uint64_t)kSrvSlots) return EVS_OK;
    volatile unsigned *ans = srv_ans(s);
    const unsigned slot = (unsigned)(ticket % (unsigned)kSrvSlots);
    long long spins = 0;
    while (!srv_answered(s, slot, (unsigned)ticket)) {
        if ((++spins & 255) == 0 && ans[kSrvStatus] == 0u) {   // the grid has left (idle) with this batch still in the ring: start it again
            const hipError_t q = hipStreamQuery(s->stream);
            if (q == hipSuccess) { if (srv_answered(s, slot, (unsigned)ticket)) break; srv_launch(s); if (hipGetLastError() != hipSuccess) return EVS_EHIP; }
            else if (q != hipErrorNotReady) { (void)hipGetLastError(); return EVS_EHIP; }
            else (void)hipGetLastError();
        }
        if (spins > (1ll << 31)) { (void)srv_pause(s); set_error("evs_emb_interact_serve_wait: the grid did not answer"); return EVS_EHIP; }
        __builtin_ia32_pause();
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return EVS_OK;
}

// 1: the host publishes descriptors through the PCIe aperture (large BAR); 0: the leader reads a mailbox in host memory
extern "C" int evs_emb_interact_serve_mode(evs_rf_server *s) { return s && s->front ? 1 : 0; }

extern "C" int evs_emb_interact_serve_stop(evs_rf_server *s) {
    EVS_REQUIRE(s, "evs_emb_interact_serve_stop: NULL server");
    if (s->posted) { const int rc = evs_emb_interact_serve_wait(s, s->posted); if (rc) return rc; }
    return srv_pause(s);
}

extern "C" int evs_emb_interact_serve_destroy(evs_rf_server *s) {
    if (!s) return EVS_OK;
    if (s->mbox && s->stream) (void)srv_pause(s);
    if (s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
    if (s->mbox) (void)hipHostFree(s->mbox);
    if (s->tmpl_dev) (void)hipFree(s->tmpl_dev);
    if (s->st_dev) (void)hipFree(s->st_dev);
    if (s->front) (void)hipFree(s->front);
    delete s;
    return EVS_OK;
}

#ifdef EVS_X_PT
extern "C" __attribute__((visibility("default"))) int evs_x_pt(unsigned long long *out, int reset) {   // out: 16 (summed over the blocks)
    static unsigned long long h[1024 * 16], z[1024 * 16];
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(evs::g_pt), sizeof h) != hipSuccess) return -2;
    if (evs::rf_lean_pt_add(h, reset) != 0) return -4;   // (the lean entries keep their own table: evs_fused_rf_lean.hip)
    if (out) for (int k = 0; k < 16; k++) { out[k] = 0; for (int b = 0; b < 1024; b++) out[k] += h[b * 16 + k]; }
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(evs::g_pt), z, sizeof z) != hipSuccess) return -3;
    return 0;
}
#endif
#ifdef EVS_X_LOG
// developer tool (tools/dbg_inline.py): the event log of the folded update -- (type, word address, old word, new word)
extern "C" __attribute__((visibility("default"))) long long evs_x_log_fetch(unsigned long long *out, long long max_events, int reset) {
    unsigned n = 0;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(evs::g_xlog_n), 4) != hipSuccess) return -2;
    long long m = n < (1u << 18) ? n : (1u << 18);
    if (m > max_events) m = max_events;
    if (out && m && hipMemcpyFromSymbol(out, HIP_SYMBOL(evs::g_xlog), (size_t)m * 32) != hipSuccess) return -3;
    if (reset) { n = 0; if (hipMemcpyToSymbol(HIP_SYMBOL(evs::g_xlog_n), &n, 4) != hipSuccess) return -4; }
    return m;
}
#endif
