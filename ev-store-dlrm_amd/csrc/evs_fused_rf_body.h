// The body of the rows-in-registers fused kernel (see evs_fused_rf.hip for what it computes and how): shared by the
// translation units that hold its __global__ entries (evs_fused_rf.hip, evs_fused_rf_lean.hip).
#pragma once
#include "evs_fused.h"

namespace evs {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) f32x4 *gf4_t;

#ifndef EVS_RF_DEPTH
#define EVS_RF_DEPTH 4
#endif
#ifndef EVS_RF_LB
#define EVS_RF_LB 4
#endif
#ifndef EVS_OUT_CPOL
#define EVS_OUT_CPOL 2   // nt: R is written once and streams out (see evs_fused.hip)
#endif

// MLP: the first top-MLP layer (dlrm_s_pytorch.py:601-605: p = apply_mlp(z, top_l); its first nn.Linear + ReLU) fused
// behind the interaction.  The 16 output rows of the block's chunk stay in LDS (s_R, zero-padded to kp columns) and are
// the A operand (M = 16 samples) of Z1 = act(R W1^T + b1): 16 x 16 output tiles, one v_mfma_f32_16x16x4_f32 chain of
// kp / 4 steps each, the four waves taking the n1 / 16 tiles in turn; W1 arrives zero-padded and row-aligned (w1p) and
// is read straight from L2 (the whole 0.8 MB matrix is re-read per 16 samples: 0.8 GB of L2 traffic at B = 16 384, and
// 100 MFMAs per tile -- with the layer the kernel is matrix-core-bound, not HBM-bound).  k-slot q of the MFMA owns the
// contiguous columns [q * kp/4, (q+1) * kp/4) of both operands, so they are read as 16-byte pieces.  R itself is
// written only when asked for.
constexpr int kMlpRowStride = 452;   // floats per staged row: kp <= 448 (F <= 28, d <= 36, diagonal kept) + 4 (bank spread)

// IDS: the cache tier's consumer -- features 1..F-1 come as one (B, F-1) int32 table of row ids (FusedArgs::row_ids): bit 30
// says "row of the cache arena", else the row of the feature's own table; 4 bytes per key instead of an 8-byte address,
// and the rows travel exactly as in the plain launch.
// PROBE (implies IDS): the kernel reads the REQUEST rows and probes the cache's hash itself in its head -- what
// cache_batch_probe_gather_kernel does as a launch of its own (hash probe, agg_hit per request, priority bump, hit flags,
// the block's miss list for the update kernel, hit statistics) -- and goes on with the ids it found.
// CHECK (lS_o given, whole batches: nnz == B, B or B + 1 offsets -- what the reference's loop passes): the block also loads
// the offsets of its 16 samples and checks that every bag is exactly {idx[b]} (offsets[b] == b and the bag ends at b + 1:
// the neighbour lane's offset, one extra load behind the block's last sample).  A block that finds anything else pools ITS
// samples in a slow loop straight from global memory (general semantics: empty bags, several indices summed in index
// order, bad offsets / indices skipped and flagged -- the arithmetic of evs_fused.hip's general loop) and feeds the same
// MFMA + output code: no flag, no second launch, as in the index-tile loop of evs_fused.hip and in evs_fused_rfq.hip.
// SERVE (round 6; evs_emb_interact_serve_*): the same body run by a RESIDENT grid, once per (descriptor, chunk) -- what varies
// from batch to batch (x, the (T, B) index / offsets arrays, R, B) comes from the descriptor `sd`, everything else (tables,
// shapes) from a FusedArgs the server keeps in device memory (`ka` points at it, `args` is a copy of its scalar fields); R is
// stored with agent-scope write-through stores (sc1): a resident kernel has no end-of-kernel release that would write its L2
// back for the launches (on other XCDs) that read R afterwards.
// what a RESIDENT grid reads of a batch's inputs (indices, offsets, x) goes through agent-scope loads: the grid never passes a
// kernel boundary, so nothing invalidates its L1 / L2 between two batches that reuse the same addresses (an acquire fence per
// descriptor does -- buffer_inv sc1 by a thousand blocks: measured, +27 us per batch)
template <bool COHERENT>
__device__ __forceinline__ int64_t rf_ld_i64(const int64_t *p) {
    typedef const __attribute__((address_space(1))) int64_t *g_t;
    if constexpr (COHERENT) return __hip_atomic_load(reinterpret_cast<g_t>(reinterpret_cast<uintptr_t>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *reinterpret_cast<g_t>(reinterpret_cast<uintptr_t>(p));
}
template <bool COHERENT>
__device__ __forceinline__ float rf_ld_f32(const float *p) {
    typedef const __attribute__((address_space(1))) float *g_t;
    if constexpr (COHERENT) return __hip_atomic_load(reinterpret_cast<g_t>(reinterpret_cast<uintptr_t>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *reinterpret_cast<g_t>(reinterpret_cast<uintptr_t>(p));
}
struct RfServeDesc {
    const float *x; const int64_t *idx; const int64_t *off; float *R;
    int64_t B, x_stride, idx_stride, off_stride;
};
// LEAN (round 7; evs_fused_rf_lean.hip): the stacked call's entry whose kernel arguments are a handful of scalars -- what the
// body reads of `args` is filled from them in registers, and what the launch form reads per feature out of the kernel-argument
// segment (table addresses, row counts) comes from a per-model descriptor that lives in device memory (RfModelDesc,
// evs_fused.h): lines no host write has touched since the model was first used.  `ka` is not read.
struct RfLeanX {
    const RfModelDesc *md; const float *x; int x_stride;
};
#ifndef EVS_PT_TABLE
#define EVS_PT_TABLE g_pt   // (one table per translation unit that holds entries of this body)
#endif
#ifdef EVS_X_PT   // developer instrumentation (tools/probe_stage_probe.py): per block, 100 MHz ticks from the block's entry to stage k, summed over launches
__device__ unsigned long long EVS_PT_TABLE[1024][16];     // (a row per block: launches do not overlap, a block adds to its own words)
#define EVS_PT(k) do { if (threadIdx.x == 0) EVS_PT_TABLE[blockIdx.x & 1023][k] += (unsigned long long)((long long)wall_clock64() - pt_t0); } while (0)
#define EVS_PTW(k) do { __builtin_amdgcn_s_waitcnt(0x0F70); EVS_PT(k); } while (0)     // behind everything this wave has asked for
#else
#define EVS_PT(k) do { } while (0)
#define EVS_PTW(k) do { } while (0)
#endif
template <int CQ, int REM, int NT, int D, bool MLP, bool IDS, bool PROBE, bool CHECK, bool SERVE, bool LEAN = false>
__device__ __forceinline__ void rf_body(const FusedArgs &args, const FusedArgs *ka, const RfServeDesc &sd, const int blk_in, const bool srv_first = false,
                                        const RfLeanX &lx = RfLeanX{}) {
    static_assert(!LEAN || (!SERVE && !MLP && !IDS && !PROBE), "the lean entry is the stacked call's");
    static_assert(!CHECK || (!MLP && !IDS && !PROBE), "the offsets check belongs to the plain launch");
    static_assert(!SERVE || (CHECK && !MLP && !IDS && !PROBE), "the resident form serves the drop-in call (lS_o given)");
#ifdef EVS_X_PT
    const long long pt_t0 = (long long)wall_clock64();
    if (threadIdx.x == 0) EVS_PT_TABLE[blockIdx.x & 1023][15] += 1ull;
#endif
#ifndef EVS_X_SRV
#define EVS_X_SRV 0     // developer A/B of the resident form (timing only): 2 = R stores without sc1, 4 = workers sleep longer between polls
#endif
    constexpr int kCpol = (SERVE && !(EVS_X_SRV & 2)) ? (EVS_OUT_CPOL | 16) : EVS_OUT_CPOL;   // (aux bit 4 = sc1 on gfx940+: agent scope, write-through)
    constexpr int NR = NT;
    constexpr int NC = CQ + REM;
    constexpr int d = 4 * (4 * CQ + REM);
    constexpr int LPRD = d / 4;             // lanes per fp32 row (16 B each)
    constexpr int RPI = 64 / LPRD;          // rows per load instruction
    constexpr int NROWS = 16 * NT;
    constexpr int MAXF = NT == 2 ? kTileMaxF : 16;
    constexpr int NJ = (MAXF + RPI - 1) / RPI;   // load instructions per sample
    constexpr int row_bytes = d * 4;
    static_assert(NJ * RPI <= 32, "a tile row per fetched row");
    __shared__ __attribute__((aligned(16))) char s_rows[4][NJ * 1024];   // per wave: transpose buffer (DMA image of one sample)
    __shared__ int s_idx[2 * 512];                                        // [2][32 features][16 samples]: row id, sample id (dense), -1 = zeros
    __shared__ const int64_t *s_tile_p[32];
    __shared__ unsigned s_tile_nr[32];
    __shared__ int s_tile_kind[32];                                       // 0 absent, 1 dense (x, received pooled vectors), 2 table
    __shared__ unsigned long long s_feat_base[32];                        // per feature: first row / bytes between rows -- read per
    __shared__ unsigned s_feat_scale[32];                                 // load instead of living in 12 VGPRs per lane
    __shared__ unsigned s_sa_base[PROBE ? 32 : 1];                        // PROBE, set-associative cache: dense row number of row 0 of feature f's table
    // PROBE, the update folded in as well (ProbeArgs::arena_w): totals of the inserts this block makes
    __shared__ int s_udelta[PROBE ? kMaxBuckets : 1];
    __shared__ int s_ustat[PROBE ? 2 : 1];
    __shared__ unsigned long long s_srv_src[SERVE ? 32 : 1];              // SERVE: the tables' addresses and row counts, read from the template ONCE per
    __shared__ unsigned s_srv_nr[SERVE ? 32 : 1];                         // block (srv_first) -- the launch form pays that round trip per chunk
    __shared__ const int64_t *s_tile_o[CHECK ? 32 : 1];                   // CHECK: offsets arrays, their readable entries, nnz
    __shared__ int64_t s_tile_ol[CHECK ? 32 : 1], s_tile_nz[CHECK ? 32 : 1];
    constexpr int OUT_MAX = ((d + NROWS * (NROWS + 1) / 2 + 63) / 64) * 64;
    // staged output rows: one slot per wave (flushed an iteration later), or with MLP all 16 rows of the chunk
    constexpr int kOutRows = MLP ? 16 : 4;
    constexpr int kOutStride = MLP ? kMlpRowStride : OUT_MAX + 16;
    __shared__ __attribute__((aligned(16))) float s_out[kOutRows][kOutStride];
    __shared__ float s_dump[MLP ? 4 * 16 : 1];   // MLP: where the never-stored accumulator elements go

    // (SERVE: the resident grid runs this body in a loop; every lane-invariant table below -- staging offsets, flush offsets,
    //  operand addresses -- derives from the thread index, and left alone the compiler hoists all of them out of the loop and
    //  keeps them alive across the head: 128 VGPRs and 65 spilled.  An opaque copy of the index per call keeps them where the
    //  launch form has them.)
    unsigned tid_x = threadIdx.x;
    if constexpr (SERVE) asm volatile("" : "+v"(tid_x));
    const int lane = tid_x & (kWave - 1);
    const int r16 = lane & 15;
    const int q = lane >> 4;
    const int F = args.F, itself = args.itself;
    const int out_row = d + args.P;
    const int64_t B = SERVE ? sd.B : args.B;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(tid_x >> 6));
    char *my_lds = s_rows[wave_in_block];
    float *my_out = s_out[wave_in_block];   // (MLP: re-pointed per sample)
    const char *zeros_l = LEAN ? nullptr : reinterpret_cast<const char *>(args.zeros);   // (LEAN: read from the descriptor behind the index loads)

    // ---- the block's sample range and the feature table of the tile ------------------------------------
    // K batches in one launch (multi_n > 0; plain and CHECK launches): block i = chunk i % multi_cpb of batch i / multi_cpb;
    // sample numbers below are the batch's own, x / indices / offsets / R come from the batch's entries
    const int64_t per = args.tile_per;
    int blk_id = blk_in, batch_k = 0;
    if constexpr (!MLP && !IDS && !PROBE) {
        if (!LEAN && args.multi_n > 0) { batch_k = blk_id / args.multi_cpb; blk_id -= batch_k * args.multi_cpb; }
    }
    const bool multi = SERVE || (!LEAN && !MLP && !IDS && !PROBE && args.multi_n > 0);
    float *const R_base = SERVE ? sd.R : (multi ? ka->multi_R[batch_k] : args.R);
    const int64_t blk_first = (int64_t)blk_id * per;
    const int64_t blk_end = blk_first + per < B ? blk_first + per : B;
    if (blk_first >= blk_end) return;       // block-uniform
    const int blk_n = (int)(blk_end - blk_first);
    const int n_samples = blk_n > wave_in_block ? (blk_n - wave_in_block + 3) / 4 : 0;
    // Round 6: the stacked form of the call (FusedArgs::stk, and every batch of the resident dispatcher) -- its index / offsets
    // loads need nothing of the feature table below, so they go out FIRST and the table's round trip to the kernel arguments
    // runs under them: one dependent round trip less in the head of every block.
    const bool stk = SERVE || LEAN || (!MLP && !IDS && !PROBE && args.stk != 0 && args.multi_n == 0);
    const int64_t *const stk_idx = SERVE ? sd.idx : args.stk_idx, *const stk_off = SERVE ? sd.off : args.stk_off;
    const int64_t stk_istride = SERVE ? sd.idx_stride : args.stk_idx_stride, stk_ostride = SERVE ? sd.off_stride : args.stk_off_stride;
    const int64_t stk_ol = SERVE ? sd.B : args.stk_off_len;
    // ---- index tiles: thread e (and e + 256) owns tile element (feature e >> 4, sample-in-chunk e & 15) ----
    bool bad = false, my_ragged = false;
    bool oob[2] = {false, false};
    int64_t tile_v[2] = {-1, -1};
    int64_t tile_o0[2] = {0, 0}, tile_o1[2] = {0, 0};   // CHECK: offsets[b] and where bag b ends
    const int64_t *dummy_i = args.dummy_i64;   // any readable int64 (lanes with nothing to load read it)
    auto tile_load = [&](int c) {       // chunk c of the block -> registers; no branch, no use of the value before tile_store
        const int64_t bs = blk_first + 16 * (int64_t)c + (tid_x & 15);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = ((int)tid_x >> 4) + 16 * h;
            // (stk: x + tables behind ONE (T, B) index array -- the Criteo collate's -- whose rows are at a fixed stride: the address is
            //  arithmetic, nothing of the block's feature table is needed, and the loads leave BEFORE that table is read)
            const bool table = (stk ? (f >= 1 && f < F) : s_tile_kind[f] == 2) && bs < blk_end;
            if constexpr (IDS) {
                const int *ap = table ? args.row_ids + bs * (int64_t)(F - 1) + (f - 1) : reinterpret_cast<const int *>(dummy_i);
                tile_v[h] = *reinterpret_cast<const __attribute__((address_space(1))) int *>(reinterpret_cast<uintptr_t>(ap));
            } else {
                const int64_t *ap = table ? (stk ? stk_idx + (int64_t)(f - 1) * stk_istride : s_tile_p[f]) + bs : dummy_i;
                // (explicitly global: a flat load would force every later wait to vmcnt(0))
                tile_v[h] = rf_ld_i64<SERVE>(ap);
            }
            if constexpr (CHECK) {
                const int64_t *op = stk ? stk_off + (int64_t)(f - 1) * stk_ostride : s_tile_o[f];
                const bool own = table && ((tid_x & 15) == 15 || bs + 1 >= blk_end);
                const int64_t *p0 = table ? op + bs : dummy_i;
                const int64_t *p1 = (own && bs + 1 < (stk ? stk_ol : s_tile_ol[f])) ? op + bs + 1 : dummy_i;
                tile_o0[h] = rf_ld_i64<SERVE>(p0);
                tile_o1[h] = rf_ld_i64<SERVE>(p1);
            }
        }
    };
    if constexpr (!PROBE) { if (stk) tile_load(0); }
    if constexpr (LEAN) {
        // nothing in front of the index loads but arithmetic on the kernel's scalars: the descriptor is asked for behind them
        __builtin_amdgcn_sched_barrier(0);
        zeros_l = reinterpret_cast<const char *>(lx.md->zeros);
        if (tid_x < 32) {
            // lane f: ONE 16-byte load of feature f's record (the descriptor has 32 of them: unconditional, as below)
            const int f = (int)tid_x;
            const bool on = f < F, table = f >= 1 && on;
            typedef const __attribute__((address_space(1))) u32x4 *gu4_t;
            const u32x4 rec = *reinterpret_cast<gu4_t>(reinterpret_cast<uintptr_t>(&lx.md->feat[f]));
            const unsigned long long src = ((unsigned long long)rec[1] << 32) | rec[0];
            s_tile_p[f] = table ? stk_idx + (int64_t)(f - 1) * stk_istride : nullptr;
            s_tile_nr[f] = table ? rec[2] : 0u;
            s_tile_kind[f] = !on ? 0 : (table ? 2 : 1);
            s_feat_base[f] = !on ? 0ull : (f == 0 ? (unsigned long long)reinterpret_cast<uintptr_t>(lx.x) : src);
            s_feat_scale[f] = !on ? 0u : (table ? (unsigned)row_bytes : (unsigned)lx.x_stride * 4u);
            if constexpr (CHECK) {
                s_tile_o[f] = table ? stk_off + (int64_t)(f - 1) * stk_ostride : nullptr;
                s_tile_ol[f] = table ? stk_ol : 0;
                s_tile_nz[f] = table ? B : 0;      // (whole batches: nnz == B)
            }
        }
    } else
    if (tid_x < 32) {
        // branch-free on purpose: every FusedArgs array has EVS_MAX_FEATURES = 32 entries (those past F are NULL / 0), so
        // lane f reads entry f of each of them UNCONDITIONALLY -- all the loads leave together, one round trip -- and the
        // tests below are selects on the values.  (Written as `f < F ? ka->x[f] : 0` the compiler puts each load behind
        // its own branch and wait: three to six DEPENDENT round trips to the kernel arguments in front of the first index
        // load, in every block of every launch -- the larger part of the launch's fixed cost.)
        const int f = (int)tid_x;
        const bool on = f < F;
        const int64_t *ip = nullptr;
        unsigned long long src = 0ull;
        int64_t nr = 0, stride = 0;
        const int64_t *op = nullptr;
        int64_t ol = 0, nz = 0;
        if constexpr (SERVE) {
            if (srv_first) {   // (block-uniform) the one round trip to the template this block ever makes
                s_srv_src[f] = (unsigned long long)reinterpret_cast<uintptr_t>(ka->src[f]);
                s_srv_nr[f] = (unsigned)ka->n_rows[f];
            }
            src = s_srv_src[f]; nr = (int64_t)s_srv_nr[f];
            ol = sd.B; nz = sd.B;
        } else {
            ip = ka->indices[f];
            src = (unsigned long long)reinterpret_cast<uintptr_t>(ka->src[f]);
            nr = ka->n_rows[f];
            stride = ka->stride[f];
            if constexpr (CHECK) { op = ka->offsets[f]; ol = ka->off_len[f]; nz = ka->nnz[f]; }
        }
        unsigned long long mx = 0ull;
        const int64_t *mi = nullptr, *mo = nullptr;
        if constexpr (SERVE) {
            mx = (unsigned long long)reinterpret_cast<uintptr_t>(sd.x); mi = sd.idx; mo = sd.off;
        } else if constexpr (!MLP && !IDS && !PROBE) {
            const int kk = multi ? batch_k : 0;   // (entry 0 is always readable)
            mx = (unsigned long long)reinterpret_cast<uintptr_t>(ka->multi_x[kk]);
            mi = ka->multi_idx[kk];
            if constexpr (CHECK) mo = ka->multi_off[kk];
        }
        const int64_t m_istride = SERVE ? sd.idx_stride : args.multi_idx_stride, m_ostride = SERVE ? sd.off_stride : args.multi_off_stride;
        if (multi) ip = (f >= 1 && on) ? mi + (int64_t)(f - 1) * m_istride : nullptr;
        if (!on) ip = nullptr;
        const bool table = (IDS || PROBE) ? (f >= 1 && on) : ip != nullptr;
        s_tile_p[f] = ip;
        s_tile_nr[f] = on ? (unsigned)nr : 0u;
        s_tile_kind[f] = !on ? 0 : (table ? 2 : 1);
        s_feat_base[f] = !on ? 0ull : ((multi && f == 0) ? mx : src);
        s_feat_scale[f] = !on ? 0u : (table ? (unsigned)row_bytes : (unsigned)(((SERVE && f == 0) ? sd.x_stride : stride) * 4));
        if constexpr (PROBE) s_sa_base[f] = ka->probe.sau.row_base[(f + 31) & 31];   // (feature f = table f - 1; unconditional read, as above)
        if constexpr (CHECK) {
            s_tile_o[f] = table ? (multi ? mo + (int64_t)(f - 1) * m_ostride : op) : nullptr;
            s_tile_ol[f] = table ? ol : 0;
            s_tile_nz[f] = table ? nz : 0;
        }
    }
    __syncthreads();

    // ---- DMA-shaped mapping: for load j this lane fetches piece dma_piece of row j*RPI + dma_r0.  Lanes past the last
    // whole row of an instruction (lane 63 at d = 36) mirror the last piece: the same 16 bytes, one request, and their
    // copy lands in the padding of the 1 KiB image block.  Rows >= F have tile entries -1 and read the zero page.
    const int lane_eff = lane < RPI * LPRD ? lane : RPI * LPRD - 1;
    const int dma_piece16 = (lane_eff % LPRD) * 16;
    const int dma_r0 = lane_eff / LPRD;
    // ---- MFMA operand mapping (as the LDS-DMA loop: row r at (r / RPI) KiB + (r % RPI) * row_bytes) -------
    int lds_off[NR];
#pragma unroll
    for (int rr = 0; rr < NR; rr++) {
        const int row = r16 + 16 * rr;
        lds_off[rr] = (row / RPI) * 1024 + (row % RPI) * row_bytes + q * CQ * 16;
    }
    constexpr int kRemOff = 4 * CQ * 16;
    int rem_off[NR];   // element q of the first trailing chunk of this lane's tile rows
#pragma unroll
    for (int rr = 0; rr < NR; rr++) rem_off[rr] = lds_off[rr] - q * CQ * 16 + kRemOff + q * 4;
    constexpr int kOob = 0x7ffffff0;
    // (`on` false: a zero-length buffer resource, the hardware drops every store -- the loop body has no branch around
    //  its vector-memory operations, see the main loop)
#ifndef EVS_RF_OLDFLUSH
    // lane-invariant pieces of the flush, computed once: which 16-byte piece of the staged row this lane moves in store h
    // (an rf launch has F <= kTileMaxF: at most d + 28 * 29 / 2 = 442 floats, two store instructions of 64 x 16 bytes
    // cover them -- the generic 32-row bound would issue a third that the bounds check always drops), its offset in R's
    // row (kOob: dropped by the buffer bounds check), and the same for the 0..3 trailing floats
    constexpr int kFlushMaxRow = MLP ? OUT_MAX : ((d + MAXF * (MAXF + 1) / 2 + 3) / 4) * 4;
    constexpr int NFL = (kFlushMaxRow + 255) / 256;
    int fl_lds[NFL], fl_off[NFL], fl_tail_lds = 0, fl_tail_off = 0;   // filled by fill_hoists(), behind the row requests
    auto fill_flush = [&]() {
        const int n4 = out_row >> 2;
#pragma unroll
        for (int h = 0; h < NFL; h++) {
            const int e4 = lane + 64 * h;
            fl_lds[h] = 16 * (e4 < n4 ? e4 : 0);
            fl_off[h] = e4 < n4 ? 16 * e4 : kOob;
            // (keep them in registers: the compiler otherwise re-derives them per sample.  LEAN leaves them to the compiler: pinned, its
            //  checked d = 36 entry needs 105 VGPRs, one above the budget; unpinned 103 -- a few compares and selects per sample)
            if constexpr (!LEAN) asm volatile("" : "+v"(fl_lds[h]), "+v"(fl_off[h]));
        }
        fl_tail_lds = 4 * (4 * (out_row >> 2) + (lane & 3));
        fl_tail_off = lane < (out_row & 3) ? fl_tail_lds : kOob;
        if constexpr (LEAN) asm volatile("" : "+v"(fl_tail_lds));
        else asm volatile("" : "+v"(fl_tail_lds), "+v"(fl_tail_off));
    };
    auto flush_out = [&](int64_t bp, bool on) {
        if constexpr (MLP) on = on && args.write_r;
        float *Rb = R_base + (on ? bp : 0) * (int64_t)out_row;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Rb, 0, on ? out_row * 4 : 0, 0x00020000);
#pragma unroll
        for (int h = 0; h < NFL; h++) {
            const float4 v = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(my_out) + fl_lds[h]);
            u32x4 u = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
            __builtin_amdgcn_raw_buffer_store_b128(u, rs, fl_off[h], 0, kCpol);
        }
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(*reinterpret_cast<const float *>(reinterpret_cast<const char *>(my_out) + fl_tail_lds)),
                                              rs, fl_tail_off, 0, kCpol);
    };
#else
    auto flush_out = [&](int64_t bp, bool on) {
        if constexpr (MLP) on = on && args.write_r;
        float *Rb = R_base + (on ? bp : 0) * (int64_t)out_row;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Rb, 0, on ? out_row * 4 : 0, 0x00020000);
        const int n4 = out_row >> 2;   // whole 16-byte pieces; the 0..3 trailing floats go as dwords
        // (always the same number of store instructions: out-of-range lanes and whole out-of-range instructions are
        //  dropped by the buffer bounds check, and the waitcnt bookkeeping stays static)
#pragma unroll
        for (int h = 0; h < (OUT_MAX + 255) / 256; h++) {
            const int e4 = lane + 64 * h;
            const float4 v = reinterpret_cast<const float4 *>(my_out)[e4 < n4 ? e4 : 0];
            u32x4 u = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
            __builtin_amdgcn_raw_buffer_store_b128(u, rs, e4 < n4 ? 16 * e4 : kOob, 0, kCpol);
        }
        {
            const int e = 4 * n4 + (lane & 3);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(my_out[e]), rs, lane < (out_row & 3) ? 4 * e : kOob, 0, kCpol);
        }
    };

#endif

    auto tile_store = [&](int c) {      // registers -> tile buffer c & 1
        const int64_t bs = blk_first + 16 * (int64_t)c + (tid_x & 15);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = ((int)tid_x >> 4) + 16 * h;
            const int kind = s_tile_kind[f];
            const bool live = kind != 0 && bs < blk_end && c >= 0;
            const int64_t v = kind == 2 ? tile_v[h] : bs;       // dense features (x, received pooled vectors): the sample number
            const bool in_range = kind == 1 || (IDS ? v >= 0 : (uint64_t)v < (uint64_t)s_tile_nr[f]);   // (IDS: the probe kernel checked the row ids)
            if constexpr (CHECK) oob[h] = live & !in_range;   // (whether it counts is verify()'s call: see there)
            else bad |= live & !in_range;
            s_idx[(c & 1) * 512 + (int)tid_x + 256 * h] = (live & in_range) ? (int)v : -1;
        }
    };

    // CHECK: the verdict on the offsets -- is every bag of the chunk exactly {idx[b]}?  (Taken in front of the row requests.
    // Behind them -- rows asked for on the bet that it is, compares and the block barrier under their round trip, the slow
    // loop at the end of the kernel overwriting what the one-index code produced -- was built and measured: 22.3 instead of
    // 20.7 us at B = 16 384; the offsets pairs then live across the 64 row registers, 128 VGPRs and spills.)
    // A bag ends where the next one starts, and the next one's start is its own lane's o0 (same feature, next sample): every lane
    // checks that ITS bag starts at its own position, the lane of the chunk's last sample also where that bag ends -- no
    // exchange between lanes (round 4: the shuffle and the second 64-bit compare per key were 10 VALU instructions per
    // sample in front of the row requests).
    bool fast_bad = false;   // out-of-range indices seen by the one-index code; they count only if the block stays on it
    auto verify = [&]() {
        const int64_t bs = blk_first + (tid_x & 15);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = ((int)tid_x >> 4) + 16 * h;
            // (an index whose own bag is not {idx[b]} may sit at a position no bag refers to: the slow loop, which this
            //  block then runs, has the verdict on it)
            const bool table = s_tile_kind[f] == 2 && bs < blk_end;
            const bool own = table && ((tid_x & 15) == 15 || bs + 1 >= blk_end);
            int64_t o1 = tile_o1[h];
            if (!(bs + 1 < s_tile_ol[f])) o1 = s_tile_nz[f];   // the last bag ends at nnz
            const bool ok = (tile_o0[h] == bs) & (!own | (o1 == bs + 1));
            my_ragged |= table & !ok;
            fast_bad |= oob[h];
        }
    };

    // ---- the rows of this wave's sample n -> registers (D samples in flight) ----------------------------
    f32x4 ring[D][NJ];
    // per load j this lane always fetches a row of the SAME feature (tile row dma_r0 + j * RPI): where that feature's rows
    // start (plus this lane's 16-byte piece) and how far apart they are, read from the block's feature table once
    unsigned long long fbase[NJ];
    unsigned fscale[NJ];
    int idx_lds[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int r = dma_r0 + j * RPI;               // < 32: tile rows >= F hold -1
        fbase[j] = s_feat_base[r] + (unsigned long long)dma_piece16;
        // (LEAN: every table's rows are row_bytes apart and only tile row 0 is x, so the distance is a constant for every load but
        //  this lane's first -- no LDS read, and NJ - 1 registers less across the loop; rows >= F never use it: their entries are -1)
        if constexpr (LEAN) fscale[j] = (j == 0 && dma_r0 == 0) ? (unsigned)lx.x_stride * 4u : (unsigned)row_bytes;
        else fscale[j] = s_feat_scale[r];
        idx_lds[j] = 4 * (r * 16 + wave_in_block);    // byte address of tile entry (row r, sample wave_in_block) in s_idx
    }
    const unsigned long long zeros_piece = (unsigned long long)reinterpret_cast<uintptr_t>(zeros_l) + (unsigned long long)dma_piece16;
    auto issue = [&](int n, f32x4 (&slot)[NJ]) {
        // block-local sample m = wave_in_block + 4 n (< 16: one chunk per block): tile buffer 0, entry m of each row
        const unsigned phantom = (unsigned)n < (unsigned)n_samples ? 0u : 0xffffffffu;   // past this wave's samples: every lane reads the zero page
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int iv = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(s_idx) + idx_lds[j] + 16 * n);
            // branch-free on purpose (bit blend, not a select: the compiler turns a select over these LDS reads into
            // control flow and serialises the four loads): -1 -> the zero page
            const unsigned neg = (unsigned)(iv >> 31) | phantom;
            unsigned long long base = fbase[j];
            unsigned idx = (unsigned)iv & ~neg;
            if constexpr (IDS || PROBE) {   // bit 30: a row of the cache arena (bit blend, as below: no select over LDS reads)
                const unsigned long long in_arena = 0ull - (unsigned long long)((idx >> 30) & 1u);
                base ^= (base ^ ((unsigned long long)reinterpret_cast<uintptr_t>(args.arena) + (unsigned long long)dma_piece16)) & in_arena;
                idx &= 0x3fffffffu;
            }
            const unsigned long long p = base + (unsigned long long)idx * (unsigned long long)fscale[j];
            const unsigned long long m64 = ((unsigned long long)neg << 32) | neg;
            const unsigned long long pa = p ^ ((p ^ zeros_piece) & m64);
            slot[j] = *reinterpret_cast<gf4_t>((uintptr_t)pa);
        }
    };
    // a: this lane's CQ k-slot chunks of tile rows r16 (+ 16); rem: element q of each of the REM trailing chunks (all four
    // k-slots hold those chunks, slot q contributes element q -- read as ONE float from the image, not selected out of four)
    auto interact = [&](const float4 (&a)[NR][CQ > 0 ? CQ : 1], const float (&rem)[NR][REM > 0 ? REM : 1], f32x4 &c00, f32x4 &c10, f32x4 &c11) {
        c00 = f32x4{0.f, 0.f, 0.f, 0.f}; c10 = f32x4{0.f, 0.f, 0.f, 0.f}; c11 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < CQ; c++) {
            const float e0[4] = {a[0][c].x, a[0][c].y, a[0][c].z, a[0][c].w};
            const float e1[4] = {a[NR - 1][c].x, a[NR - 1][c].y, a[NR - 1][c].z, a[NR - 1][c].w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0[e], e0[e], c00, 0, 0, 0);
                if constexpr (NT == 2) {
                    c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1[e], e0[e], c10, 0, 0, 0);
                    c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1[e], e1[e], c11, 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < REM; m++) {
            const float s0 = rem[0][m], s1 = rem[NR - 1][m];
            c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(s0, s0, c00, 0, 0, 0);
            if constexpr (NT == 2) {
                c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1, s0, c10, 0, 0, 0);
                c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1, s1, c11, 0, 0, 0);
            }
        }
    };

    // ---- where the accumulators go in the staged output row: lane-invariant, computed ONCE (relative to my_out; left to
    // itself the compiler re-derives the twelve offsets -- multiplies, compares, exec-mask regions -- for every sample)
    int zo00h[4], zo10h[4], zo11h[4];
    int xv_off[(d + 63) / 64];
    auto fill_stage = [&]() {
        const int dump0 = 4 * (OUT_MAX + r16);
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int i = 4 * q + v;
            zo00h[v] = (i < F && r16 < i + itself) ? 4 * (d + (i * (i - 1 + 2 * itself)) / 2 + r16) : dump0;
            const int gi = 16 + i;
            const int base = (gi * (gi - 1 + 2 * itself)) / 2;
            zo10h[v] = (NT == 2 && gi < F) ? 4 * (d + base + r16) : dump0;
            zo11h[v] = (NT == 2 && gi < F && 16 + r16 < gi + itself) ? 4 * (d + base + 16 + r16) : dump0;
            asm volatile("" : "+v"(zo00h[v]), "+v"(zo10h[v]), "+v"(zo11h[v]));
        }
#pragma unroll
        for (int h = 0; h < (d + 63) / 64; h++) {
            const int e = lane + 64 * h;
            xv_off[h] = e < d ? 4 * e : 4 * (OUT_MAX + r16);
        }
    };

    auto flush_slow = [&](int64_t bp) {   // the slow block's flush: offsets computed in place (the hoisted ones are not filled yet)
        float *Rb = R_base + bp * (int64_t)out_row;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Rb, 0, out_row * 4, 0x00020000);
        const int n4 = out_row >> 2;
#pragma unroll
        for (int h = 0; h < NFL; h++) {
            const int e4 = lane + 64 * h;
            const float4 v = reinterpret_cast<const float4 *>(my_out)[e4 < n4 ? e4 : 0];
            u32x4 u = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
            __builtin_amdgcn_raw_buffer_store_b128(u, rs, e4 < n4 ? 16 * e4 : kOob, 0, kCpol);
        }
        const int e = 4 * n4 + (lane & 3);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(my_out[e]), rs, lane < (out_row & 3) ? 4 * e : kOob, 0, kCpol);
    };
    // ---- CHECK, rare: a block that finds a bag other than {idx[b]} pools ITS samples with the general semantics --------
    auto slow_block = [&]() {
        for (int u = 0; u < n_samples; u++) {
            const int64_t b = blk_first + wave_in_block + 4 * (int64_t)u;
            float4 a[NR][NC];
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                const int f = r16 + 16 * rr;
#pragma unroll
                for (int c = 0; c < NC; c++) a[rr][c] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (f >= F) continue;
                // byte offset of chunk c inside a row: this lane's k-slot chunks, then the shared remainder chunks
                auto chunk_at = [&](const char *row, int c) -> float4 {
                    return *reinterpret_cast<const float4 *>(row + (c < CQ ? (q * CQ + c) * 16 : kRemOff + (c - CQ) * 16));
                };
                const int64_t *ip = s_tile_p[f];                                            // (multi: this batch's arrays)
                const char *src = reinterpret_cast<const char *>((uintptr_t)s_feat_base[f]);
                if (!ip) {   // dense feature (x, received pooled vectors)
                    const char *row = src + (uint64_t)b * (uint64_t)(((SERVE && f == 0) ? sd.x_stride : (LEAN ? (int64_t)lx.x_stride : ka->stride[f])) * 4);
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        if constexpr (SERVE) {   // (x: fresh from memory, see rf_ld_*)
                            const float *fp = reinterpret_cast<const float *>(row + (c < CQ ? (q * CQ + c) * 16 : kRemOff + (c - CQ) * 16));
                            a[rr][c] = make_float4(rf_ld_f32<true>(fp), rf_ld_f32<true>(fp + 1), rf_ld_f32<true>(fp + 2), rf_ld_f32<true>(fp + 3));
                        } else a[rr][c] = chunk_at(row, c);
                    }
                    continue;
                }
                const int64_t *op = s_tile_o[f];
                const int64_t nnz = (SERVE || LEAN) ? B : ka->nnz[f];
                int64_t s0 = rf_ld_i64<SERVE>(op + b);
                int64_t e0 = (b + 1 < ((SERVE || LEAN) ? stk_ol : ka->off_len[f])) ? rf_ld_i64<SERVE>(op + b + 1) : nnz;
                if (!((s0 >= 0) & (e0 >= s0) & (e0 <= nnz))) { bad = true; s0 = e0 = 0; }
                const uint64_t n_rows = SERVE ? (uint64_t)s_srv_nr[f] : (LEAN ? (uint64_t)s_tile_nr[f] : (uint64_t)ka->n_rows[f]);
                for (int64_t j = s0; j < e0; j++) {
                    const int64_t r = rf_ld_i64<SERVE>(ip + j);
                    if ((uint64_t)r >= n_rows) { bad = true; continue; }   // skipped; a skipped FIRST row counts as zeros
                    const char *row = src + (uint64_t)r * (uint64_t)row_bytes;
#pragma unroll
                    for (int c = 0; c < NC; c++) {
                        const float4 t = chunk_at(row, c);
                        if (j == s0) { a[rr][c] = t; continue; }
                        a[rr][c].x = __fadd_rn(a[rr][c].x, t.x); a[rr][c].y = __fadd_rn(a[rr][c].y, t.y);
                        a[rr][c].z = __fadd_rn(a[rr][c].z, t.z); a[rr][c].w = __fadd_rn(a[rr][c].w, t.w);
                    }
                }
            }
            float xv[(d + 63) / 64];   // x[b] (feature 0, dense) for the passthrough columns
#pragma unroll
            for (int h = 0; h < (d + 63) / 64; h++) {
                const int e = lane + 64 * h;
                xv[h] = rf_ld_f32<SERVE>(reinterpret_cast<const float *>(reinterpret_cast<const char *>((uintptr_t)s_feat_base[0]) + (uint64_t)b * (uint64_t)((SERVE ? sd.x_stride : (LEAN ? (int64_t)lx.x_stride : ka->stride[0])) * 4)) + (e < d ? e : 0));
            }
            f32x4 c00, c10, c11;
            {
                float4 aq[NR][CQ > 0 ? CQ : 1];
                float ar[NR][REM > 0 ? REM : 1];
#pragma unroll
                for (int rr = 0; rr < NR; rr++) {
#pragma unroll
                    for (int c = 0; c < CQ; c++) aq[rr][c] = a[rr][c];
#pragma unroll
                    for (int m = 0; m < REM; m++) {
                        const float4 t = a[rr][CQ + m];
                        ar[rr][m] = q == 0 ? t.x : q == 1 ? t.y : q == 2 ? t.z : t.w;
                    }
                }
                interact(aq, ar, c00, c10, c11);
            }
            const int dump = 4 * (OUT_MAX + r16);
#pragma unroll
            for (int h = 0; h < (d + 63) / 64; h++) {
                const int e = lane + 64 * h;
                *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + (e < d ? 4 * e : dump)) = xv[h];
            }
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const int i = 4 * q + v;
                const int zo00 = (i < F && r16 < i + itself) ? 4 * (d + (i * (i - 1 + 2 * itself)) / 2 + r16) : dump;
                *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo00) = c00[v];
                if constexpr (NT == 2) {
                    const int gi = 16 + i;
                    const int base = (gi * (gi - 1 + 2 * itself)) / 2;
                    const int zo10 = gi < F ? 4 * (d + base + r16) : dump;
                    const int zo11 = (gi < F && 16 + r16 < gi + itself) ? 4 * (d + base + 16 + r16) : dump;
                    *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo10) = c10[v];
                    *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo11) = c11[v];
                }
            }
            flush_slow(b);
        }
        if (bad) atomicOr(LEAN ? lx.md->err : args.err, 1);
    };

    static_assert(D == 4, "a block owns one 16-sample chunk: 4 samples per wave");
    if constexpr (PROBE) {
        // ---- the cache probe, folded in: thread e (and e + 256) owns key (table (e >> 4) - 1, sample e & 15) -------------
        __shared__ int s_agg[16];                 // hits per request of the chunk
        __shared__ int s_pdelta[kMaxBuckets];     // priority histogram moves
        __shared__ int s_psum[2];                 // hits / perfect requests
        __shared__ int s_nlist;                   // misses listed
        const ProbeArgs &pa = args.probe;
        const int T = pa.T;
        for (int i = tid_x; i < kMaxBuckets; i += blockDim.x) s_pdelta[i] = 0;
        if (tid_x < 16) s_agg[tid_x] = 0;
        if (tid_x < 2) s_psum[tid_x] = 0;
        if (tid_x == 0) s_nlist = 0;
        __syncthreads();
        int pe[2], prow[2], pprio[2], pway[2];
        unsigned phint[2], ptag[2];
        bool pok[2], ptomb[2], pact[2];
        unsigned long long pkey[2], phome[2], pw0[2];
        const int64_t bs = blk_first + (tid_x & 15);
        // ---- the policy update folded in too (round 5; ProbeArgs::arena_w != nullptr: a set-associative fp32 tier alone with a
        // two-copy arena, evs_hash.h).  A thread that misses a key claims a way of the key's set right here -- it holds the
        // set's ways already: rank, ONE CAS, beside the priority raises -- and the lanes that gather the key's row from its
        // table for the interaction store it into the arena on the way (s_idx's second tile buffer carries the arena row to
        // the consume loop).  No miss lists, no update launch, no second read of anything.  What makes it legal inside the
        // launch that is still probing: the new word carries THIS batch's stamp (= pa.pend_stamp: a miss for every prober of
        // this launch -- the row may not be there yet) and names the arena copy the retired word does not, so a prober that
        // read the old word reads a row nobody is writing.
        const bool ins = pa.arena_w != nullptr;   // block-uniform
        if (ins) {
            for (int i = tid_x; i < kMaxBuckets; i += blockDim.x) s_udelta[i] = 0;
            if (tid_x < 2) s_ustat[tid_x] = 0;
        }
        // the thread's two keys side by side, one round trip per step for both: request rows, home slots, priorities
        // (a key whose home slot holds neither it nor nothing walks its chain with probe_ro: rare at load <= 0.25)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = ((int)tid_x >> 4) + 16 * h;
            pact[h] = f >= 1 && f < F && bs < blk_end;
            const int *rp = pact[h] ? pa.requests + bs * (int64_t)T + (f - 1) : reinterpret_cast<const int *>(dummy_i);
            prow[h] = *reinterpret_cast<const __attribute__((address_space(1))) int *>(reinterpret_cast<uintptr_t>(rp));
        }
        EVS_PTW(1);          // (the request rows are here)
        unsigned lw[2][8];   // the two keys' set ways (kept for the claim of a missed key)
        const bool sa = pa.sa.tags != nullptr;   // set-associative cache (evs_hash.h): one line per key, the priority inside the way word
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = ((int)tid_x >> 4) + 16 * h;
            const unsigned nrf = s_tile_nr[f & 31];
            pok[h] = pact[h] & (prow[h] >= 0) & ((unsigned)prow[h] < nrf);
            pkey[h] = ((unsigned long long)f << 32) | (unsigned)prow[h];   // table_1based = f
        }
        if (sa) {
            unsigned pset[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int f = ((int)tid_x >> 4) + 16 * h;
                sa_split(pa.sa, sa_perm(pa.sau, s_sa_base[f & 31] + (pok[h] ? (unsigned)prow[h] : 0u)), pset[h], ptag[h]);
                if (!pok[h]) pset[h] = 0u;
            }
            // (the probe is folded into this kernel for 8-way tiers only -- the host checks: evs_cache.hip -- so the way count
            //  is a compile-time constant: exactly two 16-byte loads and an 8-way search per key)
            SaLine line[2];
#pragma unroll
            for (int h = 0; h < 2; h++) sa_load<8>(pa.sa, pset[h], line[h]);
            __builtin_amdgcn_sched_barrier(0);   // both keys' set lines in one round trip
            EVS_PTW(2);          // (the set lines are here)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                unsigned w;
                const int way = sa_find<8>(pa.sa, line[h], ptag[h], w, pa.pend_stamp);
                const bool found = pok[h] && way >= 0;
                pe[h] = found ? (int)sa_entry(pa.sa, pset[h], (unsigned)way, w) : -1;
                pway[h] = way;
                pprio[h] = found ? sa_prio(w) : 0x7fffffff;
                pw0[h] = w; phint[h] = pset[h]; ptomb[h] = false;
#pragma unroll
                for (int j = 0; j < 8; j++) lw[h][j] = sa_way_word(line[h], j);
                if (found) atomicAdd(&s_agg[tid_x & 15], 1);
            }
        } else {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            phome[h] = mix64(pkey[h]) & pa.mask;
            pw0[h] = pa.slots[pok[h] ? phome[h] : 0];
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            pe[h] = -1; phint[h] = 0; ptomb[h] = false; pprio[h] = 0x7fffffff;
            if (pok[h]) {
                unsigned long long end_slot = phome[h];
                bool ht = false;
                int e = -1;
                if ((pw0[h] & kKeyMask) == pkey[h]) {
                    const unsigned fld = (unsigned)(pw0[h] >> kKeyBits);
                    e = fld >= kFieldPend ? -1 : (int)fld;
                } else if (pw0[h] != kEmpty) {
                    e = probe_ro(pa.slots, pa.mask, pkey[h], end_slot, pa.reusable_tomb, &ht);
                    if (e == kPending) e = -1;
                }
                pe[h] = e; phint[h] = (unsigned)(end_slot >> pa.hint_shift); ptomb[h] = ht;
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if (pe[h] >= 0) {
                atomicAdd(&s_agg[tid_x & 15], 1);
                pprio[h] = pa.eagg[pe[h]];   // asked for now: it travels while the block meets
            }
        }
        }
        __syncthreads();
        EVS_PT(3);
        const int agg = s_agg[tid_x & 15];
        // a missed key's claim: duplicate / victim / the CAS sent here, looked at behind the raises below (one round trip for both).
        // (Looked at behind the ROW requests instead -- the claim kept across them, block barriers that order LDS only -- was
        // built and measured on one box: 34.4 against 32.5 us per batch, the kernel sits at its 128 registers; the new rows as
        // predicated buffer stores instead of stores under an exec mask: 33.3.  The lean form of the first -- only the CAS's answer,
        // the victim's word and the way carried across the requests, a lost CAS re-reading its set: 128 registers, no spill --
        // measured EQUAL, 34.8-35.2 against 34.8-35.5 on its box: the CAS's round trip is not what the launch waits for.
        // tools/cache_lib_ab.sh)
        int uwon[2] = {-1, -1};
        unsigned uprev[2] = {0u, 0u};
        SaPick upk[2] = {{-1, 0, -1, 0u, 0u}, {-1, 0, -1, 0u, 0u}};
        bool uwait[2] = {false, false};
        if (ins) {
#pragma unroll
            for (int h = 0; h < 2; h++)
                if (pok[h] && pe[h] < 0) uwait[h] = sa_claim_issue(pa.sa, pa.pend_stamp, phint[h], ptag[h], agg, lw[h], upk[h], uprev[h], s_udelta);
        }
        EVS_PT(10);          // (the claims are ranked and sent)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = ((int)tid_x >> 4) + 16 * h;
            // monotone max like update_agg_hit; the plain read first keeps hot entries from serialising on one address
            if (pe[h] >= 0 && pprio[h] < agg) {
                int old;
                if (sa) old = sa_raise(pa.sa, sa_ways_ptr(pa.sa, phint[h]) + pway[h], (unsigned)pw0[h], agg);
                else { old = atomicMax(&pa.eagg[pe[h]], agg); old = old < agg ? old : -1; }
                if (old >= 0) { atomicSub(&s_pdelta[old], 1); atomicAdd(&s_pdelta[agg], 1); }
            }
            int v = -1;
            if (f == 0) v = bs < blk_end ? (int)bs : -1;                 // x: the sample number
            else if (pact[h]) v = pe[h] >= 0 ? (int)(0x40000000u | (unsigned)pe[h]) : (pok[h] ? prow[h] : -1);
            s_idx[(int)tid_x + 256 * h] = v;
            if (ins) {   // where the gathered row of a missed key goes (-1: nowhere)
                if (uwait[h]) uwon[h] = sa_claim_finish(pa.sa, pa.pend_stamp, phint[h], ptag[h], agg, lw[h], upk[h], uprev[h], s_udelta, s_ustat);
                s_idx[512 + (int)tid_x + 256 * h] = uwon[h];
            }
            if (pact[h]) {
                const int64_t m = bs * (int64_t)T + (f - 1);
                if (pa.hit) pa.hit[m] = pe[h] >= 0;
                if (pa.miss_rec != nullptr && pok[h] && pe[h] < 0) {
                    const int at = atomicAdd(&s_nlist, 1);
                    pa.miss_rec[(int64_t)blockIdx.x * pa.list_cap + at] =
                        make_uint4((unsigned)prow[h], (unsigned)(f - 1) | ((unsigned)agg << 8) | (ptomb[h] ? 0x10000u : 0u), phint[h], sa ? ptag[h] : (unsigned)m);
                }
            }
            if (f == 1 && bs < blk_end) { atomicAdd(&s_psum[0], agg); if (agg == T) atomicAdd(&s_psum[1], 1); }
        }
        EVS_PT(11);          // (raises done, claims looked at, the tile written)
        __syncthreads();
        EVS_PT(12);
        if (tid_x < 40) {   // the block's totals into one of the replica rows (folded by the cache's close)
            const int i = tid_x;
            const int v = i <= T ? s_pdelta[i] : i == 38 ? s_psum[0] : i == 39 ? s_psum[1] : 0;
            if (v) atomicAdd(&pa.part1[(blockIdx.x % 32) * 40 + i], v);
        }
        if (ins && tid_x < 40) {   // the inserts' totals, as the update kernels leave them (folded by the cache's close)
            const int i = tid_x;
            const int v = i <= T ? s_udelta[i] : i == 33 ? s_ustat[0] : i == 34 ? s_ustat[1] : 0;
            if (v) atomicAdd(&pa.part2[(blockIdx.x % 32) * 40 + i], v);
        }
        if (pa.list_cnt != nullptr && tid_x == 0) pa.list_cnt[blockIdx.x] = s_nlist;
        EVS_PTW(5);          // (everything the head has sent is answered; the head is over)
    } else {
        if (!stk) tile_load(0);
        tile_store(0);
        if constexpr (CHECK) {
            verify();
            if (__syncthreads_or(my_ragged)) {   // block-uniform, rare: this block's samples with general bag semantics
                slow_block();
                return;
            }
            bad |= fast_bad;
            EVS_PT(5);
        } else {
            __syncthreads();
        }
    }
    // scheduling barriers (EVS_RF_SB, developer A/B; bit 1: the four samples' requests leave in sample order, bit 0: the
    // stores of sample u - 1 leave inside iteration u).  Left alone, hipcc 7.2 interleaves the requests of samples 0 and 1
    // and sinks EVERY output store below the last MFMA of the last sample; pinned is 0.1-0.3 us faster at B = 16 384.
#ifndef EVS_RF_SB
#define EVS_RF_SB 3
#endif
#pragma unroll
    for (int u = 0; u < D; u++) {
        issue(u, ring[u]);      // (samples past the block's end: every lane reads the zero page)
        if constexpr ((EVS_RF_SB & 2) != 0) __builtin_amdgcn_sched_barrier(0);
    }
    float x_srv[SERVE ? D : 1][SERVE ? (d + 63) / 64 : 1];   // SERVE: x[b] once more, fresh from memory (rf_ld_*), asked for with the row requests
    if constexpr (SERVE) {
#pragma unroll
        for (int u = 0; u < D; u++) {
            const int64_t b = blk_first + wave_in_block + 4 * (int64_t)u;
#pragma unroll
            for (int h = 0; h < (d + 63) / 64; h++) {
                const int e = lane + 64 * h;
                const float *xp = (u < n_samples && e < d) ? sd.x + b * sd.x_stride + e : reinterpret_cast<const float *>(zeros_l);
                x_srv[u][h] = rf_ld_f32<true>(xp);
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);   // the scheduler would otherwise sink three of the four requests below the first consume
    // the lane-invariant staging / flush offsets: computed here, under the row requests' round trip, not in front of them
    // (16 waves per CU start in step: every instruction in front of the first load is paid by all of them at once)
    fill_stage();
    fill_flush();
    EVS_PT(6);               // (the row requests are out)
    const bool ins_blk = PROBE && args.probe.arena_w != nullptr;   // block-uniform: missed keys' rows go into the cache arena on the way
#pragma unroll
    for (int u = 0; u < D; u++) {
        const int64_t b = blk_first + wave_in_block + 4 * (int64_t)u;   // wave-uniform
        // the image of sample u: what the row DMA of the LDS loop would have left in the slot
#pragma unroll
        for (int j = 0; j < NJ; j++) *reinterpret_cast<f32x4 *>(my_lds + j * 1024 + lane * 16) = ring[u][j];
        if constexpr (SERVE) {   // row 0 of the image = x[b]: the copy that came through the agent-scope loads
#pragma unroll
            for (int h = 0; h < (d + 63) / 64; h++) {
                const int e = lane + 64 * h;
                if (e < d) reinterpret_cast<float *>(my_lds)[e] = x_srv[u][h];
            }
        }
        if constexpr (PROBE) {
            if (ins_blk) {   // the rows of the ways this block claimed: from the registers that gathered them into the arena
#pragma unroll
                for (int j = 0; j < NJ; j++) {
                    const int e = *reinterpret_cast<const int *>(reinterpret_cast<const char *>(s_idx) + 2048 + idx_lds[j] + 16 * u);
                    if (e >= 0)
                        *reinterpret_cast<f32x4 *>(args.probe.arena_w + (unsigned long long)(unsigned)e * (unsigned)row_bytes + (unsigned)dma_piece16) = ring[u][j];
                }
            }
        }
        float4 a[NR][CQ > 0 ? CQ : 1];
        float ar[NR][REM > 0 ? REM : 1];
#pragma unroll
        for (int rr = 0; rr < NR; rr++) {
#pragma unroll
            for (int c = 0; c < CQ; c++) a[rr][c] = *reinterpret_cast<const float4 *>(my_lds + lds_off[rr] + c * 16);
#pragma unroll
            for (int m = 0; m < REM; m++)
                ar[rr][m] = *reinterpret_cast<const float *>(my_lds + rem_off[rr] + m * 16);
        }
        float xv[(d + 63) / 64];   // x[b] is row 0 of the image
#pragma unroll
        for (int h = 0; h < (d + 63) / 64; h++) {
            const int e = lane + 64 * h;
            xv[h] = reinterpret_cast<const float *>(my_lds)[e < d ? e : 0];
        }
        flush_out(b - 4, u > 0 && u - 1 < n_samples);    // sample u-1 leaves under the MFMAs of sample u
        f32x4 c00, c10, c11;
        interact(a, ar, c00, c10, c11);
        if constexpr (MLP) my_out = s_out[wave_in_block + 4 * u];
        // never-stored elements go to a dump slot: behind the row, or (MLP) in a block of their own
        const int dump = MLP ? (int)(reinterpret_cast<char *>(&s_dump[wave_in_block * 16 + r16]) - reinterpret_cast<char *>(my_out))
                             : 4 * (OUT_MAX + r16);
        // stage the output row: x passthrough, then the packed lower triangle straight from the accumulators
        if constexpr (!MLP) {
#pragma unroll
            for (int h = 0; h < (d + 63) / 64; h++) *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + xv_off[h]) = xv[h];
#pragma unroll
            for (int v = 0; v < 4; v++) {
                *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo00h[v]) = c00[v];
                if constexpr (NT == 2) {
                    *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo10h[v]) = c10[v];
                    *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo11h[v]) = c11[v];
                }
            }
        } else {
#pragma unroll
        for (int h = 0; h < (d + 63) / 64; h++) {
            const int e = lane + 64 * h;
            *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + (e < d ? 4 * e : dump)) = xv[h];
        }
        if constexpr (MLP) {   // zero the padding columns [K, kp) of the GEMM operand
            if (lane < args.kp - out_row) my_out[out_row + lane] = 0.f;
        }
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const int i = 4 * q + v;
            const int zo00 = (i < F && r16 < i + itself) ? 4 * (d + (i * (i - 1 + 2 * itself)) / 2 + r16) : dump;
            *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo00) = c00[v];
            if constexpr (NT == 2) {
                const int gi = 16 + i;
                const int base = (gi * (gi - 1 + 2 * itself)) / 2;
                const int zo10 = gi < F ? 4 * (d + base + r16) : dump;
                const int zo11 = (gi < F && 16 + r16 < gi + itself) ? 4 * (d + base + 16 + r16) : dump;
                *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo10) = c10[v];
                *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo11) = c11[v];
            }
        }
        }
        if constexpr ((EVS_RF_SB & 1) != 0) __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (MLP) my_out = s_out[wave_in_block + 12];
    flush_out(blk_first + wave_in_block + 12, n_samples == 4);
    EVS_PT(8);               // (wave 0's last stores are out)
    EVS_PTW(9);              // (... and acknowledged)
    if (bad) atomicOr(LEAN ? lx.md->err : args.err, 1);
    if constexpr (MLP) {
        __syncthreads();   // the chunk's 16 staged rows are complete
        const int kp = args.kp, kq = kp >> 2, n1 = args.n1;
        const int n_tiles = (n1 + 15) >> 4;
        const float *arow = &s_out[r16][q * kq];                          // A: sample r16, k-slot q
        for (int nt = wave_in_block; nt < n_tiles; nt += 4) {
            const int n = 16 * nt + r16;
            const float *wrow = args.w1p + (size_t)n * kp + q * kq;       // B: output n, k-slot q (rows padded to 16 * n_tiles)
            // four accumulators, one per element of a 16-byte piece: each is an fma chain of kp / 4 terms, added at the end.  One chain
            // over all kp terms carries a running sum four times as large over four times as many steps; on same-sign data its median
            // error is 2.0 - 3.2 u sum |R||W| from kp = 160 on, the four chains' is below 1 (tests/test_gpu_mlp1_matrix.py)
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
            // software pipeline: the operand pieces of step group g + 1 (kPf steps of 4 MFMAs) are requested before the
            // MFMAs of group g issue -- W1 comes from L2 (~500 cycles), a load-use loop runs at 4 MFMAs per round trip
            // (measured at B = 16 384, n1 = 512: 229 -> 137 us; two tiles per wave sharing the A pieces: 195 us, dropped)
            constexpr int kPf = 5;
            const int nj = kq >> 2;                    // 16-byte pieces per k-slot
            f32x4 bq[kPf];
            float4 aq[kPf];
#pragma unroll
            for (int p = 0; p < kPf; p++) {
                const int j = p < nj ? p : 0;
                bq[p] = *reinterpret_cast<gf4_t>(reinterpret_cast<uintptr_t>(wrow + 4 * j));
                aq[p] = *reinterpret_cast<const float4 *>(arow + 4 * j);
            }
            for (int g = 0; g < nj; g += kPf) {
                f32x4 bc[kPf];
                float4 ac[kPf];
#pragma unroll
                for (int p = 0; p < kPf; p++) { bc[p] = bq[p]; ac[p] = aq[p]; }
#pragma unroll
                for (int p = 0; p < kPf; p++) {        // next group (clamped: the last group re-reads piece 0, unused)
                    const int j = g + kPf + p < nj ? g + kPf + p : 0;
                    bq[p] = *reinterpret_cast<gf4_t>(reinterpret_cast<uintptr_t>(wrow + 4 * j));
                    aq[p] = *reinterpret_cast<const float4 *>(arow + 4 * j);
                }
#pragma unroll
                for (int p = 0; p < kPf; p++) {
                    if (g + p < nj) {
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[p].x, bc[p][0], acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[p].y, bc[p][1], acc1, 0, 0, 0);
                        acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[p].z, bc[p][2], acc2, 0, 0, 0);
                        acc3 = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[p].w, bc[p][3], acc3, 0, 0, 0);
                    }
                }
            }
            const f32x4 acc = (acc0 + acc1) + (acc2 + acc3);
            const float bias = n < n1 ? args.b1[n] : 0.f;
#pragma unroll
            for (int v = 0; v < 4; v++) {   // lane holds Z1[sample 4q + v][output n]
                const int m = 4 * q + v;
                float z = acc[v] + bias;
                if (args.relu) z = z <= 0.f ? 0.f : z;   // NaN stays NaN, as torch.relu keeps it (z > 0 ? z : 0 would hide it)
                if (m < blk_n && n < n1) args.z1[(blk_first + m) * (int64_t)n1 + n] = z;
            }
        }
    }
}

}  // namespace evs
