// Fused embedding gather + pooling + pairwise-dot interaction on the gfx950 matrix cores.
//
// One kernel computes, per sample b,
//     R[b] = [ x[b] | Z[b][i][j], j<i ],   Z[b] = T[b].T[b]^T,   T[b] = [x[b]; V_0[b]; ...; V_{F-2}[b]]
// where every row of T[b] is either a DENSE feature (x from the bottom MLP, or pooled
// vectors that arrived over the all-to-all) or an INDIRECT feature: the sum-pooled bag
// of table rows that DLRM_Net.apply_emb would have produced
//     V_k[b] = sum_{j in bag(b)} decode(W_k[idx_k[j]]) (* w_k[idx_k[j]])
// (reference: dlrm_s_pytorch.py:407-461 apply_emb, :483-516 interact_features,
//  :588-601 sequential_forward calls them back to back).
// With all features dense this IS interact_features; with indirect features the
// (B,F,d) intermediate -- 2 x 3.7 KB of HBM traffic per sample at F=27, d=36 --
// never exists.
//
// Mapping (one wavefront per sample, NS samples in flight per wave):
//   Z for F <= 32 is a 2x2 grid of 16x16 tiles; only (0,0), (1,0), (1,1) are computed,
//   each as a chain of v_mfma_f32_16x16x4_f32 (exact fp32).  The MFMA sums over k in
//   groups of 4 "k-slots" q = lane>>4; the order of k is free as long as A and B agree,
//   so a row is cut into 16-byte CHUNKS of 4 elements and k-slot q owns chunks
//   [q*CPQ, (q+1)*CPQ), CPQ = ceil(d/16): lane (r = lane&15, q) fetches its rows' chunks
//   with aligned 16-byte loads (global_load_dwordx4) -- every byte of a row is fetched by
//   exactly one lane -- and MFMA step (c,e) multiplies element e of chunk q*CPQ+c across
//   the four q.  d=36: 9 chunks, CPQ=3, slot q=3 carries zeros (12 steps instead of 9;
//   the kernel is HBM-bound, MFMA has >2x headroom).
//   C/D layout: lane holds Z[i = 4*(lane>>4)+v][j = lane&15] -> row-major strict lower
//   triangle at R[b][d + i(i-1)/2 + j].
#include "evs_common.h"
#include <mutex>
#include "evs_fused.h"

#include <stdlib.h>

namespace evs {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// chunk = 4 consecutive elements of a row.  Reduced-precision chunks travel through the software
// pipeline RAW (bits parked in .x/.y of the float4 slot) and are decoded when the sample is
// consumed -- decoding at issue time would wait for the load and serialise the pipeline.
template <int CODEC>
__device__ __forceinline__ float4 load_raw(const char *row, int chunk) {
    if constexpr (CODEC == 32) {
        return reinterpret_cast<const float4 *>(row)[chunk];
    } else if constexpr (CODEC == 16) {
        const uint2 v = reinterpret_cast<const uint2 *>(row)[chunk];
        return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), 0.f, 0.f);
    } else if constexpr (CODEC == 8) {
        return make_float4(__uint_as_float(reinterpret_cast<const unsigned *>(row)[chunk]), 0.f, 0.f, 0.f);
    } else {
        return make_float4(__uint_as_float((unsigned)reinterpret_cast<const unsigned short *>(row)[chunk]), 0.f, 0.f, 0.f);
    }
}
template <int CODEC>
__device__ __forceinline__ float4 decode_raw(const float4 raw, const float *lut) {
    if constexpr (CODEC == 32) return raw;
    else return dec_chunk<CODEC>(__float_as_uint(raw.x), __float_as_uint(raw.y), lut);
}

// per-lane view of one row of T (one feature)
struct LaneFeat {
    const char *src;      // row base + this lane's k-slot byte offset folded in
    const int64_t *idx;   // indirect only
    const int64_t *off;   // indirect only
    const float *rw;      // WEIGHTED only
    unsigned scale;       // dense: row stride in BYTES; indirect: bytes per table row (0 for idle lanes)
    int rem_delta;        // byte distance from this lane's own chunks to the shared remainder chunks
    int nnz;              // API guarantees < 2^31
    unsigned n_rows;      // API guarantees < 2^31
    int off_len;          // readable offsets entries (>= B)
    int lane_off;         // this lane's k-slot byte offset inside a row (PTRS mode adds it to the row address)
    bool indirect;
};

typedef int i32x4 __attribute__((ext_vector_type(4)));

// Software pipeline over the samples a wave owns (sample n of the wave is b = wave_id + n*waves):
//   iteration k:  issue row loads of sample k+1   (its first index arrived during iteration k-1)
//                 issue index loads of sample k+2 (its offsets arrived during iteration k-1)
//                 issue offset loads of sample k+3
//                 consume sample k: finish its bags, the MFMA chains, write R[b]
// so the three dependent fetches (offset -> index -> row) of later samples are in flight
// under the MFMA/store phase of the current one.  All loads are unconditional: lanes with
// nothing to fetch (idle rows of the 16x16 tiles, empty bags) read a zero-filled buffer, so
// there is no select after the load and the vmcnt accounting stays static.  Stores go through
// a buffer resource sized to ONE output row: lanes whose (i,j) is outside the strict lower
// triangle carry an out-of-range offset and the hardware drops them -- no exec masking.
//
// k-slot assignment: a row has n_chunks = 4*CQ + REM 16-byte chunks.  Slot q owns chunks
// [q*CQ, (q+1)*CQ); the REM trailing chunks are fetched by all four slots (same cache line)
// and slot q uses element q of each.  d=36: CQ=2, REM=1 -> 9 MFMA steps per tile, no padding.
template <int CODEC, int CQ, int REM, int NT, bool WEIGHTED, bool HAS_INDIRECT, bool PTRS>
__global__ void __launch_bounds__(256) emb_interact_dot_kernel(const FusedArgs args) {
    constexpr int NR = NT;        // rows of T per lane: r16 and (NT==2) r16+16
    constexpr int NC = CQ + REM;  // float4 chunks held per lane per row
    const int lane = threadIdx.x & (kWave - 1);
    const int r16 = lane & 15;
    const int q = lane >> 4;
    const int F = args.F, itself = args.itself;
    constexpr int d = 4 * (4 * CQ + REM);
    const int out_row = d + args.P;
    const int64_t B = args.B;
    constexpr int kChunkBytes = CODEC / 2;  // 4 elements of CODEC bits
    constexpr int row_bytes = (4 * CQ + REM) * kChunkBytes;

    const FusedArgs *ka = (const FusedArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    LaneFeat lf[NR];
#pragma unroll
    for (int rr = 0; rr < NR; rr++) {
        const int f = r16 + 16 * rr;
        lf[rr].src = reinterpret_cast<const char *>(args.zeros);  // idle lanes read zeros
        lf[rr].idx = args.dummy_i64; lf[rr].off = args.dummy_i64; lf[rr].rw = nullptr;
        lf[rr].scale = 0; lf[rr].nnz = 0; lf[rr].n_rows = 0; lf[rr].indirect = false;
        lf[rr].off_len = (int)B;
        lf[rr].rem_delta = 4 * CQ * 16 - q * CQ * 16;
        lf[rr].lane_off = 0;
        if (f < F) {
            const int64_t *ip = ka->indices[f];
            lf[rr].indirect = HAS_INDIRECT && ip != nullptr;
            lf[rr].idx = lf[rr].indirect ? ip : args.dummy_i64;
            const int cb = lf[rr].indirect ? kChunkBytes : 16;
            lf[rr].lane_off = q * CQ * cb;
            lf[rr].src = reinterpret_cast<const char *>(ka->src[f]) + q * CQ * cb;
            lf[rr].rem_delta = 4 * CQ * cb - q * CQ * cb;
            lf[rr].off = lf[rr].indirect ? ka->offsets[f] : args.dummy_i64;
            if constexpr (WEIGHTED) lf[rr].rw = ka->row_w[f];
            lf[rr].scale = lf[rr].indirect ? (unsigned)row_bytes : (unsigned)(ka->stride[f] * 4);
            lf[rr].nnz = (int)ka->nnz[f];
            lf[rr].n_rows = (unsigned)ka->n_rows[f];
            lf[rr].off_len = lf[rr].indirect ? (int)ka->off_len[f] : (int)B;
        }
    }
    const char *zeros_l = reinterpret_cast<const char *>(args.zeros);

    // store offsets (bytes inside one output row); out-of-range = dropped by the buffer unit
    constexpr int kOob = 0x7ffffff0;
    int zo00[4], zo10[4], zo11[4];
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const int i = 4 * q + v;
        zo00[v] = (i < F && r16 < i + itself) ? 4 * (d + (i * (i - 1 + 2 * itself)) / 2 + r16) : kOob;
        const int gi = 16 + i;
        const int base = (gi * (gi - 1 + 2 * itself)) / 2;
        zo10[v] = (NT == 2 && gi < F) ? 4 * (d + base + r16) : kOob;
        zo11[v] = (NT == 2 && gi < F && 16 + r16 < gi + itself) ? 4 * (d + base + 16 + r16) : kOob;
    }

    __shared__ float s_lut[CodecLut<CODEC>::kEntries];
    if constexpr (CODEC != 32) {
        codec_lut_init<CODEC>(s_lut);
        __syncthreads();
    }

    // wave-uniform bookkeeping in SGPRs
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t waves_total = (int64_t)gridDim.x * 4;
    const int64_t wave_id = (int64_t)blockIdx.x * 4 + wave_in_block;
    if (wave_id >= B) return;
    const int n_samples = (int)((B - wave_id + waves_total - 1) / waves_total);
    bool bad = false;

    // ---- pipeline state (branch-free: every decision below is a select) ----------------
    struct Stage {                     // one sample whose rows are in flight / being consumed
        float4 a[NR][NC];
        int st[NR], len[NR];
        bool first[NR];                // first bag element valid
        float w[NR];                   // per-row weight of the first element (WEIGHTED)
    };
    int64_t off0[NR], off1[NR];        // raw offsets in flight
    int64_t idx_raw[NR];               // raw first index in flight
    int st2[NR], len2[NR];             // bag start/length of the sample whose index is in flight
    Stage sA, sB;

    // every offsets array (and the dummy, >= B entries) has two readable entries around any bag
    bool short_off = false;
#pragma unroll
    for (int rr = 0; rr < NR; rr++) short_off |= lf[rr].off_len < 2;
    const bool pair_ok = !__any(short_off);
    auto sample_b = [&](int n) -> int64_t {
        const int64_t b = wave_id + (int64_t)n * waves_total;
        return b < B ? b : B - 1;  // past-the-end pipeline slots re-read the last sample
    };
    auto issue_off = [&](int n) {
        if constexpr (HAS_INDIRECT) {
            const int b = (int)sample_b(n);
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {  // dense/idle lanes read a dummy offsets array
                if (pair_ok) {  // offsets[b], offsets[b+1] as ONE 16-byte load (the last bag reads [b-1], [b])
                    const bool has_next = b + 1 < lf[rr].off_len;
                    const longlong2 v = *reinterpret_cast<const longlong2 *>(lf[rr].off + (has_next ? b : b - 1));
                    off0[rr] = has_next ? v.x : v.y;
                    off1[rr] = v.y;
                } else {
                    off0[rr] = lf[rr].off[b];
                    off1[rr] = lf[rr].off[(b + 1 < lf[rr].off_len) ? b + 1 : b];
                }
            }
        }
    };
    auto issue_idx = [&](int n) {  // consumes off0/off1 -> st2/len2, issues the first-index load
        if constexpr (HAS_INDIRECT) {
            const int b = (int)sample_b(n);
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                const int64_t nnz = (int64_t)lf[rr].nnz;
                const int64_t s0 = off0[rr];
                const int64_t e0 = (b + 1 < lf[rr].off_len) ? off1[rr] : nnz;
                const bool valid = (s0 >= 0) & (e0 >= s0) & (e0 <= nnz);
                bad |= lf[rr].indirect & !valid;
                const bool use = lf[rr].indirect & valid;
                st2[rr] = use ? (int)s0 : 0;
                len2[rr] = use ? (int)(e0 - s0) : 0;
                const int64_t *ip = (len2[rr] > 0) ? lf[rr].idx + (PTRS ? (int64_t)st2[rr] * (F - 1) : (int64_t)st2[rr]) : args.dummy_i64;  // PTRS: (B, F-1) pointer table
                idx_raw[rr] = *ip;
            }
        }
    };
    auto issue_rows = [&](int n, Stage &S) {  // consumes idx_raw (sample n), issues its chunk loads
        const int64_t b = sample_b(n);
#pragma unroll
        for (int rr = 0; rr < NR; rr++) {
            unsigned mult = (unsigned)b;  // dense: sample number (B < 2^31 is checked on the host)
            bool ok = true;
            if constexpr (HAS_INDIRECT) {
                // PTRS: the "indices" are absolute row addresses (cache tier: arena or backing row); 0 = no row
                const bool in_range = PTRS ? idx_raw[rr] != 0 : (uint64_t)idx_raw[rr] < (uint64_t)lf[rr].n_rows;
                const bool has = len2[rr] > 0;
                if constexpr (!PTRS) bad |= lf[rr].indirect & has & !in_range;
                ok = !lf[rr].indirect | (has & in_range);
                mult = lf[rr].indirect ? (ok ? (unsigned)idx_raw[rr] : 0u) : mult;
                S.st[rr] = st2[rr];
                S.len[rr] = len2[rr];
            }
            S.first[rr] = ok;
            // one v_mad_u64_u32: base + u32*u32
            const char *row = lf[rr].src + (uint64_t)mult * (uint64_t)lf[rr].scale;
            if constexpr (PTRS) {
                if (lf[rr].indirect) row = reinterpret_cast<const char *>(idx_raw[rr]) + lf[rr].lane_off;
            }
            int rem_delta = lf[rr].rem_delta;
            if constexpr (HAS_INDIRECT && CODEC == 32) {  // empty bag / bad index: read zeros
                row = ok ? row : zeros_l;
                rem_delta = ok ? rem_delta : 0;
            }
            if constexpr (CODEC == 32 || !HAS_INDIRECT) {
#pragma unroll
                for (int c = 0; c < CQ; c++) S.a[rr][c] = reinterpret_cast<const float4 *>(row)[c];
#pragma unroll
                for (int m = 0; m < REM; m++) S.a[rr][CQ + m] = reinterpret_cast<const float4 *>(row + rem_delta)[m];
            } else {
                if (lf[rr].indirect) {
#pragma unroll
                    for (int c = 0; c < CQ; c++) S.a[rr][c] = load_raw<CODEC>(row, c);
#pragma unroll
                    for (int m = 0; m < REM; m++) S.a[rr][CQ + m] = load_raw<CODEC>(row + rem_delta, m);
                } else {
#pragma unroll
                    for (int c = 0; c < CQ; c++) S.a[rr][c] = reinterpret_cast<const float4 *>(row)[c];
#pragma unroll
                    for (int m = 0; m < REM; m++) S.a[rr][CQ + m] = reinterpret_cast<const float4 *>(row + rem_delta)[m];
                }
            }
            S.w[rr] = 1.0f;
            if constexpr (WEIGHTED) {
                const bool has_w = lf[rr].indirect && lf[rr].rw;
                const float *wp = has_w ? lf[rr].rw + mult : args.dummy_f32;
                const float wv = *wp;
                S.w[rr] = has_w ? wv : 1.0f;
            }
        }
    };

    const float *x_base = reinterpret_cast<const float *>(args.src[0]);
    const int64_t x_stride = args.stride[0];

    auto consume = [&](int k, Stage &S) {
        const int64_t b = wave_id + (int64_t)k * waves_total;  // wave-uniform
        // x passthrough: re-read x[b] (L1/L2 hit) with one lane per element, one store
        float xv[(d + 63) / 64];
#pragma unroll
        for (int h = 0; h < (d + 63) / 64; h++) {
            const int e = lane + 64 * h;
            xv[h] = x_base[b * x_stride + (e < d ? e : 0)];
        }
#pragma unroll
        for (int rr = 0; rr < NR; rr++)
#pragma unroll
            for (int c = 0; c < NC; c++) {
                if constexpr (HAS_INDIRECT && CODEC != 32) {  // decode now; dense lanes keep their fp32 chunk
                    const float4 dv = decode_raw<CODEC>(S.a[rr][c], s_lut);
                    if (lf[rr].indirect) S.a[rr][c] = S.first[rr] ? dv : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                if constexpr (WEIGHTED) {
                    S.a[rr][c].x = __fmul_rn(S.a[rr][c].x, S.w[rr]); S.a[rr][c].y = __fmul_rn(S.a[rr][c].y, S.w[rr]);
                    S.a[rr][c].z = __fmul_rn(S.a[rr][c].z, S.w[rr]); S.a[rr][c].w = __fmul_rn(S.a[rr][c].w, S.w[rr]);
                }
            }
        if constexpr (HAS_INDIRECT) {
            // bags longer than one index: remaining elements, in index order (not pipelined)
            bool more = false;
#pragma unroll
            for (int rr = 0; rr < NR; rr++) more |= S.len[rr] > 1;
            if (__any(more)) {
#pragma unroll
                for (int rr = 0; rr < NR; rr++) {
                    for (int j = 1; j < S.len[rr]; j++) {
                        const int64_t r = lf[rr].idx[S.st[rr] + j];
                        if ((uint64_t)r >= (uint64_t)lf[rr].n_rows) { bad = true; continue; }
                        const char *row = lf[rr].src + (uint64_t)(unsigned)r * (uint64_t)lf[rr].scale;
                        float w = 1.0f;
                        if constexpr (WEIGHTED) { if (lf[rr].rw) w = lf[rr].rw[r]; }
#pragma unroll
                        for (int c = 0; c < NC; c++) {
                            float4 t = decode_raw<CODEC>(c < CQ ? load_raw<CODEC>(row, c) : load_raw<CODEC>(row + lf[rr].rem_delta, c - CQ), s_lut);
                            if constexpr (WEIGHTED) {
                                t.x = __fmul_rn(t.x, w); t.y = __fmul_rn(t.y, w);
                                t.z = __fmul_rn(t.z, w); t.w = __fmul_rn(t.w, w);
                            }
                            S.a[rr][c].x = __fadd_rn(S.a[rr][c].x, t.x); S.a[rr][c].y = __fadd_rn(S.a[rr][c].y, t.y);
                            S.a[rr][c].z = __fadd_rn(S.a[rr][c].z, t.z); S.a[rr][c].w = __fadd_rn(S.a[rr][c].w, t.w);
                        }
                    }
                }
            }
        }

        f32x4 c00 = {0.f, 0.f, 0.f, 0.f}, c10 = {0.f, 0.f, 0.f, 0.f}, c11 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const float e0[4] = {S.a[0][c].x, S.a[0][c].y, S.a[0][c].z, S.a[0][c].w};
            const float e1[4] = {S.a[NR - 1][c].x, S.a[NR - 1][c].y, S.a[NR - 1][c].z, S.a[NR - 1][c].w};
            if (c < CQ) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0[e], e0[e], c00, 0, 0, 0);
                    if constexpr (NT == 2) {
                        c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1[e], e0[e], c10, 0, 0, 0);
                        c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1[e], e1[e], c11, 0, 0, 0);
                    }
                }
            } else {  // shared remainder chunk: k-slot q contributes its element q
                const float s0 = q == 0 ? e0[0] : q == 1 ? e0[1] : q == 2 ? e0[2] : e0[3];
                const float s1 = q == 0 ? e1[0] : q == 1 ? e1[1] : q == 2 ? e1[2] : e1[3];
                c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(s0, s0, c00, 0, 0, 0);
                if constexpr (NT == 2) {
                    c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1, s0, c10, 0, 0, 0);
                    c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1, s1, c11, 0, 0, 0);
                }
            }
        }
        // one buffer resource per output row: base = R + b*out_row (SGPRs), bounds = one row
        float *Rb = args.R + b * (int64_t)out_row;
#ifdef EVS_X_NOSTORE_REG
        if (c00[0] + c10[1] + c11[2] + c00[3] + c10[0] + c11[1] + c00[2] + c10[3] + c11[0] + c00[1] + c10[2] + c11[3] == 123.456f) Rb[lane] = xv[0];
        return;
#endif
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Rb, 0, out_row * 4, 0x00020000);
#pragma unroll
        for (int h = 0; h < (d + 63) / 64; h++) {
            const int e = lane + 64 * h;
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xv[h]), rs, e < d ? 4 * e : kOob, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; v++) {
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(c00[v]), rs, zo00[v], 0, 0);
            if constexpr (NT == 2) {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(c10[v]), rs, zo10[v], 0, 0);
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(c11[v]), rs, zo11[v], 0, 0);
            }
        }
    };

    // ---- prologue ---------------------------------------------------------------------
    issue_off(0);
    issue_idx(0);
    issue_off(1);
    issue_rows(0, sA);
    issue_idx(1);
    issue_off(2);

    // ---- steady state, unrolled by two so the row buffers ping-pong without copies ----
    for (int k = 0; k < n_samples; k += 2) {
        issue_rows(k + 1, sB);
        issue_idx(k + 2);
        issue_off(k + 3);
        consume(k, sA);
        if (k + 1 >= n_samples) break;
        issue_rows(k + 2, sA);
        issue_idx(k + 3);
        issue_off(k + 4);
        consume(k + 1, sB);
    }
    if (bad) atomicOr(args.err, 1);
}

// ------------------------------------------------------------------------------------------
// fp32 rows through LDS: the same computation, with the row fetch re-shaped for the memory pipe.
//
// In the kernel above each MFMA lane fetches ITS pieces of ITS rows: one wave-instruction touches
// 16 different rows (and the same lines again for the next piece) -- "fragment-shaped" loads that
// keep the texture addresser busy (SQ_WAIT_INST_ANY ~70 %, PMC in profiles/).  Here whole rows are
// moved by LDS-DMA (global_load_lds_dwordx4: per-lane SOURCE address, lane-linear 1 KiB LDS
// destination): d/4 consecutive lanes fetch one row as d*4 contiguous bytes, 64/(d/4) rows per
// instruction (7 for d=36), every cache line requested exactly once; the MFMA operands then come
// from LDS with ds_read_b128 (row stride 144 B: the 16 rows of a tile land on distinct banks).
// Row addresses are computed in the MFMA mapping (lane = row) and handed to the DMA mapping
// (lane = row piece) with one 64-bit shuffle per instruction.  The rows of sample k+1 are in
// flight into the wave's LDS slot while the MFMAs of sample k run; the row registers are
// single-buffered (24 VGPRs instead of 48), so more waves fit per SIMD.
//
// Output: the accumulator layout scatters a sample's packed triangle as 64-byte runs (12 store
// instructions, ~70 partial-line write requests per sample -- more L2 write requests than the
// whole gather has read requests; with them the kernel ran 94 us at B=65536, without any output
// 58 us).  The row is therefore staged in a second per-wave LDS slot (ds_write_b32 from the
// accumulators + the x passthrough copied from row 0 of the row slot) and leaves as contiguous
// 16-byte-per-lane buffer stores one iteration LATER, right after the top-of-loop wait and before
// the next sample's DMA is issued, so the write-acks overlap the MFMAs like the row fetch does
// (78 us).  Rows >= F of the 16*NT-row tile are never fetched (their products are never stored).
// ------------------------------------------------------------------------------------------
// BAG1: every indirect feature has exactly one index per bag and no offsets array (the Criteo collate,
// dlrm_data_pytorch.py:407-408: offsets = arange) -- the offsets stage of the pipeline disappears.
#ifndef EVS_LB
#define EVS_LB 4
#endif
// cache policy of the output stores: nt (2) -- R is written once and streams out; without it the 25 MB per
// launch push table rows out of the XCD L2s (measured 77.5 -> 75.1 us at B=65536; sc0 / sc1 do not help)
#ifndef EVS_OUT_CPOL
#define EVS_OUT_CPOL 2
#endif
#ifndef EVS_LB_GEN
#define EVS_LB_GEN 4
#endif
// resident blocks per CU the register allocator is asked to fit (more VGPRs per wave where the
// pipeline state or the decode temporaries would otherwise spill)
#ifndef EVS_LB_TILE
#define EVS_LB_TILE 5
#endif
template <int CODEC, int CQ, bool BAG1, bool TILE = false, bool CHECK = false>
constexpr int lds_min_blocks() {
    if (CHECK && CQ < 4) return 4;          // (bag starts / ends in flight + the slow loop: 110 VGPRs at d = 36)
    if (TILE && CQ < 4) return CQ < 3 ? EVS_LB_TILE : 4;   // (d = 48: the LDS slots allow 4 blocks)
    if (CQ >= 8) return 2;
    if (CQ >= 4) return 3;
    if (CODEC == 16) return 3;
    if (CODEC != 32 && !BAG1) return 3;
    return BAG1 ? EVS_LB : EVS_LB_GEN;
}
// CODEC != 32 (reduced-precision tables; feature 0 = x dense fp32, every other feature a table):
// the slot holds x in its first KiB (one 16-byte-per-lane DMA) and the ENCODED rows packed dword by
// dword behind it (4-byte-per-lane DMA: lane g of the phase moves dword g%RBd of table row g/RBd;
// u4 rows, 2-byte aligned, travel as their enclosing aligned dword window and the half-word phase
// rides along as a wave mask).  The MFMA operands are read as raw chunks (ds_read_u16/b32/b64) and
// decoded through the per-block LDS table (evs_common.h) -- x chunks overwrite row 0 afterwards.
// TILE (bag-1 tables): a block owns a CONTIGUOUS sample range and its 256 threads keep a
// [F-1][16] tile of the next 16 samples' indices in LDS (one 128-byte line per table and chunk, loaded one
// chunk ahead, two barriers per 4 iterations); the row stage reads its indices from there instead of one
// dependent 8-byte global load per lane.
// CHECK (with TILE, offsets given, whole batches: nnz == B): the block also loads the OFFSETS of every chunk and
// checks that each of its bags is exactly {idx[b]} (offsets[b] == b and the bag ends at b + 1).  The verdict is
// per chunk and block-wide (__syncthreads_or at the barrier the tile needs anyway); a block's results depend on
// its own bags only, so a chunk that fails the check sends THAT block -- from that chunk on -- into a slow
// in-kernel loop that pools its bags straight from global memory (general semantics: empty bags, several
// indices, bad offsets / indices skipped and flagged) and feeds the same MFMA + output code.  No flag, no second
// launch; the index errors a failed chunk's tile saw are dropped (they may sit at positions no bag refers to).
template <int CODEC, int CQ, int REM, int NT, bool WEIGHTED, bool HAS_INDIRECT, bool PTRS, bool BAG1, bool TILE = false, bool CHECK = false>
__global__ void __launch_bounds__(256, (lds_min_blocks<CODEC, CQ, BAG1, TILE, CHECK>())) emb_interact_dot_lds_kernel(const FusedArgs args) {
    static_assert(!CHECK || (TILE && CODEC == 32), "the offsets check rides on the index tiles; its slow loop pools fp32 rows");
    if constexpr (HAS_INDIRECT && !PTRS && !CHECK) {   // optimistic launches (see offsets_arange_kernel): the bag-1 loop runs
        if (args.opt_flag) {                             // when the offsets are arange, the general loop when they are not
            const bool ragged = *args.opt_flag == args.opt_id;
            if (BAG1 ? ragged : !ragged) return;
        }
    }
    constexpr int NR = NT;
    constexpr int NC = CQ + REM;
    constexpr int d = 4 * (4 * CQ + REM);
    constexpr int LPRD = d / 4;             // DMA lanes per fp32 row (16 B each)
    constexpr int RPI = 64 / LPRD;          // fp32 rows per DMA instruction
    constexpr int NROWS = 16 * NT;
    constexpr bool ENC = CODEC != 32;
    static_assert(!ENC || (HAS_INDIRECT && !PTRS), "encoded rows come from tables");
    constexpr int enc_row_bytes = d * CODEC / 8;
    // dwords DMA'd per encoded row (u4 rows that are not dword multiples: the aligned window around them)
    constexpr int RBd = (enc_row_bytes % 4 == 0) ? enc_row_bytes / 4 : (enc_row_bytes + 2 + 3) / 4;
    // ... moved in pieces of PB bytes per lane: 16 or 12 where the row is a whole number of them (gfx950 has the 12- and
    // 16-byte LDS DMA), else dword by dword.  A d = 36 u16 row is 6 lanes instead of 18, a u8 row 3 instead of 9: the
    // per-lane-addressed memory instructions per sample are what bounds this kernel (7.3 -> 2.4 for u16).
    constexpr int PB = !ENC ? 4 : (enc_row_bytes % 16 == 0 ? 16 : ((enc_row_bytes % 12 == 0 && CODEC != 4) ? 12 : 4));
    constexpr int RP = PB == 4 ? RBd : enc_row_bytes / PB;   // pieces per row
    // (measured on gfx950: the 12-byte DMA lays its lanes down 16 bytes apart -- dword i of a row sits at 4 i + 4 (i / 3))
    constexpr int PS = PB == 12 ? 16 : PB;                   // LDS bytes between the pieces of neighbouring lanes
    constexpr int kEncRowLds = PB == 4 ? RBd * 4 : RP * PS;  // LDS bytes per encoded row
    constexpr int NI2 = ((NROWS - 1) * RP + 63) / 64;
    constexpr int kEncBase = 1024;          // encoded rows start behind the x KiB
    constexpr int kChunkBytes = CODEC / 2;  // 4 elements
    constexpr int NINSTR = ENC ? 1 + (NI2 * 64 * PS + 1023) / 1024 : (NROWS + RPI - 1) / RPI;   // slot size in KiB
    constexpr int row_bytes = ENC ? enc_row_bytes : d * 4;
    static_assert(!TILE || (BAG1 && HAS_INDIRECT && !PTRS && !WEIGHTED), "index tiles: plain bag-1 tables");
    // TILE launches have F <= kTileMaxF: rows past that are never fetched (nor their products stored), and the
    // slot KiB they would take pays for the index tile -- 5 blocks per CU stay resident
    constexpr int kTileSlot = (kTileMaxF + RPI - 1) / RPI;
    constexpr int NSLOT = (TILE && !ENC && kTileSlot < NINSTR) ? kTileSlot : NINSTR;
    __shared__ __attribute__((aligned(16))) char s_rows[4][NSLOT * 1024];
    __shared__ int s_idx[TILE ? 2 * 512 : 1];
    __shared__ const int64_t *s_tile_p[TILE ? 32 : 1];   // per table: index array / row count (kept out of the VGPRs)
    __shared__ unsigned s_tile_nr[TILE ? 32 : 1];
    __shared__ const int64_t *s_tile_o[CHECK ? 32 : 1];  // CHECK: offsets arrays, their readable entries
    __shared__ int s_tile_ol[CHECK ? 32 : 1];
    __shared__ float s_lut[CodecLut<CODEC>::kEntries];
    if constexpr (ENC) {
        codec_lut_init<CODEC>(s_lut);
        __syncthreads();
    }
    // output row of one sample (x passthrough + packed triangle), staged so it leaves as contiguous stores
    constexpr int OUT_MAX = ((d + NROWS * (NROWS + 1) / 2 + 63) / 64) * 64;
    __shared__ __attribute__((aligned(16))) float s_out[4][OUT_MAX + 16];

    const int lane = threadIdx.x & (kWave - 1);
    const int r16 = lane & 15;
    const int q = lane >> 4;
    const int F = args.F, itself = args.itself;
    const int out_row = d + args.P;
    const int64_t B = args.B;

    const FusedArgs *ka = (const FusedArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    LaneFeat lf[NR];
#pragma unroll
    for (int rr = 0; rr < NR; rr++) {
        const int f = r16 + 16 * rr;
        lf[rr].src = reinterpret_cast<const char *>(args.zeros);
        lf[rr].idx = args.dummy_i64; lf[rr].off = args.dummy_i64; lf[rr].rw = nullptr;
        lf[rr].scale = 0; lf[rr].nnz = 0; lf[rr].n_rows = 0; lf[rr].indirect = false;
        lf[rr].off_len = (int)B; lf[rr].rem_delta = 0; lf[rr].lane_off = 0;
        if (f < F) {
            const int64_t *ip = ka->indices[f];
            lf[rr].indirect = HAS_INDIRECT && ip != nullptr;
            lf[rr].idx = lf[rr].indirect ? ip : args.dummy_i64;
            lf[rr].src = reinterpret_cast<const char *>(ka->src[f]);
            lf[rr].off = lf[rr].indirect ? ka->offsets[f] : args.dummy_i64;
            if constexpr (WEIGHTED) lf[rr].rw = ka->row_w[f];
            lf[rr].scale = lf[rr].indirect ? (unsigned)row_bytes : (unsigned)(ka->stride[f] * 4);
            lf[rr].nnz = (int)ka->nnz[f];
            lf[rr].n_rows = (unsigned)ka->n_rows[f];
            lf[rr].off_len = lf[rr].indirect ? (int)ka->off_len[f] : (int)B;
        }
    }
    const char *zeros_l = reinterpret_cast<const char *>(args.zeros);

    // DMA mapping of this lane: for instruction j it moves piece dma_piece of row j*RPI + lane/LPRD
    const int dma_piece = lane % LPRD;
    constexpr int NDMA = ENC ? 1 : NSLOT;
    int dma_src[NDMA];     // lane that holds the row address in the MFMA mapping, or -1
#pragma unroll
    for (int j = 0; j < NDMA; j++) {
        const int row = j * RPI + lane / LPRD;
        dma_src[j] = (lane < RPI * LPRD && row < NROWS) ? (row & 15) + 16 * (row >> 4) : -1;
    }
    // LDS byte offset of this lane's operand chunks (row r16 + 16*rr): block + row-in-block + chunk
    int lds_off[NR];
#pragma unroll
    for (int rr = 0; rr < NR; rr++) {
        const int row = r16 + 16 * rr;
        if constexpr (ENC && PB == 12) lds_off[rr] = kEncBase + (row > 0 ? row - 1 : 0) * kEncRowLds;   // (chunk offsets: below)
        else if constexpr (ENC) lds_off[rr] = kEncBase + (row > 0 ? row - 1 : 0) * kEncRowLds + q * CQ * kChunkBytes;
        else lds_off[rr] = (row / RPI) * 1024 + (row % RPI) * row_bytes + q * CQ * 16;
    }
    constexpr int kRemOff = 4 * CQ * (ENC ? kChunkBytes : 16);  // from the row start

    constexpr int kOob = 0x7ffffff0;
    int zo00[4], zo10[4], zo11[4];
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const int i = 4 * q + v;
        zo00[v] = (i < F && r16 < i + itself) ? 4 * (d + (i * (i - 1 + 2 * itself)) / 2 + r16) : kOob;
        const int gi = 16 + i;
        const int base = (gi * (gi - 1 + 2 * itself)) / 2;
        zo10[v] = (NT == 2 && gi < F) ? 4 * (d + base + r16) : kOob;
        zo11[v] = (NT == 2 && gi < F && 16 + r16 < gi + itself) ? 4 * (d + base + 16 + r16) : kOob;
    }

    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    char *my_lds = s_rows[wave_in_block];
    float *my_out = s_out[wave_in_block];
#pragma unroll
    for (int v = 0; v < 4; v++) {  // never-stored elements go to a dump slot past the row
        zo00[v] = zo00[v] == kOob ? 4 * (OUT_MAX + r16) : zo00[v];
        zo10[v] = zo10[v] == kOob ? 4 * (OUT_MAX + r16) : zo10[v];
        zo11[v] = zo11[v] == kOob ? 4 * (OUT_MAX + r16) : zo11[v];
    }
    auto flush_out = [&](int64_t bp) {
        float *Rb = args.R + bp * (int64_t)out_row;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Rb, 0, out_row * 4, 0x00020000);
        const int n4 = out_row >> 2;   // whole 16-byte pieces; the 0..3 trailing floats go as dwords
#pragma unroll
        for (int h = 0; h < (OUT_MAX + 255) / 256; h++) {
            if (h * 64 < n4) {
                const int e4 = lane + 64 * h;
                const float4 v = reinterpret_cast<const float4 *>(my_out)[e4 < n4 ? e4 : 0];
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                u32x4 u = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
                __builtin_amdgcn_raw_buffer_store_b128(u, rs, e4 < n4 ? 16 * e4 : kOob, 0, EVS_OUT_CPOL);
            }
        }
        if (out_row & 3) {
            const int e = 4 * n4 + (lane & 3);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(my_out[e]), rs, lane < (out_row & 3) ? 4 * e : kOob, 0, EVS_OUT_CPOL);
        }
    };
    bool bad = false;
    // sample n of this wave is b = wave_id + n * wave_step: strided over the grid, or (TILE) over the block's range
    int64_t waves_total = (int64_t)gridDim.x * 4;
    int64_t wave_id = (int64_t)blockIdx.x * 4 + wave_in_block;
    int n_samples, k_end;
    int64_t blk_first = 0, blk_end = 0;
    if constexpr (TILE) {
        const int64_t per = args.tile_per;
        blk_first = (int64_t)blockIdx.x * per;
        blk_end = blk_first + per < B ? blk_first + per : B;
        if (blk_first >= blk_end) return;       // block-uniform
        const int blk_n = (int)(blk_end - blk_first);
        wave_id = blk_first + wave_in_block;
        waves_total = 4;
        n_samples = blk_n > wave_in_block ? (blk_n - wave_in_block + 3) / 4 : 0;
        k_end = (blk_n + 3) / 4;                // every wave walks the block's iterations (barriers)
    } else {
        if (wave_id >= B) return;
        n_samples = (int)((B - wave_id + waves_total - 1) / waves_total);
        k_end = n_samples;
    }
    int64_t off0[NR], off1[NR];
    int64_t idx_raw[NR];
    // per-feature bag facts travel through the pipeline as wave masks (SGPRs), not per-lane registers:
    // has = bag non-empty, more = bag longer than one index (the rare path re-reads its offsets)
    unsigned long long has2[NR], more2[NR], more1[NR];
    unsigned long long ok1[NR], sub1[NR];   // ENC: row present (else it decodes as zeros); u4 half-word phase
    float w1[NR];


    // every offsets array (and the dummy, >= B entries) has two readable entries around any bag
    bool short_off = false;
#pragma unroll
    for (int rr = 0; rr < NR; rr++) short_off |= lf[rr].off_len < 2;
    const bool pair_ok = !__any(short_off);
    auto sample_b = [&](int n) -> int64_t {
        const int64_t b = wave_id + (int64_t)n * waves_total;
        if constexpr (TILE) return b < blk_end ? b : blk_end - 1;
        return b < B ? b : B - 1;
    };
    // TILE: thread e (and e + 256) of the block owns tile element (table e >> 4, sample-in-chunk e & 15)
    int64_t tile_v[2] = {0, 0};
    int64_t tile_o[2] = {0, 0}, tile_e[2] = {0, 0};
    bool ragged_seen = false, bad_tile = false;
    int fallback_from = 0x7fffffff;   // CHECK: first iteration (of every wave of the block) that runs the slow loop
    int tile_off[NR];
    if constexpr (TILE) {
        if (threadIdx.x < 32) {
            const int f = 1 + (int)threadIdx.x;
            s_tile_p[threadIdx.x] = f < F ? ka->indices[f] : nullptr;
            s_tile_nr[threadIdx.x] = f < F ? (unsigned)ka->n_rows[f] : 0u;
            if constexpr (CHECK) {
                s_tile_o[threadIdx.x] = (f < F && ka->indices[f]) ? ka->offsets[f] : nullptr;
                s_tile_ol[threadIdx.x] = f < F ? (int)ka->off_len[f] : 0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < NR; rr++) {
            const int f = r16 + 16 * rr;
            tile_off[rr] = (f >= 1 && f < F ? f - 1 : 0) * 16 + wave_in_block;
        }
    }
    auto tile_load = [&](int c) {       // chunk c of the block -> registers
        if constexpr (TILE) {
            const int64_t bs = blk_first + 16 * (int64_t)c + (threadIdx.x & 15);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                tile_v[h] = -1;
                const int64_t *tp = s_tile_p[((int)threadIdx.x >> 4) + 16 * h];
                if (tp && bs < blk_end) tile_v[h] = tp[bs];
                if constexpr (CHECK) {   // start and end of bag bs (the last bag of a B-entry array ends at nnz == B)
                    tile_o[h] = bs; tile_e[h] = bs + 1;
                    if (tp && bs < blk_end) {
                        const int64_t *op = s_tile_o[((int)threadIdx.x >> 4) + 16 * h];
                        tile_o[h] = op[bs];
                        if (bs + 1 < s_tile_ol[((int)threadIdx.x >> 4) + 16 * h]) tile_e[h] = op[bs + 1];
                    }
                }
            }
        }
    };
    auto tile_store = [&](int c) {      // registers -> tile buffer c & 1 (row ids as int32, -1 = none / out of range)
        if constexpr (TILE) {
            const int64_t bs = blk_first + 16 * (int64_t)c + (threadIdx.x & 15);
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const bool live = s_tile_p[((int)threadIdx.x >> 4) + 16 * h] != nullptr && bs < blk_end;
                const bool in_range = (uint64_t)tile_v[h] < (uint64_t)s_tile_nr[((int)threadIdx.x >> 4) + 16 * h];
                if constexpr (CHECK) {
                    bad_tile |= live & !in_range;
                    ragged_seen |= (tile_o[h] != bs) | (tile_e[h] != bs + 1);
                } else {
                    bad |= live & !in_range;
                }
                s_idx[(c & 1) * 512 + (int)threadIdx.x + 256 * h] = (live & in_range) ? (int)tile_v[h] : -1;
            }
        }
    };
    auto issue_off = [&](int n) {
        if constexpr (HAS_INDIRECT && !BAG1) {
            const int b = (int)sample_b(n);
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {  // dense/idle lanes read a dummy offsets array
                if (pair_ok) {  // offsets[b], offsets[b+1] as ONE 16-byte load (the last bag reads [b-1], [b])
                    const bool has_next = b + 1 < lf[rr].off_len;
                    const longlong2 v = *reinterpret_cast<const longlong2 *>(lf[rr].off + (has_next ? b : b - 1));
                    off0[rr] = has_next ? v.x : v.y;
                    off1[rr] = v.y;
                } else {
                    off0[rr] = lf[rr].off[b];
                    off1[rr] = lf[rr].off[(b + 1 < lf[rr].off_len) ? b + 1 : b];
                }
            }
        }
    };
    auto issue_idx = [&](int n) {
        if constexpr (TILE) {
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                has2[rr] = __ballot(lf[rr].indirect);
                more2[rr] = 0;
                idx_raw[rr] = s_idx[((n >> 2) & 1) * 512 + tile_off[rr] + 4 * (n & 3)];
            }
        } else if constexpr (HAS_INDIRECT && BAG1) {
            const int b = (int)sample_b(n);
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                has2[rr] = __ballot(lf[rr].indirect);
                more2[rr] = 0;
                // PTRS: the (B, F-1) pointer table of the cache tier, feature f at column f-1
                idx_raw[rr] = lf[rr].idx[lf[rr].indirect ? (PTRS ? (int64_t)b * (F - 1) : (int64_t)b) : 0];

            }
        } else if constexpr (HAS_INDIRECT) {
            const int b = (int)sample_b(n);
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                const int64_t nnz = (int64_t)lf[rr].nnz;
                const int64_t s0 = off0[rr];
                const int64_t e0 = (b + 1 < lf[rr].off_len) ? off1[rr] : nnz;
                const bool valid = (s0 >= 0) & (e0 >= s0) & (e0 <= nnz);
                bad |= lf[rr].indirect & !valid;
                const bool use = lf[rr].indirect & valid;
                const int len = use ? (int)(e0 - s0) : 0;
                has2[rr] = __ballot(len > 0);
                more2[rr] = __ballot(len > 1);
                const int64_t *ip = (len > 0) ? lf[rr].idx + (int)s0 : args.dummy_i64;
                idx_raw[rr] = *ip;
            }
        }
    };
    // row addresses of sample n in the MFMA mapping, then the DMA of all its rows into this wave's LDS slot
    auto issue_rows = [&](int n) {
        const int64_t b = sample_b(n);
        const char *rowp[NR];
#pragma unroll
        for (int rr = 0; rr < NR; rr++) {
            unsigned mult = (unsigned)b;
            bool ok = true;
            if constexpr (HAS_INDIRECT) {
                const bool in_range = TILE ? idx_raw[rr] >= 0 : PTRS ? idx_raw[rr] != 0 : (uint64_t)idx_raw[rr] < (uint64_t)lf[rr].n_rows;
                const bool has = (has2[rr] >> lane) & 1;
                if constexpr (!PTRS && !TILE) bad |= lf[rr].indirect & has & !in_range;   // (TILE: checked by tile_store)
                ok = !lf[rr].indirect | (has & in_range);
                mult = lf[rr].indirect ? (ok ? (unsigned)idx_raw[rr] : 0u) : mult;
                more1[rr] = more2[rr];
            }
            const char *row = lf[rr].src + (uint64_t)mult * (uint64_t)lf[rr].scale;
            if constexpr (PTRS) {
                if (lf[rr].indirect) row = reinterpret_cast<const char *>(idx_raw[rr]);
            }
            rowp[rr] = ok ? row : zeros_l;
            if constexpr (ENC) {
                ok1[rr] = __ballot(ok);
                const bool odd = lf[rr].indirect & ok & (((uintptr_t)row & 2u) != 0);
                sub1[rr] = __ballot(odd);
                if (lf[rr].indirect) rowp[rr] = reinterpret_cast<const char *>((uintptr_t)rowp[rr] & ~(uintptr_t)3);
            }
            w1[rr] = 1.0f;
            if constexpr (WEIGHTED) {
                const bool has_w = lf[rr].indirect && lf[rr].rw;
                const float *wp = has_w ? lf[rr].rw + mult : args.dummy_f32;
                const float wv = *wp;
                w1[rr] = has_w ? wv : 1.0f;
            }
        }
        // lanes of k-slot q publish the address of tile-row set q (rows 16q..16q+15)
        unsigned long long pub = (unsigned long long)rowp[0];
        if constexpr (NR == 2) pub = (q == 1) ? (unsigned long long)rowp[1] : pub;
        if constexpr (ENC) {
            {   // x: lanes 0..LPRD-1 move its d*4 bytes, the others park zeros behind it
                const unsigned long long p = __shfl(pub, 0);
                const char *g = lane < LPRD ? reinterpret_cast<const char *>(p) + lane * 16 : zeros_l;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                                 (__attribute__((address_space(3))) void *)my_lds, 16, 0, 0);
            }
            const int n_dw = (F - 1) * RP;
#pragma unroll
            for (int j = 0; j < NI2; j++) {
                if (j * 64 >= n_dw) break;
                const int gidx = j * 64 + lane;
                const int f = 1 + gidx / RP;
                const int w = gidx - (f - 1) * RP;
                const bool on = gidx < n_dw;
                const unsigned long long p = __shfl(pub, on ? (f & 15) + 16 * (f >> 4) : 0);
                const char *g = on ? reinterpret_cast<const char *>(p) + PB * w : zeros_l;
                const auto gp = (const __attribute__((address_space(1))) void *)g;
                const auto lp = (__attribute__((address_space(3))) void *)(my_lds + kEncBase + j * 64 * PS);
                // (the builtin wants a literal size)
                if constexpr (PB == 16) __builtin_amdgcn_global_load_lds(gp, lp, 16, 0, 0);
                else if constexpr (PB == 12) __builtin_amdgcn_global_load_lds(gp, lp, 12, 0, 0);
                else __builtin_amdgcn_global_load_lds(gp, lp, 4, 0, 0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NDMA; j++) {
                if (j * RPI >= F) break;   // rows >= F only feed accumulator elements that are never stored
                const unsigned long long p = __shfl(pub, dma_src[j] < 0 ? 0 : dma_src[j]);
                const char *g = dma_src[j] < 0 ? zeros_l : reinterpret_cast<const char *>(p) + dma_piece * 16;
#ifdef EVS_X_NODMA   // developer A/B: everything but the row fetch (the slot keeps whatever it holds)
                if (g == reinterpret_cast<const char *>(0x1234)) args.R[lane] = 1.f;
                continue;
#endif
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                                 (__attribute__((address_space(3))) void *)(my_lds + j * 1024), 16, 0, 0);
            }
        }
    };

    // the interaction of one sample (operands in the MFMA layout) and the staging of its output row
    auto interact = [&](const float4 (&a)[NR][NC], f32x4 &c00, f32x4 &c10, f32x4 &c11) {
#ifdef EVS_X_NOMFMA   // developer A/B: the matrix-core work replaced by three adds per operand chunk
        c00 = f32x4{0.f, 0.f, 0.f, 0.f}; c10 = c00; c11 = c00;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            c00[c & 3] += a[0][c].x + a[0][c].y; c10[c & 3] += a[NR - 1][c].z; c11[c & 3] += a[NR - 1][c].w + a[0][c].z;
        }
        return;
#endif
        c00 = f32x4{0.f, 0.f, 0.f, 0.f}; c10 = f32x4{0.f, 0.f, 0.f, 0.f}; c11 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const float e0[4] = {a[0][c].x, a[0][c].y, a[0][c].z, a[0][c].w};
            const float e1[4] = {a[NR - 1][c].x, a[NR - 1][c].y, a[NR - 1][c].z, a[NR - 1][c].w};
            if (c < CQ) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(e0[e], e0[e], c00, 0, 0, 0);
                    if constexpr (NT == 2) {
                        c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1[e], e0[e], c10, 0, 0, 0);
                        c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(e1[e], e1[e], c11, 0, 0, 0);
                    }
                }
            } else {
                const float s0 = q == 0 ? e0[0] : q == 1 ? e0[1] : q == 2 ? e0[2] : e0[3];
                const float s1 = q == 0 ? e1[0] : q == 1 ? e1[1] : q == 2 ? e1[2] : e1[3];
                c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(s0, s0, c00, 0, 0, 0);
                if constexpr (NT == 2) {
                    c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1, s0, c10, 0, 0, 0);
                    c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1, s1, c11, 0, 0, 0);
                }
            }
        }
    };
    auto stage_row = [&](const float (&xv)[(d + 63) / 64], const f32x4 &c00, const f32x4 &c10, const f32x4 &c11) {
        // stage the output row: x passthrough, then the packed lower triangle straight from the accumulators
#pragma unroll
        for (int h = 0; h < (d + 63) / 64; h++) {
            const int e = lane + 64 * h;
            my_out[e < d ? e : OUT_MAX + r16] = xv[h];
        }
#pragma unroll
        for (int v = 0; v < 4; v++) {
            *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo00[v]) = c00[v];
            if constexpr (NT == 2) {
                *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo10[v]) = c10[v];
                *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + zo11[v]) = c11[v];
            }
        }
    };
    // ---- prologue ---------------------------------------------------------------------
    if constexpr (TILE) {
        tile_load(0);
        tile_store(0);
        tile_load(1);
        if constexpr (CHECK) {
            if (__syncthreads_or(ragged_seen)) fallback_from = 0; else bad |= bad_tile;
            ragged_seen = false; bad_tile = false;
        } else {
            __syncthreads();
        }
    }
    issue_off(0);
    issue_idx(0);
    issue_off(1);
    if (!CHECK || fallback_from > 0) issue_rows(0);
    issue_idx(1);
    issue_off(2);

    for (int k = 0; k < k_end; k++) {
        const int64_t b = wave_id + (int64_t)k * waves_total;  // wave-uniform
        // rows of sample k have landed once every outstanding vector-memory op has retired
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if constexpr (CHECK) {
            if (k >= fallback_from) break;   // block-uniform: the rest of this block's samples take the slow loop below
        }
        if constexpr (TILE) {
            if ((k & 3) == 0) {   // chunk k/4 + 1 (in registers since the last turn) replaces chunk k/4 - 1
                __syncthreads();
                tile_store((k >> 2) + 1);
                if constexpr (CHECK) {   // (block-uniform: every wave leaves the tile protocol at the same iteration)
                    if (__syncthreads_or(ragged_seen)) fallback_from = k + 4; else bad |= bad_tile;
                    ragged_seen = false; bad_tile = false;
                    if (fallback_from == 0x7fffffff) tile_load((k >> 2) + 2);
                } else {
                    __syncthreads();
                    tile_load((k >> 2) + 2);
                }
            }
            if (k >= n_samples) continue;
        }

        float4 a[NR][NC];
        if constexpr (ENC) {
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
                const int sub = (int)((sub1[rr] >> lane) & 1) * 2;
                const bool present = (ok1[rr] >> lane) & 1;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    const char *cp = my_lds + lds_off[rr] + sub +
                                     (c < CQ ? c * kChunkBytes : -q * CQ * kChunkBytes + kRemOff + (c - CQ) * kChunkBytes);
                    unsigned w0 = 0, w1r = 0;
                    if constexpr (PB == 12) {   // 12 bytes in every 16: the chunk's dwords one by one
                        static_assert(PB != 12 || CODEC == 16 || CODEC == 8, "12-byte pieces: whole-dword chunks");
                        const int ch = c < CQ ? q * CQ + c : 4 * CQ + (c - CQ);
                        const int i0 = ch * (kChunkBytes / 4);
                        const char *rp = my_lds + lds_off[rr];
                        w0 = *reinterpret_cast<const unsigned *>(rp + 4 * i0 + 4 * (i0 / 3));
                        if constexpr (CODEC == 16) w1r = *reinterpret_cast<const unsigned *>(rp + 4 * (i0 + 1) + 4 * ((i0 + 1) / 3));
                    }
                    else if constexpr (CODEC == 16) { const uint2 v = *reinterpret_cast<const uint2 *>(cp); w0 = v.x; w1r = v.y; }
                    else if constexpr (CODEC == 8) w0 = *reinterpret_cast<const unsigned *>(cp);
                    else w0 = *reinterpret_cast<const unsigned short *>(cp);
                    const float4 dv = dec_chunk<CODEC>(w0, w1r, s_lut);
                    a[rr][c] = present ? dv : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            if (r16 == 0) {   // row 0 is x: plain fp32 chunks from the first KiB
#pragma unroll
                for (int c = 0; c < NC; c++)
                    a[0][c] = *reinterpret_cast<const float4 *>(my_lds + (c < CQ ? (q * CQ + c) * 16 : 4 * CQ * 16 + (c - CQ) * 16));
            }
        } else {
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
#pragma unroll
                for (int c = 0; c < CQ; c++) a[rr][c] = *reinterpret_cast<const float4 *>(my_lds + lds_off[rr] + c * 16);
#pragma unroll
                for (int m = 0; m < REM; m++)
                    a[rr][CQ + m] = *reinterpret_cast<const float4 *>(my_lds + lds_off[rr] - q * CQ * 16 + kRemOff + m * 16);
            }
        }
        unsigned long long more0[NR];
        float w0[NR];
#pragma unroll
        for (int rr = 0; rr < NR; rr++) { more0[rr] = HAS_INDIRECT ? more1[rr] : 0; w0[rr] = w1[rr]; }
        // the LDS slot is free again once the reads above have returned
        float xv[(d + 63) / 64];   // x[b] is row 0 of the slot
#pragma unroll
        for (int h = 0; h < (d + 63) / 64; h++) {
            const int e = lane + 64 * h;
            xv[h] = reinterpret_cast<const float *>(my_lds)[e < d ? e : 0];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (k > 0) flush_out(b - waves_total);   // sample k-1 leaves while sample k+1 arrives
        if (k + 1 < n_samples && (!CHECK || k + 1 < fallback_from)) issue_rows(k + 1);
        issue_idx(k + 2);
        issue_off(k + 3);
        if constexpr (WEIGHTED) {
#pragma unroll
            for (int rr = 0; rr < NR; rr++)
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    a[rr][c].x = __fmul_rn(a[rr][c].x, w0[rr]); a[rr][c].y = __fmul_rn(a[rr][c].y, w0[rr]);
                    a[rr][c].z = __fmul_rn(a[rr][c].z, w0[rr]); a[rr][c].w = __fmul_rn(a[rr][c].w, w0[rr]);
                }
        }
        if constexpr (HAS_INDIRECT && !PTRS && !BAG1) {
            if ((more0[0] | more0[NR - 1]) != 0) {  // bags longer than one index: remaining elements, in index order
#pragma unroll
                for (int rr = 0; rr < NR; rr++) {
                    int64_t s0 = 0, e0 = 0;
                    if ((more0[rr] >> lane) & 1) {  // offsets were validated when the mask was built
                        s0 = lf[rr].off[b];
                        e0 = (b + 1 < lf[rr].off_len) ? lf[rr].off[b + 1] : (int64_t)lf[rr].nnz;
                    }
                    for (int64_t j = s0 + 1; j < e0; j++) {
                        const int64_t r = lf[rr].idx[j];
                        if ((uint64_t)r >= (uint64_t)lf[rr].n_rows) { bad = true; continue; }
                        const char *row = lf[rr].src + (uint64_t)(unsigned)r * (uint64_t)lf[rr].scale + q * CQ * (ENC ? kChunkBytes : 16);
                        float w = 1.0f;
                        if constexpr (WEIGHTED) { if (lf[rr].rw) w = lf[rr].rw[r]; }
#pragma unroll
                        for (int c = 0; c < NC; c++) {
                            float4 t = decode_raw<CODEC>(c < CQ ? load_raw<CODEC>(row, c)
                                                                : load_raw<CODEC>(row - q * CQ * (ENC ? kChunkBytes : 16) + kRemOff, c - CQ), s_lut);
                            if constexpr (WEIGHTED) {
                                t.x = __fmul_rn(t.x, w); t.y = __fmul_rn(t.y, w);
                                t.z = __fmul_rn(t.z, w); t.w = __fmul_rn(t.w, w);
                            }
                            a[rr][c].x = __fadd_rn(a[rr][c].x, t.x); a[rr][c].y = __fadd_rn(a[rr][c].y, t.y);
                            a[rr][c].z = __fadd_rn(a[rr][c].z, t.z); a[rr][c].w = __fadd_rn(a[rr][c].w, t.w);
                        }
                    }
                }
            }
        }

#ifdef EVS_X_NOCOMPUTE  // developer A/B (tools/variants.sh): the gather + LDS staging alone
        if (a[0][0].x == 123.456f) args.R[b] = xv[0];
        continue;
#endif
        f32x4 c00, c10, c11;
        interact(a, c00, c10, c11);
#ifdef EVS_X_NOSTORE  // developer A/B (tools/variants.sh): everything but the output traffic
        if (c00[0] + c10[1] + c11[2] + c00[3] + c10[0] + c11[1] + c00[2] + c10[3] + c11[0] + c00[1] + c10[2] + c11[3] == 123.456f)
            args.R[b * (int64_t)out_row + lane] = xv[0];
        continue;
#endif
        stage_row(xv, c00, c10, c11);
    }
    if constexpr (CHECK) {
        const int n_fast = n_samples < fallback_from ? n_samples : fallback_from;
        if (n_fast > 0) flush_out(wave_id + (int64_t)(n_fast - 1) * waves_total);
        // slow loop (rare): pool this lane's feature of sample b straight from global memory, general bag semantics
        for (int k = fallback_from; k < n_samples; k++) {
            const int64_t b = wave_id + (int64_t)k * waves_total;
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
                    const int64_t *ip = ka->indices[f];
                    const char *src = reinterpret_cast<const char *>(ka->src[f]);
                    if (!ip) {
                        const char *row = src + (uint64_t)b * (uint64_t)(ka->stride[f] * 4);
#pragma unroll
                        for (int c = 0; c < NC; c++) a[rr][c] = chunk_at(row, c);
                        continue;
                    }
                    const int64_t *op = ka->offsets[f];
                    const int64_t nnz = ka->nnz[f];
                    int64_t s0 = op[b];
                    int64_t e0 = (b + 1 < ka->off_len[f]) ? op[b + 1] : nnz;
                    if (!((s0 >= 0) & (e0 >= s0) & (e0 <= nnz))) { bad = true; s0 = e0 = 0; }
                    const uint64_t n_rows = (uint64_t)ka->n_rows[f];
                    for (int64_t j = s0; j < e0; j++) {
                        const int64_t r = ip[j];
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
                if (r16 == 0) {   // x (row 0 of the slot) is read back below for the passthrough columns
#pragma unroll
                    for (int c = 0; c < NC; c++)
                        if (c < CQ || q == 0)
                            *reinterpret_cast<float4 *>(my_lds + (c < CQ ? (q * CQ + c) * 16 : kRemOff + (c - CQ) * 16)) = a[0][c];
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            float xv[(d + 63) / 64];
#pragma unroll
            for (int h = 0; h < (d + 63) / 64; h++) {
                const int e = lane + 64 * h;
                xv[h] = reinterpret_cast<const float *>(my_lds)[e < d ? e : 0];
            }
            f32x4 c00, c10, c11;
            interact(a, c00, c10, c11);
            stage_row(xv, c00, c10, c11);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            flush_out(b);
        }
    } else {
        if (!TILE || n_samples > 0) flush_out(wave_id + (int64_t)(n_samples - 1) * waves_total);
    }
    if (bad) atomicOr(args.err, 1);
}

// offsets[f][b] == b for every indirect feature and every bag (and offsets[f][B] == B where the array has B+1
// entries; an array of B entries needs nnz == B, checked on the host)?  Coalesced read of 8*T*B bytes.
__global__ void __launch_bounds__(256) offsets_arange_kernel(const FusedArgs args) {
    const int64_t n = args.B * args.F;
    bool ragged = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int f = (int)(i / args.B);
        const int64_t b = i - (int64_t)f * args.B;
        const int64_t *off = args.indices[f] ? args.offsets[f] : nullptr;
        if (!off) continue;
        ragged |= off[b] != b;
        if (b == args.B - 1 && args.off_len[f] > args.B) ragged |= off[args.B] != args.B;
    }
    if (__any(ragged) && (threadIdx.x & 63) == 0) atomicMax(args.opt_flag, args.opt_id);
}

static bool optimistic_enabled() {
    static int v = -1;
    if (v < 0) { const char *e = evs::env_switch("EVS_FUSED_OPTIMISTIC"); v = e ? atoi(e) : 1; }
    return v != 0;
}

static bool use_lds_rows() {
    static int v = -1;
    if (v < 0) { const char *e = evs::env_switch("EVS_FUSED_LDS"); v = e ? atoi(e) : 1; }
    return v != 0;
}

// persistent grid: exactly the resident waves of THIS kernel, each walking its samples through the pipeline
template <auto K>
static void launch_persistent(const FusedArgs &a, hipStream_t st) {
    static int per_cu = 0;
    if (!per_cu) {
        int n = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, K, 256, 0);
        per_cu = (e == hipSuccess && n > 0) ? n : 2;
    }
    int64_t blocks = (a.B + 3) / 4;
    const int64_t cap = (int64_t)kNumCu * per_cu;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(K, dim3((unsigned)blocks), dim3(256), 0, st, a);
}

// index-tile kernel: same resident grid, each block a contiguous sample range (whole 16-sample chunks when the
// batch is large enough to keep every block busy that way)
static int tile_mode() {
    static int v = -1;
    if (v < 0) { const char *e = evs::env_switch("EVS_FUSED_TILE"); v = e ? atoi(e) : 1; }
    return v;
}
static int64_t tile_min_batch() {
    static int64_t v = -1;
    if (v < 0) v = env_switch_range("EVS_FUSED_TILE_MIN_B", 2048, 0, 1ll << 40);   // (below: one chunk per block at most, nothing to win)
    return v;
}
// reduced precision, offsets given, whole batches: from this batch size on the rows-in-registers kernel checks the offsets
// itself (evs_fused_rfq.hip, CHECK)
static int64_t rfq_check_min_batch() {
    static int64_t v = -1;
    if (v < 0) v = env_switch_range("EVS_FUSED_RFQ_CHECK_MIN_B", 256, 0, 1ll << 40);
    return v;
}
static bool tile_eligible(const FusedArgs &a, int codec) {
    return codec == 32 && tile_mode() && a.B >= tile_min_batch() && a.F <= kTileMaxF;
}
template <auto K>
static void launch_tile(FusedArgs a, hipStream_t st) {
    static int per_cu = 0;
    if (!per_cu) {
        int n = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, K, 256, 0);
        per_cu = (e == hipSuccess && n > 0) ? n : 2;
    }
    const int64_t cap = (int64_t)kNumCu * per_cu;
    int64_t per = (a.B + cap - 1) / cap;
    static int align = 0;
    if (!align) { const char *e = evs::env_switch("EVS_FUSED_TILE_ALIGN"); align = e ? atoi(e) : 4; if (align < 1) align = 1; }
    per = (per + align - 1) / align * align;
    a.tile_per = (int)per;
    const int64_t blocks = (a.B + per - 1) / per;
    hipLaunchKernelGGL(K, dim3((unsigned)blocks), dim3(256), 0, st, a);
}

template <int CODEC, int CQ, int REM, bool WEIGHTED, bool HAS_INDIRECT, bool PTRS>
static void launch_nt(const FusedArgs &a, hipStream_t st) {
    const bool nt2 = a.F > 16;
    // rows through LDS: fp32 always; reduced precision when feature 0 is x and every other feature a table
    if constexpr ((4 * CQ + REM) <= 32 && (CODEC == 32 || (HAS_INDIRECT && !PTRS && !WEIGHTED))) {
        // (offsets == NULL exists only in the LDS kernel: the developer switch cannot take that away)
        if ((use_lds_rows() || a.bag1 == 1) && (CODEC == 32 || a.enc_lds)) {
            if constexpr (HAS_INDIRECT && !WEIGHTED) {
                if constexpr (!PTRS && CODEC == 32) {   // (encoded rows: no gain for u8 / u4, slower for u16 -- measured)
                    if (a.bag1 == 1 && tile_eligible(a, CODEC)) {
                        if (launch_rf(a, st)) return;   // rows in flight in registers (evs_fused_rf.hip): d = 16 / 32 / 36 / 64
                        if (nt2) launch_tile<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 2, WEIGHTED, HAS_INDIRECT, PTRS, true, true>>(a, st);
                        else launch_tile<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 1, WEIGHTED, HAS_INDIRECT, PTRS, true, true>>(a, st);
                        return;
                    }
                }
                if constexpr (!PTRS && CODEC != 32) {   // encoded rows in flight in registers (evs_fused_rfq.hip): d = 16 / 32 / 36
                    if (a.bag1 == 1 && launch_rfq(a, CODEC, st)) return;
                }
                if (PTRS || a.bag1 == 1) {
                    if (nt2) launch_persistent<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 2, WEIGHTED, HAS_INDIRECT, PTRS, true>>(a, st);
                    else launch_persistent<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 1, WEIGHTED, HAS_INDIRECT, PTRS, true>>(a, st);
                    return;
                }
                if constexpr (!PTRS) {
                    if constexpr (CODEC == 32) {
                        if (a.bag1 == 3 && launch_rf_check(a, st)) return;   // rows in flight in registers, offsets checked per block
                        if (a.bag1 == 3) {   // the index-tile loop checks the offsets itself and pools failing chunks the slow way
                            if (nt2) launch_tile<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 2, WEIGHTED, HAS_INDIRECT, PTRS, true, true, true>>(a, st);
                            else launch_tile<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 1, WEIGHTED, HAS_INDIRECT, PTRS, true, true, true>>(a, st);
                            return;
                        }
                    }
                    if constexpr (CODEC != 32) {
                        // the rows-in-registers kernel checks the offsets itself and pools the blocks that fail the slow way
                        if (a.bag1 == 4) {
                            if (launch_rfq(a, CODEC, st)) return;
                            FusedArgs g = a;   // (no zero-code page: the general loop)
                            g.bag1 = 0;
                            if (nt2) launch_persistent<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 2, WEIGHTED, HAS_INDIRECT, PTRS, false>>(g, st);
                            else launch_persistent<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 1, WEIGHTED, HAS_INDIRECT, PTRS, false>>(g, st);
                            return;
                        }
                    }
                    if (a.bag1 == 2) {   // optimistic triple: arange check, the bag-1 loop, then (below) the general loop
                        int nb = (int)((a.B * a.F + 255) / 256); if (nb > kNumCu * 4) nb = kNumCu * 4;
                        hipLaunchKernelGGL(offsets_arange_kernel, dim3(nb), dim3(256), 0, st, a);
                        bool tiled = false;
                        if constexpr (CODEC == 32) {
                            if (tile_eligible(a, CODEC)) {
                                tiled = true;
                                if (nt2) launch_tile<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 2, WEIGHTED, HAS_INDIRECT, PTRS, true, true>>(a, st);
                                else launch_tile<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 1, WEIGHTED, HAS_INDIRECT, PTRS, true, true>>(a, st);
                            }
                        }
                        if constexpr (CODEC != 32) tiled = launch_rfq(a, CODEC, st);
                        if (tiled) {
                        } else if (nt2) launch_persistent<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 2, WEIGHTED, HAS_INDIRECT, PTRS, true>>(a, st);
                        else launch_persistent<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 1, WEIGHTED, HAS_INDIRECT, PTRS, true>>(a, st);
                    }
                }
            }
            if constexpr (!HAS_INDIRECT && !WEIGHTED && !PTRS && CODEC == 32) {
                // interact_features over rows that are already there (the two-call path's second half, dlrm_s_pytorch.py:483-516):
                // every feature is dense -- the rows-in-registers kernel takes dense features as rows addressed by the sample
                // number (it does so for x and for the sharded step's received vectors), with no index round trip at all.
                // Needs 16-byte aligned rows (EVS_INTERACT_RF=0: the LDS-DMA loop).
                static const bool dense_rf = evs::env_switch_on("EVS_INTERACT_RF");
                bool ok = dense_rf && tile_eligible(a, CODEC);
                for (int f = 0; f < a.F && ok; f++)
                    ok = (reinterpret_cast<uintptr_t>(a.src[f]) & 15) == 0 && ((a.stride[f] * 4) & 15) == 0;
                if (ok) {
                    FusedArgs b = a;
                    b.bag1 = 1;
                    if (!b.dummy_i64) b.dummy_i64 = reinterpret_cast<const int64_t *>(a.zeros);   // (lanes with no index to load read it)
                    if (launch_rf(b, st)) return;
                }
            }
            if (nt2) launch_persistent<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 2, WEIGHTED, HAS_INDIRECT, PTRS, false>>(a, st);
            else launch_persistent<emb_interact_dot_lds_kernel<CODEC, CQ, REM, 1, WEIGHTED, HAS_INDIRECT, PTRS, false>>(a, st);
            return;
        }
    }
    if (nt2) launch_persistent<emb_interact_dot_kernel<CODEC, CQ, REM, 2, WEIGHTED, HAS_INDIRECT, PTRS>>(a, st);
    else launch_persistent<emb_interact_dot_kernel<CODEC, CQ, REM, 1, WEIGHTED, HAS_INDIRECT, PTRS>>(a, st);
}

template <int CODEC, bool WEIGHTED, bool HAS_INDIRECT, bool PTRS = false>
static bool launch_cpq(const FusedArgs &a, hipStream_t st) {
    switch (a.d) {
    case 16: launch_nt<CODEC, 1, 0, WEIGHTED, HAS_INDIRECT, PTRS>(a, st); return true;
    case 32: launch_nt<CODEC, 2, 0, WEIGHTED, HAS_INDIRECT, PTRS>(a, st); return true;
    case 36: launch_nt<CODEC, 2, 1, WEIGHTED, HAS_INDIRECT, PTRS>(a, st); return true;  // every EVStore script
    case 48: launch_nt<CODEC, 3, 0, WEIGHTED, HAS_INDIRECT, PTRS>(a, st); return true;
    case 64: launch_nt<CODEC, 4, 0, WEIGHTED, HAS_INDIRECT, PTRS>(a, st); return true;
    case 128: launch_nt<CODEC, 8, 0, WEIGHTED, HAS_INDIRECT, PTRS>(a, st); return true;
    default: return false;
    }
}



// Cache-tier consumer (evs_cache.hip): feature 0 = x, feature k+1 = the fp32 row at address
// row_ptrs[b*T + k] (0 = no row -> zeros).  iota: device int64 array 0..B-1 (bag b = index b).
int fused_interact_from_row_ptrs(int64_t B, int T, int d, const float *x, int64_t x_stride,
                                 const int64_t *row_ptrs, const int64_t *iota, int itself, float *R, hipStream_t st) {
    FusedArgs a;
    const int F = T + 1;
    for (int f = 0; f < EVS_MAX_FEATURES; f++) {
        a.src[f] = nullptr; a.stride[f] = 0; a.indices[f] = nullptr; a.offsets[f] = nullptr; a.nnz[f] = 0;
        a.n_rows[f] = 0; a.row_w[f] = nullptr; a.off_len[f] = B;
    }
    a.zeros = zero_page();
    a.err = index_error_flag();
    if (!a.zeros || !a.err) return EVS_EHIP;
    a.src[0] = x; a.stride[0] = x_stride;
    for (int k = 0; k < T; k++) {
        a.src[k + 1] = a.zeros; a.indices[k + 1] = row_ptrs + k; a.offsets[k + 1] = iota;   // (B,T) table, column k
        a.nnz[k + 1] = B; a.n_rows[k + 1] = 1;
    }
    a.R = R; a.B = B; a.F = F; a.d = d; a.itself = itself ? 1 : 0;
    a.P = itself ? F * (F + 1) / 2 : F * (F - 1) / 2;
    a.dummy_i64 = iota; a.dummy_f32 = x; a.bag1 = 1; a.enc_lds = 0; a.opt_flag = nullptr; a.opt_id = 0;
    if (!launch_cpq<32, false, true, true>(a, st)) { set_error("fused_interact_from_row_ptrs: no kernel for d=%d", d); return EVS_EINVAL; }
    EVS_HIP_CHECK(hipGetLastError());
    return EVS_OK;
}

// interaction over x + T features given as one (B,T) table of 32-bit row ids (cache tier; evs_fused_rf.hip, IDS variant)
bool fused_row_ids_supported(int64_t B, int T, int d) { return rf_ids_supported(B, T + 1, d); }
int fused_interact_from_row_ids(int64_t B, int T, int d, const float *x, int64_t x_stride, const int *row_ids,
                                const void *arena, const void *const *tables, int itself, float *R, hipStream_t st) {
    FusedArgs a;
    const int F = T + 1;
    for (int f = 0; f < EVS_MAX_FEATURES; f++) {
        a.src[f] = nullptr; a.stride[f] = 0; a.indices[f] = nullptr; a.offsets[f] = nullptr; a.nnz[f] = 0;
        a.n_rows[f] = 0; a.row_w[f] = nullptr; a.off_len[f] = B;
    }
    a.zeros = zero_page();
    a.err = index_error_flag();
    if (!a.zeros || !a.err) return EVS_EHIP;
    a.src[0] = x; a.stride[0] = x_stride;
    for (int k = 0; k < T; k++) a.src[k + 1] = tables[k];
    a.R = R; a.B = B; a.F = F; a.d = d; a.itself = itself ? 1 : 0;
    a.P = itself ? F * (F + 1) / 2 : F * (F - 1) / 2;
    a.dummy_i64 = reinterpret_cast<const int64_t *>(a.zeros); a.dummy_f32 = x; a.bag1 = 1; a.enc_lds = 0; a.opt_flag = nullptr; a.opt_id = 0;
    a.w1p = nullptr; a.b1 = nullptr; a.z1 = nullptr; a.n1 = 0; a.kp = 0; a.relu = 0; a.write_r = 1;
    a.row_ids = row_ids; a.arena = arena; a.probe = ProbeArgs{};
    if (!launch_rf_ids(a, st)) { set_error("fused_interact_from_row_ids: no kernel for B=%lld T=%d d=%d", (long long)B, T, d); return EVS_EINVAL; }
    EVS_HIP_CHECK(hipGetLastError());
    return EVS_OK;
}

bool fused_probe_codec_supported(int64_t B, int T, int d, int codec) { return rfq_probe_supported(B, T + 1, d, codec); }

// ... and with the cache probe folded in (evs_fused_rf.hip, PROBE variant): the request rows in, R, hit flags, the miss
// lists and the hit statistics out.  One block per 16 samples: probe.list_cnt needs ceil(B / 16) entries, probe.miss_rec
// ceil(B / 16) * probe.list_cap records with list_cap >= 16 * T.
int fused_probe_interact(int64_t B, int T, int d, const float *x, int64_t x_stride, const ProbeArgs &probe, const void *arena,
                         const void *const *tables, const long long *table_rows, int itself, float *R, hipStream_t st, int codec) {
    FusedArgs a;
    const int F = T + 1;
    for (int f = 0; f < EVS_MAX_FEATURES; f++) {
        a.src[f] = nullptr; a.stride[f] = 0; a.indices[f] = nullptr; a.offsets[f] = nullptr; a.nnz[f] = 0;
        a.n_rows[f] = 0; a.row_w[f] = nullptr; a.off_len[f] = B;
    }
    a.zeros = zero_page();
    a.err = index_error_flag();
    if (!a.zeros || !a.err) return EVS_EHIP;
    a.src[0] = x; a.stride[0] = x_stride;
    for (int k = 0; k < T; k++) { a.src[k + 1] = tables[k]; a.n_rows[k + 1] = table_rows[k]; }
    a.R = R; a.B = B; a.F = F; a.d = d; a.itself = itself ? 1 : 0;
    a.P = itself ? F * (F + 1) / 2 : F * (F - 1) / 2;
    a.dummy_i64 = reinterpret_cast<const int64_t *>(a.zeros); a.dummy_f32 = x; a.bag1 = 1; a.enc_lds = 0; a.opt_flag = nullptr; a.opt_id = 0;
    a.w1p = nullptr; a.b1 = nullptr; a.z1 = nullptr; a.n1 = 0; a.kp = 0; a.relu = 0; a.write_r = 1;
    a.row_ids = nullptr; a.arena = arena; a.probe = probe;
    if (codec != 32) {   // a reduced-precision tier: the rows decoded in the kernel (evs_fused_rfq.hip, PROBE form)
        a.enc_lds = 1;
        if (!launch_rfq_probe(a, codec, st)) { set_error("fused_probe_interact: no kernel for B=%lld T=%d d=%d codec=%d", (long long)B, T, d, codec); return EVS_EINVAL; }
        EVS_HIP_CHECK(hipGetLastError());
        return EVS_OK;
    }
    if (!launch_rf_probe(a, st)) { set_error("fused_probe_interact: no kernel for B=%lld T=%d d=%d", (long long)B, T, d); return EVS_EINVAL; }
    EVS_HIP_CHECK(hipGetLastError());
    return EVS_OK;
}

}  // namespace evs

extern "C" int evs_fused_dim_supported(int d) {
    return d == 16 || d == 32 || d == 36 || d == 48 || d == 64 || d == 128;
}

extern "C" int evs_emb_interact_dot(int64_t B, int F, int d, int codec, const evs_feature *feats_in, int itself,
                                    float *R, void *stream) {
    using namespace evs;
    EVS_REQUIRE(B >= 0 && B < (1ll << 31) && F >= 1 && F <= EVS_MAX_FEATURES && evs_fused_dim_supported(d),
                "evs_emb_interact_dot: unsupported shape B=%lld F=%d d=%d (need F<=32, d in {16,32,36,48,64,128})",
                (long long)B, F, d);
    EVS_REQUIRE(codec == 32 || codec == 16 || codec == 8 || codec == 4, "evs_emb_interact_dot: codec %d", codec);
    if (B == 0) return EVS_OK;
    EVS_REQUIRE(feats_in && R, "evs_emb_interact_dot: NULL argument");
    // A table nobody indexes in this batch arrives with nnz == 0 and, from most runtimes, a NULL indices pointer --
    // which otherwise means "dense feature".  n_rows > 0 with offsets given marks it as a table: every bag is empty.
    evs_feature feats[EVS_MAX_FEATURES];
    for (int f = 0; f < F; f++) {
        feats[f] = feats_in[f];
        if (!feats[f].indices && feats[f].n_rows > 0 && feats[f].offsets && feats[f].nnz == 0)
            feats[f].indices = feats[f].offsets;   // any valid address: never dereferenced
    }
    EVS_REQUIRE(feats[0].indices == nullptr, "evs_emb_interact_dot: feature 0 (x) must be dense");
    FusedArgs a;
    for (int f = 0; f < EVS_MAX_FEATURES; f++) {
        const bool on = f < F;
        a.src[f] = on ? feats[f].src : nullptr;
        a.stride[f] = on ? feats[f].stride : 0;
        a.indices[f] = on ? feats[f].indices : nullptr;
        a.offsets[f] = on ? feats[f].offsets : nullptr;
        a.nnz[f] = on ? feats[f].nnz : 0;
        a.n_rows[f] = on ? feats[f].n_rows : 0;
        a.row_w[f] = on ? feats[f].row_weights : nullptr;
        a.off_len[f] = on ? (feats[f].offsets_len > 0 ? feats[f].offsets_len : B) : B;
        if (!on) continue;
        EVS_REQUIRE(feats[f].src || (feats[f].indices && feats[f].n_rows == 0), "evs_emb_interact_dot: feats[%d].src is NULL", f);
        EVS_REQUIRE(reinterpret_cast<uintptr_t>(feats[f].src) % 16 == 0, "evs_emb_interact_dot: feats[%d].src must be 16-byte aligned", f);
        if (feats[f].indices) {
            // offsets == NULL: one index per bag (bag b = indices[b]); checked for all features below
            EVS_REQUIRE(feats[f].offsets_len == 0 || (feats[f].offsets_len >= B && feats[f].offsets_len < (1ll << 31)),
                        "evs_emb_interact_dot: feats[%d].offsets_len must be 0 or in [B, 2^31)", f);
            EVS_REQUIRE(feats[f].nnz >= 0 && feats[f].n_rows >= 0 && feats[f].nnz < (1ll << 31) && feats[f].n_rows < (1ll << 31),
                        "evs_emb_interact_dot: feats[%d]: nnz and n_rows must be in [0, 2^31)", f);
        } else {
            EVS_REQUIRE(feats[f].stride % 4 == 0 && feats[f].stride >= 0 && feats[f].stride < (1ll << 31),
                        "evs_emb_interact_dot: dense feats[%d].stride must be a multiple of 4 in [0, 2^31)", f);
        }
    }
    a.R = R; a.B = B; a.F = F; a.d = d; a.itself = itself ? 1 : 0;
    a.P = itself ? F * (F + 1) / 2 : F * (F - 1) / 2;
    a.err = index_error_flag();
    if (!a.err) return EVS_EHIP;
    a.zeros = zero_page();
    if (!a.zeros) return EVS_EHIP;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    bool weighted = false, indirect = false;
    a.dummy_i64 = nullptr;
    a.bag1 = 0;
    {
        int n_ind = 0, n_nooff = 0;
        for (int f = 0; f < F; f++) if (feats[f].indices) { n_ind++; if (!feats[f].offsets) n_nooff++; }
        EVS_REQUIRE(n_nooff == 0 || n_nooff == n_ind, "evs_emb_interact_dot: either every indirect feature has offsets or none (one index per bag)");
        a.bag1 = n_ind > 0 && n_nooff == n_ind;
        a.enc_lds = codec != 32 && n_ind == F - 1;
        for (int f = 1; f < F && a.enc_lds; f++)
            a.enc_lds = feats[f].indices && !feats[f].row_weights && reinterpret_cast<uintptr_t>(feats[f].src) % 4 == 0;
        if (a.bag1) {
            EVS_REQUIRE(codec == 32 || a.enc_lds, "evs_emb_interact_dot: offsets == NULL with reduced-precision tables needs x + tables only");
            for (int f = 0; f < F; f++)
                if (feats[f].indices) EVS_REQUIRE(feats[f].nnz >= B && !feats[f].row_weights, "evs_emb_interact_dot: one-index-per-bag features need nnz >= B and no row weights");
        }
    }
    a.dummy_f32 = reinterpret_cast<const float *>(feats[0].src);
    for (int f = 0; f < F; f++) {
        if (!feats[f].indices) continue;
        indirect = true;
        weighted |= feats[f].row_weights != nullptr;
        if (!a.dummy_i64) a.dummy_i64 = feats[f].offsets ? feats[f].offsets : feats[f].indices;  // >= B readable entries
        if (feats[f].n_rows == 0 || !feats[f].src) a.src[f] = a.zeros;  // never dereferenced for a valid row
    }
    EVS_REQUIRE(!weighted || codec == 32, "evs_emb_interact_dot: weighted pooling is only built for fp32 tables");
    // Offsets given: bet that they are arange (what the Criteo collate always produces).  A small kernel reads
    // the offsets once (coalesced) and records the verdict; the one-index-per-bag loop and the general loop are
    // both launched and the one that does not apply returns at once -- no host round trip.  Needs idx[b]
    // readable for every b (nnz >= B) and a last bag that ends at B.
    a.opt_flag = nullptr; a.opt_id = 0;
    // (three launches: below ~8 k samples the two extra launches cost more than the faster loop returns.)
    // Whole fp32 batches (every table nnz == B, B or B + 1 offsets) from the tile kernel's minimum batch on need no bet
    // at all: ONE launch of the index-tile loop that checks its own bags and pools the chunks that fail the slow way
    // (bag1 = 3).  Batch SLICES of longer arrays (offsets_len > B + 1: their offsets do not start at 0 unless the
    // slice does) keep the separate check.
    if (indirect && !a.bag1 && !weighted && (codec == 32 || a.enc_lds) && (B >= 8192 || tile_eligible(a, codec) || (codec != 32 && B >= rfq_check_min_batch())) && optimistic_enabled()) {
        bool can = true, whole = true;
        for (int f = 0; f < F && can; f++)
            if (feats[f].indices) {
                can = feats[f].nnz >= B && (a.off_len[f] > B || feats[f].nnz == B);
                whole = whole && feats[f].nnz == B && a.off_len[f] <= B + 1;
            }
        if (can && whole && tile_eligible(a, codec)) {
            a.bag1 = 3;
        } else if (can && whole && B >= rfq_check_min_batch() && rfq_supported(a, codec)) {
            a.bag1 = 4;
        } else if (can && B >= 8192) {
            a.opt_flag = optimistic_slot(&a.opt_id);
            if (!a.opt_flag) return EVS_EHIP;
            a.bag1 = 2;
        }
    }
    // the stacked form (evs_emb_interact_dot_stacked: x + T tables behind ONE (T, B) index array and, lS_o given, one offsets array):
    // the rows-in-registers kernel then computes every feature's index / offsets address itself and asks for them before it
    // reads its feature table out of the kernel arguments (FusedArgs::stk)
    a.stk = 0;
    static const bool stk_on = evs::env_switch_on("EVS_FUSED_STK");   // developer A/B
    if (stk_on && indirect && !weighted && codec == 32 && F >= 2 && !feats[0].indices && (a.bag1 == 1 || a.bag1 == 3)) {
        bool yes = feats[1].indices != nullptr;
        const int64_t si = F > 2 && feats[2].indices ? feats[2].indices - feats[1].indices : 0;
        const int64_t so = F > 2 && feats[1].offsets && feats[2].offsets ? feats[2].offsets - feats[1].offsets : 0;
        for (int f = 1; f < F && yes; f++) {
            yes = feats[f].indices == feats[1].indices + (int64_t)(f - 1) * si && feats[f].nnz == feats[1].nnz && a.off_len[f] == a.off_len[1] &&
                  ((a.bag1 == 1 && !feats[f].offsets) || (a.bag1 == 3 && feats[f].offsets && feats[f].offsets == feats[1].offsets + (int64_t)(f - 1) * so));
        }
        if (yes) {
            a.stk = 1; a.stk_idx = feats[1].indices; a.stk_idx_stride = si;
            a.stk_off = a.bag1 == 3 ? feats[1].offsets : nullptr; a.stk_off_stride = a.bag1 == 3 ? so : 0; a.stk_off_len = a.off_len[1];
        }
    }
    bool ok;
    if (!indirect) {
        ok = launch_cpq<32, false, false>(a, st);
    } else {
        switch (codec) {
        case 32: ok = weighted ? launch_cpq<32, true, true>(a, st) : launch_cpq<32, false, true>(a, st); break;
        case 16: ok = launch_cpq<16, false, true>(a, st); break;
        case 8: ok = launch_cpq<8, false, true>(a, st); break;
        default: ok = launch_cpq<4, false, true>(a, st); break;
        }
    }
    EVS_REQUIRE(ok, "evs_emb_interact_dot: no kernel for d=%d", d);
    (void)weighted;
    EVS_HIP_CHECK(hipGetLastError());
    return EVS_OK;
}

extern "C" int evs_emb_interact_dot_stacked(int64_t B, int T, int d, int codec, const void *const *tables,
                                            const int64_t *n_rows, const float *x, int64_t x_stride,
                                            const int64_t *indices_base, int64_t indices_row_stride,
                                            int64_t nnz_per_table, const int64_t *offsets_base,
                                            int64_t offsets_row_stride, const float *const *row_weights, int itself,
                                            float *R, void *stream) {
    using namespace evs;
    EVS_REQUIRE(T >= 0 && T + 1 <= EVS_MAX_FEATURES, "evs_emb_interact_dot_stacked: T=%d (need T+1 <= %d)", T,
                EVS_MAX_FEATURES);
    EVS_REQUIRE(B == 0 || (tables && n_rows && x && indices_base), "evs_emb_interact_dot_stacked: NULL argument");
    evs_feature ft[EVS_MAX_FEATURES];
    ft[0].src = x; ft[0].stride = x_stride; ft[0].indices = nullptr; ft[0].offsets = nullptr;
    ft[0].nnz = 0; ft[0].n_rows = 0; ft[0].row_weights = nullptr; ft[0].offsets_len = 0;
    for (int k = 0; k < T; k++) {
        evs_feature &f = ft[k + 1];
        f.src = tables[k]; f.stride = 0;
        f.indices = indices_base + (int64_t)k * indices_row_stride;
        f.offsets = offsets_base ? offsets_base + (int64_t)k * offsets_row_stride : nullptr;  // NULL: one index per bag
        f.nnz = nnz_per_table; f.n_rows = n_rows[k];
        f.row_weights = row_weights ? row_weights[k] : nullptr;
        f.offsets_len = 0;
    }
    return evs_emb_interact_dot(B, T + 1, d, codec, ft, itself, R, stream);
}

// K independent batches in ONE call (a serving loop's queue of requests) = ONE launch for up to kMultiMax of them
// (evs_fused_rf.hip: K * ceil(B / 16) one-chunk blocks, each reading its batch's x / indices / offsets / R from a table in
// the kernel arguments).  The hardware hands a CU the next block as one retires, so the drain of one batch (output rows
// of its last samples still leaving) runs under the fill of the next (indices, then rows, before the first MFMA): 15.5-16.2
// us per 16 384-sample batch instead of 19-20 for K launches -- the rate a caller alternating two HIP streams gets,
// without any stream.  (A stream pair inside the library, forked from and joined into the caller's stream, was built first
// and measured: 21.7-24.3 us per batch -- cross-stream event waits cost more on this stack than the overlap returns;
// tools/multi_probe.py, docs/HISTORY.md 3.2d.)  Shapes the one-chunk kernel does not take (reduced precision, d = 48 / 64 / 128,
// F > 28) run as K launches.  Results are bit-identical to K evs_emb_interact_dot_stacked calls either way.
extern "C" int evs_emb_interact_dot_stacked_multi(int K, int64_t B, int T, int d, int codec, const void *const *tables,
                                                  const int64_t *n_rows, const float *const *x, int64_t x_stride,
                                                  const int64_t *const *indices_base, int64_t indices_row_stride,
                                                  int64_t nnz_per_table, const int64_t *const *offsets_base,
                                                  int64_t offsets_row_stride, int itself, float *const *R, void *stream) {
    using namespace evs;
    EVS_REQUIRE(K >= 0 && K <= 4096, "evs_emb_interact_dot_stacked_multi: K=%d", K);
    if (K == 0 || B == 0) return EVS_OK;
    EVS_REQUIRE(x && indices_base && R && tables && n_rows, "evs_emb_interact_dot_stacked_multi: NULL argument");
    EVS_REQUIRE(T >= 0 && T + 1 <= EVS_MAX_FEATURES, "evs_emb_interact_dot_stacked_multi: T=%d (need T+1 <= %d)", T, EVS_MAX_FEATURES);
    for (int k = 0; k < K; k++)
        EVS_REQUIRE(x[k] && indices_base[k] && R[k] && (!offsets_base || offsets_base[k]), "evs_emb_interact_dot_stacked_multi: batch %d has a NULL pointer", k);
    const int F = T + 1;
    static const bool one_launch = evs::env_switch_on("EVS_FUSED_MULTI");
    // the one-launch form: fp32 tables, whole batches (nnz == B: what makes lS_o checkable per block), aligned operands
    bool fast = one_launch && K > 1 && codec == 32 && T >= 1 && nnz_per_table == B && B < (1ll << 31) && rf_multi_supported(B, F, d) &&
                x_stride % 4 == 0 && x_stride >= 0 && x_stride < (1ll << 31) && optimistic_enabled();
    for (int k = 0; k < K && fast; k++) fast = reinterpret_cast<uintptr_t>(x[k]) % 16 == 0;
    for (int t = 0; t < T && fast; t++) fast = tables[t] && reinterpret_cast<uintptr_t>(tables[t]) % 16 == 0 && n_rows[t] >= 0 && n_rows[t] < (1ll << 31);
    if (!fast) {
        for (int k = 0; k < K; k++) {
            const int rc = evs_emb_interact_dot_stacked(B, T, d, codec, tables, n_rows, x[k], x_stride, indices_base[k], indices_row_stride, nnz_per_table,
                                                        offsets_base ? offsets_base[k] : nullptr, offsets_row_stride, nullptr, itself, R[k], stream);
            if (rc) return rc;
        }
        return EVS_OK;
    }
    FusedArgs a;
    for (int f = 0; f < EVS_MAX_FEATURES; f++) {
        a.src[f] = nullptr; a.stride[f] = 0; a.indices[f] = nullptr; a.offsets[f] = nullptr; a.nnz[f] = 0;
        a.n_rows[f] = 0; a.row_w[f] = nullptr; a.off_len[f] = B;
    }
    a.src[0] = x[0]; a.stride[0] = x_stride;
    for (int t = 0; t < T; t++) {
        a.src[t + 1] = tables[t];
        a.indices[t + 1] = indices_base[0] + (int64_t)t * indices_row_stride;   // (non-NULL marks a table; the kernel reads multi_idx)
        a.offsets[t + 1] = offsets_base ? offsets_base[0] + (int64_t)t * offsets_row_stride : nullptr;
        a.nnz[t + 1] = B; a.n_rows[t + 1] = n_rows[t];
    }
    a.zeros = zero_page();
    a.err = index_error_flag();
    if (!a.zeros || !a.err) return EVS_EHIP;
    for (int t = 0; t < T; t++) if (n_rows[t] == 0) a.src[t + 1] = a.zeros;
    a.B = B; a.F = F; a.d = d; a.itself = itself ? 1 : 0; a.P = itself ? F * (F + 1) / 2 : F * (F - 1) / 2;
    a.dummy_i64 = indices_base[0]; a.dummy_f32 = x[0]; a.bag1 = offsets_base ? 3 : 1; a.enc_lds = 0; a.opt_flag = nullptr; a.opt_id = 0;
    a.tile_per = 16; a.row_ids = nullptr; a.arena = nullptr; a.w1p = nullptr; a.b1 = nullptr; a.z1 = nullptr; a.n1 = 0; a.kp = 0; a.relu = 0; a.write_r = 1;
    a.zero_codes = nullptr;
    a.multi_idx_stride = indices_row_stride; a.multi_off_stride = offsets_row_stride;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (int k0 = 0; k0 < K; k0 += kMultiMax) {
        const int n = K - k0 < kMultiMax ? K - k0 : kMultiMax;
        for (int k = 0; k < kMultiMax; k++) {
            const int kk = k < n ? k0 + k : k0;
            a.multi_x[k] = x[kk]; a.multi_idx[k] = indices_base[kk]; a.multi_off[k] = offsets_base ? offsets_base[kk] : nullptr; a.multi_R[k] = R[kk];
        }
        a.multi_n = n;
        a.R = R[k0];
        if (!launch_rf_multi(a, st)) { set_error("evs_emb_interact_dot_stacked_multi: no kernel for this shape"); return EVS_EINVAL; }
        EVS_HIP_CHECK(hipGetLastError());
    }
    return EVS_OK;
}

// R = interact_features(x, apply_emb(...)) followed by the FIRST layer of the top MLP, Z1 = act(R W1^T + b1), in one
// launch (dlrm_s_pytorch.py:596-605: ly = apply_emb; z = interact_features; p = apply_mlp(z, top_l)).  One index per
// bag (the Criteo collate), fp32 tables, d in {16, 32, 36}, T <= 27.  w1_padded: W1 (n1 x K, K = d + P) zero-padded to
// (n1 rounded up to 16) rows of kp = (K rounded up to 16) floats, 16-byte aligned.  R may be NULL (not written).
extern "C" int evs_emb_interact_mlp1_stacked(int64_t B, int T, int d, const void *const *tables, const int64_t *n_rows,
                                             const float *x, int64_t x_stride, const int64_t *indices_base,
                                             int64_t indices_row_stride, int itself, const float *w1_padded, int kp,
                                             const float *b1, int n1, int relu, float *Z1, float *R, void *stream) {
    using namespace evs;
    const int F = T + 1;
    EVS_REQUIRE(B >= 0 && B < (1ll << 31) && T >= 1 && F <= kTileMaxF && (d == 16 || d == 32 || d == 36),
                "evs_emb_interact_mlp1_stacked: unsupported shape B=%lld T=%d d=%d (need T <= %d, d in {16,32,36})", (long long)B, T, d, kTileMaxF - 1);
    if (B == 0) return EVS_OK;
    const int P = itself ? F * (F + 1) / 2 : F * (F - 1) / 2;
    const int K = d + P;
    EVS_REQUIRE(tables && n_rows && x && indices_base && w1_padded && b1 && Z1, "evs_emb_interact_mlp1_stacked: NULL argument");
    EVS_REQUIRE(n1 >= 1 && kp == (K + 15) / 16 * 16, "evs_emb_interact_mlp1_stacked: kp must be K = %d rounded up to 16 (got %d), n1 >= 1", K, kp);
    EVS_REQUIRE(reinterpret_cast<uintptr_t>(w1_padded) % 16 == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && x_stride % 4 == 0,
                "evs_emb_interact_mlp1_stacked: w1_padded and x must be 16-byte aligned");
    FusedArgs a;
    for (int f = 0; f < EVS_MAX_FEATURES; f++) {
        a.src[f] = nullptr; a.stride[f] = 0; a.indices[f] = nullptr; a.offsets[f] = nullptr; a.nnz[f] = 0;
        a.n_rows[f] = 0; a.row_w[f] = nullptr; a.off_len[f] = B;
    }
    a.src[0] = x; a.stride[0] = x_stride;
    for (int k = 0; k < T; k++) {
        EVS_REQUIRE(tables[k] && reinterpret_cast<uintptr_t>(tables[k]) % 16 == 0 && n_rows[k] >= 0 && n_rows[k] < (1ll << 31),
                    "evs_emb_interact_mlp1_stacked: table %d must be 16-byte aligned with fewer than 2^31 rows", k);
        a.src[k + 1] = tables[k]; a.indices[k + 1] = indices_base + (int64_t)k * indices_row_stride;
        a.nnz[k + 1] = B; a.n_rows[k + 1] = n_rows[k];
    }
    a.zeros = zero_page();
    a.err = index_error_flag();
    if (!a.zeros || !a.err) return EVS_EHIP;
    a.R = R; a.B = B; a.F = F; a.d = d; a.itself = itself ? 1 : 0; a.P = P;
    a.dummy_i64 = indices_base; a.dummy_f32 = x; a.bag1 = 1; a.enc_lds = 0; a.opt_flag = nullptr; a.opt_id = 0; a.tile_per = 16;
    a.w1p = w1_padded; a.b1 = b1; a.z1 = Z1; a.n1 = n1; a.kp = kp; a.relu = relu ? 1 : 0; a.write_r = R ? 1 : 0;
    if (!launch_rf_mlp(a, reinterpret_cast<hipStream_t>(stream))) { set_error("evs_emb_interact_mlp1_stacked: no kernel for this shape"); return EVS_EINVAL; }
    EVS_HIP_CHECK(hipGetLastError());
    return EVS_OK;
}
