// Multi-hot bags pooled AND interacted in one launch (fp32 tables, unweighted sum pooling):
//     R[b] = [ x[b] | strict-lower(T[b] T[b]^T) ],  T[b] = [x[b]; sum of bag b of table 0; ...; sum of bag b of table T-1]
// (dlrm_s_pytorch.py:407-461 apply_emb with ragged bags followed by :483-516 interact_features) without the (T, B, d) block that
// bag_sum_flat_kernel / bag_sum_long_kernel write and the interaction kernel reads again.
//
// Split.  A block of 256 threads owns one chunk of 16 consecutive samples, wave w the samples w, w + 4, w + 8, w + 12, one after
// the other.  What the two existing forms each do half of:
//   * lane groups take LOOKUPS, not bags (as bag_sum_flat_kernel): a sample's lookups are flattened in (table, position) order and
//     walked in stages of kInstr x (64 / LPRD) rows -- every lane of every load instruction busy whatever the bag lengths;
//   * a sample's rows stay on chip until the matrix cores have consumed them (as the rows-in-registers kernel): rows travel in
//     registers, go through a per-wave LDS stage where (feature, 16-byte piece) owners add them IN INDEX ORDER (__fadd_rn from
//     +0.0f, the accumulator carried across stages: the bits of the oracle's loop), and the finished pooled rows are the MFMA
//     operands of the same wave.
// Pipeline (per wave, no block barrier behind the head): the stages of the wave's samples form ONE sequence.  While stage k is
// reduced out of LDS, the rows of stage k + 1 are in flight into registers and the indices of stage k + 2 behind them -- also across
// the boundary between two samples.  The loop body has no branch around a vector-memory load.
//
// LDS.  Per block: the validated (start, length) of every bag of the chunk (2 x 32 x 16 int), the tables' addresses.  Per wave: the
// exclusive prefix of its samples' bag lengths over the tables (4 x 32 int), its samples' x (4 x d), one stage (kInstr x 64 x 16 B =
// 4 KiB; the packed output row is staged in the same bytes once the sample's last stage is reduced), the operand slot (F rows).
#include "evs_fused.h"

#include <string.h>
#include <atomic>

namespace evs {

typedef float bg_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned bg_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) bg_f32x4 *bg_gf4_t;
typedef const __attribute__((address_space(1))) int64_t *bg_gi64_t;
typedef const __attribute__((address_space(1))) float *bg_gf32_t;

constexpr int kBagsInstr = 4;       // load instructions per stage
constexpr int kBagsSlots = 32;      // entries of every per-table array (tables past T: NULL / 0)

struct BagsArgs {
    const void *table[kBagsSlots];
    const int64_t *indices[kBagsSlots];
    const int64_t *offsets[kBagsSlots];
    int64_t nnz[kBagsSlots], n_rows[kBagsSlots], off_len[kBagsSlots];
    const float *x;
    int64_t x_stride;
    float *R;
    int64_t B;
    int T, itself, P;
    int *err;
    const void *zeros;              // 4 KiB of zeros: the row of a bad index and of a slot with no lookup; also "any readable int64"
};

// lanes of one wave hand values to each other through LDS: ordered by the hardware, not by the language
#define EVS_BAGS_WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

template <int LPRD, int NT>
__global__ void __launch_bounds__(256) emb_interact_bags_kernel(const BagsArgs args) {
    constexpr int d = 4 * LPRD;
    constexpr int row_bytes = 16 * LPRD;
    constexpr int RPI = 64 / LPRD;                  // rows per load instruction
    constexpr int S = kBagsInstr * RPI;             // rows per stage
    constexpr int CQ = LPRD / 4, REM = LPRD % 4;    // the k split of rf_body: slot q owns CQ 16-byte chunks, then element q of REM more
    constexpr int NR = NT;
    constexpr int MAXF = NT == 2 ? kTileMaxF : 16;
    constexpr int MAXT = MAXF - 1;
    constexpr int OPS = LPRD == 9 ? row_bytes : row_bytes + 16;   // bytes between operand rows (a power-of-two row pitch: one bank for all 16 rows)
    constexpr int kItems = (MAXT * LPRD + 63) / 64;               // (feature, piece) sums per lane
    constexpr int OUT_MAX = ((d + MAXF * (MAXF + 1) / 2 + 63) / 64) * 64;
    static_assert((OUT_MAX + 16) * 4 <= S * row_bytes, "the output row is staged in the stage's bytes");
    static_assert(MAXT + 1 <= 28, "the prefix is read as 7 x 4 entries");
    constexpr int kOob = 0x7ffffff0;
    constexpr int kCpol = 2;                        // nt: R is written once and streams out

    __shared__ int s_st[kBagsSlots][16], s_len[kBagsSlots][16];   // [table][sample of the chunk]; a bad bag: (0, 0)
    __shared__ unsigned long long s_tb[kBagsSlots];               // the tables' first rows
    __shared__ unsigned long long s_ip[kBagsSlots];               // ... index arrays
    __shared__ unsigned s_nr[kBagsSlots];                         // ... row counts
    __shared__ __attribute__((aligned(16))) int s_pre[4][4][kBagsSlots];   // [wave][its sample u][t]: lookups in front of table t; [T] = all; beyond: INT_MAX
    __shared__ float s_x[4][4][d];
    __shared__ __attribute__((aligned(16))) char s_stage[4][S * row_bytes];
    __shared__ __attribute__((aligned(16))) char s_op[4][MAXF * OPS];

    const BagsArgs *ka = (const BagsArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const int tid = (int)threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    const int T = args.T, F = T + 1, itself = args.itself;
    const int out_row = d + args.P;
    const int64_t B = args.B;
    const int64_t b0 = (int64_t)blockIdx.x * 16;
    const int nb = (int)(B - b0 < 16 ? B - b0 : 16);
    const unsigned long long zeros = (unsigned long long)reinterpret_cast<uintptr_t>(args.zeros);
    bool bad = false;

    // ---- head: the chunk's offsets, the tables, the wave's x -- one round trip ---------------------------------------------
    {
        // thread e (and e + 256) owns bag (table e >> 4, sample e & 15): where it starts and where it ends
        const int i = tid & 15;
        const int64_t b = b0 + i;
        int64_t st[2], en[2], nz[2];
        bool on[2], has_next[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int t = (tid >> 4) + 16 * h;
            on[h] = t < T && i < nb;
            const int64_t *op = ka->offsets[t];      // (32 entries each: read unconditionally)
            nz[h] = ka->nnz[t];
            const int64_t ol = ka->off_len[t];
            has_next[h] = on[h] & (b + 1 < ol);
            const int64_t *zp = reinterpret_cast<const int64_t *>(args.zeros);
            const int64_t *p0 = on[h] ? op + b : zp;
            const int64_t *p1 = has_next[h] ? op + b + 1 : zp;
            st[h] = *reinterpret_cast<bg_gi64_t>(reinterpret_cast<uintptr_t>(p0));
            en[h] = *reinterpret_cast<bg_gi64_t>(reinterpret_cast<uintptr_t>(p1));
        }
        // (no branch around a load: everything above and below leaves in one round trip)
        const int ts = tid & (kBagsSlots - 1);
        const void *tb_v = ka->table[ts];
        const int64_t *ip_v = ka->indices[ts];
        const int64_t nr_v = ka->n_rows[ts];
        float xr[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int64_t bu = b0 + wave + 4 * u;
            const float *xp = bu < B ? args.x + bu * args.x_stride + (lane < d ? lane : 0) : reinterpret_cast<const float *>(args.zeros);
            xr[u] = *reinterpret_cast<bg_gf32_t>(reinterpret_cast<uintptr_t>(xp));
        }
        if (tid < kBagsSlots) {
            const bool t_on = tid < T;
            s_tb[tid] = t_on ? (unsigned long long)reinterpret_cast<uintptr_t>(tb_v) : 0ull;
            s_ip[tid] = t_on ? (unsigned long long)reinterpret_cast<uintptr_t>(ip_v) : 0ull;
            s_nr[tid] = t_on ? (unsigned)nr_v : 0u;
        }
        if (lane < d) {
#pragma unroll
            for (int u = 0; u < 4; u++) s_x[wave][u][lane] = xr[u];
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int t = (tid >> 4) + 16 * h;
            // every bag a valid [start, end) inside [0, nnz]: one that is not is empty and flagged (as bag_sum_flat_kernel)
            if (!has_next[h]) en[h] = nz[h];
            const bool ok = (st[h] >= 0) & (en[h] >= st[h]) & (en[h] <= nz[h]);
            bad |= on[h] & !ok;
            const bool use = on[h] & ok;
            s_st[t][i] = use ? (int)st[h] : 0;
            s_len[t][i] = use ? (int)(en[h] - st[h]) : 0;
        }
    }
    __syncthreads();
    const int n_samples = nb > wave ? (nb - wave + 3) / 4 : 0;      // wave-uniform
    if (n_samples == 0) {
        if (bad) atomicOr(args.err, 1);
        return;
    }

    // ---- the wave's samples: exclusive prefix of the bag lengths over the tables ------------------------------------------------
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int t = lane & 31;
        int incl = (t < T && u < n_samples) ? s_len[t][wave + 4 * u] : 0;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const int v = __shfl_up(incl, o, 32);
            if (t >= o) incl += v;
        }
        // lane t writes entry t + 1 (lane 31: entry 0)
        if (lane < 32) s_pre[wave][u][(t + 1) & 31] = t == 31 ? 0 : (t < T ? incl : 0x7fffffff);
    }
    EVS_BAGS_WSYNC();

    // ---- lane-invariant mappings -------------------------------------------------------------------------------------------
    // load mapping: LPRD lanes per row, RPI rows per instruction; the lanes past the last whole row (lane 63 at d = 36) mirror the
    // last piece -- the same request, the same value into the same LDS bytes
    const int lane_eff = lane < RPI * LPRD ? lane : RPI * LPRD - 1;
    const int g = lane_eff / LPRD;
    const int piece16 = (lane_eff - g * LPRD) * 16;
    char *my_stage = s_stage[wave];
    char *my_op = s_op[wave];
    float *my_out = reinterpret_cast<float *>(my_stage);
    // owners: item k of this lane is (table it_t[k], piece it_p[k])
    int it_t[kItems], it_p[kItems];
    bg_f32x4 acc[kItems];
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const int wk = lane + 64 * k;
        const int t = wk / LPRD;
        it_t[k] = t < T ? t : -1;
        it_p[k] = (wk - t * LPRD) * 16;
        acc[k] = bg_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // MFMA operand mapping: lane (r16, q) reads k-slot q of rows r16 (+ 16)
    int op_off[NR];
#pragma unroll
    for (int rr = 0; rr < NR; rr++) {
        const int row = r16 + 16 * rr < MAXF ? r16 + 16 * rr : MAXF - 1;   // (rows past F feed accumulator elements nobody stores)
        op_off[rr] = row * OPS;
    }

    // ---- the stage sequence ------------------------------------------------------------------------------------------------
    // a stage = (sample u of this wave, first flattened lookup `base`); every sample has at least one (an all-empty sample: one
    // stage of zero rows), past the wave's last sample they are phantoms that read the zero page
    struct Stage { int u, base, tot; };
    auto total_of = [&](int u) -> int {
        return u < n_samples ? __builtin_amdgcn_readfirstlane(s_pre[wave][u & 3][T]) : 0;
    };
    auto advance = [&](Stage &s) {
        s.base += S;
        if (s.base >= s.tot) { s.u++; s.base = 0; s.tot = total_of(s.u); }
    };
    // indices of a stage: slot j * RPI + g of the stage is lookup base + slot of the sample; its table from the prefix by counting
    // the tables that end at or in front of it (the whole prefix in 7 broadcast reads, shared by the kBagsInstr slots of the lane)
    auto request_idx = [&](const Stage &s, int64_t (&iv)[kBagsInstr], int (&meta)[kBagsInstr]) {
        const bool live = s.u < n_samples;
        const int uu = s.u & 3;
        const int smp = wave + 4 * uu;
        int pre[28];
#pragma unroll
        for (int c = 0; c < 7; c++) {
            const int4 v = *reinterpret_cast<const int4 *>(&s_pre[wave][uu][4 * c]);
            pre[4 * c] = v.x; pre[4 * c + 1] = v.y; pre[4 * c + 2] = v.z; pre[4 * c + 3] = v.w;
        }
#pragma unroll
        for (int j = 0; j < kBagsInstr; j++) {
            const int p = s.base + j * RPI + g;
            int tb = 0;
#pragma unroll
            for (int t = 1; t <= MAXT; t++) tb += pre[t] <= p ? 1 : 0;
            const bool valid = live && p < s.tot;
            tb = tb < MAXT ? tb : MAXT - 1;
            const int pos = s_st[tb][smp] + (p - s_pre[wave][uu][tb]);
            // (bit blend, not a select: no control flow around the load)
            const unsigned long long m = 0ull - (unsigned long long)valid;
            const unsigned long long pa = zeros ^ ((zeros ^ (s_ip[tb] + 8ull * (unsigned long long)(unsigned)pos)) & m);
            iv[j] = *reinterpret_cast<bg_gi64_t>((uintptr_t)pa);
            meta[j] = tb | (valid ? 256 : 0);
        }
    };
    // rows of a stage: an index outside its table reads the zero page and raises the flag
    auto request_rows = [&](const int64_t (&iv)[kBagsInstr], const int (&meta)[kBagsInstr], bg_f32x4 (&rows)[kBagsInstr]) {
#pragma unroll
        for (int j = 0; j < kBagsInstr; j++) {
            const int tb = meta[j] & 255;
            const bool valid = (meta[j] & 256) != 0;
            const bool ok = valid & ((uint64_t)iv[j] < (uint64_t)s_nr[tb]);
            bad |= valid & !ok;
            const unsigned long long zp = zeros + (unsigned long long)piece16;
            const unsigned long long p = s_tb[tb] + (unsigned long long)iv[j] * (unsigned long long)row_bytes + (unsigned long long)piece16;
            const unsigned long long m = 0ull - (unsigned long long)ok;
            const unsigned long long pa = zp ^ ((zp ^ p) & m);
            rows[j] = *reinterpret_cast<bg_gf4_t>((uintptr_t)pa);
        }
    };

    Stage cur{0, 0, total_of(0)};
    Stage nxt = cur; advance(nxt);
    Stage nn = nxt; advance(nn);
    // one set of registers: a stage's rows are in LDS before the next stage's are requested into the same registers, and its
    // indices are consumed by its row requests before the next indices are requested
    int64_t iv[kBagsInstr];
    int meta[kBagsInstr];
    bg_f32x4 rows[kBagsInstr];
    request_idx(cur, iv, meta);
    request_rows(iv, meta, rows);
    request_idx(nxt, iv, meta);

    while (cur.u < n_samples) {
        // stage k: registers -> LDS (slot j * RPI + g, this lane's piece)
#pragma unroll
        for (int j = 0; j < kBagsInstr; j++)
            *reinterpret_cast<bg_f32x4 *>(my_stage + (j * RPI + g) * row_bytes + piece16) = rows[j];
        EVS_BAGS_WSYNC();
        // stage k + 1's rows, then stage k + 2's indices: both in flight while stage k is reduced
        request_rows(iv, meta, rows);
        request_idx(nn, iv, meta);
        const int uu = cur.u;       // (< 4: cur is never a phantom)
#pragma unroll
        for (int k = 0; k < kItems; k++) {
            if (it_t[k] >= 0) {
                int a = s_pre[wave][uu][it_t[k]], b = s_pre[wave][uu][it_t[k] + 1];
                a = a > cur.base ? a : cur.base;
                b = b < cur.base + S ? b : cur.base + S;
                const char *sp = my_stage + it_p[k];
                for (int slot = a - cur.base; slot < b - cur.base; slot++) {     // index order
                    const bg_f32x4 v = *reinterpret_cast<const bg_f32x4 *>(sp + slot * row_bytes);
                    acc[k][0] = __fadd_rn(acc[k][0], v[0]); acc[k][1] = __fadd_rn(acc[k][1], v[1]);
                    acc[k][2] = __fadd_rn(acc[k][2], v[2]); acc[k][3] = __fadd_rn(acc[k][3], v[3]);
                }
            }
        }
        EVS_BAGS_WSYNC();           // the stage's bytes are free again
        if (cur.base + S >= cur.tot) {      // wave-uniform: the sample's last stage -- its pooled rows are complete
            const int64_t b = b0 + wave + 4 * uu;
            // operand slot: row 0 = x[b], row t + 1 = the pooled bag of table t
            if (lane < d) *reinterpret_cast<float *>(my_op + 4 * lane) = s_x[wave][uu][lane];
#pragma unroll
            for (int k = 0; k < kItems; k++) {
                if (it_t[k] >= 0) *reinterpret_cast<bg_f32x4 *>(my_op + (it_t[k] + 1) * OPS + it_p[k]) = acc[k];
                acc[k] = bg_f32x4{0.f, 0.f, 0.f, 0.f};
            }
            EVS_BAGS_WSYNC();
            float4 a[NR][CQ];
            float ar[NR][REM > 0 ? REM : 1];
#pragma unroll
            for (int rr = 0; rr < NR; rr++) {
#pragma unroll
                for (int c = 0; c < CQ; c++) a[rr][c] = *reinterpret_cast<const float4 *>(my_op + op_off[rr] + (q * CQ + c) * 16);
#pragma unroll
                for (int m = 0; m < REM; m++) ar[rr][m] = *reinterpret_cast<const float *>(my_op + op_off[rr] + (4 * CQ + m) * 16 + q * 4);
            }
            const float xv = s_x[wave][uu][lane < d ? lane : 0];
            // Z = T T^T: v_mfma_f32_16x16x4_f32 chains over d / 4 steps, the k order of rf_body
            bg_f32x4 c00 = {0.f, 0.f, 0.f, 0.f}, c10 = c00, c11 = c00;
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
                const float s0 = ar[0][m], s1 = ar[NR - 1][m];
                c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(s0, s0, c00, 0, 0, 0);
                if constexpr (NT == 2) {
                    c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1, s0, c10, 0, 0, 0);
                    c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(s1, s1, c11, 0, 0, 0);
                }
            }
            // the output row, packed in LDS: x bit for bit, then the triangle straight from the accumulators (lane (r16, q) holds
            // Z[4 q + v][r16]); elements nobody stores go to a dump slot behind the row
            const int dump = 4 * (OUT_MAX + r16);
            *reinterpret_cast<float *>(reinterpret_cast<char *>(my_out) + (lane < d ? 4 * lane : dump)) = xv;
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
            EVS_BAGS_WSYNC();
            // contiguous 16-byte-per-lane stores (what lies past the row is dropped by the buffer bounds check), then the 0..3
            // trailing floats
            float *Rb = args.R + b * (int64_t)out_row;
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Rb, 0, out_row * 4, 0x00020000);
            const int n4 = out_row >> 2;
            constexpr int NFL = (((d + MAXF * (MAXF + 1) / 2 + 3) / 4) * 4 + 255) / 256;
#pragma unroll
            for (int h = 0; h < NFL; h++) {
                const int e4 = lane + 64 * h;
                const float4 v = reinterpret_cast<const float4 *>(my_out)[e4 < n4 ? e4 : 0];
                bg_u32x4 w = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
                __builtin_amdgcn_raw_buffer_store_b128(w, rs, e4 < n4 ? 16 * e4 : kOob, 0, kCpol);
            }
            const int e = 4 * n4 + (lane & 3);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(my_out[e]), rs, lane < (out_row & 3) ? 4 * e : kOob, 0, kCpol);
            EVS_BAGS_WSYNC();       // the next stage's rows overwrite the staged row
        }
        cur = nxt; nxt = nn; advance(nn);
    }
    if (bad) atomicOr(args.err, 1);
}

// the dispatch record (evs_bags_fused_kernels_seen): id = (d: 16 / 32 / 36 / 64) * 2 + (NT - 1)
constexpr int kBagsFusedCount = 8;
static std::atomic<long long> g_bags_seen[kBagsFusedCount];

template <int LPRD, int NT>
static void launch_bags(const BagsArgs &a, hipStream_t st) {
    hipLaunchKernelGGL((emb_interact_bags_kernel<LPRD, NT>), dim3((unsigned)((a.B + 15) / 16)), dim3(256), 0, st, a);
}

static int bags_dim_id(int d) { return d == 16 ? 0 : d == 32 ? 1 : d == 36 ? 2 : d == 64 ? 3 : -1; }

}  // namespace evs

extern "C" int evs_bags_fused_stage_rows(int d) {
    return evs::bags_dim_id(d) < 0 ? 0 : evs::kBagsInstr * (64 / (d / 4));
}

extern "C" int evs_bags_fused_kernels_seen(char *buf, int n) {
    constexpr int kD[4] = {16, 32, 36, 64};
    int len = 0;
    if (buf && n > 0) buf[0] = 0;
    for (int id = 0; id < evs::kBagsFusedCount; id++) {
        char line[64];
        const int k = snprintf(line, sizeof line, "bagsf_d%d_nt%d=%lld\n", kD[id / 2], (id & 1) + 1, evs::g_bags_seen[id].load(std::memory_order_relaxed));
        if (buf && len + k < n) memcpy(buf + len, line, (size_t)k + 1);
        len += k;
    }
    return len;
}

extern "C" int evs_emb_interact_bags(int64_t B, int T, int d, const void *const *tables, const int64_t *n_rows, const float *x,
                                     int64_t x_stride, const int64_t *const *indices, const int64_t *nnz, const int64_t *const *offsets,
                                     const int64_t *offsets_len, int itself, float *R, void *stream) {
    using namespace evs;
    const int dim = bags_dim_id(d);
    EVS_REQUIRE(dim >= 0, "evs_emb_interact_bags: no kernel for d=%d (need d in {16,32,36,64})", d);
    EVS_REQUIRE(T >= 1 && T + 1 <= kTileMaxF, "evs_emb_interact_bags: no kernel for T=%d (need 1 <= T <= %d)", T, kTileMaxF - 1);
    EVS_REQUIRE(B >= 0 && B < (1ll << 31), "evs_emb_interact_bags: B=%lld must be in [0, 2^31)", (long long)B);
    if (B == 0) return EVS_OK;
    EVS_REQUIRE(tables && n_rows && x && indices && nnz && offsets && offsets_len && R, "evs_emb_interact_bags: NULL argument");
    EVS_REQUIRE(reinterpret_cast<uintptr_t>(x) % 16 == 0 && x_stride % 4 == 0 && x_stride >= 0 && x_stride < (1ll << 31),
                "evs_emb_interact_bags: x must be 16-byte aligned, x_stride a multiple of 4 in [0, 2^31)");
    const int F = T + 1;
    BagsArgs a;
    memset(&a, 0, sizeof a);
    int64_t lookups = 0;
    for (int t = 0; t < T; t++) {
        EVS_REQUIRE(offsets[t], "evs_emb_interact_bags: offsets[%d] is NULL (bags need their offsets)", t);
        EVS_REQUIRE(offsets_len[t] == B || offsets_len[t] == B + 1, "evs_emb_interact_bags: offsets_len[%d] must be B or B + 1", t);
        EVS_REQUIRE(nnz[t] >= 0 && nnz[t] < (1ll << 31) && n_rows[t] >= 0 && n_rows[t] < (1ll << 31),
                    "evs_emb_interact_bags: table %d: nnz and n_rows must be in [0, 2^31)", t);
        EVS_REQUIRE(indices[t] || nnz[t] == 0, "evs_emb_interact_bags: indices[%d] is NULL with nnz > 0", t);
        EVS_REQUIRE(tables[t] || n_rows[t] == 0, "evs_emb_interact_bags: tables[%d] is NULL", t);
        EVS_REQUIRE(reinterpret_cast<uintptr_t>(tables[t]) % 16 == 0, "evs_emb_interact_bags: tables[%d] must be 16-byte aligned", t);
        lookups += nnz[t];
        a.table[t] = tables[t];
        a.indices[t] = indices[t] ? indices[t] : offsets[t];   // (nnz == 0: a table of empty bags, never dereferenced)
        a.offsets[t] = offsets[t];
        a.nnz[t] = nnz[t]; a.n_rows[t] = n_rows[t]; a.off_len[t] = offsets_len[t];
    }
    EVS_REQUIRE(lookups < (1ll << 31), "evs_emb_interact_bags: %lld lookups in one call (need < 2^31)", (long long)lookups);
    a.x = x; a.x_stride = x_stride; a.R = R; a.B = B; a.T = T; a.itself = itself ? 1 : 0;
    a.P = itself ? F * (F + 1) / 2 : F * (F - 1) / 2;
    a.err = index_error_flag();
    if (!a.err) return EVS_EHIP;
    a.zeros = zero_page();
    if (!a.zeros) return EVS_EHIP;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const bool nt2 = F > 16;
    switch (dim) {
    case 0: if (nt2) launch_bags<4, 2>(a, st); else launch_bags<4, 1>(a, st); break;
    case 1: if (nt2) launch_bags<8, 2>(a, st); else launch_bags<8, 1>(a, st); break;
    case 2: if (nt2) launch_bags<9, 2>(a, st); else launch_bags<9, 1>(a, st); break;
    default: if (nt2) launch_bags<16, 2>(a, st); else launch_bags<16, 1>(a, st); break;
    }
    g_bags_seen[2 * dim + nt2].fetch_add(1, std::memory_order_relaxed);
    EVS_HIP_CHECK(hipGetLastError());
    return EVS_OK;
}
