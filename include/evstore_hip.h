/* evstore_hip.h -- C ABI of libevstore_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the DLRM embedding-lookup + EvLFU cache + feature
 * interaction hot path of ucare-uchicago/ev-store-dlrm.  Plain pointers and
 * sizes only; every pointer marked "device" is HBM memory of the current HIP
 * device, every `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  All entry points return 0 on success and a negative EVS_E* code
 * on failure; evs_last_error() returns a thread-local message.
 *
 * Each group cites the reference interface it replaces (paths relative to the
 * reference tree).
 */
#ifndef EVSTORE_HIP_H
#define EVSTORE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EVS_ABI_VERSION 1
#define EVS_API __attribute__((visibility("default")))

/* error codes */
#define EVS_OK 0
#define EVS_EINVAL (-1)    /* bad argument (shape, alignment, unsupported codec ...) */
#define EVS_EHIP (-2)      /* a HIP runtime call failed */
#define EVS_EINDEX (-3)    /* an index was out of range (see evs_check_index_errors) */
#define EVS_ENOMEM (-4)
#define EVS_ESTATE (-5)    /* call sequence error (e.g. cache not initialised) */
#define EVS_EIO (-6)       /* table file missing / short read */

/* row codecs = the reference's on-disk precisions (SURVEY 8(b) on-disk contracts):
 * 32: raw little-endian fp32                    (script/convert_ev_to_binary.py:58-69)
 * 16: custom ushort affine code                 (mixed_precs_caching/evlfu_16.cpp:332-356)
 *  8: uint8 affine  f=((float)u/254)*2-1        (mixed_precs_caching/evlfu_8.cpp:370-378)
 *  4: 15-entry LUT, two codes per byte, hi first (mixed_precs_caching/evlfu_4.cpp:319-341) */
#define EVS_CODEC_F32 32
#define EVS_CODEC_U16 16
#define EVS_CODEC_U8 8
#define EVS_CODEC_U4 4

#define EVS_MAX_TABLES_PER_LAUNCH 32
#define EVS_MAX_FEATURES 32

EVS_API int evs_abi_version(void);
EVS_API const char *evs_last_error(void);
/* The EVS_* environment switches this process has read so far (every switch is read once, at its dispatch site): one
 * "NAME=1\n" (the variable was set) or "NAME=0\n" (unset: the default) line per name, in first-read order, written to
 * buf (n bytes, always NUL-terminated when n > 0).  Returns the length of the whole text, which may exceed n - 1. */
EVS_API int evs_env_switches_seen(char *buf, int n);
/* Which gather kernels the table-only pooling entry points (evs_embedding_bag_sum and its _sharded / _p2p / _stacked forms)
 * have launched in this process: one "name=count\n" line per launch site and kernel instantiation that their dispatch can
 * reach -- every name is listed, a kernel never launched with count 0 -- in a fixed order; buf, n and the return value as for
 * evs_env_switches_seen.  A count goes up by one per kernel launch (a call over T > EVS_MAX_TABLES_PER_LAUNCH tables: once
 * per launch).  Names, with c = the row codec (32, 16, 8, 4) and lpr = the lanes per row the kernel was COMPILED for
 * (d / 4; 0 = read from the arguments at run time):
 *   rows_c<c>_lpr<l>_nj<n>_check | _declared   rows in registers, whole batches of one-index bags: n load instructions per
 *                                              sample; check = offsets given and checked per block, declared = offsets NULL
 *   long_c32_lpr<l>_k<k>                       a lane group per bag, k rows of it in flight (average bag length >= 2)
 *   flat_c32_lpr<l>_select | _plain            a lane group per lookup, rows through LDS; select = the form for averages above 16
 *   vec_c<c>_lpr<l>_bag1 | _offsets            the grid-stride kernel: everything else with d % 4 == 0 and d <= 256, weights included
 *   scalar_c<c>                                one element per lane: any other d, or an output that is not 16-byte aligned */
EVS_API int evs_gather_kernels_seen(char *buf, int n);
/* The same record for the mixed-precision interaction consumers (csrc/evs_mixed.hip), which evs_interact_rows_by_address and the
 * two-tier lookups with interaction (evs_cache_lookup_interact_c1c2 and its bag / fed forms) launch: one "name=count\n" line per
 * kernel instantiation, all 18 always listed, in a fixed order; buf, n and the return value as for evs_env_switches_seen.
 * Names, with d = 16 / 32 / 36 and nt = the 16-row tiles of the features (1: T + 1 <= 16, 2: T + 1 <= 32):
 *   rows_d<d>_nt<n>          one sample per wave through an fp32 image in LDS: any codec pair
 *   r84_d<d>_nt<n>           rows in registers, codec pair (8, 4), T + 1 <= 28, addresses and classes given
 *   r84_d<d>_nt<n>_probe     the same with the two-tier probe folded into its head (the (8, 4) tier pair's lookup) */
EVS_API int evs_mixed_kernels_seen(char *buf, int n);
/* The same record for the fused gather + interaction + first top-MLP layer (evs_emb_interact_mlp1_stacked): one "name=count\n" line
 * per kernel instantiation, all six always listed, in a fixed order (d = 16, 32, 36; nt = 1 then 2 within each); buf, n and the
 * return value as for evs_env_switches_seen.  A count goes up by one per kernel launch; a refused call and B == 0 launch nothing.
 *   mlp1_d<d>_nt<n>          d = 16 / 32 / 36, nt = the 16-row tiles of the features (1: T + 1 <= 16, 2: T + 1 <= 28) */
EVS_API int evs_mlp1_kernels_seen(char *buf, int n);

/* ---------------------------------------------------------------------------
 * a1: DLRM_Net.apply_emb  (dlrm_s_pytorch.py:407-461)
 *     = T x nn.EmbeddingBag(n_k, d, mode="sum") (dlrm_s_pytorch.py:276) in ONE launch.
 *
 * For every table k and bag b:  out[k][b][:] = sum_{j in bag} decode(W_k[idx_k[j]]) (* w_k[idx_k[j]])
 * bag b of table k = indices[k][ offsets[k][b] .. offsets[k][b+1] ) and the last bag
 * runs to nnz[k] (start offsets only, exactly nn.EmbeddingBag's convention).
 * Summation is in index order, fp32, multiply and add unfused (bit-exact with
 * oracle/evstore_oracle.c:orc_embedding_bag_sum).
 *
 * The four pointer arrays and n_rows/nnz are HOST arrays of length T whose
 * elements are device pointers / sizes.  tables[k]: rows of d elements in the
 * given codec, row-major, row r at byte r*d*codec/8 -- i.e. the bytes of the
 * reference's ev-table-{k+1}.bin, 16-byte aligned.  row_weights may be NULL, or
 * hold NULL entries: row_weights[k] is the per-ROW weight vector v_W_l[k]
 * (dlrm_s_pytorch.py:426 gathers it with the indices).
 * Output element (k,b,c) is written to out[k*out_table_stride + b*out_bag_stride + c];
 * strides are in floats and must be multiples of 4, out 16-byte aligned.
 *   list-of-(B,d) layout:    table_stride = B*d, bag_stride = d
 *   (B,F,d) interaction tile: out = T + d,  table_stride = d, bag_stride = F*d
 * Out-of-range indices contribute nothing and raise a sticky device flag read
 * by evs_check_index_errors() (nn.EmbeddingBag raises; a kernel cannot).
 * offsets == NULL (or every offsets[k] == NULL) states that each bag holds ONE index
 * (offsets = arange(B), what every EVStore script feeds): bag b of table k reads
 * indices[k][b], nnz[k] >= B; the offsets loads in front of the index load go away.
 * ------------------------------------------------------------------------- */
EVS_API int evs_embedding_bag_sum(int T, int64_t B, int d, int codec,
                          const void *const *tables, const int64_t *n_rows,
                          const int64_t *const *indices, const int64_t *const *offsets,
                          const int64_t *nnz, const float *const *row_weights,
                          float *out, int64_t out_table_stride, int64_t out_bag_stride,
                          void *stream);

/* The pool step of the table-sharded forward (dlrm_s_pytorch.py:543-570 distributed_forward: every rank pools ITS
 * tables for the FULL batch, then one all-to-all): evs_embedding_bag_sum with two extensions.
 *   row-split tables (row_lo / row_total, HOST arrays of T, both NULL = whole tables): tables[k] holds the global rows
 *     [row_lo[k], row_lo[k] + n_rows[k]) of a table of row_total[k] rows.  An index inside the table but outside that
 *     range belongs to another rank: it contributes nothing, silently -- the bag's sum over THIS rank's rows is written
 *     (zeros when it has none); only an index outside [0, row_total) raises the sticky flag.
 *   peer-major output (out_peer_stride / bags_per_peer; bags_per_peer <= 0 or >= B = the plain layout): element (k, b, c)
 *     goes to out[(b / bags_per_peer) * out_peer_stride + k * out_table_stride + (b % bags_per_peer) * out_bag_stride + c]
 *     -- the block of the all_to_all_single send buffer that goes to rank b / bags_per_peer (extend_distributed.py:
 *     389-426 builds that buffer with torch.cat; here the gather writes it in place).  Strides in floats, % 4 == 0. */
EVS_API int evs_embedding_bag_sum_sharded(int T, int64_t B, int d, int codec,
                          const void *const *tables, const int64_t *n_rows,
                          const int64_t *row_lo, const int64_t *row_total,
                          const int64_t *const *indices, const int64_t *const *offsets,
                          const int64_t *nnz, const float *const *row_weights,
                          float *out, int64_t out_table_stride, int64_t out_bag_stride,
                          int64_t out_peer_stride, int64_t bags_per_peer, void *stream);

/* ---------------------------------------------------------------------------
 * a15 without a collective call: the exchange step of the table-sharded forward (dlrm_s_pytorch.py:543-570,
 * extend_distributed.py:389-426 All2All_Req, :444-465 All2All_Wait) as direct writes over xGMI.
 *   evs_embedding_bag_sum_p2p   evs_embedding_bag_sum_sharded whose peer-major blocks go STRAIGHT into the peers' receive
 *                               buffers: peer_delta (DEVICE array, one entry per peer, in floats, multiples of 4) is added to
 *                               the local-layout address of peer q's block, i.e. peer_delta[q] = (address of this rank's
 *                               block inside peer q's IPC-mapped receive buffer) - (out + q * out_peer_stride).
 *   evs_p2p_alloc / _free       receive buffers and flag words: fine-grained device memory (a peer's writes are visible to
 *                               this device's loads without a cache flush), zeroed.
 *   evs_p2p_ipc_export / _open / _close   the 64-byte IPC handle of such a buffer, and its mapping in another process
 *                               (hipIpcGetMemHandle / hipIpcOpenMemHandle: the handles cross the process group once).
 *   evs_p2p_sync                one tiny launch: release-store sig_value (system scope) into n_sig words -- flag words in the
 *                               peers' blocks: "use k of your slot holds my block" / "I am through with use k of it" -- then
 *                               wait (acquire loads, bounded: a timeout raises the sticky flag evs_check_index_errors reads,
 *                               EVS_ESTATE) until n_wait words of this rank's own block have reached wait_value.  Host arrays
 *                               of device pointers, at most 64 each.
 * The layout contract is the collective's (what all_to_all_single would have delivered, block for block); sharded.py's
 * exchange_mode = "p2p" drives it, tests/test_p2p_exchange.py pins it against the RCCL / gloo paths.
 * ------------------------------------------------------------------------- */
EVS_API int evs_embedding_bag_sum_p2p(int T, int64_t B, int d, int codec,
                          const void *const *tables, const int64_t *n_rows,
                          const int64_t *row_lo, const int64_t *row_total,
                          const int64_t *const *indices, const int64_t *const *offsets,
                          const int64_t *nnz, const float *const *row_weights,
                          float *out, int64_t out_table_stride, int64_t out_bag_stride,
                          int64_t out_peer_stride, int64_t bags_per_peer, const int64_t *peer_delta, void *stream);
EVS_API int evs_p2p_alloc(void **out, int64_t bytes);
EVS_API int evs_p2p_free(void *p);
EVS_API int evs_p2p_ipc_export(void *p, void *handle64);
EVS_API int evs_p2p_ipc_open(const void *handle64, void **out);
EVS_API int evs_p2p_ipc_close(void *p);
EVS_API int evs_p2p_sync(int n_sig, uint32_t *const *sig, uint32_t sig_value, int n_wait, const uint32_t *const *wait,
                         uint32_t wait_value, void *stream);

/* The loader's collate on the device -- collate_wrapper_criteo_offset, dlrm_data_pytorch.py:397-410 -- from the raw batch as
 * CriteoDataset.__getitem__ yields it (:372-395): x_int (B, n_dense) int32 counts and x_cat (B, T) int32 ids in device
 * memory, sample s at x_int + s * x_int_stride / x_cat + s * x_cat_stride (strides in elements: n_dense / T for separate
 * row-major arrays) -> X (B, n_dense) fp32 = log(x_int + 1) (fp32 add, then logf: within 1-2 ulp of torch.log on the host),
 * lS_i (T, B) int64 = x_cat transposed, lS_o (T, B) int64 = arange(B) per table (lS_o NULL: not written -- the fused launch
 * can be told one_index_per_bag instead).  156 bytes per sample cross the bus instead of 468 (T = 26).
 * The Terabyte binary loader's batches (script/data_loader_terabyte.py:196-236 CriteoBinDataset, :68-87 _transform_features)
 * are one (B, 40) int32 block of the file -- label, 13 counts, 26 ids per record: both strides 40, x_int = block + 1,
 * x_cat = block + 14 -- with ids taken modulo max_ind_range when it is > 0 (:71-72).  1 <= T <= 64. */
EVS_API int evs_collate_criteo_offset(int64_t B, int n_dense, int T, const int32_t *x_int, int64_t x_int_stride, const int32_t *x_cat,
                                      int64_t x_cat_stride, int max_ind_range, float *X, int64_t *lS_o, int64_t *lS_i, void *stream);

/* a16 (dlrm_wrap's per-batch H2D, dlrm_s_pytorch.py:131-147) as a two-stream pipeline: signal words that one stream of a
 * device writes and another waits for (">= value") in stream order, executed by the command processors -- no event, no host
 * wake-up between the copy stream and the compute stream (inference_loop.Prefetcher(copy_stream=True)).
 * evs_signal_alloc: 8 bytes of signal memory, zeroed (EVS_ESTATE when the device has no stream wait-value operations). */
EVS_API int evs_signal_alloc(void **out);
EVS_API int evs_signal_free(void *signal);
EVS_API int evs_stream_write_value(void *stream, void *signal, uint32_t value);
EVS_API int evs_stream_wait_value(void *stream, void *signal, uint32_t value);

/* Row-split tables, receiver side (one index per bag): sample b of table k reads the partial of the rank whose row range
 * holds indices[k][b] -- rank r holds rows [r*n/world, (r+1)*n/world) -- i.e. row  row_off[r] + b  of the partials inside
 * the receive buffer (row_off: HOST array of `world` row offsets, one per source rank).  dst[k][b] (device, int64) receives
 * that row number: the index list of the "gathered" feature the fused interaction kernel then reads.  T <= 32, world <= 64. */
EVS_API int evs_rowsplit_route(int T, int64_t B, int world, const int64_t *const *indices, const int64_t *n_rows,
                               const int64_t *row_off, int64_t *const *dst, void *stream);

/* Same operation for the stacked layout of the Criteo collate
 * (dlrm_data_pytorch.py:397-410: lS_i and lS_o are (T,B) int64 tensors, one row per
 * table): indices[k] = indices_base + k*indices_row_stride (B entries each, i.e.
 * nnz[k] = nnz_per_table), offsets[k] = offsets_base + k*offsets_row_stride.
 * Strides in elements.  Saves the caller from building four T-long pointer arrays
 * per batch.  offsets_base == NULL: one index per bag (as offsets == NULL above). */
EVS_API int evs_embedding_bag_sum_stacked(int T, int64_t B, int d, int codec,
                          const void *const *tables, const int64_t *n_rows,
                          const int64_t *indices_base, int64_t indices_row_stride,
                          int64_t nnz_per_table,
                          const int64_t *offsets_base, int64_t offsets_row_stride,
                          const float *const *row_weights,
                          float *out, int64_t out_table_stride, int64_t out_bag_stride,
                          void *stream);

/* Synchronises `stream`, returns EVS_EINDEX if any launch since the last call saw
 * an out-of-range index (and clears the flag), else 0. */
EVS_API int evs_check_index_errors(void *stream);

/* ---------------------------------------------------------------------------
 * a11: the offline encoders as a GPU batch tool
 *     (script/reduce_precision.py:26-51 u16, :140-172 + :321 u4, :270 u8;
 *      script/convert_ev_to_binary.py:31-69 byte layout)
 * src: n_rows x d fp32 (device), dst: n_rows x (d*codec/8) bytes (device), the
 * reference's ev-table-N.bin layout for that precision.  Bit-exact with the
 * reference's Python arithmetic (fp64 on the widened fp32 values).
 * ------------------------------------------------------------------------- */
EVS_API int evs_encode_table(int codec, int64_t n_rows, int d, const float *src, void *dst, void *stream);

/* Device-side address of a pinned (hipHostMalloc / torch pin_memory) host buffer, NULL when the
 * buffer is not device-accessible.  The batch-1 entry points (evs_cache_request*, ev_lookup) take
 * such pointers for the ids, the rows and the hit flags: a request of 26 ids and 936 floats then
 * crosses the bus inside the kernel -- one launch and one synchronise per request, no copy commands
 * (the reference's loop is one request at a time: cache_manager.cpp:231-237). */
EVS_API void *evs_host_device_pointer(void *host_ptr);

/* ---------------------------------------------------------------------------
 * a3: DLRM_Net.interact_features, arch_interaction_op="dot"
 *     (dlrm_s_pytorch.py:483-516)
 *
 * feats: HOST array of F device pointers; feature f of sample b is the d
 * floats at feats[f] + b*feat_strides[f]  (feats[0] = x, feats[1..] = ly).
 * R: device (B, d + P) row-major, P = F(F-1)/2 (itself=0) or F(F+1)/2 (itself=1):
 *   R[b] = [ x[b] | Z[b][i][j] for i in 0..F-1 for j in 0..i-1(+itself) ],  Z = T.T^T
 * fp32 in, fp32 accumulate on the matrix cores (v_mfma_f32_16x16x4_f32).
 * Requires F <= 32, d % 4 == 0, d <= 256.
 * ------------------------------------------------------------------------- */
EVS_API int evs_interact_dot(int64_t B, int F, int d, const float *const *feats,
                     const int64_t *feat_strides, int itself, float *R, void *stream);

/* ---------------------------------------------------------------------------
 * a4: the apply_emb -> interact_features pair of DLRM_Net.sequential_forward
 *     (dlrm_s_pytorch.py:588-601) as ONE kernel: R = interact_features(x, apply_emb(...)).
 *
 * Every row of the per-sample matrix T[b] (F x d) is described by an evs_feature:
 *   dense    (indices == NULL): the d floats at (const float*)src + b*stride
 *                               -- x, or pooled vectors received from the all-to-all;
 *   indirect (indices != NULL): the sum-pooled bag b of table `src` (row-major rows of d
 *                               elements in `codec`), exactly evs_embedding_bag_sum's
 *                               definition for one table (offsets = B bag starts, the
 *                               last bag runs to nnz; row_weights = per-ROW weights or NULL).
 * feats: HOST array of F entries, feats[0] must be dense (x).  All indirect features
 * share `codec`.  Output as evs_interact_dot.  Requires F <= 32, B < 2^31,
 * evs_fused_dim_supported(d), src 16-byte aligned, dense strides % 4 == 0.
 * The (B,F,d) intermediate is never written.  Pooled sums round exactly as in
 * evs_embedding_bag_sum; dot products are fp32 MFMA chains (rtol 1e-5 vs the oracle).
 * ------------------------------------------------------------------------- */
typedef struct evs_feature {
    const void *src;
    int64_t stride;
    const int64_t *indices;   /* NULL = dense feature -- except: n_rows > 0, nnz == 0 and offsets given = a table whose
                                 bags are all empty in this batch (an empty index array has no address) */
    const int64_t *offsets;   /* indirect: B bag starts; NULL on EVERY indirect feature = one index per bag */
    int64_t nnz;
    int64_t n_rows;
    const float *row_weights;
    int64_t offsets_len;   /* readable entries of `offsets` (>= B); 0 means B.  A batch SLICE of a longer
                              offsets array passes offsets+b0 and offsets_len = B_total-b0: the slice's last
                              bag then ends at offsets[B] instead of nnz. */
} evs_feature;

/* 1 if the fused kernel is built for this embedding dimension (16,32,36,48,64,128). */
EVS_API int evs_fused_dim_supported(int d);

EVS_API int evs_emb_interact_dot(int64_t B, int F, int d, int codec, const evs_feature *feats,
                                 int itself, float *R, void *stream);

/* Stacked-layout form (Criteo collate: indices and offsets are (T,B) int64 tensors, see
 * evs_embedding_bag_sum_stacked): feature 0 = x (B,d) with row stride x_stride floats,
 * feature k+1 = bag-sum over tables[k].  F = T + 1.  offsets_base == NULL declares ONE INDEX PER BAG
 * (the Criteo collate's offsets = arange(B), dlrm_data_pytorch.py:407-408): bag b = indices[k][b]; the
 * offsets stage of the kernel is skipped (fp32 tables, unweighted). */
EVS_API int evs_emb_interact_dot_stacked(int64_t B, int T, int d, int codec,
                                 const void *const *tables, const int64_t *n_rows,
                                 const float *x, int64_t x_stride,
                                 const int64_t *indices_base, int64_t indices_row_stride,
                                 int64_t nnz_per_table,
                                 const int64_t *offsets_base, int64_t offsets_row_stride,
                                 const float *const *row_weights, int itself, float *R, void *stream);

/* K independent batches of B samples in one call (a serving loop's queue): x, indices_base, offsets_base (NULL = one
 * index per bag for every batch) and R are HOST arrays of K device pointers, every batch with the same shape and strides.
 * fp32 tables with d in {16, 32, 36} and T <= 27: ONE launch per 8 batches -- a batch's last blocks drain under the
 * next batch's first ones, the rate a caller alternating two HIP streams gets, with no stream but `stream`; other
 * shapes: K launches.  Bit-identical to K calls of evs_emb_interact_dot_stacked either way. */
EVS_API int evs_emb_interact_dot_stacked_multi(int K, int64_t B, int T, int d, int codec, const void *const *tables,
                                               const int64_t *n_rows, const float *const *x, int64_t x_stride,
                                               const int64_t *const *indices_base, int64_t indices_row_stride,
                                               int64_t nnz_per_table, const int64_t *const *offsets_base,
                                               int64_t offsets_row_stride, int itself, float *const *R, void *stream);
/* The same call -- R = interact_features(x, apply_emb(lS_o, lS_i, emb_l, v_W_l)), lS_o given and checked per 16-sample block
 * (dlrm_s_pytorch.py:596-601; the inference loop calls it once per batch, :801-836) -- through a RESIDENT DISPATCHER (round 6):
 * the latency half of the metric.  A launched-and-waited-for batch spends ~12 us outside its kernel (the launch call, the
 * dispatch of a thousand blocks, the completion signal), and below ~4 000 samples a launch IS that floor.  serve_start keeps
 * the tables (fp32, d in {16, 32, 36, 64}, T <= 27; HBM addresses as evs_emb_interact_dot_stacked takes them) and arms a grid
 * of n_blocks blocks (0 = 4 per CU, at most 4 096) that starts with the first post and STAYS on the device: serve_post writes
 * one 64-byte descriptor (no launch: ~1 us of host time) and returns a ticket -- where the host can address device memory
 * (large BAR) straight into the lines in device memory the blocks poll, through the PCIe aperture; elsewhere
 * (or EVS_SERVE_PUBLISH=leader) into a ring in pinned host memory that the grid's leader wavefront reads over the bus and
 * republishes on the device --, every block runs the chunks that fall to it with the very body of the launched kernel (same
 * bits), R is written through to memory, the blocks that complete the batch's arrival counters write the ticket into an
 * answer line in host memory and serve_wait spins on that.  Up to 64 batches may be in flight (a post blocks on the batch 64
 * tickets back); consecutive small batches land on different blocks and overlap.
 *   WHAT THE CALLER GUARANTEES: x / lS_i / lS_o of a batch are complete when it is posted (no stream orders a post), R may be
 *   read by anything STARTED after serve_wait has returned, and nothing else needs the GPU urgently while the grid is
 *   resident -- it holds its compute units; it leaves by itself after idle_us without a post (the next post starts it again;
 *   a device-wide synchronise elsewhere waits that long), and serve_stop sends it home at once.
 * Out-of-range indices / bad offsets: skipped and flagged exactly as the launch form does (evs_check_index_errors).
 * x: 16-byte aligned, row stride a multiple of 4 floats; lS_i / lS_o: (T, B) int64 with unit inner stride, given by the address of
 * row 0 and the elements between two rows; one server is driven by ONE host thread (posts and waits are not locked). */
typedef struct evs_rf_server evs_rf_server;
EVS_API int evs_emb_interact_serve_start(evs_rf_server **out, int T, int d, const void *const *tables, const int64_t *n_rows,
                                         int itself, int n_blocks, int64_t idle_us);
EVS_API int evs_emb_interact_serve_post(evs_rf_server *s, int64_t B, const float *x, int64_t x_stride,
                                        const int64_t *indices_base, int64_t indices_row_stride,
                                        const int64_t *offsets_base, int64_t offsets_row_stride, float *R, uint64_t *ticket);
EVS_API int evs_emb_interact_serve_wait(evs_rf_server *s, uint64_t ticket);
/* which front end this server runs: 1 = host-published (descriptors through the PCIe aperture), 0 = the leader's mailbox */
EVS_API int evs_emb_interact_serve_mode(evs_rf_server *s);
EVS_API int evs_emb_interact_serve_stop(evs_rf_server *s);
EVS_API int evs_emb_interact_serve_destroy(evs_rf_server *s);
/* SURVEY 8(f).3, second half: the apply_emb -> interact_features -> FIRST top-MLP layer chain of
 * DLRM_Net.sequential_forward (dlrm_s_pytorch.py:596-605) in one launch: Z1 = act(R W1^T + b1), act = ReLU when relu != 0
 * (create_mlp, dlrm_s_pytorch.py:205-245: nn.Linear + nn.ReLU).  The interaction rows of 16 samples stay in LDS and feed
 * fp32 MFMA tiles against W1; R reaches HBM only when R != NULL.  One index per bag (indices (T,B) int64, bag b = index b),
 * fp32 tables, d in {16, 32, 36}, T <= 27.  w1_padded: W1 (n1 x K row-major, K = d + P) zero-padded to ((n1 + 15) / 16 * 16)
 * rows of kp = (K + 15) / 16 * 16 floats, 16-byte aligned; b1: n1 floats; Z1: (B, n1) fp32. */
EVS_API int evs_emb_interact_mlp1_stacked(int64_t B, int T, int d, const void *const *tables, const int64_t *n_rows,
                                          const float *x, int64_t x_stride, const int64_t *indices_base,
                                          int64_t indices_row_stride, int itself, const float *w1_padded, int kp,
                                          const float *b1, int n1, int relu, float *Z1, float *R, void *stream);

/* The interaction over x and T rows given BY ADDRESS, each in one of two precisions: what the two-tier lookups with interaction
 * run over the rows their probe finds (csrc/evs_mixed.hip), as an entry point of its own.
 *   R[b] = [ x[b] | Z[b][i][j] for i in 0..T for j in 0..i-1(+itself) ],  Z = M M^T,  M = (x[b]; row (b, 0); ...; row (b, T - 1))
 * x: device, sample b at x + b * x_stride (floats), 16-byte aligned, x_stride a multiple of 4 and >= d.
 * row_ptrs: device (B, T) int64 row-major: element (b, k) is the DEVICE ADDRESS of the row feature k + 1 of sample b takes.
 * row_class: device (B, T) uint8, same layout: 1 = the row is in codec1, 2 = in codec2, 0 = no row.  NULL: every row is of class
 * default_class (1 or 2).  Address 0 or class 0 -- either alone -- means a row of zeros: nothing is read for it.  The classes are device
 * data the host cannot check: a value other than 0, 1 or 2 is undefined (the row is then decoded by one of the two codecs, which one
 * depends on the kernel).
 * A row is d elements, row-major: 4 d bytes (codec 32, fp32), 2 d (16), d (8), d / 2 (4: two codes per byte, high nibble first).
 * Alignment the kernels assume: every row address is a 16-byte aligned base plus a multiple of the row size of its codec -- what
 * the rows of a cache arena or of a backing table have.  (For d = 36 that makes a u4 row 2-byte and a u8 row 4-byte aligned.)
 * The kernels read no byte outside a row they are given.
 * R: device (B, d + P) row-major, 16-byte aligned, P = F (F - 1) / 2 (itself = 0) or F (F + 1) / 2 with F = T + 1; as evs_interact_dot.
 * Checked on the host (EVS_EINVAL, nothing launched): d in {16, 32, 36}; 1 <= T <= 31; both codecs in {32, 16, 8, 4}; default_class
 * 1 or 2; 0 <= B < 2^31; x, R, row_ptrs not NULL and aligned as above.  B == 0 is success and touches nothing.
 * Which kernel runs is the library's choice (evs_mixed_kernels_seen tells): rows in registers for the pair (8, 4) with T <= 27, one
 * sample per wave through LDS otherwise. */
EVS_API int evs_interact_rows_by_address(int64_t B, int T, int d, const float *x, int64_t x_stride, const int64_t *row_ptrs,
                                         const unsigned char *row_class, int codec1, int codec2, int itself, int default_class,
                                         float *R, void *stream);

/* "cat" interaction (dlrm_s_pytorch.py:506-508): R[b] = [x[b] | ly_0[b] | ...], (B, F*d). */
EVS_API int evs_interact_cat(int64_t B, int F, int d, const float *const *feats,
                     const int64_t *feat_strides, float *R, void *stream);

/* ---------------------------------------------------------------------------
 * a6/a7/a8: the cache tier, GPU resident.
 *   EvLFU: cache_algo/EvLFU_C1.py:21-166 (init/set/update_agg_hit/update/request_to_ev_lfu)
 *   LRU:   cache_algo/LRU.py:14-64        LFU: cache_algo/LFU.py:12-95
 * policy: 0 EvLFU, 1 LRU, 2 LFU.  capacity in ENTRIES (--cache-size).  n_tables keys per
 * request (<= 64), table = position, key = (table_1based, row).
 * EvLFU constants: (flush_rate, perfect_item_cap, flush_extra, perfect_mode) =
 *   (0.3, 0.95, 1, 0) cache_algo/EvLFU_C1.py:18-19,:40,:43
 *   (0.3, 0.95, 0, 2) mixed_precs_caching/evlfu_8.hpp:50-51, evlfu_8.cpp:256-270
 *   (0.4, 1.0, 1, 1)  cache_algo/EvLFU_C1_Cython/EvLFU.cpp:12-13,:80-86
 * Rows are cached in the table's codec (arena bytes = capacity * dim*codec/8) and
 * decoded to fp32 on output.  The hash table, priority lists and arena live in HBM.
 * ------------------------------------------------------------------------- */
typedef struct evs_cache evs_cache;
EVS_API int evs_cache_create(evs_cache **out, int policy, int64_t capacity, int n_tables, int dim, int codec,
                             double flush_rate, double perfect_item_cap, int flush_extra, int perfect_mode);
EVS_API int evs_cache_destroy(evs_cache *c);
/* Miss path: tables[k] is DEVICE-ACCESSIBLE memory holding table k in the cache's codec
 * (HBM, or pinned host memory mapped into the device = the host-mmap miss tier,
 * emb_storage/mmap_file_read.py / evlfu_8.cpp:191-250); HOST arrays of n_tables entries.
 * With host-memory tables the batched lookups (one tier, or the two- / three-tier forms) fetch
 * each missing row once (de-duplicated, into the arena) and serve the whole batch from HBM; hits
 * of the running batch are never evicted by it. */
EVS_API int evs_cache_set_backing(evs_cache *c, const void *const *tables, const int64_t *n_rows);
/* B requests replayed strictly in order (exact reference semantics; B=1 is the reference's
 * request_to_ev_lfu / request_to_lru / request_to_lfu).  rows: device (B, n_tables) int32;
 * out: device (B, n_tables, dim) fp32; hit: device (B, n_tables) bytes (0/1).
 * approx_thres > 0: EvLFU approximate mode (EvLFU_C1.py:122-125,:142-152). */
EVS_API int evs_cache_request(evs_cache *c, int64_t B, const int32_t *rows, float *out, uint8_t *hit,
                              int approx_thres, void *stream);
/* a9: two-tier request, mixed_precs_caching/evlfu_8.cpp:669-796 (request_to_c1_c2): C1 = main
 * precision tier, C2 = secondary precision tier, both EvLFU caches created with the
 * mixed_precs_caching constants (0.3, 0.95, 0, 2), each with its own backing tables in its own
 * codec.  tier (device, (B,n_tables) bytes): 1 = C1 hit, 2 = C2 hit, 0 = miss.  When C1 is full and
 * the combined agg_hit < high_agghit_threshold (23, evlfu_8.hpp:70) double misses with odd table
 * index go to C1, even ones to C2; at or above the threshold all go to C2; while C1 is not full
 * every C1 miss goes to C1 and C2 is left untouched.  Victims are FIFO-oldest (the C++ evicts in
 * unordered_set order); perfect requests are counted in c1's n_perfect_hits. */
EVS_API int evs_cache_request_c1c2(evs_cache *c1, evs_cache *c2, int64_t B, const int32_t *rows, float *out,
                                   uint8_t *tier, int high_agghit_threshold, void *stream);
/* The exact policy as a RESIDENT SERVER on the GPU (round 5) -- the reference serves one request at a time
 * (cache_algo/EvLFU_C1.py:97-166, dlrm_s_pytorch_C1.py:227-275, cpp_socket_client.py:129-157), where evs_cache_request
 * costs a launch and a synchronise per request on top of the request itself.  evs_cache_serve_start arms a one-wavefront
 * kernel (the same code as evs_cache_request's: same hit flags, rows, list order) that stays on the device and takes requests
 * from a mailbox in pinned host memory: the host writes the T ids and a sequence number into one 128-byte line, the server
 * polls that line over the bus, runs the request, writes the T x dim fp32 rows into slot (sequence % n_slots) of `ring`
 * (DEVICE memory, n_slots x T x dim floats: the caller gets device rows without a launch, a copy or a synchronise) and the
 * hit flags + the sequence number into a host line the caller spins on.  evs_cache_serve_request blocks until the answer is
 * there (hit: T bytes on the host; *slot_out: which ring slot holds the rows).
 * HOW LONG A SLOT'S ROWS STAY VALID: the server overwrites slot s when the request n_slots later is POSTED -- host order,
 * not the order of the caller's stream.  A caller that enqueues its reads of the slot (a copy, a kernel) on a stream and does
 * not synchronise must say so: evs_cache_serve_consumed(c, slot, stream) records an event behind those reads, and the request
 * that is about to hand the slot out again waits for it on the host.  Without that call the caller has to have FINISHED
 * reading a slot before it posts the (n_slots - 1)-th request after it.
 * An idle server leaves by itself after idle_us (a device-wide synchronise elsewhere -- hipDeviceSynchronize,
 * torch.cuda.synchronize -- waits for it, i.e. up to idle_us longer than it otherwise would) and is
 * started again by the next request; evs_cache_stats / _dump / _request / _request_c1c2 / _set_backing / _reset_counters /
 * _destroy send it home first (it writes the policy state back on its way out), and a server started after an exact-path
 * launch waits for that launch on its own stream.  A request that fails (EVS_EHIP: the server did not answer / could not be
 * started) leaves host and device agreeing on the sequence number, so the next request is a fresh one.
 * At most 28 tables (the 128-byte request line: four 32-byte sectors of seven ids and a guard word each -- ids are accepted
 * only from a sector whose guard holds the number awaited, whatever granularity the bus delivers the line in);
 * EVS_ESTATE for a cache on the batched path. */
EVS_API int evs_cache_serve_start(evs_cache *c, int approx_thres, float *ring, int n_slots, int64_t idle_us);
EVS_API int evs_cache_serve_request(evs_cache *c, const int32_t *rows_host, uint8_t *hit_host, int *slot_out);
/* ... with the T ids given by ADDRESS (round 6): ids_dev[t * ids_stride], int64 in device memory -- element 0 of each row of the
 * (T, B) lS_i the reference's loop has moved to the GPU (dlrm_wrap, dlrm_s_pytorch.py:131-147; apply_emb_evstore then takes it back
 * with lS_i.cpu(), dlrm_s_pytorch_C1.py:233-239: a copy and a synchronise per request).  The server reads the ids itself; they
 * must be complete when the call is made. */
EVS_API int evs_cache_serve_request_dev(evs_cache *c, const int64_t *ids_dev, int64_t ids_stride, uint8_t *hit_host, int *slot_out);
/* ... with the rows delivered to a DEVICE buffer of the caller's (out_dev: T x dim floats) instead of a ring slot (round 6): what
 * the reference's loop wants is a fresh tensor per request (EvLFU_C1.py:157-161 builds 26 of them), and copying the slot into
 * one was a launch and an event per request.  Exactly one of rows_host / ids_dev (+ ids_stride, as above) is given; at most 26
 * tables (the address rides in the line's last two id words).  Nothing orders the server's stores against the caller's
 * streams: out_dev must not be in use by work still pending when the call is made (a block a stream-ordered allocator has just
 * handed out counts as in use until that stream is idle), and holds the rows when the call returns. */
EVS_API int evs_cache_serve_request_to(evs_cache *c, const int32_t *rows_host, const int64_t *ids_dev, int64_t ids_stride, float *out_dev, uint8_t *hit_host);
EVS_API int evs_cache_serve_consumed(evs_cache *c, int slot, void *stream);
EVS_API int evs_cache_serve_stop(evs_cache *c);
/* Batched EvLFU lookup with snapshot semantics (the throughput path; no reference counterpart --
 * the reference is batch-1): all B requests are probed against the cache as it is when the call
 * starts, rows are served at once (arena for hits, backing for misses: always exactly the table
 * rows), then priorities are raised (atomicMax to agg_hit), the batch's unique misses are inserted
 * and the lowest priorities are evicted to make room (+ the EvLFU flush rule per batch).
 * Same argument layout as evs_cache_request.  A cache object is driven either by
 * evs_cache_request (exact) or by evs_cache_lookup_batch, never both (EVS_ESTATE). */
EVS_API int evs_cache_lookup_batch(evs_cache *c, int64_t B, const int32_t *rows, float *out, uint8_t *hit,
                                   void *stream);
/* How the batched path of this cache makes room (before its first batched call; EVS_ESTATE afterwards).  A cache that
 * is not given a policy decides at its first batched call: EVS_CACHE_POLICY = plan | sampled | setassoc in the environment,
 * else 2 where it applies (tiers whose tables the kernels read in place from HBM, capacity >= 8: a single tier, or BOTH tiers
 * of a two- / three-tier lookup -- a pair is all set-associative or not at all) and 1 elsewhere.
 *   2 "setassoc": the cache is 8-way set-associative.  A key is its dense row number over all tables, permuted (a
 *     bijection of [0, 2^b)), then SPLIT: set = x mod nset, tag = x div nset -- (set, tag) IS the key, so a way is one
 *     32-bit word (priority 6 bits | batch stamp | tag + 1) and a set 32 bytes; way w of set s owns arena row 8 s + w.
 *     A probe reads that record; the update kernel's thread that inserts a new key takes the lowest priority OF THE KEY'S
 *     OWN SET (free ways first) with one CAS and writes the row.  No hash chains, tombstones, sweeps or entry arrays.
 *     capacity / 8 sets (up to 7 entries of the capacity unused); fewer than 2^32 rows over all tables; tables in HBM
 *     (host-memory / file-backed tables: EVS_ESTATE).
 *     A tier ALONE keeps TWO arena rows per way (round 5; bit 25 of the way word names the live one, a replacement writes the
 *     other and flips the bit with the CAS that installs the key), and on such a tier evs_cache_lookup_interact with fp32
 *     rows makes the policy update INSIDE its one launch: the thread that misses a key claims a way of the key's set right
 *     there (one CAS beside the priority raises) and the lanes that gather the key's row for the interaction store it into
 *     the arena -- no miss lists, no update launch (37-38 -> 32-33 us per 16 384-batch at the 10 % Kaggle cache).  What that
 *     changes: a way filled by the running batch carries the batch's stamp and is a MISS for every prober of the same launch
 *     (its row may not be there yet: the key is served from its table), and a key that was resident when the batch arrived
 *     can be retired by one of the batch's own inserts before a later block looks for it.  So under this form a hit flag
 *     says "served from the cache": flag = 1 => the key was resident when the batch arrived (always); flag = 0 => it was not,
 *     OR one of this batch's inserts retired it first (at most as many keys as the batch evicted; the row is then served from
 *     the table, exact as ever, and the key is inserted again like any other miss), OR its way was FILLED k 2^S batches ago,
 *     k >= 1: the stamp is the batch number modulo 2^S (S = 26 - 1 - tag bits), so such a way carries the running batch's
 *     stamp and is hidden from this launch's probers like one the batch filled itself.  The row is served from the table,
 *     exact as ever; the request's agg_hit does not count the key; the insert that follows the miss finds the key in its set
 *     and leaves the way as it is (priority folded, stamp unchanged), so the key is hidden again 2^S batches later.  The form
 *     is taken only with S >= 8: a resident key is hidden in one batch of 2^S, those whose number shares the residue of the
 *     batch that filled it -- at most one lookup in 256.  Keys inserted by batch k are hits from batch k + 1 on (batches
 *     k + j 2^S excepted).  Everything listed under "WHAT IS THE SAME" below holds unchanged.  EVS_CACHE_INLINE=0 (environment)
 *     keeps the update as a launch of its own behind the probe: strict snapshot flags, as evs_cache_lookup_batch always has.
 *     (A single reduced-precision tier -- codec 16 / 8 / 4, d in {16, 32, 36} -- takes the same one-launch form.)
 *     A C1 + C2 pair that starts out together SHARES its set records: one
 *     128-byte line per set index holds C1's 8 ways and C2's ways (two 8-way sub-sets, picked by one more bit of the
 *     quotient, for the reference's 1 : 2 capacity split, evlfu_8.cpp:63-78), so a key's two tier probes are ONE line
 *     request; the routing rule's "while C1 is not full" (evlfu_8.cpp:570-601) is read PER KEY: a double miss goes to C1
 *     while the key's own C1 set has a free way, and by the agg_hit / odd-even rule once it has none (the hashed forms
 *     read it off the tier's entry count);
 *   1 "sampled": a hash over an entry arena; one kernel after the consumers -- the thread that inserts a new key picks
 *     that key's victim itself, the lowest priority of one sampled group of 8 entries (free entries first);
 *   0 "plan": insert -> plan -> evict -> assign -> close, the lowest priorities of a clock-hand window go, exactly as
 *     many as the batch needs (the file-backed miss tier always takes this form).
 * WHAT IS THE SAME under all three, and tested: served rows are exactly the table rows; hit flags are residency when the
 * batch arrives (snapshot; the one-launch form of policy 2: see there); no duplicate keys; size <= capacity; priorities only rise (monotone max of agg_hit,
 * cache_algo/EvLFU_C1.py:65-79); the EvLFU flush fires when the top bucket reaches max_perfect (:36-44).
 * WHAT DIFFERS from the reference's sequential EvLFU (:97-166 evicts the FIFO-oldest entry of the globally lowest
 * bucket): 0 evicts the lowest priorities of a window, 1 the lowest of 8 sampled entries, 2 the lowest of the key's set --
 * under 1 and 2 a key that was HIT in the running batch can be a victim while lower priorities exist elsewhere, and
 * under 2 a set that receives more new keys than it has ways in one batch turns the rest away (they are served from
 * the tables and not cached this time); which keys are resident after a batch depends on thread timing under 1 and 2.
 * Hit rate at the 10 % Criteo-Kaggle cache (Zipf 0.75, B = 16 384, 600 batches): 0 0.8868, 1 0.8862, 2 0.8840, the
 * sequential oracle on the same stream 0.884 (tests/test_gpu_fullsize.py asserts |batched - sequential| <= 0.01 over
 * ten batches at full size for all three; bench.py: cache_tier.hit_rate_vs_sequential_oracle).
 *
 * LRU AND LFU CACHES (evs_cache_create policy 1 / 2) take the batched path under policy 2 only -- a cache that was given no
 * policy resolves to it; 0 and 1 are refused (EVS_EINVAL) -- as a single tier over tables in HBM, fp32 or 16 / 8 / 4-bit
 * codec, 8 ways per set (csrc/evs_cache_policy.hip).  Set geometry, key permutation, tag field and the copy-select bit of
 * the two-copy arena are the ones above, so evs_cache_batch_dump, evs_cache_update_rows and evs_cache_refresh_rows read such
 * a tier unchanged; the bits above the tag hold `last`, the number of the batch that touched the way last, modulo 2^S, and
 * for LFU a saturating 6-bit counter (1..63) in the six top bits.  LRU has no counter and its `last` takes those six bits
 * too: S = 32 - tag bits - 1 (the copy-select bit; it is free, S one more, on the tiny geometries whose tags leave no room
 * for it) for LRU, S = 26 - tag bits - 1 for LFU.  The 10 % Criteo-Kaggle tier (2^26 keys over 422 032 sets: tag + 1 <= 160,
 * 8 tag bits) has S = 23 under LRU and S = 17 under LFU.  Ages are CIRCULAR, age = (n - last) mod 2^S:
 * LRU orders correctly any two ways both touched within the last 2^S - 1 batches (a way left alone for longer looks
 * younger than it is; one whose `last` equals n modulo 2^S looks touched by the running batch and is passed over once).
 * The same reading holds in step 2 below: a HIT on a way whose `last` equals n modulo 2^S -- last touched k 2^S batches ago
 * -- finds the way stamped n already and leaves `last` and, under LFU, the counter as they are (one count lost per 2^S batches
 * of silence, the flag and the served row unaffected); and in step 3 a set whose other ways were all touched by batch n
 * turns a new key away although that way is stale.  S >= 4 always; the Kaggle tiers above wrap every 2^17 batches (LFU).
 * THE BATCHED RULE.  n = the cache's batch number (1, 2, ...).  One call (evs_cache_lookup_batch / _lookup_interact) does:
 *   1. probe (snapshot): hit[b, t] = 1 exactly when key (t + 1, rows[b, t]) was resident when the call started.  Served rows
 *      are exactly the table rows (R: the usual float64-scaled bound).
 *   2. touch: every way hit at least once in this batch gets last = n; under LFU its counter also goes up by ONE PER BATCH,
 *      not one per occurrence, saturating at 63.  Per-batch counting makes the touched word a pure function of the word of
 *      before the batch, so the probe launch writes it with a plain 4-byte store, skipped once the way carries stamp n: every
 *      writer stores the same word (counting occurrences would put thousands of same-address atomics per batch on a hot key
 *      and saturate the counter within one batch anyway).
 *   3. insert: every distinct missed key is inserted once, into its own set.  Free ways first, lowest way index first.
 *      Otherwise the victim is chosen among the ways with last != n -- a way touched or filled by the running batch is never
 *      a victim -- LRU: the oldest `last` by circular age; LFU: the lowest counter, ties to the oldest `last`; remaining
 *      ties to the lowest way index.  No eligible way: the key is turned away (served from its table, not cached this time).
 *      A new way gets last = n and counter 1.  When several new keys of one batch fall into one set, which key takes which
 *      way may depend on timing; each of them still evicts only an eligible way, and no key is ever resident twice.
 *   4. counters: evs_cache_batch_stats keeps its meaning; n_flush stays 0, n_perfect_hits counts all-hit requests,
 *      hist[0] = size and the rest 0.  evs_cache_batch_dump's first column is the way's score -- LRU: its age in batches
 *      (0 = touched by the latest batch), LFU: its counter.
 * evs_cache_lookup_interact on such a tier always runs probe, the row-id / pointer-table interaction consumer and insert as
 * three launches (strict snapshot flags); evs_cache_set_inline_update(c, 1) is refused (EVS_EINVAL), on = 0 accepted.  Also
 * refused, with a message that names the policy and the cache left usable: host-memory or file-backed tables (EVS_ESTATE), a
 * capacity below 8, 2^32 rows or more over all tables, R / 2^22 sets or fewer with R the row total rounded up to a power of two
 * (the tag would leave the stamp fewer than 4 bits; an EvLFU cache that was given no policy resolves to policy 1 there, an
 * explicit policy 2 is refused the same way), the tier as a member of a C1 + C2 (+ C3) lookup (EVS_EINVAL). */
EVS_API int evs_cache_set_batch_policy(evs_cache *c, int policy);
/* Batched two-tier lookup, snapshot semantics: the throughput form of evs_cache_request_c1c2 (no reference
 * counterpart).  Every key is probed in C1, then in C2, against the tiers as they stand when the call starts;
 * agg_hit of a request counts keys found in either tier; a hit is served, and its priority raised, in the tier
 * that holds it; a double miss is routed by the reference's rule (evlfu_8.cpp:570-601) evaluated on the snapshot
 * -- C1 not full: C1; C1 full and agg_hit < threshold: odd table index -> C1, even -> C2; else C2 -- served from
 * the destination tier's backing table at that tier's precision and inserted there once per batch.  out: (B,T,dim)
 * fp32; tier (B,T): 1 = C1 hit, 2 = C2 hit, 0 = miss.  Both caches take the batched path from then on.  One index per table
 * and sample; ragged bags (multi-hot features) go through evs_cache_lookup_bags_c1c2 / _lookup_bags_interact_c1c2.
 * MISS TIERS OUTSIDE HBM (BASELINE configs[4] composed; the reference's tiers read their misses from files inside the
 * request: evlfu_8.cpp:380-414 get_from_file, reader pool :191-250, :603-625): either tier may sit over pinned host tables
 * (evs_cache_set_backing) or file-backed ones (evs_cache_set_file_backing).  The pair then runs: probe (this batch's hits
 * and served alt rows are pinned in their arenas) -> both tiers' policy updates, each missing row fetched ONCE into its
 * tier's arena (over the bus by the thread that inserts it; staged tables: by the host's reader pool, de-duplicated) ->
 * every missed position re-pointed at the arena / staged copy -> the consumers.  Policies: "sampled" over device-visible
 * tables (pinned, registered), "plan" on BOTH tiers as soon as one has staged tables; "setassoc": EVS_ESTATE.  A position
 * whose key another request of the batch routed to C1 (odd tables only) is served C1's copy at C1's precision.
 * THE FETCH-FIRST PAIR.  A pair whose BOTH tiers were told evs_cache_set_miss_order(c, 1) before their first batched call runs
 * this call and evs_cache_lookup_interact_c1c2 as the set-associative pair over the shared 128-byte set record wherever the
 * tables of either tier live -- HBM or device-addressable host memory -- on one stream, in this order:
 *   1. the EvLFU flush an earlier close asked for;
 *   2. the unfolded probe: 8-byte row addresses, the serve byte, the tier codes, the per-tier miss lists, hit ways raised;
 *   3. the route filter and the pair's update launch (every missing row crosses the bus once, here);
 *   4. sa_repoint2 (below);
 *   5. the consumers through the pointer table;
 *   6. the close bookkeeping.
 * The folded probe is not taken.  Observable results equal what order 0 gives for the same calls: tier codes (strict snapshot),
 * the bits of out, both tiers' evs_cache_batch_dump and evs_cache_batch_stats with hist, the exported state -- the update reads
 * the same words in either order, the consumers write nothing it reads.  (R comes from the unfolded consumer: the usual
 * float64-scaled bound, not order 0's folded kernel bit for bit.)
 * The pair keeps ONE arena row per way, so a way the batch hit can be that batch's victim and hold another key's row by the time
 * the consumers run.  Hits are NOT stamped against that (the tier state would differ from order 0's).  Instead step 4 makes every
 * position's address true again from the set record as the update left it; with d the position's serve byte (1 or 2) it searches
 * tier d's ways of the key's set, and only tier d's (C2's sub-set included; both tiers' ways are one line):
 *   code 0, index in range   found: the address becomes tier d's arena row.  Not found -- the key was turned away, or, on an odd
 *                            table, routed both ways and given to C1 while this position was routed to C2 --: it stays tier d's
 *                            table row, read in place.  Either way the bytes are tier d's table row in tier d's codec.
 *   code 1 / 2               found: nothing is stored.  Not found (this call's update took the way): the address becomes tier
 *                            d's backing-table row -- served rows are exactly the table rows, so the bytes are those the arena held.
 *   bad index / serve byte 0 untouched: code 0, a zero row, counted nowhere; the launch raises the sticky index-error flag
 *                            (evs_check_index_errors) for it, which the order-0 (B, T) chains do not.
 * The kernel writes no way word, does no atomic on a record and reads no table.  evs_cache_fetch_stats(c1, ...) reports its totals.
 * The envelope, checked before anything is allocated, the pair left usable, the message naming the policy (a policy that was
 * only resolved there is forgotten again):
 *   order      both tiers at order 1; one of them: EVS_EINVAL ("a tier alone").
 *   policy     batch policy 2 on both, given or resolved -- a pair that was given none takes it wherever its tables live;
 *              plan / sampled, given or from EVS_CACHE_POLICY: EVS_EINVAL.
 *   record     the shared set record: two fresh tiers that start out together with at least 4 ways each.  EVS_SA_PAIR=0, a tier
 *              that was used alone before, capacities without such a record: EVS_EINVAL.
 *   tables     file-backed: EVS_ESTATE.
 *   tiers      no alt-key tier (the _c1c2c3 forms: EVS_EINVAL); an approximate threshold on a tier keeps its EVS_EINVAL.
 * evs_cache_pair_export / evs_cache_pair_load take such a pair over HBM tables (state version 3, unchanged; over host tables:
 * EVS_ESTATE).
 * THE FETCH-FIRST PAIR OVER BAGS.  evs_cache_lookup_bags_c1c2 / _lookup_bags_interact_c1c2 take such a pair once BOTH tiers have also
 * been told evs_cache_set_bag_count(c, 1) ("count first"): the rule, the chain and the envelope are written at
 * evs_cache_lookup_bags_c1c2 ("THE FETCH-FIRST BAG CHAIN").  Without count-first on both tiers the bag form keeps its EVS_EINVAL. */
EVS_API int evs_cache_lookup_batch_c1c2(evs_cache *c1, evs_cache *c2, int64_t B, const int32_t *rows, float *out,
                                        uint8_t *tier, int high_agghit_threshold, void *stream);
/* The same two-tier snapshot lookup with the interaction as its consumer (BASELINE configs[4] end to end):
 * R = interact_features(x, rows) with every row decoded from the precision of the tier that serves it inside the
 * interaction kernel -- the fp32 (B,T,d) rows are never materialised.  d in {16, 32, 36}, T <= 31. */
EVS_API int evs_cache_lookup_interact_c1c2(evs_cache *c1, evs_cache *c2, int64_t B, const int32_t *rows, const float *x,
                                           int64_t x_stride, int itself, float *R, uint8_t *tier,
                                           int high_agghit_threshold, void *stream);
/* Batched THREE-tier lookup: the two calls above with the alt-key tier C3 (the throughput form of request_to_c1_c2_c3,
 * evlfu_8.cpp:492-667; no reference counterpart).  A double miss whose key is a member of C3 and whose alt row is
 * resident in C1 (else C2) when the call starts is served that row -- tier code 3, decoded at the precision of the
 * tier holding it; its recency flag is set, the request's agg_hit counts it, nothing is inserted for it.  The keys
 * this batch's policy update EVICTS (not flushes) from C1 / C2 become members of C3, visible from the next batch on.
 * In this form C3 is an 8-way set-associative key set with second chance inside each set (the alt key of a key is a
 * pure function of the key: the tier only has to remember WHICH keys it knows): one line and one CAS per operation,
 * no global FIFO -- the exact FIFO order is the batch-1 machine's (evs_cache_request_c1c2c3, evs_aprx_apply_ops).
 * A tier object is driven by one of the two forms, never both (EVS_ESTATE). */
typedef struct evs_aprx evs_aprx;   /* (created with evs_aprx_create, below) */
EVS_API int evs_cache_lookup_batch_c1c2c3(evs_cache *c1, evs_cache *c2, evs_aprx *c3, int64_t B, const int32_t *rows,
                                          float *out, uint8_t *tier, int high_agghit_threshold, void *stream);
EVS_API int evs_cache_lookup_interact_c1c2c3(evs_cache *c1, evs_cache *c2, evs_aprx *c3, int64_t B, const int32_t *rows,
                                             const float *x, int64_t x_stride, int itself, float *R, uint8_t *tier,
                                             int high_agghit_threshold, void *stream);
/* Members of the batched C3 as (table_1based, row, recency flag) triples (host; may be NULL), returns their number;
 * out4 (host, may be NULL): [members counted on insert, alt hits served, capacity of the sets, 0].  Synchronises. */
EVS_API int64_t evs_aprx_batch_dump(evs_aprx *p, int64_t *triples, int64_t max_triples, int64_t *out4, void *stream);
/* The same lookup feeding the interaction directly: R = interact_features(x, [rows of the 26 keys])
 * (B, d + F(F-1)/2) without materialising the rows -- the probe writes a table of row addresses
 * (arena row for a hit, backing row for a miss) that the fused MFMA kernel consumes.  fp32 caches:
 * dimensions supported by evs_fused_dim_supported (up to 16 384 requests the probe itself runs inside that
 * kernel).  16 / 8 / 4-bit caches (tables in HBM, d in {16, 32, 36}): the rows are decoded inside the
 * interaction kernel (the reference's one-layer reduced-precision builds, cache_manager.cpp:13-20). */
EVS_API int evs_cache_lookup_interact(evs_cache *c, int64_t B, const int32_t *rows, const float *x, int64_t x_stride,
                                      int itself, float *R, uint8_t *hit, void *stream);
/* RAGGED BAGS THROUGH AN LRU / LFU / EvLFU TIER (multi-hot features behind the cache; csrc/evs_cache_policy.hip).  Input as
 * evs_embedding_bag_sum takes it: indices / offsets / nnz are HOST arrays of n_tables entries -- per table k a DEVICE int64
 * index array of nnz[k] entries and a DEVICE array of B bag start offsets (the last bag runs to nnz[k]).
 * THE RULE.  One call is batch n (1, 2, ...) of "the batched rule" (evs_cache_set_batch_policy, above); it shares the batch
 * counter with evs_cache_lookup_batch / _lookup_interact, and calls of the two forms may alternate on one cache.
 *   a lookup  is one POSITION of one index array; all sum(nnz) positions are probed, whether or not a bag covers them --
 *             offsets shape the pooling (EvLFU: and the counts) only.
 *   probe     (snapshot) hit[p] = 1 exactly when key (k + 1, indices[k][p]) was resident when the call started.  An index
 *             outside [0, n_rows[k]) is not a key: flag 0, it contributes nothing, it is never inserted, and it raises the
 *             sticky flag evs_check_index_errors reads.  All positions that carry the same key get the same flag.
 *   touch, insert  (LRU / LFU) steps 2 and 3 of the batched rule, unchanged, over the DISTINCT keys of the call: one touch per
 *             way and batch (the LFU counter rises by 1 per batch however many positions name the key), every distinct missed
 *             key inserted once.
 *   pooled    pooled[k][b] = sum over the bag's positions, in index order, of the served rows; fp32 adds, unfused, the
 *             accumulator starts at +0.0f.  Served rows are exactly the table rows, so the output is bit-equal to
 *             evs_embedding_bag_sum's general pooling over the backing tables for every input that call accepts -- a bag whose
 *             offsets are backwards or past nnz[k] is empty and raises the sticky flag, as there.
 *   counters  (evs_cache_batch_stats) n_requests += B; n_hits += the hit positions; n_perfect_hits += the samples that have
 *             at least one lookup and none missed or out of range, over all their bags; n_evict, size and hist keep their
 *             meaning.  With one index per bag this is what the (B, T) form counts.
 * AN EvLFU CACHE'S priority is a request's hit count.  The reference's EvLFU sees one key per table; what the count is over
 * bags is a choice it does not make, so the caller declares it: evs_cache_set_bag_rule(c, 1), "served bags" (below).  Without
 * it both entry points refuse an EvLFU cache (EVS_EINVAL).  With it one call is batch n of the batched EvLFU rule -- "WHAT IS
 * THE SAME" at evs_cache_set_batch_policy keeps holding -- on the set-associative tier alone (batch policy 2, 8 ways), with:
 *   probe     strict snapshot, as above.  The probe writes no way word and no way is hidden by its stamp (unlike the
 *             one-launch form of evs_cache_lookup_interact).
 *   served bag  bag (b, k) is served when none of its positions is a miss or out of range.  An empty bag is served; a bag
 *             whose offsets are backwards or past nnz[k] is empty (and raises the sticky flag), hence served.
 *   agg_hit(b)  the number of sample b's T bags that are served, 0 .. T.  With one index per bag: the (B, T) form's count.
 *   raise     every hit way named by a position of sample b gets priority max(old, agg_hit(b)) -- a monotone maximum over all
 *             positions that name it; its stamp stays.
 *   insert    every distinct missed key once, with priority = the maximum of agg_hit over the samples that name it, into its
 *             own set: free ways first (lowest index), else the lowest priority among the ways NOT stamped by this batch,
 *             lowest index among equals; no such way: turned away.  Priorities are read after all raises of the call (the
 *             raise launch ends before the insert launch starts).  The new way carries this batch's stamp.
 *   uncovered a position no valid bag covers is a lookup with count 0: a hit is not raised, a miss is inserted at priority 0.
 *             (Offsets that go back can make two valid bags of different samples cover one position; it then counts for one
 *             of them, which one is not specified.  Pooling and flags are unaffected.)
 *   counters  n_requests += B; n_hits += the hit positions; n_perfect_hits += the samples with at least one lookup and
 *             agg_hit = T; hist is the per-priority count of resident entries; n_evict, n_flush keep their meaning.
 *   flush     the EvLFU flush as it is: the close asks for it when the top bucket holds max_perfect entries, and the next
 *             batched call of either form runs it before its probe.
 *   mixing    calls may alternate with evs_cache_lookup_batch / _lookup_interact on one cache, under either setting of
 *             evs_cache_set_inline_update; they share the batch stamp and the batch counter.
 * hit: flat DEVICE uint8 array of sum(nnz) entries, table-major (table k's flags start at sum of nnz[j], j < k); may be NULL.
 * pooled: table k's bag b at pooled + k * out_table_stride + b * out_bag_stride (floats; 16-byte aligned, strides multiples of
 * 4), dim a multiple of 4 up to 256.  The interact form pools into a (T, B, d) scratch buffer the cache owns (grown on demand)
 * and runs the dense interaction (evs_interact_dot: R, itself) over x and the T pooled features.
 * Checked before the device is touched: EVS_EINVAL for B < 0, strides not multiples of 4, a NULL argument (cache, host arrays,
 * pooled / x / R, indices[k] with nnz[k] > 0, offsets[k]), nnz[k] < 0, sum(nnz) >= 2^31, a dim the pooling (interact form:
 * the interaction, evs_fused_dim_supported) does not take, n_tables + 1 > 32 features; B == 0 is success.  Refused with a
 * message that names the policy and the cache left usable: an EvLFU cache without a bag rule (EVS_EINVAL), host-memory or
 * file-backed tables (EVS_ESTATE; host memory is served in fetch-first order -- evs_cache_set_miss_order, for EvLFU with
 * evs_cache_set_bag_count(c, 1)), a cache driven by the exact path (EVS_ESTATE), a capacity below 8 or 2^32 rows over all
 * tables (EVS_EINVAL, as evs_cache_lookup_batch refuses them); an EvLFU cache whose batch policy is or resolves to plan or
 * sampled (set explicitly, through EVS_CACHE_POLICY, or because the geometry has no set-associative form), and 16-way sets
 * (EVS_SA_WAYS=16) or a tier of a C1 + C2 pair (EVS_EINVAL: the pair's bag form is evs_cache_lookup_bags_c1c2, below). */
EVS_API int evs_cache_lookup_bags(evs_cache *c, int64_t B, const int64_t *const *indices, const int64_t *const *offsets,
                                  const int64_t *nnz, float *pooled, int64_t out_table_stride, int64_t out_bag_stride,
                                  uint8_t *hit, void *stream);
EVS_API int evs_cache_lookup_bags_interact(evs_cache *c, int64_t B, const int64_t *const *indices,
                                           const int64_t *const *offsets, const int64_t *nnz, const float *x, int64_t x_stride,
                                           int itself, float *R, uint8_t *hit, void *stream);
/* RAGGED BAGS THROUGH THE BATCHED C1 + C2 PAIR (the mixed-precision pair of evs_cache_lookup_batch_c1c2 behind multi-hot
 * features; csrc/evs_cache_policy.hip).  Inputs exactly as evs_cache_lookup_bags takes them: host arrays of device pointers, B
 * bag starts per table, the last bag runs to nnz[k].
 * THE RULE.  One call is batch n of BOTH tiers.  It shares the batch number, the stamps, the counters, the closes and the pending
 * EvLFU flush with evs_cache_lookup_batch_c1c2 / _lookup_interact_c1c2; calls of the two forms may alternate on one pair.
 *   a lookup  is one POSITION of one index array; all sum(nnz) positions are probed, whether or not a bag covers them.  An
 *             index outside [0, n_rows) of EITHER tier's table k (the (B, T) probe's check) is no key: code 0, it contributes
 *             nothing, it is never inserted, and it raises the sticky flag evs_check_index_errors reads.
 *   probe     (strict snapshot) tier[p] = 1 when the key is resident in C1 when the call starts, else 2 when in C2, else 0.  The
 *             probe writes no way word.  All positions that name one key get one code.
 *   served bag, agg_hit(b)  as the single-tier EvLFU rule above defines them: bag (b, k) is served when none of its positions
 *             has code 0 or is out of range; an empty bag is served; a bag whose offsets are backwards or past nnz[k] is
 *             empty (and raises the sticky flag), hence served.  agg_hit(b) is the number of sample b's T bags that are
 *             served.  A position no valid bag covers counts as 0.  (Offsets that go back can make two valid bags of different
 *             samples cover one position -- the sticky flag is raised by the bag in between; such a position counts for one of
 *             them, which one is not specified, and with it its route, its serving tier and its share of pooled.  Codes are
 *             unaffected.)
 *   raise     every hit way named by a position of sample b goes to max(old, agg_hit(b)) in the tier that holds it; its stamp
 *             stays.
 *   route     of a missed position of sample b (evlfu_8.cpp:570-601 on the snapshot, as the (B, T) form evaluates it for
 *             set-associative tiers): the key's own C1 set has a free way in the snapshot -> C1; else agg_hit(b) < threshold ->
 *             C1 for an odd table index k, C2 for an even one; else C2.  The position is SERVED FROM THE DESTINATION TIER'S
 *             BACKING TABLE AT THAT TIER'S PRECISION.
 *   insert    every distinct missed key once, by the (B, T) form's update launch, unchanged, over the miss lists.  A key routed
 *             both ways by different positions (odd tables only) goes to C1 (the route filter), as in the (B, T) form.  Its
 *             priority is the maximum of agg_hit over the positions listed for the tier that takes it; victim choice, the
 *             turn-away and the stamp are the update's own.
 *   pooled    pooled[k][b] = sum over the bag's positions, in index order, of the served rows DECODED PER POSITION AT THE
 *             PRECISION OF THE TIER THAT SERVES THAT POSITION (a bag may mix rows of both); fp32 adds, unfused, from +0.0f.
 *             The output is a pure function of the snapshot and the input (positions two bags cover excepted, above): bit-exactly
 *             predictable on contended batches too.
 *   counters  (evs_cache_batch_stats, per tier) n_hits += the positions hit in that tier; n_requests += B; perfect requests
 *             are the samples with at least one lookup and agg_hit = T, counted where the (B, T) probe counts them (C1).  With
 *             one index per bag both tiers' counters equal what the (B, T) call leaves.
 * tier: flat DEVICE uint8 array of sum(nnz) entries, table-major; may be NULL.  pooled / x / R as evs_cache_lookup_bags /
 * _lookup_bags_interact take them; the interact form pools into a (T, B, d) block C1 owns and runs evs_interact_dot.
 * THE ENVELOPE, checked before anything is allocated, the pair left usable: the argument checks are evs_cache_lookup_bags'
 * (EVS_EINVAL; B == 0 is success); both caches EvLFU with evs_cache_set_bag_rule(c, 1) told to BOTH (EVS_EINVAL names the cache
 * that lacks it); the pair shares its set record (evs_cache_pair_load's geometry: plan-based, sampled and EVS_SA_PAIR=0 pairs,
 * tiers that did not start out together: EVS_EINVAL); both tiers' tables in HBM (host-memory / file-backed: EVS_ESTATE); miss
 * order 0, or the fetch-first bag chain below; no alt-key tier (a pair that has run evs_cache_lookup_batch_c1c2c3 / _interact_c1c2c3: EVS_EINVAL); the pairs of precisions the reference builds -- 32-16, 32-8, 32-4, 16-8, 16-4, 8-4 (others:
 * EVS_EINVAL naming the codecs); dim a multiple of 4 up to 256, the interact form evs_fused_dim_supported(dim) and
 * n_tables + 1 <= 32.
 * THE FETCH-FIRST BAG CHAIN (the bag form of "THE FETCH-FIRST PAIR" at evs_cache_lookup_batch_c1c2) is taken only when ALL of these
 * hold: both tiers are at evs_cache_set_miss_order(c, 1); both tiers have been told evs_cache_set_bag_count(c, 1) -- "count first" is
 * the statement that the samples' counts may be computed in front of everything, which is exactly what lets the update run before
 * the pooling --; both tiers have the bag rule.  The call then runs, on one stream:
 *   (flush) -> bags_probe2 -> bags_count2 -> bags_route2 -> the pair's update launch -> bags_repoint2 -> bags_pool2
 *           -> (dense interaction) -> the close bookkeeping.
 * NOTHING OF THE RULE ABOVE CHANGES: tier codes (strict snapshot), served bag, agg_hit, raise, route, insert, counters, flush and
 * mixing hold as written.  The tier state after a call is what the order-0 chain leaves for that call: the raises end before the
 * update in both orders, the update reads the same lists and the same way words, and neither the re-point nor the pooling writes
 * anything the update reads.  Codes, pooled bits, R bits, both tiers' evs_cache_batch_dump, evs_cache_batch_stats with hist and
 * n_perfect_hits and the exported state equal order 0's on every call whose outcome does not depend on timing.
 * RE-POINT (bags_repoint2).  Every position with a key -- serve byte 1 or 2, whether or not a bag covers it -- is searched again in
 * the ways of the tier its serve byte names, in the one shared 128-byte record, and only there:
 *   code 0, key now resident in that tier   that tier's arena row (counted `repointed`);
 *   code 0, key not there                   turned away, or routed both ways and given to C1 by the route filter while this position
 *                                           was routed to C2: it keeps the table row the route launch wrote (counted `in_place`);
 *   code 1 / 2, way still holds the key     nothing is stored;
 *   code 1 / 2, the update took the way     (the pair has one arena row per way) the tier's table row, the same bytes (counted
 *                                           `victim_hits`);
 *   serve byte 0 (a bad index)              untouched and counted nowhere; the probe has raised the sticky flag.
 * The kernel writes no way word, does no atomic on a record and reads no table.  Over host tables every distinct missing row
 * crosses the bus once, inside the update; only `in_place` and `victim_hits` positions are read from host memory by the pooling.
 * evs_cache_fetch_stats(c1, ...) counts the pair's bag calls and the three totals in the words the (B, T) fetch-first pair uses;
 * calls of the two forms may alternate on one pair.
 * A FAILING INTERACTION.  The interaction's argument checks (dim, feature count, x / R) are made up front, before the device is
 * touched.  Should evs_interact_dot still fail, an order-1 call leaves an already-inserted batch (the update ran in front of it);
 * in order 0 nothing is inserted, as before.  Either way the batch is counted.
 * ITS ENVELOPE, checked before anything is allocated, the pair left usable, a policy that was only resolved there forgotten again:
 * the fetch-first pair's (batch policy 2 given or resolved wherever the tables live -- plan / sampled, given or from
 * EVS_CACHE_POLICY: EVS_EINVAL; the shared set record -- EVS_SA_PAIR=0, capacities without one, tiers that started alone:
 * EVS_EINVAL; file-backed tables: EVS_ESTATE; messages name the policy) plus the bag form's own (bag rule on both, the six pairs of
 * precisions, no alt-key history, no resident server, no approximate threshold).  What the caller sees: a tier on which
 * evs_cache_serve_start was called belongs to the exact path, so the batched path's own check speaks first -- EVS_ESTATE, "this
 * evlfu cache is used through the exact path"; an order-1 pair cannot have alt-key history (the _c1c2c3 forms refuse it, EVS_EINVAL);
 * both tiers at order 1 without count-first on both is refused (EVS_EINVAL naming evs_cache_set_bag_count) BEFORE the tables are
 * looked at, so a pair over host-memory tables that forgot the setting is told so, not that its tables must be in HBM.  Each tier's tables may be in HBM or in
 * device-addressable host memory, independently; the alignment check applies to host tables too.  One tier at order 1: EVS_EINVAL
 * ("a tier alone").  Both at order 1 with count-first on none or one tier: EVS_EINVAL naming "fetch-first".  An order-0 pair
 * ignores evs_cache_set_bag_count, runs the chain at the top launch for launch and keeps EVS_ESTATE over host-memory tables. */
EVS_API int evs_cache_lookup_bags_c1c2(evs_cache *c1, evs_cache *c2, int64_t B, const int64_t *const *indices,
                                       const int64_t *const *offsets, const int64_t *nnz, float *pooled, int64_t out_table_stride,
                                       int64_t out_bag_stride, uint8_t *tier, int high_agghit_threshold, void *stream);
EVS_API int evs_cache_lookup_bags_interact_c1c2(evs_cache *c1, evs_cache *c2, int64_t B, const int64_t *const *indices,
                                                const int64_t *const *offsets, const int64_t *nnz, const float *x, int64_t x_stride,
                                                int itself, float *R, uint8_t *tier, int high_agghit_threshold, void *stream);
/* What a request's hit count is over ragged bags, for an EvLFU cache (the rule: evs_cache_lookup_bags, above): 0 none (the
 * default: the bag entry points refuse the cache), 1 "served bags".  May be called between calls.  EVS_EINVAL, with the policy
 * named: a rule outside {0, 1}; rule 1 on an LRU / LFU cache (their bag form needs none; rule 0 is accepted). */
EVS_API int evs_cache_set_bag_rule(evs_cache *c, int rule);
/* WHEN an EvLFU bag call (evs_cache_lookup_bags / _lookup_bags_interact) computes its samples' counts.  agg_hit(b) is a function
 * of the probe's flags and the offsets alone; where it is computed decides what may run in front of the pooling.
 *   0 "in the pooling walk" (the default): the chain above -- probe, pooling (which judges every sample as a by-product),
 *     (interaction,) raise + list, update -- launch for launch, and every refusal as it was: an order-1 EvLFU cache
 *     (evs_cache_set_miss_order) has no bag form, and the bag form reads its tables from HBM.
 *   1 "count first": a launch of its own between the probe and everything that needs a count walks the flag bytes of every
 *     bag (the caller's hit array when one was given, else the cache's), tells each covered position its sample, writes
 *     agg_hit(b) and counts the all-served samples with a lookup; the pooling then only pools.  THE RULE IS UNCHANGED:
 *     probe, served bag, agg_hit, raise, insert, uncovered, counters, flush and mixing hold as written at
 *     evs_cache_lookup_bags; only the launch order moves.
 *       order 0 (consume first):  (flush,) probe, count, pooling, (interaction,) raise + list, update.  Every observable result
 *         -- flags, pooled bits, R bits, evs_cache_batch_dump, evs_cache_batch_stats with hist and n_perfect_hits, the exported
 *         state -- equals what setting 0 gives for the same calls.  Over either arena (EVS_SA_DUAL=0 too); tables in HBM.
 *       order 1 (fetch first):  (flush,) probe, count, raise + list, update, sa_repoint, pooling, (interaction,) the close
 *         bookkeeping.  The tier state after a call is what the order-0 chain leaves for it: the raises end before the update
 *         starts in both orders, the update reads the same words, the consumers write nothing it reads.  A hit way that is
 *         this call's victim is read from the copy of the two-copy arena the update left alone (as in the (B, T) form).  A key
 *         whose set took 8 new keys in the call is pooled in place from its table.  evs_cache_fetch_stats counts the call and
 *         its re-pointed / in-place positions.  The envelope is an order-1 cache's (evs_cache_set_miss_order: a tier alone,
 *         batch policy 2 given or resolved, 8-way sets, the two-copy arena), checked before anything is allocated, a policy
 *         that was only resolved there forgotten on a refusal; tables in HBM or in device-addressable host memory -- the one
 *         combination in which an EvLFU bag call reads host tables; file-backed tables stay EVS_ESTATE; all four codecs; a
 *         call without a bag rule keeps its EVS_EINVAL.
 * An all-served sample with a lookup is counted once per call whichever launch judges it, and the cache's sample words are zero
 * again when a call ends, so the setting may change between calls (like evs_cache_set_bag_rule).  It is not part of the
 * warm-start state: export and load are unchanged.  The pair's bag form (evs_cache_lookup_bags_c1c2*) has its own count pass
 * in front of the pooling whatever the setting; an order-0 pair ignores it, as do the (B, T) forms.  On a pair with BOTH tiers at
 * order 1 the setting, told to both tiers, is what admits the fetch-first bag chain ("THE FETCH-FIRST BAG CHAIN" at
 * evs_cache_lookup_bags_c1c2); told to none or one of them, the call keeps its EVS_EINVAL.  EVS_EINVAL, with the policy named: a NULL cache; `when` outside {0, 1};
 * when = 1 on an LRU / LFU cache (their bag form needs no count; when = 0 is accepted). */
EVS_API int evs_cache_set_bag_count(evs_cache *c, int when);
/* The one-launch form of a set-associative tier (round 5: the policy update runs INSIDE evs_cache_lookup_interact's probe +
 * interaction launch; a hit flag then says "served from the cache": 1 => resident at arrival, 0 => not resident OR retired
 * by one of this batch's own inserts OR resident in a way filled k 2^S batches ago, see evs_cache_set_batch_policy) is the default wherever its conditions hold (a tier alone, 8 ways, two-copy arena, at
 * least 8 stamp bits in the way word).  on = 0 restores the two-launch chain with strict snapshot flags for this cache, on = 1
 * the default; the environment variable EVS_CACHE_INLINE=0 only changes the default of caches that were never told.  May be
 * called between batches.  LRU / LFU caches have the chain only: on = 1 is refused (EVS_EINVAL), on = 0 accepted. */
EVS_API int evs_cache_set_inline_update(evs_cache *c, int on);
/* Which runs first on the set-associative batched path of this cache, the consumers or the policy update.
 *   0 "consume first" (the default): today's chains -- probe, consumers, update -- and today's refusals: the set-associative
 *     tier reads its miss tier in place from HBM.
 *   1 "fetch first": one stream, in this order -- (EvLFU: the flush an earlier close asked for,) the unfolded probe, which
 *     writes 8-byte row addresses and the miss lists; the policy update; sa_repoint, which searches every position flagged 0
 *     again in its set and, where the key got a way, re-points its slot of the address table at the arena row; the consumers;
 *     the close bookkeeping.  Every missing row is read ONCE, by the update thread that installs it, so the tables may live in
 *     HBM or in host memory the device addresses (evs_cache_set_backing over pinned memory).  Flags are strict residency at
 *     arrival; the tier state after a call is what the order-0 chain leaves for the same batch (the update reads the same
 *     words either way, and the consumers write nothing the update reads).  Why the reordering is safe: the inserts read
 *     their source row through a plain global pointer; a way changes at most once per update launch and a way stamped by the
 *     running batch is never a victim -- under LRU / LFU a way hit in batch n is touched, so its arena row is intact when the
 *     consumers read it; under EvLFU a hit way CAN be that batch's victim, and the replacement writes the other copy of the
 *     two-copy arena and flips the select bit, so the address the probe computed stays valid until the consumers have read it.
 *     A key whose set took 8 new keys in the batch is turned away and served in place from its table.
 * The envelope of an order-1 cache, resolved and checked at every batched call before anything is allocated (a policy that was
 * only resolved there is forgotten again on a refusal; every message names the cache's policy):
 *   tier       a tier alone, or -- BOTH tiers at order 1 -- the C1 + C2 pair of evs_cache_lookup_batch_c1c2 / _lookup_interact_c1c2
 *              ("THE FETCH-FIRST PAIR" there: its own envelope and its own re-point kernel) and, once both tiers were also told
 *              evs_cache_set_bag_count(c, 1), of evs_cache_lookup_bags_c1c2 / _lookup_bags_interact_c1c2.  One tier of a pair at
 *              order 1, the triple, the pair's bag form without count-first on both tiers: refused at that call, EVS_EINVAL.  A
 *              member of a pair stays refused by the single-tier calls.
 *   policy     batch policy 2, given or resolved: LRU / LFU as always; an EvLFU cache that was given no policy and no
 *              EVS_CACHE_POLICY takes it wherever the geometry has a set-associative form, wherever its tables live (the one
 *              resolution rule that differs from order 0).  plan / sampled, given or from the environment: EVS_EINVAL.
 *   ways       8-way sets (EVS_SA_WAYS=16: EVS_EINVAL).  EvLFU needs the two-copy arena (EVS_SA_DUAL=0: EVS_EINVAL); LRU / LFU
 *              run over either arena.
 *   tables     HBM or device-addressable host memory.  File-backed tables: EVS_ESTATE.  Order 1 over HBM tables is legal and
 *              gives the results of order 0.
 *   served     evs_cache_lookup_batch (every codec); evs_cache_lookup_interact (fp32 rows; reduced precision with the tables in
 *              HBM only); evs_cache_lookup_bags / _lookup_bags_interact for LRU / LFU, and for EvLFU once
 *              evs_cache_set_bag_count(c, 1) ("count first") has been told; without it EvLFU bags are EVS_EINVAL -- a sample's
 *              count exists only after the pooling walk, so the update cannot run in front of it.  evs_cache_batch_stats,
 *              _batch_dump, _update_rows and _refresh_rows work as before; the warm start over HBM tables too (over host
 *              tables it keeps its EVS_ESTATE).  The inline setting of an order-1 cache that was never given one is 0.
 * May be called only before the cache's first batched call or load: EVS_ESTATE afterwards.  EVS_EINVAL: a NULL cache, an order
 * outside {0, 1}, order 1 on a cache that was told evs_cache_set_inline_update(c, 1) (and that call on an order-1 cache).
 * The exact path ignores the setting. */
EVS_API int evs_cache_set_miss_order(evs_cache *c, int order);
/* out4 (host): [batched calls run fetch-first, positions re-pointed at the arena, positions served in place from their
 * table, 0], cumulative since creation.  An index out of range is no key and is counted nowhere.  Synchronises the stream.
 * C1 of a fetch-first pair counts the pair: [pair calls run fetch-first, miss positions re-pointed at an arena (of either
 * tier), miss positions left in place, hit positions whose way the call's own update took]; C2's own counters are not used.
 * The fourth word stays 0 for a tier alone.
 * EVS_EINVAL for a NULL cache or a NULL out4, before the device is touched. */
EVS_API int evs_cache_fetch_stats(evs_cache *c, int64_t *out4, void *stream);
/* FED BACKING: the set-associative tier over rows the caller supplies -- the fetch-first chain cut in two where the bus fetch sits.
 * evs_cache_set_fed_backing is evs_cache_set_backing, except that tables[k] may be NULL for a table with n_rows[k] > 0.  Such a
 * table is a FED TABLE: the GPU never reads it, its missing rows come from the caller between evs_cache_fed_begin and
 * evs_cache_fed_finish (a file larger than the pinned budget, a key-value store, a parameter server: whatever answers
 * "rows for keys").  Non-NULL tables are read in place as today, from HBM or from pinned host memory.  A cache with at least one
 * fed table is a FED CACHE; evs_cache_set_backing / evs_cache_set_file_backing make it an ordinary one again.
 * EVS_EINVAL: a NULL argument, more than 32 tables, a negative row count.
 *
 * THE RULE.  A begin + finish pair is batch n of the cache under the fetch-first contract written at evs_cache_set_miss_order;
 * nothing else changes.  Given rows equal to the table rows, flags, outputs, evs_cache_batch_dump, evs_cache_batch_stats (with
 * hist) and evs_cache_fetch_stats are what the same calls leave on a fetch-first cache over the same tables in HBM, on every
 * call whose outcome does not depend on timing.  Stronger than that: a served row of a fed table is always, byte for byte, a row
 * the caller fed for that key -- from the arena once it is installed, from the fed block itself for a position whose set took 8
 * new keys in the call (the chain's "left in place").
 *
 * evs_cache_fed_begin(c, B, rows, hit, keys, n_keys_host, stream) runs the pending EvLFU flush and the fetch-first probe (a form
 *   that leaves the way words alone: see the abort): hit
 *   (device, B * T) carries strict snapshot flags exactly as evs_cache_lookup_batch at order 1 writes them.  It then builds the
 *   FED LIST: every distinct valid key of a fed table with flag 0, exactly once, as table_1based << 32 | row (the format
 *   evs_filetier_fetch takes), in no particular order.  keys is device-addressable memory (device or pinned host, 8-byte
 *   aligned) with room for B * T entries.  The call synchronises the stream and writes the count to *n_keys_host.  Not in the
 *   list: an index out of range (no key: flag 0, a zero row; the finish raises the sticky flag of evs_check_index_errors for
 *   it), a key of an addressed table, a hit.  rows and hit must stay valid until the finish.
 * evs_cache_fed_finish(c, fed, fed_stride_bytes, out, stream) / evs_cache_fed_finish_interact(c, fed, fed_stride_bytes, x,
 *   x_stride, itself, R, stream) run the update, the re-point, the consumers (evs_cache_lookup_batch's out / evs_cache_lookup_
 *   interact's R) and the close bookkeeping.  fed is DEVICE memory: row i, in the cache's codec, is at fed + i * fed_stride_bytes
 *   and is the row of keys[i].  fed and fed_stride_bytes are multiples of what a table gives its rows -- the largest of 16, 8,
 *   4, 2, 1 that divides the row size -- and the stride is at least the row size.  fed == NULL is accepted when the list was
 *   empty.  fed must stay valid until the consumers have run, in stream order; afterwards every installed key lives in the arena.
 * evs_cache_fed_abort(c) drops the open call: nothing was inserted, the batch is not counted -- neither its requests nor the
 *   hits its probe saw -- its ordinal and its stamp are given back, and the cache serves on.  The begin writes no way word (the
 *   LRU / LFU touch and EvLFU's raise of the ways a call hits are the finish's first launch), so the tier, evs_cache_batch_stats
 *   with hist, evs_cache_batch_dump with its scores and the other counters are what they were before the begin, whatever batch
 *   follows; the same begin lists the same keys.  Nothing is launched and no stream is touched.  (An EvLFU flush that an
 *   EARLIER close asked for and the begin ran is the tier's, not the call's: evs_cache_batch_stats runs it as well.)
 * evs_cache_fed_stats(c, out4, stream): cumulative [calls finished, keys listed, missed positions of fed tables, positions served
 *   straight from a fed block].  Synchronises the stream.
 *
 * THE ENVELOPE, checked at the begin before anything is allocated (the cache stays usable, the message names the policy): a tier
 * alone; batch policy 2, given or resolved; 8-way sets; evs_cache_set_miss_order(c, 1); EvLFU over the two-copy arena, LRU or
 * LFU; all four codecs (the interact form: evs_cache_lookup_interact's dimensions; a reduced-precision cache with its addressed
 * tables in HBM).  Refused:
 *   a fed cache at order 0                                         EVS_EINVAL, naming fetch-first
 *   a threshold of evs_cache_set_batch_approx in force               EVS_EINVAL
 *   evs_cache_lookup_batch / _lookup_interact on a fed cache         EVS_ESTATE, naming the begin / finish calls
 *   evs_cache_lookup_bags / _lookup_bags_interact                    EVS_ESTATE, naming evs_cache_fed_begin_bags / _fed_finish_bags
 *   a fed cache as a tier of any pair / triple call (batched, bags, the exact request, the tier server)   EVS_EINVAL
 *   evs_cache_batch_export / _batch_load / _pair_load                EVS_EINVAL
 *   evs_cache_request, the resident server, evs_cache_exact_load     EVS_ESTATE
 *   evs_cache_update_rows / _refresh_rows (no table to write or to read again: the file-backed case)   EVS_ESTATE
 * Protocol errors are EVS_ESTATE: a begin on a cache without a fed table; finish or abort without an open call; a second begin;
 * any other batched call, stats, dump, export, load, row update or change of backing while a call is open.  evs_cache_destroy
 * with an open call is fine.  Argument errors are EVS_EINVAL and leave an open call open: NULL arguments, B < 1, fed == NULL with
 * a non-empty list, a misaligned fed or stride, a stride below the row size.  A consumer that refuses behind the update ends the
 * call as it ends evs_cache_lookup_batch: the batch is not counted.
 *
 * SEVERAL CALLS OPEN AT ONCE.  A store with latency L behind the begin / finish pair costs L + G per batch (G: the GPU time of a
 * begin and a finish) while one call may be open; with D calls open and their fetches in flight together it approaches
 * max(G, (L + G) / D).  The tier alone takes that in its (B, T) form, under all three policies and all four codecs.
 * evs_cache_set_fed_depth(c, depth): depth 1 .. 4 calls open at a time, 1 the default.  EVS_EINVAL for a NULL cache or a depth
 *   outside 1 .. 4, EVS_ESTATE while a call is open; allowed at any other time.  It allocates nothing: the scratch of a call slot is
 *   grown by the begin that takes it.  At depth 1 every entry point behaves as written above, the EVS_ESTATE of a second begin and
 *   its wording included.
 * evs_cache_fed_open_calls(c): the number of open calls, 0 .. depth; -1 for a NULL cache.
 * evs_cache_fed_begin with fewer than `depth` calls open is accepted.  It probes the tier AS IT STANDS: every finished call is
 *   applied, no open call's touch, raise or insert is.  Its flags are strict snapshot flags of that state, its list is the list
 *   written above, its ordinal and stamp are the next ones, and every way it hit is HELD until the call ends: no other call's
 *   update takes a held way (an update that finds no other way in the set turns its key away -- "left in place", served from that
 *   call's fed block).  A hold is WRITTEN only by a begin made while another call is open: a call that begins alone is the oldest
 *   call until it ends, no other call's update runs in front of its finish, so nothing could take its ways and it sets no bit
 *   (evs_cache_fed_ahead_stats counts no hold bit for it).  With `depth` calls open already: EVS_ESTATE, naming the depth.  Only (B, T) calls overlap:
 *   evs_cache_fed_begin_bags and evs_cache_pair_fed_begin while any call is open, and any begin while a bag call or a pair call is
 *   open, are EVS_ESTATE as ever.
 * evs_cache_fed_finish / _fed_finish_interact end the OLDEST open call: the steps written above -- fold, touch / raise of the ways
 *   its begin hit, update, re-point, consumers, close -- on that call's own stamp, records and pointer table; fed holds the rows of
 *   THAT call's list.  Two things differ, and only while another call is open: the ways the other open calls hold are no
 *   victims, and a pending EvLFU flush is not run by a begin (the request stands; the next begin that finds no call open runs
 *   it, as evs_cache_batch_stats does).  A key two open calls both missed is in both lists; the older call installs it, the newer
 *   call's record finds it resident ("another copy got there first": EvLFU folds the priority, LRU / LFU leave the way as it is)
 *   and its positions are served the arena row.
 * evs_cache_fed_abort drops the NEWEST open call, as written above: nothing is launched, its ordinal and stamp are given back, its
 *   holds lapse.  To drop an older call, abort down to it.
 * THE ROW RULE, restated: a served row of a fed table is, byte for byte, a row the caller fed for that key in this call or in a
 *   call that was open together with it.  A caller whose store changes under open calls gets either version.
 * EQUIVALENCE: a call that is alone between its begin and its finish runs exactly as at depth 1, whatever depth is set.
 * ORDERING: all calls of a cache go on one stream, or are ordered by the caller, as for every other call on a cache.
 * REFUSALS: everything refused while one call is open stays refused while any is: evs_cache_batch_stats, the dump, export and
 *   load, row updates, a change of backing, every other batched call.
 * evs_cache_fed_ahead_stats(c, out4, stream): cumulative [begins made with another call open, hold bits set, miss records whose key
 *   an earlier call had installed by the time of the finish -- keys fetched twice, the price of the stale snapshot --, 0].
 *   Synchronises the stream; refuses as evs_cache_fed_stats does. */
EVS_API int evs_cache_set_fed_backing(evs_cache *c, const void *const *tables, const int64_t *n_rows);
EVS_API int evs_cache_fed_begin(evs_cache *c, int64_t B, const int32_t *rows, uint8_t *hit, uint64_t *keys, int64_t *n_keys_host, void *stream);
EVS_API int evs_cache_fed_finish(evs_cache *c, const void *fed, int64_t fed_stride_bytes, float *out, void *stream);
EVS_API int evs_cache_fed_finish_interact(evs_cache *c, const void *fed, int64_t fed_stride_bytes, const float *x, int64_t x_stride, int itself,
                                          float *R, void *stream);
EVS_API int evs_cache_fed_abort(evs_cache *c);
EVS_API int evs_cache_fed_stats(evs_cache *c, int64_t *out4, void *stream);
EVS_API int evs_cache_set_fed_depth(evs_cache *c, int depth);
EVS_API int evs_cache_fed_open_calls(evs_cache *c);
EVS_API int evs_cache_fed_ahead_stats(evs_cache *c, int64_t *out4, void *stream);
/* RAGGED BAGS OVER FED BACKING: the begin / finish form of evs_cache_lookup_bags / _lookup_bags_interact on a fed cache -- the
 * count-first fetch-first bag chain cut in two where the bus fetch sits.  evs_cache_fed_abort and evs_cache_fed_stats serve
 * both forms.
 *
 * THE RULE.  A bag begin + finish pair is batch n of the cache and runs exactly as evs_cache_lookup_bags runs it on an order-1
 * cache (EvLFU: with evs_cache_set_bag_rule(c, 1) and evs_cache_set_bag_count(c, 1)); nothing else changes.  Given rows equal to
 * the table rows, the flags, the pooled bits, R, evs_cache_batch_dump, evs_cache_batch_stats (with hist and n_perfect_hits) and
 * evs_cache_fetch_stats are what the same calls leave on a fetch-first cache over the same tables in HBM, on every call whose
 * outcome does not depend on timing.  A served row of a fed table is, byte for byte, a row the caller fed for that key: from the
 * arena once installed, from the fed block for a position whose set took 8 new keys in the call.
 *
 * evs_cache_fed_begin_bags(c, B, indices, offsets, nnz, hit, keys, n_keys_host, stream): the bag inputs are evs_cache_lookup_bags'
 *   (host arrays of device pointers, B bag starts per table, the last bag runs to nnz[k]); B >= 1.  hit is a flat device array of
 *   sum(nnz) bytes, table-major, or NULL (the cache's own flag bytes are used).  Runs the pending EvLFU flush, a probe that leaves
 *   the way words alone and, EvLFU, the count pass; then builds the FED LIST into keys (device-addressable, 8-byte aligned, room
 *   for sum(nnz) entries): every distinct valid key of a fed table that at least one position missed, exactly once, as
 *   table_1based << 32 | row, in no particular order -- however many positions, bags and samples name it, and whether or not a
 *   valid bag covers those positions (an uncovered key is inserted at priority 0, as the bag rule has it).  Not in the list: an
 *   index out of range, a key of an addressed table, a hit.  Synchronises the stream and writes the count to *n_keys_host.
 *   indices, offsets and hit must stay valid until the finish.
 * evs_cache_fed_finish_bags(c, fed, fed_stride_bytes, pooled, out_table_stride, out_bag_stride, stream) /
 * evs_cache_fed_finish_bags_interact(c, fed, fed_stride_bytes, x, x_stride, itself, R, stream) touch / raise the ways the begin
 *   hit, run the update, the re-point, the pooling (evs_cache_lookup_bags' pooled / _lookup_bags_interact's R) and the close
 *   bookkeeping.  fed is as evs_cache_fed_finish takes it.
 * The sticky flag of evs_check_index_errors is raised, at the latest when the finish returns, for every index out of range and
 *   every bad bag; a begin may already have raised it, and evs_cache_fed_abort does not clear it.
 * evs_cache_fed_abort after a bag begin: as after evs_cache_fed_begin.  The begin writes no way word (for LRU / LFU too: the touch
 *   is the finish's first launch), its totals go into rows of the call's own and the samples' words are zero again when it returns.
 *
 * THE ENVELOPE, checked at the begin before anything is allocated: a fed cache's, as above, and the order-1 bag form's -- an
 * EvLFU cache without evs_cache_set_bag_rule(c, 1) or without evs_cache_set_bag_count(c, 1) is EVS_EINVAL naming the setter; the
 * argument checks of evs_cache_lookup_bags (dim % 4 == 0 and <= 256, fewer than 2^31 lookups, no NULL indices[k] with nnz[k] > 0;
 * the interact finish: a fused-kernel dim and T <= 31).  evs_cache_lookup_bags / _lookup_bags_interact themselves stay EVS_ESTATE
 * on a fed cache.
 * PROTOCOL.  A finish of the other form than the open begin's is EVS_ESTATE, names the right call and leaves the call open
 * (evs_cache_fed_finish after a bag begin, evs_cache_fed_finish_bags after evs_cache_fed_begin).  Everything an open (B, T) call
 * refuses, an open bag call refuses.  Argument errors of the finish are EVS_EINVAL and leave the call open.  Bag calls and (B, T)
 * calls may alternate on one fed cache: they share stamp, ordinal, counters and the pending flush. */
EVS_API int evs_cache_fed_begin_bags(evs_cache *c, int64_t B, const int64_t *const *indices, const int64_t *const *offsets,
                                     const int64_t *nnz, uint8_t *hit, uint64_t *keys, int64_t *n_keys_host, void *stream);
EVS_API int evs_cache_fed_finish_bags(evs_cache *c, const void *fed, int64_t fed_stride_bytes, float *pooled,
                                      int64_t out_table_stride, int64_t out_bag_stride, void *stream);
EVS_API int evs_cache_fed_finish_bags_interact(evs_cache *c, const void *fed, int64_t fed_stride_bytes, const float *x, int64_t x_stride,
                                               int itself, float *R, void *stream);
/* Fed backing of the fetch-first C1 + C2 pair: the set-associative pair (evs_cache_lookup_batch_c1c2, "THE FETCH-FIRST PAIR")
 * over rows the caller supplies, on the (B, T) lookup and its fused interaction.  Both tiers are fed caches over the SAME fed
 * tables (evs_cache_set_fed_backing on each; a tier's fed rows are in that tier's codec), both at evs_cache_set_miss_order(c, 1).
 * THE RULE.  A begin + finish is batch n of the pair under the fetch-first pair's contract; nothing else changes.  Given fed rows
 * equal to the table rows, the tier codes, the bits of out, R, both tiers' evs_cache_batch_dump, evs_cache_batch_stats (with hist)
 * and evs_cache_fetch_stats(c1) are what evs_cache_lookup_batch_c1c2 / _lookup_interact_c1c2 leave on a fetch-first pair over the
 * same tables in HBM, on every call whose outcome does not depend on timing.  A served row of a fed table is, byte for byte, a row
 * the caller fed for that key at that tier's precision: from the arena once installed, from the fed block, or from the spill.
 * evs_cache_pair_fed_begin(c1, c2, B, rows, tier, high_agghit_threshold, keys1, n_keys1_host, keys2, n_keys2_host, stream) runs
 *   the pending EvLFU flush of either tier and the pair's probe in a form that writes NO way word and NO route-filter word: the
 *   tier codes (strict snapshot), the serve bytes, the addresses, the per-tier miss lists, the hit totals into rows of the call's
 *   own.  Then one fed list per tier: keys_d (device, 8-byte aligned, room for B * T entries) holds every distinct valid key of a
 *   fed table that at least one missed position routed to tier d names, each once, as table_1based << 32 | row.  A key on an odd
 *   table that two samples route both ways is in BOTH lists; its C2-routed position is served C2's row in C2's codec, whichever
 *   tier keeps the key.  The call synchronises the stream and writes both counts.
 * evs_cache_pair_fed_finish(c1, c2, fed1, fed1_stride_bytes, fed2, fed2_stride_bytes, out, stream) / _finish_interact(..., x,
 *   x_stride, itself, R, stream): fed_d (device) holds the row of keys_d[i] at fed_d + i * stride, in tier d's codec; alignment and
 *   stride as evs_cache_fed_finish asks, per tier; fed_d == NULL where list d was empty.  Launches: the raise of the ways the begin
 *   hit with the histogram moves and the route-filter stamps (all the begin withheld), the pair's update in fed form (a record of a
 *   fed table reads fed_d through its slot), the re-point, the consumers, the close bookkeeping.
 *   THE SPILL.  The pair keeps one arena row per way, so a way the call hit can be the call's victim, and a fed table has no table
 *   row holding "the same bytes".  The update's thread that replaces an occupied way whose old key belongs to a fed table first
 *   copies the way's arena row into a per-call spill block; the re-point points such a hit position at that copy.  A victim of an
 *   addressed table is not spilled: its hit positions are served from the table row, as on the addressed pair.  Both kinds are
 *   counted as victim hits in evs_cache_fetch_stats(c1).
 *   No address computed from a NULL table base is ever stored: between begin and finish a missed position of a fed table holds its
 *   tier's zero row, and a position whose key the scratch table does not hold keeps it (the sticky evs_check_index_errors flag is
 *   raised).  An index out of range: code 0, a zero row, in no list, the sticky flag raised by the finish.
 * evs_cache_pair_fed_abort(c1, c2) drops the open call: nothing is launched, no stream is touched; ordinals and stamps of both tiers
 *   are given back; dumps, stats (with hist) and counters are what they were; the same begin lists the same keys.
 * evs_cache_pair_fed_stats(c1, c2, out8, stream), cumulative: [calls finished, keys listed for C1, for C2, missed positions of fed
 *   tables, of those served from a fed block, rows spilled, hit positions served from the spill, 0].
 * THE ENVELOPE, checked at the begin before anything is allocated (the pair stays usable, the message names the policy): the
 *   fetch-first pair's -- both tiers at order 1, batch policy 2 given or resolved, the shared record, no alt-key tier, no approximate
 *   threshold --; both tiers fed caches with the same fed mask, else EVS_EINVAL; every codec pair the pair serves; the interact
 *   finish: d in {16, 32, 36} and T <= 31.  The bag form of the fed pair, the triple and a warm start of a fed pair do not exist.
 * PROTOCOL.  While a pair call is open, every other call on EITHER cache is EVS_ESTATE (single-tier begin / finish / abort, batched
 *   calls, stats, dump, row updates, a change of backing).  A finish / abort without an open pair call, or with another partner than
 *   the begin's, is EVS_ESTATE.  Argument errors of a finish are EVS_EINVAL and leave the call open.  evs_cache_destroy with an open
 *   call is fine.  evs_cache_lookup_batch_c1c2 and the other pair / triple / bag-pair calls still refuse a fed cache. */
EVS_API int evs_cache_pair_fed_begin(evs_cache *c1, evs_cache *c2, int64_t B, const int32_t *rows, uint8_t *tier, int high_agghit_threshold,
                                     uint64_t *keys1, int64_t *n_keys1_host, uint64_t *keys2, int64_t *n_keys2_host, void *stream);
EVS_API int evs_cache_pair_fed_finish(evs_cache *c1, evs_cache *c2, const void *fed1, int64_t fed1_stride_bytes, const void *fed2,
                                      int64_t fed2_stride_bytes, float *out, void *stream);
EVS_API int evs_cache_pair_fed_finish_interact(evs_cache *c1, evs_cache *c2, const void *fed1, int64_t fed1_stride_bytes, const void *fed2,
                                               int64_t fed2_stride_bytes, const float *x, int64_t x_stride, int itself, float *R, void *stream);
EVS_API int evs_cache_pair_fed_abort(evs_cache *c1, evs_cache *c2);
EVS_API int evs_cache_pair_fed_stats(evs_cache *c1, evs_cache *c2, int64_t *out8, void *stream);
/* The approximate-embedding mode of the batched EvLFU rule (the reference: cache_algo/EvLFU_C1.py:122-125, :142-152 -- a request
 * whose agg_hit reaches approx_emb_thres does not fetch its missing rows; each reuses the vector of the hit before it and is
 * reported as a hit; nothing is inserted for it).  The exact batch-1 engines take it as evs_cache_request's approx_thres; this is
 * the same mode for evs_cache_lookup_batch / evs_cache_lookup_interact on the set-associative tier.
 *   thres <= 0            off, the default: every call behaves as without this function, launch for launch.
 *   1 <= thres <= n_tables  on.  May be called between batched calls.
 * With a threshold in force a call is still batch n of the batched EvLFU rule (evs_cache_set_batch_policy), and on the snapshot:
 *   count       agg_hit(b) = the number of sample b's T keys resident at arrival, as ever: an approximated position never counts.
 *               The raise of hit ways to agg_hit(b) is unchanged; n_hits counts true hits only, n_perfect_hits the samples with
 *               agg_hit = T.
 *   substitute  where agg_hit(b) >= thres every missed position (b, t) -- a valid key that is not resident -- is served the row
 *               that sample b's nearest hit position t' < t is served: the arena row of key (t' + 1, rows[b, t']), in the cache's
 *               codec, bit-equal to that key's table row.  With no hit below t it is served a row of exact +0.0f (what the exact
 *               engine does; the reference draws a random vector there).
 *   flag        hit[b, t] = 2: non-zero, as the reference reports a hit, and told from a true hit's 1.
 *   no miss     an approximated position is in no miss list: not fetched, not inserted, not re-pointed by sa_repoint (which
 *               passes over every flag but 0).  A key approximated for one sample and missed by a sample below the threshold is
 *               inserted once, its priority the maximum agg_hit over the positions that were NOT approximated.
 *   bad index   an index out of range stays what it is without the mode: no key, flag 0, a zero row, never approximated.
 *   thres = T   a sample at the threshold has no miss, so nothing is approximated: flags, outputs, dump and counters are those
 *               of the same calls with the mode off.
 * The turn-away, the stamps, the EvLFU flush and the alternation with the bag forms hold as without the mode.  The bag forms
 * (evs_cache_lookup_bags*) ignore the setting.  The setting is not part of the warm-start state: export and load are unchanged.
 * The envelope of a call with a threshold in force, checked before anything is allocated (the cache stays usable, the message
 * names the policy): an EvLFU tier alone; batch policy 2, given or resolved; 8-way sets; any codec; miss order 0 (tables in HBM)
 * or 1 (HBM or pinned host tables).  The call always runs the unfolded chain in pointer mode -- no 4-byte row ids, no folded
 * probe, no one-launch inline form: evs_cache_set_inline_update(c, 1) is not refused, it is not taken while a threshold is on.
 * EVS_EINVAL: a plan or sampled policy; 16-way sets (EVS_SA_WAYS=16); a cache with a threshold on as a member of a C1 + C2 (+ C3)
 * lookup or of a pair bag call (those have the alt-key tier for the purpose).  File-backed tables keep their EVS_ESTATE.
 * The setter returns EVS_EINVAL, with the policy named, for a NULL cache, thres > n_tables, thres > 0 on an LRU / LFU cache
 * (the reference's have no such mode; thres <= 0 is accepted) and a row larger than the zero row (4 KiB fp32, 1 KiB of codes). */
EVS_API int evs_cache_set_batch_approx(evs_cache *c, int thres);
/* out4 (host), cumulative since creation: [batched calls run with a threshold in force, samples at or above it that had at
 * least one miss, positions served an earlier hit's row, positions served the zero row].  Synchronises the stream.  EVS_EINVAL
 * for a NULL cache or a NULL out4, before the device is touched. */
EVS_API int evs_cache_approx_stats(evs_cache *c, int64_t *out4, void *stream);
/* out8: [size, n_free, n_tombstones, n_flush, n_evict, n_requests, n_perfect_hits, n_hits];
 * hist (may be NULL): n_tables+1 resident-entry counts per priority (LRU / LFU caches: hist[0] = size, the rest 0). */
EVS_API int evs_cache_batch_stats(evs_cache *c, int64_t *out8, int64_t *hist, void *stream);
/* resident (priority, table_1based, row) triples of the batched path, unordered; returns the count.  An LRU / LFU cache reports
 * its score in the first column: LRU the way's age in batches (0 = touched by the latest batch), LFU its counter. */
EVS_API int64_t evs_cache_batch_dump(evs_cache *c, int64_t *triples, int64_t max_triples, void *stream);
/* Warm start of the batched set-associative tier: what a tier holds, exported and given back without replaying a workload.
 * The envelope is evs_cache_lookup_bags': a tier ALONE under batch policy 2, 8-way sets, tables in HBM; EvLFU, LRU or LFU;
 * codec 32 / 16 / 8 / 4; the two-copy arena or the single-copy one.  The host decides every placement (evs_cache_load_plan),
 * the device only places: one launch copies each entry's row from its backing table into the arena row its way owns and stores
 * the way word.  The exact batch-1 engines have a warm start of their own (evs_cache_exact_export / evs_cache_exact_load, below;
 * the two state formats are not converted into each other); the alt-key tier has none.
 *
 * evs_cache_batch_export first brings the cache to rest as evs_cache_batch_dump does (pending closes folded, an EvLFU flush the
 * last close asked for run), so an export never carries pending work, and returns the resident count (a negative error code
 * otherwise; entries == NULL: the count only).
 *   entries (host): rows of 5 int64 sorted by slot -- (table_1based, row, score, age, slot)
 *     score  EvLFU the priority 0 .. n_tables; LFU the counter 1 .. 63; LRU 0
 *     age    (stamp of batch n - the way's stamp) mod 2^S, n the cache's batch number: 0 = filled (LRU / LFU: or touched) by
 *            the latest batch.  The way's stamp is its word's stamp field under the policy's layout; LRU / LFU stamp batch n
 *            with n mod 2^S, EvLFU with (n mod 0x7ffffffe) + 1 mod 2^S
 *     slot   8 * set + way: the arena row the way owns, the copy-select bit of a two-copy arena not counted
 *   state16 (host, may be NULL): [format version = 1, policy, capacity, n_tables, dim, codec, n, n_flush, n_evict, n_requests,
 *     n_perfect_hits, n_hits, S, bag rule, inline-update setting (-1: never told), 0].  (n_tombstones of evs_cache_batch_stats
 *     means nothing to a set-associative tier and is not carried: a loaded cache starts it at 0.)
 *
 * evs_cache_batch_load takes n such rows into a cache whose backing is set and whose batched path holds nothing yet (fresh;
 * anything else is EVS_ESTATE).  Everything is checked on the host before the device is touched and a failure loads nothing:
 * EVS_EINVAL for a table outside 1 .. n_tables, a row outside its table, a duplicate key, a score outside the policy's range,
 * a negative age, a format version other than 1, a state of another policy.
 *   strict = 1  state16 is required; its capacity, n_tables and S must be the cache's (the key universe is held by S and by the
 *               slot check).  Every entry goes to its own slot, which must lie in the key's set and hold one entry (EVS_EINVAL);
 *               the way words come back as exported: score, stamp = (stamp of batch n - age) mod 2^S, copy-select bit 0.
 *   strict = 0  re-placement into THIS cache's geometry: every key's set is computed anew, ages are clamped to 2^S' - 2 (no
 *               loaded way carries the next batch's stamp), the entries are sorted by (set, score descending, age ascending,
 *               table, row), the first 8 of a set take its ways 0 .. 7 in that order and the rest are turned away.
 *   state16 given: n and the five counters are restored; NULL: n = the largest (clamped) age, the counters 0.
 *   Size, the free count and the EvLFU histogram are rebuilt from what was placed; a top bucket of max_perfect entries or more
 *   asks for the flush exactly as a close does (it runs with the next batched call).  The bag rule and the inline-update setting
 *   are reported, not applied.  out4 (host, may be NULL) = [placed, turned away, S of this cache, batch number after the load].
 *   n = 0 is success without a launch.  The call returns when the load has run.  (EVS_EHIP from the launch itself -- a device
 *   failure -- is the one error behind which the cache is no longer fresh: its batched-path state exists, another load is refused.)
 * Refused with the reason named and the cache left usable: a tier of a C1 + C2 (+ C3) lookup, 16-way sets (EVS_SA_WAYS=16), a
 * batch policy that is or resolves to plan / sampled (EVS_EINVAL); host-memory or file-backed tables, a cache driven by the exact
 * path or with a resident server running, a cache whose batched path already holds state (EVS_ESTATE).
 *
 * evs_cache_load_plan is the placement itself, pure host code without a GPU call -- evs_cache_batch_load runs exactly this
 * function: for a tier alone of `capacity` entries over n_tables tables of n_rows[k] rows it writes, per entry, dest_slot (-1:
 * turned away) and the way word, and out4 as above.  EVS_EINVAL as listed, and for a geometry the set-associative form cannot
 * take. */
EVS_API int64_t evs_cache_batch_export(evs_cache *c, int64_t *entries, int64_t max_entries, int64_t *state16, void *stream);
EVS_API int evs_cache_batch_load(evs_cache *c, int64_t n, const int64_t *entries, const int64_t *state16, int strict,
                                 int64_t *out4, void *stream);
EVS_API int evs_cache_load_plan(int policy, int64_t capacity, int n_tables, const int64_t *n_rows, int64_t n, const int64_t *entries,
                                const int64_t *state16, int strict, int64_t *dest_slot, uint32_t *words, int64_t *out4);
/* Warm start of the batched C1 + C2 pair (evs_cache_lookup_batch_c1c2 / _lookup_interact_c1c2 and their three-tier forms): both
 * tiers of a pair that shares its set records -- one 128-byte record per set index holds C1's 4 .. 16 ways and then C2's, C2
 * possibly as two 8-way sub-sets picked by a quotient bit -- exported together and given back together.  EvLFU tiers, tables in
 * HBM, any two codecs.  The calls above keep refusing a tier of a pair; these refuse everything that is not such a pair.  An
 * alt-key tier (evs_aprx) may be passed to the lookups that follow a load: its membership is NOT carried, it starts as it is.
 *
 * evs_cache_pair_export brings BOTH tiers to rest as evs_cache_batch_export does for one (the pair's pending closes folded, a
 * flush the last close asked of either tier run), reads the shared records once and returns the entry count of both tiers (a
 * negative error code otherwise; entries == NULL: the count only).  EVS_EINVAL for two caches that are not such a pair.
 *   entries (host): rows of 6 int64 sorted by (tier, slot) -- (tier 1 | 2, table_1based, row, score, age, slot)
 *     score  the EvLFU priority 0 .. n_tables
 *     age    (stamp of batch n - the way's stamp) mod 2^S of its tier, S = 26 - tag bits of the tier's geometry (a pair keeps one
 *            arena row per way: no copy-select bit); batch n is stamped (n mod 0x7ffffffe) + 1 mod 2^S
 *     slot   effective set * ways + way = the tier's arena row; effective set = (set index << s) | sub-set, s = log2 of the
 *            tier's sub-sets per record
 *   state32 (host, may be NULL): [format version = 3, n_tables, dim, nset], then per tier a block of 12 -- [capacity, codec, ways,
 *     sub-sets per record (1 | 2), S, batch number n, n_flush, n_evict, n_requests, n_perfect_hits, n_hits, 0] -- and zeros.
 *     (Version 1 is the single tier's state16, version 2 the exact engines' state20: each call refuses the others' by version.)
 *
 * evs_cache_pair_load takes n such rows into two caches that are BOTH fresh -- backing set, nothing served on either path yet,
 * no state loaded (anything else: EVS_ESTATE, both left as they were).  Everything is decided and checked on the host before
 * the device is touched; a failure loads nothing and leaves both caches fresh (a batch policy that was only resolved here is
 * forgotten again), so a lookup that follows starts a cold pair.  The pair is started exactly as its first lookup starts it
 * (the shared records, each tier's counters), then ONE launch copies every entry's row from its tier's table into its tier's
 * arena and stores its way word into the shared record.
 *   strict = 1  state32 is required; its n_tables, nset, and per tier capacity, ways, sub-sets and S must be this pair's (and its
 *               dim).  Every entry goes to its own slot of its own tier, which must lie in the key's effective set and hold one
 *               entry; the words come back as exported; n and the five counters of each tier are restored.
 *   strict = 0  re-placement into THIS pair's geometry: a key stays in the tier it was exported from (the tier is its precision;
 *               nothing spills into the other), its effective set is computed anew, ages are clamped to 2^S' - 2, per effective
 *               set the `ways` best of (score descending, age ascending, table, row) take ways 0 .. ways - 1 and the rest are
 *               turned away.  state32 given: each tier's n and counters are its block's; NULL: n = the largest clamped age over
 *               both tiers, the same for both, the counters 0.
 *   EVS_EINVAL, the reason named: a tier outside {1, 2}, a table or row outside its tier's table, a score outside 0 .. n_tables, a
 *   negative age, a key twice in one tier, a key in both tiers, a format version other than 3.
 *   Size, free count and priority histogram of each tier are rebuilt from what was placed; a tier whose top bucket holds
 *   max_perfect entries or more asks for its flush as a close does (it runs with the next pair call).
 *   out8 (host, may be NULL) = [placed in C1, turned away from C1, S1, placed in C2, turned away from C2, S2, batch number after
 *   the load, 0].  n = 0 is success without a launch.  The call returns when the load has run.  (EVS_EHIP from the launch itself
 *   is the one error behind which the pair is no longer fresh.)
 * Refused with the reason named and both caches left usable: a cache that is not EvLFU, tiers that disagree on n_tables or dim,
 * a batch policy that is or resolves to plan / sampled on either tier, a cache set to fetch-first (evs_cache_set_miss_order),
 * capacities for which the pair gets no shared record -- a tier would have fewer than 4 ways, or EVS_SA_PAIR=0: the shared
 * record is the only geometry this call loads -- (EVS_EINVAL); host-memory or file-backed tables, a resident server running,
 * a cache that is not fresh (EVS_ESTATE).
 *
 * evs_cache_pair_load_plan is the placement itself, pure host code without a GPU call -- evs_cache_pair_load runs exactly this
 * function: for a pair of cap1 + cap2 entries over n_tables tables of n_rows1[k] / n_rows2[k] rows (the key universe is built
 * from the larger of the two per table) it writes, per entry, dest_slot (its slot in its tier; -1: turned away) and the way
 * word, and out8 as above.  EVS_EINVAL as listed and for capacities without a shared record; a refusal writes nothing. */
EVS_API int64_t evs_cache_pair_export(evs_cache *c1, evs_cache *c2, int64_t *entries, int64_t max_entries, int64_t *state32, void *stream);
EVS_API int evs_cache_pair_load(evs_cache *c1, evs_cache *c2, int64_t n, const int64_t *entries, const int64_t *state32, int strict,
                                int64_t *out8, void *stream);
EVS_API int evs_cache_pair_load_plan(int64_t cap1, int64_t cap2, int n_tables, const int64_t *n_rows1, const int64_t *n_rows2, int64_t n,
                                     const int64_t *entries, const int64_t *state32, int strict, int64_t *dest_slot, uint32_t *words,
                                     int64_t *out8);
/* File-backed miss tier: the reference's mmap miss path (emb_storage/mmap_file_read.py:32-40,
 * reader pool mixed_precs_caching/evlfu_8.cpp:191-250) under the GPU cache.  evs_filetier_open maps every
 * ev-table-N.bin read-only (row r at byte row_bytes * r) and REGISTERS tables with the GPU (hipHostRegister, mapped:
 * kernels read them over the bus, zero-copy) smallest first while their total fits pinned_budget_bytes; the others stay
 * plain mappings ("staged"): the batched lookup lists the batch's de-duplicated new keys, a pool of host threads copies
 * those rows out of the mappings into a pinned staging buffer and the fill kernel takes them from there -- every missing
 * row is read from the file once per batch.  evs_cache_set_file_backing replaces evs_cache_set_backing; with staged
 * tables only the batched lookups (evs_cache_lookup_batch / _interact, and the two- / three-tier forms) are served.  The tier outlives the cache's use
 * of it; evs_filetier_close unmaps.  evs_filetier_fetch is the reader pool itself (host memory in, host memory out). */
typedef struct evs_filetier evs_filetier;
EVS_API int evs_filetier_open(evs_filetier **out, int n_tables, const char *const *paths, int64_t row_bytes,
                              int64_t pinned_budget_bytes);
EVS_API int evs_filetier_info(evs_filetier *ft, int64_t *n_rows, const void **dev_ptrs, int *registered, int64_t *pinned_bytes);
EVS_API int evs_filetier_fetch(evs_filetier *ft, int64_t n, const uint64_t *keys /* table_1based << 32 | row */, void *dst,
                               uint32_t skip_mask);
EVS_API int evs_filetier_close(evs_filetier *ft);
EVS_API int evs_cache_set_file_backing(evs_cache *c, evs_filetier *ft);
EVS_API int64_t evs_cache_staged_rows(evs_cache *c);   /* rows the reader pool has fetched for this cache so far */
/* a12: the alt-key ("approximate embedding") tier C3 -- mixed_precs_caching/aprx_embedding.cpp and
 * evlfu_8.cpp:474-490,492-667 (request_to_c1_c2_c3).  DETERMINISTIC RE-SPECIFICATION, parity unpinned:
 * the reference fills the tier from asynchronous threads racing the request thread.  Here keys evicted
 * (not flushed) from C1/C2 are queued; when 50 (IO_JOB_Q_SIZE) are pending the batch is inserted at the
 * start of the next request (second-chance FIFO eviction makes room).  On a double miss whose alt key is
 * mapped and whose alt row is resident in C1 (else C2), that row's vector is served (tier code 3),
 * decoded at the precision of the tier holding it; the key's recency flag is set; the request's agg_hit
 * counts it; nothing is inserted for it.  alt_tables[k]: device-accessible uint32[n_rows[k]] with
 * alt_key = alt_row*100 + alt_table_1based (the reference's alt-key files store this big-endian,
 * script/convert_altkeys_to_binary.py:27-57; convert to native order when loading). */
typedef struct evs_aprx evs_aprx;
EVS_API int evs_aprx_create(evs_aprx **out, int64_t capacity, int n_tables);
EVS_API int evs_aprx_destroy(evs_aprx *p);
EVS_API int evs_aprx_set_altkeys(evs_aprx *p, const uint32_t *const *alt_tables, const int64_t *n_rows);
EVS_API int evs_aprx_stats(evs_aprx *p, int64_t *out4 /* size, n_hit, n_pending, error */, void *stream);
/* APRX_EV's public single-key methods applied in order (the part of the tier that IS pinned to the compiled reference,
 * driven single-threaded): ops = n x (op, table_1based, row), op 0 insert_altkey (aprx_embedding.cpp:278-288: evict one
 * when full, push on the FIFO, map[key] = {alt key of the row, false}), 1 get_altkey_str (:341-350), 2 set_recency_flag_c3
 * (:402-411), 3 evict_one_key (:390-400, second chance :360-388).  res[i] (device): op 0 the alt key, op 1 the alt key or
 * 0xffffffff on a miss, else 0.  evs_aprx_dump_queue: the FIFO front to back as (table_1based, row) pairs (host),
 * stale duplicates included (print_all_keys_in_c3, :430-434); returns its length. */
EVS_API int evs_aprx_apply_ops(evs_aprx *p, int64_t n, const int32_t *ops, uint32_t *res, void *stream);
EVS_API int64_t evs_aprx_dump_queue(evs_aprx *p, int64_t *pairs, int64_t max_pairs, void *stream);
/* evs_cache_request_c1c2 with the alt-key tier (c3 may be NULL = plain two tiers). */
EVS_API int evs_cache_request_c1c2c3(evs_cache *c1, evs_cache *c2, evs_aprx *c3, int64_t B, const int32_t *rows,
                                     float *out, uint8_t *tier, int high_agghit_threshold, void *stream);
/* The tier pair / triple as a RESIDENT SERVER: request_to_c1_c2 / request_to_c1_c2_c3 one request at a time, as the
 * reference's cache manager drives them (mixed_precs_caching/cache_manager.cpp:170-229, evlfu_8.cpp:492-667, 669-796), without the
 * launch and the synchronise evs_cache_request_c1c2[c3] costs per call.  The same kernel body as that call's (same tier codes,
 * rows, list order, counters) stays on the device and is fed through the mailbox of evs_cache_serve_*: same request line (7 ids +
 * a guard per 32-byte sector, ids by value or by address, optional destination address), same ring rule (slot = sequence %
 * n_slots, valid until n_slots - 1 more requests are POSTED unless evs_tiers_serve_consumed says who still reads it), same
 * limits (at most 28 tables; _request_to at most 26), one host thread per server, idle time-out idle_us.  tier_host: the T tier
 * codes of evs_cache_request_c1c2c3 (0 miss, 1 C1, 2 C2, 3 alt-key hit).  c3 may be NULL.
 * evs_tiers_serve_start (cache_manager.cpp:36-53: the tiers are built once and serve every later request): EVS_EINVAL for NULL
 * out / c1 / c2 / ring, n_slots < 1, idle_us < 1, c1 == c2, tiers that are not EvLFU or disagree on n_tables / dim, more than
 * 28 tables; EVS_ESTATE for a tier without backing tables, with staged file tables, used through the batched path, running
 * its own single-tier server, or already a member of a tier server.  A member cannot start a single-tier server either.
 * Every call that reads or writes a member's exact state -- evs_cache_stats / _dump / _request / _request_c1c2[c3] / _set_backing /
 * _set_file_backing / _reset_counters / _destroy, evs_aprx_stats / _apply_ops / _dump_queue / _batch_dump / _set_altkeys /
 * _destroy -- sends the server home first (it writes the policy state back on its way out); the next request starts it again,
 * behind any launch-per-call request made on the members in between.  Destroying a member stops the server for good: later
 * requests return EVS_ESTATE.
 * evs_tiers_serve_request (evlfu_8.cpp:492-667 / 669-796 for one request): rows in ring slot *slot_out (device).
 * evs_tiers_serve_request_to (the same; cache_manager.cpp:231-237 hands the rows to the caller's buffer): rows to out_dev,
 * exactly one of rows_host / ids_dev given, as evs_cache_serve_request_to.
 * evs_tiers_serve_consumed / _stop / _destroy: as evs_cache_serve_consumed / _stop (cache_manager.cpp has no teardown: the
 * process exits); _destroy frees the server, not its members. */
typedef struct evs_tier_server evs_tier_server;
EVS_API int evs_tiers_serve_start(evs_tier_server **out, evs_cache *c1, evs_cache *c2, evs_aprx *c3 /* may be NULL */,
                                  int high_agghit_threshold, float *ring, int n_slots, int64_t idle_us);
EVS_API int evs_tiers_serve_request(evs_tier_server *s, const int32_t *rows_host, uint8_t *tier_host, int *slot_out);
EVS_API int evs_tiers_serve_request_to(evs_tier_server *s, const int32_t *rows_host, const int64_t *ids_dev,
                                       int64_t ids_stride, float *out_dev, uint8_t *tier_host);
EVS_API int evs_tiers_serve_consumed(evs_tier_server *s, int slot, void *stream);
EVS_API int evs_tiers_serve_stop(evs_tier_server *s);
EVS_API int evs_tiers_serve_destroy(evs_tier_server *s);
/* out8 (host): [min_C1, n_perfect, size, n_flush, n_evict, n_requests, n_perfect_hits, n_hits].
 * Synchronises the stream.  Returns EVS_ESTATE if the policy hit an inconsistency. */
EVS_API int evs_cache_stats(evs_cache *c, int64_t *out8, void *stream);
EVS_API int evs_cache_reset_counters(evs_cache *c, void *stream);
/* Resident keys in list order as (bucket | frequency | 0, table_1based, row) triples (host);
 * returns the number of resident keys (or a negative error). */
EVS_API int64_t evs_cache_dump(evs_cache *c, int64_t *triples, int64_t max_triples, void *stream);
/* Warm start of the EXACT batch-1 engines -- this one and the host engine below (evs_hostcache_export / _load) share the format,
 * so a state saved by one loads into the other.  The exact policies are deterministic: a fresh cache that loads the export of
 * a cache cut anywhere in a request stream and continues the stream gives, bit for bit, the hit flags, rows, list order and
 * counters of the uncut run (tests/test_exact_warm_host.py, tests/test_gpu_exact_warm.py on the reference's golden traces).
 *   entries (host): n rows of 3 int64 = evs_cache_dump's triples in its order: (score, table_1based, row); score = the EvLFU
 *     bucket 0 .. n_tables, the LFU frequency >= 1, 0 for LRU.  Array order IS list order: EvLFU buckets ascending and front to
 *     back inside a bucket, LFU frequencies ascending and FIFO inside a frequency, LRU the recency list front to back.
 *   state20 (host): [format version = 2, policy, capacity, n_tables, dim, codec, min_C1, n_perfect, least_freq, n_flush, n_evict,
 *     n_requests, n_perfect_hits, n_hits, max_perfect, flush_n, perfect_mode, 0, 0, 0].  (Version 1 is the batched tier's state16;
 *     neither loader accepts the other's state.)  Arena slot numbers, the free-stack order and the hash layout are not part of
 *     the state: no entry point can observe them.
 * evs_cache_exact_export = evs_cache_dump (a resident server is sent home first) plus the state; returns the resident count,
 *   entries == NULL: the count only; state20 may be NULL.  EVS_ESTATE for a cache on the batched path.
 * evs_cache_exact_load gives a state to a FRESH cache: backing set, never used through either path, no server running, not a
 *   member of a tier server -- anything else is EVS_ESTATE and the cache stays usable, as for staged file-backed tables (the
 *   exact path does not serve them; pinned-host tables and registered file-tier tables are accepted, the kernel reads their rows
 *   over the bus as the exact engine's miss path does).  Everything is checked on the host before the device is touched, by
 *   evs_exact_load_check (pure host code, callable without a GPU; both loaders run exactly this function), and a failure loads
 *   nothing: EVS_EINVAL, the reason named, for a table outside 1 .. n_tables, a row outside its table, a duplicate key, a score
 *   outside the policy's range (EvLFU 0 .. n_tables, LRU 0, LFU 1 .. max_freq - 2 with max_freq the device engine's 2^22; the
 *   host engine passes 0 = unbounded), scores that are not non-decreasing along the array (the lists must be contiguous runs),
 *   n > capacity (no shrinking: re-placement into a smaller tier is the batched tier's feature), a version other than 2, a state
 *   of another policy, state scalars out of range (min_C1 outside 0 .. n_tables, least_freq < 1 or beyond max_freq - 1, a
 *   negative counter).
 *     strict = 1  state20 is required; its policy, capacity, n_tables, max_perfect, flush_n and perfect_mode must equal the
 *                 cache's; min_C1, n_perfect, least_freq and the five counters are restored; dim and codec are reported, not
 *                 compared (rows always come from the cache's own backing).  The cache then continues exactly as the exporter
 *                 would have.
 *     strict = 0  any capacity >= n and any constants; with state20 the scalars are taken from it -- range-checked and otherwise
 *                 TRUSTED: min_C1, least_freq and n_perfect are not functions of the entries (the reference lets the first two
 *                 rest on an empty list and recounts the third only at a perfect request or a flush), so they are not compared
 *                 with the run lengths; a made-up value moves a flush or an eviction, or raises the policy's sticky error
 *                 (EVS_ESTATE from evs_cache_stats), and corrupts nothing --, with state20 = NULL they are
 *                 derived: min_C1 = the lowest non-empty bucket (0 when empty), n_perfect = the length of bucket n_tables,
 *                 least_freq = the lowest frequency present (1 when empty), counters 0.
 *   The device load is ONE parallel launch: entry i of the array becomes entry index i (arena row i); a lane group per entry
 *   copies the row from the backing table, one lane writes the entry record and its list links and claims the key's slot of the
 *   open-address map with a 64-bit compare-and-swap; the same launch writes the free stack and the LFU list heads.  No request
 *   is replayed.  n = 0 is success without a launch; the call returns when the load has run.  On success the cache is an
 *   exact-path cache: evs_cache_lookup_batch on it is refused (EVS_ESTATE) as for any exact-path cache.  Both map forms are
 *   built: the packed one (capacity <= 2^25: key and entry in the one word the compare-and-swap installs) and the unpacked one
 *   (larger caches: the key by compare-and-swap, the entry beside it in slot_entry[]).
 *   (EVS_EHIP from the copies or the launch is the one error behind which the cache is no longer fresh.)
 * A C1 + C2 pair is exported and loaded one cache at a time: without an alt-key tier the pair keeps no state outside its two
 * caches.  OUT OF SCOPE: the alt-key tier (evs_aprx / evs_hostaprx: its pending-eviction queue is not dumpable), and converting
 * between this format and the batched tier's. */
EVS_API int64_t evs_cache_exact_export(evs_cache *c, int64_t *entries, int64_t max_entries, int64_t *state20, void *stream);
EVS_API int evs_cache_exact_load(evs_cache *c, int64_t n, const int64_t *entries, const int64_t *state20, int strict, void *stream);
EVS_API int evs_exact_load_check(int policy, int64_t capacity, int n_tables, const int64_t *n_rows, int64_t n, const int64_t *entries,
                                 const int64_t *state20, int strict, int64_t max_freq);   /* pure host */

/* ---------------------------------------------------------------------------
 * a6-a9, a12 at batch 1: the HOST engine of the exact policies (csrc/evs_hostcache.hip).
 * The reference's EVStore loop is one request at a time (--test-mini-batch-size=1, dlrm_s_pytorch_C1.py:236-239) and
 * its policies are sequential by definition; a chain of dependent pointer updates is a CPU cache hierarchy's job (one
 * wavefront replays a request in 28 us + launch + synchronise, one host core in a few).  Same policies, same constants,
 * same argument meaning as evs_cache_create / evs_cache_request / evs_cache_request_c1c2c3 / evs_aprx_* above, same
 * golden traces bit for bit -- but every pointer is HOST memory, there is no stream, and nothing touches the GPU:
 *   tables[k]   any host-readable mapping of ev-table-{k+1}.bin in the tier's codec (mmap, pinned, malloc);
 *               a miss reads ONE row from it (evlfu_8.cpp:380-414 get_from_file: fseek + fread)
 *   rows        (B, n_tables) int32, requests replayed strictly in order
 *   out         (B, n_tables, dim) fp32, decoded from the tier's codec
 *   hit / tier  (B, n_tables) bytes
 * The tier's arena (capacity x dim*codec/8 bytes) and its hash / lists live in host memory.  Errors as everywhere:
 * EVS_EINDEX for a row id outside its table, EVS_ESTATE when the policy state is inconsistent (what the Python
 * reference would raise on).  The batched (snapshot) lookups stay on the GPU tier.
 * evs_hostcache_stats out8 = [min_C1 | LFU least_freq, n_perfect, size, n_flush, n_evict, n_requests, n_perfect_hits,
 * n_hits]; evs_hostcache_dump = evs_cache_dump's triples; evs_hostaprx_* = evs_aprx_* (alt_tables: host uint32 arrays,
 * native byte order).
 * ------------------------------------------------------------------------- */
typedef struct evs_hostcache evs_hostcache;
typedef struct evs_hostaprx evs_hostaprx;
EVS_API int evs_hostcache_create(evs_hostcache **out, int policy, int64_t capacity, int n_tables, int dim, int codec,
                                 double flush_rate, double perfect_item_cap, int flush_extra, int perfect_mode);
EVS_API int evs_hostcache_destroy(evs_hostcache *c);
EVS_API int evs_hostcache_set_backing(evs_hostcache *c, const void *const *tables, const int64_t *n_rows);
EVS_API int evs_hostcache_request(evs_hostcache *c, int64_t B, const int32_t *rows, float *out, uint8_t *hit,
                                  int approx_thres);
EVS_API int evs_hostcache_request_c1c2c3(evs_hostcache *c1, evs_hostcache *c2, evs_hostaprx *c3 /* may be NULL */,
                                         int64_t B, const int32_t *rows, float *out, uint8_t *tier,
                                         int high_agghit_threshold);
EVS_API int evs_hostcache_stats(evs_hostcache *c, int64_t *out8);
EVS_API int evs_hostcache_reset_counters(evs_hostcache *c);
EVS_API int64_t evs_hostcache_dump(evs_hostcache *c, int64_t *triples, int64_t max_triples);
/* Warm start of the host engine: evs_cache_exact_export / evs_cache_exact_load's format, checks and strict / non-strict rules
 * (above), in pure host code -- the load builds the tier from its own take / push_back primitives in array order, then sets the
 * scalars.  The target must be fresh (backing set, no request served, nothing loaded): EVS_ESTATE otherwise. */
EVS_API int64_t evs_hostcache_export(evs_hostcache *c, int64_t *entries, int64_t max_entries, int64_t *state20);
EVS_API int evs_hostcache_load(evs_hostcache *c, int64_t n, const int64_t *entries, const int64_t *state20, int strict);
EVS_API int evs_hostaprx_create(evs_hostaprx **out, int64_t capacity, int n_tables);
EVS_API int evs_hostaprx_destroy(evs_hostaprx *p);
EVS_API int evs_hostaprx_set_altkeys(evs_hostaprx *p, const uint32_t *const *alt_tables, const int64_t *n_rows);
EVS_API int evs_hostaprx_stats(evs_hostaprx *p, int64_t *out4 /* size, n_hit, n_pending, error */);
EVS_API int evs_hostaprx_apply_ops(evs_hostaprx *p, int64_t n, const int32_t *ops, uint32_t *res);
EVS_API int64_t evs_hostaprx_dump_queue(evs_hostaprx *p, int64_t *pairs, int64_t max_pairs);

/* ---------------------------------------------------------------------------
 * Online row updates: a model refresh while the store serves (no reference counterpart -- the reference's tables are files
 * written offline, script/reduce_precision.py + script/convert_ev_to_binary.py, and its tiers are filled from them).
 * A delta of (table, row) -> new fp32 vector is encoded in the table's codec (bit-exact with evs_encode_table for the same
 * values), stored at its row in the table AND into every cached copy of that row, in stream order, so that "served rows are
 * exactly the table rows" (evs_cache_set_batch_policy, above) keeps holding for resident keys.
 *   keys    device (n, 2) int32, 8-byte aligned: keys[i] = (table index 0-based, row) -- "table = position", as in the
 *           request arrays.  The keys of ONE call must be distinct: with duplicates the table and a cached copy may keep
 *           different ones of the duplicated values.
 *   values  device fp32, row i at values + i * values_stride, values_stride >= d (16-byte aligned with a stride % 4 == 0:
 *           vector loads).
 *   n == 0 is success; arguments are checked before the device is touched (EVS_EINVAL); a key out of range is skipped and
 *   raises the sticky flag evs_check_index_errors reports.
 * evs_table_update_rows   tables without a cache in front: tables / n_rows are HOST arrays of n_tables (<= 64) device-
 *                         accessible table addresses / row counts, rows of d elements in `codec` (32 / 16 / 8 / 4).
 * evs_cache_update_rows   ONE launch: encode in the cache's codec, store the row into c's backing table, look the key up in c
 *                         and store the same bytes into the arena row when it is resident.  n_resident (device int64, may be
 *                         NULL) receives the number of keys that were resident WHEN THE CALL RAN: an EvLFU flush that the last
 *                         batch's close has asked for runs with the next batched call (or evs_cache_batch_stats / _dump), not
 *                         here, and may retire keys this call counted -- their arena rows were written all the same.
 * evs_cache_refresh_rows  the same look-up; the arena row is re-copied from the backing row -- for callers who wrote the table
 *                         themselves, and for tables the kernels can read but must not write (registered file mappings,
 *                         host tables written by the host).
 * Every form of the tier is served: the exact engines (EvLFU / LRU / LFU: entry e owns arena row e), the batched policies 0
 * and 1 (the packed hash words), the set-associative policy 2 (one tier with 8 or 16 ways and its two-copy arena -- the live
 * copy is the one the way word's select bit names --, or a tier's view of a shared C1 + C2 record).  A tier pair or triple is
 * updated by one call per cache, each in its own codec on its own backing; the alt-key tier stores no rows and needs
 * nothing.  A fresh cache only has its table written and stays fresh.  Backing in HBM or in pinned device-visible host memory.
 * EVS_ESTATE: a cache without backing; evs_cache_update_rows on a file-backed cache (read-only mappings);
 * evs_cache_refresh_rows on a file tier with staged tables (no device-visible rows).
 * THE POLICY STATE DOES NOT MOVE: no way word, hash word, priority, list link, stamp or counter changes; evs_cache_dump /
 * _batch_dump / _stats / _batch_stats return the same before and after.  An update never changes residency.
 * ORDERING: stream-ordered like the lookups -- a lookup on the same stream after the call sees the new rows; concurrent lookups
 * on other streams are the caller's to order.  A resident server (evs_cache_serve_*, evs_tiers_serve_*) is sent home first, as
 * evs_cache_stats does, and the next request starts it again BEHIND the update launch: per-XCD L2s are not coherent inside a
 * running launch, so a resident kernel cannot be relied on to see the new bytes; a kernel boundary can.  (The dispatcher of
 * evs_emb_interact_serve_* reads its tables from a resident launch too: serve_stop it around an update.)
 * evs_hostcache_refresh_rows: the host engine's form of evs_cache_refresh_rows -- the caller writes its host tables, then
 * refreshes; keys_host (n, 2) int32 and n_resident_host (may be NULL) are HOST memory; keys out of range are skipped and the
 * call then returns EVS_EINDEX (the host engine has no sticky flag).
 * ------------------------------------------------------------------------- */
EVS_API int evs_table_update_rows(int codec, int d, int n_tables, void *const *tables, const int64_t *n_rows, int64_t n,
                                  const int32_t *keys, const float *values, int64_t values_stride, void *stream);
EVS_API int evs_cache_update_rows(evs_cache *c, int64_t n, const int32_t *keys, const float *values, int64_t values_stride,
                                  int64_t *n_resident, void *stream);
EVS_API int evs_cache_refresh_rows(evs_cache *c, int64_t n, const int32_t *keys, int64_t *n_resident, void *stream);
EVS_API int evs_hostcache_refresh_rows(evs_hostcache *c, int64_t n, const int32_t *keys_host, int64_t *n_resident_host);

/* ---------------------------------------------------------------------------
 * a14: the reference's cache-manager C ABI (mixed_precs_caching/cache_manager.cpp), bound by
 * cache_algo/cpp_socket_client.py:69-83 through ctypes.  Same names, same signatures.
 *   ev_lookup: reads 26 int32 row ids (0-based; table = position), returns a pointer to the
 *   library-owned static float[26*36], table-major, valid until the next call; not re-entrant;
 *   side effect perfect-hit counter += (all 26 hit).  NULL (after printing) on a configuration error
 *   (the reference prints and exit(-1)s).
 * Configuration: the reference's five compile-time knobs (cache_manager.cpp:13-20) at run time.
 *   n_caching_layer 1 (C1), 2 (C1 + C2 = request_to_c1_c2) or 3 (+ the alt-key tier = request_to_c1_c2_c3;
 *   needs evs_manager_set_altkey_dir / EVS_ALTKEY_DIR; sizes from size_proportion "a-b-c" as evlfu_8.cpp:63-92),
 *   main_precision 32|16|8|4, secondary_precision 16|8|4,
 *   total_size in fp32-row equivalents (one tier: capacity = total_size * 32/main_precision entries;
 *   two tiers: total_size/2 each, i.e. (total/2)*32/main and (total/2)*32/secondary entries -- except an 8-bit
 *   secondary tier under a 32/16-bit main tier, which gets (total/2)*16 entries because the reference's
 *   EVLFU_8BIT constructor multiplies an already-multiplied capacity by 4 again: evlfu_32.cpp:102, evlfu_16.cpp:95,
 *   evlfu_8.cpp:93; evs_manager_tier_capacity reports what was built),
 *   ev_table_root = directory holding ev-table/binary, ev-table-16/binary, ev-table-8/binary,
 *   ev-table-4/binary (evlfu_*.hpp EV_TABLE_PATH), backing 0 = tables in HBM, 1 = pinned host.
 *   Without a call, ev_lookup reads EVS_N_CACHING_LAYER, EVS_MAIN_PRECISION, EVS_TOTAL_SIZE,
 *   EVS_EV_TABLE_ROOT, EVS_BACKING from the environment on first use.
 * ------------------------------------------------------------------------- */
EVS_API int evs_manager_configure(int n_caching_layer, int main_precision, int secondary_precision,
                                  int64_t total_size, const char *size_proportion, const char *ev_table_root,
                                  int backing);
EVS_API int evs_manager_set_altkey_dir(const char *dir);  /* n_caching_layer 3: directory of the alt-key ev-table-N.bin files */
EVS_API long long evs_manager_perfect_hit(void);
EVS_API long long evs_manager_tier_capacity(int tier);   /* entries of tier 1 | 2 | 3 as configured (0 = absent) */
EVS_API long long evs_manager_aprx_hit(void);             /* evlfu_8bit->aprx_ev_hit (cache_manager.cpp:279) */
/* which engine ev_lookup runs on (cache_manager.cpp:170-229 has one, compiled in): 0 not initialised, 1 the host engine,
 * 2 the GPU engine launched per request, 3 the GPU engine through a resident server (EVS_MANAGER_SERVE=1 with EVS_BACKING=hbm |
 * pinned: evs_cache_serve_request_to for one layer, evs_tiers_serve_request_to for two / three; the server is stopped at exit).
 * Reads the manager's fields only: callable without a GPU. */
EVS_API int evs_manager_engine(void);
/* Warm start of the manager's tiers: evs_cache_exact_export / evs_hostcache_export (and the strict loads) forwarded to tier 1 | 2
 * of whichever engine ev_lookup runs; the manager is initialised first, as ev_lookup does.  A resident server is stopped first
 * and started again by the next lookup.  n_caching_layer == 3 is refused (EVS_EINVAL): the alt-key tier has no export. */
EVS_API int64_t evs_manager_export(int tier, int64_t *entries, int64_t max, int64_t *state20);
EVS_API int evs_manager_load(int tier, int64_t n, const int64_t *entries, const int64_t *state20);
EVS_API float *ev_lookup(int *arr);                      /* cache_manager.cpp:231 */
EVS_API float *get_ev_values(int *arr);                  /* cache_manager.cpp:257 */
EVS_API void print_perfect_hit(void);                    /* cache_manager.cpp:262 */
EVS_API int ev_lookup_based_on_list_keys(int *arr);      /* cache_manager.cpp:239 (dead in the reference) */
EVS_API void test_arr(int *arr);                         /* cache_manager.cpp:154 */
EVS_API void init_global_vars(void);                     /* cache_manager.cpp:410 (socket server: not built) */
EVS_API void start_server_threads(void);                 /* cache_manager.cpp:419 (socket server: not built) */

#ifdef __cplusplus
}
#endif
#endif /* EVSTORE_HIP_H */
