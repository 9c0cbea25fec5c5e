// Wide models (33 <= F <= 128): what the fp32 unit (evs_fused_wide.hip) and the encoded unit (evs_fused_wide_q.hip) share -- the
// kernel arguments, the instantiation ids, the packed triangle's row offset and the refusals of the C entries.
#pragma once
#include "evs_common.h"

namespace evs {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f32x4 global_f32x4;

struct WideArgs {
    const char *base[EVS_MAX_WIDE_FEATURES];   // dense: feature f.  gather: x, then table f - 1
    int64_t aux[EVS_MAX_WIDE_FEATURES];        // dense: row stride in BYTES.  gather: x's stride in bytes, then the rows of table f - 1
    const int64_t *idx;                        // gather: the (T, B) indices; NULL = dense form
    int64_t idx_stride;
    float *R;
    const char *zeros;                         // zero_page(); encoded tables: zero_code_page(codec)
    int *err;
    int B, F, itself, out_row;                 // out_row = d + P
};

constexpr int kWideD[4] = {16, 32, 36, 64};
constexpr int kWideNt[4] = {3, 4, 6, 8};
constexpr int wide_d_id(int d) { return d == 16 ? 0 : d == 32 ? 1 : d == 36 ? 2 : d == 64 ? 3 : -1; }
constexpr int wide_nt_id(int F) { return F <= 48 ? 0 : F <= 64 ? 1 : F <= 96 ? 2 : 3; }
// pairs in front of row i of the packed triangle
__device__ __forceinline__ int wide_tri(int i, int itself) { return (i * (i - 1 + 2 * itself)) >> 1; }

// what both entries refuse alike, before a device is touched
static inline int wide_shape_ok(const char *who, int64_t B, int F, int d) {
    EVS_REQUIRE(B >= 0, "%s: bad shape B=%lld", who, (long long)B);
    EVS_REQUIRE(F > EVS_MAX_FEATURES && F <= EVS_MAX_WIDE_FEATURES, "%s: F=%d features (the wide kernel takes %d to %d)", who, F,
                EVS_MAX_FEATURES + 1, EVS_MAX_WIDE_FEATURES);
    EVS_REQUIRE(wide_d_id(d) >= 0, "%s: no kernel for d=%d (16, 32, 36, 64)", who, d);
    return EVS_OK;
}
static inline bool aligned16(const void *p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace evs
