// evs_table_update_rows: the scatter-encode kernel of the online row updates (evs_update.h) over plain tables -- each value
// row is encoded to the tables' codec and stored at its row, bit-exact with evs_encode_table for the same values.  The cache
// tiers' forms (the same kernel with a look-up in front of the stores) live in evs_cache.hip, next to struct evs_cache.
#include "evs_update.h"

extern "C" int evs_table_update_rows(int codec, int d, int n_tables, void *const *tables, const int64_t *n_rows, int64_t n,
                                     const int32_t *keys, const float *values, int64_t values_stride, void *stream) {
    using namespace evs;
    EVS_REQUIRE(codec == 32 || codec == 16 || codec == 8 || codec == 4, "evs_table_update_rows: codec %d (32, 16, 8 or 4)", codec);
    EVS_REQUIRE(d >= 1 && (codec != 4 || d % 2 == 0), "evs_table_update_rows: d=%d (4-bit rows need an even dimension)", d);
    EVS_REQUIRE(n_tables >= 1 && n_tables <= kMaxTables, "evs_table_update_rows: n_tables=%d (1..%d)", n_tables, kMaxTables);
    { const int cc = upd_check_common("evs_table_update_rows", n, keys); if (cc) return cc < 0 ? cc : EVS_OK; }
    EVS_REQUIRE(tables && n_rows && values, "evs_table_update_rows: NULL argument");
    EVS_REQUIRE(reinterpret_cast<uintptr_t>(keys) % 8 == 0, "evs_table_update_rows: keys must be 8-byte aligned");
    EVS_REQUIRE(values_stride >= d, "evs_table_update_rows: values_stride %lld is below d = %d", (long long)values_stride, d);
    RowUpdateArgs<NoLookup> a{};
    for (int k = 0; k < n_tables; k++) {
        EVS_REQUIRE(tables[k] || n_rows[k] == 0, "evs_table_update_rows: table %d is NULL", k);
        EVS_REQUIRE(n_rows[k] >= 0, "evs_table_update_rows: table %d has %lld rows", k, (long long)n_rows[k]);
        a.tables[k] = static_cast<unsigned char *>(tables[k]);
        a.n_rows[k] = n_rows[k];
    }
    a.keys = keys; a.values = values; a.values_stride = values_stride; a.n = n;
    a.n_tables = n_tables; a.d = d; a.row_bytes = d * codec / 8;
    a.values_aligned = (reinterpret_cast<uintptr_t>(values) % 16 == 0 && values_stride % 4 == 0) ? 1 : 0;
    a.n_resident = nullptr;
    a.err = index_error_flag();
    if (!a.err) return EVS_EHIP;
    launch_row_update(codec, a, reinterpret_cast<hipStream_t>(stream));
    EVS_HIP_CHECK(hipGetLastError());
    return EVS_OK;
}
