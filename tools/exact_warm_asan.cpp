// AddressSanitizer / UBSan run of the host engine's warm start (csrc/evs_hostcache.hip compiled host-only, with the checks of
// csrc/evs_exact_warm.h): random tables, all four codecs, EvLFU / LRU / LFU -- requests, export, load into a fresh twin (strict,
// and without a state into a larger one), 2 000 requests on exporter and twin side by side (same flags, same rows), export again;
// then states that must be refused.  Built and run by tests/test_exact_warm_asan.py.
#include "evstore_hip.h"
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s (line %d): %s\n", #cond, __LINE__, evs_last_error()); return 1; } } while (0)
int main() {
    std::mt19937_64 rng(11);
    const int codecs[] = {32, 16, 8, 4};
    long total = 0, refused = 0;
    for (int iter = 0; iter < 36; iter++) {
        const int T = (int)(rng() % 26) + 1, d = (rng() & 1) ? 36 : 16, codec = codecs[iter % 4], policy = (iter / 4) % 3;
        const int64_t cap = (int64_t)(rng() % 300) + T;
        const int row_bytes = d * codec / 8;
        std::vector<int64_t> n_rows(T);
        std::vector<std::vector<unsigned char>> tabs(T);
        std::vector<const void *> ptrs(T);
        for (int k = 0; k < T; k++) {
            n_rows[k] = (int64_t)(rng() % 500) + 1;
            tabs[k].resize((size_t)n_rows[k] * row_bytes);
            for (auto &b : tabs[k]) b = (unsigned char)(rng() % 200);
            ptrs[k] = tabs[k].data();
        }
        auto make = [&](int64_t capacity) {
            evs_hostcache *c = nullptr;
            if (evs_hostcache_create(&c, policy, capacity, T, d, codec, 0.3, 0.95, 1, 0)) return (evs_hostcache *)nullptr;
            evs_hostcache_set_backing(c, ptrs.data(), n_rows.data());
            return c;
        };
        const int B = 50;
        std::vector<int32_t> rows((size_t)B * T);
        std::vector<float> out((size_t)B * T * d), out2(out.size());
        std::vector<uint8_t> hit((size_t)B * T), hit2(hit.size());
        auto draw = [&]() { for (int b = 0; b < B; b++) for (int k = 0; k < T; k++) rows[(size_t)b * T + k] = (int32_t)((rng() % 3 ? rng() % 40 : rng()) % n_rows[k]); };
        evs_hostcache *a = make(cap);
        CHECK(a);
        const int pre = (int)(rng() % 12);   // 0: an empty export
        for (int rep = 0; rep < pre; rep++) { draw(); CHECK(evs_hostcache_request(a, B, rows.data(), out.data(), hit.data(), -1) == 0); }
        const int64_t n = evs_hostcache_export(a, nullptr, 0, nullptr);
        CHECK(n >= 0 && n <= cap);
        std::vector<int64_t> entries((size_t)n * 3 + 3), again(entries.size()), state(20), state2(20);
        CHECK(evs_hostcache_export(a, entries.data(), n, state.data()) == n);
        CHECK(evs_exact_load_check(policy, cap, T, n_rows.data(), n, entries.data(), state.data(), 1, 0) == 0);
        evs_hostcache *b = make(cap), *big = make(cap + 57);
        CHECK(b && big);
        CHECK(evs_hostcache_load(b, n, entries.data(), state.data(), 1) == 0);
        CHECK(evs_hostcache_load(big, n, entries.data(), nullptr, 0) == 0);
        CHECK(evs_hostcache_export(b, again.data(), n, state2.data()) == n && again == entries && state2 == state);
        CHECK(evs_hostcache_export(big, again.data(), n, nullptr) == n && again == entries);
        CHECK(evs_hostcache_load(b, n, entries.data(), state.data(), 1) == EVS_ESTATE);   // no longer fresh
        for (int rep = 0; rep < 40; rep++) {   // 2 000 requests, exporter and twin side by side
            draw();
            CHECK(evs_hostcache_request(a, B, rows.data(), out.data(), hit.data(), -1) == 0);
            CHECK(evs_hostcache_request(b, B, rows.data(), out2.data(), hit2.data(), -1) == 0);
            CHECK(hit == hit2 && memcmp(out.data(), out2.data(), out.size() * sizeof(float)) == 0);
            CHECK(evs_hostcache_request(big, B, rows.data(), out2.data(), hit2.data(), -1) == 0);
            total += 3 * B;
        }
        int64_t s1[8], s2[8];
        CHECK(evs_hostcache_stats(a, s1) == 0 && evs_hostcache_stats(b, s2) == 0 && memcmp(s1, s2, sizeof s1) == 0);
        const int64_t m = evs_hostcache_export(b, nullptr, 0, nullptr);
        std::vector<int64_t> ea((size_t)m * 3 + 3), eb(ea.size());
        CHECK(evs_hostcache_export(a, ea.data(), m, state.data()) == m && evs_hostcache_export(b, eb.data(), m, state2.data()) == m && ea == eb && state == state2);
        // states that must be refused, each into a fresh cache that must stay fresh
        if (m >= 2) {
            evs_hostcache *f = make(cap);
            CHECK(f);
            std::vector<int64_t> bad = ea;
            bad[4] = T + 1;                                        // a table outside 1 .. n_tables
            CHECK(evs_hostcache_load(f, m, bad.data(), state.data(), 1) == EVS_EINVAL);
            bad = ea; bad[5] = n_rows[bad[4] - 1];                 // a row outside its table
            CHECK(evs_hostcache_load(f, m, bad.data(), state.data(), 1) == EVS_EINVAL);
            bad = ea; bad[4] = bad[1]; bad[5] = bad[2];            // a duplicate key
            CHECK(evs_hostcache_load(f, m, bad.data(), state.data(), 1) == EVS_EINVAL);
            bad = ea; bad[0] = bad[3 * (m - 1)] + 1;               // scores that go down (or leave the range)
            CHECK(evs_hostcache_load(f, m, bad.data(), state.data(), 1) == EVS_EINVAL);
            std::vector<int64_t> st3 = state; st3[0] = 1;          // the batched tier's version
            CHECK(evs_hostcache_load(f, m, ea.data(), st3.data(), 1) == EVS_EINVAL);
            CHECK(evs_hostcache_load(f, m, ea.data(), nullptr, 1) == EVS_EINVAL);
            refused += 6;
            CHECK(evs_hostcache_load(f, m, ea.data(), state.data(), 1) == 0);   // ... and it has
            evs_hostcache_destroy(f);
        }
        evs_hostcache_destroy(a); evs_hostcache_destroy(b); evs_hostcache_destroy(big);
    }
    printf("exact warm start sanitizer run ok: %ld requests, %ld refusals\n", total, refused);
    return 0;
}
