// gpx_stretch_check.cpp -- drives tsp_optimization_amd/csrc/gpx_stretch.hpp (the text the kernels of gpx.hip compile) against
// naive loops: every cyclic interval of n <= 12 positions read in both directions, and the chunked nearest-boundary scan for
// every flag pattern of n <= 12 under several chunk counts.  Prints the number of checks and "ok"; exits 1 at the first mismatch.
// tests/test_cpu_gpx.py builds it with the host compiler, once plain and once under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gpx_stretch.hpp"

using namespace tsp;

static long long g_checks = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        ++g_checks;                                                                  \
        if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

static void intervals(int n) {
    for (int first = 0; first < n; ++first)
        for (int last = 0; last < n; ++last) {
            // the interval, by walking it
            std::vector<int> seq;
            for (int p = first;; p = (p + 1) % n) { seq.push_back(p); if (p == last) break; }
            const int len = (int)seq.size();
            CHECK(gpx_cyc_len(first, last, n) == len);
            std::vector<char> in((size_t)n, 0);
            for (int k = 0; k < len; ++k) {
                in[(size_t)seq[(size_t)k]] = 1;
                CHECK(gpx_cyc_off(first, seq[(size_t)k], n) == k);
                CHECK(gpx_read_pos(first, last, k, false, n) == seq[(size_t)k]);
                CHECK(gpx_read_pos(first, last, k, true, n) == seq[(size_t)(len - 1 - k)]);
                CHECK(gpx_read_off(first, last, seq[(size_t)k], false, n) == k);
                CHECK(gpx_read_off(first, last, seq[(size_t)k], true, n) == len - 1 - k);
            }
            for (int p = 0; p < n; ++p) CHECK(gpx_cyc_has(first, last, p, n) == (in[(size_t)p] != 0));
            // a child piece written from such reads holds the interval's positions in order, forwards and backwards
            for (int back = 0; back < 2; ++back) {
                std::vector<int> piece((size_t)len, -1);
                for (int k = 0; k < len; ++k) {
                    const int p = seq[(size_t)k];
                    piece[(size_t)gpx_read_off(first, last, p, back != 0, n)] = p;
                }
                for (int k = 0; k < len; ++k) CHECK(piece[(size_t)k] == gpx_read_pos(first, last, k, back != 0, n));
            }
        }
    for (int p = 0; p < n; ++p) {
        CHECK(gpx_next(p, n) == (p + 1) % n);
        CHECK(gpx_prev(p, n) == (p + n - 1) % n);
    }
}

static void scans(int n) {
    for (unsigned mask = 0; mask < (1u << n); ++mask) {
        auto flag = [&](int p) { return ((mask >> p) & 1u) != 0; };
        std::vector<int> want_l((size_t)n, -1), want_r((size_t)n, -1);
        for (int p = 0; p < n; ++p)
            for (int k = 0; k < n; ++k) {
                if (want_l[(size_t)p] < 0 && flag((p - k + n) % n)) want_l[(size_t)p] = (p - k + n) % n;
                if (want_r[(size_t)p] < 0 && flag((p + k) % n)) want_r[(size_t)p] = (p + k) % n;
            }
        for (int threads : {1, 2, 3, 5, 16}) {
            const int CH = gpx_chunk_size(n, threads);
            std::vector<int> last((size_t)threads), first((size_t)threads);
            auto lo_of = [&](int t) { return t * CH < n ? t * CH : n; };
            auto hi_of = [&](int t) { return lo_of(t) + CH < n ? lo_of(t) + CH : n; };
            for (int t = 0; t < threads; ++t) gpx_chunk_ends(flag, lo_of(t), hi_of(t), &last[(size_t)t], &first[(size_t)t]);
            int all_first = -1, all_last = -1;
            for (int t = 0; t < threads; ++t) {
                if (all_first < 0) all_first = first[(size_t)t];
                if (last[(size_t)t] >= 0) all_last = last[(size_t)t];
            }
            // left and right live in vectors of exactly n: the sanitizer sees any step outside a chunk
            std::vector<int> left((size_t)n, -7), right((size_t)n, -7);
            for (int t = 0; t < threads; ++t) {
                int cl = -1, cr = -1;
                for (int u = 0; u < t; ++u)
                    if (last[(size_t)u] >= 0) cl = last[(size_t)u];
                for (int u = threads - 1; u > t; --u)
                    if (first[(size_t)u] >= 0) cr = first[(size_t)u];
                gpx_chunk_fill(flag, lo_of(t), hi_of(t), cl, cr, all_first, all_last, left.data(), right.data());
            }
            for (int p = 0; p < n; ++p) {
                CHECK(left[(size_t)p] == want_l[(size_t)p]);
                CHECK(right[(size_t)p] == want_r[(size_t)p]);
            }
        }
    }
}

int main() {
    for (int n = 1; n <= 12; ++n) intervals(n);
    for (int n = 1; n <= 12; ++n) scans(n);
    printf("%lld checks ok\n", g_checks);
    return 0;
}
