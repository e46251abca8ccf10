// lds_layout_check.cpp -- csrc/lds_layout.hpp as k_lds_two_opt and lds_bytes_needed include it, built with the host compiler and
// run by tests/test_cpu_lds_layout.py (and, for the `max` form, by tests/test_gpu_lds_variants.py).
//   lds_layout_check [n_lo n_hi]     for every n in n_lo .. n_hi (default 3 .. 8200) and both edge-cache flags: the regions
//                                    rows | coord | order | pos | (dsp) | scratch | rowsf in this order without overlap, each
//                                    aligned for the widest type the kernel reads it as, every pad the smallest that aligns
//                                    (0 .. 15 bytes), the last byte used the total's last, the total non-decreasing in n and not
//                                    smaller with the cache than without.  Prints every 500th n as
//                                      n cache rows coord order pos dsp scratch rowsf total
//   lds_layout_check max BYTES       prints "max <largest n without the cache> <largest n with it>" for an LDS of BYTES, each
//                                    confirmed by the totals of n and n + 1.
// Exit status 1 and a line "MISMATCH ..." when anything differs; the last line of the first form is "cases <count>".
#include "lds_layout.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {
struct Region { const char *name; size_t at, bytes, align; };

int fail(const char *what, int n, int cache, size_t a, size_t b) {
    std::printf("MISMATCH %s n %d cache %d: %zu %zu\n", what, n, cache, a, b);
    return 1;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && !std::strcmp(argv[1], "max")) {
        const size_t bytes = (size_t)std::atoll(argv[2]);
        int out[2];
        for (int cache = 0; cache < 2; ++cache) {
            const int m = tsp::lds_layout_max_n(bytes, cache != 0);
            if (m > 0 && tsp::lds_layout(m, cache != 0).total > bytes) return fail("max fits", m, cache, tsp::lds_layout(m, cache != 0).total, bytes);
            if (tsp::lds_layout(m + 1, cache != 0).total <= bytes) return fail("max is the largest", m, cache, tsp::lds_layout(m + 1, cache != 0).total, bytes);
            out[cache] = m;
        }
        std::printf("max %d %d\n", out[0], out[1]);
        return 0;
    }
    const int n_lo = argc > 2 ? std::atoi(argv[1]) : 3, n_hi = argc > 2 ? std::atoi(argv[2]) : 8200;
    if (n_lo < 1 || n_hi < n_lo) return 2;
    long long cases = 0;
    int bad = 0;
    size_t prev_total[2] = {0, 0};
    for (int n = n_lo; n <= n_hi; ++n) {
        size_t total[2];
        for (int cache = 0; cache < 2; ++cache, ++cases) {
            const tsp::LdsLayout l = tsp::lds_layout(n, cache != 0);
            const size_t un = (size_t)n;
            // what the kernel reads each region as: row records, double2, int4 votes and float4 in 16-byte words; uint16; float
            const Region r[7] = {{"rows", l.rows, 48 * 32, 16},    {"coord", l.coord, 16 * un, 16},
                                 {"order", l.order, 2 * un, 2},    {"pos", l.pos, 2 * un, 2},
                                 {"dsp", l.dsp, cache ? 4 * un : 0, 16},
                                 {"scratch", l.scratch, 1024, 16}, {"rowsf", l.rowsf, 16 * 32, 16}};
            size_t end = 0;
            for (int k = 0; k < 7; ++k) {
                if (r[k].at % r[k].align) bad |= fail(r[k].name, n, cache, r[k].at, r[k].align);
                if (r[k].at < end) bad |= fail("overlap before", n, cache, r[k].at, end);
                // the smallest pad that aligns: the region starts at the first multiple of its alignment behind the one before
                if (r[k].at != (end + r[k].align - 1) / r[k].align * r[k].align) bad |= fail("pad before", n, cache, r[k].at, end);
                end = r[k].at + r[k].bytes;
            }
            if (end != l.total) bad |= fail("total", n, cache, end, l.total);
            if (!cache && l.dsp != l.scratch) bad |= fail("no cache, no dsp", n, cache, l.dsp, l.scratch);
            if (l.total < prev_total[cache]) bad |= fail("monotone", n, cache, l.total, prev_total[cache]);
            prev_total[cache] = total[cache] = l.total;
            if (n % 500 == 0 || n == n_lo || n == n_hi)
                std::printf("%d %d %zu %zu %zu %zu %zu %zu %zu %zu\n", n, cache, l.rows, l.coord, l.order, l.pos, l.dsp, l.scratch, l.rowsf, l.total);
        }
        if (total[1] < total[0] + 4 * (size_t)n) bad |= fail("cache adds the edge lengths", n, 1, total[1], total[0]);
    }
    std::printf("cases %lld\n", cases);
    return bad;
}
