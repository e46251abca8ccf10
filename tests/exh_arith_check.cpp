// Host driver for tests/test_cpu_exh_arith.py: compiles csrc/exh_arith.hpp -- the very text k_move_pos and k_exh compile for the
// device -- and compares it with integer arithmetic.
//   exh_arith_check sweep          roots: prints "roots cases=<n> mismatches=<m>" (+ the first mismatches)
//   exh_arith_check norms          norm form of s: prints "norms cases=<n> mismatches=<m>"
//   exh_arith_check strips         exh_strip / exh_total_rows: prints "strips sizes=<n> pairs=<n> uncovered=<m> bad_totals=<m> total10000=<t>"
//   exh_arith_check sample <step>  every <step>-th root case as "mode s delta_index got", for a second opinion from math.isqrt
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "exh_arith.hpp"

using namespace tsp;
typedef unsigned long long u64;
typedef long long i64;

static u64 isqrt_u64(u64 s) {   // floor(sqrt(s)), integers only
    u64 lo = 0, hi = 1ull << 32;
    while (lo + 1 < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (mid * mid <= s) lo = mid; else hi = mid;
    }
    return lo;
}

static i64 ref_root(int mode, u64 s) {
    if (mode == EXH_NINT) { const u64 k = isqrt_u64(s); return (i64)(s > k * k + k ? k + 1 : k); }   // nint(sqrt s)
    if (mode == EXH_CEIL) { const u64 k = isqrt_u64(s); return (i64)(k * k == s ? k : k + 1); }       // ceil(sqrt s)
    u64 k = isqrt_u64(s / 10);                                                                        // smallest k: 10 k^2 >= s
    while (10 * k * k < s) ++k;
    return (i64)k;
}

static const double kDelta[5] = {0.0, 0x1p-25, -0x1p-25, 0x1p-23, -0x1p-23};
static const i64 kKMax = (1ll << 21) - 2;

template <int MODE>
static int got_root(u64 s, int di) {
    const double sd = (double)s;
    const double g = std::sqrt(exh_root_arg<MODE>(sd)) * (1.0 + kDelta[di]);
    return exh_round<MODE>(sd, g);
}

static int got_root_rt(int mode, u64 s, int di) {
    return mode == EXH_NINT ? got_root<EXH_NINT>(s, di) : (mode == EXH_CEIL ? got_root<EXH_CEIL>(s, di) : got_root<EXH_ATT>(s, di));
}

// the s values around k: on both sides of every rounding boundary of the three metrics
static int s_values(i64 k, i64 out[16]) {
    int m = 0;
    for (int d = -1; d <= 2; ++d) out[m++] = k * k + k + d;
    for (int d = -1; d <= 2; ++d) out[m++] = k * k + d;
    for (int d = -1; d <= 2; ++d) out[m++] = 10 * k * k + d;
    for (int d = -1; d <= 2; ++d) out[m++] = 10 * k * k + 5 * k + d;
    return m;
}

// the root (of s, of s / 10 for ATT) stays below 2^21: the domain the *_ICOORD metrics guarantee
static bool in_domain(int mode, i64 s) {
    if (s < 0) return false;
    const i64 lim = (kKMax + 1) * (kKMax + 1);
    return mode == EXH_ATT ? s <= 10 * lim : s <= lim;
}

template <class F>
static void for_each_k(F f) {
    const i64 dense = 1 << 15;
    for (i64 k = 0; k <= dense; ++k) f(k);
    u64 x = 88172645463325252ull;
    for (i64 k = dense + 1; k < kKMax - dense;) {   // sampled: steps of 1 .. 32 (about 1.2e5 values)
        f(k);
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        k += 1 + (i64)(x & 31);
    }
    for (i64 k = kKMax - dense; k <= kKMax; ++k) f(k);
}

static int run_roots(long sample_step) {
    u64 cases = 0, bad = 0, nk = 0;
    for_each_k([&](i64 k) {
        ++nk;
        i64 sv[16];
        const int m = s_values(k, sv);
        for (int mode = 0; mode < 3; ++mode)
            for (int i = 0; i < m; ++i) {
                if (!in_domain(mode, sv[i])) continue;
                const i64 want = ref_root(mode, (u64)sv[i]);
                for (int di = 0; di < 5; ++di) {
                    const int got = got_root_rt(mode, (u64)sv[i], di);
                    ++cases;
                    if (sample_step > 0) {
                        if (cases % (u64)sample_step == 0) printf("%d %lld %d %d\n", mode, sv[i], di, got);
                        continue;
                    }
                    if (got != want && bad++ < 20) printf("MISMATCH mode=%d s=%lld delta=%d got=%d want=%lld\n", mode, sv[i], di, got, want);
                }
            }
    });
    if (sample_step <= 0) printf("roots k_values=%llu cases=%llu mismatches=%llu\n", nk, cases, bad);
    return 0;
}

static int run_norms() {
    // translated integer coordinates of magnitude < 2^21 (any two instance positions), and the pad position against them
    u64 x = 0x9E3779B97F4A7C15ull, cases = 0, bad = 0;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    const i64 R = (1ll << 21) - 1;
    auto coord = [&](int edge) -> i64 {
        if (edge == 1) return R;
        if (edge == 2) return -R;
        return (i64)(rnd() % (u64)(2 * R + 1)) - R;
    };
    for (int it = 0; it < 2000000; ++it) {
        i64 ax = coord((int)(rnd() % 16)), ay = coord((int)(rnd() % 16)), bx = coord((int)(rnd() % 16)), by = coord((int)(rnd() % 16));
        if (it % 8 == 0) { bx = -6000000; by = -6000000; }   // the row is a pad
        if (it % 8 == 1) { ax = -6000000; ay = -6000000; }   // the column is a pad
        if (it % 64 == 2) { ax = bx = -6000000; ay = by = -6000000; }
        ExhRec c, r;
        exh_rec_xy((double)ax, (double)ay, c);
        exh_rec_xy((double)bx, (double)by, r);
        const double s = exh_s(exh_col(c.m2x), exh_col(c.m2y), c.nrm, r.m2x, r.m2y, r.nrm);
        const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by;
        const double s_old = dx * dx + dy * dy;
        const i64 s_int = (ax - bx) * (ax - bx) + (ay - by) * (ay - by);
        ++cases;
        const bool ok = s == s_old && s == (double)s_int && (i64)s == s_int && exh_col(c.m2x) == (double)ax && c.nrm == (double)(ax * ax + ay * ay);
        if (!ok && bad++ < 20) printf("MISMATCH a=(%lld,%lld) b=(%lld,%lld) s=%.17g old=%.17g int=%lld\n", ax, ay, bx, by, s, s_old, s_int);
    }
    printf("norms cases=%llu mismatches=%llu\n", cases, bad);
    return 0;
}

// The pairs k_exh evaluates, enumerated the way it walks them: strip s, rows p = 1 .. rows, D-columns q = q0 .. q0 + weff; the
// pair of (p, q) is (p - 1, q - 1), not evaluated for the strip's first column (no left neighbour) and masked unless q > p.
// Every pair p' < q' <= n - 1 must be met at least once, and more than once only where the clamped strip 0 overlaps strip 1.
static int run_strips() {
    const int weff = 255;
    const int sizes[] = {5, 6, 64, 254, 255, 256, 257, 300, 509, 510, 511, 512, 764, 765, 766, 1000, 1021, 1275, 1276, 2000};
    u64 pairs = 0, uncovered = 0, bad_totals = 0, nsizes = 0;
    for (int n : sizes) {
        ++nsizes;
        const int ns = exh_strips(n, weff);
        std::vector<unsigned char> seen((size_t)n * n, 0);
        long long total = 0, old_total = 0;
        for (int s = 0; s < ns; ++s) {
            const ExhStrip st = exh_strip(n, weff, s);
            total += st.rows;
            old_total += s * weff + weff - 1 < n - 1 ? s * weff + weff - 1 : n - 1;   // strips laid out from column 0
            if (st.q0 < 0 || st.rows < 0 || st.rows > n - 1 || st.q0 + weff > n + 1 + (ns == 1 ? weff : 0)) ++bad_totals;
            for (int p = 1; p <= st.rows; ++p)
                for (int q = st.q0 + 1; q <= st.q0 + weff; ++q)
                    if (q > p && q - 1 < n) {
                        unsigned char &c = seen[(size_t)(p - 1) * n + (q - 1)];
                        if (c && s > 1) ++bad_totals;   // only strips 0 and 1 may share a pair
                        c = 1;
                    }
        }
        if (total != exh_total_rows(n, weff) || total > old_total || (n <= weff && total != n - 1)) ++bad_totals;
        for (int a = 0; a + 1 < n; ++a)
            for (int b = a + 1; b < n; ++b) { ++pairs; if (!seen[(size_t)a * n + b]) ++uncovered; }
    }
    printf("strips sizes=%llu pairs=%llu uncovered=%llu bad_totals=%llu total10000=%lld\n", nsizes, pairs, uncovered, bad_totals,
           exh_total_rows(10000, weff));
    return 0;
}

int main(int argc, char **argv) {
    static_assert(sizeof(ExhRec) == 32 && alignof(ExhRec) == 32, "one row record is one aligned 32-byte load");
    if (argc >= 2 && !strcmp(argv[1], "sweep")) return run_roots(0);
    if (argc >= 2 && !strcmp(argv[1], "norms")) return run_norms();
    if (argc >= 2 && !strcmp(argv[1], "strips")) return run_strips();
    if (argc >= 3 && !strcmp(argv[1], "sample")) return run_roots(atol(argv[2]));
    fprintf(stderr, "usage: exh_arith_check sweep | norms | strips | sample <step>\n");
    return 2;
}
