// Host driver for tests/test_cpu_exh_seed.py: compiles the seed form of csrc/exh_arith.hpp -- the very text k_exh compiles for the
// device: the integer root from an fp32 seed under the one-sided fix-up in fp64 -- and compares it with integer arithmetic.
//   exh_seed_check sweep          roots below 2^21, the seed moved by 0, +-1 and +-2 fp32 ulps:
//                                 prints "seed k_values=<n> cases=<n> mismatches=<m>" (+ the first mismatches)
//   exh_seed_check beyond         roots in (2^21, 2.9e6], the seed moved by +-2 ulps -- past the form's domain, where it must fail:
//                                 prints "beyond k_values=<n> cases=<n> mismatches=<m>"
//   exh_seed_check sample <step>  every <step>-th case of the sweep as "mode s ulps got", for a second opinion from math.isqrt
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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

static const int kUlps[5] = {0, 1, -1, 2, -2};
static const i64 kKMax = (1ll << 21) - 2;
static const i64 kBeyondMax = 2900000;

// the seed: the correctly rounded fp32 root of the fp32 argument, moved by `ulps` representable values
template <int MODE>
static int got_root(u64 s, int ulps) {
    const double sd = (double)s;
    float g = std::sqrt(exh_seed_arg<MODE>(sd));
    for (int u = 0; u < (ulps < 0 ? -ulps : ulps); ++u) g = std::nextafterf(g, ulps < 0 ? -INFINITY : INFINITY);
    return exh_seed_round<MODE>(sd, g);
}

static int got_root_rt(int mode, u64 s, int ulps) {
    return mode == EXH_NINT ? got_root<EXH_NINT>(s, ulps) : (mode == EXH_CEIL ? got_root<EXH_CEIL>(s, ulps) : got_root<EXH_ATT>(s, ulps));
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

// the root (of s, of s / 10 for ATT) in [0, hi] and, where lo > 0, above lo
static bool in_range(int mode, i64 s, i64 lo, i64 hi) {
    if (s < 0) return false;
    const i64 f = mode == EXH_ATT ? 10 : 1;
    return s <= f * hi * hi && (lo == 0 || s > f * lo * lo);
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

static int run_sweep(long sample_step) {
    u64 cases = 0, bad = 0, nk = 0, zero = 0;
    for_each_k([&](i64 k) {
        ++nk;
        i64 sv[16];
        const int m = s_values(k, sv);
        for (int mode = 0; mode < 3; ++mode)
            for (int i = 0; i < m; ++i) {
                if (!in_range(mode, sv[i], 0, kKMax + 1)) continue;
                const i64 want = ref_root(mode, (u64)sv[i]);
                // s = 0 (two nodes on one point): the hardware's root of 0 is 0, nothing to move
                const int nd = sv[i] == 0 ? 1 : 5;
                zero += sv[i] == 0;
                for (int di = 0; di < nd; ++di) {
                    const int got = got_root_rt(mode, (u64)sv[i], kUlps[di]);
                    ++cases;
                    if (sample_step > 0) {
                        if (cases % (u64)sample_step == 0) printf("%d %lld %d %d\n", mode, sv[i], kUlps[di], got);
                        continue;
                    }
                    if (got != want && bad++ < 20) printf("MISMATCH mode=%d s=%lld ulps=%d got=%d want=%lld\n", mode, sv[i], kUlps[di], got, want);
                }
            }
    });
    if (sample_step <= 0) printf("seed k_values=%llu cases=%llu zero_cases=%llu mismatches=%llu\n", nk, cases, zero, bad);
    return 0;
}

static int run_beyond() {
    u64 cases = 0, bad = 0, nk = 0;
    for (i64 k = (1ll << 21) + 1; k <= kBeyondMax; k += 3) {
        ++nk;
        i64 sv[16];
        const int m = s_values(k, sv);
        for (int mode = 0; mode < 3; ++mode)
            for (int i = 0; i < m; ++i) {
                if (!in_range(mode, sv[i], 1ll << 21, kBeyondMax)) continue;
                const i64 want = ref_root(mode, (u64)sv[i]);
                for (int di = 3; di < 5; ++di) {
                    ++cases;
                    if (got_root_rt(mode, (u64)sv[i], kUlps[di]) != want) ++bad;
                }
            }
    }
    printf("beyond k_values=%llu cases=%llu mismatches=%llu\n", nk, cases, bad);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "sweep")) return run_sweep(0);
    if (argc >= 2 && !strcmp(argv[1], "beyond")) return run_beyond();
    if (argc >= 3 && !strcmp(argv[1], "sample")) return run_sweep(atol(argv[2]));
    fprintf(stderr, "usage: exh_seed_check sweep | beyond | sample <step>\n");
    return 2;
}
