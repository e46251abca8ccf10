// Host driver for tests/test_cpu_exh_permute.py: compiles csrc/exh_arith.hpp -- the very text k_move_pos permutes the previous
// sweep's records with (exh_perm, exh_perm_rec) -- and compares, for every case on standard input, the records permuted from the
// old tour's records with records built from scratch from the reversed tour, field for field and bit for bit.
//   case   = mode n pa pb hi seed       (the move reverses positions pa + 1 .. pb, cyclic; coordinates are integers in [0, hi))
//   answer = one line: mismatches zero fwd bwd wrap_fwd wrap_bwd cut_lo cut_hi pads
// The records from scratch use nothing of the header but exh_rec_xy: the reversal is done by swaps (no mirror), the edge lengths
// come from an integer square root.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "exh_arith.hpp"

using namespace tsp;
typedef unsigned long long u64;
typedef long long i64;

static const int kPads = 9;   // positions past n (k_move_pos: kExhPad of them)

static u64 isqrt_u64(u64 s) {   // floor(sqrt(s)), integers only
    u64 lo = 0, hi = 1ull << 32;
    while (lo + 1 < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (mid * mid <= s) lo = mid; else hi = mid;
    }
    return lo;
}

static int ref_dist(int mode, i64 ax, i64 ay, i64 bx, i64 by) {
    const u64 s = (u64)((ax - bx) * (ax - bx) + (ay - by) * (ay - by));
    if (mode == EXH_NINT) { const u64 k = isqrt_u64(s); return (int)(s > k * k + k ? k + 1 : k); }   // nint(sqrt s)
    if (mode == EXH_CEIL) { const u64 k = isqrt_u64(s); return (int)(k * k == s ? k : k + 1); }       // ceil(sqrt s)
    u64 k = isqrt_u64(s / 10);                                                                        // smallest k: 10 k^2 >= s
    while (10 * k * k < s) ++k;
    return (int)k;
}

// what k_move_pos's cold path writes for a tour: position p < n the record of order[p] relative to node 0 with the length of
// the edge that ends there (0 at position 0), position n repeats position 0 with the closing edge, then the pads
static void from_scratch(int mode, const std::vector<i64> &x, const std::vector<i64> &y, const std::vector<int> &order,
                         std::vector<ExhRec> &rec) {
    const int n = (int)order.size();
    rec.resize((size_t)n + kPads);
    for (int k = 0; k < n + kPads; ++k) {
        ExhRec r;
        const int u = k < n ? order[(size_t)k] : (k == n ? order[0] : -1);
        const int v = k >= 1 && k <= n ? order[(size_t)k - 1] : -1;
        if (u >= 0) exh_rec_xy((double)(x[(size_t)u] - x[0]), (double)(y[(size_t)u] - y[0]), r);
        else exh_rec_xy(-6.0e6, -6.0e6, r);
        r.eprev = v >= 0 ? ref_dist(mode, x[(size_t)v], y[(size_t)v], x[(size_t)u], y[(size_t)u]) : 0;
        r.id = u;
        rec[(size_t)k] = r;
    }
}

template <int MODE>
static ExhRec permuted(const ExhPerm &pm, const std::vector<ExhRec> &old, int n) {
    return exh_perm_rec<MODE>(pm, old[(size_t)pm.a], old[(size_t)pm.b], old[(size_t)n].eprev, [](double v) { return std::sqrt(v); });
}

int main() {
    static_assert(sizeof(ExhRec) == 32 && alignof(ExhRec) == 32, "one row record is one aligned 32-byte load");
    int mode, n, pa, pb, hi;
    u64 seed;
    std::vector<i64> x, y;
    std::vector<int> order, order2;
    std::vector<ExhRec> old, want;
    while (scanf("%d %d %d %d %d %llu", &mode, &n, &pa, &pb, &hi, &seed) == 6) {
        const int L = ((pb - pa) % n + n) % n;
        if (mode < 0 || mode > 2 || n < 5 || pa < 0 || pa >= n || pb < 0 || pb >= n || L < 2 || hi < 2 || hi > 1000000) {
            fprintf(stderr, "exh_permute_check: bad case\n");
            return 2;
        }
        u64 s = seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull;
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
        x.resize((size_t)n); y.resize((size_t)n); order.resize((size_t)n);
        for (int v = 0; v < n; ++v) { x[(size_t)v] = (i64)(rnd() % (u64)hi); y[(size_t)v] = (i64)(rnd() % (u64)hi); order[(size_t)v] = v; }
        for (int v = n - 1; v > 0; --v) std::swap(order[(size_t)v], order[(size_t)(rnd() % (u64)(v + 1))]);
        from_scratch(mode, x, y, order, old);
        order2 = order;
        for (int t = 0; t < L / 2; ++t) std::swap(order2[(size_t)((pa + 1 + t) % n)], order2[(size_t)((pb - t + n) % n)]);
        from_scratch(mode, x, y, order2, want);
        const int pa1 = pa + 1 == n ? 0 : pa + 1;
        long long bad = 0, cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // zero fwd bwd wrap_fwd wrap_bwd cut_lo cut_hi pads
        for (int k = 0; k < n + kPads; ++k) {
            const ExhPerm pm = exh_perm(k, n, pa1, L);
            if (pm.a < 0 || pm.a >= n + kPads || pm.b < 0 || pm.b >= n + kPads) { fprintf(stderr, "exh_permute_check: index out of range\n"); return 3; }
            const ExhRec got = mode == EXH_NINT ? permuted<EXH_NINT>(pm, old, n)
                                                : (mode == EXH_CEIL ? permuted<EXH_CEIL>(pm, old, n) : permuted<EXH_ATT>(pm, old, n));
            const ExhRec &w = want[(size_t)k];
            // field for field, bit for bit (the record has no padding bytes: 3 x 8 + 2 x 4 = 32)
            if (memcmp(&got.m2x, &w.m2x, 8) || memcmp(&got.m2y, &w.m2y, 8) || memcmp(&got.nrm, &w.nrm, 8) || got.eprev != w.eprev ||
                got.id != w.id)
                ++bad;
            if (k > n) ++cnt[7];
            else if (pm.e == EXH_E_ZERO) ++cnt[0];
            else if (pm.e == EXH_E_B) ++cnt[1];
            else if (pm.e == EXH_E_A) ++cnt[2];
            else if (pm.e == EXH_E_WRAP) ++cnt[pm.b == 0 ? 3 : 4];
            else if (pm.e == EXH_E_CUT) ++cnt[(k == n ? 0 : k) == pa1 ? 5 : 6];
        }
        printf("%lld", bad);
        for (int q = 0; q < 8; ++q) printf(" %lld", cnt[q]);
        printf("\n");
    }
    return 0;
}
