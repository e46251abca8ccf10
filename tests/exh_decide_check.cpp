// Host driver for tests/test_cpu_exh_decide.py: compiles csrc/exh_decide.hpp -- the very text k_move_pos and k_exh_close decide an
// exhaustive sweep's move with -- and checks, for every case on standard input,
//   D nslots n pool seed   the decision over `nslots` candidate slots dealt to 256 simulated threads (slot s to thread s mod 256, as
//                          exh_cand_load deals them), against a brute-force arg-min of (delta, (min id, max id)) over the slots;
//                          the tour has n positions and a random permutation as its ids, the slots draw from `pool` different
//                          pairs (each with ONE delta out of three values, so ties are the norm, and the same pair may fill
//                          several slots) or are empty
//                          answer: bad_pair bad_orient bad_L bad_flag found ambiguous p_first repeated
//   P mode n seed          for every pair of positions p < q with 2 <= q - p <= n - 2: the records of the next sweep, taken as
//                          k_move_pos<HOT> takes them -- exh_perm for both orientations, the one kept in which pa is the position
//                          of the smaller id -- against records built from scratch from the tour the reference's move leaves
//                          answer: mismatches moves p_first_moves q_first_moves
// The block-wide steps (arg-min, OR) are plain loops over the simulated threads here; everything a thread does is the header's.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "exh_decide.hpp"

using namespace tsp;
typedef unsigned long long u64;
typedef long long i64;

static const int kThreads = 256;
static const int kPads = 9;

struct Rng {
    u64 s;
    explicit Rng(u64 seed) : s(seed * 0x9E3779B97F4A7C15ull + 88172645463325252ull) {}
    u64 next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    int below(int m) { return (int)(next() % (u64)m); }
};

static void shuffle(std::vector<int> &v, Rng &r) {
    for (int k = (int)v.size() - 1; k > 0; --k) std::swap(v[(size_t)k], v[(size_t)r.below(k + 1)]);
}

// ---- D: the decision --------------------------------------------------------------------------------------------------------
static int decide_case(int nslots, int n, int pool, u64 seed) {
    Rng rng(seed);
    std::vector<int> id((size_t)n);
    for (int v = 0; v < n; ++v) id[(size_t)v] = v;
    shuffle(id, rng);
    // the pool: different pairs of positions p < q, one delta each out of {-7, -4, -1}
    std::vector<ExhCand> pairs;
    while ((int)pairs.size() < pool) {
        int p = rng.below(n), q = rng.below(n);
        if (p == q) continue;
        if (p > q) std::swap(p, q);
        bool seen = false;
        for (const ExhCand &c : pairs) seen = seen || (c.p == p && c.q == q);
        if (seen) continue;
        static const int kDelta[3] = {-7, -4, -1};
        pairs.push_back(ExhCand{kDelta[rng.below(3)], p, q, 0});
    }
    std::vector<ExhCand> slot((size_t)nslots);
    for (ExhCand &c : slot) {
        if (rng.below(4) == 0) c = ExhCand{rng.below(3) - 9, -1, -1, 0};   // empty: whatever its delta says
        else c = pairs[(size_t)rng.below(pool)];
    }
    // brute force: arg-min of (delta, (min id, max id)); how many DIFFERENT pairs hold the minimal delta; repeated pairs
    int want_found = 0, want_delta = 0, want_p = -1, want_q = -1;
    u64 want_key = kExhNoPair;
    for (const ExhCand &c : slot) {
        if (c.p < 0) continue;
        const int i = id[(size_t)c.p], j = id[(size_t)c.q];
        const u64 k = ((u64)(unsigned)(i < j ? i : j) << 32) | (unsigned)(i < j ? j : i);
        if (!want_found || c.delta < want_delta || (c.delta == want_delta && k < want_key)) {
            want_found = 1; want_delta = c.delta; want_key = k; want_p = c.p; want_q = c.q;
        }
    }
    int at_min = 0, repeated = 0;
    for (const ExhCand &c : pairs) {
        int uses = 0;
        for (const ExhCand &s : slot) uses += s.p == c.p && s.q == c.q;
        if (uses > 0 && want_found && c.delta == want_delta) ++at_min;
        if (uses > 1 && want_found && c.delta == want_delta) repeated = 1;
    }
    // the header's rule, thread by thread
    std::vector<ExhBest> best((size_t)kThreads);
    for (int s = 0; s < nslots; ++s) exh_fold(best[(size_t)(s % kThreads)], slot[(size_t)s]);
    int found = 0, delta = 0;
    u64 key = kExhNoPair;
    for (const ExhBest &b : best)
        if (b.key != kExhNoPair && (!found || b.delta < delta || (b.delta == delta && b.key < key))) { found = 1; delta = b.delta; key = b.key; }
    int ambiguous = 0;
    if (found) {
        for (const ExhBest &b : best) ambiguous |= exh_ambiguous(b, delta, key) ? 1 : 0;
        if (ambiguous) {
            std::vector<ExhIdBest> ib((size_t)kThreads);
            for (int s = 0; s < nslots; ++s)
                exh_fold_ids(ib[(size_t)(s % kThreads)], slot[(size_t)s], delta, [&](int p) { return id[(size_t)p]; });
            u64 idkey = kExhNoPair;
            for (const ExhIdBest &b : ib) if (b.idkey < idkey) { idkey = b.idkey; key = b.poskey; }
        }
    }
    int bad_pair = found != want_found, bad_orient = 0, bad_L = 0, p_first = 0;
    if (found && want_found) {
        const int p = exh_key_hi(key), q = exh_key_lo(key);
        bad_pair = p != want_p || q != want_q || !(p < q);
        if (!bad_pair) {
            p_first = id[(size_t)p] < id[(size_t)q];
            const ExhMove m = exh_orient(p, q, n, p_first != 0);
            // the reference: i < j the ids, pa = pos[i], pb = pos[j], positions pa + 1 .. pb (cyclic) reversed
            const int pa = p_first ? p : q, pb = p_first ? q : p;
            bad_orient = m.pa != pa || m.pb != pb || m.pa1 != (pa + 1) % n;
            bad_L = m.L != ((pb - pa) % n + n) % n;
        }
    }
    const int bad_flag = found && ambiguous != (at_min >= 2);
    printf("%d %d %d %d %d %d %d %d\n", bad_pair, bad_orient, bad_L, bad_flag, found, ambiguous, p_first, repeated);
    return 0;
}

// ---- P: the records behind the orientation -------------------------------------------------------------------------------------
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

// the records of a tour as tests/exh_permute_check.cpp builds them (k_move_pos's cold path): nothing of the rule in them
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

static int permute_case(int mode, int n, u64 seed) {
    Rng rng(seed);
    std::vector<i64> x((size_t)n), y((size_t)n);
    std::vector<int> order((size_t)n), order2;
    for (int v = 0; v < n; ++v) { x[(size_t)v] = rng.below(1000000); y[(size_t)v] = rng.below(1000000); order[(size_t)v] = v; }
    shuffle(order, rng);
    std::vector<ExhRec> old, want;
    from_scratch(mode, x, y, order, old);
    i64 bad = 0, moves = 0, p_firsts = 0;
    for (int p = 0; p < n; ++p)
        for (int q = p + 2; q < n && q - p <= n - 2; ++q) {
            // the reference's move: i < j the ids of the pair, positions pos[i] + 1 .. pos[j] (cyclic) reversed, by swaps
            const bool id_p_first = order[(size_t)p] < order[(size_t)q];
            const int pa = id_p_first ? p : q, pb = id_p_first ? q : p, L = ((pb - pa) % n + n) % n;
            order2 = order;
            for (int t = 0; t < L / 2; ++t) std::swap(order2[(size_t)((pa + 1 + t) % n)], order2[(size_t)((pb - t + n) % n)]);
            from_scratch(mode, x, y, order2, want);
            // k_move_pos<HOT>: both orientations evaluated, the one kept that the ids IN THE OLD RECORDS name
            const ExhMove m1 = exh_orient(p, q, n, true), m2 = exh_orient(p, q, n, false);
            const bool p_first = old[(size_t)p].id < old[(size_t)q].id;
            for (int k = 0; k < n + kPads; ++k) {
                const ExhPerm pm1 = exh_perm(k, n, m1.pa1, m1.L), pm2 = exh_perm(k, n, m2.pa1, m2.L);
                const ExhPerm pm = p_first ? pm1 : pm2;
                const ExhRec got = mode == EXH_NINT ? permuted<EXH_NINT>(pm, old, n)
                                                    : (mode == EXH_CEIL ? permuted<EXH_CEIL>(pm, old, n) : permuted<EXH_ATT>(pm, old, n));
                const ExhRec &w = want[(size_t)k];
                if (memcmp(&got.m2x, &w.m2x, 8) || memcmp(&got.m2y, &w.m2y, 8) || memcmp(&got.nrm, &w.nrm, 8) || got.eprev != w.eprev ||
                    got.id != w.id)
                    ++bad;
            }
            ++moves;
            p_firsts += p_first;
        }
    printf("%lld %lld %lld %lld\n", bad, moves, p_firsts, moves - p_firsts);
    return 0;
}

int main() {
    static_assert(sizeof(ExhCand) == 16 && alignof(ExhCand) == 16, "one candidate is one aligned 16-byte store");
    char kind;
    while (scanf(" %c", &kind) == 1) {
        if (kind == 'D') {
            int nslots, n, pool;
            u64 seed;
            if (scanf("%d %d %d %llu", &nslots, &n, &pool, &seed) != 4 || nslots < 1 || nslots > 8192 || n < 5 || pool < 1 ||
                (i64)pool > (i64)n * (n - 1) / 2) {
                fprintf(stderr, "exh_decide_check: bad case\n");
                return 2;
            }
            decide_case(nslots, n, pool, seed);
        } else if (kind == 'P') {
            int mode, n;
            u64 seed;
            if (scanf("%d %d %llu", &mode, &n, &seed) != 3 || mode < 0 || mode > 2 || n < 5 || n > 4096) {
                fprintf(stderr, "exh_decide_check: bad case\n");
                return 2;
            }
            permute_case(mode, n, seed);
        } else {
            fprintf(stderr, "exh_decide_check: bad case\n");
            return 2;
        }
    }
    return 0;
}
