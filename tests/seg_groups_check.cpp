// seg_groups_check.cpp -- csrc/seg_groups.hpp as k_seg_commit includes it, built with the host compiler and run by
// tests/test_cpu_seg_groups.py.  Arguments: the window W (default 9) and the stride of the printed sample (default 997).
// For G = 1 .. 4 every placement of the G groups is enumerated: a group offers nothing or one of the intervals 1 <= lo <= hi <=
// W - 2 with gain -1 or -2, so equal gains occur.  A group without an offer carries lo = 1, hi = W - 2, gain = -100: values that
// would win everything if they were read.  segg_commits is compared with the rule stated by brute force: the changed edges of an
// offer as a bit set (slots lo - 1 .. hi), a conflict as two sets that share a bit, the order as the pair (gain, g).  Also
// checked: the committed sets are pairwise disjoint, and the least (gain, g) among the offers commits.  Every `stride`-th case
// is printed as
//   G  offer lo hi gain (G times)  :  commit (G times)
// Exit status 1 and a line "MISMATCH ..." when anything differs; the last line is "cases <count>".
#include "seg_groups.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    const int W = argc > 1 ? std::atoi(argv[1]) : 9;
    const long long stride = argc > 2 ? std::atoll(argv[2]) : 997;
    if (W < 9 || W > 30 || stride < 1) return 2;
    std::vector<tsp::SegOffer> states;
    states.push_back(tsp::SegOffer{0, 1, W - 2, -100.0});
    for (int lo = 1; lo <= W - 2; ++lo)
        for (int hi = lo; hi <= W - 2; ++hi)
            for (int q = 1; q <= 2; ++q) states.push_back(tsp::SegOffer{1, lo, hi, -(double)q});
    const long long ns = (long long)states.size();
    long long cases = 0;
    int bad = 0;
    for (int G = 1; G <= 4; ++G) {
        long long total = 1;
        for (int g = 0; g < G; ++g) total *= ns;
        for (long long c = 0; c < total; ++c, ++cases) {
            tsp::SegOffer o[4];
            unsigned edges[4];
            long long r = c;
            for (int g = 0; g < G; ++g) {
                o[g] = states[(size_t)(r % ns)];
                r /= ns;
                edges[g] = 0;
                for (int k = o[g].lo - 1; k <= o[g].hi; ++k) edges[g] |= 1u << k;
            }
            int got[4], want[4], best = -1;
            bool same = true;
            for (int g = 0; g < G; ++g) {
                got[g] = tsp::segg_commits(o, G, g) ? 1 : 0;
                want[g] = o[g].offer;
                for (int h = 0; h < G && want[g]; ++h) {
                    if (h == g || !o[h].offer || !(edges[g] & edges[h])) continue;
                    if (o[h].gain < o[g].gain || (o[h].gain == o[g].gain && h < g)) want[g] = 0;
                }
                same = same && got[g] == want[g];
                if (o[g].offer && (best < 0 || o[g].gain < o[best].gain)) best = g;   // the first of the least gain
            }
            if (best >= 0) same = same && got[best] == 1;
            for (int g = 0; g < G; ++g)
                for (int h = g + 1; h < G; ++h) {
                    if (got[g] && got[h]) same = same && !(edges[g] & edges[h]);
                    if (o[g].offer && o[h].offer)
                        same = same && tsp::segg_conflict(o[g].lo, o[g].hi, o[h].lo, o[h].hi) == ((edges[g] & edges[h]) != 0);
                }
            if (cases % stride == 0 || !same) {
                std::printf("%d ", G);
                for (int g = 0; g < G; ++g) std::printf(" %d %d %d %g", o[g].offer, o[g].lo, o[g].hi, o[g].gain);
                std::printf("  :");
                for (int g = 0; g < G; ++g) std::printf(" %d", got[g]);
                std::printf("\n");
            }
            if (!same) { std::printf("MISMATCH case %lld of G = %d\n", c, G); bad = 1; }
        }
    }
    std::printf("cases %lld\n", cases);
    return bad;
}
