// seg_move3_check.cpp -- csrc/seg_move3.hpp as k_seg_ils includes it, built with the host compiler and run by
// tests/test_cpu_seg_ils3.py.  Argument: the window W (default 9).  The tour is 0, 1, .., W + 1 in this order, the window its nodes
// 0 .. W - 1 (node = slot), W and W + 1 the outside.  For every 0 <= i < j < k <= W - 2, every r and every type one line
//   i j k r type form  src(i+1) .. src(k)
// from seg3_make / seg3_src, compared here with the definition: the move (a, b, c, type), a the tail at the r-th of the three
// slots and b, c behind it in tour order, applied by the table of include/tsp_hip.h (S2 S1, S1' S2', S2' S1, S2 S1', then S3) and
// the tour turned so that W + 1 comes before node 0 again.  Exit status 1 and a line "MISMATCH ..." when they differ.
#include "seg_move3.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv) {
    const int W = argc > 1 ? std::atoi(argv[1]) : 9;
    if (W < 9) return 2;
    const int n = W + 2;
    int bad = 0;
    for (int i = 0; i <= W - 2; ++i)
        for (int j = i + 1; j <= W - 2; ++j)
            for (int k = j + 1; k <= W - 2; ++k)
                for (int r = 0; r < 3; ++r)
                    for (int type = 0; type < 4; ++type) {
                        const int t[3] = {i, j, k};
                        const int a = t[r], b = t[(r + 1) % 3], c = t[(r + 2) % 3];
                        const tsp::SegMove3 m = tsp::seg3_make(a, b, c, type);
                        // the definition
                        auto path = [&](int x, int y) {
                            std::vector<int> out(1, x % n);
                            while (out.back() != y) out.push_back((out.back() + 1) % n);
                            return out;
                        };
                        std::vector<int> S1 = path(a + 1, b), S2 = path(b + 1, c), S3 = path(c + 1, a);
                        if (type == 1 || type == 3) std::reverse(S1.begin(), S1.end());
                        if (type == 1 || type == 2) std::reverse(S2.begin(), S2.end());
                        std::vector<int> seq = type == 1 ? S1 : S2;
                        const std::vector<int> &second = type == 1 ? S2 : S1;
                        seq.insert(seq.end(), second.begin(), second.end());
                        seq.insert(seq.end(), S3.begin(), S3.end());
                        const int at0 = (int)(std::find(seq.begin(), seq.end(), 0) - seq.begin());
                        const int step = seq[(at0 + n - 1) % n] == n - 1 ? 1 : n - 1;   // forward, or the tour came out reversed
                        bool same = m.i == i && m.j == j && m.k == k && seq[(at0 + n - step) % n] == n - 1;
                        std::vector<int> seen((size_t)W, 0);
                        std::printf("%d %d %d %d %d %d ", i, j, k, r, type, m.form);
                        for (int s = 0; s < W; ++s) {
                            const int got = s > i && s <= k ? tsp::seg3_src(m, s) : s;
                            if (s > i && s <= k) std::printf(" %d", got);
                            same = same && got > (s > i && s <= k ? i : s - 1) && got <= (s > i && s <= k ? k : s);
                            if (got >= 0 && got < W) seen[(size_t)got] += 1;
                            same = same && seq[(at0 + s * step) % n] == got;
                        }
                        for (int s = 0; s < W; ++s) same = same && seen[(size_t)s] == 1;
                        std::printf("\n");
                        if (!same) { std::printf("MISMATCH %d %d %d %d %d\n", i, j, k, r, type); bad = 1; }
                    }
    return bad;
}
