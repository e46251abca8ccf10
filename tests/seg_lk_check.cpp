// seg_lk_check.cpp -- csrc/seg_lk.hpp as k_seg_ils includes it, built with the host compiler and run by tests/test_cpu_seg_lk.py.
// Arguments: the number of cases (default 4000) and the stride of the printed sample (default 197).
// A case is a window of W = 9 slots holding nine of n = 11 nodes in an order drawn by a fixed generator, a symmetric table of
// distances 0 .. 6 (small, so that equal gains and equal g2 are common), and lists of K = 1 .. 5 entries that may name the node
// itself, a node twice and the two nodes outside the window.  For every case, every slot i = 0 .. 8, both sides and the depths 1,
// 2, 3 and 16 the chain is run twice: through the header (the entries of a step one after the other, folded by seglk_beats as the
// kernel's lanes fold them) and by the rule stated by brute force: a copy of the window, read backwards for side 1, on which
// every reversal is carried out for real.  Compared: whether there is a first edge, the reversals made, the best prefix, the bits
// of its gain, every j, e, y and p, the hull, and the window that the header's inverse map gives for the first h* reversals
// against the brute force's array at that point.  Every `stride`-th case is printed at depth 16 as
//   C case K / S the window / D the table, row by row / N the lists / R i s first steps hstar best j_1 .. j_steps (18 lines)
// Exit status 1 and a line "MISMATCH ..." when anything differs; the last line is "cases <count> chains <count> deepest <steps>".
#include "seg_lk.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

constexpr int N = 11, W = 9;
using u16 = unsigned short;

struct Case {
    int K;
    int seq[W];
    int slot[N];        // -1: outside the window
    double dist[N][N];
    int nbr[N][5];
};

struct View {
    const Case *c;
    int W;
    int entry(int e, int k) const { const int y = c->nbr[e][k]; return c->slot[y] < 0 ? -1 : y; }
    int slot(int id) const { return c->slot[id]; }
    int at(int s) const { return c->seq[s]; }
    double d(int a, int b) const { return a < b ? c->dist[a][b] : c->dist[b][a]; }
};

struct Result {
    bool first;
    int steps, hstar;
    double best;
    int j[16], e[16], y[16], p[16];
    int after[W];       // the window (as stored) after the first hstar reversals
    int lo, hi;         // their hull in window slots; lo > hi without one
};

unsigned long long g_state;
unsigned draw(unsigned m) {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)((g_state >> 33) % m);
}

Case make_case(long long id) {
    g_state = 0x9E3779B97F4A7C15ull ^ (unsigned long long)id;
    Case c;
    c.K = 1 + (int)(id % 5);
    int perm[N];
    for (int k = 0; k < N; ++k) perm[k] = k;
    for (int k = N - 1; k > 0; --k) { const int r = (int)draw((unsigned)k + 1); const int t = perm[k]; perm[k] = perm[r]; perm[r] = t; }
    for (int k = 0; k < N; ++k) c.slot[k] = -1;
    for (int k = 0; k < W; ++k) { c.seq[k] = perm[k]; c.slot[perm[k]] = k; }
    for (int a = 0; a < N; ++a)
        for (int b = a; b < N; ++b) c.dist[a][b] = c.dist[b][a] = a == b ? 0.0 : (double)draw(7);
    for (int a = 0; a < N; ++a)
        for (int k = 0; k < 5; ++k) c.nbr[a][k] = (int)draw(N);
    return c;
}

Result by_header(const Case &c, int i_win, int s, int depth) {
    Result r;
    std::memset(&r, 0, sizeof r);
    View v{&c, W};
    const int i = tsp::seglk_side(s, W, i_win);
    r.first = i <= W - 2;
    r.lo = 1; r.hi = 0;
    for (int k = 0; k < W; ++k) r.after[k] = c.seq[k];
    if (!r.first) return r;
    u16 j[tsp::kSegLkMaxDepth], ends[3 * tsp::kSegLkMaxDepth];
    const int t1 = c.seq[i_win];
    tsp::SegLkChain ch;
    tsp::seglk_begin(ch, v.at(tsp::seglk_side(s, W, i + 1)));
    while (ch.h < depth) {
        const double x = v.d(t1, ch.e);
        tsp::SegLkPick best = tsp::seglk_entry(v, s, i, j, ends, ch, x, 0);
        for (int k = 1; k < c.K; ++k) {
            const tsp::SegLkPick q = tsp::seglk_entry(v, s, i, j, ends, ch, x, k);
            if (tsp::seglk_beats(q.g2, q.k, best.g2, best.k)) best = q;
        }
        if (best.k >= tsp::kSegLkLanes) break;
        tsp::seglk_take(ch, best, v.d(best.p, t1), j, ends);
    }
    r.steps = ch.h; r.hstar = ch.hstar; r.best = ch.best;
    for (int q = 0; q < ch.h; ++q) { r.j[q] = j[q]; r.e[q] = ends[3 * q]; r.y[q] = ends[3 * q + 1]; r.p[q] = ends[3 * q + 2]; }
    if (ch.hstar >= 1) {
        const int lo_c = i + 1, hi_c = tsp::seglk_hull_hi(j, ch.hstar);
        r.lo = s ? W - 1 - hi_c : lo_c; r.hi = s ? W - 1 - lo_c : hi_c;
        for (int k = r.lo; k <= r.hi; ++k)   // the source function of the kernel's seg_permute
            r.after[k] = c.seq[tsp::seglk_side(s, W, tsp::seglk_inv(i, j, ch.hstar, tsp::seglk_side(s, W, k)))];
    }
    return r;
}

Result by_force(const Case &c, int i_win, int s, int depth) {
    Result r;
    std::memset(&r, 0, sizeof r);
    int cur[W], keep[W];
    for (int k = 0; k < W; ++k) keep[k] = cur[k] = s ? c.seq[W - 1 - k] : c.seq[k];
    const int i = s ? W - 1 - i_win : i_win;
    r.first = i <= W - 2;
    r.lo = 1; r.hi = 0;
    for (int k = 0; k < W; ++k) r.after[k] = c.seq[k];
    if (!r.first) return r;
    auto d = [&](int a, int b) { return a < b ? c.dist[a][b] : c.dist[b][a]; };
    const int t1 = cur[i];
    double G = 0.0, best = 0.0;
    bool used[N];
    for (int k = 0; k < N; ++k) used[k] = false;
    int top = 0;
    for (int h = 1; h <= depth; ++h) {
        const int e = cur[i + 1];
        const double x = d(t1, e);
        bool any = false;
        double bg2 = 0.0;
        int bj = 0, by = 0, bp = 0;
        for (int k = 0; k < c.K; ++k) {
            const int y = c.nbr[e][k];
            if (y == e || used[y]) continue;
            int jj = -1;
            for (int q = 0; q < W; ++q) if (cur[q] == y) jj = q;
            if (jj < i + 3 || jj > W - 1) continue;
            const double g1 = (G + x) - d(e, y);
            if (!(g1 > best)) continue;
            const int p = cur[jj - 1];
            const double g2 = g1 + d(p, y);
            if (!any || g2 > bg2) { any = true; bg2 = g2; bj = jj; by = y; bp = p; }
        }
        if (!any) break;
        for (int a = i + 1, b = bj - 1; a < b; ++a, --b) { const int t = cur[a]; cur[a] = cur[b]; cur[b] = t; }
        used[e] = used[by] = true;
        r.j[h - 1] = bj; r.e[h - 1] = e; r.y[h - 1] = by; r.p[h - 1] = bp;
        r.steps = h;
        G = bg2 - d(bp, t1);
        if (G > best) {
            best = G; r.hstar = h;
            for (int k = 0; k < W; ++k) keep[k] = cur[k];
        }
    }
    r.best = best;
    // the hull covers every reversal up to the best prefix, also those that did not improve on the one before
    for (int q = 0; q < r.hstar; ++q) top = r.j[q] > top ? r.j[q] : top;
    if (r.hstar >= 1) {
        for (int k = 0; k < W; ++k) r.after[s ? W - 1 - k : k] = keep[k];
        const int lo_c = i + 1, hi_c = top - 1;
        r.lo = s ? W - 1 - hi_c : lo_c; r.hi = s ? W - 1 - lo_c : hi_c;
    }
    return r;
}

bool same(const Result &a, const Result &b) {
    if (a.first != b.first || a.steps != b.steps || a.hstar != b.hstar || std::memcmp(&a.best, &b.best, sizeof a.best)) return false;
    for (int q = 0; q < a.steps; ++q)
        if (a.j[q] != b.j[q] || a.e[q] != b.e[q] || a.y[q] != b.y[q] || a.p[q] != b.p[q]) return false;
    if (a.lo != b.lo || a.hi != b.hi) return false;
    for (int k = 0; k < W; ++k)
        if (a.after[k] != b.after[k]) return false;
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    const long long cases = argc > 1 ? std::atoll(argv[1]) : 4000;
    const long long stride = argc > 2 ? std::atoll(argv[2]) : 197;
    if (cases < 1 || stride < 1) return 2;
    const int depths[4] = {1, 2, 3, 16};
    long long chains = 0;
    int bad = 0, deepest = 0;
    for (long long id = 0; id < cases; ++id) {
        const Case c = make_case(id);
        const bool show = id % stride == 0;
        if (show) {
            std::printf("C %lld %d\nS", id, c.K);
            for (int k = 0; k < W; ++k) std::printf(" %d", c.seq[k]);
            std::printf("\nD");
            for (int a = 0; a < N; ++a)
                for (int b = 0; b < N; ++b) std::printf(" %g", c.dist[a][b]);
            std::printf("\nN");
            for (int a = 0; a < N; ++a)
                for (int k = 0; k < c.K; ++k) std::printf(" %d", c.nbr[a][k]);
            std::printf("\n");
        }
        for (int i = 0; i < W; ++i)
            for (int s = 0; s < 2; ++s)
                for (int q = 0; q < 4; ++q) {
                    const Result h = by_header(c, i, s, depths[q]), f = by_force(c, i, s, depths[q]);
                    chains += 1;
                    deepest = h.steps > deepest ? h.steps : deepest;
                    // a window move: the ends stay, and nothing outside the hull moves
                    bool ok = same(h, f) && h.after[0] == c.seq[0] && h.after[W - 1] == c.seq[W - 1] && h.steps <= depths[q];
                    if (h.hstar >= 1) ok = ok && 1 <= h.lo && h.lo <= h.hi && h.hi <= W - 2 && h.best > 0.0;
                    if (!ok) {
                        std::printf("MISMATCH case %lld slot %d side %d depth %d\n", id, i, s, depths[q]);
                        bad = 1;
                    }
                    if (show && q == 3) {
                        std::printf("R %d %d %d %d %d %g", i, s, h.first ? 1 : 0, h.steps, h.hstar, h.best);
                        for (int t = 0; t < h.steps; ++t) std::printf(" %d", h.j[t]);
                        std::printf("\n");
                    }
                }
    }
    std::printf("cases %lld chains %lld deepest %d\n", cases, chains, deepest);
    return bad;
}
