// cluster_deal.hpp -- the CLUSTER engine's group-pair table: which of a tour's C workgroups tests which pair of rank-order groups
// in every step of the sorted scan.  Pure host arithmetic on plain arrays (nothing of HIP: tests/cluster_deal_check.cpp compiles it
// with the host compiler).
#pragma once
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

namespace tsp {

// gbox: ng x {min x, max x, min y, max y}; sperm: rank slot -> node, or -1 for padding (ng * 64 slots); xy: the raw coordinates
// (2n); order: the tour the handle holds now (node at position p), or nullptr; sc: 1 / sqrt(10) for ATT, else 1.
// tab = C x ntests pair ids (row << 16 | column), every pair r <= c once, each workgroup's row padded with -1; returns ntests.
// Every pair is tested in every step whoever it is dealt to: the table decides the time of a step, never a result.
inline long long cluster_deal(const double *gbox, const int *sperm, const double *xy, const int *order, int n, int ng, int C,
                              bool by_cost, double sc, std::vector<int> &tab) {
    const long long npairs = (long long)ng * (ng + 1) / 2;
    const long long ntests = (npairs + C - 1) / C;
    std::vector<std::pair<double, int>> pr((size_t)npairs);
    size_t w = 0;
    for (int r = 0; r < ng; ++r)
        for (int cg = r; cg < ng; ++cg) {
            const double *rb = gbox + 4 * (size_t)r, *cb = gbox + 4 * (size_t)cg;
            const double gx = std::max(0.0, std::max(rb[0] - cb[1], cb[0] - rb[1])), gy = std::max(0.0, std::max(rb[2] - cb[3], cb[2] - rb[3]));
            pr[w++] = {gx * gx + gy * gy, (r << 16) | cg};
        }
    std::sort(pr.begin(), pr.end());
    tab.assign((size_t)C * ntests, -1);
    bool dealt = false;
    if (by_cost && order) {
        // Deal by estimated cost instead of in turn.  A step costs the time of its slowest workgroup (1.9 us of an 11.4 us
        // best-improvement step at n = 10 000 were spent waiting for it), and what a group pair costs is decided by the tour:
        // whether it survives the box test and how many of its rows survive the culling.  Both are estimated here on the
        // tour the handle holds now (Euclidean lengths: a cost model, not a decision), the survivors are dealt heaviest
        // first to the least loaded workgroup (LPT), the others fill the tables up in turn.  Every pair is still tested in
        // every step; only who tests it changes.
        auto X = [&](int v) { return xy[2 * (size_t)v]; };
        auto Y = [&](int v) { return xy[2 * (size_t)v + 1]; };
        auto len = [&](int u, int v) { return sc * std::sqrt((X(u) - X(v)) * (X(u) - X(v)) + (Y(u) - Y(v)) * (Y(u) - Y(v))) + 1.0; };
        std::vector<double> ds((size_t)n, 0.0), inc((size_t)n, 0.0), gmx((size_t)ng, 0.0);
        bool tour_ok = true;
        for (int q = 0; q < n && tour_ok; ++q) tour_ok = order[q] >= 0 && order[q] < n;
        if (tour_ok) {
            for (int q = 0; q < n; ++q) {
                const int v = order[q], su = order[q + 1 == n ? 0 : q + 1], pv = order[q == 0 ? n - 1 : q - 1];
                ds[v] = len(v, su);
                inc[v] = std::max(ds[v], len(v, pv));
            }
            for (int g = 0; g < ng; ++g)
                for (int k = 0; k < 64; ++k) { const int v = sperm[(size_t)g * 64 + k]; if (v >= 0) gmx[g] = std::max(gmx[g], inc[v]); }
            struct Item { double cost; int e; };
            std::vector<Item> heavy, light;
            for (long long k = 0; k < npairs; ++k) {
                const int e = pr[(size_t)k].second, r = e >> 16, cg = e & 0xffff;
                const double T = gmx[r] + gmx[cg] + 2.0;
                double cost = 0.0;
                if (sc * sc * pr[(size_t)k].first < T * T) {
                    const double *cb = gbox + 4 * (size_t)cg;
                    int live = 0;
                    for (int q = 0; q < 64; ++q) {
                        const int v = sperm[(size_t)r * 64 + q];
                        if (v < 0) continue;
                        const double gx = std::max(0.0, std::max(cb[0] - X(v), X(v) - cb[1])), gy = std::max(0.0, std::max(cb[2] - Y(v), Y(v) - cb[3]));
                        const double Tr = ds[v] + gmx[cg] + 2.0;
                        live += sc * sc * (gx * gx + gy * gy) < Tr * Tr;
                    }
                    cost = 8.0 + live;   // staging the pair's 128 records + its live rows against 64 columns
                }
                (cost > 0.0 ? heavy : light).push_back({cost, e});
            }
            std::stable_sort(heavy.begin(), heavy.end(), [](const Item &x, const Item &y) { return x.cost > y.cost; });
            std::vector<double> load((size_t)C, 0.0);
            std::vector<int> cnt((size_t)C, 0);
            // least loaded workgroup with room: a heap keyed by load
            std::vector<std::pair<double, int>> heap;
            for (int w = 0; w < C; ++w) heap.push_back({0.0, w});
            auto cmp = [](const std::pair<double, int> &x, const std::pair<double, int> &y) { return x.first > y.first || (x.first == y.first && x.second > y.second); };
            std::make_heap(heap.begin(), heap.end(), cmp);
            for (const Item &it : heavy) {
                std::pop_heap(heap.begin(), heap.end(), cmp);
                auto top = heap.back(); heap.pop_back();
                const int w = top.second;
                tab[(size_t)w * ntests + (size_t)cnt[w]++] = it.e;
                load[w] += it.cost;
                if (cnt[w] < ntests) { heap.push_back({load[w], w}); std::push_heap(heap.begin(), heap.end(), cmp); }
            }
            int w = 0;
            for (const Item &it : light) {   // the rest in turn, wherever there is room
                while (cnt[w] >= ntests) w = (w + 1) % C;
                tab[(size_t)w * ntests + (size_t)cnt[w]++] = it.e;
                w = (w + 1) % C;
            }
            dealt = true;
        }
    }
    if (!dealt)
        for (long long k = 0; k < npairs; ++k) tab[(size_t)(k % C) * ntests + (size_t)(k / C)] = pr[(size_t)k].second;
    return ntests;
}

}  // namespace tsp
