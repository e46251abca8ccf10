// row_scan.hpp -- the parts shared by the row scans: KNN lists (nl_opt.hip), 1-trees (held_karp.hip), alpha-nearness (alpha.hip)
// and greedy-edge construction (greedy_edge.hip); DESIGN.md 4.18.
//
// The scan.  One lane owns one row node; the column is wave-uniform and its 32-byte record (ScanCol) comes from scalar loads.
// The columns are cut into chunks across blockIdx.y (scan_chunks); every (row, chunk) writes a partial result, and a second
// kernel merges a row's chunks IN COLUMN ORDER.  Within a row the other end grows with the column, so `<` on ascending columns
// and ascending chunks is the strict order (weight, lo, hi).  The merges themselves stay with their kernels (one best edge:
// k_hk_min1, k_ge_merge; the 16 best: knn_insert in nl_opt.hip, al_insert in alpha.hip): shared forms changed those kernels' code.
// Both ends of an edge must see the same bits of its length: pair_dist.  Nothing here adds floating-point numbers.
// The first part is free of HIP: tests/test_cpu_row_scan.py compiles this text with the host compiler.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

namespace tsp {
// ---- chunk geometry -----------------------------------------------------------------------------
struct ScanChunks { int CH, Cc; };   // columns per chunk, chunks: (Cc - 1) * CH < n <= Cc * CH
inline ScanChunks chunks_of(int n, int want, int min_columns) {
    const int CH = std::max(min_columns, (n + want - 1) / want);
    return {CH, (n + CH - 1) / CH};
}
// about target_waves waves of 64 rows in the scan's grid, at most max_chunks chunks of at least min_columns columns
inline ScanChunks scan_chunks(int n, int target_waves, int max_chunks, int min_columns) {
    const int waves = (n + 63) / 64;
    return chunks_of(n, std::max(1, std::min(max_chunks, (target_waves + waves - 1) / waves)), min_columns);
}
// greedy edge: its late rounds scan a handful of rows, whose time is one chunk's: as many chunks of min_columns as n holds
inline ScanChunks scan_chunks_few_rows(int n, int max_chunks, int min_columns) {
    return chunks_of(n, std::max(1, std::min(max_chunks, n / min_columns)), 1);
}

// ---- device scratch carved from one block -------------------------------------------------------
// A layout is a function that names every array once: lay(c) { c(ptr_a, count_a); c(ptr_b, count_b); ... }.  It runs twice:
// carve_bytes(lay) adds up the sizes, each rounded up to 256 bytes; carve(base, lay) hands out the pointers (256-aligned when
// base is).
struct Carver {
    char *base;
    size_t off = 0;
    template <typename T>
    void operator()(T *&p, size_t count) {
        if (base) p = reinterpret_cast<T *>(base + off);
        off += (sizeof(T) * count + 255) & ~(size_t)255;
    }
};
template <typename LAY> size_t carve_bytes(LAY &&lay) { Carver c{nullptr}; lay(c); return c.off; }
template <typename LAY> void carve(void *base, LAY &&lay) { Carver c{static_cast<char *>(base)}; lay(c); }

// ---- host odds and ends -------------------------------------------------------------------------
inline bool pi_finite(const double *pi, int n) {   // NULL = zeros
    for (int v = 0; pi && v < n; ++v)
        if (!std::isfinite(pi[v])) return false;
    return true;
}

// Edges {lo, hi} as keys that sort by (lo, hi); write_sorted_keys sorts them into edges[2 e], edges[2 e + 1].
inline long long edge_key(int lo, int hi) { return ((long long)lo << 32) | (long long)hi; }
inline void write_sorted_keys(std::vector<long long> &e, int *edges) {
    std::sort(e.begin(), e.end());
    for (size_t k = 0; k < e.size(); ++k) { edges[2 * k] = (int)(e[k] >> 32); edges[2 * k + 1] = (int)(e[k] & 0xffffffffll); }
}
// The same for the slots with lo[k] >= 0.  Returns their number; they are written only when there are exactly `want` of them.
inline int write_sorted_edges(const int *lo, const int *hi, int count, int *edges, int want) {
    std::vector<long long> e;
    e.reserve((size_t)count);
    for (int k = 0; k < count; ++k)
        if (lo[k] >= 0) e.push_back(edge_key(lo[k], hi[k]));
    if ((int)e.size() == want) write_sorted_keys(e, edges);
    return (int)e.size();
}
}  // namespace tsp

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "tsp_dist.hpp"
namespace tsp {
// The column record: 32 bytes, so that a wave-uniform column is one aligned scalar load.
// (x, y): lat, lon in radians for GEO.
struct alignas(32) ScanCol { double x, y, pi; int tag, pad; };                // 1-tree: tag = component; alpha: tag = node id
struct alignas(32) ScanColDeg { double x, y; int deg, pad0; long long pad1; };   // greedy edge
static_assert(sizeof(ScanCol) == 32 && sizeof(ScanColDeg) == 32, "a column record is one 32-byte scalar load");

// d(a, b) with the same bits from either end.  Every metric but GEO is symmetric to the bit (a - b = -(b - a) exactly, and only
// squares and absolute values of it are used), so the row goes first.  GEO (products of cosines, acos) is symmetric only if
// ocml's cos is even: measured so on gfx950 -- the distance matrices of tests/test_gpu_geo.py are symmetric to the bit -- but
// promised nowhere, so GEO takes the lower id first.  k_alpha_scan's lane carries the same two rules written out (DESIGN.md
// 4.18).  k_knn_scan does NOT use this: its lists are defined on the device's distance matrix, which is computed row first
// (test_knn_geo_on_the_devices_own_matrix).
template <int WT, bool INT>
__device__ __forceinline__ double pair_dist(int ida, double ax, double ay, int idb, double bx, double by) {
    const bool alo = WT != WT_GEO || ida < idb;
    return dist_xy<WT, INT>(alo ? ax : bx, alo ? ay : by, alo ? bx : ax, alo ? by : ay);
}
// the penalised weight, the lower id's penalty added first: (d + pi_lo) + pi_hi
template <int WT, bool INT>
__device__ __forceinline__ double pair_weight(int ida, double ax, double ay, double pia, int idb, double bx, double by, double pib) {
    const bool alo = ida < idb;
    const double d = pair_dist<WT, INT>(ida, ax, ay, idb, bx, by);
    return (d + (alo ? pia : pib)) + (alo ? pib : pia);
}
}  // namespace tsp
#endif
