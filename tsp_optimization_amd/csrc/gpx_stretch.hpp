// gpx_stretch.hpp -- index arithmetic of the partition crossover: cyclic intervals of a tour's order, the way a
// stretch is read forwards or backwards, and the pieces of the nearest-boundary scans that one thread works through alone.  Plain
// C++ for the host compiler and for hipcc: the kernels of gpx.hip and tests/gpx_stretch_check.cpp compile this very text.
//
// Positions are 0 .. n - 1 and cyclic.  The interval first .. last is first, first + 1, ... up to last, past n - 1 -> 0 when
// last < first; first == last is one position (never the whole cycle).  A piece of the child is such an interval of the other
// parent's order, read from either end.
#pragma once

#if defined(__HIPCC__)
#define TSP_GPX_HD __host__ __device__ __forceinline__
#else
#define TSP_GPX_HD inline
#endif

namespace tsp {

TSP_GPX_HD int gpx_next(int p, int n) { return p + 1 == n ? 0 : p + 1; }
TSP_GPX_HD int gpx_prev(int p, int n) { return p == 0 ? n - 1 : p - 1; }

// steps from `first` forwards to p: 0 .. n - 1
TSP_GPX_HD int gpx_cyc_off(int first, int p, int n) { return p >= first ? p - first : p - first + n; }
// positions of the interval first .. last: 1 .. n
TSP_GPX_HD int gpx_cyc_len(int first, int last, int n) { return gpx_cyc_off(first, last, n) + 1; }
// p lies in first .. last
TSP_GPX_HD bool gpx_cyc_has(int first, int last, int p, int n) { return gpx_cyc_off(first, p, n) <= gpx_cyc_off(first, last, n); }

// The k-th position (k = 0 .. len - 1) of the interval first .. last read forwards (from first) or backwards (from last) ...
TSP_GPX_HD int gpx_read_pos(int first, int last, int k, bool backward, int n) {
    if (backward) return last >= k ? last - k : last - k + n;
    return first + k >= n ? first + k - n : first + k;   // first, k < n: no overflow below 2^30 nodes
}
// ... and the k at which such a read meets position p of the interval
TSP_GPX_HD int gpx_read_off(int first, int last, int p, bool backward, int n) {
    return backward ? gpx_cyc_off(p, last, n) : gpx_cyc_off(first, p, n);
}

// ---- nearest boundary to the left / right, cyclic, in chunks --------------------------------------------------------------------
// flag[0 .. n-1] marks boundaries.  left[p] = the nearest boundary at or before p, right[p] = the nearest at or after p, both
// cyclic (left[p] may lie behind p past position 0), -1 everywhere when nothing is marked.  The positions are cut into chunks of
// CH; one thread (or one loop iteration of the check program) owns a chunk:
//   1. gpx_chunk_ends: the chunk's own last and first boundary (-1: none);
//   2. across chunks: carry_left[t] = the last boundary of the chunks before t, carry_right[t] = the first one of the chunks behind
//      t (-1: none), and the first and last boundary of all (a scan over the workgroup's chunks in gpx.hip, plain loops in the check
//      program);
//   3. gpx_chunk_fill: the chunk's left[] and right[] from its carries; what no chunk on its side holds wraps to the other end.
TSP_GPX_HD int gpx_chunk_size(int n, int threads) { return (n + threads - 1) / threads; }

template <typename FLAG>
TSP_GPX_HD void gpx_chunk_ends(FLAG flag, int lo, int hi, int *last, int *first) {
    int l = -1, f = -1;
    for (int p = lo; p < hi; ++p)
        if (flag(p)) { l = p; if (f < 0) f = p; }
    *last = l; *first = f;
}

template <typename FLAG>
TSP_GPX_HD void gpx_chunk_fill(FLAG flag, int lo, int hi, int carry_left, int carry_right, int all_first, int all_last, int *left,
                               int *right) {
    int l = carry_left >= 0 ? carry_left : all_last;   // nothing before this chunk: the last boundary of all, behind position 0
    for (int p = lo; p < hi; ++p) {
        if (flag(p)) l = p;
        left[p] = l;
    }
    int r = carry_right >= 0 ? carry_right : all_first;
    for (int p = hi - 1; p >= lo; --p) {
        if (flag(p)) r = p;
        right[p] = r;
    }
}

}  // namespace tsp
