// seg_groups.hpp -- several trial groups per window of the windowed iterated local search: which of the offers of
// a window's groups are written to the tour.  Plain C++ for the host compiler and for hipcc: k_seg_commit (seg_ils.hip) and
// tests/seg_groups_check.cpp compile this very text.
//
// Group g of a window offers the slots lo .. hi (1 <= lo <= hi <= W - 2) of its final window, which differs from the window the
// iteration found at lo and at hi and nowhere outside them, and gain = its window cost minus the starting one (< 0).  The edges it
// changed are those of the slots lo - 1 .. hi.  Two offers conflict iff those edge ranges meet; g loses to h iff they conflict and
// (gain_h, h) < (gain_g, g); g commits iff it offers and loses to no group.  The committed intervals are pairwise disjoint and the
// best offer of a window always commits.
#pragma once

#if defined(__HIPCC__)
#define TSP_SEGG_HD __host__ __device__ __forceinline__
#else
#define TSP_SEGG_HD inline
#endif

namespace tsp {

struct SegOffer {
    int offer;     // 0: the group accepted no trial; lo, hi and gain mean nothing
    int lo, hi;
    double gain;
};

// the edge ranges lo - 1 .. hi of two offers meet
TSP_SEGG_HD bool segg_conflict(int lo_g, int hi_g, int lo_h, int hi_h) { return lo_h - 1 <= hi_g && lo_g - 1 <= hi_h; }

// the offer of group g loses to group h
TSP_SEGG_HD bool segg_loses(const SegOffer &og, int g, const SegOffer &oh, int h) {
    if (!oh.offer || h == g || !segg_conflict(og.lo, og.hi, oh.lo, oh.hi)) return false;
    return oh.gain < og.gain || (oh.gain == og.gain && h < g);
}

// group g of the G groups o[0 .. G-1] commits
TSP_SEGG_HD bool segg_commits(const SegOffer *o, int G, int g) {
    if (!o[g].offer) return false;
    for (int h = 0; h < G; ++h)
        if (segg_loses(o[g], g, o[h], h)) return false;
    return true;
}

}  // namespace tsp
