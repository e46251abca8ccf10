// seg_move3.hpp -- a 3-opt move inside a window of the windowed iterated local search: the relabelling of the
// move's type under the window's orientation and the permutation of the slot interval it rewrites.  Plain C++ for the host
// compiler and for hipcc: k_seg_ils (seg_ils.hip) and tests/seg_move3_check.cpp compile this very text.
//
// The three removed edges have their tails at the slots i < j < k (k <= W - 2); X = slots i+1 .. j, Y = slots j+1 .. k.  The move
// (a, b, c, type) of include/tsp_hip.h names the tails in tour order from a, the tail of lowest node id, through the outside of
// the window where that is the way round: a sits at slot i (r = 0), j (r = 1) or k (r = 2).  The move's tour, turned so that the
// outside of the window keeps its direction, has the slots i+1 .. k in one of four forms (' = reversed):
//            type 0   type 1   type 2   type 3
//     r = 0   Y X     X' Y'    Y' X     Y X'
//     r = 1   Y X     Y X'     X' Y'    Y' X
//     r = 2   Y X     Y' X     Y X'     X' Y'
// Slots 0 .. i and k+1 .. W-1 keep their nodes.
#pragma once

#if defined(__HIPCC__)
#define TSP_SEG3_HD __host__ __device__ __forceinline__
#else
#define TSP_SEG3_HD inline
#endif

namespace tsp {

enum { kSeg3YX = 0, kSeg3XrYr = 1, kSeg3YrX = 2, kSeg3YXr = 3 };

struct SegMove3 {
    int i, j, k;   // the slots of the three tails, i < j < k
    int form;      // what the slots i+1 .. k become
};

// the form of the table: type 0 is Y X, the others turn with r through (X' Y', Y' X, Y X')
TSP_SEG3_HD int seg3_form(int r, int type) { return type == 0 ? kSeg3YX : 1 + (type - 1 + 2 * r) % 3; }

// The move (a, b, c, type) with a, b, c at the slots sa, sb, sc (pairwise different; b and c follow a in tour order).
TSP_SEG3_HD SegMove3 seg3_make(int sa, int sb, int sc, int type) {
    // in tour order from a: (sa, sb, sc) is (i, j, k), (j, k, i) or (k, i, j)
    const int r = sa < sb ? (sa < sc ? 0 : 1) : 2;
    SegMove3 m;
    m.i = r == 0 ? sa : (r == 1 ? sc : sb);
    m.j = r == 0 ? sb : (r == 1 ? sa : sc);
    m.k = r == 0 ? sc : (r == 1 ? sb : sa);
    m.form = seg3_form(r, type);
    return m;
}

// The slot whose node slot s takes, i + 1 <= s <= k: a permutation of i+1 .. k.
TSP_SEG3_HD int seg3_src(const SegMove3 &m, int s) {
    const int q = s - (m.i + 1), lx = m.j - m.i, ly = m.k - m.j;
    if (m.form == kSeg3XrYr) return q < lx ? m.j - q : m.k - (q - lx);
    if (q < ly) return m.form == kSeg3YrX ? m.k - q : m.j + 1 + q;   // Y or Y' first
    return m.form == kSeg3YXr ? m.j - (q - ly) : m.i + 1 + (q - ly);
}

}  // namespace tsp
