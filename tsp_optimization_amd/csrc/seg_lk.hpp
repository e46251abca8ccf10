// seg_lk.hpp -- a Lin-Kernighan chain inside a window of the windowed iterated local search (tsp_dev_seg_ils_lk):
// the slot map of a chain and its inverse, the test and the choice of a step, and the best-prefix bookkeeping.  Plain C++ for the
// host compiler and for hipcc: k_seg_ils (seg_ils.hip) and tests/seg_lk_check.cpp compile this very text.
//
// A chain of side 0 starts at the node t1 of slot i <= W - 2 and is a list of reversals of the slots i + 1 .. j_h - 1, h = 1, 2, ..:
// every one starts behind t1, so the chain is i and the list j_1, j_2, ...  It never copies the window: the slot a node has under
// the first h reversals is its slot passed through them in order (seglk_fwd), and the slot whose node stands at a slot under
// them is that slot passed through them backwards (seglk_inv).  Side 1 is the same chain on the window read backwards
// (seglk_side maps a slot of one reading to the other).  "Window slot" below is a slot of the window as stored, "chain slot" one
// of the chain's reading under its reversals so far.
//
// A view V gives the chain what it reads, in ids of the caller's choice (the kernel: 16-bit home ids; the check: node ids):
//   int  W                      the window
//   int  entry(int e, int k)    the id of entry k of e's list, -1 when it is no window node
//   int  slot(int id)           the window slot of a window node
//   int  at(int slot)           the id at a window slot
//   double d(int a, int b)      the distance, the lower node id first
#pragma once

#if defined(__HIPCC__)
#define TSP_SEGLK_HD __host__ __device__ __forceinline__
#else
#define TSP_SEGLK_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace tsp {

constexpr int kSegLkMaxDepth = 16;   // TSP_SEG_LK_MAX_DEPTH
constexpr int kSegLkLanes = 16;      // entries a step looks at side by side: TSP_NL_MAX_K

// chain slot <-> window slot of the other reading
TSP_SEGLK_HD int seglk_side(int s, int W, int k) { return s ? W - 1 - k : k; }

// the chain slot k after the first h reversals of the chain (i; j[0 .. h-1])
TSP_SEGLK_HD int seglk_fwd(int i, const unsigned short *j, int h, int k) {
    for (int q = 0; q < h; ++q)
        if (k > i && k < (int)j[q]) k = i + (int)j[q] - k;
    return k;
}

// the chain slot before any reversal whose node stands at chain slot k after the first h reversals
TSP_SEGLK_HD int seglk_inv(int i, const unsigned short *j, int h, int k) {
    for (int q = h - 1; q >= 0; --q)
        if (k > i && k < (int)j[q]) k = i + (int)j[q] - k;
    return k;
}

// what one list entry offers to a step
struct SegLkPick {
    double g2;   // -inf: not admissible
    int k;       // the entry; kSegLkLanes: not admissible
    int j, y, p;
};

// (g2, k) of a beats that of b: the largest g2, the lowest k on ties; an entry that is not admissible beats nothing
TSP_SEGLK_HD bool seglk_beats(double g2a, int ka, double g2b, int kb) {
    return ka < kSegLkLanes && (kb >= kSegLkLanes || g2a > g2b || (g2a == g2b && ka < kb));
}

struct SegLkChain {
    double G, best;
    int h, hstar;   // reversals made, and the best prefix
    int e;          // the node behind t1
};

TSP_SEGLK_HD void seglk_begin(SegLkChain &c, int e) { c.G = 0.0; c.best = 0.0; c.h = 0; c.hstar = 0; c.e = e; }

// Entry k of the list of c.e in step c.h + 1 of the chain (s, i; j[0 .. c.h-1]) from t1, x = d(t1, c.e).  ends[3 q], ends[3 q + 1],
// q < c.h, are e and y of the steps made: the used set.
template <typename V>
TSP_SEGLK_HD SegLkPick seglk_entry(const V &v, int s, int i, const unsigned short *j, const unsigned short *ends, const SegLkChain &c,
                                   double x, int k) {
    SegLkPick r;
    r.g2 = -__builtin_inf(); r.k = kSegLkLanes; r.j = 0; r.y = 0; r.p = 0;
    const int y = v.entry(c.e, k);
    if (y < 0 || y == c.e) return r;
    const int jj = seglk_fwd(i, j, c.h, seglk_side(s, v.W, v.slot(y)));
    if (jj < i + 3) return r;   // jj <= W - 1 as every slot
    for (int q = 0; q < c.h; ++q)
        if ((int)ends[3 * q] == y || (int)ends[3 * q + 1] == y) return r;
    const double g1 = (c.G + x) - v.d(c.e, y);
    if (!(g1 > c.best)) return r;
    const int p = v.at(seglk_side(s, v.W, seglk_inv(i, j, c.h, jj - 1)));
    r.g2 = g1 + v.d(p, y); r.k = k; r.j = jj; r.y = y; r.p = p;
    return r;
}

// The step takes the pick: the reversal of the chain slots i + 1 .. pick.j - 1 goes behind the chain's, e, y, p behind its ends,
// and the prefix is the best one when its closed-up gain beats every shorter one's.  dpt = d(p, t1).
TSP_SEGLK_HD void seglk_take(SegLkChain &c, const SegLkPick &pick, double dpt, unsigned short *j, unsigned short *ends) {
    j[c.h] = (unsigned short)pick.j;
    ends[3 * c.h] = (unsigned short)c.e; ends[3 * c.h + 1] = (unsigned short)pick.y; ends[3 * c.h + 2] = (unsigned short)pick.p;
    c.h += 1;
    c.G = pick.g2 - dpt;
    if (c.G > c.best) { c.best = c.G; c.hstar = c.h; }
    c.e = pick.p;
}

// the hull in chain slots of the first hstar >= 1 reversals: i + 1 .. the return value
TSP_SEGLK_HD int seglk_hull_hi(const unsigned short *j, int hstar) {
    int m = 0;
    for (int q = 0; q < hstar; ++q) m = (int)j[q] > m ? (int)j[q] : m;
    return m - 1;
}

}  // namespace tsp
