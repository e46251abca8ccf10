// nl_arc.hpp -- the arc of a move of the list descents: the cyclic range of tour positions that nl_apply_move
// writes, extended by the ends of the removed edges, and when two arcs are disjoint; and the key of a 3-opt move (nl3_key,
// nl3_unkey).  Plain C++ for the host compiler and for hipcc: the scans of the batched descent, its claim kernels (nl_batch.hip),
// the scans and the decoders of the 3-opt kind and tests/nl_arc_check.cpp compile this very text.
// All positions are along the successor orientation, modulo n.
#pragma once

#if defined(__HIPCC__)
#define TSP_ARC_HD __host__ __device__ __forceinline__
#else
#define TSP_ARC_HD inline
#endif

namespace tsp {

struct NlArc {
    int start, len;   // positions start, start + 1, .., start + len - 1 (mod n); 1 <= len <= n
};

// p - from mod n, for 0 <= p, from < n
TSP_ARC_HD int arc_ahead(int p, int from, int n) {
    const int g = p - from;
    return g < 0 ? g + n : g;
}

// x mod n for -n <= x < 2 n
TSP_ARC_HD int arc_wrap(int x, int n) { return x >= n ? x - n : (x < 0 ? x + n : x); }

TSP_ARC_HD NlArc arc_make(int start, int len, int n) { return NlArc{start, len > n ? n : len}; }

// 2-opt (i, j): the forward path i1 .. j is reversed; with the ends of the removed edges, i .. j1
TSP_ARC_HD NlArc nl_arc_two(int pi, int pj, int n) { return arc_make(pi, arc_ahead(pj, pi, n) + 2, n); }

// 3-opt (a, b, c, T): whatever the type, the positions of a1 .. c are rewritten; with the ends, a .. c1
TSP_ARC_HD NlArc nl_arc_three(int pa, int pc, int n) { return arc_make(pa, arc_ahead(pc, pa, n) + 2, n); }

// Or-opt (f, L, a, o): or_shift_apply moves the shorter of the two paths between the segment and the insertion point.  m1 nodes
// s .. a lie behind the segment, m2 nodes b .. p ahead of it: m1 <= m2 rewrites f .. a (arc p .. b), else b .. l (arc a .. s).
TSP_ARC_HD NlArc nl_arc_or(int pf, int pa, int L, int n) {
    const int m1 = arc_ahead(pa, arc_wrap(pf + L, n), n) + 1;
    const int m2 = n - L - m1;
    if (m1 <= m2) return arc_make(arc_wrap(pf - 1, n), m1 + L + 2, n);
    return arc_make(pa, m2 + L + 2, n);
}

// The 3-opt kind's own key, ((a n + b) n + c) 4 + type, below the kind bit of the decision key (nl_common.hpp), and back.  The
// decoded move divides when it is asked, so that a caller pays for the tails it reads, in the order it reads them.
TSP_ARC_HD unsigned long long nl3_key(int a, int b, int c, int type, int n) {
    const unsigned long long un = (unsigned long long)n;
    return (((unsigned long long)a * un + (unsigned long long)b) * un + (unsigned long long)c) * 4ull + (unsigned long long)type;
}
struct Nl3Move {
    unsigned long long key;
    int n;
    TSP_ARC_HD unsigned long long abc() const { return key >> 2; }
    TSP_ARC_HD int type() const { return (int)(key & 3); }
    TSP_ARC_HD int a() const { return (int)(abc() / ((unsigned long long)n * (unsigned long long)n)); }
    TSP_ARC_HD int b() const { return (int)((abc() / (unsigned long long)n) % (unsigned long long)n); }
    TSP_ARC_HD int c() const { return (int)(abc() % (unsigned long long)n); }
};
TSP_ARC_HD Nl3Move nl3_unkey(unsigned long long key, int n) { return Nl3Move{key, n}; }

// The arc of the move with decision key `key` (nl_common.hpp: bit 63 the 3-opt kind over nl3_key, bit 62 Or-opt over
// (((f 3 + L - 1) n + a) 2 + o), neither 2-opt over i n + j) on the tour whose node v is at position pos[v].
TSP_ARC_HD NlArc nl_arc_of_key(const int *pos, int n, unsigned long long key) {
    const unsigned long long un = (unsigned long long)n;
    if (key >> 63) {
        const Nl3Move m = nl3_unkey(key & ~(1ull << 63), n);
        return nl_arc_three(pos[m.a()], pos[m.c()], n);
    }
    if (key >> 62) {
        const unsigned long long t = (key & ~(1ull << 62)) >> 1;
        const int fl = (int)(t / un);
        return nl_arc_or(pos[fl / 3], pos[(int)(t % un)], fl % 3 + 1, n);
    }
    return nl_arc_two(pos[(int)(key / un)], pos[(int)(key % un)], n);
}

// no position in both
TSP_ARC_HD bool nl_arc_disjoint(NlArc x, NlArc y, int n) {
    return arc_ahead(y.start, x.start, n) >= x.len && arc_ahead(x.start, y.start, n) >= y.len;
}

// position p lies in the arc
TSP_ARC_HD bool nl_arc_holds(NlArc x, int p, int n) { return arc_ahead(p, x.start, n) < x.len; }

}  // namespace tsp
