// exh_decide.hpp -- the rule by which an exhaustive sweep's move is decided from candidates that name their pairs by tour
// POSITION (two_opt_exh.hpp), free of HIP: k_move_pos and k_exh_close compile exactly this text for the device,
// tests/test_cpu_exh_decide.py compiles it with the host compiler and checks it against a brute-force arg-min.
//
// The decision is the arg-min of (delta, (i, j)), i < j the NODE IDS of the pair (tabusearch.c:151 keeps the first pair in
// (i < j) order among the minimal deltas).  The ids matter in two places only: the tie-break among different pairs that share the
// minimal delta, which is rare, and the orientation of the move (the position of the smaller id is pa).  k_exh therefore leaves
// one candidate {delta, p, q} per workgroup, p < q tour positions, and never asks for an id unless two different pairs tie inside
// the workgroup (one thread folds its four waves by steps 1 and 4); whoever decides
//   1. folds its candidates by (delta, position key) and remembers whether two DIFFERENT pairs shared its best delta (exh_fold);
//   2. takes the block's arg-min of (delta, position key);
//   3. calls the sweep ambiguous if some thread's best delta equals the block's and its flag is set or its pair is another one
//      (exh_ambiguous, OR-ed over the block).  Not ambiguous: one pair holds the minimal delta, whatever its ids -- decided;
//   4. ambiguous: every candidate at the minimal delta gets its two ids and the arg-min of make_key(min id, max id) decides
//      (exh_fold_ids; a thread goes over ALL its candidates again: its fold of step 1 kept one pair per thread);
//   5. orients the move by the ids at p and q (exh_orient).
// The same pair in several slots (strip 0 overlaps strip 1) is one pair: never ambiguous by itself.
#pragma once
#include "exh_arith.hpp"

namespace tsp {

typedef unsigned long long exh_u64;
constexpr exh_u64 kExhNoPair = ~0ull;

// what a workgroup of k_exh leaves: its best pair by position, p < q; p = -1: none (delta then means nothing)
struct alignas(16) ExhCand {
    int delta, p, q, pad;
};

TSP_EXH_HD exh_u64 exh_pair_key(int a, int b) {   // (a, b) lexicographic; a < 0: no pair
    return a < 0 ? kExhNoPair : (((exh_u64)(unsigned)a << 32) | (exh_u64)(unsigned)b);
}
TSP_EXH_HD int exh_key_hi(exh_u64 k) { return (int)(k >> 32); }
TSP_EXH_HD int exh_key_lo(exh_u64 k) { return (int)(k & 0xffffffffu); }

// step 1: a thread's best by (delta, position key); `tie`: two different pairs share `delta`
struct ExhBest {
    int delta = 0;
    exh_u64 key = kExhNoPair;
    int tie = 0;
};
TSP_EXH_HD void exh_fold(ExhBest &b, const ExhCand &c) {   // (selects, no branches: several of these in a row per thread)
    const exh_u64 k = exh_pair_key(c.p, c.q);
    const bool lower = c.p >= 0 && (b.key == kExhNoPair || c.delta < b.delta);
    const bool other = c.p >= 0 && !lower && c.delta == b.delta && k != b.key;
    b.tie = lower ? 0 : (other ? 1 : b.tie);
    b.key = lower || (other && k < b.key) ? k : b.key;
    b.delta = lower ? c.delta : b.delta;
}

// step 3: this thread's word of the OR, given the block's arg-min (delta, position key)
TSP_EXH_HD bool exh_ambiguous(const ExhBest &b, int delta, exh_u64 key) {
    return b.key != kExhNoPair && b.delta == delta && (b.tie != 0 || b.key != key);
}

// step 4: a thread's best by id key among its candidates at the minimal delta; id_at(position) = the node there
struct ExhIdBest {
    exh_u64 idkey = kExhNoPair, poskey = kExhNoPair;
};
template <class IdAt>
TSP_EXH_HD void exh_fold_ids(ExhIdBest &b, const ExhCand &c, int delta, IdAt id_at) {
    if (c.p < 0 || c.delta != delta) return;
    const int i = id_at(c.p), j = id_at(c.q);
    const exh_u64 k = exh_pair_key(i < j ? i : j, i < j ? j : i);
    if (k < b.idkey) { b.idkey = k; b.poskey = exh_pair_key(c.p, c.q); }
}

// step 5: the move of the pair at positions p < q.  The reference reverses what lies between its nodes i < j, from succ(i) to
// j: pa is the position of the smaller id.  p_first: id(p) < id(q).  The L positions pa1 .. pa1 + L - 1 (cyclic) are reversed.
struct ExhMove {
    int pa, pb, pa1, L;
};
TSP_EXH_HD ExhMove exh_orient(int p, int q, int n, bool p_first) {
    ExhMove m;
    m.pa = p_first ? p : q;
    m.pb = p_first ? q : p;
    m.L = p_first ? q - p : n - (q - p);
    m.pa1 = m.pa + 1 == n ? 0 : m.pa + 1;
    return m;
}

}  // namespace tsp
