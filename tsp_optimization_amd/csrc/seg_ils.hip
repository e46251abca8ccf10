// seg_ils.hip -- windowed iterated local search (tsp_dev_seg_ils, tsp_dev_seg_ils3, tsp_dev_seg_ils_groups, tsp_dev_seg_ils_lk;
// DESIGN.md 4.20 - 4.23).
// The definitions are in include/tsp_hip.h.
//
// Launch   k_seg_ils, one per iteration: grid (windows, chains), one workgroup = the T trials of one window of W consecutive tour
//          nodes.  The window lives in LDS under "home" ids, the slot a node had when the kernel loaded it: seq (home id per slot),
//          lpos (slot per home id), node (node per home id), the incumbent copy of seq, the edge lengths E, the active list (two
//          copies, a decision compacts one into the other) with its bitmap and the hit flags.  A node's home id is the incumbent's
//          global pos minus the window's first position, mod n: below W or not decides "is a window node", and global pos is not
//          written before the trials are over.  Kick, moves and restore are permutations of a slot interval (seg_permute) followed
//          by the edge lengths of that interval; a trial keeps the hull of its intervals and copies or restores nothing else.
//          rem of an Or-opt segment is taken from E and one distance, in k_nl_prep's order, rather than kept per slot.
//          With the 3-opt kind (k_seg_ils<.., true>) a decision also deals one lane per (p, u, w) of the active nodes p, and a
//          3-opt move is the slot permutation of seg_move3.hpp.
//          With groups (k_seg_ils<.., .., true>, tsp_dev_seg_ils_groups) the grid is (windows * G, chains): workgroup w * G + g runs
//          the T trials of group g of window w on stream index w * G + g and writes no order / pos.  It leaves a record {offer,
//          lo, hi, gain; the node ids of slots lo .. hi} in scratch, and k_seg_commit, one workgroup per (window, chain) behind it
//          on the stream, copies the intervals that commit by the rule of seg_groups.hpp.  No workgroup waits for another.
//          With the chain kind (k_seg_ils<.., true, true, true>, tsp_dev_seg_ils_lk when kinds has TSP_NL_LK) a decision also runs
//          the two chains of every active node, one chain per group of 16 lanes and 16 chains side by side; a chain is the list
//          of its reversals (seg_lk.hpp) in 128 bytes of LDS, and the chain that wins is one slot permutation of its hull.
// Host     Descent::run queues the launches and looks at the clock between its batches; nothing is read per launch.
#include "descent.hpp"
#include "ils_common.hpp"
#include "nl_common.hpp"
#include "seg_groups.hpp"
#include "seg_lk.hpp"
#include "seg_move3.hpp"

#include <cstddef>

#pragma clang fp contract(off)

using namespace tsp;

namespace {

constexpr int kSegThreads = 256;
using u16 = unsigned short;
static_assert(TSP_SEG_ILS_MAX_WINDOW <= 65536, "slots and home ids are 16-bit");
static_assert(TSP_SEG_ILS_MAX_GROUPS <= 64, "one lane of one wave per group decides a window's commits");
// a group's record: ints 0 .. 2 = offer, lo, hi, ints 4 .. 5 = gain (fp64), then the node id of slot k at int kSegRecHead + k
constexpr int kSegRecHead = 8;
// a chain's key: both kind bits above 2 t1 + s, so that a chain is the last kind in the order (delta, kind, key)
constexpr u64 kSegLkBits = kNlOrBit | kNl3Bit;
constexpr int kSegLkGroups = kSegThreads / kSegLkLanes;          // chains side by side
constexpr int kSegLkRec = kSegLkMaxDepth + 3 * kSegLkMaxDepth;   // a chain in LDS: its j, then e, y, p of every step (home ids)
static_assert(kSegLkMaxDepth == TSP_SEG_LK_MAX_DEPTH && kSegLkLanes == TSP_NL_MAX_K, "seg_lk.hpp follows include/tsp_hip.h");

__host__ __device__ __forceinline__ int seg_round8(int W) { return (W + 7) & ~7; }
// entries of the cost tree behind its first level: P / 2, P the next power of two >= W - 1; its bytes also stage a permutation
__host__ __device__ __forceinline__ int seg_tree_len(int W) {
    int P = 8;
    while (P < W - 1) P *= 2;
    const int ids = seg_round8(W) / 4;
    return P / 2 > ids ? P / 2 : ids;
}
size_t seg_lds_bytes(int W) { return (size_t)24 * seg_round8(W) + (size_t)8 * seg_tree_len(W); }

struct SegWin {
    double *E, *tree;
    int *node;
    u16 *seq, *inc, *lpos, *alist;   // alist: two lists of W8 ids, one behind the other
    unsigned char *act, *hit;
};

// k_nl3_scan's helpers (nl3_opt.hip) over window slots: two slots that hold different nodes which are not tour neighbours
__device__ __forceinline__ bool seg_apart(int px, int py) { return px - py > 1 || py - px > 1; }
__device__ __forceinline__ unsigned seg_pair_slots(int s, int t) { return ((unsigned)t << (3 * s)) | ((unsigned)s << (3 * t)); }
__device__ __forceinline__ bool seg_same_edge(int x, int y, int p, int u) { return (x == p && y == u) || (x == u && y == p); }

// What a lane of the scan reads the window through: NlView's two / oro / roles and k_nl3_scan's lane over slots, a move kept only
// when every edge it removes is a window edge (the tails at slots 0 .. W - 2) and, Or-opt, its segment is a window path.
template <int WT, bool INT>
struct SegView {
    const double2 *coord;
    SegWin w;
    int n, W;
    double bd;
    u64 bk;
    unsigned cnt;
    bool found;

    __device__ __forceinline__ int at(int p) const { return w.node[w.seq[p]]; }
    __device__ __forceinline__ double d(int u, int v) const { return dsym<WT, INT>(coord, u, v); }
    __device__ __forceinline__ void take(double delta, u64 key) {
        cnt += 1;
        if (delta < 0.0) {
            found = true;
            if (better(delta, key, bd, bk)) { bd = delta; bk = key; }
        }
    }

    __device__ __forceinline__ void two(int x, int px, int y, int py, int known, double dk) {
        if (px < 0 || py < 0 || px > W - 2 || py > W - 2) return;
        if (x > y) { int t = x; x = y; y = t; t = px; px = py; py = t; }
        const int i1 = at(px + 1), j1 = at(py + 1);
        if (y == i1 || j1 == x) return;
        const double dij = known == 0 ? dk : d(x, y), d11 = known == 1 ? dk : d(i1, j1);
        take(((dij + d11) - w.E[px]) - w.E[py], (u64)x * (u64)n + (u64)y);
    }

    __device__ __forceinline__ void oro(int f, int pf, int L, int a, int pa, int o, int known, double dk) {
        if (pf < 1 || pf + L > W - 1 || pa < 0 || pa > W - 2) return;   // p, s and b are window nodes
        if (pa >= pf - 1 && pa <= pf + L - 1) return;                     // a in {p, f .. l}
        const int l = at(pf + L - 1), bb = at(pa + 1);
        const double d1 = known == 0 ? dk : (o ? d(a, l) : d(a, f));
        const double d2 = known == 1 ? dk : (o ? d(f, bb) : d(l, bb));
        const double rem = (w.E[pf - 1] + w.E[pf + L - 1]) - d(at(pf - 1), at(pf + L));
        take(((d1 + d2) - w.E[pa]) - rem, kNlOrBit | or_key(f, L, a, o, n));
    }

    __device__ __forceinline__ void roles(int x, int px, int y, int py, double dk) {
        const int pa = py - 1;
        const int a = pa >= 0 ? at(pa) : 0;
#pragma unroll
        for (int L = 1; L <= 3; ++L) {
            oro(y, py, L, x, px, 0, 0, dk);
            const int pf = px - (L - 1);
            if (pf >= 0 && pa >= 0) oro(at(pf), pf, L, a, pa, 0, 1, dk);
            if (L > 1) {
                const int pg = py - (L - 1);
                if (pg >= 0) oro(at(pg), pg, L, x, px, 1, 0, dk);
                if (pa >= 0) oro(x, px, L, a, pa, 1, 1, dk);
            }
        }
    }

    // k_nl3_scan's lane (nl3_opt.hip) for one w of the list of q = succ p, over slots: the moves that remove (p, q) and add {p, u}
    // and {q, w}; pos is the slot, order[] is at(), E[node] is E[the tail's slot].  p is a tail (pp <= W - 2), u and w are window
    // nodes.  Two window slots differ by what their positions differ by (W <= n - 1), so the cyclic differences stay mod n.
    __device__ __forceinline__ void three(int p, int pp, int u, int pu, int wn, int pw, double dk) {
        const int pq = pp + 1, q = at(pq);
        if (!seg_apart(pp, pu) || !seg_apart(pq, pw)) return;
        const double dqw = d(q, wn);
        // the neighbours of u and w inside the window (a choice that needs another one is no window move)
        const int uP = pu >= 1 ? at(pu - 1) : 0, uS = pu <= W - 2 ? at(pu + 1) : 0;
        const int wP = pw >= 1 ? at(pw - 1) : 0, wS = pw <= W - 2 ? at(pw + 1) : 0;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const int su = ch & 1, sw = ch >> 1;   // 0: the removed edge starts at u / w, 1: it ends there
            if ((su ? pu < 1 : pu > W - 2) || (sw ? pw < 1 : pw > W - 2)) continue;   // the tail is at slot -1 or W - 1
            const int tY = su ? uP : u, ptY = su ? pu - 1 : pu, hY = su ? u : uS;
            const int tZ = sw ? wP : wn, ptZ = sw ? pw - 1 : pw, hZ = sw ? wn : wS;
            const int yo = su ? uP : uS, pyo = su ? pu - 1 : pu + 1;   // the ends that the third new edge joins
            const int zo = sw ? wP : wS, pzo = sw ? pw - 1 : pw + 1;
            if (ptY == pp || ptZ == pp || ptY == ptZ || !seg_apart(pyo, pzo)) continue;
            // roles 0, 1, 2 = a, b, c: a has the lowest tail, b and c follow it in tour order
            const int pA = (p < tY && p < tZ) ? pp : (tY < tZ ? ptY : ptZ);
            const int oX = ahead(pp, pA, n), oY = ahead(ptY, pA, n), oZ = ahead(ptZ, pA, n);
            const int rX = (oY < oX) + (oZ < oX), rY = (oX < oY) + (oZ < oY), rZ = (oX < oZ) + (oY < oZ);
            // the new edges as a matching of the slots role * 2 + (0 tail, 1 head)
            const unsigned M = seg_pair_slots(rX * 2, rY * 2 + su) | seg_pair_slots(rX * 2 + 1, rZ * 2 + sw) |
                               seg_pair_slots(rY * 2 + 1 - su, rZ * 2 + 1 - sw);
            const int m0 = M & 7, m1 = (M >> 3) & 7, m3 = (M >> 9) & 7, m4 = (M >> 12) & 7;
            int T = -1;
            if (m0 == 3) T = m4 == 1 ? 0 : (m4 == 2 ? 3 : -1);   // (a,b1): with (c,a1) type 0, with (c,b) type 3
            else if (m0 == 2) T = m1 == 4 ? 1 : -1;              // (a,b) (a1,c)
            else if (m0 == 4) T = m3 == 1 ? 2 : -1;              // (a,c) (b1,a1)
            if (T < 0) continue;
            const int a = rX == 0 ? p : (rY == 0 ? tY : tZ), a1 = rX == 0 ? q : (rY == 0 ? hY : hZ);
            const int b = rX == 1 ? p : (rY == 1 ? tY : tZ), b1 = rX == 1 ? q : (rY == 1 ? hY : hZ);
            const int c = rX == 2 ? p : (rY == 2 ? tY : tZ), c1 = rX == 2 ? q : (rY == 2 ? hY : hZ);
            const int pB = rX == 1 ? pp : (rY == 1 ? ptY : ptZ), pC = rX == 2 ? pp : (rY == 2 ? ptY : ptZ);
            const int ob = rX == 1 ? oX : (rY == 1 ? oY : oZ), oc = rX == 2 ? oX : (rY == 2 ? oY : oZ);
            const int s1 = ob, s2 = oc - ob, s3 = n - oc;
            // a segment of one node: type 0 and the type that reverses that segment are the same new edges
            int T2 = -1;
            if (T == 0) T2 = s1 == 1 ? 3 : (s2 == 1 ? 2 : (s3 == 1 ? 1 : -1));
            else if ((T == 3 && s1 == 1) || (T == 2 && s2 == 1) || (T == 1 && s3 == 1)) T2 = 0;
            const double d3 = d(yo, zo);
            const double old = (w.E[pA] + w.E[pB]) + w.E[pC];
            const u64 key0 = nl3_key(a, b, c, 0, n);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int Tq = r ? T2 : T;
                if (Tq < 0) continue;
                // (e1, e2, e3) of the type; each is one of the lane's three edges
                const int x1 = a, y1 = Tq == 1 ? b : (Tq == 2 ? c : b1);
                const int x2 = Tq == 1 ? a1 : (Tq == 2 ? b1 : c), y2 = Tq == 0 ? a1 : (Tq == 1 ? c : (Tq == 2 ? a1 : b));
                const int x3 = Tq == 1 ? b1 : (Tq == 3 ? a1 : b), y3 = c1;
                const double e1 = seg_same_edge(x1, y1, p, u) ? dk : (seg_same_edge(x1, y1, q, wn) ? dqw : d3);
                const double e2 = seg_same_edge(x2, y2, p, u) ? dk : (seg_same_edge(x2, y2, q, wn) ? dqw : d3);
                const double e3 = seg_same_edge(x3, y3, p, u) ? dk : (seg_same_edge(x3, y3, q, wn) ? dqw : d3);
                take(((e1 + e2) + e3) - old, kNl3Bit | (key0 + (u64)Tq));
            }
        }
    }
};

// What a chain (seg_lk.hpp) reads the window through, in home ids.
template <int WT, bool INT>
struct SegLkView {
    const double2 *coord;
    const int *nbr, *pos;
    SegWin w;
    int n, W, K, p0;

    __device__ __forceinline__ int entry(int e, int k) const {
        const int hu = ahead(pos[nbr[(size_t)w.node[e] * K + k]], p0, n);
        return hu < W ? hu : -1;
    }
    __device__ __forceinline__ int slot(int id) const { return w.lpos[id]; }
    __device__ __forceinline__ int at(int p) const { return w.seq[p]; }
    __device__ __forceinline__ double d(int a, int b) const { return dsym<WT, INT>(coord, w.node[a], w.node[b]); }
};

// chain(r, s) of at most D steps by the kSegLkLanes lanes of a group: lane gl tests entry gl of a step, the group folds by
// (g2, k), and every lane carries the chain on.  rec: the group's kSegLkRec ids, written by all its lanes with the same values.
// -> false: r has no first edge on this side.
template <typename V>
__device__ __forceinline__ bool seg_lk_chain(const V &v, int r, int s, int D, u16 *rec, int gl, SegLkChain &c) {
    const int i = seglk_side(s, v.W, v.slot(r));
    seglk_begin(c, 0);
    if (i > v.W - 2) return false;
    c.e = v.at(seglk_side(s, v.W, i + 1));
    u16 *js = rec, *es = rec + kSegLkMaxDepth;
    while (c.h < D) {
        const double x = v.d(r, c.e);
        SegLkPick pk;
        pk.g2 = -INFINITY; pk.k = kSegLkLanes; pk.j = 0; pk.y = 0; pk.p = 0;
        if (gl < v.K) pk = seglk_entry(v, s, i, js, es, c, x, gl);
        SegLkPick win = pk;
#pragma unroll
        for (int m = kSegLkLanes / 2; m >= 1; m >>= 1) {
            const double og = __shfl_xor(win.g2, m, kSegLkLanes);
            const int ok = __shfl_xor(win.k, m, kSegLkLanes);
            if (seglk_beats(og, ok, win.g2, win.k)) { win.g2 = og; win.k = ok; }
        }
        if (win.k >= kSegLkLanes) break;
        win.j = __shfl(pk.j, win.k, kSegLkLanes); win.y = __shfl(pk.y, win.k, kSegLkLanes); win.p = __shfl(pk.p, win.k, kSegLkLanes);
        seglk_take(c, win, v.d(win.p, r), js, es);
    }
    return true;
}

// Slots lo .. hi take the home ids of the slots src(k), a permutation of lo .. hi.  By every thread; `stage` holds hi - lo + 1 ids.
template <typename Src>
__device__ __forceinline__ void seg_permute(const SegWin &w, u16 *stage, int lo, int hi, Src src) {
    const int tid = threadIdx.x;
    for (int k = lo + tid; k <= hi; k += kSegThreads) stage[k - lo] = w.seq[src(k)];
    __syncthreads();
    for (int k = lo + tid; k <= hi; k += kSegThreads) {
        const u16 r = stage[k - lo];
        w.seq[k] = r; w.lpos[r] = (u16)k;
    }
    __syncthreads();
}

// E of the slots lo .. hi that have one.  By every thread, behind the barrier that follows the last write of seq.
template <int WT, bool INT>
__device__ __forceinline__ void seg_edges(const double2 *coord, const SegWin &w, int W, int lo, int hi) {
    lo = max(lo, 0); hi = min(hi, W - 2);
    for (int k = lo + (int)threadIdx.x; k <= hi; k += kSegThreads)
        w.E[k] = dsym<WT, INT>(coord, w.node[w.seq[k]], w.node[w.seq[k + 1]]);
    __syncthreads();
}

// The window cost of include/tsp_hip.h: the halving tree over E padded with +0.0 to P entries.  By every thread; every thread gets it.
__device__ __forceinline__ double seg_cost(const SegWin &w, int W) {
    const int tid = threadIdx.x;
    int P = 8;
    while (P < W - 1) P *= 2;
    int h = P / 2;
    for (int k = tid; k < h; k += kSegThreads) {
        const double hi = k + h < W - 1 ? w.E[k + h] : 0.0;
        w.tree[k] = w.E[k] + hi;   // k < P / 2 < W - 1
    }
    __syncthreads();
    for (h /= 2; h >= 1; h /= 2) {
        for (int k = tid; k < h; k += kSegThreads) w.tree[k] += w.tree[k + h];   // entries k + h >= h are only read at this level
        __syncthreads();
    }
    const double c = w.tree[0];
    __syncthreads();   // the tree's bytes stage the next permutation
    return c;
}

struct SegArgs {
    int n, K, kinds, W, S, T;
    long long cap;   // < 0: none
    u64 seed;
    long long it;
    int G;      // groups per window (k_seg_ils<.., .., true> and k_seg_commit)
    int D;      // steps of a chain at most (k_seg_ils<.., .., .., true>)
    int *rec;   // their records: (chain, window, group) major, seg_round8(W) + kSegRecHead ints each
    u64 *lk;    // the chain kind's counters, four per tsp chain: moves, flips, chains, steps
};

// K3: with the 3-opt kind (tsp_dev_seg_ils3 when kinds has TSP_NL_3OPT); without it no 3-opt code is compiled.
// GR: a workgroup is one group of a window (tsp_dev_seg_ils_groups): it ends with a record in place of order / pos.
// LK: with the chain kind (tsp_dev_seg_ils_lk when kinds has TSP_NL_LK); without it no chain code is compiled.
template <int WT, bool INT, bool K3, bool GR = false, bool LK = false>
__global__ __launch_bounds__(kSegThreads) void k_seg_ils(const double2 *__restrict__ coord, int *__restrict__ orders,
                                                         int *__restrict__ poss, const int *__restrict__ nbr,
                                                         NlState *__restrict__ st, u64 *__restrict__ acc, SegArgs g) {
    extern __shared__ double seg_lds[];
    __shared__ double s_d[kSegThreads / 64];
    __shared__ u64 s_k[kSegThreads / 64];
    __shared__ int s_na, s_cnt;
    const int tid = threadIdx.x, b = blockIdx.y;
    const int sx = blockIdx.x;                 // the index of the workgroup's draws: w, with groups w * G + g
    const int wi = GR ? sx / g.G : sx;
    const int n = g.n, W = g.W, S = g.S, K = g.K, W8 = seg_round8(W);
    int *order = orders + (size_t)b * n, *pos = poss + (size_t)b * n;
    SegWin w;
    w.E = seg_lds; w.tree = w.E + W8;
    w.node = reinterpret_cast<int *>(w.tree + seg_tree_len(W));
    w.seq = reinterpret_cast<u16 *>(w.node + W8); w.inc = w.seq + W8; w.lpos = w.inc + W8;
    w.alist = w.lpos + W8;
    w.act = reinterpret_cast<unsigned char *>(w.alist + 2 * W8); w.hit = w.act + W8;
    u16 *stage = reinterpret_cast<u16 *>(w.tree);
    u16 *lk_rec = nullptr;   // LK: kSegLkRec ids per group of lanes; the chain that is applied is worked out again into the first
    int *lk_h = nullptr;     // LK: its best prefix
    if constexpr (LK) {
        __shared__ u16 s_lk[kSegLkGroups * kSegLkRec];
        __shared__ int s_lkh;
        lk_rec = s_lk; lk_h = &s_lkh;
    }

    const u64 base = ils_base(g.seed, b, g.it);
    const int s = (int)(ils_mix(base) % (u64)n);
    int p0 = (int)(((long long)pos[s] + (long long)wi * W) % n);   // pos[s]: the anchor is slot 0 of window 0 and keeps its position
    for (int k = tid; k < W; k += kSegThreads) {
        w.node[k] = order[or_wrap(p0 + k, n)];
        w.seq[k] = w.inc[k] = w.lpos[k] = (u16)k;
        w.act[k] = w.hit[k] = 0;
    }
    __syncthreads();
    seg_edges<WT, INT>(coord, w, W, 0, W - 2);
    double c0 = seg_cost(w, W);
    const double c_start = c0;

    SegView<WT, INT> view;
    view.coord = coord; view.w = w; view.n = n; view.W = W; view.cnt = 0;
    // the same values in every thread; thread 0 adds them to the chain's
    long long decisions = 0, moves_all = 0, m2 = 0, mor = 0, ml1 = 0, ml2 = 0, ml3 = 0, mrev = 0, reversed = 0, active = 0, accepted = 0;
    long long m3 = 0, mt[4] = {0, 0, 0, 0};   // K3
    long long mlk = 0, flips = 0;             // LK
    unsigned lk_chains = 0, lk_steps = 0;     // LK: of the chains this thread led
    SegLkView<WT, INT> lkv;
    if constexpr (LK) { lkv.coord = coord; lkv.nbr = nbr; lkv.pos = pos; lkv.w = w; lkv.n = n; lkv.W = W; lkv.K = K; lkv.p0 = p0; }
    // the slot of a window node
    auto slot_of = [&](int v) { return (int)w.lpos[ahead(pos[v], p0, n)]; };

    for (int t = 0; t < g.T; ++t) {
        const u64 bw = ils_mix(base + 8 + (u64)sx * (u64)g.T + (u64)t);
        const int off = (int)(ils_mix(bw) % (u64)(W - S));
        const IlsCuts c = ils_cuts_from(0, S, ils_mix(bw + 1), ils_mix(bw + 2), ils_mix(bw + 3), ils_mix(bw + 4));
        const int o[4] = {c.o1, c.o2, c.o3, c.o4};
        int e[8];
#pragma unroll
        for (int q = 0; q < 4; ++q) { e[2 * q] = w.seq[off + o[q] - 1]; e[2 * q + 1] = w.seq[off + o[q]]; }   // off + o4 <= W - 1
        int ne = 8;   // ends of the kick, then of a move: 4 or 6
        int tlo = off + c.o1, thi = off + c.o4 - 1;   // the hull of what the trial has permuted
        {
            const int lD = c.o4 - c.o3, lC = c.o3 - c.o2, kb = off + c.o1;
            const int sB = off + c.o1, sC = off + c.o2, sD = off + c.o3;
            seg_permute(w, stage, tlo, thi, [=](int k) {
                const int q = k - kb;
                return q < lD ? sD + q : (q < lD + lC ? sC + (q - lD) : sB + (q - lD - lC));
            });
        }
        seg_edges<WT, INT>(coord, w, W, tlo - 1, thi);
        int cur = 0;
        if (tid == 0) {
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (!w.act[e[q]]) { w.act[e[q]] = 1; w.alist[cnt++] = (u16)e[q]; }   // single-node blocks name a node twice
            s_na = cnt;
        }
        __syncthreads();
        int na = s_na;
        long long moves = 0;
        while (g.cap < 0 || moves < g.cap) {
            decisions += 1; active += na;
            view.bd = INFINITY; view.bk = kNoKey;
            const u16 *list = w.alist + cur * W8;
            for (int ln = tid; ln < na * K; ln += kSegThreads) {
                const int r = list[ln / K];
                const int v = w.node[r], u = nbr[(size_t)v * K + (ln % K)];
                if (u == v) continue;
                const int hu = ahead(pos[u], p0, n);
                if (hu >= W) continue;   // a move over the entry (v, u) removes an edge at u
                const int pv = w.lpos[r], pu = w.lpos[hu];
                const double dk = view.d(v, u);
                view.found = false;
                if (g.kinds & TSP_NL_2OPT) {
                    view.two(v, pv, u, pu, 0, dk);
                    if (pv >= 1 && pu >= 1) view.two(view.at(pv - 1), pv - 1, view.at(pu - 1), pu - 1, 1, dk);
                }
                if (g.kinds & TSP_NL_OROPT) {
                    view.roles(v, pv, u, pu, dk);
                    view.roles(u, pu, v, pv, dk);
                }
                if (view.found) w.hit[r] = 1;
            }
            if constexpr (K3) {
                // one lane per (p, u, w): entry k1 of p's list and entry k2 of the list of q = succ p
                if (g.kinds & TSP_NL_3OPT)
                    for (int ln = tid; ln < na * K * K; ln += kSegThreads) {
                        const int r = list[ln / (K * K)], k1 = (ln / K) % K, k2 = ln % K;
                        const int pv = w.lpos[r];
                        if (pv > W - 2) continue;   // p is no tail
                        const int v = w.node[r], u = nbr[(size_t)v * K + k1];
                        const int hu = ahead(pos[u], p0, n);
                        if (hu >= W) continue;
                        const int x = nbr[(size_t)view.at(pv + 1) * K + k2];
                        const int hx = ahead(pos[x], p0, n);
                        if (hx >= W) continue;
                        view.found = false;
                        view.three(v, pv, u, w.lpos[hu], x, w.lpos[hx], view.d(v, u));
                        if (view.found) w.hit[r] = 1;
                    }
            }
            if constexpr (LK) {
                // chain 2 q + s is chain(list[q], s); kSegLkGroups of them at a time, the leader of a group reports
                if (g.kinds & TSP_NL_LK)
                    for (int c = tid / kSegLkLanes; c < 2 * na; c += kSegLkGroups) {
                        const int r = list[c >> 1], s = c & 1;
                        SegLkChain ch;
                        const bool first = seg_lk_chain(lkv, r, s, g.D, lk_rec + (tid / kSegLkLanes) * kSegLkRec, tid % kSegLkLanes, ch);
                        if (tid % kSegLkLanes == 0 && first) {
                            lk_chains += 1; lk_steps += (unsigned)ch.h;
                            if (ch.hstar >= 1) {
                                w.hit[r] = 1;
                                const u64 key = kSegLkBits | (2 * (u64)w.node[r] + (u64)s);
                                if (better(-ch.best, key, view.bd, view.bk)) { view.bd = -ch.best; view.bk = key; }
                            }
                        }
                    }
            }
            double bd = view.bd;
            u64 bk = view.bk;
            block_argmin<true>(bd, bk, s_d, s_k);   // (its barriers also stand between the hit flags and their readers)
            if (bk == kNoKey) break;                // no lane held an improving move: hit is all zero
            // the move in slots: lo .. hi are permuted, ends(m) as home ids from the window before the move
            int lo, hi;
            bool is3 = false;
            SegMove3 mv3 = {0, 0, 0, 0};
            bool isLK = false;
            int lkS = 0, lkI = 0, lkH = 0, lkR = 0;   // LK: the side, t1's chain slot, the best prefix, t1's home id
            if constexpr (LK) isLK = (bk & kSegLkBits) == kSegLkBits;
            if constexpr (K3) is3 = (bk & kNl3Bit) != 0 && !isLK;
            if constexpr (LK) {
                if (isLK) {
                    lkS = (int)(bk & 1);
                    lkR = ahead(pos[(int)((bk & (kNlOrBit - 1)) >> 1)], p0, n);
                    if (tid < kSegLkLanes) {
                        SegLkChain ch;
                        seg_lk_chain(lkv, lkR, lkS, g.D, lk_rec, tid, ch);
                        if (tid == 0) *lk_h = ch.hstar;
                    }
                    __syncthreads();
                    lkH = *lk_h;
                    lkI = seglk_side(lkS, W, w.lpos[lkR]);
                    const int top = seglk_hull_hi(lk_rec, lkH);   // the hull in chain slots: lkI + 1 .. top
                    lo = lkS ? W - 1 - top : lkI + 1; hi = lkS ? W - 2 - lkI : top;
                    ne = 0;
                    mlk += 1; flips += lkH;
                }
            }
            if (isLK) {
                // lo, hi and the ends are set above, behind the barrier of the chain worked out again
            } else if (is3) {
                const Nl3Move m = nl3_unkey(bk & (kNl3Bit - 1), n);
                const int type = m.type();
                mv3 = seg3_make(slot_of(m.a()), slot_of(m.b()), slot_of(m.c()), type);
                e[0] = w.seq[mv3.i]; e[1] = w.seq[mv3.i + 1]; e[2] = w.seq[mv3.j]; e[3] = w.seq[mv3.j + 1];
                e[4] = w.seq[mv3.k]; e[5] = w.seq[mv3.k + 1];
                ne = 6;
                lo = mv3.i + 1; hi = mv3.k;
                m3 += 1; mt[type] += 1;
            } else if (!(bk & kNlOrBit)) {
                const int px = slot_of((int)(bk / (u64)n)), py = slot_of((int)(bk % (u64)n));
                lo = min(px, py) + 1; hi = max(px, py);
                e[0] = w.seq[lo - 1]; e[1] = w.seq[lo]; e[2] = w.seq[hi]; e[3] = w.seq[hi + 1];
                ne = 4;
                m2 += 1; reversed += hi - lo + 1;
            } else {
                const OrMove mv = or_unkey(bk & (kNlOrBit - 1), n);
                const int pf = slot_of(mv.f), pa = slot_of(mv.a), L = mv.L;
                e[0] = w.seq[pf - 1]; e[1] = w.seq[pf]; e[2] = w.seq[pf + L - 1]; e[3] = w.seq[pf + L];
                e[4] = w.seq[pa]; e[5] = w.seq[pa + 1];
                ne = 6;
                lo = pa > pf ? pf : pa + 1; hi = pa > pf ? pa : pf + L - 1;
                mor += 1; ml1 += L == 1; ml2 += L == 2; ml3 += L == 3; mrev += mv.o;
            }
            // A: the listed nodes with a hit, then the ends that are not among them
            if (tid == 0) s_cnt = 0;
            __syncthreads();
            u16 *next = w.alist + (cur ^ 1) * W8;
            for (int q = tid; q < na; q += kSegThreads) {
                const int r = list[q];
                if (w.hit[r]) { w.hit[r] = 0; next[atomicAdd(&s_cnt, 1)] = (u16)r; }
                else w.act[r] = 0;
            }
            __syncthreads();
            if (tid == 0) {
                int cnt = s_cnt;
#pragma unroll
                for (int q = 0; q < 6; ++q)
                    if (q < ne && !w.act[e[q]]) { w.act[e[q]] = 1; next[cnt++] = (u16)e[q]; }
                if constexpr (LK) {
                    if (isLK) {   // t1, then e, y, p of the steps kept
                        if (!w.act[lkR]) { w.act[lkR] = 1; next[cnt++] = (u16)lkR; }
                        for (int q = 0; q < 3 * lkH; ++q) {
                            const u16 x = lk_rec[kSegLkMaxDepth + q];
                            if (!w.act[x]) { w.act[x] = 1; next[cnt++] = x; }
                        }
                    }
                }
                s_na = cnt;
            }
            if (isLK) {
                if constexpr (LK) {
                    const u16 *js = lk_rec;
                    seg_permute(w, stage, lo, hi, [=](int k) {
                        return seglk_side(lkS, W, seglk_inv(lkI, js, lkH, seglk_side(lkS, W, k)));
                    });
                }
            } else if (is3) {
                seg_permute(w, stage, lo, hi, [=](int k) { return seg3_src(mv3, k); });
            } else if (!(bk & kNlOrBit)) {
                const int sum = lo + hi;
                seg_permute(w, stage, lo, hi, [=](int k) { return sum - k; });
            } else {
                const OrMove mv = or_unkey(bk & (kNlOrBit - 1), n);
                const int pf = slot_of(mv.f), pa = slot_of(mv.a), L = mv.L, o = mv.o;
                // where the segment lands, and by how much the slots between it and the insertion point shift
                const int land = pa > pf ? pa - L + 1 : pa + 1, shift = pa > pf ? L : -L;
                seg_permute(w, stage, lo, hi, [=](int k) {
                    const int q = k - land;
                    return q >= 0 && q < L ? (o ? pf + L - 1 - q : pf + q) : k + shift;
                });
            }
            seg_edges<WT, INT>(coord, w, W, lo - 1, hi);
            tlo = min(tlo, lo); thi = max(thi, hi);
            cur ^= 1;
            na = s_na;   // written ahead of seg_permute's barriers
            moves += 1;
        }
        moves_all += moves;
        for (int q = tid; q < na; q += kSegThreads) w.act[w.alist[cur * W8 + q]] = 0;   // also what a descent ended by the cap left
        const double c1 = seg_cost(w, W);   // (its barriers stand between the bitmap and the next trial's list)
        if (c1 < c0) {
            for (int k = tlo + tid; k <= thi; k += kSegThreads) w.inc[k] = w.seq[k];
            c0 = c1;
            accepted += 1;
            __syncthreads();
        } else {
            for (int k = tlo + tid; k <= thi; k += kSegThreads) {
                const u16 r = w.inc[k];
                w.seq[k] = r; w.lpos[r] = (u16)k;
            }
            __syncthreads();
            seg_edges<WT, INT>(coord, w, W, tlo - 1, thi);
        }
    }
    if constexpr (GR) {
        int *rec = g.rec + ((size_t)b * gridDim.x + (size_t)sx) * (size_t)(W8 + kSegRecHead);
        if (accepted) {
            // an accepted trial made the window cheaper, so some slot holds another home id than its own
            if (tid == 0) { s_na = W; s_cnt = -1; }
            __syncthreads();
            int lo = W, hi = -1;
            for (int k = tid; k < W; k += kSegThreads)
                if (w.inc[k] != k) { lo = min(lo, k); hi = max(hi, k); }
            if (hi >= 0) { atomicMin(&s_na, lo); atomicMax(&s_cnt, hi); }
            __syncthreads();
            lo = s_na; hi = s_cnt;   // 1 <= lo <= hi <= W - 2: no trial permutes slot 0 or W - 1
            for (int k = lo + tid; k <= hi; k += kSegThreads) rec[kSegRecHead + k] = w.node[w.inc[k]];
            if (tid == 0) {
                rec[0] = 1; rec[1] = lo; rec[2] = hi;
                *reinterpret_cast<double *>(rec + 4) = c0 - c_start;
            }
        } else if (tid == 0) {
            rec[0] = 0;
        }
    } else if (accepted) {
        for (int k = tid; k < W; k += kSegThreads) {
            const int v = w.node[w.inc[k]], p = or_wrap(p0 + k, n);
            order[p] = v; pos[v] = p;
        }
    }
    NlState &Z = st[b];
    auto add = [](long long &to, long long x) { if (x) atomicAdd((unsigned long long *)&to, (unsigned long long)x); };
    if (tid == 0) {
        add(Z.decisions, decisions); add(Z.moves, moves_all); add(Z.moves_2opt, m2); add(Z.moves_oropt, mor);
        add(Z.moves_len[0], ml1); add(Z.moves_len[1], ml2); add(Z.moves_len[2], ml3);
        add(Z.moves_rev, mrev); add(Z.reversed, reversed); add(Z.active_nodes, active);
        if constexpr (K3) {
            add(Z.moves_3opt, m3);
            for (int q = 0; q < 4; ++q) add(Z.moves_type[q], mt[q]);
        }
        if (accepted) atomicAdd(&acc[b], (u64)accepted);
        if constexpr (LK) {
            if (mlk) { atomicAdd(&g.lk[4 * b], (u64)mlk); atomicAdd(&g.lk[4 * b + 1], (u64)flips); }
        }
    }
    if constexpr (LK) {
        if (lk_chains) { atomicAdd(&g.lk[4 * b + 2], (u64)lk_chains); atomicAdd(&g.lk[4 * b + 3], (u64)lk_steps); }
    }
    unsigned long long cnt = view.cnt;
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((tid & 63) == 0) add(Z.deltas, (long long)cnt);
}

// Behind k_seg_ils<.., .., true> on the stream: grid (windows, chains).  One lane per group reads the G headers of the window and
// decides by seg_groups.hpp; the intervals of the committing groups, pairwise disjoint and each a permutation of itself, go to
// order / pos.  grp[2 b], grp[2 b + 1]: the chain's offers and commits.
__global__ __launch_bounds__(kSegThreads) void k_seg_commit(int *__restrict__ orders, int *__restrict__ poss,
                                                            u64 *__restrict__ grp, SegArgs g) {
    __shared__ SegOffer s_o[TSP_SEG_ILS_MAX_GROUPS];
    __shared__ int s_c[TSP_SEG_ILS_MAX_GROUPS];
    const int tid = threadIdx.x, wi = blockIdx.x, b = blockIdx.y;
    const int n = g.n, W = g.W, G = g.G;
    const size_t stride = (size_t)(seg_round8(W) + kSegRecHead);
    int *order = orders + (size_t)b * n, *pos = poss + (size_t)b * n;
    const int *recs = g.rec + ((size_t)b * gridDim.x + (size_t)wi) * (size_t)G * stride;
    if (tid < G) {
        const int *h = recs + (size_t)tid * stride;
        SegOffer o;
        o.offer = h[0]; o.lo = h[1]; o.hi = h[2];
        o.gain = *reinterpret_cast<const double *>(h + 4);
        s_o[tid] = o;
    }
    __syncthreads();
    if (tid < G) s_c[tid] = segg_commits(s_o, G, tid) ? 1 : 0;
    __syncthreads();
    const int s = (int)(ils_mix(ils_base(g.seed, b, g.it)) % (u64)n);
    const int p0 = (int)(((long long)pos[s] + (long long)wi * W) % n);   // the anchor is slot 0 of window 0: nobody writes its pos
    int offers = 0, commits = 0;
    for (int q = 0; q < G; ++q) {
        offers += s_o[q].offer;
        if (!s_c[q]) continue;
        commits += 1;
        const int *ids = recs + (size_t)q * stride + kSegRecHead;
        for (int k = s_o[q].lo + tid; k <= s_o[q].hi; k += kSegThreads) {
            const int v = ids[k], p = or_wrap(p0 + k, n);
            order[p] = v; pos[v] = p;
        }
    }
    if (tid == 0) {
        if (offers) atomicAdd(&grp[2 * b], (u64)offers);
        if (commits) atomicAdd(&grp[2 * b + 1], (u64)commits);
    }
}

// Descent::run ends when every iteration has been queued (and, behind its poll, carried out).
struct SegHooks : DescentPlain {
    const long long *queued;
    long long iterations;
    bool finished(const NlState &, int) const { return *queued >= iterations; }
};

}  // namespace

static_assert(offsetof(tsp_seg_ils_stats, iterations) == sizeof(tsp_nl_opt_stats), "tsp_seg_ils_stats starts as tsp_nl_opt_stats");
static_assert(offsetof(tsp_seg_ils3_stats, moves_3opt) == sizeof(tsp_seg_ils_stats), "tsp_seg_ils3_stats starts as tsp_seg_ils_stats");

static_assert(offsetof(tsp_seg_ils_groups_stats, groups) == sizeof(tsp_seg_ils3_stats),
              "tsp_seg_ils_groups_stats starts as tsp_seg_ils3_stats");
static_assert(offsetof(tsp_seg_ils_lk_stats, lk_depth) == sizeof(tsp_seg_ils_groups_stats) &&
                  sizeof(tsp_seg_ils_lk_stats) == sizeof(tsp_seg_ils_groups_stats) + 40,
              "tsp_seg_ils_lk_stats starts as tsp_seg_ils_groups_stats");

// What the entry points do.  `allowed` is the kinds mask the entry point takes; the B records are `stride` bytes apart and
// start as tsp_seg_ils_stats, with3: they are tsp_seg_ils3_stats.  grouped: tsp_dev_seg_ils_groups with its `groups`, the records
// are tsp_seg_ils_groups_stats.  lk_depth > 0: tsp_dev_seg_ils_lk with that D, the records are tsp_seg_ils_lk_stats; the chain kernel
// runs only when kinds has TSP_NL_LK, else the launches are those of tsp_dev_seg_ils_groups.
static int seg_run(tsp_dev_inst *inst, int kinds, int allowed, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                   uint64_t seed, int64_t iterations, int window, int span, int trials, int64_t max_moves_per_trial,
                   double time_limit_s, void *stats, size_t stride, bool with3, bool grouped = false, int groups = 1,
                   int lk_depth = 0) {
    int rc = tsp_nl_check(inst, &kinds, allowed, B, succ, succ_stride, tour_stride, obj);
    if (rc) return rc;
    if (iterations < 0 || trials < 1) return TSP_DEV_E_ARG;
    if (grouped && groups > TSP_SEG_ILS_MAX_GROUPS) return TSP_DEV_E_ARG;
    const int n = inst->n;
    const bool none = n < 10;   // no window
    int W = 0, S = 0;
    if (!none) {
        const int top = std::min(TSP_SEG_ILS_MAX_WINDOW, n - 1);
        W = window <= 0 ? std::min(TSP_SEG_ILS_DEFAULT_WINDOW, n - 1) : window;
        if (W < 9 || W > top) return TSP_DEV_E_ARG;
        S = span <= 0 ? W - 1 : span;
        if (S < 8 || S > W - 1) return TSP_DEV_E_ARG;
    }
    const long long I = none ? 0 : iterations, M = none ? 0 : n / W;
    // the default fills the 256 CUs x 4 resident workgroups of the kernel; a function of n and W only
    const long long G = !grouped ? 1 : (groups >= 1 ? groups : (none ? 1 : std::max(1LL, std::min((long long)TSP_SEG_ILS_MAX_GROUPS, 1024 / M))));
    Descent run;
    rc = run.open(inst, B, succ, succ_stride, tour_stride, obj);
    if (rc) return rc;
    NlData *x = nullptr;
    rc = tsp_nl_prepare(inst, B, &x);
    if (rc) return rc;
    hipStream_t s = inst->ctx->stream;
    tsp_dev_tours *t = run.t;
    if (!x->d_seg_acc) TSP_HIP_TRY(hipMalloc(&x->d_seg_acc, sizeof(u64) * B));
    TSP_HIP_TRY(hipMemsetAsync(x->d_seg_acc, 0, sizeof(u64) * B, s));
    const size_t rec_len = grouped ? (size_t)B * (size_t)M * (size_t)G * (size_t)(seg_round8(W) + kSegRecHead) : 0;
    if (grouped) {
        if (!x->d_seg_grp) TSP_HIP_TRY(hipMalloc(&x->d_seg_grp, sizeof(u64) * 2 * B));
        TSP_HIP_TRY(hipMemsetAsync(x->d_seg_grp, 0, sizeof(u64) * 2 * B, s));
        if (rec_len > x->seg_rec_len) {
            (void)hipFree(x->d_seg_rec);
            x->d_seg_rec = nullptr; x->seg_rec_len = 0;
            TSP_HIP_TRY(hipMalloc(&x->d_seg_rec, sizeof(int) * rec_len));
            x->seg_rec_len = rec_len;
        }
    }
    const bool chains = lk_depth > 0 && (kinds & TSP_NL_LK);
    if (chains) {
        if (!x->d_seg_lk) TSP_HIP_TRY(hipMalloc(&x->d_seg_lk, sizeof(u64) * 4 * B));
        TSP_HIP_TRY(hipMemsetAsync(x->d_seg_lk, 0, sizeof(u64) * 4 * B, s));
    }
    std::vector<double> start((size_t)B);
    if (int e = tsp_grid_tour_cost(t, x->d_cost)) return e;
    TSP_HIP_TRY(hipMemcpyAsync(start.data(), x->d_cost, sizeof(double) * B, hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipStreamSynchronize(s));
    SegArgs g;
    g.n = n; g.K = x->K; g.kinds = kinds; g.W = W; g.S = S; g.T = trials;
    g.cap = max_moves_per_trial < 0 ? -1 : max_moves_per_trial; g.seed = seed; g.it = 0;
    g.G = (int)G; g.rec = grouped ? x->d_seg_rec : nullptr;
    g.D = lk_depth; g.lk = chains ? x->d_seg_lk : nullptr;
    long long queued = 0;
    SegHooks hooks;
    hooks.queued = &queued; hooks.iterations = I;
    const size_t lds = none ? 0 : seg_lds_bytes(W);
    const int status = run.run(x->d_st, x->h_st, x->d_cost, I == 0, 256, -1, time_limit_s,
                               [&](bool) {
                                   if (queued >= I) return;
                                   g.it = queued++;
                                   TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
                                       if (chains)
                                           hipLaunchKernelGGL((k_seg_ils<WTC, INTC, true, true, true>), dim3((unsigned)(M * G), B),
                                                              dim3(kSegThreads), lds, s, inst->d_coord, t->d_order, t->d_pos, x->d_nbr,
                                                              x->d_st, x->d_seg_acc, g);
                                       else if (grouped && (kinds & TSP_NL_3OPT))
                                           hipLaunchKernelGGL((k_seg_ils<WTC, INTC, true, true>), dim3((unsigned)(M * G), B),
                                                              dim3(kSegThreads), lds, s, inst->d_coord, t->d_order, t->d_pos, x->d_nbr,
                                                              x->d_st, x->d_seg_acc, g);
                                       else if (grouped)
                                           hipLaunchKernelGGL((k_seg_ils<WTC, INTC, false, true>), dim3((unsigned)(M * G), B),
                                                              dim3(kSegThreads), lds, s, inst->d_coord, t->d_order, t->d_pos, x->d_nbr,
                                                              x->d_st, x->d_seg_acc, g);
                                       else if (kinds & TSP_NL_3OPT)
                                           hipLaunchKernelGGL((k_seg_ils<WTC, INTC, true>), dim3((unsigned)M, B), dim3(kSegThreads), lds,
                                                              s, inst->d_coord, t->d_order, t->d_pos, x->d_nbr, x->d_st, x->d_seg_acc, g);
                                       else
                                           hipLaunchKernelGGL((k_seg_ils<WTC, INTC, false>), dim3((unsigned)M, B), dim3(kSegThreads), lds,
                                                              s, inst->d_coord, t->d_order, t->d_pos, x->d_nbr, x->d_st, x->d_seg_acc, g);
                                   });
                                   if (grouped)
                                       hipLaunchKernelGGL(k_seg_commit, dim3((unsigned)M, B), dim3(kSegThreads), 0, s, t->d_order,
                                                          t->d_pos, x->d_seg_grp, g);
                               },
                               hooks);
    if (status != TSP_OK && status != TSP_TIME_LIMIT_EXCEEDED) return status;
    std::vector<u64> acc((size_t)B, 0);
    TSP_HIP_TRY(hipMemcpy(acc.data(), x->d_seg_acc, sizeof(u64) * B, hipMemcpyDeviceToHost));
    std::vector<u64> grp((size_t)2 * B, 0);
    if (grouped) TSP_HIP_TRY(hipMemcpy(grp.data(), x->d_seg_grp, sizeof(u64) * 2 * B, hipMemcpyDeviceToHost));
    std::vector<u64> lk((size_t)4 * B, 0);
    if (chains) TSP_HIP_TRY(hipMemcpy(lk.data(), x->d_seg_lk, sizeof(u64) * 4 * B, hipMemcpyDeviceToHost));
    const double seconds = wall_s() - run.t0;
    for (int b = 0; b < B && stats; ++b) {
        tsp_seg_ils_stats &o = *reinterpret_cast<tsp_seg_ils_stats *>(static_cast<char *>(stats) + (size_t)b * stride);
        tsp_nl_write_stats(NlStatsOut{&o, sizeof o, 0}, 0, x->h_st[b], nullptr, 0.0, seconds, run.device_ms);
        o.iterations = queued; o.windows = M; o.trials = queued * M * G * trials; o.accepted = (int64_t)acc[b];
        o.active_nodes = x->h_st[b].active_nodes; o.start_cost = start[b];
        if (with3) {
            tsp_seg_ils3_stats &o3 = reinterpret_cast<tsp_seg_ils3_stats &>(o);
            o3.moves_3opt = x->h_st[b].moves_3opt;
            for (int k = 0; k < 4; ++k) o3.moves_by_type[k] = x->h_st[b].moves_type[k];
        }
        if (grouped) {
            tsp_seg_ils_groups_stats &og = reinterpret_cast<tsp_seg_ils_groups_stats &>(o);
            og.groups = G; og.offers = (int64_t)grp[2 * b]; og.commits = (int64_t)grp[2 * b + 1];
        }
        if (lk_depth > 0) {
            tsp_seg_ils_lk_stats &ol = reinterpret_cast<tsp_seg_ils_lk_stats &>(o);
            ol.lk_depth = lk_depth; ol.moves_lk = (int64_t)lk[4 * b]; ol.lk_flips = (int64_t)lk[4 * b + 1];
            ol.lk_chains = (int64_t)lk[4 * b + 2]; ol.lk_steps = (int64_t)lk[4 * b + 3];
        }
    }
    return status;
}

extern "C" {

int tsp_dev_seg_ils(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj, uint64_t seed,
                    int64_t iterations, int window, int span, int trials, int64_t max_moves_per_trial, double time_limit_s,
                    tsp_seg_ils_stats *stats) {
    return seg_run(inst, kinds, TSP_NL_2OPT | TSP_NL_OROPT, B, succ, succ_stride, tour_stride, obj, seed, iterations, window, span,
                   trials, max_moves_per_trial, time_limit_s, stats, sizeof *stats, false);
}

int tsp_dev_seg_ils3(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj, uint64_t seed,
                     int64_t iterations, int window, int span, int trials, int64_t max_moves_per_trial, double time_limit_s,
                     tsp_seg_ils3_stats *stats) {
    return seg_run(inst, kinds, TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT, B, succ, succ_stride, tour_stride, obj, seed, iterations,
                   window, span, trials, max_moves_per_trial, time_limit_s, stats, sizeof *stats, true);
}

int tsp_dev_seg_ils_groups(tsp_dev_inst *inst, int kinds, int groups, int B, int *succ, int succ_stride, int64_t tour_stride,
                           double *obj, uint64_t seed, int64_t iterations, int window, int span, int trials,
                           int64_t max_moves_per_trial, double time_limit_s, tsp_seg_ils_groups_stats *stats) {
    return seg_run(inst, kinds, TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT, B, succ, succ_stride, tour_stride, obj, seed, iterations,
                   window, span, trials, max_moves_per_trial, time_limit_s, stats, sizeof *stats, true, true, groups);
}

int tsp_dev_seg_ils_lk(tsp_dev_inst *inst, int kinds, int lk_depth, int groups, int B, int *succ, int succ_stride, int64_t tour_stride,
                       double *obj, uint64_t seed, int64_t iterations, int window, int span, int trials,
                       int64_t max_moves_per_trial, double time_limit_s, tsp_seg_ils_lk_stats *stats) {
    if (lk_depth > TSP_SEG_LK_MAX_DEPTH) return TSP_DEV_E_ARG;
    return seg_run(inst, kinds, TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT | TSP_NL_LK, B, succ, succ_stride, tour_stride, obj, seed,
                   iterations, window, span, trials, max_moves_per_trial, time_limit_s, stats, sizeof *stats, true, true, groups,
                   lk_depth <= 0 ? TSP_SEG_LK_DEFAULT_DEPTH : lk_depth);
}

}  // extern "C"
