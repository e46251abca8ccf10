// nl3_opt.hip -- the 3-opt kind of the list descent (tsp_dev_nl_3opt).  The definitions are in include/tsp_hip.h.
//
// Decision k_nl_prep and k_nl_scan of nl_opt.hip (edge lengths; the 2-opt and Or-opt candidates) -> k_nl3_scan (one lane = one
//          list entry (p, u): with q = succ p it walks w over the list of q, and for each (u, w) the <= 4 choices of the removed
//          edges at u and at w; one (delta, key) per workgroup) -> k_nl3_pick_apply (the candidates of both scans, then the move
//          of whichever kind on order/pos; one workgroup per tour).
// A lane works on the six ends of the three removed edges ("slots": tail and head of a, b, c) and not on node ids, because a
// segment of one node puts two slots on one node.  Such a move has the same new edges as a second type with the segment
// reversed, and both are moves of the neighbourhood, so the lane offers both, each summed in its own order.
#include "nl_common.hpp"

#include <algorithm>

#pragma clang fp contract(off)

using namespace tsp;

namespace {

constexpr int kMaxN3 = 1 << 20;   // 4 n^3 must stay below the kind bits of the decision key

// two positions that hold different nodes which are not tour neighbours
__device__ __forceinline__ bool apart(int px, int py, int n) {
    int g = px - py;
    if (g < 0) g += n;
    return g != 0 && g != 1 && g != n - 1;
}

__device__ __forceinline__ int ahead(int px, int from, int n) {   // px - from mod n
    const int g = px - from;
    return g < 0 ? g + n : g;
}

__device__ __forceinline__ unsigned pair_slots(int s, int t) { return ((unsigned)t << (3 * s)) | ((unsigned)s << (3 * t)); }

__device__ __forceinline__ bool same_edge(int x, int y, int p, int u) { return (x == p && y == u) || (x == u && y == p); }

// One lane per list entry (p, k1), u = nbr[p][k1], q = succ p: the moves that remove (p, q) and add {p, u} and {q, w}, w in N(q).
template <int WT, bool INT>
__global__ __launch_bounds__(256) void k_nl3_scan(const double2 *__restrict__ coord, const int *__restrict__ orders,
                                                  const int *__restrict__ poss, NlState *__restrict__ st, int n, int K,
                                                  const int *__restrict__ nbr, const double *__restrict__ Es,
                                                  NlBest *__restrict__ parts) {
    const int bt = blockIdx.y;
    if (st[bt].done) return;
    __shared__ double sd[4];
    __shared__ u64 sk[4];
    const int *order = orders + (size_t)bt * n, *pos = poss + (size_t)bt * n;
    const double *E = Es + (size_t)bt * n;
    double bd = INFINITY;
    u64 bk = kNoKey;
    unsigned cnt = 0;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < (long long)n * K) {
        const int p = (int)(t / K);
        const int u = nbr[t];
        const int pp = pos[p], pu = pos[u];
        if (apart(pp, pu, n)) {
            const int pq = or_wrap(pp + 1, n), q = order[pq];
            const double dk = dsym<WT, INT>(coord, p, u);
            const int puS = or_wrap(pu + 1, n), puP = or_wrap(pu - 1, n);
            const int uS = order[puS], uP = order[puP];
            const int *lq = nbr + (size_t)q * K;
            for (int k2 = 0; k2 < K; ++k2) {
                const int w = lq[k2];
                const int pw = pos[w];
                if (!apart(pq, pw, n)) continue;
                const double dqw = dsym<WT, INT>(coord, q, w);
                const int pwS = or_wrap(pw + 1, n), pwP = or_wrap(pw - 1, n);
                const int wS = order[pwS], wP = order[pwP];
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const int su = ch & 1, sw = ch >> 1;   // 0: the removed edge starts at u / w, 1: it ends there
                    const int tY = su ? uP : u, ptY = su ? puP : pu, hY = su ? u : uS;
                    const int tZ = sw ? wP : w, ptZ = sw ? pwP : pw, hZ = sw ? w : wS;
                    const int yo = su ? uP : uS, pyo = su ? puP : puS;   // the ends that the third new edge joins
                    const int zo = sw ? wP : wS, pzo = sw ? pwP : pwS;
                    if (ptY == pp || ptZ == pp || ptY == ptZ || !apart(pyo, pzo, n)) continue;
                    // roles 0, 1, 2 = a, b, c: a has the lowest tail, b and c follow it in tour order
                    const int pA = (p < tY && p < tZ) ? pp : (tY < tZ ? ptY : ptZ);
                    const int oX = ahead(pp, pA, n), oY = ahead(ptY, pA, n), oZ = ahead(ptZ, pA, n);
                    const int rX = (oY < oX) + (oZ < oX), rY = (oX < oY) + (oZ < oY), rZ = (oX < oZ) + (oY < oZ);
                    // the new edges as a matching of the slots role * 2 + (0 tail, 1 head)
                    const unsigned M = pair_slots(rX * 2, rY * 2 + su) | pair_slots(rX * 2 + 1, rZ * 2 + sw) |
                                       pair_slots(rY * 2 + 1 - su, rZ * 2 + 1 - sw);
                    const int m0 = M & 7, m1 = (M >> 3) & 7, m3 = (M >> 9) & 7, m4 = (M >> 12) & 7;
                    int T = -1;
                    if (m0 == 3) T = m4 == 1 ? 0 : (m4 == 2 ? 3 : -1);   // (a,b1): with (c,a1) type 0, with (c,b) type 3
                    else if (m0 == 2) T = m1 == 4 ? 1 : -1;              // (a,b) (a1,c)
                    else if (m0 == 4) T = m3 == 1 ? 2 : -1;              // (a,c) (b1,a1)
                    if (T < 0) continue;
                    const int a = rX == 0 ? p : (rY == 0 ? tY : tZ), a1 = rX == 0 ? q : (rY == 0 ? hY : hZ);
                    const int b = rX == 1 ? p : (rY == 1 ? tY : tZ), b1 = rX == 1 ? q : (rY == 1 ? hY : hZ);
                    const int c = rX == 2 ? p : (rY == 2 ? tY : tZ), c1 = rX == 2 ? q : (rY == 2 ? hY : hZ);
                    const int ob = rX == 1 ? oX : (rY == 1 ? oY : oZ), oc = rX == 2 ? oX : (rY == 2 ? oY : oZ);
                    const int s1 = ob, s2 = oc - ob, s3 = n - oc;
                    // a segment of one node: type 0 and the type that reverses that segment are the same new edges
                    int T2 = -1;
                    if (T == 0) T2 = s1 == 1 ? 3 : (s2 == 1 ? 2 : (s3 == 1 ? 1 : -1));
                    else if ((T == 3 && s1 == 1) || (T == 2 && s2 == 1) || (T == 1 && s3 == 1)) T2 = 0;
                    const double d3 = dsym<WT, INT>(coord, yo, zo);
                    const double old = (E[a] + E[b]) + E[c];
                    const u64 key0 = (((u64)a * (u64)n + (u64)b) * (u64)n + (u64)c) * 4ull;
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const int Tq = r ? T2 : T;
                        if (Tq < 0) continue;
                        // (e1, e2, e3) of the type; each is one of the lane's three edges
                        const int x1 = a, y1 = Tq == 1 ? b : (Tq == 2 ? c : b1);
                        const int x2 = Tq == 1 ? a1 : (Tq == 2 ? b1 : c), y2 = Tq == 0 ? a1 : (Tq == 1 ? c : (Tq == 2 ? a1 : b));
                        const int x3 = Tq == 1 ? b1 : (Tq == 3 ? a1 : b), y3 = c1;
                        const double e1 = same_edge(x1, y1, p, u) ? dk : (same_edge(x1, y1, q, w) ? dqw : d3);
                        const double e2 = same_edge(x2, y2, p, u) ? dk : (same_edge(x2, y2, q, w) ? dqw : d3);
                        const double e3 = same_edge(x3, y3, p, u) ? dk : (same_edge(x3, y3, q, w) ? dqw : d3);
                        const double delta = ((e1 + e2) + e3) - old;
                        cnt += 1;
                        nl_offer(delta, kNl3Bit | (key0 + (u64)Tq), bd, bk);
                    }
                }
            }
        }
    }
    block_argmin<true>(bd, bk, sd, sk);
    if (threadIdx.x == 0) parts[(size_t)bt * gridDim.x + blockIdx.x] = NlBest{bd, bk};
    unsigned long long c64 = cnt;
    for (int off = 32; off > 0; off >>= 1) c64 += __shfl_down(c64, off);
    if ((threadIdx.x & 63) == 0 && c64) atomicAdd((unsigned long long *)&st[bt].deltas, c64);
}

// Decision over the candidates of k_nl_scan (parts2) and k_nl3_scan (parts3; either may be NULL: no kind of it is enabled), then
// the move.  One workgroup per tour.
__global__ __launch_bounds__(kNlPickThreads) void k_nl3_pick_apply(int *__restrict__ orders, int *__restrict__ poss,
                                                                   NlState *__restrict__ st, int n, int nparts,
                                                                   const NlBest *__restrict__ parts2,
                                                                   const NlBest *__restrict__ parts3) {
    constexpr int NT = kNlPickThreads;
    const int bt = blockIdx.x;
    NlState &S = st[bt];
    if (S.done) return;
    __shared__ double sd[NT / 64];
    __shared__ u64 sk[NT / 64];
    const int tid = threadIdx.x;
    if (S.max_moves >= 0 && S.moves >= S.max_moves) {
        if (tid == 0) S.done = 1;
        return;
    }
    double bd = INFINITY; u64 bk = kNoKey;
    for (int h = 0; h < 2; ++h) {
        const NlBest *part = h ? parts3 : parts2;
        if (!part) continue;
        part += (size_t)bt * nparts;
        for (int r = tid; r < nparts; r += NT) {
            const NlBest q = part[r];
            if (q.k != kNoKey && better(q.d, q.k, bd, bk)) { bd = q.d; bk = q.k; }
        }
    }
    block_argmin<true>(bd, bk, sd, sk);
    __syncthreads();
    if (tid == 0) { S.decisions += 1; if (bk == kNoKey) S.done = 1; }
    if (bk == kNoKey) return;
    int *order = orders + (size_t)bt * n, *pos = poss + (size_t)bt * n;
    if (bk & kNl3Bit) {
        const u64 key = bk & (kNl3Bit - 1);
        const int T = (int)(key & 3);
        const u64 abc = key >> 2;
        const int c = (int)(abc % (u64)n), b = (int)((abc / (u64)n) % (u64)n), a = (int)(abc / ((u64)n * (u64)n));
        const int pa = pos[a];
        const int s1 = ahead(pos[b], pa, n), s2 = ahead(pos[c], pa, n) - s1;
        const int at1 = or_wrap(pa + 1, n), at2 = or_wrap(at1 + s1, n);   // where S1 = a1 .. b and S2 = b1 .. c start
        __syncthreads();   // every thread has read the tour before anything moves
        if (tid == 0) {
            S.moves += 1; S.moves_3opt += 1; S.moves_type[T] += 1;
            if (S.max_moves >= 0 && S.moves >= S.max_moves) S.done = 1;
        }
        if (T <= 1) {          // S1 and S2 each reversed; type 0: then the two together, which leaves S2 S1
            nl_reverse_path<NT>(order, pos, n, at1, s1);
            nl_reverse_path<NT>(order, pos, n, at2, s2);
            if (T == 0) {
                __syncthreads();
                nl_reverse_path<NT>(order, pos, n, at1, s1 + s2);
            }
        } else {               // the two together (S2' S1'), then its second part (type 2: S2' S1) or its first (type 3: S2 S1')
            nl_reverse_path<NT>(order, pos, n, at1, s1 + s2);
            __syncthreads();
            if (T == 2) nl_reverse_path<NT>(order, pos, n, or_wrap(at1 + s2, n), s1);
            else nl_reverse_path<NT>(order, pos, n, at1, s2);
        }
        return;
    }
    if (!(bk & kNlOrBit)) {
        // 2-opt: the forward path i1 .. j (positions pi + 1 .. pi + len) is reversed in place
        const int i = (int)(bk / (u64)n), j = (int)(bk % (u64)n);
        const int pi = pos[i];
        const int len = ahead(pos[j], pi, n);
        __syncthreads();
        if (tid == 0) {
            S.moves += 1; S.moves_2opt += 1; S.reversed += len - 1;   // the successors rewritten: all of the path but i1's
            if (S.max_moves >= 0 && S.moves >= S.max_moves) S.done = 1;
        }
        nl_reverse_path<NT>(order, pos, n, or_wrap(pi + 1, n), len);
        return;
    }
    const u64 key = bk & (kNlOrBit - 1);
    const int o = (int)(key & 1);
    const u64 t = key >> 1;
    const int a = (int)(t % (u64)n);
    const int fl = (int)(t / (u64)n);
    const int L = fl % 3 + 1, f = fl / 3;
    const int i = pos[f], ja = pos[a];
    int x[3] = {0, 0, 0};
    for (int q = 0; q < L; ++q) x[q] = order[or_wrap(i + q, n)];
    __syncthreads();   // every thread has read the tour before anything moves
    if (tid == 0) {
        S.moves += 1; S.moves_oropt += 1; S.moves_len[L - 1] += 1; S.moves_rev += o;
        if (S.max_moves >= 0 && S.moves >= S.max_moves) S.done = 1;
    }
    or_shift_apply<NT>(order, pos, n, i, ja, L, o, x);
}

void launch_decision3(tsp_dev_tours *t, NlData *x, int kinds) {
    tsp_dev_inst *inst = t->inst;
    hipStream_t s = inst->ctx->stream;
    const int n = t->n, B = t->B;
    const bool low = kinds & (TSP_NL_2OPT | TSP_NL_OROPT), three = kinds & TSP_NL_3OPT;
    NlBest *parts3 = x->d_part + (size_t)B * x->nparts;
    tsp_nl_launch_scan(t, x, kinds);
    if (three) {
        TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
            hipLaunchKernelGGL((k_nl3_scan<WTC, INTC>), dim3(x->nparts, B), dim3(256), 0, s, inst->d_coord, t->d_order, t->d_pos,
                               x->d_st, n, x->K, x->d_nbr, x->d_E, parts3);
        });
    }
    hipLaunchKernelGGL(k_nl3_pick_apply, dim3(B), dim3(kNlPickThreads), 0, s, t->d_order, t->d_pos, x->d_st, n, x->nparts,
                       low ? x->d_part : nullptr, three ? parts3 : nullptr);
}

}  // namespace

extern "C" {

int tsp_dev_nl_3opt(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                    int64_t max_moves, double time_limit_s, tsp_nl3_opt_stats *stats) {
    if (!inst || !succ || !obj || B < 1 || succ_stride < 1) return TSP_DEV_E_ARG;
    if (kinds < 1 || kinds > (TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT)) return TSP_DEV_E_ARG;
    const int n = inst->n;
    if ((kinds & TSP_NL_3OPT) && n > kMaxN3) return TSP_DEV_E_ARG;
    if (B > 1 && tour_stride < (int64_t)n * succ_stride) return TSP_DEV_E_ARG;
    // a kind without any move at this size is left out: 2-opt needs four nodes, Or-opt and 3-opt five
    if (n < 4) kinds &= ~TSP_NL_2OPT;
    if (n < 5) kinds &= ~(TSP_NL_OROPT | TSP_NL_3OPT);
    NlData *x = nullptr;
    double t0 = 0.0;
    float ms = 0.f;
    const int status = tsp_nl_descend(inst, kinds, launch_decision3, B, succ, succ_stride, tour_stride, obj, max_moves,
                                      time_limit_s, &x, &t0, &ms);
    if (status != TSP_OK && status != TSP_TIME_LIMIT_EXCEEDED) return status;
    for (int b = 0; b < B && stats; ++b) {
        const NlState &z = x->h_st[b];
        tsp_nl3_opt_stats &o = stats[b];
        memset(&o, 0, sizeof o);
        o.decisions = z.decisions; o.moves = z.moves; o.moves_2opt = z.moves_2opt; o.moves_oropt = z.moves_oropt;
        for (int q = 0; q < 3; ++q) o.moves_by_len[q] = z.moves_len[q];
        o.moves_reversed = z.moves_rev; o.reversed = z.reversed; o.deltas_executed = z.deltas;
        o.seconds = tsp_nl_wall_s() - t0; o.device_ms = ms;
        o.moves_3opt = z.moves_3opt;
        for (int q = 0; q < 4; ++q) o.moves_by_type[q] = z.moves_type[q];
    }
    return status;
}

}  // extern "C"
