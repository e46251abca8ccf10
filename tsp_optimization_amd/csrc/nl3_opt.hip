// nl3_opt.hip -- the 3-opt kind of the list descent (tsp_dev_nl_3opt).  The definitions are in include/tsp_hip.h.
//
// Decision k_nl_prep and k_nl_scan of nl_opt.hip (edge lengths; the 2-opt and Or-opt candidates) -> k_nl3_scan (one lane = one
//          list entry (p, u): with q = succ p it walks w over the list of q, and for each (u, w) the <= 4 choices of the removed
//          edges at u and at w; one (delta, key) per workgroup) -> k_nl_pick_apply of nl_opt.hip (the candidates of both scans,
//          then the move of whichever kind on order/pos; one workgroup per tour).
// A lane works on the six ends of the three removed edges ("slots": tail and head of a, b, c) and not on node ids, because a
// segment of one node puts two slots on one node.  Such a move has the same new edges as a second type with the segment
// reversed, and both are moves of the neighbourhood, so the lane offers both, each summed in its own order.
// The two entry points are a mode check, the NlStatsOut of their record type and tsp_nl_run (nl_opt.hip).
#include "nl_common.hpp"

#pragma clang fp contract(off)

using namespace tsp;

namespace {

// two positions that hold different nodes which are not tour neighbours
__device__ __forceinline__ bool apart(int px, int py, int n) {
    int g = px - py;
    if (g < 0) g += n;
    return g != 0 && g != 1 && g != n - 1;
}

__device__ __forceinline__ unsigned pair_slots(int s, int t) { return ((unsigned)t << (3 * s)) | ((unsigned)s << (3 * t)); }

__device__ __forceinline__ bool same_edge(int x, int y, int p, int u) { return (x == p && y == u) || (x == u && y == p); }

// One lane per list entry (p, k1), u = nbr[p][k1], q = succ p: the moves that remove (p, q) and add {p, u} and {q, w}, w in N(q).
// DLB: the lanes of the active nodes alone, as k_nl_scan<.., true> of nl_opt.hip maps and reports them.  PN: the per-node form,
// as k_nl_scan<.., false, true> (the owner of a lane is p).
template <int WT, bool INT, bool DLB, bool PN = false>
__global__ __launch_bounds__(256) void k_nl3_scan(const double2 *__restrict__ coord, const int *__restrict__ orders,
                                                  const int *__restrict__ poss, NlState *__restrict__ st, int n, int K,
                                                  const int *__restrict__ nbr, const double *__restrict__ Es,
                                                  NlBest *__restrict__ parts, NlDlb dlb, NlPn pn) {
    static_assert(!(DLB && PN), "the per-node form has no active sets");
    const int bt = blockIdx.y;
    if (st[bt].done) return;
    long long lanes = (long long)n * K;
    if constexpr (DLB) {
        lanes = (long long)st[bt].nact * K;
        if ((long long)blockIdx.x * blockDim.x >= lanes) return;
    }
    __shared__ double sd[4];
    __shared__ u64 sk[4];
    const int *order = orders + (size_t)bt * n, *pos = poss + (size_t)bt * n;
    const double *E = Es + (size_t)bt * n;
    double bd = INFINITY;
    u64 bk = kNoKey;
    unsigned cnt = 0;
    double cd = INFINITY;   // PN: the lane's best move of a short arc
    u64 ck = kNoKey;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool on = t < lanes;
    int p = (int)(t / K);
    long long e = t;
    if constexpr (PN) on = nl_pn_lane(n, K, &p, &e);
    if (on) {
        if constexpr (DLB) {
            e = t - (long long)p * K;
            p = dlb.list[(size_t)bt * n + p];
            e += (long long)p * K;
        }
        const int u = nbr[e];
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
                    const u64 key0 = nl3_key(a, b, c, 0, n);
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
                        offer(delta, kNl3Bit | (key0 + (u64)Tq), bd, bk);
                        if constexpr (PN)   // a .. c1: positions pA .. pA + oc + 1
                            if (arc_make(pA, oc + 2, n).len <= pn.max_arc) offer(delta, kNl3Bit | (key0 + (u64)Tq), cd, ck);
                    }
                }
            }
        }
        if constexpr (DLB)
            if (bk != kNoKey) dlb.hit[(size_t)bt * n + p] = 1;
    }
    if constexpr (PN) {
        __shared__ double pd[256];
        __shared__ u64 pk[256];
        nl_pn_reduce(cd, ck, on, K, p, pn.cand + (size_t)bt * n, pn.merge, pd, pk);
    }
    block_argmin<true>(bd, bk, sd, sk);
    if (threadIdx.x == 0) parts[(size_t)bt * gridDim.x + blockIdx.x] = NlBest{bd, bk};
    unsigned long long c64 = cnt;
    for (int off = 32; off > 0; off >>= 1) c64 += __shfl_down(c64, off);
    if ((threadIdx.x & 63) == 0 && c64) atomicAdd((unsigned long long *)&st[bt].deltas, c64);
}

}  // namespace

void tsp_nl3_launch_scan(tsp_dev_tours *t, NlData *x, NlBest *parts3, int dlb_mode) {
    tsp_dev_inst *inst = t->inst;
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        TSP_DISPATCH_DLB(dlb_mode, {
            hipLaunchKernelGGL((k_nl3_scan<WTC, INTC, DLBC>), dim3(x->nparts, t->B), dim3(256), 0, inst->ctx->stream, inst->d_coord,
                               t->d_order, t->d_pos, x->d_st, t->n, x->K, x->d_nbr, x->d_E, parts3, x->dlb(dlb_mode), NlPn{});
        });
    });
}

void tsp_nl3_launch_scan_pn(tsp_dev_tours *t, NlData *x, int nparts, NlBest *parts3, const NlPn &pn) {
    tsp_dev_inst *inst = t->inst;
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_nl3_scan<WTC, INTC, false, true>), dim3(nparts, t->B), dim3(256), 0, inst->ctx->stream, inst->d_coord,
                           t->d_order, t->d_pos, x->d_st, t->n, x->K, x->d_nbr, x->d_E, parts3, x->dlb(0), pn);
    });
}

extern "C" {

int tsp_dev_nl_3opt(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                    int64_t max_moves, double time_limit_s, tsp_nl3_opt_stats *stats) {
    return tsp_nl_run(inst, kinds, TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT, B, succ, succ_stride, tour_stride, obj, max_moves,
                      time_limit_s, NlStatsOut{stats, sizeof *stats, kNlStats3}, TSP_DLB_OFF, nullptr);
}

int tsp_dev_nl_3opt_dlb(tsp_dev_inst *inst, int kinds, int dlb_mode, int B, int *succ, int succ_stride, int64_t tour_stride,
                        double *obj, const unsigned char *active, int64_t max_moves, double time_limit_s, tsp_nl_dlb_stats *stats) {
    if (dlb_mode != TSP_DLB_OFF && dlb_mode != TSP_DLB_ON && dlb_mode != TSP_DLB_CLOSE) return TSP_DEV_E_ARG;
    return tsp_nl_run(inst, kinds, TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT, B, succ, succ_stride, tour_stride, obj, max_moves,
                      time_limit_s, NlStatsOut{stats, sizeof *stats, kNlStats3 | kNlStatsDlb}, dlb_mode, active);
}

}  // extern "C"
