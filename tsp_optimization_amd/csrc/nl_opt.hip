// nl_opt.hip -- candidate neighbour lists: the exact KNN build (tsp_dev_inst_knn_*) and the 2-opt + Or-opt descent over the
// list neighbourhood (tsp_dev_nl_opt).  The definitions are in include/tsp_hip.h.
//
// KNN      k_knn_scan (a row scan, row_scan.hpp: each lane keeps its 16 best (distance, id)) -> k_knn_merge (the first K ids stored).
// Decision k_nl_prep (per node: length of its tour edge, rem of the three segments that start at it) -> k_nl_scan (one
//          lane = one list entry (v, u): the 2 + 20 moves whose new / attaching edge is {v, u}; one (delta, kind, key) per
//          workgroup) -> k_nl_pick_apply (the workgroups' candidates, then the move on order/pos; one workgroup per tour).
// Every distance goes through dsym(): the lower node id first, so that a move reached through several (v, u, role)
// combinations has the same delta bits each time.  A 2-opt move always reverses the forward path i1 .. j in place, so that
// order/pos keep the orientation of succ and the Or-opt shift works unchanged.
// Host: tsp_nl_run is the body of every descent entry point of this file and of nl3_opt.hip (and of ils.hip below eight nodes);
// tsp_nl_write_stats fills the records of all five stats types, told by an NlStatsOut which groups a record has.
#include "descent.hpp"
#include "nl_common.hpp"
#include "row_scan.hpp"

#include <cstddef>

#pragma clang fp contract(off)

using namespace tsp;

namespace {

constexpr int kK = TSP_NL_MAX_K;     // k_knn_scan keeps this many per row whatever K is asked for: the K best are a prefix
constexpr int kKnnChunks = 16;       // k_knn_scan: most column chunks per row
constexpr int kKnnWaves = 4096;      // ... chosen so that about this many waves exist

// (d, id) into the sorted list; d == a held distance goes behind it (the callers offer equal distances in id order)
__device__ __forceinline__ void knn_insert(double (&kd)[kK], int (&ki)[kK], double d, int id) {
#pragma unroll
    for (int s = kK - 1; s >= 1; --s) {
        const bool shift = d < kd[s - 1], here = !shift && d < kd[s];
        kd[s] = shift ? kd[s - 1] : (here ? d : kd[s]);
        ki[s] = shift ? ki[s - 1] : (here ? id : ki[s]);
    }
    const bool first = d < kd[0];
    kd[0] = first ? d : kd[0];
    ki[0] = first ? id : ki[0];
}

// Row node v = one lane, columns [chunk * CH, chunk * CH + CH): pd / pi [(chunk * 16 + s) * n + v] = s-th best of the chunk
// (+inf, -1 where the chunk has fewer).  The column's coordinates are its record; the distance is taken row first (see pair_dist).
template <int WT, bool INT>
__global__ __launch_bounds__(256) void k_knn_scan(const double2 *__restrict__ coord, int n, int CH, double *__restrict__ pd,
                                                  int *__restrict__ pi) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int chunk = blockIdx.y;
    const int c0 = chunk * CH, c1 = min(n, c0 + CH);
    const double2 cv = coord[min(v, n - 1)];
    double kd[kK];
    int ki[kK];
#pragma unroll
    for (int s = 0; s < kK; ++s) { kd[s] = INFINITY; ki[s] = -1; }
    for (int c = c0; c < c1; ++c) {
        const double2 cc = coord[c];
        const double d = dist_xy<WT, INT>(cv.x, cv.y, cc.x, cc.y);
        if (d < kd[kK - 1] && c != v) knn_insert(kd, ki, d, c);
    }
    if (v >= n) return;
#pragma unroll
    for (int s = 0; s < kK; ++s) {
        const size_t at = ((size_t)chunk * kK + s) * n + v;
        pd[at] = kd[s]; pi[at] = ki[s];
    }
}

// nbr[v * K + s] = s-th best of row v over the chunks (taken in column order, so that equal distances stay in id order)
__global__ __launch_bounds__(256) void k_knn_merge(int n, int Cc, int K, const double *__restrict__ pd, const int *__restrict__ pi,
                                                   int *__restrict__ nbr) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    double kd[kK];
    int ki[kK];
#pragma unroll
    for (int s = 0; s < kK; ++s) { kd[s] = INFINITY; ki[s] = -1; }
    for (int c = 0; c < Cc; ++c)
        for (int s = 0; s < kK; ++s) {
            const size_t at = ((size_t)c * kK + s) * n + v;
            const int id = pi[at];
            if (id < 0) break;
            const double d = pd[at];
            if (d < kd[kK - 1]) knn_insert(kd, ki, d, id);
        }
#pragma unroll
    for (int s = 0; s < kK; ++s)
        if (s < K) nbr[(size_t)v * K + s] = ki[s];
}

// Per node v at position i: E[v] = d(v, succ v), rem[(L-1) * n + v] of the segment of L nodes that starts at v.
template <int WT, bool INT>
__global__ void k_nl_prep(const double2 *__restrict__ coord, const int *__restrict__ orders, const NlState *__restrict__ st,
                          int n, double *__restrict__ Es, double *__restrict__ rems) {
    const int b = blockIdx.y;
    if (st[b].done) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int *order = orders + (size_t)b * n;
    const int v = order[i];
    const int pm = order[or_wrap(i - 1, n)], v1 = order[or_wrap(i + 1, n)];
    const double dpf = dsym<WT, INT>(coord, pm, v);
    const double e0 = dsym<WT, INT>(coord, v, v1);
    Es[(size_t)b * n + v] = e0;
    if (n < 5) return;   // no Or-opt move
    double *rem = rems + (size_t)b * 3 * n;
    rem[v] = (dpf + e0) - dsym<WT, INT>(coord, pm, v1);
    const int v2 = order[or_wrap(i + 2, n)], v3 = order[or_wrap(i + 3, n)];
    rem[n + v] = (dpf + dsym<WT, INT>(coord, v1, v2)) - dsym<WT, INT>(coord, pm, v2);
    rem[2 * n + v] = (dpf + dsym<WT, INT>(coord, v2, v3)) - dsym<WT, INT>(coord, pm, v3);
}

// What a lane of k_nl_scan reads the tour through.  PN: the lane also keeps its best move of an arc of at most max_arc positions.
template <int WT, bool INT, bool PN = false>
struct NlView {
    const double2 *coord;
    const int *order, *pos;
    const double *E, *rem;
    int n;
    double bd;
    u64 bk;
    unsigned cnt;
    int max_arc;
    double cd;
    u64 ck;

    __device__ __forceinline__ int at(int p) const { return order[or_wrap(p, n)]; }
    __device__ __forceinline__ double d(int u, int v) const { return dsym<WT, INT>(coord, u, v); }

    // 2-opt move of the pair {x, y}; `known` says which new edge has the length dk: 0 = d(i,j), 1 = d(i1,j1)
    __device__ __forceinline__ void two(int x, int px, int y, int py, int known, double dk) {
        if (x > y) { int t = x; x = y; y = t; t = px; px = py; py = t; }
        const int i1 = at(px + 1), j1 = at(py + 1);
        if (y == i1 || j1 == x) return;
        const double dij = known == 0 ? dk : d(x, y), d11 = known == 1 ? dk : d(i1, j1);
        const double delta = ((dij + d11) - E[x]) - E[y];
        cnt += 1;
        offer(delta, (u64)x * (u64)n + (u64)y, bd, bk);
        if constexpr (PN)
            if (nl_arc_two(px, py, n).len <= max_arc) offer(delta, (u64)x * (u64)n + (u64)y, cd, ck);
    }

    // Or-opt move (f, L, a, o); `known` says which attaching edge has the length dk: 0 = the one at a, 1 = the one at b
    __device__ __forceinline__ void oro(int f, int pf, int L, int a, int pa, int o, int known, double dk) {
        int dj = pa - (pf - 1);   // in [-(n - 2), n]
        if (dj < 0) dj += n;
        else if (dj >= n) dj -= n;
        if (dj <= L) return;      // a in {p, f .. l}
        const int l = at(pf + L - 1), bb = at(pa + 1);
        const double d1 = known == 0 ? dk : (o ? d(a, l) : d(a, f));
        const double d2 = known == 1 ? dk : (o ? d(f, bb) : d(l, bb));
        const double delta = ((d1 + d2) - E[a]) - rem[(size_t)(L - 1) * n + f];
        cnt += 1;
        offer(delta, kNlOrBit | or_key(f, L, a, o, n), bd, bk);
        if constexpr (PN)
            if (nl_arc_or(pf, pa, L, n).len <= max_arc) offer(delta, kNlOrBit | or_key(f, L, a, o, n), cd, ck);
    }

    // the ten Or-opt moves that attach the segment with the edge x -> y (x ahead of y in the new tour)
    __device__ __forceinline__ void roles(int x, int px, int y, int py, double dk) {
        const int pa = or_wrap(py - 1, n), a = order[pa];
#pragma unroll
        for (int L = 1; L <= 3; ++L) {
            oro(y, py, L, x, px, 0, 0, dk);                              // (a, f) = (x, y)
            const int pf = or_wrap(px - (L - 1), n);
            oro(order[pf], pf, L, a, pa, 0, 1, dk);                      // (l, b) = (x, y)
            if (L > 1) {
                const int pg = or_wrap(py - (L - 1), n);
                oro(order[pg], pg, L, x, px, 1, 0, dk);                  // (a, l) = (x, y)
                oro(x, px, L, a, pa, 1, 1, dk);                          // (f, b) = (x, y)
            }
        }
    }
};

// One lane per list entry (v, k), u = nbr[v][k]: the moves whose new (2-opt) or attaching (Or-opt) edge is {v, u}.
// DLB: the same lanes of the active nodes alone, lane t = (slot t / K of the tour's list, k = t % K), on the same grid: a
// workgroup whose first lane lies beyond |A| K returns (and writes no candidate), and a lane that holds an improving move
// says so in hit[v].
// PN (without DLB): the per-node form of the batched descent, lanes as nl_pn_lane deals them, and behind the lane loop one
// candidate per node over the moves of a short arc (NlPn); the workgroup's overall candidate is written all the same.
template <int WT, bool INT, bool DLB, bool PN = false>
__global__ __launch_bounds__(256) void k_nl_scan(const double2 *__restrict__ coord, const int *__restrict__ orders,
                                                 const int *__restrict__ poss, NlState *__restrict__ st, int n, int K, int kinds,
                                                 const int *__restrict__ nbr, const double *__restrict__ Es,
                                                 const double *__restrict__ rems, NlBest *__restrict__ parts, NlDlb dlb,
                                                 NlPn pn) {
    static_assert(!(DLB && PN), "the per-node form has no active sets");
    const int b = blockIdx.y;
    if (st[b].done) return;
    long long lanes = (long long)n * K;
    if constexpr (DLB) {
        lanes = (long long)st[b].nact * K;
        if ((long long)blockIdx.x * blockDim.x >= lanes) return;
    }
    __shared__ double sd[4];
    __shared__ u64 sk[4];
    NlView<WT, INT, PN> w;
    w.coord = coord; w.order = orders + (size_t)b * n; w.pos = poss + (size_t)b * n;
    w.E = Es + (size_t)b * n; w.rem = rems + (size_t)b * 3 * n; w.n = n;
    w.bd = INFINITY; w.bk = kNoKey; w.cnt = 0;
    w.max_arc = pn.max_arc; w.cd = INFINITY; w.ck = kNoKey;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool on = t < lanes;
    int v = (int)(t / K);
    long long e = t;
    if constexpr (PN) on = nl_pn_lane(n, K, &v, &e);
    if (on) {
        if constexpr (DLB) {
            e = t - (long long)v * K;
            v = dlb.list[(size_t)b * n + v];
            e += (long long)v * K;
        }
        const int u = nbr[e];
        if (u != v) {
            const int pv = w.pos[v], pu = w.pos[u];
            const double dk = w.d(v, u);
            if (kinds & TSP_NL_2OPT) {
                w.two(v, pv, u, pu, 0, dk);                                      // {i, j} = {v, u}
                const int qv = or_wrap(pv - 1, n), qu = or_wrap(pu - 1, n);
                w.two(w.order[qv], qv, w.order[qu], qu, 1, dk);                  // {i1, j1} = {v, u}
            }
            if (kinds & TSP_NL_OROPT) {
                w.roles(v, pv, u, pu, dk);
                w.roles(u, pu, v, pv, dk);
            }
        }
        if constexpr (DLB)
            if (w.bk != kNoKey) dlb.hit[(size_t)b * n + v] = 1;
    }
    if constexpr (PN) {
        __shared__ double pd[256];
        __shared__ u64 pk[256];
        nl_pn_reduce(w.cd, w.ck, on, K, v, pn.cand + (size_t)b * n, pn.merge, pd, pk);
    }
    double bd = w.bd;
    u64 bk = w.bk;
    block_argmin<true>(bd, bk, sd, sk);
    if (threadIdx.x == 0) parts[(size_t)b * gridDim.x + blockIdx.x] = NlBest{bd, bk};
    unsigned long long cnt = w.cnt;
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd((unsigned long long *)&st[b].deltas, cnt);
}

// ends(m): the tails and heads of the edges that move `bk` removes, read from the tour before the move (scalars, not an array:
// they stay in registers)
struct NlEnds {
    int ne = 0;   // 0: no move
    int e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0, e5 = 0;
};
__device__ __forceinline__ NlEnds nl_move_ends(const int *__restrict__ order, const int *__restrict__ pos, int n, u64 bk) {
    NlEnds r;
    if (bk & kNl3Bit) {
        const u64 abc = (bk & (kNl3Bit - 1)) >> 2;   // nl3_unkey's divisions, written out: see profiles/nl3_lane_refactor.txt
        r.e0 = (int)(abc / ((u64)n * (u64)n)); r.e2 = (int)((abc / (u64)n) % (u64)n); r.e4 = (int)(abc % (u64)n);
        r.e1 = order[or_wrap(pos[r.e0] + 1, n)]; r.e3 = order[or_wrap(pos[r.e2] + 1, n)]; r.e5 = order[or_wrap(pos[r.e4] + 1, n)];
        r.ne = 6;
    } else if (!(bk & kNlOrBit)) {
        r.e0 = (int)(bk / (u64)n); r.e2 = (int)(bk % (u64)n);
        r.e1 = order[or_wrap(pos[r.e0] + 1, n)]; r.e3 = order[or_wrap(pos[r.e2] + 1, n)];
        r.ne = 4;
    } else {
        const OrMove mv = or_unkey(bk & (kNlOrBit - 1), n);
        const int pf = pos[mv.f];
        r.e0 = order[or_wrap(pf - 1, n)]; r.e1 = mv.f;
        r.e2 = order[or_wrap(pf + mv.L - 1, n)]; r.e3 = order[or_wrap(pf + mv.L, n)];
        r.e4 = mv.a; r.e5 = order[or_wrap(pos[mv.a] + 1, n)];
        r.ne = 6;
    }
    return r;
}

// The active set of one tour behind a decision that looked at its `na` nodes, by every thread of the workgroup (NT threads) that
// owns the tour.  With a move (its ends in e): the listed nodes without a hit leave A, the others keep their order at the
// front of the list (compacted in place: a chunk's writes lie at or below its own reads), then the ends that are not yet in A
// join.  Without one, in mode TSP_DLB_CLOSE and with A smaller than V: A = V.  hit is left all zero.
template <int NT>
__device__ __forceinline__ void nl_dlb_update(unsigned char *__restrict__ act, unsigned char *__restrict__ hit,
                                              int *__restrict__ list, NlState &S, int n, int na, int mode, const NlEnds &e,
                                              int *s_w) {
    const int tid = threadIdx.x;
    if (e.ne == 0) {   // no lane held an improving move: hit is all zero
        if (mode != TSP_DLB_CLOSE || na == n) return;
        for (int v = tid; v < n; v += NT) { act[v] = 1; list[v] = v; }
        if (tid == 0) { S.nact = n; S.closing_scans += 1; }
        return;
    }
    const int lane = tid & 63, wv = tid >> 6;
    int base = 0;
    for (int c0 = 0; c0 < na; c0 += NT) {
        const int slot = c0 + tid;
        int v = -1;
        bool keep = false;
        if (slot < na) {
            v = list[slot];
            keep = hit[v] != 0;
            hit[v] = 0;
            if (!keep) act[v] = 0;
        }
        const u64 m = __ballot(keep);
        if (lane == 0) s_w[wv] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int q = 0; q < NT / 64; ++q) {
            const int c = s_w[q];
            if (q < wv) off += c;
            base += c;
        }
        if (keep) list[off + __popcll(m & ((1ull << lane) - 1ull))] = v;
        __syncthreads();   // the next chunk rewrites s_w; the bitmap is complete behind the last one
    }
    if (tid == 0) {
        // the bitmap keeps an end that is listed, or named twice, out
        auto join = [&](int v) { if (!act[v]) { act[v] = 1; list[base++] = v; } };
        join(e.e0); join(e.e1); join(e.e2); join(e.e3);
        if (e.ne == 6) { join(e.e4); join(e.e5); }
        S.nact = base;
    }
}

// Decision over the candidates of k_nl_scan (parts2) and k_nl3_scan (parts3; either may be NULL: no kind of it is enabled), then
// the move.  One workgroup per tour.  DLB: only the candidates of the workgroups that had lanes (|A| K of them, K lanes a
// node), and behind the move the new active set; a decision without a move ends the descent only in mode TSP_DLB_ON or when
// it looked at every node.
template <bool DLB>
__global__ __launch_bounds__(kNlPickThreads) void k_nl_pick_apply(int *__restrict__ orders, int *__restrict__ poss,
                                                                  NlState *__restrict__ st, int n, int nparts,
                                                                  const NlBest *__restrict__ parts2,
                                                                  const NlBest *__restrict__ parts3, int K, NlDlb dlb) {
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
    const int na = DLB ? S.nact : n;
    const int used = DLB ? (int)(((long long)na * K + 255) / 256) : nparts;
    double bd = INFINITY; u64 bk = kNoKey;
    for (int h = 0; h < 2; ++h) {
        const NlBest *part = h ? parts3 : parts2;
        if (!part) continue;
        part += (size_t)bt * nparts;
        for (int r = tid; r < used; r += NT) {
            const NlBest q = part[r];
            if (q.k != kNoKey && better(q.d, q.k, bd, bk)) { bd = q.d; bk = q.k; }
        }
    }
    block_argmin<true>(bd, bk, sd, sk);
    __syncthreads();
    int *order = orders + (size_t)bt * n, *pos = poss + (size_t)bt * n;
    if constexpr (!DLB) {
        if (tid == 0) { S.decisions += 1; if (bk == kNoKey) S.done = 1; }
        if (bk == kNoKey) return;
        nl_apply_move<NT>(order, pos, S, n, bk);
    } else {
        __shared__ int s_w[NT / 64];
        if (tid == 0) {
            S.decisions += 1; S.active_nodes += na;
            if (bk == kNoKey && (dlb.mode != TSP_DLB_CLOSE || na == n)) S.done = 1;
        }
        NlEnds e;
        if (bk != kNoKey) {
            e = nl_move_ends(order, pos, n, bk);
            nl_apply_move<NT>(order, pos, S, n, bk);
        }
        const size_t at = (size_t)bt * n;
        nl_dlb_update<NT>(dlb.act + at, dlb.hit + at, dlb.list + at, S, n, na, dlb.mode, e, s_w);
    }
}

NlData *nl_data(tsp_dev_inst *inst) {
    if (!inst->nl_data) inst->nl_data = new NlData();
    return static_cast<NlData *>(inst->nl_data);
}

int scratch_alloc(NlData *x, int B, int n, int K) {
    x->free_scratch();
    x->nparts = (int)(((long long)n * K + 255) / 256);   // of k_nl_scan and of k_nl3_scan: both have one lane per list entry
    x->parts_K = K;
    const size_t Bn = (size_t)B * n;
    TSP_HIP_TRY(hipMalloc(&x->d_st, sizeof(NlState) * B));
    TSP_HIP_TRY(hipHostMalloc(&x->h_st, sizeof(NlState) * B, hipHostMallocDefault));
    TSP_HIP_TRY(hipMalloc(&x->d_E, sizeof(double) * Bn));
    TSP_HIP_TRY(hipMalloc(&x->d_rem, sizeof(double) * 3 * Bn));
    TSP_HIP_TRY(hipMalloc(&x->d_cost, sizeof(double) * B));
    TSP_HIP_TRY(hipMalloc(&x->d_part, sizeof(NlBest) * 2 * (size_t)B * x->nparts));
    x->B = B;
    return TSP_OK;
}

bool bad_k(const tsp_dev_inst *inst, int K) { return K < 1 || K > TSP_NL_MAX_K || K > inst->n - 1; }

}  // namespace

void tsp_nl_data_free(void *p) { delete static_cast<NlData *>(p); }

// Lists built elsewhere on the device (alpha.hip) become the handle's lists; nothing queued may still read the old ones.
int tsp_nl_adopt_lists(tsp_dev_inst *inst, int K, int *d_nbr) {
    TSP_HIP_TRY(hipStreamSynchronize(inst->ctx->stream));
    NlData *x = nl_data(inst);
    (void)hipFree(x->d_nbr);
    x->d_nbr = d_nbr;
    x->K = K;
    return TSP_OK;
}

// The handle's lists where they lie on the device, built as tsp_dev_nl_opt builds them when it has none (held_karp_sparse.hip).
int tsp_nl_lists(tsp_dev_inst *inst, int *K, const int **d_nbr) {
    NlData *x = nl_data(inst);
    if (x->K == 0) {
        const int rc = tsp_dev_inst_knn_build(inst, std::min(TSP_NL_DEFAULT_K, inst->n - 1), nullptr);
        if (rc) return rc;
    }
    *K = x->K; *d_nbr = x->d_nbr;
    return TSP_OK;
}

// One whole decision of every tour that is not done, queued on the engine's stream: k_nl_prep, k_nl_scan when kinds has one of
// its two (candidates in the first B x nparts entries of d_part), k_nl3_scan when it has the third (in the second), the pick.
void tsp_nl_launch_decision(tsp_dev_tours *t, NlData *x, int kinds, int dlb_mode) {
    tsp_dev_inst *inst = t->inst;
    hipStream_t s = inst->ctx->stream;
    const int n = t->n, B = t->B;
    const bool low = kinds & (TSP_NL_2OPT | TSP_NL_OROPT), three = kinds & TSP_NL_3OPT;
    NlBest *parts3 = x->d_part + (size_t)B * x->nparts;
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_nl_prep<WTC, INTC>), dim3((n + 255) / 256, B), dim3(256), 0, s, inst->d_coord, t->d_order, x->d_st, n,
                           x->d_E, x->d_rem);
        if (low)
            TSP_DISPATCH_DLB(dlb_mode, {
                hipLaunchKernelGGL((k_nl_scan<WTC, INTC, DLBC>), dim3(x->nparts, B), dim3(256), 0, s, inst->d_coord, t->d_order,
                                   t->d_pos, x->d_st, n, x->K, kinds, x->d_nbr, x->d_E, x->d_rem, x->d_part, x->dlb(dlb_mode), NlPn{});
            });
    });
    if (three) tsp_nl3_launch_scan(t, x, parts3, dlb_mode);
    TSP_DISPATCH_DLB(dlb_mode, {
        hipLaunchKernelGGL(k_nl_pick_apply<DLBC>, dim3(B), dim3(kNlPickThreads), 0, s, t->d_order, t->d_pos, x->d_st, n, x->nparts,
                           low ? x->d_part : nullptr, three ? parts3 : nullptr, x->K, x->dlb(dlb_mode));
    });
}

void tsp_nl_launch_scan_pn(tsp_dev_tours *t, NlData *x, int kinds, int nparts, NlBest *parts, const NlPn &pn) {
    tsp_dev_inst *inst = t->inst;
    hipStream_t s = inst->ctx->stream;
    const int n = t->n, B = t->B;
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_nl_prep<WTC, INTC>), dim3((n + 255) / 256, B), dim3(256), 0, s, inst->d_coord, t->d_order, x->d_st, n,
                           x->d_E, x->d_rem);
        if (kinds & (TSP_NL_2OPT | TSP_NL_OROPT))
            hipLaunchKernelGGL((k_nl_scan<WTC, INTC, false, true>), dim3(nparts, B), dim3(256), 0, s, inst->d_coord, t->d_order,
                               t->d_pos, x->d_st, n, x->K, kinds, x->d_nbr, x->d_E, x->d_rem, parts, x->dlb(0), pn);
    });
}

int tsp_nl_dlb_start(tsp_dev_inst *inst, NlData *x, int B, const unsigned char *active, std::vector<int> *nact) {
    const int n = inst->n;
    const size_t Bn = (size_t)B * n;
    hipStream_t s = inst->ctx->stream;
    if (!x->d_act) {
        TSP_HIP_TRY(hipMalloc(&x->d_act, Bn));
        TSP_HIP_TRY(hipMalloc(&x->d_hit, Bn));
        TSP_HIP_TRY(hipMalloc(&x->d_alist, sizeof(int) * Bn));
    }
    std::vector<unsigned char> act(Bn);
    std::vector<int> list(Bn, 0);
    nact->assign((size_t)B, 0);
    for (int b = 0; b < B; ++b) {
        int c = 0;
        for (int v = 0; v < n; ++v) {
            const bool on = !active || active[(size_t)b * n + v] != 0;
            act[(size_t)b * n + v] = on ? 1 : 0;
            if (on) list[(size_t)b * n + c++] = v;
        }
        (*nact)[b] = c;
    }
    TSP_HIP_TRY(hipMemsetAsync(x->d_hit, 0, Bn, s));
    TSP_HIP_TRY(hipMemcpyAsync(x->d_act, act.data(), Bn, hipMemcpyHostToDevice, s));
    TSP_HIP_TRY(hipMemcpyAsync(x->d_alist, list.data(), sizeof(int) * Bn, hipMemcpyHostToDevice, s));
    TSP_HIP_TRY(hipStreamSynchronize(s));   // the two host arrays end here
    return TSP_OK;
}

int tsp_nl_check(const tsp_dev_inst *inst, int *kinds, int allowed, int B, const int *succ, int succ_stride, int64_t tour_stride,
                 const double *obj) {
    if (!inst || !succ || !obj || B < 1 || succ_stride < 1) return TSP_DEV_E_ARG;
    if (*kinds < 1 || (*kinds & ~allowed)) return TSP_DEV_E_ARG;
    const int n = inst->n;
    if ((*kinds & TSP_NL_3OPT) && n > kNlMaxN3) return TSP_DEV_E_ARG;
    if (B > 1 && tour_stride < (int64_t)n * succ_stride) return TSP_DEV_E_ARG;
    // a kind without any move at this size is left out: 2-opt needs four nodes, Or-opt and 3-opt five
    if (n < 4) *kinds &= ~TSP_NL_2OPT;
    if (n < 5) *kinds &= ~(TSP_NL_OROPT | TSP_NL_3OPT);
    return TSP_OK;
}

int tsp_nl_prepare(tsp_dev_inst *inst, int B, NlData **out) {
    const int n = inst->n;
    NlData *x = nl_data(inst);
    if (x->K == 0) {
        const int rc = tsp_dev_inst_knn_build(inst, std::min(TSP_NL_DEFAULT_K, n - 1), nullptr);
        if (rc) return rc;
    }
    if (x->B != B || x->parts_K != x->K) {
        const int rc = scratch_alloc(x, B, n, x->K);
        if (rc) { x->free_scratch(); return rc; }
    }
    *out = x;
    return TSP_OK;
}

// The layouts that let one writer serve the five record types: each starts as the one before it.
static_assert(offsetof(tsp_nl3_opt_stats, moves_3opt) == sizeof(tsp_nl_opt_stats), "tsp_nl3_opt_stats starts as tsp_nl_opt_stats");
static_assert(offsetof(tsp_nl_dlb_stats, active_nodes) == sizeof(tsp_nl3_opt_stats), "tsp_nl_dlb_stats starts as tsp_nl3_opt_stats");
static_assert(offsetof(tsp_ils_stats, iterations) == sizeof(tsp_nl3_opt_stats), "tsp_ils_stats starts as tsp_nl3_opt_stats");
static_assert(offsetof(tsp_ils_dlb_stats, active_nodes) == sizeof(tsp_ils_stats), "tsp_ils_dlb_stats starts as tsp_ils_stats");

void tsp_nl_write_stats(const NlStatsOut &out, int b, const NlState &z, const IlsState *q, double start_cost, double seconds,
                        float device_ms) {
    if (!out.p) return;
    char *rec = static_cast<char *>(out.p) + (size_t)b * out.stride;
    tsp_nl_opt_stats &o = *reinterpret_cast<tsp_nl_opt_stats *>(rec);
    o.decisions = z.decisions; o.moves = z.moves; o.moves_2opt = z.moves_2opt; o.moves_oropt = z.moves_oropt;
    for (int k = 0; k < 3; ++k) o.moves_by_len[k] = z.moves_len[k];
    o.moves_reversed = z.moves_rev; o.reversed = z.reversed; o.deltas_executed = z.deltas;
    o.seconds = seconds; o.device_ms = device_ms;
    if (out.parts & kNlStats3) {
        tsp_nl3_opt_stats &o3 = *reinterpret_cast<tsp_nl3_opt_stats *>(rec);
        o3.moves_3opt = z.moves_3opt;
        for (int k = 0; k < 4; ++k) o3.moves_by_type[k] = z.moves_type[k];
    }
    const bool chain = out.parts & kNlStatsChain;
    if (chain) {
        tsp_ils_stats &c = *reinterpret_cast<tsp_ils_stats *>(rec);
        const bool begun = q && q->it >= 0;   // the first descent has ended
        c.iterations = begun ? q->it : 0; c.accepted = q ? q->accepted : 0; c.last_improved = q ? q->last_improved : -1;
        c.start_cost = begun ? q->start_cost : start_cost;
    }
    if (!(out.parts & kNlStatsDlb)) return;
    if (chain) {
        tsp_ils_dlb_stats &d = *reinterpret_cast<tsp_ils_dlb_stats *>(rec);
        d.active_nodes = z.active_nodes; d.closing_scans = z.closing_scans;
    } else {
        tsp_nl_dlb_stats &d = *reinterpret_cast<tsp_nl_dlb_stats *>(rec);
        d.active_nodes = z.active_nodes; d.closing_scans = z.closing_scans;
    }
}

int tsp_nl_run(tsp_dev_inst *inst, int kinds, int allowed, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
               int64_t max_moves, double time_limit_s, const NlStatsOut &out, int dlb_mode, const unsigned char *active) {
    int rc = tsp_nl_check(inst, &kinds, allowed, B, succ, succ_stride, tour_stride, obj);
    if (rc) return rc;
    Descent run;
    rc = run.open(inst, B, succ, succ_stride, tour_stride, obj);
    if (rc) return rc;
    NlData *x = nullptr;
    rc = tsp_nl_prepare(inst, B, &x);
    if (rc) return rc;
    std::vector<int> nact;
    NlHooks hooks;
    if (dlb_mode) {
        rc = tsp_nl_dlb_start(inst, x, B, active, &nact);
        if (rc) return rc;
        hooks.nact = nact.data();
    }
    const int status = run.run(x->d_st, x->h_st, x->d_cost, kinds == 0 || max_moves == 0, 256, max_moves, time_limit_s,
                               [&](bool) { tsp_nl_launch_decision(run.t, x, kinds, dlb_mode); }, hooks);
    if (status != TSP_OK && status != TSP_TIME_LIMIT_EXCEEDED) return status;
    const double seconds = wall_s() - run.t0;
    for (int b = 0; b < B; ++b) tsp_nl_write_stats(out, b, x->h_st[b], nullptr, obj[b], seconds, run.device_ms);
    return status;
}

extern "C" {

int tsp_dev_inst_knn_build(tsp_dev_inst *inst, int K, float *kernel_ms) {
    if (!inst || bad_k(inst, K)) return TSP_DEV_E_ARG;
    const int n = inst->n;
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    hipStream_t s = inst->ctx->stream;
    const ScanChunks g = scan_chunks(n, kKnnWaves, kKnnChunks, 1);
    DevBuf<double> pd;
    DevBuf<int> pi, nbr;
    TSP_HIP_TRY(pd.alloc((size_t)g.Cc * kK * n));
    TSP_HIP_TRY(pi.alloc((size_t)g.Cc * kK * n));
    TSP_HIP_TRY(nbr.alloc((size_t)n * K));
    if (int e = tsp_inst_events(inst)) return e;
    TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_knn_scan<WTC, INTC>), dim3((n + 255) / 256, g.Cc), dim3(256), 0, s, inst->d_coord, n, g.CH, pd.p, pi.p);
    });
    hipLaunchKernelGGL(k_knn_merge, dim3((n + 255) / 256), dim3(256), 0, s, n, g.Cc, K, pd.p, pi.p, nbr.p);
    TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
    TSP_HIP_TRY(hipEventSynchronize(inst->ev1));
    TSP_HIP_TRY(hipGetLastError());
    float ms = 0.f;
    TSP_HIP_TRY(hipEventElapsedTime(&ms, inst->ev0, inst->ev1));
    if (kernel_ms) *kernel_ms = ms;
    NlData *x = nl_data(inst);
    (void)hipFree(x->d_nbr);
    x->d_nbr = nbr.p; nbr.p = nullptr;
    x->K = K;
    return TSP_OK;
}

int tsp_dev_inst_knn_set(tsp_dev_inst *inst, int K, const int *nbr) {
    if (!inst || !nbr || bad_k(inst, K)) return TSP_DEV_E_ARG;
    const int n = inst->n;
    for (int v = 0; v < n; ++v)
        for (int k = 0; k < K; ++k) {
            const int u = nbr[(size_t)v * K + k];
            if (u < 0 || u >= n || u == v) return TSP_DEV_E_ARG;
        }
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    DevBuf<int> d;
    TSP_HIP_TRY(d.alloc((size_t)n * K));
    TSP_HIP_TRY(hipMemcpy(d.p, nbr, sizeof(int) * (size_t)n * K, hipMemcpyHostToDevice));
    TSP_HIP_TRY(hipStreamSynchronize(inst->ctx->stream));   // nothing queued may still read the old lists
    NlData *x = nl_data(inst);
    (void)hipFree(x->d_nbr);
    x->d_nbr = d.p; d.p = nullptr;
    x->K = K;
    return TSP_OK;
}

int tsp_dev_inst_knn_get(tsp_dev_inst *inst, int *K, int *nbr) {
    if (!inst || !K) return TSP_DEV_E_ARG;
    const NlData *x = static_cast<const NlData *>(inst->nl_data);
    *K = x ? x->K : 0;
    if (!nbr || *K == 0) return TSP_OK;
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    TSP_HIP_TRY(hipStreamSynchronize(inst->ctx->stream));
    TSP_HIP_TRY(hipMemcpy(nbr, x->d_nbr, sizeof(int) * (size_t)inst->n * x->K, hipMemcpyDeviceToHost));
    return TSP_OK;
}

int tsp_dev_nl_opt(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                   int64_t max_moves, double time_limit_s, tsp_nl_opt_stats *stats) {
    return tsp_nl_run(inst, kinds, TSP_NL_2OPT | TSP_NL_OROPT, B, succ, succ_stride, tour_stride, obj, max_moves, time_limit_s,
                      NlStatsOut{stats, sizeof *stats, 0}, TSP_DLB_OFF, nullptr);
}

}  // extern "C"
