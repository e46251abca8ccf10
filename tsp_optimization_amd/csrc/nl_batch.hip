// nl_batch.hip -- the batched list descent (tsp_dev_nl_3opt_batch): a decision carries out a set of improving
// moves with pairwise disjoint arcs (nl_arc.hpp) instead of one.  The definitions are in include/tsp_hip.h.
//
// Decision k_nl_prep and the per-node forms of k_nl_scan / k_nl3_scan (nl_opt.hip, nl3_opt.hip: one candidate per node over the
//          moves of an arc of at most max_arc positions, and the overall best per workgroup as ever) -> `rounds` times
//          { k_nlb_claim_d, k_nlb_claim_k, k_nlb_resolve } over B x n claim words -> k_nlb_pick (one workgroup per tour: the overall
//          best, the fall-back to it, max_moves, decisions and done) -> k_nlb_apply (one workgroup per accepted move).
// A claim round: every live candidate puts the order-preserving image of its delta on every position of its arc with atomicMin,
// then its key on the positions that hold its delta; it is accepted when every position holds both.  That is the exact
// (delta, key) order without a 128-bit atomic and without a sort.  The candidates of the three claim kernels are one wave each.
// The same move under several nodes claims with the same words; the taken word of the arc's first position admits one of them.
#include "nl_common.hpp"

#pragma clang fp contract(off)

using namespace tsp;

namespace {

constexpr int kNlbWaves = 4;              // candidates per workgroup of the claim kernels
constexpr int kNlbApplyThreads = 1024;    // as k_nl_pick_apply: a fall-back move reverses up to n / 2 positions
constexpr int kNlbApplyGrid = 1024;       // most workgroups per tour of k_nlb_apply

// The live candidate of wave (blockIdx.x, threadIdx.x / 64) of tour b and its arc; false: none (uniform over the wave).
__device__ __forceinline__ bool nlb_candidate(const NlState *__restrict__ st, const NlBest *__restrict__ cand,
                                              const int *__restrict__ poss, int n, int b, int *v, NlBest *c, NlArc *arc) {
    if (st[b].done) return false;
    *v = (int)blockIdx.x * kNlbWaves + ((int)threadIdx.x >> 6);
    if (*v >= n) return false;
    *c = cand[(size_t)b * n + *v];
    if (c->k == kNoKey) return false;
    *arc = nl_arc_of_key(poss + (size_t)b * n, n, c->k);
    return true;
}

// Round step 1: the candidates whose arc meets an accepted arc die (check: not in a decision's first round, where nothing is
// accepted yet); the others claim their positions with the image of their delta.
__global__ __launch_bounds__(kNlbWaves * 64) void k_nlb_claim_d(const int *__restrict__ poss, const NlState *__restrict__ st, int n,
                                                                NlBest *__restrict__ cand, u64 *__restrict__ clm_d,
                                                                const int *__restrict__ taken, int check) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    int v;
    NlBest c;
    NlArc arc;
    if (!nlb_candidate(st, cand, poss, n, b, &v, &c, &arc)) return;
    const size_t row = (size_t)b * n;
    if (check) {
        bool met = false;
        for (int q = lane; q < arc.len; q += 64) met = met || taken[row + or_wrap(arc.start + q, n)] != 0;
        if (__any(met)) {
            if (lane == 0) cand[row + v].k = kNoKey;
            return;
        }
    }
    const u64 img = ordered_bits(c.d);
    for (int q = lane; q < arc.len; q += 64) atomicMin(&clm_d[row + or_wrap(arc.start + q, n)], img);
}

// Round step 2: among the candidates that hold a position's delta, the smallest key.
__global__ __launch_bounds__(kNlbWaves * 64) void k_nlb_claim_k(const int *__restrict__ poss, const NlState *__restrict__ st, int n,
                                                                const NlBest *__restrict__ cand, const u64 *__restrict__ clm_d,
                                                                u64 *__restrict__ clm_k) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    int v;
    NlBest c;
    NlArc arc;
    if (!nlb_candidate(st, cand, poss, n, b, &v, &c, &arc)) return;
    const size_t row = (size_t)b * n;
    const u64 img = ordered_bits(c.d);
    for (int q = lane; q < arc.len; q += 64) {
        const size_t at = row + or_wrap(arc.start + q, n);
        if (clm_d[at] == img) atomicMin(&clm_k[at], c.k);
    }
}

// Round step 3: a candidate that holds all of its positions is accepted: its arc is taken, and the one wave that takes the
// arc's first position appends the move to the tour's accepted list (in no particular order: the moves commute).
__global__ __launch_bounds__(kNlbWaves * 64) void k_nlb_resolve(const int *__restrict__ poss, const NlState *__restrict__ st, int n,
                                                                NlBest *__restrict__ cand, const u64 *__restrict__ clm_d,
                                                                const u64 *__restrict__ clm_k, int *__restrict__ taken,
                                                                NlBest *__restrict__ acc, NlbCtl *__restrict__ ctl) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    int v;
    NlBest c;
    NlArc arc;
    if (!nlb_candidate(st, cand, poss, n, b, &v, &c, &arc)) return;
    const size_t row = (size_t)b * n;
    const u64 img = ordered_bits(c.d);
    bool mine = true;
    for (int q = lane; q < arc.len; q += 64) {
        const size_t at = row + or_wrap(arc.start + q, n);
        mine = mine && clm_d[at] == img && clm_k[at] == c.k;
    }
    if (!__all(mine)) return;
    if (lane == 0) {
        cand[row + v].k = kNoKey;
        if (atomicExch(&taken[row + arc.start], 1) == 0) acc[row + atomicAdd(&ctl[b].nacc, 1)] = c;
    }
    for (int q = lane; q < arc.len; q += 64) taken[row + or_wrap(arc.start + q, n)] = 1;
}

// One workgroup per tour behind the claim rounds: the overall best of the scans' workgroups (parts2 / parts3, either may be NULL),
// which is the decision's single move when no candidate was accepted; max_moves; decisions and done.  Leaves in the tour's
// control words what k_nlb_apply carries out.
__global__ __launch_bounds__(kNlPickThreads) void k_nlb_pick(NlState *__restrict__ st, int n, int nparts,
                                                             const NlBest *__restrict__ parts2, const NlBest *__restrict__ parts3,
                                                             NlBest *__restrict__ acc, NlbCtl *__restrict__ ctl) {
    constexpr int NT = kNlPickThreads;
    const int bt = blockIdx.x, tid = threadIdx.x;
    NlState &S = st[bt];
    NlbCtl &Cw = ctl[bt];
    if (S.done || (S.max_moves >= 0 && S.moves >= S.max_moves)) {
        if (tid == 0) { S.done = 1; Cw.nacc = 0; Cw.napply = 0; Cw.keep = -1; }
        return;
    }
    __shared__ double sd[NT / 64];
    __shared__ u64 sk[NT / 64];
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
    if (tid != 0) return;
    S.decisions += 1;
    int na = Cw.nacc, keep = -1;
    if (na == 0 && bk != kNoKey) { acc[(size_t)bt * n] = NlBest{bd, bk}; na = 1; }
    if (na == 0) S.done = 1;   // no improving move of any arc: a local optimum of the list neighbourhood
    if (na > 0 && S.max_moves >= 0) {
        const long long left = S.max_moves - S.moves;
        if ((long long)na >= left) S.done = 1;
        if ((long long)na > left) keep = (int)left;
    }
    Cw.nacc = 0; Cw.napply = na; Cw.keep = keep;
}

// One workgroup per accepted move, the grid looping over the tour's list.  The arcs are disjoint, so the workgroups read and
// write disjoint positions (and the pos of disjoint nodes); a move's counters reach the tour's state through atomics.  keep >= 0:
// only the moves with fewer than `keep` better ones in the list.
__global__ __launch_bounds__(kNlbApplyThreads) void k_nlb_apply(int *__restrict__ orders, int *__restrict__ poss,
                                                                NlState *__restrict__ st, int n, const NlBest *__restrict__ acc,
                                                                const NlbCtl *__restrict__ ctl) {
    constexpr int NT = kNlbApplyThreads;
    const int bt = blockIdx.y, tid = threadIdx.x;
    const int napply = ctl[bt].napply, keep = ctl[bt].keep;
    if ((int)blockIdx.x >= napply) return;
    __shared__ int s_cnt[NT / 64];
    int *order = orders + (size_t)bt * n, *pos = poss + (size_t)bt * n;
    const NlBest *list = acc + (size_t)bt * n;
    for (int m = blockIdx.x; m < napply; m += gridDim.x) {
        const NlBest c = list[m];
        if (keep >= 0) {
            int cnt = 0;
            for (int j = tid; j < napply; j += NT) cnt += better(list[j].d, list[j].k, c.d, c.k) ? 1 : 0;
            for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
            if ((tid & 63) == 0) s_cnt[tid >> 6] = cnt;
            __syncthreads();
            int rank = 0;
            for (int w = 0; w < NT / 64; ++w) rank += s_cnt[w];
            __syncthreads();
            if (rank >= keep) continue;
        }
        NlState loc;
        if (tid == 0) {
            loc.max_moves = -1; loc.done = 0;
            loc.moves = loc.moves_2opt = loc.moves_oropt = loc.moves_rev = loc.reversed = loc.moves_3opt = 0;
            loc.moves_len[0] = loc.moves_len[1] = loc.moves_len[2] = 0;
            loc.moves_type[0] = loc.moves_type[1] = loc.moves_type[2] = loc.moves_type[3] = 0;
        }
        nl_apply_move<NT>(order, pos, loc, n, c.k);
        if (tid == 0) {
            NlState &S = st[bt];
            auto add = [](long long &to, long long by) { if (by) atomicAdd((unsigned long long *)&to, (unsigned long long)by); };
            add(S.moves, loc.moves); add(S.moves_2opt, loc.moves_2opt); add(S.moves_oropt, loc.moves_oropt);
            add(S.moves_rev, loc.moves_rev); add(S.reversed, loc.reversed); add(S.moves_3opt, loc.moves_3opt);
            for (int k = 0; k < 3; ++k) add(S.moves_len[k], loc.moves_len[k]);
            for (int k = 0; k < 4; ++k) add(S.moves_type[k], loc.moves_type[k]);
        }
        __syncthreads();   // the workgroup's next move starts behind this one's last write
    }
}

int batch_alloc(NlData *x, int B, int n) {
    if (x->d_cand) return TSP_OK;   // of this B and K: tsp_nl_prepare frees the batch scratch with the rest
    const size_t Bn = (size_t)B * n;
    x->bparts = (n + 256 / x->K - 1) / (256 / x->K);
    TSP_HIP_TRY(hipMalloc(&x->d_cand, sizeof(NlBest) * Bn));
    TSP_HIP_TRY(hipMalloc(&x->d_acc, sizeof(NlBest) * Bn));
    TSP_HIP_TRY(hipMalloc(&x->d_bpart, sizeof(NlBest) * 2 * (size_t)B * x->bparts));
    TSP_HIP_TRY(hipMalloc(&x->d_clm, sizeof(u64) * 2 * Bn));
    TSP_HIP_TRY(hipMalloc(&x->d_taken, sizeof(int) * Bn));
    TSP_HIP_TRY(hipMalloc(&x->d_bctl, sizeof(NlbCtl) * B));
    return TSP_OK;
}

// One whole batched decision of every tour that is not done, queued on the engine's stream.
void launch_decision(tsp_dev_tours *t, NlData *x, int kinds, int max_arc, int rounds) {
    hipStream_t s = t->inst->ctx->stream;
    const int n = t->n, B = t->B;
    const size_t Bn = (size_t)B * n;
    const bool low = kinds & (TSP_NL_2OPT | TSP_NL_OROPT), three = kinds & TSP_NL_3OPT;
    NlBest *parts3 = x->d_bpart + (size_t)B * x->bparts;
    tsp_nl_launch_scan_pn(t, x, kinds, x->bparts, x->d_bpart, NlPn{x->d_cand, max_arc, 0});
    if (three) tsp_nl3_launch_scan_pn(t, x, x->bparts, parts3, NlPn{x->d_cand, max_arc, low ? 1 : 0});
    (void)hipMemsetAsync(x->d_taken, 0, sizeof(int) * Bn, s);
    u64 *clm_d = x->d_clm, *clm_k = x->d_clm + Bn;
    const dim3 grid((n + kNlbWaves - 1) / kNlbWaves, B), block(kNlbWaves * 64);
    for (int r = 0; r < rounds; ++r) {
        (void)hipMemsetAsync(x->d_clm, 0xff, sizeof(u64) * 2 * Bn, s);
        hipLaunchKernelGGL(k_nlb_claim_d, grid, block, 0, s, t->d_pos, x->d_st, n, x->d_cand, clm_d, x->d_taken, r > 0 ? 1 : 0);
        hipLaunchKernelGGL(k_nlb_claim_k, grid, block, 0, s, t->d_pos, x->d_st, n, x->d_cand, clm_d, clm_k);
        hipLaunchKernelGGL(k_nlb_resolve, grid, block, 0, s, t->d_pos, x->d_st, n, x->d_cand, clm_d, clm_k, x->d_taken, x->d_acc,
                           x->d_bctl);
    }
    hipLaunchKernelGGL(k_nlb_pick, dim3(B), dim3(kNlPickThreads), 0, s, x->d_st, n, x->bparts, low ? x->d_bpart : nullptr,
                       three ? parts3 : nullptr, x->d_acc, x->d_bctl);
    hipLaunchKernelGGL(k_nlb_apply, dim3(std::min(kNlbApplyGrid, n), B), dim3(kNlbApplyThreads), 0, s, t->d_order, t->d_pos, x->d_st,
                       n, x->d_acc, x->d_bctl);
}

}  // namespace

extern "C" {

int tsp_dev_nl_3opt_batch(tsp_dev_inst *inst, int kinds, int max_arc, int rounds, int B, int *succ, int succ_stride,
                          int64_t tour_stride, double *obj, int64_t max_moves, double time_limit_s, tsp_nl3_opt_stats *stats) {
    int rc = tsp_nl_check(inst, &kinds, TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT, B, succ, succ_stride, tour_stride, obj);
    if (rc) return rc;
    const int n = inst->n;
    if (max_arc <= 0) max_arc = n / 2;
    max_arc = std::min(max_arc, n);
    if (rounds <= 0) rounds = TSP_NL_BATCH_DEFAULT_ROUNDS;
    rounds = std::min(rounds, n);   // a round with a live candidate accepts one: n rounds leave none
    Descent run;
    rc = run.open(inst, B, succ, succ_stride, tour_stride, obj);
    if (rc) return rc;
    NlData *x = nullptr;
    rc = tsp_nl_prepare(inst, B, &x);
    if (rc) return rc;
    rc = batch_alloc(x, B, n);
    if (rc) { x->free_scratch(); return rc; }
    TSP_HIP_TRY(hipMemsetAsync(x->d_bctl, 0, sizeof(NlbCtl) * B, inst->ctx->stream));
    const int status = run.run(x->d_st, x->h_st, x->d_cost, kinds == 0 || max_moves == 0, 256, max_moves, time_limit_s,
                               [&](bool) { launch_decision(run.t, x, kinds, max_arc, rounds); }, NlHooks{});
    if (status != TSP_OK && status != TSP_TIME_LIMIT_EXCEEDED) return status;
    const double seconds = wall_s() - run.t0;
    const NlStatsOut out{stats, sizeof *stats, kNlStats3};
    for (int b = 0; b < B; ++b) tsp_nl_write_stats(out, b, x->h_st[b], nullptr, obj[b], seconds, run.device_ms);
    return status;
}

}  // extern "C"
