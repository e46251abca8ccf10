// ils.hip -- iterated local search over the list descent (tsp_dev_ils, tsp_dev_ils_kick).  The definitions are in
// include/tsp_hip.h.
//
// Decision the four launches of nl_opt.hip / nl3_opt.hip (k_nl_prep, k_nl_scan, k_nl3_scan, k_nl_pick_apply) -> k_ils_step (one
//          workgroup per chain; it returns at once unless the chain's descent has just ended: then the cost of the work tour,
//          work -> incumbent or back, the next kick on order/pos and the descent re-armed, or the chain marked finished).
// The work tours are the instance's scratch tours handle, the incumbents a second order/pos per chain.  An iteration moves
// nothing to the host, which queues decisions and polls both control blocks as it does for a single descent.  The records are
// written by tsp_nl_write_stats (nl_opt.hip) from both control blocks; below eight nodes the call is tsp_nl_run.
#include "descent.hpp"
#include "ils_common.hpp"
#include "nl_common.hpp"

#pragma clang fp contract(off)

using namespace tsp;

namespace {

// The kick of iteration `it` of chain b on order/pos (n >= 8, W >= 8), by every thread of the one workgroup (NT threads) that
// owns the tour, behind a barrier that follows the last write of the tour.  Positions pos[s] + o1 .. pos[s] + o4 - 1 hold
// Bk Ck Dk; reversed as one path they hold Dk' Ck' Bk', and each block reversed again leaves Dk Ck Bk.
__device__ __forceinline__ IlsCuts ils_cuts(int n, int W, u64 seed, int b, long long it) {
    const u64 base = ils_base(seed, b, it);
    return ils_cuts_from((int)(ils_mix(base) % (u64)n), W, ils_mix(base + 1), ils_mix(base + 2), ils_mix(base + 3),
                         ils_mix(base + 4));
}

template <int NT>
__device__ __forceinline__ void ils_kick(int *__restrict__ order, int *__restrict__ pos, int n, int W, u64 seed, int b,
                                         long long it) {
    const IlsCuts c = ils_cuts(n, W, seed, b, it);
    const int s = c.s, o1 = c.o1, o2 = c.o2, o3 = c.o3, o4 = c.o4;
    const int at = or_wrap(pos[s] + o1, n);   // position pos[s] is outside the window: no reversal moves s
    const int lB = o2 - o1, lC = o3 - o2, lD = o4 - o3;
    nl_reverse_path<NT>(order, pos, n, at, lB + lC + lD);
    __syncthreads();
    nl_reverse_path<NT>(order, pos, n, at, lD);
    nl_reverse_path<NT>(order, pos, n, or_wrap(at + lD, n), lC);
    nl_reverse_path<NT>(order, pos, n, or_wrap(at + lD + lC, n), lB);
}

__global__ __launch_bounds__(kNlPickThreads) void k_ils_kick(int *__restrict__ orders, int *__restrict__ poss, int n, int W,
                                                             u64 seed, long long it) {
    const int b = blockIdx.x;
    ils_kick<kNlPickThreads>(orders + (size_t)b * n, poss + (size_t)b * n, n, W, seed, b, it);
}

// One workgroup per chain, behind every decision.  inc: the incumbents, B x n of order, then B x n of pos.
// DLB: the kick also sets the active set of the descent it re-arms: the tails and heads of its four removed edges, read from
// the tour before the kick, and nothing else.
template <int WT, bool INT, bool DLB>
__global__ __launch_bounds__(kNlPickThreads) void k_ils_step(const double2 *__restrict__ coord, int *__restrict__ orders,
                                                             int *__restrict__ poss, int *__restrict__ inc,
                                                             NlState *__restrict__ st, IlsState *__restrict__ ils, int n, int W,
                                                             u64 seed, long long iterations, long long M, NlDlb dlb) {
    constexpr int NT = kNlPickThreads;
    const int b = blockIdx.x;
    NlState &S = st[b];
    IlsState &I = ils[b];
    if (I.finished || !S.done) return;
    __shared__ double s_d[NT / 64];
    __shared__ double s_chunk[(INT || WT == WT_CEIL_2D) ? 1 : 4096];
    const int tid = threadIdx.x;
    int *order = orders + (size_t)b * n, *pos = poss + (size_t)b * n;
    int *iorder = inc + (size_t)b * n, *ipos = iorder + (size_t)gridDim.x * n;
    const long long it = I.it;          // the iteration whose descent has ended; -1: the first descent
    const double best = I.cost;
    const int na = S.nact;              // what that descent left active
    const double c = tour_cost_block<WT, INT>(coord, order, pos, n, s_d, s_chunk);
    const bool accept = it < 0 || c < best;
    __syncthreads();   // every thread has read the chain's state
    if (accept)
        for (int p = tid; p < n; p += NT) { iorder[p] = order[p]; ipos[p] = pos[p]; }
    else
        for (int p = tid; p < n; p += NT) { order[p] = iorder[p]; pos[p] = ipos[p]; }
    const long long next = it + 1;      // iterations completed, and the iteration that starts now
    if (tid == 0) {
        if (it < 0) I.start_cost = c;
        else if (accept) { I.accepted += 1; I.last_improved = it; }
        if (accept) I.cost = c;
        I.it = next;
        if (next >= iterations) I.finished = 1;
    }
    if (next >= iterations) return;     // the work tour is the incumbent
    __syncthreads();
    int cut[8];
    if constexpr (DLB) {
        const IlsCuts c = ils_cuts(n, W, seed, b, next);
        const int p0 = pos[c.s], o[4] = {c.o1, c.o2, c.o3, c.o4};   // o4 <= n: position p0 + o4 wraps to s itself at the most
        for (int q = 0; q < 4; ++q) {
            cut[2 * q] = order[or_wrap(p0 + o[q] - 1, n)];
            cut[2 * q + 1] = order[or_wrap(p0 + o[q], n)];
        }
        __syncthreads();   // every thread has read the tour before the kick moves it
    }
    ils_kick<NT>(order, pos, n, W, seed, b, next);
    if constexpr (DLB) {
        // hit is all zero behind a decision.  Whatever the descent left in A goes, also what a descent ended by M left there.
        unsigned char *act = dlb.act + (size_t)b * n;
        int *list = dlb.list + (size_t)b * n;
        for (int slot = tid; slot < na; slot += NT) act[list[slot]] = 0;
        __syncthreads();
        if (tid == 0) {
            int c = 0;
            for (int q = 0; q < 8; ++q)
                if (!act[cut[q]]) { act[cut[q]] = 1; list[c++] = cut[q]; }   // single-node blocks name a node twice
            S.nact = c;
        }
    }
    if (tid == 0) {
        S.done = M == 0 ? 1 : 0;
        S.max_moves = M < 0 ? -1 : S.moves + M;
    }
}

// What Descent::run needs to know of a chain beyond its NlState.
struct IlsHooks : NlHooks {   // nact: |A| of the first descent
    tsp_dev_tours *t;
    NlData *x;
    long long M;
    void init(NlState &z, int b) const { z.done = M == 0 ? 1 : 0; NlHooks::init(z, b); }
    int fetch(hipStream_t s) const {
        TSP_HIP_TRY(hipMemcpyAsync(x->h_ils, x->d_ils, sizeof(IlsState) * t->B, hipMemcpyDeviceToHost, s));
        return TSP_OK;
    }
    bool finished(const NlState &, int b) const { return x->h_ils[b].finished; }
    // at the time limit the work tours are in the middle of an iteration: the incumbents are what the call returns
    int finish(int status) const {
        hipStream_t s = t->inst->ctx->stream;
        const size_t Bn = (size_t)t->B * t->n;
        if (status == TSP_TIME_LIMIT_EXCEEDED) {
            TSP_HIP_TRY(hipMemcpyAsync(t->d_order, x->d_inc, sizeof(int) * Bn, hipMemcpyDeviceToDevice, s));
            TSP_HIP_TRY(hipMemcpyAsync(t->d_pos, x->d_inc + Bn, sizeof(int) * Bn, hipMemcpyDeviceToDevice, s));
        }
        return fetch(s);
    }
};

bool bad_span(int span) { return span >= 1 && span <= 7; }

}  // namespace

// What both entry points do; `out` names their record type.
static int ils_run(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj, uint64_t seed,
                   int64_t iterations, int span, int64_t max_moves_per_descent, double time_limit_s, int dlb_mode,
                   const NlStatsOut &out) {
    const int allowed = TSP_NL_2OPT | TSP_NL_OROPT | TSP_NL_3OPT;
    const int asked = kinds;
    int rc = tsp_nl_check(inst, &kinds, allowed, B, succ, succ_stride, tour_stride, obj);
    if (rc) return rc;
    if (iterations < 0 || bad_span(span)) return TSP_DEV_E_ARG;
    const int n = inst->n;
    const long long M = max_moves_per_descent < 0 ? -1 : max_moves_per_descent;
    if (n < 8)   // no kick: the descent alone
        return tsp_nl_run(inst, asked, allowed, B, succ, succ_stride, tour_stride, obj, M, time_limit_s, out, dlb_mode, nullptr);
    Descent run;
    rc = run.open(inst, B, succ, succ_stride, tour_stride, obj);
    if (rc) return rc;
    NlData *x = nullptr;
    rc = tsp_nl_prepare(inst, B, &x);
    if (rc) return rc;
    hipStream_t s = inst->ctx->stream;
    const size_t Bn = (size_t)B * n;
    if (!x->d_inc) {
        TSP_HIP_TRY(hipMalloc(&x->d_inc, sizeof(int) * 2 * Bn));
        TSP_HIP_TRY(hipMalloc(&x->d_ils, sizeof(IlsState) * B));
        TSP_HIP_TRY(hipHostMalloc(&x->h_ils, sizeof(IlsState) * B, hipHostMallocDefault));
    }
    // the incumbents start as the caller's tours, the chains in their first descent
    tsp_dev_tours *t = run.t;
    for (int b = 0; b < B; ++b) {
        IlsState q;
        memset(&q, 0, sizeof q);
        q.it = -1; q.last_improved = -1;
        x->h_ils[b] = q;
    }
    TSP_HIP_TRY(hipMemcpyAsync(x->d_inc, t->d_order, sizeof(int) * Bn, hipMemcpyDeviceToDevice, s));
    TSP_HIP_TRY(hipMemcpyAsync(x->d_inc + Bn, t->d_pos, sizeof(int) * Bn, hipMemcpyDeviceToDevice, s));
    TSP_HIP_TRY(hipMemcpyAsync(x->d_ils, x->h_ils, sizeof(IlsState) * B, hipMemcpyHostToDevice, s));
    const int W = span <= 0 ? n : std::min(span, n);
    std::vector<int> nact;   // step 1 of a chain starts with A = V
    if (dlb_mode) {
        rc = tsp_nl_dlb_start(inst, x, B, nullptr, &nact);
        if (rc) return rc;
    }
    IlsHooks hooks;
    hooks.nact = dlb_mode ? nact.data() : nullptr; hooks.t = t; hooks.x = x; hooks.M = M;
    const int status = run.run(x->d_st, x->h_st, x->d_cost, false, 256, M, time_limit_s,
                               [&](bool) {
                                   tsp_nl_launch_decision(t, x, kinds, dlb_mode);
                                   TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
                                       TSP_DISPATCH_DLB(dlb_mode, {
                                           hipLaunchKernelGGL((k_ils_step<WTC, INTC, DLBC>), dim3(B), dim3(kNlPickThreads), 0, s,
                                                              inst->d_coord, t->d_order, t->d_pos, x->d_inc, x->d_st, x->d_ils, n, W,
                                                              (u64)seed, (long long)iterations, M, x->dlb(dlb_mode));
                                       });
                                   });
                               },
                               hooks);
    if (status != TSP_OK && status != TSP_TIME_LIMIT_EXCEEDED) return status;
    const double seconds = wall_s() - run.t0;
    // a chain whose first descent the limit ended starts from the caller's tour, whose cost obj[b] then is
    for (int b = 0; b < B; ++b) tsp_nl_write_stats(out, b, x->h_st[b], &x->h_ils[b], obj[b], seconds, run.device_ms);
    return status;
}

extern "C" {

int tsp_dev_ils(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj, uint64_t seed,
                int64_t iterations, int span, int64_t max_moves_per_descent, double time_limit_s, tsp_ils_stats *stats) {
    return ils_run(inst, kinds, B, succ, succ_stride, tour_stride, obj, seed, iterations, span, max_moves_per_descent, time_limit_s,
                   TSP_DLB_OFF, NlStatsOut{stats, sizeof *stats, kNlStats3 | kNlStatsChain});
}

int tsp_dev_ils_dlb(tsp_dev_inst *inst, int kinds, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                    uint64_t seed, int64_t iterations, int span, int64_t max_moves_per_descent, double time_limit_s, int dlb_mode,
                    tsp_ils_dlb_stats *stats) {
    if (dlb_mode != TSP_DLB_OFF && dlb_mode != TSP_DLB_ON && dlb_mode != TSP_DLB_CLOSE) return TSP_DEV_E_ARG;
    for (int b = 0; b < B && stats; ++b) stats[b].active_nodes = stats[b].closing_scans = 0;   // also when a check below fails
    return ils_run(inst, kinds, B, succ, succ_stride, tour_stride, obj, seed, iterations, span, max_moves_per_descent, time_limit_s,
                   dlb_mode, NlStatsOut{stats, sizeof *stats, kNlStats3 | kNlStatsChain | kNlStatsDlb});
}

int tsp_dev_ils_kick(tsp_dev_inst *inst, int B, int *succ, int succ_stride, int64_t tour_stride, uint64_t seed, int64_t it,
                     int span) {
    if (!inst || !succ || B < 1 || succ_stride < 1 || it < 0 || bad_span(span) || inst->n < 8) return TSP_DEV_E_ARG;
    const int n = inst->n;
    if (B > 1 && tour_stride < (int64_t)n * succ_stride) return TSP_DEV_E_ARG;
    std::vector<double> obj((size_t)B, 0.0);
    Descent run;
    int rc = run.open(inst, B, succ, succ_stride, tour_stride, obj.data());
    if (rc) return rc;
    tsp_dev_tours *t = run.t;
    hipLaunchKernelGGL(k_ils_kick, dim3(B), dim3(kNlPickThreads), 0, inst->ctx->stream, t->d_order, t->d_pos, n,
                       span <= 0 ? n : std::min(span, n), (u64)seed, (long long)it);
    TSP_HIP_TRY(hipGetLastError());
    return tsp_dev_tours_download(t, succ, succ_stride, tour_stride, nullptr, nullptr);   // (synchronises)
}

}  // extern "C"
