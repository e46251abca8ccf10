// held_karp.hip -- Held-Karp lower bound: minimum 1-trees under node penalties (tsp_dev_one_tree) and the subgradient ascent
// over them (tsp_dev_held_karp).  The definitions are in include/tsp_hip.h.
//
// Tree     k_hk_init (column records {x, y, pi, tag = component}, every node its own component) -> R Boruvka rounds over nodes
//          1 .. n-1 -> k_hk_finish (one workgroup: the two smallest edges at node 0, W, |g|^2 and, in the ascent, the step).
// Round r  k_hk_scan (a row scan, row_scan.hpp: each lane keeps its smallest edge into another component) -> k_hk_min1 (the
//          chunks merged per node; per component the smallest weight) -> k_hk_min2 (among the nodes that hold it the smallest
//          (lo, hi)) -> k_hk_hook (per root: its component's edge; two components that chose the same edge keep the lower root;
//          the hooked root stores the edge in ITS slot, so no slot is written twice) -> k_hk_relabel.
// The edge order (w, lo, hi) is strict, so the chosen edges never close a cycle and every algorithm returns this tree.  Across
// nodes the minimum goes through 64-bit INTEGER atomic minima (of the ordered bits of w, then of lo << 32 | hi), whose result
// does not depend on arrival order.  No floating-point atomic anywhere; every sum is a fixed tree in one workgroup.
// A tree of R rounds is queued without a wait: round r reads ncomp[r] and adds to ncomp[r + 1], rounds behind the last one
// return at once.  The ascent queues R = (rounds of the last tree) + 1; a tree that is not finished after them raises `stop`,
// which turns everything queued behind it into no-ops, and the host repeats that iteration with the full ceil(log2(n - 1)).
// The kernels, the control block and the scratch are in hk_common.hpp, which held_karp_sparse.hip shares.
#include "hk_common.hpp"

void tsp_hk_data_free(void *p) { delete static_cast<HkData *>(p); }

// The minimum 1-tree of pi (NULL = zeros; the caller has checked it) built and waited for: what alpha.hip works from.
int tsp_hk_tree(tsp_dev_inst *inst, const double *pi, tsp::HkTree *out, tsp_lb_stats *stats) {
    const double t0 = wall_s();
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    hipStream_t s = inst->ctx->stream;
    HkData *x = nullptr;
    int rc = hk_alloc(inst, &x);
    if (rc) return rc;
    HkCtl c0;
    memset(&c0, 0, sizeof c0);
    rc = hk_begin(inst, x, pi, c0);
    if (rc) return rc;
    if (int e = tsp_inst_events(inst)) return e;
    TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
    queue_tree(inst, x, x->Rmax, 0);
    TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
    rc = poll_ctl(s, x->h_ctl, x->d_ctl);
    if (rc) return rc;
    float ms = 0.f;
    TSP_HIP_TRY(hipEventElapsedTime(&ms, inst->ev0, inst->ev1));
    if (x->h_ctl->stop || x->h_ctl->trees != 1) {
        tsp::set_last_error_text("tsp_dev_one_tree: the Boruvka rounds did not end in one component");
        return TSP_DEV_E_HIP;
    }
    out->d_elo = x->d_elo; out->d_ehi = x->d_ehi; out->d_ew = x->d_ew; out->d_pi = x->d_pi;
    out->W = x->h_ctl->W; out->rounds = x->h_ctl->rounds; out->device_ms = ms;
    fill_stats(stats, *x->h_ctl, t0, ms);
    return TSP_OK;
}

extern "C" {

int tsp_dev_one_tree(tsp_dev_inst *inst, const double *pi, int *edges, int *deg, double *value, tsp_lb_stats *stats) {
    if (!inst || inst->n < 3 || !pi_finite(pi, inst->n)) {
        tsp::set_last_error_text("tsp_dev_one_tree: no instance, fewer than 3 nodes or a penalty that is not finite");
        return TSP_DEV_E_ARG;
    }
    const int n = inst->n;
    tsp::HkTree tr;
    int rc = tsp_hk_tree(inst, pi, &tr, stats);
    if (rc) return rc;
    HkData *x = static_cast<HkData *>(inst->hk_data);
    if (value) *value = x->h_ctl->W;
    if (deg) TSP_HIP_TRY(hipMemcpy(deg, x->d_deg, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    if (edges) {
        std::vector<int> lo((size_t)n + 1), hi((size_t)n + 1);
        TSP_HIP_TRY(hipMemcpy(lo.data(), x->d_elo, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
        TSP_HIP_TRY(hipMemcpy(hi.data(), x->d_ehi, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
        if (write_sorted_edges(lo.data(), hi.data(), n + 1, edges, n) != n) {
            tsp::set_last_error_text("tsp_dev_one_tree: the 1-tree does not have n edges");
            return TSP_DEV_E_HIP;
        }
    }
    return TSP_OK;
}

int tsp_dev_held_karp(tsp_dev_inst *inst, double ub, int max_iters, double lambda0, int patience, double time_limit_s, double *pi,
                      double *bound, tsp_lb_stats *stats) {
    if (!inst || inst->n < 3 || !bound || !std::isfinite(ub) || !(ub > 0.0) || max_iters < 1 || !std::isfinite(lambda0) ||
        !(lambda0 > 0.0) || !pi_finite(pi, inst ? inst->n : 0)) {
        tsp::set_last_error_text("tsp_dev_held_karp: needs an instance of 3 or more nodes, a finite ub > 0, max_iters >= 1, lambda0 > 0 "
                                 "and finite penalties");
        return TSP_DEV_E_ARG;
    }
    const double t0 = wall_s();
    const int n = inst->n;
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    hipStream_t s = inst->ctx->stream;
    HkData *x = nullptr;
    int rc = hk_alloc(inst, &x);
    if (rc) return rc;
    HkCtl c0;
    memset(&c0, 0, sizeof c0);
    c0.ub = ub; c0.lambda = lambda0; c0.best = -INFINITY; c0.max_iters = max_iters; c0.first = 1;
    c0.patience = patience > 0 ? patience : std::max(10, n / 20);
    rc = hk_begin(inst, x, pi, c0);
    if (rc) return rc;
    if (int e = tsp_inst_events(inst)) return e;
    TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
    int status = TSP_OK, R = x->Rmax, batch = 1;
    long long left = max_iters;
    double per = 0.0;   // seconds per iteration of the last batch
    for (;;) {
        int next = (int)std::min<long long>(batch, left);
        if (time_limit_s > 0 && per > 0.0)   // no more iterations than the budget left holds at the last batch's rate
            next = (int)std::max(1.0, std::min((double)next, (time_limit_s - (wall_s() - t0)) / per));
        const double tq = wall_s();
        for (int k = 0; k < next; ++k) queue_tree(inst, x, R, 1);
        rc = poll_ctl(s, x->h_ctl, x->d_ctl);
        if (rc) return rc;
        const HkCtl &c = *x->h_ctl;
        per = (wall_s() - tq) / next;
        if (c.stop) {
            // a tree needed more rounds than were queued: that iteration and those behind it did nothing
            if (R == x->Rmax) {
                tsp::set_last_error_text("tsp_dev_held_karp: the Boruvka rounds did not end in one component");
                return TSP_DEV_E_HIP;
            }
            R = x->Rmax;
            TSP_HIP_TRY(hipMemsetAsync(&x->d_ctl->stop, 0, sizeof(int), s));
        } else {
            R = std::min(x->Rmax, c.last_rounds + 1);
        }
        left = max_iters - c.iters;
        if (c.done || left <= 0) break;
        if (time_limit_s > 0 && wall_s() - t0 > time_limit_s) { status = TSP_TIME_LIMIT_EXCEEDED; break; }
        batch = std::min(batch * 2, 64);
    }
    TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
    TSP_HIP_TRY(hipEventSynchronize(inst->ev1));
    float ms = 0.f;
    TSP_HIP_TRY(hipEventElapsedTime(&ms, inst->ev0, inst->ev1));
    *bound = x->h_ctl->best;
    if (pi) TSP_HIP_TRY(hipMemcpy(pi, x->d_pi_best, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    fill_stats(stats, *x->h_ctl, t0, ms);
    return status;
}

}  // extern "C"
