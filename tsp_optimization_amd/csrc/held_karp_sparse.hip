// held_karp_sparse.hip -- 1-trees over the candidate graph of the handle's lists (tsp_dev_one_tree_sparse) and the two-phase
// ascent: penalties from sparse trees, the bound from dense ones (tsp_dev_held_karp_sparse).  The definitions
// are in include/tsp_hip.h; the control block, the scratch and the round kernels are hk_common.hpp's.
//
// Call     k_hks_dist once: d(lo, hi) of every list entry and, for the entries at node 0, flag and distance of the other end.
// Tree     k_hk_init -> Rs rounds over the list entries -> k_hks_gate (the sparse rounds must have left exactly the candidate
//          graph's components; the first tree records that number, which no penalty changes) -> Rc rounds of the dense kernels
//          when there are several components -> k_hks_finish (hk_finish_body<SP = true>).
// Round r  k_hks_scan1 (one lane per entry (v, k): the weight of {v, nbr[v][k]} when its ends lie in two components, into both
//          components' smallest weight) -> k_hks_scan2 (the entries that hold their component's weight: the smallest (lo, hi))
//          -> k_hk_hook -> k_hk_relabel, both unchanged.  An entry serves both ends of its edge, so no adjacency structure is
//          needed and a node that every list names costs contention on one word, not a long row.
// Minima are 64-bit integer atomics as in the dense rounds; no floating-point atomic, every sum a fixed tree in one workgroup.
// Queueing is blind as in the dense ascent: Rs = (sparse rounds of the last tree) + 1; a tree whose sparse rounds were too few
// raises `stop` in k_hks_gate (a round in which nothing hooks does not read as "finished": the component count decides).
#include "hk_common.hpp"

namespace {

// entry e = (v, k), v = e / K: d(lo, hi) with the lower id first, as pair_weight takes it
template <int WT, bool INT>
__global__ __launch_bounds__(256) void k_hks_dist(const double2 *__restrict__ coord, int K, long long M, const int *__restrict__ nbr,
                                                  double *__restrict__ ed, unsigned char *__restrict__ zflag, double *__restrict__ zd) {
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e >= M) return;
    const int v = (int)(e / K), u = nbr[e];
    const int lo = min(v, u), hi = max(v, u);
    const double2 a = coord[lo], b = coord[hi];
    const double d = pair_dist<WT, INT>(lo, a.x, a.y, hi, b.x, b.y);
    ed[e] = d;
    if (lo == 0) { zflag[hi] = 1; zd[hi] = d; }   // entries that name the same edge store the same bits
}

__global__ __launch_bounds__(256) void k_hks_scan1(const HkCol *__restrict__ col, const HkCtl *__restrict__ ctl,
                                                   HkSpCtl *__restrict__ sctl, int r, int K, long long M,
                                                   const int *__restrict__ nbr, const double *__restrict__ ed,
                                                   hk_u64 *__restrict__ entk, hk_u64 *__restrict__ compw) {
    if (hk_idle(ctl) || ctl->ncomp[r] <= 1) return;
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    if (e == 0) sctl->weights += M;
    bool valid = false;
    int tv = 0, tu = 0;
    hk_u64 key = kNone;
    if (e < M) {
        const int v = (int)(e / K), u = nbr[e];
        if (v >= 1 && u >= 1) {   // node 0 is not part of the spanning tree
            tv = col[v].tag; tu = col[u].tag;
            if (tv != tu) {
                const double pv = col[v].pi, pu = col[u].pi;
                const double w = (ed[e] + (v < u ? pv : pu)) + (v < u ? pu : pv);
                key = ord_of(w);
                valid = true;
            }
        }
        entk[e] = key;
    }
    comp_atomic_min(compw, tv, key, valid);
    comp_atomic_min(compw, tu, key, valid);
}

__global__ __launch_bounds__(256) void k_hks_scan2(const HkCol *__restrict__ col, const HkCtl *__restrict__ ctl, int r, int K,
                                                   long long M, const int *__restrict__ nbr, const hk_u64 *__restrict__ entk,
                                                   const hk_u64 *__restrict__ compw, hk_u64 *__restrict__ compe) {
    if (hk_idle(ctl) || ctl->ncomp[r] <= 1) return;
    const long long e = blockIdx.x * 256ll + threadIdx.x;
    bool av = false, au = false;
    int tv = 0, tu = 0;
    hk_u64 key = kNone;
    if (e < M) {
        const hk_u64 k = entk[e];
        if (k != kNone) {
            const int v = (int)(e / K), u = nbr[e];
            tv = col[v].tag; tu = col[u].tag;
            av = compw[tv] == k; au = compw[tu] == k;
            key = ((hk_u64)(unsigned)min(v, u) << 32) | (hk_u64)(unsigned)max(v, u);
        }
    }
    comp_atomic_min(compe, tv, key, av);
    comp_atomic_min(compe, tu, key, au);
}

// Behind the sparse rounds: they must have left the candidate graph's components (expect < 0: record them).
__global__ void k_hks_gate(HkCtl *__restrict__ ctl, HkSpCtl *__restrict__ sctl, int Rs, int expect) {
    if (hk_idle(ctl)) return;
    const int c = ctl->ncomp[Rs];
    if (expect < 0) sctl->components = c;
    else if (c != expect) ctl->stop = 1;
}

template <int WT, bool INT>
__global__ __launch_bounds__(kFinThreads) void k_hks_finish(const HkCol *__restrict__ col, HkCtl *__restrict__ ctl, int R, int n,
                                                            int ascent, double *__restrict__ pi, double *__restrict__ pi_best,
                                                            int *__restrict__ gprev, int *__restrict__ deg, int *__restrict__ elo,
                                                            int *__restrict__ ehi, double *__restrict__ ew, HkSpFin sp) {
    hk_finish_body<WT, INT, true>(col, ctl, R, n, ascent, pi, pi_best, gprev, deg, elo, ehi, ew, &sp);
}

struct SpRun {
    HkData *x = nullptr;
    int K = 0;
    const int *d_nbr = nullptr;
    long long M = 0;
    int comps = -1;    // components of the candidate graph on nodes 1 .. n-1; -1 until the first tree has counted them
    int Rc = 0;        // completion rounds queued per tree
    int Rs_full = 0;   // sparse rounds that exhaust any tree (as far as kHkMaxRounds lets them)
    float dist_ms = 0.f;
};

// init, Rs rounds over the entries, the gate
void queue_sparse_head(tsp_dev_inst *inst, const SpRun &run, int Rs, int expect) {
    hipStream_t s = inst->ctx->stream;
    HkData *x = run.x;
    const int n = x->n;
    const int gn = (n + 255) / 256, ge = (int)((run.M + 255) / 256);
    queue_init(inst, x);
    for (int r = 0; r < Rs; ++r) {
        hipLaunchKernelGGL(k_hks_scan1, dim3(ge), dim3(256), 0, s, x->d_col, x->d_ctl, x->d_sctl, r, run.K, run.M, run.d_nbr, x->d_ed,
                           x->d_entk, x->d_compw);
        hipLaunchKernelGGL(k_hks_scan2, dim3(ge), dim3(256), 0, s, x->d_col, x->d_ctl, r, run.K, run.M, run.d_nbr, x->d_entk,
                           x->d_compw, x->d_compe);
        hipLaunchKernelGGL(k_hk_hook, dim3(gn), dim3(256), 0, s, x->d_col, x->d_ctl, r, n, 0, x->d_compw, x->d_compe, x->d_parent,
                           x->d_deg, x->d_elo, x->d_ehi, x->d_ew);   // rows = 0: `dists` counts the completion's scans alone
        hipLaunchKernelGGL(k_hk_relabel, dim3(gn), dim3(256), 0, s, x->d_col, x->d_ctl, r, n, x->d_parent, x->d_compw, x->d_compe);
    }
    hipLaunchKernelGGL(k_hks_gate, dim3(1), dim3(1), 0, s, x->d_ctl, x->d_sctl, Rs, expect);
}

// the completion's rounds and the closing kernel
void queue_sparse_tail(tsp_dev_inst *inst, const SpRun &run, int Rs, int Rc, int ascent) {
    HkData *x = run.x;
    const HkSpFin sp = {x->d_zflag, x->d_zd, x->d_sctl, Rs};
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        queue_dense_rounds<WTC, INTC>(inst, x, Rs, Rs + Rc);
        hipLaunchKernelGGL((k_hks_finish<WTC, INTC>), dim3(1), dim3(kFinThreads), 0, inst->ctx->stream, x->d_col, x->d_ctl, Rs + Rc,
                           x->n, ascent, x->d_pi, x->d_pi_best, x->d_gprev, x->d_deg, x->d_elo, x->d_ehi, x->d_ew, sp);
    });
}

int poll_both(tsp_dev_inst *inst, HkData *x) {
    hipStream_t s = inst->ctx->stream;
    TSP_HIP_TRY(hipMemcpyAsync(x->h_sctl, x->d_sctl, sizeof(HkSpCtl), hipMemcpyDeviceToHost, s));
    return poll_ctl(s, x->h_ctl, x->d_ctl);
}

// The call's first tree: all sparse rounds, a look at the component count, then as many dense rounds as it asks for (none for
// connected lists).
int first_tree(tsp_dev_inst *inst, SpRun *run, int ascent) {
    HkData *x = run->x;
    const int Rs = std::min(x->Rmax, kHkMaxRounds);
    queue_sparse_head(inst, *run, Rs, -1);
    int rc = poll_both(inst, x);
    if (rc) return rc;
    run->comps = x->h_sctl->components;
    int need = 0;
    while ((1ll << need) < run->comps) need += 1;
    run->Rc = run->comps > 1 ? need + 1 : 0;
    if (need > kHkMaxRounds - 1) {
        tsp::set_last_error_text("held_karp_sparse: the candidate graph has more components than 32 queued rounds can join");
        return TSP_DEV_E_HIP;
    }
    run->Rc = std::min(run->Rc, kHkMaxRounds - 1);
    run->Rs_full = std::min(x->Rmax, kHkMaxRounds - run->Rc);
    queue_sparse_tail(inst, *run, Rs, std::min(run->Rc, kHkMaxRounds - Rs), ascent);
    return TSP_OK;
}

// The handle's scratch, the lists, the entries' distances and fresh sparse words: everything a call needs before its first tree.
int sp_prepare(tsp_dev_inst *inst, SpRun *run) {
    hipStream_t s = inst->ctx->stream;
    const int n = inst->n;
    int rc = tsp_nl_lists(inst, &run->K, &run->d_nbr);
    if (rc) return rc;
    HkData *x = nullptr;
    rc = hk_alloc(inst, &x);
    if (rc) return rc;
    run->x = x;
    run->M = (long long)n * run->K;
    if (!x->sp_block) {
        const size_t N = (size_t)n, E = N * (size_t)std::min(TSP_NL_MAX_K, n - 1);
        auto lay = [&](Carver &c) { c(x->d_ed, E); c(x->d_entk, E); c(x->d_zd, N); c(x->d_sctl, 1); c(x->d_zflag, N); };
        TSP_HIP_TRY(hipMalloc(&x->sp_block, carve_bytes(lay)));
        carve(x->sp_block, lay);
        x->sp_entries = E;
        TSP_HIP_TRY(hipHostMalloc(&x->h_sctl, sizeof(HkSpCtl), hipHostMallocDefault));
    }
    if ((size_t)run->M > x->sp_entries) {
        tsp::set_last_error_text("held_karp_sparse: the handle's lists are longer than TSP_NL_MAX_K");
        return TSP_DEV_E_HIP;
    }
    if (int e = tsp_inst_events(inst)) return e;
    memset(x->h_sctl, 0, sizeof(HkSpCtl));
    x->h_sctl->components = -1;
    TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
    TSP_HIP_TRY(hipMemcpyAsync(x->d_sctl, x->h_sctl, sizeof(HkSpCtl), hipMemcpyHostToDevice, s));
    TSP_HIP_TRY(hipMemsetAsync(x->d_zflag, 0, (size_t)n, s));
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_hks_dist<WTC, INTC>), dim3((unsigned)((run->M + 255) / 256)), dim3(256), 0, s, inst->d_coord, run->K,
                           run->M, run->d_nbr, x->d_ed, x->d_zflag, x->d_zd);
    });
    TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
    TSP_HIP_TRY(hipEventSynchronize(inst->ev1));
    TSP_HIP_TRY(hipGetLastError());
    TSP_HIP_TRY(hipEventElapsedTime(&run->dist_ms, inst->ev0, inst->ev1));
    return TSP_OK;
}

void fill_sparse(tsp_lb_sparse_stats *st, const SpRun &run, const HkCtl &c, const HkSpCtl &sc, float sparse_ms) {
    st->sparse_iterations = c.iters; st->sparse_trees = c.trees; st->sparse_rounds = sc.sparse_rounds;
    st->completion_rounds = sc.completion_rounds; st->candidate_entries = run.M; st->components = run.comps < 0 ? 0 : run.comps;
    st->weights_executed = sc.weights; st->sparse_best = c.best; st->lambda_sparse_final = c.lambda;
    st->sparse_device_ms = sparse_ms;
}

}  // namespace

static_assert(offsetof(tsp_lb_sparse_stats, sparse_iterations) == sizeof(tsp_lb_stats), "tsp_lb_sparse_stats starts as tsp_lb_stats");

extern "C" {

int tsp_dev_one_tree_sparse(tsp_dev_inst *inst, const double *pi, int *edges, int *deg, double *value, tsp_lb_sparse_stats *stats) {
    if (!inst || inst->n < 3 || !pi_finite(pi, inst->n)) {
        tsp::set_last_error_text("tsp_dev_one_tree_sparse: no instance, fewer than 3 nodes or a penalty that is not finite");
        return TSP_DEV_E_ARG;
    }
    const double t0 = wall_s();
    const int n = inst->n;
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    hipStream_t s = inst->ctx->stream;
    SpRun run;
    int rc = sp_prepare(inst, &run);
    if (rc) return rc;
    HkData *x = run.x;
    HkCtl c0;
    memset(&c0, 0, sizeof c0);
    c0.best = -INFINITY;
    rc = hk_begin(inst, x, pi, c0);
    if (rc) return rc;
    TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
    rc = first_tree(inst, &run, 0);
    if (rc) return rc;
    TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
    rc = poll_both(inst, x);
    if (rc) return rc;
    float ms = 0.f;
    TSP_HIP_TRY(hipEventElapsedTime(&ms, inst->ev0, inst->ev1));
    if (x->h_ctl->stop || x->h_ctl->trees != 1) {
        tsp::set_last_error_text("tsp_dev_one_tree_sparse: the Boruvka rounds did not end in one component");
        return TSP_DEV_E_HIP;
    }
    if (value) *value = x->h_ctl->W;
    if (deg) TSP_HIP_TRY(hipMemcpy(deg, x->d_deg, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    if (edges) {
        std::vector<int> lo((size_t)n + 1), hi((size_t)n + 1);
        TSP_HIP_TRY(hipMemcpy(lo.data(), x->d_elo, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
        TSP_HIP_TRY(hipMemcpy(hi.data(), x->d_ehi, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
        if (write_sorted_edges(lo.data(), hi.data(), n + 1, edges, n) != n) {
            tsp::set_last_error_text("tsp_dev_one_tree_sparse: the 1-tree does not have n edges");
            return TSP_DEV_E_HIP;
        }
    }
    if (stats) {
        memset(stats, 0, sizeof *stats);
        fill_sparse(stats, run, *x->h_ctl, *x->h_sctl, ms + run.dist_ms);
        stats->sparse_best = x->h_ctl->W;
        stats->dists_executed = x->h_ctl->dists;   // the completion's dense scans; 0 for connected lists
        stats->seconds = wall_s() - t0; stats->device_ms = ms + run.dist_ms;
    }
    return TSP_OK;
}

int tsp_dev_held_karp_sparse(tsp_dev_inst *inst, double ub, int sparse_iters, int dense_iters, double lambda0, int patience,
                             double time_limit_s, double *pi, double *bound, tsp_lb_sparse_stats *stats) {
    if (!inst || inst->n < 3 || !bound || !std::isfinite(ub) || !(ub > 0.0) || sparse_iters < 0 || dense_iters < 1 ||
        !std::isfinite(lambda0) || !(lambda0 > 0.0) || !pi_finite(pi, inst ? inst->n : 0)) {
        tsp::set_last_error_text("tsp_dev_held_karp_sparse: needs an instance of 3 or more nodes, a finite ub > 0, sparse_iters >= 0, "
                                 "dense_iters >= 1, lambda0 > 0 and finite penalties");
        return TSP_DEV_E_ARG;
    }
    const double t0 = wall_s();
    const int n = inst->n;
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    hipStream_t s = inst->ctx->stream;
    SpRun run;
    int rc = sp_prepare(inst, &run);
    if (rc) return rc;
    HkData *x = run.x;
    HkCtl c0;
    memset(&c0, 0, sizeof c0);
    c0.ub = ub; c0.lambda = lambda0; c0.best = -INFINITY; c0.max_iters = sparse_iters; c0.first = 1;
    c0.patience = patience > 0 ? patience : std::max(10, n / 20);
    HkCtl sparse_c = c0;   // what the sparse phase left (as it began, when it has no iteration)
    HkSpCtl sparse_sc = *x->h_sctl;
    float sparse_ms = run.dist_ms;
    bool timed_out = false;
    std::vector<double> start;   // the dense phase's start and result
    if (pi) start.assign(pi, pi + n);
    if (sparse_iters > 0) {
        rc = hk_begin(inst, x, pi, c0);
        if (rc) return rc;
        TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
        int Rs = 0, batch = 1;
        long long left = sparse_iters;
        double per = 0.0;   // seconds per iteration of the last batch
        for (;;) {
            int next = (int)std::min<long long>(batch, left);
            if (time_limit_s > 0 && per > 0.0)
                next = (int)std::max(1.0, std::min((double)next, (time_limit_s - (wall_s() - t0)) / per));
            const double tq = wall_s();
            if (run.comps < 0) {
                next = 1;
                rc = first_tree(inst, &run, 1);
                if (rc) return rc;
            } else {
                for (int k = 0; k < next; ++k) {
                    queue_sparse_head(inst, run, Rs, run.comps);
                    queue_sparse_tail(inst, run, Rs, run.Rc, 1);
                }
            }
            rc = poll_both(inst, x);
            if (rc) return rc;
            const HkCtl &c = *x->h_ctl;
            per = (wall_s() - tq) / next;
            if (c.stop) {
                // a tree needed more sparse rounds than were queued: that iteration and those behind it did nothing
                if (Rs == run.Rs_full || Rs == 0) {
                    tsp::set_last_error_text("tsp_dev_held_karp_sparse: the Boruvka rounds did not end in one component");
                    return TSP_DEV_E_HIP;
                }
                Rs = run.Rs_full;
                TSP_HIP_TRY(hipMemsetAsync(&x->d_ctl->stop, 0, sizeof(int), s));
            } else {
                Rs = std::min(run.Rs_full, x->h_sctl->last_sparse + 1);
            }
            left = sparse_iters - c.iters;
            if (c.done || left <= 0) break;
            if (time_limit_s > 0 && wall_s() - t0 > time_limit_s) { timed_out = true; break; }
            batch = std::min(batch * 2, 64);
        }
        TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
        TSP_HIP_TRY(hipEventSynchronize(inst->ev1));
        float ms = 0.f;
        TSP_HIP_TRY(hipEventElapsedTime(&ms, inst->ev0, inst->ev1));
        sparse_ms += ms;
        sparse_c = *x->h_ctl; sparse_sc = *x->h_sctl;
        start.resize((size_t)n);
        TSP_HIP_TRY(hipMemcpy(start.data(), x->d_pi_best, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    }
    // the dense phase: the public ascent from pi_best_C with the lambda the sparse phase ended on
    double left_s = time_limit_s;
    if (time_limit_s > 0) left_s = std::max(1e-9, time_limit_s - (wall_s() - t0));
    tsp_lb_stats dense;
    memset(&dense, 0, sizeof dense);
    rc = tsp_dev_held_karp(inst, ub, dense_iters, sparse_c.lambda, patience, left_s, start.empty() ? nullptr : start.data(), bound,
                           &dense);
    if (rc != TSP_OK && rc != TSP_TIME_LIMIT_EXCEEDED) return rc;
    if (pi) memcpy(pi, start.data(), sizeof(double) * (size_t)n);
    if (stats) {
        memset(stats, 0, sizeof *stats);
        memcpy(stats, &dense, sizeof dense);
        fill_sparse(stats, run, sparse_c, sparse_sc, sparse_ms);
        stats->seconds = wall_s() - t0; stats->device_ms = dense.device_ms + sparse_ms;
    }
    return timed_out ? TSP_TIME_LIMIT_EXCEEDED : rc;
}

}  // extern "C"
