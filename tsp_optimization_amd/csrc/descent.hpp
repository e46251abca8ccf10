// descent.hpp -- the host side of a descent on order/pos that the device drives through per-tour control blocks: Or-opt
// (or_opt.hip) and the list descents (nl_opt.hip, nl3_opt.hip).  The kernels of a decision return at once for a tour whose block
// says `done`; the host only queues decisions and polls.
#pragma once
#include "tsp_internal.hpp"

#include <algorithm>

namespace tsp {

// What a driver adds to Descent::run when a tour is not finished at its first `done` (ils.hip).  DescentPlain: nothing.
//   init(z, b)      the start of control block b, behind run's own
//   fetch(s)        queues the copies of the driver's own state that a poll needs, behind run's copy of the control blocks
//   finished(z, b)  after a poll: tour b needs no more decisions
//   finish(status)  queued behind the last decision, ahead of the recomputed costs and the download
struct DescentPlain {
    template <typename State> void init(State &, int) const {}
    int fetch(hipStream_t) const { return TSP_OK; }
    template <typename State> bool finished(const State &z, int) const { return z.done; }
    int finish(int) const { return TSP_OK; }
};

// open(): the scratch tours handle of the instance with the caller's tours on it.  run(): the decisions, the cost of the final
// tours and the way back to the caller's arrays.  Between the two the caller sees to its own buffers (and lists).
struct Descent {
    tsp_dev_tours *t = nullptr;
    double t0 = 0.0;         // the call's start on the host clock
    float device_ms = 0.f;   // from the first decision to the recomputed costs

    Descent() = default;
    Descent(const Descent &) = delete;
    Descent &operator=(const Descent &) = delete;
    ~Descent() { if (owned_) tsp_dev_tours_destroy(t); }

    int open(tsp_dev_inst *inst, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj) {
        t0 = wall_s();
        TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
        int rc = TSP_OK;
        t = tsp_scratch_tours(inst, B, &owned_, &rc);
        if (rc) return rc;
        succ_ = succ; succ_stride_ = succ_stride; tour_stride_ = tour_stride; obj_ = obj;
        return tsp_dev_tours_upload(t, succ, succ_stride, tour_stride, obj);   // checks every successor list
    }

    // State: the per-tour control block (d_st on the device, h_st pinned, B of each), with `max_moves` (< 0: unlimited) and
    // `done`; everything else in it starts at zero.  queue(first) queues one decision of every tour on the engine's stream.
    // `trivial`: no tour has a move to look for.  Decisions are queued in batches that double up to batch_cap.  Returns TSP_OK
    // or TSP_TIME_LIMIT_EXCEEDED with the final states in h_st and the recomputed costs in obj, or an error.
    template <typename State, typename Queue>
    int run(State *d_st, State *h_st, double *d_cost, bool trivial, int batch_cap, int64_t max_moves, double time_limit_s,
            Queue queue) {
        return run(d_st, h_st, d_cost, trivial, batch_cap, max_moves, time_limit_s, queue, DescentPlain{});
    }

    template <typename State, typename Queue, typename Hooks>
    int run(State *d_st, State *h_st, double *d_cost, bool trivial, int batch_cap, int64_t max_moves, double time_limit_s,
            Queue queue, Hooks hooks) {
        tsp_dev_inst *inst = t->inst;
        hipStream_t s = inst->ctx->stream;
        const int B = t->B;
        for (int b = 0; b < B; ++b) {
            State z;
            memset(&z, 0, sizeof z);
            z.max_moves = max_moves < 0 ? -1 : max_moves;
            z.done = trivial ? 1 : 0;
            hooks.init(z, b);
            h_st[b] = z;
        }
        TSP_HIP_TRY(hipMemcpyAsync(d_st, h_st, sizeof(State) * B, hipMemcpyHostToDevice, s));
        if (int e = tsp_inst_events(inst)) return e;
        TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
        int status = TSP_OK;
        if (!trivial) {
            double tq = wall_s();
            queue(true);
            int batch = 4, queued = 1;
            for (;;) {
                TSP_HIP_TRY(hipMemcpyAsync(h_st, d_st, sizeof(State) * B, hipMemcpyDeviceToHost, s));
                if (int e = hooks.fetch(s)) return e;
                TSP_HIP_TRY(hipStreamSynchronize(s));
                TSP_HIP_TRY(hipGetLastError());
                bool all = true;
                for (int b = 0; b < B; ++b) all = all && hooks.finished(h_st[b], b);
                if (all) break;
                const double now = wall_s();
                if (time_limit_s > 0 && now - t0 > time_limit_s) { status = TSP_TIME_LIMIT_EXCEEDED; break; }
                int next = batch;
                if (time_limit_s > 0) {
                    // no more decisions than the budget left holds at the last batch's rate: the overshoot stays within about
                    // one decision however long a decision takes (a full sweep of a large instance)
                    const double per = (now - tq) / queued, left = time_limit_s - (now - t0);
                    if (per > 0.0) next = (int)std::max(1.0, std::min((double)batch, left / per));
                }
                // decisions queued back to back; those behind a tour's last one return at once (done)
                tq = now;
                for (int k = 0; k < next; ++k) queue(false);
                queued = next;
                batch = std::min(batch * 2, batch_cap);
            }
        }
        if (int e = hooks.finish(status)) return e;
        if (int e = tsp_grid_tour_cost(t, d_cost)) return e;
        TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
        TSP_HIP_TRY(hipEventSynchronize(inst->ev1));
        TSP_HIP_TRY(hipGetLastError());
        TSP_HIP_TRY(hipEventElapsedTime(&device_ms, inst->ev0, inst->ev1));
        std::vector<double> cost((size_t)B);
        TSP_HIP_TRY(hipMemcpyAsync(cost.data(), d_cost, sizeof(double) * B, hipMemcpyDeviceToHost, s));
        TSP_HIP_TRY(hipMemcpyAsync(h_st, d_st, sizeof(State) * B, hipMemcpyDeviceToHost, s));
        if (int e = tsp_dev_tours_download(t, succ_, succ_stride_, tour_stride_, nullptr, nullptr)) return e;   // (synchronises)
        for (int b = 0; b < B; ++b) obj_[b] = cost[b];
        return status;
    }

private:
    bool owned_ = false;
    int *succ_ = nullptr;
    int succ_stride_ = 0;
    int64_t tour_stride_ = 0;
    double *obj_ = nullptr;
};

}  // namespace tsp
