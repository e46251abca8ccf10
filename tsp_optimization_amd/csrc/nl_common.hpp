// nl_common.hpp -- what the list descents share: nl_opt.hip (2-opt + Or-opt, tsp_dev_nl_opt) and nl3_opt.hip (those two and the
// 3-opt kind, tsp_dev_nl_3opt).  The decision word, the per-tour state, the symmetric distance, the reversal of a forward path on
// order/pos, the lists and scratch of an instance, and the host functions of nl_opt.hip that nl3_opt.hip drives.
#pragma once
#include "or_opt_shift.hpp"

#pragma clang fp contract(off)

namespace tsp {

constexpr int kNlPickThreads = 1024;
// decision key: the kind above the kind's own key, so that the unsigned order is (kind, key): 2-opt nothing, Or-opt bit 62,
// 3-opt bit 63 (6 n^2 < 2^62; 4 n^3 <= 2^62 for n <= 2^20).  kNoKey (all ones) is no key of any kind.
constexpr u64 kNlOrBit = 1ull << 62;
constexpr u64 kNl3Bit = 1ull << 63;

struct alignas(16) NlBest {
    double d;
    u64 k;
};

struct alignas(16) NlState {
    long long max_moves;   // < 0: unlimited
    long long decisions, moves, moves_2opt, moves_oropt, moves_len[3], moves_rev, reversed, deltas;
    long long moves_3opt, moves_type[4];
    int done, pad;
};

__device__ __forceinline__ void nl_offer(double delta, u64 key, double &bd, u64 &bk) {
    if (delta < 0.0 && better(delta, key, bd, bk)) { bd = delta; bk = key; }
}

// calc_dist of two nodes, the lower id first
template <int WT, bool INT>
__device__ __forceinline__ double dsym(const double2 *coord, int u, int v) {
    const double2 a = coord[min(u, v)], b = coord[max(u, v)];
    return dist_xy<WT, INT>(a.x, a.y, b.x, b.y);
}

// The forward path of `len` nodes that starts at position s (0 <= s < n, 0 <= len <= n; it may wrap past n - 1) is reversed in
// place.  Called by every thread of the one workgroup (NT threads) that owns the tour; the swaps touch disjoint positions, so
// the caller needs a barrier only between two reversals and behind its last read of the old tour.
template <int NT>
__device__ __forceinline__ void nl_reverse_path(int *__restrict__ order, int *__restrict__ pos, int n, int s, int len) {
    for (int q = threadIdx.x; q < len / 2; q += NT) {
        const int pa = or_wrap(s + q, n), pb = or_wrap(s + len - 1 - q, n);
        const int va = order[pa], vb = order[pb];
        order[pa] = vb; pos[vb] = pa;
        order[pb] = va; pos[va] = pb;
    }
}

// Lists and scratch of one instance.
struct NlData {
    int K = 0;                 // 0: no lists
    int *d_nbr = nullptr;      // n x K
    int B = 0, nparts = 0, parts_K = 0;
    NlState *d_st = nullptr;
    NlState *h_st = nullptr;   // pinned
    double *d_E = nullptr, *d_rem = nullptr, *d_cost = nullptr;
    NlBest *d_part = nullptr;  // B x nparts of k_nl_scan, then B x nparts of k_nl3_scan
    void free_scratch() {
        (void)hipFree(d_st); (void)hipHostFree(h_st); (void)hipFree(d_E); (void)hipFree(d_rem); (void)hipFree(d_cost);
        (void)hipFree(d_part);
        d_st = nullptr; h_st = nullptr; d_E = d_rem = d_cost = nullptr; d_part = nullptr; B = 0;
    }
    ~NlData() { free_scratch(); (void)hipFree(d_nbr); }
};

}  // namespace tsp

// nl_opt.hip
double tsp_nl_wall_s();
// k_nl_prep, then k_nl_scan when kinds has one of its two: the edge lengths E, and one candidate per workgroup in the first
// B x nparts entries of d_part
void tsp_nl_launch_scan(tsp_dev_tours *t, tsp::NlData *x, int kinds);
// One whole decision (scans, pick, apply) of every tour that is not done, queued on the engine's stream.
typedef void (*tsp_nl_decision_fn)(tsp_dev_tours *t, tsp::NlData *x, int kinds);
// The descent both entry points run: upload, the default lists, `decision` queued in growing batches until every tour is done,
// the cost of the final tours, download.  `kinds` already holds only kinds that have a move at this size.  On return (>= 0)
// x->h_st[0 .. B-1] are the final states, *t0 the call's start on the host clock, *ms the device time.
int tsp_nl_descend(tsp_dev_inst *inst, int kinds, tsp_nl_decision_fn decision, int B, int *succ, int succ_stride,
                   int64_t tour_stride, double *obj, int64_t max_moves, double time_limit_s, tsp::NlData **xo, double *t0o, float *ms);
