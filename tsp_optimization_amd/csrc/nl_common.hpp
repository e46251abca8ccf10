// nl_common.hpp -- what the list descents share: nl_opt.hip (2-opt + Or-opt, tsp_dev_nl_opt) and nl3_opt.hip (those two and the
// 3-opt kind, tsp_dev_nl_3opt).  The decision word, the per-tour state, the symmetric distance, the reversal of a forward path on
// order/pos, the lists and scratch of an instance, where a call's stats records go (NlStatsOut), the hooks and the DLB dispatch of
// the launches, the move itself (nl_apply_move), the per-node scan form and the scratch of the batched descent (nl_batch.hip), and
// the host functions the files call in each other (ils.hip too).
#pragma once
#include "descent.hpp"
#include "nl_arc.hpp"
#include "or_opt_shift.hpp"

#pragma clang fp contract(off)

namespace tsp {

constexpr int kNlPickThreads = 1024;
// decision key: the kind above the kind's own key, so that the unsigned order is (kind, key): 2-opt nothing, Or-opt bit 62,
// 3-opt bit 63 (6 n^2 < 2^62; 4 n^3 <= 2^62 for n <= 2^20).  kNoKey (all ones) is no key of any kind.  The kinds' own keys: or_key /
// or_unkey (or_opt_shift.hpp), nl3_key / nl3_unkey (nl_arc.hpp, which the host compiler reads too).
constexpr u64 kNlOrBit = 1ull << 62;
constexpr u64 kNl3Bit = 1ull << 63;
constexpr int kNlMaxN3 = 1 << 20;   // 4 n^3 must stay below the kind bits of the decision key

struct alignas(16) NlBest {
    double d;
    u64 k;
};

struct alignas(16) NlState {
    long long max_moves;   // < 0: unlimited
    long long decisions, moves, moves_2opt, moves_oropt, moves_len[3], moves_rev, reversed, deltas;
    long long moves_3opt, moves_type[4];
    long long active_nodes, closing_scans;   // don't-look bits: sum of |A| over the decisions, times A was reset to V
    int done;
    int nact;                                // don't-look bits: |A|, the entries of the tour's row of NlDlb::list
};

// Don't-look bits: the active set A of every tour, as a bitmap and as a list without duplicates in no
// particular order, and what the lanes of a decision's scans report per node.  Between two decisions hit is all zero.
struct NlDlb {
    unsigned char *act;   // B x n: 1 = the node is in A
    unsigned char *hit;   // B x n: a lane of the node held an improving move in this decision (same-value plain stores)
    int *list;            // B x n: the nodes of A, NlState::nact of them
    int mode;             // TSP_DLB_ON or TSP_DLB_CLOSE
};

// The per-node form of the scans (batched descent): cand[b n + v] = the best (delta, key) that the K lanes of
// node v offer over the moves whose arc (nl_arc.hpp) has at most max_arc positions, (+inf, kNoKey) when there is none.  merge:
// the slot already holds the candidate of the scan before this one.
struct NlPn {
    NlBest *cand;
    int max_arc;
    int merge;
};

// Per-tour control words of a batched decision (nl_batch.hip).
struct NlbCtl {
    int nacc;     // accepted moves appended by the claim rounds of this decision
    int napply;   // entries of the tour's row of the accepted list that k_nlb_apply carries out
    int keep;     // >= 0: only the `keep` smallest of them by (delta, key) (max_moves cuts the batch)
    int pad;
};

// Per-chain state of the iterated local search (ils.hip), written by thread 0 of k_ils_step.
struct alignas(16) IlsState {
    long long it;              // iterations completed; -1 until the first descent has ended
    long long accepted, last_improved;
    double cost, start_cost;   // of the incumbent; after the first descent
    int finished, pad;
};

__device__ __forceinline__ int ahead(int px, int from, int n) {   // px - from mod n
    const int g = px - from;
    return g < 0 ? g + n : g;
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

// The move `bk` of whichever kind on order/pos and in the counters.  Called by every thread of the one workgroup (NT threads) that
// owns the tour, with nothing of the tour written since the last barrier.
template <int NT>
__device__ __forceinline__ void nl_apply_move(int *__restrict__ order, int *__restrict__ pos, NlState &S, int n, u64 bk) {
    const int tid = threadIdx.x;
    if (bk & kNl3Bit) {
        const Nl3Move m = nl3_unkey(bk & (kNl3Bit - 1), n);
        const int T = m.type();
        const int c = m.c(), b = m.b(), a = m.a();
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
    const OrMove mv = or_unkey(bk & (kNlOrBit - 1), n);
    const int L = mv.L, o = mv.o;
    const int i = pos[mv.f], ja = pos[mv.a];
    int x[3] = {0, 0, 0};
    for (int q = 0; q < L; ++q) x[q] = order[or_wrap(i + q, n)];
    __syncthreads();   // every thread has read the tour before anything moves
    if (tid == 0) {
        S.moves += 1; S.moves_oropt += 1; S.moves_len[L - 1] += 1; S.moves_rev += o;
        if (S.max_moves >= 0 && S.moves >= S.max_moves) S.done = 1;
    }
    or_shift_apply<NT>(order, pos, n, i, ja, L, o, x);
}

// The lanes of the per-node scan forms: thread tid of workgroup wg is lane tid % K of node wg * (256 / K) + tid / K; the threads
// behind the workgroup's last whole node, and the nodes behind n - 1, have no lane.
__device__ __forceinline__ bool nl_pn_lane(int n, int K, int *v, long long *e) {
    const int npw = 256 / K, loc = (int)threadIdx.x / K;
    *v = (int)blockIdx.x * npw + loc;
    *e = (long long)*v * K + ((int)threadIdx.x - loc * K);
    return loc < npw && *v < n;
}

// ... and their reduction to one candidate per node: every thread of the workgroup calls it with its lane's best short-arc move
// ((+inf, kNoKey) without one, or without a lane); the node's first lane folds the K of them and writes or merges the slot.
__device__ __forceinline__ void nl_pn_reduce(double cd, u64 ck, bool on, int K, int v, NlBest *__restrict__ cand, int merge,
                                             double *pd, u64 *pk) {
    const int tid = threadIdx.x;
    pd[tid] = cd; pk[tid] = ck;
    __syncthreads();
    if (on && tid % K == 0) {
        for (int k = 1; k < K; ++k)
            if (pk[tid + k] != kNoKey && better(pd[tid + k], pk[tid + k], cd, ck)) { cd = pd[tid + k]; ck = pk[tid + k]; }
        if (merge) {
            const NlBest q = cand[v];
            if (q.k != kNoKey && better(q.d, q.k, cd, ck)) { cd = q.d; ck = q.k; }
        }
        cand[v] = NlBest{cd, ck};
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
    // ils.hip, allocated by its first call at this B: the incumbents' order and pos (B x n each) and the chains' states
    int *d_inc = nullptr;
    IlsState *d_ils = nullptr;
    IlsState *h_ils = nullptr; // pinned
    // don't-look bits, allocated by the first call at this B that asks for them: NlDlb::act, hit (B x n bytes each) and list
    unsigned char *d_act = nullptr, *d_hit = nullptr;
    int *d_alist = nullptr;
    NlDlb dlb(int mode) const { return NlDlb{d_act, d_hit, d_alist, mode}; }
    // batched descent (nl_batch.hip), allocated by the first batched call at this B: the per-node candidates and the accepted
    // list (B x n each), the claim words (B x n images of delta, then B x n keys), the taken map (B x n), the control words
    // and the overall candidates of the per-node scans (B x bparts of k_nl_scan, then of k_nl3_scan)
    NlBest *d_cand = nullptr, *d_acc = nullptr, *d_bpart = nullptr;
    u64 *d_clm = nullptr;
    int *d_taken = nullptr;
    NlbCtl *d_bctl = nullptr;
    int bparts = 0;
    // windowed iterated local search (seg_ils.hip), allocated by its first call at this B: accepted trials per chain
    u64 *d_seg_acc = nullptr;
    // ... with groups: offers and commits per chain (2 x B), and the groups' records, grown to what a call needs (seg_rec_len ints)
    u64 *d_seg_grp = nullptr;
    int *d_seg_rec = nullptr;
    size_t seg_rec_len = 0;
    // ... with the chain kind: its four counters per chain (4 x B)
    u64 *d_seg_lk = nullptr;
    void free_scratch() {
        (void)hipFree(d_seg_acc); (void)hipFree(d_seg_grp); (void)hipFree(d_seg_rec); (void)hipFree(d_seg_lk);
        d_seg_acc = d_seg_grp = d_seg_lk = nullptr; d_seg_rec = nullptr; seg_rec_len = 0;
        (void)hipFree(d_st); (void)hipHostFree(h_st); (void)hipFree(d_E); (void)hipFree(d_rem); (void)hipFree(d_cost);
        (void)hipFree(d_part); (void)hipFree(d_inc); (void)hipFree(d_ils); (void)hipHostFree(h_ils);
        d_st = nullptr; h_st = nullptr; d_E = d_rem = d_cost = nullptr; d_part = nullptr; B = 0;
        d_inc = nullptr; d_ils = nullptr; h_ils = nullptr;
        (void)hipFree(d_act); (void)hipFree(d_hit); (void)hipFree(d_alist);
        d_act = d_hit = nullptr; d_alist = nullptr;
        (void)hipFree(d_cand); (void)hipFree(d_acc); (void)hipFree(d_bpart); (void)hipFree(d_clm); (void)hipFree(d_taken);
        (void)hipFree(d_bctl);
        d_cand = d_acc = d_bpart = nullptr; d_clm = nullptr; d_taken = nullptr; d_bctl = nullptr; bparts = 0;
    }
    ~NlData() { free_scratch(); (void)hipFree(d_nbr); }
};

// What Descent::run needs to know of a list descent beyond its NlState: with don't-look bits |A| at the start (else nact is NULL).
struct NlHooks : DescentPlain {
    const int *nact = nullptr;
    void init(NlState &z, int b) const { if (nact) z.nact = nact[b]; }
};

// Where the stats records of a call go: B records `stride` bytes apart, of the public type that `parts` names.  Every record type
// starts as tsp_nl_opt_stats; kNlStats3 adds the 3-opt counters (tsp_nl3_opt_stats), kNlStatsChain the fields of a chain behind
// them (tsp_ils_stats), kNlStatsDlb the two don't-look counters behind whatever else it has (tsp_nl_dlb_stats, tsp_ils_dlb_stats).
enum { kNlStats3 = 1, kNlStatsChain = 2, kNlStatsDlb = 4 };
struct NlStatsOut {
    void *p;   // may be NULL: no records
    size_t stride;
    int parts;
};

}  // namespace tsp

// Runs the statements with the compile-time constant DLBC = (dlb_mode != 0): one launch site for both forms of a kernel.
#define TSP_DISPATCH_DLB(DLB_RT, ...)                           \
    do {                                                        \
        auto dlb_call__ = [&](auto dlb_c) {                     \
            constexpr bool DLBC = decltype(dlb_c)::value;       \
            __VA_ARGS__                                         \
        };                                                      \
        if (!(DLB_RT)) dlb_call__(std::false_type{}); else dlb_call__(std::true_type{}); \
    } while (0)

// nl_opt.hip: record b of `out` from the final state of its tour: the groups the record type has and nothing behind them.  q: the
// chain's state, or NULL (no chain ran: no iterations, last_improved -1).  start_cost: of a chain whose first descent has not
// ended (q NULL, or q->it < 0).
void tsp_nl_write_stats(const tsp::NlStatsOut &out, int b, const tsp::NlState &z, const tsp::IlsState *q, double start_cost,
                        double seconds, float device_ms);
// nl3_opt.hip: k_nl3_scan of every tour that is not done, one candidate per workgroup in parts3 (B x nparts); dlb_mode != 0: over
// the lanes of the active nodes alone
void tsp_nl3_launch_scan(tsp_dev_tours *t, tsp::NlData *x, tsp::NlBest *parts3, int dlb_mode);
// nl_opt.hip, nl3_opt.hip: the per-node forms (NlPn) of k_nl_prep + k_nl_scan and of k_nl3_scan for the batched descent: a workgroup
// owns 256 / K whole nodes, grid x = nparts workgroups a tour, one overall candidate per workgroup in parts (B x nparts)
void tsp_nl_launch_scan_pn(tsp_dev_tours *t, tsp::NlData *x, int kinds, int nparts, tsp::NlBest *parts, const tsp::NlPn &pn);
void tsp_nl3_launch_scan_pn(tsp_dev_tours *t, tsp::NlData *x, int nparts, tsp::NlBest *parts3, const tsp::NlPn &pn);
// nl_opt.hip: the argument checks of a list descent; *kinds loses the kinds without a move at the instance's size
int tsp_nl_check(const tsp_dev_inst *inst, int *kinds, int allowed, int B, const int *succ, int succ_stride, int64_t tour_stride,
                 const double *obj);
// nl_opt.hip: the instance's lists (the default lists when it has none) and the scratch of B tours -> *x
int tsp_nl_prepare(tsp_dev_inst *inst, int B, tsp::NlData **x);
// nl_opt.hip: one whole decision of every tour that is not done, queued on the engine's stream; dlb_mode != 0: a decision with
// active sets (tsp_nl_dlb_start has set them)
void tsp_nl_launch_decision(tsp_dev_tours *t, tsp::NlData *x, int kinds, int dlb_mode);
// nl_opt.hip: the active sets of the B tours of *x at the start of a call, queued on the engine's stream: `active` (B x n bytes,
// non-zero = active) or, when NULL, every node.  nact[b] = |A| of tour b, for NlState::nact.
int tsp_nl_dlb_start(tsp_dev_inst *inst, tsp::NlData *x, int B, const unsigned char *active, std::vector<int> *nact);
// nl_opt.hip: what the descents' entry points do.  `allowed` is the kinds mask the entry point takes; `out` takes the B records
// (chain fields as tsp_nl_write_stats fills them without a chain, start_cost = the final cost).  dlb_mode != 0: the descent with
// don't-look bits from the set `active` (as tsp_nl_dlb_start takes it).
int tsp_nl_run(tsp_dev_inst *inst, int kinds, int allowed, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
               int64_t max_moves, double time_limit_s, const tsp::NlStatsOut &out, int dlb_mode, const unsigned char *active);
