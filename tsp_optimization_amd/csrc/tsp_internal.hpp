// tsp_internal.hpp -- data laid out in HBM and the opaque handle types behind include/tsp_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <time.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/tsp_hip.h"
#include "tsp_dist.hpp"
#include "exh_arith.hpp"
#include "exh_decide.hpp"

namespace tsp {

// One scan block's candidate.  i < 0 means "none".
struct alignas(16) Partial {
    double delta;
    int i, j;
};
static_assert(sizeof(Partial) == 16, "Partial must be 16 bytes");

// Per-tour control block, read by every scan block (scalar loads) and written by the apply
// kernel's thread 0.  The descent is driven entirely by this block: the host only polls `done`.
struct alignas(16) TourState {
    // FIRST mode cursor: every pair up to and including (ci, cj) in (i<j) lexicographic order has
    // been scanned in the current sweep; (0,0) at the start of a sweep.
    int ci, cj;
    int chunk_rows;   // FIRST: number of rows the next scan covers
    int done;         // local optimum reached (or nothing to do)
    double obj;       // FIRST: running obj_best (+= delta); BEST: recomputed cost once done
    double seen_cost; // FIRST: best_cost of heuristics.c:442,492,495
    long long sweeps, evals, moves, reversed, pairs_scanned, steps;
    // sorted sweep: order/pos exist twice; `parity` says which copy holds the tour, `pending` that the move
    // (reverse positions mv_pa+1 .. mv_pb) chosen by the last sweep has not been carried out yet
    int parity, pending, mv_pa, mv_pb;
    // what the device really executed (CLUSTER engine; added to by every workgroup of the tour with atomics):
    // pairs a lane evaluated a bound or the delta for, pairs that reached tier 1, delta expressions executed, node
    // records derived for the sorted scan
    long long lane_pairs, tier1_pairs, exact_pairs, staged_recs;
    // FIRST on the CLUSTER engine: running mean of the rows between two hits (decides between the tiles scan and the
    // box-pruned scan of a step; survives k_rearm, so that a driver's next call starts with what the last one learnt)
    int hit_rows;
    // exhaustive sweep (k_move_pos + k_exh): the sweep's candidates are written and its move is not decided yet -- the next
    // k_move_pos decides it, or k_exh_close before the host looks.  Never set together with `pending`, never seen by the host.
    int open;
    // exhaustive sweep: which record buffer (1 or 2: d_prec[0], d_prec[1]) holds the tour's records, written by k_move_pos with
    // them; 0 between run calls (k_flush_state) and for a tour no launch of the run call has written records of.  Read by
    // k_exh_settle alone.
    int rec_buf;
    int pad2;
};

constexpr int kScanThreads = 256;
constexpr int kApplyThreads = 1024;

}  // namespace tsp

// ---- switches: TSP_<NAME> environment variables.  None of them changes a result.  They are read ONCE per
// instance handle (tsp_dev_inst_create) into this table; nothing on a call path calls getenv. ------------------------------
#define TSP_SWITCH_LIST(X)                                                                                                  \
    X(ENGINE) X(CLUSTER_BLOCKS) X(CLUSTER_MIN_ROWS) X(CLUSTER_MAX_ROWS) X(CLUSTER_HIT_CAP) X(CLUSTER_SPIN_LIMIT)            \
    X(CLUSTER_SPIN_MS) X(CLUSTER_COPIES) X(CLUSTER_TILE_ROWS) X(CLUSTER_XCD_LOCAL) X(CLUSTER_ALLOW_OVERSUB) X(CLUSTER_DEBUG) X(CLUSTER_PROBE) X(CLUSTER_FIRST_SORTED) X(TABU_DENSE)     \
    X(LDS_PROBE) X(LDS_MIN_ROWS) X(LDS_EDGE_CACHE) X(NO_ICOORD) X(NO_FILTER) X(NO_PRUNE) X(SORTED_MIN_N)      \
    X(SWEEP_BLOCKS) X(SWEEP_TABLE) X(BEST_ROWS_PER_BLOCK) X(BEST_RECS) X(FIRST_GRID_ROWS) X(FIRST_MIN_ROWS)                \
    X(FIRST_MAX_ROWS) X(CONSTRUCT_GLOBAL) X(CONSTRUCT_NN) X(CLUSTER_FS_ROWS) X(LDS_F32_MIN_N) X(EXH_POS) X(TABU_INKERNEL) X(OROPT_FULL)
namespace tsp {
enum SwitchId {
#define TSP_SW_ENUM(name) SW_##name,
    TSP_SWITCH_LIST(TSP_SW_ENUM)
#undef TSP_SW_ENUM
    SW_COUNT
};
struct Switches {
    int v[SW_COUNT];
    bool has[SW_COUNT];
    int get(SwitchId k, int dflt) const { return has[k] ? v[k] : dflt; }
};
void read_switches(Switches *sw);   // api.hip
}  // namespace tsp
#define TSP_SW(inst_, NAME, dflt) ((inst_)->sw.get(tsp::SW_##NAME, (dflt)))

// ---- opaque handles ------------------------------------------------------------------------

struct tsp_dev_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int num_cus = 0;
    int lds_bytes = 0;        // LDS one workgroup may be granted (hipDeviceAttributeMaxSharedMemoryPerBlock; 160 KiB on gfx950)
    // CLUSTER engine under AUTO: after a give-up (a workgroup was not resident: the device is shared or CU-masked) the next
    // `cl_skip` AUTO decisions go to the other engines; the back-off doubles with every further give-up (64 .. 4096 calls)
    int cl_skip = 0, cl_backoff = 0;
    long long cl_giveups = 0;
    long long cl_chain_losses = 0;   // give-ups in the middle of a chain of tabu() iterations (the search went on from the incumbent)
};

namespace tsp { struct NodeRec; }
struct tsp_dev_tours;
struct tsp_dev_inst {
    tsp_dev_ctx *ctx = nullptr;
    int n = 0;
    int wtype = 0;        // kernel variant: unknown -> EUC_2D; *_ICOORD when the coordinates allow it
    int wtype_public = 0; // the caller's weight type
    tsp_dev_tours *scratch1 = nullptr;  // reusable single-tour handle of the host-tour entry points (B == 1)
    tsp_dev_tours *scratch_b = nullptr; // ... and the handle of the last batch size used
    int scratch_b_count = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // reusable timing events
    double filter_margin = 1e300; // root filter margin of the 2-opt scans (tsp_dist.hpp); 1e300 = off
    double prune_margin = 1e300;  // new-edge bound margin (tsp_dist.hpp); 1e300 = off
    double sum_margin = 1e300;    // sorted sweep, both new edges: |ab| + |a1 b1| < bound + d(a,a1) + d(b,b1) + this
    int integer_cost = 1;
    double2 *d_coord = nullptr; // n x (x,y) or (lat,lon) for GEO
    // Sorted sweep (sqrt metrics): nodes ranked along a Hilbert curve, 64 consecutive ranks = one group.
    // d_sperm[slot] = node (or -1 for padding), n_slots = (ng + 1) * 64 (one extra all-padding group);
    // d_gbox[g] = {min x, max x, min y, max y} of group g's nodes (the padding group sits far away).
    int *d_sperm = nullptr;
    double4 *d_gbox = nullptr;
    std::vector<double4> h_gbox;   // host copy (pair tables of the sorted sweep and scan: read as ng x 4 doubles, cluster_deal.hpp)
    int ng = 0, n_slots = 0;
    double org_x = 0.0, org_y = 0.0;   // min corner of the coordinates
    double cost_bound = 1e300;         // no distance of the instance exceeds this (bounding-box diagonal + rounding)
    std::vector<int> h_sinv;           // node -> rank slot
    void *io_pool = nullptr;           // call-local device scratch of the small host-array entry points (fitness, spot
    size_t io_pool_bytes = 0;          // distances, stamp reads/writes), grown on demand: no hipMalloc per call
    void *cons_pool = nullptr;         // scratch of tsp_dev_construct, grown on demand
    size_t cons_pool_bytes = 0;
    void *d_sxy = nullptr;             // coordinates in rank order (float2 / double2), built on first use by the large greedy
    double2 *d_rcoord = nullptr;       // CLUSTER engine, sorted scan: coordinates in rank order, padding far away (ng * 64)
    int *d_sinv = nullptr;             // CLUSTER engine, sorted scan: node -> rank slot
    std::vector<double> h_xy;   // host copy of the raw coordinates (2n)
    tsp::Switches sw;           // the TSP_* switches as they stood when this handle was created
    void *or_scratch = nullptr; // Or-opt buffers of the last batch size (or_opt.hip)
    void *nl_data = nullptr;    // neighbour lists and the buffers of their descent (nl_opt.hip)
    void *hk_data = nullptr;    // 1-tree / Held-Karp buffers (held_karp.hip)
};
static_assert(sizeof(double4) == 4 * sizeof(double), "tsp_dev_inst::h_gbox is handed to cluster_deal as ng x {min x, max x, min y, max y}");

struct tsp_dev_tabu {
    tsp_dev_inst *inst = nullptr;
    long long count = 0;
    int *d_stamp = nullptr;
    // compact list of the non-zero stamps (two_opt_tabu_list.hpp): what a sweep with a list works from
    int2 *d_list = nullptr;
    int *d_list_n = nullptr;                     // entries (device); may exceed list_cap after a scan = unusable
    unsigned long long *d_tabu_pairs = nullptr;  // pairs the sweeps of the current run skipped as tabu
    int *h_list_n = nullptr;                     // pinned
    int list_cap = 0;
    bool list_valid = false;                     // the list covers every non-zero stamp
    long long list_ub = 0;                       // host's upper bound of the entry count
    long long list_compact_at = 0;               // compaction when list_ub passes this
    bool last_run_list = false;                  // the last run with this handle worked from the list
};

struct tsp_dev_tours {
    tsp_dev_inst *inst = nullptr;
    int B = 0;
    int n = 0;
    // device
    int *d_order = nullptr;          // B x n : node at tour position p
    int *d_pos = nullptr;            // B x n : position of node v
    int *d_order2 = nullptr, *d_pos2 = nullptr;   // second copies (sorted sweep: moves are applied out of place)
    tsp::TourState *d_state = nullptr;       // the current control blocks: d_state_base + slot * B
    tsp::TourState *d_state_base = nullptr;  // 2 x B: k_first and k_move_pos read one slot and write the other
    int slot = 0;
    tsp::Partial *d_partial = nullptr;
    size_t partial_per_tour = 0;
    tsp::NodeRec *d_rec = nullptr;   // B x max(n, n_slots) node records, rebuilt before every BEST step (k_recs*)
    double *d_gmax = nullptr;        // B x (ng + 1): longest tour edge leaving a node of the group (sorted sweep)
    int sorted_min_n = 0;            // BEST sweeps of instances with n >= this use the sorted sweep (GRID engine)
    int cl_sorted_min_n = 8;         // ... the sorted scan (CLUSTER engine: ahead of its tiles scan from n = 52 up, tools/small_best.py)
    int sweep_blocks = 512;          // k_sweep blocks per tour
    int *d_cl_ticket = nullptr;      // k_sweep: arrival counters per tour x cluster
    // exhaustive sweep in position order (two_opt_exh.hpp): the tour's row records by position (padded), node id included.
    // Two buffers: k_move_pos writes d_prec[exh_buf ^ 1] -- from d_prec[exh_buf] when exh_hot says that those are the records of
    // the tour as it stands -- and the k_exh behind it reads what it wrote; the host flips exh_buf with the pair of launches.
    // exh_hot is true only inside a run call that has queued an exhaustive pair (tsp_grid_run): between calls anything may
    // move the tour (the flush carries out a pending move, other engines, an upload).  While it is true the records are the
    // tour and d_order / d_pos (both copies) are STALE: hot launches of k_move_pos do not write them.  Whoever takes exh_hot
    // back (launch_flush) queues k_exh_settle first, which writes them from the records; nothing else may read them before.
    tsp::ExhRec *d_prec[2] = {nullptr, nullptr};
    int exh_buf = 0;
    bool exh_hot = false;
    int exh_share[4] = {0, 0, 0, 0};   // k_exh: rows per wave of each part of the grid (0: equal shares)
    int exh_gens = 0;                  // ... parts (= workgroups per CU)
    tsp::ExhDeal *d_exh_deal = nullptr;   // k_exh: where each wave of a tour's grid starts and how many row units it has (exh_deal)
    tsp::ExhCand *d_exh_cand = nullptr;   // k_exh: each workgroup's candidate by tour position (exh_decide.hpp), B x exh_blocks
    int exh_lds = 0;                 // k_exh: dynamic LDS a workgroup asks for (unused; it pins the number of workgroups per CU)
    int exh_blocks = 0;              // k_exh: workgroups per tour (0: the tiled k_step executes the exhaustive sweep)
    int *d_pairtab = nullptr;        // group pairs per cluster of k_sweep blocks (host-built), or nullptr
    int *d_ticket = nullptr;         // per tour: scan blocks still to arrive in the current step
    int *d_row_ticket = nullptr;     // per tour x tile row (BEST two-level hand-off)
    tsp::Partial *d_row_slot = nullptr;
    int *d_row_evals = nullptr;
    int max_tile_rows = 0;
    int *d_slot_evals = nullptr;     // per scan block: pairs evaluated (tabu runs only)
    // CLUSTER engine (two_opt_cluster.hip): exchange area (+ error word) and the group-pair table dealt to cl_C workgroups
    unsigned long long *d_cl_slots = nullptr;
    size_t cl_slot_words = 0;
    int cl_C = 0;
    long long *d_cl_stats = nullptr; // B x 256 x 4: the CLUSTER engine's executed-work counters per workgroup (summed at download)
    unsigned cl_epoch = 0;           // exchange epochs handed out so far (they run on from launch to launch)
    int *d_cl_pairtab = nullptr;
    int cl_ntests = 0;
    // drivers on resident tours: the incumbent kept on the device (tsp_dev_tours_snapshot / _restore), kick results
    int *d_order_snap = nullptr;
    std::vector<double> h_obj_snap;
    int *d_kick_result = nullptr;    // 8 ints: {accepted, a1, b1, 0, acted, improved, 0, 0}
    int *h_kick_result = nullptr;    // pinned
    int *d_chain = nullptr, *h_chain = nullptr;   // device words of a chain of tabu() iterations (tabu_chain.hpp), pinned mirror
    bool h_state_fresh = false;   // h_state holds what d_state holds (set by a CLUSTER run's last poll, cleared by whatever queues work after it)
    int *h_cl_err = nullptr;         // pinned: the CLUSTER engine's error word, read with every poll
    bool tabu_list_run = false;      // the current tsp_grid_run goes through k_sweep<TABU> (two_opt_tabu_list.hpp)
    // reset point (device copies of the uploaded tours)
    int *d_order0 = nullptr;
    std::vector<double> h_obj0;
    std::vector<int> h_order_buf;    // staging of tsp_dev_tours_upload
    // pinned host mirror of the states, for polling: 3 x B.  The first B are what every reader of h_state looks at; the other two
    // slots take the copies of a run whose polls stay one burst behind the queue (tsp_grid_run), poll k into slot 1 + k mod 2 and
    // poll_ev[k mod 2] recorded behind it, so that a copy in flight never lands in a block the host is reading.
    tsp::TourState *h_state = nullptr;
    hipEvent_t poll_ev[2] = {nullptr, nullptr};
    // scan geometry
    int first_grid_rows = 32;        // k_first: tile rows of its fixed grid
    int first_max_rows2 = 2048;      // k_first: largest chunk
    int first_min_rows = 8;
    int best_rows_per_block = 32;
    int use_recs = 1;                // BEST: materialise the node records once per step (k_recs)
    // accumulated device time
    double device_ms = 0.0;
};

// ---- error plumbing ------------------------------------------------------------------------
namespace tsp {
void set_last_error(const char *what, hipError_t e, const char *file, int line);
void set_last_error_text(const char *text);   // for failures that are not a HIP call's

// Call-local device scratch: released when the scope ends, so an early error return leaks nothing.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t count) { return hipMalloc(&p, sizeof(T) * count); }
    operator T *() const { return p; }
};
}
// ---- hooks between the extension files ---------------------------------------------------------
namespace tsp {
// The 1-tree that held_karp.hip built last, resident on the device: edge slots 0 .. n (slot 0 / n: the smaller / larger edge
// at node 0; slots 1 .. n-1: the spanning tree's edges, lo = -1 in the one empty slot) and the penalties it was built for.
struct HkTree {
    const int *d_elo = nullptr, *d_ehi = nullptr;
    const double *d_ew = nullptr, *d_pi = nullptr;
    double W = 0.0;
    long long rounds = 0;
    float device_ms = 0.f;
};
// What a tabu() driver hands down through tsp_tabu_run to tsp_cluster_run: the list the descent runs with, and the work the
// CLUSTER run queues for the driver behind its launches, before the run's wait for the device (one wait per iteration of tabu(),
// or per chain of them, instead of two).  Plain data; the arrays are the caller's.
struct TabuRide {
    tsp_dev_tabu *tabu = nullptr;   // the list counts when tabu && iter >= 0 && tenure >= 0 (check_tenure, tabusearch.c:84)
    int iter = 0, tenure = 0;
    // iterations INSIDE the launch (TSP_TABU_INKERNEL, the default): the kernel runs ik_n of them from the words the driver has
    // put into d_chain (tabu_chain.hpp) and keeps the incumbent in d_order_snap; ik_pairs = kick trials there (0: one per iteration)
    int ik_n = 0, ik_pairs = 0;
    // ... or queued behind the run's FIRST launch (tsp_grid_tabu_follow).  kPost: k_tabu_post -- incumbent (cost `best`) and the
    // kick's trial a, b decided on the device from the finished descent.  kChain: the same by k_tabu_post_chain, then launch
    // k = 1 .. count - 1 of the same kernel as iteration iter + k with tenures[k], each followed by its own k_tabu_post_chain
    // (trial ab[2k], ab[2k + 1]): a stop word on the device turns what follows a failed iteration into no-ops.
    enum Follow { kNone, kPost, kChain } follow = kNone;
    int a = 0, b = 0, count = 0;
    double best = 0.0;
    const int *tenures = nullptr, *ab = nullptr;
    // what the run reports back
    bool follow_ran = false;   // the follow-up of the first launch was queued
    int launched = 0;          // launches queued in all (1 + the chained ones)
};
}
int tsp_hk_tree(tsp_dev_inst *inst, const double *pi, tsp::HkTree *out, tsp_lb_stats *stats);   // held_karp.hip
int tsp_nl_adopt_lists(tsp_dev_inst *inst, int K, int *d_nbr);                                  // nl_opt.hip: takes d_nbr over
int tsp_nl_lists(tsp_dev_inst *inst, int *K, const int **d_nbr);                                 // nl_opt.hip: built if there are none
tsp_dev_tours *tsp_scratch_tours(tsp_dev_inst *inst, int B, bool *owned, int *rc);             // api.hip
int tsp_perm_cost_device(tsp_dev_inst *inst, const int *d_perm, long long stride, int B, double *d_out, size_t out_stride_bytes);   // api.hip
void tsp_or_scratch_free(void *p);   // or_opt.hip
void tsp_nl_data_free(void *p);      // nl_opt.hip
void tsp_hk_data_free(void *p);      // held_karp.hip
int tsp_lds_run(tsp_dev_tours *t, int mode, double time_limit_s, int *all_done);   // two_opt_lds.hip
bool tsp_lds_fits(const tsp_dev_inst *inst);
// two_opt_cluster.hip.  tabu_list: the run carries a tabu list (it takes the sorted scan at any size); ride: nullptr = none
bool tsp_cluster_fits(const tsp_dev_tours *t, int mode, bool tabu_list = false);
bool tsp_cluster_sorted(const tsp_dev_tours *t, int mode, bool tabu_list = false);
int tsp_cluster_size(const tsp_dev_tours *t, int mode, bool tabu_list = false);
int tsp_cluster_run(tsp_dev_tours *t, int mode, int C, int64_t max_steps, double time_limit_s, int *all_done, int *fell_through,
                    tsp::TabuRide *ride = nullptr);
// two_opt_grid.hip
int tsp_grid_tour_cost(tsp_dev_tours *t, double *d_out);
int tsp_grid_run(tsp_dev_tours *t, int mode, tsp_dev_tabu *tabu, int iter, int tenure, int64_t max_steps,
                 double time_limit_s, int sync, int *all_done);
int tsp_grid_after_external_run(tsp_dev_tours *t, int mode, int timed_out, bool pos_written = false);
void tsp_grid_tabu_follow(tsp_dev_tours *t, const tsp::TabuRide &r, int k, const int *d_err);
int tsp_grid_rearm(tsp_dev_tours *t, int mode);
int tsp_grid_tabu_kick(tsp_dev_tours *t, tsp_dev_tabu *tabu, int a, int b, int iter, int tenure, int *accepted);
int tsp_grid_vns_kick(tsp_dev_tours *t, int p1, int p2, int p3, double *obj);
int tsp_grid_snapshot(tsp_dev_tours *t, bool restore);
int tsp_grid_resident_tabu(tsp_dev_tours *t, tsp_dev_tabu *tabu, int iter, int tenure, double time_limit_s, double *obj);
int tsp_grid_tabu_iteration(tsp_dev_tours *t, tsp_dev_tabu *tabu, int iter, int tenure, double time_limit_s, int a, int b,
                            double *best_obj, double *obj, int *improved, int *accepted);
int tsp_grid_tabu_iterations(tsp_dev_tours *t, tsp_dev_tabu *tabu, int iter0, int count, const int *tenure, int pairs, const int *ab, double time_limit_s,
                             double *best_obj, double *obj, int *improved, int *trials, int *completed, int *last_accepted);

// Per-instance scratch for the host-array entry points (not for concurrent use, like every handle): >= bytes, 256-aligned.
void *tsp_io_pool(tsp_dev_inst *inst, size_t bytes);

#define TSP_HIP_TRY(expr)                                                    \
    do {                                                                     \
        hipError_t e__ = (expr);                                             \
        if (e__ != hipSuccess) {                                             \
            tsp::set_last_error(#expr, e__, __FILE__, __LINE__);             \
            return TSP_DEV_E_HIP;                                            \
        }                                                                    \
    } while (0)

namespace tsp {
// the host's monotonic clock, in seconds
inline double wall_s() {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}
}  // namespace tsp

// Everything queued on the stream waited for and a control block copied back: the look a host loop takes between two batches.
namespace tsp {
template <typename CTL>
inline int poll_ctl(hipStream_t s, CTL *host, const CTL *dev) {
    TSP_HIP_TRY(hipMemcpyAsync(host, dev, sizeof(CTL), hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipStreamSynchronize(s));
    TSP_HIP_TRY(hipGetLastError());
    return TSP_OK;
}
}  // namespace tsp

// The instance's reusable pair of timing events, created on first use.
inline int tsp_inst_events(tsp_dev_inst *inst) {
    if (!inst->ev0) { TSP_HIP_TRY(hipEventCreate(&inst->ev0)); TSP_HIP_TRY(hipEventCreate(&inst->ev1)); }
    return TSP_OK;
}
