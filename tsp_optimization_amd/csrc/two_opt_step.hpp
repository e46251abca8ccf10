// two_opt_step.hpp -- what every step kernel of the GRID engine shares: launch arguments, the in-launch hand-off,
// the tour seen through a pending move, the tour cost, the decision of a sweep a finished launch left (exhaustive sweep),
// and the apply executed by a step's last block
// Part of the GRID engine; included by two_opt_grid.hip only (one translation unit).
#pragma once
#include "two_opt_common.hpp"
#include "exh_arith.hpp"

#pragma clang fp contract(off)

namespace tsp {


constexpr int kMaxRowsPerBlock = 256;

// Diagnostic build only (-DTSP_STAMPS): 100 MHz wall-clock stamps of the last block of each step,
// accumulated into a buffer nothing else reads (cdna_hip_programming.md section 7, in-kernel stamps).
#ifdef TSP_STAMPS
__device__ unsigned long long g_stamp_sum[16];
__device__ unsigned long long g_stamp_n;
__device__ unsigned long long g_clk_core, g_clk_real;   // row-loop time of every block: shader cycles vs 100 MHz ticks
#define TSP_STAMP(k) do { if (threadIdx.x == 0) stamps[k] = wall_clock64(); } while (0)
#else
#define TSP_STAMP(k) do { } while (0)
#endif

__global__ void k_build_pos(const int *__restrict__ orders, int *__restrict__ poss, int n) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const size_t base = (size_t)blockIdx.y * n;
    poss[base + orders[base + p]] = p;
}

// ---- in-launch hand-off of the block candidates ---------------------------------------------
// Producer (lane 0 of each block): two 8-byte write-through (sc1) stores, drain, then one relaxed
// agent-scope countdown on the tour's ticket.  Consumer (the block whose decrement returned 1):
// sc1 loads after the block barrier that the decrementing wave joins.  Every slot is written once
// and read once per launch and launches are separated by kernel boundaries, so no stale copy of a
// slot can sit in the reader's caches (cdna_hip_programming.md G16 / MI355X_MICROARCH.md
// "Valid forms", first row).  order/pos/state are only written by the last block, after every
// other block of the tour has finished, and are next read in the following launch.
using gu64 = __attribute__((address_space(1))) unsigned long long;
using gi32 = __attribute__((address_space(1))) int;

__device__ __forceinline__ void publish_partial(Partial *slot, double delta, int i, int j) {
    gu64 *g = (gu64 *)slot;
    __hip_atomic_store(g, (u64)__double_as_longlong(delta), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(g + 1, ((u64)(unsigned)j << 32) | (u64)(unsigned)i, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void read_partial(const Partial *slot, double &delta, int &i, int &j) {
    gu64 *g = (gu64 *)slot;
    const u64 a = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 b = __hip_atomic_load(g + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    delta = __longlong_as_double((long long)a);
    i = (int)(b & 0xffffffffu);
    j = (int)(b >> 32);
}

// Blocks of a step that own at least one column above their first row (the others return at
// once and take no ticket).  Block (bx, by) is skipped iff bx < (r0(by) + 1) / TJ.
__device__ __forceinline__ int skipped_in_tile_row(int r0, int gx, int TJ) { return min(gx, (r0 + 1) / TJ); }


// ---- tour cost: tour_cost_block of two_opt_common.hpp -------------------------------------
// out[b] = recomputed cost of tour b (BEST runs that stop early; multi-start "true cost")
template <int WT, bool INT>
__global__ __launch_bounds__(kApplyThreads) void k_tour_cost(const double2 *__restrict__ coord,
                                                             const int *__restrict__ orders,
                                                             const int *__restrict__ poss, int n,
                                                             double *__restrict__ out, size_t out_stride_bytes) {
    __shared__ double s_d[kApplyThreads / 64];
    __shared__ double s_chunk[(INT || WT == WT_CEIL_2D) ? 1 : 4096];
    const size_t base = (size_t)blockIdx.x * n;
    const double c = tour_cost_block<WT, INT>(coord, orders + base, poss + base, n, s_d, s_chunk);
    if (threadIdx.x == 0)
        *reinterpret_cast<double *>(reinterpret_cast<char *>(out) + blockIdx.x * out_stride_bytes) = c;
}

// The move a sweep chose is carried out by the NEXT launch, by all of its blocks: order/pos exist twice, the
// reversal of positions pa+1 .. pb is a gather from the current copy into the other one
//     new_order[p] = old_order[mirror(p)],  mirror(p) = pa + 1 + (L - 1 - t) for t = (p - pa - 1) mod n < L, else p
// and the records of the next sweep are built from the same closed form, so nothing waits for the copy.
struct MoveView {
    const int *order, *pos;   // the current copy
    int n, pa1, L;            // pending reversal: positions pa1 .. pa1 + L - 1 (cyclic); L == 0: none
    __device__ __forceinline__ int mirror(int p) const { return exh_mirror(p, n, pa1, L); }   // (exh_arith.hpp: the CPU tests it)
    __device__ __forceinline__ int node_at(int p) const { return order[mirror(p)]; }   // node at new position p
    __device__ __forceinline__ int pos_of(int v) const { return mirror(pos[v]); }       // the mirror is an involution
};

// (from the control block's words, for a caller that has loaded them itself)
__device__ __forceinline__ MoveView move_view(int parity, int pending, int mv_pa, int mv_pb, const int *o1, const int *p1,
                                              const int *o2, const int *p2, int n) {
    MoveView m;
    const bool second = parity != 0;
    m.order = second ? o2 : o1; m.pos = second ? p2 : p1; m.n = n;
    m.L = 0; m.pa1 = 0;
    if (pending) {
        int L = mv_pb - mv_pa; if (L < 0) L += n;
        m.L = L; m.pa1 = mv_pa + 1 == n ? 0 : mv_pa + 1;
    }
    return m;
}
__device__ __forceinline__ MoveView move_view(const TourState *st, const int *o1, const int *p1, const int *o2,
                                              const int *p2, int n) {
    return move_view(st->parity, st->pending, st->mv_pa, st->mv_pb, o1, p1, o2, p2, n);
}

// ---- the decision of a sweep whose block candidates a FINISHED launch has left in memory ----------------------
// Block-wide (kScanThreads threads), for every block that wants the answer: the arg-min of (delta, (i, j)) over the `nslots`
// candidates of a tour -- apply_step's rule: better() on (delta, key), a move only when delta < 0 -- and the winner's
// positions.  The candidates were written by an earlier launch: ordinary loads, all of a thread's in flight at once.
// The positions: with `wpos` (the exhaustive sweep: k_exh knows its pairs by position and leaves (pos[i], pos[j]) beside each
// candidate) they are loaded in the same round as the candidates, and the thread that owns the winning key hands them out
// through LDS; without it (wpos == nullptr) they cost one more latency for pos[i] and pos[j] in the current copy of pos.
// The reduction order differs from apply_step's; the arg-min with a strict tie-break does not depend on it.  Two slots may
// hold the same pair (k_exh: strip 0 overlaps strip 1): they hold the same positions.  s_d, s_k: >= kScanThreads / 64
// entries each.
// Two halves.  The candidates' addresses depend on the thread alone, so a caller with loads of its own to wait for (k_move_pos:
// the control block) issues sweep_load first and lets both travel together; sweep_reduce is everything behind the wait.
struct SweepDecision {
    int found = 0, i = -1, j = -1;   // found == 0: local optimum (i = j = -1)
    int pa = 0, pb = 0, L = 0;       // pos[i], pos[j]; reverse positions pa + 1 .. pb (cyclic), L = (pb - pa) mod n of them
};

constexpr int kDecidePU = 8;   // 2 048 candidates = 8 per thread: one round
struct SweepLoads { Partial p[kDecidePU]; int2 w[kDecidePU]; };

// one round of a thread's loads: slots s0, s0 + kScanThreads, ... (s0 = threadIdx.x for the first round).
// WPOS: the caller always has the array of positions (the exhaustive sweep) -- no test per load, no path through pos.
template <bool WPOS = false>
__device__ __forceinline__ SweepLoads sweep_load(const Partial *__restrict__ part, const int2 *__restrict__ wpos, int nslots, int s0) {
    SweepLoads l;
#pragma unroll
    for (int k = 0; k < kDecidePU; ++k) {
        const int s = s0 + k * kScanThreads;
        l.p[k].delta = 0.0; l.p[k].i = -1; l.p[k].j = -1;
        l.w[k] = make_int2(0, 0);
        if (s < nslots) {
            l.p[k] = part[s];
            if (WPOS || wpos) l.w[k] = wpos[s];
        }
    }
    return l;
}

// keeps the loads of a round where they were issued: to be called behind the caller's own loads and a scheduling barrier,
// before the first use of any of them (the device k_exh starts its strips with)
__device__ __forceinline__ void sweep_pin(const SweepLoads &l) {
#pragma unroll
    for (int k = 0; k < kDecidePU; ++k)
        asm volatile("" : : "v"(l.p[k].delta), "v"(l.p[k].i), "v"(l.p[k].j), "v"(l.w[k].x), "v"(l.w[k].y));
}

// `first`: the round sweep_load(part, wpos, nslots, threadIdx.x) fetched; further rounds (nslots > 2 048) are fetched here
template <bool WPOS = false>
__device__ __forceinline__ SweepDecision sweep_reduce(const SweepLoads &first, const Partial *__restrict__ part,
                                                      const int2 *__restrict__ wpos, int nslots, const int *__restrict__ pos, int n,
                                                      double *s_d, u64 *s_k) {
    __shared__ int2 s_wpos;
    const int tid = threadIdx.x;
    double bd = 0.0;
    u64 key = kNoKey;
    int2 bw = make_int2(0, 0);
    auto fold = [&](const SweepLoads &l) {
#pragma unroll
        for (int k = 0; k < kDecidePU; ++k) {
            const u64 kk = make_key(l.p[k].i, l.p[k].j);
            if (better(l.p[k].delta, kk, bd, key)) { bd = l.p[k].delta; key = kk; bw = l.w[k]; }
        }
    };
    fold(first);
    for (int s0 = tid + kDecidePU * kScanThreads; s0 < nslots; s0 += kDecidePU * kScanThreads) fold(sweep_load<WPOS>(part, wpos, nslots, s0));
    const u64 mine = key;
    block_argmin<true>(bd, key, s_d, s_k);
    SweepDecision d;
    d.found = key != kNoKey && bd < 0;   // (block-uniform)
    if (d.found) {
        d.i = key_i(key); d.j = key_j(key);
        if (WPOS || wpos) {
            if (mine == key) s_wpos = bw;   // every owner of the key holds the same pair of positions
            __syncthreads();
            d.pa = s_wpos.x; d.pb = s_wpos.y;
        } else {
            d.pa = pos[d.i]; d.pb = pos[d.j];
        }
        d.L = d.pb - d.pa; if (d.L < 0) d.L += n;
    }
    return d;
}

// the two halves back to back
__device__ __forceinline__ SweepDecision sweep_decide(const Partial *__restrict__ part, const int2 *__restrict__ wpos, int nslots,
                                                      const int *__restrict__ pos, int n, double *s_d, u64 *s_k) {
    return sweep_reduce(sweep_load(part, wpos, nslots, threadIdx.x), part, wpos, nslots, pos, n, s_d, s_k);
}

// What apply_step's thread 0 adds to the control block for one exhaustive sweep, at the moment the sweep is decided; without a
// move the tour is done and `cost` is its recomputed cost.  parity and pending are the caller's: they depend on who decides
// (two_opt_exh.hpp).
__device__ __forceinline__ void sweep_count(TourState &z, const SweepDecision &d, int n, double cost) {
    z.steps += 1;
    z.sweeps += 1;
    z.evals += (long long)n * (n - 1) / 2 - n;   // non-adjacent pairs (n >= 4)
    z.pairs_scanned += (long long)n * (n - 1) / 2;
    if (d.found) { z.moves += 1; z.reversed += d.L - 1; }
    else { z.obj = cost; z.done = 1; }
    z.mv_pa = d.pa; z.mv_pb = d.pb;
    z.open = 0;
}


// ---- apply: executed by the last block of a tour's step ------------------------------------
struct StepArgs {
    const double2 *coord;
    int *orders;
    int *poss;
    TourState *states;
    Partial *partials;
    int *tickets;      // per tour
    int *row_tickets;  // per tour x tile row (BEST: two-level hand-off)
    Partial *row_slots; // per tour x tile row
    int *row_evals;    // per tour x tile row (tabu runs)
    int max_tile_rows;
    int *slot_evals;   // tabu runs only
    int *tabu;
    const NodeRec *recs;   // BEST: materialised by k_recs before the step; nullptr = derive per tile
    size_t partial_per_tour;
    int n, rows_per_block, first_min_rows, first_max_rows, iter, tenure;
    int slot;          // k_first: which of the tour's two control blocks this launch reads (the other is written)
    double margin;     // root filter (tsp_dist.hpp); 1e300 = every pair is evaluated exactly
    double prune;      // new-edge bound margin (tsp_dist.hpp); 1e300 = never prune
    // sorted sweep (k_sweep): records in Hilbert-rank order, group boxes, per-group longest edge, shared bound
    double sum_margin; // k_sweep tier 1: rounding of the two new distances + fp slack (doubled: keeps ties)
    const int *pairtab;    // k_sweep: group pairs (r << 16 | c, -1 = none) per cluster, or nullptr (computed)
    int *cl_tickets;       // k_sweep: per tour x cluster arrival counters, 64 ints apart
    int *orders2, *poss2;  // k_sweep / k_move_recs: the second copy of order/pos (TourState::parity says which is current)
    const double4 *gbox;
    const double *gmax;
    int ng, n_slots, flat_slots;
    // k_sweep<TABU> (two_opt_tabu_list.hpp): the compact list of non-zero stamps and the sweep's skipped-pair counter
    const int2 *tabu_list;
    const int *tabu_list_n;
    int tabu_list_cap;
    unsigned long long *tabu_pairs;
};

template <int WT, bool INT, int MODE, int RJ, bool TABU, bool FLAT = false>
__device__ __forceinline__ void apply_step(const StepArgs &a, int tour, int row_lo, int row_hi
#ifdef TSP_STAMPS
                                           , unsigned long long *stamps
#endif
                                           , double *chunk_buf = nullptr   // FLAT: 4096 doubles of LDS the caller no longer needs
) {
    const int n = a.n, rpb = a.rows_per_block;
    const int gy = gridDim.y;
    TourState *st = a.states + tour;
    const int tid = threadIdx.x;
    int *order = a.orders + (size_t)tour * n;
    int *pos = a.poss + (size_t)tour * n;
    int cur_parity = 0;
    if constexpr (FLAT) {
        // k_move_recs has just carried the previous step's move out into the other copy: that one is current now
        cur_parity = st->parity ^ st->pending;
        if (cur_parity) { order = a.orders2 + (size_t)tour * n; pos = a.poss2 + (size_t)tour * n; }
    }
    const Partial *part = a.partials + (size_t)tour * a.partial_per_tour;

    __shared__ double s_d[kScanThreads / 64];
    __shared__ u64 s_k[kScanThreads / 64];
    __shared__ long long s_ll[kScanThreads / 64];

    // BEST: one pre-reduced candidate per tile row; FLAT (sorted sweep): one candidate per block, all live
    static_assert(MODE == TSP_2OPT_BEST, "first improvement runs through k_first");
    constexpr bool HIER = !FLAT;
    const int tile_rows = min((row_hi - row_lo + rpb - 1) / rpb, gy);
    const int nslots = FLAT ? a.flat_slots : tile_rows;
    if constexpr (HIER) part = a.row_slots + (size_t)tour * a.max_tile_rows;

    // 1. winner over the blocks that published a candidate (loads batched: they are sc1 loads
    //    that go to memory, so eight slots per lane are kept in flight)
    double bd = 0.0;
    u64 key = kNoKey;
    long long tabu_evals = 0;
    constexpr int PU = 4;
    for (int s0 = tid; s0 < nslots; s0 += PU * kScanThreads) {
        double pd[PU]; int pi[PU], pj[PU]; bool live[PU];
#pragma unroll
        for (int k = 0; k < PU; ++k) {
            const int s = s0 + k * kScanThreads;
            live[k] = s < nslots;
            pd[k] = 0.0; pi[k] = -1; pj[k] = -1;
            if (live[k]) read_partial(part + s, pd[k], pi[k], pj[k]);
        }
#pragma unroll
        for (int k = 0; k < PU; ++k) {
            const u64 kk = make_key(pi[k], pj[k]);
            const bool take = live[k] && better(pd[k], kk, bd, key);
            if (take) { bd = pd[k]; key = kk; }
            if constexpr (TABU) {
                if (live[k])
                    tabu_evals += __hip_atomic_load(
                        (gi32 *)(a.row_evals + (size_t)tour * a.max_tile_rows + s0 + k * kScanThreads),
                        __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    block_argmin<true>(bd, key, s_d, s_k);
    TSP_STAMP(6);
    if constexpr (TABU) tabu_evals = block_sum<long long>(tabu_evals, s_ll);
    const bool found = key != kNoKey && bd < 0;
    const int wi = found ? key_i(key) : -1, wj = found ? key_j(key) : -1;
    int pa = 0, pb = 0;
    if (found) { pa = pos[wi]; pb = pos[wj]; }

    __syncthreads();  // every read of the old order/pos is done
    TSP_STAMP(7);

    // 2. the move: reverse positions pa+1 .. pb (cyclic)
    int L = 0;
    if (found) { L = pb - pa; if (L < 0) L += n; }
    if (found && !FLAT) {   // FLAT: the move is left to the next launch of k_move_recs (all blocks, not one)
        const int half = L >> 1;
        constexpr int U = 4;
        for (int t0 = tid; t0 < half; t0 += U * kScanThreads) {
            int p[U], q[U], u[U], w[U];
#pragma unroll
            for (int k = 0; k < U; ++k) {
                const int t = t0 + k * kScanThreads;
                p[k] = pa + 1 + t; if (p[k] >= n) p[k] -= n;
                q[k] = pb - t; if (q[k] < 0) q[k] += n;
                u[k] = 0; w[k] = 0;
                if (t < half) { u[k] = order[p[k]]; w[k] = order[q[k]]; }
            }
#pragma unroll
            for (int k = 0; k < U; ++k) {
                if (t0 + k * kScanThreads < half) {
                    order[p[k]] = w[k]; order[q[k]] = u[k];
                    pos[w[k]] = p[k]; pos[u[k]] = q[k];
                }
            }
        }
    }

    TSP_STAMP(8);
    // 3. at the local optimum: recomputed cost
    double final_cost = 0.0;
    if (!found) {
        // the sequential cost of non-integer lengths is staged through 32 KB of LDS: the sweep lends its staging
        // area (its own 32 KB would cost the float-cost variants two thirds of their resident blocks)
        __shared__ double s_chunk[(INT || WT == WT_CEIL_2D || FLAT) ? 1 : 4096];
        final_cost = tour_cost_block<WT, INT>(a.coord, order, pos, n, s_d, FLAT ? chunk_buf : s_chunk);
    }

    // 4. the tickets for the next launch
    const int done = found ? 0 : 1;
    const double obj = found ? st->obj : final_cost;
    if constexpr (HIER) {   // count-up tickets back to zero for the next launch
        for (int k = tid; k < tile_rows; k += kScanThreads)
            __hip_atomic_store((gi32 *)(a.row_tickets + (size_t)tour * a.max_tile_rows + k), 0, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }

    if (tid == 0) {
        st->steps += 1;
        st->sweeps += 1;
        st->evals += TABU ? tabu_evals : (long long)n * (n - 1) / 2 - n;  // non-adjacent pairs (n >= 4)
        st->pairs_scanned += (long long)n * (n - 1) / 2;
        if (found) { st->moves += 1; st->reversed += L - 1; }
        st->obj = obj;
        st->done = done;
        if constexpr (FLAT) { st->parity = cur_parity; st->pending = found ? 1 : 0; st->mv_pa = pa; st->mv_pb = pb; }
#ifdef TSP_STAMPS
        stamps[9] = wall_clock64();
        for (int k = 1; k < 10; ++k) atomicAdd(&g_stamp_sum[k], stamps[k] - stamps[k - 1]);
        atomicAdd(&g_stamp_n, 1ull);
#endif
    }
}

}  // namespace tsp
