// two_opt_exh.hpp -- the exhaustive best-improvement sweep in tour-position order: k_move_pos + k_exh.
// Part of the GRID engine; included by two_opt_grid.hip only (one translation unit).
//
// What it is for.  alg_2opt_tabu (src/tabusearch.c:127-157) executes the delta expression for every non-adjacent pair
// of every sweep: 49 985 000 at n = 10 000.  The product's sweeps decide most pairs by bounds (two_opt_sweep.hpp,
// two_opt_cluster.hip); THIS kernel executes every one of them exactly -- it is the sweep SURVEY.md 8(d) defines the
// evals/s headline on ("every one of 49 985 000 pairs evaluated per sweep"), bench.py's timed region, and what a caller
// gets with TSP_NO_FILTER=1 on the integer-coordinate metrics.
//
// Why position order.  delta(i, j) = d(a, b) + d(a1, b1) - d(a, a1) - d(b, b1) with a1 = succ a, b1 = succ b.  In the
// reference's node-id order the four distances of a pair are unrelated to its neighbours'.  Number the nodes by tour
// position instead -- u_p = node at position p, D(p, q) = d(u_p, u_q), e[p] = d(u_p, u_{p+1}) -- and
//     delta(p, q) = D(p, q) + D(p + 1, q + 1) - e[p] - e[q]:
// the second new edge of pair (p, q) IS the first new edge of pair (p + 1, q + 1).  A lane that owns column q and walks
// down the rows therefore needs ONE new distance per pair (the other arrives from its left neighbour, which computed it
// one row earlier) instead of two, and both removed edges come from arrays built once per sweep.  A best-improvement
// sweep may visit the pairs in any order: the decision is the arg-min of (delta, (i, j)) with the nodes' own ids as the
// tie-break (strict '<' at tabusearch.c:151 keeps the first pair in (i < j) order), which is what every lane keeps.
// Every delta is still computed exactly (integer-valued distances from the exact roots of tsp_dist.hpp's int_root).
//
// Layout.  k_move_pos (one thread per position) DECIDES the previous sweep's move -- every block for itself, from the
// candidates k_exh left (sweep_decide, two_opt_step.hpp) --, carries it out of place (as k_move_recs does)
// and writes, in position order and padded: rec[p] = the record of u_p (exh_arith.hpp: -2x, -2y and the norm of its
// coordinates relative to node 0, and e[p - 1]; position n repeats position 0; further pads lie far outside the instance),
// pid[p] = u_p.
// Hand-off.  k_exh ends at its block's candidate: no counter, no last block.  No word is read and written by different blocks
// of one launch: a tour has two control blocks, k_move_pos reads slot s and its block 0 writes the advanced block to slot
// s ^ 1; k_exh reads `done` there and one thread of it sets `open` there ("candidates written, not decided"), which nobody
// else in that launch reads.  The host flips s per pair of launches; before it looks at a control block k_exh_close (one
// block per tour) turns an open sweep into a pending move, which the next k_move_pos or the flush carries out.
// k_exh: the pair-columns are cut into strips of W - 1 (W = 64 RJ columns of D per wave, RJ adjacent columns per lane),
// laid out from the RIGHT end (exh_strip: the partial strip is the leftmost one, which has the fewest rows);
// a strip's rows are its units of work, and the units of all strips, laid end to end, are dealt to the waves in
// contiguous ranges (at most two strips per wave).  Per row step a lane
// computes D(p, q) for its RJ columns (row operands are wave-uniform: scalar loads, no LDS), forms
//     sum = D(p - 1, q - 1) + D(p, q) - e[q - 1]             (one three-operand add; D(p - 1, q - 1): own register, or
//                                                             v_mov_b32_dpp wave_shr:1 for the lane's first column)
// and compares it with wbd + e[p - 1], wbd = the best delta any lane of the WAVE has seen so far: a wave-uniform bound, so the
// common path is one integer minimum per pair and one compare against a scalar per row step, and a rarely taken branch
// does the exact bookkeeping (delta, tie-break on node ids) for the few pairs that reach that bound -- about ln(pairs of the
// wave) times per wave.  Measured and not kept: a per-lane bound (a wave's 64 RJ pairs per row step held one that beat its
// own lane's best almost every step: 47.7 us per sweep at RJ = 4); a bound shared by all waves through one word per tour
// (atomicMin on improvement, re-read every 16 rows: 4 096 waves on one L2 line cost more than the pruning saves, 69.6 us).
#pragma once
#include "two_opt_step.hpp"
#include "exh_arith.hpp"

#pragma clang fp contract(off)

namespace tsp {

#ifdef TSP_STAMPS
// diagnostic build: per wave {100 MHz wall clock at start, at the end of its rows, shader cycles in between, 0}; [4] last
// block's candidate stored in g_exh_t (tools/diag_exh.py reads them).  Plain stores to slots of their own: 4 096
// atomics on one word at the start of a kernel would be the thing measured.
__device__ unsigned long long g_exh_w[8192 * 4];
__device__ unsigned long long g_exh_t[8];
#endif

constexpr int kExhPad = 1152;          // positions past n that k_move_pos fills (>= the widest strip + 2)
constexpr int kRowBatch = 4;           // rows whose records one batch of scalar loads fetches
constexpr int kExhRJ = 4;              // k_exh: columns per lane (8 and 16, and 1 and 2, measured slower)

template <int WT>
constexpr bool exh_metric() { return WT == WT_EUC_2D_ICOORD || WT == WT_CEIL_2D_ICOORD || WT == WT_ATT_ICOORD; }

template <int WT>
constexpr int exh_mode() { return WT == WT_EUC_2D_ICOORD ? EXH_NINT : (WT == WT_CEIL_2D_ICOORD ? EXH_CEIL : EXH_ATT); }

// the exact integer-valued distance of tsp_dist.hpp's int_root as an int32 (exh_arith.hpp)
template <int WT>
__device__ __forceinline__ int exh_dist(double cx, double cy, double cn, const ExhRec &r) {
    const double s = exh_s(cx, cy, cn, r.m2x, r.m2y, r.nrm);
    return exh_round<exh_mode<WT>()>(s, __builtin_amdgcn_sqrt(exh_root_arg<exh_mode<WT>()>(s)));
}

// The same for the RJ columns of a lane against one row, STAGE BY STAGE across the columns: the wave issues in order, so the RJ
// dependent chains (add -> fma -> fma -> sqrt -> round -> fma -> compare -> convert -> add-with-carry) only overlap if
// their instructions are interleaved in the stream.  Left to itself the scheduler keeps most of a chain together (fewer live
// registers) and a lone wave then runs the chains one after the other (RJ = 16, one wave per SIMD: 2 960 cycles per row step
// against 1 056 of issue).  The scheduling barriers pin the stage order.
template <int WT, int RJ>
__device__ __forceinline__ void exh_dist_row(const double (&cx)[RJ], const double (&cy)[RJ], const double (&cn)[RJ], const ExhRec &r,
                                             int (&D)[RJ]) {
    constexpr int M = exh_mode<WT>();
    double s[RJ], k[RJ], e[RJ];
    int ki[RJ];
    bool up[RJ];
#pragma unroll
    for (int q = 0; q < RJ; ++q) s[q] = exh_s(cx[q], cy[q], cn[q], r.m2x, r.m2y, r.nrm);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) k[q] = __builtin_amdgcn_sqrt(exh_root_arg<M>(s[q]));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) k[q] = exh_k<M>(k[q]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) e[q] = exh_e<M>(s[q], k[q]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) { ki[q] = exh_ki(k[q]); up[q] = exh_up<M>(k[q], e[q]); }   // every compare before the first
    __builtin_amdgcn_sched_barrier(0);   // add-with-carry, each with a carry register of its own (back to back they wait on VCC)
#pragma unroll
    for (int q = 0; q < RJ; ++q) {
        D[q] = exh_d(ki[q], up[q]);
        asm("" : "+v"(D[q]));   // D itself in a register (the next row needs it): the caller's sums are then one v_add3_u32 each
    }
    __builtin_amdgcn_sched_barrier(0);
}

// (1) the move: the open sweep's, decided here by every block for itself, or a pending one (decided by k_exh_close); (2) that move,
// out of place; (3) the tour AFTER it in position order: records and ids.  Reads the control block `states`, which no block of
// this launch writes; block 0 writes the advanced one to `states_next` (the tour's other slot), which no block of this launch reads.
template <int WT, bool INT>
__global__ __launch_bounds__(kScanThreads) void k_move_pos(const double2 *__restrict__ coord, int *orders, int *poss, int *orders2,
                                                           int *poss2, const TourState *__restrict__ states,
                                                           TourState *__restrict__ states_next, const Partial *__restrict__ partials,
                                                           size_t partial_per_tour, int flat_slots, ExhRec *__restrict__ rec,
                                                           int *__restrict__ pid, int n) {
    static_assert(exh_metric<WT>() && INT, "integer-coordinate metrics only (integer costs: the tour cost needs no staging)");
    __shared__ double s_d[kScanThreads / 64];
    __shared__ u64 s_k[kScanThreads / 64];
    const int tour = blockIdx.y;
    const TourState *st = states + tour;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    if (st->done) {   // a finished tour stays finished in both slots
        if (writer) states_next[tour] = *st;
        return;
    }
    const size_t base = (size_t)tour * n, pbase = (size_t)tour * (n + kExhPad);
    MoveView mv = move_view(st, orders + base, poss + base, orders2 + base, poss2 + base, n);
    const bool open = st->open != 0;   // (then nothing is pending: mv.L == 0)
    SweepDecision dec;
    if (open) {
        dec = sweep_decide(partials + (size_t)tour * partial_per_tour, flat_slots, mv.pos, n, s_d, s_k);
        if (!dec.found) {   // the local optimum: block 0 recomputes the cost (tabusearch.c:168-172), nobody has records to build
            if (blockIdx.x != 0) return;
            const double cost = tour_cost_block<WT, INT>(coord, mv.order, mv.pos, n, s_d, nullptr);
            if (writer) {
                TourState z = *st;
                sweep_count(z, dec, n, cost);
                z.pending = 0;
                states_next[tour] = z;
            }
            return;
        }
        mv.L = dec.L; mv.pa1 = dec.pa + 1 == n ? 0 : dec.pa + 1;
    }
    const int k = blockIdx.x * kScanThreads + threadIdx.x;
    if (k >= n + kExhPad) return;
    // every load of the current copy (which this kernel never writes) comes before the first store
    const int u = k < n ? mv.node_at(k) : (k == n ? mv.node_at(0) : -1);
    const int v = k >= 1 && k <= n ? mv.node_at(k - 1) : -1;   // the position before
    const double2 c0 = coord[0];
    double2 cu = make_double2(c0.x - 6.0e6, c0.y - 6.0e6);   // pads: farther from every node than any tour edge is long
    int len = 0;
    if (u >= 0) cu = coord[u];
    if (v >= 0) { const double2 cv = coord[v]; len = (int)dist_xy<WT, INT>(cv.x, cv.y, cu.x, cu.y); }
    if (mv.L > 0 && k < n) {
        int *o_new = (st->parity ? orders : orders2) + base, *p_new = (st->parity ? poss : poss2) + base;
        o_new[k] = u;
        p_new[u] = k;
    }
    ExhRec r;
    exh_rec_xy(cu.x - c0.x, cu.y - c0.y, r);   // exact: integers whose difference is below 2^21 (the pads: 6e6)
    r.eprev = len;
    r.pad_ = 0;
    rec[pbase + k] = r;
    pid[pbase + k] = u;
    if (writer) {   // the next control block: the sweep counted, the move carried out (the other copy is the current one now)
        // (the writer is thread 0 of block 0: k = 0, never past the early return above)
        TourState z = *st;
        if (open) sweep_count(z, dec, n, 0.0);
        if (mv.L > 0) z.parity ^= 1;
        z.pending = 0;
        states_next[tour] = z;
    }
}

// Before the host looks at a control block (a poll, the end of a run): an open sweep becomes a decided one -- the counters, and
// either a pending move, which the next k_move_pos or the flush carries out, or the finished tour's recomputed cost.  One block
// per tour, so it updates the control block it reads (behind the barriers of the decision).
template <int WT, bool INT>
__global__ __launch_bounds__(kScanThreads) void k_exh_close(const double2 *__restrict__ coord, const int *orders, const int *poss,
                                                            const int *orders2, const int *poss2, TourState *states,
                                                            const Partial *__restrict__ partials, size_t partial_per_tour,
                                                            int flat_slots, int n) {
    static_assert(exh_metric<WT>() && INT, "integer-coordinate metrics only");
    __shared__ double s_d[kScanThreads / 64];
    __shared__ u64 s_k[kScanThreads / 64];
    const int tour = blockIdx.x;
    TourState *st = states + tour;
    if (st->done || !st->open) return;
    const size_t base = (size_t)tour * n;
    const bool second = st->parity != 0;
    const int *order = (second ? orders2 : orders) + base, *pos = (second ? poss2 : poss) + base;
    const SweepDecision dec = sweep_decide(partials + (size_t)tour * partial_per_tour, flat_slots, pos, n, s_d, s_k);
    double cost = 0.0;
    if (!dec.found) cost = tour_cost_block<WT, INT>(coord, order, pos, n, s_d, nullptr);
    if (threadIdx.x == 0) {
        TourState z = *st;
        sweep_count(z, dec, n, cost);
        z.pending = dec.found;
        *st = z;
    }
}

// RJ = kExhRJ columns per lane, four workgroups of four waves per CU (the host pins that with its LDS request)
template <int WT, bool INT, int RJ>
__global__ __launch_bounds__(kScanThreads, 1) void k_exh(const StepArgs a, const ExhRec *__restrict__ rec_all,
                                                      const int *__restrict__ pid_all, int waves_total, int4 share, int gens) {
    // the position arrays are kernel arguments of their own, restrict-qualified: the row operands are wave-uniform loads, and
    // the compiler only issues them as scalar loads (s_load: no vector-memory slot, no VGPRs) when it can prove that the
    // kernel's own stores (the candidate slot, `open`) never touch them
    static_assert(exh_metric<WT>(), "integer-coordinate metrics only");
    constexpr int W = 64 * RJ, WEFF = W - 1;
    const int tour = blockIdx.z;
    const TourState *st = a.states + tour;
    if (st->done) return;
    const int n = a.n, tid = threadIdx.x, lane = tid & 63;
    const size_t pbase = (size_t)tour * (n + kExhPad);
    const ExhRec *__restrict__ rec = rec_all + pbase;
    const int *__restrict__ pid = pid_all + pbase;

#ifdef TSP_STAMPS
    const unsigned long long stamp_r0 = wall_clock64(), stamp_c0 = clock64();
    unsigned long long stamp_hits = 0, stamp_hit_cycles = 0;
#endif
    // ---- this wave's share: units [u_lo, u_hi) of the strips' rows laid end to end --------------------------------
    const int gw = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (kScanThreads / 64) + (tid >> 6));
    const int strips = exh_strips(n, WEFF);                         // pair-columns 0 .. n-1
    const long long total = exh_total_rows(n, WEFF);                // pair-rows p' < q' <= q0 + WEFF - 1, p' <= n - 2
    // A SIMD serves its oldest wave first, and the workgroups of a CU are as old as their place in the grid: the first quarter of
    // the grid leaves its rows at 13.7 us, the others at 20.6 / 28.2 / 35.4 (equal shares; tools/diag_exh.py) -- while four waves
    // are active the SIMD's issue slots go 53 / 26 / 13 / 8 %.  share = the rows per wave of each part of the grid (quarters at four workgroups per CU) in those
    // proportions (host: tsp_dev_tours_create), so that the four waves of a SIMD finish together; share.x == 0: equal shares.
    long long per = (total + waves_total - 1) / waves_total;
    long long u_lo = per * gw;
    if (share.x > 0 && gens > 0) {   // gens = workgroups per CU = equal parts of the grid with a share of their own (2 .. 4)
        const int wq = waves_total / gens, g = min(gens - 1, gw / wq), idx = gw - g * wq;
        const int sh[4] = {share.x, share.y, share.z, share.w};
        u_lo = 0;
        for (int q = 0; q < g; ++q) u_lo += (long long)sh[q] * wq;
        per = sh[g];
        u_lo += per * idx;
    }
    long long u_hi = min(total, u_lo + per);
    u_lo = min(u_lo, total);

    int bd = -1, bp = -1, bq = -1;     // integer costs: delta < 0  <=>  delta <= -1; (bd, no pair) loses every tie
    int wbd = -1;                      // wave-uniform: the lowest delta any lane of this wave has seen

    // exact bookkeeping for a pair that reached the wave's best: delta, then -- on a tie only -- the reference's tie-break on
    // node ids (two dependent global loads: not on the path of a strict improvement)
    auto consider = [&](int sum, int erow, int pp, int qq, bool valid) {
        const int d = sum - erow;
        if (valid && d <= bd) {
            bool take = d < bd || bp < 0;
            if (!take) {
                const int i1 = pid[pp], j1 = pid[qq], i0 = pid[bp], j0 = pid[bq];
                take = make_key(min(i1, j1), max(i1, j1)) < make_key(min(i0, j0), max(i0, j0));
            }
            if (take) { bd = d; bp = pp; bq = qq; }
        }
    };

    long long cum = 0;
    for (int s = 0; s < strips && u_lo < u_hi; ++s) {
        const ExhStrip strip = exh_strip(n, WEFF, s);
        const int rows_s = strip.rows;
        if (u_lo >= cum + rows_s) { cum += rows_s; continue; }
        // segment of strip s: pair-rows [pa, pb)
        const int pa = (int)(u_lo - cum), pb = (int)min<long long>(rows_s, u_hi - cum);
        u_lo = cum + pb;
        cum += rows_s;
        const int Q0 = strip.q0;
        double cx[RJ], cy[RJ], cn[RJ];
        int nce[RJ], Dp[RJ], qk[RJ];   // nce[k] = -e[q_k - 1]: what the pair of column k removes on the column side
#pragma unroll
        for (int k = 0; k < RJ; ++k) {
            qk[k] = Q0 + RJ * lane + k;
            const ExhRec c = rec[qk[k]];
            cx[k] = exh_col(c.m2x); cy[k] = exh_col(c.m2y); cn[k] = c.nrm; nce[k] = -c.eprev;
        }
        // lane 0's first column has no left neighbour in this wave (the DPP hands it 0, and position 0 has no edge before it):
        // its pair belongs to the strip on the left; should D alone ever pass the test below, the bookkeeping drops it
        if (lane == 0) nce[0] = 0;
#pragma unroll
        for (int k = 0; k < RJ; ++k) asm("" : "+v"(nce[k]));   // kept negated: an addend of v_add3_u32, not a subtraction of its own
        {   // row pa: distances only
            const ExhRec r = rec[pa];
#pragma unroll
            for (int k = 0; k < RJ; ++k) Dp[k] = exh_dist<WT>(cx[k], cy[k], cn[k], r);
        }
        // rows p = pa + 1 .. pb: D(p, .), then the pairs (p - 1, q - 1).  Up to p = Q0 every column of the strip lies above
        // the row (q_k > p for every evaluated pair); beyond it the pairs on and below the diagonal are masked.
        auto step = [&](int p, const ExhRec r, auto pred_c) {
            constexpr bool PRED = decltype(pred_c)::value;
            int D[RJ], sum[RJ];
            const int erow = r.eprev;   // e[p - 1]
            exh_dist_row<WT, RJ>(cx, cy, cn, r, D);
            sum[0] = __builtin_amdgcn_update_dpp(0, Dp[RJ - 1], 0x138 /* wave_shr:1 */, 0xf, 0xf, true) + D[0] + nce[0];
#pragma unroll
            for (int k = 1; k < RJ; ++k) sum[k] = Dp[k - 1] + D[k] + nce[k];
            const int thr = wbd + erow;   // scalar
            bool hit = false;
#pragma unroll
            for (int k = 0; k < RJ; ++k) hit = hit || (sum[k] <= thr && (!PRED || qk[k] > p));
#pragma unroll
            for (int k = 0; k < RJ; ++k) Dp[k] = D[k];
            if (__builtin_expect(__any(hit), 0)) {
#ifdef TSP_STAMPS
                const unsigned long long sc0 = clock64();
#endif
#pragma unroll
                for (int k = 0; k < RJ; ++k) consider(sum[k], erow, p - 1, qk[k] - 1, (k > 0 || lane > 0) && qk[k] > p);
                const int nb = (int)(unsigned)(wave_min_u64((u64)((unsigned)bd ^ 0x80000000u)) ^ 0x80000000u);
                wbd = min(wbd, nb);
#ifdef TSP_STAMPS
                stamp_hits += 1; stamp_hit_cycles += clock64() - sc0;
#endif
            }
        };
        // The row records are wave-uniform: scalar loads, kRowBatch rows per batch, and the NEXT batch is on its way
        // while this one is worked (a scalar load that misses the CU's constant cache takes longer than one row step: with a
        // prefetch distance of one row the waves spent a quarter of their cycles in s_waitcnt, SQ_WAIT_ANY).  Positions up to
        // n + 2 kRowBatch exist: k_move_pos pads.
        struct Rows { ExhRec r[kRowBatch]; };
        const int p_plain = min(pb, Q0);
        int p = pa + 1;
        Rows nx = *reinterpret_cast<const Rows *>(rec + p);
        for (; p <= pb; p += kRowBatch) {
            const Rows cur = nx;
            nx = *reinterpret_cast<const Rows *>(rec + p + kRowBatch);
            if (p + kRowBatch - 1 <= p_plain) {
#pragma unroll
                for (int u = 0; u < kRowBatch; ++u) step(p + u, cur.r[u], std::false_type{});
            } else {
#pragma unroll
                for (int u = 0; u < kRowBatch; ++u)
                    if (p + u <= pb) step(p + u, cur.r[u], std::true_type{});   // the predicate is harmless above the diagonal
            }
        }
    }

    // ---- the wave's and the block's arg-min (delta, (i, j)); the tour's is taken by the next launch -----------------------
#ifdef TSP_STAMPS
    if (lane == 0 && tour == 0) {
        const int w = (int)blockIdx.x * (kScanThreads / 64) + (tid >> 6);
        if (w < 8192) { g_exh_w[4 * w] = stamp_r0; g_exh_w[4 * w + 1] = wall_clock64(); unsigned hwid, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            g_exh_w[4 * w + 2] = (clock64() - stamp_c0) | ((unsigned long long)hwid << 32); g_exh_w[4 * w + 3] = 1 | (stamp_hits << 8) | ((unsigned long long)(xcc & 0xf) << 60) | ((stamp_hit_cycles & 0xfffffffffull) << 24); }
    }
#endif
    // only the lanes that hold the wave's lowest delta need their pair's node ids (usually one lane: one pair of loads)
    double d = 0.0;
    u64 key = kNoKey;
    {
        const int wmin = (int)(unsigned)(wave_min_u64((u64)((unsigned)bd ^ 0x80000000u)) ^ 0x80000000u);
        if (bp >= 0 && bd == wmin) {
            const int i = pid[bp], j = pid[bq];
            d = (double)bd;
            key = make_key(min(i, j), max(i, j));
        }
    }
    __shared__ double s_d[kScanThreads / 64];
    __shared__ u64 s_k[kScanThreads / 64];
    block_argmin<true>(d, key, s_d, s_k);
    // The launch ends here: the block's candidate, empty or not, as plain stores -- its readers (every block of the next
    // k_move_pos, or k_exh_close) are later launches.  `open` tells them so; nothing in this launch reads it.
    if (tid == 0) {
        Partial p;
        p.delta = d; p.i = key_i(key); p.j = key_j(key);
        a.partials[(size_t)tour * a.partial_per_tour + blockIdx.x] = p;
        if (blockIdx.x == 0) a.states[tour].open = 1;
#ifdef TSP_STAMPS
        atomicMax(&g_exh_t[4], wall_clock64());
#endif
    }
}

}  // namespace tsp
