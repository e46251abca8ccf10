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
// The root.  k_exh takes the integer root from an fp32 seed (exh_arith.hpp, the seed form): s, exact in fp64, is rounded to
// fp32, v_sqrt_f32 gives the seed, the integer comes out of the fp32 value (truncated for EUC_2D, rounded for CEIL_2D and ATT), its
// fp64 image feeds the exact residual s - k^2, and the one-sided fix-up adds the carry: convert, root, convert, convert, fma,
// compare, add-with-carry -- no v_sqrt_f64 (16 cycles of the port against 8), no fp64 floor, no fp64-to-integer conversion.
// Exact for every root below 2^21 with the seed up to 2 fp32 ulps off (tests/test_cpu_exh_seed.py, tests/test_gpu_exh_seed.py;
// +3.2 % on bench.py).  k_move_pos keeps the fp64 root for its two cut-point distances per sweep (exh_perm_rec): both
// forms give the same integers.
//
// Layout.  k_move_pos (one thread per position) DECIDES the previous sweep's move -- every block for itself, from the
// candidates k_exh left, which name their pairs by tour POSITION (exh_decide below, the rule in exh_decide.hpp: pos is not read, a
// node id only when two different pairs share the minimal delta; the candidates are asked for together with the control block,
// one wait) --, carries it out of place (as k_move_recs does) and writes, in position order and padded: rec[p] = the record of
// u_p (exh_arith.hpp: -2x, -2y and the norm of its coordinates relative to node 0, e[p - 1], and u_p itself; position n repeats
// position 0; further pads lie far outside the instance and carry the id -1).  There is no array of ids by position beside them.
// Records by permutation.  A 2-opt move only permutes positions: but for the two cut points, the record of the new position k is
// bit for bit an old record and its e is an old e (exh_perm, exh_arith.hpp; tests/test_cpu_exh_permute.py).  A tour has two
// record buffers; k_move_pos<HOT> reads one and writes the other, the k_exh behind it reads what it wrote, the host flips
// them with the pair of launches.  The chain of a hot launch is {control block, candidates} -> arg-min -> {old records, the ids
// at the pair's two positions} -> stores (their addresses come from preloaded kernel arguments): the pair is decided by position
// and its orientation -- pa is the position of the smaller id -- is not known when the records are asked for, so a thread
// evaluates exh_perm for both orientations, asks for the records of both and the two ids in one round, and keeps one behind the
// single wait.  order, pos and coord are neither read nor written, and the pads (written into both buffers when the handle is
// created, k_exh_pads) are not touched: a hot launch covers positions 0 .. n.
// Who owns the truth.  The first sweep of a run call is cold: built from order and coord, which describe the tour between run
// calls.  From then on, for as long as the host's tsp_dev_tours::exh_hot holds, the RECORDS are the tour (the buffer a tour's
// control block names, TourState::rec_buf; a pending move not yet carried out in them) and order / pos / parity are stale: no
// launch of the run reads them -- the decision, the orientation, the tie-break and the finished tour's cost (the sum of eprev)
// all come from the records, in k_move_pos and in k_exh_close alike.  Where exh_hot ends -- the flush at the end of a run call,
// a failed launch, an error return -- k_exh_settle writes order and pos back from the records, one launch, and only then is a
// pending move carried out in them: when the run call returns they describe the tour exactly as before.
// Hand-off.  k_exh ends at its block's candidate {delta, p, q}, p < q the POSITIONS of the pair, one 16-byte store: no counter,
// no last block, and no node id -- behind a wave's last row come one wave_min, a ballot, one barrier and one thread's fold of the
// block's four waves.  The ids are needed for the tie-break among different pairs at the minimal delta (rare: loaded from the
// records inside that branch, in a lane's bookkeeping, in the wave, in the block and in k_move_pos alike) and for the move's
// orientation, which k_move_pos settles in the round of loads it waits for anyway: +3.2 % on bench.py, DESIGN 4.9.  (Measured
// and not kept: the ids of a lane's pair taken from the records and kept in registers -- four more VGPRs and their moves at every
// strip start: -1.5 %; one candidate per WAVE, 4 096 of them and no barrier in k_exh -- k_exh as short as with one per block,
// k_move_pos 0.3 us longer with sixteen candidates per thread instead of four: +0.4 to +1.0 % only)
// No word is read and written by different blocks
// of one launch: a tour has two control blocks, k_move_pos reads slot s and its block 0 writes the advanced block to slot
// s ^ 1; k_exh reads `done` there and one thread of it sets `open` there ("candidates written, not decided"), which nobody
// else in that launch reads.  The host flips s per pair of launches; before it looks at a control block k_exh_close (one
// block per tour) turns an open sweep into a pending move, which the next k_move_pos (in the records) or the flush (in order / pos,
// behind k_exh_settle) carries out.
// k_exh: the pair-columns are cut into strips of W - 1 (W = 64 RJ columns of D per wave, RJ adjacent columns per lane),
// laid out from the RIGHT end (exh_strip: the partial strip is the leftmost one, which has the fewest rows);
// a strip's rows are its units of work, and the units of all strips, laid end to end, are dealt to the waves in
// contiguous ranges -- by the host, once per tours handle (exh_deal, exh_arith.hpp: strip, row and number of units per wave, in
// a table the wave reads with one scalar load); the wave walks the strips from there, over as many as its range covers.
// The start of a wave, which every wave of the launch goes through at once and nothing hides, is two waits on memory: `done`
// and the descriptor; the columns' records, row pa and the first batch of rows.  The kernel arguments those need are in the
// wave's SGPRs when it starts (kernel-argument preload: the parameters of both kernels are ordered for it; firmware that does
// not preload runs the compiler's prologue, which loads them, and then the waits are three).  Measured and not kept, DESIGN
// 4.9: the descriptor evaluated by the wave in closed form instead of loaded (one wait, but about 90 scalar instructions more
// per wave: -2.0 %), and the ids of a lane's best pair asked for where the pair is taken (the compiler waits for them at the
// join behind every row's branch: -2.8 %).  Per row step a lane
// computes D(p, q) for its RJ columns (row operands are wave-uniform: scalar loads, no LDS), forms
//     sum = D(p - 1, q - 1) + D(p, q) - e[q - 1]             (one three-operand add; D(p - 1, q - 1): own register, or
//                                                             v_mov_b32_dpp wave_shr:1 for the lane's first column)
// and compares it with wbd + e[p - 1], wbd = the best delta any lane of the WAVE has seen so far: a wave-uniform bound, so the
// common path is one integer minimum per pair and one compare against a scalar per row step, and a rarely taken branch
// does the exact bookkeeping (delta, tie-break on node ids) for the few pairs that reach that bound -- about ln(pairs of the
// wave) times per wave.  Measured and not kept: a per-lane bound (a wave's 64 RJ pairs per row step held one that beat its
// own lane's best almost every step: 47.7 us per sweep at RJ = 4); a bound shared by all waves through one word per tour
// (atomicMin on improvement, re-read every 16 rows: 4 096 waves on one L2 line cost more than the pruning saves, 69.6 us);
// the bound tested once per batch of kRowBatch rows instead of once per row (the rows of a batch one basic block, their hit
// masks OR-ed, one branch; with the stage order of a row kept, with a row's integer tail free to issue among the next row's
// first stage, and with the rows of a batch scheduled freely: k_exh 29.37 us per launch in every form, as with the branch
// per row -- the model loop of tools/ubench/dist3.hip promised 15 % of a row step).
#pragma once
#include "two_opt_step.hpp"
#include "exh_arith.hpp"
#include "exh_decide.hpp"

#pragma clang fp contract(off)

namespace tsp {

#ifdef TSP_STAMPS
// diagnostic build: per wave {100 MHz wall clock at start, at the end of its rows, shader cycles in between, 0}; [4] last
// wave's candidate stored in g_exh_t (tools/diag_exh.py reads them).  Plain stores to slots of their own: 4 096
// atomics on one word at the start of a kernel would be the thing measured.
__device__ unsigned long long g_exh_w[8192 * 4];
__device__ unsigned long long g_exh_t[8];
__device__ unsigned long long g_exh_f[8192];   // per wave: wall clock when its first row step begins (0: a wave without rows)
#endif

constexpr int kExhPad = 1152;          // positions past n that k_move_pos fills (>= the widest strip + 2)
constexpr int kRowBatch = 4;           // rows whose records one batch of scalar loads fetches
constexpr int kExhRJ = 4;              // k_exh: columns per lane (8 and 16, and 1 and 2, measured slower)

template <int WT>
constexpr bool exh_metric() { return WT == WT_EUC_2D_ICOORD || WT == WT_CEIL_2D_ICOORD || WT == WT_ATT_ICOORD; }

template <int WT>
constexpr int exh_mode() { return WT == WT_EUC_2D_ICOORD ? EXH_NINT : (WT == WT_CEIL_2D_ICOORD ? EXH_CEIL : EXH_ATT); }

// the exact integer-valued distance of tsp_dist.hpp's int_root as an int32 (exh_arith.hpp, the seed form: an fp32 root under
// the one-sided fix-up in fp64)
template <int WT>
__device__ __forceinline__ int exh_dist(double cx, double cy, double cn, const ExhRec &r) {
    const double s = exh_s(cx, cy, cn, r.m2x, r.m2y, r.nrm);
    return exh_seed_round<exh_mode<WT>()>(s, __builtin_amdgcn_sqrtf(exh_seed_arg<exh_mode<WT>()>(s)));
}

// The same for the RJ columns of a lane against one row, STAGE BY STAGE across the columns: the wave issues in order, so the RJ
// dependent chains (add -> fma -> fma -> convert to fp32 -> fp32 root -> convert to integer -> convert to fp64 -> fma -> compare ->
// add-with-carry; CEIL_2D and ATT round the fp32 root first, ATT multiplies twice more) only overlap if
// their instructions are interleaved in the stream.  Left to itself the scheduler keeps most of a chain together (fewer live
// registers) and a lone wave then runs the chains one after the other (RJ = 16, one wave per SIMD: 2 960 cycles per row step
// against 1 056 of issue).  The scheduling barriers pin the stage order.
template <int WT, int RJ>
__device__ __forceinline__ void exh_dist_row(const double (&cx)[RJ], const double (&cy)[RJ], const double (&cn)[RJ], const ExhRec &r,
                                             int (&D)[RJ]) {
    constexpr int M = exh_mode<WT>();
    double s[RJ], k[RJ], e[RJ];
    float g[RJ];
    int ki[RJ];
    bool up[RJ];
#pragma unroll
    for (int q = 0; q < RJ; ++q) s[q] = exh_s(cx[q], cy[q], cn[q], r.m2x, r.m2y, r.nrm);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) g[q] = exh_seed_arg<M>(s[q]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) g[q] = __builtin_amdgcn_sqrtf(g[q]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) ki[q] = exh_seed_ki<M>(g[q]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) k[q] = exh_seed_k(ki[q]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) e[q] = exh_e<M>(s[q], k[q]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < RJ; ++q) up[q] = exh_up<M>(k[q], e[q]);   // every compare before the first
    __builtin_amdgcn_sched_barrier(0);   // add-with-carry, each with a carry register of its own (back to back they wait on VCC)
#pragma unroll
    for (int q = 0; q < RJ; ++q) {
        D[q] = exh_d(ki[q], up[q]);
        asm("" : "+v"(D[q]));   // D itself in a register (the next row needs it): the caller's sums are then one v_add3_u32 each
    }
    __builtin_amdgcn_sched_barrier(0);
}

// ---- the decision of a sweep from the candidates a FINISHED k_exh has left (exh_decide.hpp has the rule) -------------------------
// One candidate per workgroup of k_exh: kExhCandPU per thread and round, and at most two rounds (k_exh's grid is capped at 2 048
// workgroups of four waves).  The candidates' addresses depend on the thread alone, so a caller with loads of its own to wait for
// (k_move_pos: the control block) issues exh_cand_load first and lets both travel together.
constexpr int kExhCandPU = 4;   // 1 024 candidates = 4 per thread: one round
constexpr int kExhMaxCand = 2 * kExhCandPU * kScanThreads;
struct ExhCandLoads { ExhCand c[kExhCandPU]; };

// one round of a thread's loads: slots s0, s0 + kScanThreads, ...  Every load is issued, none under a condition of its own (the
// compiler waits for a load inside a branch at the branch's end: a round trip per load instead of one for all): a slot past the end reads
// the last one and is emptied by exh_cand_settle, behind the wait.  nslots >= 1.
__device__ __forceinline__ ExhCandLoads exh_cand_load(const ExhCand *__restrict__ cand, int nslots, int s0) {
    ExhCandLoads l;
#pragma unroll
    for (int k = 0; k < kExhCandPU; ++k) l.c[k] = cand[min(s0 + k * kScanThreads, nslots - 1)];
    return l;
}
__device__ __forceinline__ void exh_cand_settle(ExhCandLoads &l, int nslots, int s0) {
#pragma unroll
    for (int k = 0; k < kExhCandPU; ++k)
        if (s0 + k * kScanThreads >= nslots) l.c[k].p = -1;
}

// keeps the loads of a round where they were issued: to be called behind the caller's own loads and a scheduling barrier,
// before the first use of any of them
__device__ __forceinline__ void exh_cand_pin(const ExhCandLoads &l) {
#pragma unroll
    for (int k = 0; k < kExhCandPU; ++k) asm volatile("" : : "v"(l.c[k].delta), "v"(l.c[k].p), "v"(l.c[k].q));
}

// Block-wide (kScanThreads threads), for every block that wants the answer: the pair the sweep chose, by position (p < q), or
// found == 0 at the local optimum.  `first`: the round exh_cand_load(cand, nslots, threadIdx.x) fetched; the second round, where
// there is one, is issued here before the first fold.  id_at(position) is asked only when two different pairs share the minimal
// delta.  s_d, s_k: >= kScanThreads / 64 entries each.
struct ExhPair { int found, p, q; };
template <class IdAt>
__device__ __forceinline__ ExhPair exh_decide(const ExhCandLoads &first, const ExhCand *__restrict__ cand, int nslots, IdAt id_at,
                                              double *s_d, u64 *s_k) {
    __shared__ u64 s_pair;
    const bool two = nslots > kExhCandPU * kScanThreads;   // (block-uniform)
    const int tid = threadIdx.x;
    ExhCandLoads one = first, more;
    if (two) more = exh_cand_load(cand, nslots, tid + kExhCandPU * kScanThreads);
    exh_cand_settle(one, nslots, tid);
    ExhBest b;
#pragma unroll
    for (int k = 0; k < kExhCandPU; ++k) exh_fold(b, one.c[k]);
    if (two) {
        exh_cand_settle(more, nslots, tid + kExhCandPU * kScanThreads);
#pragma unroll
        for (int k = 0; k < kExhCandPU; ++k) exh_fold(b, more.c[k]);
    }
    // The block's arg-min of (delta, position key) and the OR of exh_ambiguous in ONE exchange through LDS: a wave hands on its
    // arg-min and whether one of its lanes is ambiguous against THAT -- which is the lane's word against the block's arg-min
    // wherever the wave's delta is the block's, and is not looked at elsewhere; a wave whose arg-min is another pair at the
    // block's delta is ambiguous by itself.  (block_argmin of two_opt_common.hpp with a third word: no barrier of its own.)
    __shared__ int s_amb[kScanThreads / 64];
    double d = (double)b.delta;
    u64 key = b.key;
    wave_argmin<true>(d, key);
    const bool wave_amb = __any(exh_ambiguous(b, (int)d, key));
    __syncthreads();
    if ((tid & 63) == 0) { s_d[tid >> 6] = d; s_k[tid >> 6] = key; s_amb[tid >> 6] = wave_amb; }
    __syncthreads();
    d = s_d[0]; key = s_k[0];
    for (int w = 1; w < kScanThreads / 64; ++w)
        if (better(s_d[w], s_k[w], d, key)) { d = s_d[w]; key = s_k[w]; }
    if (key == kNoKey || !(d < 0)) return {0, -1, -1};   // (block-uniform)
    const int delta = (int)d;
    bool ambiguous = false;
    for (int w = 0; w < kScanThreads / 64; ++w)
        ambiguous = ambiguous || (s_k[w] != kNoKey && s_d[w] == d && (s_amb[w] != 0 || s_k[w] != key));
    if (ambiguous) {   // (block-uniform)
        ExhIdBest ib;
#pragma unroll
        for (int k = 0; k < kExhCandPU; ++k) exh_fold_ids(ib, one.c[k], delta, id_at);
        if (two) {
#pragma unroll
            for (int k = 0; k < kExhCandPU; ++k) exh_fold_ids(ib, more.c[k], delta, id_at);
        }
        u64 idkey = ib.idkey;
        double unused = 0.0;
        block_argmin<false>(unused, idkey, s_d, s_k);
        if (ib.idkey == idkey) s_pair = ib.poskey;   // an id key names one pair: every owner holds the same positions
        __syncthreads();
        key = s_pair;
    }
    return {1, exh_key_hi(key), exh_key_lo(key)};
}

// the decided and oriented pair as the move the control block counts (sweep_count)
__device__ __forceinline__ SweepDecision exh_decision(const ExhMove &m) {
    SweepDecision d;
    d.found = 1; d.pa = m.pa; d.pb = m.pb; d.L = m.L;
    return d;
}

// The cost of the tour whose records these are (tabusearch.c:168-172): the sum of the edges that end at positions 1 .. n, position
// n being the repeat of position 0 with the closing edge.  Integer-valued terms below 2^53 in all: exact in any order, so the
// same double, bit for bit, as tour_cost_block's sum over the nodes.  Block-wide.
__device__ __forceinline__ double exh_rec_cost(const ExhRec *__restrict__ rec, int n, double *s_d) {
    double c = 0.0;
    for (int k = 1 + (int)threadIdx.x; k <= n; k += (int)blockDim.x) c += (double)rec[k].eprev;
    return block_sum<double>(c, s_d);
}

// Positions n + 1 .. n + kExhPad - 1 of both record buffers, once per tours handle: far outside the instance, no edge, id -1 --
// what a cold k_move_pos writes there.  Hot launches stop at position n.
__global__ void k_exh_pads(const double2 *__restrict__ coord, ExhRec *__restrict__ rec_a, ExhRec *__restrict__ rec_b, int n) {
    const int k = n + 1 + blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n + kExhPad) return;
    const double2 c0 = coord[0];
    const double2 cu = make_double2(c0.x - 6.0e6, c0.y - 6.0e6);
    ExhRec r;
    exh_rec_xy(cu.x - c0.x, cu.y - c0.y, r);
    r.eprev = 0;
    r.id = -1;
    const size_t at = (size_t)blockIdx.y * (n + kExhPad) + k;
    rec_a[at] = r;
    rec_b[at] = r;
}

// When the records stop being the tour (the end of a run call, before the flush carries out a pending move; a failed launch):
// order and pos, in the copy that parity names, back from the tour's last records.  One launch per run call instead of two
// stores per thread and sweep.  (The flush behind it clears the mark with parity and pending, k_flush_state.)
// Which buffer: the one the tour's control block names (rec_buf: 1 or 2, set by the last k_move_pos that wrote records of this
// tour -- a tour that finished some launches ago has its last records in either buffer, whatever the host's exh_buf says now);
// 0: no launch since the last flush has written any (a tour that was finished when the run call began), order and pos are current.
__global__ void k_exh_settle(const ExhRec *__restrict__ rec_a, const ExhRec *__restrict__ rec_b, const TourState *__restrict__ states,
                             int *orders, int *poss, int *orders2, int *poss2, int n) {
    const int tour = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
    const int mark = states[tour].rec_buf;
    if (k >= n || mark == 0) return;
    const bool second = states[tour].parity != 0;
    const size_t base = (size_t)tour * n;
    const int u = (mark == 1 ? rec_a : rec_b)[(size_t)tour * (n + kExhPad) + k].id;
    if ((unsigned)u >= (unsigned)n) return;   // (positions 0 .. n - 1 of written records hold node ids; never a store out of bounds)
    ((second ? orders2 : orders) + base)[k] = u;
    ((second ? poss2 : poss) + base)[u] = k;
}

// (1) the move: the open sweep's, decided here by every block for itself, or a pending one (decided by k_exh_close); (2) that move,
// out of place; (3) the tour AFTER it in position order: records, ids in them.  Reads the control block `states`, which no block of
// this launch writes; block 0 writes the advanced one to `states_next` (the tour's other slot), which no block of this launch reads.
// HOT: `rec_old` holds the records of the tour BEFORE the move (the previous sweep's, written by the previous k_move_pos of the
// same run call: the host knows, tsp_dev_tours::exh_hot) and the new ones are a permutation of them (exh_perm, exh_arith.hpp):
// order, pos and coord are not read, no root is taken but at the move's two cut points, and the chain of the launch is
// {control block, candidates} -> arg-min -> old records -> stores.  Otherwise (the first sweep of a run
// call) the records are built from order and coord, two round trips more.
// The order of the parameters: what the head of the chain needs comes first and fills the 14 dwords that a wave finds in its
// SGPRs when it starts (kernel-argument preload, csrc/Makefile), so {control block, candidates} are asked for with no wait in
// front of them; the rest is fetched by the entry's one batch of scalar loads.
template <int WT, bool INT, bool HOT>
__global__ __launch_bounds__(kScanThreads) void k_move_pos(const TourState *__restrict__ states, const ExhCand *__restrict__ cands,
                                                           const ExhRec *__restrict__ rec_old, int cand_per_tour, int n,
                                                           ExhRec *__restrict__ rec, TourState *__restrict__ states_next,
                                                           const double2 *__restrict__ coord, int *orders, int *poss, int *orders2,
                                                           int *poss2, int rec_mark) {
    static_assert(exh_metric<WT>() && INT, "integer-coordinate metrics only (integer costs: the tour cost needs no staging)");
    __shared__ double s_d[kScanThreads / 64];
    __shared__ u64 s_k[kScanThreads / 64];
    const int tour = blockIdx.y;
    const TourState *st = states + tour;
    const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
    // The candidates' addresses do not depend on the control block: both are asked for before either is used -- one wait.
    // (A finished tour, or one without an open sweep, has loaded candidates it does not look at.)
    const ExhCand *cand = cands + (size_t)tour * cand_per_tour;
    const ExhCandLoads first = exh_cand_load(cand, cand_per_tour, threadIdx.x);
    int done = st->done, is_open = st->open, parity = st->parity, pending = st->pending, mv_pa = st->mv_pa, mv_pb = st->mv_pb;
    __builtin_amdgcn_sched_barrier(0);
    // (and every kernel argument fetched by the entry's one batch of loads, not by batches of their own further down; the
    // pointers only as a comparison, as at the head of k_exh)
    const int args_null = (int)(coord == nullptr) | (int)(orders == nullptr) | (int)(poss == nullptr) | (int)(orders2 == nullptr) |
                          (int)(poss2 == nullptr) | (int)(states_next == nullptr) | (int)(rec_old == nullptr) | (int)(rec == nullptr);
    asm volatile("" : "+s"(done), "+s"(is_open), "+s"(parity), "+s"(pending), "+s"(mv_pa), "+s"(mv_pb) : "s"(n), "s"(args_null));
    exh_cand_pin(first);
    if (done) {   // a finished tour stays finished in both slots
        if (writer) states_next[tour] = *st;
        return;
    }
    const size_t base = (size_t)tour * n, pbase = (size_t)tour * (n + kExhPad);
    MoveView mv = move_view(parity, pending, mv_pa, mv_pb, orders + base, poss + base, orders2 + base, poss2 + base, n);
    const ExhRec *__restrict__ old = rec_old + pbase;   // (HOT only)
    const bool open = is_open != 0;   // (then nothing is pending: mv.L == 0)
    SweepDecision dec;
    ExhPair pr = {0, -1, -1};
    if (open) {
        // the pair by position; its ids only if two different pairs share the minimal delta (from the old records, or through order)
        pr = exh_decide(first, cand, cand_per_tour, [&](int p) { if constexpr (HOT) return old[p].id; else return mv.order[p]; }, s_d, s_k);
        if (!pr.found) {   // the local optimum: block 0 recomputes the cost (tabusearch.c:168-172), nobody has records to build
            if (blockIdx.x != 0) return;
            double cost;
            if constexpr (HOT) cost = exh_rec_cost(old, n, s_d);   // (order / pos may be stale: the records are the tour)
            else cost = tour_cost_block<WT, INT>(coord, mv.order, mv.pos, n, s_d, nullptr);
            if (writer) {
                TourState z = *st;
                sweep_count(z, dec, n, cost);
                z.pending = 0;
                states_next[tour] = z;
            }
            return;
        }
    }
    const int k = blockIdx.x * kScanThreads + threadIdx.x;
    if (k >= (HOT ? n + 1 : n + kExhPad)) return;   // (the pads never change: written once per buffer, k_exh_pads)
    int u;
    ExhRec r;
    if constexpr (HOT) {
        // The pair is known, its orientation is not: the position of the smaller id is pa.  Both orientations are evaluated and
        // everything either of them needs is asked for in ONE round -- old records a and b of both, old record n's eprev (the
        // closing edge), the ids at p and q -- so no thread, the two at the cut points included, waits a second time.  (A pending
        // move is oriented already: the same move twice.)
        ExhMove m1 = {mv_pa, mv_pb, mv.pa1, mv.L}, m2 = m1;
        if (open) { m1 = exh_orient(pr.p, pr.q, n, true); m2 = exh_orient(pr.p, pr.q, n, false); }
        const ExhPerm pm1 = exh_perm(k, n, m1.pa1, m1.L), pm2 = exh_perm(k, n, m2.pa1, m2.L);
        const ExhRec ra1 = old[pm1.a], rb1 = old[pm1.b], ra2 = old[pm2.a], rb2 = old[pm2.b];
        const int wrap = old[n].eprev;
        int idp = 0, idq = 1;
        if (open) { idp = old[pr.p].id; idq = old[pr.q].id; }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : : "v"(ra1.m2x), "v"(ra1.m2y), "v"(ra1.nrm), "v"(ra1.eprev), "v"(rb1.m2x), "v"(rb1.m2y), "v"(rb1.nrm),
                     "v"(rb1.eprev), "v"(rb1.id), "v"(wrap));
        asm volatile("" : : "v"(ra2.m2x), "v"(ra2.m2y), "v"(ra2.nrm), "v"(ra2.eprev), "v"(rb2.m2x), "v"(rb2.m2y), "v"(rb2.nrm),
                     "v"(rb2.eprev), "v"(rb2.id), "v"(idp), "v"(idq));
        const bool p_first = idp < idq;
        const ExhMove m = p_first ? m1 : m2;
        r = exh_perm_rec<exh_mode<WT>()>(p_first ? pm1 : pm2, p_first ? ra1 : ra2, p_first ? rb1 : rb2, wrap,
                                         [](double v) { return __builtin_amdgcn_sqrt(v); });
        u = r.id;
        mv.L = m.L; mv.pa1 = m.pa1;
        if (open) dec = exh_decision(m);
    } else {
        if (open) {   // the orientation by two dependent loads through order (nothing is pending: order is the tour as it stands)
            const ExhMove m = exh_orient(pr.p, pr.q, n, mv.order[pr.p] < mv.order[pr.q]);
            mv.L = m.L; mv.pa1 = m.pa1;
            dec = exh_decision(m);
        }
        // every load of the current copy (which this kernel never writes) comes before the first store
        u = k < n ? mv.node_at(k) : (k == n ? mv.node_at(0) : -1);
        const int v = k >= 1 && k <= n ? mv.node_at(k - 1) : -1;   // the position before
        const double2 c0 = coord[0];
        double2 cu = make_double2(c0.x - 6.0e6, c0.y - 6.0e6);   // pads: farther from every node than any tour edge is long
        int len = 0;
        if (u >= 0) cu = coord[u];
        if (v >= 0) { const double2 cv = coord[v]; len = (int)dist_xy<WT, INT>(cv.x, cv.y, cu.x, cu.y); }
        exh_rec_xy(cu.x - c0.x, cu.y - c0.y, r);   // exact: integers whose difference is below 2^21 (the pads: 6e6)
        r.eprev = len;
        r.id = u;
    }
    // A cold launch keeps order and pos current (it can only have a move to carry out when someone left one pending).  A hot
    // one leaves them alone, and parity with them: while the host's exh_hot holds, the records are the tour and nobody reads
    // order or pos; k_exh_settle brings them back from the records before anybody does.
    if constexpr (!HOT) {
        if (mv.L > 0 && k < n) {
            int *o_new = (parity ? orders : orders2) + base, *p_new = (parity ? poss : poss2) + base;
            o_new[k] = u;
            p_new[u] = k;
        }
    }
    rec[pbase + k] = r;
    if (writer) {   // the next control block: the sweep counted, the move carried out (the other copy is the current one now)
        // (the writer is thread 0 of block 0: k = 0, never past the early return above)
        TourState z = *st;
        if (open) sweep_count(z, dec, n, 0.0);
        if (!HOT && mv.L > 0) z.parity ^= 1;
        z.pending = 0;
        z.rec_buf = rec_mark;   // `rec` holds this tour's records from here on (a finished tour keeps the mark of its last ones)
        states_next[tour] = z;
    }
}

// Before the host looks at a control block (a poll, the end of a run): an open sweep becomes a decided one -- the counters, and
// either a pending move, which the next k_move_pos or the flush carries out, or the finished tour's recomputed cost.  One block
// per tour, so it updates the control block it reads (behind the barriers of the decision).  Ids, orientation and the finished
// tour's cost from the records the open sweep ran on (a sweep is only ever open behind its own pair of launches: `rec_all` is the
// buffer that pair wrote and read); order, pos and coord are not read.  Dependent loads: one launch in many.
template <int WT, bool INT>
__global__ __launch_bounds__(kScanThreads) void k_exh_close(const ExhRec *__restrict__ rec_all, TourState *states,
                                                            const ExhCand *__restrict__ cands, int cand_per_tour, int n) {
    static_assert(exh_metric<WT>() && INT, "integer-coordinate metrics only");
    __shared__ double s_d[kScanThreads / 64];
    __shared__ u64 s_k[kScanThreads / 64];
    const int tour = blockIdx.x;
    TourState *st = states + tour;
    if (st->done || !st->open) return;
    const ExhRec *__restrict__ rec = rec_all + (size_t)tour * (n + kExhPad);
    const ExhCand *cand = cands + (size_t)tour * cand_per_tour;
    const ExhPair pr = exh_decide(exh_cand_load(cand, cand_per_tour, threadIdx.x), cand, cand_per_tour,
                                  [&](int p) { return rec[p].id; }, s_d, s_k);
    SweepDecision dec;
    double cost = 0.0;
    if (pr.found) dec = exh_decision(exh_orient(pr.p, pr.q, n, rec[pr.p].id < rec[pr.q].id));
    else cost = exh_rec_cost(rec, n, s_d);
    if (threadIdx.x == 0) {
        TourState z = *st;
        sweep_count(z, dec, n, cost);
        z.pending = dec.found;
        *st = z;
    }
}

// RJ = kExhRJ columns per lane, four workgroups of four waves per CU (the host pins that with its LDS request).
// The order of the parameters: `states` (the read-only view: `done`), the records, n, the stride of the candidates, the table of
// the dealing, the candidates and the control block to set `open` in are 12 dwords, all within the 14 which a wave finds in its
// SGPRs when it starts (kernel-argument preload, csrc/Makefile: a struct by value ends the preload, so there is none), and the
// loads of `done` and of the descriptor are issued with no wait in front of them.
// The tail: the wave's candidate by position -- one wave_min over the lanes' best deltas, a ballot of the lanes that hold it;
// one owner, or owners that all hold the same pair: no id is loaded (owners with different pairs, rare, load theirs inside that
// branch) --, then the block's from its four waves' behind the kernel's one barrier, one 16-byte store.  Ties between blocks and
// the orientation of the move are k_move_pos's (exh_decide.hpp), which holds the records with the ids in them.
template <int WT, bool INT, int RJ>
__global__ __launch_bounds__(kScanThreads, 1) void k_exh(const TourState *__restrict__ states, const ExhRec *__restrict__ rec_all, int n,
                                                      int cand_per_tour, const ExhDeal *__restrict__ deal,
                                                      ExhCand *__restrict__ cand_all, TourState *states_w) {
    // the position arrays and the table of the dealing are kernel arguments of their own, restrict-qualified: the row operands
    // and a wave's descriptor are wave-uniform loads, and the compiler only issues them as scalar loads (s_load: no
    // vector-memory slot, no VGPRs) when it can prove that the kernel's own stores (the candidate slot, `open`) never touch them
    static_assert(exh_metric<WT>(), "integer-coordinate metrics only");
    constexpr int W = 64 * RJ, WEFF = W - 1;
#ifdef TSP_STAMPS
    const unsigned long long stamp_r0 = __builtin_amdgcn_s_memrealtime(), stamp_c0 = __builtin_amdgcn_s_memtime();
    unsigned long long stamp_hits = 0, stamp_hit_cycles = 0, stamp_first = 0;
#endif
    const int tour = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63;
    // ---- this wave's share (exh_deal, evaluated by the host when the handle was created) and the tour's `done`: every wave of
    // the launch is here at once and nothing hides the latency, so the two loads travel together -- one wait, then the branch
    const int gw = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (kScanThreads / 64) + (tid >> 6));
    int done = states[tour].done;
    ExhDeal dl = deal[gw];
    // (both loaded before the branch; and, on firmware that does not preload, every kernel argument fetched by the entry's one
    // batch of loads, not by a batch of their own behind the last row.  The array the kernel reads only as a comparison: handed to
    // the statement itself it would count as escaped, and the loads through it would no longer be scalar loads; the two
    // pointers it only stores through as they are.)
#ifdef TSP_STAMPS
    // (in the stamped build the compiler fetches `done` with a vector load: back to scalar registers for the statement below)
    done = __builtin_amdgcn_readfirstlane(done);
    dl.strip = __builtin_amdgcn_readfirstlane(dl.strip); dl.row = __builtin_amdgcn_readfirstlane(dl.row);
    dl.count = (long long)(((u64)(unsigned)__builtin_amdgcn_readfirstlane((int)((u64)dl.count >> 32)) << 32) |
                           (unsigned)__builtin_amdgcn_readfirstlane((int)(u64)dl.count));
#endif
    const int args_null = (int)(rec_all == nullptr);
    asm volatile("" : "+s"(done), "+s"(dl.strip), "+s"(dl.row), "+s"(dl.count)
                 : "s"(n), "s"(args_null), "s"(cand_per_tour), "s"(cand_all), "s"(states_w));
    if (done) return;
    const size_t pbase = (size_t)tour * (n + kExhPad);
    const ExhRec *__restrict__ rec = rec_all + pbase;

    int bd = -1, bp = -1, bq = -1;     // integer costs: delta < 0  <=>  delta <= -1; (bd, no pair) loses every tie
    int wbd = -1;                      // wave-uniform: the lowest delta any lane of this wave has seen

    // the reference's scan-order key of the pair at positions (pp, qq): its node ids, from the records
    auto id_key = [&](int pp, int qq) {
        const int i = rec[pp].id, j = rec[qq].id;
        return make_key(min(i, j), max(i, j));
    };
    // exact bookkeeping for a pair that reached the wave's best: delta, then -- on a tie only -- first the positions (the same
    // pair once more, from a range that runs from strip 0 into strip 1: skipped), then the reference's tie-break on node ids
    // (dependent global loads: not on the path of a strict improvement)
    auto consider = [&](int sum, int erow, int pp, int qq, bool valid) {
        const int d = sum - erow;
        if (valid && d <= bd) {
            bool take = d < bd || bp < 0;
            if (!take && (pp != bp || qq != bq)) take = id_key(pp, qq) < id_key(bp, bq);
            if (take) { bd = d; bp = pp; bq = qq; }
        }
    };

    // the walk: `count` units from row dl.row of strip dl.strip, on into the following strips (any number of them)
    const int strips = exh_strips(n, WEFF);
    int pa = dl.row;
    long long rem = dl.count;
    for (int s = dl.strip; rem > 0 && s < strips; ++s) {
        const ExhStrip strip = exh_strip(n, WEFF, s);
        // segment of strip s: pair-rows [pa, pb)
        const int pb = (int)min<long long>(strip.rows, pa + rem);
        rem -= pb - pa;
        const int Q0 = strip.q0;
        double cx[RJ], cy[RJ], cn[RJ];
        int nce[RJ], Dp[RJ], qk[RJ];   // nce[k] = -e[q_k - 1]: what the pair of column k removes on the column side
        // Every operand of the segment's start in flight together: the columns' whole records (vector loads), row pa's record
        // and the first batch of rows (scalar loads); the first use of any of them comes behind the barrier below, and the
        // empty statements keep every one of these loads here (left alone, the compiler fetches the columns' eprev first, waits,
        // and only then asks for the rest).
        // The row records are wave-uniform: scalar loads, kRowBatch rows per batch, and the NEXT batch is on its way
        // while this one is worked (a scalar load that misses the CU's constant cache takes longer than one row step: with a
        // prefetch distance of one row the waves spent a quarter of their cycles in s_waitcnt, SQ_WAIT_ANY).  Positions up to
        // n + 2 kRowBatch exist: k_move_pos pads.
        struct Rows { ExhRec r[kRowBatch]; };
        ExhRec col[RJ];
#pragma unroll
        for (int k = 0; k < RJ; ++k) {
            qk[k] = Q0 + RJ * lane + k;
            col[k] = rec[qk[k]];
        }
        const ExhRec rpa = rec[pa];
        int p = pa + 1;
        Rows nx = *reinterpret_cast<const Rows *>(rec + p);
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" : : "s"(rpa.m2x), "s"(rpa.m2y), "s"(rpa.nrm), "s"(rpa.eprev));
#pragma unroll
        for (int u = 0; u < kRowBatch; ++u) asm volatile("" : : "s"(nx.r[u].m2x), "s"(nx.r[u].m2y), "s"(nx.r[u].nrm), "s"(nx.r[u].eprev));
#pragma unroll
        for (int k = 0; k < RJ; ++k) asm volatile("" : : "v"(col[k].m2x), "v"(col[k].m2y), "v"(col[k].nrm), "v"(col[k].eprev));
#pragma unroll
        for (int k = 0; k < RJ; ++k) {
            cx[k] = exh_col(col[k].m2x); cy[k] = exh_col(col[k].m2y); cn[k] = col[k].nrm; nce[k] = -col[k].eprev;
        }
        // lane 0's first column has no left neighbour in this wave (the DPP hands it 0, and position 0 has no edge before it):
        // its pair belongs to the strip on the left; should D alone ever pass the test below, the bookkeeping drops it
        if (lane == 0) nce[0] = 0;
#pragma unroll
        for (int k = 0; k < RJ; ++k) asm("" : "+v"(nce[k]));   // kept negated: an addend of v_add3_u32, not a subtraction of its own
        {   // row pa: distances only
#pragma unroll
            for (int k = 0; k < RJ; ++k) Dp[k] = exh_dist<WT>(cx[k], cy[k], cn[k], rpa);
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
        const int p_plain = min(pb, Q0);
#ifdef TSP_STAMPS
        if (!stamp_first) stamp_first = wall_clock64();   // the first row step begins
#endif
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
        pa = 0;
    }

    // ---- the wave's candidate, then the block's: the arg-min of (delta, (i, j)) by position; the tour's is taken by the next launch
#ifdef TSP_STAMPS
    if (lane == 0 && tour == 0) {
        const int w = (int)blockIdx.x * (kScanThreads / 64) + (tid >> 6);
        if (w < 8192) { g_exh_f[w] = stamp_first; g_exh_w[4 * w] = stamp_r0; g_exh_w[4 * w + 1] = wall_clock64(); unsigned hwid, xcc;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
            g_exh_w[4 * w + 2] = (clock64() - stamp_c0) | ((unsigned long long)hwid << 32); g_exh_w[4 * w + 3] = 1 | (stamp_hits << 8) | ((unsigned long long)(xcc & 0xf) << 60) | ((stamp_hit_cycles & 0xfffffffffull) << 24); }
    }
#endif
    const int wmin = (int)(unsigned)(wave_min_u64((u64)((unsigned)bd ^ 0x80000000u)) ^ 0x80000000u);
    const bool owner = bp >= 0 && bd == wmin;
    const u64 owners = __ballot(owner);
    int cp = -1, cq = -1;
    if (owners) {
        const int first = __builtin_ctzll(owners);
        cp = __builtin_amdgcn_readlane(bp, first); cq = __builtin_amdgcn_readlane(bq, first);
        // owners with different pairs (rare): the reference's tie-break, the ids loaded and consumed inside this branch
        if (__builtin_expect(__any(owner && (bp != cp || bq != cq)), 0)) {
            u64 key = kNoKey;
            if (owner) key = id_key(bp, bq);
            const int src = __builtin_ctzll(__ballot(key == wave_min_u64(key)));
            cp = __builtin_amdgcn_readlane(bp, src); cq = __builtin_amdgcn_readlane(bq, src);
        }
    }
    // The block's candidate: its waves' candidates meet in LDS behind the kernel's one barrier and one thread folds them by
    // exh_decide.hpp's rule -- (delta, position key), and the ids of the pairs at the minimal delta only if two different pairs
    // share it (rare: loaded and consumed inside that branch).
    __shared__ int s_wd[kScanThreads / 64];
    __shared__ u64 s_wk[kScanThreads / 64];
    if (lane == 0) { s_wd[tid >> 6] = wmin; s_wk[tid >> 6] = exh_pair_key(cp, cq); }
    __syncthreads();
    // The launch ends here: the block's candidate, empty or not, as one plain 16-byte store -- its readers (every block of the
    // next k_move_pos, or k_exh_close) are later launches.  `open` tells them so; nothing in this launch reads it.
    if (tid == 0) {
        auto wave_cand = [&](int w) {
            ExhCand c;
            c.delta = s_wd[w]; c.p = s_wk[w] == kExhNoPair ? -1 : exh_key_hi(s_wk[w]); c.q = exh_key_lo(s_wk[w]); c.pad = 0;
            return c;
        };
        ExhBest b;
        for (int w = 0; w < kScanThreads / 64; ++w) exh_fold(b, wave_cand(w));
        if (__builtin_expect(b.tie, 0)) {
            ExhIdBest ib;
            for (int w = 0; w < kScanThreads / 64; ++w) exh_fold_ids(ib, wave_cand(w), b.delta, [&](int p) { return rec[p].id; });
            b.key = ib.poskey;
        }
        ExhCand c;
        c.delta = b.delta; c.p = b.key == kExhNoPair ? -1 : exh_key_hi(b.key); c.q = exh_key_lo(b.key); c.pad = 0;
        cand_all[(size_t)tour * (size_t)cand_per_tour + blockIdx.x] = c;
        if (blockIdx.x == 0) states_w[tour].open = 1;
#ifdef TSP_STAMPS
        atomicMax(&g_exh_t[4], wall_clock64());
#endif
    }
}

}  // namespace tsp
