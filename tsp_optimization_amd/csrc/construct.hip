// construct.hip -- greedy() / grasp() (src/heuristics.c:18-156) for B starting nodes at once, and the
// n x n distance matrix build.
//
// Construction: one workgroup per start.  Each of the n steps is a block-wide arg-min of
// calc_dist(cur, k) over the unvisited k, lowest index winning ties (the reference's strict '<'
// scan in index order, :51 / :117).  GRASP's runner-up is "the running minimum just before the
// final one" (:117-122), i.e. the arg-min over unvisited k < best -- a second, shorter arg-min that
// is only needed on the ~10 % of steps whose draw is >= GRASP_RAND (:127-128).
#include "tsp_internal.hpp"
#include "two_opt_common.hpp"
#include <algorithm>   // wave_min_u64

#include <cfloat>

#pragma clang fp contract(off)

namespace tsp {

constexpr int kConsThreads = 1024;
constexpr double kGraspPickBest = 0.9;  // src/heuristics.c:10

struct ArgMin {
    double d;
    int k;
};

__device__ __forceinline__ bool lt(const ArgMin &a, const ArgMin &b) { return a.d < b.d || (a.d == b.d && a.k < b.k); }

// block-wide (d, k) lexicographic minimum; k == INT_MAX means "none"
__device__ __forceinline__ ArgMin wave_argmin_dk(ArgMin v);
__device__ __forceinline__ ArgMin block_argmin(ArgMin v, double *s_d, int *s_k) {
    v = wave_argmin_dk(v);
    const int tid = threadIdx.x;
    __syncthreads();
    if ((tid & 63) == 0) { s_d[tid >> 6] = v.d; s_k[tid >> 6] = v.k; }
    __syncthreads();
    ArgMin r;
    r.d = s_d[0]; r.k = s_k[0];
    for (int w = 1; w < kConsThreads / 64; ++w) {
        ArgMin o;
        o.d = s_d[w]; o.k = s_k[w];
        if (lt(o, r)) r = o;
    }
    return r;
}

template <int WT, bool INT, bool IS_GRASP>
__global__ __launch_bounds__(kConsThreads) void k_construct(const double2 *__restrict__ coord, int n,
                                                           const int *__restrict__ starts,
                                                           const double *__restrict__ urand,
                                                           unsigned char *__restrict__ visited_all,
                                                           int *__restrict__ succ_all, double *__restrict__ obj,
                                                           int *__restrict__ status) {
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int start = starts[b];
    if (start < 0 || start >= n) {  // heuristics.c:20 / :84 (negative starts would index out of bounds there)
        if (tid == 0) { status[b] = TSP_WRONG_STARTING_NODE; obj[b] = 0.0; }
        return;
    }
    unsigned char *visited = visited_all + (size_t)b * n;
    int *succ = succ_all + (size_t)b * n;
    const double *u = IS_GRASP ? urand + (size_t)b * n : nullptr;
    __shared__ double s_d[kConsThreads / 64];
    __shared__ int s_k[kConsThreads / 64];

    for (int k = tid; k < n; k += kConsThreads) visited[k] = (k == start) ? 1 : 0;
    __syncthreads();

    double total = 0.0;
    int cur = start;
    for (int step = 0;; ++step) {
        const double2 c = coord[cur];
        ArgMin mine;
        mine.d = DBL_MAX; mine.k = 0x7fffffff;
        for (int k = tid; k < n; k += kConsThreads) {
            if (k == cur || visited[k]) continue;
            const double2 o = coord[k];
            const double d = dist_xy<WT, INT>(c.x, c.y, o.x, o.y);
            if (d < mine.d) { mine.d = d; mine.k = k; }
        }
        const ArgMin best = block_argmin(mine, s_d, s_k);
        int pick = best.k == 0x7fffffff ? -1 : best.k;
        double pick_d = best.d;
        if constexpr (IS_GRASP) {
            const double draw = u[step];
            if (!(draw < kGraspPickBest) && pick >= 0) {
                ArgMin m2;
                m2.d = DBL_MAX; m2.k = 0x7fffffff;
                for (int k = tid; k < pick; k += kConsThreads) {
                    if (k == cur || visited[k]) continue;
                    const double2 o = coord[k];
                    const double d = dist_xy<WT, INT>(c.x, c.y, o.x, o.y);
                    if (d < m2.d) { m2.d = d; m2.k = k; }
                }
                const ArgMin runner = block_argmin(m2, s_d, s_k);
                if (runner.k != 0x7fffffff) { pick = runner.k; pick_d = runner.d; }
            }
        }
        if (pick < 0) {  // every node visited: close the cycle
            if (tid == 0) succ[cur] = start;
            if constexpr (IS_GRASP) {  // heuristics.c:135
                const double2 s0 = coord[start];
                total += dist_xy<WT, INT>(c.x, c.y, s0.x, s0.y);
            }
            break;
        }
        if (tid == 0) { succ[cur] = pick; visited[pick] = 1; }
        total += pick_d;
        cur = pick;
        __syncthreads();  // visited[pick] before the next scan
    }
    {   // heuristics.c:74 / :152
        const double2 c = coord[cur], s0 = coord[start];
        total += dist_xy<WT, INT>(c.x, c.y, s0.x, s0.y);
    }
    if (tid == 0) { obj[b] = total; status[b] = TSP_OK; }
}

// LDS-resident variant (n <= 16384, 16 n bytes of LDS): four waves, one per SIMD, so the per-step
// reduction work is not multiplied by sixteen co-resident waves fighting for the same issue slots (that,
// not memory, bounds k_construct: ~2.5 us per step at any n).  Thread t owns the candidates t + 256 m and
// keeps their "unvisited" flags in a 64-bit mask; coordinates sit in LDS.  One barrier per arg-min: each
// wave reduces (d, k) with shuffles, the lane holding the wave's winner writes (d, k, x, y) into the wave's
// slot of a rotating LDS table, and after the barrier every thread scans the four slots, so the picked
// node's coordinates arrive with the result.  Same arg-min and tie-break as k_construct.
constexpr int kConsLdsThreads = 256;
constexpr int kConsLdsMaxN = 64 * kConsLdsThreads;
struct alignas(16) ConsSlot { double d, x, y; int k; int pad; };

// (d, k) minimum of the wave in every lane: distances are >= 0 (or DBL_MAX), so they order like their bits
__device__ __forceinline__ ArgMin wave_argmin_dk(ArgMin v) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v.d);
    const unsigned long long md = wave_min_u64(bits);
    const unsigned long long mk = wave_min_u64(bits == md ? (unsigned long long)(unsigned)v.k : ~0ull);
    ArgMin r;
    r.d = __longlong_as_double((long long)md); r.k = (int)(unsigned)mk;
    return r;
}

__device__ __forceinline__ ConsSlot cons_argmin(ArgMin mine, double mx, double my, ConsSlot *table) {
    const ArgMin w = wave_argmin_dk(mine);
    const int tid = threadIdx.x;
    if (mine.k == w.k && (w.k != 0x7fffffff || (tid & 63) == 0)) {  // the winner's lane (lane 0 if the wave has none)
        ConsSlot sl;
        sl.d = w.d; sl.k = w.k; sl.x = mx; sl.y = my; sl.pad = 0;
        table[tid >> 6] = sl;
    }
    __syncthreads();
    ConsSlot r = table[0];
#pragma unroll
    for (int q = 1; q < kConsLdsThreads / 64; ++q) {
        const ConsSlot o = table[q];
        if (o.d < r.d || (o.d == r.d && o.k < r.k)) r = o;
    }
    return r;
}

template <int WT, bool INT, bool IS_GRASP>
__global__ __launch_bounds__(kConsLdsThreads) void k_construct_lds(const double2 *__restrict__ coord, int n,
                                                                  const int *__restrict__ starts,
                                                                  const double *__restrict__ urand,
                                                                  int *__restrict__ succ_all, double *__restrict__ obj,
                                                                  int *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char cons_smem[];
    ConsSlot *s_tab = reinterpret_cast<ConsSlot *>(cons_smem);                          // 4 tables x 4 slots
    double2 *s_xy = reinterpret_cast<double2 *>(cons_smem + 4 * (kConsLdsThreads / 64) * sizeof(ConsSlot));
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int start = starts[b];
    if (start < 0 || start >= n) {
        if (tid == 0) { status[b] = TSP_WRONG_STARTING_NODE; obj[b] = 0.0; }
        return;
    }
    int *succ = succ_all + (size_t)b * n;
    const double *u = IS_GRASP ? urand + (size_t)b * n : nullptr;
    const int M = (n + kConsLdsThreads - 1) / kConsLdsThreads;

    unsigned long long alive = 0;
    for (int m = 0; m < M; ++m) {
        const int k = tid + m * kConsLdsThreads;
        if (k < n) { s_xy[k] = coord[k]; if (k != start) alive |= 1ull << m; }
    }
    const double2 c_start = coord[start];
    double curx = c_start.x, cury = c_start.y;
    __syncthreads();

    double total = 0.0;
    int cur = start, rot = 0;
    for (int step = 0;; ++step) {
        ArgMin mine;
        mine.d = DBL_MAX; mine.k = 0x7fffffff;
        double mx = 0.0, my = 0.0;
        // candidates four at a time: the LDS reads and the four distance chains overlap (one wave per SIMD
        // has no other wave to hide latency behind); groups whose four candidates are all visited are skipped
        for (int g = 0; g < M; g += 4) {
            const unsigned nib = (unsigned)(alive >> g) & 0xFu;
            if (!nib) continue;
            double2 c[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) c[q] = s_xy[min(tid + (g + q) * kConsLdsThreads, n - 1)];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const double d = dist_xy<WT, INT>(curx, cury, c[q].x, c[q].y);
                if (((nib >> q) & 1u) && d < mine.d) {   // g, q ascend: the lowest index wins ties
                    mine.d = d; mine.k = tid + (g + q) * kConsLdsThreads; mx = c[q].x; my = c[q].y;
                }
            }
        }
        ConsSlot best = cons_argmin(mine, mx, my, s_tab + rot * (kConsLdsThreads / 64));
        rot = (rot + 1) & 3;
        if constexpr (IS_GRASP) {
            const double draw = u[step];
            if (!(draw < kGraspPickBest) && best.k != 0x7fffffff) {
                ArgMin m2;
                m2.d = DBL_MAX; m2.k = 0x7fffffff;
                double m2x = 0.0, m2y = 0.0;
                for (int g = 0; g < M && tid + g * kConsLdsThreads < best.k; g += 4) {
                    const unsigned nib = (unsigned)(alive >> g) & 0xFu;
                    if (!nib) continue;
                    double2 c[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) c[q] = s_xy[min(tid + (g + q) * kConsLdsThreads, n - 1)];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int k = tid + (g + q) * kConsLdsThreads;
                        const double d = dist_xy<WT, INT>(curx, cury, c[q].x, c[q].y);
                        if (((nib >> q) & 1u) && k < best.k && d < m2.d) { m2.d = d; m2.k = k; m2x = c[q].x; m2y = c[q].y; }
                    }
                }
                const ConsSlot runner = cons_argmin(m2, m2x, m2y, s_tab + rot * (kConsLdsThreads / 64));
                rot = (rot + 1) & 3;
                if (runner.k != 0x7fffffff) best = runner;
            }
        }
        if (best.k == 0x7fffffff) {  // every node visited: close the cycle
            if (tid == 0) succ[cur] = start;
            if constexpr (IS_GRASP) total += dist_xy<WT, INT>(curx, cury, c_start.x, c_start.y);  // heuristics.c:135
            total += dist_xy<WT, INT>(curx, cury, c_start.x, c_start.y);                           // :74 / :152
            break;
        }
        const int pick = best.k;
        if ((pick & (kConsLdsThreads - 1)) == tid) {   // the owner retires the node and records the edge
            alive &= ~(1ull << (pick / kConsLdsThreads));
            succ[cur] = pick;
        }
        total += best.d;
        cur = pick; curx = best.x; cury = best.y;
    }
    if (tid == 0) { obj[b] = total; status[b] = TSP_OK; }
}

// ---- k_construct_nn: nearest neighbour over the Hilbert groups ---------------------------------------------------
// greedy() asks n times for the nearest unvisited node (lowest index among equals, heuristics.c:51).  With the
// nodes ranked along a Hilbert curve (tsp_dev_inst_create: 64 consecutive ranks = one group with a bounding box)
// that is a spatial query: find the unvisited group whose box is nearest, evaluate its 64 nodes, then only the
// groups whose box is not provably farther than the best distance found.  One wave per start and nothing but
// wave-level reductions: no block barrier in the n-step chain (the 256-thread kernel above spends a step's 4 us
// at n = 10 000 on 40 candidates per thread and a barrier).  Coordinates (relative to the instance's corner, as
// floats when they are bounded integers: exact), node ids, the groups' alive masks and boxes live in LDS.
constexpr int kNnMaxRounds = 4;   // groups per lane: up to 256 groups = 16 384 ranks



template <typename CT>
__host__ __device__ inline size_t nn_lds_bytes(int n_slots, int ng) {
    return sizeof(CT) * (size_t)n_slots + sizeof(int) * (size_t)n_slots + (sizeof(unsigned long long) + sizeof(double4)) * (size_t)ng + 64;
}

template <int WT, bool INT, typename CT, bool PACK, bool IS_GRASP>
__global__ __launch_bounds__(64) void k_construct_nn(const double2 *__restrict__ coord, const int *__restrict__ sperm,
                                                     const double4 *__restrict__ gbox, int n, int ng, int n_slots,
                                                     double ox, double oy, const int *__restrict__ starts,
                                                     const int *__restrict__ start_slots, const double *__restrict__ urand,
                                                     int *__restrict__ succ_all, double *__restrict__ obj,
                                                     int *__restrict__ status) {
    constexpr bool ATT10 = WT == WT_ATT || WT == WT_ATT_ICOORD;
    // a distance is at least the root minus 1/2 when it is rounded to nearest (EUC_2D integer costs), at least the
    // root otherwise: a group whose box is farther than best + slack cannot hold a node as near as the best
    constexpr double kRound = (INT && (WT == WT_EUC_2D || WT == WT_EUC_2D_ICOORD)) ? 0.5 : 0.0;
    extern __shared__ __attribute__((aligned(16))) char nn_smem[];
    double4 *s_box = reinterpret_cast<double4 *>(nn_smem);
    unsigned long long *s_alive = reinterpret_cast<unsigned long long *>(s_box + ng);
    CT *s_xy = reinterpret_cast<CT *>(s_alive + ng);
    int *s_id = reinterpret_cast<int *>(s_xy + n_slots);
    const int b = blockIdx.x, lane = threadIdx.x;
    const int start = starts[b];
    if (start < 0 || start >= n) {
        if (lane == 0) { status[b] = TSP_WRONG_STARTING_NODE; obj[b] = 0.0; }
        return;
    }
    int *succ = succ_all + (size_t)b * n;
    for (int g = 0; g < ng; ++g) {
        const int k = g * 64 + lane;
        const int v = sperm[k];
        const double2 c = coord[max(v, 0)];
        CT q;
        q.x = (decltype(q.x))(c.x - ox); q.y = (decltype(q.y))(c.y - oy);
        s_xy[k] = q;
        s_id[k] = v;
        const unsigned long long m = __ballot(v >= 0);
        if (lane == 0) s_alive[g] = m;
    }
    for (int g = lane; g < ng; g += 64) {
        double4 bx = gbox[g];
        bx.x -= ox; bx.y -= ox; bx.z -= oy; bx.w -= oy;
        s_box[g] = bx;
    }
    __syncthreads();   // one wave: orders the LDS writes above against the reads below
    int cur_slot = start_slots[b], cur_id = start;
    if (lane == 0) s_alive[cur_slot >> 6] &= ~(1ull << (cur_slot & 63));
    __syncthreads();
    double curx = (double)s_xy[cur_slot].x, cury = (double)s_xy[cur_slot].y;
    const double sx = curx, sy = cury;
    double total = 0.0;

    for (int step = 1; step < n; ++step) {
        // A: the unvisited group whose box is nearest
        double lb2[kNnMaxRounds];
        double near2 = DBL_MAX;
        int near_g = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < kNnMaxRounds; ++r) {
            const int g = lane + 64 * r;
            lb2[r] = DBL_MAX;
            if (g < ng && s_alive[g] != 0ull) {
                const double4 bx = s_box[g];
                const double gx = fmax(0.0, fmax(bx.x - curx, curx - bx.y)), gy = fmax(0.0, fmax(bx.z - cury, cury - bx.w));
                lb2[r] = gx * gx + gy * gy;
                if (lb2[r] < near2) { near2 = lb2[r]; near_g = g; }
            }
        }
        if constexpr (PACK) {
            const unsigned long long nb = wave_min_u64((unsigned long long)__double_as_longlong(near2));
            near_g = __builtin_amdgcn_readlane(near_g, __builtin_ctzll(__ballot((unsigned long long)__double_as_longlong(near2) == nb)));
        } else {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const double o2 = __shfl_xor(near2, off);
                const int og = __shfl_xor(near_g, off);
                if (o2 < near2 || (o2 == near2 && og < near_g)) { near2 = o2; near_g = og; }
            }
        }
        // One query: the nearest live node with id < id_limit, (distance, id) smallest first == the reference's scan
        // with its strict '<'.  B: the nearest group's nodes; C: every other group that could hold a node as near
        // (ties included: the lower id wins) -- every live group if B found nothing.
        auto query = [&](int id_limit, double &qd, int &qid, int &qslot) -> bool {
            double bd = DBL_MAX;
            int bid = 0x7fffffff, bslot = -1;
            unsigned long long best = ~0ull;   // PACK: (distance << 30 | id << 15 | slot), integer costs below 2^31
            auto eval_group = [&](int g) {
                const int slot = g * 64 + lane;
                const int id = s_id[slot];
                const bool bit = ((s_alive[g] >> lane) & 1ull) && id < id_limit;
                const CT c = s_xy[slot];
                const double d = dist_xy<WT, INT>(curx, cury, (double)c.x, (double)c.y);
                if constexpr (PACK) {
                    const unsigned long long k = ((unsigned long long)(long long)d << 30) | ((unsigned long long)id << 15) | (unsigned)slot;
                    if (bit && k < best) best = k;
                } else {
                    if (bit && (d < bd || (d == bd && id < bid))) { bd = d; bid = id; bslot = slot; }
                }
            };
            auto reduce_best = [&]() {
                if constexpr (PACK) {
                    best = wave_min_u64(best);
                    bd = best == ~0ull ? DBL_MAX : (double)(best >> 30);
                    bid = (int)((best >> 15) & 0x7fff); bslot = (int)(best & 0x7fff);
                } else {
                    const unsigned long long md = wave_min_u64((unsigned long long)__double_as_longlong(bd));
                    const unsigned long long mi = wave_min_u64((unsigned long long)__double_as_longlong(bd) == md ? (unsigned long long)(unsigned)bid : ~0ull);
                    const int src = __builtin_ctzll(__ballot((unsigned long long)__double_as_longlong(bd) == md && (unsigned long long)(unsigned)bid == mi));
                    bd = __longlong_as_double((long long)md); bid = (int)(unsigned)mi; bslot = __builtin_amdgcn_readlane(bslot, src);
                }
            };
            eval_group(near_g);
            reduce_best();
            double thr2 = DBL_MAX;
            if (bd < DBL_MAX) { const double reach = bd + kRound; thr2 = (ATT10 ? 10.0 : 1.0) * reach * reach * (1.0 + 1e-9) + 1e-9; }
#pragma unroll
            for (int r = 0; r < kNnMaxRounds; ++r) {
                const int g = lane + 64 * r;
                unsigned long long cand = __ballot(g != near_g && lb2[r] < DBL_MAX && lb2[r] <= thr2);
                while (cand) {
                    const int bit = __builtin_ctzll(cand);
                    cand &= cand - 1;
                    eval_group(bit + 64 * r);
                }
            }
            reduce_best();
            qd = bd; qid = bid; qslot = bslot;
            return bd < DBL_MAX;
        };
        double bd;
        int bid, bslot;
        (void)query(0x7fffffff, bd, bid, bslot);   // a live node exists: step < n
        if constexpr (IS_GRASP) {
            // grasp(), heuristics.c:117-131: with probability 0.1 the "previous running minimum" of the scan, i.e.
            // the nearest node among those with a smaller index than the winner, if there is one
            const double draw = urand[(size_t)b * n + (step - 1)];
            if (!(draw < kGraspPickBest)) {
                double rd; int rid, rslot;
                if (query(bid, rd, rid, rslot)) { bd = rd; bid = rid; bslot = rslot; }
            }
        }
        // the edge, and the node leaves the candidate set
        if (lane == 0) {
            succ[cur_id] = bid;
            s_alive[bslot >> 6] &= ~(1ull << (bslot & 63));
        }
        total += bd;
        cur_id = bid; cur_slot = bslot;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        curx = (double)s_xy[cur_slot].x; cury = (double)s_xy[cur_slot].y;
    }
    if (lane == 0) {
        succ[cur_id] = start;                                   // heuristics.c:60-61
        if constexpr (IS_GRASP) total += dist_xy<WT, INT>(curx, cury, sx, sy);   // :135, counted twice by grasp()
        total += dist_xy<WT, INT>(curx, cury, sx, sy);          // :74 / :152
        obj[b] = total; status[b] = TSP_OK;
    }
}

// ---- k_construct_nn_big: the same queries for instances that do not fit in LDS (up to 262 144 nodes) ----------
// Coordinates and ids in rank order stay in HBM/L2 (static per instance); LDS holds what changes or is read every
// step: the groups' alive masks and their boxes as floats rounded outward.  One more level keeps a step short:
// 64 groups form a supergroup (one per lane, box and live-node count in registers), a query looks at the nearest
// live supergroup's groups first and afterwards only at supergroups, then groups, within reach of the best found.
template <typename CT>
__global__ void k_sorted_xy(const double2 *__restrict__ coord, const int *__restrict__ sperm, CT *__restrict__ sxy,
                            int n_slots, double ox, double oy) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_slots) return;
    const int v = sperm[k];
    const double2 c = coord[max(v, 0)];
    CT q;
    q.x = (decltype(q.x))(c.x - ox); q.y = (decltype(q.y))(c.y - oy);
    sxy[k] = q;
}

template <int WT, bool INT, typename CT, bool PACK>
__global__ __launch_bounds__(64) void k_construct_nn_big(const CT *__restrict__ sxy, const int *__restrict__ sperm,
                                                         const double4 *__restrict__ gbox, int n, int ng, double ox, double oy,
                                                         const int *__restrict__ starts, const int *__restrict__ start_slots,
                                                         int *__restrict__ succ_all, double *__restrict__ obj,
                                                         int *__restrict__ status) {
    constexpr bool ATT10 = WT == WT_ATT || WT == WT_ATT_ICOORD;
    constexpr double kRound = (INT && (WT == WT_EUC_2D || WT == WT_EUC_2D_ICOORD)) ? 0.5 : 0.0;
    extern __shared__ __attribute__((aligned(16))) char nn_smem[];
    float4 *s_box = reinterpret_cast<float4 *>(nn_smem);                       // {min x, max x, min y, max y}, outward
    unsigned long long *s_alive = reinterpret_cast<unsigned long long *>(s_box + ng);
    const int b = blockIdx.x, lane = threadIdx.x;
    const int start = starts[b];
    if (start < 0 || start >= n) {
        if (lane == 0) { status[b] = TSP_WRONG_STARTING_NODE; obj[b] = 0.0; }
        return;
    }
    int *succ = succ_all + (size_t)b * n;
    const int nsg = (ng + 63) / 64;   // <= 64: one supergroup per lane
    for (int g = lane; g < ng; g += 64) {
        const double4 bx = gbox[g];
        s_box[g] = make_float4(__double2float_rd(bx.x - ox), __double2float_ru(bx.y - ox), __double2float_rd(bx.z - oy),
                               __double2float_ru(bx.w - oy));
    }
    for (int g = 0; g < ng; ++g) {
        const unsigned long long m = __ballot(sperm[g * 64 + lane] >= 0);
        if (lane == 0) s_alive[g] = m;
    }
    __syncthreads();
    // the lane's supergroup: box and number of live nodes
    float sb0 = 3.0e38f, sb1 = -3.0e38f, sb2 = 3.0e38f, sb3 = -3.0e38f;
    int live = 0;
    if (lane < nsg) {
        for (int g = lane * 64; g < min(ng, lane * 64 + 64); ++g) {
            const float4 bx = s_box[g];
            sb0 = fminf(sb0, bx.x); sb1 = fmaxf(sb1, bx.y); sb2 = fminf(sb2, bx.z); sb3 = fmaxf(sb3, bx.w);
            live += __popcll(s_alive[g]);
        }
    }
    int cur_slot = start_slots[b], cur_id = start;
    if (lane == 0) s_alive[cur_slot >> 6] &= ~(1ull << (cur_slot & 63));
    if (lane == (cur_slot >> 12)) live -= 1;
    __syncthreads();
    double curx = (double)sxy[cur_slot].x, cury = (double)sxy[cur_slot].y;
    const double sx = curx, sy = cury;
    double total = 0.0;

    auto box_lb2 = [&](float m0, float m1, float m2, float m3) {
        const double gx = fmax(0.0, fmax((double)m0 - curx, curx - (double)m1)), gy = fmax(0.0, fmax((double)m2 - cury, cury - (double)m3));
        return gx * gx + gy * gy;
    };
    for (int step = 1; step < n; ++step) {
        // A: nearest live supergroup, then its nearest live group
        const double slb2 = (lane < nsg && live > 0) ? box_lb2(sb0, sb1, sb2, sb3) : DBL_MAX;
        const u64 smin = wave_min_u64((u64)__double_as_longlong(slb2));
        const int S0 = __builtin_ctzll(__ballot((u64)__double_as_longlong(slb2) == smin));
        double glb2 = DBL_MAX;
        {
            const int g = S0 * 64 + lane;
            if (g < ng && s_alive[g] != 0ull) { const float4 bx = s_box[g]; glb2 = box_lb2(bx.x, bx.y, bx.z, bx.w); }
        }
        const u64 gmin = wave_min_u64((u64)__double_as_longlong(glb2));
        const int g0 = S0 * 64 + __builtin_ctzll(__ballot((u64)__double_as_longlong(glb2) == gmin));
        // B / C: (distance, id) smallest first == the reference's scan with its strict '<'
        double bd = DBL_MAX;
        int bid = 0x7fffffff, bslot = -1;
        u64 best = ~0ull;
        auto eval_group = [&](int g) {
            const int slot = g * 64 + lane;
            const bool bit = (s_alive[g] >> lane) & 1ull;
            const CT c = sxy[slot];
            const int id = sperm[slot];
            const double d = dist_xy<WT, INT>(curx, cury, (double)c.x, (double)c.y);
            if constexpr (PACK) {
                const u64 k = ((u64)(long long)d << 36) | ((u64)(unsigned)id << 18) | (unsigned)slot;
                if (bit && k < best) best = k;
            } else {
                if (bit && (d < bd || (d == bd && id < bid))) { bd = d; bid = id; bslot = slot; }
            }
        };
        auto reduce_best = [&]() {
            if constexpr (PACK) {
                const u64 w = wave_min_u64(best);
                bd = (double)(w >> 36); bid = (int)((w >> 18) & 0x3ffff); bslot = (int)(w & 0x3ffff);
            } else {
                const u64 md = wave_min_u64((u64)__double_as_longlong(bd));
                const u64 mi = wave_min_u64((u64)__double_as_longlong(bd) == md ? (u64)(unsigned)bid : ~0ull);
                const int src = __builtin_ctzll(__ballot((u64)__double_as_longlong(bd) == md && (u64)(unsigned)bid == mi));
                bd = __longlong_as_double((long long)md); bid = (int)(unsigned)mi; bslot = __builtin_amdgcn_readlane(bslot, src);
            }
        };
        eval_group(g0);
        reduce_best();
        const double reach = bd + kRound;
        const double thr2 = (ATT10 ? 10.0 : 1.0) * reach * reach * (1.0 + 1e-9) + 1e-9;
        u64 scand = __ballot(slb2 <= thr2);
        while (scand) {
            const int S = __builtin_ctzll(scand);
            scand &= scand - 1;
            const int g = S * 64 + lane;
            bool in = false;
            if (g < ng && g != g0 && s_alive[g] != 0ull) { const float4 bx = s_box[g]; in = box_lb2(bx.x, bx.y, bx.z, bx.w) <= thr2; }
            u64 cand = __ballot(in);
            while (cand) {
                const int bit = __builtin_ctzll(cand);
                cand &= cand - 1;
                eval_group(S * 64 + bit);
            }
        }
        reduce_best();
        if (lane == 0) {
            succ[cur_id] = bid;
            s_alive[bslot >> 6] &= ~(1ull << (bslot & 63));
        }
        if (lane == (bslot >> 12)) live -= 1;
        total += bd;
        cur_id = bid; cur_slot = bslot;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const CT cc = sxy[cur_slot];
        curx = (double)cc.x; cury = (double)cc.y;
    }
    if (lane == 0) {
        succ[cur_id] = start;                                   // heuristics.c:60-61
        total += dist_xy<WT, INT>(curx, cury, sx, sy);          // :74
        obj[b] = total; status[b] = TSP_OK;
    }
}

// ---- distance matrix ------------------------------------------------------------------------
// Block = kDmRows rows x 1024 columns.  Each lane keeps the coordinates of its 4 consecutive
// columns in registers for all rows of the block, computes 4 entries per row and streams them out
// with one 16-byte (int32) or two 16-byte (double) non-temporal stores: a wave writes 1 KiB / 2 KiB
// contiguous per row.  The row's coordinates are wave-uniform (scalar loads).  Write-bandwidth
// bound: 4 n^2 (int32) or 8 n^2 (double) bytes to HBM against 16 n bytes of coordinates.
// rows per block: few -- measured on MI355X at n = 10 000 (400 / 800 MB written): int32 16 rows 4.9, 8 rows 5.5, 4 rows 5.8-6.2,
// 2 rows 5.7, 1 row 3.6 TB/s; double 16 rows 5.2, 4 rows 5.5, 1 row 6.2 TB/s.  More, shorter blocks keep more rows' segments in
// flight next to each other; below that the per-block column loads stop being amortised.
template <typename OUT> constexpr int dm_rows() { return sizeof(OUT) == 4 ? 4 : 1; }

template <int WT, bool INT, typename OUT>
__global__ __launch_bounds__(256) void k_dist_matrix(const double2 *__restrict__ coord, int n, OUT *__restrict__ out) {
    constexpr bool I32 = sizeof(OUT) == 4;
    constexpr int kDmRows = dm_rows<OUT>();
    const int i0 = blockIdx.y * kDmRows;
    const int base = blockIdx.x * 1024;
    if (base >= n) return;
    // int32: lane owns 4 consecutive columns (one 16-byte store).  double: lane owns two column
    // pairs 512 apart (two 16-byte stores), so that every store instruction of a wave is 1 KiB contiguous.
    int col[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        col[k] = I32 ? base + threadIdx.x * 4 + k : base + threadIdx.x * 2 + (k & 1) + (k >> 1) * 512;
    double2 cj[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cj[k] = coord[min(col[k], n - 1)];
    const int i1 = min(i0 + kDmRows, n);
    for (int i = i0; i < i1; ++i) {
        const double2 ci = coord[i];
        OUT v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double d = (col[k] == i) ? 0.0 : dist_xy<WT, INT>(ci.x, ci.y, cj[k].x, cj[k].y);
            v[k] = (OUT)d;
        }
        OUT *row = out + (size_t)i * n;
        if constexpr (I32) {
            if (col[3] < n && (((size_t)i * n + col[0]) * 4) % 16 == 0) {
                typedef int v4i __attribute__((ext_vector_type(4)));
                v4i pk = {(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
                __builtin_nontemporal_store(pk, reinterpret_cast<v4i *>(row + col[0]));
            } else {
                for (int k = 0; k < 4; ++k) if (col[k] < n) row[col[k]] = v[k];
            }
        } else {
            typedef double v2d __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                if (col[2 * h + 1] < n && (((size_t)i * n + col[2 * h]) * 8) % 16 == 0) {
                    v2d a = {(double)v[2 * h], (double)v[2 * h + 1]};
                    __builtin_nontemporal_store(a, reinterpret_cast<v2d *>(row + col[2 * h]));
                } else {
                    for (int k = 2 * h; k < 2 * h + 2; ++k) if (col[k] < n) row[col[k]] = v[k];
                }
            }
        }
    }
}

// ---- which kernel a construction runs ------------------------------------------------------------------------------
// Decided in one place, for tsp_dev_construct and for tsp_dev_construct_describe (tests assert the path they mean to cover).
enum ConsPath { CONS_NN, CONS_NN_BIG, CONS_LDS, CONS_GLOBAL };
struct ConstructPlan {
    ConsPath path;
    bool float_xy;      // spatial kernels: float2 coordinates relative to the instance's corner (bounded integers), else double2
    bool pack;          // spatial kernels: one 64-bit (distance, id, slot) key per candidate
    size_t lds_bytes;   // dynamic LDS of the launch (0 for k_construct)
};

static ConstructPlan construct_plan(const tsp_dev_inst *inst, int kind) {
    ConstructPlan p;
    // greedy on a sqrt metric with the Hilbert groups at hand: the spatial kernel, one wave per start
    const bool nn_off = TSP_SW(inst, CONSTRUCT_NN, 1) == 0;
    const bool icoord = inst->wtype == WT_EUC_2D_ICOORD || inst->wtype == WT_CEIL_2D_ICOORD || inst->wtype == WT_ATT_ICOORD;
    const size_t need = icoord ? nn_lds_bytes<float2>(inst->n_slots, inst->ng) : nn_lds_bytes<double2>(inst->n_slots, inst->ng);
    const bool small = inst->ng <= 64 * kNnMaxRounds && need <= (size_t)158 * 1024;
    // larger instances: coordinates stay in HBM/L2, LDS holds the alive masks and float boxes (k_construct_nn_big)
    const size_t need_big = (sizeof(float4) + sizeof(unsigned long long)) * (size_t)inst->ng + 64;
    const bool big = !small && inst->ng <= 4096 && need_big <= (size_t)158 * 1024;
    // greedy: both kernels; grasp (its runner-up is one more query with an id limit): the LDS-resident one
    const bool use_nn = inst->d_sperm && !nn_off && (small || (big && kind == TSP_CONSTRUCT_GREEDY));
    // one 64-bit key per candidate when the costs are integers and ids/slots fit their fields
    const bool pack = inst->integer_cost && (small ? (inst->n_slots <= 32768 && inst->cost_bound < 2147483647.0)
                                                   : (inst->n_slots <= 262144 && inst->cost_bound < 268435455.0));
    p.float_xy = icoord;
    p.pack = pack;
    if (use_nn) {
        p.path = small ? CONS_NN : CONS_NN_BIG;
        p.lds_bytes = small ? need : need_big;
        return p;
    }
    const size_t lds_bytes = 4 * (kConsLdsThreads / 64) * sizeof(ConsSlot) + sizeof(double2) * (size_t)inst->n;
    const bool use_lds = TSP_SW(inst, CONSTRUCT_GLOBAL, 0) != 1 && inst->n <= kConsLdsMaxN && lds_bytes <= (size_t)160 * 1024;
    p.path = use_lds ? CONS_LDS : CONS_GLOBAL;
    p.lds_bytes = use_lds ? lds_bytes : 0;
    return p;
}

}  // namespace tsp

using namespace tsp;

extern "C" {

int tsp_dev_construct(tsp_dev_inst *inst, int kind, int B, const int *starts, const double *urand, int *succ,
                      int succ_stride, int64_t tour_stride, double *obj, int *status_out) {
    if (!inst || !starts || !succ || !obj || B < 1 || succ_stride < 1) return TSP_DEV_E_ARG;
    if (kind != TSP_CONSTRUCT_GREEDY && kind != TSP_CONSTRUCT_GRASP) return TSP_DEV_E_ARG;
    if (kind == TSP_CONSTRUCT_GRASP && !urand) return TSP_DEV_E_ARG;
    const int n = inst->n;
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    hipStream_t s = inst->ctx->stream;
    // scratch of a call, carved out of one per-instance allocation that only grows (multi-start loops call again
    // and again with the same shape; seven hipMallocs cost more than a batch of small starts)
    const bool grasp_call = kind == TSP_CONSTRUCT_GRASP;
    const size_t bn = (size_t)B * n;
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_urand = 0, o_obj = o_urand + up(grasp_call ? 8 * bn : 0), o_succ = o_obj + up(8 * (size_t)B),
                 o_starts = o_succ + up(4 * bn), o_status = o_starts + up(4 * (size_t)B), o_slots = o_status + up(4 * (size_t)B),
                 o_vis = o_slots + up(4 * (size_t)B), total_bytes = o_vis + up(bn);
    if (inst->cons_pool_bytes < total_bytes) {
        (void)hipFree(inst->cons_pool);
        inst->cons_pool = nullptr; inst->cons_pool_bytes = 0;
        TSP_HIP_TRY(hipMalloc(&inst->cons_pool, total_bytes));
        inst->cons_pool_bytes = total_bytes;
    }
    char *pool = static_cast<char *>(inst->cons_pool);
    struct { double *p; } d_urand{grasp_call ? reinterpret_cast<double *>(pool + o_urand) : nullptr};
    double *d_obj = reinterpret_cast<double *>(pool + o_obj);
    int *d_succ = reinterpret_cast<int *>(pool + o_succ), *d_starts = reinterpret_cast<int *>(pool + o_starts),
        *d_status = reinterpret_cast<int *>(pool + o_status), *d_slots = reinterpret_cast<int *>(pool + o_slots);
    unsigned char *d_vis = reinterpret_cast<unsigned char *>(pool + o_vis);
    TSP_HIP_TRY(hipMemcpyAsync(d_starts, starts, sizeof(int) * (size_t)B, hipMemcpyHostToDevice, s));
    TSP_HIP_TRY(hipMemsetAsync(d_succ, 0, sizeof(int) * bn, s));  // CALLOC'd edges, solver.c:270
    if (grasp_call)
        TSP_HIP_TRY(hipMemcpyAsync(d_urand.p, urand, sizeof(double) * bn, hipMemcpyHostToDevice, s));
    const ConstructPlan plan = construct_plan(inst, kind);
    const bool use_nn = plan.path == CONS_NN || plan.path == CONS_NN_BIG;
    {
        const bool small = plan.path == CONS_NN, pack = plan.pack;
        if (use_nn) {
            std::vector<int> slots((size_t)B, 0);
            for (int b = 0; b < B; ++b) if (starts[b] >= 0 && starts[b] < n) slots[b] = inst->h_sinv[starts[b]];
            TSP_HIP_TRY(hipMemcpyAsync(d_slots, slots.data(), sizeof(int) * (size_t)B, hipMemcpyHostToDevice, s));
            TSP_HIP_TRY(hipStreamSynchronize(s));   // `slots` dies with this scope
            hipError_t e_nn = hipSuccess;
            TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
                if constexpr (has_root_filter<WTC>()) {
                    constexpr bool IC = WTC == tsp::WT_EUC_2D_ICOORD || WTC == tsp::WT_CEIL_2D_ICOORD || WTC == tsp::WT_ATT_ICOORD;
                    using CT = std::conditional_t<IC, float2, double2>;
                    const double ox = IC ? inst->org_x : 0.0, oy = IC ? inst->org_y : 0.0;
                    if (small) {
                        const bool grasp = kind == TSP_CONSTRUCT_GRASP;
                        auto kf = grasp ? (pack ? k_construct_nn<WTC, INTC, CT, true, true> : k_construct_nn<WTC, INTC, CT, false, true>)
                                        : (pack ? k_construct_nn<WTC, INTC, CT, true, false> : k_construct_nn<WTC, INTC, CT, false, false>);
                        e_nn = hipFuncSetAttribute(reinterpret_cast<const void *>(kf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes);
                        hipLaunchKernelGGL(kf, dim3(B), dim3(64), plan.lds_bytes, s, inst->d_coord, inst->d_sperm, inst->d_gbox, n, inst->ng,
                                           inst->n_slots, ox, oy, d_starts, d_slots, (const double *)d_urand.p, d_succ, d_obj, d_status);
                    } else {
                        if (!inst->d_sxy) {   // rank-ordered coordinates, once per instance
                            e_nn = hipMalloc(&inst->d_sxy, sizeof(CT) * (size_t)inst->n_slots);
                            if (e_nn == hipSuccess)
                                hipLaunchKernelGGL((k_sorted_xy<CT>), dim3((inst->n_slots + 255) / 256), dim3(256), 0, s, inst->d_coord,
                                                   inst->d_sperm, (CT *)inst->d_sxy, inst->n_slots, ox, oy);
                        }
                        if (e_nn == hipSuccess) {
                            auto kf = pack ? k_construct_nn_big<WTC, INTC, CT, true> : k_construct_nn_big<WTC, INTC, CT, false>;
                            e_nn = hipFuncSetAttribute(reinterpret_cast<const void *>(kf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes);
                            hipLaunchKernelGGL(kf, dim3(B), dim3(64), plan.lds_bytes, s, (const CT *)inst->d_sxy, inst->d_sperm, inst->d_gbox, n,
                                               inst->ng, ox, oy, d_starts, d_slots, d_succ, d_obj, d_status);
                        }
                    }
                }
            });
            TSP_HIP_TRY(e_nn);
        }
    }
    const bool use_lds = plan.path == CONS_LDS;
    hipError_t attr_err = hipSuccess;
    if (!use_nn) TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        if (use_lds) {
            if (kind == TSP_CONSTRUCT_GRASP) {
                auto kf = k_construct_lds<WTC, INTC, true>;
                attr_err = hipFuncSetAttribute(reinterpret_cast<const void *>(kf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes);
                hipLaunchKernelGGL(kf, dim3(B), dim3(kConsLdsThreads), plan.lds_bytes, s, inst->d_coord, n, d_starts, d_urand.p,
                                   d_succ, d_obj, d_status);
            } else {
                auto kf = k_construct_lds<WTC, INTC, false>;
                attr_err = hipFuncSetAttribute(reinterpret_cast<const void *>(kf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes);
                hipLaunchKernelGGL(kf, dim3(B), dim3(kConsLdsThreads), plan.lds_bytes, s, inst->d_coord, n, d_starts,
                                   (const double *)nullptr, d_succ, d_obj, d_status);
            }
        } else if (kind == TSP_CONSTRUCT_GRASP)
            hipLaunchKernelGGL((k_construct<WTC, INTC, true>), dim3(B), dim3(kConsThreads), 0, s, inst->d_coord, n,
                               d_starts, d_urand.p, d_vis, d_succ, d_obj, d_status);
        else
            hipLaunchKernelGGL((k_construct<WTC, INTC, false>), dim3(B), dim3(kConsThreads), 0, s, inst->d_coord, n,
                               d_starts, (const double *)nullptr, d_vis, d_succ, d_obj, d_status);
    });
    TSP_HIP_TRY(attr_err);
    std::vector<int> h_succ((size_t)B * n), h_status((size_t)B);
    TSP_HIP_TRY(hipMemcpyAsync(h_succ.data(), d_succ, sizeof(int) * (size_t)B * n, hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipMemcpyAsync(h_status.data(), d_status, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipMemcpyAsync(obj, d_obj, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipStreamSynchronize(s));
    TSP_HIP_TRY(hipGetLastError());
    int worst = TSP_OK;
    for (int b = 0; b < B; ++b) {
        if (status_out) status_out[b] = h_status[b];
        if (h_status[b] != TSP_OK) { worst = h_status[b]; continue; }  // edges untouched, like :20
        int *sp = succ + (size_t)b * tour_stride;
        for (int v = 0; v < n; ++v) sp[(size_t)v * succ_stride] = h_succ[(size_t)b * n + v];
    }
    return (B == 1) ? worst : TSP_OK;
}

int tsp_dev_construct_describe(tsp_dev_inst *inst, int kind, char *buf, int cap) {
    if (!inst || !buf || cap < 1 || (kind != TSP_CONSTRUCT_GREEDY && kind != TSP_CONSTRUCT_GRASP)) return TSP_DEV_E_ARG;
    const ConstructPlan p = construct_plan(inst, kind);
    if (p.path == CONS_NN || p.path == CONS_NN_BIG)
        snprintf(buf, (size_t)cap, "%s<%s, %s>", p.path == CONS_NN ? "k_construct_nn" : "k_construct_nn_big",
                 p.float_xy ? "float2" : "double2", p.pack ? "packed" : "generic");
    else
        snprintf(buf, (size_t)cap, "%s", p.path == CONS_LDS ? "k_construct_lds" : "k_construct");
    return TSP_OK;
}

int tsp_dev_dist_matrix(tsp_dev_inst *inst, void *out_host, int as_int32, float *kernel_ms) {
    if (!inst) return TSP_DEV_E_ARG;
    if (as_int32 && !inst->integer_cost && inst->wtype_public != TSP_CEIL_2D) return TSP_DEV_E_ARG;
    const int n = inst->n;
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    hipStream_t s = inst->ctx->stream;
    const size_t bytes = (size_t)n * n * (as_int32 ? 4 : 8);
    // Timing-only calls (out_host == NULL) rotate over several output buffers, more than 768 MB in all and at least three:
    // a launch never stores into lines that the 256 MB Infinity Cache may still hold from the launch before it, so the
    // rate that comes out is an HBM write rate (back-to-back launches into ONE 400 MB buffer measured ~8 % high).
    const int nbuf = out_host ? 1 : (int)std::max<size_t>(3, ((size_t)800 << 20) / std::max<size_t>(bytes, 1) + 1);
    std::vector<DevBuf<char>> bufs((size_t)nbuf);
    for (int k = 0; k < nbuf; ++k) TSP_HIP_TRY(bufs[k].alloc(bytes));
    hipEvent_t e0, e1;
    TSP_HIP_TRY(hipEventCreate(&e0));
    TSP_HIP_TRY(hipEventCreate(&e1));
    const int rows_per_block = as_int32 ? dm_rows<int>() : dm_rows<double>();
    const dim3 grid((n + 1023) / 1024, (n + rows_per_block - 1) / rows_per_block);
    const int reps = out_host ? 1 : 4 * nbuf;  // timing-only calls: warm once per buffer, then average back-to-back launches
    float ms = 0.f;
    auto launch = [&](int k) {
        void *d_out = bufs[(size_t)(k % nbuf)].p;
        TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
            if (as_int32)
                hipLaunchKernelGGL((k_dist_matrix<WTC, INTC, int>), grid, dim3(256), 0, s, inst->d_coord, n, (int *)d_out);
            else
                hipLaunchKernelGGL((k_dist_matrix<WTC, INTC, double>), grid, dim3(256), 0, s, inst->d_coord, n,
                                   (double *)d_out);
        });
    };
    if (!out_host) for (int k = 0; k < nbuf; ++k) launch(k);
    TSP_HIP_TRY(hipEventRecord(e0, s));
    for (int r = 0; r < reps; ++r) launch(r);
    TSP_HIP_TRY(hipEventRecord(e1, s));
    TSP_HIP_TRY(hipEventSynchronize(e1));
    TSP_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    ms /= (float)reps;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (out_host) {
        TSP_HIP_TRY(hipMemcpyAsync(out_host, bufs[0].p, bytes, hipMemcpyDeviceToHost, s));
        TSP_HIP_TRY(hipStreamSynchronize(s));
    }
    TSP_HIP_TRY(hipGetLastError());
    if (kernel_ms) *kernel_ms = ms;
    return TSP_OK;
}

}  // extern "C"
