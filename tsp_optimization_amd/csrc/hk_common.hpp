// hk_common.hpp -- what the dense 1-trees (held_karp.hip) and the 1-trees over the candidate graph (held_karp_sparse.hip) share:
// the control block, the instance's scratch, the Boruvka round kernels and the closing kernel's body.
// The kernels have internal linkage: each of the two files that include this compiles its own.  The structures are tsp::'s, so
// that both files mean the same HkData behind tsp_dev_inst::hk_data.
#pragma once
#include "tsp_internal.hpp"
#include "row_scan.hpp"
#include <math.h>
#include <algorithm>

#pragma clang fp contract(off)

namespace tsp {

typedef unsigned long long hk_u64;

constexpr int kHkMaxRounds = 32;      // ceil(log2(n - 1)) <= 31
constexpr int kHkWaves = 8192;        // k_hk_scan: column chunks chosen so that about this many waves exist
constexpr int kHkMaxChunks = 64;
constexpr int kHkMinChunk = 32;       // ... of at least this many columns
constexpr int kFinThreads = 1024;
constexpr hk_u64 kNone = ~0ull;

typedef ScanCol HkCol;   // tag = the node's component

struct alignas(16) HkCtl {
    double ub, lambda, best, W;
    long long iters, max_iters, trees, rounds, dists, gnorm2;
    int patience, stall, done, stop, tour_found, first, last_rounds, pad;
    int ncomp[kHkMaxRounds + 4];   // components among nodes 1 .. n-1 at the start of round r
};

// The sparse trees' own words beside HkCtl.  sparse_rounds: rounds over the candidate graph in which a component hooked;
// completion_rounds: rounds over the complete graph behind them; both summed over the finished trees, last_* of the last one.
// components: what the candidate graph leaves of nodes 1 .. n-1 (-1: not known yet; it does not depend on the penalties).
struct alignas(16) HkSpCtl {
    long long sparse_rounds, completion_rounds, weights;
    int components, last_sparse, last_completion, pad;
};

// What the closing kernel of a sparse tree needs beyond the dense one's arguments: node 0's candidate edges (flag and distance
// per other end), the sparse words and the number of queued rounds that ran over the candidate graph.
struct HkSpFin {
    const unsigned char *zflag;
    const double *zd;
    HkSpCtl *sctl;
    int Rs;
};

}  // namespace tsp

using namespace tsp;

namespace {

__device__ __forceinline__ bool hk_idle(const HkCtl *c) { return (c->done | c->stop) != 0; }

// monotone map double -> u64 (no NaN occurs: coordinates and penalties are finite)
__device__ __forceinline__ hk_u64 ord_of(double w) {
    const hk_u64 b = (hk_u64)__double_as_longlong(w + 0.0);   // -0.0 -> +0.0: they compare equal
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}
__device__ __forceinline__ double ord_back(hk_u64 k) {
    return __longlong_as_double((long long)(k ^ ((k >> 63) ? (1ull << 63) : ~0ull)));
}

// arr[comp] = min(arr[comp], key) for the lanes with `valid`; the first four distinct components of a wave are reduced in
// the wave first (late rounds: a few components, tens of thousands of nodes).  Every lane of the wave must call this.
__device__ __forceinline__ void comp_atomic_min(hk_u64 *arr, int comp, hk_u64 key, bool valid) {
    const int lane = threadIdx.x & 63;
    hk_u64 todo = __ballot(valid);
    for (int it = 0; it < 4 && todo; ++it) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __shfl(comp, leader);
        const bool mine = valid && comp == lc;
        hk_u64 k = mine ? key : kNone;
        for (int off = 32; off > 0; off >>= 1) {
            const hk_u64 o = __shfl_xor(k, off);
            k = o < k ? o : k;
        }
        if (lane == leader) atomicMin(&arr[lc], k);
        todo &= ~__ballot(mine);
        valid = valid && !mine;
    }
    if (valid) atomicMin(&arr[comp], key);
}

// Per tree: column records from the resident penalties, every node its own component, empty edge slots.
__global__ __launch_bounds__(256) void k_hk_init(const double2 *__restrict__ coord, const double *__restrict__ pi, int n,
                                                 HkCtl *__restrict__ ctl, HkCol *__restrict__ col, hk_u64 *__restrict__ compw,
                                                 hk_u64 *__restrict__ compe, int *__restrict__ deg, int *__restrict__ elo,
                                                 double *__restrict__ ew) {
    if (hk_idle(ctl)) return;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v <= kHkMaxRounds) ctl->ncomp[v] = v == 0 ? n - 1 : 0;
    if (v > n) return;
    elo[v] = -1; ew[v] = 0.0;   // n + 1 slots
    if (v == n) return;
    const double2 c = coord[v];
    HkCol r;
    r.x = c.x; r.y = c.y; r.pi = pi[v]; r.tag = v; r.pad = 0;
    col[v] = r;
    compw[v] = kNone; compe[v] = kNone; deg[v] = 0;
}

// Row node v = one lane, columns [max(1, chunk * CH), chunk * CH + CH): pw / po [chunk * n + v] = the smallest edge (w, other
// end) from v into another component (+inf, -1: none).
template <int WT, bool INT>
__global__ __launch_bounds__(256) void k_hk_scan(const HkCol *__restrict__ col, const HkCtl *__restrict__ ctl, int r, int n, int CH,
                                                 double *__restrict__ pw, int *__restrict__ po) {
    if (hk_idle(ctl) || ctl->ncomp[r] <= 1) return;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    const int chunk = blockIdx.y;
    const int c0 = max(1, chunk * CH), c1 = min(n, chunk * CH + CH);
    const HkCol me = col[min(v, n - 1)];
    double bw = INFINITY;
    int bo = -1;
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {   // (unrolled: four columns' scalar loads in flight)
        const HkCol cc = col[c];
        const double w = pair_weight<WT, INT>(v, me.x, me.y, me.pi, c, cc.x, cc.y, cc.pi);
        if (cc.tag != me.tag && w < bw) { bw = w; bo = c; }
    }
    if (v >= n) return;
    const size_t at = (size_t)chunk * n + v;
    pw[at] = bw; po[at] = bo;
}

// The chunks of node v merged in column order; the smallest weight of its component.
__global__ __launch_bounds__(256) void k_hk_min1(const HkCol *__restrict__ col, const HkCtl *__restrict__ ctl, int r, int n, int Cc,
                                                 const double *__restrict__ pw, const int *__restrict__ po,
                                                 double *__restrict__ candw, int *__restrict__ cando, hk_u64 *__restrict__ compw) {
    if (hk_idle(ctl) || ctl->ncomp[r] <= 1) return;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    double bw = INFINITY;
    int bo = -1;
    if (v >= 1 && v < n) {
        for (int c = 0; c < Cc; ++c) {
            const size_t at = (size_t)c * n + v;
            const double w = pw[at];
            if (w < bw) { bw = w; bo = po[at]; }
        }
        candw[v] = bw; cando[v] = bo;
    }
    const bool valid = bo >= 0;
    comp_atomic_min(compw, valid ? col[v].tag : 0, valid ? ord_of(bw) : kNone, valid);
}

// Among the nodes that hold their component's smallest weight: the smallest (lo, hi).
__global__ __launch_bounds__(256) void k_hk_min2(const HkCol *__restrict__ col, const HkCtl *__restrict__ ctl, int r, int n,
                                                 const double *__restrict__ candw, const int *__restrict__ cando,
                                                 const hk_u64 *__restrict__ compw, hk_u64 *__restrict__ compe) {
    if (hk_idle(ctl) || ctl->ncomp[r] <= 1) return;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    int comp = 0;
    hk_u64 key = kNone;
    if (v >= 1 && v < n) {
        const int o = cando[v];
        if (o >= 0) {
            comp = col[v].tag;
            valid = ord_of(candw[v]) == compw[comp];
            key = ((hk_u64)(unsigned)min(v, o) << 32) | (hk_u64)(unsigned)max(v, o);
        }
    }
    comp_atomic_min(compe, comp, key, valid);
}

// Per root r0: parent = the root of the component its edge leads to, or itself when both chose the same edge and r0 is the
// lower root.  A root that is hooked keeps the edge in its own slot and counts it into the degrees (integer atomics).
__global__ __launch_bounds__(256) void k_hk_hook(const HkCol *__restrict__ col, HkCtl *__restrict__ ctl, int r, int n, int rows,
                                                 const hk_u64 *__restrict__ compw, const hk_u64 *__restrict__ compe,
                                                 int *__restrict__ parent, int *__restrict__ deg, int *__restrict__ elo,
                                                 int *__restrict__ ehi, double *__restrict__ ew) {
    if (hk_idle(ctl)) return;
    const int nc = ctl->ncomp[r];
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (nc <= 1) {
        if (v == 0) atomicAdd(&ctl->ncomp[r + 1], nc);
        return;
    }
    bool hooked = false;
    if (v >= 1 && v < n && col[v].tag == v) {
        const hk_u64 e = compe[v];
        int p = v;
        if (e != kNone) {
            const int lo = (int)(e >> 32), hi = (int)(e & 0xffffffffu);
            const int other = col[lo].tag == v ? col[hi].tag : col[lo].tag;
            if (!(compe[other] == e && v < other)) {
                p = other; hooked = true;
                elo[v] = lo; ehi[v] = hi; ew[v] = ord_back(compw[v]);
                atomicAdd(&deg[lo], 1); atomicAdd(&deg[hi], 1);
            }
        }
        parent[v] = p;
    }
    const int cnt = __popcll(__ballot(hooked));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&ctl->ncomp[r + 1], -cnt);
    if (v == 0) {
        atomicAdd(&ctl->ncomp[r + 1], nc);
        ctl->dists += (long long)rows * (long long)(n - 1);
    }
}

// New component of every node: the root its old root's parent chain ends in (the chain is a path: the edge order is strict).
__global__ __launch_bounds__(256) void k_hk_relabel(HkCol *__restrict__ col, const HkCtl *__restrict__ ctl, int r, int n,
                                                    const int *__restrict__ parent, hk_u64 *__restrict__ compw,
                                                    hk_u64 *__restrict__ compe) {
    if (hk_idle(ctl) || ctl->ncomp[r] <= 1) return;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v < 1 || v >= n) return;
    int root = col[v].tag;
    for (int hop = 0; hop < n; ++hop) {   // bounded whatever the arrays hold
        const int p = parent[root];
        if (p == root) break;
        root = p;
    }
    col[v].tag = root;
    compw[v] = kNone; compe[v] = kNone;
}

// top two of two top-two lists by (w, c)
__device__ __forceinline__ bool hk_less(double w, int c, double w2, int c2) { return w < w2 || (w == w2 && c < c2); }
__device__ __forceinline__ void top2_offer(double w, int c, double &w1, int &c1, double &w2, int &c2) {
    if (hk_less(w, c, w1, c1)) { w2 = w1; c2 = c1; w1 = w; c1 = c; }
    else if (hk_less(w, c, w2, c2)) { w2 = w; c2 = c; }
}

// the workgroup's top two of every thread's top two; every thread receives them
__device__ __forceinline__ void top2_reduce(double &w1, int &c1, double &w2, int &c2, double *sw1, int *sc1, double *sw2, int *sc2) {
    const int tid = threadIdx.x;
    sw1[tid] = w1; sc1[tid] = c1; sw2[tid] = w2; sc2[tid] = c2;
    __syncthreads();
    for (int s = kFinThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            double a1 = sw1[tid], a2 = sw2[tid];
            int b1 = sc1[tid], b2 = sc2[tid];
            if (sc1[tid + s] >= 0) top2_offer(sw1[tid + s], sc1[tid + s], a1, b1, a2, b2);
            if (sc2[tid + s] >= 0) top2_offer(sw2[tid + s], sc2[tid + s], a1, b1, a2, b2);
            sw1[tid] = a1; sw2[tid] = a2; sc1[tid] = b1; sc2[tid] = b2;
        }
        __syncthreads();
    }
    w1 = sw1[0]; w2 = sw2[0]; c1 = sc1[0]; c2 = sc2[0];
}

template <typename T>
__device__ __forceinline__ T fin_sum(T v, T *sh) {   // fixed tree over the workgroup; every thread receives the sum
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int s = kFinThreads / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}

// One workgroup.  After R rounds: the two smallest edges at node 0 (slots 0 and n), W = sum w(e) - 2 sum pi, |g|^2; with
// ascent != 0 steps 2 - 5 of the ascent (include/tsp_hip.h).  A tree that still has several components raises `stop`.
// SP (k_hks_finish, held_karp_sparse.hip): node 0's edges come from its candidate edges when it has two of them; a tree that is
// a tour, or whose value has reached ub, ends the phase without tour_found and without a step; the rounds go into sp.sctl.
// With SP = false (k_hk_finish) every one of those branches is compiled out and sp is not read.
template <int WT, bool INT, bool SP>
__device__ __forceinline__ void hk_finish_body(const HkCol *__restrict__ col, HkCtl *__restrict__ ctl, int R, int n,
                                               int ascent, double *__restrict__ pi, double *__restrict__ pi_best,
                                               int *__restrict__ gprev, int *__restrict__ deg, int *__restrict__ elo,
                                               int *__restrict__ ehi, double *__restrict__ ew, const HkSpFin *__restrict__ spp) {
    if (hk_idle(ctl)) return;
    const int tid = threadIdx.x;
    if (ctl->ncomp[R] != 1) {
        if (tid == 0) ctl->stop = 1;
        return;
    }
    __shared__ double sw1[kFinThreads], sw2[kFinThreads];
    __shared__ int sc1[kFinThreads], sc2[kFinThreads];
    __shared__ long long sll[kFinThreads];
    // the control block as the iteration found it (thread 0 writes it at the end, behind a barrier)
    const double ub = ctl->ub, lambda = ctl->lambda, best = ctl->best;
    const long long iters = ctl->iters, max_iters = ctl->max_iters;
    const int patience = ctl->patience, stall = ctl->stall, first = ctl->first;
    const HkCol z = col[0];
    double w1 = INFINITY, w2 = INFINITY;
    int c1 = -1, c2 = -1;
    bool have = false;   // node 0's two edges are known
    if constexpr (SP) {
        // the candidate edges at node 0, each once whatever the lists repeat: other end c is flagged, d(0, c) resident
        for (int c = 1 + tid; c < n; c += kFinThreads) {
            if (!spp->zflag[c]) continue;
            const double w = (spp->zd[c] + z.pi) + col[c].pi;
            top2_offer(w, c, w1, c1, w2, c2);
        }
        top2_reduce(w1, c1, w2, c2, sw1, sc1, sw2, sc2);
        have = c2 >= 0;
        if (!have) { w1 = INFINITY; w2 = INFINITY; c1 = -1; c2 = -1; }   // fewer than two: all n - 1 edges, as in the dense tree
        __syncthreads();
    }
    if (!SP || !have) {
        for (int c = 1 + tid; c < n; c += kFinThreads) {
            const HkCol cc = col[c];
            const double w = pair_weight<WT, INT>(0, z.x, z.y, z.pi, c, cc.x, cc.y, cc.pi);
            top2_offer(w, c, w1, c1, w2, c2);
        }
        sw1[tid] = w1; sc1[tid] = c1; sw2[tid] = w2; sc2[tid] = c2;
        __syncthreads();
        for (int s = kFinThreads / 2; s > 0; s >>= 1) {
            if (tid < s) {
                double a1 = sw1[tid], a2 = sw2[tid];
                int b1 = sc1[tid], b2 = sc2[tid];
                if (sc1[tid + s] >= 0) top2_offer(sw1[tid + s], sc1[tid + s], a1, b1, a2, b2);
                if (sc2[tid + s] >= 0) top2_offer(sw2[tid + s], sc2[tid + s], a1, b1, a2, b2);
                sw1[tid] = a1; sw2[tid] = a2; sc1[tid] = b1; sc2[tid] = b2;
            }
            __syncthreads();
        }
        w1 = sw1[0]; w2 = sw2[0]; c1 = sc1[0]; c2 = sc2[0];
    }
    if (tid == 0) {
        elo[0] = 0; ehi[0] = c1; ew[0] = w1;
        elo[n] = 0; ehi[n] = c2; ew[n] = w2;
    }
    // sums in a fixed order: thread t takes elements t, t + 1024, ...
    double s1 = 0.0, s2 = 0.0;
    long long g2 = 0;
    for (int v = tid; v < n; v += kFinThreads) {
        const int d = deg[v] + (v == 0 ? 2 : 0) + (v == c1 ? 1 : 0) + (v == c2 ? 1 : 0);
        deg[v] = d;
        g2 += (long long)(d - 2) * (d - 2);
        s2 += pi[v];
        if (v >= 1) s1 += ew[v];   // the last root's slot holds 0
    }
    s1 = fin_sum(s1, sw1);
    s2 = fin_sum(s2, sw2);
    g2 = fin_sum(g2, sll);
    const double W = ((s1 + w1) + w2) - 2.0 * s2;
    int rounds = 0;
    for (int r = 0; r < R; ++r) rounds += ctl->ncomp[r] > 1 ? 1 : 0;
    double new_best = best, new_lambda = lambda;
    int new_stall = stall, done = 0, tour = 0;
    if (ascent) {
        if (W > best) {
            new_best = W; new_stall = 0;
            for (int v = tid; v < n; v += kFinThreads) pi_best[v] = pi[v];
        } else if (++new_stall >= patience) {
            new_lambda = lambda * 0.5; new_stall = 0;
        }
        if (g2 == 0) {
            tour = SP ? 0 : 1; done = 1;
        } else if (SP && W >= ub) {
            done = 1;   // no step: its length would not be positive
        } else {
            const double t = new_lambda * (ub - W) / (double)g2;
            for (int v = tid; v < n; v += kFinThreads) {
                const int g = deg[v] - 2;
                const int gp = first ? g : gprev[v];
                pi[v] += t * (0.7 * (double)g + 0.3 * (double)gp);
                gprev[v] = g;
            }
            if (iters + 1 >= max_iters) done = 1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        ctl->W = W; ctl->gnorm2 = g2; ctl->trees += 1; ctl->rounds += rounds; ctl->last_rounds = rounds;
        if (ascent) {
            ctl->best = new_best; ctl->lambda = new_lambda; ctl->stall = new_stall; ctl->iters = iters + 1;
            ctl->first = 0; ctl->tour_found = tour; ctl->done = done;
        }
        if constexpr (SP) {
            int rs = 0, rc = 0;
            for (int r = 0; r < R; ++r) {
                if (r < spp->Rs) rs += ctl->ncomp[r + 1] < ctl->ncomp[r] ? 1 : 0;
                else rc += ctl->ncomp[r] > 1 ? 1 : 0;
            }
            spp->sctl->sparse_rounds += rs; spp->sctl->completion_rounds += rc;
            spp->sctl->last_sparse = rs; spp->sctl->last_completion = rc;
        }
    }
}

template <int WT, bool INT>
__global__ __launch_bounds__(kFinThreads) void k_hk_finish(const HkCol *__restrict__ col, HkCtl *__restrict__ ctl, int R, int n,
                                                           int ascent, double *__restrict__ pi, double *__restrict__ pi_best,
                                                           int *__restrict__ gprev, int *__restrict__ deg, int *__restrict__ elo,
                                                           int *__restrict__ ehi, double *__restrict__ ew) {
    hk_finish_body<WT, INT, false>(col, ctl, R, n, ascent, pi, pi_best, gprev, deg, elo, ehi, ew, nullptr);
}


}  // namespace

namespace tsp {

// Scratch of one instance: one device block of its own (the tree's outputs outlive the call that built it) and the pinned h_ctl.
// The sp_* part belongs to held_karp_sparse.hip, which allocates it on its first call: one more block for the list entries.
struct HkData {
    int n = 0, Rmax = 0;
    ScanChunks g = {0, 0};
    void *block = nullptr;
    HkCol *d_col = nullptr;
    HkCtl *d_ctl = nullptr, *h_ctl = nullptr;   // h_ctl pinned
    double *d_pi = nullptr, *d_pi_best = nullptr, *d_candw = nullptr, *d_pw = nullptr, *d_ew = nullptr;
    int *d_gprev = nullptr, *d_deg = nullptr, *d_parent = nullptr, *d_cando = nullptr, *d_po = nullptr, *d_elo = nullptr,
        *d_ehi = nullptr;
    hk_u64 *d_compw = nullptr, *d_compe = nullptr;
    void *sp_block = nullptr;
    size_t sp_entries = 0;                          // list entries the block holds
    double *d_ed = nullptr, *d_zd = nullptr;        // d(lo, hi) per list entry; d(0, c) per node
    hk_u64 *d_entk = nullptr;                       // the round's ordered weight per entry (kNone: not an outgoing edge)
    unsigned char *d_zflag = nullptr;               // {0, c} is a candidate edge
    HkSpCtl *d_sctl = nullptr, *h_sctl = nullptr;   // h_sctl pinned
    ~HkData() { (void)hipFree(block); (void)hipHostFree(h_ctl); (void)hipFree(sp_block); (void)hipHostFree(h_sctl); }
};

inline int hk_alloc_arrays(HkData *x, int n) {
    x->n = n;
    x->g = scan_chunks(n, kHkWaves, kHkMaxChunks, kHkMinChunk);
    while ((1ll << x->Rmax) < n - 1) x->Rmax += 1;
    const size_t N = (size_t)n, P = (size_t)x->g.Cc * N;
    auto lay = [&](Carver &c) {
        c(x->d_col, N); c(x->d_ctl, 1); c(x->d_pi, N); c(x->d_pi_best, N); c(x->d_candw, N); c(x->d_pw, P); c(x->d_ew, N + 1);
        c(x->d_gprev, N); c(x->d_deg, N); c(x->d_parent, N); c(x->d_cando, N); c(x->d_po, P); c(x->d_elo, N + 1);
        c(x->d_ehi, N + 1); c(x->d_compw, N); c(x->d_compe, N);
    };
    TSP_HIP_TRY(hipMalloc(&x->block, carve_bytes(lay)));
    carve(x->block, lay);
    TSP_HIP_TRY(hipHostMalloc(&x->h_ctl, sizeof(HkCtl), hipHostMallocDefault));
    return TSP_OK;
}

// allocated on first use, freed with the instance
inline int hk_alloc(tsp_dev_inst *inst, HkData **out) {
    if (!inst->hk_data) {
        HkData *x = new HkData();
        const int rc = hk_alloc_arrays(x, inst->n);
        if (rc) { delete x; return rc; }
        inst->hk_data = x;
    }
    *out = static_cast<HkData *>(inst->hk_data);
    return TSP_OK;
}

// pi (NULL = zeros) and a fresh control block onto the device
inline int hk_begin(tsp_dev_inst *inst, HkData *x, const double *pi, const HkCtl &c0) {
    hipStream_t s = inst->ctx->stream;
    const size_t bytes = sizeof(double) * (size_t)x->n;
    if (pi) TSP_HIP_TRY(hipMemcpyAsync(x->d_pi, pi, bytes, hipMemcpyHostToDevice, s));
    else TSP_HIP_TRY(hipMemsetAsync(x->d_pi, 0, bytes, s));
    TSP_HIP_TRY(hipMemcpyAsync(x->d_pi_best, x->d_pi, bytes, hipMemcpyDeviceToDevice, s));
    *x->h_ctl = c0;
    TSP_HIP_TRY(hipMemcpyAsync(x->d_ctl, x->h_ctl, sizeof(HkCtl), hipMemcpyHostToDevice, s));
    TSP_HIP_TRY(hipStreamSynchronize(s));   // h_ctl is polled into from here on; a pageable pi has been consumed
    return TSP_OK;
}

inline void fill_stats(tsp_lb_stats *st, const HkCtl &c, double t0, float ms) {
    if (!st) return;
    memset(st, 0, sizeof *st);
    st->iterations = c.iters; st->trees = c.trees; st->rounds = c.rounds; st->dists_executed = c.dists;
    st->tour_found = c.tour_found; st->lambda_final = c.lambda; st->seconds = wall_s() - t0; st->device_ms = ms;
}

}  // namespace tsp

namespace {

inline void queue_init(tsp_dev_inst *inst, HkData *x) {
    const int n = x->n;
    hipLaunchKernelGGL(k_hk_init, dim3((n + 1 + 255) / 256), dim3(256), 0, inst->ctx->stream, inst->d_coord, x->d_pi, n, x->d_ctl,
                       x->d_col, x->d_compw, x->d_compe, x->d_deg, x->d_elo, x->d_ew);
}

// Boruvka rounds r0 .. r1 - 1 over the complete graph
template <int WT, bool INT>
void queue_dense_rounds(tsp_dev_inst *inst, HkData *x, int r0, int r1) {
    hipStream_t s = inst->ctx->stream;
    const int n = x->n;
    const int gn = (n + 255) / 256;
    for (int r = r0; r < r1; ++r) {
        hipLaunchKernelGGL((k_hk_scan<WT, INT>), dim3(gn, x->g.Cc), dim3(256), 0, s, x->d_col, x->d_ctl, r, n, x->g.CH, x->d_pw, x->d_po);
        hipLaunchKernelGGL(k_hk_min1, dim3(gn), dim3(256), 0, s, x->d_col, x->d_ctl, r, n, x->g.Cc, x->d_pw, x->d_po, x->d_candw,
                           x->d_cando, x->d_compw);
        hipLaunchKernelGGL(k_hk_min2, dim3(gn), dim3(256), 0, s, x->d_col, x->d_ctl, r, n, x->d_candw, x->d_cando, x->d_compw,
                           x->d_compe);
        hipLaunchKernelGGL(k_hk_hook, dim3(gn), dim3(256), 0, s, x->d_col, x->d_ctl, r, n, gn * 256, x->d_compw, x->d_compe,
                           x->d_parent, x->d_deg, x->d_elo, x->d_ehi, x->d_ew);
        hipLaunchKernelGGL(k_hk_relabel, dim3(gn), dim3(256), 0, s, x->d_col, x->d_ctl, r, n, x->d_parent, x->d_compw, x->d_compe);
    }
}

// One 1-tree of at most R rounds for the resident penalties, then k_hk_finish; nothing waits.
inline void queue_tree(tsp_dev_inst *inst, HkData *x, int R, int ascent) {
    queue_init(inst, x);
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        queue_dense_rounds<WTC, INTC>(inst, x, 0, R);
        hipLaunchKernelGGL((k_hk_finish<WTC, INTC>), dim3(1), dim3(kFinThreads), 0, inst->ctx->stream, x->d_col, x->d_ctl, R, x->n,
                           ascent, x->d_pi, x->d_pi_best, x->d_gprev, x->d_deg, x->d_elo, x->d_ehi, x->d_ew);
    });
}

}  // namespace
