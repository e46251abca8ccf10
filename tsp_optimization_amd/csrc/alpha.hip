// alpha.hip -- alpha-nearness from the minimum 1-tree: candidate lists (tsp_dev_inst_alpha_build) and whole alpha rows
// (tsp_dev_alpha_rows).  The definitions are in include/tsp_hip.h.
//
// Tree     tsp_hk_tree (held_karp.hip) leaves the 1-tree's edge slots and the penalties on the device.
// Order    host, O(n log n): the spanning-tree edges in ascending (w, lo, hi) order merge components Kruskal-style; a merge
//          concatenates two node sequences and writes the edge's weight at the junction, h[k] between positions k and k + 1 of
//          the final sequence, so that beta(node at p, node at q) = max(h[p .. q-1]), bit for bit a tree weight.
//          Node 0 takes the last position, n - 1; every pair with it uses w0, the larger of its two tree edges.
// Columns  k_alpha_cols: the records {x, y, pi, node} in position order.  k_alpha_bounds: per column chunk and position the
//          running maximum a lane starts the chunk with (left of the chunk: up to its first column; right of it: down to its last).
// Scan     k_alpha_scan (a row scan, row_scan.hpp, over positions; columns right of the lane ascend, columns left of it descend,
//          m = max(m, h) in a register; alpha = w - m; LISTS: the lane's 16 best (alpha, w, node); ROWS: alpha stored per
//          column) -> k_alpha_merge (LISTS: the first K stored per node).
// Nothing is accumulated in floating point and no atomic is used: two runs return the same bits.
#include "tsp_internal.hpp"
#include "row_scan.hpp"
#include <math.h>
#include <algorithm>
#include <numeric>

#pragma clang fp contract(off)

using namespace tsp;

namespace {

constexpr int kK = TSP_NL_MAX_K;     // k_alpha_scan keeps this many per row whatever K is asked for: the K best are a prefix
constexpr int kAlChunks = 16;        // most column chunks
constexpr int kAlWaves = 4096;       // ... chosen so that about this many waves exist

typedef ScanCol AlCol;               // tag = the node at this position

// the strict order of list entries: (alpha, w, node)
__device__ __forceinline__ bool al_less(double a, double w, int id, double a2, double w2, int id2) {
    return a < a2 || (a == a2 && (w < w2 || (w == w2 && id < id2)));
}

__device__ __forceinline__ void al_insert(double (&ka)[kK], double (&kw)[kK], int (&ki)[kK], double a, double w, int id) {
#pragma unroll
    for (int s = kK - 1; s >= 1; --s) {
        const bool shift = al_less(a, w, id, ka[s - 1], kw[s - 1], ki[s - 1]);
        const bool here = !shift && al_less(a, w, id, ka[s], kw[s], ki[s]);
        ka[s] = shift ? ka[s - 1] : (here ? a : ka[s]);
        kw[s] = shift ? kw[s - 1] : (here ? w : kw[s]);
        ki[s] = shift ? ki[s - 1] : (here ? id : ki[s]);
    }
    const bool first = al_less(a, w, id, ka[0], kw[0], ki[0]);
    ka[0] = first ? a : ka[0];
    kw[0] = first ? w : kw[0];
    ki[0] = first ? id : ki[0];
}

// col[p] = record of the node at position p
__global__ __launch_bounds__(256) void k_alpha_cols(const double2 *__restrict__ coord, const double *__restrict__ pi,
                                                    const int *__restrict__ ids, int n, AlCol *__restrict__ col) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int v = ids[p];
    const double2 c = coord[v];
    AlCol r;
    r.x = c.x; r.y = c.y; r.pi = pi[v]; r.tag = v; r.pad = 0;
    col[p] = r;
}

// One workgroup per column chunk [q0, q1): T[chunk * n + p] = max(h[p .. q0-1]) for p < q0, max(h[q1 .. p-1]) for p > q1,
// -inf between.  Each thread owns a run of positions; the runs' maxima are combined through LDS.
__global__ __launch_bounds__(256) void k_alpha_bounds(const double *__restrict__ h, int n, int CH, double *__restrict__ T) {
    __shared__ double seg[256];
    const int tid = threadIdx.x;
    const int q0 = blockIdx.x * CH, q1 = min(n, q0 + CH);
    double *out = T + (size_t)blockIdx.x * n;
    for (int p = q0 + tid; p <= min(q1, n - 1); p += 256) out[p] = -INFINITY;
    {   // left of the chunk: suffix maxima of h[0 .. q0-1]
        const int per = (q0 + 255) / 256;
        const int a = min(q0, tid * per), b = min(q0, a + per);
        double m = -INFINITY;
        for (int p = a; p < b; ++p) m = fmax(m, h[p]);
        seg[tid] = m;
        __syncthreads();
        double run = -INFINITY;
        for (int t = tid + 1; t < 256; ++t) run = fmax(run, seg[t]);
        for (int p = b - 1; p >= a; --p) { run = fmax(run, h[p]); out[p] = run; }
        __syncthreads();
    }
    {   // right of it: out[q1 + 1 + j] = max(h[q1 .. q1 + j]), j = 0 .. R-1
        const int R = max(0, n - q1 - 1);
        const int per = (R + 255) / 256;
        const int a = min(R, tid * per), b = min(R, a + per);
        double m = -INFINITY;
        for (int j = a; j < b; ++j) m = fmax(m, h[q1 + j]);
        seg[tid] = m;
        __syncthreads();
        double run = -INFINITY;
        for (int t = 0; t < tid; ++t) run = fmax(run, seg[t]);
        for (int j = a; j < b; ++j) { run = fmax(run, h[q1 + j]); out[q1 + 1 + j] = run; }
    }
}

// What a lane does with one column.  `beta` is the running maximum; pairs with node 0 (position n - 1) use w0 instead, and
// the smaller tree edge at node 0 (other end c1) has alpha 0 by definition (the larger one's is w0 - w0).
template <int WT, bool INT, bool ROWS>
struct AlLane {
    AlCol me;
    int p, n, c1;
    double w0;
    bool live;
    double ka[kK], kw[kK];
    int ki[kK];
    double *out;   // ROWS: this lane's row

    __device__ __forceinline__ void visit(int q, const AlCol &cc, double beta) {
        const bool vlo = me.tag < cc.tag;
        double d;   // pair_dist and pair_weight (row_scan.hpp), written out: through them the GEO scans are allocated other registers
        if constexpr (WT == WT_GEO) {
            const double ax = vlo ? me.x : cc.x, ay = vlo ? me.y : cc.y, bx = vlo ? cc.x : me.x, by = vlo ? cc.y : me.y;
            d = dist_xy<WT, INT>(ax, ay, bx, by);
        } else {
            d = dist_xy<WT, INT>(me.x, me.y, cc.x, cc.y);
        }
        const double w = (d + (vlo ? me.pi : cc.pi)) + (vlo ? cc.pi : me.pi);
        const bool zero = p == n - 1 || q == n - 1;
        double a = w - (zero ? w0 : beta);
        if (zero && (me.tag | cc.tag) == c1) a = 0.0;   // one of the two ids is 0
        if constexpr (ROWS) {
            if (live) out[cc.tag] = a;
        } else {
            if (al_less(a, w, cc.tag, ka[kK - 1], kw[kK - 1], ki[kK - 1])) al_insert(ka, kw, ki, a, w, cc.tag);
        }
    }
};

// Lane t = row position t (LISTS) or position rowpos[t] (ROWS), columns [chunk * CH, chunk * CH + CH) in position order.
// LISTS: pa / pw / pid [(chunk * 16 + s) * n + position] = s-th best of the chunk (id -1 where the chunk has fewer).
// ROWS: out[t * n + node] = alpha(row t, node); the row's own entry is not written.
template <int WT, bool INT, bool ROWS>
__global__ __launch_bounds__(256) void k_alpha_scan(const AlCol *__restrict__ col, const double *__restrict__ h,
                                                    const double *__restrict__ T, const int *__restrict__ rowpos, int nrows, int n,
                                                    int CH, double w0, int c1, double *__restrict__ pa, double *__restrict__ pw,
                                                    int *__restrict__ pid, double *__restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int chunk = blockIdx.y;
    const int q0 = chunk * CH, q1 = min(n, q0 + CH);
    AlLane<WT, INT, ROWS> L;
    L.live = t < nrows;
    L.p = ROWS ? rowpos[min(t, nrows - 1)] : min(t, n - 1);
    L.n = n; L.c1 = c1; L.w0 = w0;
    L.me = col[L.p];
    L.out = ROWS ? out + (size_t)min(t, nrows - 1) * n : nullptr;
#pragma unroll
    for (int s = 0; s < kK; ++s) { L.ka[s] = INFINITY; L.kw[s] = INFINITY; L.ki[s] = 0x7fffffff; }
    const int p = L.p;
    const double m0 = T[(size_t)chunk * n + p];
    // the wave's range of row positions bounds both loops (a wave of LISTS holds 64 adjacent positions)
    int lo = p, hi = p;
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
    }
    const int plo = __builtin_amdgcn_readfirstlane(lo), phi = __builtin_amdgcn_readfirstlane(hi);
    double m = m0;
#pragma unroll 2
    for (int q = max(q0, plo); q < q1; ++q) {   // columns right of the row: beta = max(h[p .. q-1])
        const AlCol cc = col[q];
        const double hq = h[q];
        if (q > p) L.visit(q, cc, m);
        m = q >= p ? fmax(m, hq) : m;
    }
    m = m0;
#pragma unroll 2
    for (int q = min(q1, phi) - 1; q >= q0; --q) {   // columns left of it: beta = max(h[q .. p-1])
        const AlCol cc = col[q];
        const double hq = h[q];
        if (q < p) {
            m = fmax(m, hq);
            L.visit(q, cc, m);
        }
    }
    if constexpr (!ROWS) {
        if (t >= n) return;
#pragma unroll
        for (int s = 0; s < kK; ++s) {
            const size_t at = ((size_t)chunk * kK + s) * n + t;
            const bool have = L.ki[s] != 0x7fffffff;
            pa[at] = L.ka[s]; pw[at] = L.kw[s]; pid[at] = have ? L.ki[s] : -1;
        }
    }
}

// nbr[v * K + s], alpha[v * K + s] = s-th best of the node v at position p over the chunks (the order is strict: the result
// does not depend on the order the chunks are taken in)
__global__ __launch_bounds__(256) void k_alpha_merge(int n, int Cc, int K, const int *__restrict__ ids, const double *__restrict__ pa,
                                                     const double *__restrict__ pw, const int *__restrict__ pid,
                                                     int *__restrict__ nbr, double *__restrict__ alpha) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    double ka[kK], kw[kK];
    int ki[kK];
#pragma unroll
    for (int s = 0; s < kK; ++s) { ka[s] = INFINITY; kw[s] = INFINITY; ki[s] = 0x7fffffff; }
    for (int c = 0; c < Cc; ++c)
        for (int s = 0; s < kK; ++s) {
            const size_t at = ((size_t)c * kK + s) * n + p;
            const int id = pid[at];
            if (id < 0) break;
            const double a = pa[at], w = pw[at];
            if (al_less(a, w, id, ka[kK - 1], kw[kK - 1], ki[kK - 1])) al_insert(ka, kw, ki, a, w, id);
        }
    const int v = ids[p];
#pragma unroll
    for (int s = 0; s < kK; ++s)
        if (s < K) { nbr[(size_t)v * K + s] = ki[s]; alpha[(size_t)v * K + s] = ka[s]; }
}

// The dendrogram order of the spanning tree in the edge slots: ids[p] = node at position p (node 0 last), h[p] = junction
// between p and p + 1 (-inf from n - 2 on), pos = the inverse of ids.  False: the slots do not hold a tree.
bool dendrogram(int n, const std::vector<int> &lo, const std::vector<int> &hi, const std::vector<double> &w, std::vector<int> &ids,
                std::vector<double> &h, std::vector<int> &pos) {
    std::vector<int> e;
    for (int k = 1; k < n; ++k)
        if (lo[k] >= 0) e.push_back(k);
    if ((int)e.size() != n - 2) return false;
    std::sort(e.begin(), e.end(), [&](int a, int b) {
        if (w[a] != w[b]) return w[a] < w[b];
        if (lo[a] != lo[b]) return lo[a] < lo[b];
        return hi[a] < hi[b];
    });
    std::vector<int> parent((size_t)n), head((size_t)n), tail((size_t)n), next((size_t)n, -1);
    std::vector<double> after((size_t)n, -INFINITY);   // junction behind a node
    std::iota(parent.begin(), parent.end(), 0);
    std::iota(head.begin(), head.end(), 0);
    std::iota(tail.begin(), tail.end(), 0);
    auto find = [&](int a) {
        while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; }
        return a;
    };
    for (int k : e) {
        if (lo[k] < 1 || hi[k] >= n || lo[k] >= hi[k]) return false;
        const int a = find(lo[k]), b = find(hi[k]);
        if (a == b) return false;
        next[tail[a]] = head[b];
        after[tail[a]] = w[k];
        tail[a] = tail[b];
        parent[b] = a;
    }
    ids.assign((size_t)n, 0);
    h.assign((size_t)n, -INFINITY);
    pos.assign((size_t)n, 0);
    int v = head[find(1)], p = 0;
    for (; v >= 0 && p < n - 1; v = next[v], ++p) {
        ids[p] = v; pos[v] = p;
        if (p < n - 2) h[p] = after[v];
    }
    if (p != n - 1 || v >= 0) return false;
    ids[n - 1] = 0; pos[0] = n - 1;
    return true;
}

// Everything the scans need, built for one pi.
struct AlPrep {
    int n = 0, c1 = 0;
    ScanChunks g = {0, 0};
    double w0 = 0.0, W = 0.0;
    long long rounds = 0;
    float tree_ms = 0.f;
    std::vector<int> pos;
    DevBuf<AlCol> col;
    DevBuf<double> h, T;
    DevBuf<int> ids;
};

// the tree, its dendrogram order, the column records and the chunk bounds; queued on the stream, not waited for
int prepare(tsp_dev_inst *inst, const double *pi, AlPrep *P) {
    const int n = inst->n;
    HkTree tr;
    int rc = tsp_hk_tree(inst, pi, &tr, nullptr);
    if (rc) return rc;
    hipStream_t s = inst->ctx->stream;
    std::vector<int> lo((size_t)n + 1), hi((size_t)n + 1), ids;
    std::vector<double> w((size_t)n + 1), h;
    TSP_HIP_TRY(hipMemcpy(lo.data(), tr.d_elo, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    TSP_HIP_TRY(hipMemcpy(hi.data(), tr.d_ehi, sizeof(int) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    TSP_HIP_TRY(hipMemcpy(w.data(), tr.d_ew, sizeof(double) * ((size_t)n + 1), hipMemcpyDeviceToHost));
    if (lo[0] != 0 || lo[n] != 0 || hi[0] < 1 || hi[0] >= n || !dendrogram(n, lo, hi, w, ids, h, P->pos)) {
        tsp::set_last_error_text("alpha: the edge slots do not hold a 1-tree");
        return TSP_DEV_E_HIP;
    }
    P->n = n; P->c1 = hi[0]; P->w0 = w[n]; P->W = tr.W; P->rounds = tr.rounds; P->tree_ms = tr.device_ms;
    P->g = scan_chunks(n, kAlWaves, kAlChunks, 1);
    TSP_HIP_TRY(P->col.alloc((size_t)n));
    TSP_HIP_TRY(P->h.alloc((size_t)n));
    TSP_HIP_TRY(P->T.alloc((size_t)P->g.Cc * n));
    TSP_HIP_TRY(P->ids.alloc((size_t)n));
    TSP_HIP_TRY(hipMemcpy(P->ids.p, ids.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    TSP_HIP_TRY(hipMemcpy(P->h.p, h.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    if (int e = tsp_inst_events(inst)) return e;
    TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
    hipLaunchKernelGGL(k_alpha_cols, dim3((n + 255) / 256), dim3(256), 0, s, inst->d_coord, tr.d_pi, P->ids.p, n, P->col.p);
    hipLaunchKernelGGL(k_alpha_bounds, dim3(P->g.Cc), dim3(256), 0, s, P->h.p, n, P->g.CH, P->T.p);
    return TSP_OK;
}

int fail_arg(const char *text) {
    tsp::set_last_error_text(text);
    return TSP_DEV_E_ARG;
}

}  // namespace

extern "C" {

int tsp_dev_inst_alpha_build(tsp_dev_inst *inst, int K, const double *pi, double *alpha, tsp_alpha_stats *stats) {
    if (!inst || inst->n < 3) return fail_arg("tsp_dev_inst_alpha_build: no instance, or fewer than 3 nodes");
    if (K < 1 || K > TSP_NL_MAX_K || K > inst->n - 1) return fail_arg("tsp_dev_inst_alpha_build: K must be in 1 .. min(TSP_NL_MAX_K, n - 1)");
    if (!pi_finite(pi, inst->n)) return fail_arg("tsp_dev_inst_alpha_build: a penalty is not finite");
    const double t0 = wall_s();
    const int n = inst->n;
    AlPrep P;
    int rc = prepare(inst, pi, &P);
    if (rc) return rc;
    hipStream_t s = inst->ctx->stream;
    DevBuf<double> pa, pw, d_alpha;
    DevBuf<int> pid, nbr;
    const size_t part = (size_t)P.g.Cc * kK * n;
    TSP_HIP_TRY(pa.alloc(part));
    TSP_HIP_TRY(pw.alloc(part));
    TSP_HIP_TRY(pid.alloc(part));
    TSP_HIP_TRY(nbr.alloc((size_t)n * K));
    TSP_HIP_TRY(d_alpha.alloc((size_t)n * K));
    const int gn = (n + 255) / 256;
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_alpha_scan<WTC, INTC, false>), dim3(gn, P.g.Cc), dim3(256), 0, s, P.col.p, P.h.p, P.T.p, (const int *)nullptr, n,
                           n, P.g.CH, P.w0, P.c1, pa.p, pw.p, pid.p, (double *)nullptr);
    });
    hipLaunchKernelGGL(k_alpha_merge, dim3(gn), dim3(256), 0, s, n, P.g.Cc, K, P.ids.p, pa.p, pw.p, pid.p, nbr.p, d_alpha.p);
    TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
    TSP_HIP_TRY(hipEventSynchronize(inst->ev1));
    TSP_HIP_TRY(hipGetLastError());
    float ms = 0.f;
    TSP_HIP_TRY(hipEventElapsedTime(&ms, inst->ev0, inst->ev1));
    if (alpha) TSP_HIP_TRY(hipMemcpy(alpha, d_alpha.p, sizeof(double) * (size_t)n * K, hipMemcpyDeviceToHost));
    rc = tsp_nl_adopt_lists(inst, K, nbr.p);
    if (rc) return rc;
    nbr.p = nullptr;
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->trees = 1; stats->rounds = P.rounds; stats->pairs_executed = (long long)gn * 256 * n;
        stats->tree_value = P.W; stats->seconds = wall_s() - t0; stats->device_ms = (double)P.tree_ms + (double)ms;
    }
    return TSP_OK;
}

int tsp_dev_alpha_rows(tsp_dev_inst *inst, const double *pi, int m, const int *rows, double *out) {
    if (!inst || inst->n < 3) return fail_arg("tsp_dev_alpha_rows: no instance, or fewer than 3 nodes");
    if (m < 1 || !rows || !out) return fail_arg("tsp_dev_alpha_rows: needs m >= 1 rows and a place for them");
    const int n = inst->n;
    for (int r = 0; r < m; ++r)
        if (rows[r] < 0 || rows[r] >= n) return fail_arg("tsp_dev_alpha_rows: a row index is out of range");
    if (!pi_finite(pi, n)) return fail_arg("tsp_dev_alpha_rows: a penalty is not finite");
    AlPrep P;
    int rc = prepare(inst, pi, &P);
    if (rc) return rc;
    hipStream_t s = inst->ctx->stream;
    std::vector<int> rp((size_t)m);
    for (int r = 0; r < m; ++r) rp[r] = P.pos[rows[r]];
    DevBuf<int> d_rp;
    DevBuf<double> d_out;
    TSP_HIP_TRY(d_rp.alloc((size_t)m));
    TSP_HIP_TRY(d_out.alloc((size_t)m * n));
    TSP_HIP_TRY(hipMemcpyAsync(d_rp.p, rp.data(), sizeof(int) * (size_t)m, hipMemcpyHostToDevice, s));
    TSP_HIP_TRY(hipMemsetAsync(d_out.p, 0, sizeof(double) * (size_t)m * n, s));   // out[r][rows[r]] = 0
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_alpha_scan<WTC, INTC, true>), dim3((m + 255) / 256, P.g.Cc), dim3(256), 0, s, P.col.p, P.h.p, P.T.p, d_rp.p, m,
                           n, P.g.CH, P.w0, P.c1, (double *)nullptr, (double *)nullptr, (int *)nullptr, d_out.p);
    });
    TSP_HIP_TRY(hipStreamSynchronize(s));
    TSP_HIP_TRY(hipGetLastError());
    TSP_HIP_TRY(hipMemcpy(out, d_out.p, sizeof(double) * (size_t)m * n, hipMemcpyDeviceToHost));
    return TSP_OK;
}

}  // extern "C"
