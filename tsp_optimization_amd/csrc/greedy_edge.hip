// greedy_edge.hip -- greedy-edge tour construction (tsp_dev_greedy_edge).  The definition is in include/tsp_hip.h.
//
// State per node: the column record {x, y, deg}, other[v] (the other end of v's fragment; v itself at degree 0), the cached
// smallest valid edge best[v] = (bw[v], bo[v]) and two adjacency slots.  A partner c is valid for a free node u (deg < 2) iff
// deg[c] < 2, c != u and c != other[u].
// Round r  k_ge_scan (a row scan, row_scan.hpp, over the rows of the stale list: each lane keeps its smallest valid edge) ->
//          k_ge_merge (a row's chunks into best[u]) -> k_ge_decide (edge {u, v} joins iff best(F_u) = e = best(F_v); every node
//          writes its own verdict) -> k_ge_apply (the verdicts carried out) -> k_ge_stale (the free nodes whose cached best is
//          no longer valid, compacted into the next round's list).
// Validity only shrinks, so a cached best that is still valid is still the minimum and is not rescanned: about 3 n rows are
// scanned in all, not rounds x n.  A fragment's two ends know each other through other[], so the fragment minimum is one
// comparison; a fragment takes part in at most one join per round, so no two joins touch the same state.  The only atomics are
// integer adds (edge count, list cursor); the order of the stale list does not reach any result.  Rounds are queued in batches
// without a wait: round r reads ecnt[r & 3] and adds to ecnt[(r + 1) & 3]; at n - 1 the rounds behind return at once.
#include "tsp_internal.hpp"
#include "row_scan.hpp"
#include <math.h>
#include <algorithm>

#pragma clang fp contract(off)

using namespace tsp;

namespace {

constexpr int kGeMaxChunks = 32;     // k_ge_scan: column chunks (the late rounds have a handful of rows: their time is one chunk)
constexpr int kGeMinChunk = 32;      // ... of at least this many columns
constexpr int kGeFirstBatch = 16, kGeMaxBatch = 64;   // rounds queued between two looks at the control block
constexpr int kCostThreads = 1024;

typedef ScanColDeg GeCol;

struct alignas(16) GeCtl {
    long long rounds, rows_scanned, dists, max_edges;
    int ecnt[4];   // ecnt[r & 3]: accepted edges at the start of round r
    int ns[2];     // ns[r & 1]: rows in the stale list of round r
    int pad[2];
};

__device__ __forceinline__ bool ge_over(const GeCtl *c, int r, int n) { return c->ecnt[r & 3] >= n - 1; }

// (d, lo, hi) of edge {a, b} before that of {c, e}
__device__ __forceinline__ bool ge_less(double d1, int a, int b, double d2, int c, int e) {
    const int lo1 = min(a, b), hi1 = max(a, b), lo2 = min(c, e), hi2 = max(c, e);
    return d1 < d2 || (d1 == d2 && (lo1 < lo2 || (lo1 == lo2 && hi1 < hi2)));
}

__global__ __launch_bounds__(256) void k_ge_init(const double2 *__restrict__ coord, int n, GeCol *__restrict__ col,
                                                 int *__restrict__ other, double *__restrict__ bw, int *__restrict__ bo,
                                                 int *__restrict__ adj, int *__restrict__ list) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const double2 c = coord[v];
    GeCol r;
    r.x = c.x; r.y = c.y; r.deg = 0; r.pad0 = 0; r.pad1 = 0;
    col[v] = r;
    other[v] = v; bw[v] = INFINITY; bo[v] = -1; adj[2 * v] = -1; adj[2 * v + 1] = -1; list[v] = v;
}

// Slot i of the stale list = one lane, columns [chunk * CH, chunk * CH + CH): pw / po [chunk * n + i] = the smallest valid edge
// (d, partner) of row list[i] (+inf, -1: none).  The grid covers n slots; the workgroups past the list return at once.
template <int WT, bool INT>
__global__ __launch_bounds__(256) void k_ge_scan(const GeCol *__restrict__ col, const int *__restrict__ other,
                                                 const int *__restrict__ list, const GeCtl *__restrict__ ctl, int r, int n, int CH,
                                                 double *__restrict__ pw, int *__restrict__ po) {
    if (ge_over(ctl, r, n)) return;
    const int ns = ctl->ns[r & 1];
    const int chunk = blockIdx.y;
    const int c0 = chunk * CH, c1 = min(n, chunk * CH + CH);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if ((i & ~63) >= ns) return;   // the whole wave is past the list
    const int u = list[min(i, ns - 1)];
    const GeCol me = col[u];
    const int ou = other[u];
    double bw = INFINITY;
    int bo = -1;
#pragma unroll 4
    for (int c = c0; c < c1; ++c) {   // (unrolled: four columns' scalar loads in flight)
        const GeCol cc = col[c];
        const double d = pair_dist<WT, INT>(u, me.x, me.y, c, cc.x, cc.y);
        if (cc.deg < 2 && c != u && c != ou && d < bw) { bw = d; bo = c; }
    }
    if (i < ns) {
        const size_t at = (size_t)chunk * n + i;
        pw[at] = bw; po[at] = bo;
    }
}

// The chunks of every scanned row merged in column order into best[u]; the next round's list is emptied.
__global__ __launch_bounds__(256) void k_ge_merge(GeCtl *__restrict__ ctl, int r, int n, int Cc, const int *__restrict__ list,
                                                  const double *__restrict__ pw, const int *__restrict__ po,
                                                  double *__restrict__ bw, int *__restrict__ bo) {
    if (ge_over(ctl, r, n)) return;
    const int ns = ctl->ns[r & 1];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) ctl->ns[(r + 1) & 1] = 0;
    if (i >= ns) return;
    double w = INFINITY;
    int o = -1;
    for (int c = 0; c < Cc; ++c) {
        const size_t at = (size_t)c * n + i;
        const double x = pw[at];
        if (x < w) { w = x; o = po[at]; }
    }
    const int u = list[i];
    bw[u] = w; bo[u] = o;
}

// Node u's verdict: jn[u] = {v, other[u], other[v], 0} when edge {u, v} joins in this round, else v = -1.  Both ends of a
// joining edge reach the same verdict from their own side.
__global__ __launch_bounds__(256) void k_ge_decide(const GeCol *__restrict__ col, const int *__restrict__ other,
                                                   const double *__restrict__ bw, const int *__restrict__ bo,
                                                   const GeCtl *__restrict__ ctl, int r, int n, int4 *__restrict__ jn) {
    if (ge_over(ctl, r, n)) return;
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= n) return;
    int4 j = make_int4(-1, 0, 0, 0);
    const int v = col[u].deg < 2 ? bo[u] : -1;
    if (v >= 0 && bo[v] == u) {
        const int ou = other[u], ov = other[v];
        const double d = bw[u];
        bool ok = true;
        if (ou != u && bo[ou] >= 0) ok = ge_less(d, u, v, bw[ou], ou, bo[ou]);
        if (ok && ov != v && bo[ov] >= 0) ok = ge_less(d, u, v, bw[ov], ov, bo[ov]);
        if (ok) j = make_int4(v, ou, ov, 0);
    }
    jn[u] = j;
}

// The verdicts carried out.  Node u writes its own degree and adjacency slot and the new `other` of its fragment's far end;
// nothing it reads here is written by another node.  Runs in the rounds behind the last one too: it hands the count on.
__global__ __launch_bounds__(256) void k_ge_apply(GeCol *__restrict__ col, int *__restrict__ other, int *__restrict__ adj,
                                                  const int4 *__restrict__ jn, GeCtl *__restrict__ ctl, int r, int n) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const int have = ctl->ecnt[r & 3];
    if (u == 0) {
        ctl->ecnt[(r + 2) & 3] = 0;
        atomicAdd(&ctl->ecnt[(r + 1) & 3], have);
    }
    if (have >= n - 1) return;
    bool counted = false;
    if (u < n) {
        const int4 j = jn[u];
        if (j.x >= 0) {
            const int d = col[u].deg;
            adj[2 * u + d] = j.x;
            col[u].deg = d + 1;
            other[j.y] = j.z;
            counted = u < j.x;
        }
    }
    const int cnt = __popcll(__ballot(counted));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&ctl->ecnt[(r + 1) & 3], cnt);
}

// The free nodes whose cached best is missing or no longer valid -> the list of round r + 1; the round's counters.
__global__ __launch_bounds__(256) void k_ge_stale(const GeCol *__restrict__ col, const int *__restrict__ other,
                                                  const int *__restrict__ bo, GeCtl *__restrict__ ctl, int r, int n, int rows_cols,
                                                  int *__restrict__ list) {
    if (ge_over(ctl, r, n)) return;
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u == 0) {
        const int ns = ctl->ns[r & 1];
        const long long added = ctl->ecnt[(r + 1) & 3] - ctl->ecnt[r & 3];
        ctl->rounds += 1;
        ctl->rows_scanned += ns;
        ctl->dists += (long long)((ns + 63) & ~63) * (long long)rows_cols;   // the lanes of the waves that scanned
        if (added > ctl->max_edges) ctl->max_edges = added;
    }
    bool stale = false;
    if (u < n && col[u].deg < 2) {
        const int c = bo[u];
        stale = c < 0 || col[c].deg >= 2 || c == other[u];
    }
    const unsigned long long m = __ballot(stale);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0) base = atomicAdd(&ctl->ns[(r + 1) & 1], __popcll(m));
    base = __shfl(base, 0);
    if (stale) list[base + __popcll(m & ((1ull << lane) - 1ull))] = u;
}

// *out = the sum over nodes in node order of d(v, succ v), by one workgroup (tour_cost_block's rule: integer-valued terms are
// exact in any order; the others are added one by one in node order, staged through LDS).
template <int WT, bool INT>
__global__ __launch_bounds__(kCostThreads) void k_ge_cost(const double2 *__restrict__ coord, const int *__restrict__ succ, int n,
                                                          double *__restrict__ out) {
    __shared__ double sh[4096];
    const int tid = threadIdx.x;
    if constexpr (INT || WT == WT_CEIL_2D) {
        double c = 0.0;
        for (int v = tid; v < n; v += kCostThreads) {
            const double2 a = coord[v], b = coord[succ[v]];
            c += dist_xy<WT, INT>(a.x, a.y, b.x, b.y);
        }
        sh[tid] = c;
        __syncthreads();
        for (int s = kCostThreads / 2; s > 0; s >>= 1) {
            if (tid < s) sh[tid] += sh[tid + s];
            __syncthreads();
        }
        if (tid == 0) *out = sh[0];
    } else {
        double acc = 0.0;
        for (int base = 0; base < n; base += 4096) {
            __syncthreads();
            for (int t = tid; t < 4096 && base + t < n; t += kCostThreads) {
                const int v = base + t;
                const double2 a = coord[v], b = coord[succ[v]];
                sh[t] = dist_xy<WT, INT>(a.x, a.y, b.x, b.y);
            }
            __syncthreads();
            if (tid == 0) {
                const int m = min(4096, n - base);
                for (int t = 0; t < m; ++t) acc += sh[t];
            }
        }
        if (tid == 0) *out = acc;
    }
}

// One call's scratch, carved from the instance's pooled block.
struct GeBufs {
    GeCtl *ctl;
    double *cost;
    GeCol *col;
    int4 *jn;
    double *bw, *pw;
    int *other, *bo, *adj, *list, *po, *succ;
    ScanChunks g;
};

int ge_carve(tsp_dev_inst *inst, GeBufs *b) {
    b->g = scan_chunks_few_rows(inst->n, kGeMaxChunks, kGeMinChunk);
    const size_t N = (size_t)inst->n, P = (size_t)b->g.Cc * N;
    auto lay = [&](Carver &c) {
        c(b->ctl, 1); c(b->cost, 1); c(b->col, N); c(b->jn, N); c(b->bw, N); c(b->pw, P);
        c(b->other, N); c(b->bo, N); c(b->adj, 2 * N); c(b->list, N); c(b->po, P); c(b->succ, N);
    };
    void *pool = tsp_io_pool(inst, carve_bytes(lay));
    if (!pool) return TSP_DEV_E_NOMEM;
    carve(pool, lay);
    return TSP_OK;
}

// rounds r0 .. r0 + count - 1; nothing waits
void queue_rounds(tsp_dev_inst *inst, const GeBufs &b, int r0, int count) {
    hipStream_t s = inst->ctx->stream;
    const int n = inst->n;
    const int gn = (n + 255) / 256;
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        for (int r = r0; r < r0 + count; ++r) {
            hipLaunchKernelGGL((k_ge_scan<WTC, INTC>), dim3(gn, b.g.Cc), dim3(256), 0, s, b.col, b.other, b.list, b.ctl, r, n, b.g.CH,
                               b.pw, b.po);
            hipLaunchKernelGGL(k_ge_merge, dim3(gn), dim3(256), 0, s, b.ctl, r, n, b.g.Cc, b.list, b.pw, b.po, b.bw, b.bo);
            hipLaunchKernelGGL(k_ge_decide, dim3(gn), dim3(256), 0, s, b.col, b.other, b.bw, b.bo, b.ctl, r, n, b.jn);
            hipLaunchKernelGGL(k_ge_apply, dim3(gn), dim3(256), 0, s, b.col, b.other, b.adj, b.jn, b.ctl, r, n);
            hipLaunchKernelGGL(k_ge_stale, dim3(gn), dim3(256), 0, s, b.col, b.other, b.bo, b.ctl, r, n, n, b.list);
        }
    });
}

}  // namespace

extern "C" {

int tsp_dev_greedy_edge(tsp_dev_inst *inst, int *succ, int succ_stride, double *obj, int *edges, tsp_greedy_edge_stats *stats) {
    if (!inst || inst->n < 3 || (succ && succ_stride < 1)) {
        tsp::set_last_error_text("tsp_dev_greedy_edge: no instance, fewer than 3 nodes or a successor stride below 1");
        return TSP_DEV_E_ARG;
    }
    const double t0 = wall_s();
    const int n = inst->n;
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    hipStream_t s = inst->ctx->stream;
    GeBufs b;
    int rc = ge_carve(inst, &b);
    if (rc) return rc;
    if (int e = tsp_inst_events(inst)) return e;
    GeCtl c;
    memset(&c, 0, sizeof c);
    c.ns[0] = n;
    TSP_HIP_TRY(hipMemcpyAsync(b.ctl, &c, sizeof c, hipMemcpyHostToDevice, s));
    TSP_HIP_TRY(hipStreamSynchronize(s));   // c is written into again below
    TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
    hipLaunchKernelGGL(k_ge_init, dim3((n + 255) / 256), dim3(256), 0, s, inst->d_coord, n, b.col, b.other, b.bw, b.bo, b.adj,
                       b.list);
    int queued = 0, batch = kGeFirstBatch;
    for (;;) {
        queue_rounds(inst, b, queued, batch);
        queued += batch;
        rc = poll_ctl(s, &c, b.ctl);
        if (rc) return rc;
        if (c.ecnt[queued & 3] >= n - 1) break;
        if (c.rounds != queued || queued >= n - 1) {   // every round adds an edge: n - 1 rounds always suffice
            tsp::set_last_error_text("tsp_dev_greedy_edge: the rounds did not end in one path");
            return TSP_DEV_E_HIP;
        }
        batch = std::min(batch * 2, kGeMaxBatch);
    }
    // the path's 2n adjacency entries -> the closing edge, the orientation and the edge list, on the host
    std::vector<int> adj(2 * (size_t)n), sc((size_t)n);
    TSP_HIP_TRY(hipMemcpyAsync(adj.data(), b.adj, sizeof(int) * 2 * (size_t)n, hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipStreamSynchronize(s));
    std::vector<long long> el;
    el.reserve((size_t)n);
    int e0 = -1, e1 = -1;
    bool good = c.ecnt[queued & 3] == n - 1;
    for (int v = 0; v < n && good; ++v) {
        for (int k = 0; k < 2; ++k) {
            const int w = adj[2 * (size_t)v + k];
            if (w < -1 || w >= n || w == v) good = false;
            else if (w > v) el.push_back(edge_key(v, w));
        }
        if (adj[2 * (size_t)v] < 0) good = false;
        else if (adj[2 * (size_t)v + 1] < 0) {
            if (e0 < 0) e0 = v; else if (e1 < 0) e1 = v; else good = false;
        }
    }
    good = good && e1 >= 0 && (int)el.size() == n - 1;
    if (good) {
        adj[2 * (size_t)e0 + 1] = e1; adj[2 * (size_t)e1 + 1] = e0;
        int prev = 0, v = std::min(adj[0], adj[1]), steps = 1;
        sc[0] = v;
        while (v != 0 && steps < n) {
            const int a = adj[2 * (size_t)v], nx = a == prev ? adj[2 * (size_t)v + 1] : a;
            sc[(size_t)v] = nx; prev = v; v = nx; ++steps;
        }
        good = v == 0 && steps == n;
    }
    if (!good) {
        tsp::set_last_error_text("tsp_dev_greedy_edge: the accepted edges do not form one Hamiltonian path");
        return TSP_DEV_E_HIP;
    }
    TSP_HIP_TRY(hipMemcpyAsync(b.succ, sc.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_ge_cost<WTC, INTC>), dim3(1), dim3(kCostThreads), 0, s, inst->d_coord, b.succ, n, b.cost);
    });
    TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
    double cost = 0.0;
    TSP_HIP_TRY(hipMemcpyAsync(&cost, b.cost, sizeof cost, hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipStreamSynchronize(s));
    TSP_HIP_TRY(hipGetLastError());
    float ms = 0.f;
    TSP_HIP_TRY(hipEventElapsedTime(&ms, inst->ev0, inst->ev1));
    if (succ)
        for (int v = 0; v < n; ++v) succ[(size_t)v * succ_stride] = sc[(size_t)v];
    if (obj) *obj = cost;
    if (edges) write_sorted_keys(el, edges);
    if (stats) {
        memset(stats, 0, sizeof *stats);
        stats->rounds = c.rounds; stats->edges = c.ecnt[queued & 3]; stats->rows_scanned = c.rows_scanned;
        stats->dists_executed = c.dists; stats->max_edges_in_round = c.max_edges;
        stats->seconds = wall_s() - t0; stats->device_ms = ms;
    }
    return TSP_OK;
}

}  // extern "C"
