// gpx.hip -- partition crossover of two tours (include/tsp_hip.h, "partition crossover").
//
// P pairs are grid rows.  Both parents of a pair lie on the device as order / pos (position 0 = node 0); which of them is the
// base is known to the host after the first poll (the sums of q come back with the change flags of the component rounds), and
// the kernels behind it take the pair's `base` word and swap the two roles by address.  Everything that is added up is an
// integer; there is no floating-point atomic here, so two runs return the same bits.
//
// Launches of one call: k_gpx_mark, R x k_gpx_comp (R = O(log n), queued in batches, a finished pair's rounds return at once),
// k_gpx_runs (one workgroup per pair and parent), k_gpx_decide, k_gpx_emit (one workgroup per pair), then the existing tour-cost
// kernel over the children and over the parents.
#include "tsp_internal.hpp"
#include "gpx_stretch.hpp"
#include "row_scan.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

using namespace tsp;

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int kGpxThreads = 256;    // one lane per node: k_gpx_mark, k_gpx_comp, k_gpx_decide
constexpr int kGpxWide = 1024;      // one workgroup per tour: k_gpx_runs, k_gpx_emit (chunks of ceil(n / 1024) positions a thread)
constexpr int kGpxJumps = 2;        // pointer jumps of a lane behind its hooks, per round

// rounds allowed.  Every round hooks each tree that has a smaller neighbour and halves the depth of what the hooks built; that the
// rounds stay O(log n) on every input is argued, not proven: the cap turns a miss into an error, never a hang.
inline int gpx_round_cap(int n) {
    int lg = 1;
    while ((1LL << lg) < n) ++lg;
    return 8 * lg + 16;
}

// Per pair, on the device.  Tour 0 is the caller's A, tour 1 the caller's B.
struct GpxCtl {
    u64 q_lo[2], q_hi[2];   // sum of q over the edges of tour 0 / 1, low 32 bits and the bits above them added up apart (no carry
                            // can be lost: each part stays below n 2^32)
    int q_over;             // an edge's q does not fit 2^62 (or its distance is not finite)
    int common;             // common edges
    int err;                // an index left its range (never, for an algorithm that is right): TSP_DEV_E_INTERNAL
    int stretches;
    i64 components, exchangeable, taken, gain_q;
};

struct GpxBufs {
    GpxCtl *ctl;       // P
    int *base;         // P: which tour is the base
    int *chg;          // P x cap: round r of the pair changed a label
    int *order, *pos;  // 2 x P x n (tour-major)
    int *cm;           // 2 x P x n: the edge behind position p of the tour is common
    int *ext;          // 2 x P x n: ... lies in an external common run
    int *left, *right; // 2 x P x n: nearest boundary scans (first the non-common edges, then the external ones)
    int *partner;      // 2 x P x n: the other end of the stretch that ends at this node, by node
    i64 *qe;           // 2 x P x n: q of the node's successor edge in the tour, 0 when it is common
    int *nbr;          // P x 4n: the node's neighbours in H (-1: none)
    int *label;        // P x n
    int *flags;        // P x n, by component: bit 0 = has a stretch, bit 1 = a stretch whose ends do not pair
    i64 *qsum;         // 2 x P x n, by component: sum of qe over its nodes
    int *off;          // P x n: where the piece that starts at base position p begins in the child
    int *child;        // P x n: the child's order
    int *succ;         // P x n
    double *cost;      // 3P: children, then the 2P parents
};

// ---- sums over a workgroup, integers only --------------------------------------------------------
__device__ __forceinline__ u64 wave_sum(u64 v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// ---- k_gpx_mark: one lane per node ---------------------------------------------------------------
// Common flags of the node's four tour edges, its neighbours in H, q of its two successor edges, the sums of q and the start of
// the labels and of the per-component slots.
template <int WT, bool INT>
__global__ __launch_bounds__(kGpxThreads) void k_gpx_mark(const double2 *__restrict__ coord, GpxBufs b, int n, int P) {
    const int pr = blockIdx.y;
    const int v = blockIdx.x * kGpxThreads + threadIdx.x;
    const size_t t0 = (size_t)pr * n, t1 = ((size_t)P + pr) * n;
    u64 lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0, ncommon = 0;
    int over = 0;
    if (v < n) {
        const int pa = b.pos[t0 + v], pb = b.pos[t1 + v];
        const int an = b.order[t0 + gpx_next(pa, n)], ap = b.order[t0 + gpx_prev(pa, n)];
        const int bn = b.order[t1 + gpx_next(pb, n)], bp = b.order[t1 + gpx_prev(pb, n)];
        const bool c_an = an == bn || an == bp, c_ap = ap == bn || ap == bp;
        const bool c_bn = bn == an || bn == ap, c_bp = bp == an || bp == ap;
        b.cm[t0 + pa] = c_an;
        b.cm[t1 + pb] = c_bn;
        int *nb = b.nbr + ((size_t)pr * n + v) * 4;
        nb[0] = c_an ? -1 : an; nb[1] = c_ap ? -1 : ap; nb[2] = c_bn ? -1 : bn; nb[3] = c_bp ? -1 : bp;
        const double2 cv = coord[v], ca = coord[an], cb = coord[bn];
        // d with the lower id first, as tsp_dev_dist_pairs is asked for it
        const double da = v < an ? dist_xy<WT, INT>(cv.x, cv.y, ca.x, ca.y) : dist_xy<WT, INT>(ca.x, ca.y, cv.x, cv.y);
        const double db = v < bn ? dist_xy<WT, INT>(cv.x, cv.y, cb.x, cb.y) : dist_xy<WT, INT>(cb.x, cb.y, cv.x, cv.y);
        i64 qa = 0, qb = 0;
        if (da >= 0.0 && da < 0x1p42) qa = llrint(ldexp(da, 20)); else over = 1;
        if (db >= 0.0 && db < 0x1p42) qb = llrint(ldexp(db, 20)); else over = 1;
        b.qe[t0 + v] = c_an ? 0 : qa;
        b.qe[t1 + v] = c_bn ? 0 : qb;
        lo0 = (u64)qa & 0xffffffffull; hi0 = (u64)qa >> 32;
        lo1 = (u64)qb & 0xffffffffull; hi1 = (u64)qb >> 32;
        ncommon = c_an ? 1 : 0;
        b.label[t0 + v] = v;
        b.flags[t0 + v] = 0;
        b.qsum[t0 + v] = 0;
        b.qsum[t1 + v] = 0;
    }
    lo0 = wave_sum(lo0); hi0 = wave_sum(hi0); lo1 = wave_sum(lo1); hi1 = wave_sum(hi1); ncommon = wave_sum(ncommon);
    over = __any(over);
    if ((threadIdx.x & 63) == 0) {
        GpxCtl *c = b.ctl + pr;
        atomicAdd(&c->q_lo[0], lo0); atomicAdd(&c->q_hi[0], hi0);
        atomicAdd(&c->q_lo[1], lo1); atomicAdd(&c->q_hi[1], hi1);
        if (ncommon) atomicAdd(&c->common, (int)ncommon);
        if (over) atomicOr(&c->q_over, 1);
    }
}

// ---- k_gpx_comp: one round of hook and jump --------------------------------------------------------
// label[v] only ever falls, and only to the id of a node of v's own component, so any interleaving of the lanes is safe.  A lane
// hooks what its label points at (and itself) below every smaller label next to it, then jumps.  A round in which no lane found
// anything smaller wrote nothing: then every edge of H has one label at both ends and every label is its own label, i.e. the
// smallest id of the component.  Such a round leaves chg[r] = 0, and the rounds behind it return at once.
__global__ __launch_bounds__(kGpxThreads) void k_gpx_comp(GpxBufs b, int n, int cap, int r) {
    const int pr = blockIdx.y;
    int *chg = b.chg + (size_t)pr * cap;
    if (r > 0 && chg[r - 1] == 0) return;
    const int v = blockIdx.x * kGpxThreads + threadIdx.x;
    if (v >= n) return;
    int *label = b.label + (size_t)pr * n;
    const int *nb = b.nbr + ((size_t)pr * n + v) * 4;
    int lv = __hip_atomic_load(label + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bool changed = false;
    for (int k = 0; k < 4; ++k) {
        const int u = nb[k];
        if (u < 0) continue;
        const int lu = __hip_atomic_load(label + u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (lu < lv) {
            atomicMin(label + lv, lu);
            atomicMin(label + v, lu);
            lv = lu;
            changed = true;
        }
    }
    for (int j = 0; j < kGpxJumps; ++j) {
        const int l2 = __hip_atomic_load(label + lv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (l2 >= lv) break;
        atomicMin(label + v, l2);
        lv = l2;
        changed = true;
    }
    if (changed) chg[r] = 1;
}

// ---- nearest boundary to the left and right over one tour, by one workgroup -------------------------
// gpx_stretch.hpp has the three steps; step 2 here is a scan over the workgroup's kGpxWide chunks in LDS.  left / right are the
// tour's n words in HBM.  Every thread of the workgroup calls this; it ends behind a barrier, the results visible to all of them.
template <typename FLAG>
__device__ void gpx_nearest(FLAG flag, int n, int *left, int *right, int *s_last, int *s_first) {
    const int tid = threadIdx.x, CH = gpx_chunk_size(n, kGpxWide);
    const int lo = min(n, tid * CH), hi = min(n, lo + CH);
    int mine_last, mine_first;
    gpx_chunk_ends(flag, lo, hi, &mine_last, &mine_first);
    __syncthreads();   // whoever still reads the LDS of an earlier call
    s_last[tid] = mine_last;
    s_first[tid] = mine_first < 0 ? n : mine_first;
    __syncthreads();
    // inclusive scans: s_last[t] = the last boundary of the chunks 0 .. t, s_first[t] = the first one of the chunks t .. end
    for (int d = 1; d < kGpxWide; d <<= 1) {
        const int a = tid >= d ? s_last[tid - d] : -1;
        const int c = tid + d < kGpxWide ? s_first[tid + d] : n;
        __syncthreads();
        s_last[tid] = max(s_last[tid], a);
        s_first[tid] = min(s_first[tid], c);
        __syncthreads();
    }
    const int all_last = s_last[kGpxWide - 1], all_first = s_first[0] >= n ? -1 : s_first[0];
    const int cl = tid > 0 ? s_last[tid - 1] : -1;
    const int cr = tid + 1 < kGpxWide && s_first[tid + 1] < n ? s_first[tid + 1] : -1;
    gpx_chunk_fill(flag, lo, hi, cl, cr, all_first, all_last, left, right);
    __syncthreads();
}

// ---- k_gpx_runs: one workgroup per (pair, parent) -------------------------------------------------------
// 1. nearest non-common edge on either side of every edge position: a common edge's run starts behind the one and ends at the other;
// 2. the run is external when the labels of its two end nodes differ;
// 3. nearest external edge on either side: the stretch of a node starts behind the one to its left and ends at the one to its right;
// 4. every stretch writes its two ends into each other's partner slot.
// blockIdx.x = 0: the base, 1: the other parent.
__global__ __launch_bounds__(kGpxWide) void k_gpx_runs(GpxBufs b, int n, int P) {
    __shared__ int s_last[kGpxWide], s_first[kGpxWide];
    __shared__ int s_count;
    const int pr = blockIdx.y, tid = threadIdx.x;
    const int tour = blockIdx.x ^ b.base[pr];
    const size_t tb = ((size_t)tour * P + pr) * n;
    const int *order = b.order + tb, *cm = b.cm + tb, *label = b.label + (size_t)pr * n;
    int *ext = b.ext + tb, *left = b.left + tb, *right = b.right + tb, *partner = b.partner + tb;
    if (tid == 0) s_count = 0;
    gpx_nearest([&](int p) { return cm[p] == 0; }, n, left, right, s_last, s_first);
    for (int p = tid; p < n; p += kGpxWide) {
        int e = 0;
        if (cm[p] && left[p] >= 0) e = label[order[gpx_next(left[p], n)]] != label[order[right[p]]];
        ext[p] = e;
    }
    __syncthreads();
    gpx_nearest([&](int p) { return ext[p] != 0; }, n, left, right, s_last, s_first);
    int count = 0;
    for (int p = tid; p < n; p += kGpxWide) {
        if (ext[gpx_prev(p, n)] && !ext[p]) {   // the first node of a stretch
            const int x = order[p], y = order[right[p]];
            partner[x] = y;
            partner[y] = x;
            ++count;
        }
    }
    if (count) atomicAdd(&s_count, count);
    __syncthreads();
    if (tid == 0 && blockIdx.x == 0) b.ctl[pr].stretches = s_count;
}

// A component's verdict from its slots.
__device__ __forceinline__ bool gpx_taken(const GpxBufs &b, size_t ta, size_t tb, size_t tp, int c) {
    return b.flags[tp + c] == 1 && b.qsum[tb + c] < b.qsum[ta + c];
}

// ---- k_gpx_decide: one lane per node ------------------------------------------------------------------
// The end of a stretch folds "my partners agree" into its component's slot; every node adds q of its non-common successor edges
// to the component's two sums; roots are counted.
__global__ __launch_bounds__(kGpxThreads) void k_gpx_decide(GpxBufs b, int n, int P) {
    const int pr = blockIdx.y;
    const int v = blockIdx.x * kGpxThreads + threadIdx.x;
    const int base = b.base[pr];
    const size_t ta = ((size_t)base * P + pr) * n, tb = ((size_t)(base ^ 1) * P + pr) * n, tp = (size_t)pr * n;
    u64 roots = 0;
    if (v < n) {
        const int c = b.label[tp + v];
        const int *nb = b.nbr + (tp + v) * 4;
        const bool in_h = (nb[0] & nb[1] & nb[2] & nb[3]) >= 0;   // some neighbour is not -1
        if (in_h) {
            const int pa = b.pos[ta + v];
            if (b.ext[ta + gpx_prev(pa, n)] != b.ext[ta + pa])   // one external run ends here: the end of a stretch in both parents
                atomicOr(b.flags + tp + c, b.partner[ta + v] == b.partner[tb + v] ? 1 : 3);
            const i64 qa = b.qe[ta + v], qb = b.qe[tb + v];
            if (qa) atomicAdd(reinterpret_cast<u64 *>(b.qsum + ta + c), (u64)qa);
            if (qb) atomicAdd(reinterpret_cast<u64 *>(b.qsum + tb + c), (u64)qb);
            roots = c == v ? 1 : 0;
        }
    }
    roots = wave_sum(roots);
    if ((threadIdx.x & 63) == 0 && roots) atomicAdd(reinterpret_cast<u64 *>(&b.ctl[pr].components), roots);
}

// ---- k_gpx_emit: one workgroup per pair ------------------------------------------------------------------
// 1. the verdicts are counted (roots);
// 2. piece lengths along the base's order -- the first node of a stretch of a taken component stands for the other parent's stretch
//    of the same ends, the stretch's other nodes for nothing, every other node for itself -- and their exclusive scan;
// 3. the child's order: the base's own nodes by base position, the taken stretches by the other parent's position, read
//    forwards or backwards (gpx_stretch.hpp);
// 4. the successor list.
__global__ __launch_bounds__(kGpxWide) void k_gpx_emit(GpxBufs b, int n, int P) {
    __shared__ int s_sum[kGpxWide];
    const int pr = blockIdx.x, tid = threadIdx.x;
    const int base = b.base[pr];
    const size_t ta = ((size_t)base * P + pr) * n, tb = ((size_t)(base ^ 1) * P + pr) * n, tp = (size_t)pr * n;
    const int *oa = b.order + ta, *ob = b.order + tb, *pa = b.pos + ta, *pb = b.pos + tb;
    const int *exta = b.ext + ta, *extb = b.ext + tb, *label = b.label + tp;
    int *off = b.off + tp, *child = b.child + tp, *succ = b.succ + tp;
    GpxCtl *ctl = b.ctl + pr;

    for (int v = tid; v < n; v += kGpxWide) {
        const int *nb = b.nbr + (tp + v) * 4;
        if (label[v] != v || (nb[0] & nb[1] & nb[2] & nb[3]) < 0) continue;
        if (b.flags[tp + v] != 1) continue;
        atomicAdd(reinterpret_cast<u64 *>(&ctl->exchangeable), 1ull);
        const i64 qa = b.qsum[ta + v], qb = b.qsum[tb + v];
        if (qb < qa) {
            atomicAdd(reinterpret_cast<u64 *>(&ctl->taken), 1ull);
            atomicAdd(reinterpret_cast<u64 *>(&ctl->gain_q), (u64)(qa - qb));
        }
    }

    // the stretch of the node at position p of a parent: first .. last; false when p lies inside an external run (or there is none)
    auto stretch = [&](const int *ext, const int *left, const int *right, int p, int *first, int *last) {
        const int q = gpx_prev(p, n);
        if (left[q] < 0 || (ext[q] && ext[p])) return false;
        *first = gpx_next(left[q], n);
        *last = right[p];
        return true;
    };
    const int *la = b.left + ta, *ra = b.right + ta, *lb = b.left + tb, *rb = b.right + tb;
    auto piece_len = [&](int p) {
        int f, l;
        if (!stretch(exta, la, ra, p, &f, &l)) return 1;
        const int x = oa[f];
        if (!gpx_taken(b, ta, tb, tp, label[x])) return 1;
        if (p != f) return 0;
        int fb, lb2;
        if (!stretch(extb, lb, rb, pb[x], &fb, &lb2)) return 1;   // (an end of a stretch in one parent is one in the other)
        return gpx_cyc_len(fb, lb2, n);
    };
    const int CH = gpx_chunk_size(n, kGpxWide);
    const int lo = min(n, tid * CH), hi = min(n, lo + CH);
    int mine = 0;
    for (int p = lo; p < hi; ++p) mine += piece_len(p);
    s_sum[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kGpxWide; d <<= 1) {
        const int a = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += a;
        __syncthreads();
    }
    int run = tid > 0 ? s_sum[tid - 1] : 0;
    for (int p = lo; p < hi; ++p) {
        off[p] = run;
        run += piece_len(p);
    }
    if (tid == kGpxWide - 1 && s_sum[tid] != n) atomicOr(&ctl->err, 1);
    __syncthreads();

    for (int p = tid; p < n; p += kGpxWide) {
        // the base's node at p, unless a taken stretch holds it
        int f, l;
        const bool own = !stretch(exta, la, ra, p, &f, &l) || !gpx_taken(b, ta, tb, tp, label[oa[f]]);
        if (own) {
            const int at = off[p];
            if (at >= 0 && at < n) child[at] = oa[p]; else atomicOr(&ctl->err, 2);
        }
        // the other parent's node at p, when a taken stretch holds it
        int fb, lb2;
        if (stretch(extb, lb, rb, p, &fb, &lb2)) {
            const int xb = ob[fb], yb = ob[lb2];
            if (gpx_taken(b, ta, tb, tp, label[xb])) {
                // the base runs through this stretch from the end at which its external run comes first
                const bool forward = exta[gpx_prev(pa[xb], n)] != 0;
                const int start = forward ? pa[xb] : pa[yb];
                const int at = off[start] + gpx_read_off(fb, lb2, p, !forward, n);
                if (at >= 0 && at < n) child[at] = ob[p]; else atomicOr(&ctl->err, 4);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += kGpxWide) {
        const int v = child[i];
        if (v >= 0 && v < n) succ[v] = child[gpx_next(i, n)]; else atomicOr(&ctl->err, 8);
    }
}

int gpx_carve(tsp_dev_inst *inst, int P, int cap, GpxBufs *b) {
    const size_t N = (size_t)inst->n, PN = (size_t)P * N;
    auto lay = [&](Carver &c) {
        c(b->ctl, P); c(b->base, P); c(b->chg, (size_t)P * cap); c(b->order, 2 * PN); c(b->pos, 2 * PN); c(b->cm, 2 * PN);
        c(b->ext, 2 * PN); c(b->left, 2 * PN); c(b->right, 2 * PN); c(b->partner, 2 * PN); c(b->qe, 2 * PN); c(b->nbr, 4 * PN);
        c(b->label, PN); c(b->flags, PN); c(b->qsum, 2 * PN); c(b->off, PN); c(b->child, PN); c(b->succ, PN); c(b->cost, 3 * (size_t)P);
    };
    void *pool = tsp_io_pool(inst, carve_bytes(lay));
    if (!pool) return TSP_DEV_E_NOMEM;
    carve(pool, lay);
    return TSP_OK;
}

// order / pos of one successor list, position 0 = node 0; the checks of tsp_dev_tours_upload
bool gpx_order(const int *succ, int stride, int n, int *order, int *pos, std::vector<char> &seen) {
    std::fill(seen.begin(), seen.end(), 0);
    int v = 0;
    for (int p = 0; p < n; ++p) {
        if (v < 0 || v >= n || seen[v]) return false;
        seen[v] = 1;
        order[p] = v;
        pos[v] = p;
        v = succ[(size_t)v * stride];
    }
    return v == 0;
}

}  // namespace

extern "C" {

int tsp_dev_gpx(tsp_dev_inst *inst, int P, const int *succ_a, const int *succ_b, int succ_stride, int64_t tour_stride, int *succ_child,
                double *obj, tsp_gpx_stats *stats) {
    if (!inst || inst->n < 3 || P < 1 || !succ_a || !succ_b || !succ_child || succ_stride < 1) {
        tsp::set_last_error_text("tsp_dev_gpx: no instance, fewer than 3 nodes, no pair, a NULL tour or a successor stride below 1");
        return TSP_DEV_E_ARG;
    }
    const double t0 = wall_s();
    const int n = inst->n;
    const size_t N = (size_t)n, PN = (size_t)P * N;
    std::vector<int> h_order(2 * PN), h_pos(2 * PN);
    {
        std::vector<char> seen(N);
        for (int pr = 0; pr < P; ++pr) {
            if (!gpx_order(succ_a + (size_t)pr * tour_stride, succ_stride, n, &h_order[pr * N], &h_pos[pr * N], seen) ||
                !gpx_order(succ_b + (size_t)pr * tour_stride, succ_stride, n, &h_order[PN + pr * N], &h_pos[PN + pr * N], seen)) {
                tsp::set_last_error_text("tsp_dev_gpx: a parent's successor list is not one Hamiltonian cycle");
                return TSP_DEV_E_NOT_A_TOUR;
            }
        }
    }
    TSP_HIP_TRY(hipSetDevice(inst->ctx->device));
    hipStream_t s = inst->ctx->stream;
    const int cap = gpx_round_cap(n);
    GpxBufs b;
    int rc = gpx_carve(inst, P, cap, &b);
    if (rc) return rc;
    if (int e = tsp_inst_events(inst)) return e;
    TSP_HIP_TRY(hipMemcpyAsync(b.order, h_order.data(), sizeof(int) * 2 * PN, hipMemcpyHostToDevice, s));
    TSP_HIP_TRY(hipMemcpyAsync(b.pos, h_pos.data(), sizeof(int) * 2 * PN, hipMemcpyHostToDevice, s));
    TSP_HIP_TRY(hipMemsetAsync(b.ctl, 0, sizeof(GpxCtl) * P, s));
    TSP_HIP_TRY(hipMemsetAsync(b.chg, 0, sizeof(int) * (size_t)P * cap, s));
    TSP_HIP_TRY(hipMemsetAsync(b.child, 0, sizeof(int) * PN, s));   // whatever k_gpx_emit leaves out is a node the cost kernel can read
    TSP_HIP_TRY(hipEventRecord(inst->ev0, s));
    const dim3 by_node((n + kGpxThreads - 1) / kGpxThreads, P);
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_gpx_mark<WTC, INTC>), by_node, dim3(kGpxThreads), 0, s, inst->d_coord, b, n, P);
    });
    // component rounds in batches; the first look also brings the sums of q
    std::vector<GpxCtl> ctl((size_t)P);
    std::vector<int> chg((size_t)P * cap);
    std::vector<int64_t> rounds((size_t)P, 0);
    int queued = 0, batch = std::max(4, (cap - 16) / 8);   // ceil(log2 n) rounds first
    for (;;) {
        batch = std::min(batch, cap - queued);
        for (int k = 0; k < batch; ++k, ++queued) hipLaunchKernelGGL(k_gpx_comp, by_node, dim3(kGpxThreads), 0, s, b, n, cap, queued);
        TSP_HIP_TRY(hipMemcpyAsync(ctl.data(), b.ctl, sizeof(GpxCtl) * P, hipMemcpyDeviceToHost, s));
        TSP_HIP_TRY(hipMemcpyAsync(chg.data(), b.chg, sizeof(int) * (size_t)P * cap, hipMemcpyDeviceToHost, s));
        TSP_HIP_TRY(hipStreamSynchronize(s));
        TSP_HIP_TRY(hipGetLastError());
        bool all = true;
        for (int pr = 0; pr < P; ++pr) {
            int r = 0;
            while (r < queued && chg[(size_t)pr * cap + r]) ++r;
            rounds[pr] = r + 1;   // the round that found nothing is one of them
            all = all && r < queued;
        }
        if (all) break;
        if (queued >= cap) {
            tsp::set_last_error_text("tsp_dev_gpx: the component rounds did not settle within their cap");
            return TSP_DEV_E_INTERNAL;
        }
    }
    std::vector<int> base((size_t)P);
    for (int pr = 0; pr < P; ++pr) {
        const GpxCtl &c = ctl[pr];
        unsigned __int128 q[2];
        for (int k = 0; k < 2; ++k) q[k] = ((unsigned __int128)c.q_hi[k] << 32) + c.q_lo[k];
        const unsigned __int128 top = (unsigned __int128)1 << 62;
        if (c.q_over || q[0] >= top || q[1] >= top) {
            tsp::set_last_error_text("tsp_dev_gpx: a parent's fixed-point length reaches 2^62");
            return TSP_DEV_E_ARG;
        }
        base[pr] = q[1] < q[0] ? 1 : 0;
    }
    TSP_HIP_TRY(hipMemcpyAsync(b.base, base.data(), sizeof(int) * P, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_gpx_runs, dim3(2, P), dim3(kGpxWide), 0, s, b, n, P);
    hipLaunchKernelGGL(k_gpx_decide, by_node, dim3(kGpxThreads), 0, s, b, n, P);
    hipLaunchKernelGGL(k_gpx_emit, dim3(P), dim3(kGpxWide), 0, s, b, n, P);
    if (int e = tsp_perm_cost_device(inst, b.child, n, P, b.cost, sizeof(double))) return e;
    if (int e = tsp_perm_cost_device(inst, b.order, n, 2 * P, b.cost + P, sizeof(double))) return e;
    TSP_HIP_TRY(hipEventRecord(inst->ev1, s));
    std::vector<int> h_succ(PN);
    std::vector<double> cost(3 * (size_t)P);
    TSP_HIP_TRY(hipMemcpyAsync(ctl.data(), b.ctl, sizeof(GpxCtl) * P, hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipMemcpyAsync(h_succ.data(), b.succ, sizeof(int) * PN, hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipMemcpyAsync(cost.data(), b.cost, sizeof(double) * 3 * P, hipMemcpyDeviceToHost, s));
    TSP_HIP_TRY(hipStreamSynchronize(s));
    TSP_HIP_TRY(hipGetLastError());
    float ms = 0.f;
    TSP_HIP_TRY(hipEventElapsedTime(&ms, inst->ev0, inst->ev1));
    {
        // the child is one cycle, or nothing is written
        std::vector<int> o(N), p(N);
        std::vector<char> seen(N);
        for (int pr = 0; pr < P; ++pr)
            if (ctl[pr].err || !gpx_order(&h_succ[pr * N], 1, n, o.data(), p.data(), seen)) {
                tsp::set_last_error_text("tsp_dev_gpx: the child is not one Hamiltonian cycle");
                return TSP_DEV_E_INTERNAL;
            }
    }
    for (int pr = 0; pr < P; ++pr) {
        int *out = succ_child + (size_t)pr * tour_stride;
        for (int v = 0; v < n; ++v) out[(size_t)v * succ_stride] = h_succ[pr * N + v];
        if (obj) obj[pr] = cost[pr];
    }
    const double seconds = wall_s() - t0;
    for (int pr = 0; pr < P && stats; ++pr) {
        const GpxCtl &c = ctl[pr];
        tsp_gpx_stats &o = stats[pr];
        memset(&o, 0, sizeof o);
        o.common_edges = c.common; o.components = c.components; o.exchangeable = c.exchangeable; o.taken = c.taken;
        o.stretches = c.stretches; o.gain_q = c.gain_q; o.rounds = rounds[pr]; o.base = base[pr];
        o.cost_a = cost[P + pr]; o.cost_b = cost[2 * (size_t)P + pr]; o.cost_child = cost[pr];
        o.seconds = seconds; o.device_ms = ms;
    }
    return TSP_OK;
}

}  // extern "C"
