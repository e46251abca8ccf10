// or_opt.hip -- Or-opt local search on the device (tsp_dev_or_opt, tsp_dev_two_opt_or_opt).
//
// A move takes a segment f = x1 -> .. -> xL = l (L = 1..3, p = pred f, s = succ l) out of the tour and puts it between a and
// b = succ a (a not in {p, x1..xL}), forward (a f .. l b) or reversed (a l .. f b):
//     rem = (d(p,f) + d(l,s)) - d(p,s),   ins = (d(a,f) + d(l,b)) - d(a,b)  [reversed: (d(a,l) + d(f,b)) - d(a,b)],
//     delta = ins - rem.
// Best improvement: the smallest delta < 0, ties -> smallest key ((f*3 + L-1)*n + a)*2 + o (node ids, not positions).
//
// Tour state lives in HBM as order/pos per tour (the scratch tours handle of the instance), grid.z / grid.y = tour.
// A decision is either
//   FULL        k_or_prep (positions' coordinates, edge lengths, rem per row) -> k_or_scan (pair space, per-row bests per
//               column chunk) -> k_or_rows (per-row best over the chunks, stored by node) -> k_or_pick_apply, or
//   INCREMENTAL k_or_mark (rows whose window or cached best a move touched are listed for a rescan; every other row
//               checks its candidates on the move's new edges) -> k_or_rescan (listed rows, all columns) -> k_or_pick_apply.
// Per row (f, L) the cache holds the lexicographically smallest (delta, key) among its improving candidates, or none.
// A row whose segment, p and s kept their succ / pred and whose cached insertion edge still exists keeps every old
// candidate's delta, so its new best is min(cached, candidates on the new edges): both paths take the same decisions.
#include "descent.hpp"
#include "or_opt_shift.hpp"

#pragma clang fp contract(off)

using namespace tsp;

namespace {

constexpr int kRowsPerWave = 62;   // k_or_scan: rows per wave (lanes 62, 63 only complete the windows of rows 60, 61)
constexpr int kMaxChunks = 16;     // k_or_scan: column chunks per row (partials kept per chunk)
constexpr int kRescanBlocks = 256; // k_or_rescan: workgroups per tour that share the list of rows to rescan
constexpr int kPickThreads = 1024;

struct alignas(16) OrBest {
    double d;
    u64 k;
};

// Per-tour control block (written by k_or_pick_apply's thread 0 and by the counting atomics).
struct alignas(16) OrState {
    long long max_moves;       // < 0: unlimited
    long long sweeps, moves, moves_len[3], moves_rev, deltas;
    int done, ndirty;
    int nchg, ntail;
    int chg[10];               // tails and heads of the last move's new edges
    int tail[5];               // tails of the new edges = tails of the removed edges
    int pad;
};

template <int WT, bool INT>
__device__ __forceinline__ double dnode(const double2 *coord, int u, int v) {
    const double2 a = coord[u], b = coord[v];
    return dist_xy<WT, INT>(a.x, a.y, b.x, b.y);
}

// wave_shr:1 of a double (lane 0 receives 0)
__device__ __forceinline__ double shr1(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// (delta, key) minimum over the block; every thread receives it.  Lanes without a candidate hold (inf, kNoKey).
// Not block_argmin<true> of two_opt_common.hpp: every thread walks the waves' entries there, k_or_pick_apply then takes 38 VGPRs for 12.
__device__ __forceinline__ void block_argmin(double &d, u64 &k, double *sd, u64 *sk) {
    wave_argmin<true>(d, k);
    const int w = threadIdx.x >> 6, nw = (int)(blockDim.x >> 6);
    if ((threadIdx.x & 63) == 0) { sd[w] = d; sk[w] = k; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double bd = INFINITY; u64 bk = kNoKey;
        for (int q = 0; q < nw; ++q)
            if (sk[q] != kNoKey && better(sd[q], sk[q], bd, bk)) { bd = sd[q]; bk = sk[q]; }
        sd[0] = bd; sk[0] = bk;
    }
    __syncthreads();
    d = sd[0]; k = sk[0];
    __syncthreads();
}

// Per position i: P[i] = coord of order[i] (P[n] = P[0]), E[i] = d(order[i], order[i+1]), rem[L-1][i] of the row at i.
template <int WT, bool INT>
__global__ void k_or_prep(const double2 *__restrict__ coord, const int *__restrict__ orders, const OrState *__restrict__ st,
                          int n, double2 *__restrict__ Ps, double *__restrict__ Es, double *__restrict__ rems) {
    const int b = blockIdx.y;
    if (st[b].done) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const int *order = orders + (size_t)b * n;
    double2 *P = Ps + (size_t)b * (n + 1);
    if (i == n) { P[n] = coord[order[0]]; return; }
    const int v = order[i];
    P[i] = coord[v];
    const int pm = order[or_wrap(i - 1, n)], v1 = order[or_wrap(i + 1, n)];
    const double dpf = dnode<WT, INT>(coord, pm, v);
    const double e0 = dnode<WT, INT>(coord, v, v1);
    Es[(size_t)b * n + i] = e0;
    double *rem = rems + (size_t)b * 3 * n;
    // L = 1: l = v, s = v1
    rem[i] = (dpf + e0) - dnode<WT, INT>(coord, pm, v1);
    const int v2 = order[or_wrap(i + 2, n)], v3 = order[or_wrap(i + 3, n)];
    rem[n + i] = (dpf + dnode<WT, INT>(coord, v1, v2)) - dnode<WT, INT>(coord, pm, v2);
    rem[2 * n + i] = (dpf + dnode<WT, INT>(coord, v2, v3)) - dnode<WT, INT>(coord, pm, v3);
}

// Pair space over (row position u, column position k): lane l of a wave owns row position u = base + l and walks the
// columns of one chunk; D(u, k) is computed once and handed to lanes u+1 and u+2 (wave_shr:1, twice), so that with
// D(u, k-1) etc. kept from the previous column every distance feeds up to five deltas of the rows ending at u:
//     L = 1, row u:     fwd (D(u,j) + D(u,j+1))
//     L = 2, row u-1:   fwd (D(u-1,j) + D(u,j+1)),  rev (D(u,j) + D(u-1,j+1))
//     L = 3, row u-2:   fwd (D(u-2,j) + D(u,j+1)),  rev (D(u,j) + D(u-2,j+1))       (j = k - 1, the insertion edge)
// Partials: part[(chunk * 3 + L-1) * n + i] = best (delta, key) of row (i, L) over the chunk's columns.
// deltas_executed counts what the waves run: 5 expressions per lane and column, the lanes and expressions that own no row
// (lanes 62-63, the L = 2 / 3 expressions of lanes 0-1, the halo of the last row group) included -- about 1.04 x n(5n - 16)
// per full decision.
template <int WT, bool INT>
__global__ __launch_bounds__(256) void k_or_scan(const int *__restrict__ orders, OrState *__restrict__ st, int n, int CH,
                                                 const double2 *__restrict__ Ps, const double *__restrict__ Es,
                                                 const double *__restrict__ rems, OrBest *__restrict__ parts, int Cc) {
    const int b = blockIdx.z;
    if (st[b].done) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nrg = (n + kRowsPerWave - 1) / kRowsPerWave;
    const int rg = blockIdx.x * 4 + wave;
    if (rg >= nrg) return;
    const int chunk = blockIdx.y;
    const int c0 = chunk * CH, c1 = min(n, c0 + CH);
    if (c0 >= n) return;
    const int *order = orders + (size_t)b * n;
    const double2 *P = Ps + (size_t)b * (n + 1);
    const double *E = Es + (size_t)b * n;
    const double *rem = rems + (size_t)b * 3 * n;
    const int base = rg * kRowsPerWave;
    const int pu = (base + lane) % n;
    const double2 cu = P[pu];
    // the rows this lane decides: (u, 1), (u-1, 2), (u-2, 3), each when its start lies in [base, base + 62) and below n
    const int i1 = base + lane, i2 = i1 - 1, i3 = i1 - 2;
    const bool own1 = i1 >= base && i1 < base + kRowsPerWave && i1 < n;
    const bool own2 = i2 >= base && i2 < base + kRowsPerWave && i2 < n;
    const bool own3 = i3 >= base && i3 < base + kRowsPerWave && i3 < n;
    const int f1 = order[pu], f2 = order[or_wrap(pu - 1, n)], f3 = order[or_wrap(pu - 2, n)];
    const double r1 = rem[pu], r2 = rem[n + or_wrap(pu - 1, n)], r3 = rem[2 * n + or_wrap(pu - 2, n)];
    double bd1 = INFINITY, bd2 = INFINITY, bd3 = INFINITY;
    u64 bk1 = kNoKey, bk2 = kNoKey, bk3 = kNoKey;
    double p0, p1, p2;   // D(u, j), D(u-1, j), D(u-2, j)
    {
        const double2 c = P[c0];
        p0 = dist_xy<WT, INT>(cu.x, cu.y, c.x, c.y);
        p1 = shr1(p0);
        p2 = shr1(p1);
    }
    for (int k = c0 + 1; k <= c1; ++k) {
        const int j = k - 1;
        const double2 c = P[k];
        const double d0 = dist_xy<WT, INT>(cu.x, cu.y, c.x, c.y);
        const double d1 = shr1(d0), d2 = shr1(d1);
        const double e = E[j];
        // row (u-L+1, L) may not insert at j in {u-L .. u}
        int dj = pu - j;
        if (dj < 0) dj += n;
        const double a1 = ((p0 + d0) - e) - r1;
        const double a2 = ((p1 + d0) - e) - r2, b2 = ((p0 + d1) - e) - r2;
        const double a3 = ((p2 + d0) - e) - r3, b3 = ((p0 + d2) - e) - r3;
        const double lo = fmin(fmin(a1, a2), fmin(fmin(b2, a3), b3));
        if (__builtin_expect(lo < 0.0, 0)) {
            const int a = __builtin_nontemporal_load(order + j);
            if (dj > 1) offer(a1, or_key(f1, 1, a, 0, n), bd1, bk1);
            if (dj > 2) { offer(a2, or_key(f2, 2, a, 0, n), bd2, bk2); offer(b2, or_key(f2, 2, a, 1, n), bd2, bk2); }
            if (dj > 3) { offer(a3, or_key(f3, 3, a, 0, n), bd3, bk3); offer(b3, or_key(f3, 3, a, 1, n), bd3, bk3); }
        }
        p0 = d0; p1 = d1; p2 = d2;
    }
    OrBest *part = parts + (size_t)b * Cc * 3 * n;
    if (own1) part[(size_t)(chunk * 3 + 0) * n + i1] = OrBest{bd1, bk1};
    if (own2) part[(size_t)(chunk * 3 + 1) * n + i2] = OrBest{bd2, bk2};
    if (own3) part[(size_t)(chunk * 3 + 2) * n + i3] = OrBest{bd3, bk3};
    if (lane == 0) atomicAdd((unsigned long long *)&st[b].deltas, (unsigned long long)(5ull * 64ull * (unsigned)(c1 - c0)));
}

// best[(L-1) * n + f] = min over the chunks of row (pos f, L)
__global__ void k_or_rows(const int *__restrict__ orders, const OrState *__restrict__ st, int n, int Cc,
                          const OrBest *__restrict__ parts, OrBest *__restrict__ bests) {
    const int b = blockIdx.y;
    if (st[b].done) return;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= 3 * n) return;
    const int Lm = r / n, i = r - Lm * n;
    const OrBest *part = parts + (size_t)b * Cc * 3 * n;
    double bd = INFINITY; u64 bk = kNoKey;
    for (int c = 0; c < Cc; ++c) {
        const OrBest q = part[(size_t)(c * 3 + Lm) * n + i];
        if (q.k != kNoKey && better(q.d, q.k, bd, bk)) { bd = q.d; bk = q.k; }
    }
    bests[(size_t)b * 3 * n + (size_t)Lm * n + orders[(size_t)b * n + i]] = OrBest{bd, bk};
}

// Candidate deltas of row (f at position i, L) at insertion edge (a, bb); both orientations when L > 1.
template <int WT, bool INT>
__device__ __forceinline__ int row_edge(const double2 *coord, int n, int f, int l, int L, double rem, int a, int bb,
                                        double &bd, u64 &bk) {
    const double dab = dnode<WT, INT>(coord, a, bb);
    const double fwd = ((dnode<WT, INT>(coord, f, a) + dnode<WT, INT>(coord, l, bb)) - dab) - rem;
    offer(fwd, or_key(f, L, a, 0, n), bd, bk);
    if (L == 1) return 1;
    const double rev = ((dnode<WT, INT>(coord, l, a) + dnode<WT, INT>(coord, f, bb)) - dab) - rem;
    offer(rev, or_key(f, L, a, 1, n), bd, bk);
    return 2;
}

// After a move: list the rows to rescan, let every other row check its candidates on the move's new edges.
template <int WT, bool INT>
__global__ __launch_bounds__(256) void k_or_mark(const double2 *__restrict__ coord, const int *__restrict__ orders,
                                                 const int *__restrict__ poss, OrState *__restrict__ st, int n,
                                                 OrBest *__restrict__ bests, int *__restrict__ dirty) {
    const int b = blockIdx.y;
    OrState &S = st[b];
    if (S.done) return;
    __shared__ unsigned s_cnt;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < 3 * n) {
        const int *order = orders + (size_t)b * n, *pos = poss + (size_t)b * n;
        const int Lm = r / n, L = Lm + 1, f = r - Lm * n;
        const int i = pos[f];
        const int nchg = S.nchg, ntail = S.ntail;
        bool rescan = false;
        int win[5];
        for (int q = 0; q < L + 2; ++q) {   // p, x1 .. xL, s
            const int v = order[or_wrap(i - 1 + q, n)];
            win[q] = v;
            for (int c = 0; c < nchg; ++c) rescan = rescan || v == S.chg[c];
        }
        OrBest *best = bests + (size_t)b * 3 * n + r;
        OrBest cur = *best;
        if (!rescan && cur.k != kNoKey) {
            const int a = (int)((cur.k >> 1) % (u64)n);
            for (int c = 0; c < ntail; ++c) rescan = rescan || a == S.tail[c];
        }
        if (rescan) {
            dirty[(size_t)b * 3 * n + atomicAdd(&S.ndirty, 1)] = r;
        } else {
            const int p = win[0], l = win[L], s = win[L + 1];
            const double rem = (dnode<WT, INT>(coord, p, f) + dnode<WT, INT>(coord, l, s)) - dnode<WT, INT>(coord, p, s);
            unsigned cnt = 0;
            for (int c = 0; c < ntail; ++c) {
                const int a = S.tail[c];
                bool inside = false;
                for (int q = 0; q <= L; ++q) inside = inside || a == win[q];
                if (inside) continue;
                cnt += row_edge<WT, INT>(coord, n, f, l, L, rem, a, order[or_wrap(pos[a] + 1, n)], cur.d, cur.k);
            }
            if (cur.k != best->k) *best = cur;
            atomicAdd(&s_cnt, cnt);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd((unsigned long long *)&S.deltas, (unsigned long long)s_cnt);
}

// Rows listed by k_or_mark: every column, one workgroup per row (kRescanBlocks workgroups per tour share the list).
template <int WT, bool INT>
__global__ __launch_bounds__(256) void k_or_rescan(const double2 *__restrict__ coord, const int *__restrict__ orders,
                                                   const int *__restrict__ poss, OrState *__restrict__ st, int n,
                                                   OrBest *__restrict__ bests, const int *__restrict__ dirty) {
    const int b = blockIdx.y;
    OrState &S = st[b];
    if (S.done) return;
    __shared__ double sd[4];
    __shared__ u64 sk[4];
    const int *order = orders + (size_t)b * n, *pos = poss + (size_t)b * n;
    const int nd = S.ndirty;
    unsigned long long cnt = 0;
    for (int q = blockIdx.x; q < nd; q += gridDim.x) {
        const int r = dirty[(size_t)b * 3 * n + q];
        const int Lm = r / n, L = Lm + 1, f = r - Lm * n;
        const int i = pos[f];
        const int p = order[or_wrap(i - 1, n)], l = order[or_wrap(i + L - 1, n)], s = order[or_wrap(i + L, n)];
        const double rem = (dnode<WT, INT>(coord, p, f) + dnode<WT, INT>(coord, l, s)) - dnode<WT, INT>(coord, p, s);
        double bd = INFINITY; u64 bk = kNoKey;
        for (int j = threadIdx.x; j < n; j += blockDim.x) {
            int dj = j - (i - 1);    // in [-(n - 1), n]: j = n - 1 at i = 0 is p
            if (dj < 0) dj += n;
            else if (dj >= n) dj -= n;
            if (dj <= L) continue;   // a in {p, x1 .. xL}
            const int a = order[j], bb = order[j + 1 == n ? 0 : j + 1];
            cnt += row_edge<WT, INT>(coord, n, f, l, L, rem, a, bb, bd, bk);
        }
        block_argmin(bd, bk, sd, sk);
        if (threadIdx.x == 0) bests[(size_t)b * 3 * n + r] = OrBest{bd, bk};
    }
    // the lanes' counts: one atomic per wave
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd((unsigned long long *)&S.deltas, cnt);
}

// Decision over the 3n row bests, then the move: order/pos shift the shorter arc between the segment and the insertion
// point by L and take the segment in its orientation.  One workgroup per tour.
__global__ __launch_bounds__(kPickThreads) void k_or_pick_apply(int *__restrict__ orders, int *__restrict__ poss,
                                                                OrState *__restrict__ st, int n,
                                                                const OrBest *__restrict__ bests) {
    const int b = blockIdx.x;
    OrState &S = st[b];
    if (S.done) return;
    __shared__ double sd[kPickThreads / 64];
    __shared__ u64 sk[kPickThreads / 64];
    const int tid = threadIdx.x;
    if (S.max_moves >= 0 && S.moves >= S.max_moves) {
        if (tid == 0) S.done = 1;
        return;
    }
    const OrBest *best = bests + (size_t)b * 3 * n;
    double bd = INFINITY; u64 bk = kNoKey;
    for (int r = tid; r < 3 * n; r += kPickThreads) {
        const OrBest q = best[r];
        if (q.k != kNoKey && better(q.d, q.k, bd, bk)) { bd = q.d; bk = q.k; }
    }
    block_argmin(bd, bk, sd, sk);
    if (tid == 0) { S.sweeps += 1; if (bk == kNoKey) S.done = 1; }
    if (bk == kNoKey) return;
    int *order = orders + (size_t)b * n, *pos = poss + (size_t)b * n;
    const OrMove mv = or_unkey(bk, n);
    const int f = mv.f, L = mv.L, a = mv.a, o = mv.o;
    const int i = pos[f], ja = pos[a];
    int x[3];
    for (int q = 0; q < L; ++q) x[q] = order[or_wrap(i + q, n)];
    const int p = order[or_wrap(i - 1, n)], l = x[L - 1], s = order[or_wrap(i + L, n)], bb = order[or_wrap(ja + 1, n)];
    __syncthreads();   // every thread has read the tour before anything moves
    if (tid == 0) {
        int nt = 0, nc = 0;
        auto edge = [&](int u, int v) { S.tail[nt++] = u; S.chg[nc++] = u; S.chg[nc++] = v; };
        edge(p, s);
        if (o == 0) { edge(a, f); edge(l, bb); }
        else { edge(a, l); for (int q = 1; q < L; ++q) edge(x[q], x[q - 1]); edge(f, bb); }
        S.ntail = nt; S.nchg = nc; S.ndirty = 0;
        S.moves += 1; S.moves_len[L - 1] += 1; S.moves_rev += o;
        if (S.max_moves >= 0 && S.moves >= S.max_moves) S.done = 1;
    }
    or_shift_apply<kPickThreads>(order, pos, n, i, ja, L, o, x);
}

// Scratch of one (B, n): kept on the instance like the scratch tours handle.
struct OrScratch {
    int B = 0, n = 0, CH = 0, Cc = 0;
    OrState *d_st = nullptr;
    OrState *h_st = nullptr;   // pinned
    double2 *d_P = nullptr;
    double *d_E = nullptr, *d_rem = nullptr, *d_cost = nullptr;
    OrBest *d_part = nullptr, *d_best = nullptr;
    int *d_dirty = nullptr;
    ~OrScratch() {
        (void)hipFree(d_st); (void)hipHostFree(h_st); (void)hipFree(d_P); (void)hipFree(d_E); (void)hipFree(d_rem);
        (void)hipFree(d_cost); (void)hipFree(d_part); (void)hipFree(d_best); (void)hipFree(d_dirty);
    }
};

int scratch_alloc(OrScratch *x, int B, int n) {
    x->B = B; x->n = n;
    x->CH = std::max(512, (n + kMaxChunks - 1) / kMaxChunks);
    x->Cc = (n + x->CH - 1) / x->CH;
    const size_t Bn = (size_t)B * n;
    TSP_HIP_TRY(hipMalloc(&x->d_st, sizeof(OrState) * B));
    TSP_HIP_TRY(hipHostMalloc(&x->h_st, sizeof(OrState) * B, hipHostMallocDefault));
    TSP_HIP_TRY(hipMalloc(&x->d_P, sizeof(double2) * (Bn + B)));
    TSP_HIP_TRY(hipMalloc(&x->d_E, sizeof(double) * Bn));
    TSP_HIP_TRY(hipMalloc(&x->d_rem, sizeof(double) * 3 * Bn));
    TSP_HIP_TRY(hipMalloc(&x->d_cost, sizeof(double) * B));
    TSP_HIP_TRY(hipMalloc(&x->d_part, sizeof(OrBest) * 3 * Bn * x->Cc));
    TSP_HIP_TRY(hipMalloc(&x->d_best, sizeof(OrBest) * 3 * Bn));
    TSP_HIP_TRY(hipMalloc(&x->d_dirty, sizeof(int) * 3 * Bn));
    return TSP_OK;
}

void launch_full(tsp_dev_tours *t, OrScratch *x) {
    tsp_dev_inst *inst = t->inst;
    hipStream_t s = inst->ctx->stream;
    const int n = t->n, B = t->B;
    const int nrg = (n + kRowsPerWave - 1) / kRowsPerWave;
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_or_prep<WTC, INTC>), dim3((n + 1 + 255) / 256, B), dim3(256), 0, s, inst->d_coord, t->d_order,
                           x->d_st, n, x->d_P, x->d_E, x->d_rem);
        hipLaunchKernelGGL((k_or_scan<WTC, INTC>), dim3((nrg + 3) / 4, x->Cc, B), dim3(256), 0, s, t->d_order, x->d_st, n,
                           x->CH, x->d_P, x->d_E, x->d_rem, x->d_part, x->Cc);
    });
    hipLaunchKernelGGL(k_or_rows, dim3((3 * n + 255) / 256, B), dim3(256), 0, s, t->d_order, x->d_st, n, x->Cc, x->d_part,
                       x->d_best);
    hipLaunchKernelGGL(k_or_pick_apply, dim3(B), dim3(kPickThreads), 0, s, t->d_order, t->d_pos, x->d_st, n, x->d_best);
}

void launch_incremental(tsp_dev_tours *t, OrScratch *x) {
    tsp_dev_inst *inst = t->inst;
    hipStream_t s = inst->ctx->stream;
    const int n = t->n, B = t->B;
    TSP_DISPATCH_METRIC(inst->wtype, inst->integer_cost, {
        hipLaunchKernelGGL((k_or_mark<WTC, INTC>), dim3((3 * n + 255) / 256, B), dim3(256), 0, s, inst->d_coord, t->d_order,
                           t->d_pos, x->d_st, n, x->d_best, x->d_dirty);
        hipLaunchKernelGGL((k_or_rescan<WTC, INTC>), dim3(kRescanBlocks, B), dim3(256), 0, s, inst->d_coord, t->d_order,
                           t->d_pos, x->d_st, n, x->d_best, x->d_dirty);
    });
    hipLaunchKernelGGL(k_or_pick_apply, dim3(B), dim3(kPickThreads), 0, s, t->d_order, t->d_pos, x->d_st, n, x->d_best);
}

}  // namespace

void tsp_or_scratch_free(void *p) { delete static_cast<OrScratch *>(p); }

extern "C" {

int tsp_dev_or_opt(tsp_dev_inst *inst, int B, int *succ, int succ_stride, int64_t tour_stride, double *obj,
                   int64_t max_moves, double time_limit_s, tsp_or_opt_stats *stats) {
    if (!inst || !succ || !obj || B < 1 || succ_stride < 1) return TSP_DEV_E_ARG;
    const int n = inst->n;
    if (B > 1 && tour_stride < (int64_t)n * succ_stride) return TSP_DEV_E_ARG;
    Descent run;
    int rc = run.open(inst, B, succ, succ_stride, tour_stride, obj);
    if (rc) return rc;
    tsp_dev_tours *t = run.t;
    OrScratch *x = static_cast<OrScratch *>(inst->or_scratch);
    if (!x || x->B != B || x->n != n) {
        tsp_or_scratch_free(x);
        inst->or_scratch = nullptr;
        x = new OrScratch();
        rc = scratch_alloc(x, B, n);
        if (rc) { delete x; return rc; }
        inst->or_scratch = x;
    }
    const bool trivial = n < 5 || max_moves == 0;
    const bool full = TSP_SW(inst, OROPT_FULL, 0) == 1;
    // the first decision is a full one, the later ones work from what the move before them changed
    auto queue = [&](bool first) {
        if (first || full) launch_full(t, x);
        else launch_incremental(t, x);
    };
    const int status = run.run(x->d_st, x->h_st, x->d_cost, trivial, 128, max_moves, time_limit_s, queue);
    if (status != TSP_OK && status != TSP_TIME_LIMIT_EXCEEDED) return status;
    const long long N = n >= 5 ? (long long)n * (5LL * n - 16) : 0;
    for (int b = 0; b < B && stats; ++b) {
        const OrState &z = x->h_st[b];
        tsp_or_opt_stats &o = stats[b];
        memset(&o, 0, sizeof o);
        o.sweeps = z.sweeps; o.evals = z.sweeps * N; o.moves = z.moves;
        for (int q = 0; q < 3; ++q) o.moves_by_len[q] = z.moves_len[q];
        o.moves_reversed = z.moves_rev; o.deltas_executed = z.deltas;
        o.rounds = 0;
        o.seconds = wall_s() - run.t0; o.device_ms = run.device_ms;
    }
    return status;
}

int tsp_dev_two_opt_or_opt(tsp_dev_inst *inst, int two_opt_mode, int B, int *succ, int succ_stride, int64_t tour_stride,
                           double *obj, double time_limit_s, tsp_two_opt_stats *two_opt_stats, tsp_or_opt_stats *or_opt_stats) {
    if (!inst || !succ || !obj || B < 1 || succ_stride < 1) return TSP_DEV_E_ARG;
    if (two_opt_mode != TSP_2OPT_FIRST && two_opt_mode != TSP_2OPT_BEST) return TSP_DEV_E_ARG;
    const int n = inst->n;
    if (B > 1 && tour_stride < (int64_t)n * succ_stride) return TSP_DEV_E_ARG;
    {   // every tour is checked before any is touched
        std::vector<char> seen((size_t)n);
        for (int b = 0; b < B; ++b) {
            const int *sp = succ + (size_t)b * tour_stride;
            std::fill(seen.begin(), seen.end(), 0);
            int v = 0;
            for (int p = 0; p < n; ++p) {
                if (v < 0 || v >= n || seen[v]) return TSP_DEV_E_NOT_A_TOUR;
                seen[v] = 1;
                v = sp[(size_t)v * succ_stride];
            }
            if (v != 0) return TSP_DEV_E_NOT_A_TOUR;
        }
    }
    const double t0 = wall_s();
    int status = TSP_OK;
    for (int b = 0; b < B; ++b) {   // one tour at a time: the tours need different numbers of rounds
        int *sp = succ + (size_t)b * tour_stride;
        tsp_two_opt_stats acc2;
        tsp_or_opt_stats acco;
        memset(&acc2, 0, sizeof acc2);
        memset(&acco, 0, sizeof acco);
        double ms2 = 0.0;
        bool in_or_opt = false;   // the budget ran out in an Or-opt phase (which leaves the recomputed cost)
        for (;;) {
            double left = -1.0;
            if (time_limit_s > 0) {
                left = time_limit_s - (wall_s() - t0);
                if (left <= 0) { status = TSP_TIME_LIMIT_EXCEEDED; break; }
            }
            tsp_two_opt_stats s2;
            int rc = tsp_dev_two_opt(inst, two_opt_mode, TSP_ENGINE_AUTO, 1, sp, succ_stride, n, obj + b, left, &s2);
            if (rc < 0) return rc;
            acc2.sweeps += s2.sweeps; acc2.evals += s2.evals; acc2.moves += s2.moves; acc2.reversed += s2.reversed;
            acc2.pairs_scanned += s2.pairs_scanned; acc2.steps += s2.steps; ms2 += s2.device_ms;
            acc2.lane_pairs += s2.lane_pairs;
            if (rc == TSP_TIME_LIMIT_EXCEEDED) { status = rc; break; }
            if (time_limit_s > 0) {
                left = time_limit_s - (wall_s() - t0);
                if (left <= 0) { status = TSP_TIME_LIMIT_EXCEEDED; break; }
            }
            tsp_or_opt_stats so;
            rc = tsp_dev_or_opt(inst, 1, sp, succ_stride, n, obj + b, -1, left, &so);
            if (rc < 0) return rc;
            acco.sweeps += so.sweeps; acco.evals += so.evals; acco.moves += so.moves;
            for (int q = 0; q < 3; ++q) acco.moves_by_len[q] += so.moves_by_len[q];
            acco.moves_reversed += so.moves_reversed; acco.deltas_executed += so.deltas_executed;
            acco.device_ms += so.device_ms;
            acco.rounds += 1;
            if (rc == TSP_TIME_LIMIT_EXCEEDED) { status = rc; in_or_opt = true; break; }
            if (so.moves == 0) break;
        }
        if (status == TSP_TIME_LIMIT_EXCEEDED && !in_or_opt) {
            // stopped inside (or before) a 2-opt phase: the cost of the tour as it stands, recomputed
            tsp_or_opt_stats so;
            const int rc = tsp_dev_or_opt(inst, 1, sp, succ_stride, n, obj + b, 0, -1.0, &so);
            if (rc < 0) return rc;
        }
        if (two_opt_stats) {
            acc2.seconds = wall_s() - t0; acc2.device_ms = ms2;
            acc2.tier1_pairs = acc2.exact_pairs = acc2.staged_recs = -1;
            two_opt_stats[b] = acc2;
        }
        if (or_opt_stats) { acco.seconds = wall_s() - t0; or_opt_stats[b] = acco; }
        if (status == TSP_TIME_LIMIT_EXCEEDED) {
            // the remaining tours are left as they came, with their recomputed costs
            for (int c = b + 1; c < B; ++c) {
                int *sc = succ + (size_t)c * tour_stride;
                tsp_or_opt_stats so;
                const int rc = tsp_dev_or_opt(inst, 1, sc, succ_stride, n, obj + c, 0, -1.0, &so);
                if (rc < 0) return rc;
                if (two_opt_stats) { memset(&two_opt_stats[c], 0, sizeof(tsp_two_opt_stats)); }
                if (or_opt_stats) memset(&or_opt_stats[c], 0, sizeof(tsp_or_opt_stats));
            }
            break;
        }
    }
    return status;
}

}  // extern "C"
