// or_opt_shift.hpp -- the Or-opt move, its key and its shift on order/pos, shared by or_opt.hip and the list descent (nl_opt.hip).
#pragma once
#include "two_opt_common.hpp"

namespace tsp {

__device__ __forceinline__ int or_wrap(int x, int n) { return x >= n ? x - n : (x < 0 ? x + n : x); }

// an improving candidate replaces the held one when it is the smaller (delta, key)
__device__ __forceinline__ void offer(double delta, u64 key, double &bd, u64 &bk) {
    if (delta < 0.0 && better(delta, key, bd, bk)) { bd = delta; bk = key; }
}

// The move (f, L, a, o) -- segment of L nodes from f, between a and succ a, o = 1: reversed -- as a key, node ids not positions.
struct OrMove {
    int f, L, a, o;
};
__device__ __forceinline__ u64 or_key(int f, int L, int a, int o, int n) {
    return (u64)((((long long)f * 3 + (L - 1)) * n + a) * 2 + o);
}
__device__ __forceinline__ OrMove or_unkey(u64 key, int n) {
    const u64 t = key >> 1;
    const int fl = (int)(t / (u64)n);
    return OrMove{fl / 3, fl % 3 + 1, (int)(t % (u64)n), (int)(key & 1)};
}

// Segment x[0 .. L-1] at positions i .. i+L-1 goes between position ja and ja + 1 (o = 1: reversed): order/pos shift the
// shorter arc between the segment and the insertion point by L and take the segment in its orientation.  Called by every
// thread of the one workgroup (NT threads) that owns the tour, after a barrier behind the last read of the old tour.
template <int NT>
__device__ __forceinline__ void or_shift_apply(int *__restrict__ order, int *__restrict__ pos, int n, int i, int ja, int L, int o,
                                               const int (&x)[3]) {
    const int tid = threadIdx.x;
    int m1 = ja - (i + L);
    if (m1 < 0) m1 += n;
    m1 += 1;                      // nodes s .. a
    const int m2 = n - L - m1;    // nodes b .. p
    int seg0;
    if (m1 <= m2) {   // s .. a move back by L (ascending chunks: a chunk's writes lie below every later chunk's reads)
        for (int t0 = 0; t0 < m1; t0 += NT) {
            const int q = t0 + tid;
            const int v = q < m1 ? order[or_wrap(i + L + q, n)] : -1;
            __syncthreads();
            if (v >= 0) { const int np = or_wrap(i + q, n); order[np] = v; pos[v] = np; }
            __syncthreads();
        }
        seg0 = i + m1;
    } else {          // b .. p move on by L (descending chunks)
        for (int t0 = ((m2 - 1) / NT) * NT; t0 >= 0; t0 -= NT) {
            const int q = t0 + tid;
            const int v = q < m2 ? order[or_wrap(ja + 1 + q, n)] : -1;
            __syncthreads();
            if (v >= 0) { const int np = or_wrap(ja + 1 + L + q, n); order[np] = v; pos[v] = np; }
            __syncthreads();
        }
        seg0 = ja + 1;
    }
    if (tid < L) {
        const int v = o ? x[L - 1 - tid] : x[tid];
        const int np = or_wrap(seg0 + tid, n);
        order[np] = v; pos[v] = np;
    }
}

}  // namespace tsp
