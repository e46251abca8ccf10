// or_opt_shift.hpp -- the Or-opt move on order/pos, shared by k_or_pick_apply (or_opt.hip) and k_nl_pick_apply (nl_opt.hip).
#pragma once
#include "two_opt_common.hpp"

namespace tsp {

__device__ __forceinline__ int or_wrap(int x, int n) { return x >= n ? x - n : (x < 0 ? x + n : x); }

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
