// ils_common.hpp -- the counter-based random stream and the cuts of the double-bridge kick, shared by ils.hip (one kick per chain
// on the whole tour) and seg_ils.hip (one kick per window).  The definitions are in include/tsp_hip.h.
#pragma once
#include "two_opt_common.hpp"

namespace tsp {

__host__ __device__ __forceinline__ u64 ils_mix(u64 x) {
    x += 0x9E3779B97F4A7C15ull;
    u64 z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the ILS base of chain b at iteration `it`
__host__ __device__ __forceinline__ u64 ils_base(u64 seed, int b, long long it) {
    return ils_mix(ils_mix(seed ^ ((u64)b * 0x100000001B3ull)) + (u64)it);
}

struct IlsCuts {
    int s, o1, o2, o3, o4;
};
// The cuts 1 <= o1 < o2 < o3 < o4 <= W of a kick within W >= 8 nodes of the anchor s, from the four draws u1 .. u4.
__host__ __device__ __forceinline__ IlsCuts ils_cuts_from(int s, int W, u64 u1, u64 u2, u64 u3, u64 u4) {
    IlsCuts c;
    c.s = s;
    c.o1 = 1 + (int)(u1 % (u64)(W - 3));
    c.o2 = c.o1 + 1 + (int)(u2 % (u64)(W - 2 - c.o1));
    c.o3 = c.o2 + 1 + (int)(u3 % (u64)(W - 1 - c.o2));
    c.o4 = c.o3 + 1 + (int)(u4 % (u64)(W - c.o3));
    return c;
}

}  // namespace tsp
