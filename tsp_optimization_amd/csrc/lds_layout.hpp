// lds_layout.hpp -- the LDS engine's carve-up of a workgroup's dynamic LDS (two_opt_lds.hip): where each array of
// k_lds_two_opt starts and how many bytes a launch asks for.  Plain C++ for the host compiler and for hipcc: the kernel takes its
// pointers from lds_layout(), lds_bytes_needed takes its total from it, and tests/lds_layout_check.cpp compiles this very text.
//
// Offsets are bytes from the 16-byte aligned base of the dynamic LDS:
//   rows     32 row records (NodeRec, 48 bytes each; read as 16-byte words)
//   coord    n double2
//   order    n uint16
//   pos      n uint16
//   dsp      n float, edge length leaving tour position p -- only with the edge cache; padded up to 16 bytes before it
//   scratch  1 024 bytes of reduction scratch (doubles, 64-bit keys, int4 votes), padded up to 16 bytes before it
//   rowsf    32 float4, the block's rows as floats (fp32 first tier), directly behind the scratch
// Each pad is computed, not bounded: the total is exactly the last byte used + 1.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define TSP_LDSL_HD __host__ __device__ __forceinline__
#else
#define TSP_LDSL_HD inline
#endif

namespace tsp {

constexpr int kLdsLayoutRows = 32;            // rows of a block of the rows x columns scan
constexpr size_t kLdsRowRecBytes = 48;        // sizeof(NodeRec)
constexpr size_t kLdsCoordBytes = 16;         // sizeof(double2)
constexpr size_t kLdsIdxBytes = 2;            // sizeof(unsigned short)
constexpr size_t kLdsEdgeBytes = 4;           // sizeof(float)
constexpr size_t kLdsScratchBytes = 1024;
constexpr size_t kLdsRowFloatBytes = 16;      // sizeof(float4)

struct LdsLayout {
    size_t rows, coord, order, pos, dsp, scratch, rowsf;   // dsp == scratch without the edge cache (no bytes of its own)
    size_t total;
};

TSP_LDSL_HD size_t lds_up16(size_t x) { return (x + 15) & ~(size_t)15; }

TSP_LDSL_HD LdsLayout lds_layout(int n, bool edge_cache) {
    const size_t un = (size_t)n;
    LdsLayout l;
    l.rows = 0;
    l.coord = l.rows + kLdsRowRecBytes * kLdsLayoutRows;
    l.order = l.coord + kLdsCoordBytes * un;
    l.pos = l.order + kLdsIdxBytes * un;
    l.dsp = lds_up16(l.pos + kLdsIdxBytes * un);
    l.scratch = edge_cache ? lds_up16(l.dsp + kLdsEdgeBytes * un) : l.dsp;
    l.rowsf = l.scratch + kLdsScratchBytes;
    l.total = l.rowsf + kLdsRowFloatBytes * kLdsLayoutRows;
    return l;
}

// the largest n whose layout fits `lds_bytes` (0: none does); the total is non-decreasing in n
inline int lds_layout_max_n(size_t lds_bytes, bool edge_cache) {
    int lo = 0, hi = 1 << 20;
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (lds_layout(mid, edge_cache).total <= lds_bytes) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace tsp
