// Micro-benchmark: what one exact integer-root distance of the exhaustive sweep (two_opt_exh.hpp: exh_dist) costs a SIMD, in
// cycles per wave, for several ways of rounding the raw root, plus the conversion instructions on their own.
// 4 waves per SIMD, 8 independent columns per lane, no memory traffic in the loop.
// `dist verify`: the seed form of csrc/exh_arith.hpp (the header's own text) with the HARDWARE v_sqrt_f32, for every k in
// 0 .. 2^21 - 2 and every s on and beside the rounding boundaries of the three metrics, against integer arithmetic on the
// device; prints the number of cases and of mismatches (0 required).  A tool run once, not a test.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include "../../tsp_optimization_amd/csrc/exh_arith.hpp"
#pragma clang fp contract(off)

#define ITER 4096
template <int V>
__device__ __forceinline__ int dist(double cx, double cy, double rx, double ry) {
    const double dx = cx - rx, dy = cy - ry;
    const double s = __builtin_fma(dx, dx, dy * dy);
    const double g = __builtin_amdgcn_sqrt(s);
    if (V == 0) {          // floor + cvt (the first form)
        const double k = floor(g + 0.25);
        const double e = __builtin_fma(-k, k, s);
        return __double2int_rz(k) + (e > k ? 1 : 0);
    } else if (V == 1) {   // magic constant: the integer falls out of the low word, no floor, no cvt
        const double t = (g - 0.25) + 6755399441055744.0;   // 1.5 * 2^52: round to nearest integer
        const double k = t - 6755399441055744.0;
        const double e = __builtin_fma(-k, k, s);
        return __double2loint(t) + (e > k ? 1 : 0);
    } else if (V == 2) {   // rndne + cvt
        const double k = rint(g - 0.25);
        const double e = __builtin_fma(-k, k, s);
        return __double2int_rz(k) + (e > k ? 1 : 0);
    } else if (V == 3) {   // no fix-up at all (not exact: the floor of the issue cost)
        return __double2loint(g + 6755399441055744.0);
    } else if (V == 4) {   // f32 seed: s rounded to f32, v_sqrt_f32, two-sided fix-up in f64
        const float gf = __builtin_amdgcn_sqrtf((float)s);
        const double t = (double)gf + 6755399441055744.0;
        const double k = t - 6755399441055744.0;
        const double e = __builtin_fma(-k, k, s);           // s - k^2
        return __double2loint(t) + (e > k ? 1 : 0) - (e < -k ? 1 : 0);
    } else if (V == 5) {   // f32 seed under the ONE-sided fix-up, the rest as k_exh had it: floor and cvt_i32 in f64
        const double k = floor((double)__builtin_amdgcn_sqrtf((float)s));
        const double e = __builtin_fma(-k, k, s);
        return __double2int_rz(k) + (e > k ? 1 : 0);
    } else if (V == 6) {   // the shortened chain, NINT: cvt_f32_f64, sqrt_f32, cvt_i32_f32, cvt_f64_i32, fma, cmp, addc
        return tsp::exh_seed_round<tsp::EXH_NINT>(s, __builtin_amdgcn_sqrtf(tsp::exh_seed_arg<tsp::EXH_NINT>(s)));
    } else if (V == 7) {   // the shortened chain, CEIL: v_rndne_f32 before the cvt_i32_f32
        return tsp::exh_seed_round<tsp::EXH_CEIL>(s, __builtin_amdgcn_sqrtf(tsp::exh_seed_arg<tsp::EXH_CEIL>(s)));
    } else {               // the shortened chain, ATT: as CEIL, with s * 0.1 before the root and -10 k in the residual
        return tsp::exh_seed_round<tsp::EXH_ATT>(s, __builtin_amdgcn_sqrtf(tsp::exh_seed_arg<tsp::EXH_ATT>(s)));
    }
}

// ---- verify: one thread per k; s = k^2 + k + d, k^2 + d, 10 k^2 + d, 10 k^2 + 5 k + d (d = -1 .. 2), three metrics, wherever the
// root stays below 2^21.  The wanted integer is tested, not computed: d = nint(sqrt s) iff d^2 - d < s <= d^2 + d;
// d = ceil(sqrt s) iff (d - 1)^2 < s <= d^2; ATT: 10 (d - 1)^2 < s <= 10 d^2 (s = 0: d = 0) -- 64-bit integers throughout.
__device__ __forceinline__ bool root_ok(int mode, long long s, long long d) {
    if (d < 0) return false;
    if (d == 0) return s == 0;
    if (mode == tsp::EXH_NINT) return d * d - d < s && s <= d * d + d;
    if (mode == tsp::EXH_CEIL) return (d - 1) * (d - 1) < s && s <= d * d;
    return 10 * (d - 1) * (d - 1) < s && s <= 10 * d * d;
}
template <int MODE>
__device__ __forceinline__ int seed_root(long long s) {
    const double sd = (double)s;
    return tsp::exh_seed_round<MODE>(sd, __builtin_amdgcn_sqrtf(tsp::exh_seed_arg<MODE>(sd)));
}
__global__ __launch_bounds__(256) void k_verify(unsigned long long *out, long long kmax) {
    const long long kk = (long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long cases = 0, bad = 0;
    if (kk <= kmax) {
        const long long lim = (kmax + 1) * (kmax + 1);
        const long long base[4] = {kk * kk + kk, kk * kk, 10 * kk * kk, 10 * kk * kk + 5 * kk};
        for (int b = 0; b < 4; ++b)
            for (int d = -1; d <= 2; ++d) {
                const long long s = base[b] + d;
                if (s < 0) continue;
                if (s <= lim) {
                    cases += 2;
                    bad += !root_ok(tsp::EXH_NINT, s, seed_root<tsp::EXH_NINT>(s));
                    bad += !root_ok(tsp::EXH_CEIL, s, seed_root<tsp::EXH_CEIL>(s));
                }
                if (s <= 10 * lim) {
                    cases += 1;
                    bad += !root_ok(tsp::EXH_ATT, s, seed_root<tsp::EXH_ATT>(s));
                }
            }
    }
    if (cases) { atomicAdd(&out[0], cases); atomicAdd(&out[1], bad); }
}
static int verify() {
    const long long kmax = (1ll << 21) - 2;
    const int blocks = (int)((kmax + 256) / 256);   // one thread per k in 0 .. kmax, the last block partly idle (kk <= kmax)
    unsigned long long *d, h[2] = {0, 0};
    if (hipMalloc(&d, sizeof(h)) != hipSuccess || hipMemset(d, 0, sizeof(h)) != hipSuccess) return 2;
    hipLaunchKernelGGL(k_verify, dim3(blocks), dim3(256), 0, 0, d, kmax);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 2;
    printf("verify (hardware v_sqrt_f32, seed form of exh_arith.hpp): k = 0 .. %lld, cases=%llu mismatches=%llu\n", kmax, h[0], h[1]);
    return h[1] == 0 ? 0 : 1;
}

template <int V>
__global__ __launch_bounds__(256) void k(int *out, double seed) {
    double cx[8], cy[8];
    int acc[8];
    for (int q = 0; q < 8; ++q) { cx[q] = seed * 1000 + threadIdx.x * 37 + q * 1001; cy[q] = seed * 777 + threadIdx.x * 11 + q * 313; acc[q] = 0; }
    double rx = seed, ry = seed * 2;
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += dist<V>(cx[q], cy[q], rx, ry);
        rx += 3.0; ry += 5.0;
    }
    int s = 0;
    for (int q = 0; q < 8; ++q) s += acc[q];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int OP>
__global__ __launch_bounds__(256) void kop(double *out, double seed) {
    double a[8];
    int i[8];
    for (int q = 0; q < 8; ++q) { a[q] = seed + threadIdx.x * 1e-3 + q; i[q] = threadIdx.x + q; }
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (OP == 0) a[q] = floor(a[q]) + 1.5;                                   // v_floor_f64 + add
            if (OP == 1) { i[q] += __double2int_rz(a[q]); a[q] += 1.5; }            // v_cvt_i32_f64 + add_u32 + add_f64
            if (OP == 2) a[q] = a[q] + 1.5;                                          // add alone
            if (OP == 3) { a[q] = (double)i[q] + a[q]; i[q] += 3; }                  // v_cvt_f64_i32 + add_f64 + add_u32
            if (OP == 4) { i[q] += (a[q] > 3.0) ? 1 : 0; a[q] += 1.5; }              // v_cmp_gt_f64 + addc + add_f64
            if (OP == 5) { i[q] = min(min(i[q] + 3, i[(q + 1) & 7]), i[(q + 2) & 7]); }   // add + min3
            if (OP == 6) a[q] = rint(a[q]) + 1.5;                                    // v_rndne_f64 + add
            if (OP == 7) { a[q] = (double)(float)a[q] + 1.5; }                       // cvt_f32_f64 + cvt_f64_f32 + add
        }
    }
    double s = 0;
    for (int q = 0; q < 8; ++q) s += a[q] + i[q];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <typename F>
double timeit(F launch) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    launch();
    hipEventRecord(e0);
    launch();
    hipEventRecord(e1); hipEventSynchronize(e1);
    float ms; hipEventElapsedTime(&ms, e0, e1);
    return ms;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "verify")) return verify();
    const int blocks = 256 * 4;   // 4 waves per SIMD
    void *d; hipMalloc(&d, 8 * blocks * 256);
    const double per_simd = 4.0 * ITER * 8;   // wave-level calls per SIMD
    const char *names[] = {"floor + cvt_i32 (first form)", "magic constant (no floor, no cvt)", "rndne + cvt_i32", "no fix-up (not exact)", "f32 seed, two-sided fix-up",
                           "f32 seed, one-sided, floor + cvt_i32", "f32 seed, short chain, NINT", "f32 seed, short chain, CEIL (rint)",
                           "f32 seed, short chain, ATT (rint)"};
    double ms[9];
    ms[0] = timeit([&] { hipLaunchKernelGGL(k<0>, dim3(blocks), dim3(256), 0, 0, (int *)d, 3.0); });
    ms[1] = timeit([&] { hipLaunchKernelGGL(k<1>, dim3(blocks), dim3(256), 0, 0, (int *)d, 3.0); });
    ms[2] = timeit([&] { hipLaunchKernelGGL(k<2>, dim3(blocks), dim3(256), 0, 0, (int *)d, 3.0); });
    ms[3] = timeit([&] { hipLaunchKernelGGL(k<3>, dim3(blocks), dim3(256), 0, 0, (int *)d, 3.0); });
    ms[4] = timeit([&] { hipLaunchKernelGGL(k<4>, dim3(blocks), dim3(256), 0, 0, (int *)d, 3.0); });
    ms[5] = timeit([&] { hipLaunchKernelGGL(k<5>, dim3(blocks), dim3(256), 0, 0, (int *)d, 3.0); });
    ms[6] = timeit([&] { hipLaunchKernelGGL(k<6>, dim3(blocks), dim3(256), 0, 0, (int *)d, 3.0); });
    ms[7] = timeit([&] { hipLaunchKernelGGL(k<7>, dim3(blocks), dim3(256), 0, 0, (int *)d, 3.0); });
    ms[8] = timeit([&] { hipLaunchKernelGGL(k<8>, dim3(blocks), dim3(256), 0, 0, (int *)d, 3.0); });
    for (int v = 0; v < 9; ++v) printf("exact distance, %-36s %8.3f ms  %6.1f cycles per wave-distance (2.4 GHz nominal)\n", names[v], ms[v], ms[v] * 1e-3 * 2.4e9 / per_simd);
    const char *on[] = {"v_floor_f64 + add_f64", "v_cvt_i32_f64 + add_u32 + add_f64", "v_add_f64", "v_cvt_f64_i32 + add_f64 + add_u32", "v_cmp_gt_f64 + addc + add_f64", "add_u32 + min3_i32", "v_rndne_f64 + add_f64", "cvt_f32_f64 + cvt_f64_f32 + add_f64"};
    double mo[8];
    mo[0] = timeit([&] { hipLaunchKernelGGL(kop<0>, dim3(blocks), dim3(256), 0, 0, (double *)d, 3.0); });
    mo[1] = timeit([&] { hipLaunchKernelGGL(kop<1>, dim3(blocks), dim3(256), 0, 0, (double *)d, 3.0); });
    mo[2] = timeit([&] { hipLaunchKernelGGL(kop<2>, dim3(blocks), dim3(256), 0, 0, (double *)d, 3.0); });
    mo[3] = timeit([&] { hipLaunchKernelGGL(kop<3>, dim3(blocks), dim3(256), 0, 0, (double *)d, 3.0); });
    mo[4] = timeit([&] { hipLaunchKernelGGL(kop<4>, dim3(blocks), dim3(256), 0, 0, (double *)d, 3.0); });
    mo[5] = timeit([&] { hipLaunchKernelGGL(kop<5>, dim3(blocks), dim3(256), 0, 0, (double *)d, 3.0); });
    mo[6] = timeit([&] { hipLaunchKernelGGL(kop<6>, dim3(blocks), dim3(256), 0, 0, (double *)d, 3.0); });
    mo[7] = timeit([&] { hipLaunchKernelGGL(kop<7>, dim3(blocks), dim3(256), 0, 0, (double *)d, 3.0); });
    for (int v = 0; v < 8; ++v) printf("%-40s %8.3f ms  %6.1f cycles per wave-iteration\n", on[v], mo[v], mo[v] * 1e-3 * 2.4e9 / per_simd);
    return 0;
}
