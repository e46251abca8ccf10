// exh_arith.hpp -- the arithmetic of the exhaustive sweep's distances (two_opt_exh.hpp), free of HIP: k_move_pos and k_exh
// compile exactly this text for the device, tests/test_cpu_exh_arith.py compiles it with the host compiler and checks it against
// integer arithmetic.  Every function is an exact integer identity on its stated domain; none of them rounds.  The layout of the
// strips (exh_strip), the dealing of their rows to the waves (exh_deal, at the end; tests/test_cpu_exh_deal.py) and the rule by
// which k_move_pos permutes the records of one sweep into those of the next (exh_perm; tests/test_cpu_exh_permute.py) live here
// for the same reason.
//
// Squared distance from norms.  Positions are stored relative to one node of the instance, so every coordinate is an integer
// of magnitude < 2^21 (the *_ICOORD metrics bound the instance's diagonal; the pads lie at -6e6).  With the record
// (-2x, -2y, x^2 + y^2) of the row's position,
//     s = cx * (-2 rx) + (cy * (-2 ry) + (cn + rn))  =  (cx - rx)^2 + (cy - ry)^2:
// every operand and every partial result is an integer below 2^53 (norms < 2^43 for instance positions, 1.4e14 with a pad), so
// the add and the two fmas are exact and s is the same number as dx * dx + dy * dy -- in three instructions instead of four.
//
// Integer root.  g is the hardware's approximate root of s (of s / 10 for ATT), |g - r| < 0.25 for the true root r < 2^21
// (tsp_dist.hpp).  Rounding g itself -- no constant added first -- leaves the wanted integer at k or k + 1:
//   EUC_2D   k = floor(g):  r in (k - 0.25, k + 1.25), so nint(r) is k or k + 1, and it is k + 1 iff s > k^2 + k;
//   CEIL_2D  k = rint(g):   r in (k - 0.75, k + 0.75), so ceil(r) is k or k + 1, and it is k + 1 iff s > k^2;
//   ATT      the same with r = sqrt(s / 10) and s > 10 k^2.
// The residual e = s - k^2 (s - 10 k^2) is exact in fp64, one fma.  The margin on g is 0.5 on either side.
#pragma once

#if defined(__HIPCC__)
#define TSP_EXH_HD __host__ __device__ __forceinline__
#else
#define TSP_EXH_HD inline
#endif

namespace tsp {

enum : int { EXH_NINT = 0, EXH_CEIL = 1, EXH_ATT = 2 };

// what one position contributes as a ROW of the sweep: 32 bytes, so that a batch of rows is one aligned scalar load
struct alignas(32) ExhRec {
    double m2x, m2y;   // -2 x, -2 y (relative coordinates)
    double nrm;        // x^2 + y^2
    int eprev;         // length of the tour edge that ENDS at this position: d(u_{p-1}, u_p); 0 at position 0 and on the pads
    int id;            // the node at this position (position n repeats position 0; -1 on the pads)
};

TSP_EXH_HD void exh_rec_xy(double x, double y, ExhRec &r) {
    r.m2x = -2.0 * x;
    r.m2y = -2.0 * y;
    r.nrm = __builtin_fma(x, x, y * y);   // exact: integers, the sum < 2^53
}

// the column's own coordinate back from its record (exact: a power of two)
TSP_EXH_HD double exh_col(double m2) { return -0.5 * m2; }

TSP_EXH_HD double exh_s(double cx, double cy, double cn, double rm2x, double rm2y, double rn) {
    return __builtin_fma(cx, rm2x, __builtin_fma(cy, rm2y, cn + rn));
}

// the argument of the hardware root
template <int MODE>
TSP_EXH_HD double exh_root_arg(double s) { return MODE == EXH_ATT ? s * 0.1 : s; }

// the four stages after the root; k_exh issues each of them for all columns of a lane before the next
template <int MODE>
TSP_EXH_HD double exh_k(double g) { return MODE == EXH_NINT ? __builtin_floor(g) : __builtin_rint(g); }

template <int MODE>
TSP_EXH_HD double exh_e(double s, double k) { return __builtin_fma(MODE == EXH_ATT ? -10.0 * k : -k, k, s); }

template <int MODE>
TSP_EXH_HD bool exh_up(double k, double e) { return MODE == EXH_NINT ? e > k : e > 0.0; }

TSP_EXH_HD int exh_ki(double k) { return (int)k; }

TSP_EXH_HD int exh_d(int ki, bool up) { return ki + (up ? 1 : 0); }

// the integer-valued distance of tsp_dist.hpp's int_root from s and the approximate root g of exh_root_arg(s)
template <int MODE>
TSP_EXH_HD int exh_round(double s, double g) {
    const double k = exh_k<MODE>(g);
    return exh_d(exh_ki(k), exh_up<MODE>(k, exh_e<MODE>(s, k)));
}

// ---- the seed form: the same integer from an fp32 root (what k_exh computes; tests/test_cpu_exh_seed.py) ------------------------
// The one-sided fix-up above needs the seed within 0.5 of the true root r, not 0.25, and that an fp32 root delivers: the
// argument rounded to fp32 (2^-25 relative, 2^-26 in the root) and the root instruction's own error (1 ulp) leave the seed
// within 1.25 fp32 ulps of r, and below 2^21 an ulp is at most 0.125.  (Checked with the seed moved by +-2 ulps: exact for every
// root below 2^21, and no further -- at 2^21 the ulp is 0.25 and +-2 ulps reach the 0.5.)  s = 0 gives the seed 0 and k = 0.
// The integer root then comes straight out of the fp32 value and ONE conversion feeds the residual, which is the fp64 fma of
// the form above -- exact --, so no fp64 root, no fp64 rounding and no fp64-to-integer conversion is left:
//   cvt_f32_f64 -> sqrt_f32 -> cvt_i32_f32 (NINT: truncation = floor, g >= 0; CEIL / ATT: of rint(g)) -> cvt_f64_i32 -> fma ->
//   compare -> add-with-carry.
// gf is the approximate fp32 root of exh_seed_arg(s).
template <int MODE>
TSP_EXH_HD float exh_seed_arg(double s) { return (float)exh_root_arg<MODE>(s); }

template <int MODE>
TSP_EXH_HD int exh_seed_ki(float gf) { return MODE == EXH_NINT ? (int)gf : (int)__builtin_rintf(gf); }

TSP_EXH_HD double exh_seed_k(int ki) { return (double)ki; }

// residual, compare and final add are exh_e, exh_up and exh_d of the form above
template <int MODE>
TSP_EXH_HD int exh_seed_round(double s, float gf) {
    const int ki = exh_seed_ki<MODE>(gf);
    const double k = exh_seed_k(ki);
    return exh_d(ki, exh_up<MODE>(k, exh_e<MODE>(s, k)));
}

// the same distance from two records (the first one as the column): what k_exh computes for a pair of positions, and what
// k_move_pos computes at a cut point of a move.  root(v) is the approximate root of v: the hardware's on the device.
template <int MODE, class Root>
TSP_EXH_HD int exh_dist_recs(const ExhRec &c, const ExhRec &r, Root root) {
    const double s = exh_s(exh_col(c.m2x), exh_col(c.m2y), c.nrm, r.m2x, r.m2y, r.nrm);
    return exh_round<MODE>(s, root(exh_root_arg<MODE>(s)));
}

// ---- the records of the tour AFTER a 2-opt move, by permutation of the records before it ------------------------------------
// The move reverses the L positions pa1 .. pa1 + L - 1 (cyclic) of a tour of n positions: the node at new position p is the node
// at old position exh_mirror(p) (an involution; MoveView of two_opt_step.hpp is this function).
TSP_EXH_HD int exh_mirror(int p, int n, int pa1, int L) {
    int t = p - pa1; if (t < 0) t += n;
    if (t >= L) return p;
    int q = pa1 + (L - 1 - t); if (q >= n) q -= n;
    return q;
}

// New position k in [0, n] (position n repeats position 0): a = mirror((k - 1) mod n) and b = mirror(k mod n) are old positions.
// The new record takes -2x, -2y, the norm and the id from old record b; its eprev is
//   EXH_E_ZERO  0: position 0 has no edge before it;
//   EXH_E_B     old record b's, when b = a + 1 (mod n) and b > 0: the same edge, walked the same way;
//   EXH_E_A     old record a's, when a = b + 1 (mod n) and a > 0: the same edge, walked the other way (inside the segment);
//   EXH_E_WRAP  old record n's -- the closing edge, d(u_{n-1}, u_0) --, when the pair is (n - 1, 0) in either direction;
//   EXH_E_CUT   exh_dist_recs of old records a and b: a new edge, two per move (none when L = n - 1: the segment's ends
//               were neighbours already, and the rules above find their old edge).
// Every case names an OLD EDGE between the two nodes or computes the distance, so the value is right whichever rule matches.
// Positions past n are pads: copied (a = b = k).  A thread therefore needs old records a and b and old record n's eprev: three
// loads whose addresses depend on the move alone, one round.
enum : int { EXH_E_ZERO = 0, EXH_E_B = 1, EXH_E_A = 2, EXH_E_WRAP = 3, EXH_E_CUT = 4 };
struct ExhPerm { int a, b, e; };
TSP_EXH_HD ExhPerm exh_perm(int k, int n, int pa1, int L) {
    if (k > n) return {k, k, EXH_E_B};
    const int km = k == n ? 0 : k;
    const int a = exh_mirror(km == 0 ? n - 1 : km - 1, n, pa1, L), b = exh_mirror(km, n, pa1, L);
    int e = EXH_E_CUT;
    if (k == 0) e = EXH_E_ZERO;
    else if (b == (a + 1 == n ? 0 : a + 1)) e = b > 0 ? EXH_E_B : EXH_E_WRAP;
    else if (a == (b + 1 == n ? 0 : b + 1)) e = a > 0 ? EXH_E_A : EXH_E_WRAP;
    return {a, b, e};
}

template <int MODE, class Root>
TSP_EXH_HD ExhRec exh_perm_rec(const ExhPerm &pm, const ExhRec &ra, const ExhRec &rb, int wrap_eprev, Root root) {
    ExhRec r = rb;
    r.eprev = pm.e == EXH_E_ZERO ? 0
            : pm.e == EXH_E_B    ? rb.eprev
            : pm.e == EXH_E_A    ? ra.eprev
            : pm.e == EXH_E_WRAP ? wrap_eprev
                                 : exh_dist_recs<MODE>(ra, rb, root);
    return r;
}

// The strips of pair-columns, right-aligned: strip s holds the D-columns q0 .. q0 + weff of its wave and the pair-rows
// p' < rows.  The slack strips * weff - n sits in strip 0 (rows from the unclamped q0; q0 itself clamped to 0, so strip 0
// overlaps strip 1: a pair evaluated twice cannot change an arg-min whose tie-break is strict).  The kernel walks the strips
// with exh_strip; the host (tsp_dev_tours_create's shares, exh_deal) counts the row units with these.
struct ExhStrip { int q0, rows; };
TSP_EXH_HD int exh_strips(int n, int weff) { return (n + weff - 1) / weff; }
TSP_EXH_HD ExhStrip exh_strip(int n, int weff, int s) {
    const int q0 = s * weff - (exh_strips(n, weff) * weff - n);
    return {q0 < 0 ? 0 : q0, q0 + weff - 1 < n - 1 ? q0 + weff - 1 : n - 1};
}
TSP_EXH_HD long long exh_total_rows(int n, int weff) {
    long long total = 0;
    for (int s = 0, ns = exh_strips(n, weff); s < ns; ++s) total += exh_strip(n, weff, s).rows;
    return total;
}

// The dealing.  The row units of all strips, laid end to end (strip 0 first), go to the waves of a tour's grid in contiguous
// ranges, in wave order: equal shares of ceil(total / waves_total) units, or -- share[0] > 0 and gens > 0 -- the grid in `gens`
// parts of waves_total / gens waves (the last part takes the remainder of that division) whose waves get share[part] units each
// (tsp_dev_tours_create: the older a workgroup on its CU, the larger its share).  Every input is fixed when the tours handle is
// created, so the host evaluates this once per wave into a table and k_exh loads its entry: the sum over the strips, the 64-bit
// division and the search for the first strip are not on the kernel's start-up path.
// A wave's range: `count` units from row `row` of strip `strip`, running on into the following strips from their row 0 (it may
// cover several whole strips).  count == 0: nothing to do (strip = row = 0).
struct alignas(16) ExhDeal {
    int strip, row;
    long long count;
};
TSP_EXH_HD ExhDeal exh_deal(int n, int weff, int waves_total, const int (&share)[4], int gens, int gw) {
    const long long total = exh_total_rows(n, weff);
    long long per = (total + waves_total - 1) / waves_total;
    long long u_lo = per * gw;
    if (share[0] > 0 && gens > 0) {
        const int wq = waves_total / gens, g = gens - 1 < gw / wq ? gens - 1 : gw / wq, idx = gw - g * wq;
        u_lo = 0;
        for (int q = 0; q < g; ++q) u_lo += (long long)share[q] * wq;
        per = share[g];
        u_lo += per * idx;
    }
    const long long u_hi = total < u_lo + per ? total : u_lo + per;
    ExhDeal d = {0, 0, 0};
    if (u_lo >= u_hi) return d;
    long long cum = 0;
    int s = 0;
    for (;; ++s) {   // the strip that holds unit u_lo (u_lo < total: it exists; a strip 0 without rows is passed over)
        const int rows_s = exh_strip(n, weff, s).rows;
        if (u_lo < cum + rows_s) break;
        cum += rows_s;
    }
    d.strip = s; d.row = (int)(u_lo - cum); d.count = u_hi - u_lo;
    return d;
}

}  // namespace tsp
