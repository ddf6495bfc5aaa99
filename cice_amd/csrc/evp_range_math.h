// fp64 square root and division without their range handling, for operands PROVED to lie in a window of exponents, and the
// policies by which evp_cell.inc selects them (evp_resident2.hip, the lean loops; profiles/r15_resident_range_math.txt).
//
// What the compiler emits for sqrt(x) and n / d on gfx950 is a correctly rounded core -- a hardware seed (v_rsq_f64 / v_rcp_f64)
// refined by fused multiply-adds -- wrapped in range handling: the square root scales x by 2^256 below 2^-767 and passes 0 and inf
// through (v_cmp, v_cndmask, two v_ldexp_f64, v_cmp_class, two v_cndmask); the division scales numerator and denominator
// (two v_div_scale_f64, the flag in VCC read by v_div_fmas_f64) and patches special operands and signs (v_div_fixup_f64).
// sqrt_core / div_core are those cores, operation for operation, nothing improved: that they round correctly is the compiler's
// proof, and it holds for that sequence only.
//
// The window.  W = { x : 2^-250 <= |x| < 2^250 } (biased exponents 773 .. 1272); zero, -0, denormals, inf and NaN are outside.
//   sqrt, x in W and x > 0:   x >= 2^-767, so the scale exponent is 0 and both v_ldexp_f64 shift by 0; x is neither 0 nor inf, so
//                             the class test selects the computed value.  g ~ sqrt(x) lies in [2^-125, 2^125], h ~ 0.5/g likewise,
//                             the residuals fma(-g, g, x) are 0 or at least 2^-250 * 2^-106 in magnitude: nothing leaves the
//                             normal range.
//   n / d, both in W:         v_div_scale_f64 (ISA: V_DIV_SCALE_F64) returns its operand with VCC = 0 unless an operand is 0 or
//                             denormal, exponent(n) - exponent(d) >= 768, 1/d is denormal, n/d is denormal, or exponent(n) <= 53:
//                             here the exponents differ by at most 499, |1/d| > 2^-250, |n/d| lies in (2^-500, 2^500) and
//                             exponent(n) >= 773.  With VCC = 0 v_div_fmas_f64 is v_fma_f64.  v_div_fixup_f64 returns the
//                             quotient it is given, with the sign sign(n) ^ sign(d), unless an operand is NaN, inf or 0 or the
//                             exponents differ by more than about 1020; the core's quotient has that sign already: q = n * r with
//                             r of d's sign, and the last fma cannot cancel it (|e * r| <= 2^-51 |q|).  A numerator of -0 would
//                             come out +0 from the core: zeros are outside W for that reason too.
//                             The sequence is rcp, four fmas on d alone, then mul and two fmas with n: r = recip_core(d) depends on
//                             d only and may be formed EARLIER than the quotient needs it (the rim wave's momentum step: ab2 is
//                             known after the barrier, the numerators only once the stress partials are) and shared by two
//                             quotients of one d; quot_core(n, d, r) then performs the same three operations on the same values,
//                             so the argument above covers div_core == quot_core(n, d, recip_core(d)) unchanged.  The verdict on
//                             d travels with r (same lanes active in both places).
// A caller takes the core only where EVERY active lane of the wave has all its operands in W (one ballot, a uniform branch) and
// today's code otherwise, so no bit can change; tests/test_gpu_range_math.py sweeps both against the compiler's forms.
#pragma once
#include <hip/hip_runtime.h>

namespace evp_range {

constexpr int WIN_EXP = 250;                                        // W = [2^-WIN_EXP, 2^WIN_EXP)
constexpr unsigned WIN_LO_HI = (unsigned)(1023 - WIN_EXP) << 20;    // high word of 2^-WIN_EXP
constexpr unsigned WIN_SPAN_HI = (unsigned)(2 * WIN_EXP) << 20;     // high words of W: WIN_LO_HI + [0, WIN_SPAN_HI)

__device__ __forceinline__ unsigned hi_word(double x) { return (unsigned)((unsigned long long)__double_as_longlong(x) >> 32); }
// How far the high word lies above the window's lower edge (unsigned: anything below wraps to a huge value).  off_pos: for a value
// that is in W only if positive (a negative one has bit 31 set and lands far outside); off_abs: by magnitude.
__device__ __forceinline__ unsigned off_pos(double x) { return hi_word(x) - WIN_LO_HI; }
__device__ __forceinline__ unsigned off_abs(double x) { return (hi_word(x) & 0x7fffffffu) - WIN_LO_HI; }
__device__ __forceinline__ bool outside(unsigned off) { return off >= WIN_SPAN_HI; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// sqrt(x) for x in W, x > 0
__device__ __forceinline__ double sqrt_core(double x)
{
#pragma clang fp contract(off)
    const double r = __builtin_amdgcn_rsq(x);
    double g = x * r;
    double h = 0.5 * r;
    const double e = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, e, g);
    h = __builtin_fma(h, e, h);
    double d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    return g;
}

// n / d for n, d in W, in two pieces: the first five operations read the denominator only ...
__device__ __forceinline__ double recip_core(double d)
{
#pragma clang fp contract(off)
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    return r;
}
// ... and the last three take r = recip_core(d) from wherever it was formed
__device__ __forceinline__ double quot_core(double n, double d, double r)
{
#pragma clang fp contract(off)
    double q = n * r;
    const double e = __builtin_fma(-d, q, n);
    q = __builtin_fma(e, r, q);
    return q;
}
__device__ __forceinline__ double div_core(double n, double d) { return quot_core(n, d, recip_core(d)); }

// ---- policies of evp_cell.inc -------------------------------------------------------------------------------------------------
// LibMath: the compiler's sqrt and division everywhere (every kernel but the lean resident loops: their code is what it was).
struct LibMath {
    static constexpr bool ranged = false;
    static constexpr bool lazy_taub = false;
    static constexpr bool split_div = false;
};
// RangeMath: per pass, each lane tests its operands against W, the verdicts are combined over the wave's active lanes, and the wave
// takes the cores only when all are inside.  cbad: the lanes whose per-call operands of the stress update (strength, DminTarea)
// are outside W, classified once before the loop (same active lanes as the stress update's).  off: the test build's A/B switch
// (always the library path); a constant in the product.  nlib: passes that took the library path (test build's read-out).
struct RangeMath {
    static constexpr bool ranged = true;
    static constexpr bool lazy_taub = false;
    static constexpr bool split_div = false;
    unsigned long long cbad = 0;
    bool off = false;
    bool nosplit = false;      // split_div policies, the test build's A/B switch: the U-cell's divisions the compiler's, as they were
    mutable unsigned nlib = 0;
    // wave-uniform: every active lane's operands are inside the window (carried: a wave-uniform verdict formed earlier, on the
    // same active lanes, joins it)
    __device__ __forceinline__ bool wave_inside(bool lane_outside, bool with_cbad, bool carried = true) const
    {
        if (off) { ++nlib; return false; }
        unsigned long long bad = __builtin_amdgcn_ballot_w64(lane_outside);
        if (with_cbad) bad |= cbad;
        if (__builtin_expect(bad != 0 || !carried, 0)) { ++nlib; return false; }
        return true;
    }
    // the verdict alone, for a later wave_inside to carry (counts nothing: the pass that uses it does)
    __device__ __forceinline__ bool verdict(bool lane_outside) const { return __builtin_amdgcn_ballot_w64(lane_outside) == 0; }
    static __device__ __forceinline__ bool percall_outside(double strength, double DminTarea)
    {
        return outside(off_abs(strength)) || outside(off_pos(DminTarea));
    }
};
// ... and taubx / tauby left to the caller, which forms them where it stores them (the rim-wave schedule)
struct RangeMathLazy : RangeMath {
    static constexpr bool lazy_taub = true;
};
// ... and the U-cell's two divisions by ab2 on the cores, the reciprocal formed in the first part of the momentum step
// (stepu_pre_cell: recip_core, the verdict on ab2 carried as a wave-uniform flag) and the quotients in the second (quot_core x 2)
struct RangeMathLazySplit : RangeMathLazy {
    static constexpr bool split_div = true;
};

}  // namespace evp_range
