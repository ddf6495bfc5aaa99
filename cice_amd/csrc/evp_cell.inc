// -*- c++ -*-
// Per-cell arithmetic of the EVP subcycle, included twice by evp_kernels.hip:
// once under `#pragma clang fp contract(off)` (namespace evp_strict: every
// multiply and add is rounded separately, like the reference compiled with
// -ffp-contract=off and like oracle/evp_oracle.c) and once under
// `contract(fast)` (namespace evp_fused: the compiler may fuse a*b+c).
//
// What is computed (reference, paths under cicecore/cicedyn/dynamics/):
//   strain_rates      ice_dyn_shared.F90:2127-2161
//   visc_replpress    ice_dyn_shared.F90:2469-2473
//   stress relaxation + stress combinations + str(1:8)   ice_dyn_evp.F90:1585-1739
//   stepu             ice_dyn_shared.F90:925-966
// The operation order of every expression follows the reference so that the
// strict build is bit-identical to it.

struct StressIn {
    double u_ij, u_im, u_jm, u_mm;   // uvel(i,j) (i-1,j) (i,j-1) (i-1,j-1)
    double v_ij, v_im, v_jm, v_mm;
    double dxT, dyT, dxhy, dyhx, cxp, cyp, cxm, cym, DminTarea, strength;
};

// Metric terms of one T-cell from the edge lengths, same expressions as
// init_dyn_shared (ice_dyn_shared.F90:384-388, 406-407, 434-439); tarea = dxT*dyT
// (ice_grid.F90:681), which the host verifies before selecting this path.
__device__ __forceinline__ void metrics_cell(double hte, double hte_im, double htn, double htn_jm,
                                             double deltaminEVP, StressIn &a)
{
    a.cyp = (c1p5 * hte - p5 * hte_im);
    a.cxp = (c1p5 * htn - p5 * htn_jm);
    a.cym = -(c1p5 * hte_im - p5 * hte);
    a.cxm = -(c1p5 * htn_jm - p5 * htn);
    a.dxhy = p5 * (hte - hte_im);
    a.dyhx = p5 * (htn - htn_jm);
    const double tarea = a.dxT * a.dyT;
    a.DminTarea = deltaminEVP * tarea;
}

// CAP: 1 -> capping == 1 exactly, 0 -> capping == 0 exactly, -1 -> general.
// With capping in {0,1} one of the two quotients of visc_replpress is multiplied
// by exactly 0 and added; skipping it is bit-identical for finite operands.
// SIMPLE: the caller has checked revp == 0, Ktens == 0, cosw == 1, sinw == 0 exactly (the reference's
// defaults: classic EVP, ice_dyn_shared.F90:69-70,470-480) -- every product with exactly 1.0 and every
// sum with exactly +-0.0 those values produce is dropped.  x*1.0 == x and x + (+-0.0*finite) == x bit
// for bit, so the strict build stays bit-identical to the general code (the fused build contracts
// differently: covered by its tolerance, and the same in every kernel).
// CORE: strength and fmax(Delta, DminArea) are inside evp_range_math.h's window in every active lane (CAP == 1 only): the
// division's core without its range handling, the same bits.
template <int CAP, bool SIMPLE = false, bool CORE = false>
__device__ __forceinline__ void visc_replpress(const EvpScalars &p, double strength, double DminArea,
                                               double Delta, double &zetax2, double &etax2,
                                               double &rep_prs)
{
    static_assert(!CORE || CAP == 1, "the range-proved division is instantiated for capping == 1 only");
    double tmpcalc;
    if (CORE) {
        tmpcalc = evp_range::div_core(strength, fmax(Delta, DminArea));
    } else if (CAP == 1) {
        tmpcalc = strength / fmax(Delta, DminArea);
    } else if (CAP == 0) {
        tmpcalc = strength / (Delta + DminArea);
    } else {
        tmpcalc = p.capping * (strength / fmax(Delta, DminArea)) +
                  (1.0 - p.capping) * (strength / (Delta + DminArea));
    }
    if (SIMPLE) {
        zetax2 = tmpcalc;
        rep_prs = tmpcalc * Delta;
    } else {
        zetax2 = (1.0 + p.Ktens) * tmpcalc;
        rep_prs = (1.0 - p.Ktens) * tmpcalc * Delta;
    }
    etax2 = p.epp2i * zetax2;
}

// Updates the 12 stress components s[0..11] = stressp_1..4, stressm_1..4,
// stress12_1..4 in place and returns the eight stress-divergence partials.
// POL (evp_range_math.h): LibMath -- the compiler's sqrt and division; RangeMath -- their cores where every active lane of the wave
// has the four Delta^2 (and, classified once per call, strength and DminTarea) inside the window, the library forms otherwise.
template <int CAP, bool SIMPLE = false, class POL = evp_range::LibMath>
__device__ __forceinline__ void stress_cell(const EvpScalars &p, const StressIn &a, double (&s)[12],
                                            double (&str)[8], const POL &pol = POL())
{
    // divergence  =  e_11 + e_22
    const double divune = a.cyp * a.u_ij - a.dyT * a.u_im + a.cxp * a.v_ij - a.dxT * a.v_jm;
    const double divunw = a.cym * a.u_im + a.dyT * a.u_ij + a.cxp * a.v_im - a.dxT * a.v_mm;
    const double divusw = a.cym * a.u_mm + a.dyT * a.u_jm + a.cxm * a.v_mm + a.dxT * a.v_im;
    const double divuse = a.cyp * a.u_jm - a.dyT * a.u_mm + a.cxm * a.v_jm + a.dxT * a.v_ij;
    // tension strain rate  =  e_11 - e_22
    const double tensionne = -a.cym * a.u_ij - a.dyT * a.u_im + a.cxm * a.v_ij + a.dxT * a.v_jm;
    const double tensionnw = -a.cyp * a.u_im + a.dyT * a.u_ij + a.cxm * a.v_im + a.dxT * a.v_mm;
    const double tensionsw = -a.cyp * a.u_mm + a.dyT * a.u_jm + a.cxp * a.v_mm - a.dxT * a.v_im;
    const double tensionse = -a.cym * a.u_jm - a.dyT * a.u_mm + a.cxp * a.v_jm - a.dxT * a.v_ij;
    // shearing strain rate  =  2*e_12
    const double shearne = -a.cym * a.v_ij - a.dyT * a.v_im - a.cxm * a.u_ij - a.dxT * a.u_jm;
    const double shearnw = -a.cyp * a.v_im + a.dyT * a.v_ij - a.cxm * a.u_im - a.dxT * a.u_mm;
    const double shearsw = -a.cyp * a.v_mm + a.dyT * a.v_jm - a.cxp * a.u_mm + a.dxT * a.u_im;
    const double shearse = -a.cym * a.v_jm - a.dyT * a.v_mm - a.cxp * a.u_jm + a.dxT * a.u_ij;
    // Delta (in the denominator of zeta, eta)
    double zetax2ne, etax2ne, rep_prsne, zetax2nw, etax2nw, rep_prsnw;
    double zetax2sw, etax2sw, rep_prssw, zetax2se, etax2se, rep_prsse;
    if constexpr (POL::ranged) {
        using namespace evp_range;
        const double Delta2ne = divune * divune + p.e_factor * (tensionne * tensionne + shearne * shearne);
        const double Delta2nw = divunw * divunw + p.e_factor * (tensionnw * tensionnw + shearnw * shearnw);
        const double Delta2sw = divusw * divusw + p.e_factor * (tensionsw * tensionsw + shearsw * shearsw);
        const double Delta2se = divuse * divuse + p.e_factor * (tensionse * tensionse + shearse * shearse);
        bool cores;
        const unsigned far = umax(umax(off_pos(Delta2ne), off_pos(Delta2nw)), umax(off_pos(Delta2sw), off_pos(Delta2se)));
        cores = pol.wave_inside(outside(far), true);
        if (cores) {      // uniform; Delta = sqrt(Delta^2) lies in [2^-125, 2^125], so fmax(Delta, DminTarea) is inside as well
            const double Deltane = sqrt_core(Delta2ne), Deltanw = sqrt_core(Delta2nw);
            const double Deltasw = sqrt_core(Delta2sw), Deltase = sqrt_core(Delta2se);
            visc_replpress<CAP, SIMPLE, true>(p, a.strength, a.DminTarea, Deltane, zetax2ne, etax2ne, rep_prsne);
            visc_replpress<CAP, SIMPLE, true>(p, a.strength, a.DminTarea, Deltanw, zetax2nw, etax2nw, rep_prsnw);
            visc_replpress<CAP, SIMPLE, true>(p, a.strength, a.DminTarea, Deltasw, zetax2sw, etax2sw, rep_prssw);
            visc_replpress<CAP, SIMPLE, true>(p, a.strength, a.DminTarea, Deltase, zetax2se, etax2se, rep_prsse);
        } else {
            const double Deltane = sqrt(Delta2ne), Deltanw = sqrt(Delta2nw);
            const double Deltasw = sqrt(Delta2sw), Deltase = sqrt(Delta2se);
            visc_replpress<CAP, SIMPLE>(p, a.strength, a.DminTarea, Deltane, zetax2ne, etax2ne, rep_prsne);
            visc_replpress<CAP, SIMPLE>(p, a.strength, a.DminTarea, Deltanw, zetax2nw, etax2nw, rep_prsnw);
            visc_replpress<CAP, SIMPLE>(p, a.strength, a.DminTarea, Deltasw, zetax2sw, etax2sw, rep_prssw);
            visc_replpress<CAP, SIMPLE>(p, a.strength, a.DminTarea, Deltase, zetax2se, etax2se, rep_prsse);
        }
    } else {
    const double Deltane = sqrt(divune * divune + p.e_factor * (tensionne * tensionne + shearne * shearne));
    const double Deltanw = sqrt(divunw * divunw + p.e_factor * (tensionnw * tensionnw + shearnw * shearnw));
    const double Deltasw = sqrt(divusw * divusw + p.e_factor * (tensionsw * tensionsw + shearsw * shearsw));
    const double Deltase = sqrt(divuse * divuse + p.e_factor * (tensionse * tensionse + shearse * shearse));
    visc_replpress<CAP, SIMPLE>(p, a.strength, a.DminTarea, Deltane, zetax2ne, etax2ne, rep_prsne);
    visc_replpress<CAP, SIMPLE>(p, a.strength, a.DminTarea, Deltanw, zetax2nw, etax2nw, rep_prsnw);
    visc_replpress<CAP, SIMPLE>(p, a.strength, a.DminTarea, Deltasw, zetax2sw, etax2sw, rep_prssw);
    visc_replpress<CAP, SIMPLE>(p, a.strength, a.DminTarea, Deltase, zetax2se, etax2se, rep_prsse);
    }

    // the stresses: (1) northeast, (2) northwest, (3) southwest, (4) southeast
    const double arlx1i = p.arlx1i, revp = p.revp, denom1 = p.denom1;
    if (SIMPLE) {      // revp == 0: s*(1 - arlx1i*0) == s
        s[0] = (s[0] + arlx1i * (zetax2ne * divune - rep_prsne)) * denom1;
        s[1] = (s[1] + arlx1i * (zetax2nw * divunw - rep_prsnw)) * denom1;
        s[2] = (s[2] + arlx1i * (zetax2sw * divusw - rep_prssw)) * denom1;
        s[3] = (s[3] + arlx1i * (zetax2se * divuse - rep_prsse)) * denom1;

        s[4] = (s[4] + arlx1i * etax2ne * tensionne) * denom1;
        s[5] = (s[5] + arlx1i * etax2nw * tensionnw) * denom1;
        s[6] = (s[6] + arlx1i * etax2sw * tensionsw) * denom1;
        s[7] = (s[7] + arlx1i * etax2se * tensionse) * denom1;

        s[8] = (s[8] + arlx1i * p5 * etax2ne * shearne) * denom1;
        s[9] = (s[9] + arlx1i * p5 * etax2nw * shearnw) * denom1;
        s[10] = (s[10] + arlx1i * p5 * etax2sw * shearsw) * denom1;
        s[11] = (s[11] + arlx1i * p5 * etax2se * shearse) * denom1;
    } else {
    s[0] = (s[0] * (1.0 - arlx1i * revp) + arlx1i * (zetax2ne * divune - rep_prsne)) * denom1;
    s[1] = (s[1] * (1.0 - arlx1i * revp) + arlx1i * (zetax2nw * divunw - rep_prsnw)) * denom1;
    s[2] = (s[2] * (1.0 - arlx1i * revp) + arlx1i * (zetax2sw * divusw - rep_prssw)) * denom1;
    s[3] = (s[3] * (1.0 - arlx1i * revp) + arlx1i * (zetax2se * divuse - rep_prsse)) * denom1;

    s[4] = (s[4] * (1.0 - arlx1i * revp) + arlx1i * etax2ne * tensionne) * denom1;
    s[5] = (s[5] * (1.0 - arlx1i * revp) + arlx1i * etax2nw * tensionnw) * denom1;
    s[6] = (s[6] * (1.0 - arlx1i * revp) + arlx1i * etax2sw * tensionsw) * denom1;
    s[7] = (s[7] * (1.0 - arlx1i * revp) + arlx1i * etax2se * tensionse) * denom1;

    s[8] = (s[8] * (1.0 - arlx1i * revp) + arlx1i * p5 * etax2ne * shearne) * denom1;
    s[9] = (s[9] * (1.0 - arlx1i * revp) + arlx1i * p5 * etax2nw * shearnw) * denom1;
    s[10] = (s[10] * (1.0 - arlx1i * revp) + arlx1i * p5 * etax2sw * shearsw) * denom1;
    s[11] = (s[11] * (1.0 - arlx1i * revp) + arlx1i * p5 * etax2se * shearse) * denom1;
    }

    // combinations of the stresses for the momentum equation
    const double ssigpn = s[0] + s[1];
    const double ssigps = s[2] + s[3];
    const double ssigpe = s[0] + s[3];
    const double ssigpw = s[1] + s[2];
    const double ssigp1 = (s[0] + s[2]) * p055;
    const double ssigp2 = (s[1] + s[3]) * p055;

    const double ssigmn = s[4] + s[5];
    const double ssigms = s[6] + s[7];
    const double ssigme = s[4] + s[7];
    const double ssigmw = s[5] + s[6];
    const double ssigm1 = (s[4] + s[6]) * p055;
    const double ssigm2 = (s[5] + s[7]) * p055;

    const double ssig12n = s[8] + s[9];
    const double ssig12s = s[10] + s[11];
    const double ssig12e = s[8] + s[11];
    const double ssig12w = s[9] + s[10];
    const double ssig121 = (s[8] + s[10]) * p111;
    const double ssig122 = (s[9] + s[11]) * p111;

    const double csigpne = p111 * s[0] + ssigp2 + p027 * s[2];
    const double csigpnw = p111 * s[1] + ssigp1 + p027 * s[3];
    const double csigpsw = p111 * s[2] + ssigp2 + p027 * s[0];
    const double csigpse = p111 * s[3] + ssigp1 + p027 * s[1];

    const double csigmne = p111 * s[4] + ssigm2 + p027 * s[6];
    const double csigmnw = p111 * s[5] + ssigm1 + p027 * s[7];
    const double csigmsw = p111 * s[6] + ssigm2 + p027 * s[4];
    const double csigmse = p111 * s[7] + ssigm1 + p027 * s[5];

    const double csig12ne = p222 * s[8] + ssig122 + p055 * s[10];
    const double csig12nw = p222 * s[9] + ssig121 + p055 * s[11];
    const double csig12sw = p222 * s[10] + ssig122 + p055 * s[8];
    const double csig12se = p222 * s[11] + ssig121 + p055 * s[9];

    const double str12ew = p5 * a.dxT * (p333 * ssig12e + p166 * ssig12w);
    const double str12we = p5 * a.dxT * (p333 * ssig12w + p166 * ssig12e);
    const double str12ns = p5 * a.dyT * (p333 * ssig12n + p166 * ssig12s);
    const double str12sn = p5 * a.dyT * (p333 * ssig12s + p166 * ssig12n);

    // for dF/dx (u momentum)
    double strp_tmp = p25 * a.dyT * (p333 * ssigpn + p166 * ssigps);
    double strm_tmp = p25 * a.dyT * (p333 * ssigmn + p166 * ssigms);
    // northeast (i,j)
    str[0] = -strp_tmp - strm_tmp - str12ew + a.dxhy * (-csigpne + csigmne) + a.dyhx * csig12ne;
    // northwest (i+1,j)
    str[1] = strp_tmp + strm_tmp - str12we + a.dxhy * (-csigpnw + csigmnw) + a.dyhx * csig12nw;
    strp_tmp = p25 * a.dyT * (p333 * ssigps + p166 * ssigpn);
    strm_tmp = p25 * a.dyT * (p333 * ssigms + p166 * ssigmn);
    // southeast (i,j+1)
    str[2] = -strp_tmp - strm_tmp + str12ew + a.dxhy * (-csigpse + csigmse) + a.dyhx * csig12se;
    // southwest (i+1,j+1)
    str[3] = strp_tmp + strm_tmp + str12we + a.dxhy * (-csigpsw + csigmsw) + a.dyhx * csig12sw;

    // for dF/dy (v momentum)
    strp_tmp = p25 * a.dxT * (p333 * ssigpe + p166 * ssigpw);
    strm_tmp = p25 * a.dxT * (p333 * ssigme + p166 * ssigmw);
    // northeast (i,j)
    str[4] = -strp_tmp + strm_tmp - str12ns - a.dyhx * (csigpne + csigmne) + a.dxhy * csig12ne;
    // southeast (i,j+1)
    str[5] = strp_tmp - strm_tmp - str12sn - a.dyhx * (csigpse + csigmse) + a.dxhy * csig12se;
    strp_tmp = p25 * a.dxT * (p333 * ssigpw + p166 * ssigpe);
    strm_tmp = p25 * a.dxT * (p333 * ssigmw + p166 * ssigme);
    // northwest (i+1,j)
    str[6] = -strp_tmp + strm_tmp + str12ns - a.dyhx * (csigpnw + csigmnw) + a.dxhy * csig12nw;
    // southwest (i+1,j+1)
    str[7] = strp_tmp - strm_tmp + str12sn - a.dyhx * (csigpsw + csigmsw) + a.dxhy * csig12sw;
}

// ---- stress_cell by corners (evp_resident2.hip, COOP): one lane per corner of a T-cell ----
// One corner of stress_cell: strain rates, Delta, viscosities, the corner's three stresses.  The four corners of
// strain_rates (ice_dyn_shared.F90:2127-2155) are ONE expression with per-corner operands and signs:
//     divu    =  cyA*ua + DY*ub + cxA*va + DX*vd
//     tension = -cyB*ua + DY*ub + cxB*va - DX*vd
//     shear   = -cyB*va + DY*vb - cxB*ua + DX*ud
//   corner   (ua ub vd) = velocities at          cyA cyB   cxA cxB    DY    DX
//   NE        ij  im  jm                         cyp cym   cxp cxm   -dyT  -dxT
//   NW        im  ij  mm                         cym cyp   cxp cxm   +dyT  -dxT
//   SW        mm  jm  im                         cym cyp   cxm cxp   +dyT  +dxT
//   SE        jm  mm  ij                         cyp cym   cxm cxp   -dyT  +dxT
// term by term in the reference's order; a - b*c == a + (-b)*c bit for bit, so the signs folded into DY, DX change nothing.
struct CornerIn {
    double ua, va, ub, vb, ud, vd;
    double cyA, cyB, cxA, cxB, DY, DX;
    double strength, DminTarea;
};
template <int CAP, bool SIMPLE = false>
__device__ __forceinline__ void stress_corner(const EvpScalars &p, const CornerIn &c, double &sp, double &sm, double &s12)
{
    const double divu = c.cyA * c.ua + c.DY * c.ub + c.cxA * c.va + c.DX * c.vd;
    const double tension = -c.cyB * c.ua + c.DY * c.ub + c.cxB * c.va - c.DX * c.vd;
    const double shear = -c.cyB * c.va + c.DY * c.vb - c.cxB * c.ua + c.DX * c.ud;
    const double Delta = sqrt(divu * divu + p.e_factor * (tension * tension + shear * shear));
    double zetax2, etax2, rep_prs;
    visc_replpress<CAP, SIMPLE>(p, c.strength, c.DminTarea, Delta, zetax2, etax2, rep_prs);
    const double arlx1i = p.arlx1i, revp = p.revp, denom1 = p.denom1;
    if (SIMPLE) {
        sp = (sp + arlx1i * (zetax2 * divu - rep_prs)) * denom1;
        sm = (sm + arlx1i * etax2 * tension) * denom1;
        s12 = (s12 + arlx1i * p5 * etax2 * shear) * denom1;
    } else {
        sp = (sp * (1.0 - arlx1i * revp) + arlx1i * (zetax2 * divu - rep_prs)) * denom1;
        sm = (sm * (1.0 - arlx1i * revp) + arlx1i * etax2 * tension) * denom1;
        s12 = (s12 * (1.0 - arlx1i * revp) + arlx1i * p5 * etax2 * shear) * denom1;
    }
}
// the corner's operands and signed factors from the cell's metric terms (q: 0 NE, 1 NW, 2 SW, 3 SE)
__device__ __forceinline__ void corner_operands(int q, double dxT, double dyT, double cxp, double cyp, double cxm, double cym,
                                                CornerIn &c, double &KX, double &K12X, double &KYP, double &K12Y)
{
    const bool east = q == 0 || q == 3, north = q < 2;
    c.cyA = east ? cyp : cym; c.cyB = east ? cym : cyp;
    c.cxA = north ? cxp : cxm; c.cxB = north ? cxm : cxp;
    c.DY = east ? -dyT : dyT;
    c.DX = north ? -dxT : dxT;
    KX = (east ? -p25 : p25) * dyT;         // x partial: -strp_tmp - strm_tmp at NE, SE; + at NW, SW
    K12X = (north ? -p5 : p5) * dxT;        //            -str12ew / -str12we at NE, NW; + at SE, SW
    KYP = (north ? -p25 : p25) * dxT;       // y partial: -strp_tmp + strm_tmp at NE, NW; +, - at SE, SW
    K12Y = (east ? -p5 : p5) * dyT;         //            -str12ns / -str12sn at NE, SE; + at NW, SW
}
// The two stress-divergence partials that carry corner q's coefficients, from the twelve stresses of the cell as the lane
// sees them: X0 its own corner's, X1 / X2 / X3 those of corners q^1 / q^2 / q^3 (q: 0 NE, 1 NW, 2 SW, 3 SE -- q^1 is the other
// corner of the same north / south side, q^3 the other one of the same east / west side, q^2 the opposite one).  With that
// numbering the reference's combinations (ice_dyn_evp.F90:1646-1739) read the same at every corner:
//     ssig?n/s -> X0 + X1 (near side), X2 + X3 (far);  ssig?e/w -> X0 + X3 (near), X1 + X2 (far);  ssig?1/2 -> X1 + X3
//     csig?    =  k1*X0 + (X1 + X3)*k2 + k3*X2
// (x + y == y + x bit for bit; every product and sum below is the reference's, in its order).  The signs of strp_tmp, strm_tmp
// and str12?? in str(1:8) come in through KX = (+-p25)*dyT, K12X = (+-p5)*dxT, KYP = (+-p25)*dxT, K12Y = (+-p5)*dyT:
//     x partial: NE -,-  NW +,-  SW +,+  SE -,+        y partial (strp; strm takes the other sign): NE -,-  NW -,+  SW +,+  SE +,-
__device__ __forceinline__ void stress_corner_partials(double P0, double P1, double P2, double P3, double M0, double M1, double M2,
                                                       double M3, double T0, double T1, double T2, double T3, double KX, double K12X,
                                                       double KYP, double K12Y, double dxhy, double dyhx, double &X, double &Y)
{
    const double csigp = p111 * P0 + (P1 + P3) * p055 + p027 * P2;
    const double csigm = p111 * M0 + (M1 + M3) * p055 + p027 * M2;
    const double csig12 = p222 * T0 + (T1 + T3) * p111 + p055 * T2;
    const double str12x = K12X * (p333 * (T0 + T3) + p166 * (T1 + T2));
    const double str12y = K12Y * (p333 * (T0 + T1) + p166 * (T2 + T3));
    const double strp_x = KX * (p333 * (P0 + P1) + p166 * (P2 + P3));
    const double strm_x = KX * (p333 * (M0 + M1) + p166 * (M2 + M3));
    X = strp_x + strm_x + str12x + dxhy * (-csigp + csigm) + dyhx * csig12;
    const double strp_y = KYP * (p333 * (P0 + P3) + p166 * (P1 + P2));
    const double strm_y = -KYP * (p333 * (M0 + M3) + p166 * (M1 + M2));
    Y = strp_y + strm_y + str12y - dyhx * (csigp + csigm) + dxhy * csig12;
}

struct StepuIn {
    double uold, vold;
    double vrelfac;              // (aiX*rhow)*Cw
    double uocn, vocn, waterx, watery, forcex, forcey, Umassdti, fm, uarear, TbU;
    double uvel_init, vvel_init;
    double sx0, sx1, sx2, sx3;   // str(i,j,1) str(i+1,j,2) str(i,j+1,3) str(i+1,j+1,4)
    double sy0, sy1, sy2, sy3;   // str(i,j,5) str(i,j+1,6) str(i+1,j,7) str(i+1,j+1,8)
};

struct StepuOut {
    double u, v, strintx, strinty, taubx, tauby;
};

// What the momentum step of a U-cell knows before any stress partial of the subcycle exists: it depends on the cell's previous
// velocity and on per-call operands only (stepu_pre_cell), and what needs the eight partials (stepu_post_cell).  Every expression
// is the reference's, whole and in its order, so both builds round / contract as the one-piece form did; stepu_cell is the two in
// turn.  (evp_resident2.hip, RIMU: the rim wave works out the first part for the next subcycle while it is off the hand-off chain.)
struct StepuPre {
    double taux, tauy, Cb, cca, ccb, ab2;
    double bu, bv;               // brlx*uold + revp*uvel_init, brlx*vold + revp*vvel_init (WITH_B)
    double r;                    // POL::split_div: recip_core(ab2) ...
    bool ab2_inside;             // ... and whether ab2 is inside the window in every active lane (wave-uniform)
};

// TBU: false when the host has verified TbU == 0 on every ice U-cell (seabed stress off): Cb = 0/(...) == 0
// WITH_B: the first part also forms bu, bv; without, the second part forms them inside cc1 / cc2, where the one-piece form had
// them -- stepu_cell takes that order, so that the kernels that call it compile to the code they compiled to before the split
// POL (evp_range_math.h), RangeMath: the square root's core where du^2 + dv^2 is inside the window in every active lane.  The two
// divisions of the second part stay the compiler's: the test of their three operands costs what their range handling costs.
// POL::split_div (RangeMathLazySplit; measured, not the default: profiles/r16_resident_rim_first.txt): the first part also forms
// recip_core(ab2) and the verdict on ab2, the second part tests the two numerators and takes two quot_core.
template <bool SIMPLE = false, bool TBU = true, bool WITH_B = true, class POL = evp_range::LibMath>
__device__ __forceinline__ void stepu_pre_cell(const EvpScalars &p, const StepuIn &a, StepuPre &w, const POL &pol = POL())
{
    const double uold = a.uold, vold = a.vold;
    // (magnitude of relative ocean current)*rhow*drag*aice
    const double du = a.uocn - uold, dv = a.vocn - vold;
    double vrel;
    if constexpr (POL::ranged) {
        const double speed2 = du * du + dv * dv;
        if (pol.wave_inside(evp_range::outside(evp_range::off_pos(speed2)), false)) vrel = a.vrelfac * evp_range::sqrt_core(speed2);
        else vrel = a.vrelfac * sqrt(speed2);
    } else {
    vrel = a.vrelfac * sqrt(du * du + dv * dv);
    }
    // ice/ocean stress
    w.taux = vrel * a.waterx;
    w.tauy = vrel * a.watery;
    double Cb = 0.0;
    if (TBU) Cb = a.TbU / (sqrt(uold * uold + vold * vold) + p.u0);   // for seabed stress
    w.Cb = Cb;
    // revp = 0 for classic evp, 1 for revised evp
    double cca, ccb;
    if (SIMPLE) {      // revp == 0, cosw == 1, sinw == 0: ccb = fm + (+-0) == fm for either sign of fm
        cca = p.brlx * a.Umassdti + vrel + Cb;
        ccb = a.fm;
    } else {
        cca = (p.brlx + p.revp) * a.Umassdti + vrel * p.cosw + Cb;
        ccb = a.fm + copysign(1.0, a.fm) * vrel * p.sinw;
    }
    w.cca = cca; w.ccb = ccb;
    w.ab2 = cca * cca + ccb * ccb;
    if constexpr (POL::split_div) {
        // the denominator's share of the second part's two divisions, here where it is off the hand-off chain (evp_range_math.h)
        if (!pol.nosplit) {
            w.ab2_inside = pol.verdict(evp_range::outside(evp_range::off_pos(w.ab2)));
            w.r = evp_range::recip_core(w.ab2);
        }
    }
    if (!WITH_B) return;
    if (SIMPLE) {      // revp*uvel_init == +0.0 (the kernels pass uvel_init = 0 when revp == 0); the add stays: -0 + 0 = +0
        w.bu = p.brlx * uold + 0.0;
        w.bv = p.brlx * vold + 0.0;
    } else {
        w.bu = p.brlx * uold + p.revp * a.uvel_init;
        w.bv = p.brlx * vold + p.revp * a.vvel_init;
    }
}

// the part that reads the stress partials (a.sx0 .. a.sy3; a.uarear, a.forcex / forcey, a.Umassdti besides)
// POL::lazy_taub: o.taubx / o.tauby are left to the caller, which forms them from o.u, o.v and w.Cb where it stores them
template <bool SIMPLE = false, bool WITH_B = true, class POL = evp_range::LibMath>
__device__ __forceinline__ void stepu_post_cell(const EvpScalars &p, const StepuIn &a, const StepuPre &w, StepuOut &o, const POL &pol = POL())
{
    // divergence of the internal stress tensor
    o.strintx = a.uarear * (a.sx0 + a.sx1 + a.sx2 + a.sx3);
    o.strinty = a.uarear * (a.sy0 + a.sy1 + a.sy2 + a.sy3);
    // finally, the velocity components
    double cc1, cc2;
    if (WITH_B) {
        cc1 = o.strintx + a.forcex + w.taux + a.Umassdti * w.bu;
        cc2 = o.strinty + a.forcey + w.tauy + a.Umassdti * w.bv;
    } else if (SIMPLE) {      // revp*uvel_init == +0.0 (the kernels pass uvel_init = 0 when revp == 0); the add stays: -0 + 0 = +0
        cc1 = o.strintx + a.forcex + w.taux + a.Umassdti * (p.brlx * a.uold + 0.0);
        cc2 = o.strinty + a.forcey + w.tauy + a.Umassdti * (p.brlx * a.vold + 0.0);
    } else {
        cc1 = o.strintx + a.forcex + w.taux + a.Umassdti * (p.brlx * a.uold + p.revp * a.uvel_init);
        cc2 = o.strinty + a.forcey + w.tauy + a.Umassdti * (p.brlx * a.vold + p.revp * a.vvel_init);
    }
    if constexpr (POL::split_div) {
        // a wave whose active lanes all have ab2 (the first part's verdict) and both numerators inside the window: the quotients'
        // three operations each on the reciprocal the first part formed; any other wave the compiler's divisions
        const double nu = w.cca * cc1 + w.ccb * cc2, nv = w.cca * cc2 - w.ccb * cc1;
        if (!pol.nosplit &&
            pol.wave_inside(evp_range::outside(evp_range::umax(evp_range::off_abs(nu), evp_range::off_abs(nv))), false, w.ab2_inside)) {
            o.u = evp_range::quot_core(nu, w.ab2, w.r);
            o.v = evp_range::quot_core(nv, w.ab2, w.r);
        } else {
            o.u = nu / w.ab2;
            o.v = nv / w.ab2;
        }
    } else {
    o.u = (w.cca * cc1 + w.ccb * cc2) / w.ab2;
    o.v = (w.cca * cc2 - w.ccb * cc1) / w.ab2;
    }
    // seabed stress component for outputs
    if (POL::lazy_taub) return;
    o.taubx = -o.u * w.Cb;
    o.tauby = -o.v * w.Cb;
}

template <bool SIMPLE = false, bool TBU = true, class POL = evp_range::LibMath>
__device__ __forceinline__ void stepu_cell(const EvpScalars &p, const StepuIn &a, StepuOut &o, const POL &pol = POL())
{
    StepuPre w;
    stepu_pre_cell<SIMPLE, TBU, false, POL>(p, a, w, pol);
    stepu_post_cell<SIMPLE, false>(p, a, w, o);
}

// ---------------------------------------------------------------------
// Next tier (SURVEY 8 f-1): kernels evp() runs on the final velocities.
//   deformations   ice_dyn_shared.F90:1827-1856   (strain rates as above, :2127-2161)
//   dyn_finish     ice_dyn_shared.F90:1339-1355
// ---------------------------------------------------------------------
struct DeformOut {
    double divu, shear, vort, rdg_conv, rdg_shear;
};

__device__ __forceinline__ void deform_cell(const EvpScalars &p, const StressIn &a, double tarear,
                                            double dyU_ij, double dyU_im, double dyU_jm, double dyU_mm,
                                            double dxU_ij, double dxU_im, double dxU_jm, double dxU_mm,
                                            DeformOut &o)
{
    const double divune = a.cyp * a.u_ij - a.dyT * a.u_im + a.cxp * a.v_ij - a.dxT * a.v_jm;
    const double divunw = a.cym * a.u_im + a.dyT * a.u_ij + a.cxp * a.v_im - a.dxT * a.v_mm;
    const double divusw = a.cym * a.u_mm + a.dyT * a.u_jm + a.cxm * a.v_mm + a.dxT * a.v_im;
    const double divuse = a.cyp * a.u_jm - a.dyT * a.u_mm + a.cxm * a.v_jm + a.dxT * a.v_ij;
    const double tensionne = -a.cym * a.u_ij - a.dyT * a.u_im + a.cxm * a.v_ij + a.dxT * a.v_jm;
    const double tensionnw = -a.cyp * a.u_im + a.dyT * a.u_ij + a.cxm * a.v_im + a.dxT * a.v_mm;
    const double tensionsw = -a.cyp * a.u_mm + a.dyT * a.u_jm + a.cxp * a.v_mm - a.dxT * a.v_im;
    const double tensionse = -a.cym * a.u_jm - a.dyT * a.u_mm + a.cxp * a.v_jm - a.dxT * a.v_ij;
    const double shearne = -a.cym * a.v_ij - a.dyT * a.v_im - a.cxm * a.u_ij - a.dxT * a.u_jm;
    const double shearnw = -a.cyp * a.v_im + a.dyT * a.v_ij - a.cxm * a.u_im - a.dxT * a.u_mm;
    const double shearsw = -a.cyp * a.v_mm + a.dyT * a.v_jm - a.cxp * a.u_mm + a.dxT * a.u_im;
    const double shearse = -a.cym * a.v_jm - a.dyT * a.v_mm - a.cxp * a.u_jm + a.dxT * a.u_ij;
    const double Deltane = sqrt(divune * divune + p.e_factor * (tensionne * tensionne + shearne * shearne));
    const double Deltanw = sqrt(divunw * divunw + p.e_factor * (tensionnw * tensionnw + shearnw * shearnw));
    const double Deltasw = sqrt(divusw * divusw + p.e_factor * (tensionsw * tensionsw + shearsw * shearsw));
    const double Deltase = sqrt(divuse * divuse + p.e_factor * (tensionse * tensionse + shearse * shearse));

    o.divu = p25 * (divune + divunw + divuse + divusw) * tarear;
    const double tmp = p25 * (Deltane + Deltanw + Deltase + Deltasw) * tarear;
    o.rdg_conv = -fmin(o.divu, 0.0);
    o.rdg_shear = p5 * (tmp - fabs(o.divu));
    const double tsum = tensionne + tensionnw + tensionse + tensionsw;
    const double ssum = shearne + shearnw + shearse + shearsw;
    o.shear = p25 * tarear * sqrt(tsum * tsum + ssum * ssum);
    const double dvdxn = dyU_ij * a.v_ij - dyU_im * a.v_im;
    const double dvdxs = dyU_jm * a.v_jm - dyU_mm * a.v_mm;
    const double dudye = dxU_ij * a.u_ij - dxU_jm * a.u_jm;
    const double dudyw = dxU_im * a.u_im - dxU_mm * a.u_mm;
    o.vort = p5 * tarear * (dvdxn + dvdxs - dudye - dudyw);
}

__device__ __forceinline__ void finish_cell(const EvpScalars &p, double Cw, double aiX, double uocn,
                                            double vocn, double u, double v, double fm,
                                            double &strocnx, double &strocny)
{
    const double du = uocn - u, dv = vocn - v;
    double vrel = p.rhow * Cw * sqrt(du * du + dv * dv);
    vrel = vrel * aiX;
    strocnx = vrel * ((uocn - u) * p.cosw - (vocn - v) * p.sinw * copysign(1.0, fm));
    strocny = vrel * ((vocn - v) * p.cosw + (uocn - u) * p.sinw * copysign(1.0, fm));
}
