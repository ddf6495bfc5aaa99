// Which schedule the C-grid subcycle loop runs: see cgrid_schedule.h.  The kinds exclude one another by construction here -- one
// cascade, one result -- where they used to by argument (a fused schedule needs no fold and a fold band needs one; the fused
// schedule with avg_strength needs one rank and the five-phase frame several).
#include "cgrid_schedule.h"

namespace evp_host {

// one launch per subcycle (cg_one) for every subcycle but the first after an upload (which still reads the caller's
// uvelN, vvelE, uvel, vvel): one rank, no fold.  CICE_EVP_HIP_CGRID_ONE=0 switches it off, and the marched kernel with it
bool cg_one_launch(const CgSchedFacts &f) { return f.one_tab && !f.remote && f.sw_one; }

bool cg_fused(const CgSchedFacts &f)
{
    if (f.avg_strength && !cg_one_launch(f)) return false;   // the three-launch kernels need deltaU at the neighbours: five phases
    if (f.tripole) return false;                 // recomputing a neighbour across the fold would sum in mirrored order
    return f.sw_fused;
}

// "zone marched + frame" (DESIGN.md section 7): several ranks, no fold, avg_zeta, the derived geometry, rectangles on THIS rank -- a
// rank without them runs the fused schedule, whose exchanges are the same.  ..._ONE=0 / ..._MARCH_RANKS=0 (test build) switch it off
static bool march_ranks(const CgSchedFacts &f)
{
    if (!f.frame_plan || !f.one_items || !f.remote || f.tripole || f.avg_strength || !f.geo) return false;
    return f.sw_one && f.sw_march_ranks;
}

// "marched zone + fold band" (+ frame on several ranks): tripole / tripoleT with rectangles under the fold band;
// cg_res keeps precedence where it serves the call.  Unforced: the default below and cg_strip's size rule, each rank for its own zone.
// ..._MARCH_FOLD=0 / 1 and, across ranks, ..._MARCH_FOLD_RANKS=0 / 1 (test build) switch it off / on wherever a zone forms;
// ..._MARCH_FOLD=1 alone forces the one-rank schedule only, ..._MARCH_FOLD=0 and ..._ONE=0 switch both off
static constexpr bool MARCH_FOLD_DEFAULT = true;            // measured: profiles/r09_cgrid_march_tripole.txt
static constexpr bool MARCH_FOLD_RANKS_DEFAULT = true;      // measured (two-process rehearsals): profiles/r10_cgrid_march_tripole_ranks.txt
int cg_march_fold_wanted(const CgSchedFacts &f, bool ranks)
{
    if (!f.sw_one || (ranks && f.sw_march_fold == 0)) return 0;
    const int forced = ranks ? f.sw_march_fold_ranks : f.sw_march_fold;
    if (forced != CG_SW_UNSET) return forced ? 1 : 0;
    return (ranks ? MARCH_FOLD_RANKS_DEFAULT : MARCH_FOLD_DEFAULT) ? 2 : 0;
}
static bool march_fold(const CgSchedFacts &f)
{
    if (!f.rest_plan || !f.one_items || !f.tripole) return false;
    // (visc_method = avg_strength: on request until it has been timed -- CICE_EVP_HIP_CGRID_MARCH_AVG_STRENGTH=1, set when the
    // geometry was, which allocates the scratch deltaU)
    if (f.avg_strength && !(f.sw_march_avgs && f.rest_scr5)) return false;
    const int want = cg_march_fold_wanted(f, f.remote != 0);
    return want == 1 || (want == 2 && f.by_size);
}

// Several ranks, no fold, visc_method = avg_strength, on request (the same switch): "zone marched + frame" with the frame on the five
// list-driven phase kernels -- the fused chain's frame kernels recompute neighbours and cannot serve avg_strength.  set_geometry built
// the plan (build_march_frame_tables) under the switches and the size rule that admit the fused chain's "zone marched + frame".
static bool march_frame_phases(const CgSchedFacts &f)
{
    if (!f.rest_plan || !f.rest_items || f.tripole || !f.remote || !f.avg_strength || !f.geo) return false;
    return f.sw_march_avgs && f.sw_one && f.sw_march_ranks;
}

// cg_res rides on the one-launch schedule (either visc_method), or takes the end of the five phases under a u-fold on one rank
bool cg_res_rides(const CgSchedFacts &f) { return f.tripole ? !(f.tfold || f.remote) : (cg_fused(f) && cg_one_launch(f)); }
// ... and takes every subcycle of a call but the first after an upload, from three on
static int res_subcycles(const CgSchedFacts &f)
{
    if (f.res_mode != 1 || !cg_res_rides(f) || !f.res_ok) return 0;
    const int n = f.ndte - (f.first ? 1 : 0);
    return (n >= 3 && n <= 4000) ? n : 0;
}

CgSchedule cg_choose_schedule(const CgSchedFacts &f)
{
    CgSchedule s{};
    const bool fused = cg_fused(f);
    s.nres = (fused || f.tripole) ? res_subcycles(f) : 0;
    if (fused) s.kind = cg_one_launch(f) ? CG_ONE : march_ranks(f) ? CG_ZONE_FRAME : CG_THREE;
    else if (s.nres > 0) s.kind = CG_PHASES_RESIDENT;
    else if (march_fold(f)) s.kind = f.remote ? CG_MARCH_FOLD_RANKS : CG_MARCH_FOLD;
    else if (march_frame_phases(f)) s.kind = CG_ZONE_FRAME_PHASES;
    else s.kind = CG_PHASES;
    const bool marched = cg_marched_phases(s.kind);
    s.fast = f.fast ? 1 : 0;
    s.geo = f.geo ? 1 : 0;
    s.serial = (marched && f.sw_serial) ? 1 : 0;
    s.strip_last = ((marched || s.kind == CG_ONE) && f.sw_strip_last) ? 1 : 0;
    s.sync = (marched && !f.first && !f.synced) ? 1 : 0;
    return s;
}

}  // namespace evp_host
