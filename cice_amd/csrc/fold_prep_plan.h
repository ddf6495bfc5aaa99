// Host-side plans of what runs AROUND the subcycle loop on a tripole grid whose fold rows are split over ranks: pure C++ (no
// HIP), derived from the block table and the halo plan -- nothing here adds to HaloPlan.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "halo_plan.h"

// tripoleT, the stress symmetrisation (halo_plan.h: stress_dst / stress_own_* / stress_corner_*) on ANY rank layout: the same
// three lists for this rank, in the order build_halo_plan gives them, but an operand may be a staging slot n_local + t of the
// C grid's exchange (HaloPlan::cg_peers) -- the slot cg_fold[0]'s entries already use for that cell: the centre T-fold rule
// reads the same cells (m, NY) and (m, NY-1), so the exchange of a pair (a1, a2) brings every partner value.
//   dst / src                row NY of _1 / _2 (east-west ghost columns included) <- PARTNER array's cell (NX-ig+2, NY)
//   own_dst / own_src        east-west ghost cells of row NY of _3 / _4           <- OWN array's cell (ig, NY)
//   corner_dst / corner_src  north-west corner ghost cell of a top-row block      <- partner's (NX-ig+2, NY-1), all four arrays
// collective: some rank's operand lives on another rank -- computed identically on every rank (the walk runs over all of them),
// since the exchange is a collective of all ranks.  Without it the lists equal the halo plan's.
struct StressTfoldXPlan {
    std::vector<int32_t> dst, src, own_dst, own_src, corner_dst, corner_src;
    bool collective = false;
    std::string why;          // not empty: declined (no lists), and why
    bool ok() const { return why.empty(); }
};

// Declines (X.why) where the grid is not tripoleT, a needed cell lies in an eliminated block (on any rank: the verdict is the
// same everywhere), or a cell of another rank is not among the fold sources the exchange carries.  d: what build_halo_plan
// accepted for P.
void build_stress_tfold_xplan(const cice_evp_hip_dims &d, const HaloPlan &P, StressTfoldXPlan &X);
