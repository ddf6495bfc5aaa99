// =====================================================================
// Which schedule the C-grid subcycle loop runs (evp_host_cgrid_loop.cpp), as ONE value chosen by a pure function of stated
// facts: no HIP call, no global, no environment (the host fills the facts; tests/test_cgrid_schedule_cpu.py walks their cross
// product through the test build's cice_evp_hip_debug_cgrid_choose).
// =====================================================================
#pragma once
#include <climits>
#include <tuple>

namespace evp_host {

constexpr int CG_SW_UNSET = INT_MIN;         // a tri-state switch that is not set (evp_host.h: ENV_UNSET)

// Everything the choice reads.  All int, in this order: one row of cice_evp_hip_debug_cgrid_choose
struct CgSchedFacts {
    // ---- the geometry (cice_evp_hip_cgrid_set_geometry) ----
    int one_tab;         // cg_one's window table is there (no fold, blocks of 3 x 3 cells at least)
    int remote;          // ghost cells that other ranks own
    int tripole, tfold;  // a fold; ... of the T-fold kind
    int geo;             // the derived view of the static table holds (and CICE_EVP_HIP_CGRID_GEO is not 0)
    int frame_plan;      // several ranks, no fold: the fused chain's frame plan (CG.fr)
    int one_items;       // CG.one.zone has work items for the marched kernel
    int rest_plan;       // the fold-band plan, or without a fold the five-phase frame plan (CG.mf.rest)
    int rest_items;      // ... the latter's own items (CG.mf.zone)
    int by_size;         // ... cg_strip's size rule holds for the plan's zone
    int rest_scr5;       // ... its sixth scratch array (deltaU) was allocated
    // ---- the call (finish_upload) ----
    int avg_strength;
    int fast;            // the default-configuration shortcuts hold on every ice cell (and CICE_EVP_HIP_CGRID_FAST is not 0)
    // ---- the on-chip resident kernel ----
    int res_mode;        // -1 undecided, 0 off, 1 on
    int res_ok;          // what it asks beside the schedule: tables, identities, this call's state, every window resident
    // ---- switches (CICE_EVP_HIP_CGRID_*; the two tri-states: 0, 1 or CG_SW_UNSET) ----
    int sw_one, sw_fused, sw_march_ranks, sw_march_fold, sw_march_fold_ranks, sw_march_avgs, sw_serial, sw_strip_last;
    // ---- the loop call ----
    int ndte, first, synced;      // first: no subcycle since the upload; synced: CG.mf.synced
};
constexpr int CG_NFACTS = sizeof(CgSchedFacts) / sizeof(int);

enum CgSchedKind {
    CG_PHASES,               // five launches per subcycle, in place
    CG_THREE,                // three fused launches
    CG_ONE,                  // cg_one, with cg_strip on the interior of large blocks
    CG_ZONE_FRAME,           // several ranks: zone marched + frame (the fused chain on the frame)
    CG_ZONE_FRAME_PHASES,    // ... with the five list-driven phase kernels on the frame (avg_strength)
    CG_MARCH_FOLD,           // tripole, one rank: marched zone + fold band
    CG_MARCH_FOLD_RANKS,     // tripole, several ranks: marched zone + fold band + frame
    CG_PHASES_RESIDENT,      // tripole, one rank: five phases, then cg_res FOLD
    CG_NKINDS
};

struct CgSchedule {
    int kind;            // CgSchedKind
    int nres;            // the call's last nres subcycles run inside one launch of cg_res (CG_ONE, CG_PHASES_RESIDENT)
    // what the enqueue functions and the graph key need beside the kind; 0 where the kind does not read it
    int fast, geo;       // (every kind's graph: the kernels' templates and the table view)
    int serial;          // the three marched split schedules on the five phases: zone, then rest, on one stream (A/B)
    int strip_last;      // ... and CG_ONE: the call's last subcycle with the marched kernel's LAST instantiation
    int sync;            // ... the second allocations have not been brought into line since the upload
    auto tie() const { return std::tie(kind, nres, fast, geo, serial, strip_last, sync); }
};
constexpr int CG_NSCHED = sizeof(CgSchedule) / sizeof(int);
// the zone is marched beside the five list-driven phase kernels (enqueue_march_fold)
inline bool cg_marched_phases(int kind) { return kind == CG_ZONE_FRAME_PHASES || kind == CG_MARCH_FOLD || kind == CG_MARCH_FOLD_RANKS; }

CgSchedule cg_choose_schedule(const CgSchedFacts &f);
// the parts of the choice others ask for on their own (res_eligible, build_march_fold_tables, the description)
bool cg_one_launch(const CgSchedFacts &f);
bool cg_fused(const CgSchedFacts &f);
bool cg_res_rides(const CgSchedFacts &f);                      // the schedule is one cg_res can take the end of
int cg_march_fold_wanted(const CgSchedFacts &f, bool ranks);   // 0 off, 1 forced on, 2 by the size rule

}  // namespace evp_host
