// =====================================================================
// C-grid EVP host, private to its two halves: the state (CGridState) and the few helpers both need.
//   evp_host_cgrid.cpp       geometry and tables, upload / download, preparation, after the loop, read-outs
//   evp_host_cgrid_loop.cpp  the subcycle loop: the facts for the schedule's chooser (cgrid_schedule.h), the enqueue_* functions,
//                            cice_evp_hip_cgrid_subcycle, the description of the schedule
// =====================================================================
#pragma once
#include "cgrid_schedule.h"
#include "evp_host.h"

namespace evp_host {
static_assert(CG_SW_UNSET == ENV_UNSET, "cgrid_schedule.h and evp_host.h must agree on a switch that is not set");

// the five arrays a subcycle reads in one allocation and writes in the other (every schedule but the five phases), in this order
static const int PP_FIELDS[5] = {CF_UE, CF_VN, CF_SP, CF_SM, CF_S12U};
constexpr unsigned PP_FOUR = 15u, PP_S12 = 16u, PP_ALL = PP_FOUR | PP_S12;     // bit q: PP_FIELDS[q]

// What a schedule did with a call's subcycles: the enqueue_* functions fill it in as they enqueue, the graph cache keeps it beside
// the captured graph (a replay did what the capture did), cice_evp_hip_cgrid_subcycle applies it
struct Ran {
    unsigned swapped = 0;        // bit q: PP_FIELDS[q] ended in the allocation that was the other one when the call began
    int count[CG_NKINDS] = {};   // subcycles run the way that is the kind's own: CG_ONE one launch each, the four marched split schedules
                                 // with the marched kernel beside the rest (the first after an upload never is: not counted)
};
// Everything a captured graph bakes in that can change between calls: pointers (in_alt) and kernel / template choices
// (s.strip_last among them since round 26: until then two calls of one geometry that differed in CICE_EVP_HIP_CGRID_STRIP_LAST alone
// shared the graph of the first)
struct GraphKey {
    int ndte;
    unsigned in_alt;
    bool first;
    int avg_strength;
    CgSchedule s;
    auto tie() const { return std::make_tuple(ndte, in_alt, first, avg_strength, s.tie()); }
    bool operator<(const GraphKey &o) const { return tie() < o.tie(); }
};
// The marched kernel's work items of one plan (cgrid_plan.cpp: strip_items) as uploaded
struct MarchItems {
    int *items = nullptr;
    int nitems = 0;
    int len = 0;                 // 1: the marched kernel forms six of the eight lengths from dxN, dyE
    int seg = 0;                 // rows per segment
    int ex = 0, ey = 0;          // shape of the windows the rectangles were cut from (and of the windows cg_one keeps)
    long cells = 0;              // cells the marched kernel owns
};
// The cells the marched kernel does not own, as the kernels beside it want them: per-cell bits, per level the workgroups to launch,
// scratch arrays for the intermediates of the zone cells those kernels read
struct CellLists {
    uint8_t *cells = nullptr;
    int *wg[5] = {};
    int nwg[5] = {};
    double *scr[6] = {};
    long ncells = 0;
};

struct CGridState {
    DevicePool mem;              // owns every device allocation below
    bool geo = false, uploaded = false;
    double *f[CG_NF] = {}, *in[CG_NIN] = {}, *g[CG_NG] = {};
    double *gslab = nullptr, *inslab = nullptr;   // g[k] = gslab + k * n, in[k] = inslab + k * n: one allocation per table (cg_one addresses them as base + k * stride)
    double *strengthU = nullptr;
    double *umaskd = nullptr;    // ranks > 1: iceU as a field, to learn the flags of ghost cells other ranks own
    double *fac[2] = {nullptr, nullptr};   // leading factor of vrel at E / N (once per call)
    unsigned *d_flags = nullptr;
    bool fast = false;           // the shortcuts of cg_stress_u_step<true> hold on every ice cell of this call
    // second allocations of PP_FIELDS (f[PP_FIELDS[q]] always holds the current one); [4] always, [0..3] where a schedule that
    // ping-pongs them can run (need_alt)
    double *alt[5] = {};
    unsigned in_alt = 0;         // bit q: f[PP_FIELDS[q]] is the second allocation
    // one launch per subcycle (evp_cgrid.hip: cg_one): window table
    struct One {
        int *tab = nullptr;
        int4 *tiles = nullptr;
        int ntiles = 0, per_xcd = 0, ox = 0, oy = 0;
        unsigned long long *prof = nullptr;   // test build: phase stamps (CICE_EVP_HIP_CGRID_PROF=1)
        // the interior of large blocks marched (evp_cgrid.hip: cg_strip): its items, and the windows cg_one keeps (the block edges)
        MarchItems zone;
        int4 *tiles_e = nullptr;
        int *tab_e = nullptr;
        int ntiles_e = 0;
    } one;
    // several ranks: the marched kernel on the rectangles above beside the fused chain on every other interior cell (enqueue_fused:
    // "zone marched + frame"; cgrid_plan.cpp: build_cg_frame).  cells: the EVP_CGS_* bits (REST = frame cell); three levels; scr:
    // shearU, etax2T, stresspT, stressmT of the zone cells the frame reads; ncells: frame cells
    CellLists fr;
    // tripole / tripoleT on one rank: the marched kernel on the rectangles under the fold band beside list-driven variants of the five
    // phase kernels on every other interior cell (enqueue_march_fold: "marched zone + fold band"; cgrid_plan.cpp: build_cg_march_fold).
    // On several ranks the same with the frame in the rest and the five phases' exchanges at their points ("... + frame").
    // The items live in `one.zone`
    struct MarchFold {
        CellLists rest;                      // cells: the EVP_CGS_* bits; five phases; scr: shearU, etax2T, stresspT, stressmT, stress12U, deltaU; ncells: REST cells
        uint8_t *gmask = nullptr;            // the land masks as bits on the rows the marched kernel derives its geometry on
        int band_rows = 0;
        long frame_cells = 0;                // several ranks: REST cells another rank receives or that have a ghost image here
        bool by_size = false;                // cg_strip's size rule holds for the zone
        // no fold, several ranks, visc_method = avg_strength ("zone marched + frame" on the five phases): this plan's own items --
        // CG.one's belong to the fused chain's frame plan (CG.fr), whose rectangles may differ
        MarchItems zone;
        bool synced = false;                 // the second allocations of the five ping-pong arrays agree with the current ones on every cell no
                                             // subcycle writes (false after an upload and after any call another schedule ran)
        std::string why;                     // why there is no plan on this rank
    } mf;
    // the marched kernel's stream beside S.stream, forked from and joined to it in every subcycle.  One per geometry: zone + frame
    // needs several ranks and no fold, zone + fold band (+ frame) a fold
    struct Side {
        hipStream_t st = nullptr;
        hipEvent_t fork = nullptr, join = nullptr;
    } side;
    // all subcycles of a call in one launch, state on the chip (evp_cgrid_res.hip: cg_res)
    struct Res {
        int *tab = nullptr;
        int4 *tiles = nullptr, *tiles2 = nullptr;     // (tiles2: tripole grids, cgrid_plan.cpp build_fold_window_table)
        int ntiles = 0;
        uint8_t *pubmap = nullptr;
        uint8_t *gmask = nullptr;    // tripole grids: the land masks as bits (elsewhere CG.gmask, which the one-launch kernels share)
        char *rec = nullptr;         // EVP_CGRES_SLOTS x S.n records of 32 bytes
        int *err = nullptr;
        int *d_order = nullptr;      // the windows that hold ice in this call (cg_res_live at every upload), n_live of them
        int *live_win = nullptr;     // [ntiles] 0 / 1
        uint8_t *live_cell = nullptr;   // per cell: its window runs in this call
        int n_live = 0;
        std::vector<int> h_live;
        unsigned epoch = 0;
        int par = 0;
        bool images_ok = false;      // every ghost cell's static arrays equal its source's bit for bit
        int2 *pairs = nullptr;       // (array neighbour of a position's cell, the ghost cell outside the domain the table names for the
        int npairs = 0;              // neighbouring position) where the two differ: must hold the same values (static: checked once)
        bool pairs_state_ok = true;  // ... and the same state in this call (checked on the device at every upload)
        std::string why;             // ... or why the kernel is not eligible on this rank
        int mode = -1;               // -1 undecided (first eligible call probes), 0 off, 1 on
        bool launched = false;       // a launch whose error word has not been looked at
        long cap4[8] = {};           // windows that can be resident at once (occupancy x CUs), by kernel variant (avg_strength | revised << 1 | slow << 2)
        double t_probe_ms = -1.0;    // probe: ms per subcycle
        int last_nsub = 0;           // subcycles of the last call that ran inside it
        int fallbacks = 0;           // cice_evp_hip_cgrid_run calls repeated without it after a wait gave up
        unsigned long long *prof = nullptr;   // test build: phase stamps (CICE_EVP_HIP_CGRID_PROF=1)
    } res;
    uint8_t *mask = nullptr;
    uint8_t *gmask = nullptr;    // the four land masks as bits (cg_one's derived view of the static table); null: an identity failed
    std::string geo_why;         // ... and which one
    int *img_slot = nullptr, *img_dst = nullptr;
    // tripole fold: per field location the cells of the fold row / the ghost row beyond it and their sources
    bool tripole = false;
    bool tfold = false;                  // ... of the T-fold kind (tripoleT)
    struct Fold { int *dst = nullptr, *a = nullptr, *b = nullptr; unsigned char *flip = nullptr; int n = 0; } fold[4];
    double *fold_tmp = nullptr;
    int fold_maxn = 0;
    int *zero_cells = nullptr;   // ghost cells of eliminated (land) neighbour blocks
    int n_zero = 0;
    std::vector<int> h_img_slot, h_img_dst;
    int32_t *mask4 = nullptr;    // the caller's four logical masks as uploaded (4 x n words)
    int avg_strength = 0;
    bool first = true;           // no subcycle has run since the upload
    struct Captured { hipGraphExec_t exec; Ran ran; };
    std::map<GraphKey, Captured> graphs;     // the loop of a call as a graph, with what it did
    double t_loop_ms = 0;
    int t_nsub = 0;
    Ran last;                    // what the last call's schedule did
    double *tarear = nullptr, *post[5] = {};   // deformationsC_T: 1/tarea (static), divu shear vort rdg_conv rdg_shear
    // after the loop (evp_tail.hip): strintxU strintyU / strocn{x,y}T_iavg; U-point operands of dyn_finish (cdn_ocnU aiU uocnU vocnU
    // fmU), its strocnxU / yU; work1 / work2 of step_dyn_horiz (exchanged: the length of CG.f)
    struct Tail {
        double *out[2] = {}, *uin[5] = {}, *strocn[2] = {}, *work[2] = {};
        bool strocn_ok = false;                // strocn[] / uin[1] belong to the state the loop last ran on
    } tail;
    // preparation phase on the device (cice_evp_hip_cgrid_prep)
    struct Prep {
        bool geo = false, pending = false;     // pending: prepared, cice_evp_hip_cgrid_prep_finish not yet called
        uint8_t *tmask = nullptr, *xmask[3] = {};
        double *fcor[3] = {}, *t[11] = {}, *tmass = nullptr, *maskd = nullptr;
        int *c_dst = nullptr, *c_src = nullptr;
        signed char *c_vsign = nullptr;
        int n_center = 0;
        double *hwater = nullptr, *tbt = nullptr, *aicen = nullptr, *vicen = nullptr;
        int ncat = 0;
        std::vector<int32_t> h4;               // the four mask words as they come back
        double *prod[4] = {};                  // test build, forcing layout on: strairxE strairyN ss_tltxE ss_tltyN (EvpForcing::prod)
        cice_evp_hip_prep_params pp{};
        double t_ms = 0;
    } prep;
};
extern CGridState CG;

// ---- defined in evp_host_cgrid.cpp ----
bool march_avgs_switch();        // CICE_EVP_HIP_CGRID_MARCH_AVG_STRENGTH=1 (test build): avg_strength on the marched split schedules
bool res_cull();                 // CICE_EVP_HIP_CGRID_RES_CULL (test build): cg_res runs the windows with ice only
bool verbose();
bool geo_derived();              // cg_one and the marched kernel derive 15 of the 23 static arrays (the identities hold, the switch is on)
void fill(EvpCgrid &A);
bool remote();                   // ghost cells that other ranks own
bool fold_exchange();            // the blocks next to the tripole fold have more than one owner
size_t field_len();              // length of an exchanged array (with the staging slots of the fold exchange)
// ghost cells owned by other ranks, for a pair of arrays: the fold exchange, the remote pair (masked: through the masked halo
// where the host has handed one over), nothing on one rank
int exchange(double *a, double *b, bool masked);

// tripole: the fold step of up to four fields after the launch that produced them (what their ice_HaloUpdate does
// at the fold: points ON it averaged with their partners, ghost row beyond it mirrored); loc 0 centre, 1 NE corner,
// 2 E face, 3 N face; vec: vector kind (sign change across the fold)
struct FoldField { double *x; int loc; bool vec; };
void fold(const FoldField *fs, int n);
inline void fold(std::initializer_list<FoldField> fs) { fold(fs.begin(), (int)fs.size()); }

// The current and the other allocation of PP_FIELDS as a schedule sees them while it enqueues: swap() per subcycle, `swapped` for Ran
struct PingPong {
    double *cur[5], *alt[5];
    unsigned swapped = 0;
    PingPong()
    {
        for (int q = 0; q < 5; ++q) {
            cur[q] = CG.f[PP_FIELDS[q]];
            alt[q] = CG.alt[q];
        }
    }
    void swap(unsigned which)
    {
        for (int q = 0; q < 5; ++q)
            if (which >> q & 1u) std::swap(cur[q], alt[q]);
        swapped ^= which;
    }
    // a launch that works in place, and what the call leaves: the current allocations
    void at_current(EvpCgrid &A) const
    {
        for (int q = 0; q < 5; ++q) A.f[PP_FIELDS[q]] = cur[q];
    }
    // this subcycle writes the other allocations and reads the current ones
    void aim(EvpCgrid &A, unsigned which) const
    {
        for (int q = 0; q < 5; ++q)
            if (which >> q & 1u) A.f[PP_FIELDS[q]] = alt[q];
        if (which & PP_S12) A.s12_in = cur[4];
    }
    // bring the second allocations into line: both then agree on the cells no later subcycle writes (no ice; ghost cells nothing
    // is copied into)
    // (with the fold exchange both allocations carry the staging slots behind the cells: copied along)
    int sync(unsigned which) const
    {
        for (int q = 0; q < 5; ++q)
            if (which >> q & 1u) HIPC(hipMemcpyAsync(alt[q], cur[q], field_len() * sizeof(double), hipMemcpyDeviceToDevice, S.stream));
        return 0;
    }
};
// (the resident launch reads P.cur and leaves the final state in BOTH allocations: it swaps nothing)
int res_launch(const EvpCgrid &A, int nsub, bool dry, const PingPong &P);
int res_check_error();

// ---- defined in evp_host_cgrid_loop.cpp ----
CgSchedFacts sched_switches();   // the chooser's facts (cgrid_schedule.h) with the switches of the moment filled in and nothing else

}  // namespace evp_host
