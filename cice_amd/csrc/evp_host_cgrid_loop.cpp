// =====================================================================
// C-grid EVP subcycle loop behind cice_evp_hip_cgrid_subcycle: which schedule a call runs is one value (cgrid_schedule.h:
// cg_choose_schedule on the facts sched_facts() states), the enqueue_* functions put its launches, exchanges and fold steps on
// the stream -- as a captured graph wherever the transport allows --, cgrid_schedule() describes it.  State and shared helpers:
// evp_host_cgrid.h.
// =====================================================================
#include "evp_host_cgrid.h"

namespace evp_host {

// ---- switches the loop reads: each is read here and nowhere else.  env_test(): the test build only (evp_host.h) ----
static bool one_switch() { return env_on(env("CICE_EVP_HIP_CGRID_ONE"), true); }     // =0: neither cg_one nor the marched kernel
static bool fused_switch() { return env_on(env_test("CICE_EVP_HIP_CGRID_FUSED"), true); }
static bool march_ranks_switch() { return env_on(env_test("CICE_EVP_HIP_CGRID_MARCH_RANKS"), true); }
static int march_fold_switch() { return env_int(env_test("CICE_EVP_HIP_CGRID_MARCH_FOLD"), ENV_UNSET); }
static int march_fold_ranks_switch() { return env_int(env_test("CICE_EVP_HIP_CGRID_MARCH_FOLD_RANKS"), ENV_UNSET); }
static bool march_fold_serial() { return env_on(env_test("CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL"), false); }
static bool strip_last_on() { return env_on(env_test("CICE_EVP_HIP_CGRID_STRIP_LAST"), true); }
static bool strip_ride_on() { return env_on(env_test("CICE_EVP_HIP_CGRID_STRIP_RIDE"), true); }
static bool one_xcd_on() { return env_on(env_test("CICE_EVP_HIP_CGRID_ONE_XCD"), true); }
static int resident_switch() { return env_int(env("CICE_EVP_HIP_CGRID_RESIDENT"), -1); }     // 0 / 1 forces the verdict

// Where the five phases exchange and fold -- the points at which the reference calls ice_HaloUpdate in a subcycle, after the phase
// that produces the fields: the pairs that travel to other ranks, in this order and pairing (a peer on another schedule of the five
// phases matches them because it reads the same table), then ONE fold step of the point's fields (index of CG.f, location, vector)
struct ExchangePairs { int n; int f[2][2]; };
struct PhasePoint { ExchangePairs x; int nfold; struct { int f, loc; bool vec; } fold[4]; };
static const PhasePoint AFTER_PHASE[5] = {
    {{1, {{CF_SHEARU, CF_SHEARU}}}, 1, {{CF_SHEARU, 1, false}}},
    {{2, {{CF_ETA, CF_ZETA}, {CF_SP, CF_SM}}}, 4, {{CF_ZETA, 0, false}, {CF_ETA, 0, false}, {CF_SP, 0, false}, {CF_SM, 0, false}}},
    {{1, {{CF_S12U, CF_S12U}}}, 1, {{CF_S12U, 1, false}}},
    {{1, {{CF_UE, CF_VN}}}, 2, {{CF_UE, 2, true}, {CF_VN, 3, true}}},
    {{2, {{CF_UN, CF_VE}, {CF_UU, CF_VU}}}, 4, {{CF_UN, 3, true}, {CF_VE, 2, true}, {CF_UU, 1, true}, {CF_VU, 1, true}}}};
// The fused chain (three launches; zone marched + frame) exchanges the same pairs at ITS three points, and has no fold
static const ExchangePairs AFTER_FUSED[3] = {AFTER_PHASE[0].x, AFTER_PHASE[1].x, {2, {{CF_S12U, CF_S12U}, {CF_UE, CF_VN}}}};
// (on the arrays A names at this moment: a schedule that ping-pongs has aimed it at this subcycle's allocations)
static int exchange_pairs(const EvpCgrid &A, const ExchangePairs &x)
{
    for (int k = 0; k < x.n; ++k)
        if (int rc = exchange(A.f[x.f[k][0]], A.f[x.f[k][1]], true)) return rc;
    return 0;
}
// one fold step for the fields of these points together
static void fold_points(const EvpCgrid &A, std::initializer_list<int> points)
{
    FoldField fs[4];
    int n = 0;
    for (int p : points)
        for (int k = 0; k < AFTER_PHASE[p].nfold; ++k) fs[n++] = {A.f[AFTER_PHASE[p].fold[k].f], AFTER_PHASE[p].fold[k].loc, AFTER_PHASE[p].fold[k].vec};
    fold(fs, n);
}
static int after_phase(const EvpCgrid &A, int p)
{
    if (int rc = exchange_pairs(A, AFTER_PHASE[p].x)) return rc;
    fold_points(A, {p});
    return 0;
}

// The kernels push a cell into its ghost images only where there is ice; the reference's ice_HaloUpdate copies every
// cell.  The difference shows once per call: a cell WITHOUT ice whose ghost images hold something else than the cell
// itself -- a corner that lost its ice since the last step (dyn_prep2 zeroes stress12U on ilo..ihi x jlo..jhi only,
// iceUmask is never set on ghost cells: the ghost image keeps the old stress) -- is repaired by the reference's first
// exchange of the field.  Cells without ice do not change during a call, so one unconditional copy in the first
// subcycle, right after the launch that produces the field, leaves every ghost cell as the reference has it.
static void first_exchange_copies_everything(const EvpCgrid &A, std::initializer_list<int> fields)
{
    for (int f : fields) evp_launch_cgrid_phase(A, 9, f, S.stream);
}

// five launches per subcycle, any visc_method
static int enqueue_phases(const EvpCgrid &A, int ndte, bool first)
{
    for (int k = 0; k < ndte; ++k)
        for (int p = 0; p < 5; ++p) {
            evp_launch_cgrid_phase(A, p, 1, S.stream);
            if (first && k == 0) {
                // the first strain_rates_U still reads the caller's ghost values of uvelN / vvelE
                if (p == 0) {
                    evp_launch_cgrid_phase(A, 6, 1, S.stream);
                    evp_launch_cgrid_zero_cells(A, CG.zero_cells, CG.n_zero, S.stream);
                }
                if (p == 1) first_exchange_copies_everything(A, {CF_SP, CF_SM});
                if (p == 2) first_exchange_copies_everything(A, {CF_S12U});
            }
            if (int rc = after_phase(A, p)) return rc;
        }
    return 0;
}

// The marched kernel's arguments from a plan's items, and the buffers and tables as cg_one takes them (no window list)
struct StripArgs { EvpCgOne T; EvpCgStrip Z; };
static StripArgs strip_args(const PingPong &P, const MarchItems &M, const uint8_t *gmask)
{
    return {EvpCgOne{nullptr, nullptr, 0, 0, M.ex, M.ey, 0, P.cur[0], P.cur[1], P.cur[2], P.cur[3], CG.gslab, CG.inslab, S.n, nullptr, gmask},
            EvpCgStrip{M.items, M.nitems, ((M.nitems + 3) / 4 + 7) / 8, M.len}};
}
// the items of the plan a kind marches: the five-phase frame plan has its own, every other plan CG.one's
static const MarchItems &zone_of(int kind) { return kind == CG_ZONE_FRAME_PHASES ? CG.mf.zone : CG.one.zone; }

// The three schedules that march a zone beside the five list-driven phase kernels on the rest (s.kind: cg_marched_phases): "marched
// zone + fold band" (+ frame) under a fold, "zone marched + frame" on the five phases without one (the fold steps are no-ops there).
// s.sync: the second allocations have not been brought into line since the upload (another schedule ran the calls before this one)
static int enqueue_march_fold(EvpCgrid A, int ndte, bool first, const CgSchedule &s, Ran &ran)
{
    const CGridState::MarchFold &Q = CG.mf;
    const CellLists &R = Q.rest;
    PingPong P;
    // s.serial: zone first, then the rest, on one stream (test build, A/B)
    int k = 0;
    if (first) {
        // the first subcycle after an upload still reads the caller's uvelN, vvelE, uvel, vvel and repairs the ghost cells: the five
        // full phases, in place
        if (int rc = enqueue_phases(A, 1, true)) return rc;
        k = 1;
    }
    if (first || s.sync)
        if (int rc = P.sync(PP_ALL)) return rc;
    for (; k < ndte; ++k) {
        const int last = (k == ndte - 1);
        if (last && !s.strip_last) {
            // (A/B: the call's last subcycle without the marched kernel's LAST instantiation -- the five full phases, in place)
            P.at_current(A);
            if (int rc = enqueue_phases(A, 1, false)) return rc;
            break;
        }
        // both sets read the previous subcycle's buffers and own disjoint cells of this subcycle's
        P.aim(A, PP_ALL);
        // (no fold: the five-phase frame plan's own items, on the whole-domain view of the derived geometry)
        const StripArgs Z = strip_args(P, zone_of(s.kind), CG.tripole ? Q.gmask : CG.gmask);
        EvpCgBand B{R.cells, {R.wg[0], R.wg[1], R.wg[2], R.wg[3], R.wg[4]}, {R.nwg[0], R.nwg[1], R.nwg[2], R.nwg[3], R.nwg[4]},
                    P.cur[0], P.cur[1], P.cur[2], P.cur[3], P.cur[4], R.scr[0], R.scr[1], R.scr[2], R.scr[3], R.scr[4], R.scr[5]};
        if (s.serial) {
            evp_launch_cgrid_strip(A, Z.T, Z.Z, nullptr, s.fast, last, S.stream);
            evp_launch_cgrid_band(A, B, 0, S.stream);
        } else {
            // (the rest's first launch goes ahead of the marched kernel, which fills the chip)
            HIPC(hipEventRecord(CG.side.fork, S.stream));
            evp_launch_cgrid_band(A, B, 0, S.stream);
            HIPC(hipStreamWaitEvent(CG.side.st, CG.side.fork, 0));
            evp_launch_cgrid_strip(A, Z.T, Z.Z, nullptr, s.fast, last, CG.side.st);
            HIPC(hipEventRecord(CG.side.join, CG.side.st));
        }
        // several ranks: the exchanges of the five phases at their points (after_phase: a peer on the five full phases matches them),
        // each ahead of the fold step that follows it there, on this subcycle's allocations (A is aimed at them).
        // They read REST cells only (the plan's invariant) and write ghost cells and staging slots: the marched kernel runs beside them
        for (int p = 0; p < 5; ++p) {
            if (p == 4) {
                // the averages read the new velocities of both sets: the two meet again before them.  In the call's last subcycle over
                // the whole domain: the caller gets uvelN, vvelE, uvel, vvel of every cell
                if (!s.serial) HIPC(hipStreamWaitEvent(S.stream, CG.side.join, 0));
                // (and before a last subcycle that runs as the five full phases, which read them on every cell)
                if (last || (k == ndte - 2 && !s.strip_last)) evp_launch_cgrid_phase(A, 4, 1, S.stream);
                else evp_launch_cgrid_band(A, B, 4, S.stream);
            } else if (p > 0) {
                evp_launch_cgrid_band(A, B, p, S.stream);
            }
            if (int rc = after_phase(A, p)) return rc;
        }
        P.swap(PP_ALL);
        ++ran.count[s.kind];
    }
    ran.swapped = P.swapped;
    return 0;
}

// The fused chain's kinds: three launches per subcycle + one after the loop (evp_cgrid.hip; CG_THREE); stress12U ping-pongs, and
// with it -- one launch per subcycle (CG_ONE), zone marched + frame (CG_ZONE_FRAME) -- uvelE, vvelN, stresspT, stressmT.
// cg_one: every subcycle but the first after an upload (which still reads the caller's uvelN, vvelE, uvel, vvel; measured against the three launches: HISTORY.md).
// s.nres > 0: the last nres subcycles of the call run inside ONE launch of the on-chip resident kernel (evp_cgrid_res.hip)
static int enqueue_fused(EvpCgrid A, int ndte, bool first, const CgSchedule &s, Ran &ran)
{
    const bool one = s.kind == CG_ONE, march = s.kind == CG_ZONE_FRAME;
    const int fast = s.fast;
    PingPong P;
    if (first) {
        // the caller's ghost cells of stress12U are whatever dyn_prep left there (zero: iceUmask is never set on
        // ghost cells, ice_dyn_evp.F90:683-690); the reference repairs them with the first halo update, the fused
        // kernel recomputes neighbours from their previous value: make the previous values ghost-consistent first
        evp_launch_cgrid_phase(A, 9, CF_S12U, S.stream);
        if (int rc = exchange(P.cur[4], P.cur[4], true)) return rc;
        // (ghost cells of eliminated land blocks: zero in both buffers; no ice cell reads them before the first exchange)
        evp_launch_cgrid_zero_cells(A, CG.zero_cells, CG.n_zero, S.stream);
        if (int rc = P.sync(PP_S12)) return rc;
    }
    for (int k = 0; k < ndte - s.nres; ++k) {
        const int last = (k == ndte - 1);
        P.at_current(A);
        if (one && !(first && k == 0)) {
            const MarchItems &M = CG.one.zone;
            EvpCgOne T{CG.one.tab, CG.one.tiles, CG.one.ntiles, CG.one.per_xcd, CG.one.ox, CG.one.oy, one_xcd_on() ? 0 : 1,
                       P.cur[0], P.cur[1], P.cur[2], P.cur[3], CG.gslab, CG.inslab, S.n, CG.one.prof, s.geo ? CG.gmask : nullptr};
            P.aim(A, PP_ALL);
            if (M.nitems > 0 && T.gmask && !(last && !s.strip_last)) {
                // the interior of the blocks marched, the windows along their edges as before: both read the previous
                // subcycle's buffers only and own disjoint cells
                EvpCgOne E = T;
                E.tab = CG.one.tab_e; E.tiles = CG.one.tiles_e; E.ntiles = CG.one.ntiles_e; E.per_xcd = (CG.one.ntiles_e + 7) / 8;
                E.ox = M.ex; E.oy = M.ey;
                E.prof = nullptr;
                // (the edge windows on the second stream beside the marched kernel: measured no gain, 565 us against 552 -- a
                // 1024-thread workgroup does not fit beside the marched kernel's waves on a CU anyway)
                // windows of 32 x 8 ride in the marched kernel's launch; other shapes (A/B) get a launch of their own behind it
                const bool ride = E.ox == 32 && E.oy == 8 && strip_ride_on();
                evp_launch_cgrid_strip(A, T, strip_args(P, M, T.gmask).Z, ride ? &E : nullptr, fast, last, S.stream);
                if (!ride && E.ntiles > 0) evp_launch_cgrid_one(A, E, fast, last, S.stream);
            } else if (T.ntiles > 0) {
                evp_launch_cgrid_one(A, T, fast, last, S.stream);
            }
            P.swap(PP_ALL);
            ++ran.count[CG_ONE];
            continue;
        }
        if (march && !(first && k == 0)) {
            // the rectangles marched on the second stream, every other interior cell by the frame variants of the three fused kernels
            // here, with the exchanges of the fused schedule at their points: both read the previous subcycle's buffers, own disjoint
            // cells of this subcycle's, and meet again before the buffers swap
            const StripArgs Z = strip_args(P, CG.one.zone, CG.gmask);
            const CellLists &Q = CG.fr;
            EvpCgFrame Fr{Q.cells, {Q.wg[0], Q.wg[1], Q.wg[2]}, {Q.nwg[0], Q.nwg[1], Q.nwg[2]}, P.cur[0], P.cur[1], P.cur[2], P.cur[3],
                          Q.scr[0], Q.scr[1], Q.scr[2], Q.scr[3]};
            P.aim(A, PP_ALL);
            // (the frame's first launch goes ahead of the marched kernel, which fills the chip: DESIGN.md section 7)
            HIPC(hipEventRecord(CG.side.fork, S.stream));
            evp_launch_cgrid_frame(A, Fr, 0, fast, last, S.stream);
            HIPC(hipStreamWaitEvent(CG.side.st, CG.side.fork, 0));
            evp_launch_cgrid_strip(A, Z.T, Z.Z, nullptr, fast, last, CG.side.st);
            HIPC(hipEventRecord(CG.side.join, CG.side.st));
            if (int rc = exchange_pairs(A, AFTER_FUSED[0])) return rc;
            evp_launch_cgrid_frame(A, Fr, 1, fast, last, S.stream);
            if (int rc = exchange_pairs(A, AFTER_FUSED[1])) return rc;
            evp_launch_cgrid_frame(A, Fr, 2, fast, last, S.stream);
            if (int rc = exchange_pairs(A, AFTER_FUSED[2])) return rc;
            HIPC(hipStreamWaitEvent(S.stream, CG.side.join, 0));
            P.swap(PP_ALL);
            ++ran.count[CG_ZONE_FRAME];
            continue;
        }
        if (first && k == 0 && CG.avg_strength) {
            // (only with cg_one for the rest: cg_fused) the first subcycle as the five launches, stress12U in place
            evp_launch_cgrid_phase(A, 0, 1, S.stream);
            evp_launch_cgrid_phase(A, 6, 1, S.stream);
            evp_launch_cgrid_phase(A, 1, 1, S.stream);
            first_exchange_copies_everything(A, {CF_SP, CF_SM});
            evp_launch_cgrid_phase(A, 2, 1, S.stream);
            first_exchange_copies_everything(A, {CF_S12U});
            evp_launch_cgrid_phase(A, 3, 1, S.stream);
            if (int rc = P.sync(PP_ALL)) return rc;
            continue;
        }
        if (first && k == 0) {
            evp_launch_cgrid_phase(A, 0, 1, S.stream);
            evp_launch_cgrid_phase(A, 6, 1, S.stream);
        } else {
            evp_launch_cgrid_phase(A, 7, last, S.stream);
        }
        if (int rc = exchange_pairs(A, AFTER_FUSED[0])) return rc;
        evp_launch_cgrid_phase(A, 10, last, S.stream);
        if (first && k == 0) first_exchange_copies_everything(A, {CF_SP, CF_SM});   // (stress12U: above, before the loop)
        if (int rc = exchange_pairs(A, AFTER_FUSED[1])) return rc;   // (zetax2T is stored in the last subcycle only; harmless before)
        P.aim(A, PP_S12);
        evp_launch_cgrid_phase(A, fast ? 11 : 8, last, S.stream);
        if (int rc = exchange_pairs(A, AFTER_FUSED[2])) return rc;
        P.swap(PP_S12);
        if ((one || march) && first && k == 0)          // the four others ping-pong from the next subcycle on
            if (int rc = P.sync(PP_FOUR)) return rc;
    }
    P.at_current(A);
    ran.swapped = P.swapped;
    if (s.nres > 0)
        if (int rc = res_launch(A, s.nres, false, P)) return rc;
    evp_launch_cgrid_phase(A, 4, 1, S.stream);
    return after_phase(A, 4);          // (no fold on these kinds: the exchanges alone)
}

// tripole (u-fold) on one rank: the first subcycles as five launches + fold steps, the last nres inside ONE launch of the on-chip
// resident kernel's FOLD variant, then the fold step of everything that launch leaves (ghost row beyond the fold; the points ON the fold
// come out averaged already, and the step leaves an averaged pair as it is) and the velocity averages after the loop
static int enqueue_phases_resident(const EvpCgrid &A, int ndte, bool first, int nres, Ran &ran)
{
    if (ndte > nres)
        if (int rc = enqueue_phases(A, ndte - nres, first)) return rc;
    ran = Ran{};       // (the five phases run in place, the resident launch leaves its result in both allocations)
    if (int rc = res_launch(A, nres, false, PingPong())) return rc;
    fold_points(A, {0, 2});
    fold_points(A, {1});
    fold_points(A, {3});
    evp_launch_cgrid_phase(A, 4, 1, S.stream);
    fold_points(A, {4});
    return 0;
}

// the facts of the moment for the schedule's chooser (cgrid_schedule.h); ndte: the call's subcycles, 0 outside a call
static CgSchedFacts sched_facts(int ndte);

// eligible in this call: one rank, no fold (either visc_method, classic or revised EVP), the default-configuration shortcuts hold on every ice cell, the static
// identities hold (the kernel takes -1 for a boundary ratio away from a coast), every window co-resident
// per_call (may be NULL): set when what stands in the way holds for THIS call only (the call's masks, operands, state)
// rides: the schedule is one the kernel can take the end of (cg_res_rides; a u-fold on one rank: the kernel's FOLD variant, the first
// subcycle of a call runs as the five phases).  Called with rides = true it answers what the kernel asks beside the schedule
// (CgSchedFacts::res_ok)
static bool res_eligible(bool rides, std::string *why = nullptr, bool *per_call = nullptr)
{
    auto no = [&](const char *w) { if (why) *why = w; return false; };
    const CGridState::Res &Q = CG.res;
    if (per_call) *per_call = false;
    if (!rides)
        return no(CG.tripole ? "a T-fold, or several ranks on a tripole grid" : "several ranks, a block too small, or the one-launch schedule switched off");
    if (!Q.tab) return no(Q.why.empty() ? "tables not built" : Q.why.c_str());
    if (CG.tripole ? !Q.gmask : !geo_derived()) return no("a start-up identity of the static arrays does not hold");
    if (per_call) *per_call = true;
    if (!Q.pairs_state_ok) return no("ghost cells outside the domain that the kernel treats as one position hold different state");
    if (Q.n_live < 1) return no("no window holds ice");
    // (seabed stress, waterx / watery other than the ocean currents, rheofact != 1 on some ice cell: the kernel's SLOW variant, round 6)
    if ((long)(res_cull() ? Q.n_live : Q.ntiles) > Q.cap4[(CG.avg_strength ? 1 : 0) | (S.prm.revp != 0.0 ? 2 : 0) | (CG.fast ? 0 : 4)]) return no("more windows with ice than can be resident at once");
    return true;
}

// First eligible call: a dry run (the same work on the uploaded state, nothing written back) proves that every window is
// resident and gives the steady-state cost per subcycle.  CICE_EVP_HIP_CGRID_RESIDENT=0 / 1 forces the verdict.
static int res_decide(const EvpCgrid &A)
{
    CGridState::Res &Q = CG.res;
    if (Q.mode >= 0) return 0;
    const int want = resident_switch();
    std::string why;
    bool per_call = false;
    if (want == 0 || !res_eligible(cg_res_rides(sched_facts(0)), &why, &per_call)) {
        // forced on: only what can never change (tables, geometry, rank layout) is an error; a condition of this call's masks,
        // operands or state is a fall-back for this call, as it is once the kernel has run (res_subcycles)
        if (want == 1 && !per_call) return fail(-6, "resident C-grid kernel requested but not applicable: %s", why.c_str());
        if (verbose() && want != 0) std::fprintf(stderr, "[cice_evp_hip] C grid: on-chip resident kernel not used: %s\n", why.c_str());
        // (per-call conditions -- visc_method, the shortcuts -- may hold in a later call: stay undecided unless switched off)
        if (want == 0) Q.mode = 0;
        return 0;
    }
    if (want == 1) {       // forced on: no probe launches (profiles see real launches only); a window that is not resident shows at the next sync
        Q.mode = 1;
        return 0;
    }
    const PingPong P;
    const int nshort = 8, nlong = 40;
    float tl[2] = {0, 0}, ms = 0;
    for (int rep = 0; rep < 3; ++rep) {
        const int np = rep == 2 ? nlong : nshort;
        HIPC(hipEventRecord(S.ev2, S.stream));
        if (int rc = res_launch(A, np, true, P)) return rc;
        HIPC(hipEventRecord(S.ev3, S.stream));
        HIPC(hipStreamSynchronize(S.stream));
        if (res_check_error()) {
            if (want == 1) return -7;
            g_err.clear();
            Q.mode = 0;
            if (verbose()) std::fprintf(stderr, "[cice_evp_hip] C grid: on-chip resident kernel failed its probe, not used\n");
            return 0;
        }
        HIPC(hipEventElapsedTime(&ms, S.ev2, S.ev3));
        if (rep >= 1) tl[rep - 1] = ms;
    }
    Q.t_probe_ms = (tl[1] - tl[0]) / (nlong - nshort);
    Q.mode = 1;
    return 0;
}

CgSchedFacts sched_switches()
{
    CgSchedFacts f{};
    f.sw_one = one_switch();
    f.sw_fused = fused_switch();
    f.sw_march_ranks = march_ranks_switch();
    f.sw_march_fold = march_fold_switch();
    f.sw_march_fold_ranks = march_fold_ranks_switch();
    f.sw_march_avgs = march_avgs_switch();
    f.sw_serial = march_fold_serial();
    f.sw_strip_last = strip_last_on();
    return f;
}
static CgSchedFacts sched_facts(int ndte)
{
    CgSchedFacts f = sched_switches();
    f.one_tab = CG.one.tab != nullptr;
    f.remote = remote();
    f.tripole = CG.tripole;
    f.tfold = CG.tfold;
    f.geo = geo_derived();
    f.frame_plan = CG.fr.cells != nullptr;
    f.one_items = CG.one.zone.nitems > 0;
    f.rest_plan = CG.mf.rest.cells != nullptr;
    f.rest_items = CG.mf.zone.nitems > 0;
    f.by_size = CG.mf.by_size;
    f.rest_scr5 = CG.mf.rest.scr[5] != nullptr;
    f.avg_strength = CG.avg_strength;
    f.fast = CG.fast;
    f.res_mode = CG.res.mode;
    f.res_ok = res_eligible(true);
    f.ndte = ndte;
    f.first = CG.first;
    f.synced = CG.mf.synced;
    return f;
}

// cice_evp_hip_describe_path's C-grid line: the schedule the next call would run where it marches a zone, why not where that was asked
// for, the fold exchange; "" otherwise
std::string cgrid_schedule()
{
    char buf[400];
    CgSchedFacts F = sched_facts(0);
    F.sw_fused = 1;      // (the text has never looked at the test build's CICE_EVP_HIP_CGRID_FUSED)
    const int kind = cg_choose_schedule(F).kind;
    const MarchItems &M = zone_of(kind);
    const CGridState::MarchFold &Q = CG.mf;
    const char *avgs = CG.avg_strength ? ", avg_strength" : "";
    char fx[120] = "";
    if (fold_exchange())
        std::snprintf(fx, sizeof fx, " + fold exchange, fold rows on %d ranks (%d staging slots here)", S.plan.cg_fold_ranks, S.plan.cg_tail);
    // (a schedule is named once a state is uploaded; `kind` itself is the chooser's answer either way, and the "why not" branch
    // below asks it on purpose even before an upload: a rank that WOULD march beside the frame has nothing to explain)
    switch (CG.geo && CG.uploaded ? kind : CG_PHASES) {
    case CG_ZONE_FRAME:
        std::snprintf(buf, sizeof buf, "C grid: zone marched + frame (%ld cells in %d items beside %ld frame cells, fused chain and its exchanges)",
                      M.cells, M.nitems, CG.fr.ncells);
        return buf;
    case CG_ZONE_FRAME_PHASES:
        // (the text of CG_ZONE_FRAME up to the bracket: the same counters report it)
        std::snprintf(buf, sizeof buf, "C grid: zone marched + frame (%ld cells in %d items beside %ld rest cells, %ld of them frame cells, five phases "
                      "advance the frame with their exchanges, avg_strength)", M.cells, M.nitems, Q.rest.ncells, Q.frame_cells);
        return buf;
    case CG_MARCH_FOLD_RANKS:
        std::snprintf(buf, sizeof buf, "C grid: marched zone + fold band + frame, %d rows (%ld cells in %d items beside %ld rest cells, %ld of them frame "
                      "cells, five phases with their exchanges and fold steps%s)%s", Q.band_rows, M.cells, M.nitems, Q.rest.ncells, Q.frame_cells, avgs, fx);
        return buf;
    case CG_MARCH_FOLD:
        std::snprintf(buf, sizeof buf, "C grid: marched zone + fold band, %d rows (%ld cells in %d items beside %ld cells of the band and the block edges, "
                      "five phases and their fold steps%s)", Q.band_rows, M.cells, M.nitems, Q.rest.ncells, avgs);
        return buf;
    default:
        break;
    }
    if (CG.geo && CG.tripole && cg_march_fold_wanted(F, false) == 1 && kind != CG_MARCH_FOLD_RANKS) {
        // asked for and not in use: say why
        const char *w = (remote() && cg_march_fold_wanted(F, true) != 1) ? "several ranks" : !Q.rest.cells ? Q.why.c_str() :
                        !(CG.uploaded && CG.avg_strength) ? "" : !F.sw_march_avgs ? "visc_method = avg_strength" :
                        !Q.rest.scr[5] ? "visc_method = avg_strength, and its switch was not set when the geometry was" : "";
        if (*w) {
            std::snprintf(buf, sizeof buf, "C grid: five phases + fold steps (marched zone + fold band not in use: %s)", w);
            return buf;
        }
    }
    if (!CG.geo || !fold_exchange()) return "";
    return std::string("C grid: five phases") + fx;
}

}  // namespace evp_host

using namespace evp_host;

extern "C" {

int cice_evp_hip_cgrid_subcycle(int32_t ndte)
{
    if (!CG.uploaded) return fail(-1, "C-grid EVP: nothing uploaded");
    if (ndte < 0) return fail(-1, "ndte < 0");
    if (ndte == 0) return 0;
    EvpCgrid A;
    fill(A);
    if (int rc = res_check_error()) return rc;
    if (int rc = res_decide(A)) return rc;       // (first call: the on-chip resident kernel's probe; refuses loudly when forced on a rank it cannot serve)
    const CgSchedule s = cg_choose_schedule(sched_facts(ndte));
    Ran ran;
    auto enqueue = [&]() -> int {
        switch (s.kind) {
        case CG_THREE: case CG_ONE: case CG_ZONE_FRAME: return enqueue_fused(A, ndte, CG.first, s, ran);
        case CG_PHASES_RESIDENT: return enqueue_phases_resident(A, ndte, CG.first, s.nres, ran);
        case CG_ZONE_FRAME_PHASES: case CG_MARCH_FOLD: case CG_MARCH_FOLD_RANKS: return enqueue_march_fold(A, ndte, CG.first, s, ran);
        default: return enqueue_phases(A, ndte, CG.first);      // (CG_PHASES: in place)
        }
    };
    HIPC(hipEventRecord(S.ev0, S.stream));
    // (the resident launch carries a fresh epoch in its arguments: enqueued eagerly, with the few launches around it)
    if (s.nres == 0 && S.use_graph && (!remote() || S.direct.on)) {     // RCCL point-to-point is enqueued eagerly (as the B-grid loop does)
        const GraphKey key{ndte, CG.in_alt, CG.first, CG.avg_strength, s};
        auto it = CG.graphs.find(key);
        if (it == CG.graphs.end()) {
            hipGraph_t gr = nullptr;
            hipGraphExec_t ex = nullptr;
            HIPC(hipStreamBeginCapture(S.stream, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue();
            HIPC(hipStreamEndCapture(S.stream, &gr));
            if (rc) return rc;
            HIPC(hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0));
            (void)hipGraphDestroy(gr);
            it = CG.graphs.emplace(key, CGridState::Captured{ex, ran}).first;
        }
        HIPC(hipGraphLaunch(it->second.exec, S.stream));
        ran = it->second.ran;
    } else if (enqueue()) {
        return -1;
    }
    CG.mf.synced = cg_marched_phases(s.kind);
    // the current arrays are where the schedule left them
    for (int q = 0; q < 5; ++q)
        if (ran.swapped >> q & 1u) std::swap(CG.f[PP_FIELDS[q]], CG.alt[q]);
    CG.in_alt ^= ran.swapped;
    HIPC(hipEventRecord(S.ev1, S.stream));
    HIPC(hipGetLastError());
    CG.last = ran;
    CG.res.last_nsub = s.nres;
    CG.first = false;
    CG.t_nsub = ndte;
    return 0;
}

}  // extern "C"
