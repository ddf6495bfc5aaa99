// Host side of what runs between the last subcycle and transport on the B-grid state (kernels: evp_tail.hip):
//   cice_evp_hip_strocn_t           strocn{x,y}T_iavg of step_dyn_horiz          general/ice_step_mod.F90:1012-1041
//   cice_evp_hip_principal_stress   sig1, sig2, sigP of the history output       ice_dyn_shared.F90:1691-1747
// (the C grid's forms -- cice_evp_hip_cgrid_tail, cice_evp_hip_cgrid_strocn_t -- live beside its state, evp_host_cgrid.cpp)
#include "evp_host.h"

namespace evp_host {

void fill_tail(EvpTail &G)
{
    G.blk = S.blk;
    G.nx = S.d.nx_block;
    G.ny = S.d.ny_block;
    G.nblocks = S.d.nblocks;
    G.plane = S.plane;
}

// ice_HaloUpdate(a / b, halo_info, field_loc_NEcorner, field_type_vector) of two arrays of S.nuv doubles: the steps of
// halo_uv (evp_host_loop.cpp) with nothing masked and nothing left to a kernel's pushes -- copies inside the rank (an
// eliminated neighbour block: the fill value 0), the tripole seam with its top-row averaging, the exchange with the other
// ranks over the velocity lists.  Collective wherever the loop's velocity exchange is.
int halo_pair_unmasked(double *a, double *b)
{
    evp_launch_halo_local(a, b, S.h_local_dst, S.h_local_src, (const signed char *)S.h_local_sign, S.n_local, S.stream);
    if (S.plan.tail == 0) {
        // every seam pair and every ghost image of a seam cell on this rank
        evp_launch_halo_seam(a, b, nullptr, nullptr, S.h_seam_a, S.h_seam_b, S.n_seam, S.h_seam_pole, S.n_pole, S.h_late_dst, S.h_late_src,
                             (const signed char *)S.h_late_sign, S.n_late, S.stream);
        return halo_remote_pair(a, b, false, true);
    }
    // the seam row has several owners: the exchange carries the raw seam values into the staging slots behind the cells
    if (int rc = halo_remote_pair(a, b, false, true)) return rc;
    evp_launch_halo_seam_fin(a, b, nullptr, nullptr, S.h_fin_dst, S.h_fin_a, S.h_fin_b, (const signed char *)S.h_fin_coef, S.n_fin, S.stream);
    return 0;
}

}  // namespace evp_host

using namespace evp_host;

extern "C" {

// work = strocn{x,y}U / aiU where aiU /= 0 on the physical cells, 0 elsewhere; ice_HaloUpdate(work, NE corner, vector) over
// the plain halo; strocn{x,y}T_iavg = grid_average_X2YF('SW', work, uarea, tarea).  Operands: the strocnxU / yU the last
// cice_evp_hip_dyn_finish left on the device -- the caller's arrays with the ice U-cells rewritten, so off the ice what
// dyn_prep2 left there, +0 on every physical cell (ice_dyn_shared.F90:776-784) -- and this call's aiU.
int cice_evp_hip_strocn_t(const double *uarea, const double *tarea, double *strocnxT_iavg, double *strocnyT_iavg)
{
    if (!S.ready || !S.uploaded) return fail(-1, "state not uploaded");
    State::Tail &T = S.tail;
    if (!T.strocn || T.strocn_seq != S.upload_seq)
        return fail(-1, "cice_evp_hip_strocn_t: call cice_evp_hip_dyn_finish first (its strocnxU / strocnyU of this call stay on the device)");
    if ((!T.uarea && !uarea) || (!T.tarea && !tarea)) return fail(-1, "uarea and tarea needed on the first call");
    if (!T.uarea && S.mem.alloc(T.uarea, S.n, true)) return -1;
    if (!T.tarea && S.mem.alloc(T.tarea, S.n, true)) return -1;
    if (uarea && h2d(T.uarea, uarea)) return -1;
    if (tarea && h2d(T.tarea, tarea)) return -1;
    for (auto &p : T.work)
        if (!p && S.mem.alloc(p, S.nuv, true)) return -1;
    for (int k = 0; k < 2; ++k)
        if (!T.out[k] && S.mem.alloc(T.out[k], S.n, true)) return -1;
    EvpTail G;
    fill_tail(G);
    evp_launch_tail_divide(G, S.post_out[5], S.post_out[6], S.in[F_AIX], T.work[0], T.work[1], S.stream);
    if (int rc = halo_pair_unmasked(T.work[0], T.work[1])) return rc;
    evp_launch_tail_u2t_flux(G, T.work[0], T.work[1], T.uarea, T.tarea, T.out[0], T.out[1], S.stream);
    HIPC(hipGetLastError());
    if (strocnxT_iavg && d2h(strocnxT_iavg, T.out[0])) return -1;
    if (strocnyT_iavg && d2h(strocnyT_iavg, T.out[1])) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    if (int rc = direct_check_error()) return rc;
    return 0;
}

// principal_stress on corner 1 of the device stresses and the device strength, every cell of every block array (ghost cells
// included, as the reference's loop over 1..nx_block x 1..ny_block); sig = spval_dbl where strength <= puny.
int cice_evp_hip_principal_stress(double puny, double *sig1, double *sig2, double *sigP)
{
    if (!S.ready || !S.uploaded) return fail(-1, "state not uploaded");
    // (a resident launch whose waits gave up has left no final state)
    HIPC(hipStreamSynchronize(S.stream));
    if (int rc = resident_check_error()) return rc;
    State::Tail &T = S.tail;
    for (auto &p : T.out)
        if (!p && S.mem.alloc(p, S.n, true)) return -1;
    double *const *sig = S.sig[S.cur];
    evp_launch_tail_principal(S.n, sig[0], sig[4], sig[8], S.in[F_STRENGTH], puny, T.out[0], T.out[1], T.out[2], S.stream);
    HIPC(hipGetLastError());
    double *host[3] = {sig1, sig2, sigP};
    for (int k = 0; k < 3; ++k)
        if (host[k] && d2h(host[k], T.out[k])) return -1;
    HIPC(hipStreamSynchronize(S.stream));
    return 0;
}

}  // extern "C"
