// grid_average_X2Y of the forcing from any source location to a U, E or N point (infrastructure/ice_grid.F90:3817-4036):
// the stencils of the preparation kernels' general instantiation (evp_prep.hip prep_average_prep2<true>,
// evp_cgrid_prep.hip cg_prep<true>).  Operation order of the reference; the including file keeps FMA contraction off.
//   same source and target   grid_average_X2Y_base (:3817-3841): the whole array, ghost cells included
//   'S' (state, masked)      grid_average_X2YS (:4159-4378): weights tarea / uarea / earea / narea, masks hm / uvm / epm / npm;
//                            0 where the weight sum is 0
//   'F' (flux)               grid_average_X2YF (:4616-4808): divided by the target's area
// Otherwise ghost cells are 0 (work2 = c0).
#pragma once

#include "evp_device.h"

namespace {

// cells the stencil reads, in the reference's order; returns their number (2 or 4).  Interior cells only (c - nx >= 0).
__device__ __forceinline__ int x2y_cells(int src, int dst, size_t c, int nx, size_t q[4])
{
    const size_t n = (size_t)nx;
    switch (src * 4 + dst) {
    case EVP_LOC_T * 4 + EVP_LOC_U: q[0] = c; q[1] = c + 1; q[2] = c + n; q[3] = c + n + 1; return 4;     // NE
    case EVP_LOC_T * 4 + EVP_LOC_E: q[0] = c; q[1] = c + 1; return 2;                                   // E
    case EVP_LOC_T * 4 + EVP_LOC_N: q[0] = c; q[1] = c + n; return 2;                                   // N
    case EVP_LOC_U * 4 + EVP_LOC_E: q[0] = c - n; q[1] = c; return 2;                                   // S
    case EVP_LOC_U * 4 + EVP_LOC_N: q[0] = c - 1; q[1] = c; return 2;                                   // W
    case EVP_LOC_E * 4 + EVP_LOC_U: q[0] = c; q[1] = c + n; return 2;                                   // N
    case EVP_LOC_E * 4 + EVP_LOC_N: q[0] = c - 1; q[1] = c; q[2] = c + n - 1; q[3] = c + n; return 4;   // NW
    case EVP_LOC_N * 4 + EVP_LOC_U: q[0] = c; q[1] = c + 1; return 2;                                   // E
    case EVP_LOC_N * 4 + EVP_LOC_E: q[0] = c - n; q[1] = c - n + 1; q[2] = c; q[3] = c + 1; return 4;   // SE
    }
    return 0;
}

// work2(c) of grid_average_X2Y(type, a, src, work2, dst); in: c is a physical cell of its block
__device__ __forceinline__ double x2y(bool flux, const EvpForcing &F, int src, int dst, const double *a, size_t c, int nx, bool in)
{
    if (src == dst) return a[c];
    if (!in) return 0.0;
    size_t q[4];
    const int k = x2y_cells(src, dst, c, nx, q);
    const double *w = F.area[src];
    if (flux) {
        double s = a[q[0]] * w[q[0]] + a[q[1]] * w[q[1]];
        if (k == 4) {
            s = s + a[q[2]] * w[q[2]];
            s = s + a[q[3]] * w[q[3]];
            return 0.25 * s / F.area[dst][c];
        }
        return 0.5 * s / F.area[dst][c];
    }
    const double *m = F.pm[src];
    double wtmp = m[q[0]] * w[q[0]] + m[q[1]] * w[q[1]];
    double s = m[q[0]] * a[q[0]] * w[q[0]] + m[q[1]] * a[q[1]] * w[q[1]];
    if (k == 4) {
        wtmp = wtmp + m[q[2]] * w[q[2]];
        wtmp = wtmp + m[q[3]] * w[q[3]];
        s = s + m[q[2]] * a[q[2]] * w[q[2]];
        s = s + m[q[3]] * a[q[3]] * w[q[3]];
    }
    if (wtmp == 0.0) return 0.0;
    return s / wtmp;
}

}  // namespace
