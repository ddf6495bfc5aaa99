// =====================================================================
// After the subcycle loop, before transport: the passes between "last subcycle done" and "transport may start"
// that the reference runs on full arrays on the host.
//   tail_divide       work = strocn{x,y}U / aiU where aiU /= 0, else 0     general/ice_step_mod.F90:1017-1034
//   tail_u2t_flux     grid_average_X2YF('SW', work, uarea, out, tarea)     ice_grid.F90:4665-4683 (work2 = c0: :4640)
//   tail_x2ys         grid_average_X2YS('N' / 'E', ...): E2US / N2US       ice_grid.F90:4290-4351 (dispatch :3997-4004)
//   tail_principal    principal_stress                                     ice_dyn_shared.F90:1691-1747
//   tail_zero_cells   ghost cells next to an eliminated land block (ice_HaloUpdate's fill value, ice_boundary.F90:1298-1380)
// The halo updates between them are the loops' own exchanges, enqueued by the host (evp_host_tail.cpp, evp_host_cgrid.cpp).
// Not a hot path (once per evp() call): one thread per cell, lane i <-> column i so that every load of a wave is one
// contiguous run (the (i-1, j-1) reads of the 'SW' average are the same runs shifted by one element), operation order
// of the reference, no FMA contraction in either build mode -- as the preparation kernels (evp_prep.hip) -- so that the
// results are bit-identical to it whichever build made the loop's final state.
// =====================================================================
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "evp_device.h"

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ bool cell_of(const EvpTail &G, int &i, int &j, int &bz, size_t &c)
{
    i = blockIdx.x * blockDim.x + threadIdx.x + 1;
    j = blockIdx.y + 1;
    bz = blockIdx.z;
    if (i > G.nx) return false;
    c = (size_t)bz * G.plane + (size_t)(j - 1) * G.nx + (i - 1);
    return true;
}
__device__ __forceinline__ bool interior(const EvpTail &G, int i, int j, int bz)
{
    const int4 r = G.blk[bz];
    // (a block array always has its ghost cells around the physical ones: the second half keeps every stencil read of
    // the averages inside the block whatever the table says)
    return i >= r.x && i <= r.y && j >= r.z && j <= r.w && i >= 2 && j >= 2 && i < G.nx && j < G.ny;
}

__global__ void tail_divide(EvpTail G, const double *__restrict__ sx, const double *__restrict__ sy,
                            const double *__restrict__ ai, double *__restrict__ wx, double *__restrict__ wy)
{
    int i, j, bz; size_t c;
    if (!cell_of(G, i, j, bz, c)) return;
    double x = 0.0, y = 0.0;
    if (interior(G, i, j, bz)) {
        const double a = ai[c];
        if (a != 0.0) { x = sx[c] / a; y = sy[c] / a; }
    }
    wx[c] = x; wy[c] = y;
}

__global__ void tail_u2t_flux(EvpTail G, const double *__restrict__ wx, const double *__restrict__ wy,
                              const double *__restrict__ uarea, const double *__restrict__ tarea,
                              double *__restrict__ ox, double *__restrict__ oy)
{
    int i, j, bz; size_t c;
    if (!cell_of(G, i, j, bz, c)) return;
    double x = 0.0, y = 0.0;
    if (interior(G, i, j, bz)) {
        const size_t w = c - 1, s = c - G.nx, sw = s - 1;
        const double a0 = uarea[c], a1 = uarea[w], a2 = uarea[s], a3 = uarea[sw], t = tarea[c];
        x = 0.25 * (wx[c] * a0 + wx[w] * a1 + wx[s] * a2 + wx[sw] * a3) / t;
        y = 0.25 * (wy[c] * a0 + wy[w] * a1 + wy[s] * a2 + wy[sw] * a3) / t;
    }
    ox[c] = x; oy[c] = y;
}

// out(i,j) from src(i,j) and its neighbour `stride` elements on: stride = nx ('N': E2US), 1 ('E': N2US)
__global__ void tail_x2ys(EvpTail G, const double *__restrict__ src, const double *__restrict__ wght,
                          const double *__restrict__ msk, double *__restrict__ out, int stride)
{
    int i, j, bz; size_t c;
    if (!cell_of(G, i, j, bz, c)) return;
    double x = 0.0;
    if (interior(G, i, j, bz)) {
        const size_t c1 = c + stride;
        const double m0 = msk[c], m1 = msk[c1], w0 = wght[c], w1 = wght[c1];
        const double wtmp = (m0 * w0 + m1 * w1);
        if (wtmp != 0.0) x = (m0 * src[c] * w0 + m1 * src[c1] * w1) / wtmp;
    }
    out[c] = x;
}

__global__ void tail_principal(size_t n, const double *__restrict__ sp, const double *__restrict__ sm,
                               const double *__restrict__ s12, const double *__restrict__ strength, double puny,
                               double *__restrict__ sig1, double *__restrict__ sig2, double *__restrict__ sigP)
{
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    const double spval_dbl = 1.0e30;             // ice_constants.F90:27
    double o1 = spval_dbl, o2 = spval_dbl, oP = spval_dbl;
    const double st = strength[c];
    if (st > puny) {
        const double p = sp[c], m = sm[c], q = s12[c];
        oP = -0.5 * p;
        const double root = sqrt(m * m + 4.0 * (q * q));
        o1 = (0.5 * (p + root)) / st;
        o2 = (0.5 * (p - root)) / st;
    }
    sig1[c] = o1; sig2[c] = o2; sigP[c] = oP;
}

// dyn_finish (ice_dyn_shared.F90:1291-1365) at the U points of the C grid, which evp() calls for every grid_ice
// (ice_dyn_evp.F90:1395-1406): on the physical cells with iceUmask (mask bit `bit`), every other cell keeps its value
__global__ void tail_dyn_finish_u(EvpTail G, const uint8_t *__restrict__ mask, unsigned bit, double rhow, double cosw, double sinw,
                                  const double *__restrict__ Cw, const double *__restrict__ ai, const double *__restrict__ uocn,
                                  const double *__restrict__ vocn, const double *__restrict__ fm, const double *__restrict__ u,
                                  const double *__restrict__ v, double *__restrict__ strocnx, double *__restrict__ strocny)
{
    int i, j, bz; size_t c;
    if (!cell_of(G, i, j, bz, c)) return;
    if (!interior(G, i, j, bz) || !(mask[c] & bit)) return;
    const double uo = uocn[c], vo = vocn[c], uu = u[c], vv = v[c], f = fm[c];
    const double du = uo - uu, dv = vo - vv;
    double vrel = rhow * Cw[c] * sqrt(du * du + dv * dv);
    vrel = vrel * ai[c];
    strocnx[c] = vrel * ((uo - uu) * cosw - (vo - vv) * sinw * copysign(1.0, f));
    strocny[c] = vrel * ((vo - vv) * cosw + (uo - uu) * sinw * copysign(1.0, f));
}

__global__ void tail_zero_cells(double *__restrict__ a, double *__restrict__ b, const int *__restrict__ cells, int n)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int c = cells[k];
    a[c] = 0.0;
    b[c] = 0.0;
}

dim3 cell_grid(const EvpTail &G) { return dim3((G.nx + 63) / 64, G.ny, G.nblocks); }

}  // namespace

void evp_launch_tail_divide(const EvpTail &G, const double *sx, const double *sy, const double *ai, double *wx, double *wy,
                            hipStream_t st)
{
    hipLaunchKernelGGL(tail_divide, cell_grid(G), dim3(64), 0, st, G, sx, sy, ai, wx, wy);
}

void evp_launch_tail_u2t_flux(const EvpTail &G, const double *wx, const double *wy, const double *uarea, const double *tarea,
                              double *ox, double *oy, hipStream_t st)
{
    hipLaunchKernelGGL(tail_u2t_flux, cell_grid(G), dim3(64), 0, st, G, wx, wy, uarea, tarea, ox, oy);
}

void evp_launch_tail_x2ys(const EvpTail &G, const double *src, const double *wght, const double *msk, double *out, int north,
                          hipStream_t st)
{
    hipLaunchKernelGGL(tail_x2ys, cell_grid(G), dim3(64), 0, st, G, src, wght, msk, out, north ? G.nx : 1);
}

void evp_launch_tail_principal(size_t n, const double *sp, const double *sm, const double *s12, const double *strength,
                               double puny, double *sig1, double *sig2, double *sigP, hipStream_t st)
{
    if (n) hipLaunchKernelGGL(tail_principal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, sp, sm, s12, strength, puny, sig1, sig2, sigP);
}

void evp_launch_tail_dyn_finish_u(const EvpTail &G, const uint8_t *mask, unsigned bit, double rhow, double cosw, double sinw,
                                  const double *Cw, const double *ai, const double *uocn, const double *vocn, const double *fm,
                                  const double *u, const double *v, double *strocnx, double *strocny, hipStream_t st)
{
    hipLaunchKernelGGL(tail_dyn_finish_u, cell_grid(G), dim3(64), 0, st, G, mask, bit, rhow, cosw, sinw, Cw, ai, uocn, vocn, fm, u, v,
                       strocnx, strocny);
}

void evp_launch_tail_zero_cells(double *a, double *b, const int *cells, int n, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(tail_zero_cells, dim3((n + 255) / 256), dim3(256), 0, st, a, b, cells, n);
}
