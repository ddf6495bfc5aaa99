// =====================================================================
// What runs AROUND the subcycle loop on a tripole grid whose fold rows are split over ranks (both grids): the centre fold
// step of the preparation's T-grid fields in one batch, and the tripoleT stress symmetrisation with partner values in staging
// slots.  Both are list-driven (two rows of the grid per array) and once per evp() call: two ordinary multi-workgroup
// launches each -- a gather into scratch (every read of the pass), then a scatter (every write) -- so that no read depends on
// a write of the same pass however many workgroups the list takes.  One thread per list entry (x) and array (y): the index
// loads are contiguous along x.  No FMA contraction: the fold's average is the reference's expression (evp_cgrid.hip:
// cg_fold_gather).
// =====================================================================
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "evp_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int FP_BLOCK = 256;

// ---- fold_center_batch: x[dst] = s * 0.5*(x[a] + isign*x[b])  (b >= 0, or -2: partner's block eliminated -> 0)
//                         x[dst] = s * x[a]                     (b == -1; a < 0: 0),   s = flip ? isign : 1
// an operand is a cell of the array or a staging slot n + t behind its cells (the arrays carry the exchange's tail)
__global__ __launch_bounds__(FP_BLOCK) void fold_center_gather(EvpFoldBatch F)
{
    const int k = blockIdx.x * FP_BLOCK + threadIdx.x, q = blockIdx.y;
    if (k >= F.n) return;
    const double *x = F.x[q];
    const int a = F.a[k], b = F.b[k];
    const double isign = F.isign[q];
    const double s = F.flip[k] ? isign : 1.0;
    const double xa = a >= 0 ? x[a] : 0.0;
    double v;
    if (b >= 0 || b == -2) v = s * (0.5 * (xa + isign * (b >= 0 ? x[b] : 0.0)));
    else v = s * xa;
    F.tmp[(size_t)q * F.n + k] = v;
}
__global__ __launch_bounds__(FP_BLOCK) void fold_center_scatter(EvpFoldBatch F)
{
    const int k = blockIdx.x * FP_BLOCK + threadIdx.x, q = blockIdx.y;
    if (k >= F.n) return;
    F.x[q][F.dst[k]] = F.tmp[(size_t)q * F.n + k];
}

// ---- stress_tfold_split (fold_prep_plan.h): entries [0, n) row NY of _1 / _2 <- partner array, [n, n + no) east-west ghost
// cells of row NY of _3 / _4 <- own array, [n + no, n + no + nc) north-west corner ghost cells of all four <- partner array.
// An operand < ncell is a cell, one >= ncell the staging slot whose raw value the exchange left in tails[array][slot - ncell].
__device__ __forceinline__ double stress_operand(const EvpStressTfold &T, int arr, int s)
{
    if (s < 0) return 0.0;
    return s < T.ncell ? T.sig[arr][s] : T.tails[(size_t)arr * T.ntail + (s - T.ncell)];
}
// which entries array q writes, and from which array
__device__ __forceinline__ bool stress_entry(const EvpStressTfold &T, int q, int k, int &dst, int &src, int &from)
{
    if (k < T.n) {
        if (q & 2) return false;
        dst = T.dst[k]; src = T.src[k]; from = q ^ 2;
    } else if (k < T.n + T.no) {
        if (!(q & 2)) return false;
        dst = T.odst[k - T.n]; src = T.osrc[k - T.n]; from = q;
    } else {
        dst = T.cdst[k - T.n - T.no]; src = T.csrc[k - T.n - T.no]; from = q ^ 2;
    }
    return true;
}
__global__ __launch_bounds__(FP_BLOCK) void stress_tfold_gather(EvpStressTfold T)
{
    const int k = blockIdx.x * FP_BLOCK + threadIdx.x, q = blockIdx.y, ntot = T.n + T.no + T.nc;
    if (k >= ntot) return;
    int dst, src, from;
    if (!stress_entry(T, q, k, dst, src, from)) return;
    T.tmp[(size_t)q * ntot + k] = stress_operand(T, from, src);
}
__global__ __launch_bounds__(FP_BLOCK) void stress_tfold_scatter(EvpStressTfold T)
{
    const int k = blockIdx.x * FP_BLOCK + threadIdx.x, q = blockIdx.y, ntot = T.n + T.no + T.nc;
    if (k >= ntot) return;
    int dst, src, from;
    if (!stress_entry(T, q, k, dst, src, from)) return;
    T.sig[q][dst] = T.tmp[(size_t)q * ntot + k];
}

// the cells an exchange of (a, b) sends, copied into two scratch arrays that stand in for them (arrays without a tail)
__global__ __launch_bounds__(FP_BLOCK) void fold_stage2(const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ a2,
                                                        double *__restrict__ b2, const int *__restrict__ cells, int n)
{
    const int t = blockIdx.x * FP_BLOCK + threadIdx.x;
    if (t >= n) return;
    const int c = cells[t];
    a2[c] = a[c];
    b2[c] = b[c];
}

}  // namespace

void evp_launch_fold_center_batch(const EvpFoldBatch &F, hipStream_t st)
{
    if (F.n <= 0 || F.narrays <= 0) return;
    const dim3 grid((F.n + FP_BLOCK - 1) / FP_BLOCK, F.narrays);
    hipLaunchKernelGGL(fold_center_gather, grid, dim3(FP_BLOCK), 0, st, F);
    hipLaunchKernelGGL(fold_center_scatter, grid, dim3(FP_BLOCK), 0, st, F);
}

void evp_launch_stress_tfold_split(const EvpStressTfold &T, hipStream_t st)
{
    const int ntot = T.n + T.no + T.nc;
    if (ntot <= 0) return;
    const dim3 grid((ntot + FP_BLOCK - 1) / FP_BLOCK, 12);
    hipLaunchKernelGGL(stress_tfold_gather, grid, dim3(FP_BLOCK), 0, st, T);
    hipLaunchKernelGGL(stress_tfold_scatter, grid, dim3(FP_BLOCK), 0, st, T);
}

void evp_launch_fold_stage2(const double *a, const double *b, double *a2, double *b2, const int *cells, int n, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(fold_stage2, dim3((n + FP_BLOCK - 1) / FP_BLOCK), dim3(FP_BLOCK), 0, st, a, b, a2, b2, cells, n);
}
