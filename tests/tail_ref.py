"""Test infrastructure: what the reference does between "last subcycle done" and "transport may start", restated in numpy fp64
in the reference's order of operations (numpy does not contract, so a strict comparison is by bit pattern), with the halo updates
through oracle.halo_update:

  cgrid_halo / cgrid_tail   the end of evp() for grid_ice = 'C'                    ice_dyn_evp.F90:1436-1443
                            ice_HaloUpdate(strintxE, halo_info, field_loc_Eface, field_type_vector), the same for strintyN at
                            the N face; strintxU = E2US(strintxE), strintyU = N2US(strintyN)
  x2ys                      grid_average_X2YS, dir 'N' and 'E'                     ice_grid.F90:4290-4308, 4332-4351
                            (E2US -> ('N', earea, epm), N2US -> ('E', narea, npm): the dispatch at :3997-4004;
                            work2 = c0 first: :4196)
  strocn_work               work = strocn{x,y}U / aiU where aiU /= 0, else 0       general/ice_step_mod.F90:1017-1034
  u2t_flux                  grid_average_X2YF('SW', work, uarea, out, tarea)       ice_grid.F90:4640, 4665-4683
  strocn_t                  the three steps of step_dyn_horiz                      general/ice_step_mod.F90:1012-1041
  principal_stress          sig1, sig2, sigP; spval_dbl where strength <= puny     ice_dyn_shared.F90:1726-1745,
                                                                                   ice_constants.F90:27

Arrays: (nblocks, ny_block, nx_block); blocks: per block (ilo, ihi, jlo, jhi), 1-based as type(block) holds them.

The library compiles these passes without FMA contraction in BOTH build modes (cice_amd/csrc/evp_tail.hip, as the preparation
kernels), so the fused build is compared by bit pattern too: against this restatement applied to the fused loop's own outputs.
The planted errors (fold_sign, swap_dirs, swap_neighbours) exist for the CPU tests: each must change the result."""
from __future__ import annotations

import numpy as np

import oracle

SPVAL_DBL = 1.0e30          # ice_constants.F90:27


def blocks_of(c):
    """(ilo, ihi, jlo, jhi) per block of a GoldenCase."""
    return [tuple(int(v) for v in c.blk[b, :4]) for b in range(c.nblocks)]


def blocks_of_decomp(dc, rank=0):
    return [(b.ilo, b.ihi, b.jlo, b.jhi) for b in dc.local_blocks(rank)]


def domain_of_decomp(dc, rank=0, ns=None):
    """OracleDomain of a rank's blocks; ns: another north-south boundary type (e.g. 'closed': the halo update without the fold)."""
    blks = dc.local_blocks(rank)
    return oracle.OracleDomain(dc.nx_block, dc.ny_block, len(blks), dc.nx_global, dc.ny_global, dc.ew, ns or dc.ns,
                               [b.ilo for b in blks], [b.ihi for b in blks], [b.jlo for b in blks], [b.jhi for b in blks],
                               [b.gi0 for b in blks], [b.gj0 for b in blks])


def _halo(dom, a, loc, vector=True):
    out = np.array(a, dtype=np.float64, order="C", copy=True)
    return oracle.halo_update(dom, out, loc, "vector" if vector else "scalar")


def cgrid_halo(dom, strintxE, strintyN, fold_sign=True):
    """ice_dyn_evp.F90:1437-1440 on copies.  fold_sign=False: the sign change across the fold dropped (planted error)."""
    return _halo(dom, strintxE, "Eface", fold_sign), _halo(dom, strintyN, "Nface", fold_sign)


def _interior(shape, blocks):
    on = np.zeros(shape, dtype=bool)
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        on[b, jlo - 1:jhi, ilo - 1:ihi] = True
    return on


def _shift(a, di, dj):
    """a(i + di, j + dj) at (i, j); cells whose neighbour lies outside the block array get 0 (never an interior cell)."""
    out = np.zeros_like(a)
    ny, nx = a.shape[1:]
    js, jd = (slice(dj, ny), slice(0, ny - dj)) if dj >= 0 else (slice(0, ny + dj), slice(-dj, ny))
    is_, id_ = (slice(di, nx), slice(0, nx - di)) if di >= 0 else (slice(0, nx + di), slice(-di, nx))
    out[:, jd, id_] = a[:, js, is_]
    return out


def x2ys(blocks, work1, wght1, mask1, direction):
    """grid_average_X2YS, dir 'N': (i, j), (i, j+1); 'E': (i, j), (i+1, j)."""
    di, dj = {"N": (0, 1), "E": (1, 0)}[direction]
    w0, m0, s0 = (np.asarray(x, dtype=np.float64) for x in (wght1, mask1, work1))
    w1, m1, s1 = _shift(w0, di, dj), _shift(m0, di, dj), _shift(s0, di, dj)
    wtmp = (m0 * w0 + m1 * w1)
    on = _interior(s0.shape, blocks) & (wtmp != 0.0)
    num = (m0 * s0 * w0 + m1 * s1 * w1)
    out = np.zeros_like(s0)
    out[on] = num[on] / wtmp[on]
    return out


def cgrid_tail(dom, blocks, strintxE, strintyN, static, fold_sign=True, swap_dirs=False):
    """The four arrays cice_evp_hip_cgrid_tail returns.  swap_dirs: 'N' and 'E' swapped (planted error)."""
    sx, sy = cgrid_halo(dom, strintxE, strintyN, fold_sign)
    dx, dy = ("E", "N") if swap_dirs else ("N", "E")
    return dict(strintxE=sx, strintyN=sy,
                strintxU=x2ys(blocks, sx, static["earea"], static["epm"], dx),
                strintyU=x2ys(blocks, sy, static["narea"], static["npm"], dy))


def strocn_work(blocks, strocnU, aiU):
    s, a = np.asarray(strocnU, dtype=np.float64), np.asarray(aiU, dtype=np.float64)
    on = _interior(s.shape, blocks) & (a != 0.0)
    out = np.zeros_like(s)
    out[on] = s[on] / a[on]
    return out


def u2t_flux(blocks, work1, uarea, tarea, swap_neighbours=False):
    """grid_average_X2YF 'SW'.  swap_neighbours: the (i-1, j) and (i, j-1) terms take each other's place in the sum (planted
    error: the same four products added in another order -- only the rounding moves, and only where uarea is not symmetric)."""
    w, ua, ta = (np.asarray(x, dtype=np.float64) for x in (work1, uarea, tarea))
    west, south = (-1, 0), (0, -1)
    if swap_neighbours:
        west, south = south, west
    acc = w * ua
    acc = acc + _shift(w, *west) * _shift(ua, *west)
    acc = acc + _shift(w, *south) * _shift(ua, *south)
    acc = acc + _shift(w, -1, -1) * _shift(ua, -1, -1)
    on = _interior(w.shape, blocks)
    out = np.zeros_like(w)
    out[on] = (0.25 * acc[on]) / ta[on]
    return out


def strocn_t(dom, blocks, strocnxU, strocnyU, aiU, uarea, tarea, swap_neighbours=False, land_ghosts=None):
    """strocnxT_iavg, strocnyT_iavg.  dom=None: no halo update at all (ghost cells of work stay 0).  land_ghosts: the ghost
    cells whose source lies in an eliminated land block -- ice_HaloUpdate leaves its fill value 0 there (ice_boundary.F90:1298-1380:
    the ghost cells of inner block edges are filled first, nothing is copied over them); the oracle's halo update, which gathers
    the blocks it is given into a global array, has no value for such cells."""
    out = {}
    for k, s in (("strocnxT_iavg", strocnxU), ("strocnyT_iavg", strocnyU)):
        work = strocn_work(blocks, s, aiU)
        if dom is not None:
            work = _halo(dom, work, "NEcorner")
            if land_ghosts is not None:
                work[land_ghosts] = 0.0
        out[k] = u2t_flux(blocks, work, uarea, tarea, swap_neighbours)
    return out


def principal_stress(stressp, stressm, stress12, strength, puny):
    sp, sm, s12, st = (np.asarray(x, dtype=np.float64) for x in (stressp, stressm, stress12, strength))
    on = st > puny
    safe = np.where(on, st, 1.0)
    root = np.sqrt(sm * sm + 4.0 * (s12 * s12))
    sig1 = np.where(on, (0.5 * (sp + root)) / safe, SPVAL_DBL)
    sig2 = np.where(on, (0.5 * (sp - root)) / safe, SPVAL_DBL)
    sigP = np.where(on, -0.5 * sp, SPVAL_DBL)
    return dict(sig1=sig1, sig2=sig2, sigP=sigP)
