"""Independent numpy restatement of grid_average_X2Y for the forcing layouts of evp()'s preparation (the reference's
infrastructure/ice_grid.F90: grid_average_X2Y_base :3817-3841, the dispatch :3954-4036, grid_average_X2YS :4159-4378,
grid_average_X2YF :4616-4808).  Block arrays [nblocks][ny_block][nx_block]; the physical cells of block b are
ilo..ihi x jlo..jhi (1-based), as in cice_amd.decomp.  numpy's elementwise arithmetic rounds every operation (no fused
multiply-add), so the reference's operation order gives the reference's bits."""
from __future__ import annotations

import numpy as np

LOCS = ("T", "U", "E", "N")
# (di, dj) of the cells each average reads, in the reference's order (dir of the dispatch in the comment)
STENCIL = {
    ("T", "U"): [(0, 0), (1, 0), (0, 1), (1, 1)],        # NE
    ("T", "E"): [(0, 0), (1, 0)],                        # E
    ("T", "N"): [(0, 0), (0, 1)],                        # N
    ("U", "E"): [(0, -1), (0, 0)],                       # S
    ("U", "N"): [(-1, 0), (0, 0)],                       # W
    ("E", "U"): [(0, 0), (0, 1)],                        # N
    ("E", "N"): [(-1, 0), (0, 0), (-1, 1), (0, 1)],      # NW
    ("N", "U"): [(0, 0), (1, 0)],                        # E
    ("N", "E"): [(0, -1), (1, -1), (0, 0), (1, 0)],      # SE
}
# grid_ocn / grid_atm -> (dynu, dynv), general/ice_init.F90:2016-2055
GRID_LOC = {"A": ("T", "T"), "B": ("U", "U"), "C": ("E", "N")}


def x2y(kind: str, a, src: str, dst: str, area: dict, pm: dict, blocks) -> np.ndarray:
    """grid_average_X2Y(kind, a, src, work2, dst): kind 'S' (state, masked: weights area[src], masks pm[src]) or 'F' (flux:
    divided by area[dst]).  blocks: (ilo, ihi, jlo, jhi) per block."""
    a = np.asarray(a, dtype=np.float64)
    if src == dst:
        return a.copy()                          # the whole array, ghost cells included
    out = np.zeros_like(a)                       # work2 = c0
    st = STENCIL[(src, dst)]
    w = area[src]
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        def at(x, d):
            di, dj = d
            return x[b, jlo - 1 + dj:jhi + dj, ilo - 1 + di:ihi + di]
        J, I = slice(jlo - 1, jhi), slice(ilo - 1, ihi)
        if kind == "F":
            s = at(a, st[0]) * at(w, st[0])
            for d in st[1:]:
                s = s + at(a, d) * at(w, d)
            out[b, J, I] = (0.25 if len(st) == 4 else 0.5) * s / area[dst][b, J, I]
        else:
            m = pm[src]
            wt = at(m, st[0]) * at(w, st[0])
            s = at(m, st[0]) * at(a, st[0]) * at(w, st[0])
            for d in st[1:]:
                wt = wt + at(m, d) * at(w, d)
                s = s + at(m, d) * at(a, d) * at(w, d)
            out[b, J, I] = np.where(wt != 0.0, s / np.where(wt != 0.0, wt, 1.0), 0.0)
    return out


def layout_products(grid_ice: str, calc_strair: bool, ocn: str, atm: str, t: dict, area: dict, pm: dict, blocks) -> dict:
    """The averaged forcing evp()'s preparation makes (ice_dyn_evp.F90:433-489): uocnX, vocnX, ss_tltxX, ss_tltyX, strairxX,
    strairyX for X = U on the B grid; on the C grid uocnE / vocnE / uocnN / vocnN and the components dyn_prep2 reads:
    ss_tltxE, ss_tltyN, strairxE, strairyN.  t: uocn, vocn, ss_tltx, ss_tlty (ghost cells as after their halo update) and
    strairxT / strairyT (calc_strair, halo-updated) or strax / stray (as the host holds them)."""
    ou, ov = GRID_LOC[ocn]
    wu, wv = ("T", "T") if calc_strair else GRID_LOC[atm]
    wx, wy = (t["strairxT"], t["strairyT"]) if calc_strair else (t["strax"], t["stray"])
    if grid_ice == "B":
        return {"uocnU": x2y("S", t["uocn"], ou, "U", area, pm, blocks), "vocnU": x2y("S", t["vocn"], ov, "U", area, pm, blocks),
                "ss_tltxU": x2y("S", t["ss_tltx"], ou, "U", area, pm, blocks),
                "ss_tltyU": x2y("S", t["ss_tlty"], ov, "U", area, pm, blocks),
                "strairxU": x2y("F", wx, wu, "U", area, pm, blocks), "strairyU": x2y("F", wy, wv, "U", area, pm, blocks)}
    out = {}
    for X in ("E", "N"):
        out[f"uocn{X}"] = x2y("S", t["uocn"], ou, X, area, pm, blocks)
        out[f"vocn{X}"] = x2y("S", t["vocn"], ov, X, area, pm, blocks)
    out["ss_tltxE"] = x2y("S", t["ss_tltx"], ou, "E", area, pm, blocks)
    out["ss_tltyN"] = x2y("S", t["ss_tlty"], ov, "N", area, pm, blocks)
    out["strairxE"] = x2y("F", wx, wu, "E", area, pm, blocks)
    out["strairyN"] = x2y("F", wy, wv, "N", area, pm, blocks)
    return out
