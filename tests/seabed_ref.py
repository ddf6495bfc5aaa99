"""Test infrastructure: the seabed stress factors restated in numpy, twice, and synthetic cells at their edges.

  * fp64: seabed_stress_factor_LKD (ice_dyn_shared.F90:1386-1460) at U, E and N points and seabed_stress_factor_prob
    (:1475-1683) at T points, then U or E / N faces -- the reference's operations in its order, vectorised over cells,
    exp() / log() from the C library (math.exp / math.log), as the reference and the oracle call them.  A second reading
    of the reference, independent of oracle/evp_oracle.c.
  * extended: the same expression tree in np.longdouble (64-bit significand, expl / logl), the fp64 inputs taken as
    exact.  The discrete decisions (atot > 0.05, hwater < max_depth, ii) are taken as fp64 takes them; x_k > x_kmax is
    taken from the extended x_kmax.
Arrays: (nblocks, ny_block, nx_block); aicen / vicen: (nblocks, ncat, ny_block, nx_block) -- the memory image of the
reference's (nx, ny, ncat, nblocks).  blocks: [(ilo, ihi, jlo, jhi)] 1-based, per block.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
NI = NB = 100
MAX_DEPTH, MU_S, SIGMA_B = 50.0, 0.1, 2.5
X_K = 0.5 * (np.arange(1, NI + 1, dtype=np.float64) - 0.5)          # wid_i * (k - p5), every product exact
_exp, _log = np.frompyfunc(math.exp, 1, 1), np.frompyfunc(math.log, 1, 1)


def cexp(a):
    return np.asarray(_exp(np.asarray(a, dtype=np.float64)), dtype=np.float64)


def clog(a):
    return np.asarray(_log(np.asarray(a, dtype=np.float64)), dtype=np.float64)


# ---- LKD --------------------------------------------------------------------------------------------------------------
NEIGH = {"U": ((0, 0), (1, 0), (0, 1), (1, 1)), "E": ((0, 0), (1, 0)), "N": ((0, 0), (0, 1))}   # (di, dj), ice_grid.F90:4974-5009


def _nb(a, b, blk, di, dj):
    ilo, ihi, jlo, jhi = blk
    return a[b, jlo - 1 + dj:jhi + dj, ilo - 1 + di:ihi + di]


def lkd(blocks, loc, k1, k2, alphab, threshold_hw, aice, vice, hwater, mask):
    """TbU (loc 'U') / TbE / TbN on the cells of `mask` inside each block, 0 elsewhere."""
    out = np.zeros(aice.shape)
    for b, blk in enumerate(blocks):
        ilo, ihi, jlo, jhi = blk
        nb = NEIGH[loc]
        hwu, au, hu = (_nb(f, b, blk, *nb[0]) for f in (hwater, aice, vice))
        for d in nb[1:]:             # min / max(a, b, c, d) left to right
            hwu = np.minimum(hwu, _nb(hwater, b, blk, *d))
            au = np.maximum(au, _nb(aice, b, blk, *d))
            hu = np.maximum(hu, _nb(vice, b, blk, *d))
        docalc = np.where(hwu < threshold_hw, 1.0, 0.0)
        hcu = au * hwu / k1
        tb = docalc * k2 * np.maximum(0.0, hu - hcu) * cexp(-alphab * (1.0 - au))
        m = mask[b, jlo - 1:jhi, ilo - 1:ihi] != 0
        out[b, jlo - 1:jhi, ilo - 1:ihi] = np.where(m, tb, 0.0)
    return out


# ---- probabilistic method, per T cell -------------------------------------------------------------------------------
def prob_cells(acat, vcat, hw, alphab, rhoi, rhow, gravit, pi, puny, ext=False):
    """Tbt of cells given as rows: acat, vcat (ncell, ncat), hw (ncell,).  fp64, or (ext=True) long double.
    Returns (tbt, info); info: sel (the atot / depth decision), x_kmax (fp64 value; ext: the extended one too),
    ulp_to_xk (fp64 ulps from the fp64 x_kmax to the nearest x_k), sigma_i."""
    acat, vcat, hw = (np.asarray(x, dtype=np.float64) for x in (acat, vcat, hw))
    n, ncat = acat.shape
    atot = np.zeros(n)
    for c in range(ncat):
        atot = atot + acat[:, c]
    sel = (atot > 0.05) & (hw < MAX_DEPTH)
    out = np.zeros(n, dtype=LD if ext else np.float64)
    info = dict(sel=sel, x_kmax=np.full(n, np.nan), ulp_to_xk=np.full(n, np.inf), sigma_i=np.full(n, np.nan))
    if not sel.any():
        return out, info
    a, v, h = acat[sel], vcat[sel], hw[sel]
    ns = len(h)
    F = (lambda x: LD(x)) if ext else (lambda x: np.float64(x))
    ex, lg = (np.exp, np.log) if ext else (cexp, clog)
    c0, c1, c2, c3, c6, p5 = (F(x) for x in (0.0, 1.0, 2.0, 3.0, 6.0, 0.5))
    sigma_b, pi_, puny_, rhoi_, rhow_, gravit_, mu_s = (F(x) for x in (SIGMA_B, pi, puny, rhoi, rhow, gravit, MU_S))
    wid_i, wid_b = F(MAX_DEPTH) / NI, c6 * sigma_b / NB
    kk = np.arange(1, NB + 1, dtype=np.float64).astype(LD if ext else np.float64)
    x_k = wid_i * (kk - p5)
    mu_b = h.astype(x_k.dtype)
    y_n = (mu_b - c3 * sigma_b)[:, None] + (kk - p5)[None, :] * (c6 * sigma_b / NB)
    y64 = (h - 3.0 * SIGMA_B)[:, None] + (np.arange(1, NB + 1) - 0.5)[None, :] * (6.0 * SIGMA_B / NB)
    av, vv = a.astype(x_k.dtype), v.astype(x_k.dtype)
    m_i = np.zeros(ns, dtype=x_k.dtype)
    for c in range(ncat):
        m_i = m_i + vv[:, c]
    v_i = np.zeros(ns, dtype=x_k.dtype)
    for c in range(ncat):
        v_i = v_i + vv[:, c] * vv[:, c] / np.maximum(av[:, c], puny_)
    v_i = np.maximum(v_i - m_i * m_i, puny_)
    mu_i = lg(m_i / np.sqrt(c1 + v_i / (m_i * m_i)))
    sigma_i = np.sqrt(lg(c1 + v_i / (m_i * m_i)))
    xe = ex(mu_i + np.sqrt(c2 * sigma_i) * F(1.9430))
    x_kmax = np.minimum(x_k[-1], xe)          # cut = x_k(ncat_i): the loop that would lower it never runs (:1583-1590)
    lx = lg(x_k)[None, :] - mu_i[:, None]
    g_k = ex(-(lx * lx) / (c2 * (sigma_i * sigma_i))[:, None]) / ((x_k[None, :] * sigma_i[:, None]) * np.sqrt(c2 * pi_))
    dy = y_n - mu_b[:, None]
    b_n = ex(-(dy * dy) / (c2 * (sigma_b * sigma_b))) / (sigma_b * np.sqrt(c2 * pi_))
    P_x = np.where(x_k[None, :] > x_kmax[:, None], c0, g_k * wid_i)
    P_y = b_n * wid_b
    ii = (y64[:, :, None] <= (rhoi * X_K / rhow)[None, None, :]).sum(axis=1)       # (ns, NI): fp64 decision
    tsum = np.zeros(ns, dtype=x_k.dtype)
    rows = np.arange(ns)
    for k in range(NI):
        acc = np.add.accumulate(P_y * (rhoi_ * x_k[k] - rhow_ * y_n), axis=1)       # left to right
        iik = ii[:, k]
        sm = acc[rows, np.maximum(iik - 1, 0)]
        tb = np.where(iik == 0, c0, np.maximum(mu_s * gravit_ * P_x[:, k] * sm, c0))
        tsum = tsum + tb
    at = np.zeros(ns, dtype=x_k.dtype)
    for c in range(ncat):
        at = at + av[:, c]
    out[sel] = tsum * ex(-F(alphab) * (c1 - at))
    info["x_kmax"][sel] = x_kmax.astype(np.float64)
    info["sigma_i"][sel] = sigma_i.astype(np.float64)
    xe64 = xe.astype(np.float64)                  # before the cut: x_k(100) > x_kmax flips where it lies near cut
    d = np.abs(xe64[:, None] - X_K[None, :]) / np.spacing(X_K)[None, :]
    info["ulp_to_xk"][sel] = d.min(axis=1)
    if ext:
        info["x_kmax_ext"] = x_kmax
    return out, info


def prob_t(blocks, aicen, vicen, hwater, iceTmask, alphab, rhoi, rhow, gravit, pi, puny, ext=False):
    """Tbt on the T cells of dyn_prep2's list (ilo..ihi+1 x jlo..jhi+1 where iceTmask); returns (Tbt, info) with info
    arrays of the grid's shape (ulp_to_xk: inf off the computed cells)."""
    shp = hwater.shape
    tbt = np.zeros(shp, dtype=LD if ext else np.float64)
    ulp = np.full(shp, np.inf)
    sig = np.full(shp, np.nan)
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        js, is_ = slice(jlo - 1, jhi + 1), slice(ilo - 1, ihi + 1)
        m = iceTmask[b, js, is_] != 0
        ncat = aicen.shape[1]
        ac = np.stack([aicen[b, c, js, is_][m] for c in range(ncat)], axis=1)
        vc = np.stack([vicen[b, c, js, is_][m] for c in range(ncat)], axis=1)
        t, info = prob_cells(ac, vc, hwater[b, js, is_][m], alphab, rhoi, rhow, gravit, pi, puny, ext=ext)
        for arr, val in ((tbt, t), (ulp, info["ulp_to_xk"]), (sig, info["sigma_i"])):
            sub = arr[b, js, is_]
            sub[m] = val
            arr[b, js, is_] = sub
    return tbt, dict(ulp_to_xk=ulp, sigma_i=sig)


def neighbor_max(blocks, loc, tbt, mask):
    """grid_neighbor_max(Tbt, loc) on the cells of `mask` inside each block, 0 elsewhere (dtype of tbt)."""
    out = np.zeros(tbt.shape, dtype=tbt.dtype)
    for b, blk in enumerate(blocks):
        ilo, ihi, jlo, jhi = blk
        nb = NEIGH[loc]
        r = _nb(tbt, b, blk, *nb[0])
        for d in nb[1:]:
            r = np.maximum(r, _nb(tbt, b, blk, *d))
        m = mask[b, jlo - 1:jhi, ilo - 1:ihi] != 0
        out[b, jlo - 1:jhi, ilo - 1:ihi] = np.where(m, r, 0)
    return out


def argmax_t(blocks, loc, tbt, mask):
    """Flat index (into tbt) of the T cell whose Tbt grid_neighbor_max picks, per cell of `mask` (-1 elsewhere)."""
    out = np.full(tbt.shape, -1, dtype=np.int64)
    idx = np.arange(tbt.size).reshape(tbt.shape)
    for b, blk in enumerate(blocks):
        ilo, ihi, jlo, jhi = blk
        nb = NEIGH[loc]
        best, bi = _nb(tbt, b, blk, *nb[0]), _nb(idx, b, blk, *nb[0])
        for d in nb[1:]:
            x, xi = _nb(tbt, b, blk, *d), _nb(idx, b, blk, *d)
            bi = np.where(x > best, xi, bi)
            best = np.maximum(best, x)
        m = mask[b, jlo - 1:jhi, ilo - 1:ihi] != 0
        out[b, jlo - 1:jhi, ilo - 1:ihi] = np.where(m, bi, -1)
    return out


# ---- synthetic cells at the edges ------------------------------------------------------------------------------------
PROB_FAMILIES = ["generic", "empty_cats", "atot_005", "atot_order", "hw_50", "thin", "thick", "narrow_1e-2", "narrow_1e-3",
                 "narrow_1e-4", "xk_edge"]
WELL = ("generic", "empty_cats", "atot_005", "atot_order", "hw_50", "thin", "thick")     # sigma_i >= 0.05


def _seq(x):
    s = 0.0
    for v in x:
        s = s + v
    return s


def _split(rng, total, ncat, empty=False):
    """ncat parts of `total` whose left-to-right fp64 sum is `total` exactly (uneven; some zero when `empty`)."""
    for _ in range(200):
        w = rng.random(ncat) ** 2 + 0.05
        if empty and ncat > 1:
            w[rng.random(ncat) < 0.4] = 0.0
            if w.sum() == 0:
                w[0] = 1.0
        parts = total * w / w.sum()
        nzl = np.flatnonzero(parts)[-1]
        parts[nzl] = 0.0
        part = _seq(parts)
        parts[nzl] = total - part
        for _ in range(8):
            s = _seq(parts)
            if s == total:
                return parts
            parts[nzl] = np.nextafter(parts[nzl], np.inf if s < total else -np.inf)
    raise AssertionError("no exact split")


def _cell(rng, ncat, a, h, empty=False):
    """aicen / vicen of one cell: concentration a, mean thickness h, thickness rising with the category."""
    ac = _split(rng, a, ncat, empty)
    th = h * (0.4 + 1.2 * np.arange(ncat) / max(ncat - 1, 1)) if ncat > 1 else np.array([h])
    return ac, ac * th


def prob_family_cells(family, ncat, n, rng, puny=1e-11):
    """n cells (aicen (n, ncat), vicen (n, ncat), hwater (n,)) of one family of edges of seabed_stress_factor_prob."""
    A, V, H = np.zeros((n, ncat)), np.zeros((n, ncat)), np.zeros(n)
    for q in range(n):
        hw = 2.0 + 43.0 * rng.random() ** 3
        if family in ("generic", "empty_cats"):
            a, v = _cell(rng, ncat, 0.3 + 0.65 * rng.random(), 0.5 + 5.0 * rng.random(), family == "empty_cats")
        elif family == "atot_005":           # atot == 0.05 (no factor) or the next double above it
            tot = 0.05 if q % 2 == 0 else np.nextafter(0.05, 1.0)
            a, v = _cell(rng, ncat, tot, 1.0 + 3.0 * rng.random())
        elif family == "atot_order":         # left-to-right sum on the other side of 0.05 than right-to-left
            if ncat < 3:
                tot = 0.05 if q % 2 == 0 else np.nextafter(0.05, 1.0)
                a, v = _cell(rng, ncat, tot, 2.0)
            else:
                while True:
                    a = 0.05 * (rng.random(ncat) + 0.5)
                    a = a / a.sum() * 0.05
                    a = a + rng.integers(-4, 5, ncat) * np.spacing(a)
                    fwd, bwd = _seq(a), _seq(a[::-1])
                    if (fwd > 0.05) != (bwd > 0.05):
                        break
                v = a * (0.5 + 3.0 * rng.random())
        elif family == "hw_50":              # hwater == max_depth (no factor) or the next double below
            a, v = _cell(rng, ncat, 0.9, 20.0 + 10.0 * rng.random())
            hw = 50.0 if q % 2 == 0 else np.nextafter(50.0, 0.0)
        elif family == "thin":               # x_kmax below x_k(1): every P_x is 0
            a, v = _cell(rng, ncat, 0.5 + 0.4 * rng.random(), 0.002 + 0.01 * rng.random())
        elif family == "thick":              # x_kmax above cut = x_k(100)
            a, v = _cell(rng, ncat, 0.6 + 0.3 * rng.random(), 35.0 + 10.0 * rng.random())
            hw = 2.0 + 40.0 * rng.random()
        elif family.startswith("narrow_"):   # one category, aice -> 1: sigma_i ~ sqrt(1 - aice); m_i within a few sigma_i
            sig = float(family.split("_")[1])    # of a category centre (elsewhere every g_k underflows to 0)
            a, v = np.zeros(ncat), np.zeros(ncat)
            c = int(rng.integers(ncat))
            a[c] = 1.0 - sig * sig * (0.5 + rng.random())
            v[c] = X_K[int(rng.integers(2, 12))] * np.exp(sig * (4.0 * rng.random() - 2.0))
            hw = 1.0 + 5.0 * rng.random()
        elif family == "xk_edge":            # fp64 x_kmax on a category centre x_k, or one ulp from it
            a, v, hw = _xk_edge_cell(rng, ncat, q % 3, puny)
        else:
            raise KeyError(family)
        A[q], V[q], H[q] = a, v, hw
    return A, V, H


def _xkmax64(a, m, puny):
    """fp64 x_kmax of a one-category cell (aice a, vice m): the expression of prob_cells with scalars (C library
    exp / log); the zero categories add exact zeros."""
    v_i = max(m * m / max(a, puny) - m * m, puny)
    q = 1.0 + v_i / (m * m)
    return math.exp(math.log(m / math.sqrt(q)) + math.sqrt(2.0 * math.sqrt(math.log(q))) * 1.9430)


def _xk_edge_cell(rng, ncat, want_ulps, puny):
    """1-D search on m_i (one category, a fixed): fp64 x_kmax on a category centre x_k (want_ulps 0) or one ulp from it."""
    want = 0 if want_ulps == 0 else 1
    for _ in range(50):
        a = 0.6 + 0.3 * rng.random()
        target = X_K[int(rng.integers(6, 60))]
        lo, hi = 1e-3, 30.0
        if not (_xkmax64(a, lo, puny) < target < _xkmax64(a, hi, puny)):
            continue
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid in (lo, hi):
                break
            lo, hi = (mid, hi) if _xkmax64(a, mid, puny) < target else (lo, mid)
        for s in range(600):
            m = hi + (s // 2 + 1) * (1 if s % 2 else -1) * np.spacing(hi)
            if abs(_xkmax64(a, m, puny) - target) / np.spacing(target) == want:
                c = int(rng.integers(ncat))
                aa, vv = np.zeros(ncat), np.zeros(ncat)
                aa[c], vv[c] = a, m
                return aa, vv, 3.0 + 30.0 * rng.random()
    raise AssertionError("no x_kmax on a category edge found")


LKD_FAMILIES = ["generic", "hw_thr", "hu_lt_hcu", "au_1", "deep"]


def lkd_family_cells(family, n, rng, threshold_hw=30.0, k1=7.5):
    """(aice, vice, hwater) of n T cells, planted as 2 x 2 patches so that every U / E / N point inside sees the edge."""
    a = 0.5 + 0.45 * rng.random(n)
    v = a * (0.5 + 4.0 * rng.random(n))
    h = 2.0 + 25.0 * rng.random(n)
    if family == "hw_thr":                # min(hwater) == threshold_hw (no factor) or the double below
        h = np.where(np.arange(n) % 2 == 0, threshold_hw, np.nextafter(threshold_hw, 0.0))
    elif family == "hu_lt_hcu":           # hu < hcu = au * hwu / k1: the factor is 0
        v = a * h / k1 * (0.2 + 0.7 * rng.random(n))
    elif family == "au_1":                # exp(0)
        a = np.ones(n)
        v = 3.0 + 4.0 * rng.random(n)
    elif family == "deep":
        h = threshold_hw + 1.0 + 40.0 * rng.random(n)
    return a, v, h


def plant_prob(rng, where, ncat, per_family, families=PROB_FAMILIES, fill_hw=60.0):
    """aicen / vicen (nblocks, ncat, ny, nx), hwater and a family label per T cell (-1: none): `per_family` cells of each
    family on random cells of `where`; every other cell has no ice and hwater = fill_hw."""
    shp = where.shape
    aicen, vicen = np.zeros((shp[0], ncat) + shp[1:]), np.zeros((shp[0], ncat) + shp[1:])
    hwater, fam = np.full(shp, fill_hw), np.full(shp, -1)
    idx = np.flatnonzero(where)
    rng.shuffle(idx)
    assert len(idx) >= per_family * len(families), (len(idx), per_family)
    for f, name in enumerate(families):
        cells = np.unravel_index(idx[f * per_family:(f + 1) * per_family], shp)
        A, V, H = prob_family_cells(name, ncat, per_family, rng)
        for c in range(ncat):
            aicen[cells[0], c, cells[1], cells[2]] = A[:, c]
            vicen[cells[0], c, cells[1], cells[2]] = V[:, c]
        hwater[cells], fam[cells] = H, f
    return aicen, vicen, hwater, fam


def plant_lkd(rng, shape, families=LKD_FAMILIES, patch=3):
    """aice, vice, hwater and a family label per T cell, in patches of patch x patch cells of one family."""
    nb, ny, nx = shape
    fam = rng.integers(len(families), size=(nb, -(-ny // patch), -(-nx // patch)))
    fam = np.repeat(np.repeat(fam, patch, axis=1), patch, axis=2)[:, :ny, :nx]
    a, v, h = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for f, name in enumerate(families):
        m = fam == f
        a[m], v[m], h[m] = lkd_family_cells(name, int(m.sum()), rng)
    return a, v, h, fam
