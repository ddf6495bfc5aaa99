"""Seabed stress factors on the CPU: the numpy restatements of tests/seabed_ref.py against the reference's fixtures and the
oracle (oracle/evp_oracle.c), on the fixtures and on synthetic cells at every edge of the two methods, ncat 1, 2 and 5;
the extended-precision restatement against mpmath."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import seabed_ref as R
from common import GoldenCase, bits_equal

RHOI, RHOW, GRAVIT, PI, PUNY = 917.0, 1026.0, 9.80616, np.pi, 1e-11
K1, K2, ALPHAB, THR = 7.5, 15.0, 20.0, 30.0


def blocks_of(c: GoldenCase):
    return [tuple(int(v) for v in c.blk[b, :4]) for b in range(c.nblocks)]


def test_restatement_equals_reference_b_grid_fixtures():
    """TbU of the reference's evp() on the B-grid seabed fixtures (LKD; probabilistic with one and with five thickness
    categories), every call: the fp64 restatement reproduces it bit for bit."""
    c = GoldenCase("pop_cyc_2x2_seabed")
    s = c.scal
    for icall in range(1, c.ncalls + 1):
        dyn, tm, um = c.inputs(icall)
        tb = R.lkd(blocks_of(c), "U", s[24], s[25], s[26], s[27], c.d[f"pr{icall:02d}_aice"], c.d[f"pr{icall:02d}_vice"],
                   c.d["hwater"], um)
        assert np.abs(dyn["TbU"]).max() > 0 and bits_equal(tb, dyn["TbU"]), f"LKD call {icall}"
    for name in ("pop_cyc_2x2_seabedprob", "pop_cyc_2x2_seabedprob_ncat5"):
        c = GoldenCase(name)
        s = c.scal
        for icall in range(1, c.ncalls + 1):
            dyn, tm, um = c.inputs(icall)
            tbt, _ = R.prob_t(blocks_of(c), c.aicen(icall), c.vicen(icall), c.d["hwater"], tm, s[26], s[17], s[12],
                              s[19], s[30], s[31])
            tb = R.neighbor_max(blocks_of(c), "U", tbt, um)
            assert np.abs(dyn["TbU"]).max() > 0 and bits_equal(tb, dyn["TbU"]), f"{name} call {icall}"


@pytest.mark.parametrize("name", ["cgrid_cyc_1blk_seabed", "cgrid_trip_4x3_caps_seabed", "cgrid_cyc_2x2_seabedprob",
                                  "cgrid_cyc_2x2_seabedprob_ncat5"])
def test_restatement_equals_reference_c_grid_fixtures(name):
    """TbE / TbN of the reference's evp() with grid_ice = 'C' (LKD at E / N points on a cyclic and a tripole grid; the
    probabilistic method's face maximum): the fp64 restatement reproduces them bit for bit."""
    c = GoldenCase(name)
    s = c.scal
    t, _, _ = c.cgrid_prep_inputs(1)
    _, want, masks = c.cgrid_inputs(1)
    if s[29] != 0.0:
        tbt, _ = R.prob_t(blocks_of(c), c.aicen(1), c.vicen(1), c.d["hwater"], masks["iceTmask"], s[26], s[17],
                          s[12], s[19], s[30], s[31])
    for loc in "EN":
        if s[29] != 0.0:
            got = R.neighbor_max(blocks_of(c), loc, tbt, masks[f"ice{loc}mask"])
        else:
            got = R.lkd(blocks_of(c), loc, s[24], s[25], s[26], s[27], t["aice"], t["vice"], c.d["hwater"], masks[f"ice{loc}mask"])
        assert np.abs(want["Tb" + loc]).max() > 0 and bits_equal(got, want["Tb" + loc]), f"{name} Tb{loc}"


def synthetic_prob(ncat, per_family, seed, W=40):
    """One block, closed: T list ilo..ihi+1 x jlo..jhi+1 full of the edge families; random ice masks at U, E, N."""
    rng = np.random.default_rng(seed)
    n = per_family * len(R.PROB_FAMILIES)
    H = -(-n // (W + 1))
    shape = (1, H + 2, W + 2)
    blocks = [(2, W + 1, 2, H + 1)]
    where = np.zeros(shape, dtype=bool)
    where[0, 1:, 1:] = True
    aicen, vicen, hwater, fam = R.plant_prob(rng, where, ncat, per_family)
    tm = where.astype(np.int32)
    masks = {loc: (rng.random(shape) < 0.9).astype(np.int32) for loc in "UEN"}
    dom = oracle.OracleDomain(W + 2, H + 2, 1, W, H, "closed", "closed", [2], [W + 1], [2], [H + 1], [1], [1])
    return dom, blocks, aicen, vicen, hwater, fam, tm, masks


@pytest.mark.parametrize("ncat", [1, 2, 5])
def test_prob_restatement_equals_oracle_on_edge_families(ncat):
    """seabed_stress_factor_prob on >= 2000 synthetic cells across every edge family (atot at 0.05 and on either side of it
    by summation order, hwater at max_depth, thin and thick ice, narrow distributions, x_kmax on a category centre):
    restatement and oracle -- two readings of the reference -- agree bit for bit at U, E and N points."""
    dom, blocks, aicen, vicen, hwater, fam, tm, masks = synthetic_prob(ncat, 190, seed=100 + ncat)
    tbt, info = R.prob_t(blocks, aicen, vicen, hwater, tm, ALPHAB, RHOI, RHOW, GRAVIT, PI, PUNY)
    assert (fam >= 0).sum() >= 2000
    want = oracle.seabed_prob(dom, ALPHAB, RHOI, RHOW, GRAVIT, PI, PUNY, aicen, vicen, hwater, tm, masks["U"])
    assert bits_equal(R.neighbor_max(blocks, "U", tbt, masks["U"]), want)
    we, wn = oracle.seabed_prob_c(dom, ALPHAB, RHOI, RHOW, GRAVIT, PI, PUNY, aicen, vicen, hwater, tm, masks["E"], masks["N"])
    assert bits_equal(R.neighbor_max(blocks, "E", tbt, masks["E"]), we)
    assert bits_equal(R.neighbor_max(blocks, "N", tbt, masks["N"]), wn)
    # the families reach their edges
    F = {name: fam == f for f, name in enumerate(R.PROB_FAMILIES)}
    atot = np.zeros(hwater.shape)
    for c in range(ncat):
        atot = atot + aicen[:, c]
    assert (atot[F["atot_005"]] == 0.05).any() and ((atot[F["atot_005"]] > 0.05) & (tbt[F["atot_005"]] > 0)).any()
    assert (tbt[F["atot_005"] & (atot == 0.05)] == 0).all()
    if ncat >= 3:
        bwd = np.zeros(hwater.shape)
        for c in reversed(range(ncat)):
            bwd = bwd + aicen[:, c]
        flip = F["atot_order"] & ((atot > 0.05) != (bwd > 0.05))
        assert flip.sum() == F["atot_order"].sum() and (tbt[flip & (atot > 0.05)] > 0).any()
    assert (tbt[F["hw_50"] & (hwater == 50.0)] == 0).all() and (tbt[F["hw_50"] & (hwater < 50.0)] > 0).all()
    assert (tbt[F["thin"]] == 0).all() and (tbt[F["thick"]] > 0).all()
    ulp = info["ulp_to_xk"]
    assert (ulp[F["xk_edge"]] == 0).any() and (ulp[F["xk_edge"]] == 1).any() and (ulp[F["xk_edge"]] <= 1).all()
    for sig in ("1e-2", "1e-3", "1e-4"):
        s = info["sigma_i"][F["narrow_" + sig]]
        assert (s < 1.5 * float(sig)).all() and (tbt[F["narrow_" + sig]] > 0).mean() > 0.5, sig
    assert (tbt[F["generic"]] > 0).mean() > 0.5 and (ulp[F["generic"]] > 1e6).all()


@pytest.mark.parametrize("loc", ["U", "E", "N"])
def test_lkd_restatement_equals_oracle_on_edge_families(loc):
    """seabed_stress_factor_LKD on synthetic patches (hwater at threshold_hw and the double below it, hu < hcu, au = 1,
    deep water): restatement and oracle agree bit for bit at U, E and N points."""
    rng = np.random.default_rng(7)
    W, H = 60, 50
    shape = (1, H + 2, W + 2)
    a, v, h, fam = R.plant_lkd(rng, shape)
    mask = (rng.random(shape) < 0.9).astype(np.int32)
    dom = oracle.OracleDomain(W + 2, H + 2, 1, W, H, "closed", "closed", [2], [W + 1], [2], [H + 1], [1], [1])
    got = R.lkd([(2, W + 1, 2, H + 1)], loc, K1, K2, ALPHAB, THR, a, v, h, mask)
    want = (oracle.seabed_lkd(dom, K1, K2, ALPHAB, THR, a, v, h, mask) if loc == "U"
            else oracle.seabed_lkd_c(dom, loc, K1, K2, ALPHAB, THR, a, v, h, mask))
    assert bits_equal(got, want)
    hwu = np.full(shape, np.inf)                      # grid_neighbor_min(hwater) on the interior
    for di, dj in R.NEIGH[loc]:
        hwu[0, 1:-1, 1:-1] = np.minimum(hwu[0, 1:-1, 1:-1], h[0, 1 + dj:H + 1 + dj, 1 + di:W + 1 + di])
    on = mask != 0
    assert (got[on & (hwu == THR)] == 0).all() and (hwu == THR).sum() > 5
    assert (got[on & (hwu == np.nextafter(THR, 0.0))] > 0).sum() > 5
    F = {name: fam == f for f, name in enumerate(R.LKD_FAMILIES)}
    assert (got[F["hu_lt_hcu"] & on] == 0).any() and (got[F["au_1"] & on] > 0).any() and (got[F["generic"] & on] > 0).any()


def test_extended_restatement_against_mpmath():
    """The long-double restatement against the same expression tree in 50-digit arithmetic (fp64 inputs exact, the fp64
    decisions), on cells of every family with a factor: <= 1e-17 relative where sigma_i >= 0.05; on the narrow
    distributions the cancellation in v_i - m_i**2 amplifies the long double's rounding by ~ 1 / sigma_i**2, so there
    <= 1e-19 / sigma_i**2 (still far below the fp64 evaluation's error there)."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    rng = np.random.default_rng(5)
    cells = []
    for name in R.PROB_FAMILIES:
        if name in ("thin", "xk_edge"):
            continue
        A, V, H = R.prob_family_cells(name, 5, 6, rng)
        t, info = R.prob_cells(A, V, H, ALPHAB, RHOI, RHOW, GRAVIT, PI, PUNY)
        for q in np.flatnonzero(t > 0)[:2]:
            cells.append((name, A[q], V[q], H[q]))
    assert len(cells) >= 14
    for name, a, v, hw in cells:
        ext, info = R.prob_cells(a[None], v[None], np.array([hw]), ALPHAB, RHOI, RHOW, GRAVIT, PI, PUNY, ext=True)
        exact = _mp_prob(mp, a, v, hw)
        rel = abs(_ld_to_mp(mp, ext[0]) - exact) / exact
        sig = float(info["sigma_i"][0])
        assert rel <= (1e-17 if sig >= 0.05 else 1e-19 / sig ** 2), (name, float(rel), sig)


def _ld_to_mp(mp, x):
    m, e = np.frexp(x)                                  # long double -> exact mpf
    return mp.ldexp(mp.mpf(int(np.ldexp(m, 64))), int(e) - 64)


def _mp_prob(mp, a, v, hw):
    """seabed_stress_factor_prob's Tbt of one cell in mpmath, the decisions as fp64 takes them."""
    f = lambda x: mp.mpf(float(x))
    c1, c2 = mp.mpf(1), mp.mpf(2)
    atot = mp.fsum(f(x) for x in a)
    m_i = sum((f(x) for x in v), mp.mpf(0))
    v_i = sum((f(x) ** 2 / max(f(y), f(PUNY)) for x, y in zip(v, a)), mp.mpf(0))
    v_i = max(v_i - m_i ** 2, f(PUNY))
    mu_i = mp.log(m_i / mp.sqrt(c1 + v_i / m_i ** 2))
    sigma_i = mp.sqrt(mp.log(c1 + v_i / m_i ** 2))
    x_kmax = min(f(R.X_K[-1]), mp.exp(mu_i + mp.sqrt(c2 * sigma_i) * f(1.9430)))
    sb, wid_b = f(R.SIGMA_B), mp.mpf(6) * f(R.SIGMA_B) / 100
    y_n = [(f(hw) - 3 * sb) + (mp.mpf(k) - mp.mpf(0.5)) * wid_b for k in range(1, 101)]
    y64 = (hw - 3.0 * R.SIGMA_B) + (np.arange(1, 101) - 0.5) * (6.0 * R.SIGMA_B / 100)
    P_y = [mp.exp(-(y - f(hw)) ** 2 / (c2 * sb ** 2)) / (sb * mp.sqrt(c2 * f(PI))) * wid_b for y in y_n]
    tsum = mp.mpf(0)
    for k in range(100):
        x = f(R.X_K[k])
        if x > x_kmax:
            continue
        g = mp.exp(-(mp.log(x) - mu_i) ** 2 / (c2 * sigma_i ** 2)) / (x * sigma_i * mp.sqrt(c2 * f(PI)))
        ii = int((y64 <= RHOI * R.X_K[k] / RHOW).sum())
        if ii:
            sm = sum((P_y[n] * (f(RHOI) * x - f(RHOW) * y_n[n]) for n in range(ii)), mp.mpf(0))
            tsum += max(f(R.MU_S) * f(GRAVIT) * g * mp.mpf(0.5) * sm, mp.mpf(0))
    return tsum * mp.exp(-f(ALPHAB) * (c1 - atot))
