"""Seabed stress factors on the device (cice_evp_hip_seabed_lkd / _prob, cice_evp_hip_cgrid_seabed_lkd / _prob) against the
oracle and the extended-precision restatement of tests/seabed_ref.py: both grids, both methods, ncat 1, 2 and 5, synthetic
cells at every edge of the two methods; the ghost-cell rules of the entries; calls that change ncat or keep hwater; the
TbU == 0 shortcut the B-grid entries derive from the device result."""
from __future__ import annotations

import numpy as np
import pytest

import oracle
import seabed_ref as R
from cice_amd import decomp, evp, synth
from common import GoldenCase, assert_bitwise, bits_equal, max_rel_err
from test_gpu_cgrid import cgrid_core, hip_prep_params
from test_gpu_parity import SIG, VEL, hip_from_case

pytestmark = pytest.mark.gpu

PPD = dict(dt=3600.0, rhoi=917.0, rhos=330.0, gravit=9.80616, dyn_area_min=1e-11, dyn_mass_min=1e-10)
ALPHAB, PI, PUNY, K1, K2, THR = 20.0, np.pi, 1e-11, 7.5, 15.0, 30.0
U = 2.0 ** -53
PER_FAMILY = 120            # x 11 families: ~1300 T cells through the extended evaluation per call
# device vs oracle (host libm), relative, per family: DESIGN.md's measured bounds with a margin of 2.5
BOUNDS = dict({f: 1e-14 for f in R.WELL}, **{"narrow_1e-2": 1e-13, "narrow_1e-3": 1.5e-12, "narrow_1e-4": 2e-11})


def blocks_of(dc):
    return [(b.ilo, b.ihi, b.jlo, b.jhi) for b in dc.local_blocks(0)]


def oracle_domain(dc):
    blks = dc.local_blocks(0)
    return oracle.OracleDomain(dc.nx_block, dc.ny_block, len(blks), dc.nx_global, dc.ny_global, dc.ew, dc.ns,
                               [b.ilo for b in blks], [b.ihi for b in blks], [b.jlo for b in blks],
                               [b.jhi for b in blks], [b.gi0 for b in blks], [b.gj0 for b in blks])


def t_list(dc, tm):
    """dyn_prep2's T list: ilo..ihi+1 x jlo..jhi+1 where iceTmask."""
    on = np.zeros(tm.shape, dtype=bool)
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks_of(dc)):
        on[b, jlo - 1:jhi + 1, ilo - 1:ihi + 1] = tm[b, jlo - 1:jhi + 1, ilo - 1:ihi + 1] != 0
    return on


# ---- B grid ------------------------------------------------------------------------------------------------------------
def bgrid_case(grid, bs, ns="closed", seed=4, lkd_plant=None):
    """Synthetic B-grid model state, device preparation run; returns (core, dc, dom, t (as handed in), tm, um, scal)."""
    spec = synth.GRIDS[grid]
    nx, ny = spec["nx"], spec["ny"]
    g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns=ns))
    pr = synth.make_primary(g, "full", seed=seed)
    dc = decomp.Decomp(nx, ny, *(bs or (nx, ny)), "cyclic", ns, 1)
    sc = lambda a, fill=0.0: dc.scatter(np.ascontiguousarray(a), 0, fill=fill)
    geo = {k: sc(g[k], 1.0 if k != "uarear" else 0.0) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")}
    static = {k: sc(v, (1.0 if k in ("tarea", "uarea") else 0)) for k, v in pr["static"].items()}
    t = {k: sc(v) for k, v in pr["t"].items()}
    state = {k: sc(v) for k, v in pr["state"].items()}
    if lkd_plant is not None:                    # aice / vice of the LKD families on the ocean cells
        a, v, _, _ = lkd_plant
        ocean = static["tmask"] != 0
        t["aice"] = np.where(ocean, a, 0.0)
        t["vice"] = np.where(ocean, v, 0.0)
    scal = synth.evp_scalars(120)
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(scal, strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"],
                      geo["uarear"], geo["tarea"], keepalive=keep)
    core.set_prep_geometry(static["tmask"], static["umask"], static["hm"], static["tarea"], static["uarea"], static["fcor_blk"])
    tm, um, _ = core.prep(evp.PrepParams(**PPD, ssh_stress_coupled=0), t, state)
    return core, dc, oracle_domain(dc), t, tm, um, scal


def check_prob(dev, want, ext, fam_u, near_u, what):
    """The accuracy rule of the probabilistic factor: zero pattern bit-equal to the oracle's; per family, off the cells
    whose x_kmax lies within 4 ulp of a category centre, max|dev - ext|/|ext| <= 4 max|oracle - ext|/|ext| + 8u, and the
    documented bound against the oracle (BOUNDS).  Prints what it measured."""
    measured = {}
    keep = ~near_u
    assert bits_equal(dev[keep] == 0, want[keep] == 0), f"{what}: zero pattern differs from the oracle's"
    extf = ext.astype(np.float64)
    for f, name in enumerate(R.PROB_FAMILIES):
        m = keep & (fam_u == f) & (want != 0)
        if not m.any():
            continue
        e = np.abs(extf[m])
        d_dev = float((np.abs((dev[m] - ext[m]).astype(np.float64)) / e).max())
        d_or = float((np.abs((want[m] - ext[m]).astype(np.float64)) / e).max())
        assert d_dev <= 4.0 * d_or + 8.0 * U, f"{what} {name}: device {d_dev:.3e} vs oracle {d_or:.3e} from the extended value"
        rel = float((np.abs(dev[m] - want[m]) / np.abs(want[m])).max())
        measured[name] = f"{rel:.2e}"
        assert rel <= BOUNDS[name], f"{what} {name}: {rel:.3e} from the oracle, above the documented bound"
    print(f"\n{what}: device vs oracle, relative, per family: {measured}")


def planted_prob(dc, tm, ncat, seed, blocks=None):
    rng = np.random.default_rng(seed)
    where = t_list(dc, tm) if blocks is None else list_of(blocks, tm)
    per = min(PER_FAMILY, int(where.sum()) // len(R.PROB_FAMILIES))
    aicen, vicen, hwater, fam = R.plant_prob(rng, where, ncat, per)
    return aicen, vicen, hwater, fam


def list_of(blocks, tm):
    on = np.zeros(tm.shape, dtype=bool)
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        on[b, jlo - 1:jhi + 1, ilo - 1:ihi + 1] = tm[b, jlo - 1:jhi + 1, ilo - 1:ihi + 1] != 0
    return on


BCASES = [("gx3", None, 1), ("gx3", (25, 29), 5), ("gx3", (30, 40), 2)]       # one block; 4 x 4; 4 x 3 padded


@pytest.mark.parametrize("grid,bs,ncat", BCASES)
def test_bgrid_prob_edge_families(grid, bs, ncat):
    core, dc, dom, t, tm, um, scal = bgrid_case(grid, bs)
    try:
        aicen, vicen, hwater, fam = planted_prob(dc, tm, ncat, seed=11 + ncat)
        core.seabed_prob(hwater, aicen, vicen, ALPHAB, PPD["rhoi"], PPD["gravit"], PI, PUNY)
        dev = core.prep_fetch("TbU")
        blocks = blocks_of(dc)
        args = (ALPHAB, PPD["rhoi"], scal["rhow"], PPD["gravit"], PI, PUNY)
        _, info = R.prob_t(blocks, aicen, vicen, hwater, tm, *args)
        ext, _ = R.prob_t(blocks, aicen, vicen, hwater, tm, *args, ext=True)
        want = oracle.seabed_prob(dom, *args, aicen, vicen, hwater, tm, um)
        near_t = info["ulp_to_xk"] <= 4.0
        assert set(np.unique(fam[near_t])) <= {R.PROB_FAMILIES.index("xk_edge")}, "a cell near a category edge by chance"
        print(f"\n{grid} {bs} ncat {ncat}: {int(near_t.sum())} T cells within 4 ulp of a category centre (excluded)")
        near_u = spread(blocks, "U", near_t) & (um != 0)
        fam_u = family_of(blocks, "U", ext, um, fam)
        assert np.abs(want).max() > 0 and (want[um != 0] == 0).any()
        check_prob(dev, want, R.neighbor_max(blocks, "U", ext, um), fam_u, near_u, f"{grid} {bs} ncat {ncat} TbU")
    finally:
        core.finalize()


def spread(blocks, loc, near_t):
    out = np.zeros(near_t.shape, dtype=bool)
    for b, blk in enumerate(blocks):
        ilo, ihi, jlo, jhi = blk
        for di, dj in R.NEIGH[loc]:
            out[b, jlo - 1:jhi, ilo - 1:ihi] |= R._nb(near_t, b, blk, di, dj)
    return out


def family_of(blocks, loc, ext, mask, fam):
    am = R.argmax_t(blocks, loc, ext, mask)
    return np.where(am >= 0, fam.ravel()[np.maximum(am, 0)], -1)


def stale_ghosts(dc, a, rng):
    """a copy of `a` whose ghost cells hold values no exchange would put there."""
    out = a.copy()
    ghost = np.ones(a.shape, dtype=bool)
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks_of(dc)):
        ghost[b, jlo - 1:jhi, ilo - 1:ihi] = False
    out[ghost] = a[ghost] * (0.5 + rng.random(int(ghost.sum())))
    return out


@pytest.mark.parametrize("grid,bs", [(g, b) for g, b, _ in BCASES])
def test_bgrid_lkd_edge_families_and_ghost_refresh(grid, bs):
    """LKD at U points on the edge families: <= 2 ulp from the oracle, zero pattern bit-equal.  The entry refreshes the
    ghost cells of aice, vice and hwater itself: stale hwater ghost cells handed in give the oracle's result on the arrays
    after the centre / scalar exchange."""
    spec = synth.GRIDS[grid]
    rng = np.random.default_rng(3)
    plant = R.plant_lkd(rng, decomp.Decomp(spec["nx"], spec["ny"], *(bs or (spec["nx"], spec["ny"])), "cyclic", "closed", 1).shape(0))
    core, dc, dom, t, tm, um, scal = bgrid_case(grid, bs, lkd_plant=plant)
    try:
        h = stale_ghosts(dc, plant[2], rng)
        core.seabed_lkd(h, K1, K2, ALPHAB, THR)
        dev = core.prep_fetch("TbU")
        fresh = {k: oracle.halo_update(dom, np.array(v, dtype=np.float64, order="C", copy=True), "center", "scalar")
                 for k, v in (("aice", t["aice"]), ("vice", t["vice"]), ("hwater", h))}
        want = oracle.seabed_lkd(dom, K1, K2, ALPHAB, THR, fresh["aice"], fresh["vice"], fresh["hwater"], um)
        assert not bits_equal(fresh["hwater"], h)
        assert bits_equal(dev == 0, want == 0)
        nz = want != 0
        assert nz.sum() > 100 and (want[um != 0] == 0).sum() > 100
        ulp = np.abs(dev[nz] - want[nz]) / np.spacing(np.abs(want[nz]))
        print(f"\nLKD {grid} {bs}: max {ulp.max():.0f} ulp from the oracle on {int(nz.sum())} U cells")
        assert ulp.max() <= 2.0
        # a second call with hwater = NULL keeps the device copy (refreshed ghost cells included)
        core.seabed_lkd(None, K1, K2, ALPHAB, THR)
        assert bits_equal(core.prep_fetch("TbU"), dev)
    finally:
        core.finalize()


def test_bgrid_prob_ncat_changes_between_calls():
    """ncat 1 -> 5 -> 2 on one instance (the entry reallocates aicen / vicen) gives what fresh instances give; hwater = NULL
    keeps the device copy."""
    core, dc, dom, t, tm, um, scal = bgrid_case("gx3", (25, 29))
    try:
        res = {}
        for k, ncat in enumerate((1, 5, 2)):
            aicen, vicen, hwater, _ = planted_prob(dc, tm, ncat, seed=40 + ncat)
            if k == 0:
                hw_first = hwater
            core.seabed_prob(hwater if k == 0 else None, aicen, vicen, ALPHAB, PPD["rhoi"], PPD["gravit"], PI, PUNY)
            res[ncat] = (core.prep_fetch("TbU"), aicen, vicen)
    finally:
        core.finalize()
    for ncat, (got, aicen, vicen) in res.items():
        fresh, *_ = bgrid_case("gx3", (25, 29))
        try:
            fresh.seabed_prob(hw_first, aicen, vicen, ALPHAB, PPD["rhoi"], PPD["gravit"], PI, PUNY)
            assert bits_equal(got, fresh.prep_fetch("TbU")), f"ncat {ncat}"
            assert np.abs(got).max() > 0
        finally:
            fresh.finalize()


@pytest.mark.parametrize("method", ["lkd", "prob"])
def test_bgrid_tbu_zero_shortcut(method):
    """The TbU == 0 shortcut is derived from the device result.  Deep water everywhere: TbU is all zero and the loop gives,
    bit for bit, what a run whose TbU was set to zeros gives.  One shallow ice U cell: the shortcut is off -- the loop
    equals a run fed the oracle's TbU (cice_evp_hip_set_tbu), bit for bit where the two TbU agree bit for bit, within 1e-9
    otherwise."""
    c = GoldenCase("pop_cyc_2x2_seabed" if method == "lkd" else "pop_cyc_2x2_seabedprob")
    s = c.scal
    dom = c.oracle_domain()
    t, state = c.prep_inputs(1)
    dyn, _, _ = c.inputs(1)
    deep = np.full(c.d["hwater"].shape, 80.0)
    shallow = deep.copy()
    um = c.inputs(1)[2]
    b, j, i = [int(x[len(x) // 2]) for x in np.nonzero(um)]
    shallow[b, j:j + 2, i:i + 2] = 3.0
    runs = {}
    for name, hw in (("deep", deep), ("shallow", shallow), ("zeros", None), ("set", shallow)):
        core = hip_from_case(c, strict=True)
        try:
            st = c.prep_static()
            core.set_prep_geometry(st["tmask"], st["umask"], st["hm"], st["tarea"], st["uarea"], st["fcor_blk"])
            d = c.prep_scal_dict()
            pp = evp.PrepParams(dt=d["dt"], rhoi=d["rhoi"], rhos=d["rhos"], gravit=d["gravit"], dyn_area_min=d["dyn_area_min"],
                                dyn_mass_min=d["dyn_mass_min"], ssh_stress_coupled=d["ssh_coupled"])
            tm, um, _ = core.prep(pp, t, state)
            if name == "zeros":
                core.set_tbu(np.zeros(c.d["hwater"].shape))
                tb = None
            elif name == "set":
                if method == "lkd":
                    a = oracle.halo_update(dom, np.array(t["aice"], copy=True), "center", "scalar")
                    v = oracle.halo_update(dom, np.array(t["vice"], copy=True), "center", "scalar")
                    tb = oracle.seabed_lkd(dom, s[24], s[25], s[26], s[27], a, v, hw, um)
                else:
                    tb = oracle.seabed_prob(dom, s[26], s[17], s[12], s[19], s[30], s[31], t["aice"][:, None], t["vice"][:, None],
                                            hw, tm, um)
                core.set_tbu(tb)
            elif method == "lkd":
                core.seabed_lkd(hw, s[24], s[25], s[26], s[27])
                tb = core.prep_fetch("TbU")
            else:
                core.seabed_prob(hw, t["aice"][:, None], t["vice"][:, None], s[26], s[17], s[19], s[30], s[31])
                tb = core.prep_fetch("TbU")
            core.set_strength(dyn["strength"])
            core.subcycle(c.ndte)
            runs[name] = (tb, core.download())
        finally:
            core.finalize()
    assert (runs["deep"][0] == 0).all()
    assert_bitwise(runs["deep"][1], runs["zeros"][1], f"{method}: deep water vs TbU set to zeros")
    tb_dev, tb_or = runs["shallow"][0], runs["set"][0]
    assert (tb_dev != 0).sum() >= 1 and bits_equal(tb_dev == 0, tb_or == 0)
    assert not bits_equal(runs["shallow"][1]["uvel"], runs["zeros"][1]["uvel"]), "the seabed stress changed nothing"
    if bits_equal(tb_dev, tb_or):
        assert_bitwise(runs["shallow"][1], runs["set"][1], f"{method}: one shallow U cell")
    assert max_rel_err(runs["shallow"][1], runs["set"][1], VEL + SIG + ["taubxU", "taubyU"]) < 1e-9


# ---- C grid ------------------------------------------------------------------------------------------------------------
def cgrid_case(grid, bs, seed=9):
    spec = synth.GRIDS[grid]
    nx, ny = spec["nx"], spec["ny"]
    ns = spec.get("ns", "closed")
    g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns=ns))
    cg = synth.cgrid_geometry(g)
    state, inputs, masks = synth.cgrid_state(g, cg, case="full", seed=seed, warm=True)
    t, st7, prev = synth.cgrid_prep_inputs(g, cg, case="full", seed=17, coupled=False)
    bsx, bsy = bs if bs else (nx, ny)
    dc = decomp.Decomp(nx, ny, bsx, bsy, "cyclic", ns, 1)
    static, state, inputs, masks = synth.cgrid_scatter(dc, 0, cg, state, inputs, masks)
    tb = {k: dc.scatter(v, 0, fold=("center", -1.0 if k in ("uocn", "vocn", "ss_tltx", "ss_tlty", "strairxT", "strairyT") else 1.0))
          for k, v in t.items()}
    loc = {"umaskCD": "NEcorner", "emask": "Eface", "nmask": "Nface", "fcor_blk": "NEcorner", "fcorE_blk": "Eface", "fcorN_blk": "Nface"}
    static.update({k: dc.scatter(v, 0, fill=0, fold=(loc.get(k, "center"), 1.0)) for k, v in st7.items()})
    prevb = {k: dc.scatter(v, 0, fill=0) for k, v in prev.items()}
    scal = synth.evp_scalars(120)
    dom = oracle_domain(dc)
    want = oracle.cgrid_prep(dom, oracle.PrepParams(**PPD, cosw=scal["cosw"], sinw=scal["sinw"], ssh_coupled=0), static,
                             {k: v.copy() for k, v in tb.items()}, dict(state, **prevb))
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(scal, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"],
                      1.0 / static["uarea"], static["tarea"], keepalive=keep)
    core.cgrid_set_geometry(static)
    core.cgrid_set_prep_geometry(static)
    return core, dc, dom, scal, static, state, prevb, tb, want, inputs


CCASES = [("gx3", None), ("gx3", (30, 40)), ("tx1", (90, 60))]


@pytest.mark.parametrize("grid,bs", CCASES)
@pytest.mark.parametrize("ncat", [1, 5])
def test_cgrid_prob_edge_families(grid, bs, ncat):
    """TbE / TbN by the probabilistic method on the edge families; aicen / vicen / hwater are read as handed in, ghost cells
    included (no exchange): the oracle runs on exactly those arrays."""
    core, dc, dom, scal, static, state, prevb, tb, want, inputs = cgrid_case(grid, bs)
    try:
        got = core.cgrid_prep(evp.PrepParams(**PPD, ssh_stress_coupled=0), tb, state, prevb)
        for k in oracle.C_MASKS:
            assert bits_equal(got[k] != 0, want[k] != 0), k
        tm = want["iceTmask"]
        aicen, vicen, hwater, fam = planted_prob(dc, tm, ncat, seed=70 + ncat)
        core.cgrid_seabed_prob(hwater, aicen, vicen, ALPHAB, PPD["rhoi"], PPD["gravit"], PI, PUNY)
        core.cgrid_prep_finish(inputs["strength"])
        blocks = blocks_of(dc)
        args = (ALPHAB, PPD["rhoi"], scal["rhow"], PPD["gravit"], PI, PUNY)
        _, info = R.prob_t(blocks, aicen, vicen, hwater, tm, *args)
        ext, _ = R.prob_t(blocks, aicen, vicen, hwater, tm, *args, ext=True)
        near_t = info["ulp_to_xk"] <= 4.0
        assert set(np.unique(fam[near_t])) <= {R.PROB_FAMILIES.index("xk_edge")}
        we, wn = oracle.seabed_prob_c(dom, *args, aicen, vicen, hwater, tm, want["iceEmask"], want["iceNmask"])
        for loc, w in (("E", we), ("N", wn)):
            mask = want[f"ice{loc}mask"]
            assert np.abs(w).max() > 0
            check_prob(core.cgrid_fetch("Tb" + loc), w, R.neighbor_max(blocks, loc, ext, mask),
                       family_of(blocks, loc, ext, mask, fam), spread(blocks, loc, near_t) & (mask != 0),
                       f"{grid} {bs} ncat {ncat} Tb{loc}")
    finally:
        core.finalize()


@pytest.mark.parametrize("grid,bs", CCASES)
def test_cgrid_lkd_edge_families_ghosts_as_given(grid, bs):
    """TbE / TbN by LKD on the edge families, with stale ghost cells in aice, vice and hwater: the entry reads them as
    handed in, so the oracle on exactly those arrays is matched -- <= 2 ulp, zero pattern bit-equal."""
    core, dc, dom, scal, static, state, prevb, tb, want, inputs = cgrid_case(grid, bs)
    try:
        rng = np.random.default_rng(5)
        a, v, h, _ = R.plant_lkd(rng, tb["aice"].shape)
        ocean = static["tmask"] != 0
        tb["aice"] = stale_ghosts(dc, np.where(ocean, a, 0.0), rng)
        tb["vice"] = stale_ghosts(dc, np.where(ocean, v, 0.0), rng)
        h = stale_ghosts(dc, h, rng)
        want = oracle.cgrid_prep(dom, oracle.PrepParams(**PPD, cosw=scal["cosw"], sinw=scal["sinw"], ssh_coupled=0), static,
                                 {k: x.copy() for k, x in tb.items()}, dict(state, **prevb))
        got = core.cgrid_prep(evp.PrepParams(**PPD, ssh_stress_coupled=0), tb, state, prevb)
        for k in oracle.C_MASKS:
            assert bits_equal(got[k] != 0, want[k] != 0), k
        core.cgrid_seabed_lkd(h, K1, K2, ALPHAB, THR)
        core.cgrid_prep_finish(inputs["strength"])
        for loc in "EN":
            w = oracle.seabed_lkd_c(dom, loc, K1, K2, ALPHAB, THR, tb["aice"], tb["vice"], h, want[f"ice{loc}mask"])
            dev = core.cgrid_fetch("Tb" + loc)
            assert bits_equal(dev == 0, w == 0), loc
            nz = w != 0
            assert nz.sum() > 100
            ulp = np.abs(dev[nz] - w[nz]) / np.spacing(np.abs(w[nz]))
            print(f"\nLKD {grid} {bs} Tb{loc}: max {ulp.max():.0f} ulp from the oracle on {int(nz.sum())} faces")
            assert ulp.max() <= 2.0
    finally:
        core.finalize()


def test_cgrid_prob_ncat_changes_between_calls():
    """C grid: ncat 1 -> 5 -> 2 between calls (reallocation) gives what fresh instances give; hwater = NULL keeps the copy."""
    res = []
    core, dc, dom, scal, static, state, prevb, tb, want, inputs = cgrid_case("gx3", (30, 40))
    try:
        for k, ncat in enumerate((1, 5, 2)):
            core.cgrid_prep(evp.PrepParams(**PPD, ssh_stress_coupled=0), tb, state if k == 0 else None, prevb)
            aicen, vicen, hwater, _ = planted_prob(dc, want["iceTmask"], ncat, seed=90 + ncat)
            if k == 0:
                hw_first = hwater
            core.cgrid_seabed_prob(hwater if k == 0 else None, aicen, vicen, ALPHAB, PPD["rhoi"], PPD["gravit"], PI, PUNY)
            core.cgrid_prep_finish(inputs["strength"])
            res.append((ncat, core.cgrid_fetch("TbE"), core.cgrid_fetch("TbN"), aicen, vicen))
    finally:
        core.finalize()
    for ncat, e, n, aicen, vicen in res:
        fresh, dc, dom, scal, static, state, prevb, tb, want, inputs = cgrid_case("gx3", (30, 40))
        try:
            fresh.cgrid_prep(evp.PrepParams(**PPD, ssh_stress_coupled=0), tb, state, prevb)
            fresh.cgrid_seabed_prob(hw_first, aicen, vicen, ALPHAB, PPD["rhoi"], PPD["gravit"], PI, PUNY)
            fresh.cgrid_prep_finish(inputs["strength"])
            assert bits_equal(e, fresh.cgrid_fetch("TbE")) and bits_equal(n, fresh.cgrid_fetch("TbN")), f"ncat {ncat}"
            assert np.abs(e).max() > 0
        finally:
            fresh.finalize()


def test_cgrid_seabed_shortcut_and_loop():
    """C grid, through cg_call_setup's per-call flags: deep water everywhere gives TbE = TbN = 0 and the loop of a run whose
    factors were set to zeros, bit for bit; one shallow face switches the general momentum step on -- the loop equals a run
    fed the oracle's TbE / TbN (cice_evp_hip_cgrid_set_tb), bit for bit where the factors agree bit for bit, within 1e-9."""
    c = GoldenCase("cgrid_cyc_1blk_seabed")
    s = c.scal
    dom = c.oracle_domain()
    t, st, _ = c.cgrid_prep_inputs(1)
    deep = np.full(c.d["hwater"].shape, 80.0)
    em = c.cgrid_inputs(1)[2]["iceEmask"]
    b, j, i = [int(x[len(x) // 2]) for x in np.nonzero(em)]
    shallow = deep.copy()
    shallow[b, j, i:i + 2] = 3.0
    runs = {}
    nsub = c.nsub_list[-1]
    for name, hw in (("deep", deep), ("shallow", shallow), ("zeros", None), ("set", shallow)):
        core = cgrid_core(c)
        try:
            core.cgrid_set_prep_geometry(c.cgrid_prep_static())
            masks = core.cgrid_prep(hip_prep_params(c), t, {k: st[k] for k in oracle.C_FIELDS[:12]},
                                    {k: st[k] for k in ("iceUmask", "iceEmask", "iceNmask")})
            if name == "zeros":
                z = np.zeros(deep.shape)
                core.cgrid_set_tb(z, z)
                tbs = None
            elif name == "set":
                tbs = [oracle.seabed_lkd_c(dom, loc, s[24], s[25], s[26], s[27], t["aice"], t["vice"], hw, masks[f"ice{loc}mask"])
                       for loc in "EN"]
                core.cgrid_set_tb(*tbs)
            else:
                core.cgrid_seabed_lkd(hw, s[24], s[25], s[26], s[27])
                tbs = None
            core.cgrid_prep_finish(c.d["in01_strength"], str(c.d["visc_method"]))
            if tbs is None:
                tbs = [core.cgrid_fetch("TbE"), core.cgrid_fetch("TbN")]
            core.cgrid_subcycle(nsub)
            runs[name] = (tbs, core.cgrid_download())
        finally:
            core.finalize()
    assert all((x == 0).all() for x in runs["deep"][0])
    assert_bitwise(runs["deep"][1], runs["zeros"][1], "deep water vs TbE = TbN = 0")
    (de, dn), (oe, on) = runs["shallow"][0], runs["set"][0]
    assert (de != 0).sum() >= 1 and bits_equal(de == 0, oe == 0) and bits_equal(dn == 0, on == 0)
    assert not bits_equal(runs["shallow"][1]["uvelE"], runs["zeros"][1]["uvelE"]), "the seabed stress changed nothing"
    if bits_equal(de, oe) and bits_equal(dn, on):
        assert_bitwise(runs["shallow"][1], runs["set"][1], "one shallow face")
    assert max_rel_err(runs["shallow"][1], runs["set"][1], ["uvelE", "vvelN", "stresspT", "stressmT", "stress12U"]) < 1e-9


# ---- tripole u-fold and tripoleT, both grids ---------------------------------------------------------------------------
def fold_case(case, bs):
    """A tripole case for both grids: the synthetic tx3 (u-fold) or a tripoleT fixture's grid and state.  Returns a dict with
    a core factory and what the oracle needs (C-grid static arrays; the B-grid preparation takes tmask / umaskCD)."""
    if case.startswith("cgtript_"):
        c = GoldenCase(case)
        t, st, _ = c.cgrid_prep_inputs(1)
        ua = c.d["uarea"]
        uarear = np.where(ua > 0, 1.0 / np.where(ua > 0, ua, 1.0), 0.0)
        d, keep = c.hip_dims()
        mk = lambda: evp.EvpHip(d, evp.make_params(c.scal_dict(), strict=True), c.d["dyE"], c.d["dxN"], c.d["dxT"], c.d["dyT"],
                                uarear, c.d["tarea"], keepalive=keep)
        return dict(mk=mk, dom=c.oracle_domain(), blocks=[tuple(int(v) for v in c.blk[b, :4]) for b in range(c.nblocks)],
                    static=c.cgrid_prep_static(), t=t, state={k: st[k] for k in oracle.C_FIELDS[:12]},
                    prev={k: st[k] for k in ("iceUmask", "iceEmask", "iceNmask")}, pp=hip_prep_params(c),
                    opp=oracle.PrepParams(**c.prep_scal_dict()), strength=c.d["in01_strength"], rhow=c.scal[12])
    spec = synth.GRIDS[case]
    nx, ny, ns = spec["nx"], spec["ny"], spec.get("ns", "closed")
    g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns=ns))
    cg = synth.cgrid_geometry(g)
    state, inputs, masks = synth.cgrid_state(g, cg, case="full", seed=9, warm=True)
    t, st7, prev = synth.cgrid_prep_inputs(g, cg, case="full", seed=17, coupled=False)
    dc = decomp.Decomp(nx, ny, *(bs or (nx, ny)), "cyclic", ns, 1)
    static, state, inputs, masks = synth.cgrid_scatter(dc, 0, cg, state, inputs, masks)
    vec = ("uocn", "vocn", "ss_tltx", "ss_tlty", "strairxT", "strairyT")
    tb = {k: dc.scatter(v, 0, fold=("center", -1.0 if k in vec else 1.0)) for k, v in t.items()}
    loc = {"umaskCD": "NEcorner", "emask": "Eface", "nmask": "Nface", "fcor_blk": "NEcorner", "fcorE_blk": "Eface", "fcorN_blk": "Nface"}
    static.update({k: dc.scatter(v, 0, fill=0, fold=(loc.get(k, "center"), 1.0)) for k, v in st7.items()})
    prevb = {k: dc.scatter(v, 0, fill=0) for k, v in prev.items()}
    scal = synth.evp_scalars(120)
    d, keep = evp.make_dims(dc, 0)
    mk = lambda: evp.EvpHip(d, evp.make_params(scal, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"],
                            1.0 / static["uarea"], static["tarea"], keepalive=keep)
    return dict(mk=mk, dom=oracle_domain(dc), blocks=blocks_of(dc), static=static, t=tb,
                state={k: state[k] for k in oracle.C_FIELDS[:12]}, prev=prevb, pp=evp.PrepParams(**PPD, ssh_stress_coupled=0),
                opp=oracle.PrepParams(**PPD, cosw=scal["cosw"], sinw=scal["sinw"], ssh_coupled=0), strength=inputs["strength"],
                rhow=scal["rhow"])


def ghosts_replaced(blocks, a, rng):
    out = a.copy()
    ghost = np.ones(a.shape, dtype=bool)
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        ghost[b, jlo - 1:jhi, ilo - 1:ihi] = False
    out[ghost] = a[ghost] * (0.5 + rng.random(int(ghost.sum())))
    return out


def bgrid_fold_prep(S, t):
    core = S["mk"]()
    st = S["static"]
    core.set_prep_geometry(st["tmask"], st["umaskCD"], st["hm"], st["tarea"], st["uarea"], st["fcor_blk"])
    z = np.zeros(st["tarea"].shape)
    tm, um, _ = core.prep(S["pp"], t, dict({k: z for k in SIG}, uvel=z, vvel=z, iceUmask=S["prev"]["iceUmask"]))
    return core, tm, um


FOLD_CASES = [("tx3", (25, 29)), ("tx3", None), ("cgtript_cyc_2x2_patchy", None)]


@pytest.mark.parametrize("case,bs", FOLD_CASES)
def test_bgrid_fold_lkd_refreshes_ghosts_and_prob(case, bs):
    """B grid on a tripole u-fold (tx3) and a tripoleT grid.  LKD with stale ghost cells in aice, vice and hwater: the entry
    refreshes them (centre / scalar exchange, fold included), so the oracle on the arrays after oracle.halo_update(...,
    'center', 'scalar') is matched within 2 ulp, zero pattern bit-equal.  Then the probabilistic method on the edge
    families, ncat 5, by the accuracy rule."""
    S = fold_case(case, bs)
    rng = np.random.default_rng(23)
    a, v, h, _ = R.plant_lkd(rng, S["t"]["aice"].shape)
    ocean = S["static"]["tmask"] != 0
    t = dict(S["t"], aice=ghosts_replaced(S["blocks"], np.where(ocean, a, 0.0), rng),
             vice=ghosts_replaced(S["blocks"], np.where(ocean, v, 0.0), rng))
    h = ghosts_replaced(S["blocks"], h, rng)
    core, tm, um = bgrid_fold_prep(S, t)
    try:
        core.seabed_lkd(h, K1, K2, ALPHAB, THR)
        dev = core.prep_fetch("TbU")
        fresh = {k: oracle.halo_update(S["dom"], np.array(x, dtype=np.float64, order="C", copy=True), "center", "scalar")
                 for k, x in (("aice", t["aice"]), ("vice", t["vice"]), ("hwater", h))}
        assert not bits_equal(fresh["hwater"], h) and not bits_equal(fresh["aice"], t["aice"])
        want = oracle.seabed_lkd(S["dom"], K1, K2, ALPHAB, THR, fresh["aice"], fresh["vice"], fresh["hwater"], um)
        stale = oracle.seabed_lkd(S["dom"], K1, K2, ALPHAB, THR, t["aice"], t["vice"], h, um)
        assert not bits_equal(stale, want)                  # the ghost cells matter to the result
        assert bits_equal(dev == 0, want == 0)
        nz = want != 0
        assert nz.sum() > 20
        ulp = np.abs(dev[nz] - want[nz]) / np.spacing(np.abs(want[nz]))
        print(f"\nLKD B grid {case} {bs}: max {ulp.max():.0f} ulp from the oracle on {int(nz.sum())} U cells")
        assert ulp.max() <= 2.0
        aicen, vicen, hwater, fam = planted_prob(None, tm, 5, seed=29, blocks=S["blocks"])
        core.seabed_prob(hwater, aicen, vicen, ALPHAB, PPD["rhoi"], PPD["gravit"], PI, PUNY)
        dev = core.prep_fetch("TbU")
        args = (ALPHAB, PPD["rhoi"], S["rhow"], PPD["gravit"], PI, PUNY)
        _, info = R.prob_t(S["blocks"], aicen, vicen, hwater, tm, *args)
        ext, _ = R.prob_t(S["blocks"], aicen, vicen, hwater, tm, *args, ext=True)
        want = oracle.seabed_prob(S["dom"], *args, aicen, vicen, hwater, tm, um)
        near_t = info["ulp_to_xk"] <= 4.0
        assert set(np.unique(fam[near_t])) <= {R.PROB_FAMILIES.index("xk_edge")}
        assert np.abs(want).max() > 0
        check_prob(dev, want, R.neighbor_max(S["blocks"], "U", ext, um), family_of(S["blocks"], "U", ext, um, fam),
                   spread(S["blocks"], "U", near_t) & (um != 0), f"B grid {case} {bs} ncat 5 TbU")
    finally:
        core.finalize()


@pytest.mark.parametrize("case", ["cgtript_cyc_2x2_patchy", "cgtript_cyc_1blk_full_avgstrength"])
def test_cgrid_tripoleT_lkd_and_prob(case):
    """C grid on tripoleT: LKD with stale ghost cells read as given (oracle on exactly those arrays, <= 2 ulp), then the
    probabilistic method on the edge families, ncat 2, by the accuracy rule."""
    S = fold_case(case, None)
    rng = np.random.default_rng(31)
    a, v, h, _ = R.plant_lkd(rng, S["t"]["aice"].shape)
    ocean = S["static"]["tmask"] != 0
    t = dict(S["t"], aice=ghosts_replaced(S["blocks"], np.where(ocean, a, 0.0), rng),
             vice=ghosts_replaced(S["blocks"], np.where(ocean, v, 0.0), rng))
    h = ghosts_replaced(S["blocks"], h, rng)
    want = oracle.cgrid_prep(S["dom"], S["opp"], S["static"], {k: x.copy() for k, x in t.items()}, dict(S["state"], **S["prev"]))
    core = S["mk"]()
    try:
        core.cgrid_set_geometry(S["static"])
        core.cgrid_set_prep_geometry(S["static"])
        got = core.cgrid_prep(S["pp"], t, S["state"], S["prev"])
        for k in oracle.C_MASKS:
            assert bits_equal(got[k] != 0, want[k] != 0), k
        core.cgrid_seabed_lkd(h, K1, K2, ALPHAB, THR)
        core.cgrid_prep_finish(S["strength"])
        for loc in "EN":
            w = oracle.seabed_lkd_c(S["dom"], loc, K1, K2, ALPHAB, THR, t["aice"], t["vice"], h, want[f"ice{loc}mask"])
            dev = core.cgrid_fetch("Tb" + loc)
            assert bits_equal(dev == 0, w == 0), loc
            nz = w != 0
            assert nz.sum() > 20
            ulp = np.abs(dev[nz] - w[nz]) / np.spacing(np.abs(w[nz]))
            print(f"\nLKD C grid {case} Tb{loc}: max {ulp.max():.0f} ulp from the oracle on {int(nz.sum())} faces")
            assert ulp.max() <= 2.0
        tm = want["iceTmask"]
        core.cgrid_prep(S["pp"], t, None, S["prev"])
        aicen, vicen, hwater, fam = planted_prob(None, tm, 2, seed=37, blocks=S["blocks"])
        core.cgrid_seabed_prob(hwater, aicen, vicen, ALPHAB, PPD["rhoi"], PPD["gravit"], PI, PUNY)
        core.cgrid_prep_finish(S["strength"])
        args = (ALPHAB, PPD["rhoi"], S["rhow"], PPD["gravit"], PI, PUNY)
        _, info = R.prob_t(S["blocks"], aicen, vicen, hwater, tm, *args)
        ext, _ = R.prob_t(S["blocks"], aicen, vicen, hwater, tm, *args, ext=True)
        near_t = info["ulp_to_xk"] <= 4.0
        assert set(np.unique(fam[near_t])) <= {R.PROB_FAMILIES.index("xk_edge")}
        we, wn = oracle.seabed_prob_c(S["dom"], *args, aicen, vicen, hwater, tm, want["iceEmask"], want["iceNmask"])
        for loc, w in (("E", we), ("N", wn)):
            mask = want[f"ice{loc}mask"]
            assert np.abs(w).max() > 0
            check_prob(core.cgrid_fetch("Tb" + loc), w, R.neighbor_max(S["blocks"], loc, ext, mask),
                       family_of(S["blocks"], loc, ext, mask, fam), spread(S["blocks"], loc, near_t) & (mask != 0),
                       f"C grid {case} ncat 2 Tb{loc}")
    finally:
        core.finalize()


# ---- the reference's own factors at ncat = 5 ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pop_cyc_2x2_seabedprob_ncat5", "cgrid_cyc_2x2_seabedprob_ncat5"])
def test_device_prob_against_the_reference_at_ncat5(name):
    """The fixtures made by the reference with five thickness categories: the device factors from the fixture's aicen /
    vicen have the reference's zero pattern bit for bit and lie within 1e-14 of its TbU / TbE / TbN (well-conditioned cells)."""
    c = GoldenCase(name)
    s = c.scal
    if name.startswith("cgrid_"):
        core = cgrid_core(c)
        try:
            core.cgrid_set_prep_geometry(c.cgrid_prep_static())
            t, st, _ = c.cgrid_prep_inputs(1)
            core.cgrid_prep(hip_prep_params(c), t, {k: st[k] for k in oracle.C_FIELDS[:12]},
                            {k: st[k] for k in ("iceUmask", "iceEmask", "iceNmask")})
            core.cgrid_seabed_prob(c.d["hwater"], c.aicen(1), c.vicen(1), s[26], s[17], s[19], s[30], s[31])
            core.cgrid_prep_finish(c.d["in01_strength"], str(c.d["visc_method"]))
            _, want, _ = c.cgrid_inputs(1)
            pairs = [(core.cgrid_fetch("TbE"), want["TbE"]), (core.cgrid_fetch("TbN"), want["TbN"])]
        finally:
            core.finalize()
    else:
        core = hip_from_case(c, strict=True)
        try:
            st = c.prep_static()
            core.set_prep_geometry(st["tmask"], st["umask"], st["hm"], st["tarea"], st["uarea"], st["fcor_blk"])
            t, state = c.prep_inputs(1)
            core.prep(hip_prep_params(c), t, state)
            core.seabed_prob(c.d["hwater"], c.aicen(1), c.vicen(1), s[26], s[17], s[19], s[30], s[31])
            pairs = [(core.prep_fetch("TbU"), c.inputs(1)[0]["TbU"])]
        finally:
            core.finalize()
    for got, w in pairs:
        assert np.abs(w).max() > 0 and bits_equal(got == 0, w == 0)
        nz = w != 0
        rel = np.abs(got[nz] - w[nz]) / np.abs(w[nz])
        print(f"\n{name}: max {rel.max():.2e} relative from the reference")
        assert rel.max() <= BOUNDS["generic"]
