"""What evp() does around the B grid's subcycle loop, as ONE chain that names its stages (test infrastructure, no GPU needed to
import): cice_evp_hip_prep -> set_strength / set_tbu -> the loop -> stress_halo on a fold -> download -> deformations ->
dyn_finish.  The loop has four hosts (streaming kernel, on-chip resident kernel, marching kernel, marched zone + fold band); each
leaves the block-layout state -- S.cur, the ghost cells of the final velocities, the diagnostics -- for the calls after it in its
own way.  run_chain / run_synth_chain run the chain on a core whose path the caller forced (PATHS) and compare every stage with the
reference's fixture or with the oracle's chain (oracle_fixture_chain / SynthChain.oracle), bit for bit, every message starting
with the stage; assert_path_ran is the evidence that the named path did the work."""
from __future__ import annotations

import functools

import numpy as np

import oracle
from cice_amd import decomp, evp, synth
from common import GoldenCase, assert_bitwise, bits_equal, tfold_untouched

SIG = evp.FIELDS[:12]
POST = ("divu", "shear", "vort", "rdg_conv", "rdg_shear")
# The one table of path switches (tests/test_gpu_call_flags.py takes its rows and PATH_ENV from here).  PATH_ENV: every switch a row
# of a path table sets, cleared before a row's own are set.
PATH_ENV = ("CICE_EVP_HIP_RESIDENT", "CICE_EVP_HIP_MARCH", "CICE_EVP_HIP_RES_LEAN", "CICE_EVP_HIP_RES_LOGW", "CICE_EVP_HIP_MARCH_K",
            "CICE_EVP_HIP_MARCH_SEG", "CICE_EVP_HIP_MARCH_EXT", "CICE_EVP_HIP_FLAGS")
_MARCH = {"CICE_EVP_HIP_MARCH": "1", "CICE_EVP_HIP_RESIDENT": "0"}
_K4, _K3 = dict(_MARCH, CICE_EVP_HIP_MARCH_K="4"), dict(_MARCH, CICE_EVP_HIP_MARCH_K="3", CICE_EVP_HIP_MARCH_SEG="5")
PATHS = {
    "default": {},                                  # what the library picks by itself (no evidence asked for)
    "streaming": {"CICE_EVP_HIP_RESIDENT": "0", "CICE_EVP_HIP_MARCH": "0"},
    "resident general": {"CICE_EVP_HIP_RESIDENT": "1", "CICE_EVP_HIP_RES_LEAN": "0"},
    "resident lean-eligible": {"CICE_EVP_HIP_RESIDENT": "1", "CICE_EVP_HIP_RES_LOGW": "4"},
    "marching k=4": _K4,
    "marching k=3": _K3,
    # fold grids: no redundant rim, so that an 18-row grid has a zone under its band; and a rim of four
    "marching k=4 ext=0": dict(_K4, CICE_EVP_HIP_MARCH_EXT="0"),
    "marching k=3 ext=0": dict(_K3, CICE_EVP_HIP_MARCH_EXT="0"),
    "marching k=4 ext=4": dict(_K4, CICE_EVP_HIP_MARCH_EXT="4"),
    "marching k=3 ext=4": dict(_K3, CICE_EVP_HIP_MARCH_EXT="4"),
}
LOOP_PATHS = ["streaming", "resident general", "resident lean-eligible", "marching k=4", "marching k=3"]
FOLD_PATHS = ["marching k=4 ext=0", "marching k=3 ext=0"]
SENTINEL = (7.0, -3.0)          # what dyn_finish is handed off the fixtures: the cells it does not own keep it


def set_path(monkeypatch, path):
    for k in PATH_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def is_fold(ns):
    return ns in ("tripole", "tripoleT")


def assert_path_ran(core, path, nsub, fold, lean=None, what="", fallbacks=0):
    """The loop of the call just made ran on the path `path` names.  lean: whether the lean resident variant must have run (None:
    not asked).  A single subcycle of a marching path goes through the one-subcycle kernel by design (march_schedule).
    fallbacks: calls of the resident kernel the test made fail on purpose so far (CICE_EVP_HIP_FAULT_REPLAY)."""
    if path == "default":
        return
    t, m = core.timings(), core.march_info()
    fl = core.call_flags() if path.startswith("resident") else None       # (the test build's read-out; those rows set its switches)
    assert t["resident_fallbacks"] == fallbacks, (what, t)
    if path == "streaming":
        assert t["tile_variant"] < 1000 and not m["last_call"] and m["mode"] != 1, (what, t, m)
    elif path == "resident general":
        assert t["tile_variant"] >= 2000 and not fl["resident_lean"], (what, t, fl)
    elif path == "resident lean-eligible":
        assert t["tile_variant"] == 2004, (what, t)
        if lean is not None:
            assert fl["resident_lean"] == lean, (what, fl)
    else:
        assert m["mode"] == 1 and m["declined"] == 0 and m["last_call"] and m["kpass"] == int(path.split("k=")[1][0]), (what, m, core.describe_path())
        assert (m["band_rows"] > 0) == fold, (what, m)
        if nsub >= 2:
            assert m["passes"] > 0, (what, m)
            if fold:
                assert m["band_subcycles"] == nsub - (nsub % m["kpass"] == 1), (what, m)
                assert "fold band" in core.describe_path(), core.describe_path()


# ---- the reference's fixtures ------------------------------------------------------------------------------------------------
def chain_fixtures():
    """B-grid fixtures that carry pr<call>_* inputs (all of them do today; a fixture without them cannot run the chain)."""
    from common import GOLDEN_CASES, TFOLD_CASES
    return [n for n in GOLDEN_CASES + TFOLD_CASES if "pr01_aice" in GoldenCase(n).d]


def post_counts(c: GoldenCase):
    """Subcycle counts of the fixture that have post-loop outputs."""
    return [n for n in c.nsub_list if f"o01n{n:04d}_divu" in c.d]


def open_core(c: GoldenCase, strict=True):
    """A core on the fixture's grid in the test build (call_flags() is its read-out), with the geometry of every stage."""
    d, keep = c.hip_dims()
    core = evp.EvpHip(d, evp.make_params(c.scal_dict(), strict=strict), c.d["HTE"], c.d["HTN"], c.d["dxT"], c.d["dyT"], c.d["uarear"],
                      c.d["tarea"], keepalive=keep, testing=True)
    if is_fold(c.ns):
        core.set_metrics(dxhy=c.d["dxhy"], dyhx=c.d["dyhx"])        # CICE's own (mirrored ghost row), as the Fortran shim hands them
    st = c.prep_static()
    core.set_prep_geometry(st["tmask"], st["umask"], st["hm"], st["tarea"], st["uarea"], st["fcor_blk"])
    core.set_post_geometry(c.d["dxU"], c.d["dyU"], c.d["tarear"])
    return core


def prep_params(c: GoldenCase):
    d = c.prep_scal_dict()
    return evp.PrepParams(**{k: v for k, v in d.items() if k not in ("cosw", "sinw", "ssh_coupled")}, ssh_stress_coupled=d["ssh_coupled"])


def fixture_lean(c: GoldenCase, icall):
    """Whether the lean resident variant covers this call of the fixture (cice_amd/csrc/res2_variant.cpp)."""
    s, dyn = c.scal, c.inputs(icall)[0]
    um = c.inputs(icall)[2] != 0
    simple = s[6] == 1.0 and s[3] == 0.0 and s[7] == 0.0 and s[10] == 1.0 and s[11] == 0.0
    return bool(simple and c.nblocks == 1 and not is_fold(c.ns) and not dyn["TbU"].any() and
                bits_equal(dyn["waterxU"][um], dyn["uocnU"][um]) and bits_equal(dyn["wateryU"][um], dyn["vocnU"][um]))


def assert_stage(got, want, what, keep=None):
    """assert_bitwise; keep: the cells the stresses are compared on (tripoleT against a loop-only reference)."""
    if keep is None:
        return assert_bitwise(got, want, what)
    for k, w in want.items():
        sel = keep if k in SIG else slice(None)
        assert bits_equal(got[k][sel], w[sel]), f"{what}: {k} not bit-identical"


def oracle_fixture_chain(c: GoldenCase, icall, nsub):
    """The oracle's chain on the fixture's model state, every stage fed by the one before: prep -> loop (strength and TbU are
    Icepack's / the host's: the fixture's) -> the u-fold's stress symmetrisation -> deformations -> dyn_finish (zeros handed in).
    On tripoleT the oracle has no symmetrisation: its stresses are the loop's (compare where tfold_untouched)."""
    dom, prm = c.oracle_domain(), c.oracle_params()
    t, state = c.prep_inputs(icall)
    prep = oracle.prep(dom, oracle.PrepParams(**c.prep_scal_dict()), c.prep_static(), t, state)
    fx, tm, um = c.inputs(icall)
    dyn = {k: prep[k] for k in evp.FIELDS if k in prep}
    z = np.zeros(dom.shape)
    dyn.update(strength=fx["strength"], TbU=fx["TbU"], taubxU=z, taubyU=z)
    return prep, oracle_post(dom, prm, nsub, dyn, c.static(), {k: c.d[k] for k in ("dxU", "dyU", "tarear")}, prep["iceTmask"],
                             prep["iceUmask"], c.ns, (z, z))


def oracle_post(dom, prm, nsub, dyn, static, post_geo, tm, um, ns, strocn):
    loop = oracle.subcycle(dom, prm, nsub, dyn, static, tm, um)
    if ns == "tripole":
        oracle.tripole_stress_sym(dom, loop)
    out = {k: loop[k] for k in evp.OUTPUTS}
    post = oracle.deformations(dom, prm, loop["uvel"], loop["vvel"], static, post_geo, tm)
    fin = oracle.dyn_finish(dom, prm, dyn, loop["uvel"], loop["vvel"], um, *strocn)
    return dict(loop=out, deformations=post, dyn_finish=fin)


def run_chain(core, c: GoldenCase, icall, nsub, path="default", reference="fixture"):
    """One evp() call of the fixture on `core`, stage by stage.  reference = "fixture": the reference's own arrays (nsub must be
    one of post_counts(c)); "oracle": the oracle's chain (any count -- an odd one ends on the other ping-pong buffer)."""
    from test_oracle_golden import check_prep_products
    what = f"{c.name} call {icall} nsub {nsub} on {path}"
    fold = is_fold(c.ns)
    t, state = c.prep_inputs(icall)
    fx, _, _ = c.inputs(icall)
    # -- prep --
    tm, um, _ = core.prep(prep_params(c), t, dict(state, TbU=fx["TbU"]))
    out = {k: core.prep_fetch(k) for k in evp.PREP_FETCH}
    out.update(iceTmask=tm, iceUmask=um)
    out.update({k: v for k, v in core.download().items() if k in SIG})
    check_prep_products(c, icall, out, f"prep: {what}")
    # -- loop --
    core.set_strength(fx["strength"])
    core.set_tbu(fx["TbU"])
    core.subcycle(nsub)
    assert_path_ran(core, path, nsub, fold, fixture_lean(c, icall), f"loop: {what}")
    if fold:
        core.stress_halo()
    got = core.download()
    keep = None
    if reference == "fixture":
        want = dict(loop=c.expected(icall, nsub), deformations={k: c.d[f"o{icall:02d}n{nsub:04d}_{k}"] for k in POST},
                    dyn_finish={k: c.d[f"o{icall:02d}n{nsub:04d}_{k}"] for k in ("strocnxU", "strocnyU")})
    else:
        _, want = oracle_fixture_chain(c, icall, nsub)
        keep = tfold_untouched(c) if c.ns == "tripoleT" else None
    assert_stage(got, want["loop"], f"loop + download: {what}", keep)
    # -- post-loop --
    assert_bitwise(core.deformations(), want["deformations"], f"deformations: {what}")
    z = np.zeros(core.shape)
    assert_bitwise(core.dyn_finish(z, z), want["dyn_finish"], f"dyn_finish: {what}")
    return got


# ---- off the fixtures: synthetic grids against the oracle ----------------------------------------------------------------------
PPD = dict(dt=3600.0, rhoi=917.0, rhos=330.0, gravit=9.80616, dyn_area_min=1e-11, dyn_mass_min=1e-10)


class SynthChain:
    """A gx3- / tx3-sized synthetic case of the chain.  Closed grids with cover "full" / "caps" start from a model state
    (synth.make_primary: open-water patches, cells that gain and lose ice) and run cice_evp_hip_prep; cover "holes" -- random,
    mutually independent holes in iceTmask and iceUmask, which no preparation produces (it derives one mask from the other) -- and
    the tripole / tripoleT grids start at cice_evp_hip_upload with the loop's inputs.  tripoleT: the u-fold's grid under the T-fold
    halo rule, velocities handed over with the top row as the fold's image, dxhy / dyhx as CICE's halo update leaves them; `keep`
    marks where the stresses can be compared with the oracle's loop (everywhere but the rows evp()'s symmetrisation rewrites)."""

    def __init__(self, ns, cover, bs, holes=0.0, seed=20261020):
        spec = synth.GRIDS["gx3"]
        nx, ny = spec["nx"], spec["ny"]
        self.ns, self.cover, self.bs, self.holes = ns, cover, bs or (nx, ny), holes
        self.name = f"{nx}x{ny} {ns} {cover} blocks {self.bs[0]}x{self.bs[1]}" + (f" holes {holes}" if holes else "")
        # (tripoleT: the same grid as the u-fold's; only the halo rule differs, and the top row is an image)
        g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns=("tripole" if ns == "tripoleT" else ns)))
        self.dc = dc = decomp.Decomp(nx, ny, self.bs[0], self.bs[1], "cyclic", ns, 1)
        sc = lambda a, fill=0.0: dc.scatter(np.ascontiguousarray(a), 0, fill=fill)
        self.geo = {k: sc(g[k], 1.0 if k != "uarear" else 0.0) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")}
        self.post_geo = {k: sc(g[k], 1.0 if k != "tarear" else 0.0) for k in ("dxU", "dyU", "tarear")}
        self.fold_metrics = synth.bgrid_fold_metrics(dc, 0, g) if ns == "tripole" else None
        self.scal = synth.evp_scalars(120)
        blks = dc.local_blocks(0)
        self.blocks = [(b.ilo, b.ihi, b.jlo, b.jhi) for b in blks]
        self.dom = oracle.OracleDomain(dc.nx_block, dc.ny_block, len(blks), nx, ny, dc.ew, dc.ns, [b.ilo for b in blks], [b.ihi for b in blks],
                                       [b.jlo for b in blks], [b.jhi for b in blks], [b.gi0 for b in blks], [b.gj0 for b in blks])
        self.static = dict(oracle.metrics(self.dom, self.scal["deltaminEVP"], self.geo["HTE"], self.geo["HTN"], self.geo["tarea"]),
                           dxT=self.geo["dxT"], dyT=self.geo["dyT"], uarear=self.geo["uarear"])
        self.prm = oracle.make_params(**{k: self.scal[k] for k in ("arlx1i", "denom1", "brlx", "revp", "e_factor", "epp2i", "capping", "Ktens",
                                                                   "deltaminEVP", "u0", "cosw", "sinw", "rhow")})
        if ns == "tripoleT":
            # CICE's dxhy / dyhx after their halo update as cell-centre vector fields under the T-fold rule (top row made
            # symmetric, ghost row from row NY-1): oracle.metrics restates exactly that
            self.fold_metrics = (self.static["dxhy"], self.static["dyhx"])
        # tripoleT: the oracle has the loop's stresses, not evp()'s symmetrisation after it, which rewrites the top physical row and
        # the ghost row above it (common.tfold_untouched): the stresses are compared everywhere else, every other output everywhere
        self.keep = None
        if ns == "tripoleT":
            self.keep = np.ones(dc.shape(0), dtype=bool)
            for q, b in enumerate(blks):
                if b.gj0 + b.gny - 1 == ny:
                    self.keep[q, b.jhi - 1:, :] = False
        z = np.zeros(dc.shape(0))
        self.strocn = (np.full(dc.shape(0), SENTINEL[0]), np.full(dc.shape(0), SENTINEL[1]))
        self.prep_in = None
        if ns == "closed" and cover != "holes":
            pr = synth.make_primary(g, cover, seed=4)
            pstatic = {k: sc(v, (1.0 if k in ("tarea", "uarea") else 0)) for k, v in pr["static"].items()}
            t = {k: sc(v) for k, v in pr["t"].items()}
            state = {k: sc(v) for k, v in pr["state"].items()}
            self.prep_in = (pstatic, t, state)
            self.prep_want = w = oracle.prep(self.dom, oracle.PrepParams(**PPD, cosw=self.scal["cosw"], sinw=self.scal["sinw"], ssh_coupled=0),
                                             pstatic, t, dict(state, strintxU=z, strintyU=z, strocnxU=z, strocnyU=z))
            self.tm, self.um = w["iceTmask"], w["iceUmask"]
            self.strength = np.where(self.tm != 0, 2.75e4 * t["vice"] * np.exp(-20.0 * (1.0 - t["aice"])), 0.0)
            self.dyn = {k: w[k] for k in evp.FIELDS if k in w}
            self.dyn.update(strength=self.strength, TbU=z, strintxU=z, strintyU=z, taubxU=z, taubyU=z)
        else:
            st = synth.make_state(g, case=("full" if cover == "holes" else cover), seed=seed, warm=True)
            if ns == "tripoleT":
                # velocities as a halo update leaves them, as evp() hands them over: on the T-fold the top physical U row is the
                # image of the row below, a(i, NY) = -a(NX - i + 1, NY - 1)
                for k in ("uvel", "vvel", "uvel_init", "vvel_init"):
                    st[k] = np.array(st[k], dtype=np.float64, copy=True)
                    st[k][ny - 1, :] = -st[k][ny - 2, ::-1]
            if holes:
                rng = np.random.default_rng(seed)
                keep = np.zeros((ny, nx), dtype=bool)
                if is_fold(ns):          # ice stays on the fold rows and next to the pole columns (test_gpu_march_tripole.py: tripole_case)
                    keep[-2:, :] = True
                    for col in (0, 1, nx // 2 - 2, nx // 2 - 1, nx // 2, nx // 2 + 1, nx - 2, nx - 1):
                        keep[-8:, col] = True
                tmg = (st["iceTmask"] * ((rng.random((ny, nx)) > holes) | keep)).astype(np.int32)
                umg = (st["iceUmask"] * ((rng.random((ny, nx)) > holes) | keep)).astype(np.int32)
                for k in SIG:
                    st[k] = st[k] * tmg
                for k in ("uvel", "vvel", "uvel_init", "vvel_init"):
                    st[k] = st[k] * umg
                st["iceTmask"], st["iceUmask"] = tmg, umg
            self.dyn = {k: sc(st[k]) for k in evp.FIELDS}
            self.global_masks = (st["iceTmask"], st["iceUmask"])
            self.tm, self.um = dc.scatter(st["iceTmask"], 0, fill=0), dc.scatter(st["iceUmask"], 0, fill=0)

    @functools.lru_cache(maxsize=None)
    def oracle(self, ndte):
        """The oracle's chain for `ndte` subcycles (computed once; nobody writes into it)."""
        return oracle_post(self.dom, self.prm, ndte, self.dyn, self.static, self.post_geo, self.tm, self.um, self.ns, self.strocn)

    def lean(self):
        return len(self.blocks) == 1 and not is_fold(self.ns)

    def open_core(self, strict=True):
        d, keep = evp.make_dims(self.dc, 0)
        g = self.geo
        core = evp.EvpHip(d, evp.make_params(self.scal, strict=strict), g["HTE"], g["HTN"], g["dxT"], g["dyT"], g["uarear"], g["tarea"],
                          keepalive=keep, testing=True)
        if self.fold_metrics is not None:
            core.set_metrics(dxhy=self.fold_metrics[0], dyhx=self.fold_metrics[1])
        if self.prep_in:
            s = self.prep_in[0]
            core.set_prep_geometry(s["tmask"], s["umask"], s["hm"], s["tarea"], s["uarea"], s["fcor_blk"])
        core.set_post_geometry(self.post_geo["dxU"], self.post_geo["dyU"], self.post_geo["tarear"])
        return core

    def device_loop(self, core, ndte):
        """prep (or upload) and the loop on the device; returns the downloaded state (after stress_halo on a fold)."""
        what = f"{self.name} ndte {ndte}"
        if self.prep_in:
            _, t, state = self.prep_in
            w = self.prep_want
            tm, um, _ = core.prep(evp.PrepParams(**PPD, ssh_stress_coupled=0), t, state)
            assert bits_equal(tm, w["iceTmask"]) and bits_equal(um, w["iceUmask"]), f"prep: masks, {what}"
            on = um != 0
            for k in evp.PREP_FETCH:
                g = core.prep_fetch(k)
                sel = on if k in ("fmU", "strtltxU", "strtltyU") else slice(None)       # (defined on ice U-cells only)
                assert bits_equal(g[sel], w[k][sel]), f"prep: {k}, {what}"
            raw = core.download()
            assert_bitwise({k: raw[k] for k in SIG}, {k: w[k] for k in SIG}, f"prep: stresses after dyn_prep2, {what}")
            core.set_strength(self.strength)
        else:
            core.upload(self.dyn, self.tm, self.um)
        core.subcycle(ndte)
        if is_fold(self.ns):
            core.stress_halo()
        return core.download()


class TwoCalls:
    """Two calls of the per-call entry (cice_evp_hip_run) between which cells lose their ice: full cover on the gx3-sized closed
    grid in 25 x 29 blocks, then random, mutually independent holes in both masks.  Call 2 is entered as CICE would enter it with
    the stresses resident on the device: velocities zero off the new iceUmask (dyn_prep2), the caller's strintxU / strintyU / taubxU /
    taubyU holding `off` where the new mask has no ice -- the entry writes them on interior ice U-cells only, so they come back as the
    oracle leaves them: untouched."""
    off = 5.5

    def __init__(self, ndte=9, holes=0.3, seed=11):
        self.base = b = SynthChain("closed", "holes", (25, 29), 0.0)
        self.ndte = ndte
        self.out1 = oracle.subcycle(b.dom, b.prm, ndte, b.dyn, b.static, b.tm, b.um)
        rng = np.random.default_rng(seed)
        gt, gu = b.global_masks
        self.tm2 = b.dc.scatter((gt * (rng.random(gt.shape) > holes)).astype(np.int32), 0, fill=0)
        self.um2 = b.dc.scatter((gu * (rng.random(gu.shape) > holes)).astype(np.int32), 0, fill=0)
        d = dict(b.dyn)
        for k in SIG:
            d[k] = np.where(self.tm2 != 0, self.out1[k], 0.0)        # dyn_prep2: c0 off the ice (zero_sig_off_mask on the device)
        for k in ("uvel", "vvel"):
            d[k] = np.where(self.um2 != 0, self.out1[k], 0.0)
            d[k + "_init"] = d[k]
        for k in ("strintxU", "strintyU", "taubxU", "taubyU"):
            d[k] = np.where(self.um2 != 0, self.out1[k], self.off)
        self.dyn2 = d
        self.want2 = oracle_post(b.dom, b.prm, ndte, d, b.static, b.post_geo, self.tm2, self.um2, "closed", b.strocn)


@functools.lru_cache(maxsize=None)
def two_calls():
    return TwoCalls()


def run_synth_chain(core, case: SynthChain, ndte, path):
    what = f"{case.name} ndte {ndte} on {path}"
    want = case.oracle(ndte)
    got = case.device_loop(core, ndte)
    assert_path_ran(core, path, ndte, is_fold(case.ns), case.lean(), f"loop: {what}")
    assert_stage(got, want["loop"], f"loop + download: {what}", case.keep)
    post = core.deformations()
    assert_bitwise(post, want["deformations"], f"deformations: {what}")
    fin = core.dyn_finish(*case.strocn)
    assert_bitwise(fin, want["dyn_finish"], f"dyn_finish: {what}")
    return got, post, fin


@functools.lru_cache(maxsize=None)
def synth_case(name):
    return SynthChain(*SYNTH_CASES[name])


# name -> (ns, cover, blocks, holes); the paths each runs on are the test's
SYNTH_CASES = {
    "closed full 1blk": ("closed", "full", None, 0.0),
    "closed caps 25x29": ("closed", "caps", (25, 29), 0.0),
    "closed holes 30x40": ("closed", "holes", (30, 40), 0.3),        # padded last blocks both ways
    "tripole full 1blk": ("tripole", "full", None, 0.0),
    "tripole holes 25x29": ("tripole", "full", (25, 29), 0.4),
    "tripoleT full 1blk": ("tripoleT", "full", None, 0.0),
    "tripoleT holes 25x29": ("tripoleT", "full", (25, 29), 0.4),
}
FUSED_CASE, FUSED_NDTE = "closed holes 30x40", 7       # the fused-mode check of the two post-loop kernels
SYNTH_NDTE = (9, 7)             # 1 + 4 + 4 (the leading single subcycle) and 4 + 3; with three per pass 3 x 3 and 3 + 3 + 1


def top_rows_move(case: SynthChain, ndte):
    u = case.dc.gather({0: case.oracle(ndte)["loop"]["uvel"]})
    return float(np.abs(u[-3:]).max())


def edge_blocks_with_ice(case: SynthChain):
    """Blocks with an ice T-cell in their first interior column or row: their divu reads the west / south ghost velocities."""
    return [b for b, (ilo, ihi, jlo, jhi) in enumerate(case.blocks)
            if case.tm[b, jlo - 1:jhi, ilo - 1].any() or case.tm[b, jlo - 1, ilo - 1:ihi].any()]


def zero_ghosts(case: SynthChain, a):
    """`a` with every cell outside the blocks' interiors zeroed (a stale ghost cell, in its bluntest form)."""
    out = np.zeros_like(a)
    for b, (ilo, ihi, jlo, jhi) in enumerate(case.blocks):
        out[b, jlo - 1:jhi, ilo - 1:ihi] = a[b, jlo - 1:jhi, ilo - 1:ihi]
    return out
