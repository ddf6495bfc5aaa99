"""What evp() does around the C grid's subcycle loop, as ONE chain that names its stages (test infrastructure, no GPU needed to
import; the C-grid twin of tests/evp_call_chain.py): cgrid_set_prep_geometry -> cgrid_prep (state handed in on the first call of a
core, None afterwards) -> cgrid_set_tb or no seabed stress -> cgrid_prep_finish -> cgrid_subcycle -> cgrid_download ->
cgrid_deformations -> cgrid_dyn_finish (N and E) -> cgrid_tail -> cgrid_dyn_finish_u -> cgrid_strocn_t -> cgrid_download again.
Every schedule of the loop leaves uvelE, vvelN, stresspT, stressmT and stress12U in one of two allocations each
(evp_host_cgrid.h: PingPong, Ran::swapped); every call after the loop, and the next cgrid_prep without a state, reads them where
CG.f[...] points at that moment.  run_fixture_call / run_synth_call / run_split_calls run the chain on a core whose schedule the caller forced (CG_PATHS, set_cg_path) and
compares every stage with the reference's fixture arrays or with the oracle's chain (oracle_post, SynthCg.oracle_call), bit for bit on
every cell, every message starting with the stage; assert_cg_path_ran is the evidence that the named schedule did the work and that
the five arrays ended where that schedule's swaps put them (cgrid_timings()["in_alt"])."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import oracle
import tail_ref
from cice_amd import decomp, evp, synth
from common import CGRID_CASES, CGRID_TFOLD_CASES, GoldenCase, assert_bitwise, bits_equal

SENT = 7.25                     # what the inout arrays hold off their lists when they are handed over
POST = ("divu", "shear", "vort", "rdg_conv", "rdg_shear")
FIN = ("strocnxN", "strocnyN", "strocnxE", "strocnyE")
# the stages a message can begin with: prep, loop, loop + download, deformations, dyn_finish, tail, dyn_finish_u, strocn_t, download after the tail
PREP_KEYS = oracle.C_FIELDS[:14] + [k for k in oracle.C_INPUTS if k != "strength"]
PP_FOUR, PP_S12, PP_ALL = 15, 16, 31        # bits of cgrid_timings()["in_alt"]: uvelE, vvelN, stresspT, stressmT | stress12U
ODD_EVEN = (7, 8)               # counts no fixture has: each schedule ends in either allocation

# every switch a row of CG_PATHS sets (and the ones the files that take their rows from here set beside them), cleared before a
# row's own are set
CG_SWITCHES = ("CICE_EVP_HIP_CGRID_RESIDENT", "CICE_EVP_HIP_CGRID_ONE", "CICE_EVP_HIP_CGRID_FUSED", "CICE_EVP_HIP_CGRID_STRIP",
               "CICE_EVP_HIP_CGRID_ONE_SHAPE", "CICE_EVP_HIP_CGRID_FAST", "CICE_EVP_HIP_CGRID_STRIP_LAST", "CICE_EVP_HIP_CGRID_STRIP_SEG",
               "CICE_EVP_HIP_CGRID_STRIP_LEN", "CICE_EVP_HIP_CGRID_MARCH_FOLD", "CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL")


class Row(NamedTuple):
    env: dict
    kind: str                   # one | fused | phases | strip | res | res_fold | mfold
    grids: tuple                # fixture | closed1 | closedN | strip | fold | foldT | foldres: the shapes the row runs on (SYNTH's tags)
    visc: str = "avg_zeta"
    seabed: bool = False        # the row wants TbE / TbN != 0 (cg_res: the SLOW variant)
    flags_split: object = None  # tests/test_gpu_cgrid_call_flags.py: 3 x 3 padded blocks (True), one block (False), not run there (None)


_OFF = {"CICE_EVP_HIP_CGRID_RESIDENT": "0"}
_ONE = dict(_OFF, CICE_EVP_HIP_CGRID_STRIP="0")
_FUSED = dict(_OFF, CICE_EVP_HIP_CGRID_ONE="0")
_PHASES = dict(_OFF, CICE_EVP_HIP_CGRID_FUSED="0")
_STRIP = dict(_OFF, CICE_EVP_HIP_CGRID_ONE_SHAPE="2", CICE_EVP_HIP_CGRID_STRIP="1")
_RES = {"CICE_EVP_HIP_CGRID_RESIDENT": "1"}
_MFOLD = dict(_OFF, CICE_EVP_HIP_CGRID_MARCH_FOLD="1")
# The one table of C-grid schedules.  (schedule, grid) pairs the library refuses are absent: DESIGN.md section 2 lists them with the
# refusal texts.
CG_PATHS = {
    "cg_one": Row(_ONE, "one", ("fixture", "closed1"), flags_split=True),
    "fused, three launches": Row(_FUSED, "fused", ("fixture", "closed1"), flags_split=True),
    "five phases": Row(_PHASES, "phases", ("fixture", "closed1", "foldres"), flags_split=True),
    "cg_strip": Row(_STRIP, "strip", ("strip",), flags_split=False),
    "cg_strip, STRIP_LAST=0": Row(dict(_STRIP, CICE_EVP_HIP_CGRID_STRIP_LAST="0"), "strip", ("strip",)),
    "cg_res": Row(_RES, "res", ("fixture", "closedN"), flags_split=True),          # several blocks
    "cg_res, one block": Row(_RES, "res", ("closed1",), flags_split=False),         # (no fixture has one block, no fold and deep water)
    "cg_res SLOW": Row(_RES, "res", ("fixture", "closed1"), seabed=True),
    "five phases + cg_res FOLD": Row(_RES, "res_fold", ("fixture", "foldres")),    # tripole (u-fold): enqueue_phases_resident
    "marched zone + fold band": Row(_MFOLD, "mfold", ("fold",)),
    "marched zone + fold band, tripoleT": Row(_MFOLD, "mfold", ("foldT",)),
    "marched zone + fold band, serial": Row(dict(_MFOLD, CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL="1"), "mfold", ("fold",)),
    # visc_method = avg_strength on every schedule that accepts it (the three-launch kernels and the marched zone + fold band do not)
    "cg_one, avg_strength": Row(_ONE, "one", ("fixture", "closed1"), visc="avg_strength"),
    "five phases, avg_strength": Row(_PHASES, "phases", ("fixture", "closed1", "foldres"), visc="avg_strength"),
    "cg_strip, avg_strength": Row(_STRIP, "strip", ("strip",), visc="avg_strength"),
    "cg_res, avg_strength": Row(_RES, "res", ("fixture", "closed1"), visc="avg_strength"),
    "five phases + cg_res FOLD, avg_strength": Row(_RES, "res_fold", ("fixture", "foldres"), visc="avg_strength"),
}
# (the five phases work in place; cg_res leaves its result in both allocations and, with avg_strength, follows a first subcycle in place)
PING_PONG = [p for p, r in CG_PATHS.items() if r.kind not in ("phases", "res_fold") and not (r.kind == "res" and r.visc == "avg_strength")]


def set_cg_path(monkeypatch, path, **extra):
    for k in CG_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(CG_PATHS[path].env, **extra).items():
        monkeypatch.setenv(k, v)


def strip_last(path):
    return CG_PATHS[path].env.get("CICE_EVP_HIP_CGRID_STRIP_LAST") != "0"


def resident_subcycles(n, first):
    """cg_res takes every subcycle of a call but the first after an upload, from three on (cgrid_schedule.cpp: res_subcycles)."""
    m = n - (1 if first else 0)
    return m if m >= 3 else 0


def predicted_swaps(path, n, first):
    """The bits of in_alt a call of n subcycles flips -- the host's rules restated (evp_host_cgrid_loop.cpp: enqueue_fused,
    enqueue_march_fold, enqueue_phases_resident), so that a read-out that disagrees is a finding and tests/test_cgrid_call_chain_cpu.py
    can show without a GPU that every ping-pong row's calls end in both allocations.  The first subcycle after an upload: the
    three-launch kernels (stress12U swaps alone), in place with avg_strength and beside a fold."""
    row = CG_PATHS[path]
    odd = lambda k: k % 2 == 1
    kind = row.kind
    if kind == "res":
        if resident_subcycles(n, first):         # (the launch leaves its result in both allocations: only the leading subcycle swaps)
            return PP_S12 if first and row.visc == "avg_zeta" else 0
        kind = "one"
    if kind in ("phases", "res_fold"):
        return 0
    if kind == "fused":
        return PP_S12 if odd(n) else 0
    if kind in ("one", "strip"):
        if not first:
            return PP_ALL if odd(n) else 0
        lead = PP_S12 if row.visc == "avg_zeta" else 0
        return lead ^ (PP_ALL if odd(n - 1) else 0)
    assert kind == "mfold"
    m = n - (1 if first else 0) - (0 if strip_last(path) else 1)
    return PP_ALL if odd(max(m, 0)) else 0


def assert_cg_path_ran(core, path, n, first, what, before):
    """The loop of the call just made (n subcycles; first: the first call after an upload / a preparation) ran on the schedule `path`
    names.  before: in_alt when the call began -- the word must now be before ^ predicted_swaps (the counters do not tell the three
    fused launches from the five phases: the swap of stress12U does).  Returns in_alt."""
    row = CG_PATHS[path]
    t = core.cgrid_timings()
    m = n - (1 if first else 0)
    assert t["resident_fallbacks"] == 0 and t["nsub"] == n, (what, t)
    nres = resident_subcycles(n, first) if row.kind in ("res", "res_fold") else 0
    assert t["resident_subcycles"] == nres, (what, t)
    if row.kind in ("one", "strip") or (row.kind == "res" and nres == 0):
        assert t["one_launch_subcycles"] == m and t["marched_fold_subcycles"] == 0, (what, t)
        assert (t["marched_items"] > 0) == (row.kind == "strip"), (what, t)
    elif row.kind == "res":
        assert t["one_launch_subcycles"] == 0 and t["marched_fold_subcycles"] == 0, (what, t)
        if core.testing:
            assert core.call_flags()["cgrid_fast"] == (not row.seabed), (what, core.call_flags())
    elif row.kind == "mfold":
        assert t["marched_fold_subcycles"] == max(m - (0 if strip_last(path) else 1), 0), (what, t)
        assert t["fold_band_rows"] > 0 and t["marched_items"] > 0 and t["fold_rest_cells"] > 0 and t["one_launch_subcycles"] == 0, (what, t)
        assert "marched zone + fold band" in core.describe_path(), (what, core.describe_path())
    else:           # fused, phases, res_fold: what tells the three launches from the five phases is the swap of stress12U below
        assert t["one_launch_subcycles"] == 0 and t["marched_fold_subcycles"] == 0 and t["marched_items"] == 0, (what, t)
        assert "marched zone" not in core.describe_path(), (what, core.describe_path())
    assert t["in_alt"] == before ^ predicted_swaps(path, n, first), (what, f"in_alt {before:#x} -> {t['in_alt']:#x}", t)
    return t["in_alt"]


class Seen:
    """in_alt after every call of a test: a ping-pong row must have ended with the word zero AND non-zero."""

    def __init__(self, path):
        self.path, self.words = path, []

    def add(self, word):
        self.words.append(word)

    def assert_both(self):
        if self.path in PING_PONG:
            assert any(w == 0 for w in self.words) and any(w != 0 for w in self.words), \
                f"{self.path}: the calls ended with in_alt {[hex(w) for w in self.words]}: never in both allocations"
        else:
            assert not any(self.words), (self.path, self.words)


# ---- the restatements after the loop, on any final state -------------------------------------------------------------------------
def interior(shape, blocks):
    return tail_ref._interior(shape, blocks)


def u_point_inputs(shape, iceU, seed):
    """U-point operands of dyn_finish for a C-grid case (the loop holds none): any numbers do."""
    rng = np.random.default_rng(seed)
    ai = np.where(iceU != 0, rng.uniform(0.2, 1.0, shape), np.where(rng.uniform(size=shape) < 0.5, 0.0, 1e-12))
    return dict(cdn_ocnU=np.full(shape, 0.00536), aiU=ai, uocnU=rng.uniform(-0.1, 0.1, shape), vocnU=rng.uniform(-0.1, 0.1, shape),
                fmU=rng.uniform(-20.0, 20.0, shape))


def sentinels(shape):
    return {k: np.full(shape, SENT) for k in POST + FIN + ("strocnxU", "strocnyU")}


def oracle_post(dom, prm, blocks, static, tarear, e_factor, loop, inputs, masks, uin, tail_halo=True):
    """Everything evp() and step_dyn_horiz compute from the loop's final state `loop` (C_FIELDS), each stage fed by the one before:
    deformationsC_T, dyn_finish at N and E points, the halo update of strintxE / strintyN and its U-point averages, dyn_finish at U
    points, the T-point ocean stress; every inout array starts as the sentinel.  tail_halo=False: strintxE / strintyN left without
    their halo update (planted error)."""
    shape = loop["uvelE"].shape
    s = sentinels(shape)
    out = dict(loop=loop)
    out["deformations"] = oracle.deformations_c_t(dom, e_factor, loop, static, tarear, masks["iceTmask"], prev={k: s[k] for k in POST})
    fin = {}
    for loc in "NE":
        fin[f"strocnx{loc}"], fin[f"strocny{loc}"] = oracle.dyn_finish_at(
            dom, prm, inputs[f"cdn_ocn{loc}"], inputs[f"ai{loc}"], inputs[f"uocn{loc}"], inputs[f"vocn{loc}"], inputs[f"fm{loc}"],
            loop[f"uvel{loc}"], loop[f"vvel{loc}"], masks[f"ice{loc}mask"], s[f"strocnx{loc}"], s[f"strocny{loc}"])
    out["dyn_finish"] = fin
    tail = tail_ref.cgrid_tail(dom, blocks, loop["strintxE"], loop["strintyN"], static)
    if not tail_halo:
        nohalo = dict(tail, strintxE=np.array(loop["strintxE"]), strintyN=np.array(loop["strintyN"]))
        nohalo["strintxU"] = tail_ref.x2ys(blocks, nohalo["strintxE"], static["earea"], static["epm"], "N")
        nohalo["strintyU"] = tail_ref.x2ys(blocks, nohalo["strintyN"], static["narea"], static["npm"], "E")
        tail = nohalo
    out["tail"] = tail
    sx, sy = oracle.dyn_finish_at(dom, prm, uin["cdn_ocnU"], uin["aiU"], uin["uocnU"], uin["vocnU"], uin["fmU"], loop["uvel"], loop["vvel"],
                                  masks["iceUmask"], s["strocnxU"], s["strocnyU"])
    out["dyn_finish_u"] = dict(strocnxU=sx, strocnyU=sy)
    out["strocn_t"] = tail_ref.strocn_t(dom, blocks, sx, sy, uin["aiU"], static["uarea"], static["tarea"])
    out["final"] = dict(loop, strintxE=tail["strintxE"], strintyN=tail["strintyN"])
    return out


def run_post(core, want, tarear, uin, what):
    """The calls after the loop on `core` against `want` (oracle_post's stages), every cell, the sentinel where nothing is owned."""
    s = sentinels(core.shape)
    assert_bitwise(core.cgrid_deformations(tarear, prev={k: s[k] for k in POST}), want["deformations"], f"deformations: {what}")
    assert_bitwise(core.cgrid_dyn_finish(prev={k: s[k] for k in FIN}), want["dyn_finish"], f"dyn_finish: {what}")
    assert_bitwise(core.cgrid_tail(), want["tail"], f"tail: {what}")
    assert_bitwise(core.cgrid_dyn_finish_u(uin, prev={k: s[k] for k in ("strocnxU", "strocnyU")}), want["dyn_finish_u"], f"dyn_finish_u: {what}")
    assert_bitwise(core.cgrid_strocn_t(), want["strocn_t"], f"strocn_t: {what}")
    assert_bitwise(core.cgrid_download(), want["final"], f"download after the tail: {what}")


def new_core(dims, keep, scal, static, prep_static=None, testing=True):
    core = evp.EvpHip(dims, evp.make_params(scal, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"],
                      np.where(static["uarea"] > 0, 1.0 / np.where(static["uarea"] > 0, static["uarea"], 1.0), 0.0), static["tarea"],
                      keepalive=keep, testing=testing)
    core.cgrid_set_geometry(static)
    if prep_static is not None:
        core.cgrid_set_prep_geometry(prep_static)
    return core


# ---- the reference's fixtures ----------------------------------------------------------------------------------------------------
def fixture_rows():
    """(fixture, row) for every C-grid fixture and every fixture-sized row whose schedule accepts the fixture's grid and
    visc_method; REFUSED: the pairs the library itself turns down (the text it gives: DESIGN.md section 2)."""
    rows = []
    for name in CGRID_CASES + CGRID_TFOLD_CASES:
        c = GoldenCase(name)
        for path, r in CG_PATHS.items():
            if "fixture" in r.grids and fixture_accepts(c, path):
                rows.append((name, path))
    return rows


# (schedule kind, fixture) the library refuses with RESIDENT=1 (cgres_dependencies: a cut whose windows have one-way hand-offs; a block
# too small for a window table)
REFUSED = {("res", "cgrid_closed_2x2_revp")}      # "static array 11 differs between the ghost cells 392 and 154 outside the domain"


def fixture_accepts(c: GoldenCase, path):
    r = CG_PATHS[path]
    fold, seabed = c.ns in ("tripole", "tripoleT"), c.scal[23] != 0.0
    if r.visc != str(c.d["visc_method"]) or (r.kind, c.name) in REFUSED:
        return False
    if r.kind == "phases":
        return True
    if r.kind == "res_fold":
        return c.ns == "tripole"
    if fold or r.kind not in ("one", "fused", "res"):
        return False
    if r.kind == "res":          # SLOW: whatever the cut; the default configuration: by the number of blocks
        return r.seabed == seabed and (seabed or r.visc != "avg_zeta" or ("one block" in path) == (c.nblocks == 1))
    return True


def fixture_masks_change(c: GoldenCase, icall):
    """Faces whose ice mask differs between call icall - 1 and call icall of the fixture, {mask: (gained, lost)}, empty where none."""
    out = {}
    for k in oracle.C_MASKS:
        new, old = c.d[f"in{icall:02d}_{k}"] != 0, c.d[f"in{icall - 1:02d}_{k}"] != 0
        if (new & ~old).any() or (old & ~new).any():
            out[k] = (int((new & ~old).sum()), int((old & ~new).sum()))
    return out


def fixture_prep_params(c: GoldenCase):
    d = c.prep_scal_dict()
    return evp.PrepParams(dt=d["dt"], rhoi=d["rhoi"], rhos=d["rhos"], gravit=d["gravit"], dyn_area_min=d["dyn_area_min"],
                          dyn_mass_min=d["dyn_mass_min"], ssh_stress_coupled=d["ssh_coupled"])


def fixture_core(c: GoldenCase):
    d, keep = c.hip_dims()
    return new_core(d, keep, c.scal_dict(), c.cgrid_static(), c.cgrid_prep_static())


def fixture_lists(c: GoldenCase, masks):
    """The lists: the ice T-cells deformationsC_T rewrites (the interior and the ghost row / column north and east of it), the ice
    N / E faces of the interior (dyn_prep2)."""
    shape = masks["iceTmask"].shape
    blocks = tail_ref.blocks_of(c)
    ring = np.zeros(shape, dtype=bool)
    for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
        ring[b, jlo - 1:jhi + 1, ilo - 1:ihi + 1] = True
    inn = interior(shape, blocks)
    return dict(T=ring & (masks["iceTmask"] != 0), N=inn & (masks["iceNmask"] != 0), E=inn & (masks["iceEmask"] != 0))


def fixture_want(c: GoldenCase, icall, nsub, uin):
    """The stages of call `icall` with `nsub` subcycles from the reference's own arrays where the fixture holds them -- the loop
    (strintxE / strintyN after the reference's halo update), deformationsC_T, dyn_finish at N and E --, the restatements on the
    reference's final state for the rest."""
    dom, prm, blocks, static = c.oracle_domain(), c.oracle_params(), tail_ref.blocks_of(c), c.cgrid_static()
    _, inputs, masks = c.cgrid_inputs(icall)
    loop = c.cgrid_expected(icall, nsub)
    want = oracle_post(dom, prm, blocks, static, c.d["tarear"], float(c.scal[4]), loop, inputs, masks, uin)
    pre = f"o{icall:02d}n{nsub:04d}_"
    on = fixture_lists(c, masks)
    want["deformations"] = {k: np.where(on["T"], c.d[pre + k], SENT) for k in POST}
    want["dyn_finish"] = {k: np.where(on[k[-1]], c.d[pre + k], SENT) for k in FIN}
    want["tail"] = dict(want["tail"], strintxE=loop["strintxE"], strintyN=loop["strintyN"])
    want["final"] = loop
    return want


def fixture_oracle_want(c: GoldenCase, icall, nsub, uin):
    """The oracle's chain on the reference's loop inputs of call `icall` (the preparation stage has been compared with exactly these
    arrays) for a count the fixture does not hold.  The state is the oracle's own preparation of the fixture's model state: the
    fixture's in* arrays are the same but for strintxE / strintyN, which were captured after evp()'s halo update, while the loop
    starts -- in the reference as on the device -- from the arrays before it (ghost cells, and the N faces on a fold, differ)."""
    dom, prm, blocks, static = c.oracle_domain(), c.oracle_params(), tail_ref.blocks_of(c), c.cgrid_static()
    _, inputs, masks = c.cgrid_inputs(icall)
    t, st, prev = c.cgrid_prep_inputs(icall)
    prep = oracle.cgrid_prep(dom, oracle.PrepParams(**c.prep_scal_dict()), c.cgrid_prep_static(), t, st, prev)
    state = {k: prep[k] for k in oracle.C_FIELDS[:14]}
    loop = oracle.cgrid_subcycle(dom, prm, nsub, state, inputs, static, masks, visc_method=str(c.d["visc_method"]))
    return oracle_post(dom, prm, blocks, static, c.d["tarear"], float(c.scal[4]), loop, inputs, masks, uin)


def run_fixture_call(core, c: GoldenCase, icall, nsub, path, seen: Seen, resident_state=False, reference="fixture"):
    """One evp() call of the fixture on `core`, stage by stage.  resident_state: cgrid_prep with state = None (the device holds what
    the reference entered this call with: the state the previous call of the chain left)."""
    what = f"{c.name} call {icall} nsub {nsub} on {path}"
    dom = c.oracle_domain()
    t, st, _ = c.cgrid_prep_inputs(icall)
    want_state, want_in, want_masks = c.cgrid_inputs(icall)
    before = core.cgrid_timings()["in_alt"]
    # -- prep --
    masks = core.cgrid_prep(fixture_prep_params(c), t, None if resident_state else {k: st[k] for k in oracle.C_FIELDS[:12]},
                            {k: st[k] for k in ("iceUmask", "iceEmask", "iceNmask")})
    if c.scal[23] != 0.0:        # seabed stress: the reference's own factors (the device's exp() has its own file)
        core.cgrid_set_tb(want_in["TbE"], want_in["TbN"])
    core.cgrid_prep_finish(want_in["strength"], str(c.d["visc_method"]))
    for k in oracle.C_MASKS:
        assert bits_equal(masks[k] != 0, want_masks[k] != 0), f"prep: {what}: {k}"
    if icall > 1:
        assert fixture_masks_change(c, icall), f"prep: {what}: no face gains or loses ice between the calls"
    got = {k: core.cgrid_fetch(k) for k in PREP_KEYS}
    oracle.halo_update(dom, got["strintxE"], "Eface", "vector")      # (the fixture's in* arrays: after a whole evp() of no subcycles)
    oracle.halo_update(dom, got["strintyN"], "Nface", "vector")
    assert_bitwise(got, {k: v for k, v in {**want_state, **want_in}.items() if k in got}, f"prep: {what}")
    # -- loop --
    core.cgrid_subcycle(nsub)
    seen.add(assert_cg_path_ran(core, path, nsub, True, f"loop: {what}", before))
    uin = u_point_inputs(core.shape, want_masks["iceUmask"], seed=17)
    want = fixture_want(c, icall, nsub, uin) if reference == "fixture" else fixture_oracle_want(c, icall, nsub, uin)
    out = core.cgrid_download()
    if reference == "fixture":
        oracle.halo_update(dom, out["strintxE"], "Eface", "vector")
        oracle.halo_update(dom, out["strintyN"], "Nface", "vector")
    assert_bitwise(out, want["loop"], f"loop + download: {what}")
    run_post(core, want, c.d["tarear"], uin, what)
    return want


def run_fixture_chain(core, c: GoldenCase, path):
    """Every call and count of the fixture as consecutive evp() calls on ONE core (call 2's first run enters with state = None, as
    the reference entered it: from the state its last run of call 1 left), then 7 and 8 subcycles through the oracle's chain."""
    seen = Seen(path)
    for icall in range(1, c.ncalls + 1):
        for q, nsub in enumerate(c.nsub_list):
            # the reference's state before call 2 is what ITS last run of call 1 left: the chain's previous call
            run_fixture_call(core, c, icall, nsub, path, seen, resident_state=(icall > 1 and q == 0))
    for nsub in ODD_EVEN:
        want = run_fixture_call(core, c, c.ncalls, nsub, path, seen, reference="oracle")
        for stage in ("deformations", "dyn_finish", "tail", "dyn_finish_u", "strocn_t"):
            assert all(np.abs(np.where(v == SENT, 0.0, v)).max() > 0 for v in want[stage].values()), (stage, c.name)
    seen.assert_both()
    return seen


# ---- off the fixtures: the smallest grids on which a zone forms, against the oracle's chain ------------------------------------------
PPD = dict(dt=3600.0, rhoi=917.0, rhos=330.0, gravit=9.80616, dyn_area_min=1e-11, dyn_mass_min=1e-10)
PREP_LOC = {"umaskCD": "NEcorner", "emask": "Eface", "nmask": "Nface", "fcor_blk": "NEcorner", "fcorE_blk": "Eface", "fcorN_blk": "Nface"}
T_VECTOR = ("uocn", "vocn", "ss_tltx", "ss_tlty", "strairxT", "strairyT")


def _loc(k):
    return PREP_LOC.get(k) or next((l for l, names in synth.CGRID_LOC.items() if k in names), "center")


class SynthCg:
    """A synthetic C-grid case of the chain that starts from a model state: T-grid fields of two consecutive calls between which
    cells gain and lose ice (synth.cgrid_prep_inputs with two seeds), the 12 state arrays evp() is first entered with, previous
    masks that differ from the ones the preparation finds.  kind "closed": a gx3-sized closed grid; "strip": cyclic in both directions (test_gpu_cgrid.marched_case's
    grid: ocean up to the top and bottom rows), "fold": a tripole (u-fold) grid with random land and ice kept on the fold rows and
    beside the poles (test_gpu_cgrid_march_tripole.fold_case's grid), "foldT": the same grid under the T-fold rule -- every block
    array's ghost cells as ice_HaloUpdate leaves them there."""

    def __init__(self, kind, nx, ny, bs, seed, land=0.02, visc="avg_zeta", seabed=False):
        self.kind, self.visc, self.bs, self.seabed = kind, visc, bs, seabed
        self.ns = {"closed": "closed", "strip": "cyclic", "fold": "tripole", "foldT": "tripoleT"}[kind]
        self.name = f"{nx}x{ny} {self.ns} blocks {bs[0]}x{bs[1]}" + (f" {visc}" if visc != "avg_zeta" else "") + (" seabed" if seabed else "")
        rng = np.random.default_rng(seed)
        if kind == "strip":
            from test_gpu_cgrid import marched_case_global
            g, cg, state, _, _ = marched_case_global(seed, nx, ny, "full", 0.0, land, ns="cyclic")
        elif kind == "closed":
            g = synth.derive_geometry(synth.make_grid(nx, ny, synth.GRIDS["gx3"]["dx0"], ns="closed"))
            cg = synth.cgrid_geometry(g)
            state, _, _ = synth.cgrid_state(g, cg, case="full", seed=seed)
        else:
            g0 = synth.make_grid(nx, ny, 2.0e4, ns="tripole")
            keep = np.zeros((ny, nx), dtype=bool)
            keep[-2:, :] = True
            for col in (0, 1, nx // 2 - 2, nx // 2 - 1, nx // 2, nx // 2 + 1, nx - 2, nx - 1):
                keep[-8:, col] = True
            g0["kmt"] = g0["kmt"] * ((rng.random((ny, nx)) >= land) | keep)
            g = synth.derive_geometry(g0)
            cg = synth.cgrid_geometry(g)
            state, _, _ = synth.cgrid_state(g, cg, case="full", seed=seed)
        # scattered by the u-fold's rule (or the cyclic one); foldT: redone below by the T-fold's
        dcs = decomp.Decomp(nx, ny, bs[0], bs[1], "cyclic", "tripole" if kind == "foldT" else self.ns, 1)
        self.dc = dc = decomp.Decomp(nx, ny, bs[0], bs[1], "cyclic", self.ns, 1)
        self.dom, self.blocks = tail_ref.domain_of_decomp(dc), tail_ref.blocks_of_decomp(dc)
        z = {k: np.zeros((ny, nx)) for k in oracle.C_INPUTS}
        static, state, _, _ = synth.cgrid_scatter(dcs, 0, cg, {k: state[k] for k in oracle.C_FIELDS[:12]}, z, {})
        self.calls = []
        for s in (seed + 100, seed + 200):
            t, st7, prev = synth.cgrid_prep_inputs(g, cg, case="full", seed=s)
            # open water in patches of 5 x 5 cells, elsewhere in each call: dyn_prep1 extends iceTmask by one cell around the pack, so
            # only the middle of a patch loses (and, where the other call's patch was, gains) its T-cell
            prng = np.random.default_rng(s)
            for _ in range(max(8, nx * ny // 800)):
                j, i = int(prng.integers(2, ny - 14)), int(prng.integers(0, nx - 5))
                for k in ("aice", "vice", "vsno", "aice_init", "strairxT", "strairyT"):
                    t[k][j:j + 5, i:i + 5] = 0.0
            tb = {k: dcs.scatter(v, 0, fold=("center", -1.0 if k in T_VECTOR else 1.0)) for k, v in t.items()}
            self.calls.append(dict(t=tb, prev={k: dcs.scatter(v, 0, fill=0) for k, v in prev.items()}))
        static.update({k: dcs.scatter(v, 0, fill=0, fold=(PREP_LOC.get(k, "center"), 1.0)) for k, v in st7.items()})
        if kind == "foldT":
            for k in static:
                self._tfold_halo(static[k], k, False)
            for b, blk in enumerate(dc.local_blocks(0)):        # the boundary-condition ratios as init_evp builds them, from these block arrays
                js, je, is_, ie = blk.jlo - 1, blk.jhi, blk.ilo - 1, blk.ihi
                rx = -static["dxN"][b][js:je, is_ + 1:ie + 1] / static["dxN"][b][js:je, is_:ie]
                ry = -static["dyE"][b][js + 1:je + 1, is_:ie] / static["dyE"][b][js:je, is_:ie]
                static["ratiodxN"][b][js:je, is_:ie], static["ratiodxNr"][b][js:je, is_:ie] = rx, 1.0 / rx
                static["ratiodyE"][b][js:je, is_:ie], static["ratiodyEr"][b][js:je, is_:ie] = ry, 1.0 / ry
            for k in state:
                self._tfold_halo(state[k], k, k in synth.CGRID_VECTOR)
            for call in self.calls:
                for k in call["t"]:
                    self._tfold_halo(call["t"][k], k, k in T_VECTOR)
        # seabed stress: water of 3 .. 60 m under 2 m of ice; the factors are the oracle's (LKD), handed to the device by cgrid_set_tb
        self.hwater = dcs.scatter(np.random.default_rng(seed + 7).uniform(3.0, 60.0, (ny, nx)), 0, fill=60.0) if seabed else None
        self.static, self.state = static, {k: np.ascontiguousarray(v) for k, v in state.items()}
        self.tarear = np.where(static["tarea"] > 0, 1.0 / static["tarea"], 0.0)
        self.scal = synth.evp_scalars(120)
        self.prm = oracle.make_params(**{k: self.scal[k] for k in ("arlx1i", "denom1", "brlx", "revp", "e_factor", "epp2i", "capping", "Ktens",
                                                                   "deltaminEVP", "u0", "cosw", "sinw", "rhow")})
        self.pp = oracle.PrepParams(**PPD, cosw=self.scal["cosw"], sinw=self.scal["sinw"], ssh_coupled=0)

    def _tfold_halo(self, a, k, vector):
        b = np.ascontiguousarray(a, dtype=np.float64)
        oracle.halo_update(self.dom, b, _loc(k), "vector" if vector else "scalar")
        a[...] = b

    def open_core(self):
        d, keep = evp.make_dims(self.dc, 0)
        return new_core(d, keep, self.scal, self.static, self.static)

    def strength(self, icall, masks):
        t = self.calls[icall - 1]["t"]
        return np.where(masks["iceTmask"] != 0, 2.75e4 * t["vice"] * np.exp(-20.0 * (1.0 - t["aice"])), 0.0)

    def uin(self, icall, masks):
        return u_point_inputs(self.dom.shape, masks["iceUmask"], seed=17 + icall)

    def oracle_prep(self, icall, prev_call=None, keep_lost_stresses=False, last_inputs=None):
        """The oracle's preparation of call `icall`: call 1 from the state handed in, call 2 from what the oracle's own call 1 left
        (prev_call: its oracle_call).  last_inputs: the loop's inputs of whatever call ran before a call 1 -- the faces without ice keep
        e.g. their old fmE, in CICE's arrays as on the device.  keep_lost_stresses: the stresses kept where a cell lost its ice (planted error: what a second
        allocation that was never cleared there holds)."""
        call = self.calls[icall - 1]
        if prev_call is None:
            state, prev_masks, prev_in = self.state, call["prev"], last_inputs
        else:
            state = {k: prev_call["final"][k] for k in oracle.C_FIELDS[:14]}
            prev_masks = {k: prev_call["masks"][k] for k in ("iceUmask", "iceEmask", "iceNmask")}
            prev_in = prev_call["inputs"]
        prep = oracle.cgrid_prep(self.dom, self.pp, self.static, call["t"], dict(state, **prev_masks), prev_in)
        if keep_lost_stresses:
            for k in ("stresspT", "stressmT", "stress12T", "stress12U"):
                prep[k] = np.where(prep[k] == 0.0, state[k], prep[k])
        return prep

    def oracle_call(self, icall, n, prev_call=None, prep=None, feed_n=None, zero_ghost_velocities=False, tail_halo=True, last_inputs=None):
        """The oracle's chain of call `icall` with n subcycles.  Planted errors (tests/test_cgrid_call_chain_cpu.py): feed_n: the
        stages after the loop are fed the state of feed_n subcycles; zero_ghost_velocities: ... the final face velocities with their
        ghost cells zeroed; tail_halo=False: strintxE / strintyN without their halo update."""
        prep = prep if prep is not None else self.oracle_prep(icall, prev_call, last_inputs=last_inputs)
        masks = {k: prep[k] for k in oracle.C_MASKS}
        inputs = {k: prep[k] for k in oracle.C_INPUTS}
        inputs["strength"] = self.strength(icall, masks)
        if self.seabed:
            t = self.calls[icall - 1]["t"]
            for loc in "EN":
                inputs["Tb" + loc] = oracle.seabed_lkd_c(self.dom, loc, 7.5, 15.0, 20.0, 30.0, t["aice"], t["vice"], self.hwater, masks[f"ice{loc}mask"])
            prep = dict(prep, TbE=inputs["TbE"], TbN=inputs["TbN"])
        state = {k: prep[k] for k in oracle.C_FIELDS[:14]}
        run = lambda m: oracle.cgrid_subcycle(self.dom, self.prm, m, state, inputs, self.static, masks, visc_method=self.visc)
        loop = run(n)
        fed = loop if feed_n is None else run(feed_n)
        if zero_ghost_velocities:
            inn = interior(self.dom.shape, self.blocks)
            fed = dict(fed, **{k: np.where(inn, fed[k], 0.0) for k in ("uvelE", "vvelE", "uvelN", "vvelN", "uvel", "vvel")})
        out = oracle_post(self.dom, self.prm, self.blocks, self.static, self.tarear, float(self.scal["e_factor"]), fed, inputs, masks,
                          self.uin(icall, masks), tail_halo=tail_halo)
        out.update(loop=loop, prep=prep, masks=masks, inputs=inputs)
        if feed_n is None and not zero_ghost_velocities:
            out["final"] = dict(loop, strintxE=out["tail"]["strintxE"], strintyN=out["tail"]["strintyN"])
        return out

    @functools.lru_cache(maxsize=None)
    def chain(self):
        """The oracle's chain of the calls of PAIRS on one core, [(call 1, call 2), ...]: call 1 of every pair from the state handed
        in, call 2 from what call 1 left (computed once; nobody writes into it)."""
        out, last = [], None
        for n1, n2 in PAIRS:
            a = self.oracle_call(1, n1, last_inputs=last)
            b = self.oracle_call(2, n2, prev_call=a)
            out.append((a, b))
            last = b["inputs"]
        return out

    def gains_and_losses(self, icall, prep, prev_masks):
        for k in ("iceEmask", "iceNmask") + (("iceTmask", "iceUmask") if "iceTmask" in prev_masks else ()):
            new, old = prep[k] != 0, prev_masks[k] != 0
            assert (new & ~old).any() and (old & ~new).any(), f"call {icall}: no face gains / loses ice ({k}, {self.name})"

    def top_rows_move(self, before, after):
        """the ice moves on the top three rows of the blocks at the fold"""
        for b in self.dc.local_blocks(0):
            if b.gj0 + b.gny - 1 != self.dc.ny_global:
                continue
            rows = slice(b.jhi - 3, b.jhi)
            for k in ("uvelE", "vvelN"):
                assert np.abs(after[k][b.local, rows, b.ilo - 1:b.ihi] - before[k][b.local, rows, b.ilo - 1:b.ihi]).max() > 0, (k, b.local)


def run_synth_call(core, case: SynthCg, icall, n, path, want, seen: Seen, prev_masks=None, reference=None):
    """Call `icall` of the case on `core` against the oracle's chain `want` (SynthCg.oracle_call): cgrid_prep with the state handed
    in on call 1 and None on call 2 (prev_masks: the masks call 1 returned).  reference: on tripoleT the loop stage is ALSO compared with the five-phase schedule's
    download of the same call (a dict of C_FIELDS)."""
    what = f"{case.name} call {icall} ndte {n} on {path}"
    call = case.calls[icall - 1]
    prev_masks = call["prev"] if icall == 1 else prev_masks
    before = core.cgrid_timings()["in_alt"]
    masks = core.cgrid_prep(evp.PrepParams(**PPD, ssh_stress_coupled=0), call["t"], case.state if icall == 1 else None, prev_masks)
    if case.seabed:
        core.cgrid_set_tb(want["inputs"]["TbE"], want["inputs"]["TbN"])
    core.cgrid_prep_finish(case.strength(icall, want["masks"]), case.visc)
    for k in oracle.C_MASKS:
        assert bits_equal(masks[k] != 0, want["masks"][k] != 0), f"prep: {what}: {k}"
    case.gains_and_losses(icall, want["prep"], prev_masks)
    assert_bitwise({k: core.cgrid_fetch(k) for k in PREP_KEYS}, {k: want["prep"][k] for k in PREP_KEYS}, f"prep: {what}")
    core.cgrid_subcycle(n)
    seen.add(assert_cg_path_ran(core, path, n, True, f"loop: {what}", before))
    out = core.cgrid_download()
    if reference is not None:
        assert_bitwise(out, reference, f"loop + download: {what} (against the five phases)")
    assert_bitwise(out, want["loop"], f"loop + download: {what}")
    run_post(core, want, case.tarear, case.uin(icall, want["masks"]), what)
    return out, {k: masks[k] for k in ("iceUmask", "iceEmask", "iceNmask")}


# name -> (tag the rows ask for, kind, nx, ny, blocks, seed, land, visc, seabed): the smallest shapes at which each schedule still
# forms; the fixture-sized schedules on a gx3- / tx3-sized grid, so that every row has its second call with state = None
SYNTH = {
    "closed 100x116": ("closed1", "closed", 100, 116, (100, 116), 5, 0.0, "avg_zeta", False),
    "closed 100x116 avg_strength": ("closed1", "closed", 100, 116, (100, 116), 5, 0.0, "avg_strength", False),
    "closed 100x116 seabed": ("closed1", "closed", 100, 116, (100, 116), 5, 0.0, "avg_zeta", True),
    "closed 100x116 in 50x58": ("closedN", "closed", 100, 116, (50, 58), 5, 0.0, "avg_zeta", False),
    "strip 200x48": ("strip", "strip", 200, 48, (200, 48), 77, 0.02, "avg_zeta", False),
    "strip 260x72 in 140x40": ("strip", "strip", 260, 72, (140, 40), 78, 0.02, "avg_zeta", False),
    "strip 200x48 avg_strength": ("strip", "strip", 200, 48, (200, 48), 77, 0.02, "avg_strength", False),
    "fold 100x116": ("foldres", "fold", 100, 116, (100, 116), 47, 0.0, "avg_zeta", False),
    "fold 100x116 avg_strength": ("foldres", "fold", 100, 116, (100, 116), 47, 0.0, "avg_strength", False),
    "fold 200x64": ("fold", "fold", 200, 64, (200, 64), 41, 0.02, "avg_zeta", False),
    "fold 400x80 in 200x40": ("fold", "fold", 400, 80, (200, 40), 43, 0.0, "avg_zeta", False),
    "foldT 200x64": ("foldT", "foldT", 200, 64, (200, 64), 41, 0.02, "avg_zeta", False),
    "foldT 400x80 in 200x40": ("foldT", "foldT", 400, 80, (200, 40), 43, 0.0, "avg_zeta", False),
}


@functools.lru_cache(maxsize=None)
def synth_case(name):
    return SynthCg(*SYNTH[name][1:])


def synth_rows():
    """(case, row): every row that runs off the fixtures on every shape of its kind."""
    rows = []
    for path, r in CG_PATHS.items():
        for name, (tag, *_rest, visc, seabed) in SYNTH.items():
            if tag in r.grids and visc == r.visc and seabed == r.seabed:
                rows.append((name, path))
    return rows


# (call 1, call 2) counts on one core: both odd, then an even and an odd one from a fresh state -- with the first subcycle of a call
# in place an odd count swaps the four others an even number of times, so the second pair is what leaves them in their second
# allocations when call 2's cgrid_prep reads them
PAIRS = ((7, 9), (8, 7))



# ---- split subcycle calls: upload, subcycle(a), subcycle(b), then the calls after the loop -----------------------------------------
SPLITS = ((3, 4), (4, 3))       # (beside a fold the first subcycle of the first call runs in place: 3 + 4 swaps 2 + 4 times, 4 + 3 swaps 3 + 3 times)


class LoopCase(NamedTuple):
    """The loop's own inputs (cice_evp_hip_cgrid_upload) of a case and what the restatements need."""
    name: str
    open_core: object
    dom: object
    prm: object
    blocks: list
    static: dict
    tarear: object
    e_factor: float
    state: dict
    inputs: dict
    masks: dict
    visc: str


def split_case(path) -> LoopCase:
    """One case per row: the first fixture the row accepts, or -- off the fixtures -- the smallest grid of the row's kind with random,
    mutually independent holes in the four ice masks, which no preparation produces (test_gpu_cgrid.marched_case,
    test_gpu_cgrid_march_tripole.fold_case)."""
    r = CG_PATHS[path]
    if "fixture" in r.grids:
        c = GoldenCase(next(n for n, p in fixture_rows() if p == path))
        state, inputs, masks = c.cgrid_inputs(1)
        return LoopCase(c.name, lambda: fixture_core(c), c.oracle_domain(), c.oracle_params(), tail_ref.blocks_of(c), c.cgrid_static(),
                        c.d["tarear"], float(c.scal[4]), state, inputs, masks, str(c.d["visc_method"]))
    kind = r.grids[0]
    if kind == "closed1":
        from test_gpu_cgrid import synth_cgrid
        dc, _, static, state, inputs, masks = synth_cgrid("gx3", case="caps", seed=3)
        name = "gx3 one block, caps"
    elif kind == "strip":
        from test_gpu_cgrid import marched_case
        dc, _, static, state, inputs, masks = marched_case(77, 200, 48, (200, 48), "full", 0.2, 0.02, ew="cyclic", ns="cyclic")
        name = "200x48 cyclic, holes 0.2"
    else:
        from test_gpu_cgrid_march_tripole import fold_case
        dc, static, state, inputs, masks = fold_case(43, 400, 80, (200, 40), "full", 0.3, 0.0)
        name = "400x80 tripole in 200x40, holes 0.3"
        if kind == "foldT":
            dcT = decomp.Decomp(400, 80, 200, 40, "cyclic", "tripoleT", 1)
            domT = tail_ref.domain_of_decomp(dcT)
            for group, vec in ((static, ()), (state, synth.CGRID_VECTOR), (inputs, synth.CGRID_VECTOR), (masks, ())):
                for k in group:
                    b = np.ascontiguousarray(group[k], dtype=np.float64)
                    oracle.halo_update(domT, b, _loc(k), "vector" if k in vec else "scalar")
                    group[k] = b.astype(group[k].dtype)
            dc, name = dcT, "400x80 tripoleT in 200x40, holes 0.3"
    scal = synth.evp_scalars(120)
    prm = oracle.make_params(**{k: scal[k] for k in ("arlx1i", "denom1", "brlx", "revp", "e_factor", "epp2i", "capping", "Ktens",
                                                      "deltaminEVP", "u0", "cosw", "sinw", "rhow")})

    def open_core():
        d, keep = evp.make_dims(dc, 0)
        return new_core(d, keep, scal, static)
    return LoopCase(name, open_core, tail_ref.domain_of_decomp(dc), prm, tail_ref.blocks_of_decomp(dc), static,
                    np.where(static["tarea"] > 0, 1.0 / static["tarea"], 0.0), float(scal["e_factor"]), state, inputs, masks, r.visc)


def split_want(case: LoopCase, n, feed_n=None):
    """The oracle's chain from the loop's inputs: n subcycles, the stages after the loop fed their state (feed_n: another count's --
    the planted stale allocation)."""
    run = lambda m: oracle.cgrid_subcycle(case.dom, case.prm, m, case.state, case.inputs, case.static, case.masks, visc_method=case.visc)
    loop = run(n)
    uin = u_point_inputs(case.dom.shape, case.masks["iceUmask"], seed=23)
    out = oracle_post(case.dom, case.prm, case.blocks, case.static, case.tarear, case.e_factor, loop if feed_n is None else run(feed_n),
                      case.inputs, case.masks, uin)
    out["loop"] = loop
    return out, uin


def run_split_calls(core, case: LoopCase, path, seen: Seen, a, b):
    what = f"{case.name}: upload, subcycle({a}), subcycle({b}) on {path}"
    want, uin = split_want(case, a + b)
    before = core.cgrid_timings()["in_alt"]
    core.cgrid_upload(case.state, case.inputs, case.masks, visc_method=case.visc)
    core.cgrid_subcycle(a)
    mid = assert_cg_path_ran(core, path, a, True, f"loop: {what}: first call", before)
    seen.add(mid)
    core.cgrid_subcycle(b)
    seen.add(assert_cg_path_ran(core, path, b, False, f"loop: {what}: second call", mid))
    assert_bitwise(core.cgrid_download(), want["loop"], f"loop + download: {what}")
    run_post(core, want, case.tarear, uin, what)
    return want
