"""GPU (-m gpu): visc_method = avg_strength on the marched split schedules of the C grid, which take it on request
(CICE_EVP_HIP_CGRID_MARCH_AVG_STRENGTH=1; cice_amd/csrc/cgrid_schedule.cpp: march_fold) -- here "marched zone + fold band" on tripole /
tripoleT grids on one rank: cg_strip<AVGS> on the rectangles under the fold band, the list-driven phase kernels on every other interior
cell, phase 2 forming the corner viscosity from strengthU and the corner's own deltaU (a zone corner's from the scratch copy phase 0
made).  Built like tests/test_gpu_cgrid_march_tripole.py, whose helpers it uses: forced with CICE_EVP_HIP_CGRID_MARCH_FOLD=1, the
on-chip resident kernel off, every array of cgrid_run compared as bits, ghost cells included -- with the CPU oracle (u-fold), with the
reference's own evp() through the prebuilt harness (tripoleT, and u-fold once more; these run the LEN instantiation), with the five-phase
schedule and with the serial order of the two sets.  Without the switch the same call keeps the five phases, says why, and gives the
same bits.

The masks have independent random holes; what only they show -- a corner WITHOUT ice must take the previous stress12U along into this
subcycle's buffer, on a rest corner and on a zone corner evaluated for a rest cell's sake -- is asserted to occur, from the plan's
cell flags and iceUmask."""
import numpy as np
import pytest

import oracle
from cice_amd import decomp, evp, synth
from common import assert_bitwise
from test_gpu_cgrid import cgrid_core, reference_cgrid_case
from test_gpu_cgrid_march_tripole import assert_ran, fold_case, force, hip_run, oracle_run, top_rows_move

pytestmark = pytest.mark.gpu

SWITCH = "CICE_EVP_HIP_CGRID_MARCH_AVG_STRENGTH"
VISC = "avg_strength"
REST, ZONE, U = 1, 8, 16          # EVP_CGS_* (cice_amd/csrc/evp_device.h)

# seed, nx, ny, block size, ice cover, holes, land, revised EVP, general momentum step (with a turning angle), ndte, switches
ORACLE_CASES = [
    (141, 200, 64, (200, 64), "full", 0.2, 0.02, False, False, 9, {}),                                   # one block
    (142, 100, 116, (100, 116), "caps", 0.1, 0.0, True, False, 8, {"STRIP_SEG": "5", "STRIP_LEN": "0"}),   # a rectangle narrower than a strip
    (143, 400, 80, (200, 40), "full", 0.3, 0.0, False, False, 7, {"STRIP_SEG": "1"}),                    # only the upper blocks have a band
    (144, 260, 72, (140, 40), "caps", 0.0, 0.0, True, True, 8, {}),                                      # padded blocks
    (145, 200, 64, (200, 64), "full", 0.0, 0.0, False, True, 7, {"STRIP_LAST": "0"}),                    # full cover; the last subcycle without LAST
]


def corners_without_ice(dc, masks, tt, env):
    """(zone corners without ice that phase 2 evaluates for a rest cell's sake, rest corners without ice), from the plan the host made:
    the planner's with the same knobs (the synthetic grid's lengths are not formed: lengths = 0), held against the run's counters"""
    d, keep = evp.make_dims(dc, 0)
    plan = evp.cgrid_march_fold_plan(d, seg=int(env.get("STRIP_SEG", 0)), lengths=0)
    assert plan["zone_cells"] == tt["marched_cells"] and plan["rest_cells"] == tt["fold_rest_cells"] and len(plan["items"]) == tt["marched_items"], (plan, tt)
    cells, noice = plan["cells"], np.asarray(masks["iceUmask"]) == 0
    assert cells.shape == noice.shape
    return int((((cells & ZONE) != 0) & ((cells & U) != 0) & noice).sum()), int((((cells & REST) != 0) & noice).sum())


@pytest.mark.parametrize("seed,nx,ny,bs,case,holes,land,revised,general,ndte,env", ORACLE_CASES)
def test_cgrid_march_fold_avg_strength_vs_oracle_and_five_phases(seed, nx, ny, bs, case, holes, land, revised, general, ndte, env, monkeypatch):
    dc, static, state, inputs, masks = fold_case(seed, nx, ny, bs, case, holes, land, general=general)
    scal = synth.evp_scalars(120, **(dict(revised_evp=True, arlx=300.0, brlx=300.0) if revised else {}))
    if general:
        scal.update(cosw=np.cos(0.4), sinw=np.sin(0.4))
    want = oracle_run(dc, scal, ndte, static, state, inputs, masks, visc=VISC)
    top_rows_move(dc, state, want)
    force(monkeypatch, **env)
    monkeypatch.setenv(SWITCH, "1")
    strip_last = env.get("STRIP_LAST") != "0"
    got, tt, path = hip_run(dc, scal, static, state, inputs, masks, ndte, visc=VISC)
    assert_ran(tt[0], ndte, strip_last=strip_last)
    assert f"marched zone + fold band, {tt[0]['fold_band_rows']} rows" in path and "avg_strength" in path, path
    assert_bitwise(got, want, f"avg_strength, marched zone + fold band vs the oracle, seed {seed}")
    nz, nr = corners_without_ice(dc, masks, tt[0], env)
    print(f"seed {seed}: {nz} zone corners without ice beside the rest, {nr} rest corners without ice")
    if holes > 0.0:
        assert nz > 0 and nr > 0, (seed, nz, nr)
    # the serial order of the two sets
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL", "1")
    ser, ts, _ = hip_run(dc, scal, static, state, inputs, masks, ndte, visc=VISC)
    assert_ran(ts[0], ndte, strip_last=strip_last)
    assert_bitwise(ser, got, f"avg_strength, serial order vs concurrent, seed {seed}")
    # the five full-domain phases + fold steps
    monkeypatch.delenv("CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL")
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_ONE", "0")
    old, to, path0 = hip_run(dc, scal, static, state, inputs, masks, ndte, visc=VISC)
    assert to[0]["marched_fold_subcycles"] == 0 and "marched zone" not in path0, (to, path0)
    assert_bitwise(got, old, f"avg_strength, marched zone + fold band vs five phases, seed {seed}")


REF_CASES = [
    ("tripoleT", 200, 64, (200, 64)),
    ("tripoleT", 260, 72, (130, 36)),                  # cut in both directions
    ("tripole", 200, 64, (100, 32)),
]


@pytest.mark.parametrize("ns,nx,ny,bs", REF_CASES)
def test_cgrid_march_fold_avg_strength_vs_reference(ns, nx, ny, bs, tmp_path, monkeypatch):
    """against the reference's own evp() with visc_method = 'avg_strength' (unmodified sources, strict build): two calls with an
    evolving state, 1 and 7 subcycles each; the reference's own lengths, so the marched kernel forms them (LEN under AVGS)"""
    c = reference_cgrid_case(tmp_path, nx, ny, bs, "cyclic", ns, icecase="full", nsub_list=[1, 7], ncalls=2, h_ndte=7, h_evolve=True,
                             h_visc_method=VISC)
    assert str(c.d["visc_method"]) == VISC
    dom = c.oracle_domain()
    force(monkeypatch)
    monkeypatch.setenv(SWITCH, "1")
    core = cgrid_core(c)
    try:
        for icall in range(1, c.ncalls + 1):
            state, inputs, masks = c.cgrid_inputs(icall)
            for nsub in c.nsub_list:
                out = core.cgrid_run(nsub, state, inputs, masks, visc_method=VISC)
                assert_ran(core.cgrid_timings(), nsub)
                assert core.cgrid_timings()["marched_lengths_derived"], "the reference's own lengths: formed in the kernel"
                oracle.halo_update(dom, out["strintxE"], "Eface", "vector")
                oracle.halo_update(dom, out["strintyN"], "Nface", "vector")
                want = c.cgrid_expected(icall, nsub)
                assert_bitwise(out, want, f"avg_strength {ns} {nx}x{ny} blocks {bs}: call {icall} nsub {nsub} vs the reference")
        path = core.describe_path()
        assert "marched zone + fold band" in path and "avg_strength" in path, path
        top_rows_move(decomp.Decomp(nx, ny, bs[0], bs[1], "cyclic", ns, 1), state, want)
    finally:
        core.finalize()


def test_cgrid_march_fold_avg_strength_across_calls(monkeypatch):
    """upload, subcycle(5), subcycle(1), subcycle(6), download = one call of 12 = the oracle: an odd and an even count of buffer swaps,
    and the later calls run every subcycle in the schedule"""
    dc, static, state, inputs, masks = fold_case(151, 200, 64, (200, 64), "full", 0.2, 0.02)
    scal = synth.evp_scalars(120)
    want = oracle_run(dc, scal, 12, static, state, inputs, masks, visc=VISC)
    top_rows_move(dc, state, want)
    force(monkeypatch)
    monkeypatch.setenv(SWITCH, "1")
    one, t1, _ = hip_run(dc, scal, static, state, inputs, masks, 12, visc=VISC)
    assert_ran(t1[0], 12)
    got, tt, _ = hip_run(dc, scal, static, state, inputs, masks, [5, 1, 6], visc=VISC)
    assert_ran(tt[0], 5)
    assert_ran(tt[1], 1, first=False)
    assert_ran(tt[2], 6, first=False)
    assert_bitwise(one, want, "avg_strength: one call of 12 vs the oracle")
    assert_bitwise(got, one, "avg_strength: 5 + 1 + 6 subcycles vs one call of 12")


@pytest.mark.parametrize("value", [None, "0"])
def test_cgrid_march_fold_avg_strength_stays_off_without_the_switch(value, monkeypatch):
    """the first oracle case's state with the switch unset (or 0): the five phases, the reason in the schedule line, and the bits of the
    schedule (which equal the oracle's)"""
    seed, nx, ny, bs, case, holes, land, revised, general, ndte, env = ORACLE_CASES[0]
    dc, static, state, inputs, masks = fold_case(seed, nx, ny, bs, case, holes, land)
    scal = synth.evp_scalars(120)
    force(monkeypatch)
    monkeypatch.setenv(SWITCH, "1")
    on, tt, path = hip_run(dc, scal, static, state, inputs, masks, ndte, visc=VISC)
    assert_ran(tt[0], ndte)
    if value is None:
        monkeypatch.delenv(SWITCH)
    else:
        monkeypatch.setenv(SWITCH, value)
    off, to, path0 = hip_run(dc, scal, static, state, inputs, masks, ndte, visc=VISC)
    assert to[0]["marched_fold_subcycles"] == 0, to
    assert "marched zone + fold band not in use: visc_method = avg_strength" in path0, path0
    assert_bitwise(off, on, "avg_strength: the switch unset vs set")

