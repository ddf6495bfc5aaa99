"""GPU (-m gpu): the C-grid loop on tripole (u-fold) and tripoleT grids on one rank as "marched zone + fold band"
(cice_amd/csrc/evp_host_cgrid_loop.cpp: enqueue_march_fold) -- cg_strip on the rectangles under the fold band, list-driven variants of the
five phase kernels with the fold steps on every other interior cell.  Forced with CICE_EVP_HIP_CGRID_MARCH_FOLD=1 and the on-chip
resident kernel off; every array of cgrid_run compared as bits, ghost cells included: with the CPU oracle (u-fold), with the reference
itself through the prebuilt harness (tripoleT, and u-fold once more), with today's schedule (CICE_EVP_HIP_CGRID_ONE=0) and with the
serial order of the two sets.  Every case asserts that the schedule ran (marched_fold_subcycles, fold_band_rows, marched_items) and that
the ice moves on the top three rows: otherwise it would not exercise the fold.

Two limits of what is covered.  The synthetic tripole grid's dxE / dyN are not the reference's four-point means bit for bit, so the host
refuses to form the lengths there: the LEN instantiation runs in the reference-harness cases only (which skip where the harness is
absent), and the STRIP_LEN draw of the sweep's even seeds changes nothing.  The schedule has no edge windows (every cell outside the
rectangles belongs to the phase kernels), so the sweep has no edge-window shape to vary."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle
from cice_amd import decomp, evp, synth
from common import assert_bitwise
from test_gpu_cgrid import cgrid_core, reference_cgrid_case, stir_momentum

pytestmark = pytest.mark.gpu

SWITCHES = ("CICE_EVP_HIP_CGRID_MARCH_FOLD", "CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL", "CICE_EVP_HIP_CGRID_ONE", "CICE_EVP_HIP_CGRID_STRIP_SEG",
            "CICE_EVP_HIP_CGRID_STRIP_LEN", "CICE_EVP_HIP_CGRID_STRIP_LAST")


def fold_case(seed, nx, ny, bs, case, holes, land, general=False):
    """test_gpu_cgrid.marched_case on a tripole (u-fold) grid: the default configuration's geometry (the start-up identities hold) with
    random land cells inside the ocean and random, mutually independent holes in the four ice masks -- but ice kept on the top two rows
    and beside the pole columns, so that the fold step always has ice on both sides"""
    rng = np.random.default_rng(seed)
    g0 = synth.make_grid(nx, ny, 2.0e4, ns="tripole")
    keep = np.zeros((ny, nx), dtype=bool)
    keep[-2:, :] = True
    for c in (0, 1, nx // 2 - 2, nx // 2 - 1, nx // 2, nx // 2 + 1, nx - 2, nx - 1):
        keep[-8:, c] = True
    g0["kmt"] = g0["kmt"] * ((rng.random((ny, nx)) >= land) | keep)
    g = synth.derive_geometry(g0)
    cg = synth.cgrid_geometry(g)
    state, inputs, masks = synth.cgrid_state(g, cg, case=case, seed=seed, seabed=general)
    if general:
        stir_momentum(inputs, masks, rng)
    for k in masks:
        masks[k] = masks[k] * ((rng.random((ny, nx)) >= holes) | keep).astype(np.int32)
    for k in ("stresspT", "stressmT", "stress12T"):
        state[k] = state[k] * masks["iceTmask"]
    state["stress12U"] = state["stress12U"] * masks["iceUmask"]
    dc = decomp.Decomp(nx, ny, bs[0], bs[1], "cyclic", "tripole", 1)
    return (dc,) + synth.cgrid_scatter(dc, 0, cg, state, inputs, masks)


def oracle_run(dc, scal, ndte, static, state, inputs, masks, visc="avg_zeta"):
    blks = dc.local_blocks(0)
    dom = oracle.OracleDomain(dc.nx_block, dc.ny_block, len(blks), dc.nx_global, dc.ny_global, dc.ew, dc.ns,
                              [b.ilo for b in blks], [b.ihi for b in blks], [b.jlo for b in blks],
                              [b.jhi for b in blks], [b.gi0 for b in blks], [b.gj0 for b in blks])
    prm = oracle.make_params(**{k: scal[k] for k in ("arlx1i", "denom1", "brlx", "revp", "e_factor", "epp2i", "capping",
                                                      "Ktens", "deltaminEVP", "u0", "cosw", "sinw", "rhow")})
    return oracle.cgrid_subcycle(dom, prm, ndte, state, inputs, static, masks, visc_method=visc)


def hip_run(dc, scal, static, state, inputs, masks, calls, visc="avg_zeta"):
    """calls: one int = cgrid_run(ndte); a list = upload, subcycle(n) for each, download.  Returns the arrays, the timings after the
    first subcycle call, the schedule line"""
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(scal, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"],
                      1.0 / static["uarea"], static["tarea"], keepalive=keep)
    try:
        core.cgrid_set_geometry(static)
        if isinstance(calls, int):
            out = core.cgrid_run(calls, state, inputs, masks, visc_method=visc)
            tt = [core.cgrid_timings()]
        else:
            core.cgrid_upload(state, inputs, masks, visc_method=visc)
            tt = []
            for n in calls:
                core.cgrid_subcycle(n)
                tt.append(core.cgrid_timings())
            out = core.cgrid_download()
        return out, tt, core.describe_path()
    finally:
        core.finalize()


def top_rows_move(dc, before, after):
    """the ice moves on the top three rows of the blocks at the fold"""
    for b in dc.local_blocks(0):
        if b.gj0 + b.gny - 1 != dc.ny_global:
            continue
        rows = slice(b.jhi - 3, b.jhi)
        for k in ("uvelE", "vvelN"):
            assert np.abs(after[k][b.local, rows, b.ilo - 1:b.ihi] - before[k][b.local, rows, b.ilo - 1:b.ihi]).max() > 0, (k, b.local)


def assert_ran(tt, ndte, first=True, strip_last=True):
    # (CICE_EVP_HIP_CGRID_STRIP_LAST=0 takes the call's last subcycle out of the schedule: the counter says what ran in it)
    assert tt["marched_fold_subcycles"] == ndte - (1 if first else 0) - (0 if strip_last else 1), tt
    assert tt["fold_band_rows"] > 0 and tt["marched_items"] > 0 and tt["fold_rest_cells"] > 0 and tt["marched_cells"] > 0, tt
    assert tt["resident_subcycles"] == 0 and tt["one_launch_subcycles"] == 0, tt


def force(monkeypatch, **env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_RESIDENT", "0")
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_MARCH_FOLD", "1")
    for k, v in env.items():
        monkeypatch.setenv("CICE_EVP_HIP_CGRID_" + k, v)


# seed, nx, ny, block size, ice cover, holes, land, revised EVP, general momentum step, ndte, switches
ORACLE_CASES = [
    (41, 200, 64, (200, 64), "full", 0.2, 0.02, False, False, 9, {}),                               # one block, default segments, LEN on
    (42, 100, 116, (100, 116), "caps", 0.1, 0.05, True, False, 8, {"STRIP_SEG": "5", "STRIP_LEN": "0"}),   # tx3: a rectangle narrower than a strip
    (43, 400, 80, (200, 40), "full", 0.3, 0.0, False, False, 7, {"STRIP_SEG": "1"}),                # 2 x 2 blocks: only the upper ones have a band
    (44, 260, 72, (140, 40), "caps", 0.1, 0.02, True, True, 8, {}),                                 # padded blocks; revised EVP, general momentum step
    (45, 200, 64, (200, 64), "full", 0.0, 0.03, False, True, 7, {"STRIP_SEG": "5", "STRIP_LAST": "0"}),   # full cover; the last subcycle without LAST
]


@pytest.mark.parametrize("seed,nx,ny,bs,case,holes,land,revised,general,ndte,env", ORACLE_CASES)
def test_cgrid_march_fold_vs_oracle_and_todays_schedule(seed, nx, ny, bs, case, holes, land, revised, general, ndte, env, monkeypatch):
    dc, static, state, inputs, masks = fold_case(seed, nx, ny, bs, case, holes, land, general=general)
    scal = synth.evp_scalars(120, **(dict(revised_evp=True, arlx=300.0, brlx=300.0) if revised else {}))
    if general:
        scal.update(cosw=np.cos(0.4), sinw=np.sin(0.4))
    want = oracle_run(dc, scal, ndte, static, state, inputs, masks)
    top_rows_move(dc, state, want)
    force(monkeypatch, **env)
    strip_last = env.get("STRIP_LAST") != "0"
    got, tt, path = hip_run(dc, scal, static, state, inputs, masks, ndte)
    assert_ran(tt[0], ndte, strip_last=strip_last)
    # (the synthetic tripole grid's dxE, dyN are not the reference's four-point means bit for bit: the host's check refuses, all eight
    # lengths stay loaded; the reference-made grids below have them formed)
    assert not tt[0]["marched_lengths_derived"], tt
    assert f"marched zone + fold band, {tt[0]['fold_band_rows']} rows" in path, path
    assert_bitwise(got, want, f"marched zone + fold band vs the oracle, seed {seed}")
    # the serial order of the two sets
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL", "1")
    ser, ts, _ = hip_run(dc, scal, static, state, inputs, masks, ndte)
    assert_ran(ts[0], ndte, strip_last=strip_last)
    assert_bitwise(ser, got, f"serial order vs concurrent, seed {seed}")
    # today's schedule: five full-domain phases + fold steps
    monkeypatch.delenv("CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL")
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_ONE", "0")
    old, to, path0 = hip_run(dc, scal, static, state, inputs, masks, ndte)
    assert to[0]["marched_fold_subcycles"] == 0 and "marched zone" not in path0, (to, path0)
    assert_bitwise(got, old, f"marched zone + fold band vs five phases, seed {seed}")


REF_CASES = [
    ("tripoleT", 200, 64, (200, 64), {}),
    ("tripoleT", 260, 72, (130, 36), {}),                  # cut in both directions
    ("tripole", 200, 64, (100, 32), {}),
    ("tripoleT", 200, 64, (200, 64), {"h_seabed": True}),
]


@pytest.mark.parametrize("ns,nx,ny,bs,kw", REF_CASES)
def test_cgrid_march_fold_vs_reference(ns, nx, ny, bs, kw, tmp_path, monkeypatch):
    """against the reference itself (unmodified sources, strict build, run here on the box): two calls with an evolving state, 1 and
    7 subcycles each"""
    c = reference_cgrid_case(tmp_path, nx, ny, bs, "cyclic", ns, icecase="full", nsub_list=[1, 7], ncalls=2, h_ndte=7, h_evolve=True, **kw)
    dom = c.oracle_domain()
    force(monkeypatch)
    core = cgrid_core(c)
    try:
        for icall in range(1, c.ncalls + 1):
            state, inputs, masks = c.cgrid_inputs(icall)
            for nsub in c.nsub_list:
                out = core.cgrid_run(nsub, state, inputs, masks, visc_method=str(c.d["visc_method"]))
                assert_ran(core.cgrid_timings(), nsub)
                assert core.cgrid_timings()["marched_lengths_derived"], "the reference's own lengths: formed in the kernel"
                oracle.halo_update(dom, out["strintxE"], "Eface", "vector")
                oracle.halo_update(dom, out["strintyN"], "Nface", "vector")
                want = c.cgrid_expected(icall, nsub)
                assert_bitwise(out, want, f"{ns} {nx}x{ny} blocks {bs}: call {icall} nsub {nsub} vs the reference")
        assert "marched zone + fold band" in core.describe_path()
        top_rows_move(decomp.Decomp(nx, ny, bs[0], bs[1], "cyclic", ns, 1), state, want)
    finally:
        core.finalize()


def test_cgrid_march_fold_across_calls(monkeypatch):
    """upload, subcycle(5), subcycle(1), subcycle(6), download = one call of 12: the later calls run every subcycle in the schedule"""
    dc, static, state, inputs, masks = fold_case(51, 200, 64, (200, 64), "full", 0.2, 0.02)
    scal = synth.evp_scalars(120)
    want = oracle_run(dc, scal, 12, static, state, inputs, masks)
    top_rows_move(dc, state, want)
    force(monkeypatch)
    one, t1, _ = hip_run(dc, scal, static, state, inputs, masks, 12)
    assert_ran(t1[0], 12)
    got, tt, _ = hip_run(dc, scal, static, state, inputs, masks, [5, 1, 6])
    assert_ran(tt[0], 5)
    assert_ran(tt[1], 1, first=False)
    assert_ran(tt[2], 6, first=False)
    assert_bitwise(one, want, "one call of 12 vs the oracle")
    assert_bitwise(got, one, "5 + 1 + 6 subcycles vs one call of 12")


@pytest.mark.parametrize("what", ["avg_strength", "no room for a zone"])
def test_cgrid_march_fold_stays_off_with_the_reason(what, monkeypatch):
    """what the schedule does not serve keeps today's, bit-identical to the oracle, and cgrid_schedule() says why"""
    ny = 10 if what == "no room for a zone" else 64
    visc = "avg_strength" if what == "avg_strength" else "avg_zeta"
    dc, static, state, inputs, masks = fold_case(61, 200, ny, (200, ny), "full", 0.2, 0.02)
    scal = synth.evp_scalars(120)
    want = oracle_run(dc, scal, 7, static, state, inputs, masks, visc=visc)
    force(monkeypatch)
    got, tt, path = hip_run(dc, scal, static, state, inputs, masks, 7, visc=visc)
    assert tt[0]["marched_fold_subcycles"] == 0, tt
    assert "marched zone + fold band not in use" in path, path
    assert ("visc_method = avg_strength" if what == "avg_strength" else "no rectangle") in path, path
    assert_bitwise(got, want, f"stays off ({what}) vs the oracle")


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def test_cgrid_march_fold_stays_off_on_two_ranks():
    """tx1 cut in y over two ranks (two processes on the one GPU, tools/mailbox_2proc.py --cgrid) with the switch set: both ranks keep
    the five phases, say why, and their arrays -- the ghost row beyond the fold included -- equal the one-rank run of the same state
    bit for bit (which runs the schedule, and is held against the oracle above)"""
    root = Path(__file__).resolve().parents[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(root / "tools" / "mailbox_2proc.py"), "--cgrid", "--fold-ghosts",
           "--workload", "tx1", "--shape", "1x2", "--ndte", "8"]
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000", CICE_EVP_HIP_CGRID_MARCH_FOLD="1", CICE_EVP_HIP_CGRID_RESIDENT="0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "MAILBOX_2PROC OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count("marched zone + fold band not in use: several ranks") == 2, r.stdout[-2000:]


def test_cgrid_march_fold_after_a_call_of_the_resident_kernel(monkeypatch):
    """the on-chip resident kernel keeps precedence call by call: upload, subcycle(10) inside it, subcycle(2) -- too few for it -- as
    marched zone + fold band, whose second buffers nobody has brought into line since the upload.  tx1, against one call of 12."""
    from test_gpu_cgrid import synth_cgrid
    dc, g, static, state, inputs, masks = synth_cgrid("tx1", case="caps")
    scal = synth.evp_scalars(120)
    want = oracle_run(dc, scal, 12, static, state, inputs, masks)
    top_rows_move(dc, state, want)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.delenv("CICE_EVP_HIP_CGRID_RESIDENT", raising=False)
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_MARCH_FOLD", "1")
    got, tt, _ = hip_run(dc, scal, static, state, inputs, masks, [10, 2])
    assert tt[0]["resident_subcycles"] == 9 and tt[0]["marched_fold_subcycles"] == 0, tt[0]
    assert tt[1]["resident_subcycles"] == 0 and tt[1]["marched_fold_subcycles"] == 2 and tt[1]["marched_items"] > 0, tt[1]
    assert_bitwise(got, want, "resident call, then marched zone + fold band, vs the oracle")


def test_cgrid_march_fold_is_the_default_on_a_large_grid(monkeypatch):
    """1800 x 240 tripole in one block -- above cg_strip's size rule of 300 000 cells with its zone -- and nothing forced but the
    resident kernel off: the schedule is chosen by the size rule (it beat five phases in every run on 3600 x 2400,
    profiles/r09_cgrid_march_tripole.txt) and gives the bits of CICE_EVP_HIP_CGRID_ONE=0; a grid below the rule keeps five phases"""
    dc, static, state, inputs, masks = fold_case(71, 1800, 240, (1800, 240), "full", 0.0, 0.0)
    scal = synth.evp_scalars(120)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_RESIDENT", "0")
    got, tt, path = hip_run(dc, scal, static, state, inputs, masks, 4)
    assert_ran(tt[0], 4)
    assert tt[0]["marched_cells"] >= 300000 and 2 * tt[0]["marched_cells"] >= 1800 * 240 and "marched zone + fold band" in path, (tt, path)
    top_rows_move(dc, state, got)
    monkeypatch.setenv("CICE_EVP_HIP_CGRID_ONE", "0")
    old, to, _ = hip_run(dc, scal, static, state, inputs, masks, 4)
    assert to[0]["marched_fold_subcycles"] == 0, to
    assert_bitwise(got, old, "1800x240 by the size rule vs CICE_EVP_HIP_CGRID_ONE=0")
    monkeypatch.delenv("CICE_EVP_HIP_CGRID_ONE")
    small = fold_case(72, 200, 64, (200, 64), "full", 0.0, 0.0)
    _, ts, ps = hip_run(small[0], scal, *small[1:], 4)
    assert ts[0]["marched_fold_subcycles"] == 0 and ts[0]["fold_band_rows"] == 0 and "marched zone" not in ps, (ts, ps)


@pytest.mark.parametrize("seed", [4101, 4102, 4103, 4104] + [int(s) for s in os.environ.get("CGRID_MARCH_FOLD_SWEEP_SEEDS", "").split() if s])
def test_cgrid_march_fold_random_cuts(seed, tmp_path, monkeypatch):
    """everything that shapes the plan, seeded: size, cut, fold kind (odd seeds: tripoleT through the reference harness; even seeds:
    u-fold against the oracle), segment length, lengths formed or loaded, ice cover"""
    rng = np.random.default_rng(seed)
    nx, ny = 2 * int(rng.integers(65, 160)), int(rng.integers(40, 100))
    nbx, nby = (int(rng.integers(1, 3)) if nx >= 260 else 1), (int(rng.integers(1, 3)) if ny >= 70 else 1)
    bs = (-(-nx // nbx), -(-ny // nby))
    env = {"STRIP_SEG": str(int(rng.integers(1, 12))), "STRIP_LEN": str(int(rng.integers(0, 2)))}
    case = str(rng.choice(["full", "caps"]))
    what = f"seed {seed}: {nx}x{ny} blocks {bs} {env} {case}"
    force(monkeypatch, **env)
    if seed % 2:
        c = reference_cgrid_case(tmp_path, nx, ny, bs, "cyclic", "tripoleT", icecase="full", nsub_list=[7], ncalls=1, h_ndte=7)
        state, inputs, masks = c.cgrid_inputs(1)
        core = cgrid_core(c)
        try:
            out = core.cgrid_run(7, state, inputs, masks, visc_method=str(c.d["visc_method"]))
            tt = core.cgrid_timings()
        finally:
            core.finalize()
        dom = c.oracle_domain()
        oracle.halo_update(dom, out["strintxE"], "Eface", "vector")
        oracle.halo_update(dom, out["strintyN"], "Nface", "vector")
        assert_ran(tt, 7)
        assert_bitwise(out, c.cgrid_expected(1, 7), what)
    else:
        dc, static, state, inputs, masks = fold_case(seed, nx, ny, bs, case, float(rng.uniform(0.0, 0.4)), float(rng.uniform(0.0, 0.05)))
        scal = synth.evp_scalars(120)
        want = oracle_run(dc, scal, 7, static, state, inputs, masks)
        top_rows_move(dc, state, want)
        got, tt, _ = hip_run(dc, scal, static, state, inputs, masks, 7)
        assert_ran(tt[0], 7)
        assert_bitwise(got, want, what)
    print(f"MARCH_FOLD_SWEEP {what}: items {tt['marched_items'] if isinstance(tt, dict) else tt[0]['marched_items']}")
