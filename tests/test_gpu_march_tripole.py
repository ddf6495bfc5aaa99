"""GPU (-m gpu): the marching path on tripole (u-fold) and tripoleT grids on one rank (cice_amd/csrc/evp_host_march.cpp).  The fold
does not go into the marching kernel: global rows 1 .. NY - H (the zone) are marched in the strip-major rectangle, the top H rows
and the ghost row beyond the fold (the band) advance one subcycle per launch in the block layout with the tile kernel over a tile
list and the seam step; every ext + 4 subcycles the two trade the rows between them on the device (march_scatter / march_gather over
row windows).  Strict mode: bit for bit against the reference's fixtures and the CPU oracle; fused mode: bit for bit against the
one-subcycle kernel.  Forced on small grids as in test_gpu_march.py (CICE_EVP_HIP_MARCH=1, resident kernel off); every case
asserts that the path ran with a band -- without the feature march_info()["mode"] is 0 on every tripole grid."""
import numpy as np
import pytest

import oracle  # noqa: F401
from cice_amd import decomp, evp, synth
from common import GoldenCase, assert_bitwise, bits_equal, tfold_untouched
from test_gpu_parity import SIG, hip_from_case, post_evp, run_oracle

pytestmark = pytest.mark.gpu

TRIPOLE_FIXTURES = ["trip_cyc_2x2_full", "trip_cyc_1blk_patchy", "trip_cyc_4x3_caps", "tript_cyc_2x2_full", "tript_cyc_1blk_patchy"]
K_FULL = dict(zip(TRIPOLE_FIXTURES, (4, 3, 2, 3, 4)))       # the K at which a fixture also runs its 120-subcycle case (suite time)


@pytest.fixture
def march(monkeypatch):
    monkeypatch.setenv("CICE_EVP_HIP_MARCH", "1")
    monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "0")
    return monkeypatch


def npasses(ndte, k=4):
    q, rem = divmod(ndte, k)
    return q + (1 if rem >= 2 else 0)


def assert_band_ran(info, ndte=None, kpass=None):
    assert info["mode"] == 1 and info["declined"] == 0 and info["passes"] > 0 and info["band_rows"] > 0, info
    if ndte is not None and ndte >= 2:
        k = kpass or info["kpass"]
        assert info["last_call"] and info["band_subcycles"] == ndte - (ndte % k == 1), info


@pytest.mark.parametrize("kpass", [4, 3, 2])
@pytest.mark.parametrize("name", TRIPOLE_FIXTURES)
def test_march_tripole_golden_strict_bitwise(name, kpass, march):
    """The reference's tripole and tripoleT fixtures (28 x 20 in 2 x 2 blocks, 24 x 18 in one block, 32 x 24 in 4 x 3 blocks),
    every call and every subcycle count, four / three / two subcycles per pass, short segments; ext = 0 so that an 18-row grid
    has a zone (12 marched rows under a band of 6)."""
    march.setenv("CICE_EVP_HIP_MARCH_K", str(kpass))
    march.setenv("CICE_EVP_HIP_MARCH_SEG", "5")
    march.setenv("CICE_EVP_HIP_MARCH_EXT", "0")
    c = GoldenCase(name)
    keep = tfold_untouched(c) if c.ns == "tripoleT" else None
    core = hip_from_case(c, strict=True)
    marched = 0
    try:
        for icall in range(1, c.ncalls + 1):
            dyn, tm, um = c.inputs(icall)
            for nsub in c.nsub_list:
                if nsub >= 120 and kpass != K_FULL[name]:
                    continue
                marched += nsub >= 2
                out = core.run(dyn, tm, um, ndte=nsub)
                info = core.march_info()
                what = f"{name} call {icall} nsub {nsub} k {kpass} (march + fold band)"
                want = c.expected(icall, nsub)
                if c.ns == "tripoleT":
                    # (whole-evp() fixtures: the stresses of the top row and its ghost row are rewritten after the loop)
                    for k, w in want.items():
                        sel = keep if k in SIG else slice(None)
                        assert bits_equal(out[k][sel], w[sel]), f"{what}: {k}"
                else:
                    assert_bitwise(post_evp(c, out), want, what)
                if nsub >= 2:
                    assert_band_ran(info, nsub, kpass)
                    assert info["kpass"] == kpass, info
        info = core.march_info()
        assert info["mode"] == 1 and info["declined"] == 0 and info["band_rows"] > 0 and (info["passes"] > 0) == (marched > 0), info
        assert "fold band" in core.describe_path(), core.describe_path()
    finally:
        core.finalize()


def tripole_case(nx, ny, dx0, case, seed, bs=None, holes=0.0):
    """A synthetic tripole grid as bench.py sets it up (cyclic east-west, CICE's own dxhy / dyhx with the mirrored ghost row);
    holes > 0: random, mutually independent holes in both masks on the GLOBAL grid (ghost cells are images), with the ice kept on
    the two top rows and next to the two pole columns."""
    g = synth.derive_geometry(synth.make_grid(nx, ny, dx0, ns="tripole"))
    st = synth.make_state(g, case=case, seed=seed, warm=True)
    if holes:
        rng = np.random.default_rng(seed)
        keep = np.zeros((ny, nx), dtype=bool)
        keep[-2:, :] = True
        for col in (0, 1, nx // 2 - 2, nx // 2 - 1, nx // 2, nx // 2 + 1, nx - 2, nx - 1):
            keep[-8:, col] = True
        tmg = (st["iceTmask"] * ((rng.random((ny, nx)) > holes) | keep)).astype(np.int32)
        umg = (st["iceUmask"] * ((rng.random((ny, nx)) > holes) | keep)).astype(np.int32)
        for k in evp.FIELDS[:12]:
            st[k] = st[k] * tmg
        for k in ("uvel", "vvel", "uvel_init", "vvel_init"):
            st[k] = st[k] * umg
        st["iceTmask"], st["iceUmask"] = tmg, umg
    bs = bs or (nx, ny)
    dc = decomp.Decomp(nx, ny, bs[0], bs[1], "cyclic", "tripole", 1)
    geo = {k: dc.scatter(g[k], 0, fill=(1.0 if k != "uarear" else 0.0)) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")}
    fields = {k: dc.scatter(st[k], 0) for k in evp.FIELDS}
    tm = dc.scatter(st["iceTmask"], 0, fill=0)
    um = dc.scatter(st["iceUmask"], 0, fill=0)
    return dc, geo, fields, tm, um, synth.bgrid_fold_metrics(dc, 0, g)


def make_core(dc, geo, metrics, scal, strict=True):
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(scal, strict=strict), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"], geo["uarear"],
                      geo["tarea"], keepalive=keep)
    core.set_metrics(dxhy=metrics[0], dyhx=metrics[1])
    return core


def top_rows_move(dc, want):
    u = dc.gather({0: want["uvel"]})
    assert np.abs(u[-3:]).max() > 0, "no ice moves on the fold rows: the case does not exercise the fold"


@pytest.mark.parametrize("grid,case,bs,ext,ndte,seg,holes", [
    ("tx3", "full", None, 0, 14, 0, 0.0), ("tx3", "caps", (25, 29), 4, 33, 7, 0.0), ("tx3", "full", (50, 58), 8, 14, 16, 0.0),
    ("tx3", "full", (30, 40), 4, 14, 9, 0.0),                  # padded last blocks in both directions
    ("tx3", "full", None, 4, 33, 0, 0.4), ("tx3", "caps", (50, 58), 0, 14, 11, 0.7), ("tx3", "full", (25, 29), 8, 33, 0, 0.3),
    ("tx1", "full", None, 8, 14, 0, 0.0), ("tx1", "caps", (90, 60), 4, 33, 40, 0.0), ("tx1", "full", (100, 37), 0, 14, 0, 0.5)])
def test_march_tripole_synthetic_vs_oracle_strict_bitwise(grid, case, bs, ext, ndte, seg, holes, march):
    """tx3- and tx1-sized tripole grids against the CPU oracle: one block, blocks cut both ways, padded blocks; redundant rims of
    0 / 4 / 8 rows (the ring is exchanged every 4th / 8th / 12th subcycle); 14 subcycles = three passes of four and one of two,
    33 = one subcycle of the streaming kernel and eight passes; full cover, polar caps, random independent holes in both masks."""
    march.setenv("CICE_EVP_HIP_MARCH_EXT", str(ext))
    march.setenv("CICE_EVP_HIP_MARCH_K", "4")
    if seg:
        march.setenv("CICE_EVP_HIP_MARCH_SEG", str(seg))
    spec = synth.GRIDS[grid]
    dc, geo, fields, tm, um, metrics = tripole_case(spec["nx"], spec["ny"], spec["dx0"], case, seed=20260928, bs=bs, holes=holes)
    scal = synth.evp_scalars(120)
    core = make_core(dc, geo, metrics, scal)
    try:
        got = core.run(fields, tm, um, ndte=ndte)
        info = core.march_info()
        assert_band_ran(info, ndte, 4)
        assert info["passes"] == npasses(ndte, 4) and info["band_rows"] >= ext + 4, info
    finally:
        core.finalize()
    want = run_oracle(dc, geo, fields, tm, um, scal, ndte)
    top_rows_move(dc, want)
    assert_bitwise(got, want, f"{grid}/{case} blocks {bs} ext {ext} ndte {ndte} holes {holes}: march + fold band vs oracle")


@pytest.mark.parametrize("variant", ["revised", "seabed", "capping"])
def test_march_tripole_non_lean_variants_vs_oracle(variant, march):
    """Revised EVP, seabed stress and fractional capping on tx3: the marching kernel's general variants beside the band's."""
    march.setenv("CICE_EVP_HIP_MARCH_EXT", "4")
    kw = dict(revised=dict(revised_evp=True, arlx=280.0, brlx=310.0), seabed={}, capping=dict(capping=0.4, Ktens=0.2))[variant]
    scal = synth.evp_scalars(120, **kw)
    spec = synth.GRIDS["tx3"]
    dc, geo, fields, tm, um, metrics = tripole_case(spec["nx"], spec["ny"], spec["dx0"], "full", seed=7, bs=(50, 58))
    fields = dict(fields)
    if variant == "seabed":
        tb = np.zeros_like(fields["TbU"])
        tb[:, tb.shape[1] // 3:, :] = 0.7          # the northern two thirds of every block: the band's rows among them
        fields["TbU"] = tb * um
    core = make_core(dc, geo, metrics, scal)
    try:
        got = core.run(fields, tm, um, ndte=14)
        assert_band_ran(core.march_info(), 14)
    finally:
        core.finalize()
    want = run_oracle(dc, geo, fields, tm, um, scal, 14)
    top_rows_move(dc, want)
    assert_bitwise(got, want, f"tx3 {variant}: march + fold band vs oracle")


def test_march_tripole_across_calls_and_stress_halo(march):
    """upload / subcycle(60) / subcycle(57) / subcycle(2) / subcycle(1) / download on a tripole fixture: 57 = 4 x 14 + 1 starts with
    one subcycle of the streaming kernel over the whole domain, 2 is one pass of two, 1 does not march at all; the block-layout
    state is complete after every call.  Then the stress symmetrisation on the device equals the streaming path's."""
    march.setenv("CICE_EVP_HIP_MARCH_K", "4")
    march.setenv("CICE_EVP_HIP_MARCH_EXT", "0")
    c = GoldenCase("trip_cyc_2x2_full")
    dyn, tm, um = c.inputs(1)
    res = {}
    for mode in ("1", "0"):
        march.setenv("CICE_EVP_HIP_MARCH", mode)
        core = hip_from_case(c, strict=True)
        try:
            core.upload(dyn, tm, um)
            for n in (60, 57, 2, 1):
                core.subcycle(n)
            core.sync()
            raw = core.download()
            if mode == "1":
                info = core.march_info()
                assert info["mode"] == 1 and info["declined"] == 0 and info["band_rows"] > 0, info
                assert info["passes"] == 15 + 14 + 1 and info["subcycles"] == 60 + 56 + 2, info
                assert_bitwise(post_evp(c, {k: v.copy() for k, v in raw.items()}), c.expected(1, 120), "march + band: upload/subcycle x4/download")
            core.stress_halo()
            core.sync()
            res[mode] = (raw, core.download())
        finally:
            core.finalize()
    assert_bitwise(res["1"][0], res["0"][0], "state after the four calls: march + band vs streaming")
    assert_bitwise(res["1"][1], res["0"][1], "after stress_halo(): march + band vs streaming")


def test_march_tripole_fused_mode_equals_streaming_fused(march):
    scal = synth.evp_scalars(120)
    spec = synth.GRIDS["tx3"]
    dc, geo, fields, tm, um, metrics = tripole_case(spec["nx"], spec["ny"], spec["dx0"], "full", seed=4, bs=(50, 58))
    out = {}
    for mode in ("1", "0"):
        march.setenv("CICE_EVP_HIP_MARCH", mode)
        core = make_core(dc, geo, metrics, scal, strict=False)
        try:
            out[mode] = core.run(fields, tm, um, ndte=20)
            if mode == "1":
                assert_band_ran(core.march_info(), 20)
            else:
                assert core.march_info()["mode"] == 0
        finally:
            core.finalize()
    assert_bitwise(out["1"], out["0"], "fused, tripole: march + fold band vs streaming")


def test_march_tripole_full_size_default_vs_oracle_bitwise(monkeypatch):
    """3600 x 2400 tripole, one block, nothing forced but the resident kernel off: the marching path is chosen by the size rule,
    with a band; 9 subcycles = one of the streaming kernel and two passes of four, against the CPU oracle on every cell."""
    monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "0")
    scal = synth.evp_scalars(480)
    dc, geo, fields, tm, um, metrics = tripole_case(3600, 2400, 1.1e4, "full", seed=2)
    want = run_oracle(dc, geo, fields, tm, um, scal, 9)
    core = make_core(dc, geo, metrics, scal)
    try:
        got = core.run(fields, tm, um, ndte=9)
        info = core.march_info()
        assert_band_ran(info, 9, 4)
        assert info["kpass"] == 4 and info["passes"] == 2 and info["subcycles"] == 8, info
        path = core.describe_path()
        assert "four subcycles per pass" in path and "marching path: on" in path and "fold band" in path, path
    finally:
        core.finalize()
    top_rows_move(dc, want)
    assert np.abs(want["uvel"]).max() > 1e-3
    assert_bitwise(got, want, "3600x2400 tripole: march + fold band vs oracle, 9 subcycles")


def test_march_stays_off_on_a_tripole_grid_of_two_ranks():
    """Several ranks: unchanged -- the plan of either rank refuses, with the reason."""
    dc = decomp.per_rank_blocks(360, 240, 2, "cyclic", "tripole", proc_shape=(2, 1))
    for rank in (0, 1):
        d, keep = evp.make_dims(dc, rank)
        with pytest.raises(evp.EvpHipError, match="tripole grid on several ranks"):
            evp.march_plan(d, ext=4)
        with pytest.raises(evp.EvpHipError, match="tripole grid on several ranks"):
            evp.march_fold_plan(d, 4, 5)
