"""GPU (-m gpu): device memory of the library is owned by registration (cice_amd/csrc/evp_host.h: DevicePool) and
cice_evp_hip_finalize releases all of it.  The test build counts what its pools hold (cice_evp_hip_debug_device_allocs: B-grid
state + marching path + C-grid state); here init -> run -> finalize runs twice in one process on every path of one rank, the count
is > 0 while the library is live and 0 after each finalize, it does not grow from the second call of an instance to the fifth, and
a change of ncat replaces the category arrays instead of adding to them.  Every cycle's output is compared with the reference's
committed fixture (or the CPU oracle), bit for bit where the library promises that -- never one cycle with the other.

What only several ranks allocate -- the mailbox and its tables, HIP-IPC mappings, the send / receive buffers of the halo and of the
marching path's ring -- is exercised functionally by the multiprocess files (tests/test_gpu_zz_*) and is not counted here."""
import numpy as np
import pytest

import oracle
from cice_amd import evp
from common import GoldenCase, assert_bitwise, bits_equal
from test_gpu_cgrid import cgrid_core
from test_gpu_parity import SIG, hip_from_case, post_evp
from test_gpu_seabed import (ALPHAB, PI, PPD, PUNY, bgrid_case, blocks_of, check_prob, family_of, planted_prob, spread)
from test_oracle_golden import check_prep_products
import seabed_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _testing_library(monkeypatch):
    """Every instance of this file lives in the test build: the count is that library's."""
    monkeypatch.setattr(evp, "testing_wanted", lambda: True)


class ResidentPrep:
    """On-chip resident kernel behind the device preparation: set_prep_geometry + prep, seabed_prob with two thickness categories,
    the loop, set_post_geometry + deformations / dyn_finish.  (The library takes the kernel by itself where its timing probe
    beats the streaming kernel's; asked for here, so that the path does not hang on a timing.)"""
    fixture = "pop_cyc_2x2_seabedprob"

    def __init__(self, monkeypatch):
        monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "1")
        self.c = c = GoldenCase(self.fixture)
        d = c.prep_scal_dict()
        self.pp = evp.PrepParams(**{k: v for k, v in d.items() if k not in ("cosw", "sinw", "ssh_coupled")}, ssh_stress_coupled=d["ssh_coupled"])

    def open(self):
        c = self.c
        core = hip_from_case(c, strict=True)
        st = c.prep_static()
        core.set_prep_geometry(st["tmask"], st["umask"], st["hm"], st["tarea"], st["uarea"], st["fcor_blk"])
        core.set_post_geometry(c.d["dxU"], c.d["dyU"], c.d["tarear"])
        return core

    def run(self, core, what):
        c, s = self.c, self.c.scal
        t, state = c.prep_inputs(1)
        dyn, tm_ref, um_ref = c.inputs(1)
        tm, um, _ = core.prep(self.pp, t, dict(state, TbU=dyn["TbU"]))
        out = {k: core.prep_fetch(k) for k in evp.PREP_FETCH}
        out.update(iceTmask=tm, iceUmask=um)
        out.update({k: v for k, v in core.download().items() if k in SIG})
        check_prep_products(c, 1, out, f"{what}: preparation")
        # two categories that share the cell's ice 3 : 2 / 1 : 1; exp() / log() are the device library's: the bound of
        # test_gpu_parity.py::test_seabed_stress_factor_on_device_probabilistic for this fixture's data
        aicen = np.stack([0.6 * t["aice"], 0.4 * t["aice"]], axis=1)
        vicen = np.stack([0.5 * t["vice"], 0.5 * t["vice"]], axis=1)
        core.seabed_prob(c.d["hwater"], aicen, vicen, s[26], s[17], s[19], s[30], s[31])
        tb = core.prep_fetch("TbU")
        ref = oracle.seabed_prob(c.oracle_domain(), s[26], s[17], s[12], s[19], s[30], s[31], aicen, vicen, c.d["hwater"], tm_ref, um_ref)
        assert np.abs(ref).max() > 0 and bits_equal(tb == 0, ref == 0), f"{what}: zero pattern of TbU"
        nz = ref != 0
        rel = float((np.abs(tb[nz] - ref[nz]) / np.abs(ref[nz])).max())
        print(f"\n{what}: TbU (ncat 2) from the oracle, relative: {rel:.2e}")
        assert rel <= 1e-12, f"{what}: TbU differs from the oracle by {rel:.2e} relative"
        # the rest of evp() with the reference's own factor: bit for bit
        core.set_tbu(dyn["TbU"])
        core.set_strength(dyn["strength"])
        core.subcycle(c.ndte)
        assert_bitwise(core.download(), c.expected(1, c.ndte), f"{what}: prep + loop")
        got = core.deformations()
        z = np.zeros(core.shape)
        got.update(core.dyn_finish(z, z))
        assert_bitwise(got, {k: c.d[f"o01n{c.ndte:04d}_{k}"] for k in got}, f"{what}: deformations / dyn_finish")
        tm_ = core.timings()
        assert tm_["resident_fallbacks"] == 0 and tm_["tile_variant"] >= 1000, tm_       # (>= 1000: the on-chip resident kernel ran)


class StreamingTripole:
    """One-subcycle kernel on a tripole fixture, with evp()'s stress symmetrisation on the device."""
    fixture = "trip_cyc_2x2_full"

    def __init__(self, monkeypatch):
        monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "0")
        monkeypatch.setenv("CICE_EVP_HIP_MARCH", "0")
        self.c = GoldenCase(self.fixture)

    def open(self):
        return hip_from_case(self.c, strict=True)

    def run(self, core, what):
        c = self.c
        dyn, tm, um = c.inputs(1)
        core.upload(dyn, tm, um)
        core.subcycle(c.ndte)
        core.stress_halo()
        assert_bitwise(core.download(), c.expected(1, c.ndte), f"{what}: loop + device stress halo")
        assert core.march_info()["mode"] != 1 and core.timings()["tile_variant"] < 1000, (core.march_info(), core.timings())


class March:
    """Marching path, forced on a small grid: a closed grid, and a tripole fixture (marched zone + fold band)."""

    def __init__(self, monkeypatch, fixture):
        monkeypatch.setenv("CICE_EVP_HIP_MARCH", "1")
        monkeypatch.setenv("CICE_EVP_HIP_RESIDENT", "0")
        monkeypatch.setenv("CICE_EVP_HIP_MARCH_SEG", "5")
        monkeypatch.setenv("CICE_EVP_HIP_MARCH_EXT", "0")       # (an 18-row tripole grid then has a zone under its band)
        self.c = GoldenCase(fixture)

    def open(self):
        return hip_from_case(self.c, strict=True)

    def run(self, core, what):
        c = self.c
        dyn, tm, um = c.inputs(1)
        out = core.run(dyn, tm, um, ndte=c.ndte)
        assert_bitwise(post_evp(c, out), c.expected(1, c.ndte), f"{what}: march")
        info = core.march_info()
        assert info["mode"] == 1 and info["last_call"] and info["declined"] == 0 and info["passes"] > 0, info
        assert (info["band_rows"] > 0) == (c.ns == "tripole"), info


class CGrid:
    fixture = "cgrid_trip_2x2_full"

    def __init__(self, monkeypatch):
        self.c = GoldenCase(self.fixture)
        self.dom = self.c.oracle_domain()

    def open(self):
        return cgrid_core(self.c)

    def run(self, core, what):
        c = self.c
        state, inputs, masks = c.cgrid_inputs(1)
        nsub = c.nsub_list[-1]
        out = core.cgrid_run(nsub, state, inputs, masks, visc_method=str(c.d["visc_method"]))
        oracle.halo_update(self.dom, out["strintxE"], "Eface", "vector")
        oracle.halo_update(self.dom, out["strintyN"], "Nface", "vector")
        assert_bitwise(out, c.cgrid_expected(1, nsub), f"{what}: C grid")


PATHS = {
    "resident_prep": ResidentPrep,
    "streaming_tripole": StreamingTripole,
    "march_closed": lambda mp: March(mp, "pop_cyc_3x2pad_caps"),
    "march_tripole": lambda mp: March(mp, "trip_cyc_1blk_patchy"),
    "cgrid": CGrid,
}


@pytest.mark.parametrize("path", list(PATHS))
def test_init_run_finalize_twice_releases_everything(path, monkeypatch):
    p = PATHS[path](monkeypatch)
    for cycle in (1, 2):
        core = p.open()
        try:
            p.run(core, f"{path} cycle {cycle}")
            held = evp.device_allocs()
            print(f"\n{path} cycle {cycle}: {held} device allocations while live")
            assert held > 0
        finally:
            core.finalize()
        assert evp.device_allocs() == 0, f"{path}: finalize of cycle {cycle} left device allocations registered"


@pytest.mark.parametrize("path", list(PATHS))
def test_calls_do_not_grow_the_device_memory(path, monkeypatch):
    """What a call allocates lazily it allocates once: the count after the fifth call equals the count after the second."""
    p = PATHS[path](monkeypatch)
    core = p.open()
    try:
        counts = []
        for call in range(1, 6):
            p.run(core, f"{path} call {call}")
            counts.append(evp.device_allocs())
        print(f"\n{path}: device allocations after calls 1 .. 5: {counts}")
        assert counts[1] > 0 and counts[4] == counts[1], counts
    finally:
        core.finalize()
    assert evp.device_allocs() == 0


def test_ncat_change_replaces_the_category_arrays():
    """seabed_prob with ncat 2 -> 3 -> 2 on one instance: aicen / vicen are released and allocated anew, nothing is added over the
    second change, and every result meets the accuracy rule of tests/test_gpu_seabed.py against tests/seabed_ref.py."""
    core, dc, dom, t, tm, um, scal = bgrid_case("gx3", (25, 29))
    try:
        blocks = blocks_of(dc)
        args = (ALPHAB, PPD["rhoi"], scal["rhow"], PPD["gravit"], PI, PUNY)
        counts = []
        for k, ncat in enumerate((2, 3, 2)):
            aicen, vicen, hwater, fam = planted_prob(dc, tm, ncat, seed=60 + k)
            core.seabed_prob(hwater, aicen, vicen, ALPHAB, PPD["rhoi"], PPD["gravit"], PI, PUNY)
            counts.append(evp.device_allocs())
            dev = core.prep_fetch("TbU")
            _, info = R.prob_t(blocks, aicen, vicen, hwater, tm, *args)
            ext, _ = R.prob_t(blocks, aicen, vicen, hwater, tm, *args, ext=True)
            want = oracle.seabed_prob(dom, *args, aicen, vicen, hwater, tm, um)
            near_t = info["ulp_to_xk"] <= 4.0
            assert set(np.unique(fam[near_t])) <= {R.PROB_FAMILIES.index("xk_edge")}, "a cell near a category edge by chance"
            assert np.abs(want).max() > 0
            check_prob(dev, want, R.neighbor_max(blocks, "U", ext, um), family_of(blocks, "U", ext, um, fam),
                       spread(blocks, "U", near_t) & (um != 0), f"ncat {ncat} (step {k}) TbU")
        print(f"\ndevice allocations after ncat 2, 3, 2: {counts}")
        assert counts[0] > 0 and counts[2] == counts[1] == counts[0], counts
    finally:
        core.finalize()
    assert evp.device_allocs() == 0
