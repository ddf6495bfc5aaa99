"""CPU: which instantiation of the resident B-grid kernel a launch runs (cice_amd/csrc/res2_variant.cpp: res2_choose, read through the
test build's cice_evp_hip_debug_res2_choose) against the rules restated in numpy, over the full cross product of the boolean
facts; and the table of built instantiations (cice_amd/csrc/evp_resident2.hip, cice_evp_hip_debug_res2_built).

The rules:
  COOP  wanted (RES_COOP), possible for the tables, 16 x 16 tiles, no neighbours on other GPUs (and no rimg table), built, fitting
        the chip.  It excludes lean.
  lean  cap 3, 16 x 16 tiles, no rimg table, one block, none of seam / T-fold / img3 / rraw / nlate (= COOP), revp == 0, both
        WATER_IS_OCN and TBU_ZERO, RES_LEAN not 0
  RIMU  lean, RES_RIMU not 0, valid rim-wave tables, none of the hooks 32, 256, 512
The variant's strict, cap and logw are the launch's; its remote is "the launch carries the rimg table"; rim_plan's tables are
bound exactly where RIMU runs."""
import ctypes as C

import numpy as np

from cice_amd import evp

FACTS = ["strict", "remote", "one_block", "seam", "tfold", "img3", "rimg", "rraw", "revp_zero", "water_is_ocn", "tbu_zero",
         "coop_ok", "coop_built", "coop_fits", "rimu_ok", "want_coop", "want_lean", "want_rimu"]       # bit k of a case
CAPS, LOGWS = (3, 1, 0, -1), (4, 5, 6)
ALL_HOOKS = 1 | 2 | 4 | 8 | 16 | 32 | 64 | 256 | 512 | 1024 | 2048 | 4096 | 8192 | 16384
BARS_RIMU = 32 | 256 | 512
# every (cap, logw) without hooks; where RIMU can run, each hook that bars it alone, and all the others together
SETTINGS = [(cap, logw, 0) for cap in CAPS for logw in LOGWS] + [(3, 4, h) for h in (32, 256, 512, ALL_HOOKS & ~BARS_RIMU)]


def _built(lib, strict, cap, logw, remote, coop, lean, rimu):
    return bool(lib.cice_evp_hip_debug_res2_built(int(strict), cap, logw, int(remote), int(coop), int(lean), int(rimu)))


def test_table_of_built_variants():
    """The test build: 48 general kernels, lean and lean + RIMU for strict / fused, one COOP kernel -- and nothing else."""
    lib = evp.load_library(testing=True)
    got, want = set(), set()
    for strict in (False, True):
        for cap in (3, 2, 1, 0, -1, -2):
            for logw in (3, 4, 5, 6, 7):
                for remote in (False, True):
                    for coop, lean, rimu in np.ndindex(2, 2, 2):
                        v = (strict, cap, logw, remote, bool(coop), bool(lean), bool(rimu))
                        if _built(lib, *v):
                            got.add(v)
                        base = cap == 3 and logw == 4 and not remote
                        if cap in CAPS and logw in LOGWS and (
                                (not coop and not lean and not rimu) or (base and lean and not coop) or
                                (base and strict and coop and not lean and not rimu)):
                            want.add(v)
    assert got == want
    assert len(got) == 48 + 2 + 2 + 1


def test_chooser_against_the_rules():
    lib = evp.load_library(testing=True)
    n = 1 << len(FACTS)
    case = np.arange(n, dtype=np.uint32)
    f = {name: (case >> k & 1).astype(bool) for k, name in enumerate(FACTS)}
    chosen = np.empty(n, np.uint32)
    returned = set()
    for cap, logw, hooks in SETTINGS:
        rc = lib.cice_evp_hip_debug_res2_choose(C.c_int64(n), case.ctypes.data_as(C.POINTER(C.c_uint32)), cap, logw, hooks,
                                                chosen.ctypes.data_as(C.POINTER(C.c_uint32)))
        assert rc == 0
        tile16 = (logw == 4) & ~f["rimg"]
        coop = f["want_coop"] & f["coop_ok"] & tile16 & ~f["remote"] & f["coop_built"] & f["coop_fits"]
        lean = (~coop & f["want_lean"] & (cap == 3) & tile16 & f["one_block"] & ~f["seam"] & ~f["tfold"] & ~f["img3"] & ~f["rraw"] &
                f["revp_zero"] & f["water_is_ocn"] & f["tbu_zero"])
        rimu = lean & f["want_rimu"] & f["rimu_ok"] & ((hooks & BARS_RIMU) == 0)
        want = (f["strict"].astype(np.uint32) | f["rimg"].astype(np.uint32) << 1 | coop.astype(np.uint32) << 2 |
                lean.astype(np.uint32) << 3 | rimu.astype(np.uint32) << 4 | rimu.astype(np.uint32) << 5 |
                np.uint32(logw << 8) | np.uint32((cap + 1) << 16))
        bad = np.flatnonzero(chosen != want)
        assert bad.size == 0, (cap, logw, hooks, {k: bool(v[bad[0]]) for k, v in f.items()}, hex(chosen[bad[0]]), hex(want[bad[0]]))
        # what the chooser can return where the fact "COOP is built" is the table's own answer, as the host states it
        table = np.zeros(n, bool)
        for strict in (False, True):
            for rimg in (False, True):
                table[(f["strict"] == strict) & (f["rimg"] == rimg)] = _built(lib, strict, cap, logw, rimg, True, False, False)
        returned |= {int(c) for c in np.unique(chosen[f["coop_built"] == table])}
    assert any(c >> 2 & 1 for c in returned) and any(c >> 4 & 1 for c in returned) and any((c >> 2 & 7) == 2 for c in returned)
    for c in returned:
        v = (c & 1, (c >> 16 & 0xFF) - 1, c >> 8 & 0xFF, c >> 1 & 1, c >> 2 & 1, c >> 3 & 1, c >> 4 & 1)
        assert _built(lib, *v), v
