"""CPU: the reference's own post-loop routines against their numpy restatement (tests/tail_ref.py).

oracle/_ref/evp_ref_harness_strict with `hiptail` dumps, after every reference evp() run, what the host computes next, made
by calling the reference's compiled routines: strocn{x,y}T_iavg (the quotient of general/ice_step_mod.F90:1017-1034 written in
the harness, then the reference's ice_HaloUpdate at the NE corner and its grid_average_X2Y('F', U -> T)), on the B grid
sig1 / sig2 / sigP of the reference's principal_stress (ice_dyn_shared.F90:1691), on the C grid the strintxU / strintyU that
evp() itself forms from the halo-updated strintxE / strintyN (ice_dyn_evp.F90:1437-1443).  These dumps are the expected side
of every assertion in tests/test_gpu_dropin_tail.py; here tail_ref's restatement is applied to the SAME run's dumped inputs
and must give the same bits, on every cell, ghost cells included.  Until this test the restatement was pinned on hand-worked
values only.  Skips when the harness is not built (it needs the reference tree)."""
import numpy as np
import pytest

import oracle
import run_ref
import tail_ref
from cice_amd import synth
from common import bits_equal

NDTE = 5
GRIDS = [
    # nx, ny, bx, by, ew, ns, icecase
    (40, 36, 20, 18, "cyclic", "closed", "full"),
    (72, 40, 36, 20, "cyclic", "tripole", "patchy"),
]
_cache = {}


def ref_run(tmp_path_factory, grid, grid_ice):
    """One harness run per (grid, staggering), shared by the tests below and left unchanged."""
    key = (grid, grid_ice)
    if key not in _cache:
        nx, ny, bx, by, ew, ns, icecase = grid
        tmp = tmp_path_factory.mktemp("tailref")
        g = synth.make_grid(nx, ny, dx0=1.1e5, ns=ns)
        run_ref.write_pop_grid(tmp / "grid.bin", g["ULAT"], g["ULON"], g["HTN"] * 100.0, g["HTE"] * 100.0)
        run_ref.write_kmt(tmp / "kmt.bin", g["kmt"])
        d, _ = run_ref.run_harness(nx, ny, bx, by, ew=ew, ns=ns, variant="strict", h_ndte=NDTE, ncalls=2, nsub_list=[1, NDTE],
                                   grid_kind=("tripolefile" if ns == "tripole" else "popfile"), icecase=icecase,
                                   h_grid_ice=grid_ice, hiptail=True, grid_files=(tmp / "grid.bin", tmp / "kmt.bin"))
        for a in d.values():
            a.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def blocks_of_dump(d):
    nb = int(d["dims"][2])
    return [tuple(int(v) for v in row[:4]) for row in np.asarray(d["blkinfo"]).reshape(nb, 8)]


def tags():
    return [f"o{icall:02d}n{nsub:04d}" for icall in (1, 2) for nsub in (1, NDTE)]


pytestmark = pytest.mark.skipif(not run_ref.harness_knows("strict", "hiptail"),
                                reason="oracle/_ref/evp_ref_harness_strict not built from this tree's harness (needs the reference tree)")


@pytest.mark.parametrize("grid_ice", ["B", "C"])
@pytest.mark.parametrize("grid", GRIDS, ids=["rect40x36", "tripole72x40"])
def test_strocn_t_restatement_equals_the_reference_routines(tmp_path_factory, grid, grid_ice):
    d = ref_run(tmp_path_factory, grid, grid_ice)
    dom = oracle.OracleDomain.from_dump(d, grid[4], grid[5])
    blocks = blocks_of_dump(d)
    for tag in tags():
        sx, sy, ai = d[f"{tag}_strocnxU"], d[f"{tag}_strocnyU"], d[f"{tag}_aiU"]
        want = tail_ref.strocn_t(dom, blocks, sx, sy, ai, d["uarea"], d["tarea"])
        for k in ("strocnxT_iavg", "strocnyT_iavg"):
            got = d[f"{tag}_{k}"]
            assert bits_equal(want[k], got), (f"{grid_ice} grid {tag} {k}: {int((want[k] != got).sum())} cells differ, "
                                              f"max|d|={np.abs(want[k] - got).max():.3e}")
            assert not (got == -7.e77).any()            # grid_average_X2Y writes every cell of the array
        # the case exercises the branch: ice-free U cells inside the domain, and a non-zero result
        on = np.zeros(ai.shape, dtype=bool)
        for b, (ilo, ihi, jlo, jhi) in enumerate(blocks):
            on[b, jlo - 1:jhi, ilo - 1:ihi] = True
        if grid[6] != "full":
            assert (ai[on] == 0.0).any() and (ai[on] != 0.0).any()
    assert np.abs(d[f"o02n{NDTE:04d}_strocnxT_iavg"]).max() > 0.0


@pytest.mark.parametrize("grid", GRIDS, ids=["rect40x36", "tripole72x40"])
def test_cgrid_strint_u_restatement_equals_the_reference_routines(tmp_path_factory, grid):
    d = ref_run(tmp_path_factory, grid, "C")
    dom = oracle.OracleDomain.from_dump(d, grid[4], grid[5])
    blocks = blocks_of_dump(d)
    static = {k: d[k] for k in ("earea", "epm", "narea", "npm")}
    for tag in tags():
        # evp()'s strintxE / strintyN are dumped after their halo update: the update applied again must leave them as they are
        # (on the fold the N-face row is the mean of a value and its own image), and E2US / N2US of them give strintxU / strintyU
        want = tail_ref.cgrid_tail(dom, blocks, d[f"{tag}_strintxE"], d[f"{tag}_strintyN"], static)
        for k in ("strintxE", "strintyN", "strintxU", "strintyU"):
            got = d[f"{tag}_{k}"]
            assert bits_equal(want[k], got), (f"{tag} {k}: {int((want[k] != got).sum())} cells differ, "
                                              f"max|d|={np.abs(want[k] - got).max():.3e}")
    assert np.abs(d[f"o02n{NDTE:04d}_strintxU"]).max() > 0.0 and np.abs(d[f"o02n{NDTE:04d}_strintyU"]).max() > 0.0


@pytest.mark.parametrize("grid", GRIDS, ids=["rect40x36", "tripole72x40"])
def test_principal_stress_restatement_equals_the_reference_routine(tmp_path_factory, grid):
    d = ref_run(tmp_path_factory, grid, "B")
    puny = float(d["scalars"][31])
    for tag in tags():
        want = tail_ref.principal_stress(d[f"{tag}_stressp_1"], d[f"{tag}_stressm_1"], d[f"{tag}_stress12_1"],
                                         d[f"{tag}_strength"], puny)
        for k in ("sig1", "sig2", "sigP"):
            got = d[f"{tag}_{k}"]
            assert bits_equal(want[k], got), (f"{tag} {k}: {int((want[k] != got).sum())} cells differ, "
                                              f"max|d|={np.abs(want[k] - got).max():.3e}")
            assert not (got == -7.e77).any()            # every cell of the block arrays, ghost cells included
        spv = d[f"{tag}_sig1"] == tail_ref.SPVAL_DBL
        assert (~spv).any()
        if grid[6] == "patchy":
            assert spv.any()                            # cells without ice: spval_dbl
    assert np.abs(np.where(d[f"o02n{NDTE:04d}_sig1"] == tail_ref.SPVAL_DBL, 0.0, d[f"o02n{NDTE:04d}_sig1"])).max() > 0.0
