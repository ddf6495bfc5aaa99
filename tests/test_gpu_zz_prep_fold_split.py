"""GPU (-m gpu), run last: what runs AROUND the subcycle loop on tripole / tripoleT grids whose fold rows are cut in x over ranks --
the device preparation of both grids (cice_evp_hip_prep, cice_evp_hip_cgrid_prep: the T-grid fields through the C grid's fold
exchange, then the centre fold step in one batch, cice_amd/csrc/evp_fold_prep.hip) and the tripoleT stress symmetrisation
(cice_evp_hip_stress_halo: each pair through the exchange, partner values in staging slots).  Several ranks = several processes on
the one GPU of the test box (tools/mailbox_2proc.py): every rank's arrays must equal the one-rank run of the same state bit for bit.

The on-chip resident kernels are off (CICE_EVP_HIP_RESIDENT=0 / CICE_EVP_HIP_CGRID_RESIDENT=0): processes that share one GPU cannot
keep their windows resident side by side.

Each subprocess gets ONE attempt under a timeout; a failed run leaves its whole output in a file under test_failures/ (git-ignored)
and fails."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _run(name, world, workload, shape, extra, env_extra, ndte=12):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           str(ROOT / "tools" / "mailbox_2proc.py"), "--workload", workload, "--ndte", str(ndte), "--shape", shape] + extra
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000", **env_extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    ok = r.returncode == 0 and "MAILBOX_2PROC OK" in r.stdout
    if not ok:
        try:
            (ROOT / "test_failures").mkdir(exist_ok=True)
            (ROOT / "test_failures" / f"prep_fold_split_fail_{name}.log").write_text(" ".join(cmd) + "\n" + r.stdout + "\n---\n" + r.stderr)
        except OSError:
            pass
    print([ln for ln in r.stdout.splitlines() if ln.startswith("MAILBOX_2PROC")])
    assert ok, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


# B grid, tripoleT, preparation on the device: prep products, iceTmask, velocities and stresses against the one-rank run
BGRID_PREP = {
    "cut2x1": (2, "120x80:tripoleT", "2x1", []),       # every mirror pair crosses the cut; the self-mirror columns 1 and NX/2+1 are rank-local
    "cut3x1": (3, "126x60:tripoleT", "3x1", []),       # partners on a third rank; the middle rank pairs with itself
    "cut2x2": (4, "120x80:tripoleT", "2x2", []),       # both cuts
    "cut2x1_blocks2x2": (2, "120x80:tripoleT", "2x1", ["--blocks-per-rank", "2x2"]),   # local and remote partners mixed
}


@pytest.mark.parametrize("name", sorted(BGRID_PREP))
def test_bgrid_device_preparation_on_a_tripolet_grid_cut_in_x(name):
    world, workload, shape, extra = BGRID_PREP[name]
    _run("bprep_" + name, world, workload, shape, ["--prep"] + extra, {"CICE_EVP_HIP_RESIDENT": "0"})


# the stress symmetrisation: all twelve stresses, every block array whole (ghost ring included), against ONE rank owning the same
# blocks -- whose symmetrisation tests/test_gpu_parity.py pins on the reference's own arrays
STRESS = {
    "tfold_cut2x1": (2, "120x80:tripoleT", "2x1"),
    "tfold_cut3x1": (3, "126x60:tripoleT", "3x1"),
    "tfold_cut2x2": (4, "120x80:tripoleT", "2x2"),
    "ufold_tx1_cut2x1": (2, "tx1", "2x1"),             # control: the flags change nothing of what passed before
}


@pytest.mark.parametrize("name", sorted(STRESS))
def test_stress_symmetrisation_with_the_top_row_on_several_ranks(name):
    world, workload, shape = STRESS[name]
    _run("stress_" + name, world, workload, shape, ["--stress-halo", "--same-blocks-ref"], {"CICE_EVP_HIP_RESIDENT": "0"})


# C grid, preparation on the device; --fold-ghosts also compares the ghost row beyond the fold and row NY's east-west ghost cells
FORCING_FOLD = ["--forcing", "0,C,B"]                  # ocean on E / N, wind on U: the averages read the halo-updated ghost cells
MARCH_FOLD = {"CICE_EVP_HIP_CGRID_MARCH_FOLD": "1", "CICE_EVP_HIP_CGRID_MARCH_FOLD_RANKS": "1"}      # (test_gpu_zz_cgrid_march_fold_ranks.py)
CGRID_PREP = {
    "ufold_cut2x1": (2, "120x80:tripole", "2x1", [], {}),
    "tfold_cut2x1": (2, "120x80:tripoleT", "2x1", [], {}),
    "ufold_cut2x2": (4, "120x80:tripole", "2x2", [], {}),
    "tfold_cut3x1": (3, "126x60:tripoleT", "3x1", [], {}),
    "ufold_cut2x1_forcing": (2, "120x80:tripole", "2x1", FORCING_FOLD, {}),
    # the x-cut twin of test_gpu_zz_cgrid_march_fold_ranks.py's prep_cut1x2
    "ufold_marched_cut2x1": (2, "400x80:tripole", "2x1", ["--expect-marched-fold"], MARCH_FOLD),
}


@pytest.mark.parametrize("name", sorted(CGRID_PREP))
def test_cgrid_device_preparation_with_the_fold_rows_cut_in_x(name):
    world, workload, shape, extra, env = CGRID_PREP[name]
    out = _run("cprep_" + name, world, workload, shape, ["--cgrid", "--prep", "--fold-ghosts"] + extra,
               dict(env, CICE_EVP_HIP_CGRID_RESIDENT="0"))
    # (--fold-ghosts reports (fold exchange in use, ranks that hold fold rows, schedule) per rank)
    assert "(True, " in out, out[-2000:]


def test_still_refused_next_to_an_eliminated_block_on_one_rank():
    """One rank, tripoleT, a land block of the top block row eliminated: no fold exchange covers its cells.  The device preparation
    and the stress symmetrisation still refuse, and say which kind of layout it is -- plain API calls, nothing is launched."""
    from cice_amd import decomp, evp, synth
    nx, ny = 72, 40
    dc = decomp.Decomp(nx, ny, 18, 10, "cyclic", "tripoleT", 1)
    for b in dc.blocks:
        if b.jblock == dc.nblocks_y and b.iblock == 3:
            b.owner = -1
    for k, b in enumerate(sorted((b for b in dc.blocks if b.owner == 0), key=lambda b: b.gid)):
        b.local = k
    g = synth.derive_geometry(synth.make_grid(nx, ny, 1.1e5, ns="tripole"))
    geo = {k: dc.scatter(g[k], 0, fill=(1.0 if k != "uarear" else 0.0)) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")}
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(synth.evp_scalars(120), strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"],
                      geo["uarear"], geo["tarea"], keepalive=keep)
    try:
        assert core.lib.cice_evp_hip_stress_halo_available() == 0
        shape = (len(dc.local_blocks(0)), dc.ny_block, dc.nx_block)
        ones, onei = np.ones(shape), np.ones(shape, dtype=np.int32)
        with pytest.raises(evp.EvpHipError, match="eliminated block") as e1:
            core.set_prep_geometry(onei, onei, ones, ones, ones, ones)
        assert "rc=-9" in str(e1.value)
        with pytest.raises(evp.EvpHipError, match="eliminated block") as e2:
            core.stress_halo()
        assert "rc=-9" in str(e2.value)
    finally:
        core.finalize()
