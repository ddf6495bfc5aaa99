"""GPU (-m gpu): the C-grid loop on tripole grids whose fold rows are split over ranks (the C grid's fold exchange,
cice_amd/csrc/halo_plan.h: cg_*).  Processes time-slicing the one GPU of the box, their halos through the mailbox transport
(tools/mailbox_2proc.py --cgrid --fold-ghosts): every rank's arrays, the ghost row beyond the fold included, equal the
one-rank run bit for bit, and the library reports the split-fold schedule.  Then the reference's own MPI driver through the
Fortran shim on the layouts the drop-in used to refuse (run_case of test_gpu_zz_dropin_mpi.py, cgrid=True).  Named to sort
after the single-process tests, like test_gpu_zz_multiprocess.py."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from test_gpu_zz_dropin_mpi import run_case

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


@pytest.mark.parametrize("world,workload,shape,extra", [
    (2, "tx1", "2x1", []),
    (4, "tx1", "2x2", []),
    (4, "tx1", "4x1", []),
    (3, "tx1", "3x1", ["--blocks-per-rank", "2x1"]),
    (2, "tx1", "2x1", ["--visc", "avg_strength"]),
    (4, "tx1", "2x2", ["--maskhalo", "--case", "caps"]),
    (2, "120x80:tripoleT", "2x1", []),
    (4, "120x80:tripoleT", "2x2", []),
])
def test_cgrid_loop_with_the_fold_rows_split_over_processes(world, workload, shape, extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "tools" / "mailbox_2proc.py"), "--cgrid", "--fold-ghosts",
           "--workload", workload, "--shape", shape, "--ndte", "24", *extra]
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "MAILBOX_2PROC OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "(True, " in r.stdout and "C grid: five phases + fold exchange, fold rows on" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("nx,ny,bx,by,ew,ns,nprocs,dist,kw", [
    # the cuts test_gpu_zz_dropin_mpi.py skips on the C grid: 4 x 2 blocks over 3 tasks (4, 4, 0), the fold rows cut in x
    (54, 52, 14, 26, "cyclic", "tripole", 3, "cartesian", dict(grid_kind="tripolefile", icecase="full")),
    (54, 52, 14, 26, "cyclic", "tripoleT", 3, "cartesian", dict(grid_kind="tripolefile", icecase="full")),
    (72, 40, 18, 20, "cyclic", "tripole", 4, "roundrobin", dict(grid_kind="tripolefile", icecase="patchy")),
    # (a y-only cut through the fold rows cannot be built here: the reference's ice_HaloMsgCreate refuses a top block with fewer
    # rows than the fold reads -- tests/test_cgrid_fold_split_cpu.py covers that layout against the oracle)
])
def test_reference_mpi_driver_with_hip_cgrid_loop_on_a_split_fold(tmp_path, nx, ny, bx, by, ew, ns, nprocs, dist, kw):
    """dyn_evp_hip_cgrid_run on every task of the reference's driver where the blocks next to the fold belong to several
    tasks: every array the loop writes, every cell of every task (ghost cells included), the downstream fields
    (deformationsC_T, dyn_finish at E / N points) against the reference's standard_2d MPI path, and the assembled fields
    against its serial build."""
    run_case(tmp_path, nx, ny, bx, by, ew, ns, nprocs, dist, False, kw, cgrid=True)
