"""GPU (-m gpu), run last: the device preparation under forcing layouts other than the default with the domain split over
several ranks -- processes sharing this box's GPU, exchanging through the mailbox transport (tools/mailbox_2proc.py,
--prep --forcing).  With calc_strair = .false. the T-grid exchange carries eight fields instead of ten on every path
(plain pairs, the split-fold seam, the shifted-copy fold exchange): every rank must run the same count, and the wind
stress must be averaged with the ghost cells the rank holds."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def run_ranks(world, workload, shape, extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           str(ROOT / "tools" / "mailbox_2proc.py"), "--workload", workload, "--ndte", "24", "--shape", shape, "--prep"] + extra
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "MAILBOX_2PROC OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("world,workload,shape,extra", [
    # tripole grid with the fold row split in x: the seam ghosts and the shifted-copy exchange of the T-grid fields
    (2, "tx1", "2x1", ["--forcing", "0,C,B"]),
    (2, "tx1", "2x1", ["--forcing", "1,C,A"]),
    # ... and strax / stray ghost cells that differ from what an exchange would put there (read as given)
    (2, "tx1", "2x1", ["--forcing", "0,B,C", "--wind-ghosts", "own"]),
    (4, "gx3", "2x2", ["--forcing", "0,B,C", "--blocks-per-rank", "2x1"]),
])
def test_bgrid_forcing_layout_across_processes(world, workload, shape, extra):
    """B grid: every rank's preparation products (uocnU, vocnU, strairxU, strairyU, forcexU, ...) and the loop after it
    equal the one-rank run on the physical cells, bit for bit; with --wind-ghosts own the wind averages equal the numpy
    restatement applied to the rank's own strax / stray (and the changed ghost cells are read)."""
    run_ranks(world, workload, shape, extra)


@pytest.mark.parametrize("world,workload,shape,extra", [
    # (the C-grid device preparation refuses a fold row split in x: tx1 is cut in y here)
    (2, "tx1", "1x2", ["--cgrid", "--forcing", "0,C,B"]),
    (2, "tx1", "1x2", ["--cgrid", "--forcing", "0,C,B", "--wind-ghosts", "own"]),
    (4, "gx1", "2x2", ["--cgrid", "--forcing", "0,A,C", "--blocks-per-rank", "2x1"]),
])
def test_cgrid_forcing_layout_across_processes(world, workload, shape, extra):
    """C grid: the loop inputs the preparation makes at E / N points (uocnE ... vocnN, strairxE, strairyN, forcexE, ...), the
    masks and the 19 loop outputs after it equal the one-rank run, bit for bit; with --wind-ghosts own the wind averages
    equal the restatement on the rank's own strax / stray."""
    run_ranks(world, workload, shape, extra)
