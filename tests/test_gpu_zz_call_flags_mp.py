"""GPU (-m gpu), run last: the per-call shortcut verdicts are per rank.  Two ranks -- processes sharing this box's GPU, exchanging
through the mailbox transport (tools/mailbox_2proc.py --deviate RANK:KIND) -- in the default configuration, with a seabed stress
factor of 0.7 on ONE ice cell of one rank, next to the cut: that rank drops its shortcut, the other keeps it (its ghost image of
the cell is not a cell it advances), each rank reports its own read-out, and the gathered result equals the one-rank run bit for
bit."""
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


@pytest.mark.parametrize("shape,extra", [
    ("2x1", ["--deviate", "1:TbU"]),                    # B grid, gx3 cut in x: one U-cell of rank 1 in a column next to rank 0
    ("1x2", ["--cgrid", "--deviate", "0:TbN"]),         # C grid, gx3 cut in y: one N face of rank 0 in the row under rank 1
    # the marching kernel advances a rim of the other rank's cells too and exchanges the optional operands apart: with verdicts
    # that differ it must decline the call on both ranks (evp_host_march.cpp: march_run) -- the one-subcycle kernel's bits
    ("2x1", ["--march", "--deviate", "1:TbU"]),
])
def test_one_rank_drops_the_shortcut_the_other_keeps_it(shape, extra):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "tools" / "mailbox_2proc.py"), "--workload", "gx3", "--ndte", "7",
           "--shape", shape] + extra
    # (each child under its own time limit: the transport's, well inside the launcher's; the launcher ends every child at the first
    # one that fails, and its exit status is checked here)
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000")
    if "--march" in extra:
        env.update(CICE_EVP_HIP_MARCH="1", CICE_EVP_HIP_RESIDENT="0", CICE_EVP_HIP_MARCH_SEG="24", CICE_EVP_HIP_MARCH_EXT="6", CICE_EVP_HIP_MARCH_K="2")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "MAILBOX_2PROC OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
