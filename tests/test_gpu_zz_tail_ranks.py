"""GPU (-m gpu), run last: the calls between the subcycle loop and transport on several ranks -- the T-point ocean stress and the
principal stresses on the B grid (cice_evp_hip_strocn_t, cice_evp_hip_principal_stress), the end of evp() on the C grid
(cice_evp_hip_cgrid_tail, cice_evp_hip_cgrid_dyn_finish_u, cice_evp_hip_cgrid_strocn_t).  Their halo updates are the loops' own
exchanges with the unmasked lists: across a cut, across a tripole / tripoleT fold whose rows are cut in x, through the fold exchange.
Several ranks = several processes on the one GPU of the test box (tools/mailbox_2proc.py --tail): every output array of every rank,
whole blocks (ghost cells included), must equal the one-rank run of the same state cut into the same blocks, bit for bit -- and that
one-rank run is what tests/test_gpu_tail.py pins on the reference's arrays and on tests/tail_ref.py.

The on-chip resident kernels are off (CICE_EVP_HIP_RESIDENT=0 / CICE_EVP_HIP_CGRID_RESIDENT=0): processes that share one GPU cannot
keep their windows resident side by side.

Each subprocess gets ONE attempt under a timeout; a failed run leaves its whole output in a file under test_failures/ (git-ignored)
and fails."""
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


def _run(name, world, workload, shape, extra, env_extra, ndte=12):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           str(ROOT / "tools" / "mailbox_2proc.py"), "--workload", workload, "--ndte", str(ndte), "--shape", shape, "--tail"] + extra
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000", **env_extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    ok = r.returncode == 0 and "MAILBOX_2PROC OK tail" in r.stdout
    if not ok:
        try:
            (ROOT / "test_failures").mkdir(exist_ok=True)
            (ROOT / "test_failures" / f"tail_ranks_fail_{name}.log").write_text(" ".join(cmd) + "\n" + r.stdout + "\n---\n" + r.stderr)
        except OSError:
            pass
    print([ln for ln in r.stdout.splitlines() if ln.startswith("MAILBOX_2PROC")])
    assert ok, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


# name -> (ranks, workload, rank grid, further flags): at most 4 processes per case
CASES = {
    "ufold_cut2x1": (2, "120x80:tripole", "2x1", []),          # the fold row cut in x: seam partners on the other rank
    "ufold_cut1x2": (2, "120x80:tripole", "1x2", []),          # the fold on one rank, a plain cut below it
    "tfold_cut2x2": (4, "120x80:tripoleT", "2x2", []),
    "tfold_cut3x1": (3, "126x60:tripoleT", "3x1", []),         # partners on a third rank; the middle rank pairs with itself
    "closed_cut2x2": (4, "96x64", "2x2", []),
    "ufold_cut2x1_blocks2x2": (2, "120x80:tripole", "2x1", ["--blocks-per-rank", "2x2"]),      # copies inside a rank and exchanges mixed
    "closed_cut2x2_maskhalo": (4, "96x64", "2x2", ["--maskhalo"]),                              # a masked halo handed over: not used
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_bgrid_tail_on_several_ranks(name):
    world, workload, shape, extra = CASES[name]
    _run("b_" + name, world, workload, shape, extra, {"CICE_EVP_HIP_RESIDENT": "0"})


@pytest.mark.parametrize("name", sorted(CASES))
def test_cgrid_tail_on_several_ranks(name):
    world, workload, shape, extra = CASES[name]
    _run("c_" + name, world, workload, shape, ["--cgrid"] + extra, {"CICE_EVP_HIP_CGRID_RESIDENT": "0", "CICE_EVP_HIP_RESIDENT": "0"})
