"""GPU: the marching path on tripole / tripoleT grids split over several ranks -- "marched zone + fold band" with ONE band for the grid,
held by the top row of ranks (cice_amd/csrc/march_plan.h, evp_host_march.cpp) -- as processes sharing one GPU, through
tools/mailbox_2proc.py as test_gpu_zz_multiprocess.py::test_two_subcycle_kernel_across_processes_on_one_gpu runs the closed grids:
the ring exchanges and rank agreements go through the library's test transport, the band's per-subcycle velocity halo through the
mailbox; plan, lists, schedule and kernels are the product's.

Every rank's velocities (ghost cells included), 12 stresses, strintx / strinty and taubx / tauby must equal, as bit patterns, the
one-rank run of the whole grid with the marching path OFF (the one-subcycle kernels: the two sides share no marching code).  Small
grids on which the geometry can still go wrong: corners above the zone on a cut in x, the fold row split, the band on one rank of
two, a leading single subcycle, several blocks per rank on a T-fold, an odd split with pieces narrower than a strip, ice_HaloMask
lists, fused mode with an odd number of band subcycles (the block layout's ping-pong parity).

On the T-fold the velocities are handed over as a halo update leaves them (the tool, under --all-fields): the top physical row as
the image of the row below, so a resting land cell next to a pole shows up there as -0.0.  Where a rank's blocks let every computing
thread store the images of its own cell, the image of a land cell keeps the value it was handed over with, whereas the one-rank run's
gather-form halo rewrites it as -1 * 0.0: with a top row of plain +0.0 the two east-west ghost cells of that row would differ from the
one-rank run in the sign of zero on every rank of the top row, marching path on or off."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, workload, shape, extra, ndte, env_more):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           str(ROOT / "tools" / "mailbox_2proc.py"), "--march", "--ref-march-off", "--all-fields", "--workload", workload,
           "--ndte", str(ndte), "--shape", shape] + extra
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000", CICE_EVP_HIP_MARCH="1", CICE_EVP_HIP_RESIDENT="0",
               CICE_EVP_HIP_MARCH_SEG="24", **env_more)
    for k in ("CICE_EVP_HIP_MARCH_OVERLAP", "CICE_EVP_HIP_MARCH_DIRECT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    ok = r.returncode == 0 and "MAILBOX_2PROC OK" in r.stdout
    if not ok:          # (pytest shows both with the failure, whole: the tool's result line names every cell that differs)
        print(r.stdout[-8000:])
        print(r.stderr[-4000:], file=sys.stderr)
    assert ok, (r.stdout[-2500:], r.stderr[-3000:])


CASES = [
    # corners above the zone on either side of both ranks; the fold row split
    ("2x1_ext0_k4", 2, "120x80:tripole", "2x1", [], 24, dict(CICE_EVP_HIP_MARCH_EXT="0", CICE_EVP_HIP_MARCH_K="4")),
    # the band on one rank only, the other exchanges in lockstep; 25 = 1 + 8 x 3: a leading single subcycle
    ("1x2_ext4_k3", 2, "120x80:tripole", "1x2", [], 25, dict(CICE_EVP_HIP_MARCH_EXT="4", CICE_EVP_HIP_MARCH_K="3")),
    # T-fold, several blocks per rank, corners between ranks of the top row and ranks of the bottom row
    ("2x2_T_blocks", 4, "120x80:tripoleT", "2x2", ["--blocks-per-rank", "2x1"], 24, dict(CICE_EVP_HIP_MARCH_EXT="4")),
    # an odd split: pieces of 33 / 33 / 32 columns, narrower than a strip, on an odd number of rows (98 columns, not 97: the halo plan
    # of a tripole grid asks for an even nx_global, so a 97-column grid does not initialise on any path)
    ("3x1_odd", 3, "98x61:tripole", "3x1", [], 24, dict(CICE_EVP_HIP_MARCH_EXT="2", CICE_EVP_HIP_MARCH_K="2")),
    # ice in the polar caps only, ice_HaloMask lists in the band's per-subcycle exchange
    ("2x2_caps_maskhalo", 4, "120x80:tripole", "2x2", ["--case", "caps", "--maskhalo"], 24, {}),
    # fused mode on a T-fold; 23 = 7 x 3 + 2: an odd number of band subcycles, so the block layout ends on its other ping-pong buffer
    ("2x1_T_fused_odd", 2, "120x80:tripoleT", "2x1", ["--fused"], 23, dict(CICE_EVP_HIP_MARCH_EXT="0", CICE_EVP_HIP_MARCH_K="3")),
]


@pytest.mark.parametrize("tag,world,workload,shape,extra,ndte,env_more", CASES, ids=[c[0] for c in CASES])
def test_march_tripole_across_processes_bitwise_vs_one_rank_streaming(tag, world, workload, shape, extra, ndte, env_more):
    """mode == 1, declined == 0, passes > 0 on every rank (the tool's --march check); band_subcycles == ndte - (ndte % K == 1) on the
    ranks with band rows and 0 on the others, "fold band" and the number of ranks in describe_path() (--expect-fold-band); every
    compared array bit-identical to the one-rank run with CICE_EVP_HIP_MARCH=0 (--ref-march-off, --all-fields)."""
    _run(world, workload, shape, extra + ["--expect-fold-band"], ndte, env_more)


def test_march_tripole_top_rank_too_thin_every_rank_stays_off_with_the_same_reason():
    """120 x 80 as 1 x 4 ranks with a rim of 8: the top rank's 20 rows leave its share of the zone thinner than rim + ring.  Every rank
    reaches that verdict from the global block table, stays off the path, says why, and the one-subcycle kernels give the one-rank bits."""
    _run(4, "120x80:tripole", "1x4", ["--expect-march-off", "share of the marched zone is thinner than its redundant rim + ring"], 24,
         dict(CICE_EVP_HIP_MARCH_EXT="8"))
