"""GPU (-m gpu), run last: the post-loop calls of evp() on several ranks.  Two processes sharing this box's GPU
(tools/mailbox_2proc.py --post): after the loop -- the mailbox streaming path, the marching path with its ring between the ranks,
the marched zone beside ONE fold band for the grid -- and after stress_halo() where the grid has a fold, every rank runs
cice_evp_hip_deformations and cice_evp_hip_dyn_finish on its resident state.  deformations reads the final velocities at the four
corners of a T-cell: on the cut those are ghost cells that the loop's last halo update, or the marching path's final scatter, must
have left current.  Compared as bit patterns with the one-rank run of the whole grid on this rank's blocks, the T-cells of the east
and north fringe included; dyn_finish is handed a sentinel, which every cell it does not own must keep."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MARCH = dict(CICE_EVP_HIP_MARCH="1", CICE_EVP_HIP_RESIDENT="0", CICE_EVP_HIP_MARCH_SEG="24")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


CASES = [
    # gx3-size closed grid cut in x, the one-subcycle kernels with the mailbox halo; 9 subcycles: the loop ends on the other buffer
    ("streaming_2x1", "gx3", [], 9, dict(CICE_EVP_HIP_MARCH="0", CICE_EVP_HIP_RESIDENT="0")),
    # the same cut on the marching path: 9 = a leading single subcycle + two passes of four, the ring between the ranks
    ("march_2x1", "gx3", ["--march", "--ref-march-off", "--all-fields"], 9, dict(MARCH, CICE_EVP_HIP_MARCH_K="4", CICE_EVP_HIP_MARCH_EXT="4")),
    # tripole: the fold row split, one band for the grid; 7 = 3 + 3 + 1 with three subcycles per pass
    ("march_fold_band_2x1", "120x80:tripole", ["--march", "--ref-march-off", "--all-fields", "--stress-halo", "--expect-fold-band"], 7,
     dict(MARCH, CICE_EVP_HIP_MARCH_K="3", CICE_EVP_HIP_MARCH_EXT="0")),
]


@pytest.mark.parametrize("tag,workload,extra,ndte,env_more", CASES, ids=[c[0] for c in CASES])
def test_post_loop_calls_on_two_ranks_equal_the_one_rank_run(tag, workload, extra, ndte, env_more):
    """The tool's own checks carry the evidence of the path: --march fails unless mode == 1, declined == 0 and passes > 0 on every
    rank, --expect-fold-band unless the band's subcycles and describe_path() say so; the streaming case asserts the mailbox."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "tools" / "mailbox_2proc.py"), "--post", "--workload", workload,
           "--ndte", str(ndte), "--shape", "2x1"] + extra
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000", **env_more)
    for k in ("CICE_EVP_HIP_MARCH_OVERLAP", "CICE_EVP_HIP_MARCH_DIRECT"):
        env.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    ok = r.returncode == 0 and "MAILBOX_2PROC OK" in r.stdout
    print(r.stdout[-1500:])
    if not ok:
        print(r.stdout[-8000:])
        print(r.stderr[-4000:], file=sys.stderr)
    assert ok, (r.stdout[-2500:], r.stderr[-3000:])
    if "--march" not in extra:          # (tile_variant of either rank: the one-subcycle kernel)
        assert "MAILBOX_2PROC OK" in r.stdout and all(int(v) < 1000 for v in _tile_variants(r.stdout)), r.stdout[-1500:]


def _tile_variants(stdout):
    """tile_variant of every rank from the tool's result line: (rank, [], t_us, launches_per_subcycle, tile_variant) per rank."""
    import re
    line = next(l for l in stdout.splitlines() if l.startswith("MAILBOX_2PROC"))
    found = re.findall(r"\((\d+), \[\], None, [^,]*, (\d+)\)", line)
    assert sorted(int(r) for r, _ in found) == [0, 1], line
    return [v for _, v in found]
