"""GPU (-m gpu), run last: the C-grid subcycle on a tripole / tripoleT grid over several ranks as "marched zone + fold band + frame"
(cice_amd/csrc/evp_host_cgrid_loop.cpp: enqueue_march_fold; plan: cgrid_plan.cpp, build_cg_march_fold) -- cg_strip on the rectangles under
the fold band, the list-driven five phase kernels on every other interior cell, with the five phases' exchanges and fold steps at
their points.  Several ranks = several processes on the one GPU of the test box (tools/mailbox_2proc.py --cgrid --fold-ghosts
--expect-marched-fold): every rank's arrays, the ghost row beyond the fold and row NY's east-west ghost cells included, must equal the
one-rank, one-block run of the same state bit for bit, and every rank with rectangles must have run every subcycle of its last call
but the first after an upload on the schedule, with frame cells in its rest, and name it in describe_path().

The schedule is forced with CICE_EVP_HIP_CGRID_MARCH_FOLD=1 (which the one-rank reference run of the harness obeys too) and, across
ranks, CICE_EVP_HIP_CGRID_MARCH_FOLD_RANKS=1: ..._MARCH_FOLD=1 alone leaves several ranks to the size rule, as
test_gpu_cgrid_march_tripole.py pins.  The on-chip resident kernel is off (CICE_EVP_HIP_CGRID_RESIDENT=0).

Each subprocess gets ONE attempt under a timeout; a failed run leaves its whole output in a file under test_failures/ (git-ignored)
and fails."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from common import wide

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FORCED = {"CICE_EVP_HIP_CGRID_MARCH_FOLD": "1", "CICE_EVP_HIP_CGRID_MARCH_FOLD_RANKS": "1", "CICE_EVP_HIP_CGRID_RESIDENT": "0"}
SCHEDULE = "marched zone + fold band + frame"


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _run(name, world, workload, shape, extra, env_extra, ndte=12, expect=True):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           str(ROOT / "tools" / "mailbox_2proc.py"), "--cgrid", "--fold-ghosts", "--workload", workload, "--ndte", str(ndte),
           "--shape", shape] + extra + (["--expect-marched-fold"] if expect else [])
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000", **env_extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    ok = r.returncode == 0 and "MAILBOX_2PROC OK" in r.stdout
    if not ok:
        try:
            (ROOT / "test_failures").mkdir(exist_ok=True)
            (ROOT / "test_failures" / f"cgrid_march_fold_ranks_fail_{name}.log").write_text(" ".join(cmd) + "\n" + r.stdout + "\n---\n" + r.stderr)
        except OSError:
            pass
    print([ln for ln in r.stdout.splitlines() if ln.startswith("MAILBOX_2PROC")])
    assert ok, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


CASES = {
    "world2_cut2x1": (2, "400x80:tripole", "2x1", []),                 # fold rows cut in x: the fold exchange
    "world2_cut1x2": (2, "400x160:tripole", "1x2", []),                # fold rows on the top rank; the bottom rank frame only, closed south
    "world4_cut2x2": (4, "400x160:tripole", "2x2", []),                # both cuts at once, corner peers
    "world3_cut3x1_blocks2x1": (3, "600x80:tripole", "3x1", ["--blocks-per-rank", "2x1"]),   # local and remote neighbours, seam partners on a third rank
    "tfold_cut2x1": (2, "400x80:tripoleT", "2x1", []),
    "tfold_cut1x2": (2, "400x160:tripoleT", "1x2", []),
    "maskhalo_caps": (2, "400x80:tripole", "2x1", ["--maskhalo", "--case", "caps"]),
    "prep_cut1x2": (2, "400x160:tripole", "1x2", ["--prep"]),          # the preparation phase on the device first (a y-cut: it refuses split fold rows)
    "timing_odd_counts": (2, "400x80:tripole", "2x1", ["--timing"]),   # 3 x 40 + 7 more subcycles without an upload: ping-pong parity
}
# nothing forced, the product library: 1440 x 1080 tripole over 2 ranks is 777 600 cells per rank, above cg_strip's size rule.  The only
# case of its size, 9 s on the box -- beyond the few seconds a case of the default suite may take: it runs with EVP_GPU_SUITE=full
UNFORCED = {"unforced_1440x1080": (2, "1440x1080:tripole", "1x2", [])}
SPLIT_FOLD = {"world2_cut2x1", "world4_cut2x2", "world3_cut3x1_blocks2x1", "tfold_cut2x1", "maskhalo_caps", "timing_odd_counts"}


@pytest.mark.parametrize("name", sorted(CASES) + wide(sorted(UNFORCED)))
def test_cgrid_marched_beside_fold_band_and_frame_across_processes(name):
    forced = name in CASES
    world, workload, shape, extra = (CASES if forced else UNFORCED)[name]
    out = _run(name, world, workload, shape, extra, FORCED if forced else {}, ndte=12 if forced else 6)
    assert out.count(SCHEDULE) >= world, out[-2000:]
    # (--fold-ghosts reports (fold exchange in use, ranks that hold fold rows, schedule) per rank)
    assert ("(True, " in out) == (name in SPLIT_FOLD), out[-2000:]
    if name in SPLIT_FOLD:
        assert "+ fold exchange, fold rows on" in out, out[-2000:]


def test_cgrid_switch_forces_the_five_phases_on_every_rank():
    """CICE_EVP_HIP_CGRID_ONE=0 beside the forcing switches: the five full phases with the fold exchange on every rank, same bits"""
    out = _run("switch_off", 2, "400x80:tripole", "2x1", [], dict(FORCED, CICE_EVP_HIP_CGRID_ONE="0"), expect=False)
    assert SCHEDULE not in out and "C grid: five phases + fold exchange, fold rows on" in out, out[-2000:]


def test_cgrid_marching_and_non_marching_ranks_side_by_side():
    """400 x 24 tripoleT cut 1 x 2: the lower rank has a zone (one window row), the upper rank's 12 rows at the T-fold leave none
    (tests/test_cgrid_march_fold_ranks_plan_cpu.py shows which rank declines, and why no cut in x gives such a pair): it keeps the five
    full phases.  Both issue the same exchanges at the same points."""
    out = _run("mixed_400x24_tripoleT", 2, "400x24:tripoleT", "1x2", [], FORCED)
    assert out.count(SCHEDULE) == 1, out[-2000:]
