"""GPU (-m gpu), run last: the calls after the C-grid loop on several ranks BEHIND the schedules that march a zone -- "zone marched +
frame" (no fold), "marched zone + fold band + frame" on a tripole grid whose fold rows are cut in x (fold exchange, staging tails behind
the arrays) and on a tripoleT grid cut in y.  The several-rank cases of tests/test_gpu_zz_tail_ranks.py run grids on which no zone
forms; here every rank runs cgrid_deformations, cgrid_dyn_finish (a sentinel in every inout array), cgrid_tail, cgrid_dyn_finish_u,
cgrid_strocn_t and cgrid_download after 7 and after 8 subcycles -- either parity of the swaps that leave uvelE, vvelN, stresspT,
stressmT and stress12U in one of their two allocations --, one case from cice_evp_hip_cgrid_prep (a cut in y: the preparation refuses
split fold rows).  Several ranks = several processes on the one GPU of the test box (tools/mailbox_2proc.py --cgrid --post --tail):
every output array of every rank, whole blocks (ghost cells included), must equal the one-rank run of the same state cut into the same
blocks, bit for bit -- the one-rank run that tests/test_gpu_call_chain_cgrid.py pins on the reference's arrays and the oracle's chain --,
and every rank with rectangles must have run every subcycle but the first on the schedule asked for (--expect-marched /
--expect-marched-fold).

The on-chip resident kernel is off (CICE_EVP_HIP_CGRID_RESIDENT=0): processes that share one GPU cannot keep their windows resident
side by side.  Each subprocess gets ONE attempt under a timeout; a failed run leaves its whole output in a file under test_failures/
(git-ignored) and fails."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
FRAME = {"CICE_EVP_HIP_CGRID_STRIP": "1", "CICE_EVP_HIP_CGRID_RESIDENT": "0"}
FOLD = {"CICE_EVP_HIP_CGRID_MARCH_FOLD": "1", "CICE_EVP_HIP_CGRID_MARCH_FOLD_RANKS": "1", "CICE_EVP_HIP_CGRID_RESIDENT": "0"}


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _run(name, world, workload, shape, extra, env_extra, ndte):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           str(ROOT / "tools" / "mailbox_2proc.py"), "--cgrid", "--post", "--tail", "--workload", workload, "--ndte", str(ndte),
           "--shape", shape] + extra
    env = dict(os.environ, CICE_EVP_HIP_HALO_TIMEOUT_MS="20000", **env_extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    ok = r.returncode == 0 and "MAILBOX_2PROC OK tail cgrid" in r.stdout
    if not ok:
        try:
            (ROOT / "test_failures").mkdir(exist_ok=True)
            (ROOT / "test_failures" / f"cgrid_call_chain_ranks_fail_{name}.log").write_text(" ".join(cmd) + "\n" + r.stdout + "\n---\n" + r.stderr)
        except OSError:
            pass
    print([ln for ln in r.stdout.splitlines() if ln.startswith("MAILBOX_2PROC")])
    assert ok, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


# name -> (ranks, workload, rank grid, switches, evidence, the schedule's name, further flags): 2 processes per case
CASES = {
    "frame_cut2x1": (2, "400x216", "2x1", FRAME, "--expect-marched", "zone marched + frame", []),
    "ufold_cut2x1": (2, "400x80:tripole", "2x1", FOLD, "--expect-marched-fold", "marched zone + fold band + frame", []),   # fold exchange, staging tails
    "tfold_cut1x2": (2, "400x160:tripoleT", "1x2", FOLD, "--expect-marched-fold", "marched zone + fold band + frame", []),
    "tfold_cut1x2_prep": (2, "400x160:tripoleT", "1x2", FOLD, "--expect-marched-fold", "marched zone + fold band + frame", ["--prep"]),
}
ROWS = [(n, k) for n in CASES for k in ((7,) if n.endswith("_prep") else (7, 8))]


@pytest.mark.parametrize("name,ndte", ROWS)
def test_cgrid_calls_after_the_loop_behind_a_marched_zone_on_several_ranks(name, ndte):
    world, workload, shape, env, expect, schedule, extra = CASES[name]
    out = _run(f"{name}_ndte{ndte}", world, workload, shape, [expect] + extra, env, ndte)
    assert schedule in out, out[-2000:]
    if name == "ufold_cut2x1":
        assert "+ fold exchange, fold rows on" in out, out[-2000:]
