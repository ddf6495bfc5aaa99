"""GPU (-m gpu), run last: visc_method = avg_strength on the marched split schedules of the C grid over several ranks, which take it on
request (CICE_EVP_HIP_CGRID_MARCH_AVG_STRENGTH=1; cice_amd/csrc/evp_host_cgrid_loop.cpp):

  * tripole / tripoleT: "marched zone + fold band + frame" (enqueue_march_fold with the exchanges of the five phases), forced as
    tests/test_gpu_zz_cgrid_march_fold_ranks.py forces it;
  * no fold: "zone marched + frame" with the five list-driven phase kernels on the frame (march_frame_phases; plan:
    tests/test_cgrid_march_frame_phases_plan_cpu.py), under CICE_EVP_HIP_CGRID_STRIP=1 as tests/test_gpu_zz_cgrid_march_ranks.py.

Several ranks = several processes on the one GPU of the test box (tools/mailbox_2proc.py --cgrid --visc avg_strength): every rank's
arrays, ghost cells included, must equal the one-rank, one-block run of the same state bit for bit, and every rank with rectangles
must have run every subcycle of its last call but the first after an upload on the schedule.  Without the switch the cut grid keeps
the five full phases and the same bits.  Each subprocess gets one attempt under a timeout (the helpers of the two files named above)."""
import pytest

from test_gpu_zz_cgrid_march_fold_ranks import FORCED as FOLD_FORCED, SCHEDULE as FOLD_SCHEDULE, _run as run_fold
from test_gpu_zz_cgrid_march_ranks import FORCED as STRIP_FORCED, _run as run_no_fold

pytestmark = pytest.mark.gpu

SWITCH = {"CICE_EVP_HIP_CGRID_MARCH_AVG_STRENGTH": "1"}
AVGS = ["--visc", "avg_strength"]

FOLD = {
    "world2_cut1x2": (2, "400x160:tripole", "1x2"),            # fold rows on the top rank; the bottom rank zone + frame
    "world2_cut2x1": (2, "400x80:tripole", "2x1"),             # fold rows cut in x: the fold exchange
    "tfold_world4_cut2x2": (4, "400x160:tripoleT", "2x2"),
}


@pytest.mark.parametrize("name", sorted(FOLD))
def test_cgrid_avg_strength_marched_beside_fold_band_and_frame(name):
    world, workload, shape = FOLD[name]
    out = run_fold("avgs_" + name, world, workload, shape, AVGS, dict(FOLD_FORCED, **SWITCH))
    assert out.count(FOLD_SCHEDULE) >= world and "avg_strength" in out, out[-2000:]


NO_FOLD = {
    "world2_cut2x1": (2, "400x216", "2x1", []),
    "world4_cut2x2": (4, "400x432", "2x2", []),                                       # corner neighbours on other ranks
    "maskhalo_caps": (2, "400x216", "2x1", ["--maskhalo", "--case", "caps"]),         # every in-loop exchange through the masked halo
}


@pytest.mark.parametrize("name", sorted(NO_FOLD))
def test_cgrid_avg_strength_marched_beside_the_five_phase_frame(name):
    world, workload, shape, extra = NO_FOLD[name]
    run_no_fold("avgs_" + name, world, workload, shape, extra + AVGS + ["--expect-marched"], dict(STRIP_FORCED, **SWITCH), ndte=12, timeout=300)


def test_cgrid_avg_strength_without_the_switch_keeps_the_five_phases():
    """the bits only: the harness's --expect-marched is not given (with it this case fails: the counter reads 0)"""
    run_no_fold("avgs_switch_unset", 2, "400x216", "2x1", AVGS, STRIP_FORCED, ndte=12, timeout=300)
