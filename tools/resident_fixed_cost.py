"""What a launch of the on-chip resident B-grid kernel costs beside its subcycles: subcycle(8) and subcycle(40) on the state
bench.py's headline runs (gx1, "full", one block, strict fp64), several times each, timings()["loop_ms"] of every call; a line
through the two medians gives the slope (ms per subcycle) and the intercept (the fixed cost per launch: prologue, per-CU lock,
state loads, write-back, the launch itself).  Usage: python tools/resident_fixed_cost.py [repeats] [--testing]
(--testing: the test build, whose A/B switches -- CICE_EVP_HIP_RES_NOLOCK, CICE_EVP_HIP_RES_PRIO, ... -- are read from the
environment; setting one of them selects it as well)"""
import os, sys, pathlib
R = str(pathlib.Path(__file__).resolve().parents[1]); sys.path[:0] = [R, R + "/tests", R + "/oracle"]
os.environ.setdefault("CICE_EVP_HIP_RESIDENT", "1")
import numpy as np
from cice_amd import decomp, evp, synth
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 15
SHORT, LONG = 8, 40
spec = synth.GRIDS["gx1"]
nx, ny = spec["nx"], spec["ny"]
g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns="closed"))
st = synth.make_state(g, case="full", seed=20260928, warm=True)
dc = decomp.per_rank_blocks(nx, ny, 1, "cyclic", "closed", None)
geo = {k: dc.scatter(g[k], 0, fill=(1.0 if k != "uarear" else 0.0)) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")}
fields = {k: dc.scatter(st[k], 0) for k in evp.FIELDS}
tm, um = dc.scatter(st["iceTmask"], 0, fill=0), dc.scatter(st["iceUmask"], 0, fill=0)
d, keep = evp.make_dims(dc, 0)
core = evp.EvpHip(d, evp.make_params(synth.evp_scalars(120), strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"], geo["uarear"],
                  geo["tarea"], keepalive=keep, testing=(True if "--testing" in sys.argv else None))
core.upload(fields, tm, um)
for _ in range(3):
    core.subcycle(120)
core.sync()
ms = {SHORT: [], LONG: []}
for _ in range(reps):                     # alternating, so that a drift of the clock reaches both alike
    for n in (SHORT, LONG):
        core.subcycle(n)
        core.sync()
        ms[n].append(core.timings()["loop_ms"])
tt = core.timings()
path = core.describe_path()
core.finalize()
assert tt["resident_fallbacks"] == 0, tt
a, b = np.median(ms[SHORT]), np.median(ms[LONG])
slope = (b - a) / (LONG - SHORT)
icpt = a - slope * SHORT
print("RESULT fixed cost gx1 tile_variant", tt["tile_variant"], "rim-wave schedule" if "edge U-cells in the rim wave" in path else "other schedule",
      f"repeats {reps}")
for n in (SHORT, LONG):
    v = np.array(ms[n]) * 1e3
    print(f"  subcycle({n:2d}): loop_ms median {np.median(v):8.2f} us  min {v.min():8.2f}  max {v.max():8.2f}")
print(f"  slope {slope * 1e3:.3f} us per subcycle, intercept (fixed cost per launch) {icpt * 1e3:.2f} us; "
      f"from the minima: slope {(min(ms[LONG]) - min(ms[SHORT])) / (LONG - SHORT) * 1e3:.3f}, "
      f"intercept {(min(ms[SHORT]) - (min(ms[LONG]) - min(ms[SHORT])) / (LONG - SHORT) * SHORT) * 1e3:.2f} us")
