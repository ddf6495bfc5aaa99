#!/usr/bin/env python
"""Times whole cice_evp_hip_cgrid_subcycle calls on the 3600 x 2400 C-grid workload, tripole (marched zone + fold band, concurrent or
serial order, or today's five phases + fold steps) or closed (the control: cg_strip as it is), with the library of THIS tree or of
another tree (--root: e.g. the parent commit exported and built beside it), one process per run so that two libraries can be
alternated on one box:

    python tools/cgrid_march_tripole_timing.py --ns tripole --schedule march_fold --steps 5 --warmup 2 [--root DIR] [--ndte 120]
                                               [--visc avg_strength]

--schedule: march_fold (CICE_EVP_HIP_CGRID_MARCH_FOLD=1), serial (... and CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL=1), phases (the switch
off: what the parent commit runs), default (nothing forced).  --visc avg_strength: that visc_method, and on march_fold / serial /
default CICE_EVP_HIP_CGRID_MARCH_AVG_STRENGTH=1, without which the schedule stays off for it (a tree from before the switch ignores it
and runs its five phases; profiles/cgrid_march_avg_strength.txt).  Strict mode, ice on every ocean cell, the on-chip resident kernel off, HIP
events around each call (the library's own: cgrid_timings()["loop_ms"]).  Prints one JSON line.  profiles/r09_cgrid_march_tripole.txt
is where the runs this was written for belong."""
import argparse
import json
import os
import sys
from pathlib import Path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", choices=["tripole", "closed"], default="tripole")
    ap.add_argument("--schedule", choices=["march_fold", "serial", "phases", "default"], default="march_fold")
    ap.add_argument("--visc", choices=["avg_zeta", "avg_strength"], default="avg_zeta")
    ap.add_argument("--root", default=None, help="tree whose cice_amd package and library are timed (default: this one)")
    ap.add_argument("--nx", type=int, default=3600)
    ap.add_argument("--ny", type=int, default=2400)
    ap.add_argument("--ndte", type=int, default=120)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    here = Path(__file__).resolve().parents[1]
    root = Path(a.root).resolve() if a.root else here
    sys.path[:0] = [str(root)]
    os.environ.setdefault("CICE_EVP_HIP_CGRID_RESIDENT", "0")
    if a.schedule in ("march_fold", "serial"):
        os.environ["CICE_EVP_HIP_CGRID_MARCH_FOLD"] = "1"
    if a.schedule == "serial":
        os.environ["CICE_EVP_HIP_CGRID_MARCH_FOLD_SERIAL"] = "1"
    if a.schedule == "phases":
        os.environ["CICE_EVP_HIP_CGRID_MARCH_FOLD"] = "0"
    if a.visc == "avg_strength" and a.schedule != "phases":
        os.environ["CICE_EVP_HIP_CGRID_MARCH_AVG_STRENGTH"] = "1"
    import numpy as np
    from cice_amd import decomp, evp, synth
    assert Path(evp.__file__).resolve().is_relative_to(root), evp.__file__

    nx, ny, dx0 = a.nx, a.ny, 1.1e4
    g = synth.derive_geometry(synth.make_grid(nx, ny, dx0, ns=a.ns))
    cg = synth.cgrid_geometry(g)
    state, inputs, masks = synth.cgrid_state(g, cg, case="full", seed=20261017)
    dc = decomp.Decomp(nx, ny, nx, ny, "cyclic", a.ns, 1)
    static, state, inputs, masks = synth.cgrid_scatter(dc, 0, cg, state, inputs, masks)
    scal = synth.evp_scalars(a.ndte)
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(scal, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"],
                      1.0 / static["uarea"], static["tarea"], keepalive=keep)
    try:
        core.cgrid_set_geometry(static)
        core.cgrid_upload(state, inputs, masks, visc_method=a.visc)
        us = []
        for k in range(a.warmup + a.steps):
            core.cgrid_subcycle(a.ndte)
            core.cgrid_sync()
            if k >= a.warmup:
                us.append(core.cgrid_timings()["loop_ms"] * 1e3 / a.ndte)
        tt = core.cgrid_timings()
        out = dict(label=a.label or ("other tree" if a.root else "this tree"), ns=a.ns, schedule=a.schedule, visc=a.visc, ndte=a.ndte, warmup=a.warmup,
                   us_per_subcycle=[round(v, 2) for v in us], median=round(float(np.median(us)), 2),
                   marched={k: tt[k] for k in ("marched_items", "marched_cells", "marched_segment_rows", "marched_lengths_derived",
                                               "one_launch_subcycles", "marched_fold_subcycles", "fold_band_rows", "fold_rest_cells") if k in tt},
                   path=core.describe_path())
        print(json.dumps(out), flush=True)
    finally:
        core.finalize()


if __name__ == "__main__":
    main()
