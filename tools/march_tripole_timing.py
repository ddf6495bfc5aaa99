#!/usr/bin/env python
"""Times whole cice_evp_hip_subcycle calls on the 3600 x 2400 workload, tripole (the marched zone + fold band) or closed (s01), with
the library of THIS tree or of another tree (--root: e.g. the parent commit exported and built beside it), one process per run so
that two libraries can be alternated on one box:

    python tools/march_tripole_timing.py --ns tripole --steps 5 --warmup 2 [--root DIR] [--ndte 120]

Strict mode, ice on every ocean cell, HIP events around each call (the library's own: timings()["loop_ms"]).  Prints one JSON line.
profiles/r08_march_tripole.txt holds the runs this was written for."""
import argparse
import json
import os
import sys
from pathlib import Path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", choices=["tripole", "closed"], default="tripole")
    ap.add_argument("--root", default=None, help="tree whose cice_amd package and library are timed (default: this one)")
    ap.add_argument("--ndte", type=int, default=120)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--label", default=None)
    a = ap.parse_args()
    here = Path(__file__).resolve().parents[1]
    root = Path(a.root).resolve() if a.root else here
    sys.path[:0] = [str(root)]
    os.environ.setdefault("CICE_EVP_HIP_RESIDENT", "0")
    import numpy as np
    from cice_amd import decomp, evp, synth
    assert Path(evp.__file__).resolve().is_relative_to(root), evp.__file__

    nx, ny, dx0 = 3600, 2400, 1.1e4
    g = synth.derive_geometry(synth.make_grid(nx, ny, dx0, ns=a.ns))
    st = synth.make_state(g, case="full", seed=20260928, warm=True)
    dc = decomp.per_rank_blocks(nx, ny, 1, "cyclic", a.ns)
    geo = {k: dc.scatter(g[k], 0, fill=(1.0 if k != "uarear" else 0.0)) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")}
    fields = {k: dc.scatter(st[k], 0) for k in evp.FIELDS}
    tm, um = dc.scatter(st["iceTmask"], 0, fill=0), dc.scatter(st["iceUmask"], 0, fill=0)
    metrics = synth.bgrid_fold_metrics(dc, 0, g) if a.ns == "tripole" else None
    scal = synth.evp_scalars(a.ndte)
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(scal, strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"], geo["uarear"],
                      geo["tarea"], keepalive=keep)
    try:
        if metrics is not None:
            core.set_metrics(dxhy=metrics[0], dyhx=metrics[1])
        core.upload(fields, tm, um)
        us = []
        for k in range(a.warmup + a.steps):
            core.subcycle(a.ndte)
            core.sync()
            if k >= a.warmup:
                us.append(core.timings()["loop_ms"] * 1e3 / a.ndte)
        info = core.march_info()
        out = dict(label=a.label or ("other tree" if a.root else "this tree"), ns=a.ns, ndte=a.ndte, warmup=a.warmup,
                   us_per_subcycle=[round(v, 2) for v in us], median=round(float(np.median(us)), 2),
                   march={k: info[k] for k in ("mode", "kpass", "strips", "segments", "seglen") if k in info},
                   band_rows=info.get("band_rows", 0), path=core.describe_path())
        print(json.dumps(out), flush=True)
    finally:
        core.finalize()


if __name__ == "__main__":
    main()
