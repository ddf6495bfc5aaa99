#!/usr/bin/env python3
"""Device time of the calls between the subcycle loop and transport (cice_evp_hip_strocn_t, cice_evp_hip_principal_stress,
cice_evp_hip_cgrid_tail, cice_evp_hip_cgrid_dyn_finish_u + cice_evp_hip_cgrid_strocn_t) on one rank, beside the device-to-host
copies a host that calls them no longer needs and -- as a stand-in nobody should mistake for the reference -- the wall time of
the numpy restatement (tests/tail_ref.py) of the same passes on this machine's CPU.

Each figure: warm-up calls, then the median of --reps calls.  "device" = HIP events on the library's stream around a call whose
output pointers are NULL (kernels and halo steps only); "call" = wall time of the call with its outputs (pageable host arrays).

  python tools/tail_timing.py [--workload s01] [--reps 12] [--numpy]
"""
import argparse
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

PUNY = 1.0e-11


def median_ms(core, call, reps, warm=3):
    """(device ms between the marks, wall ms) of call(), medians."""
    dev, wall = [], []
    for k in range(warm + reps):
        core.sync()
        t0 = time.perf_counter()
        core.mark(0)
        call()
        core.mark(1)
        core.sync()
        t1 = time.perf_counter()
        if k >= warm:
            dev.append(float(core.timings()["marks_ms"]))
            wall.append((t1 - t0) * 1e3)
    return statistics.median(dev), statistics.median(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="s01")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--numpy", action="store_true", help="also time tests/tail_ref.py on the host (numpy, NOT the reference)")
    a = ap.parse_args()
    from cice_amd import decomp, evp, synth
    spec = synth.GRIDS[a.workload]
    nx, ny = spec["nx"], spec["ny"]
    scal = synth.evp_scalars(120)
    null = None

    def report(tag, what, dev, wall):
        print(f"TAIL_TIMING {a.workload} {nx}x{ny} {tag}: {what}: device {dev:.3f} ms, call {wall:.3f} ms", flush=True)

    for ns in ("closed", "tripole"):
        g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns=ns))
        st = synth.make_state(g, case="full", seed=7, warm=True)
        dc = decomp.single_block(nx, ny, "cyclic", ns)
        geo = {k: dc.scatter(g[k], 0, fill=(1.0 if k != "uarear" else 0.0)) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear", "uarea")}
        fields = {k: dc.scatter(st[k], 0) for k in evp.FIELDS}
        tm, um = dc.scatter(st["iceTmask"], 0, fill=0), dc.scatter(st["iceUmask"], 0, fill=0)
        d, keep = evp.make_dims(dc, 0)
        core = evp.EvpHip(d, evp.make_params(scal, strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"], geo["uarear"], geo["tarea"],
                          keepalive=keep)
        try:
            if ns == "tripole":
                m = synth.bgrid_fold_metrics(dc, 0, g)
                core.set_metrics(dxhy=m[0], dyhx=m[1])
            core.upload(fields, tm, um)
            core.subcycle(8)
            if ns == "tripole":
                core.stress_halo()
            z = np.zeros(core.shape)
            fin = core.dyn_finish(z, z)
            core.strocn_t(geo["uarea"], geo["tarea"])
            lib = core.lib
            tag = f"B grid {ns}"
            report(tag, "strocn_t, no outputs", *median_ms(core, lambda: lib.cice_evp_hip_strocn_t(null, null, null, null), a.reps))
            report(tag, "strocn_t, 2 arrays out", *median_ms(core, lambda: core.strocn_t(), a.reps))
            report(tag, "principal_stress, no outputs", *median_ms(core, lambda: lib.cice_evp_hip_principal_stress(C.c_double(PUNY), null, null, null), a.reps))
            report(tag, "principal_stress, 3 arrays out", *median_ms(core, lambda: core.principal_stress(PUNY), a.reps))
            two = {k: np.zeros(core.shape) for k in ("uvel", "vvel")}
            report(tag, "D2H of 2 arrays (strocnxU / strocnyU no longer fetched)", *median_ms(core, lambda: core.download_into(two), a.reps))
            report(tag, "D2H of the 12 stresses (fetch_stresses no longer needed for history)", *median_ms(core, lambda: core.fetch_stresses(), a.reps))
            if a.numpy:
                import tail_ref
                dom, blocks = tail_ref.domain_of_decomp(dc), tail_ref.blocks_of_decomp(dc)
                t0 = time.perf_counter()
                tail_ref.strocn_t(dom, blocks, fin["strocnxU"], fin["strocnyU"], fields["aiU"], geo["uarea"], geo["tarea"])
                t1 = time.perf_counter()
                tail_ref.principal_stress(fields["stressp_1"], fields["stressm_1"], fields["stress12_1"], fields["strength"], PUNY)
                t2 = time.perf_counter()
                print(f"TAIL_TIMING {a.workload} {nx}x{ny} {tag}: numpy restatement on the host (NOT the reference): strocn_t {1e3 * (t1 - t0):.1f} ms, "
                      f"principal_stress {1e3 * (t2 - t1):.1f} ms", flush=True)
        finally:
            core.finalize()

    # C grid, closed
    g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns="closed"))
    cg = synth.cgrid_geometry(g)
    state, inputs, masks = synth.cgrid_state(g, cg, case="full", seed=7, warm=True)
    dc = decomp.single_block(nx, ny, "cyclic", "closed")
    static, state, inputs, masks = synth.cgrid_scatter(dc, 0, cg, state, inputs, masks)
    d, keep = evp.make_dims(dc, 0)
    core = evp.EvpHip(d, evp.make_params(scal, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"], 1.0 / static["uarea"],
                      static["tarea"], keepalive=keep)
    try:
        core.cgrid_set_geometry(static)
        core.cgrid_upload(state, inputs, masks)
        core.cgrid_subcycle(8)
        rng = np.random.default_rng(3)
        shape = core.shape
        uin = dict(cdn_ocnU=np.full(shape, 0.00536), aiU=rng.uniform(0.2, 1.0, shape), uocnU=rng.uniform(-0.1, 0.1, shape),
                   vocnU=rng.uniform(-0.1, 0.1, shape), fmU=rng.uniform(-20.0, 20.0, shape))
        core.cgrid_dyn_finish_u(uin)
        lib = core.lib
        tag = "C grid closed"
        report(tag, "cgrid_tail, no outputs", *median_ms(core, lambda: lib.cice_evp_hip_cgrid_tail(null, null, null, null, C.c_int32(0)), a.reps))
        report(tag, "cgrid_tail, 4 arrays out", *median_ms(core, lambda: core.cgrid_tail(), a.reps))
        report(tag, "cgrid_strocn_t, no outputs", *median_ms(core, lambda: lib.cice_evp_hip_cgrid_strocn_t(null, null), a.reps))
        report(tag, "cgrid_strocn_t, 2 arrays out", *median_ms(core, lambda: core.cgrid_strocn_t(), a.reps))
        report(tag, "cgrid_dyn_finish_u (5 arrays in, 2 inout)", *median_ms(core, lambda: core.cgrid_dyn_finish_u(uin), a.reps))
        tab = (evp._f64p * len(evp.CGRID_FIELDS))()
        two = [np.zeros(shape), np.zeros(shape)]
        tab[evp.CGRID_FIELDS.index("uvel")], tab[evp.CGRID_FIELDS.index("vvel")] = evp._dp(two[0]), evp._dp(two[1])
        report(tag, "D2H of 2 arrays (uvel / vvel no longer fetched for dyn_finish at U)", *median_ms(core, lambda: lib.cice_evp_hip_cgrid_download(tab), a.reps))
        if a.numpy:
            import tail_ref
            dom, blocks = tail_ref.domain_of_decomp(dc), tail_ref.blocks_of_decomp(dc)
            out = core.cgrid_download()
            t0 = time.perf_counter()
            tail_ref.cgrid_tail(dom, blocks, out["strintxE"], out["strintyN"], static)
            t1 = time.perf_counter()
            print(f"TAIL_TIMING {a.workload} {nx}x{ny} {tag}: numpy restatement on the host (NOT the reference): cgrid_tail {1e3 * (t1 - t0):.1f} ms", flush=True)
    finally:
        core.finalize()


if __name__ == "__main__":
    main()
