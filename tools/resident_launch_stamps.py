"""What a launch of the on-chip resident B-grid kernel pays beside its subcycles, piece by piece: the wall-clock stamps (100 MHz)
every wave takes under CICE_EVP_HIP_RES_PROF=1 (test build, 16 x 16 tiles) on the state bench.py's headline runs -- workgroup
start, after the per-CU lock, after the lane tables and masks, after the state loads, the first ring poll matched, the loop's end,
the write-back's end.  A stamp first waits for the wave's outstanding loads and stores, so a span holds what was issued inside it:
the stamped prologue is the SUM of its levels, not their overlap, and with the stamps on every tile takes the per-CU lock.
Usage: python tools/resident_launch_stamps.py [ndte]      (CICE_EVP_HIP_RES_WRITE_ONCE / _LOCK_CAS = 0 / 1: the A/B switches)"""
import os, sys, pathlib
R = str(pathlib.Path(__file__).resolve().parents[1]); sys.path[:0] = [R, R + "/tests", R + "/oracle"]
os.environ["CICE_EVP_HIP_RES_PROF"] = "1"
os.environ.setdefault("CICE_EVP_HIP_RESIDENT", "1")
os.environ.setdefault("CICE_EVP_HIP_RES_LOGW", "4")
import numpy as np
from cice_amd import decomp, evp, synth
ndte = int(sys.argv[1]) if len(sys.argv) > 1 else 8
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
                  geo["tarea"], keepalive=keep, testing=True)
core.upload(fields, tm, um)
for _ in range(3):
    core.subcycle(120)
rows, loops = [], []
for _ in range(7):                      # the stamps of seven launches, each read back before the next
    core.subcycle(ndte)
    core.sync()
    loops.append(core.timings()["loop_ms"] * 1e3)
    s = core.debug_prof_launch().astype(np.int64)
    s = s[s[:, :, 0].min(axis=1) > 0]   # the tiles that ran
    rows.append(s)
tt = core.timings()
core.finalize()
assert tt["resident_fallbacks"] == 0 and tt["tile_variant"] == 2004, tt
names = ["start after the first wave", "per-CU lock", "lane tables, masks", "state loads (+ tile fill, zeroing)", "to the first poll's match",
         "subcycle loop", "write-back"]
print(f"RESULT launch stamps gx1 ndte {ndte}, {len(rows[0])} tiles x 4 waves, 7 launches; event time per launch median {np.median(loops):.2f} us "
      f"(min {min(loops):.2f} max {max(loops):.2f}); us, median over the launches of [median | 90th percentile | max over the waves]")
per = []
for s in rows:
    t = s[:, :, :7].reshape(-1, 7) * 0.01                     # us
    rim = (s[:, :, 7].reshape(-1) & 255) == 0                 # the waves that took chunk 0
    t0 = t[:, 0].min()
    spans = np.column_stack([t[:, 0] - t0] + [t[:, k] - t[:, k - 1] for k in (1, 2, 3)] + [t[:, 4] - t[:, 3], t[:, 5] - t[:, 4], t[:, 6] - t[:, 5]])
    spans[~rim, 4] = np.nan                                   # (the first poll is the rim wave's; an interior wave's stamp is its start)
    q = [np.nanmedian(spans, axis=0), np.nanpercentile(spans, 90, axis=0), np.nanmax(spans, axis=0)]
    per.append(q + [np.array([t[:, 3].max() - t0, t[rim, 4].max() - t0, t[:, 5].max() - t0, t[:, 6].max() - t0, t[:, 5].min() - t0])])
for k, n in enumerate(names):
    med, p90, mx = (np.median([p[j][k] for p in per]) for j in range(3))
    print(f"  {n:36s} {med:8.2f} {p90:8.2f} {mx:8.2f}")
ends = np.median([p[3] for p in per], axis=0)
print(f"  since the first wave's start: last state load landed {ends[0]:.2f}, last first poll matched {ends[1]:.2f}, first / last wave out of the loop "
      f"{ends[4]:.2f} / {ends[2]:.2f}, last write-back landed {ends[3]:.2f}")
