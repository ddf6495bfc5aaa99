#!/usr/bin/env python3
"""N ranks as N processes on ONE GPU exchanging the velocity halo through the mailbox
transport (HIP IPC mapped inboxes + flag handshake), bootstrapped over gloo -- the only
multi-process GPU configuration a 1-GPU box allows (RCCL refuses two ranks on one device).
Each rank compares its sub-domain, bit for bit, with a single-rank run of the whole domain.

  python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
         --master-port 29533 tools/mailbox_2proc.py [--workload gx3] [--ndte 24] [--timing]
"""
import argparse
import os
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
POST_SENTINEL = (7.0, -3.0)         # --post: what dyn_finish is handed in strocnxU / strocnyU
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))      # (--forcing: the numpy restatement of the averages, tests/forcing_layout_ref.py)


TAIL_PUNY = 1.0e-11


def tail_mode(a, dist, rank, world, nx, ny, ns_bnd, g, st, scal):
    """--tail: every rank runs the loop, dyn_finish and the calls after the loop (B grid: principal_stress, strocn_t; --cgrid:
    cgrid_tail, cgrid_dyn_finish_u, cgrid_strocn_t); every output array of every rank, whole blocks, is compared bit for bit with
    the one-rank run of the same state cut into the same blocks.  --cgrid --post: cgrid_deformations and cgrid_dyn_finish (a sentinel in
    every inout array) ahead of them, or alone; --cgrid --prep: the loop's inputs from cice_evp_hip_cgrid_prep on every rank;
    --expect-marched / --expect-marched-fold: the evidence that the loop before these calls ran on that schedule."""
    from cice_amd import decomp, evp, synth
    shape = tuple(int(v) for v in a.shape.split("x")) if a.shape else None
    dcN = decomp.per_rank_blocks(nx, ny, world, "cyclic", ns_bnd, proc_shape=shape)
    if a.blocks_per_rank:
        sx, sy = (int(v) for v in a.blocks_per_rank.split("x"))
        dcN = decomp.Decomp(nx, ny, -(-dcN.block_size_x // sx), -(-dcN.block_size_y // sy), "cyclic", ns_bnd, world, dcN.proc_shape)
    dc1 = decomp.Decomp(nx, ny, dcN.block_size_x, dcN.block_size_y, "cyclic", ns_bnd, 1)
    fold = ns_bnd in ("tripole", "tripoleT")
    rng = np.random.default_rng(41)
    uin_g = dict(cdn_ocnU=np.full((ny, nx), 0.00536), aiU=np.where(rng.uniform(size=(ny, nx)) < 0.2, 0.0, rng.uniform(0.2, 1.0, (ny, nx))),
                 uocnU=rng.uniform(-0.1, 0.1, (ny, nx)), vocnU=rng.uniform(-0.1, 0.1, (ny, nx)), fmU=rng.uniform(-20.0, 20.0, (ny, nx)))

    def bootstrap(core, exchange):
        if exchange:
            blobs = [None] * world
            dist.all_gather_object(blobs, core.halo_export())
            core.halo_import(blobs)

    def run_b(dc, r, exchange):
        stt = dict(st)
        if ns_bnd == "tripoleT":        # velocities as a halo update leaves them: the top row is the fold's image
            for k in ("uvel", "vvel", "uvel_init", "vvel_init"):
                stt[k] = np.array(stt[k], dtype=np.float64, copy=True)
                stt[k][ny - 1, :] = -stt[k][ny - 2, ::-1]
        geo = {k: dc.scatter(g[k], r, fill=(1.0 if k != "uarear" else 0.0)) for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear", "uarea")}
        fields = {k: dc.scatter(stt[k], r) for k in evp.FIELDS}
        tm, um = dc.scatter(stt["iceTmask"], r, fill=0), dc.scatter(stt["iceUmask"], r, fill=0)
        d, keep = evp.make_dims(dc, r)
        core = evp.EvpHip(d, evp.make_params(scal, strict=True), geo["HTE"], geo["HTN"], geo["dxT"], geo["dyT"], geo["uarear"], geo["tarea"],
                          keepalive=keep)
        try:
            bootstrap(core, exchange)
            if exchange and a.maskhalo:
                tmg = np.asarray(stt["iceTmask"]) != 0
                hmg = tmg | np.roll(tmg, 1, 1) | np.roll(tmg, -1, 1)
                hmg[1:] |= tmg[:-1]
                hmg[:-1] |= tmg[1:]
                core.halo_mask(dc.scatter(hmg.astype(np.int32), r, fill=0))
            core.upload(fields, tm, um)
            core.subcycle(a.ndte)
            if fold:
                core.stress_halo()
            out = core.principal_stress(TAIL_PUNY)
            z = np.zeros(core.shape)
            out.update(core.dyn_finish(z, z))
            out.update(core.strocn_t(geo["uarea"], geo["tarea"]))
            return out, core.timings()
        finally:
            core.finalize()

    def run_c(dc, r, exchange):
        cg = synth.cgrid_geometry(g)
        state, inputs, masks = synth.cgrid_state(g, cg, case=a.case, seed=7, warm=True, seabed=True)
        tmg = np.asarray(masks["iceTmask"]) != 0
        static, state, inputs, masks = synth.cgrid_scatter(dc, r, cg, state, inputs, masks)
        d, keep = evp.make_dims(dc, r)
        core = evp.EvpHip(d, evp.make_params(scal, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"], 1.0 / static["uarea"],
                          static["tarea"], keepalive=keep)
        try:
            bootstrap(core, exchange)
            if exchange and a.maskhalo:
                hmg = tmg | np.roll(tmg, 1, 1) | np.roll(tmg, -1, 1)
                hmg[1:] |= tmg[:-1]
                hmg[:-1] |= tmg[1:]
                core.halo_mask(dc.scatter(hmg.astype(np.int32), r, fill=0))
            core.cgrid_set_geometry(static)
            if a.prep:
                t11, st7, prev = synth.cgrid_prep_inputs(g, cg, case=a.case, seed=17)
                vec = ("uocn", "vocn", "ss_tltx", "ss_tlty", "strairxT", "strairyT")
                tb = {k: dc.scatter(v, r, fold=("center", -1.0 if k in vec else 1.0)) for k, v in t11.items()}
                loc = {"umaskCD": "NEcorner", "emask": "Eface", "nmask": "Nface", "fcor_blk": "NEcorner", "fcorE_blk": "Eface", "fcorN_blk": "Nface"}
                static.update({k: dc.scatter(v, r, fill=0, fold=(loc.get(k, "center"), 1.0)) for k, v in st7.items()})
                core.cgrid_set_prep_geometry(static)
                core.cgrid_prep(evp.PrepParams(dt=3600.0, rhoi=917.0, rhos=330.0, gravit=9.80616, dyn_area_min=1e-11, dyn_mass_min=1e-10,
                                               ssh_stress_coupled=0), tb, state, {k: dc.scatter(v, r, fill=0) for k, v in prev.items()})
                core.cgrid_prep_finish(inputs["strength"], a.visc)
            else:
                core.cgrid_upload(state, inputs, masks, visc_method=a.visc)
            core.cgrid_subcycle(a.ndte)
            out = {"_schedule": (core.cgrid_timings(), core.describe_path())}
            if a.post:          # every inout array with the sentinel: the cells no kernel owns keep it
                sent = lambda keys: {k: np.full(core.shape, POST_SENTINEL[0] if "x" in k or k in ("divu", "vort") else POST_SENTINEL[1]) for k in keys}
                tarear = np.where(static["tarea"] > 0, 1.0 / np.where(static["tarea"] > 0, static["tarea"], 1.0), 0.0)
                out.update(core.cgrid_deformations(tarear, prev=sent(("divu", "shear", "vort", "rdg_conv", "rdg_shear"))))
                out.update(core.cgrid_dyn_finish(prev=sent(("strocnxN", "strocnyN", "strocnxE", "strocnyE"))))
            if a.tail:
                out.update(core.cgrid_tail())
                out.update(core.cgrid_dyn_finish_u({k: dc.scatter(v, r) for k, v in uin_g.items()}))
                out.update(core.cgrid_strocn_t())
            dl = core.cgrid_download()
            out["download strintxE"], out["download strintyN"] = dl["strintxE"], dl["strintyN"]
            for k in ("uvelE", "vvelN", "stresspT", "stressmT", "stress12U"):       # the five arrays the schedules keep in two allocations
                out["download " + k] = dl[k]
            return out, core.timings()
        finally:
            core.finalize()

    run = run_c if a.cgrid else run_b
    ref = None
    for turn in range(world):           # (the one-rank run has the GPU to itself: the processes take turns)
        if turn == rank:
            ref, _ = run(dc1, 0, False)
        dist.barrier()
    got, tim = run(dcN, rank, True)
    assert tim["halo_transport"] == "mailbox", tim
    ref_local = {b.gid: b.local for b in dc1.blocks}
    bits = lambda x: np.ascontiguousarray(x).view(np.uint64)
    bad = []
    for k in sorted(q for q in got if not q.startswith("_")):
        if not np.abs(ref[k]).max() > 0:
            bad.append((k, "all zero in the one-rank run"))
        for b in dcN.local_blocks(rank):
            w, h = ref[k][ref_local[b.gid]], got[k][b.local]
            if not np.array_equal(bits(w), bits(h)):
                jj, ii = np.nonzero(bits(w) != bits(h))
                bad.append((k, b.gid, int(jj.size), (int(jj.min()), int(jj.max()), int(ii.min()), int(ii.max())), float(np.nanmax(np.abs(w - h)))))
    zoned = 0
    if a.cgrid and (a.expect_marched or a.expect_marched_fold):
        # every rank with rectangles ran every subcycle of the call but the first after an upload on the schedule, and says so
        cgt, path = got["_schedule"]
        zoned = 1 if cgt["marched_items"] > 0 else 0
        if a.expect_marched:
            ran = cgt["marched_ranks_subcycles"] == a.ndte - 1 and cgt["frame_cells"] > 0 and "zone marched + frame" in path
        else:
            ran = cgt["marched_fold_ranks_subcycles"] == a.ndte - 1 and cgt["fold_frame_cells"] > 0 and "marched zone + fold band + frame" in path
        if zoned and not ran:
            bad.append(("the loop before the calls did not run on the schedule asked for", cgt, path))
    res = [None] * world
    dist.all_gather_object(res, (rank, bad, sorted(q for q in got if not q.startswith("_")), zoned,
                                 got["_schedule"][1] if a.cgrid else "", got["_schedule"][0]["in_alt"] if a.cgrid else 0))
    if rank == 0:
        ok = all(not r[1] for r in res)
        if a.expect_marched or a.expect_marched_fold:
            ok = ok and any(r[3] for r in res)
        print("MAILBOX_2PROC", "OK" if ok else "FAIL", "tail" if a.tail else "post", "cgrid" if a.cgrid else "bgrid", a.workload, f"world={world}", res, flush=True)
        if not ok:
            sys.exit(1)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="gx3")
    ap.add_argument("--ndte", type=int, default=24)
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--shape", default="")          # e.g. 2x1
    ap.add_argument("--blocks-per-rank", default="", help="e.g. 2x2: split every rank's sub-domain into CICE blocks")
    ap.add_argument("--soak", type=int, default=0, help="N more launches of 120 subcycles before the comparison")
    ap.add_argument("--prep", action="store_true",
                    help="start from the primary model state: evp()'s preparation phase on the device on every "
                         "rank (T-grid halos across ranks through the same transport), then the loop")
    ap.add_argument("--maskhalo", action="store_true",
                    help="B grid or --cgrid: hand the loop the masked halo evp() builds when maskhalo_dyn (five-point dilation of "
                         "iceTmask, ice_dyn_evp.F90:739-770); ghost cells outside the mask stay stale, everything else must not change")
    ap.add_argument("--march", action="store_true",
                    help="force the marching kernel on every rank; its ring exchanges and rank agreements go "
                         "through the library's test transport (host buffers + gloo here: RCCL refuses two ranks per device)")
    ap.add_argument("--ref-march-off", action="store_true",
                    help="B grid: the one-rank reference run takes the one-subcycle kernels (CICE_EVP_HIP_MARCH=0 while it is set up and "
                         "run), so that the two sides of the comparison share no marching code")
    ap.add_argument("--all-fields", action="store_true",
                    help="B grid: compare all 12 stresses and strintx / strinty / taubx / tauby, not the usual selection, and everything "
                         "as bit patterns; on a tripoleT grid the velocities are handed over with the top row as the fold's image")
    ap.add_argument("--fused", action="store_true", help="B grid: fused mode (strict = 0) on both sides")
    ap.add_argument("--expect-fold-band", action="store_true",
                    help="with --march on a tripole grid: every rank that holds rows of the fold band must have advanced them by every "
                         "subcycle of the call but a leading single one, the others by none, and describe_path() must name the band")
    ap.add_argument("--expect-march-off", default="",
                    help="with --march: every rank must have stayed off the marching path and give these words as the reason")
    ap.add_argument("--case", default="full")
    ap.add_argument("--cgrid", action="store_true",
                    help="the C-grid subcycle (cice_evp_hip_cgrid_*): ghost cells other ranks own filled through the "
                         "same transport after every producing launch")
    ap.add_argument("--visc", default="avg_zeta")
    ap.add_argument("--fold-ghosts", action="store_true",
                    help="with --cgrid on a tripole grid: also compare the ghost row beyond the fold and the east-west ghost cells "
                         "of row NY with the one-rank run's own ghost cells (its single block has the whole ghost row), and "
                         "report the C grid's schedule")
    ap.add_argument("--expect-resident", action="store_true",
                    help="fail unless the on-chip resident kernel with remote neighbours ran")
    ap.add_argument("--expect-marched", action="store_true",
                    help="with --cgrid: every rank on which the marched kernel has rectangles must have run every subcycle of its last "
                         "call but the first after an upload as 'zone marched + frame' (cgrid_timings: marched_ranks_subcycles), "
                         "and some rank must have rectangles")
    ap.add_argument("--expect-marched-fold", action="store_true",
                    help="with --cgrid on a tripole grid: every rank on which the marched kernel has rectangles must have run every "
                         "subcycle of its last call but the first after an upload as 'marched zone + fold band + frame' (cgrid_timings: "
                         "marched_fold_ranks_subcycles) with frame cells in its rest and say so in describe_path(), and some rank must "
                         "have rectangles")
    ap.add_argument("--forcing", default="",
                    help="with --prep: a forcing layout 'calc_strair,grid_ocn,grid_atm', e.g. 0,C,B "
                         "(cice_evp_hip_set_forcing_layout): the ocean fields and strax / stray at those points")
    ap.add_argument("--wind-ghosts", default="exchange", choices=["exchange", "own"],
                    help="with --forcing and calc_strair 0: strax / stray ghost cells as an exchange would fill them, or "
                         "(own) different on the split run -- the averages must read them as given: compared with the numpy "
                         "restatement on this rank's inputs, and the wind-dependent arrays are not compared with the one-rank run")
    ap.add_argument("--stress-halo", action="store_true",
                    help="B grid: after the loop call stress_halo() on tripole AND tripoleT grids (evp()'s 12 x ice_HaloUpdate_stress "
                         "on the resident stresses; without it only the u-fold form runs)")
    ap.add_argument("--same-blocks-ref", action="store_true",
                    help="B grid: the reference run is ONE rank owning the same blocks as the split run, not one big block: every "
                         "block array of the 12 stresses is then compared whole, ghost ring included, bit for bit")
    ap.add_argument("--report-prep", action="store_true",
                    help="with --prep: run the preparation three times on the same inputs and print every rank's device time of "
                         "the quickest of the last two (the first call also builds its lists), ms")
    ap.add_argument("--deviate", default="",
                    help="RANK:KIND, KIND = TbU (B grid) or TbN (--cgrid): the default configuration (no seabed stress, water == ocean "
                         "current) with that factor 0.7 on ONE ice cell of RANK next to the cut -- that rank must drop the shortcut, "
                         "every other rank must keep it (the test build's read-out), and the result must still be the one-rank run's")
    ap.add_argument("--post", action="store_true",
                    help="--cgrid: after the loop every rank runs cgrid_deformations and cgrid_dyn_finish on its resident state, a sentinel in "
                         "every inout array; whole blocks are compared as bit patterns with the one-rank run cut into the same blocks (alone or "
                         "ahead of --tail's calls; with --prep the loop's inputs come from cgrid_prep; --expect-marched / --expect-marched-fold "
                         "ask for the schedule of the loop before them).  B grid: after the loop (and after --stress-halo) every rank runs deformations and dyn_finish on its resident "
                         "state, dyn_finish with a sentinel in both arrays; compared as bit patterns with the one-rank run on this "
                         "rank's blocks -- the T-cells of the east / north fringe (ghost cells of the block) included, every cell "
                         "neither kernel owns exactly 0 / the sentinel")
    ap.add_argument("--tail", action="store_true",
                    help="both grids: after the loop every rank runs dyn_finish and the calls between the loop and transport (B grid: "
                         "stress_halo on a fold, principal_stress, strocn_t; --cgrid: cgrid_tail, cgrid_dyn_finish_u, cgrid_strocn_t); "
                         "every output array, whole blocks, is compared as bit patterns with the one-rank run of the same state cut "
                         "into the same blocks (--same-blocks-ref is implied); --maskhalo hands the loop a masked halo the calls must not use")
    a = ap.parse_args()
    if (a.expect_marched or a.expect_marched_fold) and not a.cgrid:
        ap.error("--expect-marched / --expect-marched-fold name C-grid schedules: give --cgrid")
    import torch
    import torch.distributed as dist
    from cice_amd import decomp, evp, synth

    rank = int(os.environ["RANK"])
    world = int(os.environ["WORLD_SIZE"])
    os.environ["CICE_EVP_HIP_DEVICE"] = "0"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo", rank=rank, world_size=world)

    if a.workload in synth.GRIDS:
        spec = synth.GRIDS[a.workload]
    else:                                       # "NXxNY" or "NXxNY:tripole": any size (tools/multiproc_sweep.py)
        size, _, bnd = a.workload.partition(":")
        spec = dict(nx=int(size.split("x")[0]), ny=int(size.split("x")[1]), dx0=1.1e5, ns=bnd or "closed")
    nx, ny = spec["nx"], spec["ny"]
    ns_bnd = spec.get("ns", "closed")          # tx1: tripole north boundary (rank layouts with px = 1 only)
    # ("NXxNY:tripoleT": the T-fold -- the same grid as the u-fold's; only the halo rule differs, and the top row is an image)
    g = synth.derive_geometry(synth.make_grid(nx, ny, spec["dx0"], ns=("tripole" if ns_bnd == "tripoleT" else ns_bnd)))
    st = synth.make_state(g, case=(a.case if a.march and not a.cgrid else "full"), seed=7, warm=True)
    if a.all_fields and ns_bnd == "tripoleT" and not a.cgrid:
        # Bit patterns, ghost cells included: hand over velocities as a halo update leaves them, as evp() does.  On the T-fold the top
        # row is the image of the row below, a(i, NY) = -a(NX - i + 1, NY - 1), so a resting land cell shows as -0.0 up there.  The
        # kernels refresh the images of the cells they compute; where a rank's blocks let each computing thread store its own images,
        # the image of a land cell keeps the value it came with -- and a synthetic +0.0 would differ from the one-rank run's -0.0.
        for k in ("uvel", "vvel"):
            st[k] = np.array(st[k], dtype=np.float64, copy=True)
            st[k][ny - 1, :] = -st[k][ny - 2, ::-1]
    pr = synth.make_primary(g, "full", seed=9) if a.prep else None
    scal = synth.evp_scalars(120)
    if a.tail or (a.post and a.cgrid):
        return tail_mode(a, dist, rank, world, nx, ny, ns_bnd, g, st, scal)
    own_wind = bool(a.forcing) and a.wind_ghosts == "own"

    def deviate_cell(ice):
        """--deviate: the global (row, column) of an ice cell of the named rank with a neighbour cell on another rank."""
        who = int(a.deviate.split(":")[0])
        shp = tuple(int(v) for v in a.shape.split("x")) if a.shape else None
        dcx = decomp.per_rank_blocks(nx, ny, world, "cyclic", ns_bnd, proc_shape=shp)
        owner = np.full((ny, nx), -1)
        for b in dcx.blocks:
            owner[b.gj0 - 1:b.gj0 - 1 + b.gny, b.gi0 - 1:b.gi0 - 1 + b.gnx] = b.owner
        edge = (np.roll(owner, 1, axis=1) != who) | (np.roll(owner, -1, axis=1) != who)
        edge[1:] |= owner[:-1] != who
        edge[:-1] |= owner[1:] != who
        jj, ii = np.nonzero((owner == who) & edge & (np.asarray(ice) != 0))
        assert jj.size, "--deviate: no ice cell next to the cut"
        return int(jj[jj.size // 2]), int(ii[jj.size // 2])
    if a.deviate and not a.cgrid:
        assert a.deviate.endswith(":TbU"), a.deviate
        st["TbU"][deviate_cell(st["iceUmask"])] = 0.7
    if a.forcing:
        calc_s, ocn_s, atm_s = a.forcing.split(",")
        layout = (calc_s == "1", ocn_s, atm_s)
        fglob = synth.located_forcing((ny, nx), seed=23)       # global [ny][nx]: values at whatever points the layout names
        cgf = synth.cgrid_geometry(g)

    def apply_forcing(core, dc, r, exchange, tf, area, pm):
        """--forcing on this rank: the layout, the ocean fields and strax / stray at its points (tf updated in place); with
        --wind-ghosts own on the split run, strax / stray ghost cells that no exchange would give.  Returns the mismatches
        of the wind averages against the restatement on this rank's own inputs (checked after the preparation)."""
        from forcing_layout_ref import GRID_LOC, x2y
        calc, ocn, atm = layout
        (ou, ov), (au, av) = GRID_LOC[ocn], GRID_LOC[atm]
        where = {"T": "center", "U": "NEcorner", "E": "Eface", "N": "Nface"}
        for k, loc in (("uocn", ou), ("vocn", ov), ("ss_tltx", ou), ("ss_tlty", ov)):
            tf[k] = np.array(dc.scatter(fglob[k], r, fold=(where[loc], -1.0)), dtype=np.float64, order="C", copy=True)
        plain = {}
        for k, loc in (("strax", au), ("stray", av)):
            v = np.array(dc.scatter(fglob[k], r, fold=(where[loc], -1.0)), dtype=np.float64, order="C", copy=True)
            plain[k] = v.copy()
            if exchange and own_wind:
                for b in dc.local_blocks(r):
                    ring = np.ones(v[b.local].shape, dtype=bool)
                    ring[1:1 + b.gny, 1:1 + b.gnx] = False
                    v[b.local][ring] = 1.5 * v[b.local][ring] + 0.125
            tf[k] = v
        geo = {k: dc.scatter(cgf[k], r, fill=(1.0 if k.endswith("area") else 0.0),
                             fold=({"earea": "Eface", "epm": "Eface", "narea": "Nface", "npm": "Nface"}.get(k, "NEcorner"), 1.0))
               for k in ("earea", "narea", "uvm", "epm", "npm")}
        core.set_forcing_layout(calc, ocn, atm, **geo)
        for k, loc in (("E", "earea"), ("N", "narea")):
            area.setdefault(k, geo[loc])
        for k, m in (("U", "uvm"), ("E", "epm"), ("N", "npm")):
            pm.setdefault(k, geo[m])
        if not (exchange and own_wind) or calc:
            return lambda fetch, targets: []
        blocks = [(b.ilo, b.ihi, b.jlo, b.jhi) for b in dc.local_blocks(r)]

        def check(fetch, targets):
            bad = []
            for name, key, src, dst in ((targets[0], "strax", au, targets[0][-1]), (targets[1], "stray", av, targets[1][-1])):
                want = x2y("F", tf[key], src, dst, area, pm, blocks)
                asif = x2y("F", plain[key], src, dst, area, pm, blocks)
                got = fetch(name)
                if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
                    bad.append((name + " vs restatement (own ghost cells)", int((got != want).sum())))
                if np.array_equal(want, asif):
                    bad.append((name + ": the changed ghost cells are not read", 0))
            return bad
        return check

    def run_cgrid(dc, r, exchange):
        cg = synth.cgrid_geometry(g)
        state, inputs, masks = synth.cgrid_state(g, cg, case=a.case, seed=7, warm=True, seabed=not a.deviate)
        if a.deviate:
            assert a.deviate.endswith(":TbN"), a.deviate
            inputs["TbN"][deviate_cell(masks["iceNmask"])] = 0.7
        tmg = np.asarray(masks["iceTmask"]) != 0          # global: the halo mask of the C-grid loop
        hmg = tmg | np.roll(tmg, 1, 1) | np.roll(tmg, -1, 1)
        hmg[1:] |= tmg[:-1]
        hmg[:-1] |= tmg[1:]
        static, state, inputs, masks = synth.cgrid_scatter(dc, r, cg, state, inputs, masks)
        d, keep = evp.make_dims(dc, r)
        core = evp.EvpHip(d, evp.make_params(scal, strict=True), static["dyE"], static["dxN"], static["dxT"], static["dyT"],
                          1.0 / static["uarea"], static["tarea"], keepalive=keep, testing=(True if a.forcing or a.deviate else None))
        try:
            if exchange:
                blobs = [None] * world
                dist.all_gather_object(blobs, core.halo_export())
                core.halo_import(blobs)
            hm = dc.scatter(hmg.astype(np.int32), r, fill=0)
            if exchange and a.maskhalo:
                core.halo_mask(hm)
            core.cgrid_set_geometry(static)
            if a.prep:
                # the preparation phase on the device on every rank: T-grid halos, E / N velocities and their averages
                # across ranks through the transport.  Ghost cells of the fields the preparation halo-updates itself are
                # handed over WRONG on purpose (aice, vice, vsno are read as given: ice_dyn_evp.F90:362-371)
                t11, st7, prev = synth.cgrid_prep_inputs(g, cg, case=a.case, seed=17)
                vec = ("uocn", "vocn", "ss_tltx", "ss_tlty", "strairxT", "strairyT")
                tb = {k: np.array(dc.scatter(v, r, fold=("center", -1.0 if k in vec else 1.0)), dtype=np.float64, order="C", copy=True)
                      for k, v in t11.items()}
                for k in tb:
                    if k in ("aice", "vice", "vsno"):
                        continue
                    for b in dc.local_blocks(r):
                        ring = np.ones(tb[k][b.local].shape, dtype=bool)
                        ring[1:1 + b.gny, 1:1 + b.gnx] = False
                        tb[k][b.local][ring] = 1.5 * tb[k][b.local][ring] + 0.125
                loc = {"umaskCD": "NEcorner", "emask": "Eface", "nmask": "Nface", "fcor_blk": "NEcorner", "fcorE_blk": "Eface", "fcorN_blk": "Nface"}
                static.update({k: dc.scatter(v, r, fill=0, fold=(loc.get(k, "center"), 1.0)) for k, v in st7.items()})
                prevb = {k: dc.scatter(v, r, fill=0) for k, v in prev.items()}
                core.cgrid_set_prep_geometry(static)
                pp = evp.PrepParams(dt=3600.0, rhoi=917.0, rhos=330.0, gravit=9.80616, dyn_area_min=1e-11, dyn_mass_min=1e-10,
                                    ssh_stress_coupled=0)
                wind_check = None
                if a.forcing:
                    area = {"T": static["tarea"], "U": static["uarea"], "E": static["earea"], "N": static["narea"]}
                    pm = {"T": static["hm"], "U": static["uvm"], "E": static["epm"], "N": static["npm"]}
                    wind_check = apply_forcing(core, dc, r, exchange, tb, area, pm)
                newm = core.cgrid_prep(pp, tb, state, prevb)
                if a.report_prep:
                    ms = []
                    for _ in range(2):
                        newm = core.cgrid_prep(pp, tb, state, prevb)
                        ms.append(core.cgrid_timings()["prep_ms"])
                    print(f"PREP_MS cgrid {a.workload} {'split ' + a.shape if exchange else 'one rank'} rank {r}: {min(ms):.4f}", flush=True)
                wind_bad = wind_check(core.cgrid_fetch, ("strairxE", "strairyN")) if wind_check else []
                if exchange and a.maskhalo:
                    pass                  # (the mask above was built from the synthetic loop masks: not used together with --prep)
                core.cgrid_prep_finish(inputs["strength"], a.visc)
            else:
                core.cgrid_upload(state, inputs, masks, visc_method=a.visc)
            core.cgrid_subcycle(a.ndte)
            want_marched = a.ndte - 1            # (the first subcycle after an upload still reads the caller's averages)
            t = None
            if a.timing:
                want_marched = 7
                core.cgrid_sync()
                if exchange:
                    dist.barrier()
                t0 = time.perf_counter()
                for _ in range(3):
                    core.cgrid_subcycle(40)
                core.cgrid_sync()
                t = (time.perf_counter() - t0) / 120 * 1e6
                core.cgrid_subcycle(7)
            out = core.cgrid_download()
            out["_halomask"] = hm
            if a.deviate:
                out["_flags"] = core.call_flags()
            if a.expect_marched and exchange:
                out["_marched"] = (core.cgrid_timings(), want_marched, core.describe_path().rpartition("; ")[2])
            if a.expect_marched_fold and exchange:
                out["_marched_fold"] = (core.cgrid_timings(), want_marched, core.describe_path())
            if a.fold_ghosts:
                cgt = core.cgrid_timings()
                out["_schedule"] = (bool(cgt["fold_exchange"]), int(cgt["fold_ranks"]), core.describe_path().rpartition("; ")[2])
            if a.prep:                    # what the preparation produced, too
                for k in ("aiE", "forcexE", "emassdti", "aiN", "forceyN", "uocnN", "uvelE_init") + (
                        ("uocnE", "vocnE", "vocnN", "strairxE", "strairyN") if a.forcing else ()):
                    out["prep_" + k] = core.cgrid_fetch(k)
                out["_wind_bad"] = wind_bad
                for k, v in newm.items():
                    out["prep_" + k] = v.astype(np.float64)
            return out, core.timings(), t
        finally:
            core.finalize()

    if a.cgrid:
        ref = None
        for turn in range(world):
            if turn == rank:
                ref, _, _ = run_cgrid(decomp.single_block(nx, ny, "cyclic", ns_bnd), 0, False)
            dist.barrier()
        shape = tuple(int(v) for v in a.shape.split("x")) if a.shape else None
        dcN = decomp.per_rank_blocks(nx, ny, world, "cyclic", ns_bnd, proc_shape=shape)
        if a.blocks_per_rank:
            sx, sy = (int(v) for v in a.blocks_per_rank.split("x"))
            dcN = decomp.Decomp(nx, ny, -(-dcN.block_size_x // sx), -(-dcN.block_size_y // sy), "cyclic", ns_bnd, world,
                                dcN.proc_shape)
        got, tim, t_us = run_cgrid(dcN, rank, True)
        assert tim["halo_transport"] == "mailbox", tim
        exchanged = ("uvelE", "vvelE", "uvelN", "vvelN", "uvel", "vvel", "stresspT", "stressmT", "stress12U", "zetax2T",
                     "etax2T", "shearU")
        bad = list(got.get("_wind_bad", []))
        # (--wind-ghosts own: what depends on the wind stress is checked against the restatement above, not the one-rank run)
        wind_dep = set(evp.CGRID_FIELDS) | {"prep_forcexE", "prep_forceyN", "prep_strairxE", "prep_strairyN"} if own_wind else set()
        for k in list(evp.CGRID_FIELDS) + [q for q in ref if q.startswith("prep_")]:
            if k in wind_dep:
                continue
            want = dcN.scatter(ref[k][0][1:-1, 1:-1], rank)
            for b in dcN.local_blocks(rank):
                w = want[b.local][1:1 + b.gny, 1:1 + b.gnx]
                h = got[k][b.local][1:1 + b.gny, 1:1 + b.gnx]
                if not np.array_equal(w, h):
                    bad.append((k, int((w != h).sum()), float(np.abs(w - h).max())))
                if k in exchanged:      # ghost cells that mirror a cell (all but those beyond the closed north / south edge)
                    j0 = 1 if b.gj0 == 1 else 0
                    j1 = b.gny + 1 if b.gj0 + b.gny - 1 == ny else b.gny + 2
                    w2 = want[b.local][j0:j1, 0:b.gnx + 2]
                    h2 = got[k][b.local][j0:j1, 0:b.gnx + 2]
                    if a.maskhalo:      # ghost cells outside the mask are not refreshed (stale, as in the reference)
                        keep = got["_halomask"][b.local][j0:j1, 0:b.gnx + 2] != 0
                        w2, h2 = w2[keep], h2[keep]
                    if not np.array_equal(w2, h2):
                        bad.append((k + " ghosts", int((w2 != h2).sum()), float(np.abs(w2 - h2).max())))
                if a.fold_ghosts and k in exchanged and b.gj0 + b.gny - 1 == ny and ns_bnd in ("tripole", "tripoleT"):
                    # the one-rank run's own ghost cells: row NY+1 beyond the fold, and the east-west ghost cells of row NY
                    cols = (np.arange(b.gi0 - 1, b.gi0 + b.gnx + 1) - 1) % nx + 1        # global columns of the local ones
                    r1 = ref[k][0]
                    for jl, jr, sel in ((b.gny + 1, ny + 1, slice(None)), (b.gny, ny, [0, b.gnx + 1])):
                        w3 = r1[jr, cols][sel]
                        h3 = got[k][b.local][jl, 0:b.gnx + 2][sel]
                        if a.maskhalo:
                            keep3 = got["_halomask"][b.local][jl, 0:b.gnx + 2][sel] != 0
                            w3, h3 = w3[keep3], h3[keep3]
                        if not np.array_equal(w3.view(np.int64), h3.view(np.int64)):
                            bad.append((k + (" fold ghost row" if jr > ny else " row NY ghosts"), int((w3 != h3).sum())))
        if a.deviate:       # this rank's verdict: the shortcut dropped on the named rank (and in the one-rank run), kept on the others
            hit = rank == int(a.deviate.split(":")[0])
            fl, fl1 = got["_flags"], ref["_flags"]
            if (fl["cgrid"] & 7) != (evp.CG_TB_NONZERO if hit else 0) or fl["cgrid_fast"] == hit or fl1["cgrid_fast"]:
                bad.append(("flag word of this rank / of the one-rank run", fl, fl1))
        zoned = 0
        if a.expect_marched:
            cgt, want_marched, sched = got["_marched"]
            zoned = 1 if cgt["marched_items"] > 0 else 0
            if zoned and not (cgt["marched_ranks_subcycles"] == want_marched and cgt["frame_cells"] > 0 and "zone marched + frame" in sched):
                bad.append(("the marched kernel did not run beside the frame", cgt["marched_ranks_subcycles"], want_marched, cgt["marched_items"], sched))
        if a.expect_marched_fold:
            cgt, want_marched, path = got["_marched_fold"]
            zoned = 1 if cgt["marched_items"] > 0 else 0
            if zoned and not (cgt["marched_fold_ranks_subcycles"] == want_marched and cgt["fold_frame_cells"] > 0 and
                              "marched zone + fold band + frame" in path):
                bad.append(("the marched kernel did not run beside the fold band and the frame", cgt["marched_fold_ranks_subcycles"], want_marched,
                            cgt["marched_items"], path))
        res = [None] * world
        dist.all_gather_object(res, (rank, bad, t_us, tim["halo_send_cells"]) + ((got["_schedule"],) if a.fold_ghosts else ()) +
                               ((("fast", got["_flags"]["cgrid_fast"]),) if a.deviate else ()) +
                               (((zoned, got["_marched"][0]["marched_cells"], got["_marched"][0]["frame_cells"]),) if a.expect_marched else ()) +
                               (((zoned, got["_marched_fold"][0]["marched_cells"], got["_marched_fold"][0]["fold_frame_cells"],
                                  got["_marched_fold"][0]["marched_fold_exchange"]),) if a.expect_marched_fold else ()))
        if rank == 0:
            ok = all(not r[1] for r in res)
            if a.expect_marched or a.expect_marched_fold:
                ok = ok and any(r[-1][0] for r in res)
            if a.deviate:       # the ranks differ
                ok = ok and len({r[4][1] for r in res}) == 2
            print("MAILBOX_2PROC", "OK" if ok else "FAIL", "cgrid", a.workload, f"world={world}", res, flush=True)
            if not ok:
                sys.exit(1)
        dist.destroy_process_group()
        return

    def run(dc, r, exchange):
        geo = {k: dc.scatter(g[k], r, fill=(1.0 if k != "uarear" else 0.0))
               for k in ("HTE", "HTN", "dxT", "dyT", "tarea", "uarear")}
        fields = {k: dc.scatter(st[k], r) for k in evp.FIELDS}
        tm = dc.scatter(st["iceTmask"], r, fill=0)
        um = dc.scatter(st["iceUmask"], r, fill=0)
        d, keep = evp.make_dims(dc, r)
        # (the test transport of --march exists in the test build only; everything else runs the product library unless the
        # environment holds one of the test build's switches)
        core = evp.EvpHip(d, evp.make_params(scal, strict=not a.fused), geo["HTE"], geo["HTN"], geo["dxT"],
                          geo["dyT"], geo["uarear"], geo["tarea"], keepalive=keep, testing=(True if a.march or a.forcing or a.deviate else None))
        try:
            if exchange:
                blobs = [None] * world
                dist.all_gather_object(blobs, core.halo_export())
                core.halo_import(blobs)
            hm = None
            if exchange and a.maskhalo:
                # ice_HaloMask as evp() builds it when maskhalo_dyn: the five-point dilation of iceTmask (ice_dyn_evp.F90:739-770)
                tmg = np.asarray(st["iceTmask"]) != 0
                hmg = tmg | np.roll(tmg, 1, 1) | np.roll(tmg, -1, 1)
                hmg[1:] |= tmg[:-1]
                hmg[:-1] |= tmg[1:]
                hm = dc.scatter(hmg.astype(np.int32), r, fill=0)
                core.halo_mask(hm)
            if exchange and a.march:
                def xchg(ranks, ns, nr, send, recv):
                    ops, so, ro = [], 0, 0
                    keepalive = []
                    for q, n_s, n_r in zip(ranks, ns, nr):
                        if q == rank:                       # (self-exchange across a seam this rank spans)
                            recv[ro:ro + n_r] = send[so:so + n_s]
                        else:
                            if n_s:
                                ts = torch.from_numpy(np.ascontiguousarray(send[so:so + n_s]))
                                keepalive.append(ts)
                                ops.append(dist.P2POp(dist.isend, ts, q))
                            if n_r:
                                tr = torch.empty(n_r, dtype=torch.float64)
                                keepalive.append((tr, ro, n_r))
                                ops.append(dist.P2POp(dist.irecv, tr, q))
                        so += n_s
                        ro += n_r
                    if ops:
                        for w in dist.batch_isend_irecv(ops):
                            w.wait()
                    for item in keepalive:
                        if isinstance(item, tuple):
                            tr, o, n = item
                            recv[o:o + n] = tr.numpy()

                def reduce(op, v):
                    tt = torch.tensor([v], dtype=torch.int64)
                    dist.all_reduce(tt, op=dist.ReduceOp.MIN if op == 0 else dist.ReduceOp.MAX)
                    return int(tt.item())
                core.set_test_transport(xchg, reduce)
            if a.prep:
                sc = lambda x, fill=0.0: dc.scatter(np.ascontiguousarray(x), r, fill=fill)
                static = {k: sc(v, (1.0 if k in ("tarea", "uarea") else 0)) for k, v in pr["static"].items()}
                core.set_prep_geometry(*[static[k] for k in ("tmask", "umask", "hm", "tarea", "uarea", "fcor_blk")])
                pp = evp.PrepParams(dt=3600.0, rhoi=917.0, rhos=330.0, gravit=9.80616, dyn_area_min=1e-11,
                                    dyn_mass_min=1e-10, ssh_stress_coupled=0)
                # T-grid fields the preparation halo-updates itself are handed over with WRONG ghost cells on purpose
                # (aice, vice, vsno are read as given, ice_dyn_evp.F90:362-371)
                tf = {k: np.array(sc(v), dtype=np.float64, order="C", copy=True) for k, v in pr["t"].items()}
                for k in tf:
                    if k in ("aice", "vice", "vsno"):
                        continue
                    for b in dc.local_blocks(r):
                        ring = np.ones(tf[k][b.local].shape, dtype=bool)
                        ring[1:1 + b.gny, 1:1 + b.gnx] = False
                        tf[k][b.local][ring] = 1.5 * tf[k][b.local][ring] + 0.125
                wind_check = None
                if a.forcing:
                    area = {"T": static["tarea"], "U": static["uarea"]}
                    pm = {"T": static["hm"]}
                    wind_check = apply_forcing(core, dc, r, exchange, tf, area, pm)
                tmk, umk, _ = core.prep(pp, tf, {k: sc(v) for k, v in pr["state"].items()})
                if a.report_prep:
                    ms = []
                    for _ in range(2):
                        tmk, umk, _ = core.prep(pp, tf, {k: sc(v) for k, v in pr["state"].items()})
                        ms.append(core.timings()["prep_ms"])
                    print(f"PREP_MS bgrid {a.workload} {'split ' + a.shape if exchange else 'one rank'} rank {r}: {min(ms):.4f}", flush=True)
                core.set_strength(fields["strength"])
                extra = {k: core.prep_fetch(k) for k in ("forcexU", "umassdti", "uvel_init", "aiU") + (
                    ("uocnU", "vocnU", "strairxU", "strairyU") if a.forcing else ())}
                extra["_wind_bad"] = wind_check(core.prep_fetch, ("strairxU", "strairyU")) if wind_check else []
                extra["iceTmask"] = tmk.astype(np.float64)
            else:
                core.upload(fields, tm, um)
                extra = {"_flags": core.call_flags()["bgrid"]} if a.deviate else {}
            core.subcycle(a.ndte)
            t = None
            if a.timing:      # the same launches in the reference run: back-to-back loops are compared too
                core.sync()
                if exchange:
                    dist.barrier()
                t0 = time.perf_counter()
                for _ in range(5):
                    core.subcycle(120)
                core.sync()
                t = (time.perf_counter() - t0) / 600 * 1e6
                core.subcycle(7)          # an odd count: the record-buffer parity flips between launches
            for _ in range(a.soak):
                core.subcycle(120)
            if (ns_bnd == "tripole" and not a.timing) or (a.stress_halo and ns_bnd in ("tripole", "tripoleT")):
                core.stress_halo()          # evp()'s 12 x ice_HaloUpdate_stress on the resident stresses (any rank layout)
            out = core.download()
            out.update(extra)
            if a.post:
                core.set_post_geometry(*[dc.scatter(g[k], r, fill=(1.0 if k != "tarear" else 0.0)) for k in ("dxU", "dyU", "tarear")])
                out.update({"post_" + k: v for k, v in core.deformations().items()})
                out.update({"post_" + k: v for k, v in core.dyn_finish(np.full(core.shape, POST_SENTINEL[0]),
                                                                       np.full(core.shape, POST_SENTINEL[1])).items()})
            out["_march"] = core.march_info()
            out["_path"] = core.describe_path()
            out["_halomask"] = hm
            return out, core.timings(), t
        finally:
            core.finalize()

    # The single-rank reference run assumes it has the GPU to itself (its resident kernel needs all its
    # tiles co-resident; a tx1-sized domain fills the chip): the processes take turns.
    shape = tuple(int(v) for v in a.shape.split("x")) if a.shape else None
    dcN = decomp.per_rank_blocks(nx, ny, world, "cyclic", ns_bnd, proc_shape=shape)
    if a.blocks_per_rank:
        sx, sy = (int(v) for v in a.blocks_per_rank.split("x"))
        dcN = decomp.Decomp(nx, ny, -(-dcN.block_size_x // sx), -(-dcN.block_size_y // sy), "cyclic", ns_bnd, world,
                            dcN.proc_shape)
    # (--same-blocks-ref: the split run's blocks, all on one rank -- same block grid, same block ids)
    dc1 = (decomp.Decomp(nx, ny, dcN.block_size_x, dcN.block_size_y, "cyclic", ns_bnd, 1) if a.same_blocks_ref
           else decomp.single_block(nx, ny, "cyclic", ns_bnd))
    ref = None
    for turn in range(world):
        if turn == rank:
            was = os.environ.get("CICE_EVP_HIP_MARCH")
            if a.ref_march_off:
                os.environ["CICE_EVP_HIP_MARCH"] = "0"
            try:
                ref, _, _ = run(dc1, 0, False)
            finally:
                if a.ref_march_off:
                    os.environ.pop("CICE_EVP_HIP_MARCH")
                    if was is not None:
                        os.environ["CICE_EVP_HIP_MARCH"] = was
            if a.ref_march_off and ref["_march"]["mode"] != 0:
                raise SystemExit(f"--ref-march-off: the reference run took the marching path: {ref['_march']}")
        dist.barrier()
    ref_global = {}

    def refg(k):            # the reference run's field on the global grid (interior cells of its blocks)
        if k not in ref_global:
            ref_global[k] = dc1.gather({0: ref[k]})
        return ref_global[k]
    got, tim, t_us = run(dcN, rank, True)
    assert tim["halo_transport"] == "mailbox", tim
    bad = list(got.get("_wind_bad", []))
    if a.same_blocks_ref:
        # the 12 stresses, every block array whole: what the loop and the symmetrisation leave in the ghost ring included
        ref_local = {b.gid: b.local for b in dc1.blocks}
        for k in evp.FIELDS[:12]:
            for b in dcN.local_blocks(rank):
                w, h = ref[k][ref_local[b.gid]], got[k][b.local]
                if not np.array_equal(w.view(np.uint64), h.view(np.uint64)):
                    bad.append((k + " whole block", b.gid, int((w.view(np.uint64) != h.view(np.uint64)).sum())))
    if a.deviate:           # this rank's verdict: TBU_ZERO dropped on the named rank (and in the one-rank run), kept on the others
        hit = rank == int(a.deviate.split(":")[0])
        if bool(got["_flags"] & evp.F_TBU_ZERO) == hit or not got["_flags"] & evp.F_WATER_IS_OCN or ref["_flags"] & evp.F_TBU_ZERO:
            bad.append(("flags of this rank / of the one-rank run", hex(got["_flags"]), hex(ref["_flags"])))
    if a.march:
        mi = got["_march"]
        if a.expect_march_off:
            if not (mi["mode"] == 0 and mi["passes"] == 0 and "marching path: off -- " in got["_path"] and a.expect_march_off in got["_path"]):
                bad.append(("marching kernel: not off, or for another reason", mi, got["_path"]))
        elif a.deviate:     # the ranks' verdicts differ: every rank declines the call together and takes the one-subcycle kernel
            if not (mi["mode"] == 1 and not mi["last_call"] and mi["declined"] == 1):
                bad.append(("marching kernel: the call was not declined", mi))
        elif not (mi["mode"] == 1 and mi["last_call"] and mi["declined"] == 0 and mi["passes"] > 0):
            bad.append(("marching kernel did not run", mi))
        if a.expect_fold_band:
            holds = any(b.gj0 + b.gny - 1 == ny for b in dcN.local_blocks(rank))
            led = 1 if a.ndte % mi["kpass"] == 1 else 0
            if holds != (mi["band_rows"] > 0) or mi["band_subcycles"] != (a.ndte - led if holds else 0) or "fold band" not in got["_path"] \
                    or f"of {world} ranks" not in got["_path"]:
                bad.append(("fold band: rows, subcycles or wording", holds, mi, got["_path"]))
        want_ring = "direct stores (HIP IPC)" if os.environ.get("CICE_EVP_HIP_MARCH_DIRECT") == "1" and os.environ.get("CICE_EVP_HIP_MARCH_OVERLAP", "0") != "1" else None
        if want_ring and mi["ring"] != want_ring:
            bad.append(("ring of the marching path not exchanged through the inboxes", mi))
    wind_dep = {"uvel", "vvel", "stressp_1", "stressm_3", "stress12_4", "strintxU", "taubyU", "forcexU", "strairxU",
                "strairyU"} if own_wind else set()      # (--wind-ghosts own: checked against the restatement instead)
    same = (lambda p, q: np.array_equal(p.view(np.uint64), q.view(np.uint64))) if a.all_fields else np.array_equal      # (bit patterns)
    more = tuple(k for k in tuple(evp.FIELDS[:12]) + ("strintxU", "strintyU", "taubxU", "taubyU")
                 if k not in ("stressp_1", "stressm_3", "stress12_4", "strintxU", "taubyU", "taubxU")) if a.all_fields else ()
    for k in ("uvel", "vvel", "stressp_1", "stressm_3", "stress12_4", "strintxU", "taubyU", "taubxU",
              "forcexU", "umassdti", "uvel_init", "aiU", "iceTmask", "uocnU", "vocnU", "strairxU", "strairyU") + more:
        if k not in got or k in wind_dep:
            continue
        want = dcN.scatter(refg(k), rank)
        for b in dcN.local_blocks(rank):
            w = want[b.local][1:1 + b.gny, 1:1 + b.gnx]
            h = got[k][b.local][1:1 + b.gny, 1:1 + b.gnx]
            if not same(np.ascontiguousarray(w), np.ascontiguousarray(h)):
                jj, ii = np.nonzero(w != h)          # (where: global rows and columns, 1-based, of the cells that differ)
                where = (int(jj.min()) + b.gj0, int(jj.max()) + b.gj0, int(ii.min()) + b.gi0, int(ii.max()) + b.gi0, int(jj.size)) if jj.size else ()
                bad.append((k, float(np.abs(w - h).max())) + ((where,) if a.all_fields else ()))
        if k.startswith("stress") and ns_bnd == "tripole" and not a.timing:
            # the ghost row beyond the fold after the symmetrisation: the partner array's top row, mirrored (centre rule)
            fam, q = k.rsplit("_", 1)
            partner = f"{fam}_{((int(q) - 1) ^ 2) + 1}"
            wantp = dcN.scatter(refg(partner), rank, fold=("center", 1.0))
            for b in dcN.local_blocks(rank):
                if b.gj0 + b.gny - 1 != ny:
                    continue
                w = wantp[b.local][b.gny + 1, :b.gnx + 2]
                h = got[k][b.local][b.gny + 1, :b.gnx + 2]
                if not np.array_equal(w, h):
                    bad.append((k + " fold ghost row", int((w != h).sum()), float(np.abs(w - h).max())))
        if k in ("uvel", "vvel"):      # ghost cells too (post-condition of the drop-in boundary)
            w2, h2 = want.copy(), got[k].copy()
            if ns_bnd in ("tripole", "tripoleT"):    # (scatter() does not know the fold: leave the folded ghost row out)
                for b in dcN.local_blocks(rank):
                    if b.gj0 + b.gny - 1 == ny:           # (row gny + 1: a padded block has spare rows above it)
                        w2[b.local][b.gny + 1:, :] = 0.0
                        h2[b.local][b.gny + 1:, :] = 0.0
            if got.get("_halomask") is not None:     # ghost cells outside the mask are not refreshed (stale, as in the reference)
                for b in dcN.local_blocks(rank):
                    stale = got["_halomask"][b.local] == 0
                    stale[1:1 + b.gny, 1:1 + b.gnx] = False
                    w2[b.local][stale] = 0.0
                    h2[b.local][stale] = 0.0
            if not same(w2, h2):
                # (where, under --all-fields: the first few as (local block, row, column, wanted, got) -- a sign of zero shows in the reprs)
                nb, jj, ii = np.nonzero(w2.view(np.uint64) != h2.view(np.uint64)) if a.all_fields else ((), (), ())
                first = [(int(q), int(j), int(i), repr(float(w2[q, j, i])), repr(float(h2[q, j, i]))) for q, j, i in list(zip(nb, jj, ii))[:4]]
                bad.append((k + " ghosts", float(np.abs(w2 - h2).max())) + ((len(jj), first) if a.all_fields else ()))
    if a.post:
        bits = lambda x: np.ascontiguousarray(x).view(np.uint64)
        moved = 0
        for k in ("divu", "shear", "vort", "rdg_conv", "rdg_shear", "strocnxU", "strocnyU"):
            want = dcN.scatter(refg("post_" + k), rank)
            h_all = got["post_" + k]
            finish = k.startswith("strocn")
            rest = POST_SENTINEL[0 if k == "strocnxU" else 1] if finish else 0.0
            for b in dcN.local_blocks(rank):
                # deformations: dyn_prep2's T list, ilo .. ihi + 1 x jlo .. jhi + 1 -- the fringe cells are ghost cells of this block and
                # cells of the one-rank run's block (scatter() wraps the cyclic seam); dyn_finish: the block's own U-cells
                n1 = 0 if finish else 1
                w = want[b.local][1:1 + b.gny + n1, 1:1 + b.gnx + n1].copy()
                h = h_all[b.local][1:1 + b.gny + n1, 1:1 + b.gnx + n1]
                top = b.gj0 + b.gny - 1 == ny
                if top and not finish and ns_bnd in ("tripole", "tripoleT"):
                    # the row beyond the fold: the one-rank run's own ghost row (scatter() does not know the fold and leaves 0 there,
                    # which is right beyond a closed boundary: no ice, nothing written)
                    cols = (np.arange(b.gi0, b.gi0 + b.gnx + 1) - 1) % nx + 1
                    w[b.gny, :] = ref["post_" + k][0][ny + 1, cols]
                if not np.array_equal(bits(w), bits(h)):
                    jj, ii = np.nonzero(bits(w) != bits(h))
                    bad.append(("post " + k, b.gid, int(jj.size), (int(jj.min()) + b.gj0, int(jj.max()) + b.gj0, int(ii.min()) + b.gi0, int(ii.max()) + b.gi0),
                                float(np.abs(w - h).max())))
                other = np.ones(h_all[b.local].shape, dtype=bool)
                other[1:1 + b.gny + n1, 1:1 + b.gnx + n1] = False
                if not (h_all[b.local][other] == rest).all():
                    bad.append(("post " + k + f": a cell the kernel does not own is not {rest}", b.gid, int((h_all[b.local][other] != rest).sum())))
                if not finish:
                    moved += int((h[:, b.gnx] != 0).sum()) + int((h[b.gny, :] != 0).sum())
                elif (h == rest).all() or not (h == rest).any():
                    bad.append(("post " + k + ": the sentinel survives everywhere or nowhere inside the block", b.gid))
        if moved == 0:
            bad.append(("post: nothing on the fringe cells of this rank's blocks",))
    res = [None] * world
    dist.all_gather_object(res, (rank, bad, t_us, tim["launches_per_subcycle"], tim["tile_variant"]) +
                           ((hex(got["_flags"]),) if a.deviate else ()))
    if rank == 0:
        ok = all(not r[1] for r in res)
        if a.deviate:           # the ranks differ
            ok = ok and len({r[5] for r in res}) == 2
        if a.expect_resident:
            ok = ok and all(r[4] >= 2000 for r in res)
        print("MAILBOX_2PROC", "OK" if ok else "FAIL", a.workload, f"world={world}", res, flush=True)
        if not ok:
            sys.exit(1)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
