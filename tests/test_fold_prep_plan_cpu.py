"""CPU (gloo): the tripoleT stress symmetrisation with the top row on several ranks (cice_amd/csrc/fold_prep_plan.cpp).

Every rank builds its plan from the global block table through the C ABI (host-only cice_evp_hip_plan_build) and reads back
the C grid's exchange (cice_evp_hip_cgrid_fold_xplan) and the three stress lists whose operands may be staging slots of that
exchange (cice_evp_hip_stress_tfold_xplan).  What cice_evp_hip_stress_halo does with them is restated in numpy -- each pair
(a1, a2) exchanged over gloo, the raw values the exchange leaves in the staging slots kept per array, then all reads, then
all writes -- and must leave every cell of every block, ghost ring included, with the bit pattern the one-rank lists (the
ones tests/test_gpu_parity.py pins on the reference's own arrays) give the same blocks on one rank.

A worker that raises reports it through the queue, and one that dies is noticed by its exit code: either fails the test at once
and ends the other workers (they may be waiting for it in an exchange) -- no test waits for a time limit to run out."""
import ctypes as C
import os
import queue
import time
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cice_amd import decomp, evp
from test_cgrid_fold_split_cpu import HALO_CASES, _free_port, _layout

TFOLD_CASES = [c for c in HALO_CASES if c[4] == "tripoleT"]
assert len(TFOLD_CASES) == 6
SPLIT_CASES = [c for c in TFOLD_CASES if not (c[7] and c[7][0] == "drop")]
DROP_CASE = next(c for c in TFOLD_CASES if c[7] and c[7][0] == "drop")
PAIRS = [(q, q ^ 2) for fam in (0, 4, 8) for q in (fam, fam + 1)]        # (a1, a2) = (_1, _3), (_2, _4) of each family


def _blocks(dc, rank, glob):
    """The twelve arrays of `rank` from twelve global fields; the ghost ring of every block starts at -7.25."""
    out = []
    for g in glob:
        a = np.ascontiguousarray(dc.scatter(g, rank, fill=0.0))
        for b in dc.local_blocks(rank):
            m = np.zeros((dc.ny_block, dc.nx_block), bool)
            m[:b.gny + 2, :b.gnx + 2] = True
            m[1:1 + b.gny, 1:1 + b.gnx] = False
            a[b.local][m] = -7.25
        out.append(a)
    return out


def _apply(arrs, n, tails, dst, src, odst, osrc, cdst, csrc):
    """The three lists on twelve flat arrays: all reads (cells, or staging values in tails[array]), then all writes."""
    def val(q, s):
        cell = arrs[q][np.minimum(s, n - 1)]
        return np.where(s < n, cell, tails[q][np.maximum(s - n, 0)] if len(tails[q]) else 0.0)
    new = []
    for q in range(12):
        w = []
        if not (q & 2):
            w.append((dst, val(q ^ 2, src)))
        else:
            w.append((odst, val(q, osrc)))
        w.append((cdst, val(q ^ 2, csrc)))
        new.append(w)
    for q in range(12):
        for d, v in new[q]:
            arrs[q][d] = v


def _spawn(target, case, world):
    """One process per rank; their results by rank.  Fails as soon as a worker reports an exception or exits without a result."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_guarded, args=(target, r, world, port, case, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, deadline = [], time.monotonic() + 300
    try:
        while len(res) < world:
            try:
                r = q.get(timeout=0.2)
            except queue.Empty:
                died = [k for k, p in enumerate(procs) if p.exitcode not in (None, 0)]
                assert not died, f"worker(s) {died} exited without a result"
                assert time.monotonic() < deadline, "workers still running after 300 s"
                continue
            assert r[0] != "error", f"rank {r[1]}:\n{r[2]}"
            res.append(r)
    finally:
        for p in procs:
            p.join(timeout=0 if len(res) < world else 60)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    assert all(p.exitcode == 0 for p in procs)
    return sorted(res, key=lambda r: r[0])


def _guarded(target, rank, world, port, case, q):
    try:
        target(rank, world, port, case, q)
    except BaseException:
        q.put(("error", rank, traceback.format_exc()))


def _stress_worker(rank, world, port, case, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        nx, ny, bx, by, ns = case[:5]
        dc = _layout(case)
        d, keep = evp.make_dims(dc, rank)
        X = evp.cgrid_fold_xplan(d)
        S = evp.stress_tfold_xplan(d)
        assert S["ok"], S["why"]
        n = len(dc.local_blocks(rank)) * dc.ny_block * dc.nx_block
        assert all(int(S[k].max(initial=0)) < n + X["tail"] and int(S[k].min(initial=0)) >= 0 for k in ("src", "own_src", "corner_src"))
        glob = [np.random.default_rng(100 + k).standard_normal((ny, nx)) for k in range(12)]
        a = _blocks(dc, rank, glob)
        before = [x.copy() for x in a]
        flat = [x.reshape(-1) for x in a]
        tails = [np.zeros(X["tail"]) for _ in range(12)]
        for q1, q2 in PAIRS:                     # collective: every rank, with or without entries of its own
            ext = [np.concatenate([flat[k], np.zeros(X["tail"])]) for k in (q1, q2)]
            send = torch.from_numpy(np.stack([e[X["send_src"]] for e in ext], axis=1).copy())
            recv = torch.zeros((len(X["recv_dst"]), 2), dtype=torch.float64)
            ops, so, ro = [], 0, 0
            for p, ns_, nr_ in zip(X["peer_rank"], X["peer_nsend"], X["peer_nrecv"]):
                if ns_:
                    ops.append(dist.P2POp(dist.isend, send[so:so + ns_], int(p)))
                if nr_:
                    ops.append(dist.P2POp(dist.irecv, recv[ro:ro + nr_], int(p)))
                so += ns_
                ro += nr_
            for w in (dist.batch_isend_irecv(ops) if ops else []):
                w.wait()
            for e, k, col in zip(ext, (q1, q2), (0, 1)):
                e[X["recv_dst"]] = recv.numpy()[:, col]
                tails[k] = e[n:].copy()          # (the stresses themselves take nothing from the exchange: it runs on copies)
        _apply(flat, n, tails, S["dst"], S["src"], S["own_dst"], S["own_src"], S["corner_dst"], S["corner_src"])
        # the same blocks on one rank, the lists of the halo plan
        one = decomp.Decomp(nx, ny, bx, by, "cyclic", ns, 1)
        d1, keep1 = evp.make_dims(one, 0)
        P = evp.halo_plan(d1)
        F = evp.fold_split_plan()
        assert not P["stress_remote"]
        r = _blocks(one, 0, glob)
        n1 = r[0].size
        _apply([x.reshape(-1) for x in r], n1, [np.zeros(0)] * 12, P["stress_dst"], P["stress_src"], F["stress_own_dst"], F["stress_own_src"],
               F["stress_corner_dst"], F["stress_corner_src"])
        ob = one.local_blocks(0)
        nbad, changed = [], 0
        for k in range(12):
            for b in dc.local_blocks(rank):
                kb = next(o.local for o in ob if o.gi0 == b.gi0 and o.gj0 == b.gj0)
                same = a[k][b.local].view(np.int64) == r[k][kb].view(np.int64)
                if not same.all():
                    nbad.append((k, b.gid, int((~same).sum())))
                changed += int((a[k][b.local].view(np.int64) != before[k][b.local].view(np.int64)).sum())
        remote = int(sum((S[k] >= n).sum() for k in ("src", "own_src", "corner_src")))
        q.put((rank, nbad, changed, remote, S["collective"], len(S["dst"])))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("case", SPLIT_CASES)
def test_tripolet_stress_lists_across_ranks_equal_the_one_rank_lists(case):
    res = _spawn(_stress_worker, case, case[5])
    for rank, nbad, changed, remote, collective, ndst in res:
        assert not nbad, f"rank {rank}: (array, block, cells) differ from the one-rank symmetrisation: {nbad}"
    assert sum(r[2] for r in res) > 0, "the lists wrote nothing that differs from the input"
    assert len({r[4] for r in res}) == 1, "every rank must reach the same verdict on whether the exchange is needed"
    top_split = not (case[7] and case[7][0] == "top")          # (the y-only cut: the whole top row on one rank)
    assert res[0][4] == top_split
    assert (sum(r[3] for r in res) > 0) == top_split, "operands in staging slots exactly where the top row has several owners"


def test_tripolet_stress_lists_decline_an_eliminated_block_with_a_reason():
    dc = _layout(DROP_CASE)
    res = []
    for rank in range(DROP_CASE[5]):             # (host only, nothing is exchanged: one rank after the other in this process)
        d, keep = evp.make_dims(dc, rank)
        S = evp.stress_tfold_xplan(d)
        P = evp.halo_plan(d)
        res.append((rank, S["ok"], S["why"], bool(P["stress_remote"])))
    for rank, ok, why, stress_remote in res:
        assert not ok and "eliminated block" in why, (rank, why)
    # cice_evp_hip_stress_halo_available keeps its rule there: 0 on the ranks whose lists name a cell they do not hold, and the
    # host takes the minimum over the ranks
    assert any(r[3] for r in res)


@pytest.mark.parametrize("bx,by", [(18, 10), (25, 40), (12, 20)])
def test_one_rank_lists_equal_the_halo_plans(bx, by):
    one = decomp.Decomp(72, 40, bx, by, "cyclic", "tripoleT", 1)
    d, keep = evp.make_dims(one, 0)
    S = evp.stress_tfold_xplan(d)
    P = evp.halo_plan(d)
    F = evp.fold_split_plan()
    assert S["ok"] and not S["collective"] and len(S["dst"]) > 0 and len(S["corner_dst"]) > 0
    for new, old in ((("dst", "src"), (P["stress_dst"], P["stress_src"])),
                     (("own_dst", "own_src"), (F["stress_own_dst"], F["stress_own_src"])),
                     (("corner_dst", "corner_src"), (F["stress_corner_dst"], F["stress_corner_src"]))):
        assert np.array_equal(S[new[0]], old[0]) and np.array_equal(S[new[1]], old[1]), new


def test_not_tripolet_declines():
    d, keep = evp.make_dims(decomp.Decomp(72, 40, 36, 40, "cyclic", "tripole", 2, (2, 1)), 0)
    S = evp.stress_tfold_xplan(d)
    assert not S["ok"] and "tripoleT" in S["why"]


def test_plan_dump_untouched_by_the_new_entry():
    lib = evp.load_library(testing=True)
    for case in (TFOLD_CASES[0], TFOLD_CASES[3], DROP_CASE):
        dc = _layout(case)
        for rank in range(case[5]):
            d, keep = evp.make_dims(dc, rank)
            before = evp.halo_plan_dump(d)
            info = np.zeros(4, dtype=np.int32)
            lists = [np.zeros(4096, dtype=np.int32) for _ in range(6)]
            ip = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))
            rc = lib.cice_evp_hip_stress_tfold_xplan(ip(info), *[ip(x) for x in lists])
            assert rc in (0, 1) and int(info[:3].max()) <= 4096
            after = np.zeros(len(before), dtype=np.int32)
            assert lib.cice_evp_hip_plan_dump(ip(after), len(after)) == len(before)
            assert before.tobytes() == after.tobytes()
