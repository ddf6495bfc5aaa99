#!/usr/bin/env python3
"""Static instruction mix of the resident B-grid kernel's subcycle loop, from a cross-compile (no GPU needed).

Compiles cice_amd/csrc/evp_resident2.hip for gfx950 with the build's flags to assembly, takes the headline instantiation
(strict, default scalars, 16 x 16 tiles, one rank: the lean variant where it is built, else the general kernel), finds its
subcycle loop (the backward branch that spans the most instructions) and counts what the loop holds, per subcycle: a loop
that carries two subcycles per trip (the lean variant: one per record-buffer parity) is halved.

  python tools/resident_isa_mix.py [--general | --lean] [--asm FILE.s] [--blocks]
     --general   the general kernel <true, 3, 4, false, false> even where the lean one exists
     --lean      the lean variant on its first schedule (two workgroup barriers per subcycle) even where the rim-wave
                 schedule (RIMU) exists
     --asm       count an assembly file made earlier instead of compiling
     --blocks    also list the loop's basic blocks that hold a square root or a division: size, seeds (v_rsq_f64, v_rcp_f64) and
                 range handling (v_ldexp_f64, v_div_scale_f64, v_div_fixup_f64) -- a block with seeds and no range handling is a
                 range-proved core (csrc/evp_range_math.h), a block of range handling behind the loop's other blocks its library path
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
SRC = ROOT / "cice_amd" / "csrc" / "evp_resident2.hip"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GENERAL = ("_ZN12_GLOBAL__N_118evp_resident2_tileILb1ELi3ELi4ELb0ELb0ELb0EEEv7EvpArgs12EvpResident2",
           "_ZN12_GLOBAL__N_118evp_resident2_tileILb1ELi3ELi4ELb0ELb0EEEv7EvpArgs12EvpResident2")   # (before the LEAN parameter)
GENERAL = ("_ZN12_GLOBAL__N_118evp_resident2_tileILb1ELi3ELi4ELb0ELb0ELb0ELb0EEEv7EvpArgs12EvpResident2",) + GENERAL
LEAN = ("_ZN12_GLOBAL__N_118evp_resident2_tileILb1ELi3ELi4ELb0ELb0ELb1ELb0EEEv7EvpArgs12EvpResident2",
        "_ZN12_GLOBAL__N_118evp_resident2_tileILb1ELi3ELi4ELb0ELb0ELb1EEEv7EvpArgs12EvpResident2")          # (before the RIMU parameter)
RIMU = "_ZN12_GLOBAL__N_118evp_resident2_tileILb1ELi3ELi4ELb0ELb0ELb1ELb1EEEv7EvpArgs12EvpResident2"


def compile_asm(out: Path) -> None:
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", str(SRC), "-o", str(out)],
                   check=True, cwd=SRC.parent, stderr=subprocess.DEVNULL)


def function_body(lines, name):
    start = next((k for k, l in enumerate(lines) if l.startswith(name + ":")), None)
    if start is None:
        return None, {}
    body = []
    for l in lines[start + 1:]:
        if l.strip().startswith(".Lfunc_end"):
            break
        body.append(l)
    meta = {}
    for l in lines[start:]:
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size)\s+(\d+)", l)
        if m and m.group(1) not in meta:
            meta[m.group(1)] = int(m.group(2))
        if len(meta) == 3:
            break
    return body, meta


def instructions(body):
    """[(kind, text)]: kind 'label' (name) or 'inst' (mnemonic, operands)."""
    out = []
    for l in body:
        s = l.split(";")[0].strip()
        if not s:
            continue
        if s.endswith(":"):
            out.append(("label", s[:-1]))
        elif not s.startswith("."):
            out.append(("inst", s))
    return out


def largest_loop(ins):
    pos, n = {}, 0                             # label -> index of the instruction that follows it
    for kind, s in ins:
        if kind == "label":
            pos[s] = n
        else:
            n += 1
    best = None
    n = 0
    for kind, s in ins:
        if kind == "inst":
            m = re.match(r"s_cbranch_\w+\s+(\S+)|s_branch\s+(\S+)", s)
            if m:
                tgt = m.group(1) or m.group(2)
                if tgt in pos and pos[tgt] <= n and (best is None or n + 1 - pos[tgt] > best[1] - best[0]):
                    best = (pos[tgt], n + 1)
            n += 1
    return best


def classify(mn: str) -> str:
    if mn.startswith("v_") and "f64" in mn:
        return "fp64"
    if mn.startswith("ds_"):
        return "LDS"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if mn.startswith("s_"):
        return "SALU / branch"
    if mn.startswith("v_"):
        return "other VALU"
    return "other"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--general", action="store_true")
    ap.add_argument("--lean", action="store_true")
    ap.add_argument("--asm", default=None)
    ap.add_argument("--blocks", action="store_true")
    a = ap.parse_args()
    if a.asm:
        lines = Path(a.asm).read_text().splitlines()
    else:
        with tempfile.TemporaryDirectory() as d:
            out = Path(d) / "evp_resident2.s"
            compile_asm(out)
            lines = out.read_text().splitlines()
    body, meta, per_trip, name = None, {}, 1, None
    for cand in ([] if a.general else list(LEAN) if a.lean else [RIMU, *LEAN]):
        if body is None:
            body, meta = function_body(lines, cand)
            if body is not None:
                per_trip, name = 2, cand
    for g in GENERAL:
        if body is None:
            body, meta = function_body(lines, g)
            name = g
    if body is None:
        print("instantiation not found", file=sys.stderr)
        return 1
    ins = instructions(body)
    lo, hi = largest_loop(ins)
    loop = [s for kind, s in ins if kind == "inst"][lo:hi]
    mns = [s.split()[0] for s in loop]
    cls = Counter(classify(m) for m in mns)
    print(f"kernel   {name}")
    print(f"VGPRs    {meta.get('next_free_vgpr')} (arch VGPRs {meta.get('accum_offset')}), scratch {meta.get('private_segment_fixed_size')} B")
    print(f"loop     {len(loop)} static instructions, {per_trip} subcycle(s) per trip")
    print(f"{'class':16s} {'per trip':>9s} {'per subcycle':>13s}")
    for c in ("fp64", "other VALU", "SALU / branch", "VMEM", "LDS", "other"):
        print(f"{c:16s} {cls[c]:9d} {cls[c] / per_trip:13.1f}")
    nonfp = len(loop) - cls["fp64"]
    print(f"{'non-fp64':16s} {nonfp:9d} {nonfp / per_trip:13.1f}")
    print(f"{'total':16s} {len(loop):9d} {len(loop) / per_trip:13.1f}")
    sub = Counter(mns)
    print("most frequent non-fp64 mnemonics (per subcycle):")
    for m, k in sorted(((m, k) for m, k in sub.items() if classify(m) != "fp64"), key=lambda x: -x[1])[:16]:
        print(f"  {m:28s} {k / per_trip:7.1f}")
    if a.blocks:
        print("blocks of the loop that hold a square root or a division (label: instructions; seeds; range handling):")
        n, label, cur, rows = 0, None, [], []
        for kind, t in ins:
            if kind == "label":
                if cur:
                    rows.append((label, cur))
                label, cur = t, []
            else:
                if lo <= n < hi:
                    cur.append(t.split()[0])
                n += 1
        if cur:
            rows.append((label, cur))
        lib = 0
        for label, b in rows:
            c = Counter(m[:-4] if m.endswith("_e32") or m.endswith("_e64") else m for m in b)
            seeds, handling = c["v_rsq_f64"] + c["v_rcp_f64"], c["v_ldexp_f64"] + c["v_div_scale_f64"] + c["v_div_fixup_f64"]
            if seeds + handling:
                print(f"  {label:12s} {len(b):4d}   rsq {c['v_rsq_f64']} rcp {c['v_rcp_f64']}   ldexp {c['v_ldexp_f64']} div_scale {c['v_div_scale_f64']} "
                      f"div_fixup {c['v_div_fixup_f64']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
