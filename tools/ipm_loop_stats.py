#!/usr/bin/env python3
"""Static instruction statistics of the IPM iteration loops in the emitted gfx950 assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on -S --cuda-device-only \
        distributed_aerial_transportation_amd/csrc/dat_k_cadmm.hip -o dat.s
    python tools/ipm_loop_stats.py dat.s [--kernels k_cadmm,k_cadmm0,k_cadmm_tail,k_dd] [--min-valu 3000]

The IPM kernels live in three units (csrc/dat_launch.hpp): dat_k_cadmm.hip (k_cadmm, k_cadmm0, k_dd, above),
dat_k_cadmm_adv.hip (their advance-overlap instantiations) and dat_k_cadmm_tail.hip (the tail kernels, k_agent_qp);
csrc/dat_unity.hip is all of them as one unit, with the same device code.

The compiler annotates every basic block with the loop it belongs to ("=>This Loop Header", "Parent Loop",
"in Loop: Header=").  An IPM iteration loop (ipm_attempt's `for (it = 0;; ++it)`) is recognised by size: a loop
whose body, child loops included, holds at least --min-valu vector ALU instructions and none of whose child
loops does (the attempt / redo loops around it have such a child; the refinement and backtracking loops inside
it are far smaller).  One line per loop, in the order of the assembly (k_cadmm: one loop per env class and row
mode instantiation).

Counts are of the loop body's text (each instruction once, child loops included), not of executed
instructions.  The wait statistics follow the body in layout order with a model of the LDS / scalar-memory
counter: LDS operations complete in order, so `s_waitcnt lgkmcnt(N)` leaves the N youngest outstanding.
  lgkm waits     s_waitcnt with an lgkmcnt field, and those reached with at least one LDS read outstanding
  reads/wait     mean LDS reads outstanding at such a wait (reads in flight per exposed round trip)
  vm waits       s_waitcnt with a vmcnt field
Only ordinary instructions are looked for: vector ALU, ds_read / ds_write, scratch loads and stores,
v_accvgpr moves and s_waitcnt.
"""

from __future__ import annotations

import argparse
import re
import sys

FUNC = re.compile(r"^(_Z\w+):")
LABEL = re.compile(r"^\.L(BB\d+_\d+):")
BBCOMMENT = re.compile(r"^; %bb\.(\d+):")
HEADER = re.compile(r"=>\s*This (Inner )?Loop Header: Depth=(\d+)")
PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
INLOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
LGKM = re.compile(r"lgkmcnt\((\d+)\)")
KEYS = ("valu", "ds_read", "ds_write", "scr_ld", "scr_st", "accvgpr", "lgkm_waits", "lgkm_waits_rd", "rd_inflight",
        "vm_waits")


def kernel_name(mangled: str) -> str:
    """_ZN12_GLOBAL__N_17k_cadmmEN3dat5KArgsE -> k_cadmm; _ZN..4k_ddILb1EEE.. -> k_dd<1>"""
    m = re.search(r"\d+(k_[a-z0-9_]+?)(?:IL[bi](\d+)E)?E", mangled)
    if not m:
        return mangled
    return m.group(1) + (f"<{m.group(2)}>" if m.group(2) is not None else "")


def parse(path: str):
    """-> {function: [block]}; block = dict(label, line, loops (outermost first), insts)"""
    funcs: dict[str, list] = {}
    cur = None
    blk = None
    pending = None  # a block whose annotation continues on comment-only lines
    with open(path) as f:
        for ln, raw in enumerate(f, 1):
            line = raw.rstrip("\n")
            m = FUNC.match(line)
            if m:
                cur = funcs.setdefault(m.group(1), [])
                blk = {"label": "entry", "line": ln, "loops": [], "insts": []}
                cur.append(blk)
                pending = None
                continue
            if cur is None:
                continue
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            m = LABEL.match(line) or BBCOMMENT.match(line)
            if m:
                blk = {"label": m.group(1), "line": ln, "loops": [], "insts": []}
                cur.append(blk)
                pending = blk
                annotate(blk, line)
                continue
            s = line.strip()
            if pending is not None and s.startswith(";"):
                annotate(pending, line)
                continue
            pending = None
            if not s or s.startswith((";", ".")):
                continue
            blk["insts"].append(s.split(";")[0].strip())
    return funcs


def annotate(blk, line):
    for m in PARENT.finditer(line):
        blk["loops"].append(m.group(1))
    if HEADER.search(line):
        blk["loops"].append(blk["label"])
    m = INLOOP.search(line)
    if m:
        blk["inloop"] = m.group(1)


def loop_chains(blocks):
    """Resolve every block's loop chain (outermost first) from its header's chain."""
    chain = {b["label"]: b["loops"] for b in blocks if b["loops"] and b["loops"][-1] == b["label"]}
    for b in blocks:
        if "inloop" in b:
            b["loops"] = chain.get(b["inloop"], [b["inloop"]])
    return chain


def is_valu(op: str) -> bool:
    return op.startswith("v_") and not op.startswith(("v_accvgpr", "v_nop"))


def stats(blocks):
    c = dict.fromkeys(KEYS, 0)
    queue: list[str] = []  # outstanding LDS / scalar-memory operations, oldest first: 'r' LDS read, 'o' other
    for b in blocks:
        for inst in b["insts"]:
            op = inst.split()[0]
            if is_valu(op):
                c["valu"] += 1
            elif op.startswith("v_accvgpr"):
                c["accvgpr"] += 1
            elif op.startswith("ds_read"):
                c["ds_read"] += 1
                queue.append("r")
            elif op.startswith("ds_write"):
                c["ds_write"] += 1
                queue.append("o")
            elif op.startswith("ds_") or op.startswith("s_load") or op.startswith("s_buffer_load"):
                queue.append("o")
            elif op.startswith("scratch_load"):
                c["scr_ld"] += 1
            elif op.startswith("scratch_store"):
                c["scr_st"] += 1
            elif op == "s_waitcnt":
                if "vmcnt" in inst:
                    c["vm_waits"] += 1
                m = LGKM.search(inst)
                if m:
                    c["lgkm_waits"] += 1
                    rd = queue.count("r")
                    if rd:
                        c["lgkm_waits_rd"] += 1
                        c["rd_inflight"] += rd
                    n = int(m.group(1))
                    queue = queue[len(queue) - n:] if n else []
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("--kernels", default="k_cadmm,k_cadmm0,k_cadmm_tail,k_dd")
    ap.add_argument("--min-valu", type=int, default=3000)
    a = ap.parse_args()
    want = set(a.kernels.split(","))
    funcs = parse(a.asm)
    print(f"{'kernel':<14}{'loop':<12}{'line':>8}{'VALU':>7}{'ds_rd':>7}{'ds_wr':>7}{'scr_ld':>7}{'scr_st':>7}"
          f"{'accvgpr':>8}{'lgkm_w':>7}{'w/reads':>8}{'rd/wait':>8}{'vm_w':>6}")
    found = 0
    for fn, blocks in funcs.items():
        name = kernel_name(fn)
        if name.split("<")[0] not in want:
            continue
        chain = loop_chains(blocks)
        per = {h: stats([b for b in blocks if h in b["loops"]]) for h in chain}
        children = {h: [k for k, ch in chain.items() if len(ch) == len(chain[h]) + 1 and ch[-2] == h] for h in chain}
        for h in chain:  # dict order: the order of the assembly
            if per[h]["valu"] < a.min_valu or any(per[k]["valu"] >= a.min_valu for k in children[h]):
                continue
            c = per[h]
            line = next(b["line"] for b in blocks if b["label"] == h)
            rw = c["rd_inflight"] / c["lgkm_waits_rd"] if c["lgkm_waits_rd"] else 0.0
            print(f"{name:<14}{h:<12}{line:>8}{c['valu']:>7}{c['ds_read']:>7}{c['ds_write']:>7}{c['scr_ld']:>7}"
                  f"{c['scr_st']:>7}{c['accvgpr']:>8}{c['lgkm_waits']:>7}{c['lgkm_waits_rd']:>8}{rw:>8.2f}{c['vm_waits']:>6}")
            found += 1
    if not found:
        print("no IPM loop found (is this the device assembly of a unit with IPM kernels?)", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
