"""Static tally of the device assembly of a build, function by function: what profiles/cadmm_leaf.md tabulates.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on --save-temps -c csrc/dat_k_cadmm_adv.hip
    python tools/kernel_tally.py dat_k_cadmm_adv-hip-amdgcn-amd-amdhsa-gfx950.s [substring of a demangled name ...]

One line per function (kernels and out-of-line device functions): instructions, FP64 arithmetic, calls (s_swappc),
v_accvgpr moves, v_readlane / v_writelane, scratch loads / stores, s_waitcnt vmcnt, then the compiler's own figures
from the function's trailer and the metadata: scratch bytes per lane, VGPR and SGPR spill counts.  A reading aid for
a person comparing two builds; nothing in the test suite depends on it.
"""
import re
import subprocess
import sys

TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")
F64 = re.compile(r"^v_(add|mul|fma|fmac|div_fmas|div_fixup|div_scale|rcp|rsq|sqrt|max|min|ldexp|frexp_mant|trunc|floor|ceil|rndne|fract|cmp\w*|cmpx\w*|cvt\w*)_f64")


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def tally(path):
    out, name = {}, None
    with open(path) as f:
        lines = f.readlines()
    for k, raw in enumerate(lines):
        m = TYPE.match(raw)
        if m:
            name = m.group(1)
            out[name] = dict(insts=0, f64=0, call=0, acc=0, rdlane=0, wrlane=0, sld=0, sst=0, vmcnt=0, scratch=None)
            continue
        if raw.startswith("\t.section\t.AMDGPU.csdata") or raw.startswith("\t.amdgpu_metadata"):
            name = None
        if name is None:
            continue
        t = out[name]
        code = raw.split(";", 1)[0]
        m = INSN.match(code)
        if not m or code.lstrip().startswith("."):
            continue
        op = m.group(1)
        t["insts"] += 1
        t["f64"] += bool(F64.match(op))
        t["call"] += op.startswith("s_swappc")
        t["acc"] += op.startswith("v_accvgpr")
        t["rdlane"] += op.startswith("v_readlane")
        t["wrlane"] += op.startswith("v_writelane")
        t["sld"] += op.startswith("scratch_load")
        t["sst"] += op.startswith("scratch_store")
        t["vmcnt"] += op == "s_waitcnt" and "vmcnt" in code
    # the metadata's per-kernel figures (fields in alphabetical order after .name)
    cur = None
    for raw in lines:
        m = re.match(r"^\s+\.name:\s+(\S+)", raw)
        if m:
            cur = m.group(1)
        m = re.match(r"^\s+\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", raw)
        if m and cur in out:
            key = {"sgpr_spill_count": "sspill", "vgpr_spill_count": "vspill", "private_segment_fixed_size": "scratch"}
            out[cur][key[m.group(1)]] = int(m.group(2))
    for t in out.values():
        t.setdefault("vspill", None)
        t.setdefault("sspill", None)
    return out


def main():
    path, want = sys.argv[1], sys.argv[2:]
    t = tally(path)
    names = demangle(list(t))
    cols = ["insts", "f64", "call", "acc", "rdlane", "wrlane", "sld", "sst", "vmcnt", "scratch", "vspill", "sspill"]
    print(" ".join(f"{c:>7}" for c in cols) + "  function")
    for n, v in t.items():
        d = names[n]
        if want and not any(w in d for w in want):
            continue
        short = re.sub(r"\(anonymous namespace\)::|dat::", "", d)
        short = re.sub(r"\((KArgs|.*Args.*)\)$", "", short)
        print(" ".join(f"{'-' if v[c] is None else v[c]:>7}" for c in cols) + "  " + short)


if __name__ == "__main__":
    main()
