"""Is the device code of two builds the same?  Compares the assembly of the device side of two builds, each one
translation unit or several (the kernel units under csrc/, dat_launch.hpp; dat_unity.hip is all of them as one),

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on --cuda-device-only -S dat_k_dd.hip -o X.s

function by function (kernels and the device functions they call): the instruction stream, the .amdhsa_*
descriptor block and the .set resource lines of each symbol.  The order of the functions in a file follows the
host code's first use of each template instantiation, so comments, the numbers of local labels (.LBB<fn>_<n>,
.Lfunc_end<fn>, renumbered here by first appearance within the function) and the __hip_cuid name are dropped.

    python tools/same_kernels.py A.s B.s
    python tools/same_kernels.py A.s --vs B1.s B2.s B3.s

A side is the union of its files' symbols.  A symbol that several files of one side hold (an out-of-line device
function such as build_shared) must be equal in all of them, else it is reported as SPLIT and counts as a
difference.  One line per symbol; exit status 1 on any difference or missing symbol.
"""
import re
import sys

TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
LOCAL = re.compile(r"\.L[A-Za-z_]+[0-9][0-9_]*")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def functions(path):
    """symbol -> (is kernel, normalised lines from its .type line to its last .set line)"""
    out, name, body = {}, None, []

    def close():
        nonlocal name
        if name is not None:
            seen = {}
            text = [LOCAL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), ln) for ln in body]
            out[name] = (any(ln.startswith(".amdhsa_kernel ") for ln in text), text)
        name = None

    with open(path) as f:
        for raw in f:
            ln = CUID.sub("__hip_cuid", raw.split(";", 1)[0]).strip()
            m = TYPE.match(ln)
            if m or ln.startswith(".section\t.AMDGPU.csdata") or ln.startswith(".amdgpu_metadata"):
                close()
            if m:
                name, body = m.group(1), []
            if name is not None and ln:
                body.append(ln)
    close()
    return out


def side(paths):
    """the union of the files' symbols, and those that differ between two files of the side"""
    out, split = {}, set()
    for p in paths:
        for sym, fn in functions(p).items():
            if out.setdefault(sym, fn) != fn:
                split.add(sym)
    return out, split


args = sys.argv[1:]
if "--vs" in args:
    pa, pb = args[:args.index("--vs")], args[args.index("--vs") + 1:]
else:
    pa, pb = args[:1], args[1:]
if not pa or not pb:
    sys.exit(__doc__)
(a, sa), (b, sb) = side(pa), side(pb)
bad = kernels = 0
for sym in sorted(set(a) | set(b)):
    if sym not in a or sym not in b:
        verdict, kernel = f"MISSING in {' '.join(pb if sym in a else pa)}", (a.get(sym) or b.get(sym))[0]
    elif sym in sa or sym in sb:
        verdict, kernel = f"SPLIT: differs between the files of {' '.join(pa if sym in sa else pb)}", a[sym][0]
    else:
        verdict, kernel = ("equal" if a[sym] == b[sym] else "DIFFERENT"), a[sym][0]
    bad += verdict != "equal"
    kernels += kernel
    print(f"{verdict:>9}  {'kernel' if kernel else 'function'}  {sym}")
print(f"{kernels} kernels, {len(set(a) | set(b)) - kernels} device functions, {bad} not equal")
sys.exit(1 if bad or not a else 0)
