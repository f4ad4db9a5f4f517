"""Is the device code of two builds the same?  Compares two assembly files of a translation unit's device side,

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=on --cuda-device-only -S dat.hip -o X.s

function by function (kernels and the device functions they call): the instruction stream, the .amdhsa_*
descriptor block and the .set resource lines of each symbol.  The order of the functions in the file follows the
host code's first use of each template instantiation, so comments, the numbers of local labels (.LBB<fn>_<n>,
.Lfunc_end<fn>, renumbered here by first appearance within the function) and the __hip_cuid name are dropped.

    python tools/same_kernels.py A.s B.s

One line per symbol; exit status 1 on any difference or missing symbol.
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


a, b = functions(sys.argv[1]), functions(sys.argv[2])
bad = kernels = 0
for sym in sorted(set(a) | set(b)):
    if sym not in a or sym not in b:
        verdict, kernel = f"MISSING in {sys.argv[2 if sym in a else 1]}", (a.get(sym) or b.get(sym))[0]
    else:
        verdict, kernel = ("equal" if a[sym] == b[sym] else "DIFFERENT"), a[sym][0]
    bad += verdict != "equal"
    kernels += kernel
    print(f"{verdict:>9}  {'kernel' if kernel else 'function'}  {sym}")
print(f"{kernels} kernels, {len(set(a) | set(b)) - kernels} device functions, {bad} not equal")
sys.exit(1 if bad or not a else 0)
