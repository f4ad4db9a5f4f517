"""Block layouts shared with the HIP library, parsed from ``csrc/dat_layout.h`` (single source of truth)."""

from __future__ import annotations

import os
import re

_HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "dat_layout.h")

_const: dict = {}
_func: dict = {}
with open(_HDR) as _f:
    for _line in _f:
        _m = re.match(r"#define\s+(DAT_\w+)\((\w+)\)\s+(.+?)\s*(//.*)?$", _line)
        if _m:
            _func[_m.group(1)] = (_m.group(2), _m.group(3))
            continue
        _m = re.match(r"#define\s+(DAT_\w+)\s+([-\w.()+* ]+?)\s*(//.*)?$", _line)
        if _m:
            _const[_m.group(1)] = _m.group(2)


def _eval(expr: str, env: dict):
    expr = re.sub(r"(DAT_\w+)\((\w+)\)", lambda m: str(fn(m.group(1), int(env[m.group(2)]) if m.group(2) in env else int(m.group(2)))), expr)
    expr = re.sub(r"\bDAT_\w+\b", lambda m: str(const(m.group(0))), expr)
    return eval(expr, {}, env)  # noqa: S307 -- header arithmetic only


def const(name: str):
    return _eval(_const[name], {})


def fn(name: str, n: int) -> int:
    arg, body = _func[name]
    return int(_eval(body, {arg: n}))


P = {k[len("DAT_P_"):]: const(k) for k in _const if k.startswith("DAT_P_")}
M = {k[len("DAT_M_"):]: const(k) for k in _const if k.startswith("DAT_M_")}
T = {k[len("DAT_T_"):]: const(k) for k in _const if k.startswith("DAT_T_")}  # tracking record (dat_set_tracking)
TRACK_SIZE = const("DAT_TRACK_SIZE")
NENV = const("DAT_NENV")
GRAVITY = const("DAT_GRAVITY")


def param_size(n: int) -> int:
    return fn("DAT_PARAM_SIZE", n)


def state_size(n: int) -> int:
    return fn("DAT_STATE_SIZE", n)


def p_off(name: str, n: int) -> int:
    return fn("DAT_P_" + name, n)


def s_off(name: str, n: int) -> int:
    return fn("DAT_S_" + name, n)


# ---- episodes (DAT_EP_*: the reasons and the outcome record's words; dat_episode_*, csrc/dat_episode.hpp)
EP_REASONS = {k[len("DAT_EP_"):]: const(k) for k in ("DAT_EP_NONE", "DAT_EP_DIVERGED", "DAT_EP_COLLISION", "DAT_EP_GOAL",
                                                     "DAT_EP_STALL", "DAT_EP_TIME_LIMIT")}
EP_NREASON = const("DAT_EP_NREASON")
EP_WORDS = const("DAT_EP_WORDS")
EP = {k[len("DAT_EP_"):]: const(k) for k in ("DAT_EP_SLOT", "DAT_EP_RECORD", "DAT_EP_START", "DAT_EP_END", "DAT_EP_STEPS",
                                             "DAT_EP_ITMAX", "DAT_EP_RUN", "DAT_EP_MIND", "DAT_EP_XL", "DAT_EP_VL")}

# ---- checkpoint record (DAT_CK_*) and its field table (csrc/dat_ckpt.hpp, the lists the copy kernels are written from)
CK_HEADER_BYTES = const("DAT_CK_HEADER_BYTES")
CK_MAGIC = const("DAT_CK_MAGIC")
CK_VERSION = const("DAT_CK_VERSION")
CK_H = {k[len("DAT_CK_H_"):]: const(k) for k in _const if k.startswith("DAT_CK_H_")}  # header fields' byte offsets
CK_MODES = {0: "CENT", 1: "CADMM", 2: "DD"}  # DAT_MODE_* -> the macros' suffix
CK_INTS = {}  # int array of the handle -> index among the ints at DAT_CK_INTS(n)
_ck_lists: dict = {}  # list suffix (ALL, CADMM, DD, CENT) -> [(array of the handle, words expression, offset macro)]
with open(os.path.join(os.path.dirname(_HDR), "dat_ckpt.hpp")) as _f:
    _src = _f.read().replace("\\\n", " ")
for _m in re.finditer(r"#define\s+DAT_CK_FIELDS_(\w+)\(X, n\)(.*)", _src):
    _ck_lists[_m.group(1)] = re.findall(r"X\((\w+),\s*(.+?),\s*(DAT_CK_\w+)\(n\)\)", _m.group(2))
for _m in re.finditer(r"X\((\w+), (\d)\)", re.search(r"#define\s+DAT_CK_INT_FIELDS\(X\)(.*)", _src).group(1)):
    CK_INTS[_m.group(1)] = int(_m.group(2))


def ck_words(mode: int, n: int) -> int:
    """Words (8 bytes) of one checkpoint record of `mode` (DAT_MODE_*) at team size n."""
    return fn("DAT_CK_WORDS_" + CK_MODES[mode], n)


def ck_ints(n: int) -> int:
    return fn("DAT_CK_INTS", n)


def ck_fields(mode: int, n: int) -> dict:
    """The fp64 arrays of a record: array of the handle -> (record offset, words), from the table of dat_ckpt.hpp."""
    out = {}
    for arr, words, off in _ck_lists["ALL"] + _ck_lists[CK_MODES[mode]]:
        out[arr] = (fn(off, n), int(_eval(words, {"n": n})))
    return out
