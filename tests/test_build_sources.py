"""The library's source lists follow the csrc/ directory: a new translation unit is compiled and a new header
enters the source hash without anyone listing it, and the unity file (development builds, tools/build_var.sh)
includes every unit that holds kernels of dat.hip's families."""
import os
import re

from distributed_aerial_transportation_amd import _lib

CSRC = os.path.join(_lib.PKG, "csrc")


def _text(path):
    with open(path) as f:
        return f.read()


def test_srcs_are_the_hip_files_but_the_unity_file():
    hips = {os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip")}
    assert _lib.UNITY in hips
    assert set(_lib.SRCS) == hips - {_lib.UNITY}
    assert len(_lib.SRCS) == len(set(_lib.SRCS))


def test_deps_cover_csrc_and_the_abi_header():
    deps = set(_lib.DEPS)
    for f in os.listdir(CSRC):
        assert os.path.join(CSRC, f) in deps, f
    assert os.path.join(_lib.REPO, "include", "dat.h") in deps
    assert list(_lib.DEPS[:-1]) == sorted(_lib.DEPS[:-1])  # a fixed order: the hash does not depend on the listing's


def test_unity_file_includes_every_kernel_unit():
    included = set(re.findall(r'^#include "([^"]+\.hip)"', _text(_lib.UNITY), re.M))
    # the kernel units of dat.hip's families are the dat_k_*.hip (csrc/dat_launch.hpp); the centralized kernel and
    # the collectives are units of their own in every build, and the host units (dat.hip, dat_h_*.hip) hold no kernel
    names = {os.path.basename(s) for s in _lib.SRCS}
    kernel_units = {u for u in names if u.startswith("dat_k_")}
    assert kernel_units
    host_units = names - kernel_units - {"dat_cent.hip", "dat_comm.hip"}
    for u in host_units:
        assert "__global__" not in _text(os.path.join(CSRC, u)), u
    assert kernel_units <= included, kernel_units - included
    assert "dat.hip" in names and "dat.hip" in included
    assert {"dat_h_log.hip", "dat_h_episode.hip", "dat_h_ckpt.hip"} <= host_units
    assert host_units <= included, host_units - included  # every unit but the two that stand alone
    assert included <= names, included - names
    assert re.search(r"^#define DAT_UNITY\b", _text(_lib.UNITY), re.M)


def test_rule_and_handle_headers_stay_with_the_host_units():
    """dat_modes.hpp and dat_handle.hpp are host code: no kernel unit, and no header a kernel unit includes, includes
    them; dat_modes.hpp includes nothing of HIP's"""
    names = {os.path.basename(s) for s in _lib.SRCS}
    host = {"dat.hip", "dat_unity.hip", "dat_handle.hpp"} | {u for u in names if u.startswith("dat_h_")}
    for f in os.listdir(CSRC):
        if f not in host:
            assert not re.search(r'#include "dat_(modes|handle)\.hpp"', _text(os.path.join(CSRC, f))), f
    modes = _text(os.path.join(CSRC, "dat_modes.hpp"))
    assert "hip" not in re.sub(r"//.*", "", modes).lower()
