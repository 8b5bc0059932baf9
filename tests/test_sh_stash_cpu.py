"""CPU tests of the SH stash (include/stp_raster.h: stp_set_forward_sh_stash): the C ABI's declarations and exports, the request called
without a device, and the geometry buffer's size and layout with and without the stash."""
import ctypes
import os
import re
import subprocess

import pytest

from helpers import FULL_STP, settings_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("stp_set_forward_sh_stash", "stp_geometry_buffer_size_stash")


def test_header_declares_the_request_and_the_size_query():
    h = open(os.path.join(ROOT, "include", "stp_raster.h")).read()
    assert int(re.search(r"#define\s+STP_ABI_VERSION\s+(\d+)\b", h).group(1)) == 7
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"void\s+stp_set_forward_sh_stash\s*\(\s*int\s+enable\s*\)\s*;", h)
    assert re.search(r"size_t\s+stp_geometry_buffer_size_stash\s*\(\s*int\s+P\s*,\s*const\s+StpSettings\s*\*\s*settings\s*\)\s*;", h)


@pytest.mark.parametrize("lib", ["libstp_raster.so", "libstp_raster_fma.so"])
def test_both_libraries_export_them(lib):
    from diff_gaussian_rasterization import _C
    path = os.path.join(os.path.dirname(_C.library_path()), lib)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in SYMBOLS:
        assert name in exported, (lib, name)


def test_request_is_callable_without_a_device_and_the_abi_is_still_7():
    from diff_gaussian_rasterization import _C
    L = _C._load()
    assert L.stp_abi_version() == 7
    for name in SYMBOLS:
        assert hasattr(L, name) and _C._require(name) is not None
    L.stp_set_forward_sh_stash(1)   # a pending request ...
    L.stp_set_forward_sh_stash(0)   # ... cleared


@pytest.mark.parametrize("sd", [settings_dict(0), settings_dict(**FULL_STP)], ids=["global", "full_stp"])
@pytest.mark.parametrize("P", [1, 257, 300, 100003])
def test_geometry_buffer_grows_by_the_stash_only(P, sd):
    """The plain size query -- what a forward without the request asks its allocator for -- is unchanged by a pending request; the stash
    query is larger by the nine planes of P floats, which lie behind every other sub-array: "sh_stash" starts where the plain buffer's
    sub-arrays end (at the carve's next aligned offset), and no other sub-array moves."""
    from diff_gaussian_rasterization import _C
    L = _C._load()
    s = _C.settings_from_dict(sd)
    plain = int(L.stp_geometry_buffer_size(P, ctypes.byref(s)))
    L.stp_set_forward_sh_stash(1)
    assert int(L.stp_geometry_buffer_size(P, ctypes.byref(s))) == plain   # (only a forward that asks gets the larger buffer)
    L.stp_set_forward_sh_stash(0)
    stash = int(L.stp_geometry_buffer_size_stash(P, ctypes.byref(s)))
    off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.stp_geometry_layout(P, ctypes.byref(s), b"sh_stash", ctypes.byref(off), ctypes.byref(cnt)) == 0
    assert cnt.value == 9 * P
    # both totals are an aligned end + one alignment unit: the difference is the sub-array and its padding to the alignment, nothing else
    align = 256
    assert stash - plain >= 36 * P and stash - plain < 36 * P + 2 * align, (plain, stash)
    assert off.value % 16 == 0 and plain - 2 * align <= off.value <= plain and off.value + 36 * P <= stash
    last_off, last_cnt = ctypes.c_size_t(), ctypes.c_size_t()
    assert L.stp_geometry_layout(P, ctypes.byref(s), b"invz", ctypes.byref(last_off), ctypes.byref(last_cnt)) == 0
    assert last_off.value + 4 * last_cnt.value <= off.value   # behind invz, the last sub-array of the plain carve
