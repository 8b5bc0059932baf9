"""CPU tests of three host-only pieces of the library: the cache of what a scratch buffer was carved with (csrc/stp_layout_cache.h, run by
tests/cpp/layout_cache_check.cpp under the address and undefined-behaviour sanitizers), the render passes' ids, predicates and selector
(csrc/stp_render_pass.h, run by tests/cpp/render_pass_check.cpp the same way), and the rules by which a call consumes the one-shot
per-thread requests (csrc/stp_api.hip: take_forward_requests / take_backward_requests), seen through the C ABI on paths that return
before any HIP call."""
import ctypes
import os
import subprocess

import diff_gaussian_rasterization as dgr
from diff_gaussian_rasterization import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ci, cf, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
ALLOC_FN = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
STP_DEBUG_DEPTH = 1


def _run_host_check(tmp_path, name):
    """Build tests/cpp/<name>.cpp, a stand-alone program over one host-only header of csrc/, under the sanitizers and run it."""
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "stopthepop-rasterization_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n" and r.stderr == "", r.stdout + r.stderr


def test_layout_cache_hits_misses_and_evicts(tmp_path):
    _run_host_check(tmp_path, "layout_cache_check")


def test_render_pass_selector_and_predicates(tmp_path):
    """csrc/stp_render_pass.h: the selector over all 16 combinations of (backward, record, depth visualisation, inverse depth) and the four
    predicates on the seven pass ids, against the tables of tests/cpp/render_pass_check.cpp."""
    _run_host_check(tmp_path, "render_pass_check")


def _lib():
    L = ctypes.CDLL(_C.library_path())   # (a handle of its own: the argument types set here are not the package's)
    L.stp_last_error.restype = ctypes.c_char_p
    L.stp_set_backward_absgrad.argtypes = [vp]
    L.stp_set_backward_blend_stats.argtypes = [vp]
    L.stp_set_forward_background.argtypes = [vp, vp]
    for f in (L.stp_set_backward_absgrad, L.stp_set_backward_blend_stats, L.stp_set_forward_background):
        f.restype = None
    L.stp_backward_phases.argtypes = ([ci] * 5 + [vp, ci, ci, vp] + [vp] * 5 + [cf] + [vp] * 2 + [vp] * 4 + [cf, cf] + [vp] * 5 + [vp] * 10 + [ci, vp])
    L.stp_backward_phases.restype = ci
    L.stp_forward.argtypes = ([ALLOC_FN, vp] * 3 + [ci] * 3 + [vp, ci, ci, vp] + [vp] * 5 + [cf] + [vp] * 2 + [vp] * 4 + [cf, cf, ci] + [vp, vp, ci, vp])
    L.stp_forward.restype = ci
    return L


def _backward(L, phases):
    """P = 4, settings = NULL, every pointer NULL: refused at the latest by the null-settings check, before any HIP call."""
    rc = L.stp_backward_phases(phases, 4, 0, 0, 0, None, 16, 16, None, *([None] * 5), 1.0, None, None, *([None] * 4), 1.0, 1.0, *([None] * 15), 0, None)
    return rc, L.stp_last_error().decode()


def test_backward_refused_for_one_request_leaves_neither_behind():
    L = _lib()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    # case A: both requests pending, the call is refused for absgrad -- the blend-statistics request is gone too
    L.stp_set_backward_absgrad(p)
    L.stp_set_backward_blend_stats(p)
    rc, msg = _backward(L, 3 | 4)
    assert rc == -1 and msg == "absgrad is not available with compact gradient records (phases bit 2): the 36-byte record has no room for the two extra sums"
    rc, msg = _backward(L, 3 | 4)
    assert rc == -1 and msg == "null settings"
    # case B: blend statistics alone, refused from a chunked per-Gaussian half
    L.stp_set_backward_blend_stats(p)
    rc, msg = _backward(L, 3 | (2 << 8))
    assert rc == -1 and msg == "blend statistics are not available from a chunked per-Gaussian half (phases bits 8-23)"
    rc, msg = _backward(L, 3 | 4)
    assert rc == -1 and msg == "null settings"


def test_forward_requests_are_consumed_by_the_next_forward_whatever_its_outcome():
    L = _lib()
    dummy = ctypes.create_string_buffer(256)
    p = ctypes.addressof(dummy)
    s = _C.settings_from_dict(dgr.ExtendedSettings().to_dict())
    s.debug_visualization = STP_DEBUG_DEPTH
    null_alloc = ALLOC_FN(lambda user, size: None)

    def forward(settings):
        # P = 1; background, means3D, opacities, scales, rotations, the four camera arrays and out_color given, SHs and precomputed colours not
        rc = L.stp_forward(null_alloc, None, null_alloc, None, null_alloc, None, 1, 0, 0, p, 16, 16, settings,
                           p, None, None, p, p, 1.0, p, None, p, p, p, p, 1.0, 1.0, 0, p, None, 0, None)
        return rc, L.stp_last_error().decode()

    refusal = ("alpha output / per-pixel background (stp_set_forward_background) are not available with the debug depth visualisation: "
               "its image is not C + T * background")
    # case A: the request is refused with the depth visualisation -- and consumed by the refused call
    L.stp_set_forward_background(p, p)
    rc, msg = forward(ctypes.addressof(s))
    assert rc == -1 and msg == refusal
    rc, msg = forward(ctypes.addressof(s))
    assert rc == -1 and msg == "neither SHs nor precomputed colours given"
    # case B: a call refused at its very first check consumes the request too
    L.stp_set_forward_background(p, p)
    rc, msg = forward(None)
    assert rc == -1 and msg == "null settings or allocator"
    rc, msg = forward(ctypes.addressof(s))
    assert rc == -1 and msg == "neither SHs nor precomputed colours given"
