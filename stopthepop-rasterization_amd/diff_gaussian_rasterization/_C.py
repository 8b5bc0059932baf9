"""`diff_gaussian_rasterization._C` -- host binding of libstp_raster.so.

Mirrors the reference's pybind module of the same name (reference ext.cpp:15-19,
rasterize_points.cu:43-253): the three functions below take and return exactly the tensors the
reference's do, in the same order.  PyTorch is used for device memory and the current HIP stream only;
all compute is in the hand-written HIP library, reached through its C ABI (include/stp_raster.h).

The hot functions -- rasterize_gaussians, rasterize_gaussians_backward, mark_visible and the scratch pool -- live in
the native module `_stp_host` (csrc/host/stp_torch_binding.cpp: a plain C++ torch extension built by g++, no kernels,
no hipify pass; it allocates through ATen, takes the current stream from c10 and calls the same C ABI).  What stays here
is cold: the settings POD for the introspection helpers, the backward-mode policy, the stage timer's readers (ctypes).

There is NO fallback: if the library or the native module is missing, or the tensors are not on a GPU, these functions raise.
"""
from __future__ import annotations

import ctypes
import os
from typing import Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_NAME = "libstp_raster.so"
_lib = None
_host = None   # the native module _stp_host, bound to the same library file as _lib


GRAD_RECORD_FLOATS = 16  # == STP_GRAD_RECORD_FLOATS (include/stp_raster.h): floats per Gaussian in the backward's hand-over buffer


class StpSettings(ctypes.Structure):
    """POD mirror of StpSettings (include/stp_raster.h) == reference SplattingSettings (rasterizer.h:129-135)."""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "sort_mode", "sort_order", "queue_tile_4x4", "queue_tile_2x2", "queue_per_pixel",
        "rect_bounding", "tight_opacity_bounding", "tile_based_culling", "hierarchical_4x4_culling",
        "load_balancing", "proper_ewa_scaling", "tile_y0", "tile_y1", "record_blend_log", "debug_visualization")]


_lib_override = None

# exports newer than ABI 7's first release: resolved when present (name -> (argtypes, restype, the feature it came with: the rebuild message names it))
_OPTIONAL_SYMBOLS = {
    "stp_camera_grad_workspace_bytes": ([ctypes.c_int], ctypes.c_size_t, "camera gradients"),
    "stp_set_backward_camera_grads": ([ctypes.c_void_p] * 4 + [ctypes.c_size_t], None, "camera gradients"),
    "stp_set_backward_absgrad": ([ctypes.c_void_p], None, "absgrad"),
    "stp_set_backward_blend_stats": ([ctypes.c_void_p], None, "blend statistics"),
    "stp_set_forward_background": ([ctypes.c_void_p] * 2, None, "the alpha output and per-pixel background"),
    "stp_set_backward_background": ([ctypes.c_void_p] * 3, None, "the alpha output and per-pixel background"),
    "stp_set_forward_invdepth": ([ctypes.c_void_p], None, "the inverse-depth output"),
    "stp_set_backward_invdepth": ([ctypes.c_void_p] * 2, None, "the inverse-depth output"),
    "stp_set_forward_split_sh": ([ctypes.c_void_p], None, "split SH inputs"),
    "stp_set_backward_split_sh": ([ctypes.c_void_p] * 2, None, "split SH inputs"),
    "stp_set_forward_sh_stash": ([ctypes.c_int], None, "the SH stash"),
    "stp_set_forward_raw_params": ([ctypes.c_int], None, "raw parameter inputs"),
    "stp_set_backward_raw_params": ([ctypes.c_int], None, "raw parameter inputs"),
    "stp_activate_params": ([ctypes.c_int] + [ctypes.c_void_p] * 7, ctypes.c_int, "raw parameter inputs"),
    "stp_geometry_buffer_size_stash": ([ctypes.c_int, ctypes.POINTER(StpSettings)], ctypes.c_size_t, "the SH stash"),
    "stp_sparse_adam": ([ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p],
                        ctypes.c_int, "the sparse Adam step"),
    "stp_dense_adam": ([ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int, "the dense Adam step"),
    "stp_mcmc_relocation": ([ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3, ctypes.c_int, "the 3DGS-MCMC kernels"),
    "stp_mcmc_add_noise": ([ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_float] * 3 + [ctypes.c_int, ctypes.c_void_p], ctypes.c_int, "the 3DGS-MCMC kernels"),
    "stp_mcmc_relocate_scratch_bytes": ([ctypes.c_int], ctypes.c_size_t, "the 3DGS-MCMC relocation kernels"),
    "stp_mcmc_sample": ([ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_size_t] + [ctypes.c_void_p] * 4,
                        ctypes.c_int, "the 3DGS-MCMC relocation kernels"),
    "stp_mcmc_relocate_apply": ([ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t,
                                 ctypes.c_void_p], ctypes.c_int, "the 3DGS-MCMC relocation kernels"),
    "stp_mcmc_add_apply": ([ctypes.c_int] * 2 + [ctypes.c_void_p] * 2 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p],
                           ctypes.c_int, "the 3DGS-MCMC relocation kernels"),
    "stp_mip_filter_3d": ([ctypes.c_int] * 2 + [ctypes.c_void_p] * 6, ctypes.c_int, "the Mip-Splatting 3D filter"),
    "stp_mip_activations_forward": ([ctypes.c_int] + [ctypes.c_void_p] * 6, ctypes.c_int, "the Mip-Splatting 3D filter"),
    "stp_mip_activations_backward": ([ctypes.c_int] + [ctypes.c_void_p] * 8, ctypes.c_int, "the Mip-Splatting 3D filter"),
    "stp_knn_scratch_bytes": ([ctypes.c_int], ctypes.c_size_t, "the nearest-neighbour kernels"),
    "stp_knn_mean_dist2": ([ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_size_t] + [ctypes.c_void_p] * 2, ctypes.c_int, "the nearest-neighbour kernels"),
    "stp_spatial_order_scratch_bytes": ([ctypes.c_int], ctypes.c_size_t, "the spatial order kernels"),
    "stp_spatial_order": ([ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3, ctypes.c_int, "the spatial order kernels"),
    "stp_gather_rows": ([ctypes.c_int] * 2 + [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 2, ctypes.c_int, "the spatial order kernels"),
    "stp_densify_stats": ([ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p], ctypes.c_int, "the densification kernels"),
    "stp_densify_plan": ([ctypes.c_int] + [ctypes.c_void_p] * 8, ctypes.c_int, "the densification kernels"),
    "stp_densify_scratch_bytes": ([ctypes.c_int], ctypes.c_size_t, "the densification kernels"),
    "stp_densify_scan": ([ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_size_t] + [ctypes.c_void_p] * 3, ctypes.c_int, "the densification kernels"),
    "stp_densify_apply": ([ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_float, ctypes.c_int, ctypes.c_void_p],
                          ctypes.c_int, "the densification kernels"),
    "stp_photometric_workspace_floats": ([ctypes.c_int] * 3, ctypes.c_size_t, "the photometric loss"),
    "stp_photometric_forward": ([ctypes.c_int] * 3 + [ctypes.c_void_p] * 6, ctypes.c_int, "the photometric loss"),
    "stp_photometric_backward": ([ctypes.c_int] * 3 + [ctypes.c_void_p] * 6, ctypes.c_int, "the photometric loss"),
    "stp_training_loss_workspace_floats": ([ctypes.c_int] * 4, ctypes.c_size_t, "the training loss"),
    "stp_training_loss_forward": ([ctypes.c_int] * 3 + [ctypes.c_void_p] * 7, ctypes.c_int, "the training loss"),
    "stp_training_loss_backward": ([ctypes.c_int] * 3 + [ctypes.c_void_p] * 10, ctypes.c_int, "the training loss"),
}
_SYMBOL_FEATURE = {name: entry[2] for name, entry in _OPTIONAL_SYMBOLS.items()}   # (a view of the table above)


def _require(name: str):
    """An optional export of the loaded library; RuntimeError naming it when the library predates it."""
    L = _load()
    if not hasattr(L, name):
        raise RuntimeError(f"{library_path()} does not export {name} (a library built before {_OPTIONAL_SYMBOLS[name][2]}): rebuild it")
    return getattr(L, name)


def camera_grad_workspace_bytes(P: int) -> int:
    """Bytes of the device workspace a backward with camera gradients needs for P Gaussians (include/stp_raster.h)."""
    return int(_require("stp_camera_grad_workspace_bytes")(int(P)))


def library_path() -> str:
    p = _lib_override or os.environ.get("STP_RASTER_LIB", os.path.join(_HERE, _LIB_NAME))
    return os.path.join(_HERE, "libstp_raster_fma.so") if p == "fma" else p   # (STP_RASTER_LIB=fma: the shipped second build, by name)


def use_library(path=None) -> None:
    """The next call loads `path` instead of the default library (None: back to the default).  `path` may be a file or one of the
    shipped builds by name: "fma" = libstp_raster_fma.so (depth keys as fused multiply-add chains: 1.4-3 % faster, keys an ulp off the
    reference's now and then), "default" = libstp_raster.so (the reference's uncontracted depth keys)."""
    global _lib, _host, _lib_override
    if path in ("fma", "default"):
        path = os.path.join(_HERE, "libstp_raster_fma.so" if path == "fma" else _LIB_NAME)
    _lib, _host, _lib_override = None, None, path


def _load():
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `make -C stopthepop-rasterization_amd/csrc` "
            f"(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    L = ctypes.CDLL(path)
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    # (stp_forward / stp_backward_phases / stp_mark_visible are called by the native module _stp_host, not from here)
    L.stp_last_error.restype = ctypes.c_char_p
    L.stp_abi_version.restype = ci
    for name in ("stp_geometry_buffer_size", "stp_binning_buffer_size", "stp_image_buffer_size"):
        getattr(L, name).restype = ctypes.c_size_t
    L.stp_geometry_buffer_size.argtypes = [ci, ctypes.POINTER(StpSettings)]
    L.stp_binning_buffer_size.argtypes = [ci]
    L.stp_image_buffer_size.argtypes = [ci, ci]
    L.stp_blend_log_bytes.argtypes = [ci, ci]
    L.stp_blend_log_bytes.restype = ctypes.c_size_t
    szp = ctypes.POINTER(ctypes.c_size_t)
    L.stp_geometry_layout.argtypes = [ci, ctypes.POINTER(StpSettings), ctypes.c_char_p, szp, szp]
    L.stp_binning_layout.argtypes = [ci, ctypes.c_char_p, szp, szp]
    L.stp_image_layout.argtypes = [ci, ci, ctypes.c_char_p, szp, szp]
    L.stp_timing_enable.argtypes = [ci]
    L.stp_timing_enable.restype = None
    L.stp_timing_read.argtypes = [ctypes.POINTER(ctypes.c_float)]
    L.stp_timing_read.restype = ci
    L.stp_hbm_probe.argtypes = [ci, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ci, ctypes.c_void_p]
    L.stp_hbm_probe.restype = ci
    L.stp_timing_history.argtypes = [ctypes.POINTER(ctypes.c_float), ci]
    L.stp_timing_history.restype = ci
    L.stp_timing_history_host.argtypes = [ctypes.POINTER(ctypes.c_float), ci]
    L.stp_timing_history_host.restype = ci
    L.stp_timing_text.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.stp_timing_text.restype = ctypes.c_size_t
    L.stp_binning_layout_count.argtypes = [vp, ci]
    L.stp_binning_layout_count.restype = ci
    L.stp_forget_buffer.argtypes = [vp]
    L.stp_forget_buffer.restype = None
    for name in _OPTIONAL_SYMBOLS:   # (an older library without them still loads: camera_grad_workspace_bytes / camera_grads=True raise)
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = _OPTIONAL_SYMBOLS[name][:2]
    if L.stp_abi_version() != 7:
        raise ImportError("libstp_raster.so ABI version mismatch")
    _lib = L
    return L


def _native():
    """The native module, bound to the library file _load() resolved."""
    global _host
    if _host is not None:
        return _host
    _load()
    try:
        from . import _stp_host
    except ImportError as ex:
        raise ImportError(f"the native host binding diff_gaussian_rasterization._stp_host is missing ({ex}): build it with "
                          f"`python stopthepop-rasterization_amd/csrc/host/build_host.py` (or python -c 'import __graft_entry__ as g; "
                          f"g.build()').  There is no pure-Python fallback.") from ex
    _stp_host.load_library(library_path())
    global _atexit_registered
    if not _atexit_registered:   # pooled tensors must not outlive the HIP runtime at interpreter shutdown
        import atexit
        atexit.register(lambda: _stp_host.clear_scratch_pool(-1))
        _atexit_registered = True
    _host = _stp_host
    return _host


_atexit_registered = False


def settings_from_dict(d: dict, tile_rows=None) -> StpSettings:
    """dict -> POD.  All keys are mandatory, as in the reference's json parser (rasterizer.h:160-182,
    every field read with .at()); a missing key raises KeyError where the reference raised json::out_of_range."""
    ss, cs = d["sort_settings"], d["culling_settings"]
    q = ss["queue_sizes"]
    s = StpSettings()
    s.sort_mode = int(ss["sort_mode"])
    s.sort_order = int(ss["sort_order"])
    s.queue_tile_4x4 = int(q["tile_4x4"])
    s.queue_tile_2x2 = int(q["tile_2x2"])
    s.queue_per_pixel = int(q["per_pixel"])
    s.rect_bounding = int(bool(cs["rect_bounding"]))
    s.tight_opacity_bounding = int(bool(cs["tight_opacity_bounding"]))
    s.tile_based_culling = int(bool(cs["tile_based_culling"]))
    s.hierarchical_4x4_culling = int(bool(cs["hierarchical_4x4_culling"]))
    s.load_balancing = int(bool(d["load_balancing"]))
    s.proper_ewa_scaling = int(bool(d["proper_ewa_scaling"]))
    tr = tile_rows if tile_rows is not None else d.get("_tile_rows")
    if tr is not None:
        s.tile_y0, s.tile_y1 = int(tr[0]), int(tr[1])
    if _records_log(d):
        s.record_blend_log = 1
    return s


# ---- backward-mode policy (blend log: 512 B per pixel of the tile grid held between forward and backward) ----------
# "replay"  every training forward records the blend log, the backward replays it (fastest; default)
# "resort"  no log: the backward re-runs the per-pixel resort like the reference's (12 B per pixel held instead of 512)
# "auto"    record while the logs held by live autograd graphs + the pooled free buffers + the new log stay within
#           the byte budget, otherwise this forward falls back to "resort" (a trainer that sums K views before one
#           backward holds K logs)
# The process-wide default comes from STP_BACKWARD, read ONCE at import; set_backward_mode() changes it at run time and a
# settings object can override it per call (ExtendedSettings._backward_mode, see __init__.py).
_BACKWARD_MODES = ("replay", "resort", "auto")
_backward_mode = os.environ.get("STP_BACKWARD", "replay")
if _backward_mode not in _BACKWARD_MODES:
    raise ImportError(f"STP_BACKWARD={_backward_mode!r}: expected one of {_BACKWARD_MODES}")
_log_budget_bytes = int(float(os.environ.get("STP_LOG_BUDGET_GB", "16")) * (1 << 30))
_log_live = {}               # device index -> bytes of blend logs held by forwards whose backward has not run yet


def set_backward_mode(mode: str, log_budget_bytes=None) -> None:
    """Process-wide default of the policy above; `log_budget_bytes` (mode "auto") bounds live + pooled + new log bytes per device."""
    global _backward_mode, _log_budget_bytes
    if mode not in _BACKWARD_MODES:
        raise ValueError(f"backward mode {mode!r}: expected one of {_BACKWARD_MODES}")
    _backward_mode = mode
    if log_budget_bytes is not None:
        _log_budget_bytes = int(log_budget_bytes)


def backward_mode() -> str:
    return _backward_mode


def blend_log_bytes(width: int, height: int, tile_rows=None, depth=None) -> int:
    """Bytes of the blend log of one forward at this resolution.  depth = None: of a frame nothing is known about (400 B per pixel of the
    16x16 tile grid; later frames of the same kind get the depth their predecessors needed: blend_log_depth); depth = n: of a log of n
    records per pixel; depth = 0: of the DEEPEST log a forward may carve (what a memory policy has to budget before the forward has run).
    tile_rows = (y0, y1): of a forward restricted to that tile-row window (a rank of a tile-row shard holds its rows' log only)."""
    L = _load()
    y0, y1 = (0, 0) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
    if depth is not None:
        L.stp_blend_log_bytes_depth.argtypes = [ctypes.c_int] * 5
        L.stp_blend_log_bytes_depth.restype = ctypes.c_size_t
        return int(L.stp_blend_log_bytes_depth(int(width), int(height), y0, y1, int(depth)))
    if tile_rows is None:
        return int(L.stp_blend_log_bytes(int(width), int(height)))
    L.stp_blend_log_bytes_rows.argtypes = [ctypes.c_int] * 4
    L.stp_blend_log_bytes_rows.restype = ctypes.c_size_t
    return int(L.stp_blend_log_bytes_rows(int(width), int(height), y0, y1))


class LogLease:
    """Accounts one forward's blend log against the device's budget until its backward has run -- or until the autograd
    graph that holds it is dropped without one (the lease is an attribute of the graph node: it dies with it)."""

    def __init__(self, index: int, nbytes: int):
        self.index, self.nbytes = index, int(nbytes)
        _log_live[index] = _log_live.get(index, 0) + self.nbytes

    def resize(self, nbytes: int) -> None:
        """The forward has run: account what its log really takes (the library chooses the depth per frame)."""
        if self.nbytes:
            _log_live[self.index] = _log_live.get(self.index, 0) - self.nbytes + int(nbytes)
            self.nbytes = int(nbytes)

    def release(self) -> None:
        if self.nbytes:
            _log_live[self.index] = _log_live.get(self.index, 0) - self.nbytes
            self.nbytes = 0

    __del__ = release


def live_log_bytes(device=None) -> int:
    return _log_live.get(_device_index(device), 0)


def decide_recording(mode, device, width: int, height: int, tile_rows=None) -> bool:
    """Does a training forward on `device` record the blend log under policy `mode` (None = the process default)?"""
    mode = mode or _backward_mode
    if mode not in _BACKWARD_MODES:
        raise ValueError(f"backward mode {mode!r}: expected one of {_BACKWARD_MODES}")
    if mode != "auto":
        return mode == "replay"
    idx = _device_index(device)
    need = blend_log_bytes(width, height, tile_rows, depth=0)   # (the deepest log the forward may carve: its depth is the library's choice)
    pooled = list(_native().pooled_sizes(idx))
    reuse = any(need <= n for n in pooled)   # a pooled buffer takes the new log: no new memory
    return _log_live.get(idx, 0) + sum(pooled) + (0 if reuse else need) <= _log_budget_bytes


def _on_device(device):
    """Context that makes `device` the calling thread's current HIP device (nothing to switch on a box without a GPU)."""
    import contextlib
    return torch.cuda.device(_device_index(device)) if torch.cuda.is_available() else contextlib.nullcontext()


def _device_index(device) -> int:
    if device is None:
        return torch.cuda.current_device()
    if isinstance(device, int):
        return device
    d = torch.device(device)
    return torch.cuda.current_device() if d.index is None else d.index


def _raise_last(rc: int):
    msg = _load().stp_last_error()
    raise RuntimeError((msg.decode() if msg else "") or f"libstp_raster error {rc}")


# ---- scratch pool (csrc/host/stp_scratch_pool.h: buffers of >= 256 MiB -- tile lists with their entry records, image
# ---- state with the blend log -- are kept on a free list per device instead of cycling through torch's caching allocator)
def clear_scratch_pool(device=None) -> int:
    """Drops the pooled scratch buffers (tile lists / blend logs waiting for reuse) of `device` (all devices when None) so
    that torch.cuda.empty_cache() can hand their memory back; returns the number of bytes released.  Buffers that a live
    autograd graph still holds are not affected."""
    return int(_native().clear_scratch_pool(-1 if device is None else _device_index(device)))   # ('cuda' = the current device)


def set_scratch_pool_limit(max_buffers: int = 4, max_bytes=None) -> None:
    """Bounds the free list: at most `max_buffers` buffers and (optionally) `max_bytes` bytes per device stay pooled."""
    _native().set_scratch_pool_limit(int(max_buffers), -1 if max_bytes is None else int(max_bytes))


def scratch_generation(buf: torch.Tensor) -> int:
    """Token the autograd function keeps with a pooled buffer (0 for ordinary ones); see check_scratch."""
    return int(_native().scratch_generation(buf))


def check_scratch(buf: torch.Tensor, generation: int) -> None:
    """A second backward through a retained graph after a later forward reused the buffer must not read that
    forward's blend log: fail loudly instead."""
    _native().check_scratch(buf, int(generation))


def set_forward_split(tile_row: int, event) -> None:
    """The next rasterize_gaussians of this thread launches its render kernel for the tile rows below `tile_row` first and records `event`
    (a torch.cuda.Event that has been recorded once, so that its handle exists) on the current stream before it launches the rest
    (include/stp_raster.h: stp_set_forward_split; tile_shard.py sends the first half of a strip behind it)."""
    _native().set_forward_split(int(tile_row), 0 if event is None else int(event.cuda_event))   # (None: clear a pending request)


def release_scratch(buf: torch.Tensor) -> None:
    """Hand a pooled buffer back after the backward that consumed it (reuse is ordered behind the releasing stream)."""
    _native().release_scratch(buf)


def _records_log(d: dict) -> bool:
    # private key set by the autograd function for training forwards (see __init__._RasterizeGaussians.forward, which
    # applies the backward-mode policy above); mode "resort" forces the reference-style re-sorting backward everywhere
    return bool(d.get("_record_blend_log")) and d.get("_backward_mode", _backward_mode) != "resort"


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, inv_viewprojmatrix, tan_fovx, tan_fovy, image_height, image_width,
                        sh, degree, campos, prefiltered, settings_dict, render_depth, debug, alpha=False, invdepth=False,
                        raw=0, dc=None) -> Tuple[int, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """== RasterizeGaussiansCUDA (reference rasterize_points.cu:43-138).
    Returns (num_rendered, out_color (3,H,W), radii (P,) int32, geomBuffer, binningBuffer, imgBuffer).

    alpha=True (extension, include/stp_raster.h: stp_set_forward_background): one more tensor, LAST in the tuple: alpha = 1 - final_T,
    (1,H,W) float32 (zeros for P == 0).  A `background` of shape exactly (3,H,W) is composed per pixel, out = C + final_T * background;
    every other background is read as three floats.  Neither is available with render_depth.

    invdepth=True (extension, include/stp_raster.h: stp_set_forward_invdepth): one more tensor, LAST in the tuple (behind alpha's): the
    inverse-depth image sum_i alpha_i T_i / z_i over the pairs the colour blends, z_i the view-space z of Gaussian i's centre; (1,H,W)
    float32, no background term (zeros where nothing blended, and for P == 0).  Not available with render_depth.

    dc=(P,1,3) or (P,3) tensor (keyword; extension, include/stp_raster.h: stp_set_forward_split_sh): the first SH coefficient as a tensor of
    its own (a trainer's _features_dc); `sh` is then the rest, (P,M-1,3) (_features_rest; empty for a degree-0 model).  No concatenated copy
    is made, and every output equals that of the call on torch.cat((dc, rest), 1) bit for bit.  Ignored with precomputed colours.

    raw=mask (keyword; extension, include/stp_raster.h: stp_set_forward_raw_params): bit 0 `opacity`, bit 1 `scales`, bit 2 `rotations` hold a
    trainer's raw parameters (logit, log, unnormalised quaternion); the kernel activates them at its load and every output equals that of the
    call on activate_params' copies bit for bit.  A mask outside 0..7 or a bit whose tensor is empty raises, naming the bit."""
    if means3D.dim() != 2 or means3D.size(1) != 3:   # (the reference's first check, rasterize_points.cu:69-71)
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if alpha or _per_pixel_background(background, image_height, image_width):
        _require("stp_set_forward_background")
    if invdepth:
        _require("stp_set_forward_invdepth")
        if render_depth:
            raise RuntimeError("the inverse-depth output (_invdepth) is not available with render_depth (the debug depth visualisation)")
    if dc is not None:
        _require("stp_set_forward_split_sh")
    if raw:
        _require("stp_set_forward_raw_params")
    out = (_host or _native()).rasterize_gaussians(
        background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
        inv_viewprojmatrix, tan_fovx, tan_fovy, int(image_height), int(image_width), sh, int(degree), campos, bool(prefiltered),
        settings_dict, bool(render_depth), bool(debug), _records_log(settings_dict), bool(alpha), bool(invdepth), dc, int(raw))
    return tuple(out[:6]) + ((out[6],) if alpha else ()) + ((out[7],) if invdepth else ())


def _per_pixel_background(background, height, width) -> bool:
    """A background of shape exactly (3, H, W) is a per-pixel one; every other is read as three floats."""
    return isinstance(background, torch.Tensor) and tuple(background.shape) == (3, int(height), int(width))


def rasterize_gaussians_backward(background, means3D, radii, opacities, colors, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, inv_viewprojmatrix, tan_fovx, tan_fovy,
                                 pixel_colors, dL_dout_color, sh, degree, campos, geomBuffer, R, binningBuffer,
                                 imageBuffer, settings_dict, debug, phases=3, partial=None, chunk=None, outputs=None,
                                 camera_grads=False, absgrad=False, blend_stats=False, dL_dalpha=None, bg_grad=False,
                                 dL_dinvdepth=None, invdepth=None, raw=0, dc=None):
    """== RasterizeGaussiansBackwardCUDA (reference rasterize_points.cu:140-232).
    Returns (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations).

    camera_grads=True (extension, include/stp_raster.h: stp_set_backward_camera_grads): three more, dL_dviewmatrix, dL_dprojmatrix and
    dL_dcampos, in the shapes of viewmatrix / projmatrix / campos, from the same per-Gaussian intermediates (per-Gaussian half only; a
    chunked half refuses them).

    absgrad=True (extension, include/stp_raster.h: stp_set_backward_absgrad): one more tensor, LAST in the tuple: (P, 3) float32, columns
    0, 1 = the per-Gaussian sums over pixels of |that pixel's contribution to dL_dmeans2D| (x, y), column 2 zero.  Needs the per-Gaussian
    half and the padded (P, 16) records: compact records and a chunked half refuse it.

    blend_stats=True (extension, include/stp_raster.h: stp_set_backward_blend_stats): one more tensor, LAST in the tuple (behind absgrad's):
    (P, 3) float32, per Gaussian the sum, the maximum and the count of its blend weights alpha * T over the pixels.  The same conditions.

    dL_dalpha=(1,H,W) tensor (extension, include/stp_raster.h: stp_set_backward_background): the gradient of the forward's alpha output, which
    joins the weight of final_T in every pixel's loss.  bg_grad=True: one more tensor, LAST in the tuple (behind the statistics):
    dL/dbackground in the background's shape -- (3,) for a uniform background, (3,H,W) for a per-pixel one (a `background` of shape
    exactly (3,H,W), which must be the forward's).  The (3,) sum runs in a fixed order: equal inputs give bit-equal results.  Both need the
    render half (phases bit 0) and work with compact records; with phases=1 and bg_grad the result is (records, dL_dbackground).

    dL_dinvdepth=(1,H,W) tensor with invdepth=the forward's inverse-depth output (extension, include/stp_raster.h:
    stp_set_backward_invdepth): the gradient of that output joins the eight gradients (and the camera's) -- through the alphas like a colour
    gradient, and through 1 / z to dL_dmeans3D (and dL_dviewmatrix).  dL_dcolors / dL_dsh get nothing from it.  No extra result.  Needs both
    halves in one call and the padded records, like absgrad.

    dc=(P,1,3) or (P,3) tensor (keyword; extension, include/stp_raster.h: stp_set_backward_split_sh): the forward's split SH input; `sh` is the
    (P,M-1,3) rest.  dL_dsh, in its usual slot, is then (P,M-1,3), and one more tensor, dL_ddc (P,3), is LAST in the tuple, behind every
    extra above: (the eight) (the camera's three) (absgrad) (blend_stats) (dL_dbackground) (dL_ddc).  Both equal the two slices of the
    concatenated call's dL_dsh bit for bit.  Per-Gaussian half (phases bit 1); works chunked, `outputs` then carries nine tensors.

    raw=mask (keyword; extension, include/stp_raster.h: stp_set_backward_raw_params): the forward's mask.  dL_dopacity / dL_dscales /
    dL_drotations of its bits are then the gradients with respect to the RAW values (the chain rule of sigmoid / exp / normalize applied at the
    kernel's stores).  Per-Gaussian half (phases bit 1; ignored by a render-only call); works chunked and with compact records.

    Extension for tile-row sharding (not in the reference): phases=1 runs only the render half and
    returns its per-Gaussian partial sums as the library's (P,16) gradient records (stp_raster.h);
    phases=2 takes the records (after the caller's all-reduce) as `partial` and runs the preprocess half.
    Adding 4 to either selects COMPACT records, (P,9) with no padding: the tensor that is all-reduced as it is.
    chunk = (k, K) with phases=2: the per-Gaussian half on chunk k of K equal ranges of Gaussian ids (the shard all-reduces the records in
    K pieces and runs chunk k as soon as piece k has arrived); outputs = the tuple an earlier chunk returned (every chunk writes its rows)."""
    if chunk is not None:
        k, K = int(chunk[0]), int(chunk[1])
        if not (0 <= k < K <= 255) or (int(phases) & 1):
            raise ValueError("chunk = (k, K) with 0 <= k < K <= 255, per-Gaussian half only")
        phases = int(phases) | (K << 8) | (k << 16)
    if camera_grads:
        _require("stp_set_backward_camera_grads")
    if absgrad:
        _require("stp_set_backward_absgrad")
    if blend_stats:
        _require("stp_set_backward_blend_stats")
    if dL_dinvdepth is not None:
        _require("stp_set_backward_invdepth")
    if dc is not None:
        _require("stp_set_backward_split_sh")
    if raw:
        _require("stp_set_backward_raw_params")
    if dL_dalpha is not None or bg_grad or _per_pixel_background(background, dL_dout_color.shape[-2], dL_dout_color.shape[-1]):
        _require("stp_set_backward_background")
    out = (_host or _native()).rasterize_gaussians_backward(
        background, means3D, radii, opacities, colors, scales, rotations, scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
        inv_viewprojmatrix, tan_fovx, tan_fovy, pixel_colors, dL_dout_color, sh, int(degree), campos, geomBuffer, int(R), binningBuffer,
        imageBuffer, settings_dict, bool(debug), _records_log(settings_dict), int(phases), partial, None if outputs is None else list(outputs),
        bool(camera_grads), bool(absgrad), bool(blend_stats), dL_dalpha, bool(bg_grad), dL_dinvdepth, invdepth, dc, int(raw))
    return out[0] if (int(phases) & 3) == 1 and not bg_grad else tuple(out)


def mark_visible(means3D, viewmatrix, projmatrix) -> torch.Tensor:
    """== markVisible (reference rasterize_points.cu:234-253)."""
    return (_host or _native()).mark_visible(means3D, viewmatrix, projmatrix)


def sparse_adam(params, grads, exp_avgs, exp_avg_sqs, visible, lrs, epss, beta1, beta2, N) -> int:
    """The fused sparse Adam step (extension, include/stp_raster.h: stp_sparse_adam) of all the quadruples (param, grad, exp_avg, exp_avg_sq)
    in ONE library call on the current stream: rows i < N with visible[i] take  m <- b1 m + (1 - b1) g,  v <- b2 v + (1 - b2) g g,
    p <- p - lr m / (sqrt(v) + eps)  in place, every other row keeps its bits.  visible: bool / uint8 (non-zero = visible) or the int32 radii
    of the forward (> 0 = visible), N elements; lrs / epss: one value per tensor.  Returns the kernel launches made (one per eight tensors)."""
    _require("stp_sparse_adam")
    return int((_host or _native()).sparse_adam(list(params), list(grads), list(exp_avgs), list(exp_avg_sqs), visible, [float(x) for x in lrs],
                                                [float(x) for x in epss], float(beta1), float(beta2), int(N)))


def adamUpdate(param, grad, exp_avg, exp_avg_sq, visible, lr, b1, b2, eps, N, M) -> None:
    """The single-tensor step under the name and argument order of the accelerated rasterizer's `_C.adamUpdate`: a one-tensor sparse_adam
    (M, the floats per Gaussian, must be numel / N)."""
    if int(N) * int(M) != param.numel():
        raise RuntimeError(f"adamUpdate: param has {param.numel()} elements, N * M = {int(N) * int(M)}")
    sparse_adam([param], [grad], [exp_avg], [exp_avg_sq], visible, [lr], [eps], b1, b2, N)


DENSE_ADAM_REG_KINDS = {None: 0, "sigmoid": 1, "exp": 2}   # StpDenseAdamTensor.reg_kind


def dense_adam_coefficients(lr, beta1, beta2, eps, step, reg_weight=0.0, numel=1):
    """The eight coefficients of one tensor of stp_dense_adam as float64 values, in StpDenseAdamTensor's order: beta1, 1 - beta1, beta2, 1 - beta2,
    step_size = lr / (1 - beta1^step), bias2_sqrt = sqrt(1 - beta2^step), eps, reg_coef = reg_weight / numel.  Formed from the Python values as
    torch.optim.Adam forms them (1 - beta from the unrounded beta); the binding rounds each to float32 once.  step: the count AFTER this step."""
    beta1, beta2, step = float(beta1), float(beta2), float(step)
    return (beta1, 1.0 - beta1, beta2, 1.0 - beta2, float(lr) / (1.0 - beta1 ** step), (1.0 - beta2 ** step) ** 0.5, float(eps),
            float(reg_weight) / max(int(numel), 1))


def dense_adam(params, grads, exp_avgs, exp_avg_sqs, coefs, reg_kinds) -> int:
    """The fused dense Adam step (extension, include/stp_raster.h: stp_dense_adam) of all the quadruples (param, grad, exp_avg, exp_avg_sq) in
    ONE library call on the current stream: every element takes  g' = g + r,  m <- b1 m + (1 - b1) g',  v <- b2 v + (1 - b2) g' g',
    p <- p - step_size m / (sqrt(v) / bias2_sqrt + eps)  in place, with r = 0, reg_coef s (1 - s) (s = sigmoid(p)) or reg_coef exp(p).
    coefs: one dense_adam_coefficients() tuple per tensor; reg_kinds: 0, 1 (sigmoid) or 2 (exp) per tensor.  grads are only read.  Returns the
    kernel launches made (one per eight tensors with elements)."""
    _require("stp_dense_adam")
    flat = [float(x) for c in coefs for x in c]
    return int((_host or _native()).dense_adam(list(params), list(grads), list(exp_avgs), list(exp_avg_sqs), flat, [int(k) for k in reg_kinds]))


RELOCATION_N_MAX = 51   # upstream's N_max: N is clamped to [1, N_max - 1]


def compute_relocation(opacity_old, scale_old, N, binoms=None, n_max=RELOCATION_N_MAX):
    """The opacity and scales of each of N copies that replace a Gaussian (extension, include/stp_raster.h: stp_mcmc_relocation), under the
    name and argument order of the 3DGS-MCMC rasterizer's `_C.compute_relocation`: -> (opacity_new of opacity_old's shape, scale_new (n, 3)),
    float32, on the current stream.  opacity_old (n,) or (n, 1) and scale_old (n, 3) float32, N (n,) or (n, 1) int32 / int64, clamped to
    [1, n_max - 1] WITHOUT being modified.  binoms: upstream's (n_max, n_max) float32 table, n_max <= 51; its shape is checked and its
    CONTENTS ARE NOT READ -- the kernel forms its own binomials (exactly, in float64) -- so only n_max, the clamp's upper bound plus one, has
    an effect.  binoms=None: no table."""
    _require("stp_mcmc_relocation")
    return tuple((_host or _native()).compute_relocation(opacity_old, scale_old, N, binoms, int(n_max)))


def mcmc_add_noise(xyz, scales, rotations, opacities, noise, noise_scale, k, x0, raw) -> int:
    """The 3DGS-MCMC position noise in one pass, IN PLACE on xyz (extension, include/stp_raster.h: stp_mcmc_add_noise), on the current stream:
    xyz[i] += R diag(s^2) R^T (noise[i] * g * noise_scale), g = 1 / (1 + exp(-k ((1 - o) - x0))); raw: scales and opacities are the model's
    raw parameters (exp and sigmoid are applied in the kernel).  xyz (P, 3) contiguous, scales (P, 3), rotations (P, 4), opacities (P,) or
    (P, 1), noise (P, 3), all float32 on one GPU.  Returns the kernel launches made (1; 0 for P == 0)."""
    _require("stp_mcmc_add_noise")
    return int((_host or _native()).mcmc_add_noise(xyz, scales, rotations, opacities, noise, float(noise_scale), float(k), float(x0), bool(raw)))


class StpMcmcTensor(ctypes.Structure):
    """include/stp_raster.h: StpMcmcTensor and StpDensifyTensor, one layout (for callers of the C ABI through ctypes; the native module builds its own)"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("param", "exp_avg", "exp_avg_sq", "param_out", "exp_avg_out", "exp_avg_sq_out")] + \
               [("row", ctypes.c_int32), ("role", ctypes.c_int32)]


StpDensifyTensor = StpMcmcTensor

MCMC_ROLES = {"plain": 0, "opacity": 1, "scaling": 2}
MCMC_SAMPLE_TILE = 2048   # == STP_MCMC_SAMPLE_TILE (include/stp_raster.h): rows of a workgroup of the sampling's scan
MCMC_RELOCATE_MAX_P = 1 << 28


def mcmc_relocate_scratch_bytes(P: int) -> int:
    """Bytes of device scratch stp_mcmc_sample and the two applies need for P Gaussians (include/stp_raster.h): a function of P alone, 0 for a
    P the calls refuse (negative, above 2^28)."""
    return int(_require("stp_mcmc_relocate_scratch_bytes")(int(P)))


def mcmc_sample(opacity, uniforms, rule, min_opacity, raw, want_weights):
    """The draw of a relocation (rule 0: uniforms (P,), one per row, read on the dead rows) or of a growth (rule 1: uniforms (n,)) (extension,
    include/stp_raster.h: stp_mcmc_sample) -> (src int32, count int32 (P,), weights int32 (P,) or None), on the current stream, without host
    synchronisation."""
    _require("stp_mcmc_sample")
    src, count, weights = (_host or _native()).mcmc_sample(opacity, uniforms, int(rule), float(min_opacity), bool(raw), bool(want_weights))
    return src, count, (weights if want_weights else None)


def mcmc_relocate_apply(src, count, tensors, roles, exp_avgs, exp_avg_sqs, min_opacity, raw, reset_dead_moments) -> int:
    """The relocation by a plan, IN PLACE on every tensor and moment (extension, include/stp_raster.h: stp_mcmc_relocate_apply).  roles: 0 plain,
    1 opacity, 2 scaling; exp_avgs / exp_avg_sqs hold None where a tensor has no moments.  Returns the kernel launches made.  No host
    synchronisation."""
    _require("stp_mcmc_relocate_apply")
    return int((_host or _native()).mcmc_relocate_apply(src, count, list(tensors), [int(r) for r in roles], list(exp_avgs), list(exp_avg_sqs), float(min_opacity),
                                                        bool(raw), bool(reset_dead_moments)))


def mcmc_add_apply(src, count, tensors, roles, exp_avgs, exp_avg_sqs, min_opacity, raw):
    """The growth by a plan (extension, include/stp_raster.h: stp_mcmc_add_apply) -> (new_tensors, new_exp_avgs, new_exp_avg_sqs) of
    P + len(src) rows, lists as long as `tensors`.  No host synchronisation."""
    _require("stp_mcmc_add_apply")
    out = (_host or _native()).mcmc_add_apply(src, count, list(tensors), [int(r) for r in roles], list(exp_avgs), list(exp_avg_sqs), float(min_opacity), bool(raw))
    return list(out[0]), list(out[1]), list(out[2])


def activate_params(scaling=None, rotation=None, opacity=None):
    """The activated copies of a trainer's raw parameters (extension, include/stp_raster.h: stp_activate_params), on the current stream:
    -> (scales, rotations, opacities) = (exp(scaling), rotation / max(|rotation|, 1e-12), sigmoid(opacity)), fresh contiguous float32 tensors in
    the inputs' shapes, None for an absent input -- the values the rasterizer's raw= path renders with, to the bit.  scaling (P, 3),
    rotation (P, 4), opacity (P,) or (P, 1), float32 on one GPU.  One launch per tensor given."""
    if scaling is None and rotation is None and opacity is None:
        return None, None, None
    _require("stp_activate_params")
    out = (_host or _native()).activate_params(scaling, rotation, opacity)
    return tuple(o if given is not None else None for o, given in zip(out, (scaling, rotation, opacity)))


def compute_3d_filter(xyz, world_view_transforms, intrinsics):
    """Mip-Splatting's 3D filter over all cameras in one pass (extension, include/stp_raster.h: stp_mip_filter_3d), on the current stream, without
    host synchronisation: xyz (P, 3), world_view_transforms (C, 4, 4) in row-vector layout, intrinsics (C, 4) = (focal_x, focal_y, width,
    height), float32 on one GPU -> filter_3d (P, 1) float32.  P == 0 gives an empty tensor; C == 0 is refused."""
    _require("stp_mip_filter_3d")
    return (_host or _native()).compute_3d_filter(xyz, world_view_transforms, intrinsics)


def mip_activations(scaling, opacity, filter_3d):
    """(scales, opacities) of Mip-Splatting's filtered activations (extension, include/stp_raster.h: stp_mip_activations_forward): one launch on
    the current stream.  scaling (P, 3), opacity and filter_3d (P,) or (P, 1), float32 on one GPU; opacities has opacity's shape."""
    _require("stp_mip_activations_forward")
    return tuple((_host or _native()).mip_activations(scaling, opacity, filter_3d))


def mip_activations_backward(scaling, opacity, filter_3d, grad_scales, grad_opacities):
    """(grad_scaling, grad_opacity) of mip_activations (extension, include/stp_raster.h: stp_mip_activations_backward), recomputed from the three
    inputs: one launch.  grad_scales (P, 3) or grad_opacities (opacity's rows) may be None (zeros), not both."""
    _require("stp_mip_activations_backward")
    return tuple((_host or _native()).mip_activations_backward(scaling, opacity, filter_3d, grad_scales, grad_opacities))


KNN_BOX = 256   # == STP_KNN_BOX (include/stp_raster.h): points per box of the search, and lanes per workgroup


def knn_scratch_bytes(P: int) -> int:
    """Bytes of device scratch stp_knn_mean_dist2 needs for P points (include/stp_raster.h): a function of P alone, non-decreasing in P."""
    return int(_require("stp_knn_scratch_bytes")(int(P)))


def knn_mean_dist2(points):
    """simple_knn's distCUDA2 (extension, include/stp_raster.h: stp_knn_mean_dist2), on the current stream, without host synchronisation:
    points (P, 3) float32 on a GPU -> (P,) float32, the mean of the three smallest squared distances from each point to the others, in
    input order.  Exact, and the bits of a float32 brute force in the header's evaluation order.  P == 0 gives an empty tensor; P in 1..3
    is refused (there are no three neighbours)."""
    _require("stp_knn_mean_dist2")
    return (_host or _native()).knn_mean_dist2(points)


def spatial_order_scratch_bytes(P: int) -> int:
    """Bytes of device scratch stp_spatial_order needs for P points (include/stp_raster.h): a function of P alone, non-decreasing in P."""
    return int(_require("stp_spatial_order_scratch_bytes")(int(P)))


def spatial_order(xyz, return_codes=False):
    """The Morton order of a cloud (extension, include/stp_raster.h: stp_spatial_order), on the current stream, without host synchronisation:
    xyz (P, 3) float32 on a GPU -> (order, codes): order int32 (P,), order[s] the row that moves to position s; codes int32 (P,), the 30-bit
    code of the row at position s, or None when not asked for."""
    _require("stp_spatial_order")
    _require("stp_spatial_order_scratch_bytes")
    order, codes = (_host or _native()).spatial_order(xyz, bool(return_codes))
    return order, (codes if return_codes else None)


class StpGatherTensor(ctypes.Structure):
    """include/stp_raster.h: StpGatherTensor == StpDensifyTensor (for callers of the C ABI through ctypes; the native module builds its own)"""
    _fields_ = [(name, ctypes.c_void_p) for name in ("param", "exp_avg", "exp_avg_sq", "param_out", "exp_avg_out", "exp_avg_sq_out")] + \
               [("row", ctypes.c_int32), ("role", ctypes.c_int32)]


def gather_rows(index, tensors, exp_avgs, exp_avg_sqs):
    """Output row s of every tensor and moment is input row index[s], bit for bit (extension, include/stp_raster.h: stp_gather_rows) ->
    (new_tensors, new_exp_avgs, new_exp_avg_sqs), lists as long as `tensors`; exp_avgs / exp_avg_sqs hold None where a tensor has no moments,
    and so do the results.  index: int32 (M,).  No host synchronisation."""
    _require("stp_gather_rows")
    out = (_host or _native()).gather_rows(index, list(tensors), list(exp_avgs), list(exp_avg_sqs))
    return list(out[0]), list(out[1]), list(out[2])


class StpDensifyRule(ctypes.Structure):
    """include/stp_raster.h: StpDensifyRule (for callers of the C ABI through ctypes; the native module builds its own)"""
    _fields_ = [(name, ctypes.c_float) for name in ("grad_threshold", "split_size", "min_opacity", "max_screen_size", "max_world_size", "split_shrink")] + \
               [("raw", ctypes.c_int32), ("prune_big", ctypes.c_int32)]


DENSIFY_ROLES = {"plain": 0, "xyz": 1, "scaling": 2, "rotation": 3}


def densify_stats(xyz_gradient_accum, denom, max_radii2D, grad2d, radii) -> int:
    """A trainer's add_densification_stats in one launch, IN PLACE on the accumulators (extension, include/stp_raster.h: stp_densify_stats), on
    the current stream, without host synchronisation.  Returns the kernel launches made."""
    _require("stp_densify_stats")
    return int((_host or _native()).densify_stats(xyz_gradient_accum, denom, max_radii2D, grad2d, radii))


def densify_plan(xyz_gradient_accum, denom, scaling, opacity, max_radii2D, rule, raw, prune_big):
    """The plan byte of every Gaussian (extension, include/stp_raster.h: stp_densify_plan): uint8 (P,), bit 0 keep, bit 1 clone, bit 2 split.
    rule: the six floats of StpDensifyRule in its order.  No host synchronisation."""
    _require("stp_densify_plan")
    return (_host or _native()).densify_plan(xyz_gradient_accum, denom, scaling, opacity, max_radii2D, [float(x) for x in rule], bool(raw), bool(prune_big))


def densify_scan(plan):
    """plan -> (offsets, (nK, nC, nS)) (extension, include/stp_raster.h: stp_densify_scan): offsets is the int32 (3P,) tensor of destination rows
    densify_apply reads.  THIS CALL SYNCHRONISES the current stream with the host -- the one synchronisation of a densification: the new row
    count has to be known to allocate the outputs."""
    _require("stp_densify_scan")
    offsets, nK, nC, nS = (_host or _native()).densify_scan(plan)
    return offsets, (int(nK), int(nC), int(nS))


def densify_apply(plan, offsets, counts, tensors, roles, exp_avgs, exp_avg_sqs, noise, split_shrink, raw):
    """The new tensors and Adam moments of a plan (extension, include/stp_raster.h: stp_densify_apply) -> (new_tensors, new_exp_avgs,
    new_exp_avg_sqs), lists as long as `tensors`; exp_avgs / exp_avg_sqs hold None where a tensor has no moments, and so do the results.
    roles: 0 plain, 1 xyz, 2 scaling, 3 rotation.  noise: (2 nS, 3), may be None where nS == 0.  No host synchronisation."""
    _require("stp_densify_apply")
    out = (_host or _native()).densify_apply(plan, offsets, [int(c) for c in counts], list(tensors), [int(r) for r in roles], list(exp_avgs),
                                             list(exp_avg_sqs), noise, float(split_shrink), bool(raw))
    return list(out[0]), list(out[1]), list(out[2])


def photometric_forward(image, target, want_maps):
    """The forward of the fused photometric loss (extension, include/stp_raster.h: stp_photometric_forward) on the current stream:
    (out2, maps) with out2 = [mean |image - target|, mean SSIM(image, target)] (float32, on the device) and maps = the three derivative
    maps (3, *image.shape) the backward reads, or None when want_maps is false.  image, target: float32 (C, H, W) or (B, C, H, W) of equal
    shape on one GPU; non-contiguous ones are made contiguous.  Two kernel launches, no host synchronisation."""
    for name in ("stp_photometric_workspace_floats", "stp_photometric_forward", "stp_photometric_backward"):
        _require(name)
    out2, maps = (_host or _native()).photometric_forward(image, target, bool(want_maps))
    return out2, (maps if want_maps else None)


def photometric_backward(image, target, maps, grad_out2):
    """dL/dimage of the fused photometric loss (stp_photometric_backward) from the maps of a forward with want_maps and grad_out2 = dL/dout2,
    two floats ON THE DEVICE (the kernel reads them there).  One kernel launch, no host synchronisation.  There is no gradient for target."""
    _require("stp_photometric_backward")
    return (_host or _native()).photometric_backward(image, target, maps, grad_out2)


class StpTrainingLoss(ctypes.Structure):
    """POD mirror of StpTrainingLoss (include/stp_raster.h): the optional inputs of stp_training_loss_forward / _backward."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("exposure", "alpha_mask", "invdepth", "mono_invdepth", "depth_mask")] + \
               [(n, ctypes.c_int32) for n in ("clamp", "exposure_batched", "alpha_mask_batched", "channels", "depth_planes")]


_TRAINING_LOSS_SYMBOLS = ("stp_training_loss_workspace_floats", "stp_training_loss_forward", "stp_training_loss_backward")


def training_loss_forward(image, target, exposure, clamp, alpha_mask, invdepth, mono_invdepth, depth_mask, want_maps):
    """The forward of the training loss (extension, include/stp_raster.h: stp_training_loss_forward) on the current stream: (out3, maps) with
    out3 = [mean |x'' - target|, mean SSIM(x'', target), mean |(invdepth - mono_invdepth) * depth_mask|] for x'' = the exposed, clamped and
    masked image, and maps = the three derivative maps (3, *image.shape) or None.  Every extra may be None.  Two kernel launches, no host
    synchronisation."""
    for name in _TRAINING_LOSS_SYMBOLS:
        _require(name)
    out3, maps = (_host or _native()).training_loss_forward(image, target, exposure, bool(clamp), alpha_mask, invdepth, mono_invdepth, depth_mask, bool(want_maps))
    return out3, (maps if want_maps else None)


def training_loss_backward(image, target, exposure, clamp, alpha_mask, invdepth, mono_invdepth, depth_mask, maps, grad_out3, want_exposure, want_invdepth):
    """(dL/dimage, dL/dexposure | None, dL/dinvdepth | None) of the training loss (stp_training_loss_backward) from the maps of a forward with
    want_maps and grad_out3 = dL/dout3, three floats ON THE DEVICE.  One kernel launch, two with dL/dexposure; no host synchronisation."""
    _require("stp_training_loss_backward")
    g_image, g_exposure, g_invdepth = (_host or _native()).training_loss_backward(image, target, exposure, bool(clamp), alpha_mask, invdepth, mono_invdepth, depth_mask,
                                                                                  maps, grad_out3, bool(want_exposure), bool(want_invdepth))
    return g_image, (g_exposure if want_exposure else None), (g_invdepth if want_invdepth else None)


# ---- introspection helpers (tests / bench; not part of the reference surface) -----------------------
_GEOM_TYPES = {"depths": torch.float32, "clamped": torch.uint8, "radii": torch.int32, "rects2D": torch.float32,
               "means2D": torch.float32, "cov3D": torch.float32, "cov3D_inv": torch.float32,
               "conic_opacity": torch.float32, "rgb": torch.float32, "tiles_touched": torch.int32,
               "point_offsets": torch.int32, "invz": torch.float32,
               "sh_stash": torch.float32}  # (9, P) planes; only in the buffer of a forward that stashed (stp_set_forward_sh_stash)
_BIN_TYPES = {"point_list": torch.int32, "point_list_unsorted": torch.int32, "keys": torch.int64, "keys_unsorted": torch.int64}
_IMG_TYPES = {"final_T": torch.float32, "n_contrib": torch.int32, "ranges": torch.int32, "tile_flags": torch.int32,
              "blend_log": torch.int16}  # the last two exist only in a buffer of a recording forward


def timing_text(device=None) -> str:
    """The reference's `timings_text` (what its viewer displays), from the stages measured on `device` since timing_enable(True)."""
    buf = ctypes.create_string_buffer(512)
    with _on_device(device):
        _load().stp_timing_text(buf, 512)
    return buf.value.decode()


def _view(buf: torch.Tensor, off: int, count: int, dtype) -> torch.Tensor:
    nbytes = count * torch.empty((), dtype=dtype).element_size()
    return buf[off:off + nbytes].view(dtype)


def has_sh_stash(geomBuffer, P, settings_dict) -> bool:
    """Does this geometry buffer carry an SH stash (include/stp_raster.h: stp_set_forward_sh_stash)?  Read from the three words the stashing
    forward leaves in the buffer's first 256 bytes (magic, P, ~P)."""
    if geomBuffer.numel() < 48:
        return False
    w = geomBuffer[32:44].view(torch.int32).cpu().tolist()
    return (w[0] & 0xFFFFFFFF) == 0x53505453 and (w[1] & 0xFFFFFFFF) == int(P) and (w[2] & 0xFFFFFFFF) == (~int(P) & 0xFFFFFFFF)


def geometry_array(geomBuffer, P, settings_dict, name):
    """Named view of a sub-array of the geometry buffer ("sh_stash": nine planes of P floats, present only where has_sh_stash says so)."""
    s = settings_from_dict(settings_dict)
    off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
    if _load().stp_geometry_layout(int(P), ctypes.byref(s), name.encode(), ctypes.byref(off), ctypes.byref(cnt)) != 0:
        raise KeyError(name)
    return _view(geomBuffer, off.value, cnt.value, _GEOM_TYPES[name])


def binning_array(binningBuffer, R, name):
    """Named view of the first R entries of a sub-array.  (A run-ahead forward carves the buffer for the capacity it guessed, not for
    num_rendered: the library remembers which, stp_binning_layout_count.)"""
    off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
    L = _load()
    if binningBuffer.is_cuda:
        _native().forget_unless_same_storage(binningBuffer)   # (a clone / recycled address is described by the header it carries, not by the address)
    lay = int(L.stp_binning_layout_count(ctypes.c_void_p(binningBuffer.data_ptr()), int(R))) if int(R) > 0 else 0
    if lay < 0:
        _raise_last(lay)
    if L.stp_binning_layout(lay, name.encode(), ctypes.byref(off), ctypes.byref(cnt)) != 0:
        raise KeyError(name)
    n = cnt.value // lay * int(R) if lay > 0 else cnt.value
    return _view(binningBuffer, off.value, n, _BIN_TYPES[name])


def image_array(imgBuffer, W, H, name, tile_rows=None):
    """Named view into an image buffer.  tile_rows = (y0, y1): the buffer of a forward restricted to that tile-row window -- it holds the
    window's pixel rows / tiles only (element 0 = the window's first pixel / tile).  "blend_log" is reported at the depth the buffer was
    carved with (its header: blend_log_depth)."""
    off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
    L = _load()
    L.stp_image_layout_depth.argtypes = [ctypes.c_int] * 5 + [ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    y0, y1 = (0, 0) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
    depth = blend_log_depth(imgBuffer) if name == "blend_log" else 0
    if L.stp_image_layout_depth(int(W), int(H), y0, y1, depth, name.encode(), ctypes.byref(off), ctypes.byref(cnt)) != 0:
        raise KeyError(name)
    return _view(imgBuffer, off.value, cnt.value, _IMG_TYPES[name])


def blend_log_depth(imgBuffer) -> int:
    """Records per pixel of the blend log in the image buffer of a recording forward (adaptive: include/stp_raster.h, stp_blend_log_bytes)."""
    L = _load()
    L.stp_blend_log_depth.argtypes = [ctypes.c_void_p]
    L.stp_blend_log_depth.restype = ctypes.c_int
    if imgBuffer.is_cuda:
        _native().forget_unless_same_storage(imgBuffer)
    d = int(L.stp_blend_log_depth(ctypes.c_void_p(imgBuffer.data_ptr())))
    if d < 0:
        _raise_last(d)
    return d


def set_run_ahead(mode) -> int:
    """Run-ahead forward: False / 0 = never, True / 1 = always, 2 = auto (small frames only; the default) -- include/stp_raster.h:
    stp_set_run_ahead.  Returns the previous mode."""
    L = _load()
    L.stp_set_run_ahead.argtypes = [ctypes.c_int]
    L.stp_set_run_ahead.restype = None
    L.stp_get_run_ahead.restype = ctypes.c_int
    prev = int(L.stp_get_run_ahead())
    L.stp_set_run_ahead(int(mode))
    return prev


def reset_size_guesses() -> None:
    """The next forward of every kind runs without a size guess (hand-over in the middle of the frame, exact binning request) -- tests."""
    L = _load()
    L.stp_reset_size_guesses.restype = None
    L.stp_reset_size_guesses()


def timing_enable(flag: bool) -> None:
    _load().stp_timing_enable(int(bool(flag)))


def hbm_probe(kind: str, dst, src, blocks: int = 4096, nontemporal: bool = False) -> None:
    """One launch of the library's float4 streaming kernel (`read` src, `write` dst, `copy` src -> dst) on torch's current stream: the
    box's HBM ceiling for a plain stream (bench.py `hbm_measured`)."""
    import torch
    t = src if src is not None else dst
    k = {"read": 0, "write": 1, "copy": 2}[kind] + (4 if nontemporal else 0)
    with _on_device(t.device):
        rc = _load().stp_hbm_probe(k, None if dst is None else dst.data_ptr(), None if src is None else src.data_ptr(),
                                   t.numel() * t.element_size(), int(blocks), torch.cuda.current_stream(t.device).cuda_stream)
    if rc < 0:
        raise RuntimeError(f"stp_hbm_probe failed ({rc})")


def timing_history(device=None, capacity=1024, host=False):
    """Stage times of the last (up to `capacity`) timed calls on `device`, one dict per forward(+backward) in chronological order;
    a stage that was not measured in a call is missing from its dict.  host=True: the launching thread's own time between the stage's two
    event records instead of the GPU interval (a long GPU interval with an equally long host one = the launches came late)."""
    arr = (ctypes.c_float * (6 * capacity))()
    with _on_device(device):
        n = (_load().stp_timing_history_host if host else _load().stp_timing_history)(arr, capacity)
    if n < 0:
        _raise_last(n)
    names = ("Preprocess", "Duplicate", "Sort", "Render", "BwdRender", "BwdPreprocess")
    return [{nm: float(arr[6 * k + i]) for i, nm in enumerate(names) if arr[6 * k + i] >= 0.0} for k in range(n)]


def timing_read(device=None):
    """Mean milliseconds of the stages timed on `device` (default: the current one) since timing_enable(True): Preprocess,
    Duplicate, Sort, Render, BwdRender, BwdPreprocess; -1 = not measured.  The library keeps one timer per device."""
    arr = (ctypes.c_float * 6)()
    with _on_device(device):
        rc = _load().stp_timing_read(arr)
    if rc < 0:
        _raise_last(rc)
    names = ("Preprocess", "Duplicate", "Sort", "Render", "BwdRender", "BwdPreprocess")
    return {n: float(v) for n, v in zip(names, arr)}
