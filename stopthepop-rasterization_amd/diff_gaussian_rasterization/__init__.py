"""diff_gaussian_rasterization -- MI355X-native drop-in for the StopThePop rasterizer's Python API.

Public surface (names, argument order, field order, defaults, error texts) follows the reference
package of the same name (reference diff_gaussian_rasterization/__init__.py):
  rasterize_gaussians            :32-53      _RasterizeGaussians (autograd.Function)  :55-172
  SortMode / GlobalSortOrder     :175-191    SortQueueSizes / SortSettings / CullingSettings / ExtendedSettings :193-246
  GaussianRasterizationSettings  :248-263    GaussianRasterizer (nn.Module)           :265-314
A trainer written against the reference imports this package unchanged.  The compute behind `_C` is the
hand-written HIP library (csrc/), reached through its C ABI; see _C.py.

Differences that do not change behaviour: the settings dataclasses use default_factory (the
reference's shared mutable defaults are rejected by Python >= 3.11); `dacite` is optional (only
ExtendedSettings.from_dict used it).
"""
from __future__ import annotations

import json
from dataclasses import asdict, dataclass, field, fields
from enum import IntEnum
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _C

__all__ = ["rasterize_gaussians", "SortMode", "GlobalSortOrder", "SortQueueSizes", "SortSettings", "CullingSettings",
           "ExtendedSettings", "GaussianRasterizationSettings", "GaussianRasterizer", "SparseGaussianAdam", "GaussianAdam",
           "photometric_terms", "fused_ssim", "photometric_loss", "training_terms", "training_loss", "compute_relocation", "mcmc_add_noise_",
           "knn_mean_dist2", "distCUDA2", "dist_cuda2", "activate_params",
           "densification_stats_", "densify_plan", "densify_tensors", "densify_and_prune",
           "mcmc_relocation_plan", "mcmc_relocate_tensors_", "mcmc_relocate_", "mcmc_add_plan", "mcmc_add_tensors", "mcmc_add_new",
           "spatial_order", "gather_tensors", "reorder_gaussians_", "compute_3d_filter", "filtered_activations"]


def enum_dict_factory(data):
    """asdict() factory that stores IntEnum members as plain ints (the C side reads ints)."""
    return {k: (v.value if isinstance(v, IntEnum) else v) for k, v in data}


def cpu_deep_copy_tuple(input_tuple):
    return tuple(item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, dc=None, raw=0):
    """dc (extension, include/stp_raster.h: stp_set_forward_split_sh): the first SH coefficient, (P, 1, 3) or (P, 3), as a tensor of its own;
    `sh` is then the rest, (P, M-1, 3).  It rides behind raster_settings in every Function, so that the inputs in front keep their places.
    raw (extension, include/stp_raster.h: stp_set_forward_raw_params): the mask of the raw parameter inputs (bit 0 opacities, bit 1 scales,
    bit 2 rotations).  It is no input of the Functions -- dc stays their last --: it rides on the settings tuple (_with_raw_mask); with a
    mask of 0 the tuple is the caller's own and the call is the one it always was."""
    if raw:
        raster_settings = _with_raw_mask(raster_settings, int(raw))
    rs = raster_settings
    if torch.is_grad_enabled() and isinstance(rs.bg, torch.Tensor) and rs.bg.requires_grad:
        # a learnable background: bg -- and the camera tensors, which get their gradients here too where they require them -- become explicit
        # inputs of a third Function
        return _RasterizeGaussiansBackground.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                                   rs.bg, rs.viewmatrix, rs.projmatrix, rs.campos, raster_settings, dc)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (rs.viewmatrix, rs.projmatrix, rs.campos)):
        # camera gradients (pose refinement): the camera tensors become explicit inputs of a second Function
        return _RasterizeGaussiansCamera.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                               rs.viewmatrix, rs.projmatrix, rs.campos, raster_settings, dc)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings, dc)


def _forward_body(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix, campos, rs,
                  save_camera=False, bg=None, dc=None):
    """The forward the autograd Functions share (the camera tensors are rs's own, or the camera Function's explicit inputs, which
    save_camera=True saves for the backward behind the twelve tensors every Function saves; bg: the background Function's explicit input,
    saved behind them; dc: the split SH input, saved behind those -- sh is then the rest --; the inverse-depth output stays LAST; a raw
    mask on rs (_with_raw_mask): opacities / scales / rotations are then saved as they came in, raw, and the backward recomputes the activations)."""
    sdict = rs.settings.to_dict()
    save_bg = bg is not None
    if bg is None:
        bg = rs.bg
    # alpha output and per-pixel background (extensions; include/stp_raster.h: stp_set_forward_background): settings._alpha = True adds
    # alpha = 1 - final_T, (1, H, W), as a third, differentiable output; a bg of shape exactly (3, H, W) is composed per pixel
    ctx.alpha = bool(sdict.get("_alpha"))
    if rs.render_depth and (ctx.alpha or save_bg or _C._per_pixel_background(bg, rs.image_height, rs.image_width)):
        # (save_bg: a bg that requires grad -- final_T * dL_dout is not the gradient of that image)
        raise RuntimeError("the alpha output (settings._alpha), a per-pixel background and a background that requires grad are not available "
                           "with render_depth=True: the depth visualisation's image is not C + T * background")
    # inverse-depth output (extension; include/stp_raster.h: stp_set_forward_invdepth): settings._invdepth = True adds
    # invdepth = sum alpha T / z, (1, H, W), as one more differentiable output, behind alpha where both are asked for
    ctx.invdepth = bool(sdict.get("_invdepth"))
    if ctx.invdepth and rs.render_depth:
        raise RuntimeError("the inverse-depth output (settings._invdepth) is not available with render_depth=True: the depth visualisation "
                           "replaces the image and has no backward")
    ctx.log_lease = None
    # absgrad (extension, settings._absgrad = True; include/stp_raster.h: stp_set_backward_absgrad): the backward also leaves the per-Gaussian
    # sums of |each pixel's contribution to dL/dmean2D| in means2D.absgrad -- the densification statistic of AbsGS / gsplat.  The tensor
    # the caller passed is kept (not saved: it takes no part in the maths) so that the backward can hang the attribute on it.
    ctx.absgrad_target = None
    if sdict.get("_absgrad"):
        if rs.render_depth:
            raise RuntimeError("absgrad (settings._absgrad) is not available with render_depth=True: the depth visualisation has no "
                               "backward that could produce it")
        ctx.absgrad_target = means2D
    # blend statistics (extension, settings._blend_stats = True; include/stp_raster.h: stp_set_backward_blend_stats): the backward also leaves
    # means2D.blend_stats, per Gaussian the sum, the maximum and the count of its blend weights alpha * T over the pixels -- what pruning
    # methods rank by.  A request of its own: with or without _absgrad.
    ctx.blend_stats_target = None
    if sdict.get("_blend_stats"):
        if rs.render_depth:
            raise RuntimeError("blend statistics (settings._blend_stats) are not available with render_depth=True: the depth visualisation "
                               "has no backward that could produce them")
        ctx.blend_stats_target = means2D
    if any(ctx.needs_input_grad) and not rs.render_depth:
        # a backward can follow: let the hierarchical / k-buffer forward record each pixel's blend order so that the
        # backward replays it instead of re-sorting (extension of ours; ignored by the other sort modes) -- unless the
        # backward-mode policy says otherwise (_C.set_backward_mode / STP_BACKWARD / settings._backward_mode: "resort",
        # or "auto" with the device's blend-log budget used up by forwards that still wait for their backward).
        # Not with render_depth: the depth-visualisation forward records no log, and a backward through it
        # (meaningless in the reference too, but memory-safe there) must take the re-sorting path.
        mode = sdict.get("_backward_mode")
        uses_log = int(sdict["sort_settings"]["sort_mode"]) in (2, 3)
        if uses_log and means3D.is_cuda and means3D.size(0) != 0 and _C.decide_recording(mode, means3D.device, rs.image_width, rs.image_height):
            sdict["_record_blend_log"] = True
            sdict["_backward_mode"] = "replay"
            ctx.log_lease = _C.LogLease(_C._device_index(means3D.device), _C.blend_log_bytes(rs.image_width, rs.image_height))
        else:
            sdict["_backward_mode"] = "resort"
        # ... and, whatever the backward mode, let the SH colour kernel keep the nine direction derivatives the per-Gaussian backward would
        # otherwise re-read the SH rows for (include/stp_raster.h: stp_set_forward_sh_stash)
        sdict["_sh_stash"] = True
    # gradients nobody receives (include/stp_raster.h: optional outputs of stp_backward): with SH coefficients / scale and rotation as inputs the
    # backward neither allocates nor writes dL_dcolors / dL_dcov3D (their slots of its result are None)
    if colors_precomp.numel() == 0:
        sdict["_no_grad_colors"] = True
    if cov3Ds_precomp.numel() == 0:
        sdict["_no_grad_cov3D"] = True
    ctx.settings_dict = sdict
    # positional layout of _C.rasterize_gaussians (22 arguments)
    args = (bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
            viewmatrix, projmatrix, rs.inv_viewprojmatrix, rs.tanfovx, rs.tanfovy, rs.image_height,
            rs.image_width, sh, rs.sh_degree, campos, rs.prefiltered, sdict, rs.render_depth,
            rs.debug)
    kw = {"alpha": True} if ctx.alpha else {}   # (the alpha tensor comes last)
    if ctx.invdepth:
        kw["invdepth"] = True                   # (... and the inverse depth behind it)
    # split SH (extension; include/stp_raster.h: stp_set_forward_split_sh): precomputed colours win, as in the library
    ctx.dc_index = None
    if dc is not None and colors_precomp.numel() == 0:
        kw["dc"] = dc
        ctx.dc_index = 12 + (3 if save_camera else 0) + (1 if save_bg else 0)
    # raw parameter inputs (extension; include/stp_raster.h: stp_set_forward_raw_params): the mask rides to the kernel, no activated copy is made
    ctx.raw = int(getattr(rs, "raw_mask", 0))
    if ctx.raw:
        kw["raw"] = ctx.raw
    if rs.debug:
        cpu_args = cpu_deep_copy_tuple(args + ((dc,) if "dc" in kw else ()) + ((ctx.raw,) if ctx.raw else ()))  # snapshot before anything can corrupt them (dc, then the raw mask: behind the 22)
        try:
            num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer, *extra = _C.rasterize_gaussians(*args, **kw)
        except Exception as ex:
            torch.save(cpu_args, "snapshot_fw.dump")
            print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
            raise ex
    else:
        num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer, *extra = _C.rasterize_gaussians(*args, **kw)

    if ctx.log_lease is not None:   # the library chose the log's depth for this frame: account what the buffer really holds
        ctx.log_lease.resize(_C.blend_log_bytes(rs.image_width, rs.image_height, depth=_C.blend_log_depth(imgBuffer)))
    ctx.raster_settings = rs
    ctx.num_rendered = num_rendered
    ctx.img_generation = _C.scratch_generation(imgBuffer)
    ctx.bin_generation = _C.scratch_generation(binningBuffer)
    ctx.save_for_backward(colors_precomp, means3D, opacities, scales, rotations, cov3Ds_precomp, radii, sh, color,
                          geomBuffer, binningBuffer, imgBuffer, *((viewmatrix, projmatrix, campos) if save_camera else ()),
                          *((bg,) if save_bg else ()), *((dc,) if ctx.dc_index is not None else ()),
                          *((extra[-1],) if ctx.invdepth else ()))   # (the inverse-depth output: LAST)
    # radii is an integer output: without these two lines autograd materialises a (P,) zero "gradient" for it in
    # every backward (a 4 MB fill kernel per step at 1 M Gaussians)
    ctx.mark_non_differentiable(radii)
    ctx.set_materialize_grads(False)
    return (color, radii, *extra)   # (alpha, invdepth: those that were asked for)


def _grad_alpha(ctx, rest):
    """The gradient of the alpha output among a backward's trailing arguments (None: alpha took no part in the loss, or there is none)."""
    return rest[0] if ctx.alpha and rest else None


def _grad_invdepth(ctx, rest):
    """The same for the inverse-depth output, which follows alpha's."""
    i = 1 if ctx.alpha else 0
    return rest[i] if ctx.invdepth and len(rest) > i else None


def _backward_body(ctx, grad_out_color, viewmatrix, projmatrix, campos, camera_grads=False, grad_alpha=None, bg=None, grad_invdepth=None):
    """The backward the autograd Functions share: the eight Gaussian gradients of _C.rasterize_gaussians_backward (+ the three camera
    gradients with camera_grads=True, + dL/dbg last with bg, the background Function's saved input).  With a split SH input the sixth
    gradient is the rest's, (P, M-1, 3), and ctx.grad_dc receives dc's in dc's own shape (None otherwise)."""
    num_rendered = ctx.num_rendered
    rs = ctx.raster_settings
    (colors_precomp, means3D, opacities, scales, rotations, cov3Ds_precomp, radii, sh, color, geomBuffer,
     binningBuffer, imgBuffer) = ctx.saved_tensors[:12]
    _C.check_scratch(imgBuffer, ctx.img_generation)
    _C.check_scratch(binningBuffer, ctx.bin_generation)
    if grad_out_color is None:  # (set_materialize_grads(False): a loss on the alpha output alone)
        grad_out_color = torch.zeros_like(color)
    bg_grad = bg is not None
    if bg is None:
        bg = rs.bg
    # positional layout of _C.rasterize_gaussians_backward (25 arguments)
    args = (bg, means3D, radii, opacities, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
            viewmatrix, projmatrix, rs.inv_viewprojmatrix, rs.tanfovx, rs.tanfovy, color, grad_out_color, sh,
            rs.sh_degree, campos, geomBuffer, num_rendered, binningBuffer, imgBuffer, ctx.settings_dict,
            rs.debug)
    kw = {"camera_grads": True} if camera_grads else {}
    if ctx.absgrad_target is not None:
        kw["absgrad"] = True
    if ctx.blend_stats_target is not None:
        kw["blend_stats"] = True
    if grad_alpha is not None:
        kw["dL_dalpha"] = grad_alpha
    if bg_grad:
        kw["bg_grad"] = True
    if grad_invdepth is not None:   # (None: the inverse depth took no part in the loss -- no pointer is set, the backward is what it is without)
        kw["dL_dinvdepth"] = grad_invdepth
        kw["invdepth"] = ctx.saved_tensors[-1]
    dc = ctx.saved_tensors[ctx.dc_index] if ctx.dc_index is not None else None
    if dc is not None:
        kw["dc"] = dc
    if ctx.raw:
        kw["raw"] = ctx.raw
    if rs.debug:
        cpu_args = cpu_deep_copy_tuple(args + ((dc,) if dc is not None else ()) + ((ctx.raw,) if ctx.raw else ()))
        try:
            out = _C.rasterize_gaussians_backward(*args, **kw)
        except Exception as ex:
            torch.save(cpu_args, "snapshot_bw.dump")
            print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
            raise ex
    else:
        out = _C.rasterize_gaussians_backward(*args, **kw)
    _C.release_scratch(imgBuffer); _C.release_scratch(binningBuffer)  # the blend log goes back to the library's free list
    if ctx.log_lease is not None:
        ctx.log_lease.release()
    # (the extra tensors come last, the statistics behind absgrad's, dL/dbg behind both, dL/ddc behind all; assigned, not accumulated: the
    # trainer keeps its own statistic)
    ctx.grad_dc = None
    if dc is not None:
        ctx.grad_dc = out[-1].view(dc.shape)   # ((P, 3) from the library: a fresh contiguous tensor in the input's own shape)
        out = out[:-1]
    grad_bg = None
    if bg_grad:
        grad_bg = out[-1]
        out = out[:-1]
        if grad_bg.shape != bg.shape:   # (a uniform background in another shape than (3,): its first three values are the colour)
            full = torch.zeros(bg.numel(), dtype=grad_bg.dtype, device=grad_bg.device)
            full[:3] = grad_bg
            grad_bg = full.reshape(bg.shape)
    if ctx.blend_stats_target is not None:
        ctx.blend_stats_target.blend_stats = out[-1]
        out = out[:-1]
    if ctx.absgrad_target is not None:
        ctx.absgrad_target.absgrad = out[-1]
        out = out[:-1]
    if ctx.raw:   # (the gradients of the raw leaves in the leaves' own shapes: an opacity of (P,) gets (P,), not the library's (P, 1))
        out = list(out)
        for i, t in ((2, opacities), (6, scales), (7, rotations)):
            if out[i] is not None and t.numel() != 0:
                out[i] = out[i].view(t.shape)
        out = tuple(out)
    return out + (grad_bg,) if bg_grad else out


def _split_grad_sh(ctx, grad_sh):
    """The rest's gradient of a split SH backward: None where the rest does not require grad."""
    return grad_sh if ctx.needs_input_grad[2] else None


def _split_grad_dc(ctx):
    """dc's gradient (dc is the LAST input of every Function): None where dc is absent or does not require grad."""
    return ctx.grad_dc if ctx.dc_index is not None and ctx.needs_input_grad[-1] else None


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, dc=None):
        rs = raster_settings
        return _forward_body(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, rs.viewmatrix,
                             rs.projmatrix, rs.campos, rs, dc=dc)

    @staticmethod
    def backward(ctx, grad_out_color, _, *rest):   # (rest: the alpha output's gradient, with settings._alpha)
        rs = ctx.raster_settings
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations) = _backward_body(ctx, grad_out_color, rs.viewmatrix, rs.projmatrix, rs.campos, grad_alpha=_grad_alpha(ctx, rest),
                                          grad_invdepth=_grad_invdepth(ctx, rest))
        # one gradient per forward input, in forward's order
        if ctx.dc_index is None:
            return (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales, grad_rotations,
                    grad_cov3Ds_precomp, None, None)
        # split SH: None for a frozen dc or rest
        return (grad_means3D, grad_means2D, _split_grad_sh(ctx, grad_sh), grad_colors_precomp, grad_opacities, grad_scales, grad_rotations,
                grad_cov3Ds_precomp, None, _split_grad_dc(ctx))


class _RasterizeGaussiansCamera(torch.autograd.Function):
    """_RasterizeGaussians with viewmatrix, projmatrix and campos as explicit inputs that get gradients (include/stp_raster.h:
    stp_set_backward_camera_grads).  rasterize_gaussians() routes here only while grad mode is on and one of the three requires grad.
    The three are independent inputs, as the forward reads them; inv_viewprojmatrix, the intrinsics and bg get none."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix, campos,
                raster_settings, dc=None):
        # (needs_input_grad counts the camera inputs: a frame where only the camera requires grad records the blend log too; the
        # camera tensors are saved like the Gaussians: an in-place change before the backward raises instead of giving wrong gradients)
        return _forward_body(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix,
                             campos, raster_settings, save_camera=True, dc=dc)

    @staticmethod
    def backward(ctx, grad_out_color, _, *rest):
        viewmatrix, projmatrix, campos = ctx.saved_tensors[12:15]
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales,
         grad_rotations, grad_view, grad_proj, grad_campos) = _backward_body(ctx, grad_out_color, viewmatrix, projmatrix, campos, True,
                                                                             grad_alpha=_grad_alpha(ctx, rest),
                                                                             grad_invdepth=_grad_invdepth(ctx, rest))
        grads = (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales, grad_rotations,
                 grad_cov3Ds_precomp, grad_view, grad_proj, grad_campos)
        # None for every input that does not require grad (frozen Gaussians: the camera's gradients only)
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad)) + (None, _split_grad_dc(ctx))


class _RasterizeGaussiansBackground(torch.autograd.Function):
    """_RasterizeGaussians with bg as an explicit input that gets a gradient (include/stp_raster.h: stp_set_backward_background): (3,) for a
    uniform background, (3, H, W) for a per-pixel one.  rasterize_gaussians() routes here only while grad mode is on and rs.bg requires
    grad.  viewmatrix, projmatrix and campos are explicit inputs too and get the camera gradients where they require grad."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, bg, viewmatrix, projmatrix, campos,
                raster_settings, dc=None):
        return _forward_body(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix,
                             campos, raster_settings, save_camera=True, bg=bg, dc=dc)

    @staticmethod
    def backward(ctx, grad_out_color, _, *rest):
        viewmatrix, projmatrix, campos, bg = ctx.saved_tensors[12:16]
        camera_grads = any(ctx.needs_input_grad[9:12])
        out = _backward_body(ctx, grad_out_color, viewmatrix, projmatrix, campos, camera_grads, grad_alpha=_grad_alpha(ctx, rest), bg=bg,
                             grad_invdepth=_grad_invdepth(ctx, rest))
        (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh, grad_scales, grad_rotations) = out[:8]
        grad_view, grad_proj, grad_campos = out[8:11] if camera_grads else (None, None, None)
        grads = (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales, grad_rotations,
                 grad_cov3Ds_precomp, out[-1], grad_view, grad_proj, grad_campos)
        return tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad)) + (None, _split_grad_dc(ctx))


class SortMode(IntEnum):
    GLOBAL = 0
    PPX_FULL = 1
    PPX_KBUFFER = 2
    HIER = 3

    def __str__(self):
        return self.name


class GlobalSortOrder(IntEnum):
    Z_DEPTH = 0
    DISTANCE = 1
    PTD_CENTER = 2
    PTD_MAX = 3

    def __str__(self):
        return self.name


class _Settable:
    """set_value(key, value): set an own field, otherwise hand the key down (reference :199-246)."""
    _children = ()

    def set_value(self, key, value):
        if key in {f.name for f in fields(self)}:
            setattr(self, key, value)
        else:
            for child in self._children:
                getattr(self, child).set_value(key, value)


@dataclass
class SortQueueSizes(_Settable):
    tile_4x4: int = 64
    tile_2x2: int = 8
    per_pixel: int = 4


@dataclass
class SortSettings(_Settable):
    queue_sizes: SortQueueSizes = field(default_factory=SortQueueSizes)
    sort_mode: SortMode = SortMode.GLOBAL
    sort_order: GlobalSortOrder = GlobalSortOrder.Z_DEPTH
    _children = ("queue_sizes",)


@dataclass
class CullingSettings(_Settable):
    rect_bounding: bool = False
    tight_opacity_bounding: bool = False
    tile_based_culling: bool = False
    hierarchical_4x4_culling: bool = False


@dataclass
class ExtendedSettings(_Settable):
    sort_settings: SortSettings = field(default_factory=SortSettings)
    culling_settings: CullingSettings = field(default_factory=CullingSettings)
    load_balancing: bool = False
    proper_ewa_scaling: bool = False
    _children = ("culling_settings", "sort_settings")

    def to_dict(self):
        # same result as asdict(self, dict_factory=enum_dict_factory) (the reference's form, __init__.py:231-233), written out:
        # dataclasses.asdict deep-copies every leaf, 50 us per call -- a visible part of a small frame's host time
        ss, cs, q = self.sort_settings, self.culling_settings, self.sort_settings.queue_sizes
        as_int = lambda v: v.value if isinstance(v, IntEnum) else v
        return {"sort_settings": {"queue_sizes": {"tile_4x4": q.tile_4x4, "tile_2x2": q.tile_2x2, "per_pixel": q.per_pixel},
                                  "sort_mode": as_int(ss.sort_mode), "sort_order": as_int(ss.sort_order)},
                "culling_settings": {"rect_bounding": cs.rect_bounding, "tight_opacity_bounding": cs.tight_opacity_bounding,
                                     "tile_based_culling": cs.tile_based_culling, "hierarchical_4x4_culling": cs.hierarchical_4x4_culling},
                "load_balancing": self.load_balancing, "proper_ewa_scaling": self.proper_ewa_scaling,
                # (extension, not a dataclass field: `settings._backward_mode = "replay" | "resort" | "auto"` overrides the
                # process-wide backward-mode policy of _C.set_backward_mode for the calls made with this settings object)
                **({"_backward_mode": self._backward_mode} if getattr(self, "_backward_mode", None) else {}),
                # (extension, not a dataclass field: `settings._absgrad = True` asks every backward of the calls made with this settings
                # object for means2D.absgrad, the per-Gaussian sums of |each pixel's contribution to dL/dmean2D|)
                **({"_absgrad": True} if getattr(self, "_absgrad", False) else {}),
                # (the same for `settings._blend_stats = True`: means2D.blend_stats, per Gaussian the sum, max and count of its blend weights)
                **({"_blend_stats": True} if getattr(self, "_blend_stats", False) else {}),
                # (and for `settings._alpha = True`: the rasterizer returns (color, radii, alpha), alpha = 1 - final_T a differentiable output)
                **({"_alpha": True} if getattr(self, "_alpha", False) else {}),
                # (and for `settings._invdepth = True`: one more differentiable output behind it, invdepth = sum alpha T / z)
                **({"_invdepth": True} if getattr(self, "_invdepth", False) else {})}

    def to_json(self):
        return json.dumps(self.to_dict())

    @staticmethod
    def from_dict(dict):
        try:
            import dacite
            return dacite.from_dict(data_class=ExtendedSettings, data=dict, config=dacite.Config(cast=[IntEnum]))
        except ImportError:
            ss, cs = dict["sort_settings"], dict["culling_settings"]
            return ExtendedSettings(
                sort_settings=SortSettings(queue_sizes=SortQueueSizes(**ss["queue_sizes"]), sort_mode=SortMode(ss["sort_mode"]),
                                           sort_order=GlobalSortOrder(ss["sort_order"])),
                culling_settings=CullingSettings(**cs), load_balancing=dict["load_balancing"],
                proper_ewa_scaling=dict["proper_ewa_scaling"])

    @staticmethod
    def from_json(json_filename):
        return ExtendedSettings.from_dict(json.load(open(json_filename)))


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    inv_viewprojmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    settings: ExtendedSettings
    render_depth: bool
    debug: bool


def _check_split_sh(dc, shs, means3D):
    """GaussianRasterizer.forward's checks of a split SH input, before any device work: RuntimeError naming the argument."""
    if not isinstance(dc, torch.Tensor):
        raise RuntimeError(f"dc must be a tensor, got {type(dc).__name__}")
    P = means3D.shape[0]
    if not ((dc.dim() == 3 and dc.shape[1] == 1 and dc.shape[2] == 3) or (dc.dim() == 2 and dc.shape[1] == 3)):
        raise RuntimeError(f"dc must have dimensions (num_points, 1, 3) or (num_points, 3), got {tuple(dc.shape)}")
    if dc.shape[0] != P:
        raise RuntimeError(f"dc must have one row per Gaussian: {dc.shape[0]} rows for {P} points")
    if dc.dtype != torch.float32:
        raise RuntimeError(f"dc must be a float32 tensor, got {dc.dtype}")
    if dc.device != means3D.device:
        raise RuntimeError(f"dc must be on the device of means3D ({means3D.device}), got {dc.device}")
    if shs is not None and shs.numel() != 0:
        if shs.dim() != 3 or shs.shape[0] != P or shs.shape[2] != 3 or shs.dtype != torch.float32 or shs.device != means3D.device:
            raise RuntimeError(f"with dc, shs is the rest of the coefficients: a float32 (num_points, M - 1, 3) tensor on the device of "
                               f"means3D, got {tuple(shs.shape)} {shs.dtype} on {shs.device}")


class _RawRasterizationSettings(GaussianRasterizationSettings):
    """The settings tuple of one call with raw parameter inputs: the caller's fields, and the mask as the attribute raw_mask."""


def _with_raw_mask(rs, mask):
    out = _RawRasterizationSettings(*rs)
    out.raw_mask = int(mask)
    return out


RAW_PARAM_BITS = {"opacities": 1, "scales": 2, "rotations": 4}   # == the mask of include/stp_raster.h: stp_set_forward_raw_params


def _raw_mask(raw, opacities, scales, rotations) -> int:
    """GaussianRasterizer's raw= argument -> the library's mask, before any device work.  True: every one of the three inputs that
    is given; False / None: none; otherwise an iterable of their names.  RuntimeError naming what is wrong."""
    given = {"opacities": opacities is not None, "scales": scales is not None, "rotations": rotations is not None}
    if raw is None or raw is False:
        return 0
    if raw is True:
        return sum(bit for name, bit in RAW_PARAM_BITS.items() if given[name])
    if isinstance(raw, str):
        raw = (raw,)
    try:
        names = list(raw)
    except TypeError:
        raise RuntimeError(f"raw must be True, False or an iterable of names out of {sorted(RAW_PARAM_BITS)}, got {type(raw).__name__}") from None
    mask = 0
    for name in names:
        if name not in RAW_PARAM_BITS:
            raise RuntimeError(f"raw: unknown name {name!r}: expected names out of {sorted(RAW_PARAM_BITS)}")
        if not given[name]:
            raise RuntimeError(f"raw: {name!r} is named but no {name} are given (with cov3D_precomp there are no scales and rotations to activate)")
        mask |= RAW_PARAM_BITS[name]
    return mask


def activate_params(scaling=None, rotation=None, opacity=None):
    """The activated copies of a trainer's raw parameters (extension; include/stp_raster.h: stp_activate_params) -> (scales, rotations,
    opacities) = (exp(scaling), rotation / max(|rotation|, 1e-12), sigmoid(opacity)): fresh float32 tensors in the inputs' shapes that never
    require grad, None for an absent input.  These are the values GaussianRasterizer(..., raw=) renders with, to the bit -- for logging,
    export and tests; the render itself needs no such copy.  scaling (P, 3), rotation (P, 4), opacity (P,) or (P, 1), float32 on one GPU."""
    return _C.activate_params(*(None if t is None else t.detach() for t in (scaling, rotation, opacity)))


class GaussianRasterizer(nn.Module):
    """raw (extension, a keyword of the constructor; include/stp_raster.h: stp_set_forward_raw_params): the opacities / scales / rotations this
    rasterizer is called with are a trainer's _opacity (logit), _scaling (log) and _rotation (unnormalised quaternion) as they are stored.
    True = every one of the three that a call gives, False = none, otherwise an iterable of the names "opacities", "scales", "rotations"
    (the others are taken as activated).  sigmoid, exp and F.normalize run inside the kernels that read the arrays, the raw tensors are
    what the backward keeps, and .grad arrives on the raw leaves.  Results equal those of the plain call on activate_params(...) bit for
    bit in the forward, and autograd's chain rule in the backward.  forward()'s own signature is the reference's plus dc."""

    def __init__(self, raster_settings, raw=False):
        super().__init__()
        self.raster_settings = raster_settings
        self.raw = raw

    def markVisible(self, positions):
        """Boolean mask of the points that pass the camera's near-plane test."""
        with torch.no_grad():
            rs = self.raster_settings
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, dc=None):
        """dc (extension; include/stp_raster.h: stp_set_forward_split_sh): a trainer's _features_dc, (P, 1, 3) or (P, 3), with shs = its
        _features_rest, (P, M-1, 3) (None or (P, 0, 3) for a degree-0 model) -- no torch.cat going in, and dc.grad / shs.grad come back as
        two fresh contiguous tensors in the inputs' shapes.  Results equal those of shs = torch.cat((dc, rest), dim=1).
        A rasterizer made with raw= (see the class) reads opacities / scales / rotations as a trainer's stored parameters."""
        rs = self.raster_settings
        have_sh = shs is not None or dc is not None
        if (not have_sh and colors_precomp is None) or (have_sh and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if dc is not None:
            _check_split_sh(dc, shs, means3D)
        mask = _raw_mask(self.raw, opacities, scales, rotations)
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')
        empty = lambda t: torch.Tensor([]) if t is None else t  # absent optional input == empty CPU tensor
        return rasterize_gaussians(means3D, means2D, empty(shs), empty(colors_precomp), opacities, empty(scales),
                                   empty(rotations), empty(cov3D_precomp), rs, dc, *((mask,) if mask else ()))


class SparseGaussianAdam(torch.optim.Adam):
    """Adam whose step updates only the Gaussians visible in the frame, all tensors in one fused kernel launch (extension; the class of the
    same name in the accelerated 3DGS rasterizer, a trainer's `--optimizer_type sparse_adam`; include/stp_raster.h: stp_sparse_adam).

        opt = SparseGaussianAdam([{"params": [xyz], "lr": ..., "name": "xyz"}, ...], lr=0.0, eps=1e-15)
        ...
        opt.step(radii > 0, N)        # or opt.step(radii, N): the forward's int32 radii are read as they are (> 0 = visible)

    For every group's tensor with a gradient, every row i < N with visibility[i] and each of its numel / N elements, in float32:
        m <- b1 m + (1 - b1) g      v <- b2 v + (1 - b2) g g      p <- p - lr m / (sqrt(v) + eps)
    There is NO bias correction (as upstream), no weight decay and no amsgrad; rows that are not visible keep param and state bit for bit and
    their gradient is not read.  Every group holds exactly one tensor; lr and eps are the group's, read at every step (a trainer's schedule
    writes group["lr"]), betas must agree across the groups.  The state is torch.optim.Adam's -- state[p]["step"], ["exp_avg"], ["exp_avg_sq"]
    -- so that densification code that concatenates, prunes or replaces those tensors and swaps group["params"][0] keeps working, and
    state_dict() / load_state_dict() are Adam's.  state["step"] counts the steps that found a gradient on the tensor.
    `last_launches` holds the kernel launches of the latest step (one per eight tensors)."""

    _REFUSED = ("weight_decay", "amsgrad", "maximize", "capturable", "fused", "foreach")

    def __init__(self, params, lr, eps, betas=(0.9, 0.999), **options):
        for name, value in options.items():
            if name not in self._REFUSED:
                raise TypeError(f"SparseGaussianAdam got an unexpected option {name!r}")
            self._refuse(name, value)
        super().__init__(params=params, lr=lr, eps=eps, betas=betas)
        for group in self.param_groups:   # (options can also ride in a group's dict)
            for name in self._REFUSED:
                self._refuse(name, group.get(name))
            self._one_tensor(group)
        self.last_launches = 0

    @staticmethod
    def _refuse(name, value):
        if value is not None and value is not False and value != 0:
            raise ValueError(f"SparseGaussianAdam does not support {name} (got {name}={value!r}): the fused step is plain Adam without bias "
                             "correction on the visible rows")

    @staticmethod
    def _one_tensor(group):
        if len(group["params"]) != 1:
            raise AssertionError("more than one tensor in group")

    @torch.no_grad()
    def step(self, visibility, N):
        params, grads, exp_avgs, exp_avg_sqs, lrs, epss = [], [], [], [], [], []
        betas = None
        for group in self.param_groups:
            self._one_tensor(group)
            param = group["params"][0]
            if param.grad is None:
                continue
            if betas is None:
                betas = tuple(group["betas"])
            elif tuple(group["betas"]) != betas:
                raise ValueError(f"SparseGaussianAdam steps all groups in one kernel launch: betas must agree, got {betas} and {tuple(group['betas'])}")
            state = self.state[param]
            if len(state) == 0:   # created as torch.optim.Adam creates it
                state["step"] = torch.tensor(0.0, dtype=torch.float32)
                state["exp_avg"] = torch.zeros_like(param, memory_format=torch.preserve_format)
                state["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.preserve_format)
            state["step"] += 1
            params.append(param)
            grads.append(param.grad)
            exp_avgs.append(state["exp_avg"])
            exp_avg_sqs.append(state["exp_avg_sq"])
            lrs.append(float(group["lr"]))
            epss.append(float(group["eps"]))
        self.last_launches = _C.sparse_adam(params, grads, exp_avgs, exp_avg_sqs, visibility, lrs, epss, betas[0], betas[1], N) if params else 0


class GaussianAdam(torch.optim.Adam):
    """torch.optim.Adam -- dense, bias-corrected, as the 3DGS trainer (optimizer_type "default") and every 3DGS-MCMC trainer construct it --
    whose step is one fused kernel launch per eight tensors, with the two 3DGS-MCMC regularisers folded in (extension;
    include/stp_raster.h: stp_dense_adam).  A trainer changes the class name only:

        opt = GaussianAdam([{"params": [xyz], "lr": ..., "name": "xyz"}, ...], lr=0.0, eps=1e-15)
        opt.set_regularizer("opacity", "sigmoid", opacity_reg)     # instead of  loss += opacity_reg * sigmoid(_opacity).abs().mean()
        opt.set_regularizer("scaling", "exp", scale_reg)           # instead of  loss += scale_reg * exp(_scaling).abs().mean()
        ...
        opt.step()

    For every tensor with a gradient, all groups in one call, every element in float32 (t = the tensor's step count after this step):
        g' = g + r      m <- b1 m + (1 - b1) g'      v <- b2 v + (1 - b2) g' g'
        p <- p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    with r = 0, or for a group whose "reg" is ("sigmoid", w): r = (w / numel) s (1 - s), s = sigmoid(p) -- the gradient of w * sigmoid(p).mean()
    -- or ("exp", w): r = (w / numel) exp(p), the gradient of w * exp(p).mean().  .grad is only read.  The regulariser's VALUE is not computed:
    a trainer that logs it computes it itself.  Coefficients are formed in float64 from the Python values, as torch forms them, and rounded to
    float32 once.  A group may hold any number of tensors; lr, eps, betas and "reg" are the group's, read at every step.
    The state is non-capturable torch.optim.Adam's -- state[p]["step"] a CPU float32 scalar tensor, ["exp_avg"] and ["exp_avg_sq"] zeros_like(p),
    created by the first step that finds a gradient -- so state_dict() / load_state_dict() (to and from a torch.optim.Adam), densify_and_prune,
    mcmc_relocate_, mcmc_add_new and a trainer's own state surgery keep working.  No weight decay, amsgrad, maximize, capturable, differentiable,
    fused or foreach option and no tensor lr (ValueError at construction).  A step is refused as a whole (RuntimeError naming the tensor, nothing
    updated, no step counted) for a CPU tensor, a dtype other than float32, a sparse gradient, a non-contiguous param, grad or state, and tensors on
    different devices.  `last_launches` holds the kernel launches of the latest step."""

    _REFUSED = ("weight_decay", "amsgrad", "maximize", "capturable", "differentiable", "fused", "foreach")
    _REG_KINDS = ("sigmoid", "exp")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, **options):
        for name, value in options.items():
            if name not in self._REFUSED:
                raise TypeError(f"GaussianAdam got an unexpected option {name!r}")
            self._refuse(name, value)
        self._refuse_tensor_lr(lr)
        super().__init__(params=params, lr=lr, betas=betas, eps=eps)
        for group in self.param_groups:   # (options can also ride in a group's dict)
            for name in self._REFUSED:
                self._refuse(name, group.get(name))
            self._refuse_tensor_lr(group["lr"])
            self._reg_of(group)
        self.last_launches = 0

    @staticmethod
    def _refuse(name, value):
        if value is not None and value is not False and value != 0:
            raise ValueError(f"GaussianAdam does not support {name} (got {name}={value!r}): the fused step is plain bias-corrected Adam")

    @staticmethod
    def _refuse_tensor_lr(lr):
        if isinstance(lr, torch.Tensor):
            raise ValueError("GaussianAdam does not support a tensor lr: the learning rate travels in the kernel arguments as a host number")

    @classmethod
    def _reg_of(cls, group):
        """-> (reg_kind of the C ABI, weight) of a group's "reg": None or (kind, weight)"""
        reg = group.get("reg")
        if reg is None:
            return 0, 0.0
        if not (isinstance(reg, (tuple, list)) and len(reg) == 2 and reg[0] in cls._REG_KINDS):
            raise ValueError(f"GaussianAdam: group {group.get('name', '?')!r}: reg must be None or (kind, weight) with kind in {cls._REG_KINDS}, got {reg!r}")
        return _C.DENSE_ADAM_REG_KINDS[reg[0]], float(reg[1])

    def set_regularizer(self, name, kind, weight=0.0):
        """The group whose "name" is `name` gets "reg" = (kind, weight), kind in {"sigmoid", "exp"}, or None for kind None: from the next step on
        the gradient of weight * mean(sigmoid(p)) or weight * mean(exp(p)) (the mean over each tensor's numel) is added to the tensor's inside the kernel."""
        found = [g for g in self.param_groups if g.get("name") == name]
        if len(found) != 1:
            raise ValueError(f"GaussianAdam.set_regularizer: {len(found)} groups are named {name!r}")
        old = found[0].get("reg")
        found[0]["reg"] = None if kind is None else (kind, float(weight))
        try:
            self._reg_of(found[0])
        except ValueError:
            found[0]["reg"] = old
            raise

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # validate first ...
        work, placed, device = [], [], None
        for gi, group in enumerate(self.param_groups):
            for name in self._REFUSED:
                self._refuse(name, group.get(name))
            self._refuse_tensor_lr(group["lr"])
            kind, weight = self._reg_of(group)
            beta1, beta2 = group["betas"]
            for ti, param in enumerate(group["params"]):
                grad = param.grad
                if grad is None or param.numel() == 0:   # (nothing to step: no state is created, none is touched)
                    continue
                who = f"GaussianAdam.step: group {group.get('name', gi)!r} tensor {ti}"
                state = self.state[param] if param in self.state else {}   # (no entry is created before the step is accepted)
                if grad.is_sparse or grad.layout != torch.strided:
                    raise RuntimeError(f"{who}: sparse gradients are not supported")
                named = [("param", param), ("grad", grad)] + [(k, state[k]) for k in ("exp_avg", "exp_avg_sq") if len(state)]
                for label, t in named:   # (what is wrong with the tensors themselves first, where they live last)
                    if t.dtype != torch.float32:
                        raise RuntimeError(f"{who}: {label}: expected float32, got {t.dtype}")
                    if not t.is_contiguous():
                        raise RuntimeError(f"{who}: {label} must be contiguous (it is updated in place)")
                    if t.shape != param.shape:
                        raise RuntimeError(f"{who}: {label} has shape {tuple(t.shape)}, param has {tuple(param.shape)}")
                work.append((param, group, kind, weight, float(beta1), float(beta2)))
                placed.append((who, named))
        for who, named in placed:
            for label, t in named:
                if not t.is_cuda:
                    raise RuntimeError(f"{who}: {label} is on {t.device}: there is no CPU path")
                device = device or t.device
                if t.device != device:
                    raise RuntimeError(f"{who}: {label} is on {t.device}, earlier tensors on {device}: one step serves one device")
        # ... count after
        params, grads, exp_avgs, exp_avg_sqs, coefs, kinds = [], [], [], [], [], []
        with torch.no_grad():
            for param, group, kind, weight, beta1, beta2 in work:
                state = self.state[param]
                if len(state) == 0:   # created as non-capturable torch.optim.Adam creates it
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(param, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(param, memory_format=torch.preserve_format)
                state["step"] += 1
                params.append(param)
                grads.append(param.grad)
                exp_avgs.append(state["exp_avg"])
                exp_avg_sqs.append(state["exp_avg_sq"])
                coefs.append(_C.dense_adam_coefficients(group["lr"], beta1, beta2, group["eps"], float(state["step"]), weight, param.numel()))
                kinds.append(kind)
            self.last_launches = _C.dense_adam(params, grads, exp_avgs, exp_avg_sqs, coefs, kinds) if params else 0
        return loss


class _PhotometricTerms(torch.autograd.Function):
    """(image, target) -> the (2,) tensor [mean |image - target|, mean SSIM(image, target)] of the fused photometric kernels.  The three
    derivative maps are stored only when a gradient can be asked for (grad mode on and image.requires_grad); target gets no gradient."""

    @staticmethod
    def forward(ctx, image, target, want_maps):
        out2, maps = _C.photometric_forward(image, target, want_maps)
        ctx.has_maps = maps is not None
        if ctx.has_maps:
            ctx.save_for_backward(image, target, maps)
        return out2

    @staticmethod
    def backward(ctx, grad_out2):
        if not ctx.has_maps:
            raise RuntimeError("photometric_terms: this forward stored no derivative maps (fused_ssim(train=False)): it cannot be differentiated")
        image, target, maps = ctx.saved_tensors
        return _C.photometric_backward(image, target, maps, grad_out2), None, None


def _photometric(image, target, store_maps=True) -> torch.Tensor:
    want_maps = bool(store_maps) and torch.is_grad_enabled() and isinstance(image, torch.Tensor) and image.requires_grad
    return _PhotometricTerms.apply(image, target, want_maps)


def photometric_terms(image: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Both terms of a 3DGS trainer's loss from one fused kernel pair (extension; include/stp_raster.h: stp_photometric_forward): the (2,)
    float32 tensor  [mean |image - target|, mean SSIM(image, target)]  on the device -- upstream's l1_loss(image, target) and
    ssim(image, target) with window_size = 11 and size_average = True (Gaussian window of sigma 1.5, zero padding of 5, C1 = 0.01^2,
    C2 = 0.03^2).  image, target: float32 (C, H, W) or (B, C, H, W) of equal shape on one GPU, every (H, W) plane on its own, H and W of
    any size; non-contiguous tensors are made contiguous.  Differentiable in image; a target that requires grad is accepted and gets NO
    gradient (None), as upstream's fused kernel gives none.  Deterministic: equal inputs give equal bits, forward and backward.  Refused
    with a RuntimeError: CPU tensors, other dtypes than float32, shapes that differ, fewer than 3 or more than 4 dimensions, tensors on
    different devices.  No host synchronisation anywhere: the backward reads the upstream gradient from device memory."""
    return _photometric(image, target)


def fused_ssim(img1: torch.Tensor, img2: torch.Tensor, padding: str = "same", train: bool = True) -> torch.Tensor:
    """The mean SSIM of img1 against img2 under the name and argument order of the `fused-ssim` package: a scalar tensor, differentiable
    in img1 (img2 gets no gradient).  padding must be "same" (zero padding of 5; "valid" is not built); train=False stores no derivative
    maps (evaluation: the result is bit-equal to train=True and cannot be differentiated)."""
    if padding != "same":
        raise ValueError(f"fused_ssim: padding={padding!r} is not supported, only \"same\" (zero padding of 5; \"valid\" is not built)")
    return _photometric(img1, img2, store_maps=train)[1]


def photometric_loss(image: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2) -> torch.Tensor:
    """The 3DGS trainers' loss  (1 - lambda_dssim) * L1(image, target) + lambda_dssim * (1 - SSIM(image, target))  as a scalar tensor,
    composed on the two device scalars of photometric_terms (which see for shapes, refusals and the gradient rules)."""
    terms = _photometric(image, target)
    return (1.0 - lambda_dssim) * terms[0] + lambda_dssim * (1.0 - terms[1])


class _TrainingTerms(torch.autograd.Function):
    """(image, target, exposure, alpha_mask, invdepth, mono_invdepth, depth_mask, clamp, want_maps) -> the (3,) tensor of training_terms.
    Gradients for image, exposure and invdepth; none for target, the masks and mono_invdepth."""

    @staticmethod
    def forward(ctx, image, target, exposure, alpha_mask, invdepth, mono_invdepth, depth_mask, clamp, want_maps):
        out3, maps = _C.training_loss_forward(image, target, exposure, clamp, alpha_mask, invdepth, mono_invdepth, depth_mask, want_maps)
        ctx.has_maps, ctx.clamp = maps is not None, clamp
        ctx.given = [t is not None for t in (exposure, alpha_mask, invdepth, mono_invdepth, depth_mask)]
        if ctx.has_maps:
            ctx.save_for_backward(image, target, maps, *[t for t in (exposure, alpha_mask, invdepth, mono_invdepth, depth_mask) if t is not None])
        return out3

    @staticmethod
    def backward(ctx, grad_out3):
        if not ctx.has_maps:
            raise RuntimeError("training_terms: this forward stored no derivative maps: it cannot be differentiated")
        image, target, maps, *rest = ctx.saved_tensors
        rest = iter(rest)
        exposure, alpha_mask, invdepth, mono_invdepth, depth_mask = [next(rest) if g else None for g in ctx.given]
        want_exposure = exposure is not None and ctx.needs_input_grad[2]
        want_invdepth = invdepth is not None and ctx.needs_input_grad[4]
        g_image, g_exposure, g_invdepth = _C.training_loss_backward(image, target, exposure, ctx.clamp, alpha_mask, invdepth, mono_invdepth, depth_mask, maps, grad_out3,
                                                                    want_exposure, want_invdepth)
        return g_image, None, g_exposure, None, g_invdepth, None, None, None, None


def training_terms(image: torch.Tensor, target: torch.Tensor, *, exposure=None, clamp: bool = False, alpha_mask=None, invdepth=None, mono_invdepth=None,
                   depth_mask=None) -> torch.Tensor:
    """The three terms of the loss a 3DGS trainer's step runs, from the fused kernels of photometric_terms (extension; include/stp_raster.h:
    stp_training_loss_forward): the (3,) float32 tensor
        [mean |x'' - target|, mean SSIM(x'', target), mean |(invdepth - mono_invdepth) * depth_mask|]        (the last exactly 0.0 without invdepth)
    with  v_j = sum_i image_i * exposure[i][j] + exposure[j][3]  (upstream's matmul(image.permute(1, 2, 0), exposure[:3, :3]) + exposure[:3, 3];
    one float32 fma chain), v clamped to [0, 1] when clamp (the gradient passes where 0 <= v <= 1), x'' = v * alpha_mask; the window's zero
    padding applies to x''.  image, target: as photometric_terms; exposure: (3, 4) or (B, 3, 4), needs C == 3; alpha_mask: (H, W), (1, H, W)
    or (B, 1, H, W); invdepth, mono_invdepth, depth_mask: (1, H, W) or (B, 1, H, W); all float32 on the image's GPU, each optional, invdepth
    and mono_invdepth together.  Differentiable in image, exposure and invdepth; target, the masks and mono_invdepth get NO gradient (None).
    Deterministic, and no host synchronisation anywhere.  With no extra given this is photometric_terms, bit for bit, and a zero."""
    tensors = (image, exposure, invdepth)
    want_maps = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)
    return _TrainingTerms.apply(image, target, exposure, alpha_mask, invdepth, mono_invdepth, depth_mask, bool(clamp), want_maps)


def training_loss(image: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, depth_weight: float = 0.0, **extras) -> torch.Tensor:
    """(1 - lambda_dssim) * t[0] + lambda_dssim * (1 - t[1]) + depth_weight * t[2]  of t = training_terms(image, target, **extras), a scalar
    tensor composed on the three device scalars."""
    t = training_terms(image, target, **extras)
    return (1.0 - lambda_dssim) * t[0] + lambda_dssim * (1.0 - t[1]) + depth_weight * t[2]


def compute_relocation(opacity_old: torch.Tensor, scale_old: torch.Tensor, N: torch.Tensor):
    """3DGS-MCMC's relocation rule (extension; include/stp_raster.h: stp_mcmc_relocation; the function a 3DGS-MCMC code base imports from its
    rasterizer package): a Gaussian of opacity o and scales s that is replaced by N copies of itself gives each copy
        o_new = 1 - (1 - o)^(1/N),    s_new = (o / denom) s,    denom = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k o_new^(k+1) / sqrt(k+1)
    -> (opacity_new, scale_new), float32.  opacity_old: (n,) or (n, 1) float32, and opacity_new keeps its shape; scale_old: (n, 3) float32;
    N: (n,) or (n, 1) int32 or int64, clamped to [1, 50] -- WITHOUT being modified (upstream clamps its N in place).  Non-contiguous inputs
    are made contiguous.  The sum is evaluated in float64; equal inputs give equal bits.  No autograd (the inputs are detached).
    Refused with a RuntimeError naming the argument: CPU tensors ("no CPU path"), other dtypes, shapes or row counts that do not match,
    tensors on different devices."""
    return _C.compute_relocation(opacity_old.detach(), scale_old.detach(), N, None, _C.RELOCATION_N_MAX)


def mcmc_add_noise_(xyz: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor, noise: torch.Tensor,
                    noise_scale: float, *, raw: bool = False, k: float = 100.0, x0: float = 0.995) -> torch.Tensor:
    """3DGS-MCMC's per-iteration position noise in ONE kernel, in place (extension; include/stp_raster.h: stp_mcmc_add_noise):
        xyz[i] += R diag(s^2) R^T (noise[i] * g * noise_scale),    g = 1 / (1 + exp(-k ((1 - o) - x0)))
    with R the rotation of rotations[i] / |rotations[i]| (w, x, y, z), s = scales[i], o = opacities[i]; raw=True reads the model's raw
    _scaling and _opacity and applies exp and sigmoid in the kernel.  noise is the caller's torch.randn_like(xyz) (random numbers stay
    torch's), noise_scale the trainer's noise_lr * xyz_lr; noise_scale, k and x0 are rounded to float32 once.  xyz (P, 3) contiguous,
    scales (P, 3), rotations (P, 4), opacities (P,) or (P, 1), noise (P, 3): float32 on one GPU.  Works on xyz's storage like an optimizer
    step: nothing is recorded in autograd, a leaf that requires grad is fine, and the SAME tensor is returned.  Float32 IEEE arithmetic: a
    gate whose exp overflows is 0, a zero quaternion gives NaN in its own row only.  Equal inputs give equal bits.  Refused with a
    RuntimeError naming the argument: CPU tensors ("no CPU path"), other dtypes than float32, shapes or row counts that do not match, tensors
    on different devices, an xyz that is not contiguous."""
    _C.mcmc_add_noise(xyz.detach(), scales.detach(), rotations.detach(), opacities.detach(), noise.detach(), noise_scale, k, x0, raw)
    return xyz


def compute_3d_filter(xyz: torch.Tensor, world_view_transforms: torch.Tensor, intrinsics: torch.Tensor) -> torch.Tensor:
    """Mip-Splatting's 3D smoothing filter over ALL training cameras in one pass (extension; include/stp_raster.h: stp_mip_filter_3d; that
    trainer's GaussianModel.compute_3D_filter) -> filter_3d, (P, 1) float32, never requiring grad, on the current
    stream without host synchronisation.  xyz: (P, 3); world_view_transforms: (C, 4, 4), every camera's world_view_transform (row-vector
    layout, p_cam = [p, 1] @ M; only M[:3, :3] and M[3, :3] are read); intrinsics: (C, 4) = (focal_x, focal_y, image_width, image_height);
    float32 on one GPU, made contiguous where they are not.  With (x, y, z) = p_cam, per Gaussian and camera:
        valid = z > 0.2  and  -0.15 W <= x / max(z, 0.001) * focal_x + W / 2 <= 1.15 W  and the same in y with focal_y and H
        distance = min over the valid cameras of z;   a row no camera sees takes the largest distance of the rows that are seen
        filter_3d = distance / max_c(focal_x) * sqrt(0.2)                                       (the maximum over all cameras)
    Where NO row is seen every row keeps the distance 100000 (upstream raises there, which needs a read-back).  A NaN coordinate is never valid.
    Equal inputs give equal bits.  P == 0 gives an empty (0, 1) tensor; C == 0 is refused.  Refused with a RuntimeError naming the argument: CPU
    tensors ("no CPU path"), other dtypes than float32, shapes or row counts that do not match, tensors on different devices."""
    return _C.compute_3d_filter(xyz.detach(), world_view_transforms.detach(), intrinsics.detach())


class _FilteredActivations(torch.autograd.Function):
    """(scaling, opacity, filter_3d) -> (scales, opacities): one kernel forward, one backward that recomputes from the three inputs."""

    @staticmethod
    def forward(ctx, scaling, opacity, filter_3d):
        ctx.save_for_backward(scaling, opacity, filter_3d)
        ctx.set_materialize_grads(False)   # (an output the loss did not use arrives as None: the kernel then skips its stream)
        return _C.mip_activations(scaling, opacity, filter_3d)

    @staticmethod
    def backward(ctx, grad_scales, grad_opacities):
        if grad_scales is None and grad_opacities is None:
            return None, None, None
        scaling, opacity, filter_3d = ctx.saved_tensors
        g_scaling, g_opacity = _C.mip_activations_backward(scaling, opacity, filter_3d, grad_scales, grad_opacities)
        return g_scaling, g_opacity, None


def filtered_activations(scaling: torch.Tensor, opacity: torch.Tensor, filter_3d: torch.Tensor):
    """Mip-Splatting's get_scaling_with_3D_filter and get_opacity_with_3D_filter in one kernel, differentiable (extension; include/stp_raster.h:
    stp_mip_activations_forward / _backward) -> (scales (P, 3), opacities of opacity's shape), the `scales=` and
    `opacities=` of the ordinary (non-raw) GaussianRasterizer call.  scaling: (P, 3) stored log-scales; opacity: (P,) or (P, 1) stored logits;
    filter_3d: (P,) or (P, 1), compute_3d_filter's buffer -- it gets NO gradient (None).  With e_j = exp(scaling_j), f = filter_3d:
        scales_j = sqrt(e_j^2 + f^2)      r_j = e_j^2 / (e_j^2 + f^2)      opacities = sigmoid(opacity) * sqrt(r_0 r_1 r_2)
    which is upstream's sqrt(prod e^2 / prod (e^2 + f^2)) without the determinants that leave float32's normal range for small scales.  The
    backward saves nothing but the three inputs; either output may go unused.  Deterministic: equal inputs give equal bits, forward and
    backward.  Refused with a RuntimeError naming the argument: CPU tensors ("no CPU path"), other dtypes than float32, shapes or row counts
    that do not match, tensors on different devices."""
    return _FilteredActivations.apply(scaling, opacity, filter_3d)


def knn_mean_dist2(points: torch.Tensor) -> torch.Tensor:
    """simple_knn's distCUDA2 (extension; include/stp_raster.h: stp_knn_mean_dist2) -- what `GaussianModel.create_from_pcd` initialises the
    scales with: for points (P, 3) float32 on a GPU, out[i] is the mean of the three smallest squared distances from point i to the points
    j != i (by index: an exact duplicate is a neighbour at distance 0), float32, (P,), in input order, on the current stream and without
    host synchronisation.  The search is exact (Morton-sorted boxes behind float32-conservative box tests) and the result is fixed to the
    bit: d2 = (dx * dx + dy * dy) + dz * dz and ((b0 + b1) + b2) / 3 in float32 with every operation rounded once -- the bits of a brute
    force in that order, whatever the cloud.  Equal inputs give equal bits.  A non-contiguous input is made contiguous; P == 0 gives an
    empty (0,) tensor; the result never requires grad.  Refused with a RuntimeError naming the argument: another dtype ("points: expected
    float32"), another shape ("points must be (P, 3)"), P in 1..3 ("needs at least 4 points"; upstream returns garbage there), a CPU
    tensor ("no CPU path").  `simple_knn._C.distCUDA2` is this function."""
    return _C.knn_mean_dist2(points.detach())


dist_cuda2 = distCUDA2 = knn_mean_dist2


def _f32(x) -> float:
    return float(torch.tensor(float(x), dtype=torch.float32))


def densification_stats_(xyz_gradient_accum: torch.Tensor, denom: torch.Tensor, max_radii2D: Optional[torch.Tensor], grad2d: torch.Tensor,
                         radii: torch.Tensor) -> None:
    """A trainer's per-step densification statistics in ONE kernel, in place, without host synchronisation (extension; include/stp_raster.h:
    stp_densify_stats) -- what `stat[vis] += grad2d[vis, :2].norm(dim=-1, keepdim=True); denom[vis] += 1; max_radii2D[vis] =
    max(max_radii2D[vis], radii[vis])` does with a `nonzero` and a synchronisation per indexed tensor.  For every i with radii[i] > 0:
        xyz_gradient_accum[i] += sqrt(gx^2 + gy^2)      denom[i] += 1      max_radii2D[i] = max(max_radii2D[i], radii[i])
    grad2d: viewspace_points.grad or .absgrad, (P, 3) or (P, 2) float32 (only the first two columns are read).  The accumulators: (P,) or
    (P, 1) float32, contiguous.  radii: the forward's int32 radii; a bool / uint8 mask is accepted where max_radii2D is None.  Rows that are
    not visible keep their bits and their gradient is never read (a NaN there changes nothing).  Equal inputs give equal bits.  Refused with a
    RuntimeError naming the argument: CPU tensors ("no CPU path"), other dtypes, shapes or row counts that do not match."""
    _C.densify_stats(xyz_gradient_accum.detach(), denom.detach(), None if max_radii2D is None else max_radii2D.detach(), grad2d.detach(), radii)


def densify_plan(xyz_gradient_accum: torch.Tensor, denom: torch.Tensor, scaling: torch.Tensor, opacity: torch.Tensor,
                 max_radii2D: Optional[torch.Tensor] = None, *, grad_threshold: float, percent_dense: float = 0.01, extent: float,
                 min_opacity: float = 0.005, max_screen_size: Optional[float] = None, raw: bool = True) -> torch.Tensor:
    """The decision of 3DGS adaptive density control as one byte per Gaussian, in ONE kernel without host synchronisation (extension;
    include/stp_raster.h: stp_densify_plan): uint8 (P,), bit 0 = the original stays, bit 1 = one copy is appended, bit 2 = two children are
    appended.  With s the scales (exp(scaling) where raw), o the opacity (its sigmoid where raw) and g = accum / denom (0 where denom == 0):
        hot = g >= grad_threshold       clone = hot and max(s) <= percent_dense * extent       split = hot and max(s) > percent_dense * extent
        pruned = o < min_opacity  or, where max_screen_size is not None,  max(s) > 0.1 * extent  or  max_radii2D > max_screen_size
    where a split's children are tested with max(s) / 1.6.  With max_radii2D=None the rows densify_tensors / densify_and_prune leave and
    their order are exactly those of upstream's densify_and_prune (which zeroes max_radii2D before its prune: its screen-size test never
    fires); with max_radii2D given the test applies to the originals.  The bits are independent, so a plan can also be written with torch:
    keep.to(torch.uint8) prunes, 1 | 2 grows.  The thresholds are rounded to float32 once."""
    big = max_screen_size is not None
    rule = (_f32(grad_threshold), _f32(float(percent_dense) * float(extent)), _f32(min_opacity), _f32(max_screen_size if big else 0.0),
            _f32(0.1 * float(extent)), _f32(0.8 * 2))
    return _C.densify_plan(xyz_gradient_accum.detach(), denom.detach(), scaling.detach(), opacity.detach(),
                           None if max_radii2D is None else max_radii2D.detach(), rule, raw, big)


def _row_lists(tensors, roles, role_ids, exp_avgs, exp_avg_sqs):
    """The lists the native row-tensor calls take: detached tensors, roles as numbers (names through role_ids; None: all plain), one moment or None
    per tensor (None: no moments at all)."""
    tensors = [t.detach() for t in tensors]
    n = len(tensors)
    roles = [0] * n if roles is None else [role_ids[r] if isinstance(r, str) else int(r) for r in roles]
    exp_avgs = [None] * n if exp_avgs is None else [None if m is None else m.detach() for m in exp_avgs]
    exp_avg_sqs = [None] * n if exp_avg_sqs is None else [None if v is None else v.detach() for v in exp_avg_sqs]
    return tensors, roles, exp_avgs, exp_avg_sqs


def _named_groups(who, optimizer, role_of):
    """-> (groups, params, roles, exp_avgs, exp_avg_sqs) of an optimizer whose groups hold one tensor each and carry "name"; role_of: {group name: role},
    every other group is plain; the moments are None where the state has none."""
    groups = list(optimizer.param_groups)
    params, roles, ms, vs = [], [], [], []
    for group in groups:
        if len(group["params"]) != 1 or "name" not in group:
            raise ValueError(f"{who}: every group must hold one tensor and carry a \"name\"")
        p = group["params"][0]
        state = optimizer.state.get(p, {})
        params.append(p)
        roles.append(role_of.get(group["name"], "plain"))
        ms.append(state.get("exp_avg"))
        vs.append(state.get("exp_avg_sq"))
    return groups, params, roles, ms, vs


def densify_tensors(plan: torch.Tensor, tensors, roles=None, exp_avgs=None, exp_avg_sqs=None, noise: Optional[torch.Tensor] = None, *,
                    split_shrink: float = 1.6, raw: bool = True):
    """Clone, split and prune a model by a plan (densify_plan's, or one written with torch) in one scan and one apply (extension;
    include/stp_raster.h: stp_densify_scan, stp_densify_apply) -> (new_tensors, new_exp_avgs, new_exp_avg_sqs, (nK, nC, nS)).
    tensors: float32 (P, ...) of any trailing shape; roles: per tensor "plain" / "xyz" / "scaling" / "rotation" (or 0..3; None: all plain);
    exp_avgs / exp_avg_sqs: the Adam moments per tensor, None where there are none (None: no moments at all).  The output has
    nK + nC + 2 nS rows: the kept rows in index order, the copies, the first children of the split rows, their second children -- the order
    upstream's cat, cat, mask sequence leaves.  Kept rows copy parameter and moments bit for bit; copies and children get zero moments;
    child j of the r-th split Gaussian i has xyz + R(q / |q|) (s * noise[j * nS + r]) and scaling log(s / split_shrink) (s / split_shrink
    where raw is False), s = exp(scaling) where raw.  noise: (2 nS, 3) standard normal (random numbers stay torch's); None draws
    torch.randn.  A split needs exactly one tensor of each of the roles xyz (P, 3), scaling (P, 3), rotation (P, 4).
    ONE host synchronisation, in the scan: the counts have to be known to allocate.  Inputs are not modified."""
    tensors, roles, exp_avgs, exp_avg_sqs = _row_lists(tensors, roles, _C.DENSIFY_ROLES, exp_avgs, exp_avg_sqs)
    offsets, counts = _C.densify_scan(plan)
    if noise is None and counts[2] > 0:
        noise = torch.randn(2 * counts[2], 3, device=plan.device, dtype=torch.float32)
    new_t, new_m, new_v = _C.densify_apply(plan, offsets, counts, tensors, roles, exp_avgs, exp_avg_sqs, noise, split_shrink, raw)
    return new_t, new_m, new_v, counts


def _replace_group_tensors(optimizer, groups, params, new_t, new_m, new_v):
    """Every group gets a new nn.Parameter of its new tensor, optimizer.state moves onto it with the new moments (a group whose state is still empty
    stays empty; other entries, "step", are kept) -> {name: new Parameter}, upstream's optimizable_tensors."""
    out = {}
    for group, old, t, m, v in zip(groups, params, new_t, new_m, new_v):
        new = torch.nn.Parameter(t.requires_grad_(old.requires_grad))
        state = optimizer.state.pop(old, None)
        if state is not None and len(state) > 0:
            if m is not None:
                state["exp_avg"], state["exp_avg_sq"] = m, v
            optimizer.state[new] = state
        group["params"][0] = new
        out[group["name"]] = new
    return out


def densify_and_prune(optimizer, plan: torch.Tensor, *, noise: Optional[torch.Tensor] = None, split_shrink: float = 1.6, raw: bool = True,
                      names=("xyz", "scaling", "rotation")):
    """upstream's densify_and_prune on an optimizer, by a plan (extension): every group of `optimizer` (a torch.optim.Adam or a
    SparseGaussianAdam whose groups hold one tensor each and carry "name") goes through ONE densify_tensors call; the groups named
    names = (xyz, scaling, rotation) play those roles.  Each group gets a new nn.Parameter in group["params"][0], optimizer.state moves onto
    it with the new exp_avg and exp_avg_sq (a group whose state is still empty stays empty; other entries, "step", are kept), and
    {name: new Parameter} -- upstream's optimizable_tensors -- is returned for the model to take.  One host synchronisation."""
    groups, params, roles, ms, vs = _named_groups("densify_and_prune", optimizer, dict(zip(names, ("xyz", "scaling", "rotation"))))
    new_t, new_m, new_v, _ = densify_tensors(plan, params, roles, ms, vs, noise, split_shrink=split_shrink, raw=raw)
    return _replace_group_tensors(optimizer, groups, params, new_t, new_m, new_v)


def mcmc_relocation_plan(opacity: torch.Tensor, uniforms: torch.Tensor, *, min_opacity: float = 0.005, raw: bool = True, return_weights: bool = False):
    """The draw of 3DGS-MCMC's relocate_gs in four small kernels without host synchronisation (extension; include/stp_raster.h: stp_mcmc_sample)
    -> (src int32 (P,), count int32 (P,)) and, with return_weights, the int32 (P,) weights.  With o the opacity (its sigmoid where raw, the model's
    stored _opacity): a row with o <= min_opacity is dead and draws a source among the rows with o > min_opacity, with replacement, with
    probability proportional to o; src[i] is the source of dead row i and -1 on every other row, count[k] the number of dead rows that drew k.
    uniforms: (P,) float32 in [0, 1), torch.rand(P) -- the random numbers stay torch's, and only the dead rows' entries are read.  The draw is an
    inverse CDF over the integer weights rint(o * 2^24) in exact 64-bit sums: equal inputs give equal bits, and a test can restate it with
    cumsum and searchsorted.  No dead row, or no live one: src is all -1 and count all 0 (decided on the device).  A NaN opacity is neither
    dead nor drawn.  min_opacity is rounded to float32 once."""
    return _mcmc_plan(opacity, uniforms, 0, min_opacity, raw, return_weights)


def _mcmc_plan(opacity, uniforms, rule, min_opacity, raw, return_weights):
    src, count, weights = _C.mcmc_sample(opacity.detach(), uniforms.detach(), rule, _f32(min_opacity), raw, return_weights)
    return (src, count, weights) if return_weights else (src, count)


def mcmc_relocate_tensors_(plan, tensors, roles, exp_avgs=None, exp_avg_sqs=None, *, min_opacity: float = 0.005, raw: bool = True,
                           reset_dead_moments: bool = False) -> None:
    """3DGS-MCMC's relocate_gs by a plan of mcmc_relocation_plan, IN PLACE on every tensor and both Adam moments, in one pass per eight tensors and
    without host synchronisation (extension; include/stp_raster.h: stp_mcmc_relocate_apply).  tensors: float32 (P, ...) of any trailing shape,
    contiguous; roles: per tensor "plain" / "opacity" / "scaling" (or 0..2) with exactly one opacity, (P,) or (P, 1), and one scaling, (P, 3);
    exp_avgs / exp_avg_sqs: the moments per tensor, None where there are none.  A drawn row k (count[k] > 0) gets the opacity and scaling
    compute_relocation gives for N = count[k] + 1 (clamped to 50), the opacity clamped to [min_opacity, 1 - eps] -- stored through logit and log
    where raw -- and zero moments in every tensor; a dead row i takes every parameter of row src[i], with that row's new opacity and scaling, and
    keeps its moments (upstream) unless reset_dead_moments.  Every other float keeps its bits.  The new values are computed per source before
    anything is written: the result does not depend on scheduling.  Works on the tensors' storage like an optimizer step (nothing is recorded
    in autograd).  Returns None."""
    src, count = plan[0], plan[1]
    tensors, roles, exp_avgs, exp_avg_sqs = _row_lists(tensors, roles, _C.MCMC_ROLES, exp_avgs, exp_avg_sqs)
    _C.mcmc_relocate_apply(src, count, tensors, roles, exp_avgs, exp_avg_sqs, _f32(min_opacity), raw, reset_dead_moments)


def _mcmc_groups(who, optimizer, names):
    groups, params, roles, ms, vs = _named_groups(who, optimizer, dict(zip(names, ("opacity", "scaling"))))
    if roles.count("opacity") != 1 or roles.count("scaling") != 1:
        raise ValueError(f"{who}: the optimizer needs exactly one group named {names[0]!r} and one named {names[1]!r}")
    return groups, params, roles, ms, vs


def mcmc_relocate_(optimizer, uniforms: Optional[torch.Tensor] = None, *, min_opacity: float = 0.005, raw: bool = True, reset_dead_moments: bool = False,
                   names=("opacity", "scaling")):
    """3DGS-MCMC's relocate_gs on an optimizer (extension): the draw and the in-place rewrite of every group's tensor and moments, without host
    synchronisation -> the plan (src, count).  `optimizer`: a torch.optim.Adam or a SparseGaussianAdam whose groups hold one tensor each and carry
    "name"; the groups named names = (opacity, scaling) play those roles.  uniforms: (P,) float32 in [0, 1); None draws torch.rand(P) on the
    model's device.  The Parameters keep their identity and optimizer.state is untouched apart from the contents of exp_avg and exp_avg_sq.
    int((plan[0] >= 0).sum()) is the number of Gaussians relocated (a host synchronisation of the caller's choosing)."""
    groups, params, roles, ms, vs = _mcmc_groups("mcmc_relocate_", optimizer, names)
    opacity = params[roles.index("opacity")]
    if uniforms is None:
        uniforms = torch.rand(opacity.shape[0], device=opacity.device, dtype=torch.float32)
    plan = mcmc_relocation_plan(opacity, uniforms, min_opacity=min_opacity, raw=raw)
    mcmc_relocate_tensors_(plan, params, roles, ms, vs, min_opacity=min_opacity, raw=raw, reset_dead_moments=reset_dead_moments)
    return plan


def mcmc_add_plan(opacity: torch.Tensor, uniforms: torch.Tensor, *, raw: bool = True):
    """The draw of 3DGS-MCMC's add_new_gs (extension; include/stp_raster.h: stp_mcmc_sample, rule 1) -> (src int32 (n,), count int32 (P,)):
    one source per entry of uniforms ((n,) float32 in [0, 1), torch.rand(n)) among ALL rows, with probability proportional to the opacity (its
    sigmoid where raw), by the inverse CDF of mcmc_relocation_plan.  A model whose opacities are all 0 gives src = -1.  No host synchronisation."""
    return _mcmc_plan(opacity, uniforms, 1, 0.0, raw, False)


def mcmc_add_tensors(plan, tensors, roles, exp_avgs=None, exp_avg_sqs=None, *, min_opacity: float = 0.005, raw: bool = True):
    """3DGS-MCMC's add_new_gs by a plan of mcmc_add_plan, out of place, without host synchronisation (extension; include/stp_raster.h:
    stp_mcmc_add_apply) -> (new_tensors, new_exp_avgs, new_exp_avg_sqs) of P + n rows.  Rows [0, P) are the model's, bit for bit with their
    moments, except that a drawn row (count > 0) gets compute_relocation's opacity and scaling for N = count + 1 (as mcmc_relocate_tensors_
    stores them) and zero moments; row P + j is a copy of row src[j] with that row's new opacity and scaling and zero moments.  tensors, roles
    and moments as for mcmc_relocate_tensors_ (non-contiguous inputs are made contiguous); the inputs are not modified."""
    src, count = plan[0], plan[1]
    tensors, roles, exp_avgs, exp_avg_sqs = _row_lists(tensors, roles, _C.MCMC_ROLES, exp_avgs, exp_avg_sqs)
    return _C.mcmc_add_apply(src, count, tensors, roles, exp_avgs, exp_avg_sqs, _f32(min_opacity), raw)


def mcmc_add_new(optimizer, cap_max: int, uniforms: Optional[torch.Tensor] = None, *, min_opacity: float = 0.005, raw: bool = True, names=("opacity", "scaling")):
    """3DGS-MCMC's add_new_gs on an optimizer (extension): the model of P Gaussians grows by n_new = max(0, min(cap_max, int(1.05 * P)) - P)
    rows -- a host number: no read-back -- drawn with probability proportional to opacity.  Groups as for mcmc_relocate_; uniforms: (n_new,)
    float32 in [0, 1), None draws torch.rand(n_new).  Each group gets a new nn.Parameter in group["params"][0], optimizer.state moves onto it
    with the new exp_avg and exp_avg_sq exactly as densify_and_prune moves it (a group whose state is still empty stays empty; "step" is
    kept), and {name: new Parameter} is returned for the model to take -- an empty dict, and nothing changed, when n_new == 0."""
    groups, params, roles, ms, vs = _mcmc_groups("mcmc_add_new", optimizer, names)
    opacity = params[roles.index("opacity")]
    P = opacity.shape[0]
    n_new = max(0, min(int(cap_max), int(1.05 * P)) - P)
    if uniforms is not None and uniforms.shape[0] != n_new:
        raise ValueError(f"mcmc_add_new: uniforms has {uniforms.shape[0]} rows, n_new = max(0, min(cap_max, int(1.05 * P)) - P) = {n_new}")
    if n_new == 0:
        return {}
    if uniforms is None:
        uniforms = torch.rand(n_new, device=opacity.device, dtype=torch.float32)
    plan = mcmc_add_plan(opacity, uniforms, raw=raw)
    new_t, new_m, new_v = mcmc_add_tensors(plan, params, roles, ms, vs, min_opacity=min_opacity, raw=raw)
    return _replace_group_tensors(optimizer, groups, params, new_t, new_m, new_v)


def spatial_order(xyz: torch.Tensor, return_codes: bool = False):
    """The Morton order of a cloud (extension; include/stp_raster.h: stp_spatial_order): for xyz (P, 3) float32 on a GPU, the int32 (P,)
    tensor whose entry s is the index of the row that moves to position s -- `xyz[order]` is the cloud sorted along the curve -- and, with
    return_codes, (order, codes) with the int32 30-bit code of the row at every position.  It is the order knn_mean_dist2 searches in, fixed
    to the bit: per axis the coordinates become order-preserving integers (-0 below +0, the infinities at the ends), 1023 splitters cut their
    sorted sequence into 1024 runs of equal length (splitter[k - 1] = sorted[k P // 1024]), a point's cell is the number of splitters <= its
    coordinate, the code interleaves the three 10-bit cells (x lowest), and the order is the stable ascending sort of (code, index).  Cells
    of equal count survive outliers and clusters; the codes depend on the multiset of coordinates only, so the order of an ordered cloud is
    arange(P).  On the current stream, without host synchronisation and without atomics: equal inputs give equal bits.  xyz is detached, a
    non-contiguous view is made contiguous, P == 0 gives empty tensors.  Refused with a RuntimeError naming the argument: another dtype
    ("xyz: expected float32"), another shape ("xyz must be (P, 3)"), a CPU tensor ("no CPU path")."""
    order, codes = _C.spatial_order(xyz.detach(), return_codes)
    return (order, codes) if return_codes else order


def gather_tensors(index: torch.Tensor, tensors, exp_avgs=None, exp_avg_sqs=None):
    """Row s of every output is row index[s] of its input, bit for bit, for every tensor and both Adam moments, in one launch per eight
    tensors and without host synchronisation (extension; include/stp_raster.h: stp_gather_rows) -> (new_tensors, new_exp_avgs,
    new_exp_avg_sqs), lists as long as `tensors` with None where there are no moments.  index: int32 (M,) (an int64 index is converted) --
    a permutation such as spatial_order's, a subset, or a list with repeats; tensors: float32 or int32 (P, ...) of any trailing shape on
    index's GPU; exp_avgs / exp_avg_sqs: the moments per tensor, None where there are none (None: no moments at all).  The rows are moved,
    never computed on: NaN payloads and -0 keep their bits.  AN INDEX OUTSIDE [0, P) IS READ AS THE NEAREST VALID ROW (nothing is read out
    of bounds, nothing is reported).  The inputs are not modified; non-contiguous ones are made contiguous."""
    if isinstance(index, torch.Tensor) and index.dtype == torch.int64:
        index = index.to(torch.int32)
    tensors, _, exp_avgs, exp_avg_sqs = _row_lists(tensors, None, None, exp_avgs, exp_avg_sqs)
    return _C.gather_rows(index, tensors, exp_avgs, exp_avg_sqs)


def reorder_gaussians_(optimizer, order: Optional[torch.Tensor] = None, *, xyz: str = "xyz", extra=()):
    """Re-sort a model along the Morton curve (or by any `order`) on its optimizer (extension) -> (new_params, order, new_extra).
    `optimizer`: a torch.optim.Adam, SparseGaussianAdam or GaussianAdam whose groups hold one tensor each and carry "name", as
    densify_and_prune takes it.  order=None computes spatial_order of the group named `xyz`; otherwise order is an int32 (P,) permutation,
    order[s] the row that moves to position s.  Every group's tensor, both moments and the tensors of `extra` -- the trainer's per-Gaussian
    side buffers (xyz_gradient_accum, denom, max_radii2D, ...: float32 or int32 (P, ...)) -- go through ONE gather_tensors call.  Each group
    gets a new nn.Parameter in group["params"][0], optimizer.state moves onto it with the new exp_avg and exp_avg_sq exactly as
    densify_and_prune moves it (a group whose state is still empty stays empty; "step" and every group option are kept); new_params =
    {name: new Parameter} is for the model to take, new_extra the permuted side buffers in the order given.  No host synchronisation.
    What indexes rows and is not handed in (a visibility mask of the last render, cached activations) is stale afterwards."""
    groups, params, _, ms, vs = _named_groups("reorder_gaussians_", optimizer, {})
    extra = list(extra)
    if order is None:
        named = [p for g, p in zip(groups, params) if g["name"] == xyz]
        if len(named) != 1:
            raise ValueError(f"reorder_gaussians_: the optimizer needs exactly one group named {xyz!r} to order by (or pass order=)")
        order = spatial_order(named[0])
    n = len(params)
    new_t, new_m, new_v = gather_tensors(order, list(params) + extra, list(ms) + [None] * len(extra), list(vs) + [None] * len(extra))
    return _replace_group_tensors(optimizer, groups, params, new_t[:n], new_m[:n], new_v[:n]), order, new_t[n:]
