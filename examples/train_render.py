#!/usr/bin/env python3
"""Trainer-side caller: the `render()` function a 3DGS / StopThePop trainer wraps around the rasterizer (upstream
`gaussian_renderer/__init__.py`), written against this package, plus a tiny optimisation
loop on a synthetic scene that shows the forward + backward of the hot path in its natural habitat.

    PYTHONPATH=stopthepop-rasterization_amd python examples/train_render.py [--iters 30] [--config full|min|kbuffer|global] [--absgrad] [--prune-views N] [--mask-weight W] [--depth-weight W] [--optimizer adam|sparse_adam|gaussian_adam] [--loss l1|l1_ssim] [--strategy none|mcmc|adc] [--relocate torch|fused] [--cap-max N] [--split-sh] [--raw-params] [--init-scales scene|knn] [--reorder N] [--filter-3d]

`render()` takes the trainer's usual objects by duck typing:
  camera : image_width, image_height, FoVx, FoVy, world_view_transform, full_proj_transform, camera_center
  model  : get_xyz, get_opacity, get_scaling, get_rotation, get_features, active_sh_degree
           (a model with `split_sh` set also has get_features_dc and get_features_rest, which are then passed as they are;
            a model with `raw_params` set hands over _scaling, _rotation and _opacity, its stored parameters, to GaussianRasterizer(..., raw=True);
            a model whose `filter_3d` is a tensor renders from filtered_activations(_scaling, _opacity, filter_3d), Mip-Splatting's 3D filter)
and returns the trainer's usual dict (render, viewspace_points, visibility_filter, radii; "alpha" and "invdepth" too when asked for).
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "stopthepop-rasterization_amd"))
from diff_gaussian_rasterization import (CullingSettings, ExtendedSettings, GaussianRasterizationSettings,  # noqa: E402
                                         GaussianRasterizer, GlobalSortOrder, SortMode, SortQueueSizes, SortSettings, GaussianAdam, SparseGaussianAdam, compute_relocation,
                                         compute_3d_filter, densification_stats_, densify_and_prune, densify_plan, filtered_activations, mcmc_add_new, mcmc_add_noise_, mcmc_relocate_, reorder_gaussians_, scenes, training_loss, training_terms)


def render(camera, model, bg_color: torch.Tensor, splat_args: ExtendedSettings, scaling_modifier: float = 1.0,
           override_color: torch.Tensor | None = None, render_depth: bool = False, debug: bool = False):
    """One frame.  Gradients flow to every model tensor; `viewspace_points.grad` is the screen-space positional
    gradient densification uses -- and with `splat_args._absgrad = True`, `viewspace_points.absgrad` (after backward) the
    sum of the ABSOLUTE per-pixel contributions to it (AbsGS / gsplat's absgrad).
    `bg_color` is three floats or a (3, H, W) image the frame is composed onto; where it requires grad it gets one.  With
    `splat_args._alpha = True` the dict also carries "alpha", the pixel's opacity (1, H, W), differentiable like the image
    (INTEGRATION.md section 3h); with `splat_args._invdepth = True` "invdepth", the blended inverse depth sum alpha T / z (1, H, W) that
    upstream's rasterizer returns as `invdepths`, differentiable too.
    A model with `split_sh` hands its two SH parameters over as they are -- dc=_features_dc, shs=_features_rest -- where a trainer
    otherwise concatenates them every step.  A model with `raw_params` hands over its stored _opacity (logit),
    _scaling (log) and _rotation (unnormalised) to a rasterizer made with raw=True: sigmoid, exp and normalize run inside the rasterizer's kernels, and the
    gradients arrive on the three leaves without an activated copy in between.  A model with a `filter_3d` buffer
    (Mip-Splatting; compute_3d_filter over the training cameras) renders from filtered_activations(_scaling, _opacity, filter_3d): one kernel in
    place of get_scaling_with_3D_filter and get_opacity_with_3D_filter, the gradients arriving on _scaling and _opacity."""
    screenspace_points = torch.zeros_like(model.get_xyz, requires_grad=True)
    raster_settings = GaussianRasterizationSettings(
        image_height=int(camera.image_height), image_width=int(camera.image_width),
        tanfovx=math.tan(camera.FoVx * 0.5), tanfovy=math.tan(camera.FoVy * 0.5), bg=bg_color,
        scale_modifier=scaling_modifier, viewmatrix=camera.world_view_transform, projmatrix=camera.full_proj_transform,
        inv_viewprojmatrix=camera.full_proj_transform.inverse(), sh_degree=model.active_sh_degree,
        campos=camera.camera_center, prefiltered=False, settings=splat_args, render_depth=render_depth, debug=debug)
    raw = bool(getattr(model, "raw_params", False))
    rasterizer = GaussianRasterizer(raster_settings=raster_settings, raw=raw)
    shs, colors, dc = (None, override_color, None) if override_color is not None else (model.get_features, None, None)
    if override_color is None and getattr(model, "split_sh", False):   # no torch.cat: the two leaves go in, their two .grad come out
        shs, dc = model.get_features_rest, model.get_features_dc
    if raw:
        image, radii, *extra = rasterizer(means3D=model.get_xyz, means2D=screenspace_points, shs=shs, colors_precomp=colors,
                                          opacities=model._opacity, scales=model._scaling, rotations=model._rotation, dc=dc)
    else:
        if getattr(model, "filter_3d", None) is not None:
            scales, opacities = filtered_activations(model._scaling, model._opacity, model.filter_3d)
        else:
            scales, opacities = model.get_scaling, model.get_opacity
        image, radii, *extra = rasterizer(means3D=model.get_xyz, means2D=screenspace_points, shs=shs, colors_precomp=colors,
                                          opacities=opacities, scales=scales, rotations=model.get_rotation, dc=dc)
    out = {"render": image, "viewspace_points": screenspace_points, "visibility_filter": radii > 0, "radii": radii}
    if getattr(splat_args, "_alpha", False):      # (the extra outputs in their order: alpha, then the inverse depth)
        out["alpha"] = extra.pop(0)
    if getattr(splat_args, "_invdepth", False):
        out["invdepth"] = extra.pop(0)
    return out


def splat_config(name: str) -> ExtendedSettings:
    """The settings files the reference ships (configs/*.json), as objects."""
    hier = lambda order: SortSettings(queue_sizes=SortQueueSizes(64, 8, 4), sort_mode=SortMode.HIER, sort_order=order)
    if name == "full":  # hierarchical resort + every culling option + per-tile depth (the paper's default)
        return ExtendedSettings(sort_settings=hier(GlobalSortOrder.PTD_MAX), culling_settings=CullingSettings(True, True, True, True),
                                load_balancing=True, proper_ewa_scaling=False)
    if name == "min":
        return ExtendedSettings(sort_settings=hier(GlobalSortOrder.Z_DEPTH))
    if name == "kbuffer":
        return ExtendedSettings(sort_settings=SortSettings(queue_sizes=SortQueueSizes(64, 8, 16), sort_mode=SortMode.PPX_KBUFFER))
    return ExtendedSettings()  # plain 3DGS: global sort by view-space z


class ToyGaussians(torch.nn.Module):
    """The part of the trainer's GaussianModel that render() touches (activations included)."""

    def __init__(self, sc: scenes.Scene, device, split_sh: bool = False, raw_params: bool = False):
        super().__init__()
        self.split_sh = split_sh
        self.raw_params = raw_params   # render() passes the stored parameters with raw=True (the regularisers keep using get_opacity / get_scaling)
        t = lambda a: torch.nn.Parameter(torch.tensor(a, device=device))
        self._xyz = t(sc.means3D)
        self._scaling = torch.nn.Parameter(torch.log(torch.tensor(sc.scales, device=device)))
        self._rotation = t(sc.rotations)
        op = torch.tensor(sc.opacities, device=device).clamp(1e-4, 1 - 1e-4)
        self._opacity = torch.nn.Parameter(torch.log(op / (1 - op)))
        if split_sh:   # the trainers' two parameters, with their two learning rates
            self._features_dc, self._features_rest = t(sc.shs[:, :1].copy()), t(sc.shs[:, 1:].copy())
        else:
            self._features = t(sc.shs)
        self.active_sh_degree = sc.sh_degree
        self.filter_3d = None   # --filter-3d: Mip-Splatting's buffer, (P, 1), no gradient

    get_xyz = property(lambda s: s._xyz)
    get_scaling = property(lambda s: torch.exp(s._scaling))
    get_rotation = property(lambda s: torch.nn.functional.normalize(s._rotation))
    get_opacity = property(lambda s: torch.sigmoid(s._opacity))
    get_features = property(lambda s: torch.cat((s._features_dc, s._features_rest), dim=1) if s.split_sh else s._features)
    get_features_dc = property(lambda s: s._features_dc)
    get_features_rest = property(lambda s: s._features_rest)

    def feature_groups(self, lr: float):
        """The optimizer groups of the SH coefficients: one, or upstream's two with feature_lr / 20 for the rest; named as
        densify_and_prune carries them."""
        if self.split_sh:
            return [{"params": [self._features_dc], "lr": lr, "name": "f_dc"}, {"params": [self._features_rest], "lr": lr / 20.0, "name": "f_rest"}]
        return [{"params": [self._features], "lr": lr, "name": "f"}]

    def feature_params(self):
        return [self._features_dc, self._features_rest] if self.split_sh else [self._features]

    def take_features(self, new: dict):
        """the Parameters densify_and_prune returned, by group name"""
        if self.split_sh:
            self._features_dc, self._features_rest = new["f_dc"], new["f_rest"]
        else:
            self._features = new["f"]


def camera_of(sc: scenes.Scene, device):
    t = lambda a: torch.tensor(a, device=device)
    return SimpleNamespace(image_width=sc.W, image_height=sc.H, FoVx=2 * math.atan(sc.tanfovx), FoVy=2 * math.atan(sc.tanfovy),
                           world_view_transform=t(sc.viewmatrix), full_proj_transform=t(sc.projmatrix), camera_center=t(sc.campos))


def update_filter_3d(model: ToyGaussians, cameras) -> None:
    """Mip-Splatting's GaussianModel.compute_3D_filter(cameras): one fused pass over all cameras, no host synchronisation.  A trainer calls it once
    after loading and again after every step that changes the rows (densification, growth, a reordering) or resets opacities."""
    views = torch.stack([c.world_view_transform for c in cameras])
    intrinsics = torch.tensor([[c.image_width / (2.0 * math.tan(c.FoVx * 0.5)), c.image_height / (2.0 * math.tan(c.FoVy * 0.5)), c.image_width, c.image_height]
                               for c in cameras], dtype=torch.float32, device=views.device)
    model.filter_3d = compute_3d_filter(model.get_xyz, views, intrinsics)


def relocate_dead(model: ToyGaussians, opt: torch.optim.Optimizer, min_opacity: float = 0.005) -> int:
    """3DGS-MCMC's relocate_gs: every Gaussian whose opacity has fallen to min_opacity or below moves onto a live one, drawn with probability
    proportional to its opacity; a live Gaussian drawn k times is then there k + 1 times, and compute_relocation gives the opacity and scales
    that leave the rendered image unchanged.  Sampling and row copies are torch's; the Adam moments of the touched rows start again from
    zero.  Returns the number of Gaussians relocated."""
    with torch.no_grad():
        opacity = model.get_opacity.reshape(-1)
        dead = opacity <= min_opacity
        n_dead = int(dead.sum())
        if n_dead == 0 or n_dead == dead.numel():
            return 0
        dead_idx, alive_idx = dead.nonzero()[:, 0], (~dead).nonzero()[:, 0]
        sampled = alive_idx[torch.multinomial(opacity[alive_idx], n_dead, replacement=True)]
        ratio = torch.bincount(sampled, minlength=dead.numel())[sampled] + 1
        new_opacity, new_scaling = compute_relocation(model.get_opacity[sampled], model.get_scaling[sampled], ratio)   # (N is clamped to 50 inside)
        new_opacity = new_opacity.clamp(min_opacity, 1.0 - torch.finfo(torch.float32).eps)
        model._opacity[sampled] = torch.log(new_opacity / (1.0 - new_opacity))
        model._scaling[sampled] = torch.log(new_scaling)
        touched = torch.cat([sampled, dead_idx])
        for param in (model._xyz, *model.feature_params(), model._opacity, model._scaling, model._rotation):
            param[dead_idx] = param[sampled]
            state = opt.state.get(param)
            if state:
                state["exp_avg"][touched] = 0
                state["exp_avg_sq"][touched] = 0
    return n_dead


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--config", default="full", choices=["full", "min", "kbuffer", "global"])
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--size", type=int, nargs=2, default=[320, 240], metavar=("W", "H"))
    ap.add_argument("--absgrad", action="store_true", help="also accumulate the absolute screen-space gradient (densification statistic of AbsGS)")
    ap.add_argument("--prune-views", type=int, default=0, metavar="N",
                    help="after training, a pruning pass over N views: the largest blend weight of every Gaussian over the views, then a threshold")
    ap.add_argument("--mask-weight", type=float, default=0.0, metavar="W",
                    help="add W * mean |alpha - target alpha| to the loss: mask supervision on the rasterizer's alpha output")
    ap.add_argument("--depth-weight", type=float, default=0.0, metavar="W",
                    help="add W * mean |invdepth - target invdepth| to the loss: depth regularisation on the rasterizer's inverse-depth output "
                         "(upstream's `-d` monocular depth priors; INTEGRATION.md section 3k), as the third term of the fused training_loss "
                         "(INTEGRATION.md section 3s)")
    ap.add_argument("--exposure", action="store_true",
                    help="learn a (3, 4) exposure, initialised to the identity, with its own Adam: the render goes through it inside the fused "
                         "training_loss, the only route by which it gets a gradient without a torch matmul (INTEGRATION.md section 3s)")
    ap.add_argument("--optimizer", default="adam", choices=["adam", "sparse_adam", "gaussian_adam"],
                    help="sparse_adam: SparseGaussianAdam, one fused launch that steps only the Gaussians visible in the frame (INTEGRATION.md section 3i).  "
                         "gaussian_adam: GaussianAdam, torch.optim.Adam's own dense bias-corrected step in one fused launch; under --strategy mcmc the "
                         "opacity and scale regularisers leave the loss and ride in that launch (INTEGRATION.md section 3t)")
    ap.add_argument("--loss", default="l1", choices=["l1", "l1_ssim"],
                    help="l1_ssim: the trainers' 0.8 * L1 + 0.2 * (1 - SSIM) from the fused training_loss (INTEGRATION.md sections 3j, 3s)")
    ap.add_argument("--strategy", default="none", choices=["none", "mcmc", "adc"],
                    help="mcmc: 3DGS-MCMC -- the fused position noise after every optimizer step, dead Gaussians relocated every 10 iterations with "
                         "compute_relocation, and the opacity / scale L1 regularisers (INTEGRATION.md section 3l).  adc: 3DGS adaptive density control "
                         "-- the fused densification statistics after every backward, densify_plan + densify_and_prune every 10 iterations "
                         "(INTEGRATION.md section 3m)")
    ap.add_argument("--relocate", default="torch", choices=["torch", "fused"],
                    help="under --strategy mcmc, fused: mcmc_relocate_ in place of the torch composition relocate_dead() -- the draw and the rewrite of every "
                         "tensor and both Adam moments without host synchronisation -- and mcmc_add_new (upstream's add_new_gs) every 10 iterations, "
                         "growing towards --cap-max (INTEGRATION.md section 3r)")
    ap.add_argument("--cap-max", type=int, default=None, metavar="N", help="the most Gaussians --relocate fused grows to (default: 1.15 x --points)")
    ap.add_argument("--split-sh", action="store_true",
                    help="the model keeps _features_dc and _features_rest as two parameters (two optimizer groups, the rest at a twentieth of the "
                         "learning rate, as upstream) and renders with dc=: no torch.cat per step (INTEGRATION.md section 3n)")
    ap.add_argument("--raw-params", action="store_true",
                    help="render from the stored parameters: _opacity, _scaling and _rotation go in with raw=True and sigmoid / exp / normalize "
                         "run inside the rasterizer's kernels (INTEGRATION.md section 3q)")
    ap.add_argument("--init-scales", default="scene", choices=["scene", "knn"],
                    help="knn: the model's initial _scaling comes from the points alone, as the trainers' GaussianModel.create_from_pcd sets it: "
                         "log(sqrt(clamp_min(distCUDA2(xyz), 1e-7))) on all three axes, with `from simple_knn._C import distCUDA2` "
                         "(INTEGRATION.md section 3p)")
    ap.add_argument("--reorder", type=int, default=0, metavar="N",
                    help="every N iterations re-sort the model along the Morton curve of its positions: reorder_gaussians_ moves every tensor, both "
                         "Adam moments and the densification statistics in one gather (INTEGRATION.md section 3u)")
    ap.add_argument("--filter-3d", action="store_true",
                    help="Mip-Splatting's 3D smoothing filter: compute_3d_filter over the example's camera once and again after every densification, growth "
                         "or reordering, and the render from filtered_activations(_scaling, _opacity, filter_3d) (INTEGRATION.md section 3v)")
    args = ap.parse_args(argv)
    if args.filter_3d and args.raw_params:
        raise SystemExit("--filter-3d cannot be combined with --raw-params: raw=True makes the rasterizer's kernels activate the stored parameters "
                         "themselves, and they do not read filter_3d; the filtered activations feed the ordinary scales= / opacities= call")
    if not torch.cuda.is_available():
        raise SystemExit("this example needs a GPU (the rasterizer has no CPU path)")
    dev = torch.device("cuda:0")
    W, H = args.size
    target_scene = scenes.make_scene(P=args.points, W=W, H=H, sigma_min=1.0, sigma_max=9.0, seed=3, camera="orbit")
    cam, bg, cfg = camera_of(target_scene, dev), torch.tensor(target_scene.bg, device=dev), splat_config(args.config)
    masked = args.mask_weight > 0.0
    target_cfg = splat_config(args.config)
    target_cfg._alpha = masked   # (the target's own opacity is the mask the fit is supervised with)
    with_depth = args.depth_weight > 0.0
    target_cfg._invdepth = with_depth   # (... and its own inverse depth the depth prior)
    with torch.no_grad():
        target_out = render(cam, ToyGaussians(target_scene, dev), bg, target_cfg)
        target, target_alpha, target_invdepth = target_out["render"], target_out.get("alpha"), target_out.get("invdepth")

    # start from perturbed colours and opacities and fit them back
    model = ToyGaussians(target_scene, dev, split_sh=args.split_sh, raw_params=args.raw_params)
    with torch.no_grad():
        for f in model.feature_params():
            f.mul_(0.3)
        model._opacity.sub_(1.0)
        if args.init_scales == "knn":   # create_from_pcd's three lines, import included
            from simple_knn._C import distCUDA2
            dist2 = torch.clamp_min(distCUDA2(model._xyz.detach().float()), 0.0000001)
            model._scaling.copy_(torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3))
            print(f"initial scales from distCUDA2 over {dist2.numel()} points: mean 3-NN distance {float(torch.sqrt(dist2).mean()):.4f}")
    if args.filter_3d:
        update_filter_3d(model, [cam])
        print(f"filter_3d over 1 camera: {float(model.filter_3d.min()):.5f} .. {float(model.filter_3d.max()):.5f}")
    adc = args.strategy == "adc"
    fused_mcmc = args.strategy == "mcmc" and args.relocate == "fused"
    cap_max = args.cap_max if args.cap_max is not None else (115 * args.points) // 100
    if args.optimizer == "gaussian_adam":   # the class name is all that changes against the torch.optim.Adam below
        opt = GaussianAdam([*model.feature_groups(2e-2), {"params": [model._opacity], "lr": 5e-2, "name": "opacity"},
                            {"params": [model._xyz], "lr": 0.0, "name": "xyz"}, {"params": [model._scaling], "lr": 0.0, "name": "scaling"},
                            {"params": [model._rotation], "lr": 0.0, "name": "rotation"}], lr=0.0, eps=1e-15)
    elif (adc or fused_mcmc or args.reorder > 0) and args.optimizer != "sparse_adam":   # densify_and_prune, mcmc_relocate_ and reorder_gaussians_ want the trainers' layout: one named group per tensor
        opt = torch.optim.Adam([*model.feature_groups(2e-2), {"params": [model._opacity], "lr": 5e-2, "name": "opacity"},
                                {"params": [model._xyz], "lr": 0.0, "name": "xyz"}, {"params": [model._scaling], "lr": 0.0, "name": "scaling"},
                                {"params": [model._rotation], "lr": 0.0, "name": "rotation"}], lr=0.0, eps=1e-15)
    elif args.optimizer == "sparse_adam":   # one group per tensor, as the trainers' training_setup() builds them
        opt = SparseGaussianAdam([*model.feature_groups(2e-2), {"params": [model._opacity], "lr": 5e-2, "name": "opacity"},
                                  {"params": [model._xyz], "lr": 0.0, "name": "xyz"}, {"params": [model._scaling], "lr": 0.0, "name": "scaling"},
                                  {"params": [model._rotation], "lr": 0.0, "name": "rotation"}], lr=0.0, eps=1e-15)
    else:
        opt = torch.optim.Adam([*model.feature_groups(2e-2), {"params": [model._opacity], "lr": 5e-2},
                                {"params": [model._xyz, model._scaling, model._rotation], "lr": 0.0}])
    exposure = exposure_opt = None
    if args.exposure:   # upstream's per-image exposure (one image here), with its own optimizer as there
        exposure = torch.eye(3, 4, device=dev).requires_grad_(True)
        exposure_opt = torch.optim.Adam([exposure], lr=1e-3)
    train_cfg = splat_config(args.config)
    train_cfg._alpha = masked
    train_cfg._invdepth = with_depth
    train_cfg._absgrad = args.absgrad   # (a request on the settings object; the depth rendering below keeps the plain settings: it refuses it)
    # the densification statistic a trainer accumulates between two densify steps: the norm of the 2D positional gradient per visible
    # Gaussian -- signed (3DGS: pulls from opposite sides cancel) and, with --absgrad, absolute (AbsGS: they add up)
    stat_signed = torch.zeros(model.get_xyz.shape[0], device=dev)
    stat_abs = torch.zeros_like(stat_signed)
    # --strategy adc: the same sums from the fused statistics kernel, with the trainer's denom and max_radii2D beside them
    stat_denom, stat_radii, abs_denom = torch.zeros_like(stat_signed), torch.zeros_like(stat_signed), torch.zeros_like(stat_signed)
    extent = 1.1 * float((model.get_xyz.detach() - model.get_xyz.detach().mean(dim=0)).norm(dim=1).max())   # (a trainer's cameras_extent)
    grown = pruned = 0
    first = last = None
    label = "L1" if args.loss == "l1" else "0.8 L1 + 0.2 (1 - SSIM)"
    mcmc = args.strategy == "mcmc"
    noise_scale = 5e5 * 1.6e-4   # upstream's noise_lr times its initial position learning rate (the positions themselves are not fitted here)
    relocated = relocations = 0   # (--relocate fused: `relocated` is a device scalar until the end: counting must not synchronise either)
    added = 0
    fused_reg = mcmc and args.optimizer == "gaussian_adam"
    reg_value = 0.0
    if fused_reg:   # opacity_reg * |sigmoid(_opacity)|.mean() and scale_reg * |exp(_scaling)|.mean(), as gradients inside the step
        opt.set_regularizer("opacity", "sigmoid", 0.01)
        opt.set_regularizer("scaling", "exp", 0.01)
    if mcmc:
        torch.manual_seed(0)   # (the noise and the sampling are torch's: a run is reproducible)
        with torch.no_grad():  # every fiftieth Gaussian starts dead (opacity 0.002), so that the first relocation has work whatever the fit does
            model._opacity[::50] = math.log(0.002 / 0.998)
    for it in range(args.iters):
        out = render(cam, model, bg, train_cfg)
        extras = {}   # what the fused loss takes beside image and target: the exposure and the depth term ride in its kernels
        if exposure is not None:
            extras["exposure"] = exposure
        if with_depth:   # (the inverse depth is an output of the same autograd node: no second render)
            extras.update(invdepth=out["invdepth"], mono_invdepth=target_invdepth)
        if args.loss == "l1_ssim":   # all terms from one fused kernel pair; the printed figure is this loss then
            loss = training_loss(out["render"], target, lambda_dssim=0.2, depth_weight=args.depth_weight, **extras)
        elif extras:
            terms = training_terms(out["render"], target, **extras)
            loss = terms[0] + args.depth_weight * terms[2]
        else:
            loss = (out["render"] - target).abs().mean()
        if masked:   # alpha is an output of the same autograd node: one backward serves both terms
            loss = loss + args.mask_weight * (out["alpha"] - target_alpha).abs().mean()
        if mcmc and fused_reg:   # the two terms' gradients are added inside the optimizer's kernel; their value is computed for the printed figure only
            if it % 10 == 0 or it == args.iters - 1:   # (the optimizer does not compute it: a trainer that logs it computes it itself, when it logs)
                with torch.no_grad():
                    reg_value = float(0.01 * torch.sigmoid(model._opacity).mean() + 0.01 * torch.exp(model._scaling).mean())
        elif mcmc:   # upstream's opacity_reg and scale_reg: L1 pressure that lets unneeded Gaussians die, to be relocated
            loss = loss + 0.01 * model.get_opacity.mean() + 0.01 * model.get_scaling.mean()
        opt.zero_grad(set_to_none=True)
        if exposure_opt is not None:
            exposure_opt.zero_grad(set_to_none=True)
        loss.backward()
        if exposure_opt is not None:
            exposure_opt.step()
        grad2d = out["viewspace_points"].grad  # what densification accumulates
        vis = out["visibility_filter"]
        if adc:   # one kernel, no mask indexing and no synchronisation: the forward's radii are the visibility
            densification_stats_(stat_signed, stat_denom, stat_radii, grad2d, out["radii"])
            if args.absgrad:
                densification_stats_(stat_abs, abs_denom, None, out["viewspace_points"].absgrad, out["radii"])
        else:
            stat_signed[vis] += grad2d[vis, :2].norm(dim=-1)
            if args.absgrad:   # assigned by every backward, never accumulated: the running sum is the trainer's
                stat_abs[vis] += out["viewspace_points"].absgrad[vis, :2].norm(dim=-1)
        if args.optimizer == "sparse_adam":   # the forward's radii are the visibility: no mask tensor on the way
            if not args.split_sh:
                # SparseGaussianAdam has no bias correction (as upstream's): its step t is (1 - b1^t) / sqrt(1 - b2^t) times Adam's, 3.2 at t = 1 and 6.5
                # at t = 10.  Upstream's groups bear that -- the higher-order SH coefficients step at a twentieth of the dc rate there -- but
                # this model's single SH tensor steps them all at the dc rate, and the fit's loss tripled within two steps (0.035 -> 0.123;
                # profiles/EXPERIMENTS.md).  The class reads group["lr"] at every step, so the correction goes in there, as a trainer's schedule would.
                group = next(g for g in opt.param_groups if g.get("name") == "f")
                b1, b2 = group["betas"]
                group["lr"] = 2e-2 * math.sqrt(1.0 - b2 ** (it + 1)) / (1.0 - b1 ** (it + 1))
            opt.step(out["radii"], model.get_xyz.shape[0])
        else:
            opt.step()
        if mcmc:
            if it > 0 and it % 10 == 0 and fused_mcmc:
                # upstream's relocate_gs and add_new_gs on the optimizer's named groups, without a host synchronisation: the Parameters keep their
                # identity through the relocation; the growth hands new ones back, as densify_and_prune does
                plan = mcmc_relocate_(opt, raw=True, reset_dead_moments=True)   # (relocate_dead() below zeroes the dead rows' moments too)
                relocated = relocated + (plan[0] >= 0).sum()
                relocations += 1
                new = mcmc_add_new(opt, cap_max, raw=True)
                if new:
                    before = model.get_xyz.shape[0]
                    model.take_features(new)
                    model._opacity, model._xyz, model._scaling, model._rotation = (new[n] for n in ("opacity", "xyz", "scaling", "rotation"))
                    added += model.get_xyz.shape[0] - before
                    stat_signed, stat_abs = (torch.zeros(model.get_xyz.shape[0], device=dev) for _ in range(2))
            elif it > 0 and it % 10 == 0:
                relocated += relocate_dead(model, opt)
                relocations += 1
            if args.filter_3d and it > 0 and it % 10 == 0:   # (relocated rows sit elsewhere now, and new rows have no entry yet)
                update_filter_3d(model, [cam])
            # xyz += Sigma (randn * op_sigmoid(1 - opacity) * noise_lr * xyz_lr) in one kernel, from the raw parameters the step just moved
            mcmc_add_noise_(model._xyz, model._scaling, model._rotation, model._opacity, torch.randn_like(model._xyz), noise_scale, raw=True)
        if args.reorder > 0 and it > 0 and it % args.reorder == 0:
            # rows that densification appended or relocation rewrote lie anywhere: every so often the model goes back into the Morton order of its
            # positions.  One gather moves every group's tensor, both Adam moments and the per-Gaussian statistics; the model takes the new
            # Parameters as after densify_and_prune.  (`out` of this iteration indexes the old rows: it is not used below this point.)
            new, order, (stat_signed, stat_abs, stat_denom, stat_radii, abs_denom) = reorder_gaussians_(
                opt, extra=[stat_signed, stat_abs, stat_denom, stat_radii, abs_denom])
            model.take_features(new)
            model._opacity, model._xyz, model._scaling, model._rotation = (new[n] for n in ("opacity", "xyz", "scaling", "rotation"))
            if args.filter_3d:   # (the rows moved)
                update_filter_3d(model, [cam])
            print(f"iter {it:3d}  reorder: {order.numel()} rows into Morton order")
        if adc and it > 0 and it % 10 == 0:
            # upstream's densify_and_prune: the decision as one byte per Gaussian, then one scan and one apply over every tensor and both
            # Adam moments; the optimizer's groups get the new Parameters and the model takes them from the returned dict
            plan = densify_plan(stat_signed, stat_denom, model._scaling, model._opacity, None, grad_threshold=0.0002, extent=extent, max_screen_size=20)
            before = plan.numel()
            new = densify_and_prune(opt, plan)
            model.take_features(new)
            model._opacity, model._xyz, model._scaling, model._rotation = (new[n] for n in ("opacity", "xyz", "scaling", "rotation"))
            after = model.get_xyz.shape[0]
            if args.filter_3d:
                update_filter_3d(model, [cam])
            kept, cloned, split = (int(((plan >> b) & 1).sum()) for b in range(3))
            grown, pruned = grown + cloned + 2 * split, pruned + before - kept
            print(f"iter {it:3d}  adc: {before} rows -> {after} (kept {kept}, cloned {cloned}, split {split} into {2 * split})")
            stat_signed, stat_abs, stat_denom, stat_radii, abs_denom = (torch.zeros(after, device=dev) for _ in range(5))   # (upstream's densification_postfix)
        last = float(loss.detach()) + reg_value
        first = last if first is None else first
        if it % 10 == 0 or it == args.iters - 1:
            print(f"iter {it:3d}  {label} {last:.5f}  visible {int(out['visibility_filter'].sum())}  |grad2D| max {float(grad2d.norm(dim=1).max()):.3e}")
    with torch.no_grad():
        depth = render(cam, model, bg, cfg, render_depth=True)["render"]
    if adc:
        print(f"adc: {grown} rows appended and {pruned} originals removed over the run, {model.get_xyz.shape[0]} Gaussians at the end")
    if mcmc:
        print(f"mcmc: relocated {int(relocated)} Gaussians in {relocations} relocation steps (opacity <= 0.005), position noise after each of {args.iters} steps")
        if fused_mcmc:
            print(f"mcmc: {added} Gaussians added towards cap_max = {cap_max}, {model.get_xyz.shape[0]} at the end")
    if exposure is not None:
        print(f"exposure: largest deviation from the identity {float((exposure.detach() - torch.eye(3, 4, device=dev)).abs().max()):.5f} after {args.iters} steps of its Adam")
    if args.absgrad:
        print(f"densification statistic, mean over Gaussians: signed {float(stat_signed.mean()):.3e}, absolute {float(stat_abs.mean()):.3e} "
              f"(absolute >= signed for {float((stat_abs >= stat_signed * (1 - 1e-5)).float().mean()) * 100:.1f} % of them)")
    if args.prune_views > 0:
        # A pruning pass (RadSplat): a Gaussian whose blend weight alpha * T stays below a threshold on EVERY ray of every view contributes
        # next to nothing to any pixel.  settings._blend_stats = True makes each backward leave means2D.blend_stats = (sum, max, count) of
        # the blend weights per Gaussian; column 1 is accumulated as a maximum over the views.  The
        # statistics do not depend on the loss: the sum of the image is as good as any.
        prune_cfg = splat_config(args.config)
        prune_cfg._blend_stats = True
        views = [cam] + [camera_of(scenes.make_scene(P=8, W=W, H=H, sigma_min=1.0, sigma_max=9.0, seed=3 + v, camera="origin" if v % 2 else "orbit"), dev)
                         for v in range(1, args.prune_views)]
        score = torch.zeros(model.get_xyz.shape[0], device=dev)
        hits = torch.zeros_like(score)
        for view in views:
            out = render(view, model, bg, prune_cfg)
            out["render"].sum().backward()
            stats = out["viewspace_points"].blend_stats   # assigned by every backward: the running maximum is the trainer's
            score = torch.maximum(score, stats[:, 1])
            hits += stats[:, 2]
        keep = score >= 0.01
        print(f"pruning pass over {len(views)} views: largest blend weight below 0.01 for {int((~keep).sum())} of {keep.numel()} Gaussians "
              f"({int((hits == 0).sum())} of them never blended); a trainer would now keep model tensors[keep]")
    print(f"{label} {first:.5f} -> {last:.5f}; depth visualisation {tuple(depth.shape)} in [{float(depth.min()):.3f}, {float(depth.max()):.3f}]")
    return first, last


if __name__ == "__main__":
    main()
