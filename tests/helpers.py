"""Shared helpers of the parity tests: settings dicts, running the product (GPU) and the oracle (CPU)
on the same synthetic scene, and comparison metrics; api_render(), the one forward + backward through the public
API that the tests of the opt-in backward outputs (camera gradients, absgrad, blend statistics) share."""
from __future__ import annotations

import numpy as np


def settings_dict(mode=0, order=0, per_pixel=4, tile_2x2=8, rect=False, tight=False, tbc=False, h44=False,
                  lb=False, ewa=False):
    """The reference's ExtendedSettings.to_dict() layout."""
    return {"sort_settings": {"queue_sizes": {"tile_4x4": 64, "tile_2x2": tile_2x2, "per_pixel": per_pixel},
                              "sort_mode": mode, "sort_order": order},
            "culling_settings": {"rect_bounding": rect, "tight_opacity_bounding": tight, "tile_based_culling": tbc,
                                 "hierarchical_4x4_culling": h44},
            "load_balancing": lb, "proper_ewa_scaling": ewa}


FULL_STP = dict(mode=3, order=3, rect=True, tight=True, tbc=True, h44=True, lb=True)  # "full StopThePop" (C2-full)


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 200.0 if mse == 0 else 10.0 * np.log10(1.0 / mse)


def max_abs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0


def ext_settings(d):
    """dict -> diff_gaussian_rasterization.ExtendedSettings"""
    import diff_gaussian_rasterization as dgr
    es = dgr.ExtendedSettings.from_dict(d)
    if d.get("_backward_mode"):   # (our per-call extension rides on the settings object, see ExtendedSettings.to_dict)
        es._backward_mode = d["_backward_mode"]
    return es


def _rel(a, b):
    """largest difference relative to b's largest entry"""
    return max_abs(a, b) / max(float(np.max(np.abs(b))), 1e-30)


GAUSS = ("means3D", "means2D", "shs", "colors_precomp", "opacities", "scales", "rotations")
CAMERA = ("viewmatrix", "projmatrix", "campos")


def _scene_a():
    from diff_gaussian_rasterization import scenes
    return scenes.make_scene(P=300, W=48, H=32, sigma_min=1.0, sigma_max=9.0, seed=4)


def _scene_b():
    from diff_gaussian_rasterization import scenes
    return scenes.make_scene(P=2500, W=48, H=32, sigma_min=2.0, sigma_max=12.0, seed=5, camera="orbit")   # lists of more than 1024 entries


def _precomp(sc, seed=11):
    """the scene with its colours given directly (colors_precomp as the leaf, no SH)"""
    sc.colors_precomp = np.random.default_rng(seed).uniform(0.05, 1.0, (len(sc.means3D), 3)).astype(np.float32)
    sc.shs = None
    return sc


def api_settings(sc, settings, device="cuda:0", render_depth=False, **camera):
    """GaussianRasterizationSettings of scene sc on `device`.  settings: an ExtendedSettings; camera: tensors that stand in for the
    scene's own viewmatrix, projmatrix, inv_viewprojmatrix or campos."""
    import torch
    import diff_gaussian_rasterization as dgr
    t = lambda n: camera[n] if n in camera else torch.tensor(np.asarray(getattr(sc, n), np.float32), device=device)
    return dgr.GaussianRasterizationSettings(
        image_height=sc.H, image_width=sc.W, tanfovx=sc.tanfovx, tanfovy=sc.tanfovy, bg=t("bg"), scale_modifier=sc.scale_modifier,
        viewmatrix=t("viewmatrix"), projmatrix=t("projmatrix"), inv_viewprojmatrix=t("inv_viewprojmatrix"), sh_degree=sc.sh_degree,
        campos=t("campos"), prefiltered=False, settings=settings, render_depth=render_depth, debug=False)


def api_render(sc, sdict, camera=(), gaussians=True, only=None, means2D_grad=True, cov3D=None, backward_mode=None, w=None,
               lit_pixel=None, render_depth=False, backwards=1, forward_only=False, absgrad=False, stats=False):
    """Forward + backward with dL_dout = w through the public API on cuda:0 (w: the scene's own dL_dout by default; the k-th of
    `backwards` rounds on the same tensors uses k * w).
    camera: the camera tensors that require grad (names; True: all three).  gaussians / only: do the Gaussian inputs require grad, and
    which of them (None: all); means2D_grad: does means2D.  cov3D: a (P, 6) array passed instead of scales and rotations.
    lit_pixel: flat index of the one pixel at which w is not zeroed.  forward_only: no backward.
    absgrad, stats: the settings._absgrad and settings._blend_stats requests.
    Returns a dict: "color", "radii", "grad_fn" (its type's name); "n_contrib" and "tile_flags" of the last forward that has a graph;
    per request "absgrad" / "stats" (means2D's attribute after the last backward, None without one), "has_absgrad" / "has_stats" and the
    list per backward, "absgrads" / "all_stats"; under its name every input's .grad (None where there is none)."""
    import torch
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    camera = CAMERA if camera is True else (camera or ())
    need = lambda n: gaussians and (only is None or n in only)
    t = lambda a, rg=False: None if a is None else torch.tensor(np.asarray(a, np.float32), device=dev).requires_grad_(rg)
    ten = {n: t(getattr(sc, n), need(n)) for n in ("means3D", "opacities", "shs", "colors_precomp", "scales", "rotations")}
    ten["cov3D_precomp"] = t(cov3D, need("cov3D_precomp"))
    if cov3D is not None:
        ten["scales"] = ten["rotations"] = None
    ten["means2D"] = torch.zeros_like(ten["means3D"], requires_grad=means2D_grad and need("means2D"))
    cam = {n: t(getattr(sc, n), n in camera) for n in CAMERA}
    d = dict(sdict)
    if backward_mode:
        d["_backward_mode"] = backward_mode
    es = ext_settings(d)
    if absgrad:
        es._absgrad = True
    if stats:
        es._blend_stats = True
    rs = api_settings(sc, es, dev, render_depth, **cam)
    out = {"absgrads": [], "all_stats": []}
    for k in range(backwards):
        color, radii = dgr.GaussianRasterizer(rs)(ten["means3D"], ten["means2D"], ten["opacities"], shs=ten["shs"],
                                                  colors_precomp=ten["colors_precomp"], scales=ten["scales"], rotations=ten["rotations"],
                                                  cov3D_precomp=ten["cov3D_precomp"])
        fn = color.grad_fn
        out["grad_fn"] = type(fn).__name__ if fn is not None else None
        if fn is not None and len(sc.means3D) > 0:
            img_buf = fn.saved_tensors[11]
            out["n_contrib"] = _C.image_array(img_buf, sc.W, sc.H, "n_contrib").reshape(-1)[:sc.W * sc.H].clone()
            try:
                out["tile_flags"] = _C.image_array(img_buf, sc.W, sc.H, "tile_flags").clone().cpu().numpy()
            except KeyError:
                out["tile_flags"] = None
        weight = torch.tensor(np.asarray(sc.dL_dout if w is None else w, np.float32), device=dev) * float(k + 1)
        if lit_pixel is not None:
            mask = torch.zeros(sc.H * sc.W, device=dev)
            mask[lit_pixel] = 1.0
            weight = weight * mask.view(1, sc.H, sc.W)
        if fn is not None and not forward_only:
            color.backward(weight)   # (dL_dout as it is: a non-finite one must reach the kernels, not a product with the image)
        for attr, every in (("absgrad", "absgrads"), ("blend_stats", "all_stats")):
            if hasattr(ten["means2D"], attr):
                out[every].append(getattr(ten["means2D"], attr))
    out["color"], out["radii"] = color.detach(), radii
    out["has_absgrad"], out["has_stats"] = hasattr(ten["means2D"], "absgrad"), hasattr(ten["means2D"], "blend_stats")
    out["absgrad"], out["stats"] = getattr(ten["means2D"], "absgrad", None), getattr(ten["means2D"], "blend_stats", None)
    for n, x in list(ten.items()) + list(cam.items()):
        out[n] = None if x is None or x.grad is None else x.grad.detach().clone()
    return out


def _direct(sc, sd, cov3D=None):
    """Forward through _C directly (the buffers a phase-split backward needs); returns the backward's positional arguments."""
    import torch
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda:0")
    empty = torch.Tensor([])
    t = lambda a: empty if a is None else torch.tensor(np.asarray(a, np.float32), device=dev)
    ten = dict(bg=t(sc.bg), means3D=t(sc.means3D), opac=t(sc.opacities), scales=t(None if cov3D is not None else sc.scales),
               rots=t(None if cov3D is not None else sc.rotations), cov=t(cov3D), shs=t(sc.shs), colors=t(sc.colors_precomp),
               view=t(sc.viewmatrix), proj=t(sc.projmatrix), inv=t(sc.inv_viewprojmatrix), cam=t(sc.campos), w=t(sc.dL_dout))
    out = _C.rasterize_gaussians(ten["bg"], ten["means3D"], ten["colors"], ten["opac"], ten["scales"], ten["rots"], sc.scale_modifier,
                                 ten["cov"], ten["view"], ten["proj"], ten["inv"], sc.tanfovx, sc.tanfovy, sc.H, sc.W, ten["shs"],
                                 sc.sh_degree, ten["cam"], False, sd, False, False)
    return (ten["bg"], ten["means3D"], out[2], ten["opac"], ten["colors"], ten["scales"], ten["rots"], sc.scale_modifier, ten["cov"],
            ten["view"], ten["proj"], ten["inv"], sc.tanfovx, sc.tanfovy, out[1], ten["w"], ten["shs"], sc.sh_degree, ten["cam"], out[3],
            out[0], out[4], out[5], sd, False)


class GpuRun:
    """Runs one scene through the product's public API on cuda:0 and keeps what the tests inspect."""

    def __init__(self, scene, sdict, backward=True, device="cuda:0", tile_rows=None, debug=False, render_depth=False,
                 cov3D_precomp=None, prefiltered=False, warm=True, run_ahead=None):
        """cov3D_precomp: (P,6) array -> passed INSTEAD of scales/rotations (ref: __init__.py:286-289 allows exactly one).
        warm: the frame is rendered TWICE.  The library's default forward takes the reference's path -- hand-over of num_rendered in the
        middle of the frame, exact binning size; with run-ahead switched on (_C.set_run_ahead) every forward but the first of its kind is
        launched as a whole on a capacity guessed from the frames before (stp_forward.hip).  The untracked first pass runs the default path,
        the second -- the one the tests inspect -- the run-ahead path; both must return the same image, radii and count, bit for bit.
        run_ahead (with warm=False): run this one frame with the switch set like this."""
        import torch
        import diff_gaussian_rasterization as dgr
        from diff_gaussian_rasterization import _C
        self.scene, self.sdict = scene, sdict
        dev = torch.device(device)
        t = lambda a, rg=False: None if a is None else torch.tensor(a, device=dev).requires_grad_(rg and backward)
        self.means3D, self.opac = t(scene.means3D, True), t(scene.opacities, True)
        self.scales, self.rots = t(scene.scales, True), t(scene.rotations, True)
        self.shs, self.colors = t(scene.shs, True), t(scene.colors_precomp, True)
        self.means2D = torch.zeros_like(self.means3D, requires_grad=backward)
        self.cov3D = t(cov3D_precomp, True)
        if self.cov3D is not None:
            self.scales = self.rots = None
        es = ext_settings(sdict)
        if tile_rows is not None:
            # tile-row window rides along in the dict through a private key (see _C.settings_from_dict)
            base = es.to_dict
            es.to_dict = lambda: {**base(), "_tile_rows": tuple(tile_rows)}
        rs = dgr.GaussianRasterizationSettings(
            image_height=scene.H, image_width=scene.W, tanfovx=scene.tanfovx, tanfovy=scene.tanfovy, bg=t(scene.bg),
            scale_modifier=scene.scale_modifier, viewmatrix=t(scene.viewmatrix), projmatrix=t(scene.projmatrix),
            inv_viewprojmatrix=t(scene.inv_viewprojmatrix), sh_degree=scene.sh_degree, campos=t(scene.campos),
            prefiltered=prefiltered, settings=es, render_depth=render_depth, debug=debug)
        self.rs = rs
        rast = dgr.GaussianRasterizer(rs)
        self.exact_pass = None
        self.run_ahead_before = None
        if warm and not debug:
            _C.reset_size_guesses()
            self.run_ahead_before = _C.set_run_ahead(0)
            empty_ = torch.Tensor([])
            e_ = lambda x: empty_ if x is None else x.detach()
            o = _C.rasterize_gaussians(rs.bg, self.means3D.detach(), e_(self.colors), self.opac.detach(), e_(self.scales), e_(self.rots),
                                       rs.scale_modifier, e_(self.cov3D), rs.viewmatrix, rs.projmatrix, rs.inv_viewprojmatrix, rs.tanfovx,
                                       rs.tanfovy, rs.image_height, rs.image_width, e_(self.shs), rs.sh_degree, rs.campos, prefiltered,
                                       es.to_dict(), render_depth, debug)
            self.exact_pass = (int(o[0]), o[1].clone(), o[2].clone())
            _C.release_scratch(o[5]); _C.release_scratch(o[4])
            del o
            _C.set_run_ahead(1)
        elif run_ahead is not None:
            self.run_ahead_before = _C.set_run_ahead(1 if run_ahead else 0)
        try:
            self._run(rast, rs, es, backward, dev, prefiltered, render_depth, debug)
        finally:
            if self.run_ahead_before is not None:
                _C.set_run_ahead(self.run_ahead_before)

    def _run(self, rast, rs, es, backward, dev, prefiltered, render_depth, debug):
        import torch
        from diff_gaussian_rasterization import _C
        scene = self.scene
        color, radii = rast(self.means3D, self.means2D, self.opac, shs=self.shs, colors_precomp=self.colors,
                            scales=self.scales, rotations=self.rots, cov3D_precomp=self.cov3D)
        self.color_t = color
        self.color = color.detach().cpu().numpy()
        self.radii = radii.cpu().numpy()
        if self.exact_pass is not None:   # exact path == run-ahead path, bit for bit (NaN == NaN: render_depth of an empty frame)
            if not torch.equal(torch.nan_to_num(self.exact_pass[1], nan=-1.0), torch.nan_to_num(color.detach(), nan=-1.0)):
                a_, b_ = self.exact_pass[1].cpu().numpy(), color.detach().cpu().numpy()
                bad = np.argwhere((a_ != b_) & ~(np.isnan(a_) & np.isnan(b_)))
                raise AssertionError(f"run-ahead forward differs from the exact one: {len(bad)} values, rows {bad[:, 1].min()}..{bad[:, 1].max()}, cols {bad[:, 2].min()}..{bad[:, 2].max()}, "
                                     f"exact {a_[tuple(bad[0])]} run-ahead {b_[tuple(bad[0])]}, counts {self.exact_pass[0]} / {getattr(color.grad_fn, 'num_rendered', None)}")
            assert torch.equal(self.exact_pass[2], radii)
        fn = color.grad_fn
        if fn is not None:
            self.num_rendered = fn.num_rendered
            assert self.exact_pass is None or self.exact_pass[0] == self.num_rendered
            saved = fn.saved_tensors
            self.geom, self.binning, self.img = saved[9], saved[10], saved[11]
        else:  # forward-only run (no tensor requires grad): fetch the scratch buffers with a direct _C call
            empty = torch.Tensor([])
            e = lambda x: empty if x is None else x
            out = _C.rasterize_gaussians(rs.bg, self.means3D, e(self.colors), self.opac, e(self.scales), e(self.rots), rs.scale_modifier,
                                         e(self.cov3D), rs.viewmatrix, rs.projmatrix, rs.inv_viewprojmatrix, rs.tanfovx, rs.tanfovy,
                                         rs.image_height, rs.image_width, e(self.shs), rs.sh_degree, rs.campos, prefiltered,
                                         es.to_dict(), render_depth, debug)
            self.num_rendered, color2 = out[0], out[1]
            assert torch.equal(torch.nan_to_num(color2, nan=-1.0), torch.nan_to_num(color, nan=-1.0))  # (render_depth of an empty frame is NaN, as in the reference)
            self.geom, self.binning, self.img = out[3], out[4], out[5]
        self._C = _C
        self.grads = None
        if backward:
            w = torch.tensor(scene.dL_dout, device=dev)
            (color * w).sum().backward()
            g = lambda x: None if x is None or x.grad is None else x.grad.detach().cpu().numpy()
            self.grads = dict(dL_dmeans3D=g(self.means3D), dL_dmeans2D=g(self.means2D), dL_dopacity=g(self.opac),
                              dL_dscales=g(self.scales), dL_drotations=g(self.rots), dL_dsh=g(self.shs),
                              dL_dcolors=g(self.colors), dL_dcov3D=g(self.cov3D))

    def geom_array(self, name):
        return self._C.geometry_array(self.geom, self.scene.P, self.sdict, name).cpu().numpy()

    def binning_array(self, name):
        a = self._C.binning_array(self.binning, self.num_rendered, name).cpu().numpy()
        return a.view(np.uint64) if a.dtype == np.int64 else a.view(np.uint32)

    def image_array(self, name):
        return self._C.image_array(self.img, self.scene.W, self.scene.H, name).cpu().numpy()


def oracle_run(scene, sdict, backward=True, tile_rows=None, render_depth=False, cov3D_precomp=None):
    from oracle import oracle as orc
    f = orc.forward_scene(scene, sdict, tile_rows=tile_rows, render_depth=render_depth, cov3D_precomp=cov3D_precomp)
    g = f.backward(scene.dL_dout) if backward else None
    return f, g
