// stp_bind_raster.h -- the reference's three functions (rasterize_points.cu:43-253): rasterize_gaussians, rasterize_gaussians_backward, mark_visible.
#pragma once

#include <tuple>

#include "stp_scratch_pool.h"
#include "stp_tensor_checks.h"

namespace {
// dict -> POD.  All keys are mandatory, as in the reference's json parser (rasterizer.h:160-182, every field read with
// .at()); a missing key raises KeyError where the reference raised json::out_of_range.
StpSettings settings_from_dict(const py::dict& d, bool record_log)
{
    StpSettings s{};
    const py::dict ss = d["sort_settings"].cast<py::dict>(), cs = d["culling_settings"].cast<py::dict>(), q = ss["queue_sizes"].cast<py::dict>();
    s.sort_mode = ss["sort_mode"].cast<int>();
    s.sort_order = ss["sort_order"].cast<int>();
    s.queue_tile_4x4 = q["tile_4x4"].cast<int>();
    s.queue_tile_2x2 = q["tile_2x2"].cast<int>();
    s.queue_per_pixel = q["per_pixel"].cast<int>();
    s.rect_bounding = cs["rect_bounding"].cast<bool>();
    s.tight_opacity_bounding = cs["tight_opacity_bounding"].cast<bool>();
    s.tile_based_culling = cs["tile_based_culling"].cast<bool>();
    s.hierarchical_4x4_culling = cs["hierarchical_4x4_culling"].cast<bool>();
    s.load_balancing = d["load_balancing"].cast<bool>();
    s.proper_ewa_scaling = d["proper_ewa_scaling"].cast<bool>();
    if (setting_present(d, "_tile_rows")) {
        const py::tuple tr = py::tuple(d["_tile_rows"]);
        s.tile_y0 = tr[0].cast<int>();
        s.tile_y1 = tr[1].cast<int>();
    }
    s.record_blend_log = record_log ? 1 : 0;
    return s;
}

// the twelve tensors that describe a frame to the forward and to the backward alike, checked and made contiguous in this order
struct FrameInputs { torch::Tensor bg, m3, sh, col, op, sc, ro, c3, vm, pm, inv, cam; };
FrameInputs prep_frame(const torch::Device& dev, const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& sh,
                       const torch::Tensor& colors, const torch::Tensor& opacity, const torch::Tensor& scales, const torch::Tensor& rotations,
                       const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                       const torch::Tensor& inv_viewprojmatrix, const torch::Tensor& campos)
{
    return {prep(background, dev), prep(means3D, dev), prep(sh, dev), prep(colors, dev), prep(opacity, dev), prep(scales, dev), prep(rotations, dev),
            prep(cov3D_precomp, dev), prep(viewmatrix, dev), prep(projmatrix, dev), prep(inv_viewprojmatrix, dev), prep(campos, dev)};
}

// a background of shape exactly (3, H, W) is a per-pixel one (include/stp_raster.h: stp_set_forward_background); every other is three floats
bool per_pixel_background(const torch::Tensor& bg, int H, int W)
{
    return bg.defined() && bg.dim() == 3 && bg.size(0) == 3 && bg.size(1) == H && bg.size(2) == W;
}

// dc (extension, include/stp_raster.h: stp_set_forward_split_sh / stp_set_backward_split_sh): the first SH coefficient as a tensor of its own,
// (P,1,3) or (P,3); `sh` is then the rest, (P,M-1,3), possibly empty.  Returns M, the total coefficient count.  Checked before any device work.
int split_sh_total(const torch::Tensor& dc, const torch::Tensor& sh, const torch::Tensor& means3D)
{
    const int64_t P = means3D.size(0);
    if (!((dc.dim() == 3 && dc.size(1) == 1 && dc.size(2) == 3) || (dc.dim() == 2 && dc.size(1) == 3)))
        throw std::runtime_error("dc must have dimensions (num_points, 1, 3) or (num_points, 3)");
    if (dc.size(0) != P) throw std::runtime_error("dc must have one row per Gaussian: " + std::to_string(dc.size(0)) + " rows for " + std::to_string(P) + " points");
    if (dc.scalar_type() != torch::kFloat32) throw std::runtime_error("dc must be a float32 tensor");
    if (dc.device() != means3D.device()) throw std::runtime_error("dc must be on the device of means3D");
    if (sh.numel() == 0) return 1;
    if (!(sh.dim() == 3 && sh.size(0) == P && sh.size(2) == 3))
        throw std::runtime_error("with dc, shs is the rest of the coefficients and must have dimensions (num_points, M - 1, 3)");
    if (sh.scalar_type() != torch::kFloat32 || sh.device() != means3D.device()) throw std::runtime_error("with dc, shs must be a float32 tensor on the device of means3D");
    return (int)sh.size(1) + 1;
}

// == RasterizeGaussiansCUDA (reference rasterize_points.cu:43-138).
// Returns (num_rendered, out_color (3,H,W), radii (P,) int32, geomBuffer, binningBuffer, imgBuffer, alpha).
// alpha (extension, include/stp_raster.h: stp_set_forward_background): with alpha = true the last element is 1 - final_T, (1,H,W); an
// undefined tensor otherwise.  A background of shape exactly (3,H,W) is composed per pixel.
// invdepth (extension, include/stp_raster.h: stp_set_forward_invdepth): with invdepth = true one more element behind alpha's: sum alpha T / z,
// (1,H,W); an undefined tensor otherwise.
// dc (keyword, extension): see split_sh_total; `sh` is then the (P,M-1,3) rest.  Ignored with precomputed colours.
// raw (keyword, extension, include/stp_raster.h: stp_set_forward_raw_params): bit 0 opacity, bit 1 scales, bit 2 rotations hold a trainer's raw
// parameters; the library checks the mask against the arrays it is handed.
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
rasterize_gaussians(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors, const torch::Tensor& opacity,
                    const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier, const torch::Tensor& cov3D_precomp,
                    const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, const torch::Tensor& inv_viewprojmatrix, const float tan_fovx,
                    const float tan_fovy, const int image_height, const int image_width, const torch::Tensor& sh, const int degree,
                    const torch::Tensor& campos, const bool prefiltered, const py::dict& settings, const bool render_depth, const bool debug,
                    const bool record_log, const bool alpha, const bool invdepth, const c10::optional<torch::Tensor>& dc, const int raw)
{
    need_library();
    if (raw != 0) require(g_api.set_forward_raw_params, "raw");
    TORCH_CHECK(means3D.dim() == 2 && means3D.size(1) == 3, "means3D must have dimensions (num_points, 3)");
    TORCH_CHECK(means3D.is_cuda(), GPU_ONLY);
    const bool split = dc.has_value() && dc->defined() && colors.numel() == 0; // (precomputed colours win)
    if (split) require(g_api.set_forward_split_sh, "dc");
    const int M_split = split ? split_sh_total(*dc, sh, means3D) : 0;
    const torch::Device dev = means3D.device();
    const int P = (int)means3D.size(0), H = image_height, W = image_width;
    const auto fopt = means3D.options().dtype(torch::kFloat32), iopt = means3D.options().dtype(torch::kInt32), bopt = means3D.options().dtype(torch::kByte);
    // the render kernels write every pixel of the tile rows they cover and preprocess writes every Gaussian's radius:
    // zero-filled outputs are only needed when nothing runs (P == 0) or when a tile-row window leaves rows untouched
    const bool zero = P == 0 || setting_present(settings, "_tile_rows");
    torch::Tensor out_color = zero ? torch::zeros({3, H, W}, fopt) : torch::empty({3, H, W}, fopt);
    torch::Tensor radii = zero ? torch::zeros({P}, iopt) : torch::empty({P}, iopt);
    const bool bg_pixels = per_pixel_background(background, H, W);
    if (alpha || bg_pixels) require(g_api.set_forward_background, "alpha / background");
    torch::Tensor out_alpha; // (like the image: every pixel of the rendered tile rows is written)
    if (alpha) out_alpha = zero ? torch::zeros({1, H, W}, fopt) : torch::empty({1, H, W}, fopt);
    if (invdepth) {
        require(g_api.set_forward_invdepth, "invdepth");
        if (render_depth) throw std::runtime_error("the inverse-depth output is not available with render_depth (the debug depth visualisation)");
    }
    torch::Tensor out_invdepth; // (like the image: every pixel of the rendered tile rows is written)
    if (invdepth) out_invdepth = zero ? torch::zeros({1, H, W}, fopt) : torch::empty({1, H, W}, fopt);
    // The SH stash (include/stp_raster.h: stp_set_forward_sh_stash) is asked for exactly when a backward can follow -- the autograd layer's
    // condition for asking for the blend log, settings._record_blend_log, or, where its policy or the sort mode rules the log out, its
    // settings._sh_stash -- and the library exports the request; settings._no_sh_stash = True keeps a differentiable forward on the legacy
    // path (tests compare the two).  An inference forward asks for nothing.
    const bool sh_stash = (setting_flag(settings, "_record_blend_log") || setting_flag(settings, "_sh_stash")) && !setting_flag(settings, "_no_sh_stash") &&
                          !render_depth && g_api.set_forward_sh_stash != nullptr;
    Resizer geom{torch::empty({0}, bopt), false, false, 0}, binning{torch::empty({0}, bopt), true, false, 1}, img{torch::empty({0}, bopt), true, false, 2};
    int rendered = 0;
    if (P != 0) {
        const int M = split ? M_split : sh.numel() != 0 ? (int)sh.size(1) : 0;
        StpSettings s = settings_from_dict(settings, record_log);
        if (render_depth) { // DebugVisualization::Depth (reference rasterize_points.cu:104-107); no log: it has no backward
            s.debug_visualization = STP_DEBUG_DEPTH;
            s.record_blend_log = 0;
        }
        const FrameInputs in = prep_frame(dev, background, means3D, sh, colors, opacity, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
                                          inv_viewprojmatrix, campos);
        torch::Tensor dc_;
        if (split) dc_ = prep(*dc, dev);
        const c10::hip::HIPGuard guard(dev.index());
        void* const stream = current_stream(dev);
        int rc;
        {
            py::gil_scoped_release nogil; // (the call blocks once, on the num_rendered hand-over)
            if (alpha || bg_pixels) // (consumed by the call below, on this thread)
                g_api.set_forward_background(bg_pixels ? fptr(in.bg) : nullptr, alpha ? out_alpha.data_ptr<float>() : nullptr);
            if (invdepth) g_api.set_forward_invdepth(out_invdepth.data_ptr<float>());
            if (split) g_api.set_forward_split_sh(dc_.data_ptr<float>());
            if (sh_stash) g_api.set_forward_sh_stash(1);
            if (raw != 0) g_api.set_forward_raw_params(raw);
            rc = g_api.forward(&Resizer::call, &geom, &Resizer::call, &binning, &Resizer::call, &img, P, degree, M, fptr(in.bg), W, H, &s, fptr(in.m3),
                               fptr(in.sh), fptr(in.col), fptr(in.op), fptr(in.sc), scale_modifier, fptr(in.ro), fptr(in.c3), fptr(in.vm), fptr(in.pm),
                               fptr(in.inv), fptr(in.cam), tan_fovx, tan_fovy, prefiltered ? 1 : 0, out_color.data_ptr<float>(), radii.data_ptr<int>(),
                               debug ? 1 : 0, stream);
        }
        rendered = checked(rc);
        remember_storage(geom.t);
        remember_storage(binning.t);
        remember_storage(img.t);
    }
    return std::make_tuple(rendered, out_color, radii, geom.t, binning.t, img.t, out_alpha, out_invdepth);
}

// == RasterizeGaussiansBackwardCUDA (reference rasterize_points.cu:140-232).
// phases / partial: extension for tile-row sharding (include/stp_raster.h, stp_backward_phases): phases = 1 runs only the
// render half and returns the (P,16) gradient records; phases = 2 takes the records (after the caller's all-reduce) and
// runs the per-Gaussian half.
// camera_grads (extension, include/stp_raster.h: stp_set_backward_camera_grads): the per-Gaussian half also returns dL/dviewmatrix,
// dL/dprojmatrix and dL/dcampos, appended to the eight gradients in the shapes of the three inputs.
// absgrad (extension, include/stp_raster.h: stp_set_backward_absgrad): one more (P,3) tensor, LAST in the result: the per-Gaussian sums over
// pixels of |each pixel's contribution to dL/dmeans2D| (x, y; column 2 zero).  Whole backwards on padded records only.
// blend_stats (extension, include/stp_raster.h: stp_set_backward_blend_stats): one more (P,3) tensor, behind absgrad's if both are asked
// for: per Gaussian the sum, the maximum and the count of its blend weights alpha * T.  Whole backwards on padded records only.
// dL_dalpha / bg_grad (extension, include/stp_raster.h: stp_set_backward_background): the gradient of the forward's alpha output (1,H,W), and one
// more tensor, LAST in the result: dL/dbackground in the background's shape, (3,) or (3,H,W).  A background of shape exactly (3,H,W) is
// the forward's per-pixel one.  Calls with the render half (phases bit 0).
// dL_dinvdepth / invdepth (extension, include/stp_raster.h: stp_set_backward_invdepth): the gradient of the forward's inverse-depth output and
// that output itself, both (1,H,W).  No extra result: the gradient arrives in the eight (and the camera's three).  Whole backwards on padded
// records only.
// dc (keyword, extension, include/stp_raster.h: stp_set_backward_split_sh): the first SH coefficient, (P,1,3) or (P,3); `sh` is then the (P,M-1,3)
// rest.  dL_dsh, in its usual slot, is (P,M-1,3), and dL_ddc, (P,3), is the LAST tensor of the result.  The full order of the result is
//   [the eight] [dL_dview, dL_dproj, dL_dcam] [absgrad] [blend_stats] [dL_dbackground] [dL_ddc]
// raw (keyword, extension, include/stp_raster.h: stp_set_backward_raw_params): the forward's mask; dL_dopacity, dL_dscales and dL_drotations of the
// mask's bits are then the gradients with respect to the raw values.  Calls with the per-Gaussian half (phases bit 1), every chunk of a chunked one.
// each bracket present when asked for.  Calls with the per-Gaussian half (phases bit 1); with `outputs` (a later chunk) a ninth tensor in it is
// the dL_ddc of the first chunk.  Ignored with precomputed colours.
std::vector<torch::Tensor>
rasterize_gaussians_backward(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& radii, const torch::Tensor& opacities,
                             const torch::Tensor& colors, const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier,
                             const torch::Tensor& cov3D_precomp, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix,
                             const torch::Tensor& inv_viewprojmatrix, const float tan_fovx, const float tan_fovy, const torch::Tensor& pixel_colors,
                             const torch::Tensor& dL_dout_color, const torch::Tensor& sh, const int degree, const torch::Tensor& campos,
                             const torch::Tensor& geomBuffer, const int R, const torch::Tensor& binningBuffer, const torch::Tensor& imageBuffer,
                             const py::dict& settings, const bool debug, const bool record_log, const int phases, const c10::optional<torch::Tensor>& partial,
                             const c10::optional<std::vector<torch::Tensor>>& outputs, const bool camera_grads, const bool absgrad, const bool blend_stats,
                             const c10::optional<torch::Tensor>& dL_dalpha, const bool bg_grad,
                             const c10::optional<torch::Tensor>& dL_dinvdepth, const c10::optional<torch::Tensor>& invdepth,
                             const c10::optional<torch::Tensor>& dc, const int raw_mask)
{
    need_library();
    TORCH_CHECK(means3D.is_cuda(), GPU_ONLY);
    const int raw = (phases & 2) ? raw_mask : 0; // (the render half reads none of the three arrays)
    if (raw != 0) require(g_api.set_backward_raw_params, "raw");
    const bool split = dc.has_value() && dc->defined() && colors.numel() == 0 && (phases & 2); // (precomputed colours win; the render half reads no SH)
    if (split) require(g_api.set_backward_split_sh, "dc");
    const int M_split = split ? split_sh_total(*dc, sh, means3D) : 0;
    if (camera_grads) {
        require(g_api.set_backward_camera_grads, "camera gradients");
        require(g_api.camera_grad_workspace_bytes, "camera gradients");
        TORCH_CHECK(phases & 2, "camera gradients come from the per-Gaussian half (phases bit 1)");
    }
    if (absgrad) {
        require(g_api.set_backward_absgrad, "absgrad");
        // (the render half leaves the two sums in the records it has just filled and the per-Gaussian half of the SAME call collects them: a
        // half on its own would need the caller to carry request and records from one call to the other)
        TORCH_CHECK((phases & 3) == 3, "absgrad needs both halves of the backward in one call (phases bits 0 and 1)");
    }
    if (blend_stats) {
        require(g_api.set_backward_blend_stats, "blend_stats");
        TORCH_CHECK((phases & 3) == 3, "blend_stats needs both halves of the backward in one call (phases bits 0 and 1)");
    }
    const torch::Device dev = means3D.device();
    const int P = (int)means3D.size(0);
    const int H = (int)dL_dout_color.size(1), W = (int)dL_dout_color.size(2);
    const bool bg_pixels = per_pixel_background(background, H, W);
    const bool have_dalpha = dL_dalpha.has_value() && dL_dalpha->defined();
    if (bg_pixels || have_dalpha || bg_grad) {
        require(g_api.set_backward_background, "alpha / background");
        TORCH_CHECK(phases & 1, "alpha gradient / per-pixel background / background gradient belong to the render half (phases bit 0)");
        TORCH_CHECK(!have_dalpha || dL_dalpha->numel() == (int64_t)H * W, "dL_dalpha must have H * W elements");
    }
    const bool have_dinv = dL_dinvdepth.has_value() && dL_dinvdepth->defined();
    if (have_dinv) {
        require(g_api.set_backward_invdepth, "invdepth");
        TORCH_CHECK((phases & 3) == 3, "the inverse-depth gradient needs both halves of the backward in one call (phases bits 0 and 1)");
        TORCH_CHECK(invdepth.has_value() && invdepth->defined(), "dL_dinvdepth needs the forward's invdepth");
        TORCH_CHECK(dL_dinvdepth->numel() == (int64_t)H * W && invdepth->numel() == (int64_t)H * W, "dL_dinvdepth and invdepth must have H * W elements");
    }
    const int M = split ? M_split : sh.numel() != 0 ? (int)sh.size(1) : 0;
    const auto fopt = means3D.options().dtype(torch::kFloat32);
    const int rec_floats = (phases & 4) ? STP_GRAD_RECORD_USED : STP_GRAD_RECORD_FLOATS; // (bit 2: compact records, the tile-row shard's wire format)
    const torch::Tensor records = partial.has_value() ? *partial : torch::zeros({P, rec_floats}, fopt);
    TORCH_CHECK(records.dim() == 2 && records.size(0) == P && records.size(1) == rec_floats && records.scalar_type() == torch::kFloat32 &&
                    records.is_contiguous(), "partial must be a contiguous float32 (P,", rec_floats, ") tensor");
    torch::Tensor dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations, dL_ddc;
    if ((phases & 2) && outputs.has_value()) {
        // a chunked per-Gaussian half (phases bits 8-23): the later chunks write into the tensors the first one allocated
        TORCH_CHECK(outputs->size() == (split ? 9u : 8u), "outputs: the eight gradient tensors of an earlier chunk (and its dL_ddc behind them with dc)");
        if (split) {
            dL_ddc = (*outputs)[8];
            TORCH_CHECK(dL_ddc.scalar_type() == torch::kFloat32 && dL_ddc.is_contiguous() && dL_ddc.numel() == (int64_t)P * 3 &&
                            (*outputs)[5].is_contiguous() && (*outputs)[5].numel() == (int64_t)P * (M - 1) * 3,
                        "outputs: dL_dsh must be a contiguous (P,M-1,3) and dL_ddc a contiguous (P,3) float32 tensor with dc");
        }
        dL_dmeans2D = (*outputs)[0]; dL_dcolors = (*outputs)[1]; dL_dopacity = (*outputs)[2]; dL_dmeans3D = (*outputs)[3];
        dL_dcov3D = (*outputs)[4]; dL_dsh = (*outputs)[5]; dL_dscales = (*outputs)[6]; dL_drotations = (*outputs)[7];
    } else if (phases & 2) {
        // the per-Gaussian half writes every row of its outputs (zeros for invisible Gaussians): no zero-fill needed,
        // except for the scale/rotation gradients when a precomputed covariance is used (then they are not touched)
        // settings._no_grad_colors / _no_grad_cov3D (set by the autograd layer where colors_precomp / cov3D_precomp are absent): nobody receives
        // that gradient, so it is neither allocated nor written (include/stp_raster.h: optional outputs) and its slot of the result is None.
        // A direct caller without the keys gets all eight, written in full.
        const bool have_scales = scales.numel() != 0, may_omit = g_api.set_forward_sh_stash != nullptr;
        const bool no_dcolors = may_omit && setting_flag(settings, "_no_grad_colors") && colors.numel() == 0;
        const bool no_dcov3D = may_omit && setting_flag(settings, "_no_grad_cov3D") && cov3D_precomp.numel() == 0;
        dL_dmeans2D = torch::empty({P, 3}, fopt); if (!no_dcolors) dL_dcolors = torch::empty({P, 3}, fopt); dL_dopacity = torch::empty({P, 1}, fopt);
        dL_dmeans3D = torch::empty({P, 3}, fopt); if (!no_dcov3D) dL_dcov3D = torch::empty({P, 6}, fopt); dL_dsh = torch::empty({P, split ? M - 1 : M, 3}, fopt);
        if (split) dL_ddc = torch::empty({P, 3}, fopt); // (written in full by the library, like dL_dsh)
        dL_dscales = have_scales ? torch::empty({P, 3}, fopt) : torch::zeros({P, 3}, fopt);
        dL_drotations = have_scales ? torch::empty({P, 4}, fopt) : torch::zeros({P, 4}, fopt);
    }
    const StpSettings s = settings_from_dict(settings, record_log);
    torch::Tensor dL_dview, dL_dproj, dL_dcam, cam_ws;
    if (camera_grads) { // written in full by the library (no zero-fill); the workspace holds one row per 256 Gaussians and the partial sums
        dL_dview = torch::empty(viewmatrix.sizes(), fopt); dL_dproj = torch::empty(projmatrix.sizes(), fopt); dL_dcam = torch::empty(campos.sizes(), fopt);
        TORCH_CHECK(dL_dview.numel() == 16 && dL_dproj.numel() == 16 && dL_dcam.numel() == 3, "camera gradients: viewmatrix and projmatrix must have 16 elements, campos 3");
        cam_ws = torch::empty({(int64_t)g_api.camera_grad_workspace_bytes(P)}, means3D.options().dtype(torch::kByte));
    }
    torch::Tensor dL_dmeans2D_abs, stats;
    if (absgrad) dL_dmeans2D_abs = torch::empty({P, 3}, fopt); // written in full by the library (zeros for invisible Gaussians)
    if (blend_stats) stats = torch::empty({P, 3}, fopt); // written in full by the library (zeros for invisible Gaussians)
    torch::Tensor dL_dbg, dal_, bgpix_;
    if (bg_grad) { // written in full by the library, except where nothing runs (P == 0) or a tile-row window leaves rows untouched
        const std::vector<int64_t> shape = bg_pixels ? std::vector<int64_t>{3, H, W} : std::vector<int64_t>{3};
        dL_dbg = (P == 0 || (bg_pixels && setting_present(settings, "_tile_rows"))) ? torch::zeros(shape, fopt) : torch::empty(shape, fopt);
    }
    if (have_dalpha) dal_ = prep(*dL_dalpha, dev);
    if (bg_pixels) bgpix_ = prep(background, dev);
    torch::Tensor dinv_, inv_out_;
    if (have_dinv) { dinv_ = prep(*dL_dinvdepth, dev); inv_out_ = prep(*invdepth, dev); }
    torch::Tensor dc_;
    if (split && P != 0) dc_ = prep(*dc, dev);
    auto make_requests = [&] { // (all are consumed by the library call that follows, on this thread)
        if ((bg_pixels || have_dalpha || bg_grad) && P != 0)
            g_api.set_backward_background(bg_pixels ? bgpix_.data_ptr<float>() : nullptr, have_dalpha ? dal_.data_ptr<float>() : nullptr,
                                          bg_grad ? dL_dbg.data_ptr<float>() : nullptr);
        if (have_dinv && P != 0) g_api.set_backward_invdepth(inv_out_.data_ptr<float>(), dinv_.data_ptr<float>());
        if (split && P != 0) g_api.set_backward_split_sh(dc_.data_ptr<float>(), dL_ddc.data_ptr<float>());
        if (raw != 0 && P != 0) g_api.set_backward_raw_params(raw);
        if (blend_stats && P != 0) g_api.set_backward_blend_stats(stats.data_ptr<float>());
        if (absgrad && P != 0) g_api.set_backward_absgrad(dL_dmeans2D_abs.data_ptr<float>());
        if (camera_grads) g_api.set_backward_camera_grads(dL_dview.data_ptr<float>(), dL_dproj.data_ptr<float>(), dL_dcam.data_ptr<float>(), cam_ws.data_ptr(), (size_t)cam_ws.numel());
    };
    if (P == 0 && camera_grads) { // nothing to differentiate: the library writes the zeros
        const c10::hip::HIPGuard guard(dev.index());
        void* const stream = current_stream(dev);
        make_requests();
        checked(g_api.backward_phases(phases, 0, degree, M, R, nullptr, W, H, &s, nullptr, nullptr, nullptr, nullptr, nullptr, scale_modifier, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, tan_fovx, tan_fovy, nullptr, nullptr, nullptr, nullptr, nullptr,
                                      nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, debug ? 1 : 0, stream));
    }
    if (P != 0) {
        const FrameInputs in = prep_frame(dev, background, means3D, sh, colors, opacities, scales, rotations, cov3D_precomp, viewmatrix, projmatrix,
                                          inv_viewprojmatrix, campos);
        const torch::Tensor pix_ = prep(pixel_colors, dev), dl_ = prep(dL_dout_color, dev);
        const torch::Tensor radii_ = radii.contiguous();
        auto optf = [](const torch::Tensor& t) -> float* { return t.defined() && t.numel() != 0 ? t.data_ptr<float>() : nullptr; };
        auto optb = [](const torch::Tensor& t) -> char* { return t.defined() && t.numel() != 0 ? reinterpret_cast<char*>(t.data_ptr()) : nullptr; };
        const c10::hip::HIPGuard guard(dev.index());
        void* const stream = current_stream(dev);
        forget_unless_same_storage(geomBuffer); // (whether it carries an SH stash)
        forget_unless_same_storage(binningBuffer); // (a clone, a copy or a recycled address: the library then reads the buffer's own header)
        forget_unless_same_storage(imageBuffer);
        make_requests(); // (consumed by the call below, on this thread)
        checked(g_api.backward_phases(phases, P, degree, M, R, fptr(in.bg), W, H, &s, fptr(in.m3), fptr(in.sh), fptr(in.op), fptr(in.col), fptr(in.sc),
                                      scale_modifier, fptr(in.ro), fptr(in.c3), fptr(in.vm), fptr(in.pm), fptr(in.inv), fptr(in.cam), tan_fovx, tan_fovy,
                                      fptr(pix_), radii_.numel() ? radii_.data_ptr<int>() : nullptr, optb(geomBuffer), optb(binningBuffer),
                                      optb(imageBuffer), fptr(dl_), optf(dL_dmeans2D), records.data_ptr<float>(), optf(dL_dopacity), optf(dL_dcolors),
                                      optf(dL_dmeans3D), optf(dL_dcov3D), optf(dL_dsh), optf(dL_dscales), optf(dL_drotations), debug ? 1 : 0, stream));
    }
    if ((phases & 3) == 1) { if (bg_grad) return {records, dL_dbg}; return {records}; }
    std::vector<torch::Tensor> result{dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations};
    if (camera_grads) result.insert(result.end(), {dL_dview, dL_dproj, dL_dcam});
    if (absgrad) result.push_back(dL_dmeans2D_abs);
    if (blend_stats) result.push_back(stats);
    if (bg_grad) result.push_back(dL_dbg);
    if (split) result.push_back(dL_ddc);
    return result;
}

// == markVisible (reference rasterize_points.cu:234-253)
torch::Tensor mark_visible(const torch::Tensor& means3D, const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix)
{
    need_library();
    TORCH_CHECK(means3D.is_cuda(), GPU_ONLY);
    const torch::Device dev = means3D.device();
    const int P = (int)means3D.size(0);
    torch::Tensor present = torch::zeros({P}, means3D.options().dtype(torch::kBool));
    if (P != 0) {
        const torch::Tensor m3_ = prep(means3D, dev), vm_ = prep(viewmatrix, dev), pm_ = prep(projmatrix, dev);
        const c10::hip::HIPGuard guard(dev.index());
        checked(g_api.mark_visible(P, fptr(m3_), fptr(vm_), fptr(pm_), reinterpret_cast<uint8_t*>(present.data_ptr()), current_stream(dev)));
    }
    return present;
}
} // namespace
