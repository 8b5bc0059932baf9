// stp_api.hip -- the C ABI of libstp_raster.so (declared in include/stp_raster.h): the per-thread error state, the argument checks
// and frame description that forward and backward share, the one-shot per-thread requests, and the backward, mark-visible, sparse
// Adam, 3DGS-MCMC, nearest-neighbour, densification and photometric-loss calls.  Replaces CudaRasterizer::Rasterizer::{backward,markVisible} (reference cuda_rasterizer/rasterizer_impl.cu:417-526,
// 161-173).  The forward is stp_forward.hip, the scratch buffers and their queries stp_buffers.hip, the stage timer stp_timer.hip.
//
// The calls are re-entrant: the scratch buffers belong to the caller, stp_last_error and the requests are per thread, and the
// per-device helpers are created once behind a lock (here: the background-gradient scratch ring).
#include "stp_internal.h"

#include <cmath>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace stp {

static thread_local std::string g_last_error; // (the ONE error message of the thread: every file sets it through fail)

int fail(int code, const std::string& msg) { g_last_error = msg; return code; }
int fail_hip(hipError_t e, const char* what) { return fail(STP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

int check_settings(const StpSettings& s, bool backward)
{
    if (s.sort_mode < MODE_GLOBAL || s.sort_mode > MODE_HIER) return fail(STP_ERR_SORT_MODE, "invalid sort mode");
    if (s.sort_order < ORDER_Z || s.sort_order > ORDER_PTD_MAX) return fail(STP_ERR_SORT_MODE, "invalid sort order");
    if (backward && s.sort_mode == MODE_FULL) return fail(STP_ERR_NO_BACKWARD, "Backward not supported for full per-pixel sort");
    if (s.sort_mode == MODE_HIER) {
        const int h = s.queue_per_pixel, m = s.queue_tile_2x2;
        if (!(m == 8 || m == 12 || m == 20)) return fail(STP_ERR_QUEUE_SIZE, "Not supported mid queue size");
        const bool head_ok = backward ? (h == 4 || h == 8 || h == 12 || h == 16) : (h == 4 || h == 8 || h == 16);
        if (!head_ok) return fail(STP_ERR_QUEUE_SIZE, "Not supported head queue size");
    }
    return 0;
}

void fill_frame(FrameParams& f, int P, int D, int M, const float* background, int width, int height, const StpSettings& s,
                const float* means3D, const float* shs, const float* colors_precomp, const float* opacities,
                const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                const float* viewmatrix, const float* projmatrix, const float* inv_viewprojmatrix, const float* cam_pos,
                float tan_fovx, float tan_fovy, int prefiltered)
{
    f.P = P; f.D = D; f.M = M; f.W = width; f.H = height;
    f.gx = (width + TILE - 1) / TILE; f.gy = (height + TILE - 1) / TILE;
    f.ty0 = s.tile_y0; f.ty1 = s.tile_y1;
    clamp_tile_rows(height, f.ty0, f.ty1);
    f.focal_y = (float)height / (2.0f * tan_fovy); // reference rasterizer_impl.cu:251-252
    f.focal_x = (float)width / (2.0f * tan_fovx);
    f.tan_fovx = tan_fovx; f.tan_fovy = tan_fovy; f.scale_modifier = scale_modifier; f.s = s;
    f.background = background; f.means3D = means3D; f.shs = shs; f.colors_precomp = colors_precomp; f.opacities = opacities;
    f.scales = scales; f.rotations = rotations; f.cov3D_precomp = cov3D_precomp; f.viewmatrix = viewmatrix; f.projmatrix = projmatrix;
    f.inv_viewprojmatrix = inv_viewprojmatrix; f.cam_pos = cam_pos; f.prefiltered = prefiltered;
    f.wild_cov = 1; // (until the forward has read the status word: the kernels with the domain check)
    f.log_depth = 0; f.log_need = nullptr; f.log_tag = 0;
}

// stp_set_forward_raw_params / stp_set_backward_raw_params: the mask against the arrays of the call that took it
int check_raw_params(int mask, const float* opacities, const float* scales, const float* rotations)
{
    if (mask < 0 || mask > 7) return fail(STP_ERR_INVALID_ARGUMENT, "raw parameters: mask " + std::to_string(mask) + " is outside 0..7 (bit 0 opacities, bit 1 scales, bit 2 rotations)");
    if ((mask & 1) && !opacities) return fail(STP_ERR_INVALID_ARGUMENT, "raw parameters: bit 0 (opacities) is set but opacities is NULL");
    if ((mask & 2) && !scales) return fail(STP_ERR_INVALID_ARGUMENT, "raw parameters: bit 1 (scales) is set but scales is NULL");
    if ((mask & 4) && !rotations) return fail(STP_ERR_INVALID_ARGUMENT, "raw parameters: bit 2 (rotations) is set but rotations is NULL");
    return 0;
}

// ---- the one-shot requests of the calling thread: set by the stp_set_* calls below, each taken by the next call it is meant for.  ALL of
// ---- them live in this one struct, and the two functions below are the only ones that take them.
struct BackwardBackground { const float* bg_image = nullptr; const float* dL_dalpha = nullptr; float* dL_dbackground = nullptr; }; // stp_set_backward_background
struct BackwardInvdepth { const float* invdepth = nullptr; const float* dL_dinvdepth = nullptr; }; // stp_set_backward_invdepth
struct BackwardSplitSh { const float* dc = nullptr; float* dL_ddc = nullptr; }; // stp_set_backward_split_sh
struct BackwardRequests { CameraGradRequest cam; float* absgrad = nullptr; float* blend_stats = nullptr; BackwardBackground background; BackwardInvdepth invdepth; BackwardSplitSh split_sh; int raw_params = 0; /* stp_set_backward_raw_params */ };
struct PendingRequests { ForwardRequests forward; BackwardRequests backward; };
static thread_local PendingRequests t_pending;

// What a forward takes: the forward split and the forward background are consumed by the next stp_forward of the thread, whatever its
// outcome.  stp_forward calls this in front of its very first check, so a call refused there has consumed them too.
ForwardRequests take_forward_requests() { return std::exchange(t_pending.forward, ForwardRequests{}); }
// What a backward with these `phases` takes; what it does not take stays pending.
//   camera gradients, split SH and raw parameters: consumed by the next backward that runs the per-Gaussian half (phases bit 1), whatever its outcome.  A call without
//       bit 1 leaves them pending.
//   backward background: consumed by the next backward that runs the render half (phases bit 0), whatever its outcome.  A call without
//       bit 0 leaves it pending (nothing of it lives in the gradient records).
//   absgrad, blend statistics and inverse depth: taken by EVERY backward, and BOTH before either one's checks, so a call that is refused for one leaves
//       neither behind.  stp_backward_phases puts them back (keep_for_per_gaussian_call) only at the end of a render-only call
//       (!(phases & 2)) that ran to its end: the sums are in the records then, and the per-Gaussian call collects them.  A call that
//       fails, or has nothing to do, leaves no pointer behind.
static BackwardRequests take_backward_requests(int phases)
{
    BackwardRequests& p = t_pending.backward;
    BackwardRequests r;
    if (phases & 2) { r.cam = std::exchange(p.cam, CameraGradRequest{}); r.split_sh = std::exchange(p.split_sh, BackwardSplitSh{}); r.raw_params = std::exchange(p.raw_params, 0); }
    r.absgrad = std::exchange(p.absgrad, nullptr); r.blend_stats = std::exchange(p.blend_stats, nullptr);
    r.invdepth = std::exchange(p.invdepth, BackwardInvdepth{});
    if (phases & 1) r.background = std::exchange(p.background, BackwardBackground{});
    return r;
}
static void keep_for_per_gaussian_call(const BackwardRequests& r)
{
    t_pending.backward.absgrad = r.absgrad; t_pending.backward.blend_stats = r.blend_stats; t_pending.backward.invdepth = r.invdepth;
}

// ---- what the calls with a caller's scratch and the calls with a table of row tensors (StpMcmcTensor, StpDensifyTensor) share: 0 = fine,
// ---- negative = refused
// a scratch (not null: the caller's check) of `bytes` bytes against what size_fn(P) returned and the alignment the kernels read it with
static int check_scratch(const char* who, const void* scratch, size_t bytes, size_t need, unsigned align, const char* size_fn)
{
    if (bytes < need)
        return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": scratch of " + std::to_string(bytes) + " bytes, " + size_fn + "(P) = " + std::to_string(need));
    if (reinterpret_cast<uintptr_t>(scratch) & (align - 1u)) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": scratch is not " + std::to_string(align) + "-byte aligned");
    return 0;
}

// The roles of a table's entries: role 0 is a plain tensor of any width, role r in [1, n] is named name[r] in the messages and has row[r]
// floats per row.  together == nullptr (3DGS-MCMC): a wrong width is refused at its tensor, and a role that is not there exactly once by its
// name; otherwise (densification) `together` is the one sentence that refuses either, and only where the roles are required.
struct RowRoles {
    int n;
    const char* const* name;
    const int* row;
    const char* known;    // the list behind "unknown role"
    const char* rows;     // what the bound rows * row < 2^31 calls its rows
    const char* together;
};

// The entry table of an apply that is flattened over `rows` rows.  in_place: the *_out pointers are not looked at; work: the call will launch
// (pointers must be there); required: exactly one entry of each of the roles 1 .. n.
template <class Entry>
static int check_row_tensors(const char* who, int n_tensors, const Entry* tensors, long long rows, const RowRoles& roles, bool in_place, bool work, bool required)
{
    if (n_tensors < 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative n_tensors");
    if (n_tensors > 64) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": " + std::to_string(n_tensors) + " tensors, at most 64 in one call");
    if (n_tensors > 0 && !tensors) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null tensor table");
    int of_role[4] = {0, 0, 0, 0}; // (n <= 3)
    bool rows_fit = true;
    for (int k = 0; k < n_tensors; k++) {
        const Entry& t = tensors[k];
        const std::string which = std::string(who) + ": tensor " + std::to_string(k);
        if (t.row <= 0) return fail(STP_ERR_INVALID_ARGUMENT, which + ": row " + std::to_string(t.row) + " <= 0");
        if (rows * t.row >= (1ll << 31)) return fail(STP_ERR_INVALID_ARGUMENT, which + ": " + roles.rows + " * row = " + std::to_string(rows * t.row) + " >= 2^31");
        if (t.role < 0 || t.role > roles.n) return fail(STP_ERR_INVALID_ARGUMENT, which + ": unknown role " + std::to_string(t.role) + " " + roles.known);
        if (t.role != 0 && t.row != roles.row[t.role]) {
            if (!roles.together)
                return fail(STP_ERR_INVALID_ARGUMENT, which + ": role " + std::to_string(t.role) + " needs row " + std::to_string(roles.row[t.role]) + ", got " + std::to_string(t.row));
            rows_fit = false;
        }
        if ((t.exp_avg == nullptr) != (t.exp_avg_sq == nullptr)) return fail(STP_ERR_INVALID_ARGUMENT, which + ": exp_avg and exp_avg_sq must both be given or both be null");
        of_role[t.role]++;
        if (work) {
            if (!t.param || (!in_place && !t.param_out)) return fail(STP_ERR_INVALID_ARGUMENT, which + ": null pointer");
            if (!in_place && t.exp_avg && (!t.exp_avg_out || !t.exp_avg_sq_out)) return fail(STP_ERR_INVALID_ARGUMENT, which + ": null pointer (moment output)");
        }
    }
    if (!required) return 0;
    for (int role = 1; role <= roles.n; role++) {
        if (roles.together) {
            if (of_role[role] != 1 || !rows_fit) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": " + roles.together);
            continue;
        }
        if (of_role[role] == 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": missing role " + roles.name[role] + ": exactly one tensor must have it");
        if (of_role[role] > 1) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": duplicated role " + roles.name[role] + ": exactly one tensor must have it");
    }
    return 0;
}

} // namespace stp

using namespace stp;

extern "C" {

int stp_abi_version(void) { return STP_ABI_VERSION; }
const char* stp_last_error(void) { return g_last_error.c_str(); }

// the setters of the one-shot requests (the rules: take_forward_requests / take_backward_requests)
void stp_set_forward_split(int tile_row, void* event) { t_pending.forward.split = ForwardSplit{tile_row, (hipEvent_t)event, event != nullptr}; }
void stp_set_forward_background(const float* bg_image, float* out_alpha) { t_pending.forward.background = ForwardBackground{bg_image, out_alpha}; }
size_t stp_camera_grad_workspace_bytes(int P) { return camera_grad_workspace_bytes(P); }
void stp_set_backward_camera_grads(float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, void* workspace, size_t workspace_bytes)
{
    t_pending.backward.cam = CameraGradRequest{};
    if (!dL_dviewmatrix || !dL_dprojmatrix || !dL_dcampos) return; // (clears a pending request)
    t_pending.backward.cam = CameraGradRequest{dL_dviewmatrix, dL_dprojmatrix, dL_dcampos, workspace, workspace_bytes};
}
void stp_set_backward_absgrad(float* dL_dmean2D_abs) { t_pending.backward.absgrad = dL_dmean2D_abs; }
void stp_set_backward_blend_stats(float* blend_stats) { t_pending.backward.blend_stats = blend_stats; }
void stp_set_backward_background(const float* bg_image, const float* dL_dalpha, float* dL_dbackground) { t_pending.backward.background = BackwardBackground{bg_image, dL_dalpha, dL_dbackground}; }
void stp_set_forward_invdepth(float* out_invdepth) { t_pending.forward.out_invdepth = out_invdepth; }
void stp_set_backward_invdepth(const float* invdepth, const float* dL_dinvdepth) { t_pending.backward.invdepth = BackwardInvdepth{invdepth, dL_dinvdepth}; }
void stp_set_forward_split_sh(const float* dc) { t_pending.forward.sh_dc = dc; }
void stp_set_forward_sh_stash(int enable) { t_pending.forward.sh_stash = enable != 0; }
void stp_set_backward_split_sh(const float* dc, float* dL_ddc) { t_pending.backward.split_sh = dc ? BackwardSplitSh{dc, dL_ddc} : BackwardSplitSh{}; }
void stp_set_forward_raw_params(int mask) { t_pending.forward.raw_params = mask; }
void stp_set_backward_raw_params(int mask) { t_pending.backward.raw_params = mask; }

namespace {
// Scratch of the uniform background gradient's two-stage sum (stp_background.hip): a small ring of partial-row buffers per device, made at the
// first request like the mailboxes, each with an event recorded behind the kernels that used it last.  A request takes the next slot and
// orders its stream behind that event, so a slot is never written while an earlier user's sum kernel can still read it -- however many
// threads and streams run backwards on the device.  The ring only keeps concurrent streams from waiting for each other in the common case.
// g_background_mutex is held from taking a slot to recording its event (launches only: microseconds).
constexpr int BG_RING = 8;
struct BackgroundSlot { float* partials = nullptr; hipEvent_t done = nullptr; bool used = false; };
struct BackgroundScratch { BackgroundSlot slot[BG_RING]; unsigned next = 0; bool ready = false; };
BackgroundScratch g_background_scratch[MAX_DEVICES];
std::mutex g_background_mutex;
int acquire_background_scratch(BackgroundSlot** out, hipStream_t st) // caller holds g_background_mutex
{
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess || device < 0 || device >= MAX_DEVICES) return fail(STP_ERR_HIP, "hipGetDevice failed");
    BackgroundScratch& r = g_background_scratch[device];
    if (!r.ready) {
        const size_t bytes = background_grad_partials() * sizeof(float);
        char* base = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&base), bytes * BG_RING) != hipSuccess) return fail(STP_ERR_HIP, "cannot create the background-gradient scratch");
        for (int i = 0; i < BG_RING; i++) {
            r.slot[i].partials = reinterpret_cast<float*>(base + bytes * i);
            if (hipEventCreateWithFlags(&r.slot[i].done, hipEventDisableTiming) != hipSuccess) { (void)hipFree(base); return fail(STP_ERR_HIP, "cannot create the background-gradient scratch"); }
        }
        r.ready = true;
    }
    BackgroundSlot& s = r.slot[r.next++ % BG_RING];
    if (s.used) STP_TRY(hipStreamWaitEvent(st, s.done, 0), "wait for the background-gradient scratch");
    *out = &s;
    return 0;
}
} // namespace

int stp_backward_phases(int phases, int P, int D, int M, int R, const float* background, int width, int height, const StpSettings* settings,
                 const float* means3D, const float* shs, const float* opacities, const float* colors_precomp, const float* scales,
                 float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* inv_viewprojmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                 const float* pixel_colors, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                 const float* dL_dpix, float* dL_dmean2D, float* grad_records, float* dL_dopacity, float* dL_dcolor,
                 float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int debug, void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    const BackwardRequests req = take_backward_requests(phases);
    const CameraGradRequest& cam = req.cam;
    float* const absgrad = req.absgrad;
    float* const blend_stats = req.blend_stats;
    const BackwardBackground& bbg = req.background;
    if (absgrad) {
        if (phases & 4)
            return fail(STP_ERR_INVALID_ARGUMENT, "absgrad is not available with compact gradient records (phases bit 2): the 36-byte record has no room for the two extra sums");
        if (((phases >> 8) & 0xFF) > 1)
            return fail(STP_ERR_INVALID_ARGUMENT, "absgrad is not available from a chunked per-Gaussian half (phases bits 8-23)");
    }
    if (blend_stats) {
        if (phases & 4)
            return fail(STP_ERR_INVALID_ARGUMENT, "blend statistics are not available with compact gradient records (phases bit 2): the 36-byte record has no room for the three extra terms");
        if (((phases >> 8) & 0xFF) > 1)
            return fail(STP_ERR_INVALID_ARGUMENT, "blend statistics are not available from a chunked per-Gaussian half (phases bits 8-23)");
    }
    const BackwardInvdepth& binv = req.invdepth;
    if (binv.invdepth || binv.dL_dinvdepth) {
        if (!binv.invdepth || !binv.dL_dinvdepth)
            return fail(STP_ERR_INVALID_ARGUMENT, "inverse depth: the forward's invdepth and dL_dinvdepth must both be given");
        if (phases & 4)
            return fail(STP_ERR_INVALID_ARGUMENT, "the inverse-depth gradient is not available with compact gradient records (phases bit 2): the 36-byte record has no room for the extra sum");
        if (((phases >> 8) & 0xFF) > 1)
            return fail(STP_ERR_INVALID_ARGUMENT, "the inverse-depth gradient is not available from a chunked per-Gaussian half (phases bits 8-23)");
    }
    const BackwardSplitSh& bsh = req.split_sh;
    if (bsh.dc && colors_precomp) shs = nullptr; // precomputed colours win, as in the forward: no SH coefficient is read, neither SH gradient is written
    if (bsh.dc && !colors_precomp) {
        if (!bsh.dL_ddc) return fail(STP_ERR_INVALID_ARGUMENT, "split SH: dL_ddc must be given with dc");
        if (M > 1 && (!shs || !dL_dsh)) return fail(STP_ERR_INVALID_ARGUMENT, "split SH: M > 1 needs the rest of the coefficients (shs) and their gradient (dL_dsh)");
    }
    if (cam.dL_dview) {
        if (!cam.workspace || (reinterpret_cast<uintptr_t>(cam.workspace) & 15) != 0 || cam.workspace_bytes < camera_grad_workspace_bytes(P))
            return fail(STP_ERR_INVALID_ARGUMENT, "camera gradients: the workspace is null, not 16-byte aligned or smaller than stp_camera_grad_workspace_bytes(P)");
        if (((phases >> 8) & 0xFF) > 1)
            return fail(STP_ERR_INVALID_ARGUMENT, "camera gradients are not available from a chunked per-Gaussian half (phases bits 8-23)");
    }
    if (int rc = check_raw_params(req.raw_params, opacities, scales, rotations)) return rc;
    if (!settings) return fail(STP_ERR_INVALID_ARGUMENT, "null settings");
    if (P == 0) { // reference rasterize_points.cu:191 (a camera request still gets its outputs: zeros; so does a background gradient -- the forward left the caller's image alone)
        if (cam.dL_dview) STP_TRY(launch_camera_grad_finalize(0, cam, st), "camera gradient launch");
        if (bbg.dL_dbackground && (!bbg.bg_image || (width > 0 && height > 0)))
            STP_TRY(hipMemsetAsync(bbg.dL_dbackground, 0, sizeof(float) * 3 * (bbg.bg_image ? (size_t)width * (size_t)height : (size_t)1), st), "background gradient fill");
        return 0;
    }
    if (int rc = check_settings(*settings, true)) return rc;
    if (!geom_buffer || !image_buffer || (R > 0 && !binning_buffer)) return fail(STP_ERR_INVALID_ARGUMENT, "null scratch buffer");
    if (!grad_records) return fail(STP_ERR_INVALID_ARGUMENT, "null gradient record buffer");
    if ((phases & 1) && (!dL_dpix || !pixel_colors)) return fail(STP_ERR_INVALID_ARGUMENT, "null image gradient");
    // (dL_dcolor and dL_dcov3D may be NULL: outputs the caller has no receiver for -- colors_precomp / cov3D_precomp absent -- are then not written)
    if ((phases & 2) && (!dL_dmean2D || !dL_dopacity || !dL_dmean3D || !dL_dscale || !dL_drot))
        return fail(STP_ERR_INVALID_ARGUMENT, "null gradient buffer");

    FrameParams f;
    fill_frame(f, P, D, M, background, width, height, *settings, means3D, shs, colors_precomp, opacities, scales, scale_modifier,
               rotations, cov3D_precomp, viewmatrix, projmatrix, inv_viewprojmatrix, cam_pos, tan_fovx, tan_fovy, 0);
    const bool with_inv = requires_depth_along_ray(*settings);
    // an SH stash (stp_set_forward_sh_stash) is asked for only where the per-Gaussian half would read SH rows; a buffer without one: the legacy path
    bool with_stash = false;
    if ((phases & 2) && !colors_precomp && (shs || bsh.dc) && M > 0) { if (int rc = stash_of(geom_buffer, P, (int64_t)R, &with_stash, (hipStream_t)stream, true)) return rc; }
    float* sh_stash = nullptr;
    GeometryState g = carve_geometry(geom_buffer, (size_t)P, with_inv, nullptr, nullptr, nullptr, with_stash ? &sh_stash : nullptr);
    // what the buffers were carved with travels with them (cache of this process, else the buffers' own headers): a buffer that carries none is refused
    uint32_t bin_cap = 0, log_depth = 0;
    if (R > 0) { if (int rc = layout_of(binning_buffer, (uint32_t)R, &bin_cap, (hipStream_t)stream, true)) return rc; } // (a run-ahead forward carved it for its capacity)
    if (uses_blend_log(*settings)) { if (int rc = log_depth_of(image_buffer, (int64_t)R, &log_depth, (hipStream_t)stream, true)) return rc; }
    BinningState b = carve_binning(binning_buffer, (size_t)bin_cap, nullptr);
    ImageState img = carve_image(image_buffer, width, height, f.ty0, f.ty1, (int)log_depth, nullptr);
    if (!radii) radii = g.internal_radii;

    BackwardParams bw;
    bw.cam = cam;
    bw.absgrad = absgrad;
    bw.blend_stats = blend_stats;
    bw.bg_image = bbg.bg_image; bw.dL_dalpha = bbg.dL_dalpha; bw.dL_dbackground = bbg.dL_dbackground;
    bw.invdepth = binv.invdepth; bw.dL_dinvdepth = binv.dL_dinvdepth;
    bw.sh_stash = sh_stash;
    if (bsh.dc && !colors_precomp) { f.sh_dc = bsh.dc; bw.dL_ddc = bsh.dL_ddc; }
    f.raw_params = req.raw_params;
    bw.pixel_colors = pixel_colors; bw.dL_dpix = dL_dpix; bw.dL_dmean2D = dL_dmean2D; bw.grad_rec = grad_records;
    bw.grad_stride = (phases & 4) ? STP_GRAD_RECORD_USED : STP_GRAD_RECORD_FLOATS;
    bw.clear_rec = (phases & 8) ? 1 : 0;
    bw.chunks = (phases >> 8) & 0xFF; bw.chunk = (phases >> 16) & 0xFF; // per-Gaussian half by id range (see stp_raster.h)
    if (bw.chunks > 1 && (bw.chunk >= bw.chunks || (phases & 1))) return fail(STP_ERR_INVALID_ARGUMENT, "chunked per-Gaussian half: chunk index out of range, or combined with the render half");
    bw.dL_dopacity = dL_dopacity; bw.dL_dcolor = dL_dcolor; bw.dL_dmean3D = dL_dmean3D; bw.dL_dcov3D = dL_dcov3D; bw.dL_dsh = dL_dsh;
    bw.dL_dscale = dL_dscale; bw.dL_drot = dL_drot;

    // the uniform background gradient's scratch is taken BEFORE anything is launched: a call that cannot get it has done nothing
    std::unique_lock<std::mutex> bg_lock;
    BackgroundSlot* bg_slot = nullptr;
    if ((phases & 1) && bw.dL_dbackground && !bw.bg_image) {
        bg_lock = std::unique_lock<std::mutex>(g_background_mutex);
        if (int rc = acquire_background_scratch(&bg_slot, st)) return rc;
    }
    if (phases & 1) {
        timer_begin_backward();
        timer_mark(5, st);
        std::string err;
        hipError_t e = launch_render_backward(f, g, b, img, bw, st, &err);
        if (e != hipSuccess) {
            if (!err.empty()) return fail(settings->sort_mode == MODE_FULL ? STP_ERR_NO_BACKWARD : STP_ERR_QUEUE_SIZE, err);
            return fail_hip(e, "backward render launch");
        }
        STP_DEBUG_SYNC("backward render");
        if (bw.dL_dbackground) { // (reads final_T and dL_dpix only: nothing the render kernels write)
            STP_TRY(launch_background_grad(f, img, bw, bg_slot ? bg_slot->partials : nullptr, st), "background gradient launch");
            if (bg_slot) { // the slot's next user waits for these kernels (no event: wait for them here)
                bg_slot->used = hipEventRecord(bg_slot->done, st) == hipSuccess;
                if (!bg_slot->used) STP_TRY(hipStreamSynchronize(st), "synchronize behind the background gradient");
                bg_lock.unlock();
            }
            STP_DEBUG_SYNC("background gradient");
        }
        timer_mark(6, st);
    }
    if (phases & 2) {
        if (!(phases & 1)) timer_mark(6, st);
        STP_TRY(launch_preprocess_backward(f, g, radii, bw, st), "backward preprocess launch");
        STP_DEBUG_SYNC("backward preprocess");
        timer_mark(7, st);
    }
    if (!(phases & 2)) keep_for_per_gaussian_call(req); // render-only: the sums are in the records, the per-Gaussian call collects them
    return 0;
}

int stp_backward(int P, int D, int M, int R, const float* background, int width, int height, const StpSettings* settings,
                 const float* means3D, const float* shs, const float* opacities, const float* colors_precomp, const float* scales,
                 float scale_modifier, const float* rotations, const float* cov3D_precomp, const float* viewmatrix,
                 const float* projmatrix, const float* inv_viewprojmatrix, const float* cam_pos, float tan_fovx, float tan_fovy,
                 const float* pixel_colors, const int* radii, char* geom_buffer, char* binning_buffer, char* image_buffer,
                 const float* dL_dpix, float* dL_dmean2D, float* grad_records, float* dL_dopacity, float* dL_dcolor,
                 float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot, int debug, void* stream)
{
    return stp_backward_phases(3, P, D, M, R, background, width, height, settings, means3D, shs, opacities, colors_precomp, scales,
                               scale_modifier, rotations, cov3D_precomp, viewmatrix, projmatrix, inv_viewprojmatrix, cam_pos, tan_fovx,
                               tan_fovy, pixel_colors, radii, geom_buffer, binning_buffer, image_buffer, dL_dpix, dL_dmean2D, grad_records,
                               dL_dopacity, dL_dcolor, dL_dmean3D, dL_dcov3D, dL_dsh, dL_dscale, dL_drot, debug, stream);
}

int stp_activate_params(int P, const float* scaling, const float* rotation, const float* opacity, float* scales, float* rotations, float* opacities,
                        void* stream)
{
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_activate_params: negative P");
    if (P >= (1 << 29)) return fail(STP_ERR_INVALID_ARGUMENT, "stp_activate_params: P must be below 2^29");
    if (!scaling != !scales || !rotation != !rotations || !opacity != !opacities)
        return fail(STP_ERR_INVALID_ARGUMENT, "stp_activate_params: an input and its output must be given, or be NULL, together");
    if (P == 0) return 0;
    hipError_t e = hipSuccess;
    const int launches = launch_activate_params(P, scaling, rotation, opacity, scales, rotations, opacities, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "activate_params launch");
    return launches;
}

int stp_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix, uint8_t* present, void* stream)
{
    (void)projmatrix; // reference checkFrustum only applies the view-space near test (rasterizer_impl.cu:113-128)
    if (P == 0) return 0;
    if (!means3D || !viewmatrix || !present) return fail(STP_ERR_INVALID_ARGUMENT, "null input");
    STP_TRY(launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream), "mark_visible launch");
    return 0;
}

int stp_sparse_adam(int n_tensors, const StpAdamTensor* tensors, int N, const void* visible, int visible_kind, float beta1, float beta2, void* stream)
{
    // everything is checked before the first launch: a refused call has updated nothing
    if (n_tensors < 0 || N < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_sparse_adam: negative count");
    if (visible_kind != 0 && visible_kind != 1)
        return fail(STP_ERR_INVALID_ARGUMENT, "stp_sparse_adam: unknown visible_kind " + std::to_string(visible_kind) + " (0: N bytes, 1: N int32 radii)");
    if (n_tensors > 0 && !tensors) return fail(STP_ERR_INVALID_ARGUMENT, "stp_sparse_adam: null tensor table");
    bool any = false;
    for (int k = 0; k < n_tensors; k++) {
        const StpAdamTensor& t = tensors[k];
        const std::string which = "stp_sparse_adam: tensor " + std::to_string(k);
        if (t.numel < 0) return fail(STP_ERR_INVALID_ARGUMENT, which + ": negative numel");
        if (t.numel >= (1ll << 31)) return fail(STP_ERR_INVALID_ARGUMENT, which + ": numel " + std::to_string(t.numel) + " >= 2^31");
        if (t.numel == 0) continue;
        if (N == 0 || t.numel % N != 0)
            return fail(STP_ERR_INVALID_ARGUMENT, which + ": numel " + std::to_string(t.numel) + " is not a multiple of N = " + std::to_string(N));
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return fail(STP_ERR_INVALID_ARGUMENT, which + ": null pointer");
        any = true;
    }
    if (!any) return 0;
    if (!visible) return fail(STP_ERR_INVALID_ARGUMENT, "stp_sparse_adam: null visible");
    hipError_t e;
    const int launches = launch_sparse_adam(n_tensors, tensors, N, visible, visible_kind, beta1, beta2, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "sparse_adam launch");
    return launches;
}

int stp_dense_adam(int n_tensors, const StpDenseAdamTensor* tensors, void* stream)
{
    // everything is checked before the first launch: a refused call has updated nothing
    if (n_tensors < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_dense_adam: negative count");
    if (n_tensors > 0 && !tensors) return fail(STP_ERR_INVALID_ARGUMENT, "stp_dense_adam: null tensor table");
    bool any = false;
    for (int k = 0; k < n_tensors; k++) {
        const StpDenseAdamTensor& t = tensors[k];
        const std::string which = "stp_dense_adam: tensor " + std::to_string(k);
        if (t.numel < 0) return fail(STP_ERR_INVALID_ARGUMENT, which + ": negative numel");
        if (t.numel >= (1ll << 31)) return fail(STP_ERR_INVALID_ARGUMENT, which + ": numel " + std::to_string(t.numel) + " >= 2^31");
        if (t.numel == 0) continue; // (nothing of an entry without elements is looked at)
        if (t.reg_kind < 0 || t.reg_kind > 2)
            return fail(STP_ERR_INVALID_ARGUMENT, which + ": unknown reg_kind " + std::to_string(t.reg_kind) + " (0: none, 1: sigmoid, 2: exp)");
        if (!(t.bias2_sqrt > 0.0f) || !std::isfinite(t.bias2_sqrt))
            return fail(STP_ERR_INVALID_ARGUMENT, which + ": bias2_sqrt " + std::to_string(t.bias2_sqrt) + " is not a positive finite number");
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return fail(STP_ERR_INVALID_ARGUMENT, which + ": null pointer");
        any = true;
    }
    if (!any) return 0;
    hipError_t e;
    const int launches = launch_dense_adam(n_tensors, tensors, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "dense_adam launch");
    return launches;
}

int stp_mcmc_relocation(int n, const float* opacity_old, const float* scale_old, const void* N, int n_kind, int n_max, float* opacity_new,
                        float* scale_new, void* stream)
{
    // everything is checked before the launch
    if (n < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mcmc_relocation: negative n");
    if (n_kind != 0 && n_kind != 1)
        return fail(STP_ERR_INVALID_ARGUMENT, "stp_mcmc_relocation: unknown n_kind " + std::to_string(n_kind) + " (0: int32, 1: int64)");
    if (n_max < 2 || n_max > 51)
        return fail(STP_ERR_INVALID_ARGUMENT, "stp_mcmc_relocation: n_max " + std::to_string(n_max) + " outside [2, 51] (N is clamped to [1, n_max - 1])");
    if (n == 0) return 0;
    if (!opacity_old || !scale_old || !N || !opacity_new || !scale_new) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mcmc_relocation: null pointer");
    hipError_t e;
    const int launches = launch_mcmc_relocation(n, opacity_old, scale_old, N, n_kind, n_max, opacity_new, scale_new, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "mcmc_relocation launch");
    return launches;
}

int stp_mcmc_add_noise(int P, float* xyz, const float* scales, const float* rotations, const float* opacities, const float* noise, float noise_scale,
                       float k, float x0, int raw, void* stream)
{
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mcmc_add_noise: negative P");
    if (raw != 0 && raw != 1) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mcmc_add_noise: raw must be 0 or 1, got " + std::to_string(raw));
    if (P == 0) return 0;
    if (!xyz || !scales || !rotations || !opacities || !noise) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mcmc_add_noise: null pointer");
    hipError_t e;
    const int launches = launch_mcmc_add_noise(P, xyz, scales, rotations, opacities, noise, noise_scale, k, x0, raw, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "mcmc_add_noise launch");
    return launches;
}

// ---- Mip-Splatting's 3D filter (stp_mip_filter.hip): everything is checked before the first launch
int stp_mip_filter_3d(int P, int C, const float* xyz, const float* world_view_transforms, const float* intrinsics, void* workspace, float* filter_3d, void* stream)
{
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_filter_3d: negative P");
    if (C < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_filter_3d: negative C");
    if (C == 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_filter_3d: C == 0: the filter needs at least one camera");
    if (C >= (1 << 24)) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_filter_3d: C must be below 2^24");
    if (P == 0) return 0;
    if (!xyz || !world_view_transforms || !intrinsics || !workspace || !filter_3d) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_filter_3d: null pointer");
    hipError_t e;
    const int launches = launch_mip_filter_3d(P, C, xyz, world_view_transforms, intrinsics, workspace, filter_3d, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "mip_filter_3d launch");
    return launches;
}

int stp_mip_activations_forward(int P, const float* scaling, const float* opacity, const float* filter_3d, float* scales, float* opacities, void* stream)
{
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_activations_forward: negative P");
    if (P == 0) return 0;
    if (!scaling || !opacity || !filter_3d || !scales || !opacities) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_activations_forward: null pointer");
    hipError_t e;
    const int launches = launch_mip_activations_forward(P, scaling, opacity, filter_3d, scales, opacities, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "mip_activations_forward launch");
    return launches;
}

int stp_mip_activations_backward(int P, const float* scaling, const float* opacity, const float* filter_3d, const float* grad_scales, const float* grad_opacities,
                                 float* grad_scaling, float* grad_opacity, void* stream)
{
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_activations_backward: negative P");
    if (P == 0) return 0;
    if (!scaling || !opacity || !filter_3d || !grad_scaling || !grad_opacity) return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_activations_backward: null pointer");
    if (!grad_scales && !grad_opacities)
        return fail(STP_ERR_INVALID_ARGUMENT, "stp_mip_activations_backward: null pointer: grad_scales and grad_opacities are both absent");
    hipError_t e;
    const int launches = launch_mip_activations_backward(P, scaling, opacity, filter_3d, grad_scales, grad_opacities, grad_scaling, grad_opacity, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "mip_activations_backward launch");
    return launches;
}

// ---- the 3DGS-MCMC relocation and growth (stp_mcmc_relocate.hip): everything is checked before the first launch
static constexpr int MCMC_RELOCATE_MAX_P = 1 << 28;
static const char* const MCMC_ROLE_NAMES[3] = {"", "1 (opacity, row 1)", "2 (scaling, row 3)"};
static const int MCMC_ROLE_ROWS[3] = {0, 1, 3};
static const RowRoles MCMC_ROLES = {2, MCMC_ROLE_NAMES, MCMC_ROLE_ROWS, "(0 plain, 1 opacity, 2 scaling)", "rows", nullptr};

// P, raw and the scratch of the three calls: 0 = fine, negative = refused
static int check_mcmc_relocate(const char* who, int P, int raw, const void* scratch, size_t scratch_bytes)
{
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative P");
    if (P > MCMC_RELOCATE_MAX_P) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": P = " + std::to_string(P) + " > 2^28");
    if (raw != 0 && raw != 1) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": raw must be 0 or 1, got " + std::to_string(raw));
    if (P == 0) return 0;
    if (!scratch) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer (scratch)");
    return check_scratch(who, scratch, scratch_bytes, mcmc_relocate_scratch_bytes(P), 16, "stp_mcmc_relocate_scratch_bytes");
}

size_t stp_mcmc_relocate_scratch_bytes(int P)
{
    if (P < 0 || P > MCMC_RELOCATE_MAX_P) return 0;
    return mcmc_relocate_scratch_bytes(P);
}

int stp_mcmc_sample(int P, const float* opacity, int rule, float min_opacity, int raw, int n_draws, const float* uniforms, void* scratch, size_t scratch_bytes,
                    uint32_t* weights, int32_t* src, int32_t* count, void* stream)
{
    static const char* const who = "stp_mcmc_sample";
    if (n_draws < 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative n_draws");
    if (rule != 0 && rule != 1) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown rule " + std::to_string(rule) + " (0: relocation, 1: growth)");
    if (const int rc = check_mcmc_relocate(who, P, raw, scratch, scratch_bytes)) return rc;
    if (rule == 0 && n_draws != P)
        return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": rule 0 draws once per row: n_draws = " + std::to_string(n_draws) + ", P = " + std::to_string(P));
    if (n_draws > 0 && (!uniforms || !src)) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    if (P == 0) {
        if (n_draws > 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": " + std::to_string(n_draws) + " draws from P = 0 rows");
        return 0;
    }
    if (!opacity || !count) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    hipError_t e;
    const int launches = launch_mcmc_sample(P, opacity, rule, min_opacity, raw, n_draws, uniforms, scratch, weights, src, count, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "mcmc_sample launch");
    return launches;
}

int stp_mcmc_relocate_apply(int P, const int32_t* src, const int32_t* count, int n_tensors, const StpMcmcTensor* tensors, float min_opacity, int raw,
                            int reset_dead_moments, void* scratch, size_t scratch_bytes, void* stream)
{
    static const char* const who = "stp_mcmc_relocate_apply";
    if (const int rc = check_mcmc_relocate(who, P, raw, scratch, scratch_bytes)) return rc;
    if (const int rc = check_row_tensors(who, n_tensors, tensors, P, MCMC_ROLES, true, P > 0, true)) return rc;
    if (P == 0) return 0;
    if (!src || !count) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    hipError_t e;
    const int launches = launch_mcmc_relocate_apply(P, src, count, n_tensors, tensors, min_opacity, raw, reset_dead_moments ? 1 : 0, scratch, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "mcmc_relocate_apply launch");
    return launches;
}

int stp_mcmc_add_apply(int P, int n_new, const int32_t* src, const int32_t* count, int n_tensors, const StpMcmcTensor* tensors, float min_opacity, int raw,
                       void* scratch, size_t scratch_bytes, void* stream)
{
    static const char* const who = "stp_mcmc_add_apply";
    if (n_new < 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative n_new");
    if (const int rc = check_mcmc_relocate(who, P, raw, scratch, scratch_bytes)) return rc;
    if (const int rc = check_row_tensors(who, n_tensors, tensors, (long long)P + n_new, MCMC_ROLES, false, P > 0, true)) return rc;
    if (P == 0) {
        if (n_new > 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": " + std::to_string(n_new) + " new rows from P = 0 rows");
        return 0;
    }
    if (!count || (n_new > 0 && !src)) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    hipError_t e;
    const int launches = launch_mcmc_add_apply(P, n_new, src, count, n_tensors, tensors, min_opacity, raw, scratch, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "mcmc_add_apply launch");
    return launches;
}

size_t stp_knn_scratch_bytes(int P) { return knn_scratch_bytes(P); }

int stp_knn_mean_dist2(int P, const float* points, void* scratch, size_t scratch_bytes, float* mean_dist2, void* stream)
{
    // everything is checked before the first launch
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_knn_mean_dist2: negative P");
    if (P == 0) return 0;
    if (P < 4)
        return fail(STP_ERR_INVALID_ARGUMENT, "stp_knn_mean_dist2: P = " + std::to_string(P) + ": the mean over three neighbours needs at least 4 points");
    if (!points || !scratch || !mean_dist2) return fail(STP_ERR_INVALID_ARGUMENT, "stp_knn_mean_dist2: null pointer");
    if (const int rc = check_scratch("stp_knn_mean_dist2", scratch, scratch_bytes, knn_scratch_bytes(P), 16, "stp_knn_scratch_bytes")) return rc;
    hipError_t e;
    const int launches = launch_knn_mean_dist2(P, points, scratch, mean_dist2, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "knn_mean_dist2");
    return launches;
}

size_t stp_spatial_order_scratch_bytes(int P) { return spatial_order_scratch_bytes(P); }

int stp_spatial_order(int P, const float* xyz, void* scratch, size_t scratch_bytes, int32_t* order, uint32_t* codes, void* stream)
{
    // everything is checked before the first launch
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, "stp_spatial_order: negative P");
    if (P == 0) return 0;
    if (!xyz) return fail(STP_ERR_INVALID_ARGUMENT, "stp_spatial_order: null pointer (xyz)");
    if (!order) return fail(STP_ERR_INVALID_ARGUMENT, "stp_spatial_order: null pointer (order)");
    if (!scratch) return fail(STP_ERR_INVALID_ARGUMENT, "stp_spatial_order: null pointer (scratch)");
    if (const int rc = check_scratch("stp_spatial_order", scratch, scratch_bytes, spatial_order_scratch_bytes(P), 16, "stp_spatial_order_scratch_bytes")) return rc;
    hipError_t e;
    const int launches = launch_spatial_order(P, xyz, scratch, order, codes, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "spatial_order");
    return launches;
}

// ---- the gather of rows (stp_reorder.hip): everything is checked before the first launch
static const int GATHER_ROLE_ROWS[1] = {0};
static const RowRoles GATHER_ROLES = {0, nullptr, GATHER_ROLE_ROWS, "(0 plain: a gather has no other)", "max(P, M)", nullptr};

int stp_gather_rows(int P, int M, const int32_t* index, int n_tensors, const StpGatherTensor* tensors, void* stream)
{
    static const char* const who = "stp_gather_rows";
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative P");
    if (M < 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative M");
    // (the work is flattened over the M output rows, and a source offset is below P * row)
    if (const int rc = check_row_tensors(who, n_tensors, tensors, P > M ? P : M, GATHER_ROLES, false, M > 0, false)) return rc;
    if (M == 0 || n_tensors == 0) return 0;
    if (P == 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": " + std::to_string(M) + " rows from P = 0 rows");
    if (!index) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer (index)");
    // out of place only: no output may overlap an input of the call (a tensor or a moment of ANY entry, or the index)
    struct Span { uintptr_t lo, hi; int tensor; const char* what; };
    std::vector<Span> in, out;
    in.push_back({reinterpret_cast<uintptr_t>(index), reinterpret_cast<uintptr_t>(index) + (uintptr_t)M * sizeof(int32_t), -1, "index"});
    for (int k = 0; k < n_tensors; k++) {
        const StpGatherTensor& t = tensors[k];
        const uintptr_t nin = (uintptr_t)P * t.row * sizeof(float), nout = (uintptr_t)M * t.row * sizeof(float);
        const auto span = [k](const void* p, uintptr_t n, const char* what) { return Span{reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + n, k, what}; };
        in.push_back(span(t.param, nin, "param"));
        out.push_back(span(t.param_out, nout, "param_out"));
        if (t.exp_avg) {
            in.push_back(span(t.exp_avg, nin, "exp_avg"));
            in.push_back(span(t.exp_avg_sq, nin, "exp_avg_sq"));
            out.push_back(span(t.exp_avg_out, nout, "exp_avg_out"));
            out.push_back(span(t.exp_avg_sq_out, nout, "exp_avg_sq_out"));
        }
    }
    for (const Span& o : out)
        for (const Span& i : in)
            if (o.lo < i.hi && i.lo < o.hi)
                return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": tensor " + std::to_string(o.tensor) + ": " + o.what + " overlaps " +
                                                          (i.tensor < 0 ? std::string("the index") : i.what + std::string(" of tensor ") + std::to_string(i.tensor)) +
                                                          ": the call is out of place only");
    hipError_t e;
    const int launches = launch_gather_rows(P, M, index, n_tensors, tensors, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "gather_rows launch");
    return launches;
}

// ---- densification (stp_densify.hip): everything is checked before the first launch
static const int DENSIFY_ROLE_ROWS[4] = {0, 3, 3, 4};
static const RowRoles DENSIFY_ROLES = {3, nullptr, DENSIFY_ROLE_ROWS, "(0 plain, 1 xyz, 2 scaling, 3 rotation)", "P",
                                       "a split needs exactly one tensor of each of the roles 1 (xyz, row 3), 2 (scaling, row 3) and 3 (rotation, row 4)"};
static int check_densify_P(const char* who, int P)
{
    if (P < 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative P");
    if (3ll * P >= (1ll << 31)) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": 3 P = " + std::to_string(3ll * P) + " >= 2^31");
    return 0;
}

int stp_densify_stats(int P, float* grad_accum, float* denom, float* max_radii2D, const float* grad2d, int grad_stride, const void* visible,
                      int visible_kind, void* stream)
{
    if (const int rc = check_densify_P("stp_densify_stats", P)) return rc;
    if (grad_stride != 2 && grad_stride != 3)
        return fail(STP_ERR_INVALID_ARGUMENT, "stp_densify_stats: grad_stride must be 2 or 3, got " + std::to_string(grad_stride));
    if (visible_kind != 0 && visible_kind != 1)
        return fail(STP_ERR_INVALID_ARGUMENT, "stp_densify_stats: unknown visible_kind " + std::to_string(visible_kind) + " (0: P bytes, 1: P int32 radii)");
    if (max_radii2D && visible_kind == 0)
        return fail(STP_ERR_INVALID_ARGUMENT, "stp_densify_stats: max_radii2D needs the radii (visible_kind 1): bytes hold no radius to read");
    if (P == 0) return 0;
    if (!grad_accum || !denom || !grad2d || !visible) return fail(STP_ERR_INVALID_ARGUMENT, "stp_densify_stats: null pointer");
    hipError_t e;
    const int launches = launch_densify_stats(P, grad_accum, denom, max_radii2D, grad2d, grad_stride, visible, visible_kind, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "densify_stats launch");
    return launches;
}

int stp_densify_plan(int P, const float* grad_accum, const float* denom, const float* scaling, const float* opacity, const float* max_radii2D,
                     const StpDensifyRule* rule, uint8_t* plan, void* stream)
{
    if (const int rc = check_densify_P("stp_densify_plan", P)) return rc;
    if (!rule) return fail(STP_ERR_INVALID_ARGUMENT, "stp_densify_plan: null rule");
    if (P == 0) return 0;
    if (!grad_accum || !denom || !scaling || !opacity || !plan) return fail(STP_ERR_INVALID_ARGUMENT, "stp_densify_plan: null pointer");
    hipError_t e;
    const int launches = launch_densify_plan(P, grad_accum, denom, scaling, opacity, max_radii2D, *rule, plan, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "densify_plan launch");
    return launches;
}

size_t stp_densify_scratch_bytes(int P)
{
    if (P < 0 || 3ll * P >= (1ll << 31)) return 0;
    return densify_scratch_bytes(P);
}

int stp_densify_scan(int P, const uint8_t* plan, void* scratch, size_t scratch_bytes, uint32_t* offsets, int64_t counts[3], void* stream)
{
    if (const int rc = check_densify_P("stp_densify_scan", P)) return rc;
    if (!counts) return fail(STP_ERR_INVALID_ARGUMENT, "stp_densify_scan: null counts");
    if (P == 0) {
        counts[0] = counts[1] = counts[2] = 0;
        return 0;
    }
    if (!plan || !scratch || !offsets) return fail(STP_ERR_INVALID_ARGUMENT, "stp_densify_scan: null pointer");
    if (const int rc = check_scratch("stp_densify_scan", scratch, scratch_bytes, densify_scratch_bytes(P), 4, "stp_densify_scratch_bytes")) return rc;
    hipError_t e;
    const int launches = launch_densify_scan(P, plan, scratch, offsets, counts, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "densify_scan");
    return launches;
}

int stp_densify_apply(int P, const uint8_t* plan, const uint32_t* offsets, const int64_t counts[3], int n_tensors, const StpDensifyTensor* tensors,
                      const float* noise, float split_shrink, int raw, void* stream)
{
    static const char* const who = "stp_densify_apply";
    if (const int rc = check_densify_P(who, P)) return rc;
    if (raw != 0 && raw != 1) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": raw must be 0 or 1, got " + std::to_string(raw));
    if (!counts) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null counts");
    for (int j = 0; j < 3; j++)
        if (counts[j] < 0 || counts[j] > P)
            return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": counts[" + std::to_string(j) + "] = " + std::to_string((long long)counts[j]) + " outside [0, P]");
    const int64_t nS = counts[2], M = counts[0] + counts[1] + 2 * nS;
    // (the work is flattened over the P source rows; without a split any role may be absent and have any width)
    if (const int rc = check_row_tensors(who, n_tensors, tensors, P, DENSIFY_ROLES, false, M > 0, nS > 0)) return rc;
    if (nS > 0) {
        if (!noise) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null noise with nS = " + std::to_string((long long)nS));
    }
    if (P == 0 || M == 0 || n_tensors == 0) return 0;
    if (!plan || !offsets) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    hipError_t e;
    const int launches = launch_densify_apply(P, plan, offsets, counts, n_tensors, tensors, noise, split_shrink, raw, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "densify_apply launch");
    return launches;
}

// the sizes of a photometric call: 0 = empty work, 1 = work, negative = refused (with the last error set)
static int check_photometric_sizes(const char* who, int planes, int H, int W)
{
    if (planes < 0 || H < 0 || W < 0) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": negative size");
    if (planes == 0 || H == 0 || W == 0) return 0;
    const long long rows = (long long)planes * H; // < 2^62
    if (rows >= (1ll << 31) || rows * W >= (1ll << 31))
        return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": planes * H * W = " + std::to_string(planes) + " * " + std::to_string(H) + " * " + std::to_string(W) + " >= 2^31");
    return 1;
}

size_t stp_photometric_workspace_floats(int planes, int H, int W)
{
    if (planes <= 0 || H <= 0 || W <= 0) return 0;
    const long long rows = (long long)planes * H;
    if (rows >= (1ll << 31) || rows * W >= (1ll << 31)) return 0; // (a size the calls refuse)
    return 2 * (size_t)photometric_groups(planes, H, W);
}

int stp_photometric_forward(int planes, int H, int W, const float* image, const float* target, float* out2, float* maps, float* workspace, void* stream)
{
    // everything is checked before the first launch
    const int work = check_photometric_sizes("stp_photometric_forward", planes, H, W);
    if (work <= 0) return work;
    if (!image || !target || !out2 || !workspace) return fail(STP_ERR_INVALID_ARGUMENT, "stp_photometric_forward: null pointer");
    hipError_t e;
    const int launches = launch_photometric_forward(planes, H, W, image, target, out2, maps, workspace, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "photometric forward launch");
    return launches;
}

int stp_photometric_backward(int planes, int H, int W, const float* image, const float* target, const float* maps, const float* dL_dout2,
                             float* dL_dimage, void* stream)
{
    const int work = check_photometric_sizes("stp_photometric_backward", planes, H, W);
    if (work <= 0) return work;
    if (!maps) return fail(STP_ERR_INVALID_ARGUMENT, "stp_photometric_backward: null maps (a forward without maps cannot be differentiated)");
    if (!image || !target || !dL_dout2 || !dL_dimage) return fail(STP_ERR_INVALID_ARGUMENT, "stp_photometric_backward: null pointer");
    hipError_t e;
    const int launches = launch_photometric_backward(planes, H, W, image, target, maps, dL_dout2, dL_dimage, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "photometric backward launch");
    return launches;
}

// the extras of a training-loss call in their final form (*x): 0 = fine, negative = refused.  Looks at sizes and pointers only
static int check_training_extras(const char* who, int planes, int H, int W, const StpTrainingLoss* extras, StpTrainingLoss* x)
{
    *x = extras ? *extras : StpTrainingLoss{};
    const std::string w = std::string(who) + ": ";
    for (const int32_t flag : {x->clamp, x->exposure_batched, x->alpha_mask_batched})
        if (flag != 0 && flag != 1) return fail(STP_ERR_INVALID_ARGUMENT, w + "clamp, exposure_batched and alpha_mask_batched must be 0 or 1");
    if (x->channels < 0 || x->depth_planes < 0) return fail(STP_ERR_INVALID_ARGUMENT, w + "negative size");
    if (x->channels == 0) x->channels = 3;
    if (x->exposure && (x->channels != 3 || planes % 3 != 0))
        return fail(STP_ERR_INVALID_ARGUMENT, w + "exposure needs three channels per image, got planes = " + std::to_string(planes) + ", channels = " + std::to_string(x->channels));
    if (x->alpha_mask && planes % x->channels != 0)
        return fail(STP_ERR_INVALID_ARGUMENT, w + "planes = " + std::to_string(planes) + " is no multiple of channels = " + std::to_string(x->channels));
    if (planes % x->channels != 0) x->channels = 1; // (no per-image input: every plane is its own image)
    if (!x->invdepth != !x->mono_invdepth) return fail(STP_ERR_INVALID_ARGUMENT, w + "invdepth and mono_invdepth come together or not at all");
    if (!x->invdepth && (x->depth_mask || x->depth_planes > 0)) return fail(STP_ERR_INVALID_ARGUMENT, w + "depth_mask or depth_planes without invdepth");
    if (x->invdepth && x->depth_planes == 0) return fail(STP_ERR_INVALID_ARGUMENT, w + "invdepth with depth_planes = 0");
    if (x->invdepth && check_photometric_sizes(who, x->depth_planes, H, W) < 0) return STP_ERR_INVALID_ARGUMENT;
    return 0;
}

size_t stp_training_loss_workspace_floats(int planes, int H, int W, int depth_planes)
{
    if (stp_photometric_workspace_floats(planes, H, W) == 0) return 0;
    if (depth_planes < 0 || (depth_planes > 0 && stp_photometric_workspace_floats(depth_planes, H, W) == 0)) return 0; // (sizes the calls refuse)
    return training_loss_workspace_floats(planes, H, W, depth_planes);
}

int stp_training_loss_forward(int planes, int H, int W, const float* image, const float* target, const StpTrainingLoss* extras, float* out3, float* maps,
                              float* workspace, void* stream)
{
    static const char* const who = "stp_training_loss_forward";
    const int work = check_photometric_sizes(who, planes, H, W);
    if (work < 0) return work;
    StpTrainingLoss x;
    if (const int rc = check_training_extras(who, planes, H, W, extras, &x)) return rc;
    if (work == 0) return 0;
    if (!image || !target || !out3 || !workspace) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    hipError_t e;
    const int launches = launch_training_loss_forward(planes, H, W, image, target, x, out3, maps, workspace, (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "training loss forward launch");
    return launches;
}

int stp_training_loss_backward(int planes, int H, int W, const float* image, const float* target, const StpTrainingLoss* extras, const float* maps,
                               const float* dL_dout3, float* dL_dimage, float* dL_dexposure, float* dL_dinvdepth, float* workspace, void* stream)
{
    static const char* const who = "stp_training_loss_backward";
    const int work = check_photometric_sizes(who, planes, H, W);
    if (work < 0) return work;
    StpTrainingLoss x;
    if (const int rc = check_training_extras(who, planes, H, W, extras, &x)) return rc;
    if (dL_dexposure && !x.exposure) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": dL_dexposure without exposure");
    if (dL_dinvdepth && !x.invdepth) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": dL_dinvdepth without invdepth");
    if (work == 0) return 0;
    if (!maps) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null maps (a forward without maps cannot be differentiated)");
    if (!image || !target || !dL_dout3 || !dL_dimage || (dL_dexposure && !workspace)) return fail(STP_ERR_INVALID_ARGUMENT, std::string(who) + ": null pointer");
    hipError_t e;
    const int launches = launch_training_loss_backward(planes, H, W, image, target, x, maps, dL_dout3, dL_dimage, dL_dexposure, dL_dinvdepth, workspace,
                                                       (hipStream_t)stream, &e);
    if (e != hipSuccess) return fail_hip(e, "training loss backward launch");
    return launches;
}

} // extern "C"
