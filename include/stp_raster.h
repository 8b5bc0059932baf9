/*
 * stp_raster.h -- C ABI of libstp_raster.so, the MI355X (gfx950) sorted Gaussian-splat rasterizer.
 *
 * This is the drop-in boundary for the hot path of r4dl/StopThePop-Rasterization.  Each entry point
 * replaces one member of the reference's C++ API `CudaRasterizer::Rasterizer`
 * (reference cuda_rasterizer/rasterizer.h:184-258), which is what the reference's pybind layer
 * (rasterize_points.cu:43-253, ext.cpp:15-19) calls.  Signatures are plain C: device pointers, sizes,
 * a POD settings struct, allocator callbacks and a stream handle -- no torch, no C++ types.
 *
 * Conventions (identical to the reference unless stated):
 *   - all array arguments are DEVICE pointers to contiguous fp32/int32 data; an absent optional
 *     input (shs / colors_precomp / scales / rotations / cov3D_precomp) is NULL
 *     (reference tests pointers against nullptr: forward.cu:126,200; rasterizer_impl.cu:367,473,500);
 *   - matrices are 16 floats in the 3DGS row-vector layout (p_hom = [x y z 1] @ M), i.e. element
 *     m[4*col+row] in kernel indexing (auxiliary.h:103-149);
 *   - `stream` is a hipStream_t (NULL = the null stream).  The reference launches on the legacy
 *     default stream; we launch everything on the stream the caller passes;
 *   - functions return >= 0 on success and a negative StpStatus on failure; stp_last_error()
 *     returns a thread-local message for the most recent failure.
 */
#ifndef STP_RASTER_H_INCLUDED
#define STP_RASTER_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STP_ABI_VERSION 7
#define STP_GRAD_RECORD_FLOATS 16 /* floats per Gaussian in grad_records (see stp_backward) */
#define STP_GRAD_RECORD_USED 9    /* of which these carry data; the record stride of stp_backward_phases' compact form (phases bit 2) */
#define STP_GRAD_RECORD_ABS 9     /* first of the two slots that carry sum |dL/dmean2D| xy under stp_set_backward_absgrad (padded records only) */
#define STP_GRAD_RECORD_STATS 11  /* first of the three slots that carry sum, max and count of the blend weights under stp_set_backward_blend_stats (padded records only) */
#define STP_GRAD_RECORD_INVDEPTH 14 /* the slot that carries dL/d(1/z) of the Gaussian under stp_set_backward_invdepth (padded records only) */

/* Replaces CudaRasterizer::SplattingSettings + SortSettings + SortQueueSizes + CullingSettings
   (rasterizer.h:27-135) and their json parser (rasterizer.h:160-182): the host binding fills this
   from the Python settings dict. */
typedef struct StpSettings {
    int32_t sort_mode;                /* 0 GLOBAL, 1 PER_PIXEL_FULL, 2 PER_PIXEL_KBUFFER, 3 HIERARCHICAL (rasterizer.h:27-33) */
    int32_t sort_order;               /* 0 VIEWSPACE_Z, 1 DISTANCE, 2 PER_TILE_DEPTH_CENTER, 3 PER_TILE_DEPTH_MAXPOS (:35-41) */
    int32_t queue_tile_4x4;           /* parsed, unused (the reference hard-wires 64: hierarchical_render.cuh:286-287) */
    int32_t queue_tile_2x2;           /* hierarchical MID queue: 8, 12 or 20 (rasterizer.h:56) */
    int32_t queue_per_pixel;          /* hierarchical HEAD queue (4, 8, 16; backward also 12) or k-buffer window */
    int32_t rect_bounding;            /* rasterizer.h:79-85 */
    int32_t tight_opacity_bounding;
    int32_t tile_based_culling;
    int32_t hierarchical_4x4_culling;
    int32_t load_balancing;           /* performance hint only; results do not depend on it */
    int32_t proper_ewa_scaling;
    /* Extension (not in the reference): restrict binning + rendering to tile rows [tile_y0, tile_y1)
       for tile-row sharding of one frame over several GPUs.  tile_y1 <= 0 selects all rows. */
    int32_t tile_y0;
    int32_t tile_y1;
    /* Extension (not in the reference): hierarchical mode only.  When non-zero the forward also records, per
       pixel, the order in which it blended its Gaussians (2 bytes per blended pair, 512 B per pixel, inside the
       image buffer); a backward called with the same flag replays that log instead of re-running the resort
       (the re-sorting backward still handles tiles whose log overflowed).  Results are the same sums in a
       different order.  Set it for training forwards; leave it 0 for inference. */
    int32_t record_blend_log;
    /* Replaces DebugVisualizationData::type (stopthepop/rasterizer_debug.h:11-21; rasterizer.h:203): 0 = disabled,
       STP_DEBUG_DEPTH = the depth visualisation the Python flag `render_depth` selects (rasterize_points.cu:104-107):
       the render kernels accumulate depth * alpha * T per pixel, the frame's minimum / maximum normalise it and the
       Turbo colormap turns it into the output image (forward.cu:674-729).  Forward only. */
    int32_t debug_visualization;
} StpSettings;

#define STP_DEBUG_DISABLED 0
#define STP_DEBUG_DEPTH 1

typedef enum StpStatus {
    STP_OK = 0,
    STP_ERR_INVALID_ARGUMENT = -1,
    STP_ERR_NEEDS_SCALE_ROTATION = -2,  /* sorted modes build Sigma^-1 from scales+rotations (forward.cu:208-220) */
    STP_ERR_QUEUE_SIZE = -3,            /* "Not supported head/mid queue size" (forward.cu:455-480, backward.cu:751-760) */
    STP_ERR_SORT_MODE = -4,
    STP_ERR_NO_BACKWARD = -5,           /* "Backward not supported for full per-pixel sort" (backward.cu:733-736) */
    STP_ERR_HIP = -6,                   /* a HIP runtime call or kernel failed; message has the detail */
    STP_ERR_ALLOC = -7,                 /* an allocator callback returned NULL */
    STP_ERR_PREFILTERED = -8            /* a point was culled although prefiltered was set (auxiliary.h:228-232) */
} StpStatus;

/* Replaces the three `std::function<char*(size_t)>` buffer-resize callbacks of Rasterizer::forward
   (rasterizer.h:196-198; rasterize_points.cu:33-41).  Must return a device pointer to at least
   `bytes` bytes, valid until the matching backward has run.
   geometry_alloc and image_alloc are called once per forward.  binning_alloc may be called TWICE: once before the
   num_rendered hand-over with a size guessed from the previous frame of the same kind on this device (P, resolution,
   tile-row window, sort mode; count + 12.5 %), and again with the exact -- larger -- size only when the guess was too
   small.  The SECOND block replaces the first (resize semantics, as the reference's callback has): an arena / bump
   allocator must be prepared to take the first block back, and the buffer it finally hands to stp_backward is the
   one of the LAST call.  A guessed request can exceed the exact size by up to 12.5 % (+ the change of num_rendered from
   frame to frame); STP_BINNING=exact in the environment restores the reference's single exact request. */
typedef void* (*stp_alloc_fn)(void* user, size_t bytes);

/* Replaces CudaRasterizer::Rasterizer::forward (rasterizer.h:195-220, rasterizer_impl.cu:221-413).
   Returns num_rendered (the number of (tile, Gaussian) duplicates) or a negative StpStatus.
   Contains exactly one host synchronisation (the read-back of num_rendered, as in
   rasterizer_impl.cu:317).  `radii` may be NULL (an internal array is used, rasterizer_impl.cu:259-262).
   `out_color` is (3,H,W), written for every pixel of the selected tile rows. */
int stp_forward(stp_alloc_fn geometry_alloc, void* geometry_user,
                stp_alloc_fn binning_alloc, void* binning_user,
                stp_alloc_fn image_alloc, void* image_user,
                int P, int D, int M,
                const float* background, int width, int height,
                const StpSettings* settings,
                const float* means3D, const float* shs, const float* colors_precomp,
                const float* opacities, const float* scales, float scale_modifier,
                const float* rotations, const float* cov3D_precomp,
                const float* viewmatrix, const float* projmatrix, const float* inv_viewprojmatrix,
                const float* cam_pos, float tan_fovx, float tan_fovy, int prefiltered,
                float* out_color, int* radii, int debug, void* stream);

/* Extension (not in the reference), for tile-row sharding: the NEXT stp_forward of the calling thread launches its render kernel twice -- tile
   rows [tile_y0, tile_row) first, then [tile_row, tile_y1) -- and records `event` (a hipEvent_t of the caller) on the stream between the two
   launches: when the event has fired, the pixel rows above 16 * tile_row are final, and a rank can put them on the wire while the rest of its
   strip is still being blended.  Same kernels and per-tile work as one launch: pixels, buffers and the backward are unchanged.  A tile_row
   outside (tile_y0, tile_y1), or a call that returns early, records the event behind everything the call enqueued.  event == NULL clears a
   pending request.  The request is consumed by the next stp_forward whatever its outcome. */
void stp_set_forward_split(int tile_row, void* event);

/* Replaces CudaRasterizer::Rasterizer::backward (rasterizer.h:222-257, rasterizer_impl.cu:417-526).
   geom/binning/image buffers are the ones the forward allocated; R is the forward's return value.
   grad_records must be zero-filled by the caller.  The dL_d* outputs need not be (the reference zero-fills them,
   rasterize_points.cu:178-186): every row of every output is written, zeros for Gaussians outside the frustum --
   except dL_dscale / dL_drot when cov3D_precomp is given (then they are left untouched, as in the reference).

   grad_records (P x STP_GRAD_RECORD_FLOATS floats) is the hand-over between the two halves of the backward.
   It takes the place of the reference's dL_dconic scratch tensor (rasterize_points.cu:181): the render half sums
   its nine per-Gaussian terms into ONE 64-byte record per Gaussian,
       [0..2] dL/dcolour rgb   [3..4] dL/dmean2D xy   [5..7] dL/dconic xx, xy, yy   [8] dL/dopacity
       [9..10] sum |dL/dmean2D| xy (only with the absgrad request)
       [11..13] sum, max, count of the blend weights (only with the blend-statistics request; the max as the float's bits)
       [14] dL/d(1/z) (only with the inverse-depth request)   [15] unused
   (one atomic instruction / one L2 request per flush instead of nine into four arrays: 9x the flush rate on
   MI355X, tools/global_atomic_bench.hip); the per-Gaussian half reads the record and writes dL_dmean2D,
   dL_dopacity and dL_dcolor in the reference's layouts along with the remaining gradients.
   OPTIONAL OUTPUTS: dL_dcolor and dL_dcov3D may be NULL -- "not wanted": the gradients of colors_precomp and cov3D_precomp, which a caller
   that renders from SH coefficients and scale / rotation has no receiver for.  The per-Gaussian half then skips those stores (24 + 12 bytes
   per Gaussian); every other output is what it is with them (dL_dscale / dL_drot are formed from dL_dcov3D in registers either way). */
int stp_backward(int P, int D, int M, int R,
                 const float* background, int width, int height,
                 const StpSettings* settings,
                 const float* means3D, const float* shs, const float* opacities, const float* colors_precomp,
                 const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                 const float* viewmatrix, const float* projmatrix, const float* inv_viewprojmatrix,
                 const float* cam_pos, float tan_fovx, float tan_fovy,
                 const float* pixel_colors, const int* radii,
                 char* geom_buffer, char* binning_buffer, char* image_buffer,
                 const float* dL_dpix,
                 float* dL_dmean2D /* P x 3 */, float* grad_records /* P x 16 */, float* dL_dopacity /* P */,
                 float* dL_dcolor /* P x 3 */, float* dL_dmean3D /* P x 3 */, float* dL_dcov3D /* P x 6 */,
                 float* dL_dsh /* P x M x 3 */, float* dL_dscale /* P x 3 */, float* dL_drot /* P x 4 */,
                 int debug, void* stream);

/* Extension (not in the reference): the two halves of the backward separately, for tile-row sharding.
   phases bit 0 = BACKWARD::render (rasterizer_impl.cu:474-495): accumulates the per-Gaussian partial
   sums of THIS rank's tile rows into grad_records (nothing else is written);
   phases bit 1 = BACKWARD::preprocess (rasterizer_impl.cu:501-525): consumes grad_records (after the
   caller has summed them across ranks) and writes every dL_d* output.  phases = 3 == stp_backward.
   phases bit 2 (value 4, with bit 0 and / or bit 1) = COMPACT records: grad_records is P x STP_GRAD_RECORD_USED floats (36 bytes per
   Gaussian, no padding) -- the buffer a tile-row shard all-reduces between the two halves crosses xGMI as it is, without a
   pack / unpack copy on either side.  (The padded 64-byte record is what a single GPU wants: one line, one atomic request per flush.)
   phases bit 3 (value 8, with bit 1) = the per-Gaussian half leaves grad_records ZERO-FILLED again: it reads every record the render
   half can have written (those of the visible Gaussians) and clears it behind the read, so that a caller who keeps the buffer between
   steps never zero-fills it after the first time (the fill is 64 B per Gaussian per step otherwise: 24 us at 1M, 0.14 ms at 6M).
   phases bits 8-15 = K, bits 16-23 = k (with bit 1 only): the per-Gaussian half on chunk k of K equal ranges of Gaussian ids (ranges of
   256-Gaussian blocks).  Gaussians are independent there, so a tile-row shard all-reduces its records in K pieces and runs chunk k as soon as
   piece k has arrived, while piece k + 1 is still on the links (tile_shard.py).  K <= 1: all Gaussians. */
int stp_backward_phases(int phases, int P, int D, int M, int R,
                        const float* background, int width, int height,
                        const StpSettings* settings,
                        const float* means3D, const float* shs, const float* opacities, const float* colors_precomp,
                        const float* scales, float scale_modifier, const float* rotations, const float* cov3D_precomp,
                        const float* viewmatrix, const float* projmatrix, const float* inv_viewprojmatrix,
                        const float* cam_pos, float tan_fovx, float tan_fovy,
                        const float* pixel_colors, const int* radii,
                        char* geom_buffer, char* binning_buffer, char* image_buffer,
                        const float* dL_dpix,
                        float* dL_dmean2D, float* grad_records, float* dL_dopacity, float* dL_dcolor,
                        float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale, float* dL_drot,
                        int debug, void* stream);

/* Extension (not in the reference): gradients with respect to the camera, for pose refinement and tracking.  The NEXT stp_backward or
   stp_backward_phases of the calling thread that runs the per-Gaussian half (phases bit 1) also writes
       dL_dviewmatrix (16 floats), dL_dprojmatrix (16 floats), dL_dcampos (3 floats)
   in full (device pointers; the caller does no zero-fill), in the matrix layout above: element [i][j] (p_view = [p 1] @ V) is m[4*i+j].
   The three inputs are differentiated as independent inputs, as the forward reads them (it never checks that projmatrix = viewmatrix @ P
   or that cam_pos is the camera centre); a caller who builds all three from one pose gets the total derivative by the chain rule.
   Differentiated: viewmatrix -> view-space mean -> the EWA Jacobian and the rotation of the covariance projection (with the same
   1.3 * tan_fov clamp masks and, under proper_ewa_scaling, the same opacity factor as dL_dmean3D), projmatrix -> the 2D mean, cam_pos ->
   the SH view direction (zero with colors_precomp).  They are sums over the visible Gaussians of the intermediates dL_dmean3D is made of.
   Not differentiated (zero by definition, as for the Gaussians): culling, the near plane, tile binning, every sort key and depth along the
   ray.  Entries the forward never reads are 0: column 3 of viewmatrix, column 2 of projmatrix.  inv_viewprojmatrix, tan_fovx / tan_fovy
   (the intrinsics) and the background get no gradient.
   `workspace` is a 16-byte aligned device buffer of at least stp_camera_grad_workspace_bytes(P) bytes, used until the call's kernels have
   run.  The sums run in a fixed order without float atomics: equal per-Gaussian gradients give bit-equal camera gradients.  Every other output
   of the call is bit-identical to that of a call without the request.
   A NULL output pointer clears a pending request.  STP_ERR_INVALID_ARGUMENT: a workspace that is too small or misaligned, or a chunked
   per-Gaussian half (phases bits 8-23).  The request is consumed by that call whatever its outcome; a render-only call (phases = 1) leaves
   it pending. */
size_t stp_camera_grad_workspace_bytes(int P);
void stp_set_backward_camera_grads(float* dL_dviewmatrix, float* dL_dprojmatrix, float* dL_dcampos, void* workspace, size_t workspace_bytes);

/* Extension (not in the reference): absolute screen-space gradients ("absgrad", the densification statistic of AbsGS / gsplat).  The NEXT
   stp_backward or stp_backward_phases of the calling thread also produces, for every Gaussian i,
       dL_dmean2D_abs[3 i], [3 i + 1] = sum over pixels p of |g_x,p(i)|, |g_y,p(i)|      dL_dmean2D_abs[3 i + 2] = 0
   where g_p(i) is what pixel p adds to dL_dmean2D[i] (the factors 0.5 W, 0.5 H included): dL_dmean2D is the signed sum of the same terms
   over the same (pixel, Gaussian) pairs, so dL_dmean2D_abs >= |dL_dmean2D| elementwise up to rounding, with equality where a Gaussian
   receives one contribution.  Every row is written (device pointer, P x 3 floats, no zero-fill by the caller): zeros for Gaussians with
   radii <= 0.  The render half takes the absolute values per blended pair, before anything is summed, and adds them to slots
   STP_GRAD_RECORD_ABS, + 1 of the Gaussian's padded record (the same atomic request as the nine sums); the per-Gaussian half moves them to
   dL_dmean2D_abs before it reads -- and, with phases bit 3, clears -- the record (the cleared 48 bytes include both slots).  Every other
   output of the call is what it is without the request, up to the run-to-run variation of the render half's float atomics.
   A NULL pointer clears a pending request.  The request is consumed by the next stp_backward / stp_backward_phases of the thread, whatever
   that call's outcome -- a call that fails, or that has nothing to do (P == 0), leaves no pointer behind -- with one exception: a render-only
   call (phases = 1) that SUCCEEDS honours it -- the sums stay in slots 9, 10 of the records it fills -- and leaves it pending for the
   per-Gaussian call, which must then get those records.  STP_ERR_INVALID_ARGUMENT: compact records (phases bit 2: 36 bytes per Gaussian have no room for the
   two sums), or a chunked per-Gaussian half (phases bits 8-23: REFUSED, as camera gradients are -- one request is one whole per-Gaussian
   half). */
void stp_set_backward_absgrad(float* dL_dmean2D_abs /* P x 3 */);

/* Extension (not in the reference): per-Gaussian blend statistics, what pruning and compaction methods rank Gaussians by.  The blend weight
   of a (pixel, Gaussian) pair is w = alpha * T, T the transmittance in front of the blend: the share of the pixel's colour that comes from
   that Gaussian.  The NEXT stp_backward or stp_backward_phases of the calling thread also produces, for every Gaussian i,
       blend_stats[3 i]     = sum over pixels of w     (Mini-Splatting, Taming-3DGS)
       blend_stats[3 i + 1] = max over pixels of w     (RadSplat)
       blend_stats[3 i + 2] = number of pixels that blended it, as a float (LightGaussian; exact: a frame has fewer than 2^24 pixels)
   over exactly the (pixel, Gaussian) pairs the forward blended, which are the pairs whose nine gradient terms the call adds: alpha >=
   1/255, not the entry that saturates the pixel.  (The replay kernel's gradient terms may leave a pixel one pair early where its
   transmittance sits on the saturation threshold to an ulp; the statistics follow the forward's blend log, so that both backward modes
   count the same pairs.)  The values do not depend on dL_dpix (all-zero or non-finite pixel gradients give the same statistics).  Every row is written
   (device pointer, P x 3 floats, no zero-fill by the caller): zeros for Gaussians with radii <= 0.  The render half adds the three terms
   per blended pair to slots STP_GRAD_RECORD_STATS .. + 2 of the Gaussian's padded record -- sum and count with float adds, the maximum
   with an unsigned integer maximum on the float's bits (w >= 0, the record starts zeroed) --; the per-Gaussian half moves them to
   blend_stats before it reads the record and, with phases bit 3, zeroes the three slots behind its read (the 48 bytes that bit clears
   end in front of slots 12, 13).  Every other output of the call is what it is without the request, up to the run-to-run variation of
   the render half's float atomics.  Independent of stp_set_backward_absgrad; both requests may be pending for one call.
   A NULL pointer clears a pending request.  Consumed like the absgrad request: by the next stp_backward / stp_backward_phases of the
   thread whatever its outcome, except that a render-only call (phases = 1) that succeeds honours it and leaves it pending for the
   per-Gaussian call, which must then get those records.  STP_ERR_INVALID_ARGUMENT: compact records (phases bit 2: the 36-byte record
   has no room for the three terms), or a chunked per-Gaussian half (phases bits 8-23). */
void stp_set_backward_blend_stats(float* blend_stats /* P x 3 */);

/* Extension (not in the reference): alpha output, per-pixel background and background gradients.  Every forward keeps final_T, the
   transmittance behind a pixel's last blend; the image is  out[ch, p] = C[ch, p] + final_T[p] * background[ch].
   stp_set_forward_background -- the NEXT stp_forward of the calling thread
       with bg_image  (3 x H x W floats): composes  out[ch, p] = C[ch, p] + final_T[p] * bg_image[ch, p]  instead; `background` is not read
                      by the render kernels (it must still be a valid pointer).  The expression is the uniform one's: a bg_image filled with
                      one colour gives the image of that `background` bit for bit;
       with out_alpha (H x W floats): also writes  out_alpha[p] = 1 - final_T[p]  (0 for a pixel nothing blended into).
   Every sort mode, PPX_FULL included; both launches of a split forward (stp_set_forward_split) and a redone run-ahead frame honour it.  The
   request costs a wave-uniform branch per pixel in the kernels' epilogues; nothing else of the forward changes, and without a request the
   forward is what it was.  P == 0 launches nothing: the caller's image and alpha stand.  STP_ERR_INVALID_ARGUMENT with
   StpSettings::debug_visualization = STP_DEBUG_DEPTH (that image is not C + T * background).
   stp_set_backward_background -- the NEXT stp_backward / stp_backward_phases of the calling thread that runs the render half (phases bit 0)
       with bg_image       : the forward's per-pixel background (it MUST be given when the forward had one: final_T's weight in the loss and
                             the colour behind each blend are formed from it), or NULL for a uniform `background`;
       with dL_dalpha      (H x W floats): the gradient of the loss with respect to out_alpha.  The pixel prologues of the render half use
                             dL/dfinal_T[p] = sum_ch B[ch, p] * dL_dpix[ch, p] - dL_dalpha[p]   (B = bg_image, or background[ch] for every p)
                             where they used the first term; the nine per-Gaussian sums are otherwise formed as before.  A backward through
                             alpha alone passes an all-zero dL_dpix;
       with dL_dbackground : receives dL/dB[ch, p] = final_T[p] * dL_dpix[ch, p] -- 3 x H x W floats when bg_image is given, otherwise its
                             sum over the pixels, 3 floats.  Written in full (no zero-fill by the caller; zeros for P == 0).  The sum
                             runs in a fixed order without float atomics, like the camera gradients: equal inputs give bit-equal results.
   All buffers are full-frame device buffers indexed by absolute pixel (W * y + x).  With a tile-row window (StpSettings::tile_y0 / tile_y1)
   only the window's pixel rows are read or written, and the uniform sum covers the window's rows.  Nothing of the request lives in the
   gradient records: compact records (phases bit 2) and a chunked per-Gaussian half are fine, and so are camera gradients, absgrad and blend
   statistics in the same call.  No backward for PPX_FULL, as without the request.
   Both requests are per thread and one-shot.  Any pointer may be NULL; all NULL clears a pending request.  The forward request is consumed
   by the next stp_forward of the thread whatever that call's outcome (an invalid argument or P == 0 included).  The backward request is
   consumed by the next stp_backward / stp_backward_phases of the thread WITH phases bit 0, whatever its outcome; a per-Gaussian-only call
   (phases = 2) neither honours nor consumes it. */
void stp_set_forward_background(const float* bg_image /* 3 x H x W */, float* out_alpha /* H x W */);
void stp_set_backward_background(const float* bg_image /* the forward's, or NULL */, const float* dL_dalpha /* H x W, or NULL */,
                                 float* dL_dbackground /* 3, or 3 x H x W when bg_image is given; or NULL */);

/* Extension (the `invdepths` output of the official 3DGS rasterizer, gsplat's RGB+ED): a differentiable inverse-depth image.
       invdepth[p] = sum_i w_i(p) / z_i,   w_i(p) = alpha_i(p) * T_i(p)
   over exactly the (pixel, Gaussian) pairs the forward blends for the colour, in the same order with the same weights.  z_i is the
   view-space z of Gaussian i's centre -- the value the near test compares with 0.2; not the sort key `depths`, not the depth along the
   pixel's ray --, 1 / z_i one IEEE division per Gaussian in the preprocess kernel (kept in the geometry buffer, sub-array "invz", for
   the backward).  No background term, no division by alpha: 0 where nothing blended.  Mathematically a fourth colour channel with a zero
   background.
   stp_set_forward_invdepth -- the NEXT stp_forward of the calling thread also writes out_invdepth (H x W floats).  Every sort mode
       (PPX_FULL forward only, as always); the render kernels are compile-time variants of their own (four accumulators), the kernels
       of a forward without the request are what they were.  Both launches of a split forward and a redone run-ahead frame honour it.
       P == 0 launches nothing: the caller's buffer stands.  STP_ERR_INVALID_ARGUMENT with StpSettings::debug_visualization =
       STP_DEBUG_DEPTH.  Consumed by the next stp_forward of the thread whatever its outcome; NULL clears a pending request.
   stp_set_backward_invdepth -- the NEXT stp_backward / stp_backward_phases of the calling thread treats (1 / z_i, invdepth, dL_dinvdepth)
       as a fourth channel of the render half's dL/dalpha sums -- the gradient reaches means2D, conics and opacities like a colour
       gradient's -- and sums alpha * T * dL_dinvdepth per Gaussian into slot STP_GRAD_RECORD_INVDEPTH of its padded record; the
       per-Gaussian half adds -slot / z_i^2 to dL/dt_z in front of dL_dmean3D and the camera gradients' partial sums (every visible
       Gaussian, whatever its covariance path), and with phases bit 3 clears the slot behind its read.  dL_dcolor / dL_dsh get nothing
       from it.  `invdepth` is the forward's output, `dL_dinvdepth` the loss gradient with respect to it (both H x W).  A backward
       through invdepth alone passes an all-zero dL_dpix.
   All three buffers are full-frame device buffers indexed by absolute pixel (W * y + x); with a tile-row window only the window's rows
   are read or written.  The backward request is taken by the next stp_backward / stp_backward_phases of the thread whatever its
   outcome, with the absgrad request's one exception: a render-only call (phases = 1) that succeeds leaves it pending for the
   per-Gaussian call, which must then get those records.  Both pointers NULL clears a pending request.  STP_ERR_INVALID_ARGUMENT: only
   one of the two pointers, compact records (phases bit 2: the 36-byte record has no slot 14), or a chunked per-Gaussian half (phases
   bits 8-23: REFUSED, as absgrad is).  Independent of the camera, absgrad, blend-statistics and background requests. */
void stp_set_forward_invdepth(float* out_invdepth /* H x W */);
void stp_set_backward_invdepth(const float* invdepth /* the forward's, H x W */, const float* dL_dinvdepth /* H x W */);

/* Extension (the `dc` / `shs` pair of the official 3DGS rasterizer's accelerated branch): SH coefficients as the two tensors a trainer keeps
   them in -- `dc`, the (P, 3) first coefficient (a trainer's _features_dc), and the (P, M-1, 3) rest (_features_rest) -- without a
   concatenated (P, M, 3) copy going in or a full-size dL_dsh coming out.  M stays the TOTAL number of coefficients per Gaussian.
   stp_set_forward_split_sh -- the NEXT stp_forward of the calling thread reads coefficient 0 of Gaussian i at dc + 3 i and coefficients
       1 .. M-1 at shs + 3 (M-1) i: `shs` is the rest.  With M == 1 `shs` is not read and may be NULL.
   stp_set_backward_split_sh -- the NEXT stp_backward / stp_backward_phases of the calling thread that runs the per-Gaussian half (phases
       bit 1) reads the coefficients the same way and writes dL_ddc (P x 3) and dL_dsh as P x (M-1) x 3 (not written, may be NULL, for
       M == 1).  Both are written in full, zeros for Gaussians with radii <= 0, as dL_dsh is.  A chunked per-Gaussian half (phases bits
       8-23) is fine: every chunk writes its own rows of both.
   Only the SH kernels' staging between global memory and LDS differs (two source / destination spans per workgroup instead of one); the
   arithmetic reads the same values, so every output of a call with the request -- the image, radii, num_rendered, all gradients, dL_ddc
   and dL_dsh against the two slices of the concatenated call's dL_dsh -- is bit-identical to that of a call on the concatenated tensor.
   The pointers need only the 4-byte alignment of their element type (rows 1.. of a larger tensor are fine): 16-byte aligned ones are
   moved 16 bytes per lane, others one float at a time.  With colors_precomp given the precomputed colours win, as without the request:
   no SH coefficient is read and the backward writes neither SH gradient.
   A NULL dc clears a pending request.  The forward request is consumed by the next stp_forward of the thread whatever its outcome; the
   backward request by the next backward with phases bit 1, whatever its outcome -- a render-only call (phases = 1) leaves it pending, as
   it does the camera request.  STP_ERR_INVALID_ARGUMENT: a backward request without dL_ddc, or M > 1 with a NULL shs / dL_dsh. */
void stp_set_forward_split_sh(const float* dc /* P x 3 */);
void stp_set_backward_split_sh(const float* dc /* P x 3 */, float* dL_ddc /* P x 3 */);

/* Extension: the SH stash.  The per-Gaussian half of the backward needs the SH coefficients of a Gaussian (192 B at degree 3) for nine
   numbers only: the derivative of each colour channel with respect to the unit view direction.  They depend on the coefficients, the mean
   and the camera position -- all of which the forward's SH -> RGB kernel holds -- and on nothing the backward adds.
   stp_set_forward_sh_stash(1) -- the NEXT stp_forward of the calling thread, if it evaluates SH colours (shs or a split dc given, M > 0, no
       colors_precomp), also writes those nine floats per visible Gaussian into one more sub-array at the END of its geometry buffer -- nine
       planes of P floats, "sh_stash" of stp_geometry_layout, plane 3 c + {0, 1, 2} = d(channel c) / d(direction x, y, z) -- and asks
       geometry_alloc for stp_geometry_buffer_size_stash(P, settings) bytes: 36 P more (rounded up to the carve's alignment); no other
       offset moves.  A forward that does not ask, or has no SH colours to evaluate, writes and allocates nothing new and runs the kernels it
       always ran.  Consumed by the next stp_forward of the thread whatever its outcome; 0 clears a pending request.
   The backward needs no request: the buffer says whether it carries a stash (three words of its first 256 bytes: a magic, P, ~P, written by
   the stashing kernel; the library also remembers it per buffer address, like the binning layout, and stp_forget_buffer forgets it), and a
   per-Gaussian half handed one reads it in the place of the SH rows -- 36 B for 192 B per visible Gaussian.  A buffer without one (no
   request, a forward of an older library) takes the path it always took.  A call with a camera request still reads the SH rows for its
   camera terms (dL_dcampos is a function of the nine numbers).  The stashed values are formed by the backward's own expressions, compiled
   with the backward's contraction setting: every gradient is the legacy path's bit for bit except dL_dmean3D above SH degree 1, which is
   within 3.5e-8 of its largest entry of it (the two kernels fuse the shared expressions differently; against a float64 evaluation both
   paths have the same error: tests/test_gpu_sh_stash.py).  The image, radii, colours and clamp flags of the forward do not change. */
void stp_set_forward_sh_stash(int enable);

/* Extension: raw parameter inputs.  A 3DGS-family trainer stores a Gaussian as _scaling (the logarithm of the scale), _rotation (an
   unnormalised quaternion) and _opacity (a logit) and runs exp, normalize and sigmoid in front of every render.  With these requests the two
   kernels that read `scales`, `rotations` and `opacities` apply the activation at the load and its chain rule at the store; no activated
   copy exists anywhere.  `mask`: bit 0 = opacities, bit 1 = scales, bit 2 = rotations hold raw values.  In float32, every step but expf one
   correctly rounded operation (csrc/stp_activations.h):
       o = 1 / (1 + expf(-x))          s = expf(x), scale_modifier * s follows unchanged          q / max(|q|, 1e-12f)
       |q| = sqrt(fma(q3, q3, fma(q2, q2, fma(q1, q1, q0 * q0))))    (torch.sigmoid, torch.exp, torch.nn.functional.normalize with its eps)
   stp_set_forward_raw_params -- the NEXT stp_forward of the calling thread reads the arrays of the mask as raw.  Every output is that of the
       plain call on stp_activate_params' copies, bit for bit.  With cov3D_precomp AND scales and rotations given the bits apply wherever
       the library reads the two arrays (Sigma^-1 of the sorted modes).
   stp_set_backward_raw_params -- the NEXT stp_backward / stp_backward_phases of the calling thread that runs the per-Gaussian half (phases
       bit 1) reads them as raw and writes the gradients with respect to the RAW values -- what autograd gives for the activations composed
       in front of the plain call, that call's conventions included (dL_dscale stays the derivative with respect to scale_modifier * s):
           dL_dopacity_raw = dL_dopacity o (1 - o)      dL_dscale_raw = dL_dscale s      dL_drot_raw = (g - qh (qh . g)) / |q|, qh = q / |q|,
       g the plain call's dL_drot; where |q| < 1e-12f the norm took no part: g / 1e-12f.  Rows with radii <= 0 get zeros.  Works with compact
       and padded records and in every chunk of a chunked half (each chunk is a call and carries its own request).  Without
       proper_ewa_scaling bit 0 makes the half read opacities (4 B per Gaussian), which it otherwise does not.
   Both requests are consumed by the call they are meant for whatever its outcome; a render-only backward (phases = 1) leaves the backward
   request pending, as it does the camera request.  Mask 0 clears a pending request: the call is the plain one, launch for launch and bit for
   bit.  STP_ERR_INVALID_ARGUMENT, before anything is launched, with a message naming the bit: a mask outside 0..7, or a bit whose array is
   NULL in that call.
   stp_activate_params -- the activated copies themselves (logging, export, tests): scales[3 P] from scaling, rotations[4 P] from rotation,
       opacities[P] from opacity, the values the raw path renders with to the bit.  Any of the three pairs may be NULL together.  One launch
       per pair; 16-byte aligned pairs move 16 bytes per lane.  Returns the launches made (0 for P == 0 or no pair), or a negative StpStatus:
       a negative P, P >= 2^29, or a pair with only one pointer. */
void stp_set_forward_raw_params(int mask);
void stp_set_backward_raw_params(int mask);
int stp_activate_params(int P, const float* scaling, const float* rotation, const float* opacity, float* scales, float* rotations,
                        float* opacities, void* stream);

/* Replaces CudaRasterizer::Rasterizer::markVisible (rasterizer.h:188-193, rasterizer_impl.cu:161-173).
   `present` is P bytes (bool). */
int stp_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                     uint8_t* present, void* stream);

/* Extension (not in the reference): the fused sparse Adam step of 3DGS trainers (the SparseGaussianAdam of the accelerated rasterizer, a
   trainer's --optimizer_type sparse_adam).  Tensor k holds numel_k = N * M_k floats, row i (M_k consecutive floats) belonging to Gaussian i.
   For every tensor, every row i < N that is visible and every element of it, in float32:
       m <- beta1 * m + (1 - beta1) * g      v <- beta2 * v + (1 - beta2) * g * g      p <- p - lr * m / (sqrt(v) + eps)
   with 1 - beta formed in float32; no bias correction, no weight decay, no amsgrad.  Elements of invisible rows keep param, exp_avg and
   exp_avg_sq bit for bit and their grad is never used (a NaN there changes nothing); non-finite gradients of visible rows propagate as the
   expressions say.  `visible` is a device pointer read as it is: visible_kind 0 = N bytes (bool / uint8), non-zero = visible;
   visible_kind 1 = N int32 (the radii a forward returned), > 0 = visible.  lr and eps are per tensor.  All pointers are device pointers to
   contiguous float32 data; 16-byte aligned ones are streamed 16 bytes per lane, others one float at a time.  One kernel launch updates up
   to eight tensors (more tensors: further launches), without atomics: equal inputs give equal bits.
   Returns the number of kernel launches made (>= 0; 0 for N == 0, n_tensors == 0 or all numel == 0), or a negative StpStatus with the
   reason in the last-error text.  Refused BEFORE anything is launched, so that nothing is half updated (STP_ERR_INVALID_ARGUMENT): a negative
   count, a numel that N does not divide, numel >= 2^31, a null pointer of a tensor with elements or a null `visible`, an unknown
   visible_kind.  A plain call: no host synchronisation, no allocation, no per-thread request state.  lr travels in the kernel arguments: a step
   captured in a graph replays the lr it was captured with. */
typedef struct { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; long long numel; float lr, eps; } StpAdamTensor;
int stp_sparse_adam(int n_tensors, const StpAdamTensor* tensors, int N, const void* visible, int visible_kind /* 0: N bytes, non-zero = visible; 1: N int32, > 0 = visible */,
                    float beta1, float beta2, void* stream);

/* Extension (not in the reference): the fused DENSE Adam step -- the bias-corrected torch.optim.Adam(lr, betas, eps) that the 3DGS trainer
   (optimizer_type "default") and every 3DGS-MCMC trainer construct -- with the two 3DGS-MCMC regularisers' gradients folded in.  For every
   tensor and every one of its numel elements, in float32:
       g' = g + r      r = 0 (reg_kind 0),   reg_coef * (s * (1 - s)) with s = 1 / (1 + exp(-p)) (reg_kind 1, "sigmoid"),
                       reg_coef * exp(p) (reg_kind 2, "exp")
       m <- beta1 * m + one_minus_beta1 * g'      v <- beta2 * v + one_minus_beta2 * g' * g'
       p <- p - (step_size * m) / (sqrt(v) / bias2_sqrt + eps)
   p in r is the value BEFORE the step.  reg_kind 1 with reg_coef = w / numel is the gradient of w * mean(sigmoid(p)), reg_kind 2 that of
   w * mean(exp(p)): a 3DGS-MCMC trainer's opacity_reg and scale_reg terms.  The CALLER forms every coefficient, as torch does: in float64
   from the unrounded hyper-parameters -- one_minus_beta = 1 - beta, step_size = lr / (1 - beta1^t), bias2_sqrt = sqrt(1 - beta2^t) with t the
   step count after this step -- rounded to float32 once; they travel per tensor, so tensors may disagree in all of them.  No weight decay, no
   amsgrad, no maximize; the regulariser's VALUE is not computed.  grad is only read.  All pointers are device pointers to contiguous float32
   data; 16-byte aligned ones are streamed 16 bytes per lane, others one float at a time, with equal bits.  One kernel launch updates up to
   eight tensors (more tensors: further launches), without atomics: equal inputs give equal bits.
   Returns the number of kernel launches made (>= 0; 0 for n_tensors == 0 or all numel == 0), or a negative StpStatus with the reason in the
   last-error text.  Refused BEFORE anything is launched, so that nothing is half updated (STP_ERR_INVALID_ARGUMENT): a negative count, a null
   table, a negative numel, numel >= 2^31, a reg_kind outside {0, 1, 2}, a bias2_sqrt that is not finite and positive, a null pointer of a
   tensor with elements.  A plain call: no host synchronisation, no allocation, no per-thread request state.  The coefficients travel in the
   kernel arguments: a step captured in a graph replays the step count it was captured with. */
typedef struct { float* param; const float* grad; float* exp_avg; float* exp_avg_sq; long long numel;
                 float beta1, one_minus_beta1, beta2, one_minus_beta2, step_size, bias2_sqrt, eps; int32_t reg_kind; float reg_coef; } StpDenseAdamTensor;
int stp_dense_adam(int n_tensors, const StpDenseAdamTensor* tensors, void* stream);

/* Extension (not in the reference): the two kernels of a 3DGS-MCMC trainer ("3D Gaussian Splatting as Markov Chain Monte Carlo").
   stp_mcmc_relocation is that project's compute_relocation: Gaussian i of opacity o and scales s, to be replaced by N_i copies of itself, gets
       o_new = 1 - (1 - o)^(1/N)     denom = sum_{j=1..N} sum_{k=0..j-1} C(j-1, k) (-1)^k o_new^(k+1) / sqrt(k+1)     s_new = (o / denom) s
   with N_i clamped to [1, n_max - 1] (the inputs are not modified).  The sum is evaluated in float64 in its collapsed form
   sum_{k=0..N-1} C(N, k+1) (-1)^k o_new^(k+1) / sqrt(k+1), o_new as -expm1(log1p(-o) / N); the results are rounded to float32 once.
   opacity_old, opacity_new: n floats; scale_old, scale_new: n x 3 floats; N: n int32 (n_kind 0) or n int64 (n_kind 1), naturally aligned.
   stp_mcmc_add_noise is the trainer's per-iteration position noise in one pass, in place on xyz:
       o = raw ? sigmoid(opacities[i]) : opacities[i]      s = raw ? exp(scales[i]) : scales[i]      q = rotations[i] / |rotations[i]|  (w, x, y, z)
       g = 1 / (1 + exp(-k ((1 - o) - x0)))                xyz[i] += R(q) diag(s^2) R(q)^T (noise[i] * g * noise_scale)
   in float32 IEEE arithmetic: a gate whose exp overflows is 0, a zero quaternion gives NaN in its own row only.  xyz, scales, noise: P x 3
   floats; rotations: P x 4; opacities: P.  Where all five pointers are 16-byte aligned the streams move 16 bytes per lane, otherwise one float
   per access; the arithmetic is the same.  No atomics: equal inputs give equal bits.
   Each call returns the number of kernel launches made (1; 0 for n == 0 / P == 0: nothing is touched), or a negative StpStatus with the reason
   in the last-error text.  Refused BEFORE anything is launched (STP_ERR_INVALID_ARGUMENT): a negative count, an n_kind other than 0 or 1, an
   n_max outside [2, 51], a raw other than 0 or 1, a null pointer.  Plain calls: no host synchronisation, no allocation, no per-thread request
   state.  All pointers are device pointers to contiguous data. */
int stp_mcmc_relocation(int n, const float* opacity_old, const float* scale_old, const void* N, int n_kind /* 0: int32, 1: int64 */, int n_max,
                        float* opacity_new, float* scale_new, void* stream);
int stp_mcmc_add_noise(int P, float* xyz, const float* scales, const float* rotations, const float* opacities, const float* noise,
                       float noise_scale, float k, float x0, int raw, void* stream);

/* Extension (not in the reference): Mip-Splatting's 3D smoothing filter ("Mip-Splatting: Alias-free 3D Gaussian Splatting"), the half of that
   method that lives outside the rasterizer (the 2D filter is proper_ewa_scaling).
   stp_mip_filter_3d is that project's compute_3D_filter over all C training cameras in one pass.  xyz: P x 3 floats; world_view_transforms:
   C x 16 floats, camera c's world-view matrix M in row-vector layout, p_cam = [p, 1] @ M (only M[:3, :3] and M[3, :3] are read); intrinsics:
   C x 4 floats (focal_x, focal_y, image_width, image_height); filter_3d: P floats; workspace: 4 bytes of device memory, 4-byte aligned, the
   call's own until the kernels have run.  With (x, y, z) = p_cam, for every Gaussian i and camera c:
       valid = z > 0.2  and  -0.15 W <= x / max(z, 0.001) * focal_x + W / 2 <= 1.15 W  and  -0.15 H <= y / max(z, 0.001) * focal_y + H / 2 <= 1.15 H
       distance[i] = min over the valid cameras of z (100000 before any)
   a row without a valid camera takes the largest distance of the rows that have one; where no row has one, every row keeps 100000 (upstream
   raises there: that needs a read-back, which this call never does).  filter_3d = distance / max_c(focal_x) * sqrt(0.2), the maximum over ALL
   cameras.  In float32, p_cam by a fixed chain of fmas and the screen test in its division-free form |x focal_x| <= (0.65 W) z
   (csrc/stp_mip_filter.hip); on inputs 1e-4 (relative to 0.2, W and H) away from every threshold each decision is that of a float64
   evaluation.  A NaN coordinate is never valid.  The maximum over rows is an integer maximum on the floats' bits: equal inputs give equal bits.
   Two kernel launches behind a 4-byte fill.
   stp_mip_activations_forward / _backward are get_scaling_with_3D_filter and get_opacity_with_3D_filter and their chain rule, one kernel each.
   scaling: P x 3 stored log-scales; opacity: P stored logits; filter_3d: P.  With e_j = exp(scaling_j), f = filter_3d, sig = 1 / (1 + exp(-opacity)):
       scales_j = sqrt(e_j^2 + f^2)      r_j = e_j^2 / (e_j^2 + f^2)      opacities = sig * sqrt(r_0 r_1 r_2)
       grad_scaling_j = grad_scales_j * e_j^2 / scales_j + grad_opacities * opacities * (1 - r_j)
       grad_opacity   = grad_opacities * sqrt(r_0 r_1 r_2) * sig * (1 - sig)
   (upstream's sqrt(prod e^2 / prod (e^2 + f^2)) without the two determinants, which leave the normal range for small scales).  The backward
   recomputes from the three inputs; grad_scales (P x 3) or grad_opacities (P) may be NULL and then counts as zero; filter_3d gets no gradient.
   Where all pointers are 16-byte aligned the streams move 16 bytes per lane, otherwise one float per access; the arithmetic is the same.
   No atomics: equal inputs give equal bits.
   Each call returns the number of kernel launches made (2, 1, 1; 0 for P == 0: nothing is touched), or a negative StpStatus with the reason in
   the last-error text.  Refused BEFORE anything is launched (STP_ERR_INVALID_ARGUMENT): a negative count, C == 0, C >= 2^24, a null pointer
   (but the two optional gradients; both NULL is refused).  Plain calls: no host synchronisation, no allocation, no per-thread request state.
   All pointers are device pointers to contiguous data. */
int stp_mip_filter_3d(int P, int C, const float* xyz, const float* world_view_transforms, const float* intrinsics, void* workspace, float* filter_3d,
                      void* stream);
int stp_mip_activations_forward(int P, const float* scaling, const float* opacity, const float* filter_3d, float* scales, float* opacities, void* stream);
int stp_mip_activations_backward(int P, const float* scaling, const float* opacity, const float* filter_3d, const float* grad_scales,
                                 const float* grad_opacities, float* grad_scaling, float* grad_opacity, void* stream);

/* Extension (not in the reference): the rest of a 3DGS-MCMC trainer's relocate_gs and add_new_gs around stp_mcmc_relocation -- the multinomial
   draw of the sources and the rewrite of every parameter and both Adam moments -- in three calls.  All tensors are float32, all pointers are
   device pointers to contiguous data, every call runs on the caller's stream, allocates nothing and NEVER synchronises with the host; no float
   atomics: equal inputs (the uniforms included) give equal bits.  o below is the opacity: opacity[i] itself, or 1 / (1 + expf(-opacity[i]))
   where raw (the evaluation of stp_mcmc_add_noise).
   stp_mcmc_sample draws sources with probability proportional to opacity by an inverse CDF over INTEGER weights:
       w_i = rint(min(max(o_i, 0), 1) * 2^24) for a candidate row (round to nearest even), 0 for any other      S_i = w_0 + ... + w_i  (64-bit: exact)
       u clamped into [0, 1) (NaN, negatives: 0; >= 1: the largest float32 below 1)         t = min(total - 1, (uint64) ((double) u * (double) total))
       the source of a draw = the smallest k with S_k > t  (never a row of weight 0)         count[k] = the number of draws that chose k
     rule 0 (relocation): the candidates are the rows with o > min_opacity; n_draws must be P, draw i is row i's (it reads uniforms[i]) and is
       made only where o_i <= min_opacity (a dead row); src[i] = -1 for every other row.  A NaN opacity is neither dead nor a candidate.
     rule 1 (growth): every row whose opacity is a number is a candidate; draw j < n_draws reads uniforms[j] and writes src[j]; min_opacity
       is not read.
     A total weight of 0 (or no dead row) leaves every src -1 and every count 0: decided on the device.  The quantisation of the weights
     moves w_i by at most half a unit, that is 2^-25 of the largest weight: a probability o_i / sum(o) moves by at most 2^-25 / o_i relative
     (opacities of 0.5 and above are exact; one of 2^-25 or below has weight 0 and is never drawn).
     weights (P uint32) may be null; src: n_draws int32; count: P int32 (cleared by the call).  The uniforms are the caller's (torch.rand).
   stp_mcmc_relocate_apply, IN PLACE, by a (src, count) pair of rule 0: with (o', s') = stp_mcmc_relocation's results for (o_k, s_k,
       N = min(count[k] + 1, 50)), o' = min(max(o', min_opacity), 1 - 2^-23), stored as they are or, where raw, as logf(o' / (1 - o')) and logf(s')
       (s_k = expf(scaling[k]) then):
     a row k with count[k] > 0 takes (o', s') in the tensors of role 1 (opacity, row 1) and 2 (scaling, row 3), keeps every other parameter
       and gets +0.0 in both moments of every tensor;
     a row i with count[i] <= 0 and src[i] in [0, P) takes row src[i] of every tensor, with that row's (o', s') in the role-1 and role-2
       tensors; its moments keep their bits, or are +0.0 where reset_dead_moments;
     every other row, and every other float, keeps its bits.  The new (o', s') are computed per source into the scratch before anything is
     written, so the result does not depend on the order in which rows are rewritten.  The pair must come from stp_mcmc_sample
     (count == the histogram of src, no src on a row that draws); a src outside [0, P) is treated as -1.
   stp_mcmc_add_apply, OUT OF PLACE, by a (src, count) pair of rule 1 with n_new draws, into P + n_new output rows: row r < P is row r with its
     moments, except that a row with count[r] > 0 takes (o', s') and +0.0 moments; row P + j is row src[j] with that row's (o', s') and +0.0
     moments (a src outside [0, P) -- a model without any weight -- gives a row of +0.0).  Inputs are not modified; outputs must not overlap
     inputs.  n_new is a host number (a trainer knows it from P and its cap): no read-back.
   Each entry: row = floats per Gaussian, exp_avg and exp_avg_sq both given or both null (then nothing is done for moments); the *_out
   pointers are read by stp_mcmc_add_apply only.  A tensor whose rows are multiples of 16 bytes and whose pointers are all 16-byte aligned
   moves 16 bytes per lane, others one float at a time, with equal bits.  Up to eight entries go in one launch.
   scratch: stp_mcmc_relocate_scratch_bytes(P) bytes (a function of P alone: max(8 (P + tiles + 4), 16 P) rounded up to 256, with tiles =
   ceil(P / STP_MCMC_SAMPLE_TILE); 0 for a P the calls refuse), 16-byte aligned; one buffer serves a sample and the apply that follows it.
   The three calls return the number of kernel launches made (0 for P == 0: nothing is touched), or a negative StpStatus with the reason in
   the last-error text.  Refused BEFORE anything is launched (STP_ERR_INVALID_ARGUMENT): a negative count, P > 2^28 (the total weight must
   stay below 2^53), a raw outside {0, 1}, an unknown rule, n_draws != P under rule 0, null pointers (of anything that would be read or
   written), a scratch that is too small or not 16-byte aligned; and by the applies: more than 64 entries, row <= 0 or (written rows) * row >=
   2^31, an unknown role, one moment pointer without the other, a role-1 tensor whose row is not 1 or a role-2 tensor whose row is not 3,
   and anything but exactly one entry of each of the roles 1 and 2. */
#define STP_MCMC_SAMPLE_TILE 2048
typedef struct { float *param, *exp_avg, *exp_avg_sq; float *param_out, *exp_avg_out, *exp_avg_sq_out; int32_t row; int32_t role; } StpMcmcTensor;
size_t stp_mcmc_relocate_scratch_bytes(int P);
int stp_mcmc_sample(int P, const float* opacity, int rule /* 0: relocation, 1: growth */, float min_opacity, int raw, int n_draws, const float* uniforms,
                    void* scratch, size_t scratch_bytes, uint32_t* weights /* may be null */, int32_t* src, int32_t* count, void* stream);
int stp_mcmc_relocate_apply(int P, const int32_t* src, const int32_t* count, int n_tensors, const StpMcmcTensor* tensors, float min_opacity, int raw,
                            int reset_dead_moments, void* scratch, size_t scratch_bytes, void* stream);
int stp_mcmc_add_apply(int P, int n_new, const int32_t* src, const int32_t* count, int n_tensors, const StpMcmcTensor* tensors, float min_opacity, int raw,
                       void* scratch, size_t scratch_bytes, void* stream);

/* Extension (not in the reference): adaptive density control of a 3DGS / StopThePop trainer -- the per-step statistics and densify_and_prune --
   in four calls.  All data is float32, all pointers are device pointers to contiguous data (stp_densify_scan's `counts` excepted), every call
   runs on the caller's stream and allocates nothing; no atomics: equal inputs give equal bits.
   stp_densify_stats, in place, one lane per Gaussian: for every visible i (visible_kind as in stp_sparse_adam: 0 = P bytes, non-zero = visible;
       1 = the P int32 radii of the forward, > 0 = visible)
       grad_accum[i] += sqrtf(gx * gx + gy * gy)  (the first two floats of row i of grad2d, rows of grad_stride = 2 or 3 floats; uncontracted)
       denom[i] += 1          max_radii2D[i] = max(max_radii2D[i], (float)radii[i])  where max_radii2D is given (visible_kind 1 only)
   Invisible rows keep their bits and their gradient is never read.  No host synchronisation.
   stp_densify_plan writes one byte per Gaussian.  With s = the three scales (exp of `scaling` where rule->raw) and o = the opacity (its sigmoid
   where rule->raw):
       g = denom > 0 ? grad_accum / denom : 0        smax = max(s)        hot = g >= grad_threshold
       clone = hot && smax <= split_size             split = hot && smax > split_size           low = o < min_opacity
       ws(x) = prune_big && x > max_world_size       vs = prune_big && max_radii2D != null && max_radii2D[i] > max_screen_size
       K = !split && !(low || ws(smax) || vs)        C = clone && !(low || ws(smax))            S = split && !(low || ws(smax / split_shrink))
       plan[i] = K | C << 1 | S << 2
   K: the original stays, C: one copy is appended, S: two children are appended.  The bits are independent: every value 0..7 is a legal plan
   (bits 3..7 are ignored), so a plan may as well be written by the caller.  With max_radii2D == null the surviving rows and their order are
   those of upstream's densify_and_prune (whose screen-size test never fires: it zeroes max_radii2D before its prune); with max_radii2D
   given the test applies to the originals.  No host synchronisation.
   stp_densify_scan: one exclusive sum over the 3P flags [K bits | C bits | S bits]: offsets[i], offsets[P + i], offsets[2P + i] are the
   destination rows of Gaussian i's original, copy and first child in the output order below; counts = (nK, nC, nS) is written to HOST memory,
   and THE CALL SYNCHRONISES THE STREAM -- the one host synchronisation of a densification (the caller must learn the new row count to
   allocate the outputs).  scratch: stp_densify_scratch_bytes(P) bytes (a function of P alone; 0 for a P the scan refuses), 4-byte aligned.
   stp_densify_apply writes the new model: for each of n_tensors entries (row = floats per Gaussian; exp_avg and exp_avg_sq both given or both
   null, and then their outputs too) the M = nK + nC + 2 nS output rows are, in this order, the K rows in index order, the C rows, the first
   children of the S rows, their second children -- what upstream's cat, cat, mask sequence leaves.  K rows copy the parameter and both
   moments bit for bit; C rows and children copy the parameter and get zero moments, except that child j of the r-th split Gaussian i has
       xyz' = xyz[i] + R(q / |q|) (s * noise[j * nS + r])          scaling' = raw ? logf(s / split_shrink) : s / split_shrink
   in the tensors of role 1 (xyz, row 3) and 2 (scaling, row 3), with q the row of the role-3 tensor (rotation, (w, x, y, z), row 4), s the
   activated scales (expf of the role-2 rows where raw) and noise the caller's 2 nS x 3 standard normal floats.  Role 0: a plain tensor.
   Inputs are not modified; outputs must not overlap inputs.  A tensor whose rows are multiples of 16 bytes and whose pointers are all
   16-byte aligned moves 16 bytes per lane, others one float at a time, with equal bits.  Up to eight entries go in one launch.
   stats / plan / scan / apply return the number of kernel launches made (0 for P == 0 or nothing to write: nothing is touched, counts = 0), or
   a negative StpStatus with the reason in the last-error text.  Refused BEFORE anything is launched (STP_ERR_INVALID_ARGUMENT): a negative P
   or one with 3P >= 2^31, null pointers (of anything that would be read or written), a grad_stride other than 2 or 3, an unknown visible_kind,
   max_radii2D with visible_kind 0 (there are no radii to read), a scratch that is too small or misaligned; and by apply: counts outside
   [0, P], more than 64 entries, row <= 0 or P * row >= 2^31, an unknown role, one moment pointer without the other, raw other than 0 or 1,
   nS > 0 without exactly one entry of each of the roles 1, 2, 3 with rows 3, 3, 4 or without noise. */
typedef struct { float grad_threshold, split_size, min_opacity, max_screen_size, max_world_size, split_shrink; int32_t raw, prune_big; } StpDensifyRule;
typedef struct { const float *param, *exp_avg, *exp_avg_sq; float *param_out, *exp_avg_out, *exp_avg_sq_out; int32_t row; int32_t role; } StpDensifyTensor;
int stp_densify_stats(int P, float* grad_accum, float* denom, float* max_radii2D /* may be null */, const float* grad2d, int grad_stride /* 2 or 3 */,
                      const void* visible, int visible_kind, void* stream);
int stp_densify_plan(int P, const float* grad_accum, const float* denom, const float* scaling, const float* opacity,
                     const float* max_radii2D /* may be null */, const StpDensifyRule* rule, uint8_t* plan, void* stream);
size_t stp_densify_scratch_bytes(int P);
int stp_densify_scan(int P, const uint8_t* plan, void* scratch, size_t scratch_bytes, uint32_t* offsets /* 3P */, int64_t counts[3] /* host */, void* stream);
int stp_densify_apply(int P, const uint8_t* plan, const uint32_t* offsets, const int64_t counts[3], int n_tensors, const StpDensifyTensor* tensors,
                      const float* noise /* (2 nS, 3) */, float split_shrink, int raw, void* stream);

/* Extension (not in the reference): simple_knn's distCUDA2, the call 3DGS code bases initialise their scales with.  For `points`, P x 3
   contiguous float32 on the device, mean_dist2[i] is the mean of the three smallest squared distances from point i to the points j != i
   (by index: an exact duplicate of i is a neighbour at distance 0), in input order.  The search is exact and the result fixed to the bit:
       dx = xj - xi, dy = yj - yi, dz = zj - zi      d2 = (dx * dx + dy * dy) + dz * dz      out[i] = ((b0 + b1) + b2) / 3.0f
   in float32, every operation rounded to nearest once and none contracted, b0 <= b1 <= b2 the three smallest d2: the bits of a brute-force
   evaluation in that order, whatever the cloud (the three smallest values of a multiset do not depend on ties or on the search order).
   The points are sorted by 30-bit Morton codes over 1024 cells of equal count per axis (rocPRIM sorts), cut into boxes of STP_KNN_BOX,
   and a workgroup per box searches the other boxes behind float32-conservative box tests.  No atomics: equal inputs give equal bits.  No host synchronisation and no allocation:
   `scratch` is stp_knn_scratch_bytes(P) bytes of device memory, 16-byte aligned, free again when the kernels have run.
   stp_knn_scratch_bytes is a function of P alone, 0 for P <= 0, non-decreasing in P, and does not overflow up to INT_MAX (32 bytes per
   point and a little).  stp_knn_mean_dist2 returns the number of launches made (the library's sort counting as one; 0 for P == 0: nothing is
   touched), or a negative StpStatus with the reason in the last-error text.  Refused BEFORE anything is launched
   (STP_ERR_INVALID_ARGUMENT): a negative P, 1 <= P <= 3 (there are no three neighbours), a null pointer, a scratch that is too small or
   misaligned. */
#define STP_KNN_BOX 256
size_t stp_knn_scratch_bytes(int P);
int stp_knn_mean_dist2(int P, const float* points /* P x 3 */, void* scratch, size_t scratch_bytes, float* mean_dist2 /* P */, void* stream);

/* Extension (not in the reference): the Morton order of a cloud, and the gather that moves a model into it (or into any other order).
   Densification and 3DGS-MCMC growth append rows and relocation rewrites rows anywhere, so after some thousand iterations a row's index
   says nothing about where its Gaussian lies; a trainer that wants neighbours in space to be neighbours in memory re-sorts every so often.
   stp_spatial_order: order[s] is the index of the row of `xyz` (P x 3 contiguous float32 on the device) that moves to position s, and
   codes[s] (where not null) the 30-bit code of that row.  It is the order stp_knn_mean_dist2 searches in (the same kernels), and it is
   fixed to the bit.  Per axis a:
       key_a(i) = the bits of xyz[i][a] as an unsigned integer of the same order (negative: ~bits, else bits | 2^31; -0 sorts below +0, the
                  infinities lie at the ends)
       sorted_a = the keys in ascending order          splitter_a[k - 1] = sorted_a[floor(k P / 1024)], k = 1 .. 1023
       cell_a(i) = the number of splitters <= key_a(i), in 0 .. 1023
   cells of equal COUNT, not of equal width: outliers take no cells from the rest, a cluster gets as many as it has points for.  Then
       code(i) = spread10(cell_x) | spread10(cell_y) << 1 | spread10(cell_z) << 2          (spread10: bit b of 10 goes to bit 3 b)
   and order is the STABLE ascending sort of (code, i): equal codes stay in index order.  The codes depend on the multiset of coordinates
   only, so the order of an already ordered cloud is the identity.  P >= 1 is accepted.  The caller's stream only, no host synchronisation,
   no atomics; `scratch` is stp_spatial_order_scratch_bytes(P) bytes of device memory, 16-byte aligned, free again when the kernels have run
   (a function of P alone, 0 for P <= 0, non-decreasing in P, no overflow up to INT_MAX: 16 bytes per point and a little).  Returns the
   number of launches made (a sort of the library counting as one; 0 for P == 0: nothing is touched), or a negative StpStatus with the
   reason in the last-error text.  Refused BEFORE anything is launched (STP_ERR_INVALID_ARGUMENT): a negative P, a null xyz, order or
   scratch, a scratch that is too small or misaligned.
   stp_gather_rows: for each of n_tensors entries (an StpDensifyTensor by layout: row = 4-byte elements per row, role must be 0, exp_avg and
   exp_avg_sq both given or both null, and then their outputs too) output row s, 0 <= s < M, of param_out, exp_avg_out and exp_avg_sq_out
   is row index[s] of the P input rows, copied bit for bit: the elements are moved, never computed on, and may as well be int32 or NaN
   payloads.  index may be a permutation (M == P), a subset, or hold repeats (M > P).  AN INDEX OUTSIDE [0, P) IS READ AS THE NEAREST VALID
   ROW (0 or P - 1): the kernel never reads out of bounds, and never reports it.  Out of place only: an output that overlaps any input of
   the call (a tensor, a moment or the index) is refused.  A tensor whose rows are multiples of 16 bytes and whose six pointers are all
   16-byte aligned moves 16 bytes per lane, others one element at a time, with equal bits.  Up to eight entries go in one launch.  Returns
   the number of launches made (0 for M == 0 or n_tensors == 0: nothing is touched) or a negative StpStatus.  Refused BEFORE anything is
   launched (STP_ERR_INVALID_ARGUMENT): a negative P or M, M > 0 rows from P == 0, a null pointer, more than 64 entries, row <= 0,
   max(P, M) * row >= 2^31, a role other than 0, one moment pointer without the other, an overlap. */
typedef StpDensifyTensor StpGatherTensor;
size_t stp_spatial_order_scratch_bytes(int P);
int stp_spatial_order(int P, const float* xyz /* P x 3 */, void* scratch, size_t scratch_bytes, int32_t* order /* P */, uint32_t* codes /* P, may be null */,
                      void* stream);
int stp_gather_rows(int P, int M, const int32_t* index /* M */, int n_tensors, const StpGatherTensor* tensors, void* stream);

/* Extension (not in the reference): the fused photometric loss of 3DGS trainers, (1 - lambda) * L1 + lambda * (1 - SSIM) -- upstream's
   l1_loss and ssim() with window_size = 11 and size_average = True, the pair the `fused-ssim` extension replaces.  `image` (x) and `target`
   (y) are `planes` contiguous float32 planes of H x W (a (C, H, W) or (B, C, H, W) tensor: planes = B * C), n = planes * H * W.  With
   blur = the 2-D correlation with the outer product of w_k = exp(-(k - 5)^2 / 4.5) / sum (k = 0 .. 10) and ZERO padding of 5, per plane:
       mu1 = blur(x), mu2 = blur(y), s1 = blur(x^2) - mu1^2, s2 = blur(y^2) - mu2^2, s12 = blur(x y) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2
       A = 2 mu1 mu2 + C1, B = 2 s12 + C2, Cc = mu1^2 + mu2^2 + C1, D = s1 + s2 + C2,  m = A B / (Cc D)
   stp_photometric_forward writes out2[0] = mean |x - y| and out2[1] = mean m (device memory) and, when `maps` is not NULL, the three
   derivative maps dm/dmu1, dm/ds1, dm/ds12 (map k of element e at maps[k * n + e]) that stp_photometric_backward reads:
       dL/dx = blur(s d1) + 2 x blur(s d2) + y blur(s d3) + (g0 / n) sign(x - y),  s = g1 / n,  sign(0) = 0,  (g0, g1) = dL_dout2
   (dL_dout2 is read from DEVICE memory; there is no gradient for `target`).  `workspace`: stp_photometric_workspace_floats floats of
   device memory, free again when the forward's kernels have run.  A kernel's workgroup owns a tile of STP_PHOTOMETRIC_TILE_W x
   STP_PHOTOMETRIC_TILE_H pixels of one plane; all sums run in a fixed order without atomics: equal inputs give equal bits.
   Each call returns the number of kernel launches made (forward 2, backward 1; 0 when planes, H or W is 0: nothing is touched), or a
   negative StpStatus with the reason in the last-error text.  Refused BEFORE anything is launched (STP_ERR_INVALID_ARGUMENT): a negative
   size, planes * H * W >= 2^31, a null image, target, out2, workspace, dL_dout2 or dL_dimage, null maps in the backward.  Plain calls: no
   host synchronisation, no allocation, no per-thread request state. */
#define STP_PHOTOMETRIC_TILE_W 64
#define STP_PHOTOMETRIC_TILE_H 16
size_t stp_photometric_workspace_floats(int planes, int H, int W);   /* floats of `workspace` (the forward's partial sums) */
int stp_photometric_forward(int planes, int H, int W, const float* image, const float* target,
                            float* out2 /* device: mean |x-y|, mean SSIM */, float* maps /* 3*planes*H*W floats, or NULL */,
                            float* workspace, void* stream);
int stp_photometric_backward(int planes, int H, int W, const float* image, const float* target, const float* maps,
                             const float* dL_dout2 /* device, 2 floats */, float* dL_dimage, void* stream);

/* Extension (not in the reference): the loss a 3DGS trainer's step really runs, in the kernels above -- the photometric terms of the
   EXPOSED, CLAMPED and MASKED render plus the inverse-depth regulariser:
       v_j = sum_i x_i E[i][j] + E[j][3]   (the row index is the INPUT channel: upstream's matmul(image.permute(1, 2, 0), E[:3, :3]) + E[:3, 3]),
             evaluated as ONE float32 chain  fma(E[2][j], x_2, fma(E[1][j], x_1, fma(E[0][j], x_0, E[j][3])))
       v_j clamped to [0, 1] when `clamp` (the gradient passes where 0 <= v_j <= 1),   x''_j = v_j * alpha_mask
       out3[0] = mean |x'' - y|,  out3[1] = mean SSIM(x'', y)  as above; the window's zero padding applies to x'' (a pixel outside the
                 image is 0, not E[j][3])
       out3[2] = mean |(invdepth - mono_invdepth) * depth_mask| over the depth_planes * H * W depth elements (exactly 0.0 without them)
   Every member of StpTrainingLoss is optional (NULL / 0) and may be given alone; invdepth and mono_invdepth come together.  `exposure`
   is 3 x 4 floats (exposure_batched = 0) or one 3 x 4 per image of the batch (1: planes / 3 of them) and needs planes % 3 == 0, the
   planes being the (B, 3, H, W) channels; alpha_mask is one H x W plane (alpha_mask_batched = 0) or one per image (1: planes / channels
   of them, `channels` = planes per image, 0 = 3).  The backward gives
       dL/dx_i = sum_j E[i][j] g'_j,   g'_j = g''_j * alpha_mask * [clamp passes],  g''_j = the photometric dL/dx''_j above
       dL/dE[i][j] = sum_p x_i g'_j,  dL/dE[j][3] = sum_p g'_j   (dL_dexposure, laid out like exposure; NULL = not wanted)
       dL/dinvdepth = (g2 / n_d) sign((d - m) mask) mask          (dL_dinvdepth; NULL = not wanted)
   with (g0, g1, g2) = dL_dout3 read from device memory.  All sums in a fixed order without atomics.  With `extras` NULL (or all of
   its members 0) the calls run the kernels of stp_photometric_forward / _backward on out3[0 .. 1] and write out3[2] = 0.
   `workspace`: stp_training_loss_workspace_floats floats, used by the forward and (with dL_dexposure) by the backward.
   Each call returns the kernel launches made (forward 2; backward 1, or 2 with dL_dexposure; 0 when planes, H or W is 0: nothing is
   touched), or a negative StpStatus.  Refused BEFORE anything is launched (STP_ERR_INVALID_ARGUMENT): a negative size or count,
   planes * H * W or depth_planes * H * W >= 2^31, a null required pointer, exposure with planes % 3 != 0 or channels != 3, planes not a
   multiple of channels, invdepth without mono_invdepth or the reverse, a depth_mask or depth_planes > 0 without them, depth_planes == 0
   with them, clamp or a _batched flag that is not 0 or 1, null maps in the backward, dL_dexposure without exposure, dL_dinvdepth without
   invdepth, dL_dexposure without workspace. */
typedef struct StpTrainingLoss {
    const float* exposure;       /* 3 x 4, or (planes / 3) x 3 x 4 */
    const float* alpha_mask;     /* H x W, or (planes / channels) x H x W */
    const float* invdepth;       /* depth_planes x H x W */
    const float* mono_invdepth;  /* depth_planes x H x W */
    const float* depth_mask;     /* depth_planes x H x W, or NULL */
    int32_t clamp;
    int32_t exposure_batched;
    int32_t alpha_mask_batched;
    int32_t channels;            /* planes per image (0 = 3) */
    int32_t depth_planes;
} StpTrainingLoss;
size_t stp_training_loss_workspace_floats(int planes, int H, int W, int depth_planes);
int stp_training_loss_forward(int planes, int H, int W, const float* image, const float* target, const StpTrainingLoss* extras,
                              float* out3 /* device: L1, SSIM, depth L1 */, float* maps /* 3*planes*H*W floats, or NULL */,
                              float* workspace, void* stream);
int stp_training_loss_backward(int planes, int H, int W, const float* image, const float* target, const StpTrainingLoss* extras,
                               const float* maps, const float* dL_dout3 /* device, 3 floats */, float* dL_dimage,
                               float* dL_dexposure /* or NULL */, float* dL_dinvdepth /* or NULL */, float* workspace, void* stream);

/* Sizes of the three scratch buffers (the reference's `required<State>()`, rasterizer_impl.h:68-75). */
size_t stp_geometry_buffer_size(int P, const StpSettings* settings);
size_t stp_geometry_buffer_size_stash(int P, const StpSettings* settings); /* of a forward with stp_set_forward_sh_stash: the above + the nine planes of P floats */
size_t stp_binning_buffer_size(int R);
size_t stp_image_buffer_size(int width, int height); /* without the optional blend log */
/* Bytes the blend log adds to the image buffer of a forward with StpSettings.record_blend_log = 1 in the hierarchical / k-buffer modes,
   for a frame nothing is known about yet: 192 records of 2 bytes per pixel of the 16x16 tile grid + eight spare rows = 400 B per pixel.
   The depth is ADAPTIVE: every recording forward reports the largest number of blends of any of its pixels, and the next forwards of
   the same kind (P, resolution, tile-row window, mode) on the device size their log by it (+12.5 %, multiple of 16, 32..512 records) --
   304 B per pixel once a frame like BASELINE's C2 (at most 114 blends per pixel) has been seen, 464 B for C5 (195).  A pixel that blends
   more than its frame's depth flags its tile, whose backward then re-sorts (correct, slow), and the frames after it get the deeper log.
   STP_LOG_DEPTH=n in the environment fixes the depth.  _rows: of a forward restricted to the tile rows [tile_y0, tile_y1). */
size_t stp_blend_log_bytes(int width, int height);
size_t stp_blend_log_bytes_rows(int width, int height, int tile_y0, int tile_y1);
/* The depth (records per pixel) of the blend log in an image buffer a forward filled (0: it recorded none).  Every forward leaves a header in
   its image and binning buffers (their first 256 bytes: magic, value, ~value), so the buffers are self-contained like the reference's: the
   library keeps a pointer -> value cache for the buffers of this process and reads the header back (one blocking 16-byte copy) for a pointer it
   does not know -- a clone, a copy, a buffer of another process.  Negative (STP_ERR_INVALID_ARGUMENT) for a buffer without a valid header. */
int stp_blend_log_depth(const void* image_buffer);
/* Drops the library's cached layout of a binning / image buffer at this address.  An allocator that recycles scratch buffers calls it when
   it releases or frees one, so that a later tenant of the address -- a clone or a restored copy of ANOTHER forward's buffer, which no forward
   of this process carved there -- is resolved from the header it carries instead of the previous tenant's entry.  (A forward that carves the
   address again overwrites the entry by itself.)  Harmless for unknown pointers. */
void stp_forget_buffer(const void* buffer);
/* Bytes of a blend log of `depth` records per pixel (depth <= 0: of the DEEPEST log a forward may carve, 512 records) for the tile rows
   [tile_y0, tile_y1) (0, 0 = the whole frame): what a memory policy should budget for a frame whose depth it does not know yet. */
size_t stp_blend_log_bytes_depth(int width, int height, int tile_y0, int tile_y1, int depth);

/* Introspection of the (otherwise opaque) scratch buffers, for parity tests and debugging.
   Fills byte offset and element count of a named sub-array; returns 0 or STP_ERR_INVALID_ARGUMENT.
   geometry names: depths clamped radii rects2D means2D cov3D cov3D_inv conic_opacity rgb tiles_touched point_offsets invz
   binning names : point_list point_list_unsorted keys keys_unsorted
   image names   : final_T n_contrib ranges */
int stp_geometry_layout(int P, const StpSettings* settings, const char* name, size_t* offset, size_t* count);
int stp_binning_layout(int R, const char* name, size_t* offset, size_t* count);
/* The entry count a binning buffer was carved with by the forward that last used it: num_rendered, or -- for a run-ahead forward, which
   carves and launches before num_rendered is known -- the capacity it guessed (>= num_rendered; the first num_rendered elements of
   every sub-array are the valid ones).  Pass the result to stp_binning_layout.  From the library's cache, else from the buffer's own header
   (see stp_blend_log_depth); negative (STP_ERR_INVALID_ARGUMENT) for a buffer that carries none or was carved for fewer than R entries.
   stp_backward does this lookup itself -- and refuses such a buffer instead of carving it on a guess: callers keep passing (buffer,
   num_rendered) as in the reference. */
int stp_binning_layout_count(const void* binning_buffer, int R);
/* Forgets the per-device size guesses (tile-list entries of the previous frames of each kind) that the run-ahead forward and the early
   binning request are sized by: the next forward of every kind takes the reference's path again (hand-over in the middle of the frame,
   exact request).  For tests and benchmarks that want a defined starting state; never needed for correctness. */
void stp_reset_size_guesses(void);
/* Run-ahead forward.  mode 0 = never, 1 = always, 2 = auto (the default; STP_RUN_AHEAD=0 / 1 in the environment sets 0 / 1 at load time).
   With it, a forward that has a size guess (i.e. every forward but the first of its kind) enqueues ALL its kernels on the guessed capacity
   before it reads num_rendered back -- no host wait in the middle of the frame; a frame that does not fit its guess is redone with the
   exact size before stp_forward returns.  Results are identical either way (keys, lists, image, gradients).  Measured on MI355X it
   costs 0.5 % at 1M Gaussians / 1080p (the padded entries pass through the device-wide sort) and gains 7 % at 1k Gaussians / 256x256
   (the round trip is a tenth of that frame): auto = run ahead when the guess is below 2^18 tile-list entries. */
void stp_set_run_ahead(int mode);
int stp_get_run_ahead(void);
int stp_image_layout(int width, int height, const char* name, size_t* offset, size_t* count);
/* ... of the image buffer of a forward restricted to the tile rows [tile_y0, tile_y1) (StpSettings::tile_y0 / tile_y1): it holds the
   window's pixel rows and tiles only, element 0 of every sub-array being the window's first pixel / tile (0, 0 = the whole frame).
   The count reported for "blend_log" is that of the default depth (see stp_blend_log_bytes). */
int stp_image_layout_rows(int width, int height, int tile_y0, int tile_y1, const char* name, size_t* offset, size_t* count);
/* ... with the blend log at the depth the buffer was really carved with (stp_blend_log_depth(buffer); 0 = the buffer holds no log, the
   name "blend_log" is then unknown): the count reported for "blend_log" matches the buffer. */
int stp_image_layout_depth(int width, int height, int tile_y0, int tile_y1, int log_depth, const char* name, size_t* offset, size_t* count);

/* Stage timer, the counterpart of the reference's `Timer` (rasterizer_impl.h:77-147; stages
   "Preprocess","Duplicate","Sort","Render", rasterizer_impl.cu:248) plus "BwdRender","BwdPreprocess".
   While enabled, every forward/backward records hipEvents around its stages on the call's stream (no extra
   host synchronisation); stp_timing_read waits for the recorded events and returns the MEAN milliseconds per
   stage over the calls since stp_timing_enable(1) (6 floats, unmeasured stages are -1).  One timer PER DEVICE behind a
   mutex: stp_timing_read / stp_timing_text report the calling thread's CURRENT device (hipSetDevice first); a backward is
   attributed to the latest forward of its device, so time one caller per device.  stp_timing_read returns STP_ERR_HIP
   when an event could not be created or recorded (the timings are then incomplete). */
void stp_timing_enable(int enabled);
int stp_timing_read(float* ms6);
/* Per-call stage times instead of their means: fills ms6[6 * k + stage] for the last n = min(calls since stp_timing_enable(1), 1024,
   capacity) forward(+backward) calls of the current device in chronological order (-1 = stage not measured in that call) and returns n.
   What makes a slow step attributable: bench.py puts the worst step's six stage times beside the median step's. */
int stp_timing_history(float* ms6, int capacity);
/* The same for the HOST: milliseconds the launching thread spent between recording a stage's two events (normally microseconds: launches are
   asynchronous).  A stage whose GPU interval is long while its kernels are not was waiting for a launch: the host figure tells a late host --
   a descheduled thread, a blocking driver call -- from a slow kernel. */
int stp_timing_history_host(float* ms6, int capacity);
/* The text the reference hands to the SIBR viewer (DebugVisualizationData::timings_text, rasterizer_impl.cu:391-399):
   "Timings: \n - Preprocess: <ms>ms\n - Duplicate: ...\n - Sort: ...\n - Render: ...\n - Total: <sum>ms\n" over the forward
   stages measured since stp_timing_enable(1); measured backward stages follow as two more lines.  Writes at most
   `size` bytes including the terminating NUL and returns the length the full text needs (as snprintf does). */
size_t stp_timing_text(char* buf, size_t size);

/* Measurement helper (bench.py `hbm_measured`; not part of the reference's interface): one launch of a plain float4 streaming kernel over
   `bytes` (a multiple of 16) on `stream` -- kind 0: read `src` (dst may be NULL), 1: write `dst`, 2: copy src -> dst, + 4: with non-temporal
   loads / stores -- with `blocks` workgroups of 256 threads, eight 16-byte accesses in flight per thread.  The caller times it with events on the same stream.  What the box's
   HBM delivers to the streaming stages of the path, next to the 8 TB/s spec peak. */
int stp_hbm_probe(int kind, void* dst, const void* src, size_t bytes, int blocks, void* stream);

const char* stp_last_error(void);
int stp_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
