// stp_internal.h -- host-side internals of libstp_raster.so: scratch-buffer carving, what the host files of the C ABI (stp_api.hip,
// stp_forward.hip, stp_buffers.hip, stp_timer.hip) need from each other, and the launcher interface between them and the kernel
// translation units.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <cstdlib>
#include <string>

#include "../../include/stp_raster.h"
#include "stp_switches.h"

namespace stp {

constexpr int TILE = 16;
constexpr size_t ALIGN = 256; // sub-array alignment inside the scratch buffers
static_assert(ALIGN == 256, "Switches::carve_skew (stp_switches.h) is masked to a multiple of 256");
constexpr int MAX_DEVICES = 32; // per-device helpers (timers, mailbox rings, side streams, size guesses, background scratch) are arrays of this size

enum SortMode { MODE_GLOBAL = 0, MODE_FULL = 1, MODE_KBUFFER = 2, MODE_HIER = 3 };
enum SortOrder { ORDER_Z = 0, ORDER_DISTANCE = 1, ORDER_PTD_CENTER = 2, ORDER_PTD_MAX = 3 };

inline bool uses_blend_log(const StpSettings& s)
{
    return s.record_blend_log != 0 && s.debug_visualization == 0 && (s.sort_mode == MODE_HIER || s.sort_mode == MODE_KBUFFER);
}

// which 16-bit sub-tile mask the entry gather leaves in the spare word of an entry's colour record (stp_device.h: subtile_mask):
// 1 = the hierarchical mode's 4x4 culling decisions, 2 = the k-buffer kernel's sub-tile pre-test, 0 = none
inline int subtile_mask_kind(const StpSettings& s)
{
    if (s.sort_mode == MODE_HIER && s.hierarchical_4x4_culling) return 1;
    return s.sort_mode == MODE_KBUFFER ? 2 : 0;
}

inline bool requires_depth_along_ray(const StpSettings& s) // reference rasterizer.h:66-71
{
    return s.sort_mode != MODE_GLOBAL || s.sort_order == ORDER_PTD_CENTER || s.sort_order == ORDER_PTD_MAX;
}

// Bump allocator over one byte buffer: the counterpart of the reference's obtain()/required()
// (rasterizer_impl.h:21-27,68-75) with our own layout.  With base == nullptr it only measures.
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(char* b) : base(b) {}
    // STP_CARVE_SKEW=n (experiment, profiles/EXPERIMENTS.md round 6: HBM channel aliasing between the SoA arrays a kernel streams side by side):
    // n extra bytes (a multiple of ALIGN) in front of every sub-array but the first
    static size_t skew() { return switches().carve_skew; }
    template <typename T> T* take(size_t count, size_t* off_out = nullptr)
    {
        off = (off + ALIGN - 1) & ~(ALIGN - 1);
        if (off) off += skew();
        if (off_out) *off_out = off;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
    size_t total() const { return ((off + ALIGN - 1) & ~(ALIGN - 1)) + ALIGN; }
};

// Per-Gaussian state (reference GeometryState, rasterizer_impl.cu:175-193).  SoA, HBM-resident
// between forward and backward.
struct GeometryState {
    uint32_t* status;        // [0] num_rendered, [1] error flags   (read back once per forward)
    float* depths;           // P
    uint8_t* clamped;        // 3P
    int32_t* internal_radii; // P
    float2* rects2D;         // P
    float2* means2D;         // P
    float* cov3D;            // 6P
    float4* cov3D_inv;       // 3P, only if requires_depth_along_ray
    float4* gpack;           // 4P, only if requires_depth_along_ray: A, B, C (id slot unused), D of the entry records, packed per
                             //     Gaussian so that gather_entries_kernel reads one contiguous 64-byte line per entry
    float4* conic_opacity;   // P
    float* rgb;              // 3P
    uint32_t* tiles_touched; // P
    uint32_t* point_offsets; // P   (inclusive scan of tiles_touched; between preprocess_kernel and duplicate_kernel: inclusive inside each block of 256)
    uint32_t* block_sums;    // ceil(P / 256): entries of each preprocess workgroup, and their exclusive scan (two-level scan, stp_preprocess.hip)
    uint32_t* block_prefix;  // ceil(P / 256)
    char* scan_temp;
    size_t scan_temp_bytes;
    float* invz;             // P: 1 / view-space z of the visible Gaussians; written only by a forward with the inverse-depth request (LAST in the carve)
};
// The SH stash (stp_set_forward_sh_stash) is one more sub-array behind invz, carved only on request (carve_geometry's sh_stash): nine planes of P
// floats, plane 3 ch + {0, 1, 2} = d(colour channel ch) / d(unit view direction x, y, z) of the visible Gaussians (stp_sh_dir.h).  It is NOT a member
// of GeometryState, which kernels take by value: their arguments, and with them the kernels, stay what they are.
// Whether a geometry buffer carries a stash travels with it: words STP_STASH_WORD .. + 2 of the status block (the buffer's first 256 bytes) hold
// {STP_HEADER_MAGIC_STASH, P, ~P}, written by the stashing sh_color_kernel; frame_init_kernel zeroes them in every forward.
constexpr int STP_STASH_WORD = 8;
constexpr uint32_t STP_HEADER_MAGIC_STASH = 0x53505453u; // "STPS"

struct ImageState { // reference ImageState, rasterizer_impl.cu:195-202 (ranges sized per tile, not per pixel)
    float* final_T;      // N
    uint32_t* n_contrib; // N
    uint2* ranges;       // T
    uint32_t* dbg_minmax; // 2 (debug depth visualisation: the frame's extrema, as order-preserving integers)
    // Binning by tile counters (stp_binning.hip: "atomic binning"): entries per tile counted by preprocess_kernel, the
    // next free slot of every tile's segment while duplicate_kernel fills it, and [0] = entries over all tiles.
    uint32_t* tile_counts; // T
    uint32_t* tile_cursor; // T
    uint32_t* bin_total;   // 2
    uint32_t* header;      // 4: {STP_HEADER_MAGIC_IMAGE, log_depth, ~log_depth, 0} -- the blend log's depth travels WITH the buffer (stp_buffers.hip: buffer headers)
    uint32_t* tile_flags; // T   0 = this tile's log is valid, 1 = its log overflowed, 0xFFFFFFFF = the forward recorded no log
    uint32_t* blend_log;  // T * 4 waves * (log_depth + spare) rows * 64 lanes of u16 (only with the blend log)
    int log_depth;        // records per pixel the log holds (0: none)
};

struct BinningState { // reference BinningState, rasterizer_impl.cu:204-217
    uint32_t* header;      // first 256 bytes of the buffer: {STP_HEADER_MAGIC_BINNING, entries the buffer was carved for, ~that, 0} (stp_buffers.hip: buffer headers)
    uint32_t* point_list;
    uint32_t* point_list_unsorted;
    uint64_t* keys;
    uint64_t* keys_unsorted;
    char* sort_temp;
    size_t sort_temp_bytes;
    // Per-entry data in LIST ORDER (no counterpart in the reference, which gathers by Gaussian id wherever it needs
    // an entry's data): written once per frame by gather_entries_kernel, read with unit stride by the per-pixel-sort
    // render kernels.  A = (S00 S01 S02 S11), B = (S12 S22 q.x q.y), C = (q.z mean2D.x mean2D.y id), D = conic + opacity,
    // F = (r g b .), with S = Sigma^-1 and q = Sigma^-1 (mu - cam).
    float4* entA;
    float4* entB;
    float4* entC;
    float4* entD;
    float4* entF;
};

constexpr uint32_t STP_HEADER_MAGIC_BINNING = 0x42505453u, STP_HEADER_MAGIC_IMAGE = 0x49505453u; // "STPB", "STPI"
struct NamedOffset { const char* name; size_t offset; size_t count; };

GeometryState carve_geometry(char* base, size_t P, bool with_inv, size_t* total, NamedOffset* names = nullptr, int* n_names = nullptr, float** sh_stash = nullptr); // sh_stash: carve the stash too, *sh_stash = where
ImageState carve_image(char* base, int W, int H, int ty0, int ty1, int log_depth /* 0: no blend log */, size_t* total, NamedOffset* names = nullptr, int* n_names = nullptr); // the tile-row window's share, frame-coordinate indexing
BinningState carve_binning(char* base, size_t R, size_t* total, NamedOffset* names = nullptr, int* n_names = nullptr);
void clamp_tile_rows(int height, int& y0, int& y1); // StpSettings::tile_y0 / tile_y1 -> the frame's tile-row window (y1 <= 0: the whole frame)

// ---- the error state (stp_api.hip): ONE message per thread, set by whichever file refuses the call ----
int fail(int code, const std::string& msg);
int fail_hip(hipError_t e, const char* what);
#define STP_TRY(expr, what) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail_hip(_e, what); } while (0)
#define STP_DEBUG_SYNC(what) /* (wherever a stream `st` and a flag `debug` are in scope) */ STP_TRY(debug ? hipStreamSynchronize(st) : hipSuccess, what)

// ---- the stage timer (stp_timer.hip): no-ops unless stp_timing_enable(1); the calling thread's current device ----
void timer_begin_forward();
void timer_begin_backward();
void timer_mark(int i, hipStream_t st); // events 0..4: forward stage boundaries, 5..7: backward

// ---- what a buffer was carved with (stp_buffers.hip: buffer headers): cache of this process, else the buffer's own header ----
void remember_layout(const void* binning, uint32_t count, int64_t R);
void remember_stash(const void* geometry, bool stash, int64_t R); // every forward says whether its geometry buffer carries an SH stash ...
int stash_of(const char* geometry, int P, int64_t R, bool* stash, hipStream_t st, bool have_stream); // ... the backward asks: cache, else the buffer's own status block
void remember_log_depth(const void* image, uint32_t depth, int64_t R);
int layout_of(const char* binning, uint32_t R, uint32_t* cap, hipStream_t st = nullptr, bool have_stream = false);
int log_depth_of(const char* image, int64_t R, uint32_t* depth, hipStream_t st = nullptr, bool have_stream = false);

int blend_log_rows(int depth); // rows of 64 records per wave in a blend log of that depth (stp_render_replay.hip / stp_blend.h)
int blend_log_default_depth(); // depth of a frame nothing is known about
int blend_log_clamp_depth(int d);
size_t scan_temp_bytes(size_t P);
size_t sort_temp_bytes(size_t R);

// Everything a kernel launcher needs about one frame.
struct FrameParams {
    int P, D, M, W, H, gx, gy;
    int ty0, ty1; // tile-row window
    float focal_x, focal_y, tan_fovx, tan_fovy, scale_modifier;
    StpSettings s;
    const float* background;
    const float* means3D;
    const float* shs;
    const float* colors_precomp;
    const float* opacities;
    const float* scales;
    const float* rotations;
    const float* cov3D_precomp;
    const float* viewmatrix;
    const float* projmatrix;
    const float* inv_viewprojmatrix;
    const float* cam_pos;
    int prefiltered;
    int log_depth;       // depth of this frame's blend log (forward: chosen by log_depth_for; backward: the forward's)
    uint32_t* log_need;  // forward: device word the recording kernels report their largest blend count per pixel to (or nullptr)
    uint32_t log_tag;    // ... tagged with 16 bits of the frame's kind
    int split_launch = 0; // this FrameParams describes ONE of the two render launches of a split forward (stp_set_forward_split): no tile order of the whole window
    int fused_gather = 0; // forward: the hierarchical render kernel sorts and gathers the tiles of up to TS_SMALL entries itself (RenderArgs::fused_gather), tile_sort_gather_kernel only the longer ones
    const float* bg_image = nullptr; // forward, stp_set_forward_background: per-pixel background (3 x H x W) in the place of `background`
    float* out_alpha = nullptr;      // ... and where the render kernels also write alpha = 1 - final_T (H x W)
    float* out_invdepth = nullptr;   // forward, stp_set_forward_invdepth: the render kernels' INVD variants also write sum(alpha T / z) (H x W); preprocess keeps 1 / z
    const float* sh_dc = nullptr;    // stp_set_forward_split_sh / stp_set_backward_split_sh: the (P, 3) first SH coefficient; `shs` is then the (P, M-1, 3) rest (nullptr allowed for M == 1)
    int raw_params = 0; // stp_set_forward_raw_params / stp_set_backward_raw_params: bit 0 opacities, bit 1 scales, bit 2 rotations hold a trainer's raw parameters (stp_activations.h)
    int wild_cov; // forward, after the status read-back: some visible Gaussian has a Sigma^-1 entry >= 1e36 or not finite (depth keys then take the reciprocal with its domain check)
};

// stp_set_backward_camera_grads: the three outputs and the workspace (camera_grad_workspace_bytes) of one request
struct CameraGradRequest {
    float* dL_dview = nullptr; // nullptr: no request
    float* dL_dproj = nullptr;
    float* dL_dcam = nullptr;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
};

struct BackwardParams {
    CameraGradRequest cam; // the per-Gaussian half also sums the camera gradients (stp_backward.hip)
    float* absgrad = nullptr; // stp_set_backward_absgrad (P x 3, or nullptr = no request): the render half also sums |dL/dmean2D| per pair into
                              // record slots 9, 10, the per-Gaussian half moves them here
    float* blend_stats = nullptr; // stp_set_backward_blend_stats (P x 3, or nullptr = no request): the render half also collects sum, max and
                                  // count of the blend weights per pair in record slots 11..13, the per-Gaussian half moves them here
    // stp_set_backward_background (all nullptr = no request): the render half reads the forward's per-pixel background and the alpha gradient in
    // its pixel prologues; launch_background_grad forms dL/dbackground (3 floats, or 3 x H x W with bg_image) from final_T and dL_dpix
    const float* bg_image = nullptr;
    const float* dL_dalpha = nullptr;
    float* dL_dbackground = nullptr;
    // stp_set_backward_invdepth (both nullptr = no request): the forward's inverse-depth image and the loss gradient with respect to it.  The
    // render half takes them as a fourth channel and sums alpha T dL per Gaussian into record slot 14, the per-Gaussian half chains it to t_z
    const float* invdepth = nullptr;
    const float* dL_dinvdepth = nullptr;
    const float* pixel_colors;
    const float* dL_dpix;
    float* grad_rec;    // P x grad_stride: written by the render half, read by the per-Gaussian half
    int grad_stride;    // STP_GRAD_RECORD_FLOATS, or STP_GRAD_RECORD_USED with phases bit 2 (compact records)
    int clear_rec;      // phases bit 3: the per-Gaussian half zero-fills the records again
    int chunk, chunks;  // the per-Gaussian half on chunk `chunk` of `chunks` equal ranges of 256-Gaussian blocks (chunks <= 1: all Gaussians)
    float* dL_dmean2D;  // outputs of the per-Gaussian half from here on
    float* dL_dopacity;
    float* dL_dcolor;
    float* dL_dmean3D;
    float* dL_dcov3D;
    float* dL_dsh;
    float* dL_dscale;
    float* dL_drot;
    const float* sh_stash = nullptr; // the forward's SH stash, where the geometry buffer carries one (stp_api.hip: stash_of): the per-Gaussian half reads it in the place of the SH rows
    float* dL_ddc = nullptr; // stp_set_backward_split_sh (with FrameParams::sh_dc): P x 3, the first coefficient's gradient; dL_dsh is then P x (M-1) x 3
};

// ---- argument checks and frame description shared by the forward and the backward (stp_api.hip) ----
int check_settings(const StpSettings& s, bool backward);
void fill_frame(FrameParams& f, int P, int D, int M, const float* background, int width, int height, const StpSettings& s, const float* means3D,
                const float* shs, const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* inv_viewprojmatrix, const float* cam_pos,
                float tan_fovx, float tan_fovy, int prefiltered);

// ---- the one-shot per-thread requests (stp_api.hip: the stp_set_* setters, and the rules by which a call takes them) ----
struct ForwardSplit { int row = 0; hipEvent_t event = nullptr; bool armed = false; };      // stp_set_forward_split
struct ForwardBackground { const float* bg_image = nullptr; float* out_alpha = nullptr; }; // stp_set_forward_background
struct ForwardRequests { ForwardSplit split; ForwardBackground background; float* out_invdepth = nullptr; /* stp_set_forward_invdepth */ const float* sh_dc = nullptr; /* stp_set_forward_split_sh */ bool sh_stash = false; /* stp_set_forward_sh_stash */ int raw_params = 0; /* stp_set_forward_raw_params */ };
ForwardRequests take_forward_requests();
int check_raw_params(int mask, const float* opacities, const float* scales, const float* rotations); // 0, or fail(STP_ERR_INVALID_ARGUMENT) naming the bit

// ---- launchers (one per stage; each returns hipSuccess or the launch error) ----
hipError_t launch_preprocess(const FrameParams& f, const GeometryState& g, int* radii, uint32_t* tile_counts, hipStream_t st); // tile_counts: nullptr = do not count per tile
hipError_t launch_frame_init(const GeometryState& g, const ImageState& img, int tile0, int n_tiles, bool with_log, bool tile_counters, hipStream_t st); // status, ranges, tile flags (+ tile counters) of the window's tiles
hipError_t launch_scan(const FrameParams& f, const GeometryState& g, hipStream_t st);
// Longest-list-first order of the window's tiles for the render kernels' workgroups (into ImageState::tile_cursor, free outside STP_SORT=counters)
bool tile_order_enabled();
// ... and does THIS frame use it: a window of up to 1024 tiles is resident on the chip all at once (1024-1280 workgroup slots), an order of its
// workgroups changes nothing and the 7 us kernel is left out (C1: 256 tiles)
inline bool tile_order_used(const FrameParams& f) { return tile_order_enabled() && f.gx * (f.ty1 - f.ty0) > 1024; }
bool gather_order_enabled();
int gather_order_mode();
hipError_t launch_tile_order(const FrameParams& f, const ImageState& img, hipStream_t st);
hipError_t launch_sh_color(const FrameParams& f, const GeometryState& g, const int* radii, float* sh_stash, hipStream_t st); // SH -> RGB of the visible Gaussians (after preprocess); with sh_stash also the stash and its mark
hipError_t launch_stash_mark(const FrameParams& f, const GeometryState& g, float* sh_stash, hipStream_t st); // the mark alone, once more (a redone run-ahead frame: frame_init_kernel has cleared the status block again)
hipError_t launch_mailbox(const uint32_t* last_offset, const uint32_t* status, uint32_t* mailbox_dev, uint32_t ticket, uint32_t* log_need, hipStream_t st);
hipError_t launch_block_prefix_mailbox(const FrameParams& f, const GeometryState& g, uint32_t* mailbox_dev, uint32_t ticket, uint32_t* log_need, hipStream_t st); // second level of the scan + the hand-over
hipError_t launch_duplicate(const FrameParams& f, const GeometryState& g, const int* radii, const BinningState& b, uint32_t* tile_cursor, uint32_t cap, uint32_t header_cap, uint32_t* zero_ptr, size_t zero_words, hipStream_t st); // header_cap: entries the buffer was carved for (its header); tile_cursor: nullptr = by point_offsets into the unsorted arrays; cap: slots of a run-ahead launch (0xFFFFFFFF = exact)
hipError_t launch_tile_scan(const FrameParams& f, const ImageState& img, hipStream_t st);
hipError_t launch_bin_pad(const BinningState& b, const ImageState& img, int R, hipStream_t st);
hipError_t launch_sort(const FrameParams& f, const BinningState& b, int R, bool tile_bits_only, bool zeroed, hipStream_t st); // zeroed: duplicate_kernel cleared sort_zero_region()
void sort_zero_region(const BinningState& b, size_t R, uint32_t tiles, uint32_t** ptr, size_t* words); // what the tile-bit sort's own driver needs cleared in front of it
hipError_t launch_tile_sort_gather(const FrameParams& f, const GeometryState& g, const BinningState& b, const ImageState& img, int R, bool unordered, hipStream_t st);
hipError_t launch_ranges(const FrameParams& f, const BinningState& b, const ImageState& img, int R, hipStream_t st);
hipError_t launch_gather_entries(const FrameParams& f, const GeometryState& g, const BinningState& b, int R, hipStream_t st);
hipError_t launch_render_forward(const FrameParams& f, const GeometryState& g, const BinningState& b, const ImageState& img,
                                 float* out_color, hipStream_t st, std::string* err);
hipError_t launch_render_debug_finish(const FrameParams& f, const ImageState& img, float* out_color, hipStream_t st);
hipError_t launch_render_backward(const FrameParams& f, const GeometryState& g, const BinningState& b, const ImageState& img,
                                  const BackwardParams& bw, hipStream_t st, std::string* err);
// dL/dbackground over the window's pixel rows (stp_background.hip): T_final * dL_dpix per pixel, or its sum in a fixed order (uniform background);
// `partials`: background_grad_partials() floats of device scratch for the uniform sum, free again when the launched kernels have run
size_t background_grad_partials();
hipError_t launch_background_grad(const FrameParams& f, const ImageState& img, const BackwardParams& bw, float* partials, hipStream_t st);
hipError_t launch_preprocess_backward(const FrameParams& f, const GeometryState& g, const int* radii, const BackwardParams& bw, hipStream_t st);
size_t camera_grad_workspace_bytes(int P);
// sums the per-workgroup rows the CAM kernel wrote (none for P == 0) into the three outputs; launch_preprocess_backward calls it itself
hipError_t launch_camera_grad_finalize(int P, const CameraGradRequest& cam, hipStream_t st);
hipError_t launch_mark_visible(int P, const float* means3D, const float* viewmatrix, uint8_t* present, hipStream_t st);
// the fused sparse Adam step (stp_adam.hip) over tensors stp_sparse_adam has validated: one launch per eight tensors with elements (the
// descriptor table's size and its search: stp_row_table.h, which stp_adam.hip, stp_densify.hip and stp_mcmc_relocate.hip include); returns
// the launches made, *err = the launch error that ended them early (or hipSuccess)
int launch_sparse_adam(int n_tensors, const StpAdamTensor* tensors, int N, const void* visible, int visible_kind, float beta1, float beta2,
                       hipStream_t st, hipError_t* err);
// the fused dense, bias-corrected Adam step (stp_adam.hip: dense_adam_kernel) over tensors stp_dense_adam has validated: one launch per eight
// tensors with elements; returns the launches made, *err = the launch error that ended them early (or hipSuccess)
int launch_dense_adam(int n_tensors, const StpDenseAdamTensor* tensors, hipStream_t st, hipError_t* err);
// the activated copies of a trainer's raw parameters (stp_activate.hip) over arguments stp_activate_params has validated (P in [1, 2^31 / 4)); any
// of the three pairs may be nullptr together: one launch per pair given; returns the launches made, *err = the launch error (or hipSuccess)
int launch_activate_params(int P, const float* scaling, const float* rotation, const float* opacity, float* scales, float* rotations, float* opacities,
                           hipStream_t st, hipError_t* err);
// the 3DGS-MCMC kernels (stp_mcmc.hip) over arguments stp_mcmc_relocation / stp_mcmc_add_noise have validated (n, P in [1, 2^31)): one launch
// each; both return the launches made, *err = the launch error (or hipSuccess)
int launch_mcmc_relocation(int n, const float* opacity_old, const float* scale_old, const void* N, int n_kind, int n_max, float* opacity_new,
                           float* scale_new, hipStream_t st, hipError_t* err);
int launch_mcmc_add_noise(int P, float* xyz, const float* scales, const float* rotations, const float* opacities, const float* noise, float noise_scale,
                          float k, float x0, int raw, hipStream_t st, hipError_t* err);
// Mip-Splatting's 3D filter (stp_mip_filter.hip) over arguments stp_mip_filter_3d / stp_mip_activations_forward / _backward have validated (P in
// [1, 2^31), C in [1, 2^24)); each returns the launches made, *err = the launch error (or hipSuccess)
int launch_mip_filter_3d(int P, int C, const float* xyz, const float* views, const float* intrinsics, void* workspace, float* filter_3d, hipStream_t st, hipError_t* err);
int launch_mip_activations_forward(int P, const float* scaling, const float* opacity, const float* filter_3d, float* scales, float* opacities, hipStream_t st,
                                   hipError_t* err);
int launch_mip_activations_backward(int P, const float* scaling, const float* opacity, const float* filter_3d, const float* grad_scales, const float* grad_opacities,
                                    float* grad_scaling, float* grad_opacity, hipStream_t st, hipError_t* err);
// the 3DGS-MCMC relocation and growth (stp_mcmc_relocate.hip) over arguments stp_mcmc_sample / stp_mcmc_relocate_apply / stp_mcmc_add_apply have
// validated (P in [1, 2^28], every written row count times row < 2^31, exactly one tensor of each of the roles 1 and 2, a scratch of
// mcmc_relocate_scratch_bytes(P) bytes, 16-byte aligned): each returns the launches made, *err = the launch error that ended it early (or
// hipSuccess).  No host synchronisation.  The applies pack their tensors with launch_row_tables and the sampling scans with block_exclusive /
// tile_prefix_kernel of stp_row_table.h, as the densification below does.
size_t mcmc_relocate_scratch_bytes(int P);
int launch_mcmc_sample(int P, const float* opacity, int rule, float min_opacity, int raw, int n_draws, const float* uniforms, void* scratch, uint32_t* weights,
                       int32_t* src, int32_t* count, hipStream_t st, hipError_t* err);
int launch_mcmc_relocate_apply(int P, const int32_t* src, const int32_t* count, int n_tensors, const StpMcmcTensor* tensors, float min_opacity, int raw,
                               int reset_dead_moments, void* scratch, hipStream_t st, hipError_t* err);
int launch_mcmc_add_apply(int P, int n_new, const int32_t* src, const int32_t* count, int n_tensors, const StpMcmcTensor* tensors, float min_opacity, int raw,
                          void* scratch, hipStream_t st, hipError_t* err);
// densification (stp_densify.hip) over arguments stp_densify_* have validated (P in [1, 2^31 / 3), every P * row < 2^31): each returns the
// launches made, *err = the error that ended it early (or hipSuccess).  launch_densify_scan copies the three counts to the host and
// SYNCHRONISES the stream; its scratch holds densify_scratch_bytes(P) bytes, 4-byte aligned.
int launch_densify_stats(int P, float* grad_accum, float* denom, float* max_radii2D, const float* grad2d, int grad_stride, const void* visible,
                         int visible_kind, hipStream_t st, hipError_t* err);
int launch_densify_plan(int P, const float* grad_accum, const float* denom, const float* scaling, const float* opacity, const float* max_radii2D,
                        const StpDensifyRule& rule, uint8_t* plan, hipStream_t st, hipError_t* err);
size_t densify_scratch_bytes(int P);
int launch_densify_scan(int P, const uint8_t* plan, void* scratch, uint32_t* offsets, int64_t counts[3], hipStream_t st, hipError_t* err);
int launch_densify_apply(int P, const uint8_t* plan, const uint32_t* offsets, const int64_t counts[3], int n_tensors, const StpDensifyTensor* tensors,
                         const float* noise, float split_shrink, int raw, hipStream_t st, hipError_t* err);
// the fused photometric loss (stp_loss.hip) over arguments stp_photometric_* have validated (planes * H * W in [1, 2^31)): workgroups of the
// tiled kernels (= rows of two partial sums in the workspace); the forward = tile kernel (with the three derivative maps when `maps`) + the
// one-workgroup sum, the backward = one tile kernel.  Both return the launches made, *err = the launch error that ended them early
uint32_t photometric_groups(int planes, int H, int W);
int launch_photometric_forward(int planes, int H, int W, const float* image, const float* target, float* out2, float* maps, float* workspace,
                               hipStream_t st, hipError_t* err);
int launch_photometric_backward(int planes, int H, int W, const float* image, const float* target, const float* maps, const float* dL_dout2,
                                float* dL_dimage, hipStream_t st, hipError_t* err);
// the training loss (stp_loss.hip) over arguments stp_training_loss_* have validated; `x` has every member in its final form (channels set,
// depth_planes = 0 without invdepth).  Without any extra the forward is the photometric tile kernel itself.  The workspace: two partial
// sums per colour workgroup, one per depth workgroup behind them (forward); 12 per (image, tile) workgroup (backward with dL_dexposure)
size_t training_loss_workspace_floats(int planes, int H, int W, int depth_planes);
int launch_training_loss_forward(int planes, int H, int W, const float* image, const float* target, const StpTrainingLoss& x, float* out3, float* maps,
                                 float* workspace, hipStream_t st, hipError_t* err);
int launch_training_loss_backward(int planes, int H, int W, const float* image, const float* target, const StpTrainingLoss& x, const float* maps,
                                  const float* dL_dout3, float* dL_dimage, float* dL_dexposure, float* dL_dinvdepth, float* workspace, hipStream_t st,
                                  hipError_t* err);

// the 3-nearest-neighbour mean squared distance (stp_knn.hip) over arguments stp_knn_mean_dist2 has validated (P in [4, 2^31), a scratch of
// knn_scratch_bytes(P) bytes, 16-byte aligned): returns the launches made (the library's sort counting as one), *err = the error that ended
// them early (or hipSuccess).  knn_scratch_bytes: 0 for P <= 0, non-decreasing in P, no overflow up to INT_MAX.
size_t knn_scratch_bytes(int P);
int launch_knn_mean_dist2(int P, const float* points, void* scratch, float* mean_dist2, hipStream_t st, hipError_t* err);
// the Morton order of a cloud (stp_knn.hip: steps 1-3 of the search above, shared with it) over arguments stp_spatial_order has validated (P in
// [1, 2^31), a scratch of spatial_order_scratch_bytes(P) bytes, 16-byte aligned; codes may be nullptr): returns the launches made, *err as
// above.  spatial_order_scratch_bytes: 0 for P <= 0, non-decreasing in P, no overflow up to INT_MAX.
size_t spatial_order_scratch_bytes(int P);
int launch_spatial_order(int P, const float* xyz, void* scratch, int32_t* order, uint32_t* codes, hipStream_t st, hipError_t* err);
// the gather of rows (stp_reorder.hip) over arguments stp_gather_rows has validated (P, M >= 1, P * row and M * row < 2^31, outputs that
// overlap no input): one launch per eight tensors through launch_row_tables; returns the launches made, *err = the launch error (or hipSuccess)
int launch_gather_rows(int P, int M, const int32_t* index, int n_tensors, const StpGatherTensor* tensors, hipStream_t st, hipError_t* err);

uint32_t higher_msb(uint32_t n);

} // namespace stp
