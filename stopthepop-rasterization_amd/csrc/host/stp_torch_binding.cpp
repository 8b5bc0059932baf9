// stp_torch_binding.cpp -- native host binding of libstp_raster.so for PyTorch-ROCm: the module
// `diff_gaussian_rasterization._stp_host` that `_C.py` delegates its three hot functions to.
//
// Replaces the reference's pybind layer (ext.cpp:15-19, rasterize_points.cu:33-253): same three functions, same argument
// and tuple orders (rasterize_points.h:26-82), tensors allocated through ATen, the current HIP stream taken from c10 --
// and NOTHING ELSE: no kernel lives here, every stage runs in libstp_raster.so behind its C ABI (include/stp_raster.h).
// It is a plain C++ translation unit built by g++ as a torch CppExtension (no .hip / .cu source, hence no hipify pass).
//
// Why it exists: the ctypes binding of rounds 1-2 spent 0.43 ms of host time per C1 step and 0.1 ms per C2 step on three
// Python allocator callbacks and ~35 argument conversions per call ("Host path").  Here the buffer-resize
// callbacks are C functions, and the scratch pool for the two large buffers (tile lists with their list-ordered entry
// records, image state with the blend log) lives in this file.
//
// The scratch pool.  Cycling a GB-sized block through torch's caching allocator every step invites splitting: smaller
// requests carve pieces off the free block, the next forward finds no hole of that size and the allocator falls back to
// hipMalloc (tens of ms per step -- observed on MI355X).  Buffers of >= 256 MiB are therefore kept on a small free list per
// device: handed out by the forward, handed back by the backward (release_scratch), capacities in steps of 64 MiB so that a
// buffer whose size follows num_rendered finds its predecessor.  Reuse across streams is ordered by an event recorded on
// the releasing stream; a generation counter per address lets the autograd function detect a backward that comes after
// its buffers were recycled (check_scratch).
#include <torch/extension.h>

#include <c10/hip/HIPCachingAllocator.h>
#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>

#include <cstdint>
#include <cstdlib>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../../include/stp_raster.h"

namespace {

constexpr int64_t BIG_BYTES = 256ll << 20, BIG_STEP = 64ll << 20;

struct Pooled { torch::Tensor t; hipEvent_t ev; }; // ev: recorded on the releasing stream (owned by g_events, never destroyed: creating an
                                                   // event can cost a driver call when the runtime's signal pool grows -- not per step)
std::mutex g_mutex;
std::map<int, std::vector<Pooled>> g_free;          // device -> free buffers (oldest first)
std::unordered_map<uintptr_t, int64_t> g_generation; // data_ptr -> how often the buffer at this address was handed out
std::unordered_map<uintptr_t, hipEvent_t> g_events;  // data_ptr -> the event that orders reuse of the buffer at this address
struct KeptRecords { torch::Tensor t; hipStream_t stream; };
std::map<int, KeptRecords> g_records;               // device -> the gradient-record buffer of the last whole backward (all zeros at rest)
int g_keep = 4;                                       // free buffers kept per device
int64_t g_max_bytes = -1;                             // optional cap on the pooled bytes per device

// The library is bound at RUN time (load_library, called by _C.py with the path it resolved: the in-tree libstp_raster.so,
// or STP_RASTER_LIB / _C.use_library for A/B runs and the test-only IEEE-depth build), not at link time.
struct Api {
    void* handle = nullptr;
    decltype(&stp_forward) forward = nullptr;
    decltype(&stp_backward_phases) backward_phases = nullptr;
    decltype(&stp_mark_visible) mark_visible = nullptr;
    decltype(&stp_last_error) last_error = nullptr;
    decltype(&stp_abi_version) abi_version = nullptr;
    decltype(&stp_forget_buffer) forget_buffer = nullptr;
    decltype(&stp_set_forward_split) set_forward_split = nullptr;
    // optional (an older library without them still loads; asking it for camera gradients raises)
    decltype(&stp_camera_grad_workspace_bytes) camera_grad_workspace_bytes = nullptr;
    decltype(&stp_set_backward_camera_grads) set_backward_camera_grads = nullptr;
    decltype(&stp_set_backward_absgrad) set_backward_absgrad = nullptr;
    decltype(&stp_set_backward_blend_stats) set_backward_blend_stats = nullptr;
    decltype(&stp_set_forward_background) set_forward_background = nullptr;
    decltype(&stp_set_backward_background) set_backward_background = nullptr;
    decltype(&stp_set_forward_invdepth) set_forward_invdepth = nullptr;
    decltype(&stp_set_backward_invdepth) set_backward_invdepth = nullptr;
    decltype(&stp_set_forward_split_sh) set_forward_split_sh = nullptr;
    decltype(&stp_set_backward_split_sh) set_backward_split_sh = nullptr;
    decltype(&stp_set_forward_sh_stash) set_forward_sh_stash = nullptr; // (a library with it also takes NULL for dL_dcolor / dL_dcov3D)
    decltype(&stp_sparse_adam) sparse_adam = nullptr;
    decltype(&stp_mcmc_relocation) mcmc_relocation = nullptr;
    decltype(&stp_mcmc_add_noise) mcmc_add_noise = nullptr;
    decltype(&stp_knn_scratch_bytes) knn_scratch_bytes = nullptr;
    decltype(&stp_knn_mean_dist2) knn_mean_dist2 = nullptr;
    decltype(&stp_densify_stats) densify_stats = nullptr;
    decltype(&stp_densify_plan) densify_plan = nullptr;
    decltype(&stp_densify_scratch_bytes) densify_scratch_bytes = nullptr;
    decltype(&stp_densify_scan) densify_scan = nullptr;
    decltype(&stp_densify_apply) densify_apply = nullptr;
    decltype(&stp_photometric_workspace_floats) photometric_workspace_floats = nullptr;
    decltype(&stp_photometric_forward) photometric_forward = nullptr;
    decltype(&stp_photometric_backward) photometric_backward = nullptr;
} g_api;

int load_library(const std::string& path)
{
    void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) throw std::runtime_error(std::string("cannot load ") + path + ": " + dlerror());
    Api a;
    a.handle = h;
    a.forward = reinterpret_cast<decltype(a.forward)>(dlsym(h, "stp_forward"));
    a.backward_phases = reinterpret_cast<decltype(a.backward_phases)>(dlsym(h, "stp_backward_phases"));
    a.mark_visible = reinterpret_cast<decltype(a.mark_visible)>(dlsym(h, "stp_mark_visible"));
    a.last_error = reinterpret_cast<decltype(a.last_error)>(dlsym(h, "stp_last_error"));
    a.abi_version = reinterpret_cast<decltype(a.abi_version)>(dlsym(h, "stp_abi_version"));
    a.forget_buffer = reinterpret_cast<decltype(a.forget_buffer)>(dlsym(h, "stp_forget_buffer"));
    a.set_forward_split = reinterpret_cast<decltype(a.set_forward_split)>(dlsym(h, "stp_set_forward_split"));
    if (!a.set_forward_split || !a.forget_buffer || !a.forward || !a.backward_phases || !a.mark_visible || !a.last_error || !a.abi_version)
        throw std::runtime_error(path + " does not export the C ABI of include/stp_raster.h");
    a.camera_grad_workspace_bytes = reinterpret_cast<decltype(a.camera_grad_workspace_bytes)>(dlsym(h, "stp_camera_grad_workspace_bytes"));
    a.set_backward_camera_grads = reinterpret_cast<decltype(a.set_backward_camera_grads)>(dlsym(h, "stp_set_backward_camera_grads"));
    a.set_backward_absgrad = reinterpret_cast<decltype(a.set_backward_absgrad)>(dlsym(h, "stp_set_backward_absgrad"));
    a.set_backward_blend_stats = reinterpret_cast<decltype(a.set_backward_blend_stats)>(dlsym(h, "stp_set_backward_blend_stats"));
    a.set_forward_background = reinterpret_cast<decltype(a.set_forward_background)>(dlsym(h, "stp_set_forward_background"));
    a.set_backward_background = reinterpret_cast<decltype(a.set_backward_background)>(dlsym(h, "stp_set_backward_background"));
    a.set_forward_invdepth = reinterpret_cast<decltype(a.set_forward_invdepth)>(dlsym(h, "stp_set_forward_invdepth"));
    a.set_backward_invdepth = reinterpret_cast<decltype(a.set_backward_invdepth)>(dlsym(h, "stp_set_backward_invdepth"));
    a.set_forward_split_sh = reinterpret_cast<decltype(a.set_forward_split_sh)>(dlsym(h, "stp_set_forward_split_sh"));
    a.set_backward_split_sh = reinterpret_cast<decltype(a.set_backward_split_sh)>(dlsym(h, "stp_set_backward_split_sh"));
    a.set_forward_sh_stash = reinterpret_cast<decltype(a.set_forward_sh_stash)>(dlsym(h, "stp_set_forward_sh_stash"));
    a.sparse_adam = reinterpret_cast<decltype(a.sparse_adam)>(dlsym(h, "stp_sparse_adam"));
    a.mcmc_relocation = reinterpret_cast<decltype(a.mcmc_relocation)>(dlsym(h, "stp_mcmc_relocation"));
    a.mcmc_add_noise = reinterpret_cast<decltype(a.mcmc_add_noise)>(dlsym(h, "stp_mcmc_add_noise"));
    a.knn_scratch_bytes = reinterpret_cast<decltype(a.knn_scratch_bytes)>(dlsym(h, "stp_knn_scratch_bytes"));
    a.knn_mean_dist2 = reinterpret_cast<decltype(a.knn_mean_dist2)>(dlsym(h, "stp_knn_mean_dist2"));
    a.densify_stats = reinterpret_cast<decltype(a.densify_stats)>(dlsym(h, "stp_densify_stats"));
    a.densify_plan = reinterpret_cast<decltype(a.densify_plan)>(dlsym(h, "stp_densify_plan"));
    a.densify_scratch_bytes = reinterpret_cast<decltype(a.densify_scratch_bytes)>(dlsym(h, "stp_densify_scratch_bytes"));
    a.densify_scan = reinterpret_cast<decltype(a.densify_scan)>(dlsym(h, "stp_densify_scan"));
    a.densify_apply = reinterpret_cast<decltype(a.densify_apply)>(dlsym(h, "stp_densify_apply"));
    a.photometric_workspace_floats = reinterpret_cast<decltype(a.photometric_workspace_floats)>(dlsym(h, "stp_photometric_workspace_floats"));
    a.photometric_forward = reinterpret_cast<decltype(a.photometric_forward)>(dlsym(h, "stp_photometric_forward"));
    a.photometric_backward = reinterpret_cast<decltype(a.photometric_backward)>(dlsym(h, "stp_photometric_backward"));
    if (a.abi_version() != STP_ABI_VERSION) throw std::runtime_error(path + ": ABI version mismatch");
    g_api = a; // (a previously loaded library stays mapped: buffers of its forwards may still be in flight)
    return a.abi_version();
}

void need_library()
{
    if (!g_api.forward) throw std::runtime_error("libstp_raster.so is not loaded (diff_gaussian_rasterization._C._load() does it); there is no CPU fallback");
}

[[noreturn]] void raise_last(int rc)
{
    const char* msg = g_api.last_error();
    throw std::runtime_error((msg && *msg) ? std::string(msg) : "libstp_raster error " + std::to_string(rc));
}

// A pooled buffer is used on whichever stream is current when it is handed out, not only on the stream torch::empty allocated it on: the caching
// allocator must know, or it could re-issue the block -- once the pool evicts it -- while kernels of another stream still read it.  (A no-op for
// the allocation stream itself, i.e. for single-stream training.)
void note_stream_use(const torch::Tensor& buf)
{
    c10::hip::HIPCachingAllocator::recordStream(buf.storage().data_ptr(), c10::hip::getCurrentHIPStream(buf.get_device()));
}

void put_back(const torch::Tensor& buf) // caller holds g_mutex
{
    auto& fl = g_free[buf.get_device()];
    for (auto& p : fl)
        if (p.t.data_ptr() == buf.data_ptr()) return;
    note_stream_use(buf);
    g_api.forget_buffer(buf.data_ptr()); // (its next tenant is described by what a forward carves there, or by the header a copy brings along)
    hipEvent_t& ev = g_events[(uintptr_t)buf.data_ptr()];
    if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
    bool recorded = ev && hipEventRecord(ev, c10::hip::getCurrentHIPStream(buf.get_device()).stream()) == hipSuccess;
    if (!recorded) (void)hipStreamSynchronize(c10::hip::getCurrentHIPStream(buf.get_device()).stream()); // (no event: order reuse the slow way)
    fl.push_back({buf, recorded ? ev : nullptr});
    auto total = [&]() { int64_t s = 0; for (auto& p : fl) s += p.t.numel(); return s; };
    while ((int)fl.size() > g_keep || (g_max_bytes >= 0 && fl.size() > 1 && total() > g_max_bytes)) fl.erase(fl.begin());
}

// The reference's resizeFunctional (rasterize_points.cu:33-41): grows a byte tensor on request.  The library may call the
// binning one twice per forward (a size guess before the num_rendered hand-over, the exact size afterwards if the guess
// was short: include/stp_raster.h): a request the current buffer already covers returns the same pointer.
// Which allocation a scratch buffer IS: the library caches (address, num_rendered) -> layout for the buffers its forwards carved, and
// an address alone does not say whose memory it is now -- a buffer is freed, a clone of ANOTHER forward's buffer lands on its address with the same
// num_rendered (static views repeat it exactly), and the stale entry would describe it.  The binding knows more than the address: it remembers the
// StorageImpl of every binning / image buffer its forwards returned (weak reference); a backward that is handed a tensor with another storage at a
// known address, or one whose storage has died since, tells the library to forget the address first, and the library reads the header the
// buffer carries (include/stp_raster.h: stp_forget_buffer).
std::unordered_map<uintptr_t, c10::weak_intrusive_ptr<c10::StorageImpl>> g_storage_of; // behind g_mutex
void remember_storage(const torch::Tensor& t)
{
    if (!t.defined() || t.numel() == 0) return;
    std::lock_guard<std::mutex> lock(g_mutex);
    if (g_storage_of.size() > 4096) // forwards whose buffers nobody came back for
        for (auto it = g_storage_of.begin(); it != g_storage_of.end();) it = it->second.expired() ? g_storage_of.erase(it) : std::next(it);
    g_storage_of.insert_or_assign((uintptr_t)t.data_ptr(), t.storage().getWeakStorageImpl());
}
void forget_unless_same_storage(const torch::Tensor& t)
{
    if (!t.defined() || t.numel() == 0) return;
    std::lock_guard<std::mutex> lock(g_mutex);
    const auto it = g_storage_of.find((uintptr_t)t.data_ptr());
    if (it != g_storage_of.end() && !it->second.expired() && it->second._unsafe_get_target() == t.storage().unsafeGetStorageImpl()) return;
    if (it != g_storage_of.end()) g_storage_of.erase(it);
    g_api.forget_buffer(t.data_ptr());
}

// Placement experiment (profiles/EXPERIMENTS.md, round 6: the k-buffer ring kernel's speed follows WHERE the frame's scratch buffers lie):
// STP_SCRATCH_OFFSET_GEOM / _BINNING / _IMAGE = bytes (multiple of 256, below 64 MiB) the buffer of that kind starts behind the start of its
// allocation.  Read at every request; unset or 0 = the allocation's own start.
constexpr int64_t OFFSET_SLACK = 64ll << 20;
int64_t scratch_offset(int kind)
{
    static const char* const names[3] = {"STP_SCRATCH_OFFSET_GEOM", "STP_SCRATCH_OFFSET_BINNING", "STP_SCRATCH_OFFSET_IMAGE"};
    const char* e = kind >= 0 && kind < 3 ? std::getenv(names[kind]) : nullptr;
    if (!e) return 0;
    const int64_t v = std::strtoll(e, nullptr, 0) & ~255ll;
    return v < 0 ? 0 : (v >= OFFSET_SLACK ? OFFSET_SLACK - 256 : v);
}
torch::Tensor empty_at_offset(int64_t n, const torch::TensorOptions& opt, int64_t off)
{
    return off ? torch::empty({n + OFFSET_SLACK}, opt).narrow(0, off, n) : torch::empty({n}, opt);
}

struct Resizer {
    torch::Tensor t;
    bool pooled = false, from_pool = false;
    int kind = -1;
    static void* call(void* user, size_t nbytes_)
    {
        auto* self = static_cast<Resizer*>(user);
        try {
            const int64_t nbytes = (int64_t)nbytes_;
            if (nbytes > 0 && nbytes <= self->t.numel()) return self->t.data_ptr();
            const int64_t off = scratch_offset(self->kind);
            if (self->pooled && nbytes >= BIG_BYTES) {
                std::lock_guard<std::mutex> lock(g_mutex);
                if (self->from_pool) put_back(self->t); // the guess was too small: the buffer goes back, a larger one comes
                const int64_t cap = (nbytes + BIG_STEP - 1) / BIG_STEP * BIG_STEP;
                auto& fl = g_free[self->t.get_device()];
                int hit = -1;
                for (int i = 0; i < (int)fl.size(); i++) {
                    const int64_t n = fl[i].t.numel();
                    if (n >= nbytes && n <= cap + cap / 4 && fl[i].t.storage_offset() == off && (hit < 0 || n < fl[hit].t.numel())) hit = i;
                }
                if (hit >= 0) {
                    Pooled p = fl[hit];
                    fl.erase(fl.begin() + hit);
                    if (p.ev) // the releasing stream's kernels may still be reading it: order this stream behind them
                        (void)hipStreamWaitEvent(c10::hip::getCurrentHIPStream(p.t.get_device()).stream(), p.ev, 0);
                    self->t = p.t;
                    note_stream_use(self->t);
                } else self->t = empty_at_offset(cap, self->t.options(), off);
                self->from_pool = true;
                g_generation[(uintptr_t)self->t.data_ptr()]++;
                return self->t.data_ptr();
            }
            if (off && nbytes) self->t = empty_at_offset(nbytes, self->t.options(), off);
            else self->t.resize_({nbytes});
            return nbytes ? self->t.data_ptr() : nullptr;
        } catch (...) { // surfaces as STP_ERR_ALLOC on the C side
            return nullptr;
        }
    }
};

const float* fptr(const torch::Tensor& t) // empty tensor -> NULL (reference convention: `torch.Tensor([])` marks an absent optional input)
{
    return t.defined() && t.numel() != 0 ? t.data_ptr<float>() : nullptr;
}

torch::Tensor prep(const torch::Tensor& t, const torch::Device& dev)
{
    if (!t.defined() || t.numel() == 0) return t;
    TORCH_CHECK(t.device() == dev, "expected all tensors on ", dev, ", got one on ", t.device());
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, "expected float32 tensor, got ", t.scalar_type());
    return t.contiguous();
}

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
    if (d.contains("_tile_rows") && !d["_tile_rows"].is_none()) {
        const py::tuple tr = py::tuple(d["_tile_rows"]);
        s.tile_y0 = tr[0].cast<int>();
        s.tile_y1 = tr[1].cast<int>();
    }
    s.record_blend_log = record_log ? 1 : 0;
    return s;
}

// a background of shape exactly (3, H, W) is a per-pixel one (include/stp_raster.h: stp_set_forward_background); every other is three floats
bool per_pixel_background(const torch::Tensor& bg, int H, int W)
{
    return bg.defined() && bg.dim() == 3 && bg.size(0) == 3 && bg.size(1) == H && bg.size(2) == W;
}
[[noreturn]] void raise_no_background_export(const char* name)
{
    throw std::runtime_error(std::string("alpha / background: the loaded libstp_raster.so does not export ") + name +
                             " (a library built before the alpha output and per-pixel background): rebuild it");
}

// dc (extension, include/stp_raster.h: stp_set_forward_split_sh / stp_set_backward_split_sh): the first SH coefficient as a tensor of its own,
// (P,1,3) or (P,3); `sh` is then the rest, (P,M-1,3), possibly empty.  Returns M, the total coefficient count.  Checked before any device work.
int split_sh_total(const torch::Tensor& dc, const torch::Tensor& sh, const torch::Tensor& means3D, const char* symbol, bool exported)
{
    if (!exported)
        throw std::runtime_error(std::string("dc: the loaded libstp_raster.so does not export ") + symbol + " (a library built before split SH inputs): rebuild it");
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
std::tuple<int, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>
rasterize_gaussians(const torch::Tensor& background, const torch::Tensor& means3D, const torch::Tensor& colors, const torch::Tensor& opacity,
                    const torch::Tensor& scales, const torch::Tensor& rotations, const float scale_modifier, const torch::Tensor& cov3D_precomp,
                    const torch::Tensor& viewmatrix, const torch::Tensor& projmatrix, const torch::Tensor& inv_viewprojmatrix, const float tan_fovx,
                    const float tan_fovy, const int image_height, const int image_width, const torch::Tensor& sh, const int degree,
                    const torch::Tensor& campos, const bool prefiltered, const py::dict& settings, const bool render_depth, const bool debug,
                    const bool record_log, const bool alpha, const bool invdepth, const c10::optional<torch::Tensor>& dc)
{
    need_library();
    TORCH_CHECK(means3D.dim() == 2 && means3D.size(1) == 3, "means3D must have dimensions (num_points, 3)");
    TORCH_CHECK(means3D.is_cuda(), "diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product");
    const bool split = dc.has_value() && dc->defined() && colors.numel() == 0; // (precomputed colours win)
    const int M_split = split ? split_sh_total(*dc, sh, means3D, "stp_set_forward_split_sh", g_api.set_forward_split_sh != nullptr) : 0;
    const torch::Device dev = means3D.device();
    const int P = (int)means3D.size(0), H = image_height, W = image_width;
    const bool windowed = settings.contains("_tile_rows") && !settings["_tile_rows"].is_none();
    const auto fopt = means3D.options().dtype(torch::kFloat32), iopt = means3D.options().dtype(torch::kInt32), bopt = means3D.options().dtype(torch::kByte);
    // the render kernels write every pixel of the tile rows they cover and preprocess writes every Gaussian's radius:
    // zero-filled outputs are only needed when nothing runs (P == 0) or when a tile-row window leaves rows untouched
    const bool zero = P == 0 || windowed;
    torch::Tensor out_color = zero ? torch::zeros({3, H, W}, fopt) : torch::empty({3, H, W}, fopt);
    torch::Tensor radii = zero ? torch::zeros({P}, iopt) : torch::empty({P}, iopt);
    const bool bg_pixels = per_pixel_background(background, H, W);
    if ((alpha || bg_pixels) && !g_api.set_forward_background) raise_no_background_export("stp_set_forward_background");
    torch::Tensor out_alpha; // (like the image: every pixel of the rendered tile rows is written)
    if (alpha) out_alpha = zero ? torch::zeros({1, H, W}, fopt) : torch::empty({1, H, W}, fopt);
    if (invdepth) {
        if (!g_api.set_forward_invdepth)
            throw std::runtime_error("invdepth: the loaded libstp_raster.so does not export stp_set_forward_invdepth (a library built before the inverse-depth output): rebuild it");
        if (render_depth) throw std::runtime_error("the inverse-depth output is not available with render_depth (the debug depth visualisation)");
    }
    torch::Tensor out_invdepth; // (like the image: every pixel of the rendered tile rows is written)
    if (invdepth) out_invdepth = zero ? torch::zeros({1, H, W}, fopt) : torch::empty({1, H, W}, fopt);
    // The SH stash (include/stp_raster.h: stp_set_forward_sh_stash) is asked for exactly when a backward can follow -- the autograd layer's
    // condition for asking for the blend log, settings._record_blend_log, or, where its policy or the sort mode rules the log out, its
    // settings._sh_stash -- and the library exports the request; settings._no_sh_stash = True keeps a differentiable forward on the legacy
    // path (tests compare the two).  An inference forward asks for nothing.
    auto flag = [&](const char* key) { return settings.contains(key) && !settings[key].is_none() && settings[key].cast<bool>(); };
    const bool sh_stash = (flag("_record_blend_log") || flag("_sh_stash")) && !flag("_no_sh_stash") && !render_depth && g_api.set_forward_sh_stash != nullptr;
    Resizer geom{torch::empty({0}, bopt), false, false, 0}, binning{torch::empty({0}, bopt), true, false, 1}, img{torch::empty({0}, bopt), true, false, 2};
    int rendered = 0;
    if (P != 0) {
        const int M = split ? M_split : sh.numel() != 0 ? (int)sh.size(1) : 0;
        StpSettings s = settings_from_dict(settings, record_log);
        if (render_depth) { // DebugVisualization::Depth (reference rasterize_points.cu:104-107); no log: it has no backward
            s.debug_visualization = STP_DEBUG_DEPTH;
            s.record_blend_log = 0;
        }
        const torch::Tensor bg_ = prep(background, dev), m3_ = prep(means3D, dev), sh_ = prep(sh, dev), col_ = prep(colors, dev), op_ = prep(opacity, dev),
                            sc_ = prep(scales, dev), ro_ = prep(rotations, dev), c3_ = prep(cov3D_precomp, dev), vm_ = prep(viewmatrix, dev),
                            pm_ = prep(projmatrix, dev), inv_ = prep(inv_viewprojmatrix, dev), cam_ = prep(campos, dev);
        torch::Tensor dc_;
        if (split) dc_ = prep(*dc, dev);
        const c10::hip::HIPGuard guard(dev.index());
        hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
        int rc;
        {
            py::gil_scoped_release nogil; // (the call blocks once, on the num_rendered hand-over)
            if (alpha || bg_pixels) // (consumed by the call below, on this thread)
                g_api.set_forward_background(bg_pixels ? fptr(bg_) : nullptr, alpha ? out_alpha.data_ptr<float>() : nullptr);
            if (invdepth) g_api.set_forward_invdepth(out_invdepth.data_ptr<float>());
            if (split) g_api.set_forward_split_sh(dc_.data_ptr<float>());
            if (sh_stash) g_api.set_forward_sh_stash(1);
            rc = g_api.forward(&Resizer::call, &geom, &Resizer::call, &binning, &Resizer::call, &img, P, degree, M, fptr(bg_), W, H, &s, fptr(m3_),
                             fptr(sh_), fptr(col_), fptr(op_), fptr(sc_), scale_modifier, fptr(ro_), fptr(c3_), fptr(vm_), fptr(pm_), fptr(inv_),
                             fptr(cam_), tan_fovx, tan_fovy, prefiltered ? 1 : 0, out_color.data_ptr<float>(), radii.data_ptr<int>(), debug ? 1 : 0,
                             (void*)stream);
        }
        if (rc < 0) raise_last(rc);
        rendered = rc;
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
                             const c10::optional<torch::Tensor>& dc)
{
    need_library();
    TORCH_CHECK(means3D.is_cuda(), "diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product");
    const bool split = dc.has_value() && dc->defined() && colors.numel() == 0 && (phases & 2); // (precomputed colours win; the render half reads no SH)
    const int M_split = split ? split_sh_total(*dc, sh, means3D, "stp_set_backward_split_sh", g_api.set_backward_split_sh != nullptr) : 0;
    if (camera_grads) {
        if (!g_api.set_backward_camera_grads || !g_api.camera_grad_workspace_bytes)
            throw std::runtime_error(std::string("camera gradients: the loaded libstp_raster.so does not export ") +
                                     (g_api.set_backward_camera_grads ? "stp_camera_grad_workspace_bytes" : "stp_set_backward_camera_grads") + "; rebuild it");
        TORCH_CHECK(phases & 2, "camera gradients come from the per-Gaussian half (phases bit 1)");
    }
    if (absgrad) {
        if (!g_api.set_backward_absgrad)
            throw std::runtime_error("absgrad: the loaded libstp_raster.so does not export stp_set_backward_absgrad (a library built before absgrad): rebuild it");
        // (the render half leaves the two sums in the records it has just filled and the per-Gaussian half of the SAME call collects them: a
        // half on its own would need the caller to carry request and records from one call to the other)
        TORCH_CHECK((phases & 3) == 3, "absgrad needs both halves of the backward in one call (phases bits 0 and 1)");
    }
    if (blend_stats) {
        if (!g_api.set_backward_blend_stats)
            throw std::runtime_error("blend_stats: the loaded libstp_raster.so does not export stp_set_backward_blend_stats (a library built before blend statistics): rebuild it");
        TORCH_CHECK((phases & 3) == 3, "blend_stats needs both halves of the backward in one call (phases bits 0 and 1)");
    }
    const torch::Device dev = means3D.device();
    const int P = (int)means3D.size(0);
    const int H = (int)dL_dout_color.size(1), W = (int)dL_dout_color.size(2);
    const bool bg_pixels = per_pixel_background(background, H, W);
    const bool have_dalpha = dL_dalpha.has_value() && dL_dalpha->defined();
    if (bg_pixels || have_dalpha || bg_grad) {
        if (!g_api.set_backward_background) raise_no_background_export("stp_set_backward_background");
        TORCH_CHECK(phases & 1, "alpha gradient / per-pixel background / background gradient belong to the render half (phases bit 0)");
        TORCH_CHECK(!have_dalpha || dL_dalpha->numel() == (int64_t)H * W, "dL_dalpha must have H * W elements");
    }
    const bool have_dinv = dL_dinvdepth.has_value() && dL_dinvdepth->defined();
    if (have_dinv) {
        if (!g_api.set_backward_invdepth)
            throw std::runtime_error("invdepth: the loaded libstp_raster.so does not export stp_set_backward_invdepth (a library built before the inverse-depth output): rebuild it");
        TORCH_CHECK((phases & 3) == 3, "the inverse-depth gradient needs both halves of the backward in one call (phases bits 0 and 1)");
        TORCH_CHECK(invdepth.has_value() && invdepth->defined(), "dL_dinvdepth needs the forward's invdepth");
        TORCH_CHECK(dL_dinvdepth->numel() == (int64_t)H * W && invdepth->numel() == (int64_t)H * W, "dL_dinvdepth and invdepth must have H * W elements");
    }
    const int M = split ? M_split : sh.numel() != 0 ? (int)sh.size(1) : 0;
    const auto fopt = means3D.options().dtype(torch::kFloat32);
    const int rec_floats = (phases & 4) ? STP_GRAD_RECORD_USED : STP_GRAD_RECORD_FLOATS; // (bit 2: compact records, the tile-row shard's wire format)
    // STP_KEEP_RECORDS=1 (MEASURED, round 4, off): a whole backward keeps its record buffer between steps and the per-Gaussian half clears what
    // it reads (phases bit 3), so that the 64 B per Gaussian are zero-filled once, not every step.  One buffer per device, reused only by the
    // stream that used it last and only at the same size.  The clearing stores cost the per-Gaussian kernel more than torch's fill saves:
    // C2-full step 2.376 -> 2.384 ms (BwdPreprocess 0.116 -> 0.126), C5 6.25 -> 6.39 ms (0.72-0.80 -> 0.90), C3 unchanged
    // (profiles/r04_keep_records_ab.txt) -- a 7 TB/s fill kernel is hard to beat with scattered 48-byte stores.
    static const bool keep_enabled = [] { const char* e = std::getenv("STP_KEEP_RECORDS"); return e && e[0] == '1'; }();
    const bool keep_records = keep_enabled && phases == 3 && !partial.has_value() && P != 0;
    torch::Tensor records;
    hipStream_t rec_stream = nullptr;
    if (keep_records) {
        rec_stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
        std::lock_guard<std::mutex> lock(g_mutex);
        auto it = g_records.find(dev.index());
        if (it != g_records.end() && it->second.stream == rec_stream && it->second.t.size(0) == P && it->second.t.size(1) == rec_floats) records = it->second.t;
        if (it != g_records.end()) g_records.erase(it); // (in use, or superseded)
    }
    if (!records.defined()) records = partial.has_value() ? *partial : torch::zeros({P, rec_floats}, fopt);
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
        const bool have_scales = scales.numel() != 0;
        auto omitted = [&](const char* key) { return g_api.set_forward_sh_stash != nullptr && settings.contains(key) && settings[key].cast<bool>(); };
        const bool no_dcolors = omitted("_no_grad_colors") && colors.numel() == 0, no_dcov3D = omitted("_no_grad_cov3D") && cov3D_precomp.numel() == 0;
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
    torch::Tensor dL_dmeans2D_abs;
    if (absgrad) dL_dmeans2D_abs = torch::empty({P, 3}, fopt); // written in full by the library (zeros for invisible Gaussians)
    torch::Tensor stats;
    if (blend_stats) stats = torch::empty({P, 3}, fopt); // written in full by the library (zeros for invisible Gaussians)
    torch::Tensor dL_dbg, dal_, bgpix_;
    if (bg_grad) { // written in full by the library, except where nothing runs (P == 0) or a tile-row window leaves rows untouched
        const std::vector<int64_t> shape = bg_pixels ? std::vector<int64_t>{3, H, W} : std::vector<int64_t>{3};
        const bool windowed = settings.contains("_tile_rows") && !settings["_tile_rows"].is_none();
        dL_dbg = (P == 0 || (bg_pixels && windowed)) ? torch::zeros(shape, fopt) : torch::empty(shape, fopt);
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
        if (blend_stats && P != 0) g_api.set_backward_blend_stats(stats.data_ptr<float>());
        if (absgrad && P != 0) g_api.set_backward_absgrad(dL_dmeans2D_abs.data_ptr<float>());
        if (camera_grads) g_api.set_backward_camera_grads(dL_dview.data_ptr<float>(), dL_dproj.data_ptr<float>(), dL_dcam.data_ptr<float>(), cam_ws.data_ptr(), (size_t)cam_ws.numel());
    };
    if (P == 0 && camera_grads) { // nothing to differentiate: the library writes the zeros
        const c10::hip::HIPGuard guard(dev.index());
        hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
        make_requests();
        const int rc = g_api.backward_phases(phases, 0, degree, M, R, nullptr, W, H, &s, nullptr, nullptr, nullptr, nullptr, nullptr, scale_modifier, nullptr,
                                           nullptr, nullptr, nullptr, nullptr, nullptr, tan_fovx, tan_fovy, nullptr, nullptr, nullptr, nullptr, nullptr,
                                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, debug ? 1 : 0, (void*)stream);
        if (rc < 0) raise_last(rc);
    }
    if (P != 0) {
        const torch::Tensor bg_ = prep(background, dev), m3_ = prep(means3D, dev), sh_ = prep(sh, dev), col_ = prep(colors, dev), op_ = prep(opacities, dev),
                            sc_ = prep(scales, dev), ro_ = prep(rotations, dev), c3_ = prep(cov3D_precomp, dev), vm_ = prep(viewmatrix, dev),
                            pm_ = prep(projmatrix, dev), inv_ = prep(inv_viewprojmatrix, dev), cam_ = prep(campos, dev), pix_ = prep(pixel_colors, dev),
                            dl_ = prep(dL_dout_color, dev);
        const torch::Tensor radii_ = radii.contiguous();
        auto optf = [](const torch::Tensor& t) -> float* { return t.defined() && t.numel() != 0 ? t.data_ptr<float>() : nullptr; };
        auto optb = [](const torch::Tensor& t) -> char* { return t.defined() && t.numel() != 0 ? reinterpret_cast<char*>(t.data_ptr()) : nullptr; };
        const c10::hip::HIPGuard guard(dev.index());
        hipStream_t stream = c10::hip::getCurrentHIPStream(dev.index()).stream();
        forget_unless_same_storage(geomBuffer); // (whether it carries an SH stash)
        forget_unless_same_storage(binningBuffer); // (a clone, a copy or a recycled address: the library then reads the buffer's own header)
        forget_unless_same_storage(imageBuffer);
        make_requests(); // (consumed by the call below, on this thread)
        const int rc = g_api.backward_phases(keep_records ? (phases | 8) : phases, P, degree, M, R, fptr(bg_), W, H, &s, fptr(m3_), fptr(sh_), fptr(op_), fptr(col_), fptr(sc_),
                                           scale_modifier, fptr(ro_), fptr(c3_), fptr(vm_), fptr(pm_), fptr(inv_), fptr(cam_), tan_fovx, tan_fovy,
                                           fptr(pix_), radii_.numel() ? radii_.data_ptr<int>() : nullptr, optb(geomBuffer), optb(binningBuffer),
                                           optb(imageBuffer), fptr(dl_), optf(dL_dmeans2D), records.data_ptr<float>(), optf(dL_dopacity), optf(dL_dcolors),
                                           optf(dL_dmeans3D), optf(dL_dcov3D), optf(dL_dsh), optf(dL_dscales), optf(dL_drotations), debug ? 1 : 0,
                                           (void*)stream);
        if (rc < 0) raise_last(rc);
        if (keep_records) { // all zeros again once the kernels just enqueued have run
            std::lock_guard<std::mutex> lock(g_mutex);
            g_records[dev.index()] = KeptRecords{records, rec_stream};
        }
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
    TORCH_CHECK(means3D.is_cuda(), "diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product");
    const torch::Device dev = means3D.device();
    const int P = (int)means3D.size(0);
    torch::Tensor present = torch::zeros({P}, means3D.options().dtype(torch::kBool));
    if (P != 0) {
        const torch::Tensor m3_ = prep(means3D, dev), vm_ = prep(viewmatrix, dev), pm_ = prep(projmatrix, dev);
        const c10::hip::HIPGuard guard(dev.index());
        const int rc = g_api.mark_visible(P, fptr(m3_), fptr(vm_), fptr(pm_), reinterpret_cast<uint8_t*>(present.data_ptr()),
                                        (void*)c10::hip::getCurrentHIPStream(dev.index()).stream());
        if (rc < 0) raise_last(rc);
    }
    return present;
}

// == the fused sparse Adam step (extension, include/stp_raster.h: stp_sparse_adam; the step of SparseGaussianAdam in __init__.py): one library call
// for all quadruples (param, grad, exp_avg, exp_avg_sq), on the caller's current stream.  visible: bool / uint8 (non-zero = visible) or the
// int32 radii of the forward (> 0 = visible), N elements, read as it is.  Returns the kernel launches the library made.
int sparse_adam(const std::vector<torch::Tensor>& params, const std::vector<torch::Tensor>& grads, const std::vector<torch::Tensor>& exp_avgs,
                const std::vector<torch::Tensor>& exp_avg_sqs, const torch::Tensor& visible, const std::vector<double>& lrs, const std::vector<double>& epss,
                const double beta1, const double beta2, const int64_t N)
{
    need_library();
    if (!g_api.sparse_adam)
        throw std::runtime_error("sparse_adam: the loaded libstp_raster.so does not export stp_sparse_adam (a library built before the sparse Adam step): rebuild it");
    const size_t n = params.size();
    TORCH_CHECK(grads.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n && lrs.size() == n && epss.size() == n,
                "sparse_adam: params, grads, exp_avgs, exp_avg_sqs, lrs and epss must have one entry per tensor");
    TORCH_CHECK(N >= 0 && N < (1ll << 31), "sparse_adam: N out of range");
    TORCH_CHECK(visible.defined() && visible.is_cuda(), "diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product");
    const torch::Device dev = visible.device();
    const auto vt = visible.scalar_type();
    TORCH_CHECK(vt == torch::kBool || vt == torch::kByte || vt == torch::kInt32, "sparse_adam: visible must be bool, uint8 or int32 (radii), got ", vt);
    TORCH_CHECK(visible.numel() == N && visible.is_contiguous(), "sparse_adam: visible must be contiguous with N = ", N, " elements, got ", visible.numel());
    std::vector<StpAdamTensor> table(n);
    for (size_t k = 0; k < n; k++) {
        const torch::Tensor* quad[4] = {&params[k], &grads[k], &exp_avgs[k], &exp_avg_sqs[k]};
        static const char* const names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
        for (int j = 0; j < 4; j++) {
            const torch::Tensor& t = *quad[j];
            TORCH_CHECK(t.defined(), "sparse_adam: tensor ", k, ": ", names[j], " is undefined");
            TORCH_CHECK(t.is_cuda(), "diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product");
            TORCH_CHECK(t.device() == dev, "expected all tensors on ", dev, ", got one on ", t.device());
            TORCH_CHECK(t.scalar_type() == torch::kFloat32, "expected float32 tensor, got ", t.scalar_type());
            TORCH_CHECK(t.is_contiguous(), "sparse_adam: tensor ", k, ": ", names[j], " must be contiguous (it is updated in place)");
            TORCH_CHECK(t.sizes() == params[k].sizes(), "sparse_adam: tensor ", k, ": ", names[j], " has shape ", t.sizes(), ", param has ", params[k].sizes());
        }
        table[k] = StpAdamTensor{params[k].data_ptr<float>(), grads[k].data_ptr<float>(), exp_avgs[k].data_ptr<float>(), exp_avg_sqs[k].data_ptr<float>(),
                                 (long long)params[k].numel(), (float)lrs[k], (float)epss[k]};
    }
    const c10::hip::HIPGuard guard(dev.index());
    const int rc = g_api.sparse_adam((int)n, table.data(), (int)N, visible.data_ptr(), vt == torch::kInt32 ? 1 : 0, (float)beta1, (float)beta2,
                                     (void*)c10::hip::getCurrentHIPStream(dev.index()).stream());
    if (rc < 0) raise_last(rc);
    return rc;
}

// == the 3DGS-MCMC kernels (extension, include/stp_raster.h: stp_mcmc_relocation / stp_mcmc_add_noise; compute_relocation and mcmc_add_noise_ in
// __init__.py), on the caller's current stream.  What is wrong with the tensors themselves is refused first, where they live last: every refusal
// can be met without a GPU.
static void mcmc_check_float(const char* who, const char* name, const torch::Tensor& t)
{
    TORCH_CHECK(t.defined(), who, ": ", name, " must be a tensor");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, who, ": ", name, ": expected float32 tensor, got ", t.scalar_type());
}
static void mcmc_check_rows(const char* who, const char* name, const torch::Tensor& t, const int64_t rows, const int64_t width)
{
    TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == width, who, ": ", name, " must be (", rows, ", ", width, "), got ", t.sizes());
}
static void mcmc_check_column(const char* who, const char* name, const torch::Tensor& t)
{
    TORCH_CHECK(t.dim() == 1 || (t.dim() == 2 && t.size(1) == 1), who, ": ", name, " must be (n,) or (n, 1), got ", t.sizes());
}
static void mcmc_check_device(const char* who, const char* name, const torch::Tensor& t, const torch::Tensor& first)
{
    TORCH_CHECK(t.device() == first.device(), who, ": ", name, ": expected all tensors on ", first.device(), ", got one on ", t.device());
    TORCH_CHECK(t.is_cuda(), who, ": ", name, ": diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product");
}

// -> (opacity_new of opacity_old's shape, scale_new (n, 3)); upstream's name and argument order.  binoms: checked for its shape only -- the kernel
// has its own binomials -- and n_max is the clamp's upper bound plus one.  N is NOT clamped in place (upstream's is).
std::tuple<torch::Tensor, torch::Tensor> compute_relocation(const torch::Tensor& opacity_old, const torch::Tensor& scale_old, const torch::Tensor& N,
                                                            const c10::optional<torch::Tensor>& binoms_in, const int64_t n_max)
{
    static const char* const who = "compute_relocation";
    need_library();
    if (!g_api.mcmc_relocation)
        throw std::runtime_error("compute_relocation: the loaded libstp_raster.so does not export stp_mcmc_relocation (a library built before the 3DGS-MCMC kernels): rebuild it");
    mcmc_check_float(who, "opacity_old", opacity_old);
    mcmc_check_float(who, "scale_old", scale_old);
    TORCH_CHECK(N.defined() && (N.scalar_type() == torch::kInt32 || N.scalar_type() == torch::kInt64), who, ": N: expected int32 or int64 tensor, got ", N.scalar_type());
    TORCH_CHECK(n_max >= 2 && n_max <= 51, who, ": n_max must be in [2, 51], got ", n_max);
    if (binoms_in.has_value()) {
        const torch::Tensor& binoms = *binoms_in;
        mcmc_check_float(who, "binoms", binoms);
        TORCH_CHECK(binoms.dim() == 2 && binoms.size(0) == n_max && binoms.size(1) == n_max, who, ": binoms must be (n_max, n_max) = (", n_max, ", ", n_max, "), got ", binoms.sizes());
    }
    mcmc_check_column(who, "opacity_old", opacity_old);
    mcmc_check_column(who, "N", N);
    const int64_t n = opacity_old.size(0);
    TORCH_CHECK(n < (1ll << 31), who, ": opacity_old: ", n, " rows >= 2^31");
    mcmc_check_rows(who, "scale_old", scale_old, n, 3);
    TORCH_CHECK(N.size(0) == n, who, ": N has ", N.size(0), " rows, opacity_old has ", n);
    mcmc_check_device(who, "scale_old", scale_old, opacity_old);
    mcmc_check_device(who, "N", N, opacity_old);
    mcmc_check_device(who, "opacity_old", opacity_old, opacity_old);
    const torch::Tensor o = opacity_old.contiguous(), s = scale_old.contiguous(), cnt = N.contiguous();
    const c10::hip::HIPGuard guard(o.device().index());
    torch::Tensor o_new = torch::empty(o.sizes(), o.options()), s_new = torch::empty(s.sizes(), s.options());
    if (n == 0) return {o_new, s_new};
    const int rc = g_api.mcmc_relocation((int)n, o.data_ptr<float>(), s.data_ptr<float>(), cnt.data_ptr(), cnt.scalar_type() == torch::kInt64 ? 1 : 0, (int)n_max,
                                         o_new.data_ptr<float>(), s_new.data_ptr<float>(), (void*)c10::hip::getCurrentHIPStream(o.device().index()).stream());
    if (rc < 0) raise_last(rc);
    return {o_new, s_new};
}

// in place on xyz (which must be contiguous: it is updated where it lies); the other four are made contiguous.  Returns the launches made.
int mcmc_add_noise(const torch::Tensor& xyz, const torch::Tensor& scales, const torch::Tensor& rotations, const torch::Tensor& opacities,
                   const torch::Tensor& noise, const double noise_scale, const double k, const double x0, const bool raw)
{
    static const char* const who = "mcmc_add_noise";
    need_library();
    if (!g_api.mcmc_add_noise)
        throw std::runtime_error("mcmc_add_noise: the loaded libstp_raster.so does not export stp_mcmc_add_noise (a library built before the 3DGS-MCMC kernels): rebuild it");
    const torch::Tensor* all[5] = {&xyz, &scales, &rotations, &opacities, &noise};
    static const char* const names[5] = {"xyz", "scales", "rotations", "opacities", "noise"};
    for (int j = 0; j < 5; j++) mcmc_check_float(who, names[j], *all[j]);
    TORCH_CHECK(xyz.dim() == 2 && xyz.size(1) == 3, who, ": xyz must be (P, 3), got ", xyz.sizes());
    const int64_t P = xyz.size(0);
    TORCH_CHECK(P < (1ll << 31), who, ": xyz: ", P, " rows >= 2^31");
    mcmc_check_rows(who, "scales", scales, P, 3);
    mcmc_check_rows(who, "rotations", rotations, P, 4);
    mcmc_check_rows(who, "noise", noise, P, 3);
    mcmc_check_column(who, "opacities", opacities);
    TORCH_CHECK(opacities.size(0) == P, who, ": opacities has ", opacities.size(0), " rows, xyz has ", P);
    for (int j = 1; j < 5; j++) mcmc_check_device(who, names[j], *all[j], xyz);
    mcmc_check_device(who, "xyz", xyz, xyz);
    TORCH_CHECK(xyz.is_contiguous(), who, ": xyz must be contiguous (it is updated in place)");
    if (P == 0) return 0;
    const torch::Tensor s = scales.contiguous(), q = rotations.contiguous(), o = opacities.contiguous(), w = noise.contiguous();
    const c10::hip::HIPGuard guard(xyz.device().index());
    const int rc = g_api.mcmc_add_noise((int)P, xyz.data_ptr<float>(), s.data_ptr<float>(), q.data_ptr<float>(), o.data_ptr<float>(), w.data_ptr<float>(),
                                        (float)noise_scale, (float)k, (float)x0, raw ? 1 : 0, (void*)c10::hip::getCurrentHIPStream(xyz.device().index()).stream());
    if (rc < 0) raise_last(rc);
    return rc;
}

// == simple_knn's distCUDA2 (extension, include/stp_raster.h: stp_knn_mean_dist2; knn_mean_dist2 in __init__.py and simple_knn._C.distCUDA2), on the
// caller's current stream: -> (P,) float32, the mean of the three smallest squared distances to the other points, in input order.  The scratch is
// a torch tensor of the caching allocator, returned to it when this function leaves (the allocator keeps it for the stream until the kernels
// have run).  No host synchronisation.
torch::Tensor knn_mean_dist2(const torch::Tensor& points_in)
{
    static const char* const who = "knn_mean_dist2";
    need_library();
    if (!g_api.knn_mean_dist2 || !g_api.knn_scratch_bytes)
        throw std::runtime_error("knn_mean_dist2: the loaded libstp_raster.so does not export stp_knn_mean_dist2 (a library built before the nearest-neighbour kernels): rebuild it");
    mcmc_check_float(who, "points", points_in);
    TORCH_CHECK(points_in.dim() == 2 && points_in.size(1) == 3, who, ": points must be (P, 3), got ", points_in.sizes());
    const int64_t P = points_in.size(0);
    TORCH_CHECK(P < (1ll << 31), who, ": points: ", P, " rows >= 2^31");
    TORCH_CHECK(P == 0 || P >= 4, who, ": points: ", P, " rows: the mean over three neighbours needs at least 4 points");
    mcmc_check_device(who, "points", points_in, points_in);
    const torch::Tensor points = points_in.detach().contiguous();
    const c10::hip::HIPGuard guard(points.device().index());
    torch::Tensor out = torch::empty({P}, points.options());
    if (P == 0) return out;
    const size_t bytes = g_api.knn_scratch_bytes((int)P);
    torch::Tensor scratch = torch::empty({(int64_t)bytes}, points.options().dtype(torch::kByte));
    const int rc = g_api.knn_mean_dist2((int)P, points.data_ptr<float>(), scratch.data_ptr(), bytes, out.data_ptr<float>(),
                                        (void*)c10::hip::getCurrentHIPStream(points.device().index()).stream());
    if (rc < 0) raise_last(rc);
    return out;
}

// == densification (extension, include/stp_raster.h: stp_densify_stats / _plan / _scan / _apply; densification_stats_, densify_plan,
// densify_tensors and densify_and_prune in __init__.py), on the caller's current stream.  As above, what is wrong with the tensors themselves is
// refused first and where they live last.  Only densify_scan synchronises with the host (inside the library: the new row count).
static const char* const DENSIFY_REBUILD = " (a library built before the densification kernels): rebuild it";
static void densify_check_column(const char* who, const char* name, const torch::Tensor& t, const int64_t P)
{
    mcmc_check_float(who, name, t);
    mcmc_check_column(who, name, t);
    TORCH_CHECK(t.size(0) == P, who, ": ", name, " has ", t.size(0), " rows, expected ", P);
}
static void densify_check_P(const char* who, const int64_t P) { TORCH_CHECK(3 * P < (1ll << 31), who, ": ", P, " rows: 3 P >= 2^31"); }

// in place on the accumulators (which must be contiguous); max_radii2D may be None.  radii: the forward's int32 radii, or a bool / uint8 mask.
int densify_stats(const torch::Tensor& grad_accum, const torch::Tensor& denom, const c10::optional<torch::Tensor>& max_radii2D, const torch::Tensor& grad2d,
                  const torch::Tensor& radii)
{
    static const char* const who = "densification_stats_";
    need_library();
    if (!g_api.densify_stats) throw std::runtime_error(std::string("densify_stats: the loaded libstp_raster.so does not export stp_densify_stats") + DENSIFY_REBUILD);
    mcmc_check_float(who, "grad2d", grad2d);
    TORCH_CHECK(grad2d.dim() == 2 && (grad2d.size(1) == 2 || grad2d.size(1) == 3), who, ": grad2d must be (P, 3) or (P, 2), got ", grad2d.sizes());
    const int64_t P = grad2d.size(0);
    densify_check_P(who, P);
    densify_check_column(who, "xyz_gradient_accum", grad_accum, P);
    densify_check_column(who, "denom", denom, P);
    if (max_radii2D.has_value()) densify_check_column(who, "max_radii2D", *max_radii2D, P);
    TORCH_CHECK(radii.defined(), who, ": radii must be a tensor");
    const auto vt = radii.scalar_type();
    TORCH_CHECK(vt == torch::kBool || vt == torch::kByte || vt == torch::kInt32, who, ": radii must be int32 (the forward's radii) or a bool / uint8 mask, got ", vt);
    TORCH_CHECK(radii.numel() == P, who, ": radii has ", radii.numel(), " elements, expected ", P);
    TORCH_CHECK(!max_radii2D.has_value() || vt == torch::kInt32, who, ": max_radii2D needs the forward's int32 radii, not a mask (pass max_radii2D=None)");
    mcmc_check_device(who, "xyz_gradient_accum", grad_accum, grad2d);
    mcmc_check_device(who, "denom", denom, grad2d);
    if (max_radii2D.has_value()) mcmc_check_device(who, "max_radii2D", *max_radii2D, grad2d);
    mcmc_check_device(who, "radii", radii, grad2d);
    mcmc_check_device(who, "grad2d", grad2d, grad2d);
    TORCH_CHECK(grad_accum.is_contiguous() && denom.is_contiguous() && (!max_radii2D.has_value() || max_radii2D->is_contiguous()), who,
                ": the accumulators must be contiguous (they are updated in place)");
    if (P == 0) return 0;
    const torch::Tensor g = grad2d.contiguous(), vis = radii.contiguous();
    const c10::hip::HIPGuard guard(g.device().index());
    const int rc = g_api.densify_stats((int)P, grad_accum.data_ptr<float>(), denom.data_ptr<float>(), max_radii2D.has_value() ? max_radii2D->data_ptr<float>() : nullptr,
                                       g.data_ptr<float>(), (int)g.size(1), vis.data_ptr(), vt == torch::kInt32 ? 1 : 0,
                                       (void*)c10::hip::getCurrentHIPStream(g.device().index()).stream());
    if (rc < 0) raise_last(rc);
    return rc;
}

// -> the plan, uint8 (P,).  rule: (grad_threshold, split_size, min_opacity, max_screen_size, max_world_size, split_shrink), rounded to float32 here.
torch::Tensor densify_plan(const torch::Tensor& grad_accum, const torch::Tensor& denom, const torch::Tensor& scaling, const torch::Tensor& opacity,
                           const c10::optional<torch::Tensor>& max_radii2D, const std::vector<double>& rule_in, const bool raw, const bool prune_big)
{
    static const char* const who = "densify_plan";
    need_library();
    if (!g_api.densify_plan) throw std::runtime_error(std::string("densify_plan: the loaded libstp_raster.so does not export stp_densify_plan") + DENSIFY_REBUILD);
    TORCH_CHECK(rule_in.size() == 6, who, ": the rule has six numbers");
    mcmc_check_float(who, "scaling", scaling);
    TORCH_CHECK(scaling.dim() == 2 && scaling.size(1) == 3, who, ": scaling must be (P, 3), got ", scaling.sizes());
    const int64_t P = scaling.size(0);
    densify_check_P(who, P);
    densify_check_column(who, "xyz_gradient_accum", grad_accum, P);
    densify_check_column(who, "denom", denom, P);
    densify_check_column(who, "opacity", opacity, P);
    if (max_radii2D.has_value()) densify_check_column(who, "max_radii2D", *max_radii2D, P);
    mcmc_check_device(who, "xyz_gradient_accum", grad_accum, scaling);
    mcmc_check_device(who, "denom", denom, scaling);
    mcmc_check_device(who, "opacity", opacity, scaling);
    if (max_radii2D.has_value()) mcmc_check_device(who, "max_radii2D", *max_radii2D, scaling);
    mcmc_check_device(who, "scaling", scaling, scaling);
    const c10::hip::HIPGuard guard(scaling.device().index());
    torch::Tensor plan = torch::empty({P}, scaling.options().dtype(torch::kByte));
    if (P == 0) return plan;
    const torch::Tensor ga = grad_accum.contiguous(), de = denom.contiguous(), sc = scaling.contiguous(), op = opacity.contiguous();
    torch::Tensor mr;
    if (max_radii2D.has_value()) mr = max_radii2D->contiguous();
    const StpDensifyRule rule = {(float)rule_in[0], (float)rule_in[1], (float)rule_in[2], (float)rule_in[3], (float)rule_in[4], (float)rule_in[5], raw ? 1 : 0, prune_big ? 1 : 0};
    const int rc = g_api.densify_plan((int)P, ga.data_ptr<float>(), de.data_ptr<float>(), sc.data_ptr<float>(), op.data_ptr<float>(), mr.defined() ? mr.data_ptr<float>() : nullptr,
                                      &rule, plan.data_ptr<uint8_t>(), (void*)c10::hip::getCurrentHIPStream(scaling.device().index()).stream());
    if (rc < 0) raise_last(rc);
    return plan;
}

static void densify_check_plan(const char* who, const torch::Tensor& plan)
{
    TORCH_CHECK(plan.defined() && plan.scalar_type() == torch::kByte, who, ": plan: expected uint8 tensor, got ", plan.scalar_type());
    TORCH_CHECK(plan.dim() == 1, who, ": plan must be (P,), got ", plan.sizes());
    densify_check_P(who, plan.size(0));
    TORCH_CHECK(plan.is_cuda(), who, ": plan: diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product");
}

// -> (offsets (3P,) int32, nK, nC, nS).  SYNCHRONISES the current stream (in the library): the caller needs the counts to allocate.
std::tuple<torch::Tensor, int64_t, int64_t, int64_t> densify_scan(const torch::Tensor& plan_in)
{
    static const char* const who = "densify_scan";
    need_library();
    if (!g_api.densify_scan || !g_api.densify_scratch_bytes)
        throw std::runtime_error(std::string("densify_scan: the loaded libstp_raster.so does not export stp_densify_scan") + DENSIFY_REBUILD);
    densify_check_plan(who, plan_in);
    const torch::Tensor plan = plan_in.contiguous();
    const int64_t P = plan.size(0);
    const c10::hip::HIPGuard guard(plan.device().index());
    torch::Tensor offsets = torch::empty({3 * P}, plan.options().dtype(torch::kInt32));
    int64_t counts[3] = {0, 0, 0};
    if (P == 0) return {offsets, 0, 0, 0};
    const size_t bytes = g_api.densify_scratch_bytes((int)P);
    torch::Tensor scratch = torch::empty({(int64_t)bytes}, plan.options());
    const int rc = g_api.densify_scan((int)P, plan.data_ptr<uint8_t>(), scratch.data_ptr(), bytes, reinterpret_cast<uint32_t*>(offsets.data_ptr<int32_t>()), counts,
                                      (void*)c10::hip::getCurrentHIPStream(plan.device().index()).stream());
    if (rc < 0) raise_last(rc);
    return {offsets, counts[0], counts[1], counts[2]};
}

// -> (new tensors, new exp_avgs, new exp_avg_sqs): lists as long as `tensors`, the moment lists holding None where none was given.  Tensor k
// is (P, ...) of any trailing shape; the outputs are (nK + nC + 2 nS, ...).  No host synchronisation.
std::tuple<std::vector<torch::Tensor>, std::vector<c10::optional<torch::Tensor>>, std::vector<c10::optional<torch::Tensor>>>
densify_apply(const torch::Tensor& plan_in, const torch::Tensor& offsets, const std::vector<int64_t>& counts_in, const std::vector<torch::Tensor>& tensors,
              const std::vector<int64_t>& roles, const std::vector<c10::optional<torch::Tensor>>& exp_avgs, const std::vector<c10::optional<torch::Tensor>>& exp_avg_sqs,
              const c10::optional<torch::Tensor>& noise_in, const double split_shrink, const bool raw)
{
    static const char* const who = "densify_apply";
    need_library();
    if (!g_api.densify_apply) throw std::runtime_error(std::string("densify_apply: the loaded libstp_raster.so does not export stp_densify_apply") + DENSIFY_REBUILD);
    const size_t n = tensors.size();
    TORCH_CHECK(roles.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n, who, ": tensors, roles, exp_avgs and exp_avg_sqs must have one entry per tensor");
    TORCH_CHECK(n <= 64, who, ": ", n, " tensors, at most 64 in one call");
    TORCH_CHECK(counts_in.size() == 3, who, ": counts must be (nK, nC, nS)");
    TORCH_CHECK(plan_in.defined() && plan_in.scalar_type() == torch::kByte && plan_in.dim() == 1, who, ": plan: expected a uint8 (P,) tensor");
    const int64_t P = plan_in.size(0);
    densify_check_P(who, P);
    const int64_t counts[3] = {counts_in[0], counts_in[1], counts_in[2]};
    for (int j = 0; j < 3; j++) TORCH_CHECK(counts[j] >= 0 && counts[j] <= P, who, ": counts[", j, "] = ", counts[j], " outside [0, P]");
    const int64_t nS = counts[2], M = counts[0] + counts[1] + 2 * nS;
    TORCH_CHECK(offsets.defined() && offsets.scalar_type() == torch::kInt32 && offsets.dim() == 1 && offsets.size(0) == 3 * P, who, ": offsets: expected an int32 (3 P,) tensor");
    for (size_t k = 0; k < n; k++) {
        const torch::Tensor& t = tensors[k];
        TORCH_CHECK(t.defined(), who, ": tensor ", k, " is undefined");
        TORCH_CHECK(t.scalar_type() == torch::kFloat32, who, ": tensor ", k, ": expected float32 tensor, got ", t.scalar_type());
        TORCH_CHECK(t.dim() >= 1 && t.size(0) == P, who, ": tensor ", k, " must have ", P, " rows (the plan's), got ", t.sizes());
        TORCH_CHECK(P == 0 || t.numel() > 0, who, ": tensor ", k, ": rows without elements, ", t.sizes());
        TORCH_CHECK(roles[k] >= 0 && roles[k] <= 3, who, ": tensor ", k, ": unknown role ", roles[k], " (0 plain, 1 xyz, 2 scaling, 3 rotation)");
        TORCH_CHECK(exp_avgs[k].has_value() == exp_avg_sqs[k].has_value(), who, ": tensor ", k, ": exp_avg and exp_avg_sq must both be given or both be None");
        if (exp_avgs[k].has_value())
            for (const torch::Tensor* m : {&*exp_avgs[k], &*exp_avg_sqs[k]}) {
                TORCH_CHECK(m->defined() && m->scalar_type() == torch::kFloat32, who, ": tensor ", k, ": moments: expected float32 tensors");
                TORCH_CHECK(m->sizes() == t.sizes(), who, ": tensor ", k, ": a moment has shape ", m->sizes(), ", the parameter has ", t.sizes());
            }
    }
    if (nS > 0) {
        TORCH_CHECK(noise_in.has_value(), who, ": nS = ", nS, " needs noise");
        mcmc_check_float(who, "noise", *noise_in);
        mcmc_check_rows(who, "noise", *noise_in, 2 * nS, 3);
    }
    TORCH_CHECK(plan_in.is_cuda(), who, ": plan: diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product");
    mcmc_check_device(who, "offsets", offsets, plan_in);
    for (size_t k = 0; k < n; k++) {
        mcmc_check_device(who, "a tensor", tensors[k], plan_in);
        if (exp_avgs[k].has_value()) {
            mcmc_check_device(who, "an exp_avg", *exp_avgs[k], plan_in);
            mcmc_check_device(who, "an exp_avg_sq", *exp_avg_sqs[k], plan_in);
        }
    }
    if (nS > 0) mcmc_check_device(who, "noise", *noise_in, plan_in);
    const torch::Tensor plan = plan_in.contiguous(), off = offsets.contiguous();
    const c10::hip::HIPGuard guard(plan.device().index());
    std::vector<torch::Tensor> held; // the contiguous inputs, alive until the launches are made
    std::vector<torch::Tensor> out_p(n);
    std::vector<c10::optional<torch::Tensor>> out_m(n), out_v(n);
    std::vector<StpDensifyTensor> table(n);
    for (size_t k = 0; k < n; k++) {
        std::vector<int64_t> shape = tensors[k].sizes().vec();
        int64_t row = 1;
        for (size_t d = 1; d < shape.size(); d++) row *= shape[d];
        TORCH_CHECK(row > 0 && P * row < (1ll << 31), who, ": tensor ", k, ": ", P, " rows of ", row, " floats: outside (0, 2^31)");
        shape[0] = M;
        held.push_back(tensors[k].contiguous());
        out_p[k] = torch::empty(shape, held.back().options());
        StpDensifyTensor& t = table[k];
        t = StpDensifyTensor{held.back().data_ptr<float>(), nullptr, nullptr, out_p[k].data_ptr<float>(), nullptr, nullptr, (int32_t)row, (int32_t)roles[k]};
        if (exp_avgs[k].has_value()) {
            held.push_back(exp_avgs[k]->contiguous());
            t.exp_avg = held.back().data_ptr<float>();
            held.push_back(exp_avg_sqs[k]->contiguous());
            t.exp_avg_sq = held.back().data_ptr<float>();
            out_m[k] = torch::empty(shape, held.back().options());
            out_v[k] = torch::empty(shape, held.back().options());
            t.exp_avg_out = out_m[k]->data_ptr<float>();
            t.exp_avg_sq_out = out_v[k]->data_ptr<float>();
        }
    }
    torch::Tensor noise;
    if (nS > 0) noise = noise_in->contiguous();
    const int rc = g_api.densify_apply((int)P, plan.data_ptr<uint8_t>(), reinterpret_cast<const uint32_t*>(off.data_ptr<int32_t>()), counts, (int)n, table.data(),
                                       noise.defined() ? noise.data_ptr<float>() : nullptr, (float)split_shrink, raw ? 1 : 0,
                                       (void*)c10::hip::getCurrentHIPStream(plan.device().index()).stream());
    if (rc < 0) raise_last(rc);
    return {out_p, out_m, out_v};
}

// == the fused photometric loss (extension, include/stp_raster.h: stp_photometric_forward / _backward; photometric_loss and fused_ssim in
// __init__.py), on the caller's current stream.  image, target: float32 (C, H, W) or (B, C, H, W) on one GPU, made contiguous here.
struct PhotometricShape { int planes, H, W; };
static PhotometricShape photometric_check(const char* who, const torch::Tensor& image, const torch::Tensor& target)
{
    if (!g_api.photometric_forward || !g_api.photometric_backward || !g_api.photometric_workspace_floats)
        throw std::runtime_error(std::string(who) + ": the loaded libstp_raster.so does not export stp_photometric_forward (a library built before the photometric loss): rebuild it");
    TORCH_CHECK(image.defined() && target.defined(), who, ": image and target must be tensors");
    // (what is wrong with the tensors themselves first, where they live last: every refusal can be met without a GPU)
    TORCH_CHECK(image.scalar_type() == torch::kFloat32, "expected float32 tensor, got ", image.scalar_type());
    TORCH_CHECK(target.scalar_type() == torch::kFloat32, "expected float32 tensor, got ", target.scalar_type());
    TORCH_CHECK(image.dim() == 3 || image.dim() == 4, who, ": image must be (C, H, W) or (B, C, H, W), got ", image.dim(), " dimensions");
    TORCH_CHECK(image.sizes() == target.sizes(), who, ": image has shape ", image.sizes(), ", target has ", target.sizes());
    TORCH_CHECK(target.device() == image.device(), "expected all tensors on ", image.device(), ", got one on ", target.device());
    TORCH_CHECK(image.is_cuda(), "diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product");
    const int64_t H = image.size(-2), W = image.size(-1), planes = H * W > 0 ? image.numel() / (H * W) : 0;
    TORCH_CHECK(image.numel() < (1ll << 31), who, ": ", image.numel(), " elements >= 2^31");
    return PhotometricShape{(int)planes, (int)H, (int)W};
}

// -> (out2 = [mean |image - target|, mean SSIM], the three derivative maps (3, *image.shape) or an undefined tensor)
std::tuple<torch::Tensor, torch::Tensor> photometric_forward(const torch::Tensor& image_in, const torch::Tensor& target_in, const bool want_maps)
{
    need_library();
    const PhotometricShape s = photometric_check("photometric_forward", image_in, target_in);
    const torch::Tensor image = image_in.contiguous(), target = target_in.contiguous();
    const auto opt = image.options();
    const c10::hip::HIPGuard guard(image.device().index());
    torch::Tensor out2 = torch::empty({2}, opt), maps;
    if (image.numel() == 0) { // the mean of nothing, as torch's
        out2.fill_(std::numeric_limits<float>::quiet_NaN());
        if (want_maps) maps = torch::empty({3, 0}, opt);
        return {out2, maps};
    }
    if (want_maps) {
        std::vector<int64_t> shape{3};
        for (const int64_t d : image.sizes()) shape.push_back(d);
        maps = torch::empty(shape, opt);
    }
    torch::Tensor workspace = torch::empty({(int64_t)g_api.photometric_workspace_floats(s.planes, s.H, s.W)}, opt);
    const int rc = g_api.photometric_forward(s.planes, s.H, s.W, image.data_ptr<float>(), target.data_ptr<float>(), out2.data_ptr<float>(),
                                             want_maps ? maps.data_ptr<float>() : nullptr, workspace.data_ptr<float>(),
                                             (void*)c10::hip::getCurrentHIPStream(image.device().index()).stream());
    if (rc < 0) raise_last(rc);
    return {out2, maps};
}

// -> dL/dimage (image's shape); grad_out2 = dL/dout2, two floats on the device (read there: no host synchronisation)
torch::Tensor photometric_backward(const torch::Tensor& image_in, const torch::Tensor& target_in, const torch::Tensor& maps, const torch::Tensor& grad_out2_in)
{
    need_library();
    const PhotometricShape s = photometric_check("photometric_backward", image_in, target_in);
    const torch::Tensor image = image_in.contiguous(), target = target_in.contiguous();
    TORCH_CHECK(maps.defined() && maps.is_cuda() && maps.device() == image.device() && maps.scalar_type() == torch::kFloat32 && maps.is_contiguous() &&
                    maps.numel() == 3 * image.numel(),
                "photometric_backward: maps must be the contiguous float32 tensor of 3 * image.numel() elements a forward with want_maps returned");
    TORCH_CHECK(grad_out2_in.defined() && grad_out2_in.is_cuda() && grad_out2_in.device() == image.device() && grad_out2_in.numel() == 2,
                "photometric_backward: grad_out2 must hold two elements on the device of image");
    const torch::Tensor grad_out2 = grad_out2_in.to(torch::kFloat32).contiguous();
    const c10::hip::HIPGuard guard(image.device().index());
    torch::Tensor dL_dimage = torch::empty(image.sizes(), image.options());
    if (image.numel() == 0) return dL_dimage;
    const int rc = g_api.photometric_backward(s.planes, s.H, s.W, image.data_ptr<float>(), target.data_ptr<float>(), maps.data_ptr<float>(),
                                              grad_out2.data_ptr<float>(), dL_dimage.data_ptr<float>(),
                                              (void*)c10::hip::getCurrentHIPStream(image.device().index()).stream());
    if (rc < 0) raise_last(rc);
    return dL_dimage;
}

// ---- scratch pool surface -------------------------------------------------------------------------------------------
int64_t scratch_generation(const torch::Tensor& buf) // token the autograd function keeps with a pooled buffer (0 for ordinary ones)
{
    if (buf.numel() < BIG_BYTES) return 0;
    std::lock_guard<std::mutex> lock(g_mutex);
    auto it = g_generation.find((uintptr_t)buf.data_ptr());
    return it == g_generation.end() ? 0 : it->second;
}

void check_scratch(const torch::Tensor& buf, int64_t generation)
{
    if (generation && scratch_generation(buf) != generation)
        throw std::runtime_error("a scratch buffer of this forward (tile lists / blend log) was recycled by a later forward pass; run the forward "
                                 "again before this backward");
}

void release_scratch(const torch::Tensor& buf) // hand a pooled buffer back after the backward that consumed it
{
    if (buf.numel() < BIG_BYTES || !buf.is_cuda()) return;
    const c10::hip::HIPGuard guard(buf.get_device());
    std::lock_guard<std::mutex> lock(g_mutex);
    put_back(buf);
}

int64_t clear_scratch_pool(int device) // device < 0: all devices; returns the bytes released
{
    std::lock_guard<std::mutex> lock(g_mutex);
    int64_t freed = 0;
    for (auto it = g_free.begin(); it != g_free.end();) {
        if (device >= 0 && it->first != device) { ++it; continue; }
        for (auto& p : it->second) freed += p.t.numel();
        it = g_free.erase(it);
    }
    for (auto it = g_records.begin(); it != g_records.end();) { // the kept gradient-record buffer goes too
        if (device >= 0 && it->first != device) { ++it; continue; }
        freed += it->second.t.numel() * (int64_t)sizeof(float);
        it = g_records.erase(it);
    }
    return freed;
}

void set_scratch_pool_limit(int max_buffers, int64_t max_bytes)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    g_keep = max_buffers;
    g_max_bytes = max_bytes;
}

std::vector<int64_t> pooled_sizes(int device)
{
    std::lock_guard<std::mutex> lock(g_mutex);
    std::vector<int64_t> out;
    auto it = g_free.find(device);
    if (it != g_free.end()) for (auto& p : it->second) out.push_back(p.t.numel());
    return out;
}

} // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "native host binding of libstp_raster.so (no kernels here: every stage runs behind the C ABI of include/stp_raster.h)";
    m.def("rasterize_gaussians", &rasterize_gaussians);
    m.def("rasterize_gaussians_backward", &rasterize_gaussians_backward);
    m.def("mark_visible", &mark_visible);
    m.def("sparse_adam", &sparse_adam);
    m.def("compute_relocation", &compute_relocation);
    m.def("mcmc_add_noise", &mcmc_add_noise);
    m.def("knn_mean_dist2", &knn_mean_dist2);
    m.def("densify_stats", &densify_stats);
    m.def("densify_plan", &densify_plan);
    m.def("densify_scan", &densify_scan);
    m.def("densify_apply", &densify_apply);
    m.def("photometric_forward", &photometric_forward);
    m.def("photometric_backward", &photometric_backward);
    m.def("scratch_generation", &scratch_generation);
    m.def("check_scratch", &check_scratch);
    m.def("release_scratch", &release_scratch);
    m.def("forget_unless_same_storage", &forget_unless_same_storage);
    m.def("set_forward_split", [](int tile_row, uintptr_t event) { need_library(); g_api.set_forward_split(tile_row, reinterpret_cast<void*>(event)); },
          "the next rasterize_gaussians of this thread renders tile rows below / from tile_row in two launches with `event` (a hipEvent_t handle) recorded between them");
    m.def("clear_scratch_pool", &clear_scratch_pool);
    m.def("set_scratch_pool_limit", &set_scratch_pool_limit);
    m.def("pooled_sizes", &pooled_sizes);
    m.def("load_library", &load_library);
    m.attr("BIG_BYTES") = BIG_BYTES;
}
