// stp_exports.h -- the exports of libstp_raster.so that the binding calls, as ONE table: the Api struct, the symbol loop of load_library, the
// required-symbols check and the "rebuild it" message are all generated from it.  A new export is one line here.
//
// The library is bound at RUN time (load_library, called by _C.py with the path it resolved: the in-tree libstp_raster.so, or STP_RASTER_LIB /
// _C.use_library for A/B runs and the test-only IEEE-depth build), not at link time.
#pragma once

#include <dlfcn.h>

#include <cstddef>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../../include/stp_raster.h"

// X(name, required, feature): the export stp_<name>.  A library without a required one does not load; one without an optional one still loads, and
// asking it for that feature raises (require), naming the feature the export came with.
#define STP_CORE "the C ABI of include/stp_raster.h"
#define STP_EXPORTS(X)                                                                     \
    X(forward, true, STP_CORE)                                                             \
    X(backward_phases, true, STP_CORE)                                                     \
    X(mark_visible, true, STP_CORE)                                                        \
    X(last_error, true, STP_CORE)                                                          \
    X(abi_version, true, STP_CORE)                                                         \
    X(forget_buffer, true, STP_CORE)                                                       \
    X(set_forward_split, true, STP_CORE)                                                   \
    X(camera_grad_workspace_bytes, false, "camera gradients")                              \
    X(set_backward_camera_grads, false, "camera gradients")                                \
    X(set_backward_absgrad, false, "absgrad")                                              \
    X(set_backward_blend_stats, false, "blend statistics")                                 \
    X(set_forward_background, false, "the alpha output and per-pixel background")          \
    X(set_backward_background, false, "the alpha output and per-pixel background")         \
    X(set_forward_invdepth, false, "the inverse-depth output")                             \
    X(set_backward_invdepth, false, "the inverse-depth output")                            \
    X(set_forward_split_sh, false, "split SH inputs")                                      \
    X(set_backward_split_sh, false, "split SH inputs")                                     \
    X(set_forward_raw_params, false, "raw parameter inputs")                               \
    X(set_backward_raw_params, false, "raw parameter inputs")                              \
    X(activate_params, false, "raw parameter inputs")                                      \
    X(set_forward_sh_stash, false, "the SH stash") /* (a library with it also takes NULL for dL_dcolor / dL_dcov3D) */ \
    X(sparse_adam, false, "the sparse Adam step")                                          \
    X(dense_adam, false, "the dense Adam step")                                            \
    X(mcmc_relocation, false, "the 3DGS-MCMC kernels")                                     \
    X(mcmc_add_noise, false, "the 3DGS-MCMC kernels")                                      \
    X(mcmc_relocate_scratch_bytes, false, "the 3DGS-MCMC relocation kernels")              \
    X(mcmc_sample, false, "the 3DGS-MCMC relocation kernels")                              \
    X(mcmc_relocate_apply, false, "the 3DGS-MCMC relocation kernels")                      \
    X(mcmc_add_apply, false, "the 3DGS-MCMC relocation kernels")                           \
    X(mip_filter_3d, false, "the Mip-Splatting 3D filter")                                 \
    X(mip_activations_forward, false, "the Mip-Splatting 3D filter")                       \
    X(mip_activations_backward, false, "the Mip-Splatting 3D filter")                      \
    X(knn_scratch_bytes, false, "the nearest-neighbour kernels")                           \
    X(knn_mean_dist2, false, "the nearest-neighbour kernels")                              \
    X(spatial_order_scratch_bytes, false, "the spatial order kernels")                     \
    X(spatial_order, false, "the spatial order kernels")                                   \
    X(gather_rows, false, "the spatial order kernels")                                     \
    X(densify_stats, false, "the densification kernels")                                   \
    X(densify_plan, false, "the densification kernels")                                    \
    X(densify_scratch_bytes, false, "the densification kernels")                           \
    X(densify_scan, false, "the densification kernels")                                    \
    X(densify_apply, false, "the densification kernels")                                   \
    X(photometric_workspace_floats, false, "the photometric loss")                         \
    X(photometric_forward, false, "the photometric loss")                                  \
    X(photometric_backward, false, "the photometric loss")                                 \
    X(training_loss_workspace_floats, false, "the training loss")                          \
    X(training_loss_forward, false, "the training loss")                                   \
    X(training_loss_backward, false, "the training loss")

namespace {
struct Api {
    void* handle = nullptr;
#define X(name, required, feature) decltype(&stp_##name) name = nullptr;
    STP_EXPORTS(X)
#undef X
} g_api;

struct Export { const char* symbol; bool required; const char* feature; size_t slot; }; // slot: where in Api the function pointer lies
const Export g_exports[] = {
#define X(name, required, feature) {"stp_" #name, required, feature, offsetof(Api, name)},
    STP_EXPORTS(X)
#undef X
};

[[noreturn]] void raise_missing(const Export& e, const std::string& who)
{
    throw std::runtime_error(who + ": the loaded libstp_raster.so does not export " + e.symbol + " (a library built before " + e.feature + "): rebuild it");
}

// fn: a member of g_api, passed as it stands there (it is recognised by its address).  Unreachable through _C.py, whose _require fires first.
template <class F> void require(const F& fn, const char* who)
{
    if (fn) return;
    const size_t slot = reinterpret_cast<const char*>(&fn) - reinterpret_cast<const char*>(&g_api);
    for (const Export& e : g_exports)
        if (e.slot == slot) raise_missing(e, who);
    throw std::logic_error(std::string(who) + ": require() takes a member of g_api");
}

int load_library(const std::string& path)
{
    void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) throw std::runtime_error(std::string("cannot load ") + path + ": " + dlerror());
    Api a;
    a.handle = h;
    for (const Export& e : g_exports) {
        void* fn = dlsym(h, e.symbol);
        if (!fn && e.required) raise_missing(e, path);
        std::memcpy(reinterpret_cast<char*>(&a) + e.slot, &fn, sizeof fn);
    }
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
} // namespace
