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
// callbacks are C functions, and the scratch pool for the two large buffers lives beside them (stp_scratch_pool.h).
//
// ONE translation unit (each one that includes torch/extension.h costs the build half a minute), cut by concern into headers: the two below,
// and under them stp_exports.h (the table of the library's exports), stp_tensor_checks.h and stp_scratch_pool.h.
#include "stp_bind_raster.h"
#include "stp_bind_train.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m)
{
    m.doc() = "native host binding of libstp_raster.so (no kernels here: every stage runs behind the C ABI of include/stp_raster.h)";
    m.def("rasterize_gaussians", &rasterize_gaussians);
    m.def("rasterize_gaussians_backward", &rasterize_gaussians_backward);
    m.def("mark_visible", &mark_visible);
    m.def("sparse_adam", &sparse_adam);
    m.def("dense_adam", &dense_adam);
    m.def("compute_relocation", &compute_relocation);
    m.def("mcmc_add_noise", &mcmc_add_noise);
    m.def("mcmc_sample", &mcmc_sample);
    m.def("mcmc_relocate_apply", &mcmc_relocate_apply);
    m.def("mcmc_add_apply", &mcmc_add_apply);
    m.def("compute_3d_filter", &compute_3d_filter);
    m.def("mip_activations", &mip_activations);
    m.def("mip_activations_backward", &mip_activations_backward);
    m.def("activate_params", &activate_params);
    m.def("knn_mean_dist2", &knn_mean_dist2);
    m.def("spatial_order", &spatial_order);
    m.def("gather_rows", &gather_rows);
    m.def("densify_stats", &densify_stats);
    m.def("densify_plan", &densify_plan);
    m.def("densify_scan", &densify_scan);
    m.def("densify_apply", &densify_apply);
    m.def("photometric_forward", &photometric_forward);
    m.def("photometric_backward", &photometric_backward);
    m.def("training_loss_forward", &training_loss_forward);
    m.def("training_loss_backward", &training_loss_backward);
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
