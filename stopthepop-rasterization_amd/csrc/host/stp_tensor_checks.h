// stp_tensor_checks.h -- what every binding function does around its library call: tensor checks, the current stream, the return code, a settings flag.
#pragma once

#include <torch/extension.h>

#include <c10/hip/HIPStream.h>

#include "stp_exports.h"

namespace {
constexpr const char* GPU_ONLY = "diff_gaussian_rasterization (MI355X build) needs tensors on a GPU device; there is no CPU path in the product";

// the calling thread's current HIP stream on dev, as the C ABI takes it
void* current_stream(const torch::Device& dev) { return (void*)c10::hip::getCurrentHIPStream(dev.index()).stream(); }
// a library call's return code: negative = the library's error, raised
int checked(int rc) { if (rc < 0) raise_last(rc); return rc; }

bool setting_present(const py::dict& d, const char* key) { return d.contains(key) && !d[key].is_none(); }
bool setting_flag(const py::dict& d, const char* key) { return setting_present(d, key) && d[key].cast<bool>(); }

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

// The named checks of the training kernels' functions.  What is wrong with the tensors themselves is refused first, where they live (check_device)
// last: every refusal can be met without a GPU.
void check_float(const char* who, const char* name, const torch::Tensor& t)
{
    TORCH_CHECK(t.defined(), who, ": ", name, " must be a tensor");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32, who, ": ", name, ": expected float32 tensor, got ", t.scalar_type());
}
void check_rows(const char* who, const char* name, const torch::Tensor& t, const int64_t rows, const int64_t width)
{
    TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == width, who, ": ", name, " must be (", rows, ", ", width, "), got ", t.sizes());
}
void check_column(const char* who, const char* name, const torch::Tensor& t)
{
    TORCH_CHECK(t.dim() == 1 || (t.dim() == 2 && t.size(1) == 1), who, ": ", name, " must be (n,) or (n, 1), got ", t.sizes());
}
// where a tensor lives: the GPU-only sentence under the function's and the tensor's name
void check_on_gpu(const char* who, const char* name, const torch::Tensor& t) { TORCH_CHECK(t.is_cuda(), who, ": ", name, ": ", GPU_ONLY); }
void check_device(const char* who, const char* name, const torch::Tensor& t, const torch::Tensor& first)
{
    TORCH_CHECK(t.device() == first.device(), who, ": ", name, ": expected all tensors on ", first.device(), ", got one on ", t.device());
    check_on_gpu(who, name, t);
}
} // namespace
