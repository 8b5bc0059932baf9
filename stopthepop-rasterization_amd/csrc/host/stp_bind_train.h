// stp_bind_train.h -- the training kernels beside the rasterizer: sparse Adam, 3DGS-MCMC, Mip-Splatting's 3D filter, nearest neighbours, densification, the photometric and the training loss.
// All run on the caller's current stream.  What is wrong with the tensors themselves is refused first, where they live last (stp_tensor_checks.h).
#pragma once

#include <algorithm>
#include <limits>
#include <tuple>

#include <c10/hip/HIPGuard.h>

#include "stp_tensor_checks.h"

namespace {
// == the fused sparse Adam step (extension, include/stp_raster.h: stp_sparse_adam; the step of SparseGaussianAdam in __init__.py): one library call
// for all quadruples (param, grad, exp_avg, exp_avg_sq), on the caller's current stream.  visible: bool / uint8 (non-zero = visible) or the
// int32 radii of the forward (> 0 = visible), N elements, read as it is.  Returns the kernel launches the library made.
int sparse_adam(const std::vector<torch::Tensor>& params, const std::vector<torch::Tensor>& grads, const std::vector<torch::Tensor>& exp_avgs,
                const std::vector<torch::Tensor>& exp_avg_sqs, const torch::Tensor& visible, const std::vector<double>& lrs, const std::vector<double>& epss,
                const double beta1, const double beta2, const int64_t N)
{
    need_library();
    require(g_api.sparse_adam, "sparse_adam");
    const size_t n = params.size();
    TORCH_CHECK(grads.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n && lrs.size() == n && epss.size() == n,
                "sparse_adam: params, grads, exp_avgs, exp_avg_sqs, lrs and epss must have one entry per tensor");
    TORCH_CHECK(N >= 0 && N < (1ll << 31), "sparse_adam: N out of range");
    TORCH_CHECK(visible.defined() && visible.is_cuda(), GPU_ONLY);
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
            TORCH_CHECK(t.is_cuda(), GPU_ONLY);
            TORCH_CHECK(t.device() == dev, "expected all tensors on ", dev, ", got one on ", t.device());
            TORCH_CHECK(t.scalar_type() == torch::kFloat32, "expected float32 tensor, got ", t.scalar_type());
            TORCH_CHECK(t.is_contiguous(), "sparse_adam: tensor ", k, ": ", names[j], " must be contiguous (it is updated in place)");
            TORCH_CHECK(t.sizes() == params[k].sizes(), "sparse_adam: tensor ", k, ": ", names[j], " has shape ", t.sizes(), ", param has ", params[k].sizes());
        }
        table[k] = StpAdamTensor{params[k].data_ptr<float>(), grads[k].data_ptr<float>(), exp_avgs[k].data_ptr<float>(), exp_avg_sqs[k].data_ptr<float>(),
                                 (long long)params[k].numel(), (float)lrs[k], (float)epss[k]};
    }
    const c10::hip::HIPGuard guard(dev.index());
    return checked(g_api.sparse_adam((int)n, table.data(), (int)N, visible.data_ptr(), vt == torch::kInt32 ? 1 : 0, (float)beta1, (float)beta2, current_stream(dev)));
}

// == the fused dense Adam step (extension, include/stp_raster.h: stp_dense_adam; the step of GaussianAdam in __init__.py): one library call for all
// quadruples (param, grad, exp_avg, exp_avg_sq), on the caller's current stream.  coefs: eight float64 values per tensor, in the order of
// StpDenseAdamTensor -- beta1, 1 - beta1, beta2, 1 - beta2, step_size, bias2_sqrt, eps, reg_coef -- rounded to float32 HERE, once; reg_kinds: 0, 1
// (sigmoid) or 2 (exp) per tensor.  Returns the kernel launches the library made.
int dense_adam(const std::vector<torch::Tensor>& params, const std::vector<torch::Tensor>& grads, const std::vector<torch::Tensor>& exp_avgs,
               const std::vector<torch::Tensor>& exp_avg_sqs, const std::vector<double>& coefs, const std::vector<int64_t>& reg_kinds)
{
    need_library();
    require(g_api.dense_adam, "dense_adam");
    const size_t n = params.size();
    TORCH_CHECK(grads.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n && reg_kinds.size() == n && coefs.size() == 8 * n,
                "dense_adam: params, grads, exp_avgs, exp_avg_sqs and reg_kinds must have one entry per tensor, coefs eight");
    if (n == 0) return 0;
    std::vector<StpDenseAdamTensor> table(n);
    for (size_t k = 0; k < n; k++) {
        const torch::Tensor* quad[4] = {&params[k], &grads[k], &exp_avgs[k], &exp_avg_sqs[k]};
        static const char* const names[4] = {"param", "grad", "exp_avg", "exp_avg_sq"};
        for (int j = 0; j < 4; j++) {
            const torch::Tensor& t = *quad[j];
            TORCH_CHECK(t.defined(), "dense_adam: tensor ", k, ": ", names[j], " is undefined");
            TORCH_CHECK(t.layout() == torch::kStrided, "dense_adam: tensor ", k, ": ", names[j], " must be dense, got layout ", t.layout());
            TORCH_CHECK(t.is_cuda(), GPU_ONLY);
            TORCH_CHECK(t.device() == params[0].device(), "expected all tensors on ", params[0].device(), ", got one on ", t.device());
            TORCH_CHECK(t.scalar_type() == torch::kFloat32, "expected float32 tensor, got ", t.scalar_type());
            TORCH_CHECK(t.is_contiguous(), "dense_adam: tensor ", k, ": ", names[j], " must be contiguous (it is updated in place)");
            TORCH_CHECK(t.sizes() == params[k].sizes(), "dense_adam: tensor ", k, ": ", names[j], " has shape ", t.sizes(), ", param has ", params[k].sizes());
        }
        const double* c = &coefs[8 * k];
        table[k] = StpDenseAdamTensor{params[k].data_ptr<float>(), grads[k].data_ptr<float>(), exp_avgs[k].data_ptr<float>(), exp_avg_sqs[k].data_ptr<float>(),
                                      (long long)params[k].numel(), (float)c[0], (float)c[1], (float)c[2], (float)c[3], (float)c[4], (float)c[5], (float)c[6],
                                      (int32_t)reg_kinds[k], (float)c[7]};
    }
    const torch::Device dev = params[0].device();
    const c10::hip::HIPGuard guard(dev.index());
    return checked(g_api.dense_adam((int)n, table.data(), current_stream(dev)));
}

// == the 3DGS-MCMC kernels (extension, include/stp_raster.h: stp_mcmc_relocation / stp_mcmc_add_noise; compute_relocation and mcmc_add_noise_ in
// __init__.py).
// -> (opacity_new of opacity_old's shape, scale_new (n, 3)); upstream's name and argument order.  binoms: checked for its shape only -- the kernel
// has its own binomials -- and n_max is the clamp's upper bound plus one.  N is NOT clamped in place (upstream's is).
std::tuple<torch::Tensor, torch::Tensor> compute_relocation(const torch::Tensor& opacity_old, const torch::Tensor& scale_old, const torch::Tensor& N,
                                                            const c10::optional<torch::Tensor>& binoms_in, const int64_t n_max)
{
    static const char* const who = "compute_relocation";
    need_library();
    require(g_api.mcmc_relocation, who);
    check_float(who, "opacity_old", opacity_old);
    check_float(who, "scale_old", scale_old);
    TORCH_CHECK(N.defined() && (N.scalar_type() == torch::kInt32 || N.scalar_type() == torch::kInt64), who, ": N: expected int32 or int64 tensor, got ", N.scalar_type());
    TORCH_CHECK(n_max >= 2 && n_max <= 51, who, ": n_max must be in [2, 51], got ", n_max);
    if (binoms_in.has_value()) {
        const torch::Tensor& binoms = *binoms_in;
        check_float(who, "binoms", binoms);
        TORCH_CHECK(binoms.dim() == 2 && binoms.size(0) == n_max && binoms.size(1) == n_max, who, ": binoms must be (n_max, n_max) = (", n_max, ", ", n_max, "), got ", binoms.sizes());
    }
    check_column(who, "opacity_old", opacity_old);
    check_column(who, "N", N);
    const int64_t n = opacity_old.size(0);
    TORCH_CHECK(n < (1ll << 31), who, ": opacity_old: ", n, " rows >= 2^31");
    check_rows(who, "scale_old", scale_old, n, 3);
    TORCH_CHECK(N.size(0) == n, who, ": N has ", N.size(0), " rows, opacity_old has ", n);
    check_device(who, "scale_old", scale_old, opacity_old);
    check_device(who, "N", N, opacity_old);
    check_device(who, "opacity_old", opacity_old, opacity_old);
    const torch::Tensor o = opacity_old.contiguous(), s = scale_old.contiguous(), cnt = N.contiguous();
    const c10::hip::HIPGuard guard(o.device().index());
    torch::Tensor o_new = torch::empty(o.sizes(), o.options()), s_new = torch::empty(s.sizes(), s.options());
    if (n == 0) return {o_new, s_new};
    checked(g_api.mcmc_relocation((int)n, o.data_ptr<float>(), s.data_ptr<float>(), cnt.data_ptr(), cnt.scalar_type() == torch::kInt64 ? 1 : 0, (int)n_max,
                                  o_new.data_ptr<float>(), s_new.data_ptr<float>(), current_stream(o.device())));
    return {o_new, s_new};
}

// in place on xyz (which must be contiguous: it is updated where it lies); the other four are made contiguous.  Returns the launches made.
int mcmc_add_noise(const torch::Tensor& xyz, const torch::Tensor& scales, const torch::Tensor& rotations, const torch::Tensor& opacities,
                   const torch::Tensor& noise, const double noise_scale, const double k, const double x0, const bool raw)
{
    static const char* const who = "mcmc_add_noise";
    need_library();
    require(g_api.mcmc_add_noise, who);
    const torch::Tensor* all[5] = {&xyz, &scales, &rotations, &opacities, &noise};
    static const char* const names[5] = {"xyz", "scales", "rotations", "opacities", "noise"};
    for (int j = 0; j < 5; j++) check_float(who, names[j], *all[j]);
    TORCH_CHECK(xyz.dim() == 2 && xyz.size(1) == 3, who, ": xyz must be (P, 3), got ", xyz.sizes());
    const int64_t P = xyz.size(0);
    TORCH_CHECK(P < (1ll << 31), who, ": xyz: ", P, " rows >= 2^31");
    check_rows(who, "scales", scales, P, 3);
    check_rows(who, "rotations", rotations, P, 4);
    check_rows(who, "noise", noise, P, 3);
    check_column(who, "opacities", opacities);
    TORCH_CHECK(opacities.size(0) == P, who, ": opacities has ", opacities.size(0), " rows, xyz has ", P);
    for (int j = 1; j < 5; j++) check_device(who, names[j], *all[j], xyz);
    check_device(who, "xyz", xyz, xyz);
    TORCH_CHECK(xyz.is_contiguous(), who, ": xyz must be contiguous (it is updated in place)");
    if (P == 0) return 0;
    const torch::Tensor s = scales.contiguous(), q = rotations.contiguous(), o = opacities.contiguous(), w = noise.contiguous();
    const c10::hip::HIPGuard guard(xyz.device().index());
    return checked(g_api.mcmc_add_noise((int)P, xyz.data_ptr<float>(), s.data_ptr<float>(), q.data_ptr<float>(), o.data_ptr<float>(), w.data_ptr<float>(),
                                        (float)noise_scale, (float)k, (float)x0, raw ? 1 : 0, current_stream(xyz.device())));
}

// == the 3DGS-MCMC relocation and growth (extension, include/stp_raster.h: stp_mcmc_sample / stp_mcmc_relocate_apply / stp_mcmc_add_apply;
// mcmc_relocation_plan, mcmc_relocate_tensors_, mcmc_add_plan and mcmc_add_tensors in __init__.py).  No host synchronisation anywhere; the scratch is
// a torch tensor of the caching allocator, returned to it when a function leaves (the allocator keeps it for the stream until the kernels have run).
constexpr int64_t MCMC_RELOCATE_MAX_P = 1ll << 28;

// rule 0 (who = mcmc_relocation_plan): uniforms (P,), one per row; rule 1 (who = mcmc_add_plan): uniforms (n,), one per new row.
// -> (src int32 (uniforms' length), count int32 (P,), weights int32 (P,) or an undefined tensor)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> mcmc_sample(const torch::Tensor& opacity_in, const torch::Tensor& uniforms_in, const int64_t rule,
                                                                    const double min_opacity, const bool raw, const bool want_weights)
{
    const char* const who = rule == 0 ? "mcmc_relocation_plan" : "mcmc_add_plan";
    need_library();
    require(g_api.mcmc_sample, who);
    require(g_api.mcmc_relocate_scratch_bytes, who);
    TORCH_CHECK(rule == 0 || rule == 1, "mcmc_sample: unknown rule ", rule);
    check_float(who, "opacity", opacity_in);
    check_float(who, "uniforms", uniforms_in);
    check_column(who, "opacity", opacity_in);
    const int64_t P = opacity_in.size(0);
    TORCH_CHECK(P <= MCMC_RELOCATE_MAX_P, who, ": opacity: ", P, " rows > 2^28");
    TORCH_CHECK(uniforms_in.dim() == 1, who, ": uniforms must be (n,), got ", uniforms_in.sizes());
    const int64_t n = uniforms_in.size(0);
    TORCH_CHECK(rule != 0 || n == P, who, ": uniforms has ", n, " rows, opacity has ", P);
    TORCH_CHECK(n < (1ll << 31), who, ": uniforms: ", n, " rows >= 2^31");
    TORCH_CHECK(P > 0 || n == 0, who, ": ", n, " draws from a model without rows");
    check_device(who, "uniforms", uniforms_in, opacity_in);
    check_device(who, "opacity", opacity_in, opacity_in);
    const torch::Tensor opacity = opacity_in.contiguous(), uniforms = uniforms_in.contiguous();
    const c10::hip::HIPGuard guard(opacity.device().index());
    const auto ints = opacity.options().dtype(torch::kInt32);
    torch::Tensor src = torch::empty({n}, ints), count = torch::empty({P}, ints), weights;
    if (want_weights) weights = torch::empty({P}, ints);
    if (P == 0) return {src, count, weights};
    const size_t bytes = g_api.mcmc_relocate_scratch_bytes((int)P);
    torch::Tensor scratch = torch::empty({(int64_t)bytes}, opacity.options().dtype(torch::kByte));
    checked(g_api.mcmc_sample((int)P, opacity.data_ptr<float>(), (int)rule, (float)min_opacity, raw ? 1 : 0, (int)n, uniforms.data_ptr<float>(), scratch.data_ptr(), bytes,
                              want_weights ? reinterpret_cast<uint32_t*>(weights.data_ptr<int32_t>()) : nullptr, src.data_ptr<int32_t>(), count.data_ptr<int32_t>(),
                              current_stream(opacity.device())));
    return {src, count, weights};
}

// == what the calls over lists of row tensors share (the two 3DGS-MCMC applies and densify_apply).
// The roles of such a call: 0 (plain) .. last, `known` the list behind "unknown role"; width[r] the floats per row of role r and width_text[r] what
// the refusal says (both nullptr: no width is asked for here -- the library asks, under a split).
struct RowRoleRules { int64_t last; const char* known; const int64_t* width; const char* const* width_text; };

// what is wrong with the lists themselves: one entry per tensor, tensors of P rows, known roles, moments both-or-neither in the tensor's shape (in
// place: all contiguous)
void check_row_lists(const char* who, const int64_t P, const std::vector<torch::Tensor>& tensors, const std::vector<int64_t>& roles,
                     const std::vector<c10::optional<torch::Tensor>>& exp_avgs, const std::vector<c10::optional<torch::Tensor>>& exp_avg_sqs, const RowRoleRules& rules,
                     const bool in_place)
{
    const size_t n = tensors.size();
    TORCH_CHECK(roles.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n, who, ": tensors, roles, exp_avgs and exp_avg_sqs must have one entry per tensor");
    TORCH_CHECK(n <= 64, who, ": ", n, " tensors, at most 64 in one call");
    for (size_t k = 0; k < n; k++) {
        const torch::Tensor& t = tensors[k];
        TORCH_CHECK(t.defined(), who, ": tensor ", k, " is undefined");
        TORCH_CHECK(t.scalar_type() == torch::kFloat32, who, ": tensor ", k, ": expected float32 tensor, got ", t.scalar_type());
        TORCH_CHECK(t.dim() >= 1 && t.size(0) == P, who, ": tensor ", k, " must have ", P, " rows (the plan's), got ", t.sizes());
        TORCH_CHECK(P == 0 || t.numel() > 0, who, ": tensor ", k, ": rows without elements, ", t.sizes());
        TORCH_CHECK(roles[k] >= 0 && roles[k] <= rules.last, who, ": tensor ", k, ": unknown role ", roles[k], " ", rules.known);
        TORCH_CHECK(!rules.width || P == 0 || roles[k] == 0 || t.numel() / P == rules.width[roles[k]], who, ": tensor ", k, ": the ", rules.width_text[roles[k]], " per row, got ",
                    t.sizes());
        TORCH_CHECK(exp_avgs[k].has_value() == exp_avg_sqs[k].has_value(), who, ": tensor ", k, ": exp_avg and exp_avg_sq must both be given or both be None");
        TORCH_CHECK(!in_place || t.is_contiguous(), who, ": tensor ", k, " must be contiguous (it is updated in place)");
        if (exp_avgs[k].has_value())
            for (const torch::Tensor* m : {&*exp_avgs[k], &*exp_avg_sqs[k]}) {
                TORCH_CHECK(m->defined() && m->scalar_type() == torch::kFloat32, who, ": tensor ", k, ": moments: expected float32 tensors");
                TORCH_CHECK(m->sizes() == t.sizes(), who, ": tensor ", k, ": a moment has shape ", m->sizes(), ", the parameter has ", t.sizes());
                TORCH_CHECK(!in_place || m->is_contiguous(), who, ": tensor ", k, ": the moments must be contiguous (they are updated in place)");
            }
    }
}

// where the lists live: on the device of `plan`
void check_row_devices(const char* who, const std::vector<torch::Tensor>& tensors, const std::vector<c10::optional<torch::Tensor>>& exp_avgs,
                       const std::vector<c10::optional<torch::Tensor>>& exp_avg_sqs, const torch::Tensor& plan)
{
    for (size_t k = 0; k < tensors.size(); k++) {
        check_device(who, "a tensor", tensors[k], plan);
        if (exp_avgs[k].has_value()) {
            check_device(who, "an exp_avg", *exp_avgs[k], plan);
            check_device(who, "an exp_avg_sq", *exp_avg_sqs[k], plan);
        }
    }
}

// The entry table (StpMcmcTensor or StpDensifyTensor) of an out-of-place call and its outputs of M rows: lists as long as `tensors`, the moment lists
// holding None where none was given.  bound_rows: the rows the library flattens its work over (bound_rows * row < 2^31).
template <class Entry> struct RowOutputs {
    std::vector<torch::Tensor> held; // the contiguous inputs, alive until the launches are made
    std::vector<torch::Tensor> out_p;
    std::vector<c10::optional<torch::Tensor>> out_m, out_v;
    std::vector<Entry> table;
};
template <class Entry>
RowOutputs<Entry> row_outputs(const char* who, const std::vector<torch::Tensor>& tensors, const std::vector<int64_t>& roles, const std::vector<c10::optional<torch::Tensor>>& exp_avgs,
                              const std::vector<c10::optional<torch::Tensor>>& exp_avg_sqs, const int64_t M, const int64_t bound_rows)
{
    const size_t n = tensors.size();
    RowOutputs<Entry> r;
    r.out_p.resize(n); r.out_m.resize(n); r.out_v.resize(n); r.table.resize(n);
    std::vector<torch::Tensor> &held = r.held, &out_p = r.out_p; // (by their own types: r's are dependent names here)
    std::vector<c10::optional<torch::Tensor>> &out_m = r.out_m, &out_v = r.out_v;
    for (size_t k = 0; k < n; k++) {
        std::vector<int64_t> shape = tensors[k].sizes().vec();
        int64_t row = 1;
        for (size_t d = 1; d < shape.size(); d++) row *= shape[d];
        TORCH_CHECK(row > 0 && bound_rows * row < (1ll << 31), who, ": tensor ", k, ": ", bound_rows, " rows of ", row, " floats: outside (0, 2^31)");
        shape[0] = M;
        held.push_back(tensors[k].contiguous());
        out_p[k] = torch::empty(shape, held.back().options());
        Entry& t = r.table[k];
        t = Entry{held.back().data_ptr<float>(), nullptr, nullptr, out_p[k].data_ptr<float>(), nullptr, nullptr, (int32_t)row, (int32_t)roles[k]};
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
    return r;
}

// what the two 3DGS-MCMC applies ask of their plan and lists; -> P (count's length)
int64_t mcmc_check_apply(const char* who, const torch::Tensor& src, const torch::Tensor& count, const std::vector<torch::Tensor>& tensors, const std::vector<int64_t>& roles,
                         const std::vector<c10::optional<torch::Tensor>>& exp_avgs, const std::vector<c10::optional<torch::Tensor>>& exp_avg_sqs, const bool in_place)
{
    static const int64_t width[3] = {0, 1, 3};
    static const char* const width_text[3] = {"", "opacity must have 1 float", "scaling must have 3 floats"};
    static const RowRoleRules rules = {2, "(0 plain, 1 opacity, 2 scaling)", width, width_text};
    TORCH_CHECK(src.defined() && src.scalar_type() == torch::kInt32 && src.dim() == 1, who, ": plan: src: expected an int32 (n,) tensor");
    TORCH_CHECK(count.defined() && count.scalar_type() == torch::kInt32 && count.dim() == 1, who, ": plan: count: expected an int32 (P,) tensor");
    const int64_t P = count.size(0);
    TORCH_CHECK(P <= MCMC_RELOCATE_MAX_P, who, ": ", P, " rows > 2^28");
    TORCH_CHECK(!in_place || src.size(0) == P, who, ": plan: src has ", src.size(0), " rows, count has ", P);
    check_row_lists(who, P, tensors, roles, exp_avgs, exp_avg_sqs, rules, in_place);
    const auto n_opacity = std::count(roles.begin(), roles.end(), 1), n_scaling = std::count(roles.begin(), roles.end(), 2);
    TORCH_CHECK(n_opacity == 1 && n_scaling == 1, who, ": exactly one tensor must have the role opacity and exactly one the role scaling, got ", n_opacity, " and ", n_scaling);
    check_on_gpu(who, "plan", count);
    check_device(who, "plan", src, count);
    check_row_devices(who, tensors, exp_avgs, exp_avg_sqs, count);
    return P;
}

// IN PLACE on every tensor and moment (all contiguous).  Returns the launches made.
int mcmc_relocate_apply(const torch::Tensor& src_in, const torch::Tensor& count_in, const std::vector<torch::Tensor>& tensors, const std::vector<int64_t>& roles,
                        const std::vector<c10::optional<torch::Tensor>>& exp_avgs, const std::vector<c10::optional<torch::Tensor>>& exp_avg_sqs, const double min_opacity,
                        const bool raw, const bool reset_dead_moments)
{
    static const char* const who = "mcmc_relocate_tensors_";
    need_library();
    require(g_api.mcmc_relocate_apply, who);
    require(g_api.mcmc_relocate_scratch_bytes, who);
    const int64_t P = mcmc_check_apply(who, src_in, count_in, tensors, roles, exp_avgs, exp_avg_sqs, true);
    if (P == 0) return 0;
    const size_t n = tensors.size();
    const torch::Tensor src = src_in.contiguous(), count = count_in.contiguous();
    const c10::hip::HIPGuard guard(count.device().index());
    std::vector<StpMcmcTensor> table(n);
    for (size_t k = 0; k < n; k++) {
        const int64_t row = tensors[k].numel() / P;
        TORCH_CHECK(tensors[k].numel() < (1ll << 31), who, ": tensor ", k, ": ", P, " rows of ", row, " floats: outside (0, 2^31)");
        table[k] = StpMcmcTensor{tensors[k].data_ptr<float>(), nullptr, nullptr, nullptr, nullptr, nullptr, (int32_t)row, (int32_t)roles[k]};
        if (exp_avgs[k].has_value()) {
            table[k].exp_avg = exp_avgs[k]->data_ptr<float>();
            table[k].exp_avg_sq = exp_avg_sqs[k]->data_ptr<float>();
        }
    }
    const size_t bytes = g_api.mcmc_relocate_scratch_bytes((int)P);
    torch::Tensor scratch = torch::empty({(int64_t)bytes}, count.options().dtype(torch::kByte));
    return checked(g_api.mcmc_relocate_apply((int)P, src.data_ptr<int32_t>(), count.data_ptr<int32_t>(), (int)n, table.data(), (float)min_opacity, raw ? 1 : 0,
                                             reset_dead_moments ? 1 : 0, scratch.data_ptr(), bytes, current_stream(count.device())));
}

// -> (new tensors, new exp_avgs, new exp_avg_sqs) of P + src.size(0) rows: lists as long as `tensors`, the moment lists holding None where none was given
std::tuple<std::vector<torch::Tensor>, std::vector<c10::optional<torch::Tensor>>, std::vector<c10::optional<torch::Tensor>>>
mcmc_add_apply(const torch::Tensor& src_in, const torch::Tensor& count_in, const std::vector<torch::Tensor>& tensors, const std::vector<int64_t>& roles,
               const std::vector<c10::optional<torch::Tensor>>& exp_avgs, const std::vector<c10::optional<torch::Tensor>>& exp_avg_sqs, const double min_opacity, const bool raw)
{
    static const char* const who = "mcmc_add_tensors";
    need_library();
    require(g_api.mcmc_add_apply, who);
    require(g_api.mcmc_relocate_scratch_bytes, who);
    const int64_t P = mcmc_check_apply(who, src_in, count_in, tensors, roles, exp_avgs, exp_avg_sqs, false);
    const int64_t n_new = src_in.size(0), M = P + n_new;
    TORCH_CHECK(P > 0 || n_new == 0, who, ": ", n_new, " new rows from a model without rows");
    const torch::Tensor src = src_in.contiguous(), count = count_in.contiguous();
    const c10::hip::HIPGuard guard(count.device().index());
    RowOutputs<StpMcmcTensor> r = row_outputs<StpMcmcTensor>(who, tensors, roles, exp_avgs, exp_avg_sqs, M, M);
    if (P == 0) return {r.out_p, r.out_m, r.out_v};
    const size_t bytes = g_api.mcmc_relocate_scratch_bytes((int)P);
    torch::Tensor scratch = torch::empty({(int64_t)bytes}, count.options().dtype(torch::kByte));
    checked(g_api.mcmc_add_apply((int)P, (int)n_new, src.data_ptr<int32_t>(), count.data_ptr<int32_t>(), (int)r.table.size(), r.table.data(), (float)min_opacity, raw ? 1 : 0,
                                 scratch.data_ptr(), bytes, current_stream(count.device())));
    return {r.out_p, r.out_m, r.out_v};
}

// == Mip-Splatting's 3D filter (extension, include/stp_raster.h: stp_mip_filter_3d / stp_mip_activations_forward / _backward; compute_3d_filter and
// filtered_activations in __init__.py).  No host synchronisation; the 4-byte workspace is a torch tensor of the caching allocator.
// -> filter_3d (P, 1).  xyz is made contiguous, and so are the two camera tensors.
torch::Tensor compute_3d_filter(const torch::Tensor& xyz_in, const torch::Tensor& views_in, const torch::Tensor& intrinsics_in)
{
    static const char* const who = "compute_3d_filter";
    need_library();
    require(g_api.mip_filter_3d, who);
    check_float(who, "xyz", xyz_in);
    check_float(who, "world_view_transforms", views_in);
    check_float(who, "intrinsics", intrinsics_in);
    TORCH_CHECK(xyz_in.dim() == 2 && xyz_in.size(1) == 3, who, ": xyz must be (P, 3), got ", xyz_in.sizes());
    const int64_t P = xyz_in.size(0);
    TORCH_CHECK(P < (1ll << 31), who, ": xyz: ", P, " rows >= 2^31");
    TORCH_CHECK(views_in.dim() == 3 && views_in.size(1) == 4 && views_in.size(2) == 4, who, ": world_view_transforms must be (C, 4, 4), got ", views_in.sizes());
    const int64_t C = views_in.size(0);
    TORCH_CHECK(C > 0, who, ": world_view_transforms: C == 0: the filter needs at least one camera");
    TORCH_CHECK(C < (1ll << 24), who, ": world_view_transforms: ", C, " cameras >= 2^24");
    check_rows(who, "intrinsics", intrinsics_in, C, 4);
    check_device(who, "world_view_transforms", views_in, xyz_in);
    check_device(who, "intrinsics", intrinsics_in, xyz_in);
    check_device(who, "xyz", xyz_in, xyz_in);
    const torch::Tensor xyz = xyz_in.detach().contiguous(), views = views_in.detach().contiguous(), intrinsics = intrinsics_in.detach().contiguous();
    const c10::hip::HIPGuard guard(xyz.device().index());
    torch::Tensor out = torch::empty({P, 1}, xyz.options());
    if (P == 0) return out;
    torch::Tensor workspace = torch::empty({1}, xyz.options().dtype(torch::kInt32));
    checked(g_api.mip_filter_3d((int)P, (int)C, xyz.data_ptr<float>(), views.data_ptr<float>(), intrinsics.data_ptr<float>(), workspace.data_ptr(), out.data_ptr<float>(),
                                current_stream(xyz.device())));
    return out;
}

// what the two activation calls ask of (scaling, opacity, filter_3d); -> P
int64_t mip_check_inputs(const char* who, const torch::Tensor& scaling, const torch::Tensor& opacity, const torch::Tensor& filter_3d)
{
    check_float(who, "scaling", scaling);
    check_float(who, "opacity", opacity);
    check_float(who, "filter_3d", filter_3d);
    TORCH_CHECK(scaling.dim() == 2 && scaling.size(1) == 3, who, ": scaling must be (P, 3), got ", scaling.sizes());
    const int64_t P = scaling.size(0);
    TORCH_CHECK(P < (1ll << 31), who, ": scaling: ", P, " rows >= 2^31");
    check_column(who, "opacity", opacity);
    TORCH_CHECK(opacity.size(0) == P, who, ": opacity has ", opacity.size(0), " rows, scaling has ", P);
    check_column(who, "filter_3d", filter_3d);
    TORCH_CHECK(filter_3d.size(0) == P, who, ": filter_3d has ", filter_3d.size(0), " rows, scaling has ", P);
    return P;
}

// -> (scales (P, 3), opacities of opacity's shape)
std::tuple<torch::Tensor, torch::Tensor> mip_activations(const torch::Tensor& scaling_in, const torch::Tensor& opacity_in, const torch::Tensor& filter_in)
{
    static const char* const who = "filtered_activations";
    need_library();
    require(g_api.mip_activations_forward, who);
    const int64_t P = mip_check_inputs(who, scaling_in, opacity_in, filter_in);
    check_device(who, "opacity", opacity_in, scaling_in);
    check_device(who, "filter_3d", filter_in, scaling_in);
    check_device(who, "scaling", scaling_in, scaling_in);
    const torch::Tensor scaling = scaling_in.detach().contiguous(), opacity = opacity_in.detach().contiguous(), filter = filter_in.detach().contiguous();
    const c10::hip::HIPGuard guard(scaling.device().index());
    torch::Tensor scales = torch::empty(scaling.sizes(), scaling.options()), opacities = torch::empty(opacity.sizes(), opacity.options());
    if (P == 0) return {scales, opacities};
    checked(g_api.mip_activations_forward((int)P, scaling.data_ptr<float>(), opacity.data_ptr<float>(), filter.data_ptr<float>(), scales.data_ptr<float>(),
                                          opacities.data_ptr<float>(), current_stream(scaling.device())));
    return {scales, opacities};
}

// -> (grad_scaling (P, 3), grad_opacity of opacity's shape); either upstream gradient may be None (zeros), not both
std::tuple<torch::Tensor, torch::Tensor> mip_activations_backward(const torch::Tensor& scaling_in, const torch::Tensor& opacity_in, const torch::Tensor& filter_in,
                                                                  const c10::optional<torch::Tensor>& grad_scales_in, const c10::optional<torch::Tensor>& grad_opacities_in)
{
    static const char* const who = "filtered_activations (backward)";
    need_library();
    require(g_api.mip_activations_backward, who);
    const int64_t P = mip_check_inputs(who, scaling_in, opacity_in, filter_in);
    TORCH_CHECK(grad_scales_in.has_value() || grad_opacities_in.has_value(), who, ": grad_scales and grad_opacities are both None");
    if (grad_scales_in.has_value()) {
        check_float(who, "grad_scales", *grad_scales_in);
        check_rows(who, "grad_scales", *grad_scales_in, P, 3);
    }
    if (grad_opacities_in.has_value()) {
        check_float(who, "grad_opacities", *grad_opacities_in);
        check_column(who, "grad_opacities", *grad_opacities_in);
        TORCH_CHECK(grad_opacities_in->size(0) == P, who, ": grad_opacities has ", grad_opacities_in->size(0), " rows, scaling has ", P);
    }
    check_device(who, "opacity", opacity_in, scaling_in);
    check_device(who, "filter_3d", filter_in, scaling_in);
    if (grad_scales_in.has_value()) check_device(who, "grad_scales", *grad_scales_in, scaling_in);
    if (grad_opacities_in.has_value()) check_device(who, "grad_opacities", *grad_opacities_in, scaling_in);
    check_device(who, "scaling", scaling_in, scaling_in);
    const torch::Tensor scaling = scaling_in.detach().contiguous(), opacity = opacity_in.detach().contiguous(), filter = filter_in.detach().contiguous();
    torch::Tensor gs, go;
    if (grad_scales_in.has_value()) gs = grad_scales_in->contiguous();
    if (grad_opacities_in.has_value()) go = grad_opacities_in->contiguous();
    const c10::hip::HIPGuard guard(scaling.device().index());
    torch::Tensor g_scaling = torch::empty(scaling.sizes(), scaling.options()), g_opacity = torch::empty(opacity.sizes(), opacity.options());
    if (P == 0) return {g_scaling, g_opacity};
    checked(g_api.mip_activations_backward((int)P, scaling.data_ptr<float>(), opacity.data_ptr<float>(), filter.data_ptr<float>(), gs.defined() ? gs.data_ptr<float>() : nullptr,
                                           go.defined() ? go.data_ptr<float>() : nullptr, g_scaling.data_ptr<float>(), g_opacity.data_ptr<float>(),
                                           current_stream(scaling.device())));
    return {g_scaling, g_opacity};
}

// == the activated copies of a trainer's raw parameters (extension, include/stp_raster.h: stp_activate_params; activate_params in __init__.py): the
// values the rasterizer's raw path renders with, to the bit.  -> (scales, rotations, opacities), fresh contiguous float32 tensors in the inputs' shapes,
// an undefined tensor (None) for an absent input.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> activate_params(const c10::optional<torch::Tensor>& scaling, const c10::optional<torch::Tensor>& rotation,
                                                                        const c10::optional<torch::Tensor>& opacity)
{
    static const char* const who = "activate_params";
    need_library();
    require(g_api.activate_params, who);
    const c10::optional<torch::Tensor>* all[3] = {&scaling, &rotation, &opacity};
    static const char* const names[3] = {"scaling", "rotation", "opacity"};
    const torch::Tensor* first = nullptr;
    for (int j = 0; j < 3; j++)
        if (all[j]->has_value()) { check_float(who, names[j], **all[j]); if (!first) first = &**all[j]; }
    if (!first) return {torch::Tensor(), torch::Tensor(), torch::Tensor()};
    const int64_t P = first->dim() > 0 ? first->size(0) : -1;
    if (scaling.has_value()) check_rows(who, "scaling", *scaling, P, 3);
    if (rotation.has_value()) check_rows(who, "rotation", *rotation, P, 4);
    if (opacity.has_value()) {
        check_column(who, "opacity", *opacity);
        TORCH_CHECK(opacity->size(0) == P, who, ": opacity has ", opacity->size(0), " rows, ", P, " expected");
    }
    TORCH_CHECK(P < (1ll << 29), who, ": ", P, " rows >= 2^29");
    for (int j = 0; j < 3; j++)
        if (all[j]->has_value()) check_device(who, names[j], **all[j], *first);
    torch::Tensor in[3], out[3];
    for (int j = 0; j < 3; j++)
        if (all[j]->has_value()) { in[j] = (*all[j])->detach().contiguous(); out[j] = torch::empty(in[j].sizes(), in[j].options()); }
    if (P == 0) return {out[0], out[1], out[2]};
    auto ptr = [](const torch::Tensor& t) -> float* { return t.defined() ? t.data_ptr<float>() : nullptr; };
    const c10::hip::HIPGuard guard(first->device().index());
    checked(g_api.activate_params((int)P, ptr(in[0]), ptr(in[1]), ptr(in[2]), ptr(out[0]), ptr(out[1]), ptr(out[2]), current_stream(first->device())));
    return {out[0], out[1], out[2]};
}

// == simple_knn's distCUDA2 (extension, include/stp_raster.h: stp_knn_mean_dist2; knn_mean_dist2 in __init__.py and simple_knn._C.distCUDA2), on the
// caller's current stream: -> (P,) float32, the mean of the three smallest squared distances to the other points, in input order.  The scratch is
// a torch tensor of the caching allocator, returned to it when this function leaves (the allocator keeps it for the stream until the kernels
// have run).  No host synchronisation.
torch::Tensor knn_mean_dist2(const torch::Tensor& points_in)
{
    static const char* const who = "knn_mean_dist2";
    need_library();
    require(g_api.knn_mean_dist2, who);
    require(g_api.knn_scratch_bytes, who);
    check_float(who, "points", points_in);
    TORCH_CHECK(points_in.dim() == 2 && points_in.size(1) == 3, who, ": points must be (P, 3), got ", points_in.sizes());
    const int64_t P = points_in.size(0);
    TORCH_CHECK(P < (1ll << 31), who, ": points: ", P, " rows >= 2^31");
    TORCH_CHECK(P == 0 || P >= 4, who, ": points: ", P, " rows: the mean over three neighbours needs at least 4 points");
    check_device(who, "points", points_in, points_in);
    const torch::Tensor points = points_in.detach().contiguous();
    const c10::hip::HIPGuard guard(points.device().index());
    torch::Tensor out = torch::empty({P}, points.options());
    if (P == 0) return out;
    const size_t bytes = g_api.knn_scratch_bytes((int)P);
    torch::Tensor scratch = torch::empty({(int64_t)bytes}, points.options().dtype(torch::kByte));
    checked(g_api.knn_mean_dist2((int)P, points.data_ptr<float>(), scratch.data_ptr(), bytes, out.data_ptr<float>(), current_stream(points.device())));
    return out;
}

// == the Morton order of a cloud (extension, include/stp_raster.h: stp_spatial_order; spatial_order in __init__.py), on the caller's current stream:
// -> (order int32 (P,), codes int32 (P,) or an undefined tensor).  The scratch comes from the caching allocator as knn_mean_dist2's does.  No host
// synchronisation.
std::tuple<torch::Tensor, torch::Tensor> spatial_order(const torch::Tensor& xyz_in, const bool return_codes)
{
    static const char* const who = "spatial_order";
    need_library();
    require(g_api.spatial_order, who);
    require(g_api.spatial_order_scratch_bytes, who);
    check_float(who, "xyz", xyz_in);
    TORCH_CHECK(xyz_in.dim() == 2 && xyz_in.size(1) == 3, who, ": xyz must be (P, 3), got ", xyz_in.sizes());
    const int64_t P = xyz_in.size(0);
    TORCH_CHECK(P < (1ll << 31), who, ": xyz: ", P, " rows >= 2^31");
    check_device(who, "xyz", xyz_in, xyz_in);
    const torch::Tensor xyz = xyz_in.detach().contiguous();
    const c10::hip::HIPGuard guard(xyz.device().index());
    torch::Tensor order = torch::empty({P}, xyz.options().dtype(torch::kInt32)), codes;
    if (return_codes) codes = torch::empty({P}, xyz.options().dtype(torch::kInt32));
    if (P == 0) return {order, codes};
    const size_t bytes = g_api.spatial_order_scratch_bytes((int)P);
    torch::Tensor scratch = torch::empty({(int64_t)bytes}, xyz.options().dtype(torch::kByte));
    checked(g_api.spatial_order((int)P, xyz.data_ptr<float>(), scratch.data_ptr(), bytes, order.data_ptr<int32_t>(),
                                return_codes ? reinterpret_cast<uint32_t*>(codes.data_ptr<int32_t>()) : nullptr, current_stream(xyz.device())));
    return {order, codes};
}

// == the gather of rows (extension, include/stp_raster.h: stp_gather_rows; gather_tensors and reorder_gaussians_ in __init__.py): -> (new tensors,
// new exp_avgs, new exp_avg_sqs) of index.size(0) rows, lists as long as `tensors`, the moment lists holding None where none was given.  Tensor k is
// float32 or int32 (P, ...) of any trailing shape -- the rows are moved as bits -- and its moments have its dtype and shape.  No host synchronisation.
std::tuple<std::vector<torch::Tensor>, std::vector<c10::optional<torch::Tensor>>, std::vector<c10::optional<torch::Tensor>>>
gather_rows(const torch::Tensor& index_in, const std::vector<torch::Tensor>& tensors, const std::vector<c10::optional<torch::Tensor>>& exp_avgs,
            const std::vector<c10::optional<torch::Tensor>>& exp_avg_sqs)
{
    static const char* const who = "gather_tensors";
    need_library();
    require(g_api.gather_rows, who);
    const size_t n = tensors.size();
    TORCH_CHECK(index_in.defined() && index_in.scalar_type() == torch::kInt32, who, ": index: expected an int32 tensor");
    TORCH_CHECK(index_in.dim() == 1, who, ": index must be (M,), got ", index_in.sizes());
    TORCH_CHECK(exp_avgs.size() == n && exp_avg_sqs.size() == n, who, ": tensors, exp_avgs and exp_avg_sqs must have one entry per tensor");
    TORCH_CHECK(n <= 64, who, ": ", n, " tensors, at most 64 in one call");
    const int64_t M = index_in.size(0), P = n > 0 && tensors[0].defined() && tensors[0].dim() >= 1 ? tensors[0].size(0) : 0;
    for (size_t k = 0; k < n; k++) {
        const torch::Tensor& t = tensors[k];
        TORCH_CHECK(t.defined(), who, ": tensor ", k, " is undefined");
        TORCH_CHECK(t.scalar_type() == torch::kFloat32 || t.scalar_type() == torch::kInt32, who, ": tensor ", k, ": expected float32 or int32 tensor, got ", t.scalar_type());
        TORCH_CHECK(t.dim() >= 1 && t.size(0) == P, who, ": tensor ", k, " must have ", P, " rows (tensor 0's), got ", t.sizes());
        TORCH_CHECK(P == 0 || t.numel() > 0, who, ": tensor ", k, ": rows without elements, ", t.sizes());
        TORCH_CHECK(exp_avgs[k].has_value() == exp_avg_sqs[k].has_value(), who, ": tensor ", k, ": exp_avg and exp_avg_sq must both be given or both be None");
        if (exp_avgs[k].has_value())
            for (const torch::Tensor* m : {&*exp_avgs[k], &*exp_avg_sqs[k]}) {
                TORCH_CHECK(m->defined() && m->scalar_type() == t.scalar_type(), who, ": tensor ", k, ": moments: expected ", t.scalar_type(), " tensors");
                TORCH_CHECK(m->sizes() == t.sizes(), who, ": tensor ", k, ": a moment has shape ", m->sizes(), ", the parameter has ", t.sizes());
            }
    }
    TORCH_CHECK(P < (1ll << 31) && M < (1ll << 31), who, ": ", P, " rows, ", M, " indices: >= 2^31");
    TORCH_CHECK(M == 0 || P > 0 || n == 0, who, ": ", M, " rows from tensors without rows");
    check_on_gpu(who, "index", index_in);
    for (size_t k = 0; k < n; k++) {
        check_device(who, "a tensor", tensors[k], index_in);
        if (exp_avgs[k].has_value()) {
            check_device(who, "an exp_avg", *exp_avgs[k], index_in);
            check_device(who, "an exp_avg_sq", *exp_avg_sqs[k], index_in);
        }
    }
    const torch::Tensor index = index_in.contiguous();
    const c10::hip::HIPGuard guard(index.device().index());
    std::vector<torch::Tensor> held, out_p(n); // held: the contiguous inputs, alive until the launches are made
    std::vector<c10::optional<torch::Tensor>> out_m(n), out_v(n);
    std::vector<StpGatherTensor> table(n);
    const auto ptr = [](const torch::Tensor& t) { return static_cast<float*>(t.data_ptr()); }; // (4-byte elements: moved, never computed on)
    for (size_t k = 0; k < n; k++) {
        std::vector<int64_t> shape = tensors[k].sizes().vec();
        int64_t row = 1;
        for (size_t d = 1; d < shape.size(); d++) row *= shape[d];
        TORCH_CHECK(P == 0 || (row > 0 && std::max(P, M) * row < (1ll << 31)), who, ": tensor ", k, ": ", std::max(P, M), " rows of ", row, " elements: outside (0, 2^31)");
        shape[0] = M;
        held.push_back(tensors[k].detach().contiguous());
        out_p[k] = torch::empty(shape, held.back().options());
        table[k] = StpGatherTensor{ptr(held.back()), nullptr, nullptr, ptr(out_p[k]), nullptr, nullptr, (int32_t)row, 0};
        if (exp_avgs[k].has_value()) {
            held.push_back(exp_avgs[k]->detach().contiguous());
            table[k].exp_avg = ptr(held.back());
            held.push_back(exp_avg_sqs[k]->detach().contiguous());
            table[k].exp_avg_sq = ptr(held.back());
            out_m[k] = torch::empty(shape, held.back().options());
            out_v[k] = torch::empty(shape, held.back().options());
            table[k].exp_avg_out = ptr(*out_m[k]);
            table[k].exp_avg_sq_out = ptr(*out_v[k]);
        }
    }
    if (M == 0 || n == 0 || P == 0) return {out_p, out_m, out_v};
    checked(g_api.gather_rows((int)P, (int)M, index.data_ptr<int32_t>(), (int)n, table.data(), current_stream(index.device())));
    return {out_p, out_m, out_v};
}

// == densification (extension, include/stp_raster.h: stp_densify_stats / _plan / _scan / _apply; densification_stats_, densify_plan,
// densify_tensors and densify_and_prune in __init__.py).  Only densify_scan synchronises with the host (inside the library: the new row count).
void densify_check_column(const char* who, const char* name, const torch::Tensor& t, const int64_t P)
{
    check_float(who, name, t);
    check_column(who, name, t);
    TORCH_CHECK(t.size(0) == P, who, ": ", name, " has ", t.size(0), " rows, expected ", P);
}
void densify_check_P(const char* who, const int64_t P) { TORCH_CHECK(3 * P < (1ll << 31), who, ": ", P, " rows: 3 P >= 2^31"); }

// in place on the accumulators (which must be contiguous); max_radii2D may be None.  radii: the forward's int32 radii, or a bool / uint8 mask.
int densify_stats(const torch::Tensor& grad_accum, const torch::Tensor& denom, const c10::optional<torch::Tensor>& max_radii2D, const torch::Tensor& grad2d,
                  const torch::Tensor& radii)
{
    static const char* const who = "densification_stats_";
    need_library();
    require(g_api.densify_stats, "densify_stats");
    check_float(who, "grad2d", grad2d);
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
    check_device(who, "xyz_gradient_accum", grad_accum, grad2d);
    check_device(who, "denom", denom, grad2d);
    if (max_radii2D.has_value()) check_device(who, "max_radii2D", *max_radii2D, grad2d);
    check_device(who, "radii", radii, grad2d);
    check_device(who, "grad2d", grad2d, grad2d);
    TORCH_CHECK(grad_accum.is_contiguous() && denom.is_contiguous() && (!max_radii2D.has_value() || max_radii2D->is_contiguous()), who,
                ": the accumulators must be contiguous (they are updated in place)");
    if (P == 0) return 0;
    const torch::Tensor g = grad2d.contiguous(), vis = radii.contiguous();
    const c10::hip::HIPGuard guard(g.device().index());
    return checked(g_api.densify_stats((int)P, grad_accum.data_ptr<float>(), denom.data_ptr<float>(), max_radii2D.has_value() ? max_radii2D->data_ptr<float>() : nullptr,
                                       g.data_ptr<float>(), (int)g.size(1), vis.data_ptr(), vt == torch::kInt32 ? 1 : 0, current_stream(g.device())));
}

// -> the plan, uint8 (P,).  rule: (grad_threshold, split_size, min_opacity, max_screen_size, max_world_size, split_shrink), rounded to float32 here.
torch::Tensor densify_plan(const torch::Tensor& grad_accum, const torch::Tensor& denom, const torch::Tensor& scaling, const torch::Tensor& opacity,
                           const c10::optional<torch::Tensor>& max_radii2D, const std::vector<double>& rule_in, const bool raw, const bool prune_big)
{
    static const char* const who = "densify_plan";
    need_library();
    require(g_api.densify_plan, who);
    TORCH_CHECK(rule_in.size() == 6, who, ": the rule has six numbers");
    check_float(who, "scaling", scaling);
    TORCH_CHECK(scaling.dim() == 2 && scaling.size(1) == 3, who, ": scaling must be (P, 3), got ", scaling.sizes());
    const int64_t P = scaling.size(0);
    densify_check_P(who, P);
    densify_check_column(who, "xyz_gradient_accum", grad_accum, P);
    densify_check_column(who, "denom", denom, P);
    densify_check_column(who, "opacity", opacity, P);
    if (max_radii2D.has_value()) densify_check_column(who, "max_radii2D", *max_radii2D, P);
    check_device(who, "xyz_gradient_accum", grad_accum, scaling);
    check_device(who, "denom", denom, scaling);
    check_device(who, "opacity", opacity, scaling);
    if (max_radii2D.has_value()) check_device(who, "max_radii2D", *max_radii2D, scaling);
    check_device(who, "scaling", scaling, scaling);
    const c10::hip::HIPGuard guard(scaling.device().index());
    torch::Tensor plan = torch::empty({P}, scaling.options().dtype(torch::kByte));
    if (P == 0) return plan;
    const torch::Tensor ga = grad_accum.contiguous(), de = denom.contiguous(), sc = scaling.contiguous(), op = opacity.contiguous();
    torch::Tensor mr;
    if (max_radii2D.has_value()) mr = max_radii2D->contiguous();
    const StpDensifyRule rule = {(float)rule_in[0], (float)rule_in[1], (float)rule_in[2], (float)rule_in[3], (float)rule_in[4], (float)rule_in[5], raw ? 1 : 0, prune_big ? 1 : 0};
    checked(g_api.densify_plan((int)P, ga.data_ptr<float>(), de.data_ptr<float>(), sc.data_ptr<float>(), op.data_ptr<float>(), mr.defined() ? mr.data_ptr<float>() : nullptr,
                               &rule, plan.data_ptr<uint8_t>(), current_stream(scaling.device())));
    return plan;
}

// -> (offsets (3P,) int32, nK, nC, nS).  SYNCHRONISES the current stream (in the library): the caller needs the counts to allocate.
std::tuple<torch::Tensor, int64_t, int64_t, int64_t> densify_scan(const torch::Tensor& plan_in)
{
    static const char* const who = "densify_scan";
    need_library();
    require(g_api.densify_scan, who);
    require(g_api.densify_scratch_bytes, who);
    TORCH_CHECK(plan_in.defined() && plan_in.scalar_type() == torch::kByte, who, ": plan: expected uint8 tensor, got ", plan_in.scalar_type());
    TORCH_CHECK(plan_in.dim() == 1, who, ": plan must be (P,), got ", plan_in.sizes());
    densify_check_P(who, plan_in.size(0));
    check_on_gpu(who, "plan", plan_in);
    const torch::Tensor plan = plan_in.contiguous();
    const int64_t P = plan.size(0);
    const c10::hip::HIPGuard guard(plan.device().index());
    torch::Tensor offsets = torch::empty({3 * P}, plan.options().dtype(torch::kInt32));
    int64_t counts[3] = {0, 0, 0};
    if (P == 0) return {offsets, 0, 0, 0};
    const size_t bytes = g_api.densify_scratch_bytes((int)P);
    torch::Tensor scratch = torch::empty({(int64_t)bytes}, plan.options());
    checked(g_api.densify_scan((int)P, plan.data_ptr<uint8_t>(), scratch.data_ptr(), bytes, reinterpret_cast<uint32_t*>(offsets.data_ptr<int32_t>()), counts,
                               current_stream(plan.device())));
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
    require(g_api.densify_apply, who);
    static const RowRoleRules rules = {3, "(0 plain, 1 xyz, 2 scaling, 3 rotation)", nullptr, nullptr};
    TORCH_CHECK(counts_in.size() == 3, who, ": counts must be (nK, nC, nS)");
    TORCH_CHECK(plan_in.defined() && plan_in.scalar_type() == torch::kByte && plan_in.dim() == 1, who, ": plan: expected a uint8 (P,) tensor");
    const int64_t P = plan_in.size(0);
    densify_check_P(who, P);
    const int64_t counts[3] = {counts_in[0], counts_in[1], counts_in[2]};
    for (int j = 0; j < 3; j++) TORCH_CHECK(counts[j] >= 0 && counts[j] <= P, who, ": counts[", j, "] = ", counts[j], " outside [0, P]");
    const int64_t nS = counts[2], M = counts[0] + counts[1] + 2 * nS;
    TORCH_CHECK(offsets.defined() && offsets.scalar_type() == torch::kInt32 && offsets.dim() == 1 && offsets.size(0) == 3 * P, who, ": offsets: expected an int32 (3 P,) tensor");
    check_row_lists(who, P, tensors, roles, exp_avgs, exp_avg_sqs, rules, false);
    if (nS > 0) {
        TORCH_CHECK(noise_in.has_value(), who, ": nS = ", nS, " needs noise");
        check_float(who, "noise", *noise_in);
        check_rows(who, "noise", *noise_in, 2 * nS, 3);
    }
    check_on_gpu(who, "plan", plan_in);
    check_device(who, "offsets", offsets, plan_in);
    check_row_devices(who, tensors, exp_avgs, exp_avg_sqs, plan_in);
    if (nS > 0) check_device(who, "noise", *noise_in, plan_in);
    const torch::Tensor plan = plan_in.contiguous(), off = offsets.contiguous();
    const c10::hip::HIPGuard guard(plan.device().index());
    RowOutputs<StpDensifyTensor> r = row_outputs<StpDensifyTensor>(who, tensors, roles, exp_avgs, exp_avg_sqs, M, P); // (the library's work is over the P source rows)
    torch::Tensor noise;
    if (nS > 0) noise = noise_in->contiguous();
    checked(g_api.densify_apply((int)P, plan.data_ptr<uint8_t>(), reinterpret_cast<const uint32_t*>(off.data_ptr<int32_t>()), counts, (int)r.table.size(), r.table.data(),
                                noise.defined() ? noise.data_ptr<float>() : nullptr, (float)split_shrink, raw ? 1 : 0, current_stream(plan.device())));
    return {r.out_p, r.out_m, r.out_v};
}

// == the fused photometric loss (extension, include/stp_raster.h: stp_photometric_forward / _backward; photometric_loss and fused_ssim in
// __init__.py).  image, target: float32 (C, H, W) or (B, C, H, W) on one GPU, made contiguous here.
struct PhotometricShape { int planes, H, W; };
// what is wrong with image and target themselves, before where they live
void photometric_tensor_check(const char* who, const torch::Tensor& image, const torch::Tensor& target)
{
    TORCH_CHECK(image.defined() && target.defined(), who, ": image and target must be tensors");
    TORCH_CHECK(image.scalar_type() == torch::kFloat32, "expected float32 tensor, got ", image.scalar_type());
    TORCH_CHECK(target.scalar_type() == torch::kFloat32, "expected float32 tensor, got ", target.scalar_type());
    TORCH_CHECK(image.dim() == 3 || image.dim() == 4, who, ": image must be (C, H, W) or (B, C, H, W), got ", image.dim(), " dimensions");
    TORCH_CHECK(image.sizes() == target.sizes(), who, ": image has shape ", image.sizes(), ", target has ", target.sizes());
    TORCH_CHECK(target.device() == image.device(), "expected all tensors on ", image.device(), ", got one on ", target.device());
}
PhotometricShape photometric_shape(const char* who, const torch::Tensor& image)
{
    TORCH_CHECK(image.is_cuda(), GPU_ONLY);
    const int64_t H = image.size(-2), W = image.size(-1), planes = H * W > 0 ? image.numel() / (H * W) : 0;
    TORCH_CHECK(image.numel() < (1ll << 31), who, ": ", image.numel(), " elements >= 2^31");
    return PhotometricShape{(int)planes, (int)H, (int)W};
}
PhotometricShape photometric_check(const char* who, const torch::Tensor& image, const torch::Tensor& target)
{
    require(g_api.photometric_forward, who);
    require(g_api.photometric_backward, who);
    require(g_api.photometric_workspace_floats, who);
    photometric_tensor_check(who, image, target);
    return photometric_shape(who, image);
}
// the outputs of a loss forward on the (contiguous) image: n_terms floats and, with want_maps, the maps (3, *image.shape).  An empty image:
// NaN terms (the means of nothing, as torch's) and (3, 0) maps -- the caller returns them as they are
struct LossOutputs { torch::Tensor terms, maps; };
LossOutputs loss_outputs(const torch::Tensor& image, const int64_t n_terms, const bool want_maps)
{
    const auto opt = image.options();
    LossOutputs o{torch::empty({n_terms}, opt), torch::Tensor()};
    if (image.numel() == 0) o.terms.fill_(std::numeric_limits<float>::quiet_NaN());
    if (want_maps) {
        std::vector<int64_t> shape{3};
        if (image.numel() == 0) shape.push_back(0);
        else shape.insert(shape.end(), image.sizes().begin(), image.sizes().end());
        o.maps = torch::empty(shape, opt);
    }
    return o;
}
// what a loss backward with n_terms terms asks of maps and of grad_out = dL/dterms -> grad_out as contiguous float32
torch::Tensor loss_backward_check(const char* who, const torch::Tensor& image, const torch::Tensor& maps, const torch::Tensor& grad_out, const int64_t n_terms)
{
    TORCH_CHECK(maps.defined() && maps.is_cuda() && maps.device() == image.device() && maps.scalar_type() == torch::kFloat32 && maps.is_contiguous() &&
                    maps.numel() == 3 * image.numel(),
                who, ": maps must be the contiguous float32 tensor of 3 * image.numel() elements a forward with want_maps returned");
    TORCH_CHECK(grad_out.defined() && grad_out.is_cuda() && grad_out.device() == image.device() && grad_out.numel() == n_terms,
                who, ": grad_out", n_terms, " must hold ", n_terms == 2 ? "two" : "three", " elements on the device of image");
    return grad_out.to(torch::kFloat32).contiguous();
}

// -> (out2 = [mean |image - target|, mean SSIM], the three derivative maps (3, *image.shape) or an undefined tensor)
std::tuple<torch::Tensor, torch::Tensor> photometric_forward(const torch::Tensor& image_in, const torch::Tensor& target_in, const bool want_maps)
{
    need_library();
    const PhotometricShape s = photometric_check("photometric_forward", image_in, target_in);
    const torch::Tensor image = image_in.contiguous(), target = target_in.contiguous();
    const c10::hip::HIPGuard guard(image.device().index());
    const LossOutputs o = loss_outputs(image, 2, want_maps);
    if (image.numel() == 0) return {o.terms, o.maps};
    torch::Tensor workspace = torch::empty({(int64_t)g_api.photometric_workspace_floats(s.planes, s.H, s.W)}, image.options());
    checked(g_api.photometric_forward(s.planes, s.H, s.W, image.data_ptr<float>(), target.data_ptr<float>(), o.terms.data_ptr<float>(),
                                      want_maps ? o.maps.data_ptr<float>() : nullptr, workspace.data_ptr<float>(), current_stream(image.device())));
    return {o.terms, o.maps};
}

// -> dL/dimage (image's shape); grad_out2 = dL/dout2, two floats on the device (read there: no host synchronisation)
torch::Tensor photometric_backward(const torch::Tensor& image_in, const torch::Tensor& target_in, const torch::Tensor& maps, const torch::Tensor& grad_out2_in)
{
    need_library();
    const PhotometricShape s = photometric_check("photometric_backward", image_in, target_in);
    const torch::Tensor image = image_in.contiguous(), target = target_in.contiguous();
    const torch::Tensor grad_out2 = loss_backward_check("photometric_backward", image, maps, grad_out2_in, 2);
    const c10::hip::HIPGuard guard(image.device().index());
    torch::Tensor dL_dimage = torch::empty(image.sizes(), image.options());
    if (image.numel() == 0) return dL_dimage;
    checked(g_api.photometric_backward(s.planes, s.H, s.W, image.data_ptr<float>(), target.data_ptr<float>(), maps.data_ptr<float>(),
                                       grad_out2.data_ptr<float>(), dL_dimage.data_ptr<float>(), current_stream(image.device())));
    return dL_dimage;
}

// == the training loss (extension, include/stp_raster.h: stp_training_loss_forward / _backward; training_terms and training_loss in
// __init__.py): the photometric terms of the exposed, clamped and masked image plus the inverse-depth term.  Every extra is optional.
using OptTensor = c10::optional<torch::Tensor>;
struct TrainingExtras {
    PhotometricShape s;
    StpTrainingLoss pod{};
    torch::Tensor exposure, alpha_mask, invdepth, mono_invdepth, depth_mask; // contiguous; undefined = not given
};
// an (H, W), (1, H, W) or (B, 1, H, W) plane set beside the image: its contiguous form and the number of planes
int64_t check_planes(const char* who, const char* name, const torch::Tensor& t, const torch::Tensor& image, const bool allow_2d)
{
    check_float(who, name, t);
    const int64_t H = image.size(-2), W = image.size(-1);
    const bool dims = (allow_2d && t.dim() == 2) || (t.dim() == 3 && t.size(0) == 1) || (t.dim() == 4 && t.size(1) == 1);
    TORCH_CHECK(dims && t.size(-2) == H && t.size(-1) == W, who, ": ", name, " must be ", allow_2d ? "(H, W), " : "", "(1, H, W) or (B, 1, H, W) with the image's H = ", H,
                ", W = ", W, ", got ", t.sizes());
    return t.dim() == 4 ? t.size(0) : 1;
}
TrainingExtras training_check(const char* who, const torch::Tensor& image, const torch::Tensor& target, const OptTensor& exposure, const bool clamp,
                              const OptTensor& alpha_mask, const OptTensor& invdepth, const OptTensor& mono_invdepth, const OptTensor& depth_mask)
{
    require(g_api.training_loss_forward, who);
    require(g_api.training_loss_backward, who);
    require(g_api.training_loss_workspace_floats, who);
    TrainingExtras x;
    photometric_tensor_check(who, image, target); // (3j's refusals, in 3j's words)
    const int64_t C = image.size(-3), B = image.dim() == 4 ? image.size(0) : 1;
    x.pod.clamp = clamp ? 1 : 0;
    x.pod.channels = (int32_t)std::max<int64_t>(C, 1);
    if (exposure.has_value()) {
        check_float(who, "exposure", *exposure);
        TORCH_CHECK(C == 3, who, ": exposure needs an image of three channels, got C = ", C);
        const bool one = exposure->dim() == 2 && exposure->size(0) == 3 && exposure->size(1) == 4;
        const bool per_image = exposure->dim() == 3 && image.dim() == 4 && exposure->size(0) == B && exposure->size(1) == 3 && exposure->size(2) == 4;
        TORCH_CHECK(one || per_image, who, ": exposure must be (3, 4) or, with a (B, 3, H, W) image, (B, 3, 4), got ", exposure->sizes());
        x.exposure = exposure->contiguous();
        x.pod.exposure = x.exposure.data_ptr<float>();
        x.pod.exposure_batched = per_image ? 1 : 0;
    }
    if (alpha_mask.has_value()) {
        const int64_t planes = check_planes(who, "alpha_mask", *alpha_mask, image, true);
        TORCH_CHECK(alpha_mask->dim() != 4 || (image.dim() == 4 && planes == B), who, ": alpha_mask of ", planes, " images beside an image batch of ", B);
        x.alpha_mask = alpha_mask->contiguous();
        x.pod.alpha_mask = x.alpha_mask.data_ptr<float>();
        x.pod.alpha_mask_batched = alpha_mask->dim() == 4 ? 1 : 0;
    }
    TORCH_CHECK(invdepth.has_value() == mono_invdepth.has_value(), who, ": invdepth and mono_invdepth come together or not at all");
    TORCH_CHECK(invdepth.has_value() || !depth_mask.has_value(), who, ": depth_mask without invdepth");
    if (invdepth.has_value()) {
        const int64_t planes = check_planes(who, "invdepth", *invdepth, image, false);
        check_planes(who, "mono_invdepth", *mono_invdepth, image, false);
        TORCH_CHECK(mono_invdepth->sizes() == invdepth->sizes(), who, ": invdepth has shape ", invdepth->sizes(), ", mono_invdepth has ", mono_invdepth->sizes());
        x.invdepth = invdepth->contiguous();
        x.mono_invdepth = mono_invdepth->contiguous();
        x.pod.depth_planes = (int32_t)planes;
        if (depth_mask.has_value()) {
            check_planes(who, "depth_mask", *depth_mask, image, false);
            TORCH_CHECK(depth_mask->sizes() == invdepth->sizes(), who, ": invdepth has shape ", invdepth->sizes(), ", depth_mask has ", depth_mask->sizes());
                x.depth_mask = depth_mask->contiguous();
        }
        if (x.invdepth.numel() > 0) {
            x.pod.invdepth = x.invdepth.data_ptr<float>();
            x.pod.mono_invdepth = x.mono_invdepth.data_ptr<float>();
            if (x.depth_mask.defined()) x.pod.depth_mask = x.depth_mask.data_ptr<float>();
        } else {
            x.pod.depth_planes = 0;
        }
    }
    // where they live, last
    x.s = photometric_shape(who, image);
    const OptTensor* extras[5] = {&exposure, &alpha_mask, &invdepth, &mono_invdepth, &depth_mask};
    static const char* const names[5] = {"exposure", "alpha_mask", "invdepth", "mono_invdepth", "depth_mask"};
    for (int k = 0; k < 5; k++)
        if (extras[k]->has_value()) check_device(who, names[k], **extras[k], image);
    return x;
}

// -> (out3 = [mean |x'' - target|, mean SSIM(x'', target), mean |(invdepth - mono_invdepth) depth_mask|], the maps (3, *image.shape) or undefined)
std::tuple<torch::Tensor, torch::Tensor> training_loss_forward(const torch::Tensor& image_in, const torch::Tensor& target_in, const OptTensor& exposure, const bool clamp,
                                                               const OptTensor& alpha_mask, const OptTensor& invdepth, const OptTensor& mono_invdepth,
                                                               const OptTensor& depth_mask, const bool want_maps)
{
    need_library();
    static const char* const who = "training_loss_forward";
    const TrainingExtras x = training_check(who, image_in, target_in, exposure, clamp, alpha_mask, invdepth, mono_invdepth, depth_mask);
    const torch::Tensor image = image_in.contiguous(), target = target_in.contiguous();
    const c10::hip::HIPGuard guard(image.device().index());
    const LossOutputs o = loss_outputs(image, 3, want_maps);
    if (image.numel() == 0) return {o.terms, o.maps};
    torch::Tensor workspace = torch::empty({(int64_t)g_api.training_loss_workspace_floats(x.s.planes, x.s.H, x.s.W, x.pod.depth_planes)}, image.options());
    checked(g_api.training_loss_forward(x.s.planes, x.s.H, x.s.W, image.data_ptr<float>(), target.data_ptr<float>(), &x.pod, o.terms.data_ptr<float>(),
                                        want_maps ? o.maps.data_ptr<float>() : nullptr, workspace.data_ptr<float>(), current_stream(image.device())));
    return {o.terms, o.maps};
}

// -> (dL/dimage, dL/dexposure (exposure's shape) or undefined, dL/dinvdepth (invdepth's shape) or undefined); grad_out3: three floats on the device
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> training_loss_backward(const torch::Tensor& image_in, const torch::Tensor& target_in, const OptTensor& exposure,
                                                                               const bool clamp, const OptTensor& alpha_mask, const OptTensor& invdepth,
                                                                               const OptTensor& mono_invdepth, const OptTensor& depth_mask, const torch::Tensor& maps,
                                                                               const torch::Tensor& grad_out3_in, const bool want_exposure, const bool want_invdepth)
{
    need_library();
    static const char* const who = "training_loss_backward";
    const TrainingExtras x = training_check(who, image_in, target_in, exposure, clamp, alpha_mask, invdepth, mono_invdepth, depth_mask);
    const torch::Tensor image = image_in.contiguous(), target = target_in.contiguous();
    const torch::Tensor grad_out3 = loss_backward_check(who, image, maps, grad_out3_in, 3);
    TORCH_CHECK(!want_exposure || x.exposure.defined(), who, ": a gradient for an exposure that was not given");
    TORCH_CHECK(!want_invdepth || x.invdepth.defined(), who, ": a gradient for an invdepth that was not given");
    const c10::hip::HIPGuard guard(image.device().index());
    torch::Tensor dL_dimage = torch::empty(image.sizes(), image.options()), dL_dexposure, dL_dinvdepth, workspace;
    if (want_exposure) dL_dexposure = torch::empty(x.exposure.sizes(), image.options());
    if (want_invdepth) dL_dinvdepth = torch::empty(x.invdepth.sizes(), image.options());
    if (image.numel() == 0) {
        if (want_exposure) dL_dexposure.zero_();
        return {dL_dimage, dL_dexposure, dL_dinvdepth};
    }
    if (want_exposure) workspace = torch::empty({(int64_t)g_api.training_loss_workspace_floats(x.s.planes, x.s.H, x.s.W, x.pod.depth_planes)}, image.options());
    checked(g_api.training_loss_backward(x.s.planes, x.s.H, x.s.W, image.data_ptr<float>(), target.data_ptr<float>(), &x.pod, maps.data_ptr<float>(),
                                         grad_out3.data_ptr<float>(), dL_dimage.data_ptr<float>(), want_exposure ? dL_dexposure.data_ptr<float>() : nullptr,
                                         want_invdepth && x.pod.invdepth ? dL_dinvdepth.data_ptr<float>() : nullptr,
                                         want_exposure ? workspace.data_ptr<float>() : nullptr, current_stream(image.device())));
    return {dL_dimage, dL_dexposure, dL_dinvdepth};
}
} // namespace
