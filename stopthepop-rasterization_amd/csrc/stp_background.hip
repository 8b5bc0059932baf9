// stp_background.hip -- dL/dbackground of a backward with stp_set_backward_background (no counterpart in the reference, which does not
// differentiate its background).
//
// The image is  out[ch, p] = C[ch, p] + T_final[p] * B[ch, p],  so  dL/dB[ch, p] = T_final[p] * dL_dpix[ch, p]:  with a per-pixel background
// that product is the gradient (background_grad_kernel<.., false>), with a uniform one its sum over the pixels.  Both stream final_T and the
// three planes of dL_dpix once over the pixel rows of the frame's tile-row window -- 16 bytes per lane and access where the planes allow it
// (W * H a multiple of four and 16-byte aligned pointers: the window starts at a multiple of 16 pixels), one float per lane otherwise.
//
// The uniform sum runs in a FIXED order without float atomics, like the camera gradients: the grid is a function of the pixel count alone,
// every thread adds its elements in index order, a workgroup's 256 threads are summed by a butterfly inside each wave and in wave order
// across the four (background_grad_kernel<.., true> -> three floats per workgroup), and ONE workgroup adds the partial rows the same way
// (background_grad_sum_kernel).  Equal inputs give bit-equal sums.
#include "stp_internal.h"

namespace stp {

namespace {

constexpr int BG_BLOCK = 256;
constexpr int BG_MAX_GROUPS = 1024;     // workgroups of the streaming kernel (four per CU); more pixels are grid-strided
constexpr int BG_ELEMS_PER_THREAD = 8;  // accesses a thread makes per plane before another workgroup is worth its launch

template <typename V> struct Lanes;
template <> struct Lanes<float> {
    static constexpr int N = 1;
    static __device__ __forceinline__ float mul(float t, float d) { return t * d; }
    static __device__ __forceinline__ float sum(float v) { return v; }
};
template <> struct Lanes<float4> {
    static constexpr int N = 4;
    static __device__ __forceinline__ float4 mul(float4 t, float4 d) { return make_float4(t.x * d.x, t.y * d.y, t.z * d.z, t.w * d.w); }
    static __device__ __forceinline__ float sum(float4 v) { return (v.x + v.y) + (v.z + v.w); }
};

// the workgroup's sum of v in thread 0: butterfly inside every wave (the same tree in every lane), then the four waves in order
__device__ __forceinline__ float block_sum(float v, float* s_wave)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads(); // (s_wave is used once per channel)
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// elements [first, first + count) of every plane, in units of V; plane = elements of V between two channels of dL_dpix / dL_dB
template <typename V, bool UNIFORM>
__global__ void __launch_bounds__(BG_BLOCK) background_grad_kernel(const V* __restrict__ final_T, const V* __restrict__ dL_dpix, V* __restrict__ dL_dB,
                                                                   float* __restrict__ partials, const size_t plane, const size_t first, const size_t count)
{
    __shared__ float s_wave[BG_BLOCK / 64];
    float acc[3] = {0.0f, 0.0f, 0.0f};
    const size_t stride = (size_t)gridDim.x * BG_BLOCK;
    for (size_t i = (size_t)blockIdx.x * BG_BLOCK + threadIdx.x; i < count; i += stride) {
        const size_t e = first + i;
        const V t = final_T[e];
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const V g = Lanes<V>::mul(t, dL_dpix[ch * plane + e]);
            if constexpr (UNIFORM) acc[ch] += Lanes<V>::sum(g);
            else dL_dB[ch * plane + e] = g;
        }
    }
    if constexpr (UNIFORM) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const float s = block_sum(acc[ch], s_wave);
            if (threadIdx.x == 0) partials[3 * blockIdx.x + ch] = s;
        }
    }
}

// one workgroup: the `groups` partial rows, thread t rows t, t + 256, ... in order, then the workgroup's sum
__global__ void __launch_bounds__(BG_BLOCK) background_grad_sum_kernel(const float* __restrict__ partials, const int groups, float* __restrict__ dL_dbg)
{
    __shared__ float s_wave[BG_BLOCK / 64];
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float acc = 0.0f;
        for (int r = (int)threadIdx.x; r < groups; r += BG_BLOCK) acc += partials[3 * r + ch];
        const float s = block_sum(acc, s_wave);
        if (threadIdx.x == 0) dL_dbg[ch] = s;
    }
}

int groups_for(size_t count)
{
    const size_t per_group = (size_t)BG_BLOCK * BG_ELEMS_PER_THREAD;
    const size_t g = (count + per_group - 1) / per_group;
    return (int)(g < 1 ? 1 : (g > BG_MAX_GROUPS ? BG_MAX_GROUPS : g));
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename V>
hipError_t launch_typed(const float* final_T, const float* dL_dpix, float* out, float* partials, bool uniform, size_t N, size_t first, size_t count, hipStream_t st)
{
    constexpr size_t L = Lanes<V>::N;
    const size_t plane = N / L, f = first / L, c = count / L;
    const int groups = groups_for(c);
    if (uniform) {
        hipLaunchKernelGGL((background_grad_kernel<V, true>), dim3(groups), dim3(BG_BLOCK), 0, st, reinterpret_cast<const V*>(final_T),
                           reinterpret_cast<const V*>(dL_dpix), static_cast<V*>(nullptr), partials, plane, f, c);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL(background_grad_sum_kernel, dim3(1), dim3(BG_BLOCK), 0, st, partials, groups, out);
    } else {
        hipLaunchKernelGGL((background_grad_kernel<V, false>), dim3(groups), dim3(BG_BLOCK), 0, st, reinterpret_cast<const V*>(final_T),
                           reinterpret_cast<const V*>(dL_dpix), reinterpret_cast<V*>(out), static_cast<float*>(nullptr), plane, f, c);
    }
    return hipGetLastError();
}

} // namespace

size_t background_grad_partials() { return (size_t)3 * BG_MAX_GROUPS; }

hipError_t launch_background_grad(const FrameParams& f, const ImageState& img, const BackwardParams& bw, float* partials, hipStream_t st)
{
    if (bw.dL_dbackground == nullptr) return hipSuccess;
    const bool uniform = bw.bg_image == nullptr;
    const size_t N = (size_t)f.W * f.H;
    // the window's pixel rows: frame-coordinate indexing, like the render kernels' (ImageState::final_T is the frame's pointer)
    const size_t y0 = (size_t)f.ty0 * TILE, y1 = (size_t)f.ty1 * TILE < (size_t)f.H ? (size_t)f.ty1 * TILE : (size_t)f.H;
    const size_t first = y0 * f.W, count = y1 > y0 ? (y1 - y0) * f.W : 0;
    if (count == 0) // an empty window: nothing to write per pixel, an empty sum
        return uniform ? hipMemsetAsync(bw.dL_dbackground, 0, 3 * sizeof(float), st) : hipSuccess;
    const bool wide = (N & 3) == 0 && (first & 3) == 0 && (count & 3) == 0 && aligned16(img.final_T) && aligned16(bw.dL_dpix) && (uniform || aligned16(bw.dL_dbackground));
    if (wide) return launch_typed<float4>(img.final_T, bw.dL_dpix, bw.dL_dbackground, partials, uniform, N, first, count, st);
    return launch_typed<float>(img.final_T, bw.dL_dpix, bw.dL_dbackground, partials, uniform, N, first, count, st);
}

} // namespace stp
